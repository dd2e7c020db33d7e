"""GPU: the C++ adapters of include/eacham/GuidedMatchHip.hpp (MatchGuided on a pair list and on a ResidentMatchGraph) return
the Python mirror's bytes on the twins case (tests/cpp/guided_driver.cpp, linked with libeacham_hip.so)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import guided_cases as GCS
from eacham_amd import HipContext
from eacham_amd import guided as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("guided") / "guided_driver")
    lib = os.path.join(ROOT, "eacham_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
           os.path.join(CPP, "guided_driver.cpp"), "-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def write_case(path, case, k):
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", case["dim"], len(case["descs"])))
        for d, xy in zip(case["descs"], case["xys"]):
            f.write(struct.pack("<i", len(d)))
            f.write(np.ascontiguousarray(d, np.float32).tobytes())
            f.write(np.ascontiguousarray(xy, np.float64).tobytes())
        f.write(struct.pack("<i", len(case["pairs"])))
        f.write(np.ascontiguousarray(case["pairs"], np.int32).tobytes())
        f.write(np.ascontiguousarray(case["models"], np.float64).tobytes())
        K = case["K"]
        f.write(struct.pack("<ii", G.KINDS[case["kind"]], int(K is not None)))
        f.write(np.ascontiguousarray(K if K is not None else np.zeros(4), np.float64).tobytes())
        f.write(struct.pack("<fdIi", float(k["max_error"]), k["ratio"], k["max_d2"], int(k["cross_check"])))


def read_graph(buf, at, P):
    total = struct.unpack_from("<q", buf, at)[0]
    at += 8
    out = []
    for dtype, n in ((np.int32, P), (np.int64, P + 1), (np.uint32, total), (np.uint32, total), (np.uint32, total), (np.int32, 3 * P)):
        a = np.frombuffer(buf, dtype=dtype, count=n, offset=at)
        at += a.nbytes
        out.append(a)
    return out, at


@pytest.mark.parametrize("name,i", [("twins128", 0), ("twins128", 1), ("twins128", 6), ("twinsE_K", 0)])
def test_adapters_return_the_mirrors_bytes(driver, tmp_path, name, i):
    case, k = GCS.case_by_name(name), GCS.calls(name)[i]
    with HipContext(0) as ctx:
        for f, d in enumerate(case["descs"]):
            ctx.upload_descriptors(f, d)
        want = G.match_guided(ctx, case["kind"], case["pairs"], case["models"], case["xys"], k["max_error"], k["ratio"], k["max_d2"], k["cross_check"], case["K"])
    assert want.counts.sum() > 0
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(src, case, k)
    r = subprocess.run([driver, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    buf = open(dst, "rb").read()
    P = len(case["pairs"])
    listed, at = read_graph(buf, 0, P)
    resident, at = read_graph(buf, at, P)
    assert at == len(buf)
    for form, got in (("list", listed), ("resident", resident)):
        for fname, a, b in zip(["counts", "offsets", "q", "t", "d2", "stats"], got, want):
            assert a.tobytes() == np.ascontiguousarray(b).tobytes(), f"{name}/{i} {form} form: {fname}"
