"""GPU: the primitives of eacham_amd/csrc/devprim.hpp called directly (tests/cpp/devprim_driver.hip, built by build() into
eacham_amd/lib/exp/devprim_driver) and held to exact references (tests/devprim_cases.py): the exclusive scan for int,
long long and I3 on both sides of every size at which it takes another path, the stable radix sort for every pass split
and at the segment, workgroup and histogram-scan edges on tie-heavy inputs, segment_of with empty segments and 64-bit
offsets. Every buffer a primitive writes lies between guards; every comparison is exact.

The driver runs ONCE for the module (one process with the GPU open); the tests only read its result file.
EACHAM_DEVPRIM_DRIVER names another driver binary (a build against a deliberately wrong devprim.hpp must fail here)."""
import os
import subprocess
import time

import numpy as np
import pytest

import devprim_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "eacham_amd", "lib", "exp", "devprim_driver")
# the driver's whole run (reading 0.41 GB of cases, every launch, writing 3.1 GB of results to the temporary directory)
# measured 1.8-1.9 s by wall on an MI355X machine (1.5-1.6 s by its own clock): the limit is 30 x that
DRIVER_TIMEOUT_S = 60

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = os.environ.get("EACHAM_DEVPRIM_DRIVER", DRIVER)
    assert os.path.isfile(exe), f"{exe} is missing: build() makes it (make -C eacham_amd/csrc devprim_driver)"
    d = tmp_path_factory.mktemp("devprim")
    fin, fout = str(d / "cases.bin"), str(d / "results.bin")
    t0 = time.perf_counter()
    DC.write_case_file(fin)
    t1 = time.perf_counter()
    try:
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=DRIVER_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the driver did not finish within {DRIVER_TIMEOUT_S} s: {e.stderr!r}")
    finally:
        os.unlink(fin)
    t2 = time.perf_counter()
    assert r.returncode == 0, f"driver exit {r.returncode}: {r.stdout[-2000:]}{r.stderr[-2000:]}"
    res = DC.read_result_file(fout)
    os.unlink(fout)   # (the mapping keeps the data until the module is done)
    print(f"\ndevprim: cases written in {t1 - t0:.2f} s, driver {t2 - t1:.2f} s by wall ({res['_driver_ms'] / 1e3:.2f} s its own), "
          f"{os.path.basename(exe)}")
    return res


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.array_equal(got, want))


# ---- scan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", DC.SCAN_SIZES)
@pytest.mark.parametrize("tname", list(DC.SCAN_TYPES))
def test_exclusive_scan(results, tname, n):
    bad = []
    for which in DC.scan_input_names(tname, n):
        want, want_total = DC.scan_reference(tname, which, n)
        x = DC.scan_input(tname, which, n)
        for form, got in results[DC.scan_case_name(tname, which, n)].items():
            tag = f"{which}, {'in place' if form & 1 else 'out of place'}, {'total' if form & 2 else 'null total'}"
            if not same(got["out"], want):
                first = np.argwhere(got["out"] != want)[:1].tolist() if got["out"].shape == want.shape else "shape"
                bad.append(f"{tag}: out differs from the exclusive cumsum, first at {first}")
            if not DC.guards_intact(got["guards"]) or got["guards"].size != 6 * DC.GUARD:
                bad.append(f"{tag}: a guard of out / ws / total was written (out[n] is the guard behind out)")
            if form & 2:
                if not same(got["total"], want_total):
                    bad.append(f"{tag}: total {got['total']} != {want_total}")
            elif not (got["total"].view(np.uint8) == DC.FILL_BYTE).all():
                bad.append(f"{tag}: a null total_dev, and the buffer beside it was written")
            if not form & 1 and not same(got["input"], x):
                bad.append(f"{tag}: the input of an out-of-place scan changed")
    assert not bad, "\n".join(bad)


# ---- sort ------------------------------------------------------------------------------------------------------------
def check_sort(results, vname, n, key_bits):
    bad = []
    for pattern in DC.sort_patterns(n):
        got = results[DC.sort_case_name(vname, pattern, n)][key_bits]
        want_keys, index = DC.sort_reference(pattern, n, key_bits)
        want_vals = DC.sort_values(vname, index)
        (rc0, k0, v0), (rc1, k1, v1) = got["runs"]
        if rc0 != (-(-key_bits // DC.RS_MAX_BITS)) % 2:
            bad.append(f"{pattern}: returned {rc0} after {-(-key_bits // DC.RS_MAX_BITS)} passes")
        if not same(k0, want_keys):
            bad.append(f"{pattern}: keys are not the input's keys in the reference order (all 32 bits compared)")
        if not same(v0, want_vals):
            bad.append(f"{pattern}: values are not the stable permutation")
        if rc1 != rc0 or k1.tobytes() != k0.tobytes() or v1.tobytes() != v0.tobytes():
            bad.append(f"{pattern}: the second run differs from the first")
        if not DC.guards_intact(got["guards"]) or got["guards"].size != 10 * DC.GUARD:
            bad.append(f"{pattern}: a guard of ka / va / kb / vb / ws was written")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("key_bits", DC.KEY_BITS)
@pytest.mark.parametrize("n", DC.SORT_SIZES)
@pytest.mark.parametrize("vname", list(DC.SORT_VALUES))
def test_radix_sort_pairs(results, vname, n, key_bits):
    check_sort(results, vname, n, key_bits)


@pytest.mark.parametrize("key_bits", DC.LARGE_KEY_BITS)
@pytest.mark.parametrize("vname", list(DC.SORT_VALUES))
def test_radix_sort_pairs_second_round_of_scan_sums(results, vname, key_bits):
    assert (-(-DC.SORT_LARGE // DC.RS_SEG)) << 10 > DC.ONE_ROUND
    check_sort(results, vname, DC.SORT_LARGE, key_bits)


@pytest.mark.parametrize("name", [c[0] for c in DC.NOOPS])
@pytest.mark.parametrize("vname", list(DC.SORT_VALUES))
def test_radix_sort_pairs_nothing_to_do(results, vname, name):
    got = results[f"sort/{vname}/noop_{name}"]
    keys = DC.sort_keys("a_uniform32", DC.NOOP_CAP)
    vals = DC.sort_values(vname, np.arange(DC.NOOP_CAP, dtype=np.uint32))
    for rc, ka, va, kb, vb in got["runs"]:
        assert rc == 0
        assert same(ka, keys) and same(va, vals), "the input pair was written"
        assert (kb.view(np.uint8) == DC.FILL_BYTE).all() and (vb.view(np.uint8) == DC.FILL_BYTE).all(), "the other pair was written"
    assert DC.guards_intact(got["guards"])


# ---- segment_of --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.segof_cases()))
def test_segment_of(results, name):
    _, ptr, v = DC.segof_cases()[name]
    assert (np.diff(ptr.astype(np.int64)) >= 0).all() and (v >= ptr[0]).all()     # the call's preconditions
    want = DC.segof_reference(ptr, v)
    got = results[name]
    assert same(got, want), f"first difference at v = {v[np.nonzero(got != want)[0][:1]]}" if got.shape == want.shape else "shape"
