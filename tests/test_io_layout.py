"""CPU: where the host-pointer entry points put their arrays in the staging buffer (eacham_amd/csrc/io_layout.hpp), compiled on
its own with g++ and run by tests/cpp/io_layout_driver.cpp. Whatever the order of the declarations: every array on a 256-byte
boundary, none overlapping, the results in one run, then the inputs, then what never leaves the device; the pinned mirror's cut
is where the device-only group starts."""
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, IN, DEV = 0, 1, 2
MAX_ARRAYS = 32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("io_layout") / "io_layout_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "io_layout_driver.cpp")],
                   check=True, capture_output=True)
    return exe


def place(exe, decls):
    text = "".join(f"{r} {e} {c}\n" for r, e, c in decls)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    return json.loads(r.stdout)


def up256(x):
    return (x + 255) // 256 * 256


def check(decls, got):
    assert not got["overflow"]
    arrays = got["arrays"]
    assert [(a["role"], a["bytes"]) for a in arrays] == [(r, e * c) for r, e, c in decls]
    for a in arrays:
        assert a["off"] % 256 == 0
    # no two arrays overlap; each group is one run in declaration order, packed to the alignment; the groups follow each other
    at = 0
    for role in (OUT, IN, DEV):
        if role == DEV:
            assert got["cut"] == at   # the first device-only offset, or the total if there is none
        for a in arrays:
            if a["role"] == role:
                assert a["off"] == at, (role, a, at)
                at = up256(at + a["bytes"])
    assert got["total"] == at


def entry_points(n=5, s=3, p=2):
    """the declaration lists of the nine entry points as their sources state them, at small sizes (n points, s samples, p problems)"""
    d, i, f, b, ll = 8, 4, 4, 1, 8
    return {
        "solve_minimal": [(IN, d, 2 * n), (IN, d, 2 * n), (IN, d, 4), (IN, i, s * 5), (OUT, d, 9 * 10 * s), (OUT, i, s)],
        "solve_pnp": [(IN, d, 3 * n), (IN, d, 2 * n), (IN, d, 4), (IN, i, s * 6), (OUT, d, 12 * s), (OUT, i, s), (DEV, d, 200 * s), (DEV, d, 39 * s)],
        "score_hypotheses": [(IN, d, 2 * n), (IN, d, 2 * n), (IN, d, 9 * s), (IN, d, 4), (OUT, i, s), (OUT, f, s), (OUT, f, n * s)],
        "score_hypotheses_medians_only": [(IN, d, 2 * n), (IN, d, 2 * n), (IN, d, 9 * s), (IN, d, 4), (OUT, i, s), (OUT, f, s), (DEV, f, 0)],
        "triangulate_tracks": [(IN, d, 16 * 4), (IN, d, 4), (IN, i, s + 1), (IN, ll, s + 1), (IN, i, n), (IN, 16, n), (OUT, d, 3 * s), (OUT, i, s),
                               (OUT, b, n), (DEV, i, 7)],
        "reprojection_errors": [(IN, d, 16 * 4), (IN, d, 4), (IN, i, n), (IN, d, 3 * n), (IN, 16, n), (OUT, f, n)],
        "two_view_points": [(IN, 16, n), (IN, 16, n), (IN, d, 4), (IN, d, 16 * 4), (OUT, d, 3 * n * 4), (OUT, b, n * 4)],
        "two_view_batch": [(OUT, i, p), (OUT, i, p), (OUT, i, p), (OUT, i, 4 * p), (OUT, b, n), (OUT, b, n), (OUT, d, 3 * n), (IN, ll, p + 1),
                           (IN, ll, p + 1), (IN, ll, p + 1), (IN, i, p), (IN, d, 4), (IN, d, 16 * 4 * p), (IN, b, 0), (IN, 16, n), (IN, 16, n),
                           (DEV, d, 3 * 4 * n), (DEV, b, 4 * n)],
        "lmeds_batch": [(OUT, d, 9 * p), (OUT, f, p), (OUT, f, p), (OUT, i, p), (OUT, i, 3 * p), (OUT, i, p), (OUT, b, n), (IN, ll, p + 1),
                        (IN, ll, p + 1), (IN, d, 4), (IN, d, 2 * n), (IN, d, 2 * n), (IN, i, s * 5), (DEV, d, 90 * s), (DEV, i, s), (DEV, i, s),
                        (DEV, i, s), (DEV, i, 1), (DEV, i, 0), (DEV, f, 10 * s), (DEV, f, 0)],
        "graph_set_frames": [(IN, i, p), (IN, ll, p + 1), (IN, b, p), (IN, b, n)],
    }


@pytest.mark.parametrize("name", sorted(entry_points()))
def test_entry_point_lists(driver, name):
    decls = entry_points()[name]
    assert len(decls) <= MAX_ARRAYS
    check(decls, place(driver, decls))


@pytest.mark.parametrize("seed", range(8))
def test_declaration_order_does_not_matter(driver, seed):
    rng = random.Random(seed)
    decls = [(rng.choice((OUT, IN, DEV)), rng.choice((1, 4, 8, 16)), rng.choice((0, 1, 7, 31, 32, 33, 255, 256, 257, 16385))) for _ in range(rng.randint(1, MAX_ARRAYS))]
    got = place(driver, decls)
    check(decls, got)
    # the same declarations in another order: the same group sizes, cut and total
    other = decls[:]
    rng.shuffle(other)
    got2 = place(driver, other)
    check(other, got2)
    assert (got2["cut"], got2["total"]) == (got["cut"], got["total"])


def test_no_device_only_group(driver):
    decls = [(IN, 8, 10), (OUT, 4, 3)]
    got = place(driver, decls)
    check(decls, got)
    assert got["cut"] == got["total"] == 512
    assert [a["off"] for a in got["arrays"]] == [256, 0]


def test_zero_length_array_takes_no_room(driver):
    """it starts where its neighbour starts and moves nothing: neither span of the mirror can grow by it"""
    with_it = [(OUT, 4, 3), (OUT, 4, 0), (IN, 8, 10), (IN, 1, 0), (IN, 8, 4), (DEV, 4, 0), (DEV, 4, 9)]
    without = [d for d in with_it if d[2]]
    a, b = place(driver, with_it), place(driver, without)
    check(with_it, a)
    assert (a["cut"], a["total"]) == (b["cut"], b["total"])
    assert [x["off"] for x in a["arrays"] if x["bytes"]] == [x["off"] for x in b["arrays"]]


def test_null_input_still_owns_its_bytes(driver):
    """the layout is not told which host pointers are null: K of solve_minimal has its 32 bytes whether it is copied or not"""
    got = place(driver, entry_points()["solve_minimal"])
    k = got["arrays"][2]
    assert k["bytes"] == 32 and got["arrays"][3]["off"] == k["off"] + 256


def test_too_many_arrays_is_flagged(driver):
    assert not place(driver, [(IN, 4, 1)] * MAX_ARRAYS)["overflow"]
    assert place(driver, [(IN, 4, 1)] * (MAX_ARRAYS + 1))["overflow"]
