"""CPU: how matching cuts a job into launches and lays a launch's arrays into the device workspace
(eacham_amd/csrc/match_plan.hpp, on eacham_amd/csrc/ws_carve.hpp) — compiled on its own with g++ and EXECUTED by
tests/cpp/match_plan_driver.cpp on plain numbers: no frame is uploaded, no device is needed.

The cut. With batch, round and tail of the plan, a job that needs more than one launch goes through two workspace slots as
  1. no launch exceeds batch;
  2. the full launches are whole rounds and differ by at most one round;
  3. with two or more launches the last holds between 1 and tail + round pairs — never the budget's remnant;
  4. the launches sum to the job
(the rules tests/test_match_launch_cut_gpu.py holds on the device, stated again), over that file's ladder of job sizes around every
boundary of the rule, for (tiles of the largest frame, budget) = (20, 16 MiB), (20, 64 MiB), (64, 1 GiB) in both forms of the column
direction; a job of one pair, a budget below one pair's bytes and the one-slot diagnostic form beside them. launch_of, the same
launches as a function of the pair (what match_openprep_kernel computes on the device), gives the launch and start that summing
next_batch gives, at every launch start, the pair before it and the last pair.

The layouts, against an independent statement: the byte formulas of the drivers as they stood before the layouts were declared once
(make_plan's per_pair sum and off_* chain, run_match_metric's call arrays, plan_match_f32, run_match_dot_screened's four offsets,
plan_ham_wide), restated here in Python. Every offset and size must agree, the regions are 256-aligned, disjoint and in the
declared order."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
SLOT_ORDER = ["rowres", "colpart", "matches", "rowcand", "candlist", "colres", "state", "items", "counters", "bytile", "aitems",
              "openlist", "openmask"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("match_plan") / "match_plan_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "match_plan_driver.cpp")],
                   check=True, capture_output=True)
    return exe


def run(exe, jobs):
    r = subprocess.run([exe], input="".join(j + "\n" for j in jobs), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    out = json.loads(r.stdout)
    assert len(out) == len(jobs)
    return out


def plans(exe, max_tiles, budget, full_cols, jobs, no_overlap=False):
    return run(exe, [f"plan {max_tiles} {n} {budget} {int(full_cols)} {int(no_overlap)}" for n in jobs])


@pytest.mark.parametrize("header", ["match_plan.hpp", "ws_carve.hpp"])
def test_the_headers_compile_alone(header, tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text(f'#include "{header}"\nint main() {{ return 0; }}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "eacham_amd", "csrc"), str(src)],
                   check=True, capture_output=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the cut
# ---------------------------------------------------------------------------------------------------------------------------
def sizes_of(p, npairs):
    starts = p["starts"]
    return [b - a for a, b in zip(starts, starts[1:] + [npairs])]


def check_cut(p, npairs):
    sizes, batch, rnd, tail = sizes_of(p, npairs), p["batch"], p["round_pairs"], p["tail_pairs"]
    what = f"npairs {npairs}: launches {sizes}, slots {p['slots']}, batch {batch}, round {rnd}, tail {tail}"
    assert p["starts"][0] == 0 and all(s > 0 for s in sizes) and sum(sizes) == npairs, what          # 4
    assert max(sizes) <= batch, what                                                                  # 1
    if len(sizes) > 1:
        assert p["slots"] == 2, what
        full = sizes[:-1]
        assert all(s % rnd == 0 for s in full) and max(full) - min(full) <= rnd, what                 # 2
        assert 1 <= sizes[-1] <= tail + rnd, what                                                     # 3
        assert len(full) == -(-sum(full) // batch), what                  # as few full launches as the budget allows
    else:
        assert p["slots"] == 1, what
    return sizes


def check_launch_of(p, npairs):
    """launch_of at every launch start, the pair before it and the last pair, against the launches summing next_batch gives."""
    starts = p["starts"]
    asked = {i for s in starts for i in (s - 1, s) if i >= 0} | {npairs - 1}
    got = {i: (l, s) for i, l, s in p["launch_of"]}
    assert set(got) == asked, (npairs, sorted(asked - set(got)))
    for i, (launch, start) in got.items():
        want = max(b for b, s in enumerate(starts) if s <= i)
        assert (launch, start) == (want, starts[want]), (npairs, i, launch, start, starts)


def ladder(exe, max_tiles, budget, full_cols):
    p = plans(exe, max_tiles, budget, full_cols, [10 ** 6])[0]     # the budget's launch, whatever the job
    batch, rnd, tail = p["batch"], p["round_pairs"], p["tail_pairs"]
    jobs = {1, rnd, batch - 1, batch, batch + 1, batch + tail - 1, batch + tail, batch + tail + 1, 2 * batch - 1, 2 * batch,
            2 * batch + 1, 2 * batch + rnd, 1540}
    jobs |= {m * batch + d for m in (3, 5) for d in range(-2, 3)}   # no remnant near a further multiple of the budget's launch
    return batch, rnd, tail, sorted(n for n in jobs if n >= 1)


@pytest.mark.parametrize("full_cols", [False, True])
@pytest.mark.parametrize("max_tiles, budget_mb", [(20, 16), (20, 64), (64, 1024)])
def test_the_cut_over_a_ladder_of_jobs(driver, max_tiles, budget_mb, full_cols):
    batch, rnd, tail, jobs = ladder(driver, max_tiles, budget_mb * MIB, full_cols)
    assert batch >= 2 and 1 <= tail <= max(batch // 8, rnd) and batch % rnd == 0
    if budget_mb == 16:
        assert 2 * batch < 1540                                    # 1 540 pairs are at least three launches
    for n, p in zip(jobs, plans(driver, max_tiles, budget_mb * MIB, full_cols, jobs)):
        sizes = check_cut(p, n)
        check_launch_of(p, n)
        if n > batch + rnd:                                        # (up to a round more may fit the budget as one launch)
            assert len(sizes) >= 2, (n, sizes)


def test_the_cut_of_the_headline_job(driver):
    """S200: 19 900 pairs of 2000-row frames (64 tiles) under 1 GiB, lean form: 109 072 bytes per pair, 9 792 pairs per launch in
    rounds of 64 — two equal launches and a short one, where full launches once left 9 792 + 9 792 + 316."""
    p = plans(driver, 64, 1024 * MIB, False, [19900])[0]
    assert p["per_pair"] == 109072
    assert (p["batch"], p["round_pairs"], p["tail_pairs"]) == (9792, 64, 1216)
    assert check_cut(p, 19900) == [9344, 9344, 1212]
    check_launch_of(p, 19900)


def test_one_pair_a_starved_budget_and_one_slot(driver):
    for full_cols in (False, True):
        p = plans(driver, 20, 16 * MIB, full_cols, [1])[0]
        assert check_cut(p, 1) == [1] and (p["batch"], p["slots"]) == (1, 1)
        check_launch_of(p, 1)
        # a budget below one pair's bytes: launches of one pair, the unit of the rule is the pair
        jobs = [1, 2, 3, 5, 64, 1540]
        for n, p in zip(jobs, plans(driver, 20, 1000, full_cols, jobs)):
            assert p["per_pair"] > 1000 and (p["batch"], p["round_pairs"], p["tail_pairs"]) == (1, 1, 1)
            assert check_cut(p, n) == [1] * n
            check_launch_of(p, n)
        # the diagnostic one-slot form: full batches and the remnant
        batch, rnd, tail, jobs = ladder(driver, 20, 16 * MIB, full_cols)
        for n, p in zip(jobs, plans(driver, 20, 16 * MIB, full_cols, jobs, no_overlap=True)):
            b = p["batch"]
            assert p["slots"] == 1 and b <= batch + rnd and p["total"] == p["slot_bytes"]
            assert sizes_of(p, n) == [b] * (n // b) + ([n % b] if n % b else []), (n, b, p["starts"])
            check_launch_of(p, n)


# ---------------------------------------------------------------------------------------------------------------------------
# the layouts against the formulas they replaced
# ---------------------------------------------------------------------------------------------------------------------------
def align(x):
    return (x + 255) & ~255


INT, INT2, UINT2, FLOAT2, INT4, UINT4, U64 = 4, 8, 8, 8, 16, 16, 8


def former_plan(max_tiles, npairs, budget, full_cols, no_overlap=False):
    """make_plan / next_batch / run_match_metric as they computed bytes and launches before match_plan.hpp: a closed-form per_pair
    sum, a chain of hand-aligned offsets, the call arrays as pointer arithmetic behind `total`."""
    rs = max_tiles * 32
    wb = (max_tiles + 8 - 1) // 8 + 1
    wgs_per_pair = (max_tiles + 8 - 1) // 8
    col_chunks = (max_tiles + 128 - 1) // 128
    colpart_pp = wb * rs * INT2 if full_cols else 0
    cand_pp = 0 if full_cols else rs * (UINT2 + 3 * INT + UINT2) + INT4 + max_tiles * (INT2 + 2 * INT4)
    per_pair = col_chunks * rs * INT4 + rs * UINT2 + colpart_pp + cand_pp
    batch = min(max(budget // per_pair, 1), npairs)
    wgs = wgs_per_pair * col_chunks
    round_pairs = 512
    g = 512
    while g >= 1:
        if wgs % g == 0:
            round_pairs = 512 // g
            break
        g >>= 1
    if batch < npairs and batch > round_pairs:
        batch -= batch % round_pairs
    if batch >= npairs and npairs >= 8 * round_pairs:
        batch = ((npairs + 1) // 2 + round_pairs - 1) // round_pairs * round_pairs
    batch = max(batch, 1)
    rp = round_pairs if batch % round_pairs == 0 else 1
    slots = 2 if (batch < npairs and not no_overlap) else 1
    tail = max(rp, batch // 8 // rp * rp)
    full_launches = full_rounds = long_launches = 0
    if slots == 2:
        last_max = min(tail, batch)
        rounds = (npairs - last_max + rp - 1) // rp
        full_launches = (rounds * rp + batch - 1) // batch
        full_rounds = rounds // full_launches
        long_launches = rounds % full_launches
    off, size = {}, {}
    cb = 0 if full_cols else batch
    mask_stride = (rs + 63) // 64
    size["rowres"] = batch * col_chunks * rs * INT4
    size["colpart"] = batch * wb * rs * INT2 if full_cols else 0
    size["matches"] = batch * rs * UINT2
    size["rowcand"] = cb * rs * UINT2
    size["candlist"] = cb * rs * INT
    size["colres"] = cb * rs * UINT2
    size["state"] = cb * INT4
    size["items"] = cb * max_tiles * INT2
    size["counters"] = 256
    size["bytile"] = cb * rs * INT
    size["aitems"] = cb * 2 * max_tiles * INT4
    size["openlist"] = cb * rs * INT
    size["openmask"] = cb * mask_stride * U64
    at = 0
    for name in SLOT_ORDER:            # off_x = align(off_previous + bytes of the previous)
        off[name] = at
        at = align(at + size[name])
    slot_bytes = at
    starts, first, b = [], 0, 0
    while first < npairs:
        starts.append(first)
        if slots == 2 and b < full_launches:
            first += (full_rounds + (1 if b < long_launches else 0)) * rp
        else:
            first += min(batch, npairs - first)
        b += 1
    call_pairs = (npairs + 63) & ~63
    return dict(batch=batch, round_pairs=rp, tail_pairs=tail, full_launches=full_launches, full_rounds=full_rounds,
                long_launches=long_launches, slots=slots, wgs_per_pair=wgs_per_pair, wb_stride=wb, row_stride=rs, col_chunks=col_chunks,
                mask_stride=mask_stride, per_pair=per_pair, slot_bytes=slot_bytes, total=slot_bytes * slots, starts=starts,
                off=off, size=size, seghead=slot_bytes * slots, segcount=slot_bytes * slots + INT * call_pairs,
                launch_items=slot_bytes * slots + 2 * INT * call_pairs, call_bytes=(2 * call_pairs + len(starts)) * INT)


@pytest.mark.parametrize("full_cols", [False, True])
@pytest.mark.parametrize("max_tiles", [4, 20, 63, 64, 129, 512])
def test_the_slot_layout_is_the_former_one(driver, max_tiles, full_cols):
    cases = [(n, mb * MIB) for n in (1, 7, 1000, 1540, 19900) for mb in (16, 1024)]
    got = run(driver, [f"plan {max_tiles} {n} {budget} {int(full_cols)} 0" for n, budget in cases])
    for (n, budget), p in zip(cases, got):
        want = former_plan(max_tiles, n, budget, full_cols)
        what = f"{max_tiles} tiles, {n} pairs, {budget >> 20} MiB, full_cols {full_cols}"
        for key in ("batch", "round_pairs", "tail_pairs", "full_launches", "full_rounds", "long_launches", "slots", "wgs_per_pair",
                    "wb_stride", "row_stride", "col_chunks", "mask_stride", "per_pair", "slot_bytes", "total", "starts", "seghead",
                    "segcount", "launch_items", "call_bytes"):
            assert p[key] == want[key], (what, key, p[key], want[key])
        assert p["col_chunks"] == (2 if max_tiles == 129 else 4 if max_tiles == 512 else 1)
        assert p["null_base_gives_null"] == 1 and p["counters"] == [0, 32, 64, 128]      # n_items, n_pre, n_aitems at ints 0, 8, 16 of 32
        for k, slot in ((0, p["slot0"]), (p["slots"] - 1, p["slot1"])):
            base, end = k * want["slot_bytes"], k * want["slot_bytes"]
            for name in SLOT_ORDER:
                if want["size"][name] == 0:          # an array the form does not have: no pointer, no bytes
                    assert slot[name] == -1, (what, name)
                    continue
                assert slot[name] == base + want["off"][name], (what, k, name, slot[name], want["off"][name])
                assert slot[name] % 256 == 0 and slot[name] >= end, (what, k, name)      # aligned, behind its predecessor's end
                end = slot[name] + want["size"][name]
            assert end <= base + p["slot_bytes"], (what, k)
        absent = {name for name in SLOT_ORDER if p["slot0"][name] == -1}
        assert absent == ({"rowcand", "candlist", "colres", "state", "items", "bytile", "aitems", "openlist", "openmask"} if full_cols
                          else {"colpart"}), (what, absent)
        # the call arrays lie behind the last slot, one after the other, and end with the last launch's counter
        assert p["seghead"] == p["total"] and p["seghead"] % 256 == 0
        assert p["seghead"] + 4 * n <= p["segcount"] and p["segcount"] + 4 * n <= p["launch_items"]
        assert p["launch_items"] + 4 * len(p["starts"]) == p["total"] + p["call_bytes"]


def former_f32(max_tiles, npairs):
    """plan_match_f32 and the four offsets run_match_dot_screened put behind its total."""
    rs, wb = max_tiles * 32, max_tiles
    per_pair = rs * INT4 + wb * rs * INT4 + rs * UINT2 + INT
    batch = max(1, min((1 << 30) // per_pair, npairs))
    off = {"rowres": 0}
    off["colpart"] = align(batch * rs * INT4)
    off["matches"] = align(off["colpart"] + batch * wb * rs * INT4)
    total = align(off["matches"] + batch * rs * UINT2)
    off["rr16"] = total
    off["cp16"] = align(off["rr16"] + batch * rs * INT4)
    off["open_idx"] = align(off["cp16"] + batch * wb * rs * INT4)
    off["open_cnt"] = align(off["open_idx"] + batch * 2 * rs * INT)
    total_screened = align(off["open_cnt"] + batch * INT2)
    size = dict(rowres=batch * rs * INT4, colpart=batch * wb * rs * INT4, matches=batch * rs * UINT2, rr16=batch * rs * INT4,
                cp16=batch * wb * rs * INT4, open_idx=batch * 2 * rs * INT, open_cnt=batch * INT2)
    return dict(batch=batch, row_stride=rs, wb_stride=wb, wgs_per_pair=(max_tiles + 3) // 4, total=total, total_screened=total_screened,
                off=off, size=size)


@pytest.mark.parametrize("max_tiles", [4, 20, 63, 64, 129, 512])
def test_the_float_layouts_are_the_former_ones(driver, max_tiles):
    jobs = (1, 7, 1000, 19900)
    for n, p in zip(jobs, run(driver, [f"f32 {max_tiles} {n}" for n in jobs])):
        want = former_f32(max_tiles, n)
        for key in ("batch", "row_stride", "wb_stride", "wgs_per_pair", "total", "total_screened"):
            assert p[key] == want[key], (max_tiles, n, key, p[key], want[key])
        assert p["carved"] == [want["total"], want["total_screened"]]
        assert p["rowres_dot"] == p["rowres"] and p["colpart_dot"] == p["colpart"]     # the dot-product form's view of the same arrays
        end = 0
        for name in ("rowres", "colpart", "matches", "rr16", "cp16", "open_idx", "open_cnt"):
            assert p[name] == want["off"][name], (max_tiles, n, name, p[name], want["off"][name])
            assert p[name] % 256 == 0 and p[name] >= end, (max_tiles, n, name)
            end = p[name] + want["size"][name]
        assert end <= p["total_screened"] and p["matches"] + want["size"]["matches"] <= p["total"]


@pytest.mark.parametrize("max_tiles", [2, 4, 20, 63, 64, 129, 512])
def test_the_wide_hamming_layout_is_the_former_one(driver, max_tiles):
    cases = [(n, budget) for n in (0, 1, 7, 1000, 19900) for budget in (1000, 16 * MIB, 1024 * MIB)]
    for (n, budget), p in zip(cases, run(driver, [f"wide {max_tiles} {n} {budget}" for n, budget in cases])):
        rs = 32 * max_tiles                                      # plan_ham_wide
        per_pair = rs * (2 * FLOAT2 + UINT2)
        batch = min(max(budget // per_pair, 1), max(n, 1))
        off_matches = (batch * 2 * rs * FLOAT2 + 255) & ~255
        total = off_matches + batch * rs * UINT2
        assert (p["batch"], p["row_stride"], p["wgs_per_pair"]) == (batch, rs, (max_tiles + 7) // 8), (max_tiles, n, budget, p)
        assert (p["rowres"], p["matches"], p["total"]) == (0, off_matches, total), (max_tiles, n, budget, p)
        assert p["matches"] % 256 == 0 and p["matches"] >= batch * 2 * rs * FLOAT2
