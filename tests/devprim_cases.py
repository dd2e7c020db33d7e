"""The cases tests/test_devprim_gpu.py runs through tests/cpp/devprim_driver.hip, their file format and their references.

The references are plain numpy on int64: an exclusive np.cumsum, np.argsort(keys & mask, kind="stable"), np.searchsorted.
Every comparison made with them is exact. What the case builder asserts here, on the CPU, are conditions on the INPUTS
(every int prefix and total below 2^31), never on the code under test.

Constants restated from DESIGN.md §4.1a (not read from the code under test)."""
import functools
import struct

import numpy as np

SCAN_TILE = 2048          # elements per workgroup of the scan
SCAN_SMALL = 16384        # one workgroup up to here, three launches above
RS_SEG = 512              # elements per wave of the sort
RS_MAX_BITS = 10          # bits per pass at the most
GUARD = 256
GUARD_BYTE = 0xC3
FILL_BYTE = 0x5A

# ---- scan ------------------------------------------------------------------------------------------------------------
SCAN_TYPES = {"int": (0, np.int32, 1), "ll": (1, np.int64, 1), "i3": (2, np.int32, 3)}   # id, dtype, fields
ONE_ROUND = SCAN_TILE * SCAN_TILE   # 4 194 304: 2048 tile sums, the most ONE round of scan_sums takes
SCAN_LARGE = [ONE_ROUND, ONE_ROUND + 1, ONE_ROUND + 9 * SCAN_TILE + 5]
SCAN_SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, 16383, 16384, 16385, 18432, 18433] + SCAN_LARGE
# a form: bit 0 = in place (out == in), bit 1 = total_dev given: all four at every size
ALL_FORMS = [0, 1, 2, 3]


def scan_forms(n):
    return ALL_FORMS


def scan_input_names(tname, n):
    if tname == "int":
        return ["flags", "bytes"]    # 0/1 flags as the products scan them, and [0, 256): 1.07e9 at the largest size
    return ["big"] if tname == "ll" else ["streams"]


@functools.lru_cache(maxsize=None)
def scan_input(tname, which, n):
    _, dt, _ = SCAN_TYPES[tname]
    rng = np.random.default_rng([n, len(which), SCAN_TYPES[tname][0]])
    if tname == "int":
        x = rng.integers(0, 2 if which == "flags" else 256, n)
    elif tname == "ll":
        x = rng.integers(0, 1 << 40, n)        # every prefix beyond the first few exceeds 2^32
    else:                                      # three independent streams of different ranges
        x = np.stack([rng.integers(0, 2, n), rng.integers(0, 7, n), rng.integers(0, 256, n)], axis=1)
    x = np.ascontiguousarray(x.astype(dt))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def scan_reference(tname, which, n):
    """(exclusive prefix sums, total), computed on int64 and cast to the type."""
    _, dt, fields = SCAN_TYPES[tname]
    x = scan_input(tname, which, n).astype(np.int64)
    inc = np.cumsum(x, axis=0, dtype=np.int64)
    zero = np.zeros((1,) + x.shape[1:], dtype=np.int64)
    excl = np.concatenate([zero, inc[:-1]], axis=0) if n else inc
    total = inc[-1] if n else zero[0]
    if dt == np.int32:   # a condition on the inputs: the int scans never wrap
        assert n == 0 or int(inc.max()) < 2 ** 31
    else:
        assert n < 10 or int(excl[9]) > 2 ** 32
    excl, total = np.ascontiguousarray(excl.astype(dt)), np.asarray(total, dtype=dt).reshape(fields)
    excl.setflags(write=False)
    return excl, total


def scan_case_name(tname, which, n):
    return f"scan/{tname}/{which}/{n}"


# ---- sort ------------------------------------------------------------------------------------------------------------
SORT_VALUES = {"u32": 0, "int2": 1}
SORT_SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 8192, 8193, 100003]
KEY_BITS = [1, 2, 5, 9, 10, 11, 16, 20, 21, 30, 31, 32]
SORT_LARGE = 2097153 + 777     # 4098 segments: the 10-bit histogram has 4 196 352 entries, scan_sums runs a second round
LARGE_KEY_BITS = [10, 20, 32]
PATTERNS = ["a_uniform32", "b_equal", "c_alternating", "d_ascending", "d_descending", "e_eight_runs", "f_distinct_rounds"]
LARGE_PATTERNS = ["a_uniform32", "b_equal", "e_eight_runs"]


def sort_patterns(n):
    return PATTERNS if n <= 8193 else LARGE_PATTERNS


def sort_key_bits(n):
    return LARGE_KEY_BITS if n == SORT_LARGE else KEY_BITS


@functools.lru_cache(maxsize=None)
def sort_keys(pattern, n):
    rng = np.random.default_rng([n, PATTERNS.index(pattern)])
    i = np.arange(n, dtype=np.int64)
    if pattern == "a_uniform32":            # bits above key_bits are set: ignored for the order, carried through
        k = rng.integers(0, 1 << 32, n)
    elif pattern == "b_equal":              # every lane a peer of every other
        k = np.full(n, 0x9E3779B9)
    elif pattern == "c_alternating":        # two values that differ in every bit
        k = np.where(i & 1, 0x5A5A5A5A, 0xA5A5A5A5)
    elif pattern == "d_ascending":
        k = i
    elif pattern == "d_descending":
        k = n - 1 - i
    elif pattern == "e_eight_runs":         # eight distinct values in runs of 1..300: across rounds of 64 and segments of 512
        vals = rng.integers(0, 1 << 32, 8)
        vals[:4] = (vals[:4] & ~0x3) | np.arange(4)          # (distinct even in the lowest two bits)
        runs = rng.integers(1, 301, n // 100 + 2)
        k = np.repeat(vals[rng.integers(0, 8, runs.size)], runs)
        k = np.resize(k, n) if k.size < n else k[:n]
    elif pattern == "f_distinct_rounds":
        # every round of 64 is a permutation p of 0..63, repeated every 6 bits: any window of >= 6 bits holds a
        # rotation of p's bits, so a first pass of >= 6 bits meets 64 distinct digits in every round
        rounds = (n + 63) // 64
        p = np.argsort(rng.random((rounds, 64)), axis=1).reshape(-1)[:n].astype(np.int64)
        k = (p | p << 6 | p << 12 | p << 18 | p << 24 | p << 30) & 0xFFFFFFFF
    else:
        raise KeyError(pattern)
    k = np.ascontiguousarray(np.asarray(k, dtype=np.int64).astype(np.uint32))
    assert k.size == n
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=64)
def sort_reference(pattern, n, key_bits):
    """(keys, index) of the stable sort by the low key_bits; the value of element i is i (u32) or (i, ~i) (int2)."""
    keys = sort_keys(pattern, n)
    perm = np.argsort(keys.astype(np.int64) & ((1 << key_bits) - 1), kind="stable")
    return keys[perm], perm.astype(np.uint32)


def sort_values(vname, index):
    if vname == "u32":
        return index
    return np.stack([index.view(np.int32), (~index).view(np.int32)], axis=1)


def sort_case_name(vname, pattern, n):
    return f"sort/{vname}/{pattern}/{n}"


NOOP_CAP = 64
NOOPS = [("n0", 0, 10), ("n_negative", -1, 10), ("bits0", NOOP_CAP, 0)]   # name, n, key_bits: returns 0, writes nothing


# ---- segment_of --------------------------------------------------------------------------------------------------------
SEG_TYPES = {"int": (0, np.int32), "ll": (1, np.int64)}


@functools.lru_cache(maxsize=None)
def segof_cases():
    """name -> (type name, ptr, v)."""
    rng = np.random.default_rng(77)
    small = {"n1": [5], "n2": [0, 4], "n2_equal": [3, 3], "n3": [0, 2, 7], "n3_all_equal": [1, 1, 1],
             "n3_empty_first": [0, 0, 5], "n3_empty_last": [0, 5, 5]}
    big = {"n1000_ascending": np.cumsum(rng.integers(1, 10, 1000)),
           "n1000_empty_runs": np.cumsum(rng.integers(0, 4, 1000) * (rng.random(1000) < 0.4))}
    out = {}
    for tname, (_, dt) in SEG_TYPES.items():
        offsets = {"": 0} if tname == "int" else {"": 0, "_above_2p31": (1 << 31) + 12345, "_above_2p40": (1 << 40) + 7}
        for suffix, off in offsets.items():
            for name, p in small.items():
                p = np.asarray(p, dtype=np.int64) + off
                out[f"segof/{tname}/{name}{suffix}"] = (tname, p.astype(dt), np.arange(p[0], p[-1] + 3, dtype=np.int64))
            for name, p in big.items():
                p = p.astype(np.int64) + off
                below = p - 1
                v = np.concatenate([p, below[below >= p[0]], rng.integers(p[0], p[-1] + 3, 500), p[-1] + np.arange(3)])
                out[f"segof/{tname}/{name}{suffix}"] = (tname, p.astype(dt), v.astype(np.int64))
    return out


def segof_reference(ptr, v):
    return (np.searchsorted(ptr.astype(np.int64), v, side="right") - 1).astype(np.int32)


# ---- the files -------------------------------------------------------------------------------------------------------
def _framed(f, a):
    a = np.ascontiguousarray(a)
    f.write(struct.pack("qq", a.size // (a.shape[-1] if a.ndim == 2 else 1), a.itemsize * (a.shape[-1] if a.ndim == 2 else 1)))
    f.write(a.tobytes() if a.nbytes < (1 << 20) else memoryview(a).cast("B"))


def _head(f, kind, name, type_id):
    f.write(struct.pack("ii", kind, len(name)) + name.encode() + struct.pack("i", type_id))


@functools.lru_cache(maxsize=None)
def case_list():
    """The cases in file order: tuples whose first field is the kind."""
    cases = []
    for tname in SCAN_TYPES:
        for n in SCAN_SIZES:
            for which in scan_input_names(tname, n):
                cases.append(("scan", tname, which, n))
    for vname in SORT_VALUES:
        for n in SORT_SIZES + [SORT_LARGE]:
            for pattern in sort_patterns(n):
                cases.append(("sort", vname, pattern, n))
        for name, n, kb in NOOPS:
            cases.append(("noop", vname, name, n, kb))
    for name in segof_cases():
        cases.append(("segof", name))
    return cases


def write_case_file(path):
    cases = case_list()
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            if c[0] == "scan":
                _, tname, which, n = c
                forms = scan_forms(n)
                _head(f, 0, scan_case_name(tname, which, n), SCAN_TYPES[tname][0])
                f.write(struct.pack(f"ii{len(forms)}i", n, len(forms), *forms))
                _framed(f, scan_input(tname, which, n))
            elif c[0] == "sort":
                _, vname, pattern, n = c
                kbs = sort_key_bits(n)
                _head(f, 1, sort_case_name(vname, pattern, n), SORT_VALUES[vname])
                f.write(struct.pack(f"iii{len(kbs)}i", n, 0, len(kbs), *kbs))
                _framed(f, sort_keys(pattern, n))
            elif c[0] == "noop":
                _, vname, name, n, kb = c
                _head(f, 1, f"sort/{vname}/noop_{name}", SORT_VALUES[vname])
                f.write(struct.pack("iiii", n, 1, 1, kb))
                _framed(f, sort_keys("a_uniform32", NOOP_CAP))
            else:
                tname, ptr, v = segof_cases()[c[1]]
                _head(f, 2, c[1], SEG_TYPES[tname][0])
                _framed(f, ptr)
                _framed(f, v)


class _Reader:
    def __init__(self, path):
        self.mem = np.memmap(path, dtype=np.uint8, mode="r")
        self.at = 0

    def take(self, dtype, fields=1):
        n, size = struct.unpack("qq", self.mem[self.at:self.at + 16].tobytes())
        assert size == np.dtype(dtype).itemsize * fields, (size, dtype, fields)
        a = self.mem[self.at + 16:self.at + 16 + n * size].view(dtype)
        self.at += 16 + n * size
        return a.reshape(n, fields) if fields > 1 else a


def read_result_file(path):
    """name -> result, as views of the mapped file. scan: {form: dict(out, guards, total, input)}; sort: {key_bits:
    dict(runs=[(rc, keys, values)] * 2, guards)}; noop: dict(runs=[(rc, ka, va, kb, vb)] * 2, guards); segof: the array.
    '_driver_ms' is the driver's own wall time."""
    r, res = _Reader(path), {}
    for c in case_list():
        if c[0] == "scan":
            _, tname, which, n = c
            _, dt, fields = SCAN_TYPES[tname]
            forms = {}
            for form in scan_forms(n):
                d = {"out": r.take(dt, fields), "guards": r.take(np.uint8), "total": r.take(dt, fields).reshape(fields)}
                d["input"] = None if form & 1 else r.take(dt, fields)
                forms[form] = d
            res[scan_case_name(tname, which, n)] = forms
        elif c[0] in ("sort", "noop"):
            vname = c[1]
            vt = (np.uint32, 1) if vname == "u32" else (np.int32, 2)
            per_kb = {}
            for kb in (sort_key_bits(c[3]) if c[0] == "sort" else [c[4]]):
                runs = []
                for _ in range(2):
                    rc = int(r.take(np.int32)[0])
                    pairs = 2 if c[0] == "noop" else 1
                    arrays = []
                    for _ in range(pairs):
                        arrays += [r.take(np.uint32), r.take(*vt)]
                    runs.append((rc, *arrays))
                per_kb[kb] = {"runs": runs, "guards": r.take(np.uint8)}
            if c[0] == "sort":
                res[sort_case_name(vname, c[2], c[3])] = per_kb
            else:
                res[f"sort/{vname}/noop_{c[2]}"] = per_kb[c[4]]
        else:
            res[c[1]] = r.take(np.int32)
    res["_driver_ms"] = float(r.take(np.float64)[0])
    assert r.at == r.mem.size, "trailing bytes in the result file"
    return res


def guards_intact(guards):
    return guards.size > 0 and guards.size % (2 * GUARD) == 0 and bool((guards == GUARD_BYTE).all())


# ---- the workspace bounds test_devprim_host.py holds the helpers to --------------------------------------------------------
def scan_ws_needed(n):
    """tile sums the three-launch form writes: one per tile of SCAN_TILE elements."""
    return -(-n // SCAN_TILE)


def radix_ws_needed(n):
    """the widest pass: a histogram of RS_MAX_BITS bits per segment of RS_SEG elements, then the scan workspace of that
    many elements right behind it (the passes place it at nseg << RS_MAX_BITS whatever their width)."""
    h = -(-n // RS_SEG) << RS_MAX_BITS
    return h + scan_ws_needed(h)
