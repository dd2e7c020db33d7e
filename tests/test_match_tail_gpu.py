"""GPU: the end of a pair under every kind of resident frame — int8 (both finalize kernels of matcher.hip), float under L2 and
under the dot product, binary rows on the int8 path, wide binary rows — on ONE set of cases built for what the kinds share
(eacham_amd/csrc/match_tail.hpp): the ordered compaction in chunks of 256 query rows, the edge rule and its two inequalities,
counts and stats, and the dynamic LDS of a tail kernel above 48 KiB. counts, offsets, q, t, the values and stats are compared as
bytes against the references that exist: tests/np_reference.py (L2; the float kind takes it too, on rows whose distances are
integers below 2^24 and therefore exact in fp32 in any order), tests/dot_reference.py, tests/ham_reference.py.

The rows are bits. A frame is an N x 256 matrix of 0 / 1 with 128 ones per row: uploaded as such by the int8 and float kinds (its
squared L2 distance is the Hamming distance, its dot product the number of common ones) and packed to 32 bytes by the binary kinds.
Two random rows lie ~128 bits apart with ~64 common ones, so a random query row fails every predicate (the two nearest of 300 are
at ~100 and ~102); a query row that is a train row with one to three ones cleared passes every one of them, both ways. Which rows
are kept is therefore chosen by the case, not found."""
import ctypes as C
import functools

import numpy as np
import pytest

from eacham_amd import synth
import dot_reference as DR
import ham_cases as HC
import ham_reference as HR
import np_reference as NR

pytestmark = pytest.mark.gpu

RATIO = 0.8
MIN_SCORE = 110.0   # common ones: a copy shares >= 124 with its original, two random rows 64 +- 4
NBITS = 256
KINDS = ("int8", "f32", "dot", "bits", "wide")
FAMILY = {"int8": "l2", "f32": "l2", "dot": "dot", "bits": "ham", "wide": "ham"}


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _rows(seed, stream, n):
    """n x 256 bits, 128 ones in every row."""
    order = np.argsort(synth.rng_u64(seed, stream, np.arange(n * NBITS, dtype=np.uint64)).reshape(n, NBITS), axis=1, kind="stable")
    bits = np.zeros((n, NBITS), np.uint8)
    np.put_along_axis(bits, order[:, : NBITS // 2], 1, axis=1)
    return bits


def _cleared(row, k):
    """The row with its first k ones cleared."""
    out = row.copy()
    out[np.nonzero(row)[0][:k]] = 0
    return out


def _pair(seed, nq, nt, kept):
    """(query, train) bits: query row kept[i] is train row tsel[i] with 1 + i % 3 ones cleared (a mutual match); every other row of
    both is random. One more train row is the FIRST kept query row with three more ones cleared: that query row still prefers its
    own train row (1 bit against 3), the extra train row's nearest query row is it — |m21| = |m12| + 1 = |mutual| + 1."""
    Q, T = _rows(seed, 1, nq), _rows(seed, 2, nt)
    tsel = synth.rng_permutation(seed, 3, nt)
    for i, q in enumerate(kept):
        Q[q] = _cleared(T[tsel[i]], 1 if i == 0 else 1 + i % 3)
    if kept and nt > len(kept):
        T[tsel[len(kept)]] = _cleared(Q[kept[0]], 3)
    return Q, T


# name -> (query rows, train rows, the query rows that keep a match). Chunks of the compaction are 256 query rows: kept rows at both
# ends of a chunk, on both sides of every boundary and in the last, partial chunk; "hole": the whole first chunk keeps nothing.
CHUNK_CASES = {
    "q255": (255, 300, [0, 3, 100, 254]),
    "q256": (256, 300, [0, 3, 100, 255]),
    "q257": (257, 300, [0, 3, 100, 255, 256]),
    "q513": (513, 300, [0, 3, 255, 256, 300, 511, 512]),
    "hole": (513, 301, [256, 300, 511, 512]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    nq, nt, kept = CHUNK_CASES[name]
    return _pair(1000 + sorted(CHUNK_CASES).index(name), nq, nt, kept)


def _tiny_frames():
    """0: 40 query rows; 1, 2, 3: train frames of 0, 1 and 2 rows (their first row is query row 5 with a one cleared); 4: no row."""
    Q, other = _rows(77, 1, 40), _rows(77, 2, 1)[0]
    near = _cleared(Q[5], 1)
    return [Q, Q[:0], near[None], np.stack([near, other]), Q[:0]]


TINY_PAIRS = np.array([[0, 1], [0, 2], [0, 3], [4, 3], [3, 0], [1, 0], [2, 0], [4, 1], [3, 4]], np.int32)


# ---- one interface over the kinds ------------------------------------------------------------------------------------------------
def _as(kind, bits):
    return np.packbits(bits, axis=1).reshape(len(bits), NBITS // 8) if FAMILY[kind] == "ham" else bits.astype(np.float32)


def _upload(ctx, kind, frames):
    ctx.clear_descriptors()
    up = {"int8": ctx.upload_descriptors, "f32": ctx.upload_descriptors_f32, "dot": ctx.upload_descriptors_f32,
          "bits": ctx.upload_descriptors_bits, "wide": ctx.upload_descriptors_bits_wide}[kind]
    for f, d in enumerate(frames):
        up(f, d)


def _l2_directed(ctx, pairs):
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    cap = int(sum(ctx.frame_rows(int(p[0])) for p in pairs))
    counts, offsets = np.zeros(len(pairs), np.int32), np.zeros(len(pairs) + 1, np.int64)
    q, t = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
    total = C.c_int64(0)
    ctx._check(ctx._L.eacham_match_pairs_directed(ctx.handle, pairs.ctypes.data, len(pairs), RATIO, counts.ctypes.data, offsets.ctypes.data,
                                                  q.ctypes.data, t.ctypes.data, cap, C.byref(total)))
    return counts, offsets, q[:total.value].copy(), t[:total.value].copy()


def _got(ctx, kind, pairs, mode, min_dir=0, min_mutual=-1, stats=True, thresh=None):
    """(counts, offsets, q, t, values or None, stats or None) of the resident frames."""
    fam = FAMILY[kind]
    thresh = (MIN_SCORE if fam == "dot" else RATIO) if thresh is None else thresh
    if mode == 1:
        if fam == "l2":
            return (*_l2_directed(ctx, pairs), None, None)
        r = ctx.match_pairs_directed_dot(pairs, thresh) if fam == "dot" else ctx.match_pairs_directed_hamming(pairs, thresh)
        return (*r, None)
    if fam == "l2":
        c, o, q, t, st = ctx.match_all_pairs(pairs, thresh, min_dir, min_mutual, stats=stats)
        return c, o, q, t, None, st
    call = ctx.match_all_pairs_dot if fam == "dot" else ctx.match_all_pairs_hamming
    return call(pairs, thresh, min_dir, min_mutual, stats=stats)


def _csr(per_pair):
    """(counts, offsets, q, t) of np_reference's per-pair (q, t, ...) results."""
    counts = np.array([len(r[0]) for r in per_pair], np.int32)
    offsets = np.zeros(len(per_pair) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return counts, offsets, *(np.concatenate([r[k] for r in per_pair]).astype(np.uint32) for k in (0, 1))


def _want(fam, frames, pairs, mode, min_dir=0, min_mutual=-1, thresh=None):
    """The same tuple from the family's reference; stats always (the caller drops them where the call did not ask)."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    thresh = (MIN_SCORE if fam == "dot" else RATIO) if thresh is None else thresh
    if fam == "l2":
        fl = [f.astype(np.float32) for f in frames]
        if mode == 1:
            return (*_csr([NR.directed(fl[a], fl[b], thresh) for a, b in pairs]), None, None)
        res = [NR.mutual(fl[a], fl[b], thresh, min_dir, min_mutual) for a, b in pairs]
        return (*_csr(res), None, np.array([r[2] for r in res], np.int32).reshape(-1, 4))
    if fam == "dot":
        fl = [f.astype(np.float32) for f in frames]
        return (*DR.match_pairs_directed(fl, pairs, thresh), None) if mode == 1 else DR.match_all_pairs(fl, pairs, thresh, min_dir, min_mutual)
    packed = [np.packbits(f, axis=1).reshape(len(f), NBITS // 8) for f in frames]
    return (*HR.match_pairs_directed(packed, pairs, thresh), None) if mode == 1 else HR.match_all_pairs(packed, pairs, thresh, min_dir, min_mutual)


NAMES = ("counts", "offsets", "q", "t", "values", "stats")


def _same(got, want, what, stats=True):
    for name, g, w in zip(NAMES, got, want):
        if name == "stats" and not stats:
            assert g is None
            continue
        if w is None:
            assert g is None, f"{what}: {name}"
            continue
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: {name} differ"


@functools.lru_cache(maxsize=None)
def _chunk_reference(fam, name, mode):
    Q, T = _case(name)
    want = _want(fam, [Q, T], [[0, 1]], mode)
    kept = CHUNK_CASES[name][2]
    assert want[2].tolist() == kept, (fam, name, want[2].tolist())          # the case keeps the rows it was built to keep
    if mode == 0:
        assert want[5][0].tolist() == [len(kept), len(kept) + 1, len(kept), 1]
    return want


# ---- chunk boundaries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CHUNK_CASES))
def test_chunk_boundaries(hip_ctx, kind, name):
    ctx = hip_ctx
    Q, T = _case(name)
    _upload(ctx, kind, [_as(kind, Q), _as(kind, T)])
    fam = FAMILY[kind]
    _same(_got(ctx, kind, [[0, 1]], 1), _chunk_reference(fam, name, 1), f"{kind} {name} directed")
    want = _chunk_reference(fam, name, 0)
    _same(_got(ctx, kind, [[0, 1]], 0), want, f"{kind} {name} mutual with stats")
    _same(_got(ctx, kind, [[0, 1]], 0, stats=False), want, f"{kind} {name} mutual without stats", stats=False)


# ---- the edge rule: n12 >= min_dir && n21 >= min_dir && mutual > min_mutual ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_reference(fam, min_dir, min_mutual):
    Q, T = _case("q257")
    return _want(fam, [Q, T], [[0, 1], [1, 0]], 0, min_dir, min_mutual)


@pytest.mark.parametrize("kind", KINDS)
def test_threshold_edges(hip_ctx, kind):
    """Pair (0, 1) has |m12| = 5, |m21| = 6, |mutual| = 5; pair (1, 0) the two directions exchanged."""
    ctx = hip_ctx
    Q, T = _case("q257")
    _upload(ctx, kind, [_as(kind, Q), _as(kind, T)])
    fam, pairs, M = FAMILY[kind], [[0, 1], [1, 0]], len(CHUNK_CASES["q257"][2])
    # (min_dir, min_mutual) -> is the pair (0, 1) an edge: strict '>' on the mutual count, '>=' on the direction counts
    for (min_dir, min_mutual), edge in (((0, M), False), ((0, M - 1), True), ((M, 0), True), ((M + 1, 0), False), ((M + 2, 0), False)):
        want = _edge_reference(fam, min_dir, min_mutual)
        assert want[5][:, 3].tolist() == [int(edge)] * 2 and want[0].tolist() == [M * edge] * 2, (min_dir, min_mutual)
        for stats in (True, False):
            _same(_got(ctx, kind, pairs, 0, min_dir, min_mutual, stats=stats), want, f"{kind} {min_dir}/{min_mutual} stats {stats}", stats=stats)
    _same(_got(ctx, kind, pairs, 1), _want(fam, [Q, T], pairs, 1), f"{kind} directed")


# ---- empty and tiny frames ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_reference(fam, mode):
    return _want(fam, _tiny_frames(), TINY_PAIRS, mode)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_and_tiny_frames(hip_ctx, kind):
    ctx = hip_ctx
    _upload(ctx, kind, [_as(kind, f) for f in _tiny_frames()])
    fam = FAMILY[kind]
    for stats in (True, False):
        _same(_got(ctx, kind, TINY_PAIRS, 0, stats=stats), _tiny_reference(fam, 0), f"{kind} tiny mutual stats {stats}", stats=stats)
    _same(_got(ctx, kind, TINY_PAIRS, 1), _tiny_reference(fam, 1), f"{kind} tiny directed")
    counts = _tiny_reference(fam, 1)[0]
    assert not counts[[0, 3, 5, 7, 8]].any() and counts[2] >= 1 and counts[4] >= 1 and counts[6] >= 1   # no row on either side: nothing
    assert counts[1] == (1 if fam == "dot" else 0)   # one train row: no second neighbour (the dot product needs none)


# ---- above 48 KiB of dynamic LDS: frames of 6200 rows, row stride > 6144 ----------------------------------------------------------------
BIG = 6200


@functools.lru_cache(maxsize=None)
def _big_l2():
    """16-D integer rows: 1500 rows of the first frame are noisy copies of rows of the second."""
    B = synth.random_u8_descriptors(BIG, 16, 31, 1)
    A = synth.random_u8_descriptors(BIG, 16, 31, 2)
    who = synth.rng_permutation(31, 3, BIG)[:1500]
    A[synth.rng_permutation(31, 4, BIG)[:1500]] = np.clip(B[who] + np.rint(2 * synth.rng_normal(31, 5, (1500, 16))), 0, 255)
    return [np.ascontiguousarray(A, np.float32), B]


@functools.lru_cache(maxsize=None)
def _big_l2_reference(min_dir, min_mutual):
    A, B = _big_l2()
    want = NR.mutual(A, B, RATIO, min_dir, min_mutual)
    assert want[2][2] > 1000 and want[2][3] == 1
    return (*_csr([want]), None, want[2].reshape(1, 4))


@pytest.mark.parametrize("kind,stats", [("int8", True), ("int8", False), ("f32", True)])
def test_large_lds_l2(hip_ctx, kind, stats):
    """int8 with stats: match_finalize_kernel; without, at the default thresholds: match_finalize2_kernel; f32: match_finalize_f32_kernel."""
    ctx = hip_ctx
    _upload(ctx, kind, _big_l2())
    _same(_got(ctx, kind, [[0, 1]], 0, 30, 30, stats=stats), _big_l2_reference(30, 30), f"{kind} 6200 rows stats {stats}", stats=stats)


def test_large_lds_dot(hip_ctx):
    ctx = hip_ctx
    frames = _big_l2()
    _, best = DR.argmax(frames[0], frames[1])
    min_score = float(np.floor(np.median(best))) + 0.5    # integer scores: about half of the rows pass
    want = DR.match_all_pairs(frames, [[0, 1]], min_score, 30, 30)
    assert want[5][0, 2] > 30 and want[5][0, 3] == 1
    _upload(ctx, "dot", frames)
    _same(_got(ctx, "dot", [[0, 1]], 0, 30, 30, thresh=min_score), want, "dot 6200 rows")


@pytest.mark.parametrize("kind,nbytes", [("wide", 40), ("bits", 4)])
def test_large_lds_hamming(hip_ctx, kind, nbytes):
    """The distance matrix comes from a float matrix product on the unpacked bits (exact: at most 320), held to ham_reference's own
    popcount on a band of rows; top-2, predicate, mutual check and edge rule are ham_reference's."""
    frames = HC.binary_frames(nbytes, [BIG, BIG], 1500, 47, inject=False)
    a, b = (np.unpackbits(f, axis=1).astype(np.float32) for f in frames)
    D = (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)
    assert np.array_equal(D[3000:3064], HR.distances(frames[0][3000:3064], frames[1]))
    ref = HR.Scene(frames)
    ref._D[(0, 1)] = D
    want = ref.match_all_pairs([[0, 1]], RATIO, 30, 30)
    assert want[5][0, 3] == 1 and want[5][0, 2] > 30
    ctx = hip_ctx
    _upload(ctx, kind, frames)
    _same(ctx.match_all_pairs_hamming([[0, 1]], RATIO, 30, 30), want, f"{kind} 6200 rows x {nbytes} bytes")
    _same(ctx.match_all_pairs_hamming([[0, 1]], RATIO, 30, 30, stats=False), want, f"{kind} 6200 rows, without stats", stats=False)
