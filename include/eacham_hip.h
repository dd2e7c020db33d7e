/*
 * eacham_hip.h — C-ABI of the MI355X (gfx950) matching + bundle-adjustment hot path.
 *
 * This is the drop-in boundary for the two hot spots of fatlipp/eacham:
 *
 *   matching : FeatureMatcherFlann::Match        modules/base/features/FeatureMatcherFlann.cpp:14-30
 *              IFeatureMatcher<T>::Match         modules/base/features/IFeatureMatcher.h:8-20
 *              pair loop + mutual cross-check    apps/sfm/main.cpp:84-147
 *   BA       : RefineBA                          modules/sfm/reconstruction/BundleAdjuster.h:13-17
 *                                                modules/sfm/reconstruction/BundleAdjuster.cpp:40-250
 *              OptimizerConfig                   modules/sfm/config/SfmConfig.h:15-22
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions across the ABI.
 *   - every call returns EACHAM_OK (0) or a negative error code; eacham_last_error(ctx)
 *     returns the message of the last failure on that context.
 *   - one context = one HIP device + one HIP stream; calls on one context are serialised by an
 *     internal mutex, so the reference's pattern of calling Match() concurrently on one shared
 *     matcher instance (apps/sfm/main.cpp:98-109) stays legal. Distinct contexts are independent.
 *   - pointers named *_dev are device pointers valid on the context's device; everything else is
 *     host memory. *_dev entry points enqueue on the context stream and do not synchronise;
 *     use eacham_ctx_sync().
 *   - match lists are emitted SORTED BY QUERY INDEX: the reference returns an unordered_map whose
 *     iteration order is unspecified; sorted is the canonical form used for bit-exact parity.
 */
#ifndef EACHAM_HIP_H
#define EACHAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EACHAM_OK 0
#define EACHAM_ERR_INVALID (-1)      /* bad argument */
#define EACHAM_ERR_HIP (-2)          /* a HIP runtime call failed */
#define EACHAM_ERR_CAPACITY (-3)     /* caller-provided output buffer too small */
#define EACHAM_ERR_UNSUPPORTED (-4)  /* e.g. descriptor dimension not supported by the kernel */
#define EACHAM_ERR_NOT_INTEGER (-5)  /* descriptors are not integer-valued in [0,255] (exact i8 path) */
#define EACHAM_ERR_NO_DEVICE (-6)    /* no HIP device / extension unusable: the product path never falls back to CPU */

typedef struct eacham_ctx eacham_ctx;

/* ---- context ------------------------------------------------------------------------------ */

/* Creates a context on HIP device `device_id`. Fails (no CPU fallback) if no device exists. */
int eacham_ctx_create(int device_id, eacham_ctx** out_ctx);
void eacham_ctx_destroy(eacham_ctx* ctx);
const char* eacham_last_error(const eacham_ctx* ctx);
/* Blocks until everything enqueued on the context stream has finished. */
int eacham_ctx_sync(eacham_ctx* ctx);
/* Diagnostic: what the search for a second stream on a hardware queue of its own decided at eacham_ctx_create (the work behind a
 * batch's distance sweep runs on it beside the next sweep). *attempt = which candidate was kept (0..3 probed, 4 = the last one,
 * kept unprobed; -1 = no search: EACHAM_STREAM2_PRIORITY), *lead_ms = how long before the end of a 40 us spin on the first stream
 * the empty kernel on it finished (above 0.010: the two do not share a queue; -1 = not measured). */
int eacham_ctx_stream2_info(const eacham_ctx* ctx, int* attempt, float* lead_ms);
/* Returns the hipStream_t of the context (as void*), so callers can order their own work. */
void* eacham_ctx_stream(eacham_ctx* ctx);
/* Library / build identification ("eacham_hip <version> gfx950"). */
const char* eacham_version(void);

/* ---- descriptor store (input of Match: Node::GetDescriptors(), modules/sfm/data/Node.h:136-139) */

/* Uploads the N x dim row-major fp32 descriptor matrix of frame `frame_id` (the layout of the
 * cv::Mat returned by FeatureExtractorSift::Extract, modules/base/features/FeatureExtractorSift.cpp:14-26)
 * and keeps it resident on the device in the kernel's fragment-major int8 layout.
 * Values must be integers in [0,255] (OpenCV SIFT descriptors are) —
 * otherwise EACHAM_ERR_NOT_INTEGER. dim must be a multiple of 16 up to 128, or any
 * dimension from 129 to 256 (rows are padded with centred zeros to 256). n may be 0.
 * Re-uploading a frame id replaces it. */
int eacham_upload_descriptors(eacham_ctx* ctx, int frame_id, const float* rowmajor, int n, int dim);
/* Same, source already on the device (enqueued on the context stream; the integrality check is
 * reported by the next synchronising call). */
int eacham_upload_descriptors_dev(eacham_ctx* ctx, int frame_id, const float* rowmajor_dev, int n, int dim);
/* Float descriptors (SuperPoint / LightGlue style, modules/onnx/lightglue/feature/Types.h:11-14: 256-D
 * fp32, any values): kept resident as fp32 MFMA fragments and matched with
 *   d2 = max(fma(-2, a.b, |a|^2 + |b|^2), 0)   (fp32, a.b and the norms as k-ordered fma chains)
 * on the f32 matrix cores. Same Match / mutual-check semantics, ties -> lower index. All resident
 * frames must be of one kind (int8 via eacham_upload_descriptors, or fp32 via this call). dim <= 256. */
int eacham_upload_descriptors_f32(eacham_ctx* ctx, int frame_id, const float* rowmajor, int n, int dim);
/* Number of rows of a resident frame, or a negative error code. */
int eacham_frame_rows(eacham_ctx* ctx, int frame_id);
/* Drops all resident frames. */
int eacham_clear_descriptors(eacham_ctx* ctx);

/* ---- directed match: FeatureMatcherFlann::Match (FeatureMatcherFlann.cpp:14-30) -------------
 * For each row q of frame f1: the two nearest rows of frame f2 under L2 (exact; ties -> lower
 * train index first); keep q -> t0 iff (float)(d0 / d1) < ratio with d = sqrtf(squared L2), the
 * quotient promoted to double as in the reference (ratio = 0.8 there, FeatureMatcherFlann.cpp:23).
 * Output sorted by q. If frame f2 has fewer than 2 rows the result is empty (the reference would
 * read m[1] out of bounds). */
int eacham_match_pair(eacham_ctx* ctx, int f1, int f2, double ratio,
                      uint32_t* out_q, uint32_t* out_t, int cap, int* out_count);

/* Batched form: npairs ORDERED pairs {f1, f2}, each one FeatureMatcherFlann::Match(d[f1], d[f2]) call, in one
 * launch sequence — what the reference's std::for_each(par_unseq) + std::async issues concurrently on its shared
 * matcher (apps/sfm/main.cpp:98-109); the C++ adapter funnels concurrent Match() callers into this entry point.
 * No thresholds, no mutual check. Result in CSR form over the pairs: counts[p], offsets (npairs + 1), and for
 * k in [offsets[p], offsets[p+1]) the match q[k] -> t[k] of pair p, sorted by q. cap = capacity of out_q / out_t
 * (sum of the query frames' rows always suffices); *out_total = matches found (EACHAM_ERR_CAPACITY if > cap). */
int eacham_match_pairs_directed(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio,
                                int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t, int64_t cap,
                                int64_t* out_total);

/* ---- all-pairs match + mutual check: apps/sfm/main.cpp:84-147 -------------------------------
 * pairs = npairs x {f1, f2} (unordered pairs; both directions are evaluated from one distance
 * tile). For each pair: directed matches m12, m21 as above; if |m12| < min_dir or |m21| < min_dir
 * the pair is dropped (main.cpp:111, literal 30); mutual = {(q,t) in m12 : m21[t] == q}
 * (main.cpp:133-140); the pair becomes an edge iff |mutual| > min_mutual (main.cpp:142, literal 30).
 *
 * Result (CSR over pairs): counts[p] = |mutual| for edges, 0 otherwise; offsets[p] = prefix sum
 * (npairs+1 entries); (q[k], t[k]) for k in [offsets[p], offsets[p+1]) sorted by q, q indexing
 * frame pairs[2p], t indexing frame pairs[2p+1]  (= Graph::Connect(n1,n2,best12); the reverse
 * edge Connect(n2,n1,best21) is its inverse, main.cpp:144-145).
 * stats (optional, may be NULL): npairs x {|m12|, |m21|, |mutual|, edge?1:0}.
 * ratio must be in (0, 1] here (the reference uses 0.8): the mutual check identifies m21[t] == q by
 * "column t passes the ratio test and its minimum is d(q,t)", which relies on a passing column having
 * a unique minimum; EACHAM_ERR_INVALID otherwise. eacham_match_pair accepts any ratio. */
int eacham_match_all_pairs(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio,
                           int min_dir, int min_mutual,
                           int32_t* counts, int64_t* offsets,
                           uint32_t* out_q, uint32_t* out_t, int64_t cap, int64_t* out_total,
                           int32_t* stats);

/* Device-resident, asynchronous form used by the benchmark and the multi-GPU shard driver.
 * pairs_dev: npairs x 2 int32. counts_dev: npairs int32. offsets_dev: npairs+1 int64.
 * edges_dev: edge_cap x {uint32 q, uint32 t}; entries beyond edge_cap are dropped and
 * *total_dev (int64, device) still holds the uncapped total. stats_dev: npairs x 4 int32 or NULL.  * A pair naming a frame that is not resident yields no match (count 0) and raises a sticky error that
 * the next eacham_ctx_sync returns as EACHAM_ERR_INVALID; it never reaches the kernels. */
int eacham_match_all_pairs_dev(eacham_ctx* ctx, const int32_t* pairs_dev, int npairs, double ratio,
                               int min_dir, int min_mutual,
                               int32_t* counts_dev, int64_t* offsets_dev,
                               uint32_t* edges_dev, int64_t edge_cap, int64_t* total_dev,
                               int32_t* stats_dev);

/* Debug getter (tests, bench.py's parity gate): how a job of `npairs` pairs of the frames resident NOW would be cut into
 * launches by eacham_match_all_pairs[_dev] (with_stats = 1: the full-column form that the `stats` argument selects). starts[b] =
 * index of the first pair of launch b (the first `cap` of them are written), *n_batches = launches, *n_slots = workspace copies
 * they rotate through (2: the work behind launch b runs on a second stream beside launch b + 1). Lets a parity test place its
 * oracle samples on both sides of every launch boundary of the job of apps/sfm/main.cpp:84-147. */
int eacham_match_debug_batches(eacham_ctx* ctx, int npairs, int with_stats, int32_t* starts, int cap, int* n_batches, int* n_slots);

/* Debug getter (tests), beside eacham_match_debug_batches: the numbers that cut is made from. *batch = the most pairs a launch may
 * hold (the workspace budget), *round_pairs = the unit launches are sized in (pairs of one round of workgroups; 1 where the budget
 * holds less than a round), *tail_pairs = the most pairs the short last launch of a job through two slots holds. */
int eacham_match_debug_plan(eacham_ctx* ctx, int npairs, int with_stats, int* batch, int* round_pairs, int* tail_pairs);

/* Debug getter (tests, A/B runs): the candidate columns of the LAST eacham_match_all_pairs[_dev] call on this context (lean form,
 * int8 frames) that were settled from the row sweep's minima without computing a distance (*settled) and that went through the
 * column pass (*verified); live pairs only. EACHAM_MATCH_COLPRUNE=0 at eacham_ctx_create sends every candidate down the column
 * pass (*settled = 0). Waits for the context's stream. */
int eacham_match_debug_colprune(eacham_ctx* ctx, int64_t* settled, int64_t* verified);

/* Debug getter (tests, A/B runs): the screen sweeps of the LAST matching call on this context (lean form, int8 frames above 128-D,
 * EACHAM_MATCH_SWEEP_FORM unset or =screen): *rows = real query rows they met, *open = rows their bound could not fail and that
 * went to the exact pass. Both 0 when the call ran another form. Waits for the context's stream. */
int eacham_match_debug_screen(eacham_ctx* ctx, int64_t* rows, int64_t* open);

/* Debug getter (tests, A/B runs), beside eacham_match_debug_screen: *items = work items of the exact pass over those open rows in the
 * LAST matching call, summed over its launches. An item holds up to 256 open rows of consecutive pairs of one launch that share their
 * train frame. 0 when the call ran another form. Waits for the context's stream. */
int eacham_match_debug_screen_items(eacham_ctx* ctx, int64_t* items);

/* Debug entry (tests): the screen sweep alone on the ordered pair (f1, f2), before any exact pass. Per row q of f1 (cap >= its rows):
 * n1[q] = the smallest |M_q - M_t|^2 over the rows t of f2 on the FP6 grid (~0 without a real row), l1[q] <= the row's true
 * smallest squared distance, u2[q] >= its true second smallest (-1 where the sweep wrote a padding value: no row, or the minima
 * of one subset only). EACHAM_ERR_UNSUPPORTED unless the resident frames are int8 above 128-D. */
int eacham_match_debug_screen_pair(eacham_ctx* ctx, int f1, int f2, uint32_t* n1, int32_t* l1, int32_t* u2, int cap);

/* ---- dot-product similarity for float descriptors, scores returned ----------------------------
 * The brute-force rule for SuperPoint-class descriptors (modules/onnx/lightglue/feature/Types.h:11-14): nearest neighbour
 * by similarity with a score threshold, where the reference's LightGlue plug-in keeps a match by `mscores0 > 0.5`
 * (FeatureMatcherLightglue.cpp:118) and hands the score on. For frames uploaded with eacham_upload_descriptors_f32
 * (any dim 1..256); int8 frames give EACHAM_ERR_UNSUPPORTED, a frame that is not resident EACHAM_ERR_INVALID.
 *   s(q,t) = a_q . b_t   in fp32, accumulated as the k-ordered fmaf chain from 0 (what the f32 matrix cores produce).
 *   Nothing is normalised: the caller's values are used as they are.
 * Directed match f1 -> f2: for each row q, t0 = argmax_t s(q,t), the lower train index on equal similarity; q -> t0 is
 * kept iff s(q,t0) > min_score (strict). No second neighbour is involved: a train frame of one row is legal, a train
 * frame of 0 rows gives an empty result. A NaN similarity never compares greater: it never wins and never passes.
 * Every emitted match k carries out_score[k] = s(q[k], t[k]), bit for bit that chain; out_score may be NULL.
 * Output sorted by q; *out_count = matches found (EACHAM_ERR_CAPACITY if > cap).
 * There is no device-pointer form and no sharded form of these calls (the float kind has neither for L2). */
int eacham_match_pair_dot(eacham_ctx* ctx, int f1, int f2, float min_score,
                          uint32_t* out_q, uint32_t* out_t, float* out_score, int cap, int* out_count);

/* npairs ORDERED pairs, each one directed dot-product match, in one launch sequence; CSR over the pairs like
 * eacham_match_pairs_directed, plus the scores. */
int eacham_match_pairs_directed_dot(eacham_ctx* ctx, const int32_t* pairs, int npairs, float min_score,
                                    int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t,
                                    float* out_score, int64_t cap, int64_t* out_total);

/* The mutual form, same shape as eacham_match_all_pairs: m12, m21 as above; the pair is dropped if |m12| < min_dir or
 * |m21| < min_dir; mutual = {(q,t) in m12 : m21[t] == q}; the pair is an edge iff |mutual| > min_mutual. counts[p] =
 * |mutual| for edges, 0 otherwise; CSR over the pairs sorted by q; out_score[k] = s(q[k], t[k]);
 * stats (may be NULL): npairs x {|m12|, |m21|, |mutual|, edge?1:0}. min_dir = 0 and min_mutual = -1 keep every pair's
 * one-to-one matches. */
int eacham_match_all_pairs_dot(eacham_ctx* ctx, const int32_t* pairs, int npairs, float min_score,
                               int min_dir, int min_mutual,
                               int32_t* counts, int64_t* offsets,
                               uint32_t* out_q, uint32_t* out_t, float* out_score, int64_t cap, int64_t* out_total,
                               int32_t* stats);

/* The screened form of eacham_match_all_pairs_dot: the same arguments, and outputs that are identical to that
 * call's byte for byte — counts, offsets, q, t, the bits of every score, stats — with the same error codes for the same bad
 * inputs. An fp16 sweep on the matrix cores decides every row and column that a proven bound on |fp16 value - fp32 value| lets
 * it decide (dead: cannot pass min_score; settled: the arg-max is certain); the exact fp32 chain is then evaluated for the
 * winners, and against the whole other frame for the rows and columns left open. A pair with a frame that holds a value that
 * is not finite or beyond the fp16 range (|x| > 65504) runs the fp32 kernel of the unscreened call. A frame's fp16 image is
 * built on its first screened call and dropped on re-upload and eacham_clear_descriptors; callers of the unscreened entry
 * points pay nothing for it. Opt-in: whether it is faster depends on how many rows the bound leaves open.
 * Out of scope: the directed calls and eacham_match_pair_dot have no screened form. */
int eacham_match_all_pairs_dot_screened(eacham_ctx* ctx, const int32_t* pairs, int npairs, float min_score,
                                        int min_dir, int min_mutual,
                                        int32_t* counts, int64_t* offsets,
                                        uint32_t* out_q, uint32_t* out_t, float* out_score, int64_t cap, int64_t* out_total,
                                        int32_t* stats);

/* Debug getter (tests, rate tools): the LAST eacham_match_all_pairs_dot_screened call on this context. out[0..2] = rows dead /
 * settled / open, out[3..5] = columns dead / settled / open (screened pairs only, real rows and columns), out[6] = pairs that
 * fell back to the fp32 kernels. Waits for the context's stream. */
int eacham_match_debug_dot_screen(eacham_ctx* ctx, int64_t out[7]);

/* Test hook: the fp16 sweep's raw similarities of the pair (f1, f2), s_coarse[q * n2 + t] (n1 x n2 floats), and the bounds the
 * screen classifies with: row_E[q] (n1) and col_E[t] (n2), |s_coarse - s| <= min(row_E[q], col_E[t]). Small frames only:
 * EACHAM_ERR_CAPACITY above 4096 x 4096; EACHAM_ERR_UNSUPPORTED for int8 frames and for a pair that is not screened.
 * These are restatements, not the matcher's own memory: s_coarse comes from an instantiation of the tile kernel that also stores
 * every accumulator (the same MFMA sequence per tile, another code object), row_E and col_E are recomputed on the host from the
 * stored norm bounds with the formula and rounding steps of the classify kernel. */
int eacham_match_debug_dot_coarse(eacham_ctx* ctx, int f1, int f2, float* s_coarse, float* row_E, float* col_E);

/* ---- binary descriptors under Hamming distance, distances returned -----------------------------
 * ORB / BRIEF / AKAZE rows (the reference's TUM, KITTI and Realsense configurations name ORB; its 256-bit popcount distance is
 * modules/base/tools/Tools3d.h:47-63), matched as cv::BFMatcher(NORM_HAMMING) + the ratio test of FeatureMatcherFlann.cpp:23
 * would: distance = the number of differing bits, an integer stored as float, and q -> t0 is kept iff
 *   (double)((float)h0 / (float)h1) < ratio        (no square root: 5 h0 = 4 h1 fails at 0.8; 0/0 fails; 0/h1 passes)
 * Everything else — two nearest rows, ties -> the lower train index, output sorted by q, fewer than 2 train rows -> empty,
 * thresholds, mutual check, ratio in (0, 1] for the mutual form, CSR layout, error codes, capacity — is word for word
 * eacham_match_pair / eacham_match_pairs_directed / eacham_match_all_pairs[_dev]. The CSR output is what eacham_graph_* and
 * eacham_tracks_build take.
 * out_dist[k] (int32, may be NULL) = the Hamming distance of emitted match k, computed from the packed rows themselves.
 *
 * Upload: n rows of bytes_per_row bytes, packed (bit order is irrelevant to the distance), bytes_per_row in 1..32; above 32
 * (more than 256 bits) EACHAM_ERR_UNSUPPORTED. Rows are padded with zero bits to the next dimension eacham_upload_descriptors
 * accepts. The host-to-device copy is the packed bytes. Binary frames are a third kind: mixing them with int8 or fp32 frames in
 * one context is EACHAM_ERR_UNSUPPORTED at upload (eacham_clear_descriptors resets the kind), the L2 and dot-product entry
 * points return EACHAM_ERR_UNSUPPORTED on binary frames and the calls below return it on other frames.
 * Limits: <= 256 bits, <= 16384 rows per frame. There is no sharded form. */
int eacham_upload_descriptors_bits(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor, int n, int bytes_per_row);
/* Same, source already on the device. */
int eacham_upload_descriptors_bits_dev(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor_dev, int n, int bytes_per_row);
int eacham_match_pair_hamming(eacham_ctx* ctx, int f1, int f2, double ratio,
                              uint32_t* out_q, uint32_t* out_t, int32_t* out_dist, int cap, int* out_count);
int eacham_match_pairs_directed_hamming(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio,
                                        int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t,
                                        int32_t* out_dist, int64_t cap, int64_t* out_total);
int eacham_match_all_pairs_hamming(eacham_ctx* ctx, const int32_t* pairs, int npairs, double ratio,
                                   int min_dir, int min_mutual,
                                   int32_t* counts, int64_t* offsets,
                                   uint32_t* out_q, uint32_t* out_t, int32_t* out_dist, int64_t cap, int64_t* out_total,
                                   int32_t* stats);
/* As eacham_match_all_pairs_dev; dist_dev: edge_cap int32 (one per entry of edges_dev that is written) or NULL. */
int eacham_match_all_pairs_hamming_dev(eacham_ctx* ctx, const int32_t* pairs_dev, int npairs, double ratio,
                                       int min_dir, int min_mutual,
                                       int32_t* counts_dev, int64_t* offsets_dev,
                                       uint32_t* edges_dev, int64_t edge_cap, int64_t* total_dev,
                                       int32_t* stats_dev, int32_t* dist_dev);

/* ---- wide binary descriptors: up to 512 bits (BRISK, FREAK: 64 bytes; AKAZE's default MLDB: 61 bytes) ------------
 * A fourth kind of resident frame (kind 3), matched by the four eacham_match_*_hamming calls above with exactly their
 * results: the same two nearest rows, ties, predicate, sorting, mutual check, thresholds, stats and int32 distances. Behind
 * them runs a sweep of its own on the FP4 matrix cores (csrc/matcher_ham_wide.hip): a bit is the E2M1 number +-1, every sum an
 * integer below 2^24, so the sweep is exact with no screen and no second pass.
 *
 * Upload: n rows (0..16384) of bytes_per_row bytes (1..64), the most significant bit of a byte first (np.unpackbits' order;
 * the distance does not depend on it). EACHAM_ERR_UNSUPPORTED: more than 64 bytes; more than 16384 rows; a context that holds
 * frames of another kind (eacham_clear_descriptors resets the kind); a bytes_per_row other than that of the resident wide
 * frames. EACHAM_ERR_INVALID: a bad shape or a null pointer. The host-to-device copy is the packed bytes. Rows of 32 bytes
 * or fewer may be uploaded either way, eacham_upload_descriptors_bits or this; the results are the same bytes.
 * The L2 and dot-product entry points return EACHAM_ERR_UNSUPPORTED on wide frames. There is no sharded form. */
int eacham_upload_descriptors_bits_wide(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor, int n, int bytes_per_row);
/* Same, source already on the device. */
int eacham_upload_descriptors_bits_wide_dev(eacham_ctx* ctx, int frame_id, const uint8_t* rowmajor_dev, int n, int bytes_per_row);
/* Test hook: the sweep's own top-2 of the ordered pair (f1, f2), per row of f1 in the caller's order, read from the buffer the
 * tail reads: best[q] = the nearest train row (the lower index on a tie), h0[q] its distance, h1[q] the runner-up's. cap >= rows
 * of f1 (EACHAM_ERR_CAPACITY); f2 needs two rows or more (EACHAM_ERR_INVALID). */
int eacham_match_debug_hamming_wide_pair(eacham_ctx* ctx, int f1, int f2, int32_t* best, int32_t* h0, int32_t* h1, int cap);
/* out = {batches, pairs per batch, sweep launches, query rows swept} of the last matching call on wide frames. */
int eacham_match_debug_hamming_wide(eacham_ctx* ctx, int64_t out[4]);

/* ---- bundle adjustment: RefineBA (modules/sfm/reconstruction/BundleAdjuster.cpp:40-250) --------
 *
 * The caller (the C++ adapter in include/eacham/BundleAdjusterHip.hpp) performs the reference's
 * graph walk (window selection :123-162, landmark filter `status && observers >= 2` :84) and
 * hands over plain arrays; the library restates everything from the factor graph on: factors and
 * noise models (:57-121, :171-178), Levenberg-Marquardt with GTSAM's Ceres defaults (:182-216),
 * error evaluation (:218-219). Write-back (:221-249) is the inverse mapping done by the adapter.
 *
 * Variable blocks: camera i -> Pose3 camera->world (the inverse of cam_T_wc, :65), tangent
 * [omega, v]; landmark j -> Point3; one shared Cal3_S2 (fx, fy, s = 0, u0, v0) (:47-49).
 * All arithmetic is fp64.
 */
typedef struct eacham_ba_problem {
    int32_t n_cams;
    int32_t n_points;
    int32_t n_obs;
    int32_t ordering;                /* EACHAM_BA_ORDER_* below: elimination order of the reduced camera system;  */
                                     /* 0 (a zero-initialised problem) = chosen by the library's cost model       */
    const double* cam_T_wc;          /* n_cams x 16, row-major world->camera (Node::GetTransform())   */
    const int32_t* cam_fixed;        /* n_cams, Graph::IsFixed(id) (:69)                              */
    const double* points;            /* n_points x 3 (Map::Get(id3d), :102)                          */
    const int32_t* point_observers;  /* n_points, Map::GetObservers(id3d).size(): the GLOBAL count,  */
                                     /* also inside a local window (:109) -> prior sigma 1/obs       */
    const uint32_t* obs_cam;         /* n_obs, index into cams                                       */
    const uint32_t* obs_point;       /* n_obs, index into points                                     */
    const double* obs_uv;            /* n_obs x 2, keypoint in pixels (cv::Point2f widened, :93)     */
    double K[4];                     /* fx, fy, cx, cy = K(0,0), K(1,1), K(0,2), K(1,2) (:47-49)     */
} eacham_ba_problem;

/* Elimination order of the reduced camera system (the counterpart of GTSAM's COLAMD ordering, which the reference
 * gets through LevenbergMarquardtParams::SetCeresDefaults, BundleAdjuster.cpp:182-190). Every choice solves the same
 * system; they differ in the height of the elimination tree (the number of dependent launches) and in fill.
 * AUTO evaluates the candidates with a cost model and keeps the cheapest (eacham_amd/csrc/ba_plan.hpp). */
#define EACHAM_BA_ORDER_AUTO 0
#define EACHAM_BA_ORDER_NATURAL 1  /* the caller's camera order: a band for a sequence                                */
#define EACHAM_BA_ORDER_RCM 2      /* reverse Cuthill-McKee: minimal band, the tree is a path                        */
#define EACHAM_BA_ORDER_ND 3       /* nested dissection: independent subtrees are factorised in the same launch      */

#define EACHAM_BA_LM 0
#define EACHAM_BA_DOGLEG 1

/* OptimizerConfig (modules/sfm/config/SfmConfig.h:15-22), fields verbatim + the reference's literal. */
typedef struct eacham_ba_options {
    int32_t method;             /* "LM" -> EACHAM_BA_LM, "DogLeg" -> EACHAM_BA_DOGLEG               */
    int32_t max_iter;           /* maxIter                                                           */
    float max_tolerance;        /* maxTolerance: absoluteErrorTol = relativeErrorTol (:187-188)      */
    float delta;                /* DogLeg deltaInitial (:211)                                        */
    int32_t use_preconditioner; /* usePreconditioner (LM only): solve every damped system with PCG +   */
                                /* block-Jacobi at 1e-10 / 1e-10 (:192-200) instead of the direct solve */
    int32_t min_landmarks;      /* literal 50 (:166): fewer landmarks -> silently do nothing         */
    int32_t lm_factor_policy;   /* EACHAM_BA_LM_FACTOR_* below; 0 (zero-initialised options) = RESET */
    int32_t reserved;
} eacham_ba_options;

/* What LevenbergMarquardtState::decreaseLambda does to the growth factor after an ACCEPTED step
 * (GTSAM 4.1.1 gtsam/nonlinear/internal/LevenbergMarquardtState.h, not in the reference tree; the
 * reference selects it through SetCeresDefaults, BundleAdjuster.cpp:184-190: lambdaFactor = 2,
 * useFixedLambdaFactor = false). Two readings of that line exist (SURVEY.md Appendix A.4 note):
 *   RESET  : currentFactor = 2 * params.lambdaFactor  (= 4: Ceres' decrease_factor reset; the default)
 *   DOUBLE : currentFactor = 2 * currentFactor        (the factor never shrinks)
 * They give the same lambda schedule until the first rejected step that follows two accepted ones. */
#define EACHAM_BA_LM_FACTOR_RESET 0
#define EACHAM_BA_LM_FACTOR_DOUBLE 1

#define EACHAM_BA_DONE 0     /* optimised                                                            */
#define EACHAM_BA_SKIPPED 1  /* fewer than min_landmarks landmarks: inputs copied through (:166-169) */
#define EACHAM_BA_INDETERMINATE 2 /* DogLeg only: the Gauss-Newton system is not positive definite. GTSAM's
                                   * DoglegOptimizer throws IndeterminantLinearSystemException there and
                                   * RefineBA never reaches its write-back; the values returned are those of
                                   * the last completed iteration (the inputs if it was the first). */

/* One row per tryLambda() call of the LM loop (for parity tests and reporting). */
typedef struct eacham_ba_trace_row {
    double lambda;          /* lambda used for this try                                              */
    double new_error;       /* nonlinear error at the tentative values (inf if not evaluated)        */
    double lin_change;      /* oldLinearizedError - newLinearizedError                               */
    int32_t accepted;       /* 1 = step taken                                                        */
    int32_t outer;          /* outer iteration index (iterate() call)                                */
} eacham_ba_trace_row;

typedef struct eacham_ba_result {
    double* cam_T_wc;        /* out: n_cams x 16 world->camera (Node::SetTransform, :247)            */
    double* points;          /* out: n_points x 3 (Map::UpdatePoint, :239)                           */
    double K[4];             /* out: fx, fy, cx, cy (:224-227)                                       */
    double initial_error;    /* graph.error(initial)   (:218)                                        */
    double final_error;      /* graph.error(result)    (:219)                                        */
    double final_lambda;
    int32_t status;          /* EACHAM_BA_DONE / EACHAM_BA_SKIPPED                                   */
    int32_t outer_iterations; /* successful LM iterations (NonlinearOptimizer::iterations())         */
    int32_t inner_iterations; /* tryLambda() calls = linear solves                                   */
    int32_t trace_cap;       /* in: capacity of `trace` (may be 0)                                   */
    int32_t trace_len;       /* out: rows written                                                    */
    int32_t reserved;        /* out: PCG iterations in total when use_preconditioner is set, else 0   */
    eacham_ba_trace_row* trace; /* optional                                                          */
} eacham_ba_result;

/* Runs RefineBA's optimisation on the device. Host pointers in, host pointers out; all state stays
 * resident on the device during the LM loop, only scalars (errors, lambda decisions) cross PCIe
 * per inner iteration. Returns EACHAM_OK also when the problem is skipped (see result->status).
 * Method DogLeg (BundleAdjuster.cpp:204-214) runs GTSAM's DoglegOptimizer control flow (mode
 * ONE_STEP_PER_ITERATION, deltaInitial = options->delta) on the same linearisation and Gauss-Newton solve;
 * its trace rows carry the trust-region radius in `lambda` and the model decrease in `lin_change`. */
int eacham_ba_solve(eacham_ctx* ctx, const eacham_ba_problem* problem, const eacham_ba_options* options,
                    eacham_ba_result* result);

/* Split form for callers that solve the same window repeatedly (the benchmark): prepare uploads the
 * problem and builds the device-side structure (observations grouped by landmark and by camera,
 * the camera-pair lists of the Schur complement); run restarts from the uploaded initial values,
 * so the timed region holds only device work and the per-try scalar read-backs. */
typedef struct eacham_ba_handle eacham_ba_handle;
int eacham_ba_prepare(eacham_ctx* ctx, const eacham_ba_problem* problem, eacham_ba_handle** out_handle);
int eacham_ba_run(eacham_ctx* ctx, eacham_ba_handle* handle, const eacham_ba_options* options,
                  eacham_ba_result* result);
void eacham_ba_release(eacham_ctx* ctx, eacham_ba_handle* handle);

/* What the analysis of the reduced camera system decided for a prepared problem (reporting: the benchmark's BA line
 * carries it): panels of 64 columns, tiles of the symbolic factor, height of the elimination tree = number of
 * dependent factorisation launches, the ordering used (EACHAM_BA_ORDER_NATURAL / _RCM / _ND), rank-64 tile updates of
 * one factorisation, the cost model's estimate for factorisation + back-substitution in microseconds, and where the
 * host time of eacham_ba_prepare went. */
typedef struct eacham_ba_plan_info {
    int32_t n_panels, n_tiles, n_levels, ordering, nd_leaf, reserved;
    int64_t tile_updates;
    double est_us;
    double prepare_us[3];  /* host time of eacham_ba_prepare: observation / pair structures | ordering + symbolic
                            * analysis | arena + upload + synchronisation */
} eacham_ba_plan_info;
int eacham_ba_get_plan_info(eacham_ctx* ctx, const eacham_ba_handle* handle, eacham_ba_plan_info* out);

/* Test/diagnostic entry point: one array of a prepared problem's device-side structure, as built by eacham_ba_prepare
 * (0 lm_ptr, 1 cam_ptr, 2 cam_obs, 3 obs_pos, 4 obs_cam, 5 obs_lm, 6 obs_uv, 7 cam_uv, 8 cam_lm, 9 pos_cam, 10 cam_chunks,
 * 11 cam_chunk_ptr, 12 blocks, 13 pair_chunks, 14 pair_entries, 15 pose0, 16 pt0, 17 lmprior, 18 K0, 19 fixed): the tests
 * hold the structure built by device sorts and scans against the one built by host loops, array by array. */
int eacham_ba_debug_structure(eacham_ctx* ctx, const eacham_ba_handle* handle, int which, void* out, int64_t cap_bytes,
                              int64_t* out_bytes);

/* Test/diagnostic entry point: linearises at the problem's initial values and returns the reduced
 * camera system of one damped Gauss-Newton step: S (n x n, row-major, n = 6*n_cams + 5, cameras
 * first, then K), its right-hand side g (n), the step delta for cameras+K (n) and for the points
 * (3*n_points), the nonlinear error at the linearisation point, and the linearised cost change. */
int eacham_ba_debug_step(eacham_ctx* ctx, const eacham_ba_problem* problem, double lambda,
                         double* S, double* g, double* delta_cams, double* delta_points,
                         double* error, double* lin_change);

/* ---- triangulation -------------------------------------------------
 * Batch form of TriangulateFrame's per-point call of TriangulatePointRansac
 * (/root/reference/modules/sfm/reconstruction/Triangulator.cpp:96-186 and :248-275; call sites
 * apps/sfm/main.cpp:203-210 with config.maxReprError / config.minTriAngle in radians).
 *   transforms   n_frames x 16 row-major world->camera matrices (Node::GetTransform)
 *   track_ptr    n_tracks+1 CSR offsets into the observation arrays (track = one candidate point, any number
 *                of observations: the reference has no limit and a long sequence can see a point a hundred times)
 *   obs_frame    row of `transforms` per observation;  obs_uv  pixel (x, y) per observation
 *   K            fx, fy, cx, cy
 * Outputs (host): points n_tracks x 3 = the `point3d` the reference leaves behind (the LAST pair's
 * triangulation); status[t] bit 0 = TriangulatePointRansac's return value, bit 1 = mask non-empty
 * and every observation an inlier — TriangulateFrame adds the point iff status[t] == 3 (:270-275);
 * masks = the reference's `inliers` vector per observation.
 * Tracks with fewer than 2 observations get status 0 and a zero point, as :104-107 does. */
int eacham_triangulate_tracks(eacham_ctx* ctx, const double* transforms, int n_frames, int n_tracks,
                              const int32_t* track_ptr, const uint32_t* obs_frame, const double* obs_uv,
                              const double* K, float max_repr_error, float min_tri_angle, double* points,
                              int32_t* status, uint8_t* masks);

/* Reprojection error of n (frame, map point, pixel) items: CalcReprojectionError(uv,
 * transformPoint3d(point, T[frame]), K) as a float (ProjectionHelper.cpp:32-38), the re-observation
 * gate of TriangulateFrame (Triangulator.cpp:222-236). */
int eacham_reprojection_errors(eacham_ctx* ctx, const double* transforms, int n_frames, int n,
                               const uint32_t* frame, const double* points, const double* uv, const double* K,
                               float* err);

/* Two-view structure for candidate relative poses (first part of SURVEY.md §8(f) rank 3): the per-match
 * loops of RecoverPoseTwoView (/root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:118-143
 * for the solutions of cv::decomposeHomographyMat, :162-186 for the pose of cv::recoverPose). Camera 1
 * is the identity; transforms[k] (row-major 4x4) maps camera-1 to camera-2 coordinates. For every
 * (transform k, match i): points[k][i] = TriangulatePoint(p1, p2, K, transform); keep[k][i] = 1 iff
 * z > 0 && reprojection error in camera 1 (rounded to float) < max_repr_error && the triangulation
 * angle passes: > min_tri_angle when angle_strict != 0 (the homography branch, :132), >= otherwise
 * (:170). counts[k] = kept matches (the reference picks the first k with the strictly largest count
 * and needs more than 20, :139-150). The robust E/H estimation itself stays with the caller. */
int eacham_two_view_points(eacham_ctx* ctx, int n_matches, const double* uv1, const double* uv2, const double* K,
                           int n_transforms, const double* transforms, float max_repr_error, float min_tri_angle,
                           int angle_strict, double* points, uint8_t* keep, int32_t* counts);

/* ---- hypothesis scoring for the robust estimators (rest of SURVEY.md §8(f) rank 3) -----------------------------
 * The part of cv::findEssentialMat / cv::findHomography (LMEDS) and cv::solvePnPRansac (EPNP, 10 000 iterations,
 * 4 px) — /root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:57-61, :75, :227-228 — that is
 * data-parallel over (hypothesis, correspondence): the error every candidate model assigns to every point, as
 * OpenCV 4.5.5's estimator callbacks define it (EMEstimatorCallback / HomographyEstimatorCallback /
 * PnPRansacCallback ::computeError), its inlier count under a
 * threshold (RANSAC: err <= threshold, the caller passes the squared pixel threshold as OpenCV does) and its median
 * (LMedS). One call scores all candidates; drawing the minimal samples and solving them stays with the caller.
 *   kind ESSENTIAL   a, b = n x 2 image points of view 1 / view 2; models = n_models x 9 row-major E. With K
 *                    (fx, fy, cx, cy) the points are normalised first, (u - cx) / fx, as findEssentialMat does;
 *                    K = NULL takes them as already normalised. err = Sampson distance (x2' E x1)^2 / (...), float.
 *   kind HOMOGRAPHY  a, b = n x 2; models = n_models x 9 row-major H (H[8] is taken as 1, as OpenCV's callback does);
 *                    err = |H a - b|^2 in float arithmetic. K unused.
 *   kind PNP         a = n x 3 object points, b = n x 2 image points; models = n_models x 12 = R (row-major) | t
 *                    (cv::Rodrigues of the candidate rvec is the caller's); K required; err = squared reprojection
 *                    error, projection in double, difference in float.
 * Outputs (each optional): errors n_models x n_points, inlier_counts n_models, medians n_models (sorted middle, or
 * the mean of the two middle values for even n; NaN for n = 0). */
#define EACHAM_SCORE_ESSENTIAL 0
#define EACHAM_SCORE_HOMOGRAPHY 1
#define EACHAM_SCORE_PNP 2
/*   kind FUNDAMENTAL a, b = n x 2 PIXELS of view 1 / view 2; models = n_models x 9 row-major F (x2' F x1 = 0). K is ignored (NULL or
 *                    not) and nothing is normalised. FMEstimatorCallback::computeError, the larger of the two squared distances
 *                    from a point to its epipolar line, fp64 with every operation rounded on its own, cast to float once:
 *                      l2[r] = (F[3r] a0 + F[3r+1] a1) + F[3r+2],  l1[r] = (F[r] b0 + F[3+r] b1) + F[6+r],
 *                      d = (b0 l2[0] + b1 l2[1]) + l2[2],  d2 = d d,
 *                      err = (float)std::max(d2 / (l1[0] l1[0] + l1[1] l1[1]), d2 / (l2[0] l2[0] + l2[1] l2[1])). */
#define EACHAM_SCORE_FUNDAMENTAL 3
int eacham_score_hypotheses(eacham_ctx* ctx, int kind, int n_points, const double* a, const double* b, int n_models,
                            const double* models, const double* K, float threshold, float* errors,
                            int32_t* inlier_counts, float* medians);

/* ---- minimal solvers of the robust estimators --------------------------------------------
 * The model-generating half of cv::findHomography / cv::findEssentialMat
 * (/root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:75, :57-61): every minimal sample of the
 * caller's list -> its model(s), one launch for the whole list (the reference asks for 100 / 1000 iterations).
 * OpenCV draws the samples from its own RNG inside the estimator; here the sample INDICES are an argument, so what is
 * defined — and tested against the CPU restatement bit for bit — is "these correspondences -> these models".
 *   kind HOMOGRAPHY4  a, b = n_points x 2 (source, destination); 4 indices per sample; 1 model = 9 doubles row-major,
 *                     H[8] = 1 (HomographyEstimatorCallback::runKernel). K unused.
 *   kind ESSENTIAL5   a, b = n_points x 2 pixels of view 1 / view 2, K = fx fy cx cy (NULL: already normalised);
 *                     5 indices per sample; up to 10 models of 9 doubles (unit Frobenius norm, x2' E x1 = 0), the slots
 *                     beyond n_models[s] are zero (Nister's five-point algorithm, EMEstimatorCallback::runKernel).
 * models: n_samples x max_models x 9 with max_models = 1 / 10; n_models: n_samples (0 = degenerate sample).
 * Pair it with eacham_score_hypotheses (all models against all correspondences) for the RANSAC / LMedS choice. */
#define EACHAM_SOLVE_HOMOGRAPHY4 0
#define EACHAM_SOLVE_ESSENTIAL5 1
/*   kind FUNDAMENTAL7 a, b = n_points x 2 pixels of view 1 / view 2; 7 indices per sample; up to 3 models of 9 doubles (row-major F,
 *                     x2' F x1 = 0, unit Frobenius norm), models = n_samples x 3 x 9, the slots beyond n_models[s] zero. K is not
 *                     read. OpenCV 4.5.5's run7Point restated with two deliberate deviations (parity with OpenCV is unpinned here
 *                     as everywhere):
 *                       1. Hartley normalisation: each image's 7 points are moved to their centroid (p0 + sum(pi - p0) / 7) and scaled to a mean distance
 *                          of sqrt(2) from it (fp64, sums in index order), the models are denormalised as T2' F^ T1. OpenCV solves
 *                          on raw pixels with an SVD of the 7 x 9 system; here the null space comes from the 9 x 9 Jacobi
 *                          eigen-solver on A'A (the homography's), which squares the condition number and needs the normalisation.
 *                       2. A model has unit Frobenius norm after denormalisation (as ESSENTIAL5's), not F[8] = 1.
 *                     Null space: f2 = eigenvector of the smallest eigenvalue, f1 = that of the second smallest, minus f2; the
 *                     cubic det(z f1 + f2) by run7Point's c[] expressions; its roots by a Durand-Kerner recipe of its own (degree
 *                     drop at 1e-14 cmax, a root is real iff |zi| <= 1e-7 (1 + |zr|), four Newton steps, real roots ascending).
 *                     A degenerate sample is no error: n_models = 0 and zero models when a normalisation scale is not finite (all
 *                     points of one image coincide), the cubic is all zero or no real root is left. */
#define EACHAM_SOLVE_FUNDAMENTAL7 2
int eacham_solve_minimal(eacham_ctx* ctx, int kind, int n_points, const double* a, const double* b, const double* K,
                         int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models);

/* EPnP, the solver inside cv::solvePnPRansac(..., 10000, 4.0f, 0.999f, inliers, cv::SOLVEPNP_EPNP)
 * (/root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:227-228): OpenCV runs it on 5-point samples inside
 * the RANSAC loop and once more on the inliers of the winning model. Here every row of sample_idx (sample_size >= 5 indices
 * into the n_points object / image points) is one EPnP problem, one launch for the whole list: 10 000 rows of 5 for the
 * loop, one row of all inliers for the refit. models: n_samples x 12 = R (row-major) | t with x_cam = R X + t — the layout
 * eacham_score_hypotheses(kind PNP) scores; n_models[s] = 1, or 0 (model zeroed) for a degenerate sample (collinear or
 * coincident points). A COPLANAR sample (smallest spread of its object points <= 1e-12 of the largest) gets a pose too, as
 * cv::solvePnPRansac returns one for a planar target: the three-control-point form of the EPnP paper (oracle/solve_oracle.c's
 * header states it). K = fx fy cx cy, no distortion (the reference passes zeros).
 * Bit-identical with oracle/solve_oracle.c's oracle_solve_pnp. */
int eacham_solve_pnp(eacham_ctx* ctx, int n_points, const double* object_points, const double* image_points, const double* K,
                     int sample_size, int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models);

/* ---- LMedS two-view estimation for a whole list of pairs ---------------------------------------------------------
 * cv::findEssentialMat(LMEDS) / cv::findHomography(LMEDS) for every edge of a match graph in ONE call: what
 * eacham_solve_minimal + eacham_score_hypotheses + the LMedS rule between them (include/eacham/TwoViewHip.hpp) do for
 * one pair, for n_problems pairs with no host turn between the stages and a launch count that does not depend on
 * n_problems. Problem p owns the points point_ptr[p] .. point_ptr[p+1] of a / b (rows of 2 doubles) and the samples
 * sample_ptr[p] .. sample_ptr[p+1] of sample_idx (4 / 5 indices per sample, LOCAL to the problem's points; drawing them
 * stays with the caller, as for eacham_solve_minimal). Both offset tables have n_problems + 1 entries, start at 0 and
 * do not decrease. kind = EACHAM_SOLVE_HOMOGRAPHY4 | EACHAM_SOLVE_ESSENTIAL5 | EACHAM_SOLVE_FUNDAMENTAL7 (7 indices per sample,
 * up to 3 candidates per sample, scored with EACHAM_SCORE_FUNDAMENTAL, K ignored); K = fx fy cx cy shared by all problems
 * (NULL as in eacham_solve_minimal). Per problem, with n points and m = 4 / 5 / 7:
 *   every sample is solved and the candidates are flattened in sample order, then root order; every candidate's median
 *   error over the problem's own points is taken; the winner is the FIRST candidate with the smallest non-NaN median
 *   (TIES: equal medians keep the earlier candidate); sigma = max(2.5 * 1.4826 * (1 + 5 / max(n - m, 1)) *
 *   sqrt((double)median), 0.001) in fp64, threshold = (float)(sigma * sigma); mask[i] = err_winner(i) <= threshold.
 * Outputs (each optional, NULL = not wanted): models n_problems x 9 (the winner as solved), medians, thresholds,
 * inliers (mask bytes set), masks (point_ptr[n_problems] bytes, in the layout of a / b), winner n_problems x 3 =
 * {candidate index in the problem's flattened list, sample (local to the problem), root}, n_candidates.
 * The "NONE" RECORD: a problem with fewer than m points (its samples are then not looked at), with no samples, with no
 * candidate (every sample degenerate) or with only NaN medians gets winner -1 -1 -1, a zero model, a NaN median, a
 * zero threshold, zero inliers and a zero mask; n_candidates is still its count. Its neighbours are not affected.
 * Bit-identical, output by output, with the composition of eacham_solve_minimal and eacham_score_hypotheses per problem.
 * EACHAM_ERR_INVALID: bad kind, negative size, an offset table that is null / does not start at 0 / decreases, a null
 * required array, a sample index outside its problem (checked on the host before anything is launched; the message
 * names the problem). */
int eacham_lmeds_batch(eacham_ctx* ctx, int kind, int n_problems, const int64_t* point_ptr, const double* a, const double* b,
                       const double* K, const int64_t* sample_ptr, const int32_t* sample_idx, double* models, float* medians,
                       float* thresholds, int32_t* inliers, uint8_t* masks, int32_t* winner, int32_t* n_candidates);

/* ---- Threshold RANSAC two-view estimation for a whole list of pairs -------------------------------------------------
 * cv::findEssentialMat / cv::findHomography / cv::findFundamentalMat with cv::RANSAC for every edge of a match graph in ONE
 * call. Inputs, layouts and host-side checks are those of eacham_lmeds_batch; the selection is RANSACPointSetRegistrator::run
 * (OpenCV 4.5.5, from memory). threshold: already SQUARED, in the error's own units, as eacham_score_hypotheses takes it
 * (essential with K: the K-normalised unit). Per problem, with n points, sample size m = 4 / 5 / 7 and S samples in order:
 *     budget = S; best = -1; winner = none
 *     for s = 0, 1, ... while s < budget:
 *         for every root r of sample s, in root order (a degenerate sample has none):
 *             cnt = #{ i : err(point i, model) <= threshold }
 *             if cnt > max(best, m - 1):                   strictly more: the earlier candidate stays
 *                 best = cnt; winner = (s, r)
 *                 budget = ransac_update_num_iters(confidence, (double)(n - cnt) / n, m, budget)     (include/eacham/RansacIters.hpp)
 *     n_used = samples whose roots were looked at
 * The budget is tested per sample: a record in root 0 that drops the budget below s + 1 does not keep roots 1.. of the same
 * sample from being counted, and they may win. ransac_update_num_iters is evaluated on the HOST only (an integer table per
 * distinct n goes to the device): no device pow / log / lround decides anything.
 * Outputs (each optional): models n_problems x 9 (the winner as solved), inliers (= best), masks (mask[i] = err_winner(i) <=
 * threshold; point_ptr[n_problems] bytes), winner n_problems x 3 = {candidate index among the candidates of the n_used consumed
 * samples, sample, root}, n_candidates = the candidates of the n_used consumed samples, n_used.
 * The "NONE" RECORD — winner -1 -1 -1, a zero model, zero inliers, a zero mask, n_used = S, n_candidates as defined — goes to a
 * problem with fewer than m points (then n_used = 0 and its samples are not looked at), with no samples, with no candidate, or
 * with no count above m - 1. Its neighbours are not affected. n == m is NOT special-cased here: OpenCV's shortcut for it (the
 * minimal solver's answer without a loop) belongs to the adapters of include/eacham/TwoViewHip.hpp.
 * stage1: the samples of every problem that are solved and counted before the budgets are first looked at; only the ranks
 * stage1 .. budget - 1 are solved after that (their number comes back in one 8-byte read). 0 = the library's default; any value
 * >= the largest S is a single pass with no read-back. Every output is byte-identical for every stage1.
 * Byte for byte the composition of eacham_solve_minimal, the inlier counts of eacham_score_hypotheses and the rule above.
 * EACHAM_ERR_INVALID: as eacham_lmeds_batch, and a NaN or negative threshold, a confidence outside (0, 1), a negative stage1. */
int eacham_ransac_batch(eacham_ctx* ctx, int kind, int n_problems, const int64_t* point_ptr, const double* a, const double* b,
                        const double* K, const int64_t* sample_ptr, const int32_t* sample_idx, float threshold, double confidence,
                        int stage1, double* models, int32_t* inliers, uint8_t* masks, int32_t* winner, int32_t* n_candidates,
                        int32_t* n_used);
/* Diagnostic: how the context's last eacham_ransac_batch / eacham_graph_verify_ransac ran (any pointer may be NULL). samples_solved =
 * minimal samples handed to the solver over both passes (a single pass: all of them), table_ms = host milliseconds spent building
 * the budget rows. */
int eacham_ransac_debug_last(eacham_ctx* ctx, int64_t* samples_solved, double* table_ms);

/* ---- PnP RANSAC for a whole list of problems ------------------------------------------------------------------------
 * cv::solvePnPRansac(..., SOLVEPNP_EPNP) (/root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:227-228) for
 * a list of (map points, pixels) problems: what eacham_solve_pnp + eacham_score_hypotheses(kind PNP) do for one frame per
 * chunk of samples, and once more for the refit, for n_problems frames per call with no host turn between the stages and a
 * launch count that does not depend on n_problems. The round loop and the sequential RANSAC rule between the two calls stay
 * on the host (include/eacham/PnPHip.hpp: SolvePnPRansacBatch). Problem p owns the rows point_ptr[p] .. point_ptr[p+1] of
 * object_points (3 doubles) and image_points (2 doubles, pixels); point_ptr has n_problems + 1 entries, starts at 0 and does
 * not decrease. K = fx fy cx cy, shared by all problems, required.
 *
 * eacham_pnp_hypotheses_batch: ONE RANSAC ROUND for every problem. Problem p owns the samples sample_ptr[p] ..
 * sample_ptr[p+1] (a table like point_ptr) of sample_idx: sample_size indices per sample (5 <= sample_size <= 64), LOCAL to
 * the problem's points. threshold: squared pixels, as eacham_score_hypotheses takes it. Per sample: models (12 doubles,
 * R | t; optional, NULL = not wanted), n_models (1, or 0 with a zero model for a degenerate sample) and inlier_counts (the
 * problem's own points with err <= threshold under the sample's model; 0 where n_models is 0). A problem with no samples
 * in this call costs nothing (later rounds address only the problems still running); one with fewer than sample_size
 * points gets n_models = 0 for all its samples, which are then not looked at.
 * Bit-identical, output by output, with eacham_solve_pnp on the problem's rows followed by
 * eacham_score_hypotheses(kind PNP) per problem.
 *
 * eacham_pnp_refit_batch: THE TAIL of solvePnPRansac for every problem. models: 12 doubles per problem, has_model: one byte
 * per problem. Per problem with a model: inlier_mask[i] = err(i) <= threshold (bytes, in the layout of image_points),
 * n_inliers, and EPnP on the inliers IN ASCENDING POINT INDEX: refit (12 doubles) and refit_ok. A problem without a model,
 * with fewer than 5 inliers or with an inlier set EPnP calls degenerate (collinear or coincident) is not an error:
 * refit_ok = 0 and a zero refit; the mask and the count are still written (the real ones; zero without a model). Its
 * neighbours are not affected. Every output is required.
 * Bit-identical with eacham_score_hypotheses (one model, errors requested), the host compaction err <= threshold and
 * eacham_solve_pnp on one row of all inliers, per problem, whatever the size of the inlier set.
 *
 * EACHAM_ERR_INVALID: a negative size, an offset table that is null / does not start at 0 / decreases, a null required
 * array, sample_size outside 5..64, a sample index outside its problem (checked on the host before anything is launched;
 * the message names the problem). EACHAM_ERR_CAPACITY: more than 2^31 - 1 points or samples in one call. */
int eacham_pnp_hypotheses_batch(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                                const double* image_points, const double* K, const int64_t* sample_ptr, int sample_size,
                                const int32_t* sample_idx, float threshold, double* models, int32_t* n_models,
                                int32_t* inlier_counts);
int eacham_pnp_refit_batch(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                           const double* image_points, const double* K, const double* models, const uint8_t* has_model,
                           float threshold, uint8_t* inlier_mask, int32_t* n_inliers, double* refit, int32_t* refit_ok);

/* ---- PnP pose refinement for a whole list of problems ---------------------------------------------------------------
 * cv::solvePnPRefineLM (the polish of SOLVEPNP_ITERATIVE; from memory of OpenCV 4.5.5, unverified: the idea, not the bits): where
 * eacham_pnp_refit_batch ends on EPnP's algebraic fit, this minimises the REPROJECTION error of a pose over the rows the caller
 * names, by Levenberg-Marquardt, for n_problems problems in ONE launch with the whole loop on the device. Tables and layouts as
 * eacham_pnp_refit_batch: problem p owns the rows point_ptr[p] .. point_ptr[p+1] of object_points / image_points; K = fx fy cx cy.
 * poses: 12 doubles R | t per problem, has_pose: one byte per problem. use_mask: one byte per point in the layout of image_points
 * (optional, NULL = every point); the USED rows of a problem are those with a non-zero byte. threshold (squared pixels) serves the
 * recount only. Outputs per problem: refined (12 doubles), cost (2 doubles: the sum of squared pixel residuals over the used rows
 * before and after), tries, status; optional (NULL = not wanted, each on its own): inlier_mask (bytes, layout of image_points) and
 * n_inliers, the recount err <= threshold of eacham_score_hypotheses(kind PNP) over ALL of the problem's points under `refined`
 * — what eacham_pnp_refit_batch writes for that pose (all zero where has_pose is 0).
 *
 * THE LOOP. fp64 throughout, only + - * /, every operation rounded on its own, every sum in the order written
 * (tests/cpp/pnp_refine_reference.c is the CPU restatement; the kernel gives its bytes):
 *   1. A row (X, (u, v)) under M = R | t:  x y z = R X + t (each ((m0 X0 + m1 X1) + m2 X2) + t),  iz = 1 / z,  xn = x iz,  yn = y iz,
 *      r = ((fx xn + cx) - u, (fy yn + cy) - v). The perturbation d = [w, v] acts in the camera frame, X_c' ~ X_c + w x X_c + v, so with
 *      a = fx iz, b = fy iz:   Ju = (-(fx xn yn), fx (1 + xn xn), -(fx yn), a, 0, -(a xn)),
 *                              Jv = (-(fy (1 + yn yn)), fy xn yn, fy xn, 0, b, -(b yn)).
 *   2. Sums. 28 numbers: H = J'J (upper triangle, row by row, 21), g = J'r (6), cost = r'r. A row adds
 *      H_ij += (Ju_i Ju_j + Jv_i Jv_j), g_i += (Ju_i r_0 + Jv_i r_1), cost += (r_0 r_0 + r_1 r_1). THE ORDER: 64 partial sums start at
 *      zero; partial l takes the used rows i of the problem (i local to it) with i mod 64 = l, in ascending i; then the partials are
 *      folded in halves, s[l] += s[l + off] for l < off, off = 32, 16, 8, 4, 2, 1, and s[0] is the sum.
 *   3. A try at damping lambda (1e-3 at the start): A = H with A_ii = H_ii + lambda H_ii; A = L D L' without pivoting (column by
 *      column, each entry minus its products L_ik D_k L_jk in ascending k, then divided by the pivot); a pivot that is not > 0 fails
 *      the try. Else L y = -g, z = y / D, L' d = z (back substitution, products subtracted in ascending k).
 *   4. If max |d_k| <= 1e-10 the loop ends CONVERGED (tested before the step is taken, whatever came before). Else the candidate is
 *      R' = C(w) R, t' = C(w) t + v with the Cayley map of the bundle adjuster's Pose3 chart,
 *      C(w) = ((4 - |w|^2) I + 2 w w' + 4 [w]x) / (4 + |w|^2), and step 2 at the candidate gives cost', H', g'.
 *   5. The candidate is ACCEPTED iff no used row has !(z > 0) under it and cost' < cost: the pose, H, g and the cost become the
 *      candidate's and lambda <- max(lambda / 10, 1e-12); if cost - cost' <= 1e-9 cost' the loop ends CONVERGED. A failed or
 *      rejected try: lambda <- min(10 lambda, 1e12).
 *   6. After max_tries tries (every solve attempted counts, also the one that finds the small step) the loop ends CAP.
 * NOT_REFINED (no error; refined = the input pose, or zero where has_pose is 0; both costs equal: the sum at the input pose, a NaN
 * as 0x7ff8000000000000, 0 without a pose; tries = 0): has_pose = 0, fewer than 3 used rows, a used row with !(z > 0) at the start,
 * a start cost that is not finite (a NaN or infinity in the pose, K or a used row). Rows that are not used are never read by the
 * loop. A problem's outputs depend on its own rows only: not on its neighbours, the length of the list or its place in it.
 *
 * EACHAM_ERR_INVALID (checked on the host before anything is launched or written; the message names the problem): a negative
 * size, an offset table that is null / does not start at 0 / decreases, a null required array, max_tries < 1, a NaN or negative
 * threshold while inlier_mask or n_inliers is asked for. EACHAM_ERR_CAPACITY: more than 2^31 - 1 points in one call. */
#define EACHAM_PNP_REFINE_CONVERGED 0
#define EACHAM_PNP_REFINE_CAP 1          /* max_tries reached */
#define EACHAM_PNP_REFINE_NOT_REFINED 2
int eacham_pnp_refine_batch(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                            const double* image_points, const double* K, const double* poses, const uint8_t* has_pose,
                            const uint8_t* use_mask, int max_tries, float threshold, double* refined, double* cost, int32_t* tries,
                            int32_t* status, uint8_t* inlier_mask, int32_t* n_inliers);

/* ---- track point refinement for a whole list of tracks ---------------------------------------------------------------
 * The non-linear step that COLMAP and OpenCV's sfm module run after triangulation, the counterpart of eacham_pnp_refine_batch with
 * the roles swapped: where eacham_triangulate_tracks ends on the two-view DLT point of the LAST pair tried, this minimises the
 * REPROJECTION error of a track's 3-D point over the observations the caller names, the cameras held fixed, by
 * Levenberg-Marquardt, for n_tracks tracks in ONE launch with the whole loop on the device. Layouts as
 * eacham_triangulate_tracks: transforms = n_frames row-major 4 x 4 world->camera matrices T, obs_frame = the row of `transforms`
 * per observation, obs_uv = its pixel (u, v), K = fx fy cx cy; track t owns the observations track_ptr[t] .. track_ptr[t+1], and
 * track_ptr is int64_t as eacham_tracks_build writes it. points: 3 doubles per track (the start), has_point: one byte per track.
 * use_mask: one byte per observation (optional, NULL = every observation); the USED observations of a track are those with a
 * non-zero byte (eacham_triangulate_tracks' masks serve as they are). max_repr_error (pixels) serves the recount only. Outputs per
 * track: refined (3 doubles), cost (2 doubles: the sum of squared pixel residuals over the used observations before and after),
 * tries, status; optional (NULL = not wanted, each on its own): inlier_mask (one byte per observation) and n_inliers, the recount
 * over ALL of the track's observations at `refined` with the predicate of eacham_triangulate_tracks: the float reprojection error
 * (float)sqrt(du du + dv dv) < max_repr_error and the depth >= DBL_EPSILON (all zero where has_point is 0).
 *
 * THE LOOP. fp64 throughout, only + - * /, every operation rounded on its own, every sum in the order written
 * (tests/cpp/tri_refine_reference.c is the CPU restatement; the kernel gives its bytes):
 *   1. An observation (T, (u, v)) at the point X:  x y z = T X (each ((T_i0 X0 + T_i1 X1) + T_i2 X2) + T_i3, i = 0, 1, 2),
 *      iz = 1 / z,  xn = x iz,  yn = y iz,  r = ((fx xn + cx) - u, (fy yn + cy) - v). The derivative by X, with a = fx iz, b = fy iz:
 *      Ju_j = a (T_0j - xn T_2j),  Jv_j = b (T_1j - yn T_2j),  j = 0, 1, 2.
 *   2. Sums. 10 numbers: H = J'J (upper triangle, row by row, 6), g = J'r (3), cost = r'r. An observation adds
 *      H_ij += (Ju_i Ju_j + Jv_i Jv_j), g_i += (Ju_i r_0 + Jv_i r_1), cost += (r_0 r_0 + r_1 r_1). THE ORDER: 8 partial sums start at
 *      zero; partial l takes the used observations i of the track (i local to it, counted over all of its observations, used or
 *      not) with i mod 8 = l, in ascending i; then the partials are folded in halves, s[l] += s[l + off] for l < off,
 *      off = 4, 2, 1, and s[0] is the sum.
 *   3. A try at damping lambda (1e-3 at the start): A = H with A_ii = H_ii + lambda H_ii; A = L D L' without pivoting (column by
 *      column, each entry minus its products L_ik D_k L_jk in ascending k, then divided by the pivot); a pivot that is not > 0 fails
 *      the try. Else L y = -g, z = y / D, L' d = z (back substitution, products subtracted in ascending k).
 *   4. If max |d_k| <= 1e-10 (1 + max |X_k|) the loop ends CONVERGED (tested before the step is taken, whatever came before).
 *      Else the candidate is X' = X + d, and step 2 at the candidate gives cost', H', g'.
 *   5. The candidate is ACCEPTED iff no used observation has !(z > 0) at it and cost' < cost: the point, H, g and the cost become
 *      the candidate's and lambda <- max(lambda / 10, 1e-12); if cost - cost' <= 1e-9 cost' the loop ends CONVERGED. A failed or
 *      rejected try: lambda <- min(10 lambda, 1e12).
 *   6. After max_tries tries (every solve attempted counts, also the one that finds the small step) the loop ends CAP.
 * NOT_REFINED (no error; refined = the input point, or zero where has_point is 0; both costs equal: the sum at the input point, a
 * NaN as 0x7ff8000000000000, 0 without a point; tries = 0): has_point = 0, fewer than 2 used observations, a used observation with
 * !(z > 0) at the start, a start cost that is not finite (a NaN or infinity in the point, K, a used pixel or its transform).
 * Observations that are not used are never read by the loop. A track's outputs depend on its own observations only: not on its
 * neighbours, the length of the list or its place in it.
 *
 * EACHAM_ERR_INVALID (checked on the host before anything is launched or written; the message names the problem): a negative
 * size, a track_ptr that is null / does not start at 0 / decreases, a null required array, max_tries < 1, an obs_frame entry
 * >= n_frames (the message names the track), a NaN or negative max_repr_error while inlier_mask or n_inliers is asked for.
 * EACHAM_ERR_CAPACITY: more than 2^31 - 1 observations in one call. */
#define EACHAM_TRI_REFINE_CONVERGED 0
#define EACHAM_TRI_REFINE_CAP 1          /* max_tries reached */
#define EACHAM_TRI_REFINE_NOT_REFINED 2
int eacham_triangulate_refine_tracks(eacham_ctx* ctx, const double* transforms, int n_frames, int n_tracks,
                                     const int64_t* track_ptr, const uint32_t* obs_frame, const double* obs_uv, const double* K,
                                     const double* points, const uint8_t* has_point, const uint8_t* use_mask, int max_tries,
                                     float max_repr_error, double* refined, double* cost, int32_t* tries, int32_t* status,
                                     uint8_t* inlier_mask, int32_t* n_inliers);

/* ---- P3P: the PnP RANSAC on its minimal sample ------------------------------------------------------------------------
 * What cv::solvePnPRansac(..., cv::SOLVEPNP_P3P) draws: FOUR indices per sample — three correspondences give up to four poses,
 * the fourth picks one. The refit of the winner's inliers stays EPnP (eacham_pnp_refit_batch, unchanged; from memory of OpenCV
 * 4.5.5, unverified: parity is unpinned here as everywhere). The sample indices are an argument, so what is defined is "these
 * four correspondences -> this pose". Layouts as eacham_solve_pnp: models = R (row-major) | t, 12 doubles, K = fx fy cx cy.
 *
 * THE SOLVER. A sample i0 i1 i2 i3 has object points X0..X3 and pixels x0..x3. fp64 throughout, only + - * / sqrt, fabs, fmax,
 * fmin, every operation rounded on its own, every sum in the order written (tests/cpp/p3p_reference.c is the CPU restatement;
 * the kernels give its bytes):
 *   1. Bearings  y_k = ((u_k - cx) / fx, (v_k - cy) / fy, 1), f_k = y_k / sqrt(y_k . y_k), k = 0, 1, 2.
 *   2. Triangle  A = |X1 - X2|^2, B = |X0 - X2|^2, C = |X0 - X1|^2; ca = f1 . f2, cb = f0 . f2, cg = f0 . f1.
 *      DEGENERATE (n_models = 0, a zero model, no error): A, B or C zero or not finite; a bearing not finite; collinear object
 *      points, |(X1 - X0) x (X2 - X0)|^2 <= 1e-20 B C.
 *   3. Grunert's quartic in v = s2 / s0 (s_k: the depth along f_k). p = (A - C) / B, q = (A + C) / B, rA = A / B, rC = C / B:
 *        A4 = (p - 1)^2 - 4 rC ca^2
 *        A3 = 4 [ p (1 - p) cb - (1 - q) ca cg + 2 rC ca^2 cb ]
 *        A2 = 2 [ p^2 - 1 + 2 p^2 cb^2 + 2 (1 - rC) ca^2 - 4 q ca cb cg + 2 (1 - rA) cg^2 ]
 *        A1 = 4 [ -p (1 + p) cb + 2 rA cg^2 cb - (1 - q) ca cg ]
 *        A0 = (1 + p)^2 - 4 rA cg^2
 *   4. Its real roots by FUNDAMENTAL7's Durand-Kerner recipe carried to degree <= 4 (degree drop at 1e-14 cmax, monic, start
 *      values r0 (0.4 + 0.9 i)^k, at most 200 sweeps stopped at a correction of 1e-11 bound, a root is real iff
 *      |zi| <= 1e-7 (1 + |zr|), four Newton steps on the real polynomial, real roots ascending).
 *   5. Per real root v, ascending: den = 2 (cg - v ca), skipped if 0; u = [(p - 1) v^2 - 2 p cb v + 1 + p] / den;
 *      d = 1 + v^2 - 2 v cb, skipped unless > 0; s0 = sqrt(B / d), s1 = u s0, s2 = v s0; then TWO Newton steps on (s0, s1, s2)
 *      for  s1^2 + s2^2 - 2 s1 s2 ca = A,  s0^2 + s2^2 - 2 s0 s2 cb = B,  s0^2 + s1^2 - 2 s0 s1 cg = C  (Cramer's rule, the
 *      determinant expanded along the first row; skipped if it is 0 or a depth comes out not finite); skipped unless all three
 *      depths are > 0. (Without the two steps a near-double root leaves errors of 1e-7 and an occasional missed pose.)
 *   6. Pose. Q_k = s_k f_k. The frame of a triangle (P0, P1, P2): e1 = (P1 - P0) / |P1 - P0|, e3 = e1 x (P2 - P0) normalised,
 *      e2 = e3 x e1, as the columns of F(P). R = F(Q) F(X)', t = Q0 - R X0.
 *   7. The fourth point chooses: the candidate with the FIRST STRICTLY SMALLEST eacham_score_hypotheses(kind PNP) error of
 *      (X3, x3), in root order; a NaN error never wins; no candidate, or only NaN errors: n_models = 0.
 * DEVIATION FROM OPENCV: cv's p3p.cpp follows Gao et al. and solves its quartic in closed form; this is Grunert's elimination of
 * the same three equations with an iterative root finder and a polish of the depths: the same solution set, not the same bits.
 * Duplicate indices are legal: one among the first three gives a zero side (degenerate); a fourth equal to one of the three is fine.
 *
 * eacham_solve_p3p: every row of sample_idx (4 indices into the n_points points) -> models (n_samples x 12) and n_models (1, or
 * 0 with a zero model). Optional (NULL = not wanted): candidates (n_samples x 4 x 12, every pose of step 5-6 in root order, the
 * slots behind the count zero) and n_candidates.
 * EACHAM_ERR_INVALID: a null required argument, a negative size, a sample index outside the points (checked on the host before
 * anything is launched).
 *
 * eacham_pnp_hypotheses_batch_p3p: ONE RANSAC ROUND for every problem of a list in ONE launch — eacham_pnp_hypotheses_batch with
 * the sample size fixed at 4 and the solver above: same tables, same outputs (models optional), same rules (a problem with no
 * samples costs nothing; one with fewer than 4 points gets n_models = 0 for all its samples, which are then not looked at).
 * Bit-identical, output by output, with eacham_solve_p3p on the problem's rows followed by eacham_score_hypotheses(kind PNP)
 * per problem. Errors: those of eacham_pnp_hypotheses_batch (there is no sample_size to be wrong). */
int eacham_solve_p3p(eacham_ctx* ctx, int n_points, const double* object_points, const double* image_points, const double* K,
                     int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models, double* candidates,
                     int32_t* n_candidates);
int eacham_pnp_hypotheses_batch_p3p(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* object_points,
                                    const double* image_points, const double* K, const int64_t* sample_ptr,
                                    const int32_t* sample_idx, float threshold, double* models, int32_t* n_models,
                                    int32_t* inlier_counts);

/* ---- two-view motion and structure for a whole list of pairs ------------------------------------------------------
 * The second half of RecoverPoseTwoView (/root/reference/modules/sfm/reconstruction/ReconstructionManager.cpp:89-180)
 * for every edge of a match graph in ONE call: what eacham_two_view_points plus the host rules behind it
 * (cv::recoverPose's cheirality vote and the structure of its winner, :153-177; the choice among the solutions of
 * cv::decomposeHomographyMat, :98-144) do for one pair, for n_problems pairs with two launches whatever n_problems is
 * and only the WINNER's structure coming back. Problem p owns the points point_ptr[p] .. point_ptr[p+1] of uv1 / uv2
 * (rows of 2 doubles, pixels) and the candidate transforms transform_ptr[p] .. transform_ptr[p+1] (16 doubles each,
 * row-major, camera-1 -> camera-2; decomposing E / H into them stays with the caller, 3x3 host work). Both offset tables
 * have n_problems + 1 entries, start at 0 and do not decrease. K = fx fy cx cy is shared; rule[p] is one of the two
 * below; in_mask (point_ptr[n_problems] bytes in the layout of uv1, NULL = all ones) is read by the POSES rule only.
 * For every (candidate k, match i) the point X, the float reprojection error in camera 1 and the triangulation angle
 * are exactly eacham_two_view_points'. Then, per problem:
 *   EACHAM_TWOVIEW_POSES      ch(k,i) = in_mask[i] && 0 < z1 < distance_thresh && 0 < z2 < distance_thresh with z1 = X[2],
 *                             z2 = ((T[8] X0 + T[9] X1) + T[10] X2) + T[11], every operation rounded on its own;
 *                             cand_counts[k] = sum of ch(k,.); the winner is candidate 0 unless a later one has a STRICTLY
 *                             larger count; good = its count, pose_mask = its ch. For the winner only, keep(i) = z > 0 &&
 *                             err < max_repr_error && !(angle < min_tri_angle) (independent of in_mask), kept = its sum.
 *   EACHAM_TWOVIEW_SOLUTIONS  keep(k,i) = z > 0 && err < max_repr_error && angle > min_tri_angle; cand_counts[k] = its sum;
 *                             the winner is the first k with the strictly largest non-zero count, accepted only if that
 *                             count is > min_solution_matches (the reference: 20); good = 0, pose_mask = 0.
 * Outputs (all required): winner, good, kept (n_problems each), cand_counts (transform_ptr[n_problems]), points (3 per
 * point: the WINNER's, all of the problem's points as eacham_two_view_points returns them), keep and pose_mask (one
 * byte per point, in the layout of uv1).
 * The "NONE" RECORD: a problem without candidates, or a SOLUTIONS problem whose best count is not accepted, gets winner
 * -1, good = kept = 0, zero keep / pose_mask and zero points; its cand_counts are still written. A POSES problem with
 * candidates and no points has winner 0 and good = 0. Its neighbours are not affected.
 * Bit-identical, output by output, with eacham_two_view_points on the problem's candidates followed by those rules.
 * EACHAM_ERR_INVALID (checked on the host before anything is launched or written; the message names the problem): an
 * unknown rule, a negative size, an offset table that is null / does not start at 0 / decreases, a null required array.
 * EACHAM_ERR_CAPACITY: more than 2^31 - 1 points, candidates or (candidate, match) items in one call. */
#define EACHAM_TWOVIEW_POSES 0
#define EACHAM_TWOVIEW_SOLUTIONS 1
int eacham_two_view_batch(eacham_ctx* ctx, int n_problems, const int64_t* point_ptr, const double* uv1, const double* uv2,
                          const double* K, const int32_t* rule, const int64_t* transform_ptr, const double* transforms,
                          const uint8_t* in_mask, float max_repr_error, float min_tri_angle, double distance_thresh,
                          int min_solution_matches, int32_t* winner, int32_t* good, int32_t* kept, int32_t* cand_counts,
                          double* points, uint8_t* keep, uint8_t* pose_mask);

/* ---- view-graph query on the CSR match graph --------------------------
 * Graph::GetBestPairForValid (/root/reference/modules/sfm/data/Graph.h:59-106) evaluated directly on the
 * wire format of eacham_match_all_pairs: pair p with counts[p] > 0 is the factor f1 -> f2 with matches
 * q -> t and the factor f2 -> f1 with t -> q (Graph::Connect both ways, apps/sfm/main.cpp:144-145).
 *   valid[f]        Node::IsValid();  excluded[f] (may be NULL) = the `excluded` set
 *   kp_offsets      n_frames+1 offsets into kp_has3d;  kp_has3d[kp_offsets[f] + k] = 1 iff
 *                   node f HasPoint3d(k) && !IsPoint3dTwoView(k)
 * best = {id, id2, points3dCount} of the reference's tuple ({UINT_MAX, UINT_MAX, 0} when no valid node
 * has a not-yet-valid, not-excluded neighbour). A candidate replaces the best unless
 * `bestScore > count`, so among equal counts the last visited wins; nodes are visited in ascending id
 * as in the reference and neighbours in ascending id (the reference's unordered_map has no order).
 * edge_counts (optional, 2*npairs): points3dCount of f1 -> f2 and of f2 -> f1 for every pair. */
int eacham_graph_best_pair(eacham_ctx* ctx, int n_frames, const int32_t* pairs, int npairs, const int32_t* counts,
                           const int64_t* offsets, const uint32_t* q, const uint32_t* t, const uint8_t* valid,
                           const uint8_t* excluded, const int64_t* kp_offsets, const uint8_t* kp_has3d,
                           uint32_t* edge_counts, uint32_t* best);

/* The resident form of the same query, for the incremental loop of apps/sfm/main.cpp:188-214, which asks it after every frame
 * it adds: the CSR match graph is validated and uploaded once (eacham_graph_create: same arguments as above minus the per-frame
 * state; kp_offsets gives every frame's keypoint count), the per-frame state — Node::IsValid() and, per keypoint,
 * HasPoint3d(k) && !IsPoint3dTwoView(k) — is set frame by frame as the loop changes it (eacham_graph_set_frame: the frame it
 * just posed and triangulated and that frame's factor neighbours are the only ones that change between two queries), and
 * eacham_graph_query(excluded set) is two small kernels. Same result as eacham_graph_best_pair on the same state. The graph
 * belongs to its context (calls are serialised with the context's others); destroy it before the context. */
typedef struct eacham_graph eacham_graph;
int eacham_graph_create(eacham_ctx* ctx, int n_frames, const int32_t* pairs, int npairs, const int32_t* counts, const int64_t* offsets,
                        const uint32_t* q, const uint32_t* t, const int64_t* kp_offsets, eacham_graph** out_graph);
void eacham_graph_destroy(eacham_graph* graph);
int eacham_graph_set_frame(eacham_graph* graph, int frame, int valid, const uint8_t* has3d, int n_keypoints);
/* Several frames in one call — what the loop does after every frame it adds: the frame and its ~20 factor neighbours
 * (apps/sfm/main.cpp:203-209: TriangulateFrame's SetPoint3d reaches exactly those). frames[i], valid[i], and the frames' flag
 * arrays one behind the other in has3d (frame i's start at has3d_offsets[i], has3d_offsets[n] = total; every frame's full
 * keypoint count). One copy and one kernel instead of two small copies per frame. */
int eacham_graph_set_frames(eacham_graph* graph, int n, const int32_t* frames, const uint8_t* valid, const uint8_t* has3d,
                            const int64_t* has3d_offsets);
int eacham_graph_query(eacham_graph* graph, const int32_t* excluded_frames, int n_excluded, uint32_t* best);

/* ---- multi-view tracks from the match graph ---------------------------------------------------
 * The stage between pairwise matches and eacham_triangulate_tracks / eacham_ba_solve: a NODE is a keypoint (global id
 * kp_offsets[f] + k), an EDGE a match (q of f1, t of f2) of a pair whose `keep` byte is non-zero (keep == NULL: every match),
 * a TRACK a connected component with at least min_len (>= 2) nodes. The reference forms a star around one frame's keypoints
 * with hash maps, frame by frame (Triangulator.cpp:202-241); this is the whole graph at once, as an exact integer answer that
 * does not depend on the order anything runs in: a component is labelled by its smallest node id, tracks come out ordered by
 * that label, the observations of a track by ascending node id (frame-major, then keypoint).
 *   pairs .. kp_offsets   the arguments of eacham_graph_create: pairs in either orientation, duplicate edges and pairs with
 *                         counts[p] == 0 are legal, so are frames without keypoints; offsets has npairs entries, starts at 0
 *                         and does not decrease
 *   keep                  optional, one byte per match, indexed like q and t (e.g. the inlier masks of eacham_lmeds_batch)
 *   conflict_policy       a track that holds two keypoints of ONE frame is a conflict: 0 = keep it, bit 0 of its track_flags
 *                         set; 1 = drop such tracks whole
 * Outputs: *n_tracks, *n_obs; track_ptr (n_tracks + 1 CSR offsets, cap_tracks + 1 entries of room), obs_frame / obs_kp
 * (cap_obs entries of room; obs_frame is what eacham_triangulate_tracks takes), track_flags (cap_tracks), node_track (optional,
 * kp_offsets[n_frames] entries: the track of every keypoint, -1 = none).
 * EACHAM_ERR_INVALID (checked on the host before anything is launched or written; the message names the problem): a null
 * required pointer, a negative size, offsets / kp_offsets that do not start at 0 or that decrease, a negative count, a frame id
 * out of range, q or t beyond the frame's keypoint count, min_len < 2, an unknown policy.
 * EACHAM_ERR_CAPACITY: more than 2^31 - 1 nodes or matches in one call (the totals are then left as they were), more than 2^30
 * nodes that a match can touch (min(nodes, 2 x matches): the sort's limit), or n_obs > cap_obs or n_tracks > cap_tracks — then
 * *n_tracks and *n_obs hold what is needed and nothing else has been written. n_obs <= min(nodes, 2 x matches) and
 * n_tracks <= n_obs / 2 always suffice.
 * EACHAM_ERR_HIP with a message if the components have not settled within the round cap (see eacham_tracks_debug_last). */
int eacham_tracks_build(eacham_ctx* ctx, int n_frames, const int32_t* pairs, int npairs, const int32_t* counts,
                        const int64_t* offsets, const uint32_t* q, const uint32_t* t, const int64_t* kp_offsets,
                        const uint8_t* keep, int min_len, int conflict_policy, int64_t cap_obs, int32_t cap_tracks,
                        int32_t* n_tracks, int64_t* n_obs, int64_t* track_ptr, uint32_t* obs_frame, uint32_t* obs_kp,
                        uint8_t* track_flags, int32_t* node_track);
/* The same kernels on the arrays a resident graph already holds: only `keep` (optional; indexed like the q and t that
 * eacham_graph_create was given) is uploaded. Same result as eacham_tracks_build, byte for byte; leaves no state in the graph. */
int eacham_graph_tracks(eacham_graph* graph, const uint8_t* keep, int min_len, int conflict_policy, int64_t cap_obs,
                        int32_t cap_tracks, int32_t* n_tracks, int64_t* n_obs, int64_t* track_ptr, uint32_t* obs_frame,
                        uint32_t* obs_kp, uint8_t* track_flags, int32_t* node_track);
/* ---- geometric verification of a resident match graph ----------------------------------------------------------
 * eacham_lmeds_batch for every pair of a graph made by eacham_graph_create, without the graph's matches leaving the device:
 * the correspondences are gathered, the minimal samples drawn and the LMedS kernels run where the graph lives; the inlier mask
 * comes out in the layout eacham_graph_tracks takes as `keep`, and can stay on the device for it.
 *
 * eacham_graph_set_keypoints: xy holds kp_offsets[n_frames] rows of 2 doubles (pixels), frame-major in the kp_offsets layout the
 * graph was created with. Uploaded once into memory the graph owns (eacham_graph_destroy frees it). A second call replaces the
 * coordinates and drops a retained mask. EACHAM_ERR_INVALID: a null xy while the graph has keypoints. */
int eacham_graph_set_keypoints(eacham_graph* graph, const double* xy);
/* eacham_graph_verify: PROBLEM p is caller pair p of eacham_graph_create (every per-pair output has npairs entries), its points
 * the pair's matches in the caller's order: a[i] = xy[kp_offsets[f1] + q[i]], b[i] = xy[kp_offsets[f2] + t[i]].
 *   kind         EACHAM_SOLVE_HOMOGRAPHY4 | EACHAM_SOLVE_ESSENTIAL5 | EACHAM_SOLVE_FUNDAMENTAL7; K as in eacham_lmeds_batch (4 doubles
 *                on the host, NULL = already normalised; read by the essential kind only)
 *   sampling     EACHAM_SAMPLING_OPENCV: per pair cv::RNG((uint64)-1), getSubset with at most 1000 attempts per subset and, for
 *                the homography and the fundamental matrix, their checkSubset on the pair's points as floats
 *                (cv_check_subset_homography / cv_check_subset_fundamental); a pair stops where getSubset gives up.
 *                EACHAM_SAMPLING_COUNTER: the counter-based stream, seeded per pair by seeds[p] (seeds == NULL: 12345 for every
 *                pair; the OpenCV stream does not read seeds). Both are the functions of include/eacham/CvSampling.hpp that the
 *                host's lmeds_samples / draw_samples call, compiled for the device.
 *   iterations   the samples LMedS asks for per pair, computed once by the caller as lmeds() does:
 *                min(maxIters, max(ransac_update_num_iters(confidence, 0.45, m, maxIters), 3))
 *   retain       != 0: this call's mask stays in the graph (replacing an earlier one) for eacham_graph_tracks_verified
 * Outputs (each optional): models .. n_candidates as eacham_lmeds_batch returns them, per caller pair; masks: n_src bytes (n_src =
 * max over pairs of offsets[p] + counts[p]) in the index space of the q / t given to eacham_graph_create — match i of pair p at
 * offsets[p] + i, bytes that belong to no pair zero: exactly the `keep` of eacham_graph_tracks; n_samples: the samples each pair
 * used; samples: npairs x iterations x m int32 at a fixed stride, slots behind a pair's n_samples = -1.
 * A pair with counts[p] == 0, with fewer than m matches or with no samples gets the "none" record of eacham_lmeds_batch.
 * Byte for byte the host composition: gather, lmeds_samples / draw_samples per pair, eacham_lmeds_batch. The match lists of
 * different pairs must not overlap in the caller's arrays.
 * EACHAM_ERR_INVALID (before anything is launched or written): keypoints not set, unknown kind or sampling, negative iterations.
 * EACHAM_ERR_CAPACITY: more than (2^31 - 1) / 2 matches, npairs x iterations x m or the candidates beyond 2^31 - 1.
 * Scratch during a call: 33 bytes per match, iterations x m x 4 bytes per pair twice over, and what eacham_lmeds_batch needs
 * for its samples; retained: one byte per n_src. */
#define EACHAM_SAMPLING_OPENCV 0
#define EACHAM_SAMPLING_COUNTER 1
int eacham_graph_verify(eacham_graph* graph, int kind, const double* K, int sampling, int iterations, const uint64_t* seeds, int retain,
                        double* models, float* medians, float* thresholds, int32_t* inliers, uint8_t* masks, int32_t* winner,
                        int32_t* n_candidates, int32_t* n_samples, int32_t* samples);
/* eacham_graph_verify_ransac: the same gather, the same draws and the same mask layout, with eacham_ransac_batch as the estimator.
 * kind, K, sampling, seeds, retain, masks, n_samples and samples are eacham_graph_verify's; iterations = the samples drawn per pair
 * (the caller's maxIters: the threshold rule stops early by itself); threshold (squared), confidence and stage1, and the outputs
 * models, inliers, winner, n_candidates and n_used, are eacham_ransac_batch's, per caller pair. The budget rows are built on the host
 * from the pairs' match counts. A retained mask replaces an LMedS one and the other way round; eacham_graph_tracks_verified takes
 * either. Byte for byte the host composition: gather, lmeds_samples / draw_samples per pair, eacham_ransac_batch.
 * EACHAM_ERR_INVALID: as eacham_graph_verify, and a NaN or negative threshold, a confidence outside (0, 1), a negative stage1. */
int eacham_graph_verify_ransac(eacham_graph* graph, int kind, const double* K, int sampling, int iterations, const uint64_t* seeds, int retain,
                               float threshold, double confidence, int stage1, double* models, int32_t* inliers, uint8_t* masks,
                               int32_t* winner, int32_t* n_candidates, int32_t* n_used, int32_t* n_samples, int32_t* samples);
/* eacham_graph_tracks with the mask the last eacham_graph_verify(retain != 0) left in the graph as `keep`: nothing is uploaded.
 * Byte for byte eacham_graph_tracks(graph, masks of that verify call, ...). EACHAM_ERR_INVALID if no mask is retained. */
int eacham_graph_tracks_verified(eacham_graph* graph, int min_len, int conflict_policy, int64_t cap_obs, int32_t cap_tracks,
                                 int32_t* n_tracks, int64_t* n_obs, int64_t* track_ptr, uint32_t* obs_frame, uint32_t* obs_kp,
                                 uint8_t* track_flags, int32_t* node_track);
/* ---- guided matching: verified pairs matched again under their two-view model --------------------------------------
 * The step behind a verification (COLMAP's guided_matching, OpenCV's masked knnMatch): for every pair, match again with
 * only the candidates admitted that agree with the pair's model. Descriptors are the context's resident int8 frames.
 *
 * ADMISSIBLE CANDIDATES. Pair p = (f1, f2) has the model M_p (9 doubles, row-major) of kind EACHAM_SCORE_ESSENTIAL |
 * EACHAM_SCORE_HOMOGRAPHY | EACHAM_SCORE_FUNDAMENTAL. The candidate (row q of f1, row t of f2) is admissible iff
 *     err(q, t) <= max_error
 * where err is the float eacham_score_hypotheses gives the correspondence a = xy1[q], b = xy2[t] under M_p, bit for bit. K:
 * 4 doubles or NULL for the essential kind (as there), ignored otherwise. max_error is in the error's own unit, as
 * eacham_ransac_batch's threshold: squared pixels for H and F. +inf is legal and admits everything whose error is a number; a
 * NaN error is never admissible. The admissible set is ONE bipartite mask per pair and serves both directions: for H it is the
 * forward transfer error of M_p as given (f1 -> f2), also when f2's rows are the queries.
 * A pair whose model is all zeros (the estimators' "none" record) has no admissible candidate, by rule.
 *
 * DIRECTED MATCH q -> t. Among the admissible t of q, the two nearest by exact squared L2 of the descriptors, ties to the
 * lower train index:
 *     no admissible candidate   no match
 *     exactly one               matched (the runner-up counts as +inf)
 *     two or more               eacham_match_pair's predicate: (float)(d0 / d1) < ratio, d = sqrtf(d2), the quotient promoted
 *                               to double; 0 / 0 is NaN and rejected
 * and in every case, if max_d2 > 0, d2(q, t0) <= max_d2 (max_d2 == 0: no bound). t -> q is the same on the transposed mask.
 * FEWER THAN 2 TRAIN ROWS are legal here: a lone admissible row matches — unlike eacham_match_pair, whose result is empty
 * then (the reference would read its second neighbour out of bounds); here the runner-up is defined.
 *
 * CROSS-CHECK. cross_check == 0: the result is m12. cross_check != 0: {(q, t) in m12 : m21[t] == q}, and ratio must be in
 * (0, 1] as for eacham_match_all_pairs. There are no min_dir / min_mutual thresholds: the caller filters.
 *
 * eacham_match_guided: kp_offsets / xy in the layout of eacham_graph_create / eacham_graph_set_keypoints (kp_offsets[f] = the
 * first row of frame f in xy, rows of 2 doubles; read for the frames the pairs name). A frame's keypoint count must equal its
 * resident row count. Output: CSR over the caller's pairs, sorted by q — exactly the counts / offsets (npairs + 1) / q / t that
 * eacham_graph_create and eacham_tracks_build take; out_d2 (optional) the uint32 squared distances; stats (optional) npairs x
 * {|m12|, |m21|, |result|} (|m21| = 0 without the cross-check: that direction is not computed).
 * eacham_graph_match_guided: pairs and keypoints are those the graph holds (eacham_graph_set_keypoints), models has npairs x 9
 * entries as eacham_graph_verify[_ransac] wrote them. Byte for byte the list form's result; leaves no state in the graph.
 *
 * All checks run on the host before anything is launched or written.
 * EACHAM_ERR_INVALID: a null required pointer, an unknown kind, a negative size, a NaN or negative max_error, a NaN ratio, a
 * ratio outside (0, 1] with cross_check, a frame that is not resident, a keypoint count other than the frame's rows (the
 * message names the frame), keypoints not set (graph form).
 * EACHAM_ERR_UNSUPPORTED: the resident frames are not int8 frames (fp32, binary and wide binary frames are out of scope).
 * EACHAM_ERR_CAPACITY: more than cap matches; *out_total holds what is needed and nothing else has been written.
 * There is no device-pointer form and no sharded form. */
int eacham_match_guided(eacham_ctx* ctx, int kind, const int32_t* pairs, int npairs, const double* models, const double* K,
                        const int64_t* kp_offsets, const double* xy, float max_error, double ratio, uint32_t max_d2,
                        int cross_check, int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t, uint32_t* out_d2,
                        int64_t cap, int64_t* out_total, int32_t* stats);
int eacham_graph_match_guided(eacham_graph* graph, int kind, const double* models, const double* K, float max_error, double ratio,
                              uint32_t max_d2, int cross_check, int32_t* counts, int64_t* offsets, uint32_t* out_q,
                              uint32_t* out_t, uint32_t* out_d2, int64_t cap, int64_t* out_total, int32_t* stats);

/* Diagnostic: how the context's last track-building call ran (any pointer may be NULL). rounds = hook-and-compress rounds until
 * one changed nothing (that one included; 0 if the call had no kept edge), round_cap = the bound it is held to,
 * 2 * ceil(log2(touched-node bound)) + 1 with the bound min(nodes, 2 x matches), readbacks = device-to-host read-backs of status words (one per batch of rounds, one
 * for the totals), kernel_ms = device time from the first kernel to the last by HIP events if eacham_profile_enable is on, else -1. */
int eacham_tracks_debug_last(eacham_ctx* ctx, int32_t* rounds, int32_t* round_cap, int32_t* readbacks, float* kernel_ms);

/* ---- kernel timing (HIP events on the context stream; used for roofline reporting) ---------- */

#define EACHAM_KERNEL_MATCH_TILE 0     /* all-pairs int8 MFMA distance + fused row/col top-2      */
#define EACHAM_KERNEL_MATCH_FINALIZE 1 /* partial merge + ratio + mutual check + compaction       */
#define EACHAM_KERNEL_BA_LINEARIZE 2
#define EACHAM_KERNEL_BA_SCHUR 3
#define EACHAM_KERNEL_BA_SOLVE 4
#define EACHAM_KERNEL_BA_ERROR 5
#define EACHAM_KERNEL_TRIANGULATE 6     /* pair DLT + scoring and the per-track selection          */
#define EACHAM_KERNEL_SCORE 7           /* hypothesis scoring (errors, inlier counts, medians)      */
#define EACHAM_KERNEL_MATCH_GUIDED 8   /* guided matching: gated sweep + tail (eacham_match_guided)       */
#define EACHAM_KERNEL_COUNT 9

/* Enables (1) / disables (0) per-launch HIP-event timing of the kernels above. */
int eacham_profile_enable(eacham_ctx* ctx, int on);
int eacham_profile_reset(eacham_ctx* ctx);
/* Synchronises, then returns launches and total milliseconds recorded for `kernel_id`. */
int eacham_profile_get(eacham_ctx* ctx, int kernel_id, int64_t* launches, double* total_ms);

/* ---- multi-GPU sharding of the pair loop (host-side helpers, no device needed) ---------------------
 * One process per GPU, one context each: every rank orders the pair list the same
 * way, takes its contiguous shard, runs eacham_match_all_pairs(_dev) on it and all-gathers counts + edges with
 * RCCL (bench.py / eacham_amd/shard.py show the torch.distributed form; the single-process form is
 * eacham_match_all_pairs_sharded below).
 * Replaces the std::for_each(par_unseq) over pairs of apps/sfm/main.cpp:98-109 across devices. */
/* Sorts [npairs][2] in place by train frame (second column), then query frame: consecutive workgroups stream
 * the same train frame, which keeps it in the XCD's L2. */
int eacham_order_pairs(int32_t* pairs, int npairs);
/* Contiguous shard of rank `rank` of `world`: [*begin, *end), sizes differ by at most one. */
int eacham_shard_bounds(int npairs, int world, int rank, int* begin, int* end);
/* Work-balanced contiguous cut of the ordered list: bounds[r] = first pair of shard r, bounds[world] = npairs. weights[k] =
 * cost of ordered pair k — the matcher's is the pair's distance matrix, rows(f1) * rows(f2), which is what makes shards of
 * ragged frames take equal time (equal pair COUNTS do not: apps/sfm/main.cpp:98-109 hands every pair to whichever thread is
 * free, a static cut has to weigh them). Shard r starts at the smallest k whose prefix weight P[k] satisfies
 * P[k] * world >= r * P[npairs]. weights == NULL (or all zero): the equal-count cut of eacham_shard_bounds. */
int eacham_shard_bounds_weighted(int npairs, int world, const int64_t* weights, int32_t* bounds);

/* ---- single-process multi-GPU form of the pair loop -----------------------
 * The reference app is ONE C++ process (apps/sfm/main.cpp:31) whose pair loop (:84-147) fans out over host threads
 * (:98-109). A communicator owns one context and one host thread per device and an RCCL communicator over them
 * (ncclCommInitAll; RCCL is loaded at run time, EACHAM_ERR_UNSUPPORTED if it cannot be): descriptors are replicated on
 * every device, the pair list is ordered by train frame and cut into contiguous shards (eacham_order_pairs /
 * eacham_shard_bounds), every device matches its shard, and the match graph is assembled on every device by
 * ncclAllGather of the per-pair counts and of the edge lists (padded to the largest shard) over xGMI, enqueued on each
 * context's stream behind its matching. devices = NULL means devices 0 .. ndev-1. */
typedef struct eacham_comm eacham_comm;
int eacham_comm_init(int ndev, const int* devices, eacham_comm** out_comm);
void eacham_comm_destroy(eacham_comm* comm);
const char* eacham_comm_last_error(const eacham_comm* comm);
int eacham_comm_size(const eacham_comm* comm);
/* The context of rank `rank` (owned by the communicator): for uploads of other kinds, profiling, BA replicas. */
eacham_ctx* eacham_comm_ctx(eacham_comm* comm, int rank);
/* eacham_upload_descriptors on every device of the communicator. */
int eacham_comm_upload_descriptors(eacham_comm* comm, int frame_id, const float* rowmajor, int n, int dim);
/* eacham_match_all_pairs over all devices: same arguments, same result (CSR over the caller's pair order, sorted by q). */
int eacham_match_all_pairs_sharded(eacham_comm* comm, const int32_t* pairs, int npairs, double ratio,
                                   int min_dir, int min_mutual, int32_t* counts, int64_t* offsets,
                                   uint32_t* out_q, uint32_t* out_t, int64_t cap, int64_t* out_total);
/* The two halves of eacham_match_all_pairs_sharded. run: order the pairs, cut them into shards (balance != 0: by work,
 * eacham_shard_bounds_weighted with rows(f1) * rows(f2); 0: by count), match every shard on its device and all-gather; the
 * gathered graph stays resident on EVERY device, *out_total = matches in it. fetch: read device 0's copy back and assemble
 * the CSR in the caller's pair order (any number of times until the next run). */
int eacham_comm_match_run(eacham_comm* comm, const int32_t* pairs, int npairs, double ratio, int min_dir, int min_mutual,
                          int balance, int64_t* out_total);
int eacham_comm_match_fetch(eacham_comm* comm, int32_t* counts, int64_t* offsets, uint32_t* out_q, uint32_t* out_t,
                            int64_t cap, int64_t* out_total);
/* Host logic of the gather's send buffers (no device needed; exported for the CPU tests): ncclAllGather sends the same
 * number of elements from every rank, so the edge region of EVERY rank's buffer holds the largest shard bound. */
int eacham_comm_edge_region(int world, const int64_t* shard_bound, int64_t* region);
/* Host-side assembly of gathered shards (what eacham_match_all_pairs_sharded does after its all-gather; also for callers
 * that run one process per GPU and gather with their own collective): g_counts = world x shard_cap per-pair counts,
 * g_edges = world x edge_cap x {q, t}; shard r holds pairs [eacham_shard_bounds(npairs, world, r)) of the ORDERED list,
 * sorted_index[k] = position of ordered pair k in the caller's list (NULL = identity). */
int eacham_assemble_match_graph(const int32_t* g_counts, const uint32_t* g_edges, int npairs, int world, int shard_cap,
                                int64_t edge_cap, const int32_t* sorted_index, int32_t* counts, int64_t* offsets,
                                uint32_t* out_q, uint32_t* out_t, int64_t cap, int64_t* out_total);

/* Same with explicit shard boundaries (bounds[world + 1] over the ordered list, as eacham_shard_bounds_weighted returns
 * them; NULL = the equal-count cut). */
int eacham_assemble_match_graph_bounds(const int32_t* g_counts, const uint32_t* g_edges, int npairs, int world, int shard_cap,
                                       int64_t edge_cap, const int32_t* bounds, const int32_t* sorted_index, int32_t* counts,
                                       int64_t* offsets, uint32_t* out_q, uint32_t* out_t, int64_t cap, int64_t* out_total);

#ifdef __cplusplus
}
#endif
#endif /* EACHAM_HIP_H */
