// ba_prepare.hip — eacham_ba_prepare: the bundle-adjustment problem that ba.hip's Levenberg-Marquardt solver runs on.
//
// Replaces the graph construction of   RefineBA   modules/sfm/reconstruction/BundleAdjuster.cpp:57-178.
// Two constructions of the same structure (BaDev, ba_dev.hpp), bit for bit alike: host loops for a local window, sorts and scans
// on the device (devprim.hpp) for the large problems; under both one skeleton: the arena pool of the context, an allocation
// sequence that runs twice over an arena (sizes, then pointers), the plan of the reduced system (ba_plan.hpp) and its upload.
// No kernel of an LM iteration lives here and none of these kernels runs inside one; the solver's work arrays are declared by
// ba.hip (ba_alloc_work_a / ba_alloc_work_b), called from the sequences below.
#include "ba_dev.hpp"
#include "devprim.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

using namespace eacham;

namespace eacham {

constexpr int PAIR_CHUNK = 256;    // pair-list entries summed by one wave of ba_schur_pairs (lane e takes entries e, e+64, ...)

static void pose_from_Twc(const double* T, double* x) {  // rigid inverse: camera->world
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) x[3 * i + j] = T[4 * j + i];
    for (int i = 0; i < 3; ++i) x[9 + i] = -(x[3 * i] * T[3] + x[3 * i + 1] * T[7] + x[3 * i + 2] * T[11]);
}

// An arena of at least `bytes` from the context's pool: the smallest free one that fits, else a new one (free arenas
// are dropped first once the pool holds eight: a long sequence of growing windows must not keep every size).
static int ba_block_acquire(eacham_ctx* ctx, size_t bytes, int* index) {
    int best = -1, n_free = 0;
    for (int i = 0; i < (int)ctx->ba_pool.size(); ++i) {
        const BaBlock& b = ctx->ba_pool[i];
        if (b.busy || !b.dev) continue;
        ++n_free;
        if (b.bytes >= bytes && (best < 0 || b.bytes < ctx->ba_pool[best].bytes)) best = i;
    }
    if (best < 0) {
        if ((int)ctx->ba_pool.size() >= 8 && n_free > 0) {
            for (BaBlock& b : ctx->ba_pool)
                if (!b.busy && b.dev) {
                    (void)hipFree(b.dev);
                    b.dev = nullptr;
                    b.bytes = 0;
                }
        }
        for (int i = 0; i < (int)ctx->ba_pool.size() && best < 0; ++i)
            if (!ctx->ba_pool[i].busy && !ctx->ba_pool[i].dev) best = i;  // an emptied slot (its pinned block is kept)
        if (best < 0) {
            ctx->ba_pool.emplace_back();
            best = (int)ctx->ba_pool.size() - 1;
        }
        BaBlock& b = ctx->ba_pool[best];
        const size_t want = bytes + bytes / 8;  // some headroom: the next window is rarely the same size
        EACHAM_HIP_TRY(ctx, hipMalloc(&b.dev, want));
        b.bytes = want;
        if (!b.pinned) {
            hipError_t e = hipHostMalloc((void**)&b.pinned, SCAL * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
            if (e != hipSuccess) {
                (void)hipFree(b.dev);
                b.dev = nullptr;
                b.bytes = 0;
                return ctx->fail(EACHAM_ERR_HIP, "hipHostMalloc failed: %s", hipGetErrorString(e));
            }
        }
    }
    ctx->ba_pool[best].busy = true;
    *index = best;
    return EACHAM_OK;
}

// The allocation sequence of a problem's device arrays, in three parts (each runs twice: sizes first, then pointers):
// the plan's tables (uploads), the work arrays sized by (nc, nl, no), and those sized by the pair lists and the plan.
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
static int ba_upload_plan(eacham_ctx* ctx, eacham_ba_handle* h, const BaPlan& plan, const std::vector<int2>& bs_ent) {
    BaDev& D = h->D;
    TRY(dev_upload(ctx, h, &D.sp_pos, plan.pos));
    TRY(dev_upload(ctx, h, &D.sp_tile_map, plan.tile_map));
    TRY(dev_upload(ctx, h, &D.sp_pad_cols, plan.pad_cols));
    TRY(dev_upload(ctx, h, &D.sp_diag_tile, plan.diag_tile));
    TRY(dev_upload(ctx, h, &h->sp_leaves, plan.leaves));
    TRY(dev_upload(ctx, h, &h->sp_items, plan.items));
    TRY(dev_upload(ctx, h, &h->sp_srcs, plan.srcs));
    TRY(dev_upload(ctx, h, &h->bs_order, plan.bs_order));
    TRY(dev_upload(ctx, h, &h->bs_ptr, plan.bs_ptr));
    TRY(dev_upload(ctx, h, &h->bs_ent, bs_ent));
    TRY(dev_upload(ctx, h, &h->sp_col_dest, plan.col_dest));
    return EACHAM_OK;
}
static int ba_upload_groups(eacham_ctx* ctx, eacham_ba_handle* h, const BaGroups& GR) {
    BaDev& D = h->D;
    D.g_rows = GR.rows; D.g_ngroups = (int)GR.groups.size(); D.g_nblk = GR.n_blk; D.g_nparts = GR.n_parts;
    D.g_nchunks = GR.n_chunks; D.g_nlong = (int)GR.longblk.size(); D.g_nent4 = GR.n_ent4;
    if (GR.rows == 0) return EACHAM_OK;
    TRY(dev_upload(ctx, h, &D.g_groups, GR.groups));
    TRY(dev_upload(ctx, h, &D.g_lmid, GR.lmid));
    TRY(dev_upload(ctx, h, &D.g_lmrow, GR.lmrow));
    TRY(dev_upload_as(ctx, h, &D.g_rowinfo, GR.rowinfo));
    TRY(dev_upload(ctx, h, &D.g_uv, GR.uv));
    TRY(dev_upload(ctx, h, &D.g_chunks, GR.chunks));
    TRY(dev_upload(ctx, h, &D.g_ent, GR.ent));
    TRY(dev_upload(ctx, h, &D.g_laneinfo, GR.laneinfo));
    TRY(dev_upload_as(ctx, h, &D.g_blk, GR.blk));
    TRY(dev_upload(ctx, h, &D.g_longblk, GR.longblk));
    return EACHAM_OK;
}

// ---- what the two constructions of the structure (host loops below, sorts and scans on the device further down) share ----

// Limits of the 32-bit indices. The camera blocks (c <= c') of the pair lists are numbered in an int; the device form also forms
// `nblk + TPB` for its grids and a thread's block number `blockIdx.x * TPB + threadIdx.x` in an int, hence its smaller bound (half
// the range: far more headroom than those sums need, kept as it was). The pair entries are indexed by int in both forms.
static constexpr long long BA_MAX_CAM_BLOCKS_HOST = 0x7fffffffLL;
static constexpr long long BA_MAX_CAM_BLOCKS_DEVICE = 0x3fffffffLL;
static constexpr long long BA_MAX_PAIR_ENTRIES = 0x7fffffffLL;

static double us_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }

// Gives a handle's arenas (and their pinned scalars) back to the context's pool and deletes it. The caller has drained what may
// still use them.
static void ba_handle_free(eacham_ctx* ctx, eacham_ba_handle* h) {
    if (h->block >= 0) ctx->ba_pool[h->block].busy = false;
    if (h->block2 >= 0) ctx->ba_pool[h->block2].busy = false;
    delete h;
}

// Owns the handle while eacham_ba_prepare builds it; release() hands it to the caller. Leaving with an error instead joins the
// plan thread of the device form, drains the context's two streams (copies out of the caller's arrays or out of host vectors of
// the construction may still be in flight), returns the arenas to the pool and deletes the handle. The success path pays none of it.
struct BaPrepareGuard {
    eacham_ctx* ctx;
    eacham_ba_handle* h;
    std::thread plan_thread;
    BaPrepareGuard(eacham_ctx* c, eacham_ba_handle* handle) : ctx(c), h(handle) {}
    ~BaPrepareGuard() {
        if (plan_thread.joinable()) plan_thread.join();
        if (!h) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->stream2);
        ba_handle_free(ctx, h);
    }
    eacham_ba_handle* release() { return std::exchange(h, nullptr); }
};

// The dimensions and the launch shapes of the per-landmark kernels.
static void ba_handle_init(const eacham_ba_problem* P, eacham_ba_handle* h) {
    BaDev& D = h->D;
    const int nl = P->n_points;
    memset(&D, 0, sizeof(D));
    D.nc = P->n_cams; D.nl = nl; D.no = P->n_obs; D.n = 6 * P->n_cams + 5;
    D.nz = make_noise();
    D.n_lm_blocks = std::max(1, (nl + TPB - 1) / TPB);
    D.lpl = nl <= 8192 ? 8 : 2;  // (the two built variants. S200: 45.7 / 40.4 / 41.0 / 45.6 us for 1 / 2 / 4 / 8, docs/HISTORY.md)
    D.n_ll_blocks = std::max(1, (int)(((long long)nl * D.lpl + TPB - 1) / TPB));
    D.lpl_step = nl <= 8192 ? 8 : 2;
    D.n_step_blocks = std::max(1, (int)(((long long)nl * D.lpl_step + TPB - 1) / TPB));
}

// The elimination ordering asked for: the problem's, or the context's (EACHAM_BA_ORDERING) where the problem leaves it open.
static int ba_ordering_hint(eacham_ctx* ctx, const eacham_ba_problem* P, int* hint) {
    *hint = P->ordering;
    if (*hint == EACHAM_BA_ORDER_AUTO && ctx->ba_ordering != EACHAM_BA_ORDER_AUTO) *hint = ctx->ba_ordering;
    if (*hint < EACHAM_BA_ORDER_AUTO || *hint > EACHAM_BA_ORDER_ND) return ctx->fail(EACHAM_ERR_INVALID, "unknown BA ordering %d", *hint);
    return EACHAM_OK;
}

// Whether a context WANTS the landmark groups as the form of the Schur stage from a construction form. Host: only when
// EACHAM_BA_SCHUR=groups. Device: unless =pairs. Whether the groups are feasible for the problem is decided where its
// data is; the pair lists serve when they are not wanted or not feasible.
static bool ba_groups_wanted(const eacham_ctx* ctx, bool device) {
    return device ? ctx->ba_schur_mode != 2 : ctx->ba_schur_mode == 1;
}

// The plan's scalars -> BaDev; its (column, source) pairs in the layout the kernels read (the tables go up with ba_upload_plan).
static std::vector<int2> ba_plan_to_dev(eacham_ba_handle* h) {
    const BaPlan& plan = h->plan;
    BaDev& D = h->D;
    D.sp_npan = plan.npan; D.sp_ntiles = plan.ntiles; D.sp_posK = plan.posK; D.sp_rhs_row = plan.rhs_row;
    D.sp_n_pad = (int)plan.pad_cols.size();
    std::vector<int2> bs_ent(plan.bs_ent.size());
    for (size_t e = 0; e < bs_ent.size(); ++e) bs_ent[e] = make_int2(plan.bs_ent[e].first, plan.bs_ent[e].second);
    return bs_ent;
}

// Every device array of a problem is carved out of an arena of the context's pool: `layout`, an allocation sequence of
// dev_alloc / dev_upload calls, runs twice, first to add up the sizes, then, with an arena of that size in pool slot `*slot`,
// to hand out the pointers and issue the uploads. `staged` is asked between the passes which byte range [lo, hi) of the arena's
// uploads is to be sent as ONE copy of a host image (h->stage, which lives as long as the handle) instead of one copy per array;
// lo == hi: none. An arena that served another problem holds its bytes: nothing may rely on fresh memory being zero (S is cleared
// by every tryLambda, Lm and the flags by ba_alloc_work_b).
template <class Layout, class Staged>
static int ba_arena_layout(eacham_ctx* ctx, eacham_ba_handle* h, int* slot, Layout layout, Staged staged) {
    h->arena = Bump(nullptr);
    TRY(layout());
    TRY(ba_block_acquire(ctx, h->arena.off, slot));
    h->arena = Bump(ctx->ba_pool[*slot].dev);
    const std::pair<size_t, size_t> image = staged();
    h->stage_base = image.first;
    h->stage.assign(image.second - image.first, 0);
    int rc = layout();
    if (!rc && !h->stage.empty() && hipMemcpyAsync(h->arena.base + h->stage_base, h->stage.data(), h->stage.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = ctx->fail(EACHAM_ERR_HIP, "BA upload failed");
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (uploads out of the caller's host vectors may be in flight: those die before the guard acts)
    return rc;
}

// The structure built by host loops (the round-1..3 form): what a local window of a few thousand observations still uses —
// a dozen dependent launches and three read-backs cost more than these loops on a problem that small — and the reference
// the device-built structure is held against bit for bit (EACHAM_BA_PREPARE=host|device forces either form).
static int ba_prepare_host(eacham_ctx* ctx, const eacham_ba_problem* P, int hint, eacham_ba_handle** out) {
    const int nc = P->n_cams, nl = P->n_points, no = P->n_obs;
    for (int o = 0; o < no; ++o)
        if (P->obs_cam[o] >= (uint32_t)nc || P->obs_point[o] >= (uint32_t)nl)
            return ctx->fail(EACHAM_ERR_INVALID, "observation %d references a camera/point out of range", o);
    eacham_ba_handle* h = new eacham_ba_handle();
    BaPrepareGuard guard(ctx, h);
    const auto t_begin = std::chrono::steady_clock::now();
    BaDev& D = h->D;
    ba_handle_init(P, h);

    // ---- structure: observations grouped by landmark (stable), then by camera ----
    std::vector<int> lm_ptr(nl + 1, 0);
    for (int o = 0; o < no; ++o) lm_ptr[P->obs_point[o] + 1]++;
    for (int j = 0; j < nl; ++j) {
        if (lm_ptr[j + 1] > 0) h->n_landmarks_used++;
        lm_ptr[j + 1] += lm_ptr[j];
    }
    std::vector<int> fill(lm_ptr.begin(), lm_ptr.end() - 1);
    h->lm_order.resize(no);
    for (int o = 0; o < no; ++o) h->lm_order[fill[P->obs_point[o]]++] = o;
    std::vector<unsigned> obs_cam(no), obs_lm(no);
    std::vector<double> obs_uv(2 * (size_t)no);
    for (int p = 0; p < no; ++p) {
        const int o = h->lm_order[p];
        obs_cam[p] = P->obs_cam[o];
        obs_lm[p] = P->obs_point[o];
        obs_uv[2 * (size_t)p] = P->obs_uv[2 * (size_t)o];
        obs_uv[2 * (size_t)p + 1] = P->obs_uv[2 * (size_t)o + 1];
    }
    std::vector<int> cam_ptr(nc + 1, 0), cam_obs(no);
    for (int p = 0; p < no; ++p) cam_ptr[obs_cam[p] + 1]++;
    for (int c = 0; c < nc; ++c) cam_ptr[c + 1] += cam_ptr[c];
    {
        std::vector<int> f2(cam_ptr.begin(), cam_ptr.end() - 1);
        for (int p = 0; p < no; ++p) cam_obs[f2[obs_cam[p]]++] = p;
    }
    std::vector<int> obs_pos(no), pos_cam(no);
    for (int p = 0; p < no; ++p) obs_pos[cam_obs[p]] = p, pos_cam[p] = (int)obs_cam[cam_obs[p]];
    std::vector<int2> cam_chunks;
    std::vector<int> cam_chunk_ptr(nc + 1, 0);
    for (int c = 0; c < nc; ++c) {
        for (int q = cam_ptr[c]; q < cam_ptr[c + 1]; q += TPB) cam_chunks.push_back(make_int2(q, std::min(TPB, cam_ptr[c + 1] - q)));
        cam_chunk_ptr[c + 1] = (int)cam_chunks.size();
    }
    D.n_cam_chunks = (int)cam_chunks.size();
    std::vector<int> cam_lm(no);
    std::vector<double> cam_uv(2 * (size_t)no);
    for (int p = 0; p < no; ++p) {
        cam_lm[p] = (int)obs_lm[cam_obs[p]];
        cam_uv[2 * (size_t)p] = obs_uv[2 * (size_t)cam_obs[p]];
        cam_uv[2 * (size_t)p + 1] = obs_uv[2 * (size_t)cam_obs[p] + 1];
    }
    // ---- the landmark-major structure of the Schur stage (ba_groups.hpp); the pair lists below only when it does not apply ----
    BaGroups& GR = h->groups;
    const bool use_groups = ba_groups_wanted(ctx, false) && build_groups(nc, nl, lm_ptr.data(), obs_cam.data(), obs_uv.data(), GR, ctx->ba_group_rows);
    if (!use_groups) GR = BaGroups();
    // ---- camera-pair lists of the Schur complement: block (c <= c') -> (o, o') pairs, landmark order ----
    // (two passes over every observation pair of every landmark — count, then fill: this loop is most of the host time of
    // preparing a local window, hence the flat 32-bit index arithmetic; entries are written as Et positions directly)
    const bool use_pairs = !use_groups;
    const long long nblk_all = use_pairs ? (long long)nc * (nc + 1) / 2 : 0;
    if (nblk_all > BA_MAX_CAM_BLOCKS_HOST) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "too many cameras (%d) for the camera-block index", nc);
    std::vector<int> rowoff(std::max(nc, 1));  // block (c, c2 >= c) has index rowoff[c] + c2
    for (int c = 0; c < nc; ++c) rowoff[c] = (int)((long long)c * nc - (long long)c * (c - 1) / 2 - c);
    auto bid = [&](int c, int c2) { return rowoff[c] + c2; };
    std::vector<int> bcount((size_t)nblk_all + 1, 0);
    if (use_pairs) {
        const unsigned* oc = obs_cam.data();
        int* bc = bcount.data() + 1;
        for (int j = 0; j < nl; ++j) {
            const int a0 = lm_ptr[j], a1 = lm_ptr[j + 1];
            for (int a = a0; a < a1; ++a) {
                const int ca = (int)oc[a];
                bc[rowoff[ca] + ca] += 1;  // (a, a)
                for (int b = a + 1; b < a1; ++b) {
                    const int cb = (int)oc[b];
                    if (ca < cb) bc[rowoff[ca] + cb] += 1;
                    else if (ca > cb) bc[rowoff[cb] + ca] += 1;
                    else bc[rowoff[ca] + ca] += 2;
                }
            }
        }
    }
    std::vector<long long> bstart((size_t)nblk_all + 1, 0);
    for (long long b = 0; b < nblk_all; ++b) bstart[b + 1] = bstart[b] + bcount[b + 1];
    const long long n_entries = bstart[nblk_all];
    if (n_entries > BA_MAX_PAIR_ENTRIES) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "Schur pair list too large (%lld entries)", n_entries);
    std::vector<int2> entries((size_t)n_entries);
    if (use_pairs) {
        std::vector<int> pos((size_t)nblk_all);
        for (long long b = 0; b < nblk_all; ++b) pos[b] = (int)bstart[b];
        const unsigned* oc = obs_cam.data();
        const int* op = obs_pos.data();  // Et records live in camera order
        int2* en = entries.data();
        int* ps = pos.data();
        for (int j = 0; j < nl; ++j) {
            const int a0 = lm_ptr[j], a1 = lm_ptr[j + 1];
            for (int a = a0; a < a1; ++a) {
                const int ca = (int)oc[a], pa = op[a];
                en[ps[rowoff[ca] + ca]++] = make_int2(pa, pa);
                for (int b = a + 1; b < a1; ++b) {
                    const int cb = (int)oc[b], pb = op[b];
                    if (ca < cb) en[ps[rowoff[ca] + cb]++] = make_int2(pa, pb);
                    else if (ca > cb) en[ps[rowoff[cb] + ca]++] = make_int2(pb, pa);
                    else {
                        int& q = ps[rowoff[ca] + ca];
                        en[q++] = make_int2(pa, pb);
                        en[q++] = make_int2(pb, pa);
                    }
                }
            }
        }
    }
    std::vector<int4> chunks, blocks;
    for (int c = 0; c < (use_pairs ? nc : 0); ++c)
        for (int c2 = c; c2 < nc; ++c2) {
            const long long b = bid(c, c2);
            const long long cnt = bstart[b + 1] - bstart[b];
            if (cnt == 0 && c != c2) continue;  // absent off-diagonal block stays zero
            const int first_chunk = (int)chunks.size();
            int k = 0;
            for (long long s = 0; s < cnt; s += PAIR_CHUNK, ++k)
                chunks.push_back(make_int4((int)blocks.size(), (int)(bstart[b] + s), (int)std::min<long long>(PAIR_CHUNK, cnt - s), k));
            blocks.push_back(make_int4(c, c2, first_chunk, k));
        }
    D.n_chunks = (int)chunks.size();
    D.n_blocks = (int)blocks.size();
    // ---- the sparse solve: ordering, panels, symbolic factor, level schedule (ba_plan.hpp) ----
    const auto t_plan = std::chrono::steady_clock::now();
    h->prep_us[0] = us_since(t_begin);
    {
        std::vector<std::pair<int, int>> cam_edges;
        cam_edges.reserve(blocks.size() + GR.blk.size());
        for (const int4& b : blocks)
            if (b.x != b.y) cam_edges.emplace_back(b.x, b.y);
        for (const GrpI4& b : GR.blk)
            if (b.x != b.y && b.y < nc) cam_edges.emplace_back(b.x, b.y);
        try {
            build_ba_plan(nc, cam_edges, hint, h->plan);
        } catch (...) {  // (no exception crosses the C-ABI)
            return ctx->fail(EACHAM_ERR_HIP, "BA preparation: the analysis of the reduced system ran out of memory or threads");
        }
    }
    h->prep_us[1] = us_since(t_plan);
    const auto t_upload = std::chrono::steady_clock::now();
    const std::vector<int2> bs_ent = ba_plan_to_dev(h);

    // ---- values ----
    std::vector<double> pose(12 * (size_t)nc), lmprior(2 * (size_t)nl), K5(5);
    for (int c = 0; c < nc; ++c) pose_from_Twc(P->cam_T_wc + 16 * (size_t)c, &pose[12 * (size_t)c]);
    for (int j = 0; j < nl; ++j) {  // BundleAdjuster.cpp:109-113: sigma = 1.0f/obs, k = 3.0f/obs (float)
        const float o = (float)(P->point_observers[j] > 0 ? P->point_observers[j] : 1);
        lmprior[2 * (size_t)j] = (double)(1.0f / o);
        lmprior[2 * (size_t)j + 1] = (double)(3.0f / o);
    }
    K5[0] = P->K[0]; K5[1] = P->K[1]; K5[2] = 0.0; K5[3] = P->K[2]; K5[4] = P->K[3];
    std::vector<double> pts(P->points, P->points + 3 * (size_t)nl);
    std::vector<int> fixed(P->cam_fixed, P->cam_fixed + nc);

    auto layout = [&]() -> int {
        const double *c_pose0, *c_pt0, *c_K0, *c_lmprior, *c_uv;
        TRY(dev_upload(ctx, h, &c_pose0, pose));
        TRY(dev_upload(ctx, h, &c_pt0, pts));
        TRY(dev_upload(ctx, h, &c_K0, K5));
        TRY(dev_upload(ctx, h, &c_lmprior, lmprior));
        TRY(dev_upload(ctx, h, &c_uv, obs_uv));
        D.pose0 = (double*)c_pose0; D.pt0 = (double*)c_pt0; D.K0 = (double*)c_K0; D.lmprior = c_lmprior; D.obs_uv = c_uv;
        h->pose_init = D.pose0; h->pt_init = D.pt0; h->K_init = D.K0;
        TRY(dev_upload(ctx, h, &D.fixed, fixed));
        TRY(dev_upload(ctx, h, &D.lm_ptr, lm_ptr));
        TRY(dev_upload(ctx, h, &D.cam_ptr, cam_ptr));
        TRY(dev_upload(ctx, h, &D.cam_obs, cam_obs));
        TRY(dev_upload(ctx, h, &D.cam_lm, cam_lm));
        TRY(dev_upload(ctx, h, &D.cam_chunks, cam_chunks));
        TRY(dev_upload(ctx, h, &D.cam_chunk_ptr, cam_chunk_ptr));
        TRY(dev_upload(ctx, h, &D.obs_pos, obs_pos));
        TRY(dev_upload(ctx, h, &D.pos_cam, pos_cam));
        TRY(dev_upload(ctx, h, &D.cam_uv, cam_uv));
        TRY(dev_upload(ctx, h, &D.obs_cam, obs_cam));
        TRY(dev_upload(ctx, h, &D.obs_lm, obs_lm));
        TRY(dev_upload(ctx, h, &D.pair_entries, entries));
        TRY(dev_upload(ctx, h, &D.pair_chunks, chunks));
        TRY(dev_upload(ctx, h, &D.blocks, blocks));
        TRY(ba_upload_groups(ctx, h, GR));
        TRY(ba_upload_plan(ctx, h, h->plan, bs_ent));
        TRY(ba_alloc_work_a(ctx, h));
        TRY(ba_alloc_work_b(ctx, h));
        return EACHAM_OK;
    };
    // a local window uploads ~20 arrays of a few KB: one copy of their image instead of 20 (each is a staged,
    // synchronous-looking call from pageable memory); large problems keep the per-array copies (no second host copy)
    TRY(ba_arena_layout(ctx, h, &h->block, layout, [&] { return std::make_pair((size_t)0, h->upload_end <= ((size_t)4 << 20) ? h->upload_end : (size_t)0); }));
    // The per-array copies of a large problem read host vectors that die here: wait for them. A small problem was sent as
    // ONE image out of h->stage, which lives as long as the handle: nothing to wait for (the first kernel of the solve
    // queues behind the copy on the same stream) — 30-40 us of every local-window call.
    if (h->stage.empty()) EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h->prep_us[2] = us_since(t_upload);
    *out = guard.release();
    return EACHAM_OK;
}

// ======================================================================================================================
// Device-side construction of the problem structure (round 4). RefineBA's graph build is part of the reference's call
// (modules/sfm/reconstruction/BundleAdjuster.cpp:57-178); as host loops it took 11.6 ms on S200 and 30 ms on config 4 in
// front of 1.8 / 3.4 ms of Levenberg-Marquardt. Here the caller's arrays are uploaded as they are and everything else is
// built by sorts and scans (devprim.hpp): observations grouped by landmark and by camera (stable radix sorts: the order of
// a sequential host loop), the camera-aligned chunk table, the observation pairs of every landmark expanded in (landmark,
// a, b) order and sorted by camera block (stable: a block's entries stay in landmark order, which is the order every
// fp64 sum of the Schur complement runs in), the block and chunk tables by a scan over the block histogram. The host
// keeps what is irregular and small: the elimination ordering + symbolic analysis of the camera graph (ba_plan.hpp), fed by
// the block table read back. Three read-backs of a few bytes / kilobytes; the result is bit-identical with ba_prepare_host.
// ======================================================================================================================

struct PrepCounters {   // device-side scalars of the construction, read back by the host
    long long n_entries;     // expanded observation pairs
    int n_used;              // landmarks with at least one observation
    int bad;                 // an observation names a camera / landmark out of range
    int n_cam_chunks;
    int pad;
    prim::I3 totals;         // {entries, blocks, chunks} after the block scan
};

__device__ __forceinline__ int block_row_start(int c, int nc) {  // index of block (c, c) in the row-major upper triangle
    return (int)((long long)c * nc - (long long)c * (c - 1) / 2);
}

__global__ __launch_bounds__(TPB) void prep_values(int nc, int nl, const double* __restrict__ T_wc, const int* __restrict__ observers,
                                                   double* __restrict__ pose0, double* __restrict__ lmprior, double* __restrict__ K0,
                                                   double fx, double fy, double cx, double cy) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i == 0) {
        K0[0] = fx; K0[1] = fy; K0[2] = 0.0; K0[3] = cx; K0[4] = cy;
    }
    if (i < nc) {  // pose_from_Twc, operation for operation (no contraction: the host form has none)
        const double* T = T_wc + 16 * (size_t)i;
        double* x = pose0 + 12 * (size_t)i;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) x[3 * a + b] = T[4 * b + a];
        {
#pragma clang fp contract(off)  // (the header-defined __dmul_rn / __dadd_rn are plain operators and would be fused)
            for (int a = 0; a < 3; ++a) x[9 + a] = -((T[a] * T[3] + T[4 + a] * T[7]) + T[8 + a] * T[11]);
        }
    } else if (i - nc < nl) {  // BundleAdjuster.cpp:109-113: sigma = 1.0f/obs, k = 3.0f/obs (float)
        const int j = i - nc;
        const float o = (float)(observers[j] > 0 ? observers[j] : 1);
        lmprior[2 * (size_t)j] = (double)(1.0f / o);
        lmprior[2 * (size_t)j + 1] = (double)(3.0f / o);
    }
}

__global__ __launch_bounds__(TPB) void prep_keys_lm(int no, int nc, int nl, const uint32_t* __restrict__ in_cam,
                                                    const uint32_t* __restrict__ in_pt, uint32_t* __restrict__ keys,
                                                    uint32_t* __restrict__ vals, PrepCounters* __restrict__ cnt) {
    const int o = blockIdx.x * TPB + threadIdx.x;
    if (o >= no) return;
    uint32_t pt = in_pt[o];
    if (pt >= (uint32_t)nl || in_cam[o] >= (uint32_t)nc) {
        cnt->bad = 1;  // (benign race: every writer stores 1)
        pt = 0;
    }
    keys[o] = pt;
    vals[o] = (uint32_t)o;
}

// fills ptr[k] = first position whose key is >= k for the keys (prev, cur] seen at a boundary; sorted keys
__device__ __forceinline__ void fill_ptr(int* __restrict__ ptr, int pos, int prev_key, int cur_key) {
    for (int k = prev_key + 1; k <= cur_key; ++k) ptr[k] = pos;
}

constexpr int GATHER_CHUNKS = 4;   // chunks of TPB positions per workgroup of prep_gather_lm
__global__ __launch_bounds__(TPB) void prep_gather_lm(int no, int nl, int nc, const uint32_t* __restrict__ lm_sorted,
                                                      const uint32_t* __restrict__ order, const uint32_t* __restrict__ in_cam,
                                                      unsigned* __restrict__ obs_cam,
                                                      unsigned* __restrict__ obs_lm, int* __restrict__ lm_ptr,
                                                      uint32_t* __restrict__ cam_keys, uint32_t* __restrict__ cam_vals,
                                                      PrepCounters* __restrict__ cnt) {
    // A workgroup takes GATHER_CHUNKS consecutive chunks of TPB positions and adds its count of first positions to n_used ONCE: as one
    // atomic per wave (7 800 of them on S200, all to one address: ~12 ns each at the L2) the counter alone was 94 us of this kernel.
    __shared__ int s_first[TPB / 64];
    int mine = 0;   // first positions seen by this wave (lane 0 carries the count)
#pragma unroll 1
    for (int i = 0; i < GATHER_CHUNKS; ++i) {
        const int p = (blockIdx.x * GATHER_CHUNKS + i) * TPB + threadIdx.x;
        bool first = false;
        if (p < no) {
            const uint32_t o = order[p];
            const int lm = (int)lm_sorted[p];
            uint32_t c = in_cam[o];
            if (c >= (uint32_t)nc) c = 0;  // (flagged by prep_keys_lm: the call fails, the kernels stay in range)
            obs_cam[p] = c;
            obs_lm[p] = (unsigned)lm;
            cam_keys[p] = c;
            cam_vals[p] = (uint32_t)p;
            const int prev = p > 0 ? (int)lm_sorted[p - 1] : -1;
            first = lm != prev;
            if (first) fill_ptr(lm_ptr, p, prev, lm);
            if (p == no - 1) fill_ptr(lm_ptr, no, lm, nl);
        }
        mine += __popcll(__ballot(first));
    }
    if ((threadIdx.x & 63) == 0) s_first[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < TPB / 64; ++w) total += s_first[w];
        if (total) atomicAdd(&cnt->n_used, total);
    }
}

__global__ __launch_bounds__(TPB) void prep_gather_cam(int no, int nc, const uint32_t* __restrict__ cam_sorted,
                                                       const uint32_t* __restrict__ cam_obs_u, const unsigned* __restrict__ obs_lm,
                                                       int* __restrict__ cam_obs,
                                                       int* __restrict__ obs_pos, int* __restrict__ pos_cam, int* __restrict__ cam_lm,
                                                       int* __restrict__ cam_ptr) {
    const int q = blockIdx.x * TPB + threadIdx.x;
    if (q >= no) return;
    const int p = (int)cam_obs_u[q], c = (int)cam_sorted[q];
    cam_obs[q] = p;
    obs_pos[p] = q;
    pos_cam[q] = c;
    cam_lm[q] = (int)obs_lm[p];
    const int prev = q > 0 ? (int)cam_sorted[q - 1] : -1;
    if (c != prev) fill_ptr(cam_ptr, q, prev, c);
    if (q == no - 1) fill_ptr(cam_ptr, no, c, nc);
}
// The measurements in landmark order and in camera order, straight from the caller's array. A kernel of its own, LATE in the first
// half: the 16 bytes per observation are the largest of the caller's arrays (8 MB on S200, ~0.25 ms of PCIe from pageable memory)
// and nothing before the group rows needs them — the upload runs on the second stream while the sorts do (it sat between the
// landmark sort and its gather before, with the device idle for its whole length).
__global__ __launch_bounds__(TPB) void prep_gather_uv(int no, const uint32_t* __restrict__ order, const int* __restrict__ cam_obs,
                                                      const double* __restrict__ in_uv, double* __restrict__ obs_uv, double* __restrict__ cam_uv) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= no) return;
    const double2 a = *reinterpret_cast<const double2*>(&in_uv[2 * (size_t)order[i]]);
    const double2 b = *reinterpret_cast<const double2*>(&in_uv[2 * (size_t)order[cam_obs[i]]]);
    *reinterpret_cast<double2*>(&obs_uv[2 * (size_t)i]) = a;
    *reinterpret_cast<double2*>(&cam_uv[2 * (size_t)i]) = b;
}

__global__ __launch_bounds__(TPB) void prep_cam_chunk_counts(int nc, const int* __restrict__ cam_ptr, int* __restrict__ nchunk) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c < nc) nchunk[c] = (cam_ptr[c + 1] - cam_ptr[c] + TPB - 1) / TPB;
}
__global__ __launch_bounds__(TPB) void prep_cam_chunk_fill(int nc, const int* __restrict__ cam_ptr, const int* __restrict__ cam_chunk_ptr,
                                                           int2* __restrict__ cam_chunks) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= nc) return;
    int k = cam_chunk_ptr[c];
    for (int q = cam_ptr[c]; q < cam_ptr[c + 1]; q += TPB) cam_chunks[k++] = make_int2(q, min(TPB, cam_ptr[c + 1] - q));
}

// pair-list entries that start at observation a (landmark order): (a, a) and one per later observation b of the landmark,
// two when a and b sit in the same camera
__global__ __launch_bounds__(TPB) void prep_pair_counts(int no, const unsigned* __restrict__ obs_cam, const unsigned* __restrict__ obs_lm,
                                                        const int* __restrict__ lm_ptr, long long* __restrict__ cnt) {
    const int a = blockIdx.x * TPB + threadIdx.x;
    if (a >= no) return;
    const int a1 = lm_ptr[obs_lm[a] + 1];
    const unsigned ca = obs_cam[a];
    int c = 1;
    for (int b = a + 1; b < a1; ++b) c += 1 + (obs_cam[b] == ca ? 1 : 0);
    cnt[a] = c;
}

// camera graph of the reduced system: adj[c][c'] = 1 iff the two cameras share a landmark (benign races: every writer
// stores 1). The host's ordering + symbolic analysis starts from it while the device is still building the pair lists.
__global__ __launch_bounds__(TPB) void prep_cam_adjacency(int no, int nc, const unsigned* __restrict__ obs_cam, const unsigned* __restrict__ obs_lm,
                                                          const int* __restrict__ lm_ptr, unsigned char* __restrict__ adj) {
    const int a = blockIdx.x * TPB + threadIdx.x;
    if (a >= no) return;
    const int a1 = lm_ptr[obs_lm[a] + 1];
    const int ca = (int)obs_cam[a];
    for (int b = a + 1; b < a1; ++b) {
        const int cb = (int)obs_cam[b];
        if (ca < cb) adj[(size_t)ca * nc + cb] = 1;
        else if (cb < ca) adj[(size_t)cb * nc + ca] = 1;
    }
}

// the entries in (landmark, a, b) order = the order of the host loops; key = camera block, value = the two Et positions
__global__ __launch_bounds__(TPB) void prep_expand(int no, int nc, const unsigned* __restrict__ obs_cam, const unsigned* __restrict__ obs_lm,
                                                   const int* __restrict__ lm_ptr, const int* __restrict__ obs_pos,
                                                   const long long* __restrict__ off, uint32_t* __restrict__ keys,
                                                   int2* __restrict__ vals) {
    const int a = blockIdx.x * TPB + threadIdx.x;
    if (a >= no) return;
    const int a1 = lm_ptr[obs_lm[a] + 1];
    const int ca = (int)obs_cam[a], pa = obs_pos[a];
    long long e = off[a];
    const int diag = block_row_start(ca, nc);  // block (ca, ca); block (c, c2 >= c) = row_start(c) + c2 - c
    keys[e] = (uint32_t)diag;
    vals[e++] = make_int2(pa, pa);
    for (int b = a + 1; b < a1; ++b) {
        const int cb = (int)obs_cam[b], pb = obs_pos[b];
        if (ca < cb) {
            const int k = diag + (cb - ca);
            keys[e] = (uint32_t)k;
            vals[e++] = make_int2(pa, pb);
        } else if (ca > cb) {
            const int k = block_row_start(cb, nc) + (ca - cb);
            keys[e] = (uint32_t)k;
            vals[e++] = make_int2(pb, pa);
        } else {
            keys[e] = (uint32_t)diag;
            vals[e++] = make_int2(pa, pb);
            keys[e] = (uint32_t)diag;
            vals[e++] = make_int2(pb, pa);
        }
    }
}

// entries per camera block from the SORTED keys: the first and the one-past-last position of every run (2.75 M atomic increments
// on 20 k counters, most of them on the diagonal blocks, were 0.28 of the 0.75 ms the preparation's kernels took on S200)
__global__ __launch_bounds__(TPB) void prep_block_runs(int n, const uint32_t* __restrict__ keys, int* __restrict__ first, int* __restrict__ last) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (i == 0 || keys[i - 1] != k) first[k] = i;
    if (i == n - 1 || keys[i + 1] != k) last[k] = i + 1;
}

// per block of the upper triangle: {entries, present, chunks}; absent off-diagonal blocks stay out of the tables
__global__ __launch_bounds__(TPB) void prep_block_counts(int nc, int nblk, const int* __restrict__ first, const int* __restrict__ last,
                                                         int* __restrict__ bcount, prim::I3* __restrict__ t) {
    const int b = blockIdx.x * TPB + threadIdx.x;
    if (b >= nblk) return;
    int lo = 0, hi = nc - 1;  // largest c with row_start(c) <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (block_row_start(mid, nc) <= b) lo = mid;
        else hi = mid - 1;
    }
    const int cnt = last[b] - first[b];   // (both zero for a block without entries)
    bcount[b] = cnt;
    const bool present = cnt > 0 || b == block_row_start(lo, nc);
    t[b] = prim::I3{cnt, present ? 1 : 0, present ? (cnt + PAIR_CHUNK - 1) / PAIR_CHUNK : 0};
}
__global__ __launch_bounds__(TPB) void prep_block_fill(int nc, int nblk, const int* __restrict__ bcount, const prim::I3* __restrict__ s,
                                                       int4* __restrict__ blocks, int4* __restrict__ chunks) {
    const int b = blockIdx.x * TPB + threadIdx.x;
    if (b >= nblk) return;
    int lo = 0, hi = nc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (block_row_start(mid, nc) <= b) lo = mid;
        else hi = mid - 1;
    }
    const int c = lo, c2 = c + (b - block_row_start(c, nc));
    const int cnt = bcount[b];
    if (cnt == 0 && c != c2) return;
    const prim::I3 at = s[b];  // {first entry, block index, first chunk}
    const int k = (cnt + PAIR_CHUNK - 1) / PAIR_CHUNK;
    blocks[at.b] = make_int4(c, c2, at.c, k);
    for (int i = 0; i < k; ++i) chunks[at.c + i] = make_int4(at.b, at.a + PAIR_CHUNK * i, min(PAIR_CHUNK, cnt - PAIR_CHUNK * i), i);
}

// ---- device form of the landmark-major structure (ba_groups.hpp holds the definition; these kernels reproduce build_groups
// bit for bit: tests/test_ba_prepare_gpu.py compares every array) -------------------------------------------------------------
struct GrpCounters {
    int cmax, emax;            // largest landmark cost / entry count (atomicMax: order-free)
    int ng, n_long, cost_total, row_total;
    int any_dup, pad;          // some landmark sees a camera twice: the sort-free entries kernel does not apply
    prim::I3 item_totals;      // {mandatory items, blocks, .} of the sorted item list
    prim::I3 totals;           // {chunks, uint4-rows of entries, segments} over all groups
};

// per landmark: sort key, rows, entries, cost (ba_groups.hpp step 1-2)
__global__ __launch_bounds__(TPB) void prep_grp_keys(int nl, const int* __restrict__ lm_ptr, const unsigned* __restrict__ obs_cam,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, int* __restrict__ cost,
                                                     GrpCounters* __restrict__ gc) {
    // (the two maxima leave the workgroup as ONE atomic each: per thread they were 100 000 atomics to two addresses on S200)
    __shared__ int s_cmax, s_emax;
    if (threadIdx.x == 0) s_cmax = 0, s_emax = 0;
    __syncthreads();
    const int j = blockIdx.x * TPB + threadIdx.x;
    int c = 0, ec = 0;
    if (j < nl) {
        const int a0 = lm_ptr[j], a1 = lm_ptr[j + 1], m = a1 - a0;
        vals[j] = (uint32_t)j;
        if (m == 0) {
            keys[j] = 0xffffffffu;
            cost[j] = 0;
        } else {
            unsigned mn = obs_cam[a0], mx = mn;
            long long e = (long long)(m + 1) * (m + 2) / 2;
            for (int a = a0; a < a1; ++a) {
                const unsigned ca = obs_cam[a];
                mn = min(mn, ca), mx = max(mx, ca);
                for (int b = a + 1; b < a1; ++b) e += obs_cam[b] == ca ? 1 : 0;
            }
            if (e != (long long)(m + 1) * (m + 2) / 2) gc->any_dup = 1;  // (benign race: every writer stores 1)
            keys[j] = grp_morton(mn, mx);
            ec = e > 0x3fffffffLL ? 0x3fffffff : (int)e;
            c = max(max(m + 1, 4), (ec + GRP_ENT_PER_ROW - 1) / GRP_ENT_PER_ROW);  // ceil(e rows / ent_max), ent_max = 16 rows
            cost[j] = c;
        }
    }
    if (c > 0) atomicMax(&s_cmax, c);      // (LDS: order-free maxima; counters start at 0 and every real value is positive)
    if (ec > 0) atomicMax(&s_emax, ec);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cmax > 0) atomicMax(&gc->cmax, s_cmax);
        if (s_emax > 0) atomicMax(&gc->emax, s_emax);
    }
}
// in sorted order: rows and cost of rank k (zero beyond the used landmarks, which the key puts last)
__global__ __launch_bounds__(TPB) void prep_grp_sorted(int nl, const uint32_t* __restrict__ lm_sorted, const int* __restrict__ lm_ptr,
                                                       const int* __restrict__ cost, int* __restrict__ rowsS, int* __restrict__ costS) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= nl) return;
    const int j = (int)lm_sorted[k], m = lm_ptr[j + 1] - lm_ptr[j];
    rowsS[k] = m > 0 ? m + 1 : 0;
    costS[k] = cost[j];
}
// group g starts at the first rank whose cost prefix reaches g R0 (empty groups: the rank behind them); lm0[ng] = n_used
__global__ __launch_bounds__(TPB) void prep_grp_bounds(int nu, const int* __restrict__ cstart, int R0, int* __restrict__ lm0, GrpCounters* __restrict__ gc) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= nu) return;
    const int g = cstart[k] / R0, gp = k > 0 ? cstart[k - 1] / R0 : -1;
    for (int gg = gp + 1; gg <= g; ++gg) lm0[gg] = k;   // (a group no rank starts in is empty: lm0[gg] = lm0[gg + 1])
    if (k == nu - 1) {
        lm0[g + 1] = nu;
        gc->ng = g + 1;
    }
}
// per rank: the padded per-group arrays (landmark ids, own rows, row records, measurements) and the group record's first half
__global__ __launch_bounds__(TPB) void prep_grp_fill(int nu, int nc, int R, int R0, const uint32_t* __restrict__ lm_sorted, const int* __restrict__ cstart,
                                                     const int* __restrict__ rstart, const int* __restrict__ lm0, const int* __restrict__ lm_ptr,
                                                     const unsigned* __restrict__ obs_cam, const double* __restrict__ obs_uv, int* __restrict__ lmid,
                                                     int* __restrict__ lmrow, int2* __restrict__ rowinfo, double* __restrict__ uv) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= nu) return;
    const int g = cstart[k] / R0, k0 = lm0[g], t = k - k0, j = (int)lm_sorted[k];
    const int a0 = lm_ptr[j], m = lm_ptr[j + 1] - a0, r0 = rstart[k] - rstart[k0];
    const int LMAX = R / 4;
    lmid[(size_t)g * LMAX + t] = j;
    lmrow[(size_t)g * LMAX + t] = r0 + m;
    const size_t base = (size_t)g * R + r0;
    for (int i = 0; i < m; ++i) {
        rowinfo[base + i] = make_int2((int)obs_cam[a0 + i], t);
        uv[2 * (base + i)] = obs_uv[2 * (size_t)(a0 + i)];
        uv[2 * (base + i) + 1] = obs_uv[2 * (size_t)(a0 + i) + 1];
    }
    rowinfo[base + m] = make_int2(nc, t);
}

__global__ __launch_bounds__(TPB) void prep_grp_records(const GrpCounters* __restrict__ gc, const int* __restrict__ lm0, const int* __restrict__ rstart,
                                                        BaGroup* __restrict__ groups) {
    const int g = blockIdx.x * TPB + threadIdx.x;
    if (g >= gc->ng) return;
    const int k0 = lm0[g], k1 = lm0[g + 1];  // (rstart has an entry behind the last rank: the total)
    groups[g] = BaGroup{k0, k1 - k0, rstart[k0], rstart[k1] - rstart[k0], 0, 0, 0, 0};
}

// One workgroup per group: ba_groups.hpp step 3-4. The group's entries are generated as 64-bit words
//   block key << 31 | emission index << 18 | r1 << 9 | r2        (rows <= 511, <= 8192 entries)
// (the 9-bit row fields bound a group to 511 rows, the host form's multiple of 4 to 508: the largest EACHAM_BA_GROUP_ROWS
// that context.hip accepts, so that both forms of the construction build groups at every size the switch can select)
// and sorted by a bitonic network in LDS (the word order IS (block key, emission index)); runs, slices, lanes, segments and
// chunks follow from scans over the sorted list. PASS 0 only counts ({chunks, uint4-rows, segments} -> counts[g]); PASS 1, given
// the scanned bases, writes the chunk table, the entries, the lane records and the (key, where) list of the segments.
constexpr int GE_THREADS = 256;
constexpr int GE_MAXE = 8192;   // most entries of a group the kernel is ever asked for (rows <= 508)
template <class T>
__device__ __forceinline__ T ge_block_scan(T v, T* lds, T* total) {  // exclusive scan over the workgroup, GE_THREADS values
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int off = 1; off < GE_THREADS; off <<= 1) {
        const T u = tid >= off ? lds[tid - off] : T(0);
        __syncthreads();
        lds[tid] += u;
        __syncthreads();
    }
    const T incl = lds[tid];
    *total = lds[GE_THREADS - 1];
    __syncthreads();
    return incl - v;
}
// A run of L entries of one block as lanes: L > 4 gives ceil(L / GRP_SLICE) lanes of L / n (+ 1) entries, in the "long" region of
// the group's lane list; a shorter run is one lane of the "short" region behind it. f(offset in the run, length, long?) per lane.
template <class F>
__device__ __forceinline__ void ge_run_lanes(int L, F&& f) {
    const bool lng = L > 4;
    const int n = lng ? (L + GRP_SLICE - 1) / GRP_SLICE : L > 0 ? 1 : 0;
    const int each = lng ? L / n : L, more = lng ? L % n : 0;   // (a short run pays no division)
    for (int q = 0, at = 0; q < n; ++q) {
        const int len = each + (q < more ? 1 : 0);
        f(at, len, lng);
        at += len;
    }
}
// From the lane list to everything but the entries, for both entry kernels: steps per chunk, segments, the PASS 0 hand-off;
// in PASS 1 the group record, the chunk table, the lane records and the (key, where) list of the segments. lane_id[l] names
// the block of lane l (equal identity = same block; block_key turns a head's identity into the block key), lane_len[l] its
// entries; base = the group's {first chunk, first uint4-row, first segment} (PASS 1). Leaves chunk_ent0 / chunk_n4
// (workgroup-shared, GE_MAXE / 64 each) for the caller's entry-writing loop; true = the kernel is done (PASS 0).
template <int PASS, class KeyOf>
__device__ __forceinline__ bool ge_lanes_tail(const uint32_t* lane_id, const unsigned char* lane_len, int nlanes, int ne, int* scan_buf,
                                              int* chunk_ent0, int* chunk_n4, const prim::I3 base, int g, BaGroup* __restrict__ groups,
                                              prim::I3* __restrict__ counts, BaChunk* __restrict__ chunks,
                                              uint32_t* __restrict__ laneinfo, uint32_t* __restrict__ seg_key, uint32_t* __restrict__ seg_where,
                                              int seg_off, KeyOf&& block_key) {
    const int tid = threadIdx.x, nchunks = (nlanes + 63) / 64;
    // thread c < nchunks: longest lane of chunk c (nchunks <= GE_MAXE / 64 = 128 <= GE_THREADS)
    int my_n4 = 0;
    if (tid < nchunks) {
        int longest = 0;
        for (int l = 64 * tid; l < min(nlanes, 64 * tid + 64); ++l) longest = max(longest, (int)lane_len[l]);
        my_n4 = (longest + 3) / 4;
    }
    int tot_n4 = 0;
    const int off_n4 = ge_block_scan<int>(my_n4, scan_buf, &tot_n4);
    if (tid < nchunks) chunk_ent0[tid] = off_n4, chunk_n4[tid] = my_n4;
    // segment heads: lane li is a head iff (li - h0) % GRP_SEG == 0, h0 = first lane of its block at or after the row start
    int my_heads = 0;
    const int lper = (nlanes + GE_THREADS - 1) / GE_THREADS;
    const int l0 = min(tid * lper, nlanes), l1 = min(l0 + lper, nlanes);
    for (int li = l0; li < l1; ++li) {
        const uint32_t id = lane_id[li];
        int h = li;
        const int cs = li & ~(GRP_ROW - 1);   // a segment stays inside its row of 16 lanes
        while (h > cs && lane_id[h - 1] == id) --h;
        if (((li - h) % GRP_SEG) == 0) ++my_heads;
    }
    int tot_heads = 0;
    const int off_heads = ge_block_scan<int>(my_heads, scan_buf, &tot_heads);
    if (PASS == 0) {
        if (tid == 0) counts[g] = prim::I3{nchunks, tot_n4, tot_heads};
        return true;
    }
    __syncthreads();
    // ---- PASS 1: write ----
    if (tid == 0) {
        groups[g].chunk0 = base.a; groups[g].nchunks = nchunks; groups[g].n_entries = ne; groups[g].n_segments = tot_heads;
    }
    if (tid < nchunks) chunks[base.a + tid] = BaChunk{base.b + chunk_ent0[tid], chunk_n4[tid]};
    // lanes: records + segment list
    int hs = off_heads;
    for (int li = l0; li < l1; ++li) {
        const uint32_t id = lane_id[li];
        const int cs = li & ~(GRP_ROW - 1), ce = min(nlanes, cs + GRP_ROW);
        int h = li;
        while (h > cs && lane_id[h - 1] == id) --h;
        h += (li - h) / GRP_SEG * GRP_SEG;
        int e = h;
        while (e < ce && e < h + GRP_SEG && lane_id[e] == id) ++e;
        uint32_t info = (uint32_t)(e - 1 - li) << 28;
        const size_t where = (size_t)64 * base.a + li;
        if (li == h) {
            seg_key[seg_off + base.c + hs] = block_key(id);
            seg_where[seg_off + base.c + hs] = (uint32_t)where;
            ++hs;
            info |= 1u;  // (prep_grp_slots writes the slot)
        }
        laneinfo[where] = info;
    }
    for (int li = nlanes + tid; li < 64 * nchunks; li += GE_THREADS) laneinfo[(size_t)64 * base.a + li] = 0;
    return false;
}
template <int PASS>
__global__ __launch_bounds__(GE_THREADS) void prep_grp_entries(int emax /* power of two >= the group bound on entries */, int nc, int R, const GrpCounters* __restrict__ gc, BaGroup* __restrict__ groups,
                                                               const int2* __restrict__ rowinfo, const int* __restrict__ lmrow,
                                                               prim::I3* __restrict__ counts, const prim::I3* __restrict__ bases,
                                                               BaChunk* __restrict__ chunks, uint32_t* __restrict__ ent, uint32_t* __restrict__ laneinfo,
                                                               uint32_t* __restrict__ seg_key, uint32_t* __restrict__ seg_where, int seg_off) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ge_lds[];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g >= gc->ng) {
        if (PASS == 0 && tid == 0) counts[g] = prim::I3{0, 0, 0};
        return;
    }
    const BaGroup G = groups[g];
    const int LMAX = R / 4;
    unsigned long long* words = ge_lds;                         // [emax]
    uint32_t* lane_key = reinterpret_cast<uint32_t*>(ge_lds + emax);                // [emax] (a lane holds at least one entry)
    unsigned short* lane_first = reinterpret_cast<unsigned short*>(lane_key + emax);  // [emax]
    unsigned char* lane_len = reinterpret_cast<unsigned char*>(lane_first + emax);    // [emax]
    int* scan_buf = reinterpret_cast<int*>(lane_len + emax);    // [GE_THREADS]
    int* eoff = scan_buf + GE_THREADS;                          // [LMAX] first entry of landmark t
    // ---- entries per landmark (recomputed from the rows: cheap) and their offsets ----
    int my_e = 0, my_r0 = 0, my_m = 0;
    if (tid < G.nlm) {
        const int own = lmrow[(size_t)g * LMAX + tid];
        const int prev = tid > 0 ? lmrow[(size_t)g * LMAX + tid - 1] + 1 : 0;
        my_r0 = prev, my_m = own - prev;
        my_e = (my_m + 1) * (my_m + 2) / 2;
        const int2* ri = rowinfo + (size_t)g * R + my_r0;
        for (int a = 0; a < my_m; ++a)
            for (int b = a + 1; b < my_m; ++b) my_e += ri[a].x == ri[b].x ? 1 : 0;
    }
    int ne = 0;
    {
        // LMAX may exceed GE_THREADS only for rows > 1024 (not supported): one landmark per thread
        const int off = ge_block_scan<int>(my_e, scan_buf, &ne);
        if (tid < G.nlm) eoff[tid] = off;
    }
    __syncthreads();
    int npow = 64;
    while (npow < ne) npow <<= 1;
    const unsigned long long W = (unsigned long long)nc + 1;
    for (int i = tid; i < npow; i += GE_THREADS) words[i] = ~0ull;
    __syncthreads();
    if (tid < G.nlm) {
        const int2* ri = rowinfo + (size_t)g * R + my_r0;
        unsigned long long idx = (unsigned long long)eoff[tid];
        auto emit = [&](unsigned long long c1, unsigned long long c2, int r1, int r2) {
            words[idx] = ((c1 * W + c2) << 31) | (idx << 18) | ((unsigned long long)r1 << 9) | (unsigned long long)r2;
            ++idx;
        };
        for (int a = 0; a <= my_m; ++a) {
            const int ca = ri[a].x, ra = my_r0 + a;
            emit(ca, ca, ra, ra);
            for (int b = a + 1; b <= my_m; ++b) {
                const int cb = ri[b].x, rb = my_r0 + b;
                if (ca < cb) emit(ca, cb, ra, rb);
                else if (ca > cb) emit(cb, ca, rb, ra);
                else emit(ca, ca, ra, rb), emit(ca, ca, rb, ra);
            }
        }
    }
    __syncthreads();
    // ---- bitonic sort, ascending ----
    for (int kk = 2; kk <= npow; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < npow; i += GE_THREADS) {
                const int ixj = i ^ jj;
                if (ixj > i) {
                    const unsigned long long a = words[i], b = words[ixj];
                    const bool up = (i & kk) == 0;
                    if ((a > b) == up) words[i] = b, words[ixj] = a;
                }
            }
            __syncthreads();
        }
    // ---- runs -> lanes ----
    // per sorted position: run start flag; every thread handles a contiguous strip of positions
    const int per = (npow + GE_THREADS - 1) / GE_THREADS;  // positions per thread (strip)
    const int p0 = tid * per, p1 = min(p0 + per, ne);
    // pass over the strip: number of runs that START in it, by class (long: L > 4 counted in lanes; short: lanes = 1)
    // Run lengths need the next start: a thread finishes a run that started in its strip by walking on (runs are short: <= rows).
    int lanes_long = 0, lanes_short = 0;
    for (int i = p0; i < p1; ++i) {
        const unsigned long long key = words[i] >> 31;
        if (i > 0 && (words[i - 1] >> 31) == key) continue;
        int e = i + 1;
        while (e < ne && (words[e] >> 31) == key) ++e;
        ge_run_lanes(e - i, [&](int, int, bool lng) { lanes_long += lng ? 1 : 0, lanes_short += lng ? 0 : 1; });
    }
    int tot_long = 0, tot_short = 0;
    const int off_long = ge_block_scan<int>(lanes_long, scan_buf, &tot_long);
    const int off_short = ge_block_scan<int>(lanes_short, scan_buf, &tot_short);
    const int nlanes = tot_long + tot_short, nchunks = (nlanes + 63) / 64;
    {
        int ll = off_long, ls = tot_long + off_short;
        for (int i = p0; i < p1; ++i) {
            const unsigned long long key = words[i] >> 31;
            if (i > 0 && (words[i - 1] >> 31) == key) continue;
            int e = i + 1;
            while (e < ne && (words[e] >> 31) == key) ++e;
            ge_run_lanes(e - i, [&](int at, int len, bool lng) {
                const int l = lng ? ll : ls;
                ll += lng ? 1 : 0, ls += lng ? 0 : 1;
                lane_first[l] = (unsigned short)(i + at), lane_len[l] = (unsigned char)len, lane_key[l] = (uint32_t)key;
            });
        }
    }
    __syncthreads();
    // ---- chunks, segments, lane records (a lane's block = its key) ----
    __shared__ int s_chunk_ent0[GE_MAXE / 64], s_chunk_n4[GE_MAXE / 64];
    const prim::I3 base = PASS == 0 ? prim::I3{0, 0, 0} : bases[g];   // {first chunk, first uint4-row, first segment}
    if (ge_lanes_tail<PASS>(lane_key, lane_len, nlanes, ne, scan_buf, s_chunk_ent0, s_chunk_n4, base, g, groups, counts, chunks, laneinfo,
                            seg_key, seg_where, seg_off, [](uint32_t key) { return key; }))
        return;
    // entries: [chunk][step][lane][4], null beyond a slice
    const uint32_t null_ent = (uint32_t)R | ((uint32_t)R << 16);
    for (int c = 0; c < nchunks; ++c) {
        const int n4 = s_chunk_n4[c];
        uint32_t* dst = ent + (size_t)(base.b + s_chunk_ent0[c]) * 256;
        for (int x = tid; x < n4 * 256; x += GE_THREADS) {
            const int step = x >> 8, l = (x >> 2) & 63, i = 4 * step + (x & 3), li = 64 * c + l;
            uint32_t v = null_ent;
            if (li < nlanes && i < (int)lane_len[li]) {
                const unsigned long long w = words[lane_first[li] + i];
                v = (uint32_t)((w >> 9) & 0x1ffu) | ((uint32_t)(w & 0x1ffu) << 16);
            }
            dst[x] = v;
        }
    }
}
// The same two passes WITHOUT a sort, for problems in which no landmark sees a camera twice (prep_grp_keys knows; the general
// kernel above serves the others): with the group's cameras numbered locally in ascending order, the run of block (la, lb) is
// the landmarks that see both — M[la] & M[lb] for per-camera bit masks over the group's <= 128 landmarks — in ascending
// landmark order, which IS the (block key, emission index) order of the definition. Pairs are walked in key order by strips,
// their runs cut into lanes by ge_run_lanes, the lane list handed to ge_lanes_tail (a lane's identity is its pair's index;
// the block key of a head comes from the pair's two cameras), and a lane's entries are read off the mask (the bits from its
// start position on; the two rows by a search through the landmark's few rows). 0.56 ms per pass on S200 with the bitonic sort,
// the per-group time here is a small sort of the <= 512 row cameras and a few scans.
__device__ __forceinline__ int gf_pairs_before(int la, int U) { return la * U - la * (la - 1) / 2; }
template <int PASS>
__global__ __launch_bounds__(GE_THREADS) void prep_grp_entries_fast(int lane_cap, int nc, int R, const GrpCounters* __restrict__ gc, BaGroup* __restrict__ groups,
                                                                    const int2* __restrict__ rowinfo, const int* __restrict__ lmrow,
                                                                    prim::I3* __restrict__ counts, const prim::I3* __restrict__ bases,
                                                                    BaChunk* __restrict__ chunks, uint32_t* __restrict__ ent, uint32_t* __restrict__ laneinfo,
                                                                    uint32_t* __restrict__ seg_key, uint32_t* __restrict__ seg_where, int seg_off) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long gf_lds[];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g >= gc->ng) {
        if (PASS == 0 && tid == 0) counts[g] = prim::I3{0, 0, 0};
        return;
    }
    const BaGroup G = groups[g];
    const int LMAX = R / 4;
    int RP2 = 64;
    while (RP2 < R) RP2 <<= 1;
    unsigned long long* mask = gf_lds;                                   // [2 R] landmarks that see local camera la (two words)
    int* camsort = reinterpret_cast<int*>(mask + 2 * R);                 // [RP2]
    int* ucam = camsort + RP2;                                           // [R] local camera -> camera
    int* scan_buf = ucam + R;                                            // [GE_THREADS]
    uint32_t* lane_q = reinterpret_cast<uint32_t*>(scan_buf + GE_THREADS);  // [lane_cap] pair of the lane
    unsigned short* row_la = reinterpret_cast<unsigned short*>(lane_q + lane_cap);  // [R] local camera of a row
    unsigned short* lm_r0 = row_la + R;                                  // [LMAX + 1] first row of landmark t
    unsigned char* lane_at = reinterpret_cast<unsigned char*>(lm_r0 + LMAX + 2);    // [lane_cap] first position of the lane inside its run
    unsigned char* lane_len = lane_at + lane_cap;                        // [lane_cap]
    __shared__ int s_chunk_ent0[GE_MAXE / 64], s_chunk_n4[GE_MAXE / 64];
    // ---- the group's cameras, ascending, without repetition ----
    for (int r = tid; r < RP2; r += GE_THREADS) {
        const int c = r < G.nrows ? rowinfo[(size_t)g * R + r].x : 0x7fffffff;
        camsort[r] = c;
    }
    for (int t = tid; t <= G.nlm; t += GE_THREADS) lm_r0[t] = (unsigned short)(t == 0 ? 0 : lmrow[(size_t)g * LMAX + t - 1] + 1);
    for (int i = tid; i < 2 * R; i += GE_THREADS) mask[i] = 0ull;
    __syncthreads();
    for (int kk = 2; kk <= RP2; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < RP2; i += GE_THREADS) {
                const int ixj = i ^ jj;
                if (ixj > i) {
                    const int a = camsort[i], b = camsort[ixj];
                    if ((a > b) == ((i & kk) == 0)) camsort[i] = b, camsort[ixj] = a;
                }
            }
            __syncthreads();
        }
    int U = 0;
    {
        const int per = RP2 / GE_THREADS > 0 ? RP2 / GE_THREADS : 1;   // consecutive elements per thread
        const int i0 = tid * per, i1 = min(i0 + per, RP2);
        int mine = 0;
        for (int i = i0; i < i1; ++i) mine += (camsort[i] != 0x7fffffff && (i == 0 || camsort[i] != camsort[i - 1])) ? 1 : 0;
        int at = ge_block_scan<int>(i0 < RP2 ? mine : 0, scan_buf, &U);
        for (int i = i0; i < i1; ++i)
            if (camsort[i] != 0x7fffffff && (i == 0 || camsort[i] != camsort[i - 1])) ucam[at++] = camsort[i];
    }
    __syncthreads();
    for (int r = tid; r < G.nrows; r += GE_THREADS) {
        const int2 ri = rowinfo[(size_t)g * R + r];
        int lo = 0, hi = U - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ucam[mid] < ri.x) lo = mid + 1;
            else hi = mid;
        }
        row_la[r] = (unsigned short)lo;
        atomicOr(&mask[2 * lo + (ri.y >> 6)], 1ull << (ri.y & 63));
    }
    __syncthreads();
    // ---- pairs (la <= lb) in key order, by strips ----
    const int P = U * (U + 1) / 2;
    const int per = (P + GE_THREADS - 1) / GE_THREADS;
    const int q0 = min(tid * per, P), q1 = min(q0 + per, P);
    auto pair_of = [&](int q, int& la, int& lb) {
        int lo = 0, hi = U - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (gf_pairs_before(mid, U) <= q) lo = mid;
            else hi = mid - 1;
        }
        la = lo, lb = lo + (q - gf_pairs_before(lo, U));
    };
    auto run_len = [&](int la, int lb) {
        return __popcll(mask[2 * la] & mask[2 * lb]) + __popcll(mask[2 * la + 1] & mask[2 * lb + 1]);
    };
    int lanes_long = 0, lanes_short = 0, my_entries = 0;
    if (q0 < q1) {
        int la, lb;
        pair_of(q0, la, lb);
        for (int q = q0; q < q1; ++q) {
            const int L = run_len(la, lb);
            my_entries += L;
            ge_run_lanes(L, [&](int, int, bool lng) { lanes_long += lng ? 1 : 0, lanes_short += lng ? 0 : 1; });
            if (++lb == U) ++la, lb = la;
        }
    }
    int tot_long = 0, tot_short = 0, ne = 0;
    const int off_long = ge_block_scan<int>(lanes_long, scan_buf, &tot_long);
    const int off_short = ge_block_scan<int>(lanes_short, scan_buf, &tot_short);
    (void)ge_block_scan<int>(my_entries, scan_buf, &ne);
    const int nlanes = tot_long + tot_short, nchunks = (nlanes + 63) / 64;
    if (q0 < q1) {
        int la, lb, ll = off_long, ls = tot_long + off_short;
        pair_of(q0, la, lb);
        for (int q = q0; q < q1; ++q) {
            ge_run_lanes(run_len(la, lb), [&](int at, int len, bool lng) {
                const int l = lng ? ll : ls;
                ll += lng ? 1 : 0, ls += lng ? 0 : 1;
                lane_q[l] = (uint32_t)q, lane_at[l] = (unsigned char)at, lane_len[l] = (unsigned char)len;
            });
            if (++lb == U) ++la, lb = la;
        }
    }
    __syncthreads();
    // ---- chunks, segments, lane records (a lane's block = its pair; the key of a head's block from the pair's two cameras) ----
    const uint32_t W = (uint32_t)nc + 1;
    const prim::I3 base = PASS == 0 ? prim::I3{0, 0, 0} : bases[g];   // {first chunk, first uint4-row, first segment}
    if (ge_lanes_tail<PASS>(lane_q, lane_len, nlanes, ne, scan_buf, s_chunk_ent0, s_chunk_n4, base, g, groups, counts, chunks, laneinfo,
                            seg_key, seg_where, seg_off, [&](uint32_t q) {
                                int la, lb;
                                pair_of((int)q, la, lb);
                                return (uint32_t)ucam[la] * W + (uint32_t)ucam[lb];
                            }))
        return;
    // entries, a lane per thread: the landmarks of the run from position lane_at on; the two rows by a search through the landmark's rows
    const uint32_t null_ent = (uint32_t)R | ((uint32_t)R << 16);
    for (int li = tid; li < 64 * nchunks; li += GE_THREADS) {
        const int c = li >> 6, l = li & 63, n4 = s_chunk_n4[c];
        uint4* dst = reinterpret_cast<uint4*>(ent + (size_t)(base.b + s_chunk_ent0[c]) * 256) + l;
        int len = 0, la = 0, lb = 0;
        unsigned long long m0 = 0, m1 = 0;
        if (li < nlanes) {
            pair_of((int)lane_q[li], la, lb);
            m0 = mask[2 * la] & mask[2 * lb], m1 = mask[2 * la + 1] & mask[2 * lb + 1];
            len = lane_len[li];
            for (int skip = lane_at[li]; skip > 0; --skip) {  // drop the run's first lane_at landmarks
                if (m0) m0 &= m0 - 1;
                else m1 &= m1 - 1;
            }
        }
        for (int step = 0; step < n4; ++step) {
            uint32_t v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = null_ent;
                if (4 * step + i < len) {
                    int t;
                    if (m0) t = __builtin_ctzll(m0), m0 &= m0 - 1;
                    else t = 64 + __builtin_ctzll(m1), m1 &= m1 - 1;
                    int r1 = 0, r2 = 0;
                    for (int r = lm_r0[t]; r < (int)lm_r0[t + 1]; ++r) {
                        const int x = row_la[r];
                        r1 = x == la ? r : r1;
                        r2 = x == lb ? r : r2;
                    }
                    v[i] = (uint32_t)r1 | ((uint32_t)r2 << 16);
                }
            }
            dst[(size_t)step * 64] = make_uint4(v[0], v[1], v[2], v[3]);
        }
    }
}
__host__ inline size_t grp_entries_fast_lds_bytes(int lane_cap, int R) {
    int RP2 = 64;
    while (RP2 < R) RP2 <<= 1;
    return sizeof(unsigned long long) * 2 * R + sizeof(int) * ((size_t)RP2 + R + GE_THREADS) + sizeof(uint32_t) * (size_t)lane_cap +
           sizeof(unsigned short) * ((size_t)R + R / 4 + 2) + 2 * (size_t)lane_cap + 16;
}
__host__ inline size_t grp_entries_lds_bytes(int emax, int R) {
    return (size_t)emax * (8 + 4 + 2 + 1) + sizeof(int) * ((size_t)GE_THREADS + R / 4 + 8);
}

// the mandatory blocks, first in the input of the stable sort by block key: (c, c), (c, K) for every camera, then (K, K)
__global__ __launch_bounds__(TPB) void prep_grp_mandatory(int nc, uint32_t* __restrict__ seg_key, uint32_t* __restrict__ seg_where) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i > 2 * nc) return;
    const uint32_t W = (uint32_t)nc + 1;
    seg_key[i] = i == 2 * nc ? (uint32_t)nc * W + nc : (i & 1) ? (uint32_t)(i >> 1) * W + nc : (uint32_t)(i >> 1) * W + (i >> 1);
    seg_where[i] = 0xffffffffu;
}
// over the sorted items: {mandatory, run start, 0} flags for the scan
__global__ __launch_bounds__(TPB) void prep_grp_flags(int n, const uint32_t* __restrict__ key, const uint32_t* __restrict__ where, prim::I3* __restrict__ f) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    f[i] = prim::I3{where[i] == 0xffffffffu ? 1 : 0, (i == 0 || key[i - 1] != key[i]) ? 1 : 0, 0};
}
// slot of every segment (its rank among the segments in sorted order) into its lane record; the block table from the runs
__global__ __launch_bounds__(TPB) void prep_grp_slots(int n, int nc, const uint32_t* __restrict__ key, const uint32_t* __restrict__ where,
                                                      const prim::I3* __restrict__ s, uint32_t* __restrict__ laneinfo, int4* __restrict__ blk,
                                                      int* __restrict__ blk_first_item) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const prim::I3 at = s[i];  // {mandatory items before i, run starts before i, .}
    if (where[i] != 0xffffffffu) laneinfo[where[i]] = (laneinfo[where[i]] & 0xf0000000u) | (uint32_t)(i - at.a + 1);
    if (i == 0 || key[i - 1] != key[i]) {
        const uint32_t W = (uint32_t)nc + 1;
        blk[at.b] = make_int4((int)(key[i] / W), (int)(key[i] % W), i - at.a, 0);
        blk_first_item[at.b] = i;
    }
}
// count of every block = items of its run - its mandatory item; the long-block flags
__global__ __launch_bounds__(TPB) void prep_grp_blk_counts(const GrpCounters* __restrict__ gc, int n_items, const uint32_t* __restrict__ where,
                                                           const int* __restrict__ blk_first_item, int4* __restrict__ blk, int* __restrict__ longflag) {
    const int b = blockIdx.x * TPB + threadIdx.x, nblk = gc->item_totals.b;
    if (b >= n_items) return;
    if (b >= nblk) {
        longflag[b] = 0;
        return;
    }
    const int i0 = blk_first_item[b], i1 = b + 1 < nblk ? blk_first_item[b + 1] : n_items;
    const int cnt = i1 - i0 - (where[i0] == 0xffffffffu ? 1 : 0);  // (the mandatory item, if any, is the run's first: stable sort, first in the input)
    blk[b].w = cnt;
    longflag[b] = cnt > GRP_LONG ? 1 : 0;
}
__global__ __launch_bounds__(TPB) void prep_grp_long(const GrpCounters* __restrict__ gc, const int* __restrict__ longflag, const int* __restrict__ pos, int* __restrict__ longblk) {
    const int b = blockIdx.x * TPB + threadIdx.x;
    if (b < gc->item_totals.b && longflag[b]) longblk[pos[b]] = b;
}

static int ba_scratch(eacham_ctx* ctx, int which, size_t bytes, void** out) {
    BaScratch& sc = ctx->ba_scratch[which];
    if (bytes > sc.bytes) {
        if (sc.dev) {
            EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipFree(sc.dev);
            sc.dev = nullptr;
            sc.bytes = 0;
        }
        const size_t want = bytes + bytes / 4;
        EACHAM_HIP_TRY(ctx, hipMalloc(&sc.dev, want));
        sc.bytes = want;
    }
    *out = sc.dev;
    return EACHAM_OK;
}

// Scratch buffer `which` of the context, sized and carved by `carve` (a Bump sequence; a null base gives the size only).
template <class Carve>
static int ba_scratch_carve(eacham_ctx* ctx, int which, Carve carve) {
    void* base = nullptr;
    TRY(ba_scratch(ctx, which, carve(nullptr), &base));
    (void)carve(base);
    return EACHAM_OK;
}

static int bits_for(long long n) { int b = 1; while ((1ll << b) < n) ++b; return b; }

// The device construction, cut into stages at its read-backs: what one stage leaves for a later one lives here, everything else
// is local to its stage. ba_prepare_device runs the stages in the order they are written in; every launch, copy, event and
// synchronisation keeps its place on its stream (the overlap of the device work with the plan thread and with the uploads on the
// second stream is what the call's time rests on: docs/HISTORY.md).
struct BaDevicePrep {
    eacham_ctx* const ctx;
    const eacham_ba_problem* const P;
    eacham_ba_handle* const h;
    BaDev& D;
    const int hint, nc, nl, no, nblk;
    const hipStream_t st;
    const unsigned gobs;      // blocks of a launch over the observations
    const bool try_groups;    // the landmark groups are wanted (ba_groups_wanted) and the problem can be keyed for them
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    // arena A: the structure arrays (BaDev holds most of them as pointers to const)
    int *lm_ptr = nullptr, *cam_ptr = nullptr, *cam_obs = nullptr, *cam_lm = nullptr, *cam_chunk_ptr = nullptr, *obs_pos = nullptr, *pos_cam = nullptr, *fixed = nullptr;
    int2* cam_chunks = nullptr;
    double *lmprior = nullptr, *obs_uv = nullptr, *cam_uv = nullptr;
    unsigned *obs_cam = nullptr, *obs_lm = nullptr;
    // scratch 0: the caller's arrays as they are + the temporaries of the observation sorts
    uint32_t *raw_cam, *raw_pt, *kA, *kB, *vA, *vB, *kC, *vC, *lm_order = nullptr;
    double *raw_uv, *raw_T;
    int *raw_obs, *sort_ws, *nchunk, *nchunk_ws;
    long long *pcnt, *poff, *pws;
    PrepCounters* cnt;
    unsigned char* adj_dev;
    uint32_t *gkA, *gkB, *gvA, *gvB;
    int *gcost, *growsS, *gcostS, *gcstart, *grstart, *gscan_ws, *gsort_ws;
    GrpCounters* gcnt;
    int w_g = 0;
    // read-back 1 and what follows from it
    PrepCounters hc{};
    GrpCounters hg{};
    int R = 0, n_entries = 0;
    bool use_groups = false;
    // the pair lists (scratch 1), until arena B takes them
    int2 *evA = nullptr, *evB = nullptr;
    int4 *blocks_tmp = nullptr, *chunks_tmp = nullptr;
    int w_e = 0;
    // the landmark groups: what the first half (scratch 2) and the second half (scratch 3) staged, until arena B takes it
    int g_emax = 64, n_items = 0;
    BaGroup* tg_groups = nullptr;
    int *tg_lmid = nullptr, *tg_lmrow = nullptr;
    int2* tg_rowinfo = nullptr;
    double* tg_uv = nullptr;
    prim::I3* tg_bases = nullptr;
    BaChunk* sg_chunks = nullptr;
    uint32_t *sg_ent = nullptr, *sg_laneinfo = nullptr;
    int4* sg_blk = nullptr;
    int* sg_longblk = nullptr;
    // the plan thread's input and verdict
    std::vector<unsigned char> adj_h;
    bool plan_failed = false;
    BaPrepareGuard guard;  // the LAST member: destroyed first, so that an error return joins the plan thread while what it uses exists

    BaDevicePrep(eacham_ctx* c, const eacham_ba_problem* p, int ordering_hint)
        : ctx(c), P(p), h(new eacham_ba_handle()), D(h->D), hint(ordering_hint), nc(p->n_cams), nl(p->n_points), no(p->n_obs),
          nblk((int)((long long)nc * (nc + 1) / 2)), st(c->stream), gobs((unsigned)((no + TPB - 1) / TPB)),
          try_groups(ba_groups_wanted(c, true) && nc < 65535 && no > 0), guard(c, h) {
        ba_handle_init(P, h);
    }

    // ---- arena A: everything whose size follows from (nc, nl, no); scratch 0 ----
    int first_arena() {
        const int max_cam_chunks = no / TPB + nc + 1;
        auto layout_a = [&]() -> int {
            dev_alloc(h, &D.pose0, 12 * (size_t)nc);
            dev_alloc(h, &D.pt0, 3 * (size_t)nl);
            dev_alloc(h, &D.K0, 8);
            dev_alloc(h, &lmprior, 2 * (size_t)nl);
            dev_alloc(h, &obs_uv, 2 * (size_t)no);
            dev_alloc(h, &fixed, (size_t)nc);
            dev_alloc(h, &lm_ptr, (size_t)nl + 1);
            dev_alloc(h, &cam_ptr, (size_t)nc + 1);
            dev_alloc(h, &cam_obs, (size_t)no);
            dev_alloc(h, &cam_lm, (size_t)no);
            dev_alloc(h, &cam_chunks, (size_t)max_cam_chunks);
            dev_alloc(h, &cam_chunk_ptr, (size_t)nc + 1);
            dev_alloc(h, &obs_pos, (size_t)no);
            dev_alloc(h, &pos_cam, (size_t)no);
            dev_alloc(h, &cam_uv, 2 * (size_t)no);
            dev_alloc(h, &obs_cam, (size_t)no);
            dev_alloc(h, &obs_lm, (size_t)no);
            TRY(ba_alloc_work_a(ctx, h));
            return EACHAM_OK;
        };
        TRY(ba_arena_layout(ctx, h, &h->block, layout_a, [] { return std::make_pair((size_t)0, (size_t)0); }));
        D.lmprior = lmprior; D.obs_uv = obs_uv; D.fixed = fixed; D.lm_ptr = lm_ptr; D.cam_ptr = cam_ptr; D.cam_obs = cam_obs; D.cam_lm = cam_lm;
        D.cam_chunks = cam_chunks; D.cam_chunk_ptr = cam_chunk_ptr; D.obs_pos = obs_pos; D.pos_cam = pos_cam; D.cam_uv = cam_uv;
        D.obs_cam = obs_cam; D.obs_lm = obs_lm;
        h->pose_init = D.pose0; h->pt_init = D.pt0; h->K_init = D.K0;
        return ba_scratch_carve(ctx, 0, [&](void* base) {
            Bump b(base);
            raw_pt = b.take<uint32_t>(no); raw_cam = b.take<uint32_t>(no); raw_uv = b.take<double>(2 * (size_t)no);
            raw_T = b.take<double>(16 * (size_t)nc); raw_obs = b.take<int>(nl);
            kA = b.take<uint32_t>(no); kB = b.take<uint32_t>(no); vA = b.take<uint32_t>(no); vB = b.take<uint32_t>(no);
            kC = b.take<uint32_t>(no); vC = b.take<uint32_t>(no);   // the camera sort's second pair (the landmark order stays: the late uv gather reads it)
            sort_ws = b.take<int>(prim::radix_ws_ints(no));
            nchunk = b.take<int>(nc); nchunk_ws = b.take<int>(prim::scan_ws_elems(nc));
            pcnt = b.take<long long>(no); poff = b.take<long long>((size_t)no + 1); pws = b.take<long long>(prim::scan_ws_elems(no));
            cnt = b.take<PrepCounters>(1);
            adj_dev = b.take<unsigned char>((size_t)nc * nc);
            // the landmark order of the group structure (ba_groups.hpp): keys, ranks, per-rank rows / costs and their prefixes
            gkA = b.take<uint32_t>(nl); gkB = b.take<uint32_t>(nl); gvA = b.take<uint32_t>(nl); gvB = b.take<uint32_t>(nl);
            gcost = b.take<int>(nl); growsS = b.take<int>(nl); gcostS = b.take<int>(nl);
            gcstart = b.take<int>((size_t)nl + 1); grstart = b.take<int>((size_t)nl + 1); gscan_ws = b.take<int>(prim::scan_ws_elems(nl));
            gsort_ws = b.take<int>(prim::radix_ws_ints(nl));
            gcnt = b.take<GrpCounters>(1);
            return b.off;
        });
    }

    // ---- the uploads; observations grouped by landmark and by camera, the camera graph, the chunk table, the groups' landmark order ----
    int structure() {
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(cnt, 0, sizeof(PrepCounters), st));
        // the landmark ids first: their sort runs while the host stages the rest
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(raw_pt, P->obs_point, sizeof(uint32_t) * (size_t)no, hipMemcpyHostToDevice, st));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(raw_cam, P->obs_cam, sizeof(uint32_t) * (size_t)no, hipMemcpyHostToDevice, st));
        if (no > 0) prep_keys_lm<<<gobs, TPB, 0, st>>>(no, nc, nl, raw_cam, raw_pt, kA, vA, cnt);
        const int w_lm = prim::radix_sort_pairs<uint32_t>(st, kA, vA, kB, vB, no, bits_for(std::max(nl, 2)), sort_ws);
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(raw_T, P->cam_T_wc, sizeof(double) * 16 * (size_t)nc, hipMemcpyHostToDevice, st));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(raw_obs, P->point_observers, sizeof(int) * (size_t)nl, hipMemcpyHostToDevice, st));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(D.pt0, P->points, sizeof(double) * 3 * (size_t)nl, hipMemcpyHostToDevice, st));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(fixed, P->cam_fixed, sizeof(int) * (size_t)nc, hipMemcpyHostToDevice, st));
        prep_values<<<(unsigned)((nc + nl + TPB) / TPB), TPB, 0, st>>>(nc, nl, raw_T, raw_obs, D.pose0, lmprior, D.K0, P->K[0], P->K[1], P->K[2], P->K[3]);
        uint32_t *lm_sorted = w_lm ? kB : kA, *ck = w_lm ? kA : kB, *cv = w_lm ? vA : vB;  // the other pair of buffers feeds the camera sort
        lm_order = w_lm ? vB : vA;
        if (no > 0) {
            prep_gather_lm<<<(gobs + GATHER_CHUNKS - 1) / GATHER_CHUNKS, TPB, 0, st>>>(no, nl, nc, lm_sorted, lm_order, raw_cam, obs_cam, obs_lm, lm_ptr, ck, cv, cnt);
        } else {
            EACHAM_HIP_TRY(ctx, hipMemsetAsync(lm_ptr, 0, sizeof(int) * ((size_t)nl + 1), st));
            EACHAM_HIP_TRY(ctx, hipMemsetAsync(cam_ptr, 0, sizeof(int) * ((size_t)nc + 1), st));
        }
        // the camera graph leaves for the host on the second stream as soon as the landmark grouping exists
        if (nc > 0) EACHAM_HIP_TRY(ctx, hipMemsetAsync(adj_dev, 0, (size_t)nc * nc, st));
        if (no > 0 && nc > 0) prep_cam_adjacency<<<gobs, TPB, 0, st>>>(no, nc, obs_cam, obs_lm, lm_ptr, adj_dev);
        EACHAM_HIP_TRY(ctx, hipEventRecord(ctx->ev_join, st));
        const int w_cam = prim::radix_sort_pairs<uint32_t>(st, ck, cv, kC, vC, no, bits_for(std::max(nc, 2)), sort_ws);
        if (no > 0) {
            const uint32_t *cs = w_cam ? kC : ck, *co = w_cam ? vC : cv;
            prep_gather_cam<<<gobs, TPB, 0, st>>>(no, nc, cs, co, obs_lm, cam_obs, obs_pos, pos_cam, cam_lm, cam_ptr);
            if (!try_groups) prep_pair_counts<<<gobs, TPB, 0, st>>>(no, obs_cam, obs_lm, lm_ptr, pcnt);
        }
        if (try_groups) {  // ba_groups.hpp steps 1-2 as far as they go without the group size: order, rows, costs, their prefixes
            EACHAM_HIP_TRY(ctx, hipMemsetAsync(gcnt, 0, sizeof(GrpCounters), st));
            const unsigned glm = (unsigned)((nl + TPB - 1) / TPB);
            prep_grp_keys<<<glm, TPB, 0, st>>>(nl, lm_ptr, obs_cam, gkA, gvA, gcost, gcnt);
            // (the key interleaves two camera ids: 2 bits_for(nc + 1) bits; landmarks without observations carry the largest key of that width)
            const int gkey_bits = std::min(32, 2 * bits_for((long long)nc + 1));
            w_g = prim::radix_sort_pairs<uint32_t>(st, gkA, gvA, gkB, gvB, nl, gkey_bits, gsort_ws);
            prep_grp_sorted<<<glm, TPB, 0, st>>>(nl, w_g ? gvB : gvA, lm_ptr, gcost, growsS, gcostS);
            prim::exclusive_scan<int>(st, gcostS, gcstart, nl, gscan_ws, &gcnt->cost_total);
            prim::exclusive_scan<int>(st, growsS, grstart, nl, gscan_ws, &gcnt->row_total);
            EACHAM_HIP_TRY(ctx, hipMemcpyAsync(grstart + nl, &gcnt->row_total, sizeof(int), hipMemcpyDeviceToDevice, st));
        }
        prep_cam_chunk_counts<<<(unsigned)((nc + TPB) / TPB), TPB, 0, st>>>(nc, cam_ptr, nchunk);
        prim::exclusive_scan<int>(st, nchunk, cam_chunk_ptr, nc, nchunk_ws, &cnt->n_cam_chunks);
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(cam_chunk_ptr + nc, &cnt->n_cam_chunks, sizeof(int), hipMemcpyDeviceToDevice, st));
        prep_cam_chunk_fill<<<(unsigned)((nc + TPB) / TPB), TPB, 0, st>>>(nc, cam_ptr, cam_chunk_ptr, cam_chunks);
        if (!try_groups) prim::exclusive_scan<long long>(st, pcnt, poff, no, pws, &cnt->n_entries);
        return EACHAM_OK;
    }

    // ---- the host's share, beside the device's: ordering, panels, symbolic factor, level schedule (ba_plan.hpp) on a thread of its
    // own; the measurements; read-back 1 and the choice between the landmark groups and the pair lists ----
    int plan_and_counts() {
        adj_h.resize((size_t)nc * nc + 1);
        EACHAM_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_join, 0));
        if (nc > 0) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(adj_h.data(), adj_dev, (size_t)nc * nc, hipMemcpyDeviceToHost, ctx->stream2));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
        // (no HIP call in there, and no exception may leave it: a failed allocation or thread start inside the analysis comes back as
        // an error code of the call — std::terminate in a process that holds the GPU is not an answer)
        auto plan_body = [this]() {
            try {
                const auto t_plan = std::chrono::steady_clock::now();
                std::vector<std::pair<int, int>> cam_edges;
                for (int c = 0; c < nc; ++c)
                    for (int c2 = c + 1; c2 < nc; ++c2)
                        if (adj_h[(size_t)c * nc + c2]) cam_edges.emplace_back(c, c2);
                build_ba_plan(nc, cam_edges, hint, h->plan);
                h->prep_us[1] = us_since(t_plan);
            } catch (...) {
                plan_failed = true;
            }
        };
        try {
            guard.plan_thread = std::thread(plan_body);
        } catch (const std::system_error&) {
            plan_body();  // no thread to be had: the analysis runs here, before the rest of the device work is queued
        }
        // ---- the measurements: uploaded on the second stream beside the kernels queued above, gathered behind them ----
        if (no > 0) {
            EACHAM_HIP_TRY(ctx, hipMemcpyAsync(raw_uv, P->obs_uv, sizeof(double) * 2 * (size_t)no, hipMemcpyHostToDevice, ctx->stream2));
            EACHAM_HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
            EACHAM_HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
            prep_gather_uv<<<gobs, TPB, 0, st>>>(no, lm_order, cam_obs, raw_uv, obs_uv, cam_uv);
        }
        // ---- read-back 1: the number of pair entries sizes the next stage ----
        memset(&hg, 0, sizeof(hg));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, st));
        if (try_groups) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(&hg, gcnt, sizeof(hg), hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        if (hc.bad) return ctx->fail(EACHAM_ERR_INVALID, "an observation references a camera/point out of range");
        // the landmark-major structure applies unless a landmark is too heavy for a group (ba_groups.hpp step 2)
        const long long total_rows = (long long)no + hc.n_used;
        R = ctx->ba_group_rows > 0 ? ctx->ba_group_rows : grp_rows_for(total_rows);
        use_groups = try_groups && total_rows <= 0x7fffffffLL && R % 4 == 0 && hg.emax <= GRP_ENT_PER_ROW * R && hg.cmax <= R / 2 && std::max(hg.cmax, 4) >= 4;
        if (try_groups && !use_groups) {  // the pair lists of rounds 1-4 after all: their counts were not taken yet
            prep_pair_counts<<<gobs, TPB, 0, st>>>(no, obs_cam, obs_lm, lm_ptr, pcnt);
            prim::exclusive_scan<long long>(st, pcnt, poff, no, pws, &cnt->n_entries);
            EACHAM_HIP_TRY(ctx, hipMemcpyAsync(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, st));
            EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        if (use_groups) hc.n_entries = 0;
        if (hc.n_entries > BA_MAX_PAIR_ENTRIES) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "Schur pair list too large (%lld entries)", hc.n_entries);
        n_entries = (int)hc.n_entries;
        h->n_landmarks_used = hc.n_used;
        D.n_cam_chunks = hc.n_cam_chunks;
        return EACHAM_OK;
    }

    // ---- scratch 1: expansion, sort by camera block, block / chunk tables (the pair lists: only when the groups do not apply) ----
    int pair_lists() {
        const int max_blocks = (int)std::min<long long>(nblk, (long long)n_entries + nc);
        const int max_chunks = n_entries / PAIR_CHUNK + max_blocks + 1;
        uint32_t *ekA, *ekB;
        int *esort_ws, *bcount, *bfirst, *blast;
        prim::I3 *bt, *bs, *bws;
        TRY(ba_scratch_carve(ctx, 1, [&](void* base) {
            Bump b(base);
            ekA = b.take<uint32_t>(n_entries); ekB = b.take<uint32_t>(n_entries); evA = b.take<int2>(n_entries); evB = b.take<int2>(n_entries);
            esort_ws = b.take<int>(prim::radix_ws_ints(n_entries));
            bcount = b.take<int>(nblk); bfirst = b.take<int>(2 * (size_t)nblk); blast = bfirst ? bfirst + nblk : nullptr; bt = b.take<prim::I3>(nblk); bs = b.take<prim::I3>(nblk); bws = b.take<prim::I3>(prim::scan_ws_elems(nblk));
            blocks_tmp = b.take<int4>(max_blocks); chunks_tmp = b.take<int4>(max_chunks);
            return b.off;
        }));
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(bfirst, 0, sizeof(int) * 2 * (size_t)std::max(nblk, 1), st));
        if (no > 0) prep_expand<<<gobs, TPB, 0, st>>>(no, nc, obs_cam, obs_lm, lm_ptr, obs_pos, poff, ekA, evA);
        w_e = prim::radix_sort_pairs<int2>(st, ekA, evA, ekB, evB, n_entries, bits_for(std::max(nblk, 2)), esort_ws);
        if (n_entries > 0) prep_block_runs<<<(unsigned)((n_entries + TPB - 1) / TPB), TPB, 0, st>>>(n_entries, w_e ? ekB : ekA, bfirst, blast);
        const unsigned gblk = (unsigned)((nblk + TPB) / TPB);
        if (nblk > 0) prep_block_counts<<<gblk, TPB, 0, st>>>(nc, nblk, bfirst, blast, bcount, bt);
        prim::exclusive_scan<prim::I3>(st, bt, bs, nblk, bws, &cnt->totals);
        if (nblk > 0) prep_block_fill<<<gblk, TPB, 0, st>>>(nc, nblk, bcount, bs, blocks_tmp, chunks_tmp);
        // ---- read-back 2: the table sizes ----
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        if (hc.totals.a != n_entries) return ctx->fail(EACHAM_ERR_HIP, "BA structure build: %d pair entries counted, %d placed", n_entries, hc.totals.a);
        D.n_blocks = hc.totals.b;
        D.n_chunks = hc.totals.c;
        return EACHAM_OK;
    }

    // One pass of the entries kernel over `ngrid` groups: the general form (it sorts every group's entries) when some landmark
    // sees a camera twice, the sort-free form otherwise. The first pass raises the LDS limit of both passes of the form it takes.
    template <int PASS>
    int launch_grp_entries(int ngrid, prim::I3* counts, const prim::I3* bases, BaChunk* chunks, uint32_t* ent, uint32_t* laneinfo,
                           uint32_t* seg_key, uint32_t* seg_where, int seg_off) {
        const bool general = hg.any_dup != 0;
        const int cap = general ? g_emax : GRP_ENT_PER_ROW * R;   // the kernel's first argument: entries (a power of two) / lanes
        const size_t lds = general ? grp_entries_lds_bytes(cap, R) : grp_entries_fast_lds_bytes(cap, R);
        const auto pass0 = general ? prep_grp_entries<0> : prep_grp_entries_fast<0>;
        const auto pass1 = general ? prep_grp_entries<1> : prep_grp_entries_fast<1>;
        if (PASS == 0) {
            EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)pass0, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)pass1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        (PASS == 0 ? pass0 : pass1)<<<ngrid, GE_THREADS, lds, st>>>(cap, nc, R, gcnt, tg_groups, tg_rowinfo, tg_lmrow, counts, bases, chunks, ent,
                                                                     laneinfo, seg_key, seg_where, seg_off);
        return EACHAM_OK;
    }

    // ---- the landmark-major structure (ba_groups.hpp steps 2-4 on the device), first half: groups, padded per-group arrays,
    // the counting pass over every group's entries ----
    int groups_first() {
        const int nu = hc.n_used, LMAXg = R / 4, R0g = R - std::max(hg.cmax, 4) + 1;
        const int ng_max = hg.cost_total / R0g + 1;
        while (g_emax < GRP_ENT_PER_ROW * R) g_emax <<= 1;
        if (g_emax > GE_MAXE || R > 511) return ctx->fail(EACHAM_ERR_UNSUPPORTED, "group size %d rows is beyond the device construction", R);
        int* tg_lm0;
        prim::I3 *tg_counts, *tg_ws;
        TRY(ba_scratch_carve(ctx, 2, [&](void* base) {
            Bump b(base);
            tg_groups = b.take<BaGroup>(ng_max); tg_lmid = b.take<int>((size_t)ng_max * LMAXg); tg_lmrow = b.take<int>((size_t)ng_max * LMAXg);
            tg_rowinfo = b.take<int2>((size_t)ng_max * R); tg_uv = b.take<double>(2 * (size_t)ng_max * R);
            tg_lm0 = b.take<int>((size_t)ng_max + 2);
            tg_counts = b.take<prim::I3>(ng_max); tg_bases = b.take<prim::I3>(ng_max); tg_ws = b.take<prim::I3>(prim::scan_ws_elems(ng_max));
            return b.off;
        }));
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(tg_groups, 0, sizeof(BaGroup) * (size_t)ng_max, st));
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(tg_lmid, 0xff, sizeof(int) * (size_t)ng_max * LMAXg, st));
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(tg_lmrow, 0, sizeof(int) * (size_t)ng_max * LMAXg, st));
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(tg_rowinfo, 0xff, sizeof(int2) * (size_t)ng_max * R, st));
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(tg_uv, 0, sizeof(double) * 2 * (size_t)ng_max * R, st));
        const uint32_t* g_sorted = w_g ? gvB : gvA;
        const unsigned gnu = (unsigned)((nu + TPB - 1) / TPB);
        if (nu > 0) {
            prep_grp_bounds<<<gnu, TPB, 0, st>>>(nu, gcstart, R0g, tg_lm0, gcnt);
            prep_grp_records<<<(unsigned)((ng_max + TPB - 1) / TPB), TPB, 0, st>>>(gcnt, tg_lm0, grstart, tg_groups);
            prep_grp_fill<<<gnu, TPB, 0, st>>>(nu, nc, R, R0g, g_sorted, gcstart, grstart, tg_lm0, lm_ptr, obs_cam, obs_uv, tg_lmid, tg_lmrow, tg_rowinfo, tg_uv);
        }
        TRY(launch_grp_entries<0>(ng_max, tg_counts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0));
        prim::exclusive_scan<prim::I3>(st, tg_counts, tg_bases, ng_max, tg_ws, &gcnt->totals);
        // ---- read-back 2: groups, chunks, entry rows, segments ----
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(&hg, gcnt, sizeof(hg), hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        if (nu == 0) hg.ng = 0;
        if (hg.ng > ng_max) return ctx->fail(EACHAM_ERR_HIP, "BA structure build: %d groups, %d expected at most", hg.ng, ng_max);
        D.g_rows = R; D.g_ngroups = hg.ng; D.g_nchunks = hg.totals.a; D.g_nent4 = hg.totals.b; D.g_nparts = hg.totals.c;
        n_items = 2 * nc + 1 + hg.totals.c;
        return EACHAM_OK;
    }

    // ---- second half of the landmark-major structure: the writing pass over the groups, the slots, the block table. It needs the
    // group counters only, not the plan: it runs HERE, beside the host's analysis (which has become the longer of the two: 0.65 ms
    // against 0.45 ms of device work from the camera graph's read-back on S200, 1.5 against 0.9 ms on config 4), into staging buffers;
    // what it produced is copied into the arena once the plan has sized it (the 17 MB of entries: ~10 us device to device). Until the
    // second half of round 5 it waited for the join: 0.3 ms of every S200 call with the device idle. ----
    int groups_second() {
        const int ngf = D.g_ngroups;
        TRY(ba_scratch_carve(ctx, 3, [&](void* base) {
            Bump b(base);
            sg_chunks = b.take<BaChunk>(D.g_nchunks); sg_ent = b.take<uint32_t>(256 * (size_t)D.g_nent4); sg_laneinfo = b.take<uint32_t>(64 * (size_t)D.g_nchunks);
            sg_blk = b.take<int4>(n_items); sg_longblk = b.take<int>((size_t)D.g_nparts / GRP_LONG + 1);
            return b.off;
        }));
        uint32_t *ikA, *ikB, *iwA, *iwB;
        int *isort_ws, *blk_first, *longflag, *longpos, *long_ws;
        prim::I3 *ifl, *isc, *iws;
        TRY(ba_scratch_carve(ctx, 1, [&](void* base) {
            Bump b(base);
            ikA = b.take<uint32_t>(n_items); ikB = b.take<uint32_t>(n_items); iwA = b.take<uint32_t>(n_items); iwB = b.take<uint32_t>(n_items);
            isort_ws = b.take<int>(prim::radix_ws_ints(n_items));
            ifl = b.take<prim::I3>(n_items); isc = b.take<prim::I3>(n_items); iws = b.take<prim::I3>(prim::scan_ws_elems(n_items));
            blk_first = b.take<int>(n_items); longflag = b.take<int>(n_items); longpos = b.take<int>(n_items); long_ws = b.take<int>(prim::scan_ws_elems(n_items));
            return b.off;
        }));
        const int n_mand = 2 * nc + 1;
        prep_grp_mandatory<<<(unsigned)((n_mand + TPB - 1) / TPB), TPB, 0, st>>>(nc, ikA, iwA);
        if (ngf > 0) TRY(launch_grp_entries<1>(ngf, nullptr, tg_bases, sg_chunks, sg_ent, sg_laneinfo, ikA, iwA, n_mand));
        const int w_i = prim::radix_sort_pairs<uint32_t>(st, ikA, iwA, ikB, iwB, n_items, bits_for((long long)(nc + 1) * (nc + 1)), isort_ws);
        const uint32_t *skey = w_i ? ikB : ikA, *swhere = w_i ? iwB : iwA;
        const unsigned git = (unsigned)((n_items + TPB - 1) / TPB);
        prep_grp_flags<<<git, TPB, 0, st>>>(n_items, skey, swhere, ifl);
        prim::exclusive_scan<prim::I3>(st, ifl, isc, n_items, iws, &gcnt->item_totals);
        prep_grp_slots<<<git, TPB, 0, st>>>(n_items, nc, skey, swhere, isc, sg_laneinfo, sg_blk, blk_first);
        prep_grp_blk_counts<<<git, TPB, 0, st>>>(gcnt, n_items, swhere, blk_first, sg_blk, longflag);
        prim::exclusive_scan<int>(st, longflag, longpos, n_items, long_ws, &gcnt->n_long);
        prep_grp_long<<<git, TPB, 0, st>>>(gcnt, longflag, longpos, sg_longblk);
        // ---- read-back 3: blocks, long blocks ----
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(&hg, gcnt, sizeof(hg), hipMemcpyDeviceToHost, st));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));
        D.g_nblk = hg.item_totals.b; D.g_nlong = hg.n_long;
        return EACHAM_OK;
    }

    // What the stages left in scratch and arena B takes over, each named ONCE: f(destination in BaDev, staged source, elements).
    // second_arena walks the list twice: its layout carves the destinations in this order, then the copies fill them in it.
    template <class F>
    int staged_arrays(F f) {
        const size_t ngf = (size_t)D.g_ngroups, LMAXg = (size_t)R / 4;
        TRY(f(D.pair_entries, w_e ? evB : evA, (size_t)n_entries));
        TRY(f(D.pair_chunks, chunks_tmp, (size_t)D.n_chunks));
        TRY(f(D.blocks, blocks_tmp, (size_t)D.n_blocks));
        if (!use_groups) return EACHAM_OK;
        TRY(f(D.g_groups, tg_groups, ngf));
        TRY(f(D.g_lmid, tg_lmid, ngf * LMAXg));
        TRY(f(D.g_lmrow, tg_lmrow, ngf * LMAXg));
        TRY(f(D.g_rowinfo, tg_rowinfo, ngf * R));
        TRY(f(D.g_uv, tg_uv, 2 * ngf * R));
        TRY(f(D.g_chunks, sg_chunks, (size_t)D.g_nchunks));
        TRY(f(D.g_ent, sg_ent, 256 * (size_t)D.g_nent4));
        TRY(f(D.g_laneinfo, sg_laneinfo, 64 * (size_t)D.g_nchunks));
        TRY(f(D.g_blk, sg_blk, (size_t)n_items));                          // (blocks <= items)
        TRY(f(D.g_longblk, sg_longblk, (size_t)D.g_nparts / GRP_LONG + 1));  // (a long block holds more than GRP_LONG segments)
        return EACHAM_OK;
    }

    // ---- the join with the plan thread; arena B: the pair lists, the groups, the plan's tables, what is sized by them ----
    int second_arena() {
        h->prep_us[0] = us_since(t_begin);
        if (guard.plan_thread.joinable()) guard.plan_thread.join();  // prep_us[1] = the plan's own time; what of it was not hidden behind the device shows in [2]
        if (plan_failed) return ctx->fail(EACHAM_ERR_HIP, "BA preparation: the analysis of the reduced system ran out of memory or threads");
        const auto t_upload = std::chrono::steady_clock::now();
        const std::vector<int2> bs_ent = ba_plan_to_dev(h);
        size_t plan_lo = 0, plan_hi = 0;   // the plan's eleven tables in the arena: sent as ONE copy of their host image
        auto layout_b = [&]() -> int {
            TRY(staged_arrays([&](auto& dst, auto* src, size_t n) {
                dst = h->arena.take<std::remove_pointer_t<decltype(src)>>(n);
                return EACHAM_OK;
            }));
            plan_lo = h->arena.off;
            TRY(ba_upload_plan(ctx, h, h->plan, bs_ent));
            plan_hi = h->arena.off;
            TRY(ba_alloc_work_b(ctx, h));
            return EACHAM_OK;
        };
        TRY(ba_arena_layout(ctx, h, &h->block2, layout_b, [&] { return std::make_pair(plan_lo, plan_hi); }));
        TRY(staged_arrays([&](auto& dst, auto* src, size_t n) -> int {   // what the stages staged -> the arena
            if (n > 0) EACHAM_HIP_TRY(ctx, hipMemcpyAsync((void*)dst, src, sizeof(*src) * n, hipMemcpyDeviceToDevice, st));
            return EACHAM_OK;
        }));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(st));  // the plan's tables were copied out of host vectors
        h->prep_us[2] = us_since(t_upload);
        return EACHAM_OK;
    }
};

static int ba_prepare_device(eacham_ctx* ctx, const eacham_ba_problem* P, int hint, eacham_ba_handle** out) {
    if ((long long)P->n_cams * (P->n_cams + 1) / 2 > BA_MAX_CAM_BLOCKS_DEVICE)
        return ctx->fail(EACHAM_ERR_UNSUPPORTED, "too many cameras (%d) for the camera-block index", P->n_cams);
    BaDevicePrep S(ctx, P, hint);
    TRY(S.first_arena());
    TRY(S.structure());
    TRY(S.plan_and_counts());
    TRY(S.use_groups ? S.groups_first() : S.pair_lists());
    if (S.use_groups) TRY(S.groups_second());
    TRY(S.second_arena());
    *out = S.guard.release();
    return EACHAM_OK;
}

// One entry for both constructions: the problem and the ordering hint are checked here, once.
int ba_prepare(eacham_ctx* ctx, const eacham_ba_problem* P, eacham_ba_handle** out) {
    if (!P || P->n_cams < 0 || P->n_points < 0 || P->n_obs < 0) return ctx->fail(EACHAM_ERR_INVALID, "bad BA problem");
    if (P->n_obs > 0 && (!P->obs_cam || !P->obs_point || !P->obs_uv)) return ctx->fail(EACHAM_ERR_INVALID, "null observation arrays");
    if ((P->n_cams > 0 && (!P->cam_T_wc || !P->cam_fixed)) || (P->n_points > 0 && (!P->points || !P->point_observers)))
        return ctx->fail(EACHAM_ERR_INVALID, "null camera/point arrays");
    int hint = 0;
    TRY(ba_ordering_hint(ctx, P, &hint));
    // a local window (the reference's per-frame call, ~10 k observations) is cheaper through the host loops: the device
    // construction is ~45 dependent launches and three read-backs whatever the size. (Which form of the Schur stage serves:
    // ba_groups_wanted — the landmark groups or the pair lists.)
    const bool device = ctx->ba_prepare_mode == 2 || (ctx->ba_prepare_mode == 0 && P->n_obs >= 65536);
    return device ? ba_prepare_device(ctx, P, hint, out) : ba_prepare_host(ctx, P, hint, out);
}
#undef TRY

void ba_release(eacham_ctx* ctx, eacham_ba_handle* h) {
    if (!h) return;
    (void)hipStreamSynchronize(ctx->stream);
    ba_handle_free(ctx, h);
}

}  // namespace eacham

extern "C" {

int eacham_ba_prepare(eacham_ctx* ctx, const eacham_ba_problem* problem, eacham_ba_handle** out_handle) {
    if (!ctx || !out_handle) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    *out_handle = nullptr;
    return ba_prepare(ctx, problem, out_handle);
}

int eacham_ba_get_plan_info(eacham_ctx* ctx, const eacham_ba_handle* handle, eacham_ba_plan_info* out) {
    if (!ctx || !handle || !out) return EACHAM_ERR_INVALID;
    const BaPlan& pl = handle->plan;
    out->n_panels = pl.npan; out->n_tiles = pl.ntiles; out->n_levels = pl.n_levels;
    out->ordering = pl.ordering; out->nd_leaf = pl.nd_leaf; out->reserved = 0;
    out->tile_updates = pl.tile_updates;
    out->est_us = pl.est_us;
    out->prepare_us[0] = handle->prep_us[0];
    out->prepare_us[1] = handle->prep_us[1];
    out->prepare_us[2] = handle->prep_us[2];
    return EACHAM_OK;
}

int eacham_ba_debug_structure(eacham_ctx* ctx, const eacham_ba_handle* h, int which, void* out, int64_t cap_bytes, int64_t* out_bytes) {
    if (!ctx || !h || !out_bytes) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    const BaDev& D = h->D;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case 0: src = D.lm_ptr; bytes = sizeof(int) * ((size_t)D.nl + 1); break;
        case 1: src = D.cam_ptr; bytes = sizeof(int) * ((size_t)D.nc + 1); break;
        case 2: src = D.cam_obs; bytes = sizeof(int) * (size_t)D.no; break;
        case 3: src = D.obs_pos; bytes = sizeof(int) * (size_t)D.no; break;
        case 4: src = D.obs_cam; bytes = sizeof(unsigned) * (size_t)D.no; break;
        case 5: src = D.obs_lm; bytes = sizeof(unsigned) * (size_t)D.no; break;
        case 6: src = D.obs_uv; bytes = sizeof(double) * 2 * (size_t)D.no; break;
        case 7: src = D.cam_uv; bytes = sizeof(double) * 2 * (size_t)D.no; break;
        case 8: src = D.cam_lm; bytes = sizeof(int) * (size_t)D.no; break;
        case 9: src = D.pos_cam; bytes = sizeof(int) * (size_t)D.no; break;
        case 10: src = D.cam_chunks; bytes = sizeof(int2) * (size_t)D.n_cam_chunks; break;
        case 11: src = D.cam_chunk_ptr; bytes = sizeof(int) * ((size_t)D.nc + 1); break;
        case 12: src = D.blocks; bytes = sizeof(int4) * (size_t)D.n_blocks; break;
        case 13: src = D.pair_chunks; bytes = sizeof(int4) * (size_t)D.n_chunks; break;
        case 14: {
            long long n = 0;  // entries = first entry + count of the last chunk
            if (D.n_chunks > 0) {
                int4 last;
                EACHAM_HIP_TRY(ctx, hipMemcpy(&last, D.pair_chunks + (D.n_chunks - 1), sizeof(int4), hipMemcpyDeviceToHost));
                n = (long long)last.y + last.z;
            }
            src = D.pair_entries; bytes = sizeof(int2) * (size_t)n;
            break;
        }
        case 15: src = D.pose0; bytes = sizeof(double) * 12 * (size_t)D.nc; break;
        case 16: src = D.pt0; bytes = sizeof(double) * 3 * (size_t)D.nl; break;
        case 17: src = D.lmprior; bytes = sizeof(double) * 2 * (size_t)D.nl; break;
        case 18: src = D.K0; bytes = sizeof(double) * 5; break;
        case 19: src = D.fixed; bytes = sizeof(int) * (size_t)D.nc; break;
        // the landmark-major structure of the Schur stage (ba_groups.hpp); all empty when the pair lists serve
        case 20: src = D.g_groups; bytes = D.g_rows ? sizeof(BaGroup) * (size_t)D.g_ngroups : 0; break;
        case 21: src = D.g_lmid; bytes = D.g_rows ? sizeof(int) * (size_t)D.g_ngroups * (D.g_rows / 4) : 0; break;
        case 22: src = D.g_lmrow; bytes = D.g_rows ? sizeof(int) * (size_t)D.g_ngroups * (D.g_rows / 4) : 0; break;
        case 23: src = D.g_rowinfo; bytes = D.g_rows ? sizeof(int2) * (size_t)D.g_ngroups * D.g_rows : 0; break;
        case 24: src = D.g_uv; bytes = D.g_rows ? sizeof(double) * 2 * (size_t)D.g_ngroups * D.g_rows : 0; break;
        case 25: src = D.g_ent; bytes = D.g_rows ? sizeof(uint32_t) * 256 * (size_t)D.g_nent4 : 0; break;
        case 26: src = D.g_chunks; bytes = D.g_rows ? sizeof(BaChunk) * (size_t)D.g_nchunks : 0; break;
        case 27: src = D.g_laneinfo; bytes = D.g_rows ? sizeof(uint32_t) * 64 * (size_t)D.g_nchunks : 0; break;
        case 28: src = D.g_blk; bytes = D.g_rows ? sizeof(int4) * (size_t)D.g_nblk : 0; break;
        case 29: src = D.g_longblk; bytes = D.g_rows ? sizeof(int) * (size_t)D.g_nlong : 0; break;
        default: return ctx->fail(EACHAM_ERR_INVALID, "unknown structure array %d", which);
    }
    *out_bytes = (int64_t)bytes;
    if ((int64_t)bytes > cap_bytes) return ctx->fail(EACHAM_ERR_CAPACITY, "structure array %d needs %zu bytes", which, bytes);
    EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) EACHAM_HIP_TRY(ctx, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return EACHAM_OK;
}

}  // extern "C"
