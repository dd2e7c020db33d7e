// ba_dev.hpp — what the two halves of the bundle adjustment share: ba.hip (the Levenberg-Marquardt solver, every kernel of an
// iteration) and ba_prepare.hip (eacham_ba_prepare: the problem's structure and its device arrays). The device-side view of a
// prepared problem (BaDev), the handle, the carving of a problem's arrays out of its arena, and the functions that cross the seam.
#pragma once

#include "context.hpp"
#include "ba_plan.hpp"
#include "ba_groups.hpp"
#include "ws_carve.hpp"

#include <cstring>
#include <vector>

namespace eacham {

// ---- noise parameters with the reference's float arithmetic (BundleAdjuster.cpp:28-33) ----------
inline double rot_sigma_host(float deg) { return (double)(deg * 3.141592f / 180.0f); }
struct Noise {
    double pose_sigma[6], fixed_sigma[6];
    double pose_huber, pix_sigma, pix_huber;
    double k_sigma[5];
};
inline Noise make_noise() {
    Noise nz;
    for (int k = 0; k < 3; ++k) {
        nz.pose_sigma[k] = rot_sigma_host(45.0f);
        nz.pose_sigma[3 + k] = (double)0.35f;
        nz.fixed_sigma[k] = rot_sigma_host(0.0001f);
        nz.fixed_sigma[3 + k] = (double)0.0001f;
    }
    nz.pose_huber = (double)2.5f;
    nz.pix_sigma = (double)1.5f;
    nz.pix_huber = (double)3.0f;
    const double ks[5] = {25, 25, 0.00001, 0.0001, 0.0001};
    for (int k = 0; k < 5; ++k) nz.k_sigma[k] = ks[k];
    return nz;
}

constexpr int TPB = 256;           // threads per block of the streaming kernels
constexpr int SCAL = 16;           // scalar block read back per try

// ---- device-side view of a prepared problem --------------------------------------------------------
struct BaDev {
    int nc, nl, no, n;          // n = 6 nc + 5
    // the reduced system in tiles (ba_plan.hpp): camera c starts at padded column sp_pos[c], K at sp_posK, the
    // right-hand side is row sp_rhs_row (row 63 of the root panel); sp_tile_map[I (I + 1) / 2 + J] = tile of (I >= J)
    int sp_npan, sp_ntiles, sp_posK, sp_rhs_row, sp_n_pad;
    const int *sp_pos, *sp_tile_map, *sp_pad_cols, *sp_diag_tile;
    double *T, *Xrow, *zsol;    // tiles [sp_ntiles][64][64]; X of every panel row-major; z of the back-substitution
    // values
    double *pose, *pose0, *pose_new, *pt, *pt0, *pt_new, *Kc, *K0, *K_new;  // Kc: fx fy s u0 v0
    const int* fixed;
    const double* lmprior;  // [nl][2] sigma, k
    // structure
    const int *lm_ptr, *cam_ptr, *cam_obs;
    const int2* cam_chunks; // camera-aligned chunks of <= TPB positions {first, count}; cam_chunk_ptr[c] .. [c+1] = camera c's
    const int* cam_chunk_ptr;
    int n_cam_chunks;
    const int* cam_lm;      // landmark of cam_obs[p], camera order: one hop less in the per-camera gathers
    const int* pos_cam;     // camera of position p (camera order)
    int store_E;            // 1: the linearisation keeps E (DogLeg reads it); 0: the E -> Et kernel recomputes it
    const int* obs_pos;     // inverse of cam_obs: Et is stored in CAMERA order (record of observation o at obs_pos[o])
    const double* cam_uv;   // measurement of cam_obs[p], camera order
    const unsigned *obs_cam, *obs_lm;
    const double* obs_uv;
    const int2* pair_entries;
    const int4* pair_chunks;  // {block id, first entry, count, chunk index within block}
    const int4* blocks;       // {c, c', first chunk, n chunks}
    int n_chunks, n_blocks;
    // the landmark-major form of the Schur stage (ba_groups.hpp; g_rows == 0: the pair lists above serve)
    int g_rows, g_ngroups, g_nblk, g_nparts, g_nchunks, g_nlong;
    long long g_nent4;
    const BaGroup* g_groups;
    const int *g_lmid, *g_lmrow;    // [group][rows / 4]: landmark t of the group (-1: none), local row of its own row
    const int2* g_rowinfo;          // [group][rows]: {camera (nc: a landmark's own row, -1: no row), landmark index inside the group}
    const double* g_uv;             // [group][rows][2]
    const BaChunk* g_chunks;        // {first uint4-row of the chunk's entries, steps of 4 entries}
    const uint32_t* g_ent;          // [uint4-row][lane][4]: r1 | r2 << 16, local rows (null row = g_rows)
    const uint32_t* g_laneinfo;     // [chunk][lane]: lanes after this one in its segment << 28 | (slot + 1 at a segment's first lane)
    const int4* g_blk;              // {c1, c2 (nc = the calibration / right-hand-side pseudo-camera), first slot, count}
    const int* g_longblk;           // blocks with more than GRP_LONG partials
    // linearisation
    double *E, *lmlin, *camlin, *klin;
    // per try
    double *Et, *lmtry, *Winv, *Wops, *partial, *kk_part, *delta_c, *delta_l, *err_part, *lin_part, *scal;
    // DogLeg: Gauss-Newton step (cameras+K | landmarks) and per-block partial sums of the six forms
    double *dl_nc, *dl_nl, *dl_part;
    double* bpart;  // [n_cam_chunks][36] partial border sums
    // PCG + block-Jacobi (use_preconditioner): x = delta_c | delta_l; r, z, p, q over [cameras + K | landmarks];
    // inverse diagonal blocks Mc (36 per camera), MK (25), Ml (9 per landmark); damping diagonals Dc, Dl;
    // pcg_p1 [n_lm_blocks][6], pcg_p2 [n_cam_chunks][6], pcg_p3 [n_lm_blocks + 1] partial sums;
    // pcg_s = {gamma, threshold, alpha, beta, done, iterations, p.q}
    double *pcg_rc, *pcg_rl, *pcg_zc, *pcg_zl, *pcg_pc, *pcg_pl, *pcg_qc, *pcg_ql, *pcg_Mc, *pcg_MK, *pcg_Ml, *pcg_Dc, *pcg_Dl,
        *pcg_p1, *pcg_p2, *pcg_p3, *pcg_s;
    int* flags;
    double* scal_pinned;  // device view of the pinned host copy of scal[0..2] (final_sums)
    int* sync_counter;    // ticket counter of the "last workgroup makes the final sums" hand-over (self-resetting)
    int n_lm_blocks;  // grid of the per-landmark kernels
    // Small problems (a local window: 1.5 k landmarks = six workgroups) are bound by the LENGTH of a thread's instruction
    // stream, not by bandwidth: a landmark's ~8 observations cost ~3 k fp64 instructions in one lane, ~10 us per kernel
    // whatever the landmark count. There the three kernels that loop over a landmark's observations spread it over
    // lpl = 8 adjacent lanes (observation o0 + sub, o0 + sub + 8, ...; xor-shuffle sums in a fixed order), on a grid of
    // n_ll_blocks workgroups; large problems use lpl = 2 (50 k landmarks are 782 waves on 1024 SIMDs with one lane each).
    int lpl, n_ll_blocks;
    // the same idea for the kernels of the step's tail (back-substitution + error: two passes of dependent gathers per
    // observation): their own lanes-per-landmark count and grid (measured on S200 / config 4: 2 lanes 35.6 / 72 us,
    // 1 lane 41.7 / 75, 4 lanes 41.8 / 71, 8 lanes 55 / 92)
    int lpl_step, n_step_blocks;
    Noise nz;
};

}  // namespace eacham

struct eacham_ba_handle {
    eacham::BaDev D;
    int block = -1;            // index into ctx->ba_pool: the arena all device arrays of this problem live in
    int block2 = -1;           // device-built problems: a second arena for what is sized by the pair lists and the plan
    eacham::Bump arena{nullptr};  // the arena being carved (ba_arena_layout). A null base is the planning pass: sizes only, off = the total
    size_t upload_end = 0;     // end of the last uploaded array in the arena (the uploads come first in the sequence)
    std::vector<char> stage;   // host image of uploaded arrays [stage_base, stage_base + size) of the arena, sent with ONE copy
    size_t stage_base = 0;
    std::vector<int> lm_order;  // landmark-sorted observation index -> caller's observation index
    eacham::BaGroups groups;    // host-built problems: the landmark-major structure of the Schur stage (device-built: sizes only)
    double *kpart = nullptr, *err_cam = nullptr, *lin_cam = nullptr;
    bool finish_pending = false;  // the linearisation's second stage has not run yet: the next try's first launch carries it
    double* scal_host = nullptr;  // pinned: the per-try scalar read-back sits on the LM loop's critical path
    long long ticket = 0;         // number of the last ba_final_sums launch (it stores it behind the scalars)
    double *pose_init = nullptr, *pt_init = nullptr, *K_init = nullptr;
    int n_landmarks_used = 0;
    // the sparse solve (ba_plan.hpp): the plan stays on the host for the launch sequence and the diagnostic read-back
    eacham::BaPlan plan;
    double prep_us[3] = {0, 0, 0};  // eacham_ba_prepare: host structures | the plan (ordering + symbolic) | arena + upload + sync
    const int* sp_leaves = nullptr;
    const eacham::BaPlanItem* sp_items = nullptr;
    const eacham::BaPlanSrc* sp_srcs = nullptr;
    const int *bs_order = nullptr, *bs_ptr = nullptr, *sp_col_dest = nullptr;
    const int2* bs_ent = nullptr;
};

namespace eacham {

// The next array of the allocation sequence running over h->arena (ba_arena_layout in ba_prepare.hip runs every sequence twice).
template <class T>
inline void dev_alloc(eacham_ba_handle* h, T** p, size_t count) {
    *p = h->arena.take<T>(count);
}
// ... filled from a host vector: through the host image h->stage where the array lies inside it, else by a copy of its own.
template <class T>
inline int dev_upload(eacham_ctx* ctx, eacham_ba_handle* h, const T** p, const std::vector<T>& v) {
    T* q = nullptr;
    dev_alloc(h, &q, v.size());
    if (!h->arena.base) {
        h->upload_end = h->arena.off;
    } else if (!v.empty()) {
        const size_t off = (size_t)((char*)q - h->arena.base);
        if (!h->stage.empty() && off >= h->stage_base && off + v.size() * sizeof(T) <= h->stage_base + h->stage.size())
            memcpy(h->stage.data() + (off - h->stage_base), v.data(), v.size() * sizeof(T));
        else EACHAM_HIP_TRY(ctx, hipMemcpyAsync(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    }
    *p = q;
    return EACHAM_OK;
}
template <class T, class U>
inline int dev_upload_as(eacham_ctx* ctx, eacham_ba_handle* h, const T** p, const std::vector<U>& v) {  // same-layout PODs (GrpI2 = int2, ...)
    static_assert(sizeof(T) == sizeof(U), "layout");
    return dev_upload(ctx, h, p, reinterpret_cast<const std::vector<T>&>(v));
}

// ---- across the seam ----
// ba.hip, called inside the allocation sequences of ba_prepare.hip: the solver's work arrays sized by (cameras, landmarks,
// observations), then those sized by the plan and the Schur form (with the clears and the LDS grant that go with them)
int ba_alloc_work_a(eacham_ctx* ctx, eacham_ba_handle* h);
int ba_alloc_work_b(eacham_ctx* ctx, eacham_ba_handle* h);
// ba_prepare.hip: a problem checked and built by the form its size selects; the handle given back to the context's pool
int ba_prepare(eacham_ctx* ctx, const eacham_ba_problem* P, eacham_ba_handle** out);
void ba_release(eacham_ctx* ctx, eacham_ba_handle* h);

}  // namespace eacham
