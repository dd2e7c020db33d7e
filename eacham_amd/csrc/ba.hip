// ba.hip — Levenberg-Marquardt bundle adjustment for gfx950 (MI355X), all fp64.
//
// Replaces the GTSAM part of   RefineBA   modules/sfm/reconstruction/BundleAdjuster.cpp:40-250
//   factors + noise models (:57-121, :171-178), LevenbergMarquardtOptimizer::optimize (:182-216),
//   graph.error (:218-219). Semantics follow SURVEY.md Appendix A (GTSAM 4.1.1, Ceres-default LM,
//   first-order Pose3 chart with the Cayley map on Rot3).
//
// Layout in HBM (everything resident for the whole LM loop; only scalars cross PCIe per try):
//   cameras   pose[nc][12] = R (camera->world, row-major) | t          prior means pose0
//   points    pt[nl][3], prior means pt0, lmprior[nl][2] = {sigma, huber k}
//   obs       grouped by landmark (CSR lm_ptr): obs_cam[no], obs_uv[no][2]; a second CSR
//             (cam_ptr, cam_obs) lists each camera's observations, with camera-ordered copies of their
//             landmark ids / measurements (cam_lm, cam_uv) and the inverse map obs_pos; the per-observation
//             blocks E and Et are stored in CAMERA order (a camera's records are contiguous)
//   pairs     for every camera block (c <= c') the list of observation pairs (o, o') of one landmark
//             seen by both: the sparsity structure of the Schur complement, built once per problem
// Linear algebra of one damped step (H + lambda diag(clamp(diag H))) delta = g:
//   landmarks are eliminated first (3x3 blocks, one thread each), the reduced camera system
//   S (n = 6 nc + 5, the 5 shared-calibration columns are a dense border) is assembled WITHOUT
//   atomics — every block is a deterministic sequential sum over its pair list — into 64x64 TILES of the symbolic
//   pattern of its Cholesky factor under a fill-reducing camera ordering (ba_plan.hpp: what GTSAM's multifrontal solver
//   with COLAMD does for the reference, BundleAdjuster.cpp:182-190), factorised level by level of the elimination tree
//   on v_mfma_f64_16x16x4_f64 (64 columns per panel, the two 32x32 diagonal blocks of a panel factorised by one wave
//   each) with the right-hand side carried as a row of the root panel, and the landmark steps follow by back-substitution.
// Roofline: every kernel except the dense factorisation streams observation-sized arrays once
// (HBM-bound); see DESIGN.md for the per-kernel byte counts.
//
// This file is the solver: every kernel of an LM iteration, the launch sequence of a try, the LM / DogLeg loop and its entry
// points. The problem itself (eacham_ba_prepare: structure, arenas, plan upload) is built by ba_prepare.hip; ba_dev.hpp holds
// what the two share.
#include "ba_dev.hpp"

#include <cstdlib>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

namespace eacham {

constexpr int NB = 32;             // Cholesky block size
constexpr int PB = 2 * NB;         // columns of a panel: what one workgroup factorises per launch (sp_level)
constexpr int LMLIN = 24;          // per-landmark linearisation: Hll(6) gl(3) ElK(15)
constexpr int CAMLIN = 72;         // per-camera: Hcc(36) HcK(30) gc(6)
constexpr int KLIN = 30;           // HKK(25) gK(5)
constexpr int N_STATUS = 4;        // flags[0..3] status, flags[4 + P] = hand-off flag of panel P (back-substitution)

typedef double mfma_d4 __attribute__((ext_vector_type(4)));  // accumulator of v_mfma_f64_16x16x4_f64: D[(lane >> 4) + 4 reg][lane & 15]

__device__ __forceinline__ void wave_lds_sync() {  // a wave's own LDS region: order its writes before its reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double huber_weight(double n, double k) { return n <= k ? 1.0 : k / n; }
__device__ __forceinline__ double huber_loss(double n, double k) { return n <= k ? 0.5 * n * n : k * (n - 0.5 * k); }
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// GeneralSFMFactor2<Cal3_S2>::evaluateError. pose = R(9) t(3) camera->world.
// Returns false on a cheirality failure: residual and Jacobians are zero.
template <bool JAC>
__device__ __forceinline__ bool reproj(const double* __restrict__ x, const double* __restrict__ l,
                                       const double* __restrict__ K, double mu, double mv, double* r,
                                       double* Jp, double* Jl, double* Jk) {
    const double dx = l[0] - x[9], dy = l[1] - x[10], dz = l[2] - x[11];
    const double qx = x[0] * dx + x[3] * dy + x[6] * dz;
    const double qy = x[1] * dx + x[4] * dy + x[7] * dz;
    const double qz = x[2] * dx + x[5] * dy + x[8] * dz;
    if (qz <= 0.0) {
        r[0] = r[1] = 0.0;
        if (JAC) {
            for (int k = 0; k < 12; ++k) Jp[k] = 0.0;
            for (int k = 0; k < 6; ++k) Jl[k] = 0.0;
            for (int k = 0; k < 10; ++k) Jk[k] = 0.0;
        }
        return false;
    }
    const double d = 1.0 / qz, u = qx * d, v = qy * d;
    const double fx = K[0], fy = K[1], s = K[2];
    r[0] = fx * u + s * v + K[3] - mu;
    r[1] = fy * v + K[4] - mv;
    if (JAC) {
        const double Dn[12] = {u * v, -1 - u * u, v, -d, 0, d * u, 1 + v * v, -u * v, -u, 0, -d, d * v};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            Jp[j] = fx * Dn[j] + s * Dn[6 + j];
            Jp[6 + j] = fy * Dn[6 + j];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double a0 = d * (x[3 * j] - u * x[3 * j + 2]);
            const double a1 = d * (x[3 * j + 1] - v * x[3 * j + 2]);
            Jl[j] = fx * a0 + s * a1;
            Jl[3 + j] = fy * a1;
        }
        Jk[0] = u; Jk[1] = 0; Jk[2] = v; Jk[3] = 1; Jk[4] = 0;
        Jk[5] = 0; Jk[6] = v; Jk[7] = 0; Jk[8] = 0; Jk[9] = 1;
    }
    return true;
}

// whitened + Huber-reweighted Jacobian factor of one observation (Robust::WhitenSystem)
__device__ __forceinline__ void obs_factor(const double* x, const double* l, const double* K, double mu,
                                           double mv, double sig, double kh, double* Ap, double* Al,
                                           double* Ak, double* b) {
    double r[2];
    reproj<true>(x, l, K, mu, mv, r, Ap, Al, Ak);
    const double e0 = r[0] / sig, e1 = r[1] / sig;
    const double sw = sqrt(huber_weight(sqrt(e0 * e0 + e1 * e1), kh)), sc = sw / sig;
#pragma unroll
    for (int k = 0; k < 12; ++k) Ap[k] *= sc;
#pragma unroll
    for (int k = 0; k < 6; ++k) Al[k] *= sc;
#pragma unroll
    for (int k = 0; k < 10; ++k) Ak[k] *= sc;
    b[0] = -sw * e0;
    b[1] = -sw * e1;
}

// deterministic block-wide sum of NV values per thread: result valid in thread 0 (out[0..NV))
template <int NV>
__device__ __forceinline__ void block_sum(double* v, double* smem /* [TPB/64][NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double x = v[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        v[i] = x;
    }
    if (lane == 0)
        for (int i = 0; i < NV; ++i) smem[wave * NV + i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < NV; ++i) {
            double s = 0.0;
            for (int w = 0; w < TPB / 64; ++w) s += smem[w * NV + i];
            v[i] = s;
        }
    }
    __syncthreads();
}

// ---- Cayley chart --------------------------------------------------------
__device__ __forceinline__ void cayley(const double* w, double* R) {
    const double x = w[0], y = w[1], z = w[2];
    const double x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
    const double f = 1.0 / (4.0 + x2 + y2 + z2), f2 = 2.0 * f;
    R[0] = (4 + x2 - y2 - z2) * f; R[1] = (xy - 2 * z) * f2;      R[2] = (xz + 2 * y) * f2;
    R[3] = (xy + 2 * z) * f2;      R[4] = (4 - x2 + y2 - z2) * f; R[5] = (yz - 2 * x) * f2;
    R[6] = (xz - 2 * y) * f2;      R[7] = (yz + 2 * x) * f2;      R[8] = (4 - x2 - y2 + z2) * f;
}
// xi = Local(x, prior): chart coordinates of x^-1 * prior
__device__ __forceinline__ void pose_local(const double* x, const double* p, double* xi) {
    double Rd[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rd[3 * i + j] = x[i] * p[j] + x[3 + i] * p[3 + j] + x[6 + i] * p[6 + j];
    const double s = 2.0 / (1.0 + Rd[0] + Rd[4] + Rd[8]);
    xi[0] = s * (Rd[7] - Rd[5]);
    xi[1] = s * (Rd[2] - Rd[6]);
    xi[2] = s * (Rd[3] - Rd[1]);
    const double dt0 = p[9] - x[9], dt1 = p[10] - x[10], dt2 = p[11] - x[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) xi[3 + i] = x[i] * dt0 + x[3 + i] * dt1 + x[6 + i] * dt2;
}

// sum over the LPL adjacent lanes that share a landmark, the same value in all of them (fixed butterfly order)
template <int LPL>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = 1; m < LPL; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// ---- K-A: per-landmark linearisation (thread = landmark) --------------------------------------------
// Hll, gl, ElK of the landmark (+ its prior) and E_o = Ap^T Al (6x3) of each of its observations.
template <int LPL>
__device__ __forceinline__ void linearize_landmark(const BaDev& D, int gid) {
    const int j = gid / LPL, sub = gid % LPL;
    if (j >= D.nl) return;  // (the LPL lanes of a landmark leave together)
    const int o0 = D.lm_ptr[j], o1 = D.lm_ptr[j + 1];
    double* out = D.lmlin + (size_t)LMLIN * j;
    double H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, EK[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) EK[k] = 0.0;
    const double l[3] = {D.pt[3 * j], D.pt[3 * j + 1], D.pt[3 * j + 2]};
    double K[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) K[k] = D.Kc[k];
    for (int o = o0 + sub; o < o1; o += LPL) {
        const double* x = D.pose + 12 * (size_t)D.obs_cam[o];
        double xr[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) xr[k] = x[k];
        double Ap[12], Al[6], Ak[10], b[2];
        obs_factor(xr, l, K, D.obs_uv[2 * (size_t)o], D.obs_uv[2 * (size_t)o + 1], D.nz.pix_sigma, D.nz.pix_huber, Ap, Al, Ak, b);
        H[0] += Al[0] * Al[0] + Al[3] * Al[3];
        H[1] += Al[0] * Al[1] + Al[3] * Al[4];
        H[2] += Al[0] * Al[2] + Al[3] * Al[5];
        H[3] += Al[1] * Al[1] + Al[4] * Al[4];
        H[4] += Al[1] * Al[2] + Al[4] * Al[5];
        H[5] += Al[2] * Al[2] + Al[5] * Al[5];
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] += Al[a] * b[0] + Al[3 + a] * b[1];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) EK[3 * a + c] += Ak[a] * Al[c] + Ak[5 + a] * Al[3 + c];
        if (D.store_E) {
            double* E = D.E + 18 * (size_t)D.obs_pos[o];  // camera order
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) E[3 * a + c] = Ap[a] * Al[c] + Ap[6 + a] * Al[3 + c];
        }
    }
    if (LPL > 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) H[k] = group_sum<LPL>(H[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = group_sum<LPL>(g[k]);
#pragma unroll
        for (int k = 0; k < 15; ++k) EK[k] = group_sum<LPL>(EK[k]);
        if (sub != 0) return;
    }
    if (o1 > o0) {  // PriorFactor<Point3>, Robust(Huber(3/obs), Isotropic(1/obs))
        const double sg = D.lmprior[2 * j], kh = D.lmprior[2 * j + 1];
        double e[3], n2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            e[a] = (l[a] - D.pt0[3 * j + a]) / sg;
            n2 += e[a] * e[a];
        }
        const double sw = sqrt(huber_weight(sqrt(n2), kh)), w = sw / sg;
        H[0] += w * w; H[3] += w * w; H[5] += w * w;
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] += w * (-sw * e[a]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = H[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[6 + k] = g[k];
#pragma unroll
    for (int k = 0; k < 15; ++k) out[9 + k] = EK[k];
}

// ---- K-B: per-camera linearisation (block = one of LSEG segments of a camera's observations) ----------
// Every observation contributes two whitened Jacobian rows r = [Ap (6) | Ak (5) | b] (12 entries) and the camera's
// blocks are the 12 x 12 Gram matrix sum_rows r^T r: Hcc = [0:6, 0:6], HcK = [0:6, 6:11], gc = [0:6, 11],
// the camera's share of HKK = [6:11, 6:11] and of gK = [6:11, 11]. The sum over observations is the K dimension of
// v_mfma_f64_16x16x4_f64 (D += R^T R, four rows per instruction; the same register is the A and the B operand), so
// there is no block-wide reduction of 77 per-thread sums any more — those shuffle trees, not the arithmetic or the
// gathers, were the kernel's time (35 us on S200 with one block per camera, more with four). A wave stages the
// rows of 32 observations at a time in its own LDS region as 64 rows x 16 doubles (padding columns zero): the
// operand of step t is then lds[64 t + lane], one conflict-free 512-byte read.
// -> clpart[(c * LSEG + seg)][256] = the block's 16 x 16 accumulator (waves added in order).
constexpr int LSEG = 4;     // segments per camera
constexpr int CLP = 256;    // 16 x 16 accumulator image per (camera, segment)
__device__ __forceinline__ void linearize_camera_segment(const BaDev& D, double* __restrict__ clpart, int block) {
    __shared__ __attribute__((aligned(16))) double stage[TPB / 64][64 * 16];  // 8 KB per wave
    __shared__ double wsum[TPB / 64][4][64];
    const int c = block / LSEG, seg = block % LSEG;
    const int q0c = D.cam_ptr[c], q1c = D.cam_ptr[c + 1];
    const int len = (q1c - q0c + LSEG - 1) / LSEG;
    const int p0 = q0c + seg * len, p1 = min(p0 + len, q1c);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* st = stage[wave];
    double x[12], K[5];
#pragma unroll
    for (int k = 0; k < 12; ++k) x[k] = D.pose[12 * (size_t)c + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) K[k] = D.Kc[k];
    mfma_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int base = p0; base < p1; base += TPB) {  // block-uniform trip count
        const int p = base + (int)threadIdx.x;
        const bool valid = p < p1;
        double row[2][12];
        {
            const int lm = valid ? D.cam_lm[p] : 0;
            const double2 uv = valid ? *reinterpret_cast<const double2*>(&D.cam_uv[2 * (size_t)p]) : double2{0.0, 0.0};
            const double* lp = D.pt + 3 * (size_t)lm;
            const double l[3] = {lp[0], lp[1], lp[2]};
            double Ap[12], Al[6], Ak[10], b[2];
            obs_factor(x, l, K, uv.x, uv.y, D.nz.pix_sigma, D.nz.pix_huber, Ap, Al, Ak, b);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int k = 0; k < 6; ++k) row[h][k] = valid ? Ap[6 * h + k] : 0.0;
#pragma unroll
                for (int k = 0; k < 5; ++k) row[h][6 + k] = valid ? Ak[5 * h + k] : 0.0;
                row[h][11] = valid ? b[h] : 0.0;
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if ((lane >> 5) == half) {
                // rows 2 (lane & 31) and + 1; the 16-byte slots of a row are XOR-swizzled with the observation's low
                // bits so that the eight lanes of a store group hit eight different slots (stride 256 bytes otherwise)
                const int o = lane & 31;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    double2* dst = reinterpret_cast<double2*>(st + (2 * o + h) * 16);
#pragma unroll
                    for (int sl = 0; sl < 8; ++sl)
                        dst[sl ^ (o & 7)] = sl < 6 ? double2{row[h][2 * sl], row[h][2 * sl + 1]} : double2{0.0, 0.0};
                }
            }
            wave_lds_sync();
            {   // operand of step t: lane (i = lane & 15, kk = lane >> 4) <- row 4 t + kk, entry i
                const int i = lane & 15, kk = lane >> 4;
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int r = 4 * t + kk, o = r >> 1;
                    const double v = st[r * 16 + ((((i >> 1) ^ (o & 7)) << 1) | (i & 1))];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 0);
                }
            }
            wave_lds_sync();
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) wsum[wave][r][lane] = acc[r];
    __syncthreads();
    {   // thread -> (reg, lane) of the accumulator image: D[(lane >> 4) + 4 reg][lane & 15]
        const int r = threadIdx.x >> 6, l = threadIdx.x & 63;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) v += wsum[w][r][l];
        clpart[(size_t)CLP * block + 16 * ((l >> 4) + 4 * r) + (l & 15)] = v;
    }
}

// K-A and K-B in ONE launch: the landmark side and the camera side of the linearisation read the same values and
// write disjoint outputs; as two launches the second waited for the first (18 + 23 us on S200). The camera segments
// (the longer role) take the low workgroup ids.
template <int LPL>
__global__ __launch_bounds__(TPB) void ba_linearize(BaDev D, double* __restrict__ clpart, int n_cam_blocks) {
    if ((int)blockIdx.x < n_cam_blocks) linearize_camera_segment(D, clpart, (int)blockIdx.x);
    else linearize_landmark<LPL>(D, ((int)blockIdx.x - n_cam_blocks) * TPB + threadIdx.x);
}

// Second stage, one launch: blocks [0, KLIN) sum the calibration parts over every (camera, segment) in fixed order
// (strided partial sums, then a shuffle tree) and add the Cal3_S2 prior -> klin; blocks [KLIN, KLIN + nc) add a
// camera's segments in order and its pose prior -> camlin.
__device__ __forceinline__ void finish_linearize_block(const BaDev& D, const double* __restrict__ clpart, int block, int lane) {
    if (block < KLIN) {
        const int i = block;
        const int src = i < 25 ? 16 * (6 + min(i / 5, i % 5)) + 6 + max(i / 5, i % 5) : 16 * (6 + (i - 25)) + 11;  // upper triangle
        double s = 0.0;
        for (int e = lane; e < D.nc * LSEG; e += 64) s += clpart[(size_t)CLP * e + src];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if (lane == 0) {
            if (i < 25) {
                if (i / 5 == i % 5) s += 1.0 / (D.nz.k_sigma[i / 5] * D.nz.k_sigma[i / 5]);
            } else {
                const int a = i - 25;
                s += (1.0 / D.nz.k_sigma[a]) * (-(D.Kc[a] - D.K0[a]) / D.nz.k_sigma[a]);
            }
            D.klin[i] = s;
        }
        return;
    }
    const int c = block - KLIN;
    if (lane >= 57) return;
    int a, bb;  // entry of the accumulator image this lane finishes: Hcc upper triangle (21), HcK (30), gc (6)
    if (lane < 21) {
        a = 0;
        int rem = lane;
        while (rem >= 6 - a) rem -= 6 - a, ++a;
        bb = a + rem;
    } else if (lane < 51) {
        a = (lane - 21) / 5, bb = 6 + (lane - 21) % 5;
    } else {
        a = lane - 51, bb = 11;
    }
    double v = 0.0;
    for (int seg = 0; seg < LSEG; ++seg) v += clpart[(size_t)CLP * (c * LSEG + seg) + 16 * a + bb];
    // PriorFactor<Pose3>: e = -Local(x, prior), H = I; Robust(Huber 2.5) unless the node is fixed
    double x[12], xi[6], n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) x[k] = D.pose[12 * (size_t)c + k];
    pose_local(x, D.pose0 + 12 * (size_t)c, xi);
    const bool fx = D.fixed[c] != 0;
    const double* sg = fx ? D.nz.fixed_sigma : D.nz.pose_sigma;
#pragma unroll
    for (int k = 0; k < 6; ++k) n2 += (xi[k] / sg[k]) * (xi[k] / sg[k]);
    const double sw = fx ? 1.0 : sqrt(huber_weight(sqrt(n2), D.nz.pose_huber));
    double* out = D.camlin + (size_t)CAMLIN * c;
    if (lane < 21) {
        if (a == bb) v += (sw / sg[a]) * (sw / sg[a]);
        out[6 * a + bb] = v;
        out[6 * bb + a] = v;
    } else if (lane < 51) {
        out[36 + (lane - 21)] = v;
    } else {
        out[66 + a] = v + (sw / sg[a]) * (-sw * (-xi[a] / sg[a]));
    }
}

__global__ __launch_bounds__(64) void ba_finish_linearize(BaDev D, const double* __restrict__ clpart) {
    finish_linearize_block(D, clpart, (int)blockIdx.x, (int)threadIdx.x);
}

// ---- K-C: per-landmark elimination for one lambda (thread = landmark) -------------------------------
// Hd = Hll + lambda clamp(diag), Hd = L L^T, Linv; EKt = ElK Linv^T, gt = Linv gl (Et_o = E_o Linv^T: K-C2).
// Also this block's share of the (K,K) Schur term: sum EKt EKt^T (25) and EKt gt (5) -> kk_part.
// The launch also clears the tiles of S for the assembly kernels behind it (the factorisation works in place, so S is
// rebuilt for every lambda): the stores are issued first and drain under the arithmetic — no fill node per try.
// The FIRST try after a linearisation also carries that linearisation's second stage (finish_linearize_block: n_finish
// extra workgroups, one wave of each at work): it depends on the linearisation only, like this kernel, and as a launch of its own
// it was 4.6 (window) / 6.9 us (S200) on the chain of the iteration.
// the 3x3 elimination of one landmark for one lambda: Linv (lower: m00; m10 m11; m20 m21 m22), gt = Linv gl, EKt[a] = Linv ElK[a].
// ONE definition for every kernel that needs it (the thread that owns the landmark, and — in the pair-list form — every observation
// of it, which recomputes these 24 numbers instead of waiting for a launch that stores them): same instructions, same bits.
struct LmElim {
    double m[6], gt[3], ek[15];
    bool ok;
};
__device__ __forceinline__ LmElim eliminate_landmark(const double* __restrict__ in /* lmlin record */, double lambda) {
    LmElim r;
    double h0 = in[0], h1 = in[1], h2 = in[2], h3 = in[3], h4 = in[4], h5 = in[5];
    h0 += lambda * clampd(h0, 1e-6, 1e32);
    h3 += lambda * clampd(h3, 1e-6, 1e32);
    h5 += lambda * clampd(h5, 1e-6, 1e32);
    // 3x3 Cholesky, lower: [l00; l10 l11; l20 l21 l22]
    bool ok = h0 > 0.0;
    const double l00 = sqrt(ok ? h0 : 1.0);
    const double l10 = h1 / l00, l20 = h2 / l00;
    const double d1 = h3 - l10 * l10;
    ok = ok && d1 > 0.0;
    const double l11 = sqrt(d1 > 0.0 ? d1 : 1.0);
    const double l21 = (h4 - l20 * l10) / l11;
    const double d2 = h5 - l20 * l20 - l21 * l21;
    ok = ok && d2 > 0.0;
    const double l22 = sqrt(d2 > 0.0 ? d2 : 1.0);
    r.ok = ok;
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -l10 * m00 * m11;
    const double m21 = -l21 * m11 * m22;
    const double m20 = -(l20 * m00 + l21 * m10) * m22;
    r.m[0] = m00; r.m[1] = m10; r.m[2] = m11; r.m[3] = m20; r.m[4] = m21; r.m[5] = m22;
    const double g0 = in[6], g1 = in[7], g2 = in[8];
    r.gt[0] = m00 * g0; r.gt[1] = m10 * g0 + m11 * g1; r.gt[2] = m20 * g0 + m21 * g1 + m22 * g2;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const double e0 = in[9 + 3 * a], e1 = in[10 + 3 * a], e2 = in[11 + 3 * a];
        r.ek[3 * a] = m00 * e0;
        r.ek[3 * a + 1] = m10 * e0 + m11 * e1;
        r.ek[3 * a + 2] = m20 * e0 + m21 * e1 + m22 * e2;
    }
    return r;
}

__device__ __forceinline__ void eliminate_landmarks_block(const BaDev& D, double lambda, int block, int n_lm_blocks) {
    __shared__ double sm[(TPB / 64) * 30];
    const int j = block * TPB + threadIdx.x;
    {
        double2* S2 = reinterpret_cast<double2*>(D.T);
        const size_t total = (size_t)D.sp_ntiles * (PB * PB / 2);
        for (size_t e = (size_t)j; e < total; e += (size_t)n_lm_blocks * TPB) S2[e] = make_double2(0.0, 0.0);
    }
    double kk[30];
#pragma unroll
    for (int k = 0; k < 30; ++k) kk[k] = 0.0;
    if (j < D.nl) {
        const int o0 = D.lm_ptr[j], o1 = D.lm_ptr[j + 1];
        double* out = D.lmtry + (size_t)LMLIN * j;
        if (o1 > o0) {
            const LmElim e = eliminate_landmark(D.lmlin + (size_t)LMLIN * j, lambda);
            if (!e.ok) atomicOr(D.flags, 1);
#pragma unroll
            for (int k = 0; k < 6; ++k) out[k] = e.m[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) out[6 + k] = e.gt[k];
#pragma unroll
            for (int k = 0; k < 15; ++k) out[9 + k] = e.ek[k];
            const double t0 = e.gt[0], t1 = e.gt[1], t2 = e.gt[2];
            const double* ek = e.ek;
#pragma unroll
            for (int a = 0; a < 5; ++a) {
#pragma unroll
                for (int bb = 0; bb < 5; ++bb)
                    kk[5 * a + bb] = ek[3 * a] * ek[3 * bb] + ek[3 * a + 1] * ek[3 * bb + 1] + ek[3 * a + 2] * ek[3 * bb + 2];
                kk[25 + a] = ek[3 * a] * t0 + ek[3 * a + 1] * t1 + ek[3 * a + 2] * t2;
            }
        } else {
#pragma unroll
            for (int k = 0; k < LMLIN; ++k) out[k] = 0.0;
        }
    }
    block_sum<30>(kk, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < 30; ++k) D.kk_part[(size_t)30 * block + k] = kk[k];
}

// ---- K-C2: Et_o = E_o Linv^T and the calibration border, fused (thread = observation, camera order) -------------
// Levenberg-Marquardt never reads E after the linearisation, so writing its 144 bytes per observation there and
// reading them back here would be 2 x 72 MB of traffic for ~450 flops per observation: the Jacobians are recomputed
// at the linearisation point (pose / pt / Kc do not change inside the lambda loop) from camera-ordered ids and
// measurements. The same thread holds Et_o and has its landmark's record in reach, so it also forms the
// observation's share of the border, Et_o [gt | EKt^T] (6 x 6 = 36 products), which used to be a second pass over
// Et with the same gathers (ba_border_partials, 36 us on S200). Workgroups are CAMERA-ALIGNED chunks of <= 256
// observations (cam_chunks, built once per problem): a block sum per chunk -> bpart[chunk][36], added per camera in
// chunk order by assemble_border (ba_assemble). Fixed order, no atomics.
__device__ __forceinline__ void eliminate_observations_block(const BaDev& D, double lambda, int block) {
    // The border share of an observation is Et_o (6 x 3) M_o (3 x 6), M_o = [EKt^T | gt]; its sum over the chunk runs
    // on v_mfma_f64_16x16x4_f64 with TWO observations per instruction: rows 0..5 / 8..13 of the A operand hold Et of
    // the even / odd observation of a pair, columns 0..5 / 8..13 of the B operand their M, the K index (3 used of 4)
    // is shared, so the diagonal 6 x 6 blocks of D accumulate Et M of the two observations and the off-diagonal
    // blocks are discarded. A wave stages 16 observations at a time in its own LDS region, pair t as 3 x 16 doubles
    // per operand: the operands of step t are lds[48 t + lane] for the lanes of k = lane >> 4 < 3, zero otherwise.
    __shared__ __attribute__((aligned(16))) double stA[TPB / 64][8 * 48], stB[TPB / 64][8 * 48];  // 2 x 3 KB per wave: 16 observations per round
    __shared__ double wsum[TPB / 64][4][64];
    const int2 ch = D.cam_chunks[block];  // {first position, count}
    const int p = ch.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool valid = (int)threadIdx.x < ch.y;
    double et[18], lv[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) et[k] = 0.0, lv[k] = 0.0;
    if (valid) {
        const int lm = D.cam_lm[p];
        const double* x = D.pose + 12 * (size_t)D.pos_cam[p];
        const double* lp = D.pt + 3 * (size_t)lm;
        const double2 uv = *reinterpret_cast<const double2*>(&D.cam_uv[2 * (size_t)p]);
        // Linv, gt, EKt of the observation's landmark: recomputed from its linearisation record (the same 192 bytes the stored
        // result would be, ~100 flops), so that this role does not wait for the landmark role — both run in ONE launch
        const LmElim le = eliminate_landmark(D.lmlin + (size_t)LMLIN * lm, lambda);
        double xr[12], K[5];
#pragma unroll
        for (int k = 0; k < 12; ++k) xr[k] = x[k];
#pragma unroll
        for (int k = 0; k < 5; ++k) K[k] = D.Kc[k];
        const double l[3] = {lp[0], lp[1], lp[2]};
        const double m0 = le.m[0], m1 = le.m[1], m2 = le.m[2], m3 = le.m[3], m4 = le.m[4], m5 = le.m[5];
#pragma unroll
        for (int k = 0; k < 3; ++k) lv[k] = le.gt[k];
#pragma unroll
        for (int k = 0; k < 15; ++k) lv[3 + k] = le.ek[k];
        double Ap[12], Al[6], Ak[10], b[2];
        obs_factor(xr, l, K, uv.x, uv.y, D.nz.pix_sigma, D.nz.pix_huber, Ap, Al, Ak, b);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double e0 = Ap[a] * Al[0] + Ap[6 + a] * Al[3], e1 = Ap[a] * Al[1] + Ap[6 + a] * Al[4], e2 = Ap[a] * Al[2] + Ap[6 + a] * Al[5];
            et[3 * a] = m0 * e0;
            et[3 * a + 1] = m1 * e0 + m2 * e1;
            et[3 * a + 2] = m3 * e0 + m4 * e1 + m5 * e2;
        }
        double2* out = reinterpret_cast<double2*>(D.Et + 18 * (size_t)p);
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = double2{et[2 * k], et[2 * k + 1]};
    }
    mfma_d4 acc = {0.0, 0.0, 0.0, 0.0};
    double *sa = stA[wave], *sb = stB[wave];
#pragma unroll
    for (int round = 0; round < 4; ++round) {  // 16 lanes stage, the whole wave multiplies (small LDS footprint: four workgroups per CU)
        if ((lane >> 4) == round) {
            const int o = lane & 15, t = o >> 1, sub = o & 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                // A: Et[a][k] = et[3 a + k], a = 0..5 (+ two zero rows); B: M[k][j] = EKt[j][k] = lv[3 + 3 j + k] (j < 5), gt[k] = lv[k] (j = 5)
                double2* da = reinterpret_cast<double2*>(sa + 48 * t + 16 * k + 8 * sub);
                double2* db = reinterpret_cast<double2*>(sb + 48 * t + 16 * k + 8 * sub);
                da[0] = double2{et[k], et[3 + k]};
                da[1] = double2{et[6 + k], et[9 + k]};
                da[2] = double2{et[12 + k], et[15 + k]};
                da[3] = double2{0.0, 0.0};
                db[0] = double2{lv[3 + k], lv[6 + k]};
                db[1] = double2{lv[9 + k], lv[12 + k]};
                db[2] = double2{lv[15 + k], lv[k]};
                db[3] = double2{0.0, 0.0};
            }
        }
        wave_lds_sync();
        {
            const bool live = lane < 48;  // k = lane >> 4 < 3
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const double a = live ? sa[48 * t + lane] : 0.0, b = live ? sb[48 * t + lane] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
        }
        wave_lds_sync();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) wsum[wave][r][lane] = acc[r];
    __syncthreads();
    if (threadIdx.x < 36) {
        // bpart entry k: k < 30 -> (a, bb) = (k / 5, k % 5), else (k - 30, 5); D[a][b] + D[8 + a][8 + b] with
        // D[row][col] in register row >> 2 of lane (col + 16 (row & 3)); the waves are added in order
        const int k = threadIdx.x, a = k < 30 ? k / 5 : k - 30, b = k < 30 ? k % 5 : 5;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w)
            v += wsum[w][a >> 2][b + 16 * (a & 3)] + wsum[w][2 + (a >> 2)][8 + b + 16 * (a & 3)];
        D.bpart[(size_t)36 * block + k] = v;
    }
}

// K-C + K-C2 of the pair-list form in ONE launch (round 5; two launches before: 11.6 + 10.4 us on the chain of a local window's
// try): workgroups [0, n_cam_chunks) take the observation role (the longer one), the next n_lm_blocks the landmark role (lmtry for
// the step's back-substitution, the K-corner partials, the clearing of S), the last n_finish the linearisation's second stage.
__global__ __launch_bounds__(TPB) void ba_eliminate(BaDev D, double lambda, const double* __restrict__ clpart, int n_lm_blocks, int n_finish) {
    const int b = (int)blockIdx.x;  // (every branch below is workgroup-uniform)
    if (b < D.n_cam_chunks) eliminate_observations_block(D, lambda, b);
    else if (b < D.n_cam_chunks + n_lm_blocks) eliminate_landmarks_block(D, lambda, b - D.n_cam_chunks, n_lm_blocks);
    else if (threadIdx.x < 64) finish_linearize_block(D, clpart, b - D.n_cam_chunks - n_lm_blocks, (int)threadIdx.x);
    (void)n_finish;
}

// ---- K-D1: Schur pair products (wave = chunk of <= 256 entries of one camera block's pair list) ------
// lane e computes the 6x6 product Et[o_e] Et[o'_e]^T of its entry. The two 144-byte rows of an entry are NOT gathered
// by the lane that multiplies them (64 lanes x 16 bytes out of 64 different rows per instruction: 64 memory sectors
// per wave-instruction, nine instructions per row): the 128 rows of a group of 64 entries are copied into the wave's
// LDS region by LDS-DMA with per-lane source addresses, 16-byte piece c = 64 it + lane of the row-major image coming
// from row c / 9 — a wave-instruction then covers seven rows end to end (21 sectors) — and every lane reads its two
// rows back from LDS. The 36 sums over the wave's entries go through a wave-private LDS transpose (the same
// region): lane e writes its 36 products as column e, lane v < 36 then adds row v in entry order — 36 writes +
// 64 reads + 64 adds per wave instead of the 36 x 6 x (2 bpermute + add) of a shuffle tree. Fixed order, no atomics.
__global__ __launch_bounds__(TPB) void ba_schur_pairs(BaDev D) {
    constexpr int ROW = 65;  // odd stride in doubles: the row reads of the 36 summing lanes spread over the banks
    constexpr int WBUF = 36 * ROW;  // 2340 doubles per wave: >= the 128 x 18 doubles of a staged group
    static_assert(WBUF >= 128 * 18, "the staging image fits the reduction image");
    __shared__ __attribute__((aligned(16))) double tr[TPB / 64][WBUF];
    // Et is stored in CAMERA order: the two sides of a block's entries walk two cameras' contiguous regions in
    // ascending order (landmark-ordered records put every gather in a different page of 72 MB).
    // Workgroups go to the 8 XCDs round-robin, each XCD has its own 4 MB L2, and the chunk list is ordered by
    // camera block (ci, cj): every XCD takes one contiguous eighth of it, so that the rows Et of the few cameras
    // ci it is working on stay in ITS L2 (dealt round-robin every XCD sees every camera and the 2 x 144-byte
    // gathers of an entry nearly all miss: 430 MB of L2 fills per launch for 72 MB of Et).
    const int per_xcd = gridDim.x / 8;  // the grid is a multiple of 8
    const int chunk = ((blockIdx.x % 8) * per_xcd + blockIdx.x / 8) * (TPB / 64) + (threadIdx.x >> 6);
    if (chunk >= D.n_chunks) return;
    const int lane = threadIdx.x & 63;
    double* buf = tr[threadIdx.x >> 6];
    const int4 ch = D.pair_chunks[chunk];
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
    // groups of 64 entries, in order (a fixed summation order per lane); the copy of group g + 1 is issued as soon as
    // the rows of group g sit in registers and flies while they are multiplied. Measured on S200 (per launch): the
    // per-lane gathers 85 us, this staging 79 us, with the copy in flight under the products 76 us; the same image
    // staged through registers (16-byte loads + ds_write_b128) 81 us, and with the next group's pieces held in
    // registers across the products it spills.
    auto stage = [&](int g) {
        const int e = g + lane;
        const int2 pr = D.pair_entries[ch.y + (e < ch.z ? e : 0)];  // (a dead lane stages rows nobody multiplies)
#pragma unroll
        for (int it = 0; it < 18; ++it) {
            const int c = 64 * it + lane, r = c / 9, piece = c - 9 * r;  // piece of row r = side (r & 1) of entry r >> 1
            const int rx = __shfl(pr.x, r >> 1), ry = __shfl(pr.y, r >> 1);
            const double* src = D.Et + 18 * (size_t)((r & 1) ? ry : rx) + 2 * piece;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(buf + 128 * it), 16, 0, 0);
        }
    };
    stage(0);
    for (int g = 0; g < ch.z; g += 64) {
        __builtin_amdgcn_s_waitcnt(0);  // the DMA pieces have landed (vmcnt) before any lane reads them
        wave_lds_sync();
        const double2* xp = reinterpret_cast<const double2*>(buf + 36 * lane);
        double x[18], y[18];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double2 a = xp[k], b = xp[9 + k];
            x[2 * k] = a.x, x[2 * k + 1] = a.y, y[2 * k] = b.x, y[2 * k + 1] = b.y;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the rows are in registers: LDS-DMA is not ordered behind ds_read
        wave_lds_sync();
        if (g + 64 < ch.z) stage(g + 64);
        if (g + lane < ch.z) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b < 6; ++b) acc[6 * a + b] += x[3 * a] * y[3 * b] + x[3 * a + 1] * y[3 * b + 1] + x[3 * a + 2] * y[3 * b + 2];
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < 36; ++k) buf[k * ROW + lane] = acc[k];
    wave_lds_sync();
    if (lane < 36) {
        const double* rowp = buf + lane * ROW;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // four interleaved partial sums, combined in a fixed order
#pragma unroll
        for (int e = 0; e < 64; e += 4) {
            s0 += rowp[e];
            s1 += rowp[e + 1];
            s2 += rowp[e + 2];
            s3 += rowp[e + 3];
        }
        D.partial[(size_t)36 * chunk + lane] = (s0 + s1) + (s2 + s3);
    }
}

// ---- K-D2: assemble the camera blocks of S (thread = block element) ---------------------------------
// Element (r, q) of the permuted, padded matrix (ba_plan.hpp) goes to its tile; only the lower triangle of tiles is
// stored (a call that names an upper tile is dropped: the caller stores both (r, q) and (q, r)), a diagonal tile holds
// both of its triangles.
__device__ __forceinline__ void sp_store(const BaDev& D, int r, int q, double v) {
    const int I = r >> 6, J = q >> 6;
    if (I < J) return;
    D.T[(size_t)D.sp_tile_map[I * (I + 1) / 2 + J] * (PB * PB) + (r & (PB - 1)) * PB + (q & (PB - 1))] = v;
}
__device__ __forceinline__ void assemble_blocks(const BaDev& D, double lambda, unsigned block) {
    const long long idx = (long long)block * TPB + threadIdx.x;
    const int blk = (int)(idx / 36), el = (int)(idx % 36);
    if (blk >= D.n_blocks) return;
    const int4 B = D.blocks[blk];
    const int a = el / 6, b = el % 6;
    double s = 0.0;
    for (int k = 0; k < B.w; ++k) s += D.partial[(size_t)36 * (B.z + k) + el];
    double v = -s;
    if (B.x == B.y) {
        const double h = D.camlin[(size_t)CAMLIN * B.x + 6 * a + b];
        v += h;
        if (a == b) v += lambda * clampd(h, 1e-6, 1e32);
    }
    const int r = D.sp_pos[B.x] + a, q = D.sp_pos[B.y] + b;
    sp_store(D, r, q, v);
    if (B.x != B.y) sp_store(D, q, r, v);
}

// ---- K-D3: the calibration border and the right-hand side -------------------------------------------
// thread = border entry: adds the chunk partials of its camera (written by K-C2) in chunk order and writes S;
// the last block reduces the (K,K) corner.
__device__ __forceinline__ void assemble_border(const BaDev& D, double lambda, int c) {
    if (c < D.nc) {
        if (threadIdx.x < 36) {
            const int k = threadIdx.x;
            double s = 0.0;
            for (int ch = D.cam_chunk_ptr[c]; ch < D.cam_chunk_ptr[c + 1]; ++ch) s += D.bpart[(size_t)36 * ch + k];
            const double* cl = D.camlin + (size_t)CAMLIN * c;
            if (k < 30) {
                const int a = k / 5, bb = k % 5;
                const double v = cl[36 + k] - s;
                sp_store(D, D.sp_pos[c] + a, D.sp_posK + bb, v);
                sp_store(D, D.sp_posK + bb, D.sp_pos[c] + a, v);
            } else {
                sp_store(D, D.sp_rhs_row, D.sp_pos[c] + (k - 30), cl[66 + (k - 30)] - s);  // rhs row
            }
        }
    } else if (c > D.nc) {
        // identity on the padding columns of the panels; the pivot of the right-hand-side row: far above anything
        // y^T y can reach, so the last pivot of the root only ever fails through a NaN from before
        for (int k = threadIdx.x; k < D.sp_n_pad; k += TPB) {
            const int q = D.sp_pad_cols[k];
            D.T[(size_t)D.sp_diag_tile[q >> 6] * (PB * PB) + (q & (PB - 1)) * (PB + 1)] = 1.0;
        }
        if (threadIdx.x == 0) sp_store(D, D.sp_rhs_row, D.sp_rhs_row, 1e100);
    } else if (threadIdx.x < 240) {
        // K corner: 8 lanes per entry take every 8th partial (independent loads), then a fixed 3-step
        // shuffle tree
        const int i = threadIdx.x >> 3, part = threadIdx.x & 7;
        double s = 0.0;
        for (int k = part; k < D.n_lm_blocks; k += 8) s += D.kk_part[(size_t)30 * k + i];
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 1);
        if (part != 0) return;
        if (i < 25) {
            const int a = i / 5, bb = i % 5;
            double v = D.klin[i] - s;
            if (a == bb) v += lambda * clampd(D.klin[i], 1e-6, 1e32);
            sp_store(D, D.sp_posK + a, D.sp_posK + bb, v);
        } else {
            sp_store(D, D.sp_rhs_row, D.sp_posK + (i - 25), D.klin[i] - s);
        }
    }
}

// K-D2 and K-D3 write disjoint parts of S from the same inputs: one launch, the block range decides the role
// (two launches of a few microseconds each cost the chain a launch gap more).
__global__ __launch_bounds__(TPB) void ba_assemble(BaDev D, double lambda, unsigned n_block_groups) {
    if (blockIdx.x < n_block_groups) assemble_blocks(D, lambda, blockIdx.x);
    else assemble_border(D, lambda, (int)(blockIdx.x - n_block_groups));
}

// ---- The Schur stage, landmark-major (round 5): ONE launch for K-C, K-C2 and K-D1 ------------------------------------------
// A workgroup owns a group of landmarks (ba_groups.hpp): consecutive landmarks of an order that keeps their camera sets close,
// <= g_rows rows. Phase 0 (thread = landmark): the 3x3 elimination (eliminate_landmark) — Linv, gt, EKt -> lmtry (the
// step's back-substitution reads it) and, in LDS, Linv, the point and the landmark's own row Y = [EKt; gt]. Phase A (thread =
// observation row): Jacobians recomputed at the linearisation point, Et = E Linv^T -> the row's 144 bytes IN LDS (rounds 1-4
// wrote them to HBM: 72 MB per try, and gathered two rows per entry from there). Phase B (wave = chunk of 64 slices, lane =
// one slice = <= GRP_SLICE entries of ONE block): the 6x6 products X Y^T out of LDS, summed in the lane in entry order -> the
// lane's partial, 288 bytes. No cross-lane step at all (a transposed segment sum over lanes was tried first: it cost 1.5 x the
// products whatever its form). Camera blocks, the calibration border, the right-hand side and the K corner are all the same
// sum (the landmark rows act as the observations of a pseudo-camera). Fixed order everywhere, no atomics.
// The per-group arrays are padded to the group bounds, so a thread's first loads need nothing but its block index; the launch
// also clears the tiles of S and carries the linearisation's second stage, as ba_eliminate does.
__host__ __device__ inline size_t schur_groups_lds_bytes(int rows) {
    return sizeof(double) * ((size_t)18 * (rows + 1) + (size_t)9 * (rows / 4));
}
template <int NR>  // rows per thread in phase A: g_rows <= NR * TPB
__global__ __launch_bounds__(TPB, 4 - NR) void ba_schur_groups(BaDev D, double lambda, const double* __restrict__ clpart, int n_finish) {
    extern __shared__ __attribute__((aligned(16))) double g_lds[];
    const int n_grp_blocks = (int)gridDim.x - n_finish;
    if ((int)blockIdx.x >= n_grp_blocks) {  // workgroup-uniform
        if (threadIdx.x < 64) finish_linearize_block(D, clpart, (int)blockIdx.x - n_grp_blocks, (int)threadIdx.x);
        return;
    }
    const int g = blockIdx.x, R = D.g_rows, LMAX = R / 4, tid = threadIdx.x;
    const bool live = g < D.g_ngroups;
    // everything below that comes from memory and needs only the block index is requested first
    int2 ari[NR];
    double2 auv[NR];
    int lmj = -1, lmr = 0;
    BaGroup G = BaGroup{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int it = 0; it < NR; ++it) ari[it] = make_int2(-1, 0), auv[it] = double2{0.0, 0.0};
    if (live) {
        G = D.g_groups[g];
#pragma unroll
        for (int it = 0; it < NR; ++it)
            if (tid + it * TPB < R) {
                ari[it] = D.g_rowinfo[(size_t)g * R + tid + it * TPB];
                auv[it] = reinterpret_cast<const double2*>(D.g_uv)[(size_t)g * R + tid + it * TPB];
            }
        if (tid < LMAX) {
            lmj = D.g_lmid[(size_t)g * LMAX + tid];
            lmr = D.g_lmrow[(size_t)g * LMAX + tid];
        }
    }
    {
        double2* S2 = reinterpret_cast<double2*>(D.T);
        const size_t total = (size_t)D.sp_ntiles * (PB * PB / 2);
        for (size_t e = (size_t)blockIdx.x * TPB + threadIdx.x; e < total; e += (size_t)n_grp_blocks * TPB) S2[e] = make_double2(0.0, 0.0);
    }
    if (!live) return;
    double* rows = g_lds;
    double* linv = rows + 18 * (R + 1);
    double* ptl = linv + 6 * LMAX;
    const int lane = tid & 63, wave = tid >> 6;
    bool arow[NR];  // an observation row (a landmark's own row is written in phase 0)
    double axr[NR][12];
#pragma unroll
    for (int it = 0; it < NR; ++it) {
        arow[it] = ari[it].x >= 0 && ari[it].x < D.nc;
        const double* x = D.pose + 12 * (size_t)(arow[it] ? ari[it].x : 0);
#pragma unroll
        for (int k = 0; k < 12; ++k) axr[it][k] = x[k];
    }
    // ---- phase 0: the group's landmarks (one per thread: a group has at most g_rows / 4 <= TPB) ----
    if (lmj >= 0) {
        const int t = tid, j = lmj;
        double* lrw = rows + 18 * lmr;  // the landmark's own row
        const double* in = D.lmlin + (size_t)LMLIN * j;
        double* out = D.lmtry + (size_t)LMLIN * j;
        double h0 = in[0], h1 = in[1], h2 = in[2], h3 = in[3], h4 = in[4], h5 = in[5];
        h0 += lambda * clampd(h0, 1e-6, 1e32);
        h3 += lambda * clampd(h3, 1e-6, 1e32);
        h5 += lambda * clampd(h5, 1e-6, 1e32);
        bool ok = h0 > 0.0;
        const double l00 = sqrt(ok ? h0 : 1.0);
        const double l10 = h1 / l00, l20 = h2 / l00;
        const double d1 = h3 - l10 * l10;
        ok = ok && d1 > 0.0;
        const double l11 = sqrt(d1 > 0.0 ? d1 : 1.0);
        const double l21 = (h4 - l20 * l10) / l11;
        const double d2 = h5 - l20 * l20 - l21 * l21;
        ok = ok && d2 > 0.0;
        const double l22 = sqrt(d2 > 0.0 ? d2 : 1.0);
        if (!ok) atomicOr(D.flags, 1);
        const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
        const double m10 = -l10 * m00 * m11;
        const double m21 = -l21 * m11 * m22;
        const double m20 = -(l20 * m00 + l21 * m10) * m22;
        out[0] = m00; out[1] = m10; out[2] = m11; out[3] = m20; out[4] = m21; out[5] = m22;
        double* lv = linv + 6 * t;
        lv[0] = m00; lv[1] = m10; lv[2] = m11; lv[3] = m20; lv[4] = m21; lv[5] = m22;
        const double g0 = in[6], g1 = in[7], g2 = in[8];
        const double t0 = m00 * g0, t1 = m10 * g0 + m11 * g1, t2 = m20 * g0 + m21 * g1 + m22 * g2;
        out[6] = t0; out[7] = t1; out[8] = t2;
        lrw[15] = t0; lrw[16] = t1; lrw[17] = t2;
#pragma unroll
        for (int a = 0; a < 5; ++a) {  // EKt[a] = Linv * ElK[a]
            const double e0 = in[9 + 3 * a], e1 = in[10 + 3 * a], e2 = in[11 + 3 * a];
            const double k0 = m00 * e0, k1 = m10 * e0 + m11 * e1, k2 = m20 * e0 + m21 * e1 + m22 * e2;
            out[9 + 3 * a] = k0; out[10 + 3 * a] = k1; out[11 + 3 * a] = k2;
            lrw[3 * a] = k0; lrw[3 * a + 1] = k1; lrw[3 * a + 2] = k2;
        }
        ptl[3 * t] = D.pt[3 * (size_t)j]; ptl[3 * t + 1] = D.pt[3 * (size_t)j + 1]; ptl[3 * t + 2] = D.pt[3 * (size_t)j + 2];
    }
    if (tid >= TPB - 18) rows[18 * R + (tid - (TPB - 18))] = 0.0;  // the null row of the padding entries
    __syncthreads();
    // ---- phase A: Et of the group's observation rows (NR per thread) ----
#pragma unroll
    for (int it = 0; it < NR; ++it)
    if (arow[it]) {
        double K[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) K[k] = D.Kc[k];
        const int lt = ari[it].y;
        const double l[3] = {ptl[3 * lt], ptl[3 * lt + 1], ptl[3 * lt + 2]};
        const double* m = linv + 6 * lt;
        const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        double Ap[12], Al[6], Ak[10], b[2], et[18];
        obs_factor(axr[it], l, K, auv[it].x, auv[it].y, D.nz.pix_sigma, D.nz.pix_huber, Ap, Al, Ak, b);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double e0 = Ap[a] * Al[0] + Ap[6 + a] * Al[3], e1 = Ap[a] * Al[1] + Ap[6 + a] * Al[4], e2 = Ap[a] * Al[2] + Ap[6 + a] * Al[5];
            et[3 * a] = m0 * e0;
            et[3 * a + 1] = m1 * e0 + m2 * e1;
            et[3 * a + 2] = m3 * e0 + m4 * e1 + m5 * e2;
        }
        double2* out = reinterpret_cast<double2*>(rows + 18 * (tid + it * TPB));
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = double2{et[2 * k], et[2 * k + 1]};
    }
    __syncthreads();
    // ---- phase B: the slices, one per lane ----
    for (int c = wave; c < G.nchunks; c += TPB / 64) {
        // (requesting the first chunk's record, lane words and entries before phase 0 — they need only the group record — was
        // measured: 75.4 against 72.6 us, and four spilled registers in the 256-row form)
        const BaChunk ch = D.g_chunks[G.chunk0 + c];
        const uint32_t info = D.g_laneinfo[(size_t)(G.chunk0 + c) * 64 + lane];
        const uint4* ep = reinterpret_cast<const uint4*>(D.g_ent) + (size_t)ch.ent0 * 64 + lane;
        double acc[36];
#pragma unroll
        for (int k = 0; k < 36; ++k) acc[k] = 0.0;
        uint4 e4 = ep[0];
        for (int i4 = 0; i4 < ch.n4; ++i4) {  // (wave-uniform trip count: shorter slices carry null entries)
            const uint32_t ent[4] = {e4.x, e4.y, e4.z, e4.w};
            if (i4 + 1 < ch.n4) e4 = ep[(size_t)(i4 + 1) * 64];  // the next step's entries fly under this step's products
            // (holding the rows of two entries at once — the second's loads under the first's products, 235 registers, which the two
            // waves per SIMD of the 480-row form could afford — measured no gain: 75 against 72.7 us)
#pragma unroll 1
            for (int i = 0; i < 4; ++i) {
                uint32_t e = ent[0];  // (selected, not indexed: a runtime index would put the four words in scratch)
#pragma unroll
                for (int w = 1; w < 4; ++w) e = i == w ? ent[w] : e;
                const double2* xp = reinterpret_cast<const double2*>(rows + 18 * (e & 0xffffu));
                const double2* yp = reinterpret_cast<const double2*>(rows + 18 * (e >> 16));
                double x[18], y[18];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const double2 a = xp[k], b = yp[k];
                    x[2 * k] = a.x, x[2 * k + 1] = a.y, y[2 * k] = b.x, y[2 * k + 1] = b.y;
                }
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = 0; b < 6; ++b) acc[6 * a + b] += x[3 * a] * y[3 * b] + x[3 * a + 1] * y[3 * b + 1] + x[3 * a + 2] * y[3 * b + 2];
            }
        }
        // the lanes of a segment (adjacent, at most GRP_SEG): lane i takes [i, i + 2 d) in step d — after three steps the
        // segment's first lane holds its sum, in a fixed tree order
        const int after = (int)(info >> 28);
        static_assert(GRP_SEG == 8, "three steps");
        // (a segment never leaves its row of 16 lanes, so "the value d lanes up" is a DPP row shift — two v_mov_dpp per double — and not
        // two ds_bpermute through the LDS pipe the other waves' row reads are using)
        auto fold_step = [&](auto DC) {
            constexpr int d = decltype(DC)::value;
            const bool take = after >= d;
            if (!__ballot(take)) return;  // (wave-uniform: nobody in this chunk reaches that far — chunks of one-lane segments skip all three)
#pragma unroll
            for (int k = 0; k < 36; ++k) {
                const int lo = __double2loint(acc[k]), hi = __double2hiint(acc[k]);
                const int slo = __builtin_amdgcn_update_dpp(0, lo, 0x100 + d, 0xf, 0xf, true);   // row_shl:d, out-of-row sources read 0
                const int shi = __builtin_amdgcn_update_dpp(0, hi, 0x100 + d, 0xf, 0xf, true);
                const double o = __hiloint2double(shi, slo);
                acc[k] += take ? o : 0.0;
            }
        };
        fold_step(std::integral_constant<int, 1>{});
        fold_step(std::integral_constant<int, 2>{});
        fold_step(std::integral_constant<int, 4>{});
        const int slot = (int)(info & 0x0fffffffu) - 1;
        if (slot >= 0) {
            double2* dst = reinterpret_cast<double2*>(D.partial + (size_t)36 * slot);
#pragma unroll
            for (int k = 0; k < 18; ++k) dst[k] = double2{acc[2 * k], acc[2 * k + 1]};
        }
    }
}

// One WAVE per block: lane l adds the block's partials l, l + 64, ... (288 contiguous bytes each; a block's partials are contiguous)
// in that order, the 64 lane sums are folded by a fixed xor butterfly; lanes 0..35 then place one element each. Blocks with more
// than GRP_LONG partials — the pseudo-camera's and the diagonal ones collect a partial from nearly every group a camera appears
// in — get a whole WORKGROUP (thread t adds partials t, t + 256, ...; the four waves' sums are added in wave order): walked by one
// thread per element such a list alone took 0.67 ms on S200, by one wave 90 us.
__device__ __forceinline__ void place_group_block(const BaDev& D, double lambda, const int4 B, int el, double s) {
    const int a = el / 6, b = el % 6;
    if (B.y < D.nc) {  // camera block
        double v = -s;
        if (B.x == B.y) {
            const double h = D.camlin[(size_t)CAMLIN * B.x + 6 * a + b];
            v += h;
            if (a == b) v += lambda * clampd(h, 1e-6, 1e32);
        }
        const int r = D.sp_pos[B.x] + a, q = D.sp_pos[B.y] + b;
        sp_store(D, r, q, v);
        if (B.x != B.y) sp_store(D, q, r, v);
    } else if (B.x < D.nc) {  // (c, K): border | right-hand side of camera c
        const double* cl = D.camlin + (size_t)CAMLIN * B.x;
        if (b < 5) {
            const double v = cl[36 + 5 * a + b] - s;
            sp_store(D, D.sp_pos[B.x] + a, D.sp_posK + b, v);
            sp_store(D, D.sp_posK + b, D.sp_pos[B.x] + a, v);
        } else {
            sp_store(D, D.sp_rhs_row, D.sp_pos[B.x] + a, cl[66 + a] - s);
        }
    } else if (a < 5) {  // (K, K): K corner | right-hand side of K
        if (b < 5) {
            double v = D.klin[5 * a + b] - s;
            if (a == b) v += lambda * clampd(D.klin[5 * a + b], 1e-6, 1e32);
            sp_store(D, D.sp_posK + a, D.sp_posK + b, v);
        } else {
            sp_store(D, D.sp_rhs_row, D.sp_posK + a, D.klin[25 + a] - s);
        }
    }
}
// A block's partials are contiguous: element el of partial k sits at partial[36 (first + k) + el], so 36 adjacent threads read 288
// contiguous bytes per k and every thread adds ITS element in k order (eight independent loads in flight per thread).
constexpr int ASM_TPB = 1024;  // workgroup of ba_assemble_groups: 16 blocks of the table (a wave each), or ONE long block
__device__ __forceinline__ double sum_partials(const double* __restrict__ pp, int first, int n, int stride) {
    double s = 0.0;
    int k = first;
    for (; k + 7 * stride < n; k += 8 * stride) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = pp[(size_t)36 * (k + i * stride)];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; k < n; k += stride) s += pp[(size_t)36 * k];
    return s;
}
__device__ __forceinline__ void assemble_group_blocks(const BaDev& D, double lambda, unsigned block) {
    const int blk = (int)block * (ASM_TPB / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk >= D.g_nblk || lane >= 36) return;
    const int4 B = D.g_blk[blk];
    if (B.w > GRP_LONG) return;  // assemble_long_block's
    place_group_block(D, lambda, B, lane, sum_partials(D.partial + (size_t)36 * B.z + lane, 0, B.w, 1));
}
// A block with more than GRP_LONG partials — the pseudo-camera's blocks and the diagonal ones collect a partial from nearly
// every group a camera appears in — gets a WORKGROUP: thread (sub, el) adds partials sub, sub + 28, ... of element el, the 28
// sub-sums are added in order. (Walked by one thread per element such a list alone took 0.67 ms on S200.)
__device__ __forceinline__ void assemble_long_block(const BaDev& D, double lambda, int which) {
    constexpr int NSUB = ASM_TPB / 36;  // 28
    __shared__ double wsum[NSUB][36];
    const int4 B = D.g_blk[D.g_longblk[which]];
    const int sub = threadIdx.x / 36, el = threadIdx.x % 36;
    if (sub < NSUB) wsum[sub][el] = sum_partials(D.partial + (size_t)36 * B.z + el, sub, B.w, NSUB);
    __syncthreads();
    if (threadIdx.x < 36) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NSUB; ++w) s += wsum[w][threadIdx.x];
        place_group_block(D, lambda, B, (int)threadIdx.x, s);
    }
}
__global__ __launch_bounds__(ASM_TPB) void ba_assemble_groups(BaDev D, double lambda, unsigned n_block_groups) {
    // the long blocks first (they are the launch's critical path), then sixteen blocks per workgroup, then the padding columns'
    // identity and the pivot of the right-hand-side row
    if ((int)blockIdx.x < D.g_nlong) assemble_long_block(D, lambda, (int)blockIdx.x);
    else if (blockIdx.x - D.g_nlong < n_block_groups) assemble_group_blocks(D, lambda, blockIdx.x - D.g_nlong);
    else if (threadIdx.x < TPB) assemble_border(D, lambda, D.nc + 1);
}


// ---- K-E: the building blocks of the factorisation of a 64x64 diagonal tile -------------------------------------------
// (factor_32: one wave factorises a 32x32 block in MFMA accumulators; invert_behind_factor: a second wave inverts the
// factor right behind it.) The sparse, level-scheduled factorisation that uses them follows further down (sp_diag /
// sp_level / sp_backsolve); its serial chain is, per level of the elimination tree: the factorising workgroup's loads,
// its panel product, the look-ahead update of the first quadrant, the two diagonal-block factors (ONE wave each, the
// block in MFMA accumulators) and the few hundred cycles the inverting wave trails each factor by.

// first wave only; Dn complete. Publishes L (strictly lower part) and 1/diag through the FactorImage.
// The 32x32 block lives in the accumulators of v_mfma_f64_16x16x4_f64 (three 16x16 blocks of the lower
// triangle; C/D layout col = lane & 15, row = (lane >> 4) + 4 reg) and is factorised four columns at a time:
//   1. the 16-column slab holding the four pivot columns is dumped to LDS (P) — the only cross-lane step;
//   2. every lane reads the 4x4 pivot block (same addresses: LDS broadcast) and the four entries of ITS two
//      rows (l & 15 and 16 + (l & 15)), factorises the 4x4 block and solves its rows against it — all of it
//      in-lane, redundantly in the four lanes that share a row: no readlane, no broadcast;
//   3. lane l keeps component k = l >> 4 of its rows' solution: that IS the A (and B) operand layout of the
//      16x16x4 MFMA, so the rank-4 update of the trailing blocks is one MFMA per 16x16 block.
// The former version (lane = row, pivots and multipliers broadcast with 992 v_readlane into SGPR pairs feeding
// 496 v_fma_f64) spent 13.6k cycles per block, 47 % of the chain of a Cholesky step.
// The non-positive-pivot test stays off the critical path: a bad pivot is only recorded (flags bit 1, the
// solve then counts as failed and its NaNs are never used), it is not replaced. Rows and columns that are
// already factorised keep dead values in the accumulators; they only ever feed other dead elements.
constexpr int PLD = 18;  // row stride of the slab image P[32][PLD]: 16 columns + padding, 16-byte aligned rows

__device__ __forceinline__ double rsqrt_newton(double d) {
    // 1/sqrt(d): hardware estimate (~2^-26 relative, like v_rcp_f64: the compiler's own fp64 division refines it
    // with two Newton steps only to round correctly) + ONE Newton step y <- y (1.5 - (d/2) y^2): the error after
    // the step is ~1.5 e0^2 = a few 1e-16, one or two units in the last place — far inside what a Cholesky factor
    // carries anyway (tests/test_ba_gpu.py holds the step against the oracle at 1e-8). The second step cost three
    // dependent fp64 operations per pivot on the one-wave chain of the diagonal-block factor.
    const double h = 0.5 * d;
    double y = __builtin_amdgcn_rsq(d);
    const double p = h * y, q = __builtin_fma(-p, y, 1.5);
    return y * q;
}

// Fault injection for the time-out branches of the two in-kernel hand-offs (diagnostic build -DEXP_BA_FAULT,
// `make fault`; tests/test_ba_gpu.py). The product build compiles the hooks away.
#ifdef EXP_BA_FAULT
__device__ int g_ba_fault;  // 1: the last super-block of the back-substitution never raises its flag
                            // 2: the first diagonal-block factor drops its last progress store
#define BA_FAULT(k) (g_ba_fault == (k))
#else
#define BA_FAULT(k) false
#endif

typedef int __attribute__((address_space(3))) LdsInt;
constexpr int LFS = NB + 2;  // row stride of the factor image in LDS (16-byte aligned rows)
struct FactorImage {          // what the factorising wave hands to the inverting wave, four columns at a time
    double L[NB][LFS];        // only the strictly lower triangle is meaningful
    double dinv[NB];          // reciprocals of the diagonal
    int progress;             // block columns of four finished so far
};

__device__ __forceinline__ void factor_32(double (*Dn)[NB + 1], double (&P)[NB * PLD] /* LDS slab image */,
                                          FactorImage& F, int* __restrict__ flags, bool inject_fault = false) {
    static_assert(NB == 32, "two 16-row halves");
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    mfma_d4 acc00, acc10, acc11;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        acc00[reg] = Dn[g + 4 * reg][c];
        acc10[reg] = Dn[16 + g + 4 * reg][c];
        acc11[reg] = Dn[16 + g + 4 * reg][16 + c];
    }
    bool bad = false;
#pragma unroll
    for (int s = 0; s < NB / 4; ++s) {
        const int j0 = 4 * s, jb = s >> 2, c0 = j0 & 15;
        // 1. slab -> LDS
        asm volatile("" ::: "memory");
        if (jb == 0) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                P[(g + 4 * reg) * PLD + c] = acc00[reg];
                P[(16 + g + 4 * reg) * PLD + c] = acc10[reg];
            }
        } else {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) P[(16 + g + 4 * reg) * PLD + c] = acc11[reg];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // 2. pivot block (lower triangle) and this lane's rows
        double dd[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double2* src = reinterpret_cast<const double2*>(&P[(j0 + a) * PLD + c0]);
            const double2 lo = src[0], hi = src[1];
            dd[a][0] = lo.x, dd[a][1] = lo.y, dd[a][2] = hi.x, dd[a][3] = hi.y;
        }
        double xr[2][4];
#pragma unroll
        for (int h = jb; h < 2; ++h) {
            const double2* src = reinterpret_cast<const double2*>(&P[(16 * h + c) * PLD + c0]);
            const double2 lo = src[0], hi = src[1];
            xr[h][0] = lo.x, xr[h][1] = lo.y, xr[h][2] = hi.x, xr[h][3] = hi.y;
        }
        // 4x4 Cholesky of the pivot block, column by column, the rows of this lane solved alongside
        double y[4], l[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double d = dd[k][k];
#pragma unroll
            for (int m = 0; m < k; ++m) d = __builtin_fma(-l[k][m], l[k][m], d);
            // a non-positive pivot turns into NaN (rsq of a negative, 0 x inf) and stays NaN through every
            // later pivot — rows of identity padding included, 0 x NaN = NaN — so only the last one is tested
            if (s == NB / 4 - 1 && k == 3) bad = !(d > 0.0);
            y[k] = rsqrt_newton(d);
#pragma unroll
            for (int a = k + 1; a < 4; ++a) {
                double v = dd[a][k];
#pragma unroll
                for (int m = 0; m < k; ++m) v = __builtin_fma(-l[a][m], l[k][m], v);
                l[a][k] = v * y[k];
            }
#pragma unroll
            for (int h = jb; h < 2; ++h) {
                double v = xr[h][k];
#pragma unroll
                for (int m = 0; m < k; ++m) v = __builtin_fma(-xr[h][m], l[k][m], v);
                xr[h][k] = v * y[k];
            }
        }
        // 3. rank-4 update of the trailing blocks
        if (s < NB / 4 - 1) {
            // the blocks the next step dumps go first
            const double b1 = g == 0 ? xr[1][0] : (g == 1 ? xr[1][1] : (g == 2 ? xr[1][2] : xr[1][3]));
            if (s < 3) {
                const double b0 = g == 0 ? xr[0][0] : (g == 1 ? xr[0][1] : (g == 2 ? xr[0][2] : xr[0][3]));
                acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(-b0, b0, acc00, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(-b1, b0, acc10, 0, 0, 0);
            }
            acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(-b1, b1, acc11, 0, 0, 0);
        }
        // L and 1/diag of these four columns go to the inverting wave through LDS (lanes 0..15 hold rows c and
        // 16 + c), behind the MFMAs: the stores ride in their shadow. Only the STRICTLY LOWER triangle of the
        // image is meaningful — its one consumer reads nothing else — so the diagonal and what lands above
        // it are left as computed.
        if (g == 0) {  // one exec region: the sixteen lanes store the same 1/diag values and the same flag
#pragma unroll
            for (int h = jb; h < 2; ++h) {
                double2* dst = reinterpret_cast<double2*>(&F.L[16 * h + c][j0]);
                dst[0] = double2{xr[h][0], xr[h][1]}, dst[1] = double2{xr[h][2], xr[h][3]};
            }
            double2* dd2 = reinterpret_cast<double2*>(&F.dinv[j0]);
            dd2[0] = double2{y[0], y[1]}, dd2[1] = double2{y[2], y[3]};
            asm volatile("" ::: "memory");  // LDS executes a wave's operations in order: only the compiler must not reorder
            if (!(inject_fault && BA_FAULT(2) && s == NB / 4 - 1))  // the LAST store: an earlier one is made up for by the next
                *(volatile LdsInt*)&F.progress = s + 1;  // a DS store like the data before it (a flat store is not ordered with them)
        }
    }
    if (bad && threadIdx.x == 0) atomicOr(flags, 2);
}

// One wave, beside the factorising wave: W = L^-1 (lower), produced four rows at a time as soon as the four
// columns of L they end in are published (FactorImage::progress), so that it is complete a few hundred cycles
// after the factor — the next launch turns every panel solve into a product with W (MFMA) instead of a
// 32-step substitution, and the back-substitution wants W anyway. Lanes c and 32 + c own column c of W.
// Right-looking: rhs[ii] = [ii == c] - sum_{m done} L[ii][m] w_m is kept for every row; when the block columns
// 4s..4s+3 arrive, rows 4s..4s+3 are finished by a 4x4 substitution (all that is left behind the factor's
// last step) and their four w's are then folded into the rows still to come. The two halves of the wave share
// that folding: row blocks of four alternate between them (block rb belongs to half rb & 1), the finished w's
// cross with v_permlane32_swap. A lone wave issues one v_fma_f64 per ~8 cycles: on one half-wave the folding
// alone outlasts the factor.
// A lower-triangular 32x32 inverse W as the B operand of the panel product L = A W^T: lane (j = lane & 15, kk = lane >> 4)
// of k-step t holds W[j][4t + kk] (rows 0..15, t < 4: slots 0..3) or W[16 + j][4t + kk] (t < 8: slots 4..11). Stored in
// that order — two slots per 16-byte lane element, op_index — a consumer wave fetches a slot pair with ONE coalesced 1 KB load; read from the
// row-major image, 64 lanes x 8 bytes out of 16 different rows, the operand fetches of a 64-column panel product (40 per wave) took
// most of 19k cycles per launch. X (a full 32x32 block) uses slots 0..7 for its rows 0..15 and 8..15 for rows 16..31.
constexpr int WOP = 12 * 64, XOP = 16 * 64, TILE_OPS = 2 * WOP + XOP;  // per 64x64 diagonal tile: W_a | W_b | X
__device__ __forceinline__ int op_index(int slot, int lane) { return (slot >> 1) * 128 + 2 * lane + (slot & 1); }  // slot pairs: 16-byte loads
__device__ __forceinline__ int wop_index(int row, int col) {
    return row < 16 ? op_index(col >> 2, (col & 3) * 16 + row) : op_index(4 + (col >> 2), (col & 3) * 16 + row - 16);
}
__device__ __forceinline__ int xop_index(int row, int col) {
    return row < 16 ? op_index(col >> 2, (col & 3) * 16 + row) : op_index(8 + (col >> 2), (col & 3) * 16 + row - 16);
}
// W (LDS image, row stride wls) -> global memory, row-major (back-substitution) and in operand order, by `nthreads` threads
template <int NT>
__device__ __forceinline__ void publish_w(const double* Wl, int wls, double* __restrict__ Wout, double* __restrict__ Wop, int thread) {
    double v[NB * NB / NT];
#pragma unroll
    for (int m = 0; m < NB * NB / NT; ++m) v[m] = Wl[((thread + NT * m) / NB) * wls + (thread + NT * m) % NB];  // every read first
#pragma unroll
    for (int m = 0; m < NB * NB / NT; ++m) {
        const int e = thread + NT * m, row = e / NB, col = e % NB;
        Wout[e] = v[m];
        if (row >= 16 || col < 16) Wop[wop_index(row, col)] = v[m];
    }
}
__device__ __forceinline__ void invert_behind_factor(const FactorImage& F, double* __restrict__ Wout, int* __restrict__ flags,
                                                     double* Wlds = nullptr, int wls = 0 /* LDS copy, row stride; Wout may then be null */) {
    const int lane = threadIdx.x & 63, c = lane & 31, hh = lane >> 5;
    double rhs[NB / 2];  // rhs[4p + a] = row 4 (2p + hh) + a
#pragma unroll
    for (int e = 0; e < NB / 2; ++e) rhs[e] = (4 * (2 * (e >> 2) + hh) + (e & 3)) == c ? 1.0 : 0.0;
    const double* lmine = &F.L[4 * hh][0];  // row 4 (2p + hh) + a starts at lmine + (8p + a) LFS
#pragma unroll
    for (int s = 0; s < NB / 4; ++s) {
        // bounded wait (the factorising wave never waits for anybody, so this cannot expire while it runs);
        // an expired wait marks the solve failed like a hand-off time-out of the back-substitution
        int spins = 0;
        while (*(const volatile LdsInt*)&F.progress <= s && spins < (1 << 24)) {
            __builtin_amdgcn_s_sleep(1);
            ++spins;
        }
        if (spins >= (1 << 24) && lane == 0) atomicOr(flags, 4);
        asm volatile("" ::: "memory");
        const double2 dv01 = *reinterpret_cast<const double2*>(&F.dinv[4 * s]), dv23 = *reinterpret_cast<const double2*>(&F.dinv[4 * s + 2]);
        const double l10 = F.L[4 * s + 1][4 * s];
        const double2 l2x = *reinterpret_cast<const double2*>(&F.L[4 * s + 2][4 * s]);   // l20 l21
        const double2 l3x = *reinterpret_cast<const double2*>(&F.L[4 * s + 3][4 * s]);   // l30 l31
        const double l32 = F.L[4 * s + 3][4 * s + 2];
        // the substitution, meaningful in the half that owns row block s
        double w[4];
        w[0] = rhs[4 * (s >> 1)] * dv01.x;
        w[1] = __builtin_fma(-l10, w[0], rhs[4 * (s >> 1) + 1]) * dv01.y;
        w[2] = __builtin_fma(-l2x.y, w[1], __builtin_fma(-l2x.x, w[0], rhs[4 * (s >> 1) + 2])) * dv23.x;
        w[3] = __builtin_fma(-l32, w[2], __builtin_fma(-l3x.y, w[1], __builtin_fma(-l3x.x, w[0], rhs[4 * (s >> 1) + 3]))) * dv23.y;
        if (hh == (s & 1)) {
#pragma unroll
            for (int a2 = 0; a2 < 4; ++a2) {
                if (Wout) Wout[(4 * s + a2) * NB + c] = w[a2];
                if (Wlds) Wlds[(4 * s + a2) * wls + c] = w[a2];
            }
        }
        if (s == NB / 4 - 1) break;
#pragma unroll
        for (int a2 = 0; a2 < 4; ++a2) {  // the owner's w's to both halves
            const auto wl = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(w[a2]), (unsigned)__double2loint(w[a2]), false, false);
            const auto wh = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(w[a2]), (unsigned)__double2hiint(w[a2]), false, false);
            w[a2] = __hiloint2double((int)wh[s & 1], (int)wl[s & 1]);
        }
        // fold them into the rows still to come: row blocks 2p + hh, p >= (s + 1) / 2 (for even s the lower
        // half's first block is the finished one itself: dead values, harmless), two blocks = eight rows at a
        // time with every read of a group issued before its arithmetic
#pragma unroll
        for (int p0 = (s + 1) >> 1; p0 < NB / 8; p0 += 2) {
            double2 la[8], lb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (p0 + (u >> 2) < NB / 8) {
                    const double* row = lmine + (8 * (p0 + (u >> 2)) + (u & 3)) * LFS + 4 * s;
                    la[u] = *reinterpret_cast<const double2*>(row);
                    lb[u] = *reinterpret_cast<const double2*>(row + 2);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (p0 + (u >> 2) < NB / 8) {
                    double& r = rhs[4 * (p0 + (u >> 2)) + (u & 3)];
                    r = __builtin_fma(-lb[u].y, w[3], __builtin_fma(-lb[u].x, w[2], __builtin_fma(-la[u].y, w[1], __builtin_fma(-la[u].x, w[0], r))));
                }
            // the next group's reads stay behind this group's arithmetic (hoisted together they spill): a memory
            // clobber alone lets the compiler sink the FMAs below it, so the results are pinned as operands
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (p0 + (u >> 2) < NB / 8) asm volatile("" : "+v"(rhs[4 * (p0 + (u >> 2)) + (u & 3)]) : : "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- K-E in panels of 64 columns ----------------------------------------------------------------------------------
// A 64x64 diagonal tile holds two 32x32 diagonal blocks a, b, and everything the second one needs — L_ba = A'_ba W_a^T
// and D_b = A'_bb - L_ba L_ba^T — comes from the tile itself, so ONE workgroup factorises both without a launch in
// between (a third of a 32-column step was paid per LAUNCH: kernel start + dependent global loads):
//   * the panel of a tile row is ONE product with the inverse of the 64x64 factor, [L_ia L_ib] = [A_ia A_ib] W64^T,
//     W64 = [[W_a, 0], [X, W_b]], X = -W_b L_ba W_a: 40 MFMAs per 16 rows. The producer stores W_a, W_b, X in MFMA
//     operand order (wop_index), so the B operands are coalesced 16-byte loads; a wave fetches its own 16 rows of each
//     raw strip as whole rows and is their only reader in LDS: no workgroup barrier before the product;
//   * the update of a target tile is rank 64 per source panel;
//   * a factorising workgroup updates the first quadrant of its tile first (waves 0-2), then wave 0 factorises it, wave 1
//     inverts behind it and waves 2-3 update the other quadrants (kept in registers); after a barrier waves 2-3 form
//     L_ba from the rows they hold (waves 0-1 publish W_a meanwhile), waves 0-2 D_b, then wave 0 factorises D_b, wave 1
//     inverts, waves 2-3 form L_ba W_a, and all four waves finish X and publish W_b.
// LDS: two 64 x 66 strips (67.6 KB, two workgroups per CU). A diagonal target never uses the second strip, and its
// first strip is dead once the quadrants are updated: the factor images live in the second strip's region, the four
// 32 x 33 images of the second half in the first's.
constexpr int LS2 = PB + 2;  // row stride of the strips
constexpr int TS = NB + 1;   // row stride of the 32x32 images of the second half (8-byte accesses only)
constexpr int WLS = NB + 2;  // row stride of the LDS copy of W_a
constexpr int TILE = PB * PB;  // doubles per tile of the sparse storage (row-major, row stride PB)

// L = A W^T for 16 rows whose A operand a[0..7] (columns 0..31) sits in registers, W (lower triangular, row stride ws)
// in LDS or global memory: columns 0..15 -> x0, 16..31 -> x1 + x2
__device__ __forceinline__ void panel32(const double (&a)[8], const double* __restrict__ W, int ws, int mc, int mg, mfma_d4& lo,
                                        mfma_d4& hi) {
    mfma_d4 x0 = {0.0, 0.0, 0.0, 0.0}, x1 = {0.0, 0.0, 0.0, 0.0}, x2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], W[mc * ws + 4 * t + mg], x0, 0, 0, 0);
        x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], W[(16 + mc) * ws + 4 * t + mg], x1, 0, 0, 0);
        x2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t + 4], W[(16 + mc) * ws + 4 * t + 16 + mg], x2, 0, 0, 0);
    }
    lo = x0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) hi[reg] = x1[reg] + x2[reg];
}

struct DiagImages {  // LDS views of a 64x64 diagonal tile being factorised
    double (*Dn)[NB + 1];
    double* Pslab;    // [NB * PLD], 16-byte aligned
    FactorImage* F;
    double* Wa;       // [NB][WLS] copy of W_a (written by the inverting wave of the first half)
    double* T10;      // [NB][TS] A'_ba, then L_ba
    double* T11;      // [NB][TS] A'_bb
    double* P1;       // [NB][TS] L_ba W_a
    double* Wb;       // [NB][TS] copy of W_b
};

// Second half of a diagonal tile: every thread of the workgroup, after a barrier behind which W_a (LDS copy), T10 and
// T11 are complete. Stores W_b -> Wout_b (row-major) and Wop_b, X -> Xop (operand order, for the panel products of the
// launches that use this panel as a source) and Xrow (row-major, for the back-substitution).
__device__ __forceinline__ void diag_second_half(const DiagImages& I, double* __restrict__ Wout_b, double* __restrict__ Wop_b,
                                                 double* __restrict__ Xop, double* __restrict__ Xrow, int* __restrict__ flags, int w0 = 0) {
    const int tid = threadIdx.x, mc = tid & 15, mg = (tid >> 4) & 3;
    int wv = (tid >> 6) - w0;  // waves w0, w0 + 1 form L_ba (in sp_level the two that just wrote those rows of T10)
    if (wv >= 0 && wv < 2) {  // L_ba = A'_ba W_a^T, 16 rows per wave, in place (the wave's own rows: reads before writes, in LDS order)
        double a[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) a[t] = I.T10[(16 * wv + mc) * TS + 4 * t + mg];
        mfma_d4 lo, hi;
        panel32(a, I.Wa, WLS, mc, mg, lo, hi);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 16 * wv + mg + 4 * reg;
            I.T10[row * TS + mc] = lo[reg];
            I.T10[row * TS + 16 + mc] = hi[reg];
        }
    }
    if (tid == 0) I.F->progress = 0;
    wv = tid >> 6;
    __syncthreads();
    if (wv < 3) {  // D_b = A'_bb - L_ba L_ba^T, one 16x16 block of the lower triangle per wave
        const int mbi = wv == 0 ? 0 : 16, mbj = wv == 2 ? 16 : 0;
        mfma_d4 m0, m1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) m0[reg] = I.T11[(mbi + mg + 4 * reg) * TS + mbj + mc];
#pragma unroll
        for (int t = 0; t < NB / 4; t += 2) {
            const double a0 = I.T10[(mbi + mc) * TS + 4 * t + mg], b0 = I.T10[(mbj + mc) * TS + 4 * t + mg];
            const double a1 = I.T10[(mbi + mc) * TS + 4 * t + 4 + mg], b1 = I.T10[(mbj + mc) * TS + 4 * t + 4 + mg];
            m0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0, b0, m0, 0, 0, 0);
            m1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1, b1, m1, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) I.Dn[mbi + mg + 4 * reg][mbj + mc] = m0[reg] + m1[reg];
    }
    __syncthreads();
    if (wv == 0) {
        factor_32(I.Dn, *reinterpret_cast<double (*)[NB * PLD]>(I.Pslab), *I.F, flags);
    } else if (wv == 1) {
        invert_behind_factor(*I.F, nullptr, flags, I.Wb, TS);
    } else {  // P1 = L_ba W_a beside the factor: rows 16 (wv - 2) .., W_a[k][j] = 0 for k < j
        const int bi = wv - 2;
        mfma_d4 p0 = {0.0, 0.0, 0.0, 0.0}, p1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const double a = I.T10[(16 * bi + mc) * TS + 4 * t + mg];
            p0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, I.Wa[(4 * t + mg) * WLS + mc], p0, 0, 0, 0);
            if (t >= 4) p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, I.Wa[(4 * t + mg) * WLS + 16 + mc], p1, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            I.P1[(16 * bi + mg + 4 * reg) * TS + mc] = p0[reg];
            I.P1[(16 * bi + mg + 4 * reg) * TS + 16 + mc] = p1[reg];
        }
    }
    __syncthreads();
    {   // X = -W_b P1: one 16x16 block per wave, W_b[i][k] = 0 for k > i; W_b is published in the shadow of the chain
        const int bi = wv >> 1, bj = wv & 1;
        mfma_d4 x = {0.0, 0.0, 0.0, 0.0}, x2 = x;  // two chains: a dependent f64 MFMA waits out the full 64-cycle pass
#pragma unroll
        for (int t = 0; t < 8; t += 2)
            if (t < 4 * (bi + 1)) {
                x = __builtin_amdgcn_mfma_f64_16x16x4f64(-I.Wb[(16 * bi + mc) * TS + 4 * t + mg], I.P1[(4 * t + mg) * TS + 16 * bj + mc], x, 0, 0, 0);
                x2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-I.Wb[(16 * bi + mc) * TS + 4 * t + 4 + mg], I.P1[(4 * t + 4 + mg) * TS + 16 * bj + mc], x2, 0, 0, 0);
            }
        publish_w<TPB>(I.Wb, TS, Wout_b, Wop_b, tid);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 16 * bi + mg + 4 * reg, col = 16 * bj + mc;
            const double v = x[reg] + x2[reg];
            Xop[xop_index(row, col)] = v;
            Xrow[row * NB + col] = v;
        }
    }
}

// ---- the sparse, level-scheduled factorisation (plan: ba_plan.hpp) ------------------------------------------------
// S lives as 64x64 tiles of the symbolic pattern of its Cholesky factor (cameras permuted and laid out in panels by the
// plan; padding columns carry an identity diagonal, the right-hand side is row 63 of the root panel). Per panel P the
// factorisation leaves W64_P = [[W_a, 0], [X, W_b]] = (factor of the fully updated diagonal tile)^-1 in Winv (W_a, W_b
// row-major), Xrow and Wops (operand order); the off-diagonal tiles end as the RAW updated strips A'[I][P] — the factor
// strips L[I][P] = A'[I][P] W64_P^T are formed on the fly by every consumer and never stored: the back-substitution
// works on the raw tiles too (sp_backsolve).

// Launch 0: the diagonal tiles of the leaves of the elimination tree (nothing updates them), one workgroup each.
__global__ __launch_bounds__(TPB) void sp_diag(const double* __restrict__ T, const int* __restrict__ leaves, const int* __restrict__ diag_tile,
                                               double* __restrict__ Winv, double* __restrict__ Wops, double* __restrict__ Xrow,
                                               int* __restrict__ flags) {
    __shared__ double Dn[NB][NB + 1];
    __shared__ __attribute__((aligned(16))) double Pslab[NB * PLD];
    __shared__ __attribute__((aligned(16))) FactorImage Fimg;
    __shared__ double Wa[NB * WLS], T10[NB * TS], T11[NB * TS], P1[NB * TS], Wb[NB * TS];
    const int tid = threadIdx.x;
    const int P = leaves[blockIdx.x];
    const double* __restrict__ A = T + (size_t)diag_tile[P] * TILE;
    double raw[12];
#pragma unroll
    for (int m = 0; m < 12; ++m) {  // the three quadrants of the lower triangle, all loads in flight together
        const int q = m >> 2, idx = tid + TPB * (m & 3), i = idx / NB + (q > 0 ? NB : 0), j = idx % NB + (q == 2 ? NB : 0);
        raw[m] = A[i * PB + j];
    }
#pragma unroll
    for (int m = 0; m < 12; ++m) {
        const int q = m >> 2, idx = tid + TPB * (m & 3), i = idx / NB, j = idx % NB;
        if (q == 0) Dn[i][j] = raw[m];
        else if (q == 1) T10[i * TS + j] = raw[m];
        else T11[i * TS + j] = raw[m];
    }
    if (tid == 0) Fimg.progress = 0;
    __syncthreads();
    if (tid < 64) factor_32(Dn, Pslab, Fimg, flags, blockIdx.x == 0);
    else if (tid < 128) invert_behind_factor(Fimg, nullptr, flags, Wa, WLS);
    __syncthreads();
    if (tid >= 128) publish_w<128>(Wa, WLS, Winv + (size_t)(2 * P) * NB * NB, Wops + (size_t)P * TILE_OPS, tid - 128);  // (waves 0-1 form L_ba next)
    DiagImages I{Dn, Pslab, &Fimg, Wa, T10, T11, P1, Wb};
    diag_second_half(I, Winv + (size_t)(2 * P + 1) * NB * NB, Wops + (size_t)P * TILE_OPS + WOP, Wops + (size_t)P * TILE_OPS + 2 * WOP,
                     Xrow + (size_t)P * NB * NB, flags);
}

// [L_a L_b] = [A_a A_b] W64^T for the wave's 16 rows of a strip, in place: every operand read of the strip precedes the
// writes in the wave's LDS order. wa / wb: W_a / W_b in operand order (wop_index), xp: X (xop_index).
__device__ __forceinline__ void panel64(double (*strip)[LS2], int wv, int mc, int mg, const double (&wa)[12], const double (&wb)[12],
                                        const double (&xp)[16]) {
    double a[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = strip[16 * wv + mc][4 * q + mg];
    mfma_d4 x0 = {0.0, 0.0, 0.0, 0.0}, x1 = x0, x2 = x0, y0 = x0, y1 = x0, y2 = x0, y3 = x0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], wa[q], x0, 0, 0, 0);
        x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], wa[4 + q], x1, 0, 0, 0);
        x2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 + q], wa[8 + q], x2, 0, 0, 0);
        y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[8 + q], wb[q], y1, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], xp[q], y0, 0, 0, 0);
        y2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], xp[8 + q], y2, 0, 0, 0);
        y3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[8 + q], wb[4 + q], y3, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        double* row = strip[16 * wv + mg + 4 * reg];
        row[mc] = x0[reg];
        row[16 + mc] = x1[reg] + x2[reg];
        row[32 + mc] = y0[reg] + y1[reg];
        row[48 + mc] = y2[reg] + y3[reg];
    }
}

// Launch l + 1: the updates of every source panel J of level l, one workgroup per TARGET tile (I1, I2):
//   A[I1][I2] -= sum_J L[I1][J] L[I2][J]^T,   L[I][J] = A'[I][J] W64_J^T formed from the raw strip and J's operands,
// the sources in the plan's order (ascending J: a fixed summation order, no atomics; a tile is written by exactly one
// workgroup of a launch and read as a strip only in the launch of its own column's level). A diagonal target (P, P)
// whose panel P has level l + 1 is complete after its last source: that workgroup goes on and factorises it ->
// W_a, W_b, X of P (the chain of the launch: these items are dispatched first). Its tile is not written back: nothing
// reads a diagonal tile after its factorisation.
template <bool FIRST>
__device__ __forceinline__ void sp_level_item(double* lds, double* __restrict__ T, const BaPlanItem* __restrict__ items,
                                              const BaPlanSrc* __restrict__ srcs, double* __restrict__ Winv, double* __restrict__ Wops,
                                              double* __restrict__ Xrow, int* __restrict__ flags) {
    double (*Li)[LS2] = reinterpret_cast<double (*)[LS2]>(lds);
    double (*Lj)[LS2] = reinterpret_cast<double (*)[LS2]>(lds + 64 * LS2);
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, mc = tid & 15, mg = (tid >> 4) & 3;
    const BaPlanItem it = items[blockIdx.x];
    const bool first = FIRST;                          // a diagonal target that this workgroup factorises after its last source
    const bool same = FIRST || (it.flags & 1) != 0;    // a diagonal target: both strips are the same rows, one is formed
    double* __restrict__ A = T + (size_t)it.tgt * TILE;
    const int mbi = wv == 0 ? 0 : 16, mbj = wv == 2 ? 16 : 0;  // first quadrant of a factorising item: blocks (0,0), (1,0), (1,1)
    const bool block_thread = !first || wv >= 2;  // a wave owns 16 rows of the tile and its four 16-column blocks
    mfma_d4 old[4];
    if (block_thread) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                old[cb][reg] = (same && cb > wv) ? 0.0 : A[(16 * wv + mg + 4 * reg) * PB + 16 * cb + mc];
    }
    mfma_d4 mold = {0.0, 0.0, 0.0, 0.0};
    if (first && wv < 3) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) mold[reg] = A[(mbi + mg + 4 * reg) * PB + mbj + mc];
    }
    // a target that takes more sources than its window allows has shadow accumulators (ba_plan.hpp): other workgroups summed
    // part of its updates into them in earlier launches; they join the target here, in the launch of its deadline
    for (int k = 0; k < it.nshadow; ++k) {
        const double* __restrict__ Sh = T + (size_t)(it.shadow0 + k) * TILE;
        if (block_thread) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if (!(same && cb > wv)) old[cb][reg] += Sh[(16 * wv + mg + 4 * reg) * PB + 16 * cb + mc];
        }
        if (first && wv < 3) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) mold[reg] += Sh[(mbi + mg + 4 * reg) * PB + mbj + mc];
        }
    }
#pragma unroll 1
    for (int s = 0; s < it.nsrc; ++s) {
        const BaPlanSrc sr = srcs[it.src0 + s];
        // Every global read of a source is issued up front, none is predicated. A wave fetches ITS 16 rows of each raw
        // strip, two whole rows (2 x 512 bytes) per instruction, and is the only reader of their LDS image: no
        // workgroup barrier before the panel product.
        const double* __restrict__ Si = T + (size_t)sr.tile_i * TILE;
        const double* __restrict__ Sj = T + (size_t)sr.tile_j * TILE;
        double2 pi[8], pj[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) pi[m] = *reinterpret_cast<const double2*>(&Si[(16 * wv + 2 * m + (lane >> 5)) * PB + 2 * (lane & 31)]);
        if (!FIRST) {  // (a diagonal target fetches the same rows twice: a conditionally initialised array would live in scratch)
#pragma unroll
            for (int m = 0; m < 8; ++m) pj[m] = *reinterpret_cast<const double2*>(&Sj[(16 * wv + 2 * m + (lane >> 5)) * PB + 2 * (lane & 31)]);
        }
        // the B operands of the panel product, stored in operand order by the producer: one coalesced load per k-step
        const double* __restrict__ ops = Wops + (size_t)sr.J * TILE_OPS;
        double wa[12], wb[12], xp[16];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q < 6) {
                const double2 u = *reinterpret_cast<const double2*>(&ops[op_index(2 * q, lane)]), v = *reinterpret_cast<const double2*>(&ops[WOP + op_index(2 * q, lane)]);
                wa[2 * q] = u.x, wa[2 * q + 1] = u.y, wb[2 * q] = v.x, wb[2 * q + 1] = v.y;
            }
            const double2 u = *reinterpret_cast<const double2*>(&ops[2 * WOP + op_index(2 * q, lane)]);
            xp[2 * q] = u.x, xp[2 * q + 1] = u.y;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) *reinterpret_cast<double2*>(&Li[16 * wv + 2 * m + (lane >> 5)][2 * (lane & 31)]) = pi[m];
        if (!FIRST) {
#pragma unroll
            for (int m = 0; m < 8; ++m) *reinterpret_cast<double2*>(&Lj[16 * wv + 2 * m + (lane >> 5)][2 * (lane & 31)]) = pj[m];
        }
        wave_lds_sync();
        panel64(Li, wv, mc, mg, wa, wb, xp);
        if (!same) panel64(Lj, wv, mc, mg, wa, wb, xp);
        __syncthreads();
        if (first) {
            if (s + 1 == it.nsrc) break;  // the last source: its updates are interleaved with the factorisation below
            if (wv < 3) {  // first quadrant, kept in registers
                mfma_d4 m0 = mold, m1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < PB / 4; q += 2) {
                    const double a0 = Li[mbi + mc][4 * q + mg], b0 = Li[mbj + mc][4 * q + mg];
                    const double a1 = Li[mbi + mc][4 * q + 4 + mg], b1 = Li[mbj + mc][4 * q + 4 + mg];
                    m0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0, b0, m0, 0, 0, 0);
                    m1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1, b1, m1, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) mold[reg] = m0[reg] + m1[reg];
            }
            if (wv >= 2) {  // rows 32..63
#pragma unroll
                for (int q = 0; q < PB / 4; ++q) {
                    const double av = -Li[16 * wv + mc][4 * q + mg];
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb)
                        if (cb <= wv) old[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Li[16 * cb + mc][4 * q + mg], old[cb], 0, 0, 0);
                }
            }
            __syncthreads();  // every read of this source's strips is complete (no array of loads is live across this barrier)
            continue;
        }
        // A_ij -= L_i L_j^T over the 64 panel columns: the four 16-column blocks of the wave's rows as four chains
        double (*LjE)[LS2] = same ? Li : Lj;
#pragma unroll
        for (int q = 0; q < PB / 4; ++q) {
            const double av = -Li[16 * wv + mc][4 * q + mg];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (!(same && cb > wv)) old[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, LjE[16 * cb + mc][4 * q + mg], old[cb], 0, 0, 0);
        }
        if (s + 1 < it.nsrc) __syncthreads();  // every read of this source's strips is complete before the next one's land
    }
    if (!first) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (!(same && cb > wv)) A[(16 * wv + mg + 4 * reg) * PB + 16 * cb + mc] = old[cb][reg];
        return;
    }
    // ---- the factorising item, behind the barrier of its last source's panel product ----
    // images of the factorisation: second strip's region (a diagonal target never writes it)
    double* base = lds + 64 * LS2;
    double (*Dn)[NB + 1] = reinterpret_cast<double (*)[NB + 1]>(base);
    double* Pslab = base + NB * (NB + 1);  // 1056 doubles in: 16-byte aligned
    FactorImage* F = reinterpret_cast<FactorImage*>(Pslab + NB * PLD);
    double* Wal = reinterpret_cast<double*>(F) + (sizeof(FactorImage) + 7) / 8 + 1;
    static_assert(NB * (NB + 1) % 2 == 0 && (NB * PLD) % 2 == 0, "Pslab and the factor image stay 16-byte aligned");
    static_assert(NB * (NB + 1) + NB * PLD + (sizeof(FactorImage) + 7) / 8 + 1 + NB * WLS <= 64 * LS2, "the images fit the second strip");
    static_assert(4 * NB * TS <= 64 * LS2, "the images of the second half fit the first strip");
    DiagImages I{Dn, Pslab, F, Wal, lds, lds + NB * TS, lds + 2 * NB * TS, lds + 3 * NB * TS};
    const int P = it.panel;
    if (tid == 0) F->progress = 0;
    if (wv < 3) {  // first quadrant: A_00 - L_0 L_0^T over the 64 panel columns
        mfma_d4 m0 = mold, m1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < PB / 4; q += 2) {
            const double a0 = Li[mbi + mc][4 * q + mg], b0 = Li[mbj + mc][4 * q + mg];
            const double a1 = Li[mbi + mc][4 * q + 4 + mg], b1 = Li[mbj + mc][4 * q + 4 + mg];
            m0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0, b0, m0, 0, 0, 0);
            m1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1, b1, m1, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) Dn[mbi + mg + 4 * reg][mbj + mc] = m0[reg] + m1[reg];
    }
    __syncthreads();
    if (wv == 0) {
        factor_32(Dn, *reinterpret_cast<double (*)[NB * PLD]>(Pslab), *F, flags);
    } else if (wv == 1) {
        invert_behind_factor(*F, nullptr, flags, Wal, WLS);
    } else {  // rows 32..63 of the tile beside the factor; the results stay in registers until the strip is dead
#pragma unroll
        for (int q = 0; q < PB / 4; ++q) {
            const double av = -Li[16 * wv + mc][4 * q + mg];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (cb <= wv) old[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Li[16 * cb + mc][4 * q + mg], old[cb], 0, 0, 0);
        }
    }
    __syncthreads();  // the strip is dead: W_a's copy, the factor of block a and every read of Li are complete
    if (wv >= 2) {  // the wave's 16 rows of A'_ba (own rows of T10: wave-local) and of A'_bb
        const int r0 = 16 * (wv - 2);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = r0 + mg + 4 * reg, col = 16 * (cb & 1) + mc;
                if (cb < 2) I.T10[row * TS + col] = old[cb][reg];
                else I.T11[row * TS + col] = old[cb][reg];  // (block (2, 3) of wave 2 is the zero it was loaded as: never read)
            }
        wave_lds_sync();
    } else {  // waves 0-1 are idle until D_b: they publish W_a
        publish_w<128>(Wal, WLS, Winv + (size_t)(2 * P) * NB * NB, Wops + (size_t)P * TILE_OPS, tid);
    }
    diag_second_half(I, Winv + (size_t)(2 * P + 1) * NB * NB, Wops + (size_t)P * TILE_OPS + WOP, Wops + (size_t)P * TILE_OPS + 2 * WOP,
                     Xrow + (size_t)P * NB * NB, flags, 2);
}

// The factorising items of a launch come first in its item list (n_first of them): the two roles are separate code paths
// of one kernel (as two kernels the second would wait for the first: a launch more on the chain of every level).
__global__ __launch_bounds__(TPB, 2) void sp_level(double* __restrict__ T, const BaPlanItem* __restrict__ items, const BaPlanSrc* __restrict__ srcs,
                                                   int n_first, double* __restrict__ Winv, double* __restrict__ Wops,
                                                   double* __restrict__ Xrow, int* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) double lds[2 * 64 * LS2];
    if ((int)blockIdx.x < n_first) sp_level_item<true>(lds, T, items, srcs, Winv, Wops, Xrow, flags);
    else sp_level_item<false>(lds, T, items, srcs, Winv, Wops, Xrow, flags);
}

// sum of v over aligned groups of W lanes inside a 16-lane DPP row; valid in each group's last lane
template <int W>
__device__ __forceinline__ double dpp_row_sum(double v) {
    static_assert(W == 8 || W == 16, "row_shr steps 1, 2, 4 (, 8)");
#define EACHAM_DPP_STEP(ctrl)                                                                       \
    {                                                                                               \
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xf, 0xf, true);     \
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xf, 0xf, true);     \
        v += __hiloint2double(hi, lo);                                                              \
    }
    EACHAM_DPP_STEP(0x111)  // row_shr:1
    EACHAM_DPP_STEP(0x112)  // row_shr:2
    EACHAM_DPP_STEP(0x114)  // row_shr:4
    if (W == 16) EACHAM_DPP_STEP(0x118)  // row_shr:8
#undef EACHAM_DPP_STEP
    return v;
}

// Back-substitution on the elimination tree, ONE launch: workgroup b solves panel J = order[b] (root first, a panel
// after its parent) and the panels hand their solutions down through global memory with a flag per panel instead of
// kernel boundaries. With the right-hand side carried as row 63 of the root, z = [x; -1] solves L_aug^T z = -delta e_63:
//   root:   z = -W[63][:] / W[63][63]                    (W = W64 of the root, delta = its last pivot)
//   J:      t = -sum_{I in struct(J)} A'[I][J]^T z_I     (the RAW strips: L[I][J] = A'[I][J] W_J^T is never stored; the
//                                                          root's row 63 times z_root[63] = -1 brings in the rhs)
//           z_J = W_J^T (W_J t)                          (= D_J^-1 t, D_J the fully updated diagonal tile)
// The chain is one hand-off per level of the tree, and only the PARENT's strip sits on it: a workgroup consumes its
// strips from the far end (root side) as their z appear, so what is left when the parent publishes is one poll, eight
// loads, one strip of multiply-adds (its values prefetched), a cross-wave sum, two 64x64 triangular products and the
// publication. Protocol as in cdna_hip_programming.md section 6 (write-through form): z_J is stored by ONE wave with
// agent-scope atomic stores (sc1), that wave drains (vmcnt(0)) and its lane 0 sets the flag; every consuming wave polls
// the flag itself with an agent-scope atomic and reads z with agent-scope atomic loads (they bypass its CU's L1) — no
// fences, no workgroup barrier per strip. A wave whose wait expires raises flags[0] bit 2 (the solve counts as failed,
// EACHAM_ERR_HIP) and goes on: no wave can spin forever. The low workgroup ids go to the producers (the hardware
// dispatches in ascending order), so a consumer never occupies a CU its producer still needs.
constexpr int BS_THREADS = 512;  // eight waves: wave g owns rows 8 g .. 8 g + 7 of every strip
constexpr int BS_PF = 4;         // strips whose values are in flight ahead of the one being consumed
__global__ __launch_bounds__(BS_THREADS) void sp_backsolve(const double* __restrict__ T, const int* __restrict__ order, const int* __restrict__ ptr,
                                                           const int2* __restrict__ ent, const double* __restrict__ Winv,
                                                           const double* __restrict__ Xrow, double* __restrict__ z,
                                                           const int* __restrict__ col_dest, double* __restrict__ delta_c,
                                                           int* __restrict__ flags) {
    __shared__ double Wl[PB][PB + 1];
    __shared__ double part[BS_THREADS / PB][PB];
    __shared__ double tl[PB], ul[PB], zl[PB];
    const int tid = threadIdx.x, j = tid & (PB - 1), g = tid >> 6;
    constexpr int RPT = PB / (BS_THREADS / PB);  // rows of a strip per thread: 8
    const int b = blockIdx.x, J = order[b], e0 = ptr[b], e1 = ptr[b + 1];
    int* handoff = flags + N_STATUS;
    {   // W64_J = [[W_a, 0], [X, W_b]]
        const double* __restrict__ Wa = Winv + (size_t)(2 * J) * NB * NB;
        const double* __restrict__ Wb = Wa + NB * NB;
        const double* __restrict__ X = Xrow + (size_t)J * NB * NB;
        for (int idx = tid; idx < PB * PB; idx += BS_THREADS) {
            const int r = idx >> 6, c = idx & 63;
            Wl[r][c] = r < NB ? (c < NB ? Wa[r * NB + c] : 0.0) : (c < NB ? X[(r - NB) * NB + c] : Wb[(r - NB) * NB + c - NB]);
        }
    }
    if (e0 == e1) {  // the root: it waits for nobody
        __syncthreads();
        if (tid < PB) zl[tid] = -Wl[PB - 1][tid] / Wl[PB - 1][PB - 1];
    } else {
        // The strips of column J are listed nearest ancestor first; they are consumed from the FAR end: those ancestors
        // published long ago, so everything but the parent's strip is summed in the shadow of the chain. A wave polls
        // the hand-off flags itself (no workgroup barrier per strip) and reads the eight z it needs straight from
        // global memory; the strip values (independent of any z) run BS_PF strips ahead.
        double pre[BS_PF][RPT];
        auto fetch = [&](int e, double (&v)[RPT]) {
            const double* __restrict__ A = T + (size_t)ent[e].x * TILE;
#pragma unroll
            for (int r = 0; r < RPT; ++r) v[r] = A[(RPT * g + r) * PB + j];
        };
#pragma unroll
        for (int p = 0; p < BS_PF; ++p)
            if (e1 - 1 - p >= e0) fetch(e1 - 1 - p, pre[p]);
        double acc = 0.0;
        bool late = false;
        for (int base = e1 - 1; base >= e0; base -= BS_PF) {
#pragma unroll
            for (int p = 0; p < BS_PF; ++p) {
                const int e = base - p;
                if (e < e0) break;
                const int I = ent[e].y;
                int spins = 0;
                while (__hip_atomic_load(&handoff[I], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                    if (++spins > (1 << 22)) {
                        late = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the poll
                double zr[RPT];
#pragma unroll
                for (int r = 0; r < RPT; ++r) zr[r] = __hip_atomic_load(&z[(size_t)I * PB + RPT * g + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int r = 0; r < RPT; ++r) acc += pre[p][r] * zr[r];
                if (e - BS_PF >= e0) fetch(e - BS_PF, pre[p]);
            }
        }
        if (late && (tid & 63) == 0) atomicOr(flags, 4);
        part[g][j] = acc;
        __syncthreads();
        if (tid < PB) {
            double tot = 0.0;
#pragma unroll
            for (int q = 0; q < BS_THREADS / PB; ++q) tot += part[q][tid];
            tl[tid] = -tot;
        }
        __syncthreads();
        {   // u = W t: output i on 8 lanes, eight terms per lane (W is lower triangular: the rest are stored zeros)
            const int i = tid >> 3, q = tid & 7;
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v += Wl[i][8 * q + k] * tl[8 * q + k];
            v = dpp_row_sum<8>(v);
            if (q == 7) ul[i] = v;
        }
        __syncthreads();
        {   // z = W^T u
            const int c = tid >> 3, q = tid & 7;
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v += Wl[8 * q + k][c] * ul[8 * q + k];
            v = dpp_row_sum<8>(v);
            if (q == 7) zl[c] = v;
        }
    }
    __syncthreads();
    // publication by ONE wave: its stores drain (vmcnt(0)) before its lane 0 raises the flag — no workgroup barrier
    if (tid < PB) {
        __hip_atomic_store(&z[(size_t)J * PB + tid], zl[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int dst = col_dest[J * PB + tid];
        if (dst >= 0) delta_c[dst] = zl[tid];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0 && !(BA_FAULT(1) && e0 == e1)) __hip_atomic_store(&handoff[J], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- K-F / K-G: the tail of a tryLambda() in ONE launch ----------------------------------------------------------
// landmark back-substitution + tentative points + linearised-cost terms, the retraction of the cameras and K with their
// prior errors, the nonlinear error at the tentative values, and the final sums:
//   delta_l = Linv^T (gt - sum_o Et_o^T dc[c_o] - EKt^T dK);  lin += 1/2 (dl.gl + lambda dl.D dl)
//   error   = sum_o rho(|r_o(x (+) dc, l + dl, K + dK)|) + priors
// Until round 3 these were three dependent launches (back-substitution + retraction, error pass over the retracted poses,
// one-block final sums): 34 us of 0.48 ms on S200, 16 of 118 us on a local window. The error pass only waited for
// pose_new — so a landmark's thread retracts the pose of each of its observations' cameras itself (the same instructions on
// the same inputs as the retraction workgroups, which still write pose_new / K_new for the next linearisation) — and the
// final sums are made by whichever workgroup of the launch finishes LAST. The hand-over is fence-free like the
// back-substitution's: partial sums are stored write-through (agent-scope atomic stores), the storing wave drains,
// one lane takes a ticket from an agent-scope counter; the workgroup that draws the last ticket reads every partial with
// agent-scope atomic loads and adds them in index order — the same order whichever workgroup that is: the sums stay
// deterministic. The counter resets itself.
__device__ __forceinline__ void retract_pose(const double* x, const double* d, double* y) {  // x (+) [omega, v], first-order chart (Cayley)
    double C[9];
    cayley(d, C);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) y[3 * i + j] = x[3 * i] * C[j] + x[3 * i + 1] * C[3 + j] + x[3 * i + 2] * C[6 + j];
    for (int i = 0; i < 3; ++i) y[9 + i] = x[9 + i] + x[3 * i] * d[3] + x[3 * i + 1] * d[4] + x[3 * i + 2] * d[5];
}

__device__ __forceinline__ void store_wt(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double load_wt(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Every thread of the workgroup calls it after the workgroup's write-through stores; true in the workgroup that arrives last.
__device__ __forceinline__ bool last_workgroup(int* counter) {
    __shared__ int last_flag;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's partials have left for memory
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = t == (int)gridDim.x - 1;
        if (last_flag) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return last_flag != 0;
}

// ---- K-G1: retract cameras + K, pose/K prior errors and their linearised-cost terms (thread = camera) --
// err_cam[c] = prior error at the NEW pose; lin_cam[c] = 1/2 (dc.gc + lambda dc.D dc); slot nc = K.
__device__ __forceinline__ void retract_camera(const BaDev& D, int c, double lambda, const double* pose_in, double* pose_out,
                                               const double* K_in, double* K_out, int apply_delta, double* err_cam,
                                               double* lin_cam) {
    if (c < D.nc) {
        const double* x = pose_in + 12 * (size_t)c;
        double y[12];
        double lin = 0.0;
        if (apply_delta) {
            const double* d = D.delta_c + 6 * (size_t)c;
            retract_pose(x, d, y);
            const double* cl = D.camlin + (size_t)CAMLIN * c;
            for (int a = 0; a < 6; ++a) lin += 0.5 * d[a] * cl[66 + a] + 0.5 * lambda * clampd(cl[7 * a], 1e-6, 1e32) * d[a] * d[a];
        } else {
            for (int k = 0; k < 12; ++k) y[k] = x[k];
        }
        for (int k = 0; k < 12; ++k) pose_out[12 * (size_t)c + k] = y[k];
        double xi[6], n2 = 0.0;
        pose_local(y, D.pose0 + 12 * (size_t)c, xi);
        const bool fx = D.fixed[c] != 0;
        const double* sg = fx ? D.nz.fixed_sigma : D.nz.pose_sigma;
        for (int k = 0; k < 6; ++k) n2 += (xi[k] / sg[k]) * (xi[k] / sg[k]);
        store_wt(&err_cam[c], fx ? 0.5 * n2 : huber_loss(sqrt(n2), D.nz.pose_huber));
        store_wt(&lin_cam[c], lin);
    } else if (c == D.nc) {
        double e = 0.0, lin = 0.0;
        for (int a = 0; a < 5; ++a) {
            const double d = apply_delta ? D.delta_c[6 * D.nc + a] : 0.0;
            const double kn = K_in[a] + d;
            K_out[a] = kn;
            const double w = (kn - D.K0[a]) / D.nz.k_sigma[a];
            e += 0.5 * w * w;
            if (apply_delta) lin += 0.5 * d * D.klin[25 + a] + 0.5 * lambda * clampd(D.klin[6 * a], 1e-6, 1e32) * d * d;
        }
        store_wt(&err_cam[D.nc], e);
        store_wt(&lin_cam[D.nc], lin);
    }
}
__global__ void ba_retract_cameras(BaDev D, double lambda, const double* pose_in, double* pose_out,
                                   const double* K_in, double* K_out, int apply_delta, double* err_cam,
                                   double* lin_cam) {
    retract_camera(D, blockIdx.x * blockDim.x + threadIdx.x, lambda, pose_in, pose_out, K_in, K_out, apply_delta, err_cam, lin_cam);
}

// ---- K-G3: fixed-order final sums -> scal[0] = error, scal[1] = linearised cost change; one workgroup, all its threads ----
// n_err / n_lin = workgroups that left a partial in err_part / lin_part (n_lin = 0: no linearised-cost term in this pass)
__device__ __forceinline__ void final_sums(const BaDev& D, const double* err_cam, const double* lin_cam, int n_err, int n_lin,
                                           double ticket, double* sm /* [(TPB / 64) * 2] */) {
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n_err; i += TPB) v[0] += load_wt(&D.err_part[i]);
    for (int i = threadIdx.x; i < n_lin; i += TPB) v[1] += load_wt(&D.lin_part[i]);
    for (int i = threadIdx.x; i <= D.nc; i += TPB) {
        v[0] += load_wt(&err_cam[i]);
        if (n_lin) v[1] += load_wt(&lin_cam[i]);
    }
    block_sum<2>(v, sm);
    // The status word and the hand-off flags of the back-substitution are consumed here, so they are also cleared here
    // for the next tryLambda(), and the three scalars go to pinned host memory as well: a memset node and a
    // device-to-host copy less on the chain of every LM inner iteration.
    if (threadIdx.x == 0) {
        const double st = (double)D.flags[0];
        D.scal[0] = v[0];
        D.scal[1] = v[1];
        D.scal[2] = st;
        if (D.scal_pinned) {  // the host polls slot 3 for this launch's ticket (read_scal): the values first, fenced
            D.scal_pinned[0] = v[0];
            D.scal_pinned[1] = v[1];
            D.scal_pinned[2] = st;
            __threadfence_system();
            *(volatile double*)&D.scal_pinned[3] = ticket;
        }
    }
    for (int k = threadIdx.x; k < N_STATUS + D.sp_npan; k += TPB) D.flags[k] = 0;  // (thread 0 read flags[0] above, in program order)
}

// nonlinear error of a landmark's reprojection factors (this lane's share of them) + its prior (lane sub == 0).
// RETRACT: the poses are D.pose (+) delta_c, retracted here; else `pose` as given.
template <int LPL, bool RETRACT>
__device__ __forceinline__ double landmark_error(const BaDev& D, int j, int sub, const double* __restrict__ pose, const double (&l)[3],
                                                 const double (&K)[5]) {
    const int o0 = D.lm_ptr[j], o1 = D.lm_ptr[j + 1];
    double e = 0.0;
    for (int o = o0 + sub; o < o1; o += LPL) {
        const int cam = (int)D.obs_cam[o];
        const double* x = pose + 12 * (size_t)cam;
        double xr[12], r[2];
#pragma unroll
        for (int k = 0; k < 12; ++k) xr[k] = x[k];
        if (RETRACT) {
            double y[12];
            retract_pose(xr, D.delta_c + 6 * (size_t)cam, y);
#pragma unroll
            for (int k = 0; k < 12; ++k) xr[k] = y[k];
        }
        reproj<false>(xr, l, K, D.obs_uv[2 * (size_t)o], D.obs_uv[2 * (size_t)o + 1], r, nullptr, nullptr, nullptr);
        e += huber_loss(sqrt(r[0] * r[0] + r[1] * r[1]) / D.nz.pix_sigma, D.nz.pix_huber);
    }
    if (sub == 0) {  // the landmark's prior, once
        const double sg = D.lmprior[2 * j], kh = D.lmprior[2 * j + 1];
        double n2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double w = (l[a] - D.pt0[3 * (size_t)j + a]) / sg;
            n2 += w * w;
        }
        e += huber_loss(sqrt(n2), kh);
    }
    return e;
}

// The tail of a tryLambda(). Grid = the landmark workgroups, then the workgroups that retract the cameras and K.
template <int LPL>
__global__ __launch_bounds__(TPB) void ba_step_landmarks(BaDev D, double lambda, double* err_cam, double* lin_cam, double ticket) {
    __shared__ double sm[(TPB / 64) * 2];
    if ((int)blockIdx.x >= D.n_step_blocks) {
        retract_camera(D, ((int)blockIdx.x - D.n_step_blocks) * TPB + threadIdx.x, lambda, D.pose, D.pose_new, D.Kc, D.K_new, 1, err_cam, lin_cam);
    } else {
        const int gid = blockIdx.x * TPB + threadIdx.x, j = gid / LPL, sub = gid % LPL;
        double lin[1] = {0.0}, dl[3] = {0.0, 0.0, 0.0};
        if (j < D.nl) {
            const int o0 = D.lm_ptr[j], o1 = D.lm_ptr[j + 1];
            double d0 = 0.0, d1 = 0.0, d2 = 0.0;
            if (o1 > o0) {
                const double* lt = D.lmtry + (size_t)LMLIN * j;
                double t0 = lt[6], t1 = lt[7], t2 = lt[8];
                const double* dK = D.delta_c + 6 * D.nc;
    #pragma unroll
                for (int a = 0; a < 5; ++a) {
                    t0 -= lt[9 + 3 * a] * dK[a];
                    t1 -= lt[10 + 3 * a] * dK[a];
                    t2 -= lt[11 + 3 * a] * dK[a];
                }
                // sum_o Et_o^T dc = Linv sum_o E_o^T dc and E_o^T dc = Al^T (Ap dc): the Jacobians are recomputed at the
                // linearisation point (pose / pt / Kc do not change inside the lambda loop) from this landmark's own
                // observation records instead of gathering its ten 144-byte Et rows out of the camera-ordered array
                // (137 MB of HBM traffic per try, profiles/r02_pmc_ba_traffic.json of the first round-2 build)
                const double l[3] = {D.pt[3 * (size_t)j], D.pt[3 * (size_t)j + 1], D.pt[3 * (size_t)j + 2]};
                double K[5];
    #pragma unroll
                for (int k = 0; k < 5; ++k) K[k] = D.Kc[k];
                double w0 = 0.0, w1 = 0.0, w2 = 0.0;
                for (int o = o0 + sub; o < o1; o += LPL) {
                    const int cam = (int)D.obs_cam[o];
                    const double* x = D.pose + 12 * (size_t)cam;
                    const double* dc = D.delta_c + 6 * (size_t)cam;
                    double xr[12];
    #pragma unroll
                    for (int k = 0; k < 12; ++k) xr[k] = x[k];
                    double Ap[12], Al[6], Ak[10], b[2];
                    obs_factor(xr, l, K, D.obs_uv[2 * (size_t)o], D.obs_uv[2 * (size_t)o + 1], D.nz.pix_sigma, D.nz.pix_huber, Ap, Al, Ak, b);
                    double u0 = 0.0, u1 = 0.0;
    #pragma unroll
                    for (int a = 0; a < 6; ++a) {
                        u0 += Ap[a] * dc[a];
                        u1 += Ap[6 + a] * dc[a];
                    }
                    w0 += Al[0] * u0 + Al[3] * u1;
                    w1 += Al[1] * u0 + Al[4] * u1;
                    w2 += Al[2] * u0 + Al[5] * u1;
                }
                if (LPL > 1) w0 = group_sum<LPL>(w0), w1 = group_sum<LPL>(w1), w2 = group_sum<LPL>(w2);  // (a landmark's lanes take this branch together)
                const double m00 = lt[0], m10 = lt[1], m11 = lt[2], m20 = lt[3], m21 = lt[4], m22 = lt[5];
                t0 -= m00 * w0;
                t1 -= m10 * w0 + m11 * w1;
                t2 -= m20 * w0 + m21 * w1 + m22 * w2;
                d0 = m00 * t0 + m10 * t1 + m20 * t2;
                d1 = m11 * t1 + m21 * t2;
                d2 = m22 * t2;
                const double* in = D.lmlin + (size_t)LMLIN * j;
                if (sub == 0)
                    lin[0] = 0.5 * (d0 * in[6] + d1 * in[7] + d2 * in[8]) +
                             0.5 * lambda * (clampd(in[0], 1e-6, 1e32) * d0 * d0 + clampd(in[3], 1e-6, 1e32) * d1 * d1 +
                                             clampd(in[5], 1e-6, 1e32) * d2 * d2);
            }
            dl[0] = d0, dl[1] = d1, dl[2] = d2;
            if (sub == 0) {
            D.delta_l[3 * (size_t)j] = d0;
            D.delta_l[3 * (size_t)j + 1] = d1;
            D.delta_l[3 * (size_t)j + 2] = d2;
            D.pt_new[3 * (size_t)j] = D.pt[3 * (size_t)j] + d0;
            D.pt_new[3 * (size_t)j + 1] = D.pt[3 * (size_t)j + 1] + d1;
            D.pt_new[3 * (size_t)j + 2] = D.pt[3 * (size_t)j + 2] + d2;
            }
        }
        double v[2] = {0.0, lin[0]};
        if (j < D.nl && D.lm_ptr[j + 1] > D.lm_ptr[j]) {
            const double lnew[3] = {D.pt[3 * (size_t)j] + dl[0], D.pt[3 * (size_t)j + 1] + dl[1], D.pt[3 * (size_t)j + 2] + dl[2]};
            double Kn[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) Kn[a] = D.Kc[a] + D.delta_c[6 * D.nc + a];
            v[0] = landmark_error<LPL, true>(D, j, sub, D.pose, lnew, Kn);
        }
        block_sum<2>(v, sm);
        if (threadIdx.x == 0) {
            store_wt(&D.err_part[blockIdx.x], v[0]);
            store_wt(&D.lin_part[blockIdx.x], v[1]);
        }
    }
    if (last_workgroup(D.sync_counter)) final_sums(D, err_cam, lin_cam, D.n_step_blocks, D.n_step_blocks, ticket, sm);
}

// ---- K-G2: nonlinear error at given values (the first error pass of a solve, DogLeg's candidates, the PCG path): the
// reprojection + landmark-prior factors (thread = landmark); the camera / K prior errors come from ba_retract_cameras,
// launched before it; the last workgroup makes the final sums.
template <int LPL>
__global__ __launch_bounds__(TPB) void ba_error_landmarks(BaDev D, const double* __restrict__ pose, const double* __restrict__ pt,
                                                          const double* __restrict__ Kc, const double* err_cam, const double* lin_cam,
                                                          int n_lin, double ticket) {
    __shared__ double sm[(TPB / 64) * 2];
    const int gid = blockIdx.x * TPB + threadIdx.x, j = gid / LPL, sub = gid % LPL;
    double e[1] = {0.0};
    if (j < D.nl && D.lm_ptr[j + 1] > D.lm_ptr[j]) {
        const double l[3] = {pt[3 * (size_t)j], pt[3 * (size_t)j + 1], pt[3 * (size_t)j + 2]};
        double K[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) K[k] = Kc[k];
        e[0] = landmark_error<LPL, false>(D, j, sub, pose, l, K);
    }
    block_sum<1>(e, sm);
    if (threadIdx.x == 0) store_wt(&D.err_part[blockIdx.x], e[0]);
    if (last_workgroup(D.sync_counter)) final_sums(D, err_cam, lin_cam, D.n_step_blocks, n_lin, ticket, sm);
}

// ---- the iterative solve the reference can select: PCG + block-Jacobi (BundleAdjuster.cpp:192-200) -----------------
// params.linearSolverType = Iterative, PCGSolverParameters{BlockJacobi, epsilon_abs = epsilon_rel = 1e-10}: GTSAM 4.1.1
// runs preconditioned conjugate gradients on the DAMPED system over ALL variables (poses, calibration, landmarks),
// preconditioned by the Cholesky factors of its diagonal blocks, from x0 = 0, until gamma = r^T M^-1 r <=
// max(epsilon_abs, epsilon_rel^2 gamma0) or 500 iterations (gtsam/linear/PCGSolver.cpp, iterative-inl.h; restated from
// memory like SURVEY.md Appendix A). Here the operator is applied in block form on the linearisation that is already
// resident — y_c = (Hcc + lambda Dc) x_c + HcK x_K + sum_o E_o x_l(o), y_l = (Hll + lambda Dl) x_l + ElK^T x_K +
// sum_o E_o^T x_c(o), y_K likewise — with E kept by the linearisation (store_E). Five launches per iteration, every sum
// in a fixed order (no atomics), the scalars (gamma, alpha, beta, the stop flag) stay on the device and the host looks
// at the flag once per batch of iterations: after convergence the remaining launches of a batch return at once.
constexpr int PCG_MAX_IT = 500;
constexpr int PCG_BATCH = 25;

template <int M>
__device__ __forceinline__ bool spd_inverse(const double* A /* M x M, lower used */, double* inv /* M x M full */) {
    double L[M][M], W[M][M];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double d = A[j * M + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0;
        const double sd = sqrt(d > 0.0 ? d : 1.0);
        L[j][j] = sd;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double v = A[i * M + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / sd;
        }
    }
#pragma unroll
    for (int c = 0; c < M; ++c)  // W = L^-1, column by column
#pragma unroll
        for (int i = 0; i < M; ++i) {
            if (i < c) { W[i][c] = 0.0; continue; }
            double v = i == c ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k) v -= L[i][k] * W[k][c];
            W[i][c] = v / L[i][i];
        }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {  // inv = W^T W
            double v = 0.0;
#pragma unroll
            for (int k = (i > j ? i : j); k < M; ++k) v += W[k][i] * W[k][j];
            inv[i * M + j] = v;
        }
    return ok;
}

// x = 0, r = g, z = M^-1 r, p = z; partial gamma. thread = landmark
__global__ __launch_bounds__(TPB) void pcg_setup_landmarks(BaDev D, double lambda) {
    __shared__ double sm[(TPB / 64) * 1];
    const int j = blockIdx.x * TPB + threadIdx.x;
    double g[1] = {0.0};
    if (j < D.nl) {
        double r[3] = {0, 0, 0}, z[3] = {0, 0, 0}, Mi[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, dd[3] = {0, 0, 0};
        if (D.lm_ptr[j + 1] > D.lm_ptr[j]) {
            const double* in = D.lmlin + (size_t)LMLIN * j;
            dd[0] = clampd(in[0], 1e-6, 1e32), dd[1] = clampd(in[3], 1e-6, 1e32), dd[2] = clampd(in[5], 1e-6, 1e32);
            const double A[9] = {in[0] + lambda * dd[0], in[1], in[2], in[1], in[3] + lambda * dd[1], in[4], in[2], in[4], in[5] + lambda * dd[2]};
            if (!spd_inverse<3>(A, Mi)) atomicOr(D.flags, 1);
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] = in[6 + a];
#pragma unroll
            for (int a = 0; a < 3; ++a) z[a] = Mi[3 * a] * r[0] + Mi[3 * a + 1] * r[1] + Mi[3 * a + 2] * r[2];
            g[0] = r[0] * z[0] + r[1] * z[1] + r[2] * z[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            D.pcg_Dl[3 * (size_t)j + a] = dd[a];
            D.pcg_rl[3 * (size_t)j + a] = r[a];
            D.pcg_zl[3 * (size_t)j + a] = z[a];
            D.pcg_pl[3 * (size_t)j + a] = z[a];
            D.delta_l[3 * (size_t)j + a] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) D.pcg_Ml[9 * (size_t)j + k] = Mi[k];
    }
    block_sum<1>(g, sm);
    if (threadIdx.x == 0) D.pcg_p3[blockIdx.x] = g[0];
}

// the same for the cameras (thread = camera) and the calibration (thread nc); one block: also the scalars
__global__ __launch_bounds__(1024) void pcg_setup_cameras(BaDev D, double lambda) {
    __shared__ double red[1024 / 64];
    double g = 0.0;
    for (int c = threadIdx.x; c <= D.nc; c += blockDim.x) {
        if (c < D.nc) {
            const double* cl = D.camlin + (size_t)CAMLIN * c;
            double A[36], Mi[36], r[6], z[6];
#pragma unroll
            for (int k = 0; k < 36; ++k) A[k] = cl[k];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double dd = clampd(cl[7 * a], 1e-6, 1e32);
                D.pcg_Dc[6 * (size_t)c + a] = dd;
                A[7 * a] += lambda * dd;
                r[a] = cl[66 + a];
            }
            if (!spd_inverse<6>(A, Mi)) atomicOr(D.flags, 2);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double v = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) v += Mi[6 * a + b] * r[b];
                z[a] = v;
                g += r[a] * v;
            }
#pragma unroll
            for (int k = 0; k < 36; ++k) D.pcg_Mc[36 * (size_t)c + k] = Mi[k];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                D.pcg_rc[6 * (size_t)c + a] = r[a];
                D.pcg_zc[6 * (size_t)c + a] = z[a];
                D.pcg_pc[6 * (size_t)c + a] = z[a];
                D.delta_c[6 * (size_t)c + a] = 0.0;
            }
        } else {
            double A[25], Mi[25], r[5];
#pragma unroll
            for (int k = 0; k < 25; ++k) A[k] = D.klin[k];
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                const double dd = clampd(D.klin[6 * a], 1e-6, 1e32);
                D.pcg_Dc[6 * (size_t)D.nc + a] = dd;
                A[6 * a] += lambda * dd;
                r[a] = D.klin[25 + a];
            }
            if (!spd_inverse<5>(A, Mi)) atomicOr(D.flags, 2);
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                double v = 0.0;
#pragma unroll
                for (int b = 0; b < 5; ++b) v += Mi[5 * a + b] * r[b];
                g += r[a] * v;
                D.pcg_rc[6 * (size_t)D.nc + a] = r[a];
                D.pcg_zc[6 * (size_t)D.nc + a] = v;
                D.pcg_pc[6 * (size_t)D.nc + a] = v;
                D.delta_c[6 * (size_t)D.nc + a] = 0.0;
            }
#pragma unroll
            for (int k = 0; k < 25; ++k) D.pcg_MK[k] = Mi[k];
        }
    }
    for (int i = threadIdx.x; i < D.n_lm_blocks; i += blockDim.x) g += D.pcg_p3[i];  // the landmarks' partial gammas
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) g += __shfl_down(g, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < 1024 / 64; ++w) tot += red[w];
        D.pcg_s[0] = tot;                                   // gamma
        D.pcg_s[1] = fmax(1e-10, 1e-10 * 1e-10 * tot);      // max(epsilon_abs, epsilon_rel^2 gamma0)
        D.pcg_s[2] = D.pcg_s[3] = 0.0;
        D.pcg_s[4] = 0.0;                                   // done
        D.pcg_s[5] = 0.0;                                   // iterations
    }
}

// 1/5: p_l <- z_l + beta p_l (not in the first iteration); q_l = A_ll p_l + ElK^T p_K + sum_o E_o^T p_c(o); partials of p_l.q_l and ElK p_l
__global__ __launch_bounds__(TPB) void pcg_apply_landmarks(BaDev D, double lambda) {
    __shared__ double sm[(TPB / 64) * 6];
    if (D.pcg_s[4] != 0.0) return;
    const int j = blockIdx.x * TPB + threadIdx.x;
    const double beta = D.pcg_s[3];
    const bool first = D.pcg_s[5] == 0.0;
    double part[6] = {0, 0, 0, 0, 0, 0};
    if (j < D.nl) {
        const int o0 = D.lm_ptr[j], o1 = D.lm_ptr[j + 1];
        double pl[3], q[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double pv = D.pcg_pl[3 * (size_t)j + a];
            pl[a] = first ? pv : D.pcg_zl[3 * (size_t)j + a] + beta * pv;
            D.pcg_pl[3 * (size_t)j + a] = pl[a];
        }
        if (o1 > o0) {
            const double* in = D.lmlin + (size_t)LMLIN * j;
            const double* pK = D.pcg_pc + 6 * (size_t)D.nc;
            const double* dd = D.pcg_Dl + 3 * (size_t)j;
            q[0] = (in[0] + lambda * dd[0]) * pl[0] + in[1] * pl[1] + in[2] * pl[2];
            q[1] = in[1] * pl[0] + (in[3] + lambda * dd[1]) * pl[1] + in[4] * pl[2];
            q[2] = in[2] * pl[0] + in[4] * pl[1] + (in[5] + lambda * dd[2]) * pl[2];
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                const double e0 = in[9 + 3 * a], e1 = in[10 + 3 * a], e2 = in[11 + 3 * a];
                q[0] += e0 * pK[a], q[1] += e1 * pK[a], q[2] += e2 * pK[a];
                part[1 + a] = e0 * pl[0] + e1 * pl[1] + e2 * pl[2];  // (ElK p_l)[a]
            }
            for (int o = o0; o < o1; ++o) {
                const double* E = D.E + 18 * (size_t)D.obs_pos[o];
                const double* pc = D.pcg_pc + 6 * (size_t)D.obs_cam[o];
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    q[0] += E[3 * a] * pc[a];
                    q[1] += E[3 * a + 1] * pc[a];
                    q[2] += E[3 * a + 2] * pc[a];
                }
            }
            part[0] = pl[0] * q[0] + pl[1] * q[1] + pl[2] * q[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) D.pcg_ql[3 * (size_t)j + a] = q[a];
    }
    block_sum<6>(part, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) D.pcg_p1[6 * (size_t)blockIdx.x + k] = part[k];
}

// 2/5: per camera-aligned chunk: sum_o E_o p_l(o) (6 values)
__global__ __launch_bounds__(TPB) void pcg_apply_cam_chunks(BaDev D) {
    __shared__ double sm[(TPB / 64) * 6];
    if (D.pcg_s[4] != 0.0) return;
    const int2 ch = D.cam_chunks[blockIdx.x];
    double v[6] = {0, 0, 0, 0, 0, 0};
    if ((int)threadIdx.x < ch.y) {
        const int p = ch.x + threadIdx.x;
        const double* E = D.E + 18 * (size_t)p;
        const double* pl = D.pcg_pl + 3 * (size_t)D.cam_lm[p];
        const double p0 = pl[0], p1 = pl[1], p2 = pl[2];
#pragma unroll
        for (int a = 0; a < 6; ++a) v[a] = E[3 * a] * p0 + E[3 * a + 1] * p1 + E[3 * a + 2] * p2;
    }
    block_sum<6>(v, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) D.pcg_p2[6 * (size_t)blockIdx.x + k] = v[k];
}

// 3/5 (one block): q_c, q_K, p.q and alpha = gamma / p.q
__global__ __launch_bounds__(1024) void pcg_apply_finish(BaDev D, double lambda) {
    __shared__ double red[1024 / 64][6];
    if (D.pcg_s[4] != 0.0) return;
    const double* pK = D.pcg_pc + 6 * (size_t)D.nc;
    double acc[6] = {0, 0, 0, 0, 0, 0};  // p.q | HcK^T p_c + ElK p_l partials (5)
    for (int c = threadIdx.x; c < D.nc; c += blockDim.x) {
        const double* cl = D.camlin + (size_t)CAMLIN * c;
        const double* pc = D.pcg_pc + 6 * (size_t)c;
        double q[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double v = lambda * D.pcg_Dc[6 * (size_t)c + a] * pc[a];
#pragma unroll
            for (int b = 0; b < 6; ++b) v += cl[6 * a + b] * pc[b];
#pragma unroll
            for (int b = 0; b < 5; ++b) v += cl[36 + 5 * a + b] * pK[b];
            q[a] = v;
        }
        for (int chn = D.cam_chunk_ptr[c]; chn < D.cam_chunk_ptr[c + 1]; ++chn)
#pragma unroll
            for (int a = 0; a < 6; ++a) q[a] += D.pcg_p2[6 * (size_t)chn + a];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            D.pcg_qc[6 * (size_t)c + a] = q[a];
            acc[0] += pc[a] * q[a];
#pragma unroll
            for (int b = 0; b < 5; ++b) acc[1 + b] += cl[36 + 5 * a + b] * pc[a];
        }
    }
    for (int i = threadIdx.x; i < D.n_lm_blocks; i += blockDim.x)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += D.pcg_p1[6 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double x = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[6] = {0, 0, 0, 0, 0, 0};
        for (int w = 0; w < 1024 / 64; ++w)
            for (int k = 0; k < 6; ++k) tot[k] += red[w][k];
        double pq = tot[0];
        for (int a = 0; a < 5; ++a) {
            double v = lambda * D.pcg_Dc[6 * (size_t)D.nc + a] * pK[a] + tot[1 + a];
            for (int b = 0; b < 5; ++b) v += D.klin[5 * a + b] * pK[b];
            D.pcg_qc[6 * (size_t)D.nc + a] = v;
            pq += pK[a] * v;
        }
        D.pcg_s[6] = pq;
        D.pcg_s[2] = D.pcg_s[0] / pq;  // alpha
    }
}

// 4/5: x += alpha p, r -= alpha q, z = M^-1 r, partial r.z; threads [0, nl) landmarks, then cameras + K
__global__ __launch_bounds__(TPB) void pcg_update(BaDev D) {
    __shared__ double sm[(TPB / 64) * 1];
    if (D.pcg_s[4] != 0.0) return;
    const double alpha = D.pcg_s[2];
    const int idx = blockIdx.x * TPB + threadIdx.x;
    double g[1] = {0.0};
    if (idx < D.nl) {
        const size_t b = 3 * (size_t)idx;
        double r[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            D.delta_l[b + a] += alpha * D.pcg_pl[b + a];
            r[a] = D.pcg_rl[b + a] - alpha * D.pcg_ql[b + a];
            D.pcg_rl[b + a] = r[a];
        }
        const double* Mi = D.pcg_Ml + 9 * (size_t)idx;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double z = Mi[3 * a] * r[0] + Mi[3 * a + 1] * r[1] + Mi[3 * a + 2] * r[2];
            D.pcg_zl[b + a] = z;
            g[0] += r[a] * z;
        }
    } else if (idx - D.nl <= D.nc) {
        const int c = idx - D.nl, m = c < D.nc ? 6 : 5;
        const size_t b = 6 * (size_t)c;
        const double* Mi = c < D.nc ? D.pcg_Mc + 36 * (size_t)c : D.pcg_MK;
        double r[6] = {0, 0, 0, 0, 0, 0};
        for (int a = 0; a < m; ++a) {
            D.delta_c[b + a] += alpha * D.pcg_pc[b + a];
            r[a] = D.pcg_rc[b + a] - alpha * D.pcg_qc[b + a];
            D.pcg_rc[b + a] = r[a];
        }
        for (int a = 0; a < m; ++a) {
            double z = 0.0;
            for (int k = 0; k < m; ++k) z += Mi[m * a + k] * r[k];
            D.pcg_zc[b + a] = z;
            g[0] += r[a] * z;
        }
    }
    block_sum<1>(g, sm);
    if (threadIdx.x == 0) D.pcg_p3[blockIdx.x] = g[0];
}

// 5/5 (one block): gamma', beta, the stop test, p_c <- z_c + beta p_c (p_l follows in 1/5 of the next iteration)
__global__ __launch_bounds__(1024) void pcg_update_finish(BaDev D, int n_update_blocks) {
    __shared__ double red[1024 / 64];
    __shared__ double s_beta;
    if (D.pcg_s[4] != 0.0) return;
    double g = 0.0;
    for (int i = threadIdx.x; i < n_update_blocks; i += blockDim.x) g += D.pcg_p3[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) g += __shfl_down(g, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < 1024 / 64; ++w) tot += red[w];
        const double beta = tot / D.pcg_s[0];
        const double it = D.pcg_s[5] + 1.0;
        D.pcg_s[0] = tot;
        D.pcg_s[3] = beta;
        D.pcg_s[5] = it;
        // for (k = 1; k <= maxIterations && (gamma > threshold || k <= minIterations); ++k), minIterations = 1
        if (!(tot > D.pcg_s[1]) || it >= (double)PCG_MAX_IT || !(tot == tot)) D.pcg_s[4] = 1.0;
        s_beta = beta;
    }
    __syncthreads();
    const double beta = s_beta;
    for (int i = threadIdx.x; i < D.n; i += blockDim.x) D.pcg_pc[i] = D.pcg_zc[i] + beta * D.pcg_pc[i];
}

// tentative points + the landmarks' linearised-cost terms from the PCG step (the role K-F has for the direct solve)
__global__ __launch_bounds__(TPB) void pcg_landmark_step(BaDev D, double lambda) {
    __shared__ double sm[(TPB / 64) * 1];
    const int j = blockIdx.x * TPB + threadIdx.x;
    double lin[1] = {0.0};
    if (j < D.nl) {
        const bool used = D.lm_ptr[j + 1] > D.lm_ptr[j];
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            d[a] = used ? D.delta_l[3 * (size_t)j + a] : 0.0;
            D.delta_l[3 * (size_t)j + a] = d[a];
            D.pt_new[3 * (size_t)j + a] = D.pt[3 * (size_t)j + a] + d[a];
        }
        if (used) {
            const double* in = D.lmlin + (size_t)LMLIN * j;
            lin[0] = 0.5 * (d[0] * in[6] + d[1] * in[7] + d[2] * in[8]) +
                     0.5 * lambda * (clampd(in[0], 1e-6, 1e32) * d[0] * d[0] + clampd(in[3], 1e-6, 1e32) * d[1] * d[1] +
                                     clampd(in[5], 1e-6, 1e32) * d[2] * d[2]);
        }
    }
    block_sum<1>(lin, sm);
    if (threadIdx.x == 0) D.lin_part[blockIdx.x] = lin[0];
}

// ---- DogLeg (GTSAM DoglegOptimizerImpl): scalar forms of the steepest-descent direction g = A^T b and the
// Gauss-Newton step n on the UNDAMPED linearised system H = A^T A (blocks of K-A/K-B), all sums in
// fixed order. forms = {g.g, g.n, n.n, g^T H g, g^T H n, n^T H n}; landmark part here, thread = landmark.
__global__ __launch_bounds__(TPB) void ba_dl_forms_landmarks(BaDev D) {
    __shared__ double sm[(TPB / 64) * 6];
    const int j = blockIdx.x * TPB + threadIdx.x;
    double f[6] = {0, 0, 0, 0, 0, 0};
    if (j < D.nl) {
        const int o0 = D.lm_ptr[j], o1 = D.lm_ptr[j + 1];
        if (o1 > o0) {
            const double* in = D.lmlin + (size_t)LMLIN * j;
            const double gl[3] = {in[6], in[7], in[8]};
            const double nl[3] = {D.dl_nl[3 * (size_t)j], D.dl_nl[3 * (size_t)j + 1], D.dl_nl[3 * (size_t)j + 2]};
            const double* gK = D.klin + 25;
            const double* nK = D.dl_nc + 6 * D.nc;
            // a_x = ElK^T x_K + sum_o E_o^T x_c(o): the part of H x that lands on this landmark from cameras and K
            double ag[3] = {0, 0, 0}, an[3] = {0, 0, 0};
#pragma unroll
            for (int a = 0; a < 5; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    ag[c] += in[9 + 3 * a + c] * gK[a];
                    an[c] += in[9 + 3 * a + c] * nK[a];
                }
            for (int o = o0; o < o1; ++o) {
                const double* E = D.E + 18 * (size_t)D.obs_pos[o];
                const int cam = (int)D.obs_cam[o];
                const double* gc = D.camlin + (size_t)CAMLIN * cam + 66;
                const double* nc = D.dl_nc + 6 * (size_t)cam;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        ag[c] += E[3 * a + c] * gc[a];
                        an[c] += E[3 * a + c] * nc[a];
                    }
            }
            const double H00 = in[0], H01 = in[1], H02 = in[2], H11 = in[3], H12 = in[4], H22 = in[5];
            const double hg[3] = {H00 * gl[0] + H01 * gl[1] + H02 * gl[2], H01 * gl[0] + H11 * gl[1] + H12 * gl[2],
                                  H02 * gl[0] + H12 * gl[1] + H22 * gl[2]};
            const double hn[3] = {H00 * nl[0] + H01 * nl[1] + H02 * nl[2], H01 * nl[0] + H11 * nl[1] + H12 * nl[2],
                                  H02 * nl[0] + H12 * nl[1] + H22 * nl[2]};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f[0] += gl[c] * gl[c];
                f[1] += gl[c] * nl[c];
                f[2] += nl[c] * nl[c];
                f[3] += gl[c] * hg[c] + 2.0 * ag[c] * gl[c];
                f[4] += gl[c] * hn[c] + ag[c] * nl[c] + an[c] * gl[c];
                f[5] += nl[c] * hn[c] + 2.0 * an[c] * nl[c];
            }
        }
    }
    block_sum<6>(f, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) D.dl_part[6 * (size_t)blockIdx.x + k] = f[k];
}

// camera + K part and the final fixed-order sums -> scal[4..9]
__global__ __launch_bounds__(TPB) void ba_dl_forms_final(BaDev D) {
    __shared__ double sm[(TPB / 64) * 6];
    double f[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < D.n_lm_blocks; i += TPB)
        for (int k = 0; k < 6; ++k) f[k] += D.dl_part[6 * (size_t)i + k];
    const double* gK = D.klin + 25;
    const double* nK = D.dl_nc + 6 * D.nc;
    for (int c = threadIdx.x; c < D.nc; c += TPB) {
        const double* cl = D.camlin + (size_t)CAMLIN * c;
        const double* gc = cl + 66;
        const double* nc = D.dl_nc + 6 * (size_t)c;
        double hg[6], hn[6];  // Hcc x_c + HcK x_K
        for (int a = 0; a < 6; ++a) {
            double sg = 0.0, sn = 0.0;
            for (int b = 0; b < 6; ++b) {
                sg += cl[6 * a + b] * gc[b];
                sn += cl[6 * a + b] * nc[b];
            }
            double kg = 0.0, kn = 0.0;
            for (int b = 0; b < 5; ++b) {
                kg += cl[36 + 5 * a + b] * gK[b];
                kn += cl[36 + 5 * a + b] * nK[b];
            }
            hg[a] = sg + 2.0 * kg;  // x_c^T Hcc y_c + x_c^T HcK y_K + y_c^T HcK x_K, folded per form below
            hn[a] = sn + 2.0 * kn;
            f[0] += gc[a] * gc[a];
            f[1] += gc[a] * nc[a];
            f[2] += nc[a] * nc[a];
            f[3] += gc[a] * hg[a];
            f[4] += gc[a] * (sn + kn) + nc[a] * kg;
            f[5] += nc[a] * hn[a];
        }
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < 5; ++a) {
            double sg = 0.0, sn = 0.0;
            for (int b = 0; b < 5; ++b) {
                sg += D.klin[5 * a + b] * gK[b];
                sn += D.klin[5 * a + b] * nK[b];
            }
            f[0] += gK[a] * gK[a];
            f[1] += gK[a] * nK[a];
            f[2] += nK[a] * nK[a];
            f[3] += gK[a] * sg;
            f[4] += gK[a] * sn;
            f[5] += nK[a] * sn;
        }
    }
    block_sum<6>(f, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) D.scal[4 + k] = f[k];
}

// x_d = cu * g + cn * n -> delta_c / delta_l (the inputs of the retraction and error kernels) and pt_new
__global__ __launch_bounds__(TPB) void ba_dl_apply(BaDev D, double cu, double cn) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < 3 * D.nl) {
        const int j = i / 3;
        const double g = D.lm_ptr[j + 1] > D.lm_ptr[j] ? D.lmlin[(size_t)LMLIN * j + 6 + i % 3] : 0.0;
        const double d = cu * g + cn * D.dl_nl[i];
        D.delta_l[i] = d;
        D.pt_new[i] = D.pt[i] + d;
    }
    if (i < D.n) {
        const double g = i < 6 * D.nc ? D.camlin[(size_t)CAMLIN * (i / 6) + 66 + i % 6] : D.klin[25 + (i - 6 * D.nc)];
        D.delta_c[i] = cu * g + cn * D.dl_nc[i];
    }
}

}  // namespace eacham

// ====================================================================================================
// host side
// ====================================================================================================
using namespace eacham;

namespace eacham {

static void pose_to_Twc(const double* x, double* T) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = x[3 * j + i];
        T[4 * i + 3] = -(x[i] * x[9] + x[3 + i] * x[10] + x[6 + i] * x[11]);
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

// The solver's work arrays, declared where their records are defined: two parts of the allocation sequences that ba_prepare.hip
// runs over a problem's arenas (each sequence runs twice: sizes first, h->arena.base == nullptr, then pointers). Part a is sized
// by (nc, nl, no); part b by the plan and the form of the Schur stage, and needs the structure's counts in BaDev.
int ba_alloc_work_a(eacham_ctx* ctx, eacham_ba_handle* h) {
    BaDev& D = h->D;
    const int nc = D.nc, nl = D.nl, no = D.no;
    dev_alloc(h, &D.pose, 12 * (size_t)nc);
    dev_alloc(h, &D.pose_new, 12 * (size_t)nc);
    dev_alloc(h, &D.pt, 3 * (size_t)nl);
    dev_alloc(h, &D.pt_new, 3 * (size_t)nl);
    dev_alloc(h, &D.Kc, 8);
    dev_alloc(h, &D.K_new, 8);
    dev_alloc(h, &D.E, 18 * (size_t)no);
    dev_alloc(h, &D.Et, 18 * (size_t)no);
    dev_alloc(h, &D.lmlin, (size_t)LMLIN * nl);
    dev_alloc(h, &D.lmtry, (size_t)LMLIN * nl);
    dev_alloc(h, &D.camlin, (size_t)CAMLIN * nc);
    dev_alloc(h, &D.klin, (size_t)KLIN);
    dev_alloc(h, &h->kpart, (size_t)CLP * LSEG * std::max(nc, 1));
    dev_alloc(h, &D.kk_part, (size_t)30 * D.n_lm_blocks);
    dev_alloc(h, &D.delta_c, (size_t)D.n + 8);
    dev_alloc(h, &D.delta_l, 3 * (size_t)nl);
    dev_alloc(h, &D.err_part, (size_t)std::max(D.n_ll_blocks, D.n_step_blocks));
    dev_alloc(h, &D.lin_part, (size_t)std::max(std::max(D.n_ll_blocks, D.n_step_blocks), D.n_lm_blocks));
    dev_alloc(h, &h->err_cam, (size_t)nc + 1);
    dev_alloc(h, &h->lin_cam, (size_t)nc + 1);
    dev_alloc(h, &D.scal, (size_t)SCAL);
    dev_alloc(h, &D.dl_nc, (size_t)D.n);
    dev_alloc(h, &D.dl_nl, (size_t)3 * D.nl);
    dev_alloc(h, &D.dl_part, (size_t)6 * D.n_lm_blocks);
    {
        const size_t nn = (size_t)D.n + 8, n3 = 3 * (size_t)std::max(nl, 1);
        dev_alloc(h, &D.pcg_rc, nn); dev_alloc(h, &D.pcg_zc, nn); dev_alloc(h, &D.pcg_pc, nn);
        dev_alloc(h, &D.pcg_qc, nn); dev_alloc(h, &D.pcg_Dc, nn);
        dev_alloc(h, &D.pcg_rl, n3); dev_alloc(h, &D.pcg_zl, n3); dev_alloc(h, &D.pcg_pl, n3);
        dev_alloc(h, &D.pcg_ql, n3); dev_alloc(h, &D.pcg_Dl, n3);
        dev_alloc(h, &D.pcg_Mc, (size_t)36 * std::max(nc, 1)); dev_alloc(h, &D.pcg_MK, 32);
        dev_alloc(h, &D.pcg_Ml, 3 * n3);
        dev_alloc(h, &D.pcg_p1, (size_t)6 * D.n_lm_blocks);
        dev_alloc(h, &D.pcg_p3, (size_t)D.n_lm_blocks + (size_t)(nc + 1 + TPB) / TPB + 2); dev_alloc(h, &D.pcg_s, 16);
    }
    dev_alloc(h, &D.sync_counter, 4);
    if (h->arena.base) {
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(D.sync_counter, 0, 4 * sizeof(int), ctx->stream));
        h->scal_host = ctx->ba_pool[h->block].pinned;
        EACHAM_HIP_TRY(ctx, hipHostGetDevicePointer((void**)&D.scal_pinned, h->scal_host, 0));
        for (int k = 0; k < SCAL; ++k) h->scal_host[k] = 0.0;  // (tickets start at 1; the block may have served another problem)
    }
    return EACHAM_OK;
}
int ba_alloc_work_b(eacham_ctx* ctx, eacham_ba_handle* h) {
    BaDev& D = h->D;
    const BaPlan& plan = h->plan;
    dev_alloc(h, &D.T, (size_t)plan.ntiles * TILE);
    dev_alloc(h, &D.Winv, (size_t)2 * plan.npan * NB * NB);   // W_a, W_b of every panel, row-major
    dev_alloc(h, &D.Xrow, (size_t)plan.npan * NB * NB);       // X = -W_b L_ba W_a, row-major
    dev_alloc(h, &D.Wops, (size_t)plan.npan * TILE_OPS);      // W_a, W_b, X of every panel in MFMA operand order
    dev_alloc(h, &D.zsol, (size_t)plan.npan * PB);
    dev_alloc(h, &D.partial, (size_t)36 * std::max(D.g_rows > 0 ? D.g_nparts : D.n_chunks, 1));
    if (h->arena.base && D.g_rows > 0) {
        // landmarks without observations are never visited by ba_schur_groups and keep a zero record
        EACHAM_HIP_TRY(ctx, hipMemsetAsync(D.lmtry, 0, sizeof(double) * LMLIN * (size_t)D.nl, ctx->stream));
        if (!ctx->ba_groups_lds_set) {  // (the kernel asks for more than the default dynamic LDS limit)
            EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)ba_schur_groups<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)schur_groups_lds_bytes(TPB)));
            EACHAM_HIP_TRY(ctx, hipFuncSetAttribute((const void*)ba_schur_groups<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)schur_groups_lds_bytes(2 * TPB)));
            ctx->ba_groups_lds_set = true;
        }
    }
    dev_alloc(h, &D.bpart, (size_t)36 * std::max(D.n_cam_chunks, 1));
    dev_alloc(h, &D.pcg_p2, (size_t)6 * std::max(D.n_cam_chunks, 1));
    dev_alloc(h, &D.flags, (size_t)N_STATUS + plan.npan);  // [0..3] status, [4 + P] hand-off flag of panel P
    if (h->arena.base) EACHAM_HIP_TRY(ctx, hipMemsetAsync(D.flags, 0, (N_STATUS + plan.npan) * sizeof(int), ctx->stream));  // (final_sums leaves them cleared)
    return EACHAM_OK;
}

// resets the values to the uploaded initial state
static int ba_reset(eacham_ctx* ctx, eacham_ba_handle* h) {
    h->finish_pending = false;
    BaDev& D = h->D;
    EACHAM_HIP_TRY(ctx, hipMemcpyAsync(D.pose, h->pose_init, sizeof(double) * 12 * (size_t)D.nc, hipMemcpyDeviceToDevice, ctx->stream));
    EACHAM_HIP_TRY(ctx, hipMemcpyAsync(D.pt, h->pt_init, sizeof(double) * 3 * (size_t)D.nl, hipMemcpyDeviceToDevice, ctx->stream));
    EACHAM_HIP_TRY(ctx, hipMemcpyAsync(D.Kc, h->K_init, sizeof(double) * 5, hipMemcpyDeviceToDevice, ctx->stream));
    return EACHAM_OK;
}

// graph.error at (pose, pt, K) -> scal[0]
// the three kernels that walk a landmark's observations, in the lanes-per-landmark variant of the problem (BaDev::lpl, lpl_step: 8 or 2)
// error at (pose, pt, Kc) + the final sums (made by the launch's last workgroup): ba_retract_cameras ran before it
static void launch_error_landmarks(eacham_ctx* ctx, eacham_ba_handle* h, const double* pose, const double* pt, const double* Kc, int n_lin) {
    const BaDev& D = h->D;
    const double ticket = (double)++h->ticket;
    if (D.lpl_step == 8) ba_error_landmarks<8><<<D.n_step_blocks, TPB, 0, ctx->stream>>>(D, pose, pt, Kc, h->err_cam, h->lin_cam, n_lin, ticket);
    else ba_error_landmarks<2><<<D.n_step_blocks, TPB, 0, ctx->stream>>>(D, pose, pt, Kc, h->err_cam, h->lin_cam, n_lin, ticket);
}
static void launch_linearize_both(eacham_ctx* ctx, const BaDev& D, double* clpart) {
    const int ncb = D.nc * LSEG;
    if (D.lpl == 8) ba_linearize<8><<<ncb + D.n_ll_blocks, TPB, 0, ctx->stream>>>(D, clpart, ncb);
    else ba_linearize<2><<<ncb + D.n_ll_blocks, TPB, 0, ctx->stream>>>(D, clpart, ncb);
}
static void launch_step_landmarks(eacham_ctx* ctx, eacham_ba_handle* h, double lambda) {
    const BaDev& D = h->D;
    const int grid = D.n_step_blocks + (D.nc + 1 + TPB - 1) / TPB;  // + the camera retraction
    const double ticket = (double)++h->ticket;
    if (D.lpl_step == 8) ba_step_landmarks<8><<<grid, TPB, 0, ctx->stream>>>(D, lambda, h->err_cam, h->lin_cam, ticket);
    else ba_step_landmarks<2><<<grid, TPB, 0, ctx->stream>>>(D, lambda, h->err_cam, h->lin_cam, ticket);
}

static void launch_error(eacham_ctx* ctx, eacham_ba_handle* h, const double* pose, const double* pt, const double* Kc) {
    BaDev& D = h->D;
    ProfileScope ps(ctx, EACHAM_KERNEL_BA_ERROR);
    ba_retract_cameras<<<(D.nc + 1 + 63) / 64, 64, 0, ctx->stream>>>(D, 0.0, pose, D.pose_new, Kc, D.K_new, 0, h->err_cam, h->lin_cam);
    launch_error_landmarks(ctx, h, pose, pt, Kc, 0);
}

static void launch_linearize(eacham_ctx* ctx, eacham_ba_handle* h) {
    BaDev& D = h->D;
    ProfileScope ps(ctx, EACHAM_KERNEL_BA_LINEARIZE);
    launch_linearize_both(ctx, D, h->kpart);
    h->finish_pending = true;  // rides in the next try's first launch (launch_try) or is flushed by finish_linearize_now
}
static void finish_linearize_now(eacham_ctx* ctx, eacham_ba_handle* h) {
    if (!h->finish_pending) return;
    ProfileScope ps(ctx, EACHAM_KERNEL_BA_LINEARIZE);
    ba_finish_linearize<<<KLIN + h->D.nc, 64, 0, ctx->stream>>>(h->D, h->kpart);
    h->finish_pending = false;
}

// one tryLambda(): builds and solves the damped system, writes tentative values and
// scal = {new error, linearised cost change, flags}
static int launch_try(eacham_ctx* ctx, eacham_ba_handle* h, double lambda, double* S_copy /* host, optional */) {
    BaDev& D = h->D;
    const int n = D.n;
    {
        ProfileScope ps(ctx, EACHAM_KERNEL_BA_SCHUR);
        const int n_finish = h->finish_pending ? KLIN + D.nc : 0;
        h->finish_pending = false;
        if (D.g_rows > 0) {  // landmark groups: elimination, Et (in LDS) and the pair products in one launch
            if (D.g_rows <= TPB) ba_schur_groups<1><<<std::max(D.g_ngroups, 1) + n_finish, TPB, schur_groups_lds_bytes(D.g_rows), ctx->stream>>>(D, lambda, h->kpart, n_finish);
            else ba_schur_groups<2><<<std::max(D.g_ngroups, 1) + n_finish, TPB, schur_groups_lds_bytes(D.g_rows), ctx->stream>>>(D, lambda, h->kpart, n_finish);
            const unsigned nbg = (unsigned)((D.g_nblk + ASM_TPB / 64 - 1) / (ASM_TPB / 64));  // a wave per block
            ba_assemble_groups<<<D.g_nlong + nbg + 1, ASM_TPB, 0, ctx->stream>>>(D, lambda, nbg);
        } else {
            ba_eliminate<<<D.n_cam_chunks + D.n_lm_blocks + n_finish, TPB, 0, ctx->stream>>>(D, lambda, h->kpart, D.n_lm_blocks, n_finish);
            if (D.n_chunks > 0) ba_schur_pairs<<<((D.n_chunks + TPB / 64 - 1) / (TPB / 64) + 7) / 8 * 8, TPB, 0, ctx->stream>>>(D);
            const unsigned nbg = (unsigned)(((long long)D.n_blocks * 36 + TPB - 1) / TPB);
            ba_assemble<<<nbg + D.nc + 2, TPB, 0, ctx->stream>>>(D, lambda, nbg);  // camera blocks | border per camera | K corner | padding
        }
    }
    if (S_copy) {  // diagnostic read-back: S and its right-hand side in the caller's order, from the tiles
        const BaPlan& pl = h->plan;
        std::vector<double> tiles((size_t)pl.ntiles * TILE);
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        EACHAM_HIP_TRY(ctx, hipMemcpy(tiles.data(), D.T, sizeof(double) * tiles.size(), hipMemcpyDeviceToHost));
        std::vector<int> colpos((size_t)n);
        for (int c = 0; c < D.nc; ++c)
            for (int a = 0; a < 6; ++a) colpos[6 * (size_t)c + a] = pl.pos[c] + a;
        for (int k = 0; k < 5; ++k) colpos[6 * (size_t)D.nc + k] = pl.posK + k;
        auto at = [&](int r, int q) -> double {
            if (r < q) std::swap(r, q);
            const int t = pl.tile(r >> 6, q >> 6);
            return t < 0 ? 0.0 : tiles[(size_t)t * TILE + (r & 63) * PB + (q & 63)];
        };
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) S_copy[(size_t)i * n + j] = at(colpos[i], colpos[j]);
        for (int j = 0; j < n; ++j) S_copy[(size_t)n * n + j] = at(pl.rhs_row, colpos[j]);
    }
#ifdef EXP_BA_FAULT
    {
        const char* f = getenv("EACHAM_FAULT");
        const int kind = !f ? 0 : (!strcmp(f, "handoff") ? 1 : (!strcmp(f, "progress") ? 2 : 0));
        EACHAM_HIP_TRY(ctx, hipMemcpyToSymbolAsync(HIP_SYMBOL(eacham::g_ba_fault), &kind, sizeof(int), 0, hipMemcpyHostToDevice, ctx->stream));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
#endif
    {
        // the factorisation, level by level of the elimination tree, and the back-substitution (one launch)
        ProfileScope ps(ctx, EACHAM_KERNEL_BA_SOLVE);
        const BaPlan& pl = h->plan;
        sp_diag<<<(unsigned)pl.leaves.size(), TPB, 0, ctx->stream>>>(D.T, h->sp_leaves, D.sp_diag_tile, D.Winv, D.Wops, D.Xrow, D.flags);
        for (const auto& la : pl.launches)
            sp_level<<<(unsigned)la.count, TPB, 0, ctx->stream>>>(D.T, h->sp_items + la.first, h->sp_srcs, la.n_first, D.Winv, D.Wops, D.Xrow, D.flags);
        sp_backsolve<<<(unsigned)pl.npan, BS_THREADS, 0, ctx->stream>>>(D.T, h->bs_order, h->bs_ptr, h->bs_ent, D.Winv, D.Xrow, D.zsol,
                                                                        h->sp_col_dest, D.delta_c, D.flags);
    }
    {
        ProfileScope ps(ctx, EACHAM_KERNEL_BA_ERROR);
        launch_step_landmarks(ctx, h, lambda);  // back-substitution, retraction, error at the tentative values, final sums
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return EACHAM_OK;
}

// tryLambda() with the iterative solve of BundleAdjuster.cpp:192-200: PCG + block-Jacobi on the damped full system
// (needs E: the linearisation ran with store_E). Same outputs as launch_try. *pcg_iterations (optional) += iterations.
static int launch_try_pcg(eacham_ctx* ctx, eacham_ba_handle* h, double lambda, long long* pcg_iterations) {
    BaDev& D = h->D;
    finish_linearize_now(ctx, h);
    const int n_update_blocks = (D.nl + D.nc + 1 + TPB - 1) / TPB;
    {
        ProfileScope ps(ctx, EACHAM_KERNEL_BA_SOLVE);
        pcg_setup_landmarks<<<D.n_lm_blocks, TPB, 0, ctx->stream>>>(D, lambda);
        pcg_setup_cameras<<<1, 1024, 0, ctx->stream>>>(D, lambda);
        double st[2] = {0.0, 0.0};
        for (int done_it = 0; done_it < PCG_MAX_IT; done_it += PCG_BATCH) {
            for (int k = 0; k < PCG_BATCH; ++k) {
                pcg_apply_landmarks<<<D.n_lm_blocks, TPB, 0, ctx->stream>>>(D, lambda);
                if (D.n_cam_chunks > 0) pcg_apply_cam_chunks<<<D.n_cam_chunks, TPB, 0, ctx->stream>>>(D);
                pcg_apply_finish<<<1, 1024, 0, ctx->stream>>>(D, lambda);
                pcg_update<<<n_update_blocks, TPB, 0, ctx->stream>>>(D);
                pcg_update_finish<<<1, 1024, 0, ctx->stream>>>(D, n_update_blocks);
            }
            EACHAM_HIP_TRY(ctx, hipMemcpyAsync(st, D.pcg_s + 4, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
            EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (st[0] != 0.0) break;
        }
        if (pcg_iterations) *pcg_iterations += (long long)st[1];
    }
    {
        ProfileScope ps(ctx, EACHAM_KERNEL_BA_ERROR);
        pcg_landmark_step<<<D.n_lm_blocks, TPB, 0, ctx->stream>>>(D, lambda);
        ba_retract_cameras<<<(D.nc + 1 + 63) / 64, 64, 0, ctx->stream>>>(D, lambda, D.pose, D.pose_new, D.Kc, D.K_new, 1, h->err_cam, h->lin_cam);
        launch_error_landmarks(ctx, h, D.pose_new, D.pt_new, D.K_new, D.n_lm_blocks /* pcg_landmark_step's grid */);
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return EACHAM_OK;
}

static int read_scal(eacham_ctx* ctx, eacham_ba_handle* h, double* out3) {
    // ba_final_sums stored them into the pinned block itself, its ticket last. The LM loop is one host round trip per
    // tryLambda(): waking up from hipStreamSynchronize and only then deciding and launching left the device idle for
    // ~25 us per inner iteration on S200, so the host first watches the ticket for a bounded while (the stream is
    // still in order: what is launched next runs behind that kernel) and only then falls back to the blocking wait.
    {
        volatile double* sh = h->scal_host;
        const double want = (double)h->ticket;
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (int spin = 0;; ++spin) {
            if (sh[3] == want) { seen = true; break; }
            if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
        }
        if (seen) std::atomic_thread_fence(std::memory_order_acquire);
        else EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int k = 0; k < 3; ++k) out3[k] = h->scal_host[k];
    return EACHAM_OK;
}

// LevenbergMarquardtOptimizer::optimize with SetCeresDefaults + the reference's overrides
// (BundleAdjuster.cpp:184-190, :216); control flow as in SURVEY.md Appendix A.4.
static int ba_run(eacham_ctx* ctx, eacham_ba_handle* h, const eacham_ba_options* O, eacham_ba_result* R) {
    if (!O || !R || (h->D.nc > 0 && !R->cam_T_wc) || (h->D.nl > 0 && !R->points)) return ctx->fail(EACHAM_ERR_INVALID, "null BA options/result");
    BaDev& D = h->D;
    R->trace_len = 0;
    R->outer_iterations = R->inner_iterations = 0;
    R->final_lambda = 0.0;
    int rc = ba_reset(ctx, h);
    if (rc) return rc;
    auto download = [&](void) -> int {
        std::vector<double> pose(12 * (size_t)D.nc), K5(5);
        if (D.nc) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(pose.data(), D.pose, sizeof(double) * pose.size(), hipMemcpyDeviceToHost, ctx->stream));
        if (D.nl) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(R->points, D.pt, sizeof(double) * 3 * (size_t)D.nl, hipMemcpyDeviceToHost, ctx->stream));
        EACHAM_HIP_TRY(ctx, hipMemcpyAsync(K5.data(), D.Kc, sizeof(double) * 5, hipMemcpyDeviceToHost, ctx->stream));
        EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int c = 0; c < D.nc; ++c) pose_to_Twc(&pose[12 * (size_t)c], R->cam_T_wc + 16 * (size_t)c);
        R->K[0] = K5[0]; R->K[1] = K5[1]; R->K[2] = K5[3]; R->K[3] = K5[4];  // fx fy px py (:224-227)
        return EACHAM_OK;
    };
    if (h->n_landmarks_used < O->min_landmarks) {  // BundleAdjuster.cpp:166-169
        R->status = EACHAM_BA_SKIPPED;
        R->initial_error = R->final_error = NAN;
        return download();
    }
    if (O->method != EACHAM_BA_LM && O->method != EACHAM_BA_DOGLEG) return ctx->fail(EACHAM_ERR_INVALID, "unknown BA method %d", O->method);
    if (O->lm_factor_policy != EACHAM_BA_LM_FACTOR_RESET && O->lm_factor_policy != EACHAM_BA_LM_FACTOR_DOUBLE)
        return ctx->fail(EACHAM_ERR_INVALID, "unknown lm_factor_policy %d", O->lm_factor_policy);
    // use_preconditioner (BundleAdjuster.cpp:192-200) selects GTSAM's iterative solve, PCG + block-Jacobi at 1e-10, for
    // the LM steps (the option sits inside the LM branch of the reference: DogLeg never sees it)
    const bool pcg = O->method == EACHAM_BA_LM && O->use_preconditioner != 0;
    long long pcg_iterations = 0;
    D.store_E = (O->method == EACHAM_BA_DOGLEG || pcg) ? 1 : 0;  // the dog-leg forms and the PCG operator read E after the linearisation

    const double lambdaUpper = 1e32, lambdaLower = 1e-16, minModelFidelity = 1e-3;
    const double relTol = (double)O->max_tolerance, absTol = (double)O->max_tolerance, errorTol = 0.0;
    const double lambdaFactor = 2.0;  // SetCeresDefaults
    double lambda = 1e-4, factor = lambdaFactor;
    int iterations = 0, inner = 0;
    double sc[3];
    launch_error(ctx, h, D.pose, D.pt, D.Kc);
    rc = read_scal(ctx, h, sc);
    if (rc) return rc;
    double error = sc[0];
    R->initial_error = error;
    double newErrorOuter = error, currentError = error;
    bool indeterminate = false;
    if (O->method == EACHAM_BA_DOGLEG) {
        // DoglegOptimizer (BundleAdjuster.cpp:204-214; GTSAM 4.1.1 DoglegOptimizer.cpp, DoglegOptimizerImpl.h):
        // per iterate() one linearisation, the Gauss-Newton step n (the LM pipeline at lambda = 0), the
        // steepest-descent point u = (g.g / g^T H g) g, then DoglegOptimizerImpl::Iterate in mode
        // ONE_STEP_PER_ITERATION. Every candidate x_d = cu u + cn n needs one retraction + error pass; the
        // model decrease M(0) - M(x_d) = g.x_d - 1/2 x_d^T H x_d comes from six scalars computed once.
        double delta = (double)O->delta;
        if (error > errorTol && iterations < O->max_iter) {
            for (;;) {  // NonlinearOptimizer::defaultOptimize
                currentError = newErrorOuter;
                launch_linearize(ctx, h);
                rc = launch_try(ctx, h, 0.0, nullptr);
                if (rc) return rc;
                EACHAM_HIP_TRY(ctx, hipMemcpyAsync(D.dl_nc, D.delta_c, sizeof(double) * (size_t)D.n, hipMemcpyDeviceToDevice, ctx->stream));
                if (D.nl) EACHAM_HIP_TRY(ctx, hipMemcpyAsync(D.dl_nl, D.delta_l, sizeof(double) * 3 * (size_t)D.nl, hipMemcpyDeviceToDevice, ctx->stream));
                {
                    ProfileScope ps(ctx, EACHAM_KERNEL_BA_ERROR);
                    ba_dl_forms_landmarks<<<D.n_lm_blocks, TPB, 0, ctx->stream>>>(D);
                    ba_dl_forms_final<<<1, TPB, 0, ctx->stream>>>(D);
                }
                double s10[10];
                EACHAM_HIP_TRY(ctx, hipMemcpyAsync(s10, D.scal, sizeof(s10), hipMemcpyDeviceToHost, ctx->stream));
                EACHAM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if (((int)s10[2] & 4) != 0) return ctx->fail(EACHAM_ERR_HIP, "BA solve: an in-kernel hand-off timed out (flags %d)", (int)s10[2]);
                if (!(s10[2] == 0.0) || !std::isfinite(s10[1])) {  // GTSAM throws IndeterminantLinearSystemException here
                    indeterminate = true;
                    break;
                }
                const double gg = s10[4], gn0 = s10[5], nn = s10[6], gHg = s10[7], gHn = s10[8], nHn = s10[9];
                const double alpha = gg / gHg;  // u = alpha g
                const double uu = alpha * alpha * gg, un = alpha * gn0, uHu = alpha * alpha * gHg, uHn = alpha * gHn;
                const double gu = alpha * gg, gn = gn0;
                double f_new = error;
                bool zero_step = false;
                for (bool stay = true; stay;) {
                    double cu, cn;  // DoglegOptimizerImpl::ComputeDoglegPoint / ComputeBlend
                    const double DeltaSq = delta * delta;
                    if (DeltaSq < uu) {
                        cu = std::sqrt(DeltaSq / uu);
                        cn = 0.0;
                    } else if (DeltaSq < nn) {
                        const double a = uu - 2. * un + nn, b = 2. * (un - uu), c = uu - DeltaSq;
                        const double sq = std::sqrt(b * b - 4 * a * c);
                        const double tau1 = (-b + sq) / (2. * a), tau2 = (-b - sq) / (2. * a);
                        const double tau = (0.0 <= tau1 && tau1 <= 1.0) ? tau1 : tau2;
                        cu = 1. - tau;
                        cn = tau;
                    } else {
                        cu = 0.0;
                        cn = 1.0;
                    }
                    const double dnorm = std::sqrt(cu * cu * uu + 2 * cu * cn * un + cn * cn * nn);
                    {
                        ProfileScope ps(ctx, EACHAM_KERNEL_BA_ERROR);
                        const int na = std::max(3 * D.nl, D.n);
                        ba_dl_apply<<<(na + TPB - 1) / TPB, TPB, 0, ctx->stream>>>(D, cu * alpha, cn);
                        ba_retract_cameras<<<(D.nc + 1 + 63) / 64, 64, 0, ctx->stream>>>(D, 0.0, D.pose, D.pose_new, D.Kc, D.K_new, 1, h->err_cam, h->lin_cam);
                        launch_error_landmarks(ctx, h, D.pose_new, D.pt_new, D.K_new, 0);
                    }
                    rc = read_scal(ctx, h, sc);
                    if (rc) return rc;
                    f_new = sc[0];
                    const double decrease = (cu * gu + cn * gn) - 0.5 * (cu * cu * uHu + 2 * cu * cn * uHn + cn * cn * nHn);  // M(0) - M(x_d)
                    const double rho = (std::fabs(error - f_new) < 1e-15 || std::fabs(decrease) < 1e-15) ? 0.5 : (error - f_new) / decrease;
                    bool accepted = true;
                    const double delta_used = delta;
                    if (rho >= 0.75) {
                        delta = std::max(delta, 3.0 * dnorm);
                        stay = false;
                    } else if (rho >= 0.25) {
                        stay = false;
                    } else if (rho >= 0.0) {
                        if (delta > 1e-5) delta = 0.5 * delta;
                        stay = false;  // ONE_STEP_PER_ITERATION
                    } else {           // f increased (or NaN): shrink the region and try again
                        accepted = false;
                        if (delta > 1e-5) {
                            delta *= 0.5;
                        } else {
                            zero_step = true;  // dx_d.setZero(): the values and the error stay
                            stay = false;
                        }
                    }
                    if (R->trace && R->trace_len < R->trace_cap) {
                        eacham_ba_trace_row* tr = &R->trace[R->trace_len++];
                        tr->lambda = delta_used; tr->new_error = f_new; tr->lin_change = decrease;
                        tr->accepted = accepted ? 1 : 0; tr->outer = iterations;
                    }
                    ++inner;
                }
                if (!zero_step) {
                    std::swap(D.pose, D.pose_new);
                    std::swap(D.pt, D.pt_new);
                    std::swap(D.Kc, D.K_new);
                    error = f_new;
                }
                ++iterations;
                newErrorOuter = error;
                if (newErrorOuter <= errorTol) break;
                const double absDec = currentError - newErrorOuter, relDec = absDec / currentError;
                const bool converged = (relTol != 0.0 && relDec <= relTol) || (absDec <= absTol);
                if (!(iterations < O->max_iter) || converged || !std::isfinite(currentError)) break;
            }
        }
        lambda = delta;  // reported as final_lambda
    } else if (error > errorTol && iterations < O->max_iter) {
        for (;;) {  // NonlinearOptimizer::defaultOptimize
            currentError = newErrorOuter;
            launch_linearize(ctx, h);  // iterate(): linearize once, then tryLambda until it returns true
            for (;;) {
                bool success = false, stop = false;
                double newError = INFINITY, linChange = NAN, fidelity = 0.0;
                rc = pcg ? launch_try_pcg(ctx, h, lambda, &pcg_iterations) : launch_try(ctx, h, lambda, nullptr);
                if (rc) return rc;
                rc = read_scal(ctx, h, sc);
                if (rc) return rc;
                // a hand-off time-out (flags bit 2) is a failure of the machine, not of the matrix: it must not
                // be taken for "not positive definite" and silently raise lambda
                if (((int)sc[2] & 4) != 0) return ctx->fail(EACHAM_ERR_HIP, "BA solve: an in-kernel hand-off timed out (flags %d)", (int)sc[2]);
                const bool solved = sc[2] == 0.0 && std::isfinite(sc[1]);
                if (solved) {
                    linChange = sc[1];
                    // oldLinearizedError = 1/2 |b|^2; the threshold eps * oldLin is far below any
                    // representable decrease here, so `> 0` decides exactly as GTSAM's test does
                    if (linChange >= 0) {
                        newError = sc[0];
                        const double cost = error - newError;
                        if (linChange > 0.0) {
                            fidelity = cost / linChange;
                            success = fidelity > minModelFidelity;
                        }
                        if (std::fabs(cost) < relTol * error) stop = true;
                    }
                }
                if (R->trace && R->trace_len < R->trace_cap) {
                    eacham_ba_trace_row* tr = &R->trace[R->trace_len++];
                    tr->lambda = lambda; tr->new_error = newError; tr->lin_change = linChange;
                    tr->accepted = success ? 1 : 0; tr->outer = iterations;
                }
                ++inner;
                if (success) {  // decreaseLambda
                    double m = 1.0 - std::pow(2.0 * fidelity - 1.0, 3);
                    if (m < 1.0 / 3.0) m = 1.0 / 3.0;
                    lambda *= m;
                    // LevenbergMarquardtState::decreaseLambda: see EACHAM_BA_LM_FACTOR_* in eacham_hip.h
                    factor = O->lm_factor_policy == EACHAM_BA_LM_FACTOR_DOUBLE ? 2.0 * factor : 2.0 * lambdaFactor;
                    if (lambda < lambdaLower) lambda = lambdaLower;
                    std::swap(D.pose, D.pose_new);
                    std::swap(D.pt, D.pt_new);
                    std::swap(D.Kc, D.K_new);
                    error = newError;
                    ++iterations;
                    break;
                } else if (!stop) {  // increaseLambda
                    lambda *= factor;
                    factor *= 2.0;
                    if (lambda >= lambdaUpper) break;
                } else {
                    break;
                }
            }
            newErrorOuter = error;
            if (newErrorOuter <= errorTol) break;
            const double absDec = currentError - newErrorOuter, relDec = absDec / currentError;
            const bool converged = (relTol != 0.0 && relDec <= relTol) || (absDec <= absTol);
            if (!(iterations < O->max_iter) || converged || !std::isfinite(currentError)) break;
        }
    }
    R->status = indeterminate ? EACHAM_BA_INDETERMINATE : EACHAM_BA_DONE;
    R->final_error = error;
    R->final_lambda = lambda;
    R->outer_iterations = iterations;
    R->inner_iterations = inner;
    R->reserved = (int32_t)std::min<long long>(pcg_iterations, 0x7fffffff);  // PCG iterations in total (0 for the direct solve)
    return download();
}

}  // namespace eacham

extern "C" {

int eacham_ba_run(eacham_ctx* ctx, eacham_ba_handle* handle, const eacham_ba_options* options, eacham_ba_result* result) {
    if (!ctx || !handle) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    return ba_run(ctx, handle, options, result);
}

void eacham_ba_release(eacham_ctx* ctx, eacham_ba_handle* handle) {
    if (!ctx || !handle) return;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    ba_release(ctx, handle);
}

int eacham_ba_solve(eacham_ctx* ctx, const eacham_ba_problem* problem, const eacham_ba_options* options, eacham_ba_result* result) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    eacham_ba_handle* h = nullptr;
    int rc = ba_prepare(ctx, problem, &h);
    if (rc) return rc;
    rc = ba_run(ctx, h, options, result);
    ba_release(ctx, h);
    return rc;
}

int eacham_ba_debug_step(eacham_ctx* ctx, const eacham_ba_problem* problem, double lambda, double* S, double* g,
                         double* delta_cams, double* delta_points, double* error, double* lin_change) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    eacham_ba_handle* h = nullptr;
    int rc = ba_prepare(ctx, problem, &h);
    if (rc) return rc;
    BaDev& D = h->D;
    const int n = D.n;
    double sc[3];
    std::vector<double> Sg((size_t)(n + 1) * n);
    rc = ba_reset(ctx, h);
    if (!rc) {
        launch_error(ctx, h, D.pose, D.pt, D.Kc);
        rc = read_scal(ctx, h, sc);
    }
    if (!rc && error) *error = sc[0];
    if (!rc) {
        launch_linearize(ctx, h);
        rc = launch_try(ctx, h, lambda, Sg.data());
    }
    if (!rc) rc = read_scal(ctx, h, sc);
    if (!rc) {
        if (lin_change) *lin_change = sc[1];
        if (S) {
            memcpy(S, Sg.data(), sizeof(double) * (size_t)n * n);
        }
        if (g) memcpy(g, Sg.data() + (size_t)n * n, sizeof(double) * (size_t)n);
        hipError_t e1 = delta_cams ? hipMemcpy(delta_cams, D.delta_c, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) : hipSuccess;
        hipError_t e2 = (delta_points && D.nl) ? hipMemcpy(delta_points, D.delta_l, sizeof(double) * 3 * (size_t)D.nl, hipMemcpyDeviceToHost) : hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess) rc = ctx->fail(EACHAM_ERR_HIP, "debug_step download failed");
        if (!rc && ((int)sc[2] & 4) != 0) rc = ctx->fail(EACHAM_ERR_HIP, "BA solve: an in-kernel hand-off timed out (flags %d)", (int)sc[2]);
        if (!rc && sc[2] != 0.0) rc = ctx->fail(EACHAM_ERR_INVALID, "reduced system not positive definite (flags %d)", (int)sc[2]);
    }
    ba_release(ctx, h);
    return rc;
}

}  // extern "C"
