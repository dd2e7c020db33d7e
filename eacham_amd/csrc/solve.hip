// solve.hip — batched MINIMAL SOLVERS of the robust estimators eacham calls (the scoring half is
// score.hip): one thread per caller-supplied minimal sample.
//
//   cv::findHomography(pts1, pts2, cv::LMEDS, 4.0, mask2, 100, 0.999)              ReconstructionManager.cpp:75
//       -> EACHAM_SOLVE_HOMOGRAPHY4: OpenCV 4.5.5 HomographyEstimatorCallback::runKernel (fundam.cpp): per-set point
//          normalisation, LtL of the 2 x 9 constraint rows, eigenvector of the smallest eigenvalue (cyclic Jacobi), denormalised, / H[8]
//   cv::findEssentialMat(pts1, pts2, focal, pp, cv::LMEDS, 0.99, 4.0, 1000, mask)  ReconstructionManager.cpp:57-61
//       -> EACHAM_SOLVE_ESSENTIAL5: EMEstimatorCallback::runKernel (five-point.cpp), Nister's five-point algorithm: null space of
//          the 5 x 9 epipolar system (Householder), the ten cubic constraints as a 10 x 20 matrix, Gauss-Jordan, det B(z) = a
//          degree-10 polynomial, its real roots (Durand-Kerner + Newton polish), up to ten unit-norm E per sample
//   cv::solvePnPRansac(pts3d, pts2d, K, dist, rvec, t, false, 10000, 4.0f, 0.999f, inliers, cv::SOLVEPNP_EPNP)   :227-228
//       -> eacham_solve_pnp: EPnP on every 5-point sample (the RANSAC kernel) and on the inlier set (the final refit): four control
//          points, M^T M of the projection system, its four smallest eigenvectors (Jacobi 12 x 12), the 6 x 10 distance system, three
//          linearised starts + Gauss-Newton, absolute orientation (Horn), smallest reprojection error; the point passes recompute the
//          barycentric coordinates, so a thread's state does not grow with the sample size
// OpenCV draws the samples from its own RNG: the sample INDICES are an argument here (what RANSACPointSetRegistrator /
// LMeDSPointSetRegistrator::getSubset produce), so "these correspondences -> these models" is what can be held against the
// CPU restatement the tests keep (solve_oracle.c, bit for bit: this file is compiled with -ffp-contract=off and uses only
// + - * / sqrt) — end-to-end parity with cv::findHomography / findEssentialMat cannot be pinned without that RNG stream.
// A sample is ~10^4-10^5 flops of branchy fp64 with kilobytes of private state: latency-bound, no roofline claim; the
// 1000 / 100 iterations the reference asks for are one launch.
#include "context.hpp"
#include "solve_dev.hpp"

#include <algorithm>
#include <cstdint>

namespace eacham {
namespace {

// EPnP by one wave. Lane l accumulates the points l, l + 64, ... of every pass over the points; the partial sums are added in
// lane order — for at most 64 points that is the sequential sum over the points, bit for bit, and the CPU restatement defines the
// sums of more than 64 points the same way (64 strided partials) — and the small dense algebra then runs on identical values in
// every lane, with everything that is indexed at run time (M^T M, its eigenvectors, the 6 x 10 distance system) in one SHARED
// copy in LDS. BIG = false: samples of at most 64 points (the RANSAC loop's 5-point samples: a point per lane, its two rows
// of the projection system parked in LDS, an entry of M^T M per lane) — 16 KB of LDS per wave, ten waves per CU; BIG = true: the
// all-inlier refit, any number of points, a private partial M^T M per lane (40 KB).
struct PnpLds {
    double red[64];
    double A[144], V[144];   // M^T M and its eigenvectors
    double ev[48], L[60];    // the four null vectors, the distance system
    JacRound R;
};

// sum of one value per lane in LANE ORDER over the first `terms` lanes, ((v0 + v1) + v2) + ..., returned to every lane
__device__ __forceinline__ double ordered_wave_sum(double v, double* red, int terms) {
    red[threadIdx.x & 63] = v;
    wave_sync_lds();
    double t = red[0];
    for (int l = 1; l < terms; ++l) t += red[l];
    wave_sync_lds();
    return t;
}

// What the front half leaves in registers (identical in every lane) for the back half: the control-point frame and the six squared
// control-point distances; the four null vectors (S.ev) and the distance system (S.L) stay in LDS.
struct PnpFrame {
    double c0[3], ax[3][3], sc[3], rho[6];
    bool planar;  // a coplanar point set: three control points (sc[2] == 0 marks it in the stored frame), see epnp_front
};

// Front half, ONE WAVE per sample: control points, M^T M (shared), its eigenvectors by jacobi_wave, the distance system.
template <bool BIG>
__device__ static int epnp_front(int m, const int* idx, const double* obj, const double* img, const double* K, PnpFrame& F, PnpLds& S,
                                 double* rows /* !BIG: 64 x 24 */, double* part /* BIG: 78 x 64 */) {
    if (m < 4 || (!BIG && m > 64)) return 0;
    const int lane = threadIdx.x & 63;
    const int terms = m < 64 ? m : 64;  // lanes that hold a partial sum
    auto total = [&](double v) { return ordered_wave_sum(v, S.red, terms); };
    const double fu = K[0], uc = K[2], fv = K[1], vc = K[3];
    double (&c0)[3] = F.c0;
    double (&ax)[3][3] = F.ax;
    double (&sc)[3] = F.sc;
    double (&rho)[6] = F.rho;
    /* control points: centroid + principal axes scaled by the spread along them */
    c0[0] = c0[1] = c0[2] = 0.0;
    for (int k = lane; k < m; k += 64)
#pragma unroll
        for (int e = 0; e < 3; ++e) c0[e] += obj[3 * (size_t)idx[k] + e];
#pragma unroll
    for (int e = 0; e < 3; ++e) c0[e] = total(c0[e]) / (double)m;
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, V3[9], w3[3];
    for (int k = lane; k < m; k += 64) {
        double d[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) d[e] = obj[3 * (size_t)idx[k] + e] - c0[e];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) C[3 * i + j] += d[i] * d[j];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = total(C[i]);
    jacobi_eig<3>(C, V3, w3);
    double wmax = w3[0] > w3[1] ? w3[0] : w3[1];
    wmax = wmax > w3[2] ? wmax : w3[2];
    /* ax[k] = unit axis k, sc[k] = its length: control point k+1 = c0 + sc[k] ax[k] */
    if (!(wmax > 0.0)) return 0;
    const int kmin = w3[1] < w3[0] ? (w3[2] < w3[1] ? 2 : 1) : (w3[2] < w3[0] ? 2 : 0);  // the axis of the smallest spread (ties: the lower index)
    if ((kmin != 0 && !(w3[0] > 1e-12 * wmax)) || (kmin != 1 && !(w3[1] > 1e-12 * wmax)) || (kmin != 2 && !(w3[2] > 1e-12 * wmax))) return 0;  // collinear / coincident
    const double wflat = kmin == 0 ? w3[0] : (kmin == 1 ? w3[1] : w3[2]);
    const bool planar = !(wflat > 1e-12 * wmax);
    F.planar = planar;
    /* A COPLANAR set takes the paper's three-control-point form inside the same arrays (solve_oracle.c's header): the flat axis goes
     * last with length 0 — control point 3 coincides with the centroid and carries barycentric coordinate 0 — and its three
     * diagonal entries of M^T M are set above every eigenvalue of the 9 x 9 part below. A set with volume keeps the axes as the
     * eigenproblem leaves them. */
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int src = !planar ? k : (k == 0 ? (kmin == 0 ? 1 : 0) : (k == 1 ? (kmin == 2 ? 1 : 2) : kmin));
        const double wk = src == 0 ? w3[0] : (src == 1 ? w3[1] : w3[2]);
        sc[k] = (planar && k == 2) ? 0.0 : sqrt(wk / (double)m);
#pragma unroll
        for (int e = 0; e < 3; ++e) ax[k][e] = src == 0 ? V3[3 * e] : (src == 1 ? V3[3 * e + 1] : V3[3 * e + 2]);
    }
#define EPNP_ALPHAS(i, al)                                                                        \
    {                                                                                             \
        double d_[3];                                                                             \
        _Pragma("unroll") for (int e_ = 0; e_ < 3; ++e_) d_[e_] = obj[3 * (size_t)(i) + e_] - c0[e_];               \
        _Pragma("unroll") for (int k_ = 0; k_ < 3; ++k_)                                           \
            (al)[k_ + 1] = (planar && k_ == 2) ? 0.0 : (ax[k_][0] * d_[0] + ax[k_][1] * d_[1] + ax[k_][2] * d_[2]) / sc[k_]; \
        (al)[0] = 1.0 - (al)[1] - (al)[2] - (al)[3];                                              \
    }
    /* M^T M of the 2m x 12 projection system  sum_j alpha_j (fu Xc_j + (uc - u) Zc_j) = 0, same with v */
    if constexpr (!BIG) {
        if (lane < m) {  // this lane's point: its two rows
            double al[4];
            EPNP_ALPHAS(idx[lane], al);
            const double du = uc - img[2 * (size_t)idx[lane]], dv = vc - img[2 * (size_t)idx[lane] + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rows[24 * lane + 3 * j] = al[j] * fu, rows[24 * lane + 3 * j + 1] = 0.0, rows[24 * lane + 3 * j + 2] = al[j] * du;
                rows[24 * lane + 12 + 3 * j] = 0.0, rows[24 * lane + 12 + 3 * j + 1] = al[j] * fv, rows[24 * lane + 12 + 3 * j + 2] = al[j] * dv;
            }
        }
        wave_sync_lds();
        for (int e = lane; e < 144; e += 64) {  // an entry per lane: the points in order, as the sequential loop adds them
            const int i = e / 12, j = e % 12;
            if (j < i) continue;
            double acc = 0.0;
            for (int k = 0; k < m; ++k) acc += rows[24 * k + i] * rows[24 * k + j] + rows[24 * k + 12 + i] * rows[24 * k + 12 + j];
            S.A[12 * i + j] = acc;
            S.A[12 * j + i] = acc;
        }
        wave_sync_lds();
    } else {
        for (int e = 0; e < 78; ++e) part[64 * e + lane] = 0.0;
        for (int k = lane; k < m; k += 64) {
            double al[4], r1[12], r2[12];
            EPNP_ALPHAS(idx[k], al);
            const double du = uc - img[2 * (size_t)idx[k]], dv = vc - img[2 * (size_t)idx[k] + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r1[3 * j] = al[j] * fu, r1[3 * j + 1] = 0.0, r1[3 * j + 2] = al[j] * du;
                r2[3 * j] = 0.0, r2[3 * j + 1] = al[j] * fv, r2[3 * j + 2] = al[j] * dv;
            }
            int e = 0;
#pragma unroll
            for (int i = 0; i < 12; ++i)
#pragma unroll
                for (int j = i; j < 12; ++j, ++e) part[64 * e + lane] += r1[i] * r1[j] + r2[i] * r2[j];
        }
        wave_sync_lds();
        for (int e = lane; e < 78; e += 64) {  // entry e of the upper triangle: the 64 partials in lane order
            double t = part[64 * e];
            for (int l = 1; l < 64; ++l) t += part[64 * e + l];
            int i = 0, rem = e;
            while (rem >= 12 - i) rem -= 12 - i, ++i;
            const int j = i + rem;
            S.A[12 * i + j] = t;
            S.A[12 * j + i] = t;
        }
        wave_sync_lds();
    }
    if (planar) {  // rows / columns 9..11 are exact zeros: their diagonal goes above every eigenvalue of the 9 x 9 part
        if (lane == 0) {
            double tr = 0.0;
            for (int i = 0; i < 9; ++i) tr += S.A[13 * i];
            for (int i = 9; i < 12; ++i) S.A[13 * i] = 2.0 * tr + 1.0;
        }
        wave_sync_lds();
    }
    double w[12];
    jacobi_wave<12>(S.A, S.V, w, S.R);
    int ord[4];  /* the four smallest eigenvalues, ascending (ties: lower index first) */
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int best = -1;
        double wbest = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            bool used = false;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < k) used |= ord[q] == i;
            if (!used && (best < 0 || w[i] < wbest)) best = i, wbest = w[i];
        }
        ord[k] = best;
    }
    // ev[k][i] = V[12 i + ord[k]]: the shared copy, an element per lane
    if (lane < 48) {
        const int k = lane / 12, i = lane % 12;
        int o = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q == k) o = ord[q];
        S.ev[12 * k + i] = S.V[12 * i + o];
    }
    wave_sync_lds();
    /* the six control-point distance constraints, quadratic in beta: L (6 x 10) over [b00 b01 b11 b02 b12 b22 b03 b13 b23 b33] */
    double cw[4][3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        cw[0][e] = c0[e];
#pragma unroll
        for (int k = 0; k < 3; ++k) cw[k + 1][e] = c0[e] + sc[k] * ax[k][e];
    }
    {
        constexpr int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        if (lane < 60) {  // entry (p, col) of L per lane
            const int p = lane / 10, col = lane % 10;
            int i = 0, j = 0, cc = 0;
            for (int jj = 0; jj < 4; ++jj)
                for (int ii = 0; ii <= jj; ++ii, ++cc)
                    if (cc == col) i = ii, j = jj;
            int a_ = 0, b_ = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (q == p) a_ = pa[q], b_ = pb[q];
            double di[3], dj[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                di[e] = S.ev[12 * i + 3 * a_ + e] - S.ev[12 * i + 3 * b_ + e];
                dj[e] = S.ev[12 * j + 3 * a_ + e] - S.ev[12 * j + 3 * b_ + e];
            }
            const double d = di[0] * dj[0] + di[1] * dj[1] + di[2] * dj[2];
            S.L[10 * p + col] = i == j ? d : 2.0 * d;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            rho[p] = 0.0;
#pragma unroll
            for (int e = 0; e < 3; ++e) rho[p] += (cw[pa[p]][e] - cw[pb[p]][e]) * (cw[pa[p]][e] - cw[pb[p]][e]);
        }
        wave_sync_lds();
    }
    return 1;
}

// One linearised start of the back half (variant 0 / 1 / 2 = the first 1 / 2 / 3 null vectors' leading terms): least squares for
// the start, five Gauss-Newton steps, Horn's absolute orientation, the reprojection error. Returns the error (< 0: no pose) and
// the pose in cand[12].
template <bool LANE, int variant>
__device__ static double epnp_back_variant(int m, const int* idx, const double* obj, const double* img, const double* K, const PnpFrame& F,
                                           const double* ev, const double* L, size_t es, double* red, double* cand) {
    const int lane = LANE ? 0 : (int)(threadIdx.x & 63);
    const int kstep = LANE ? 1 : 64;
    const int terms = m < 64 ? m : 64;
    auto total = [&](double v) { return LANE ? v : ordered_wave_sum(v, red, terms); };
    const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
    const double (&c0)[3] = F.c0;
    const double (&ax)[3][3] = F.ax;
    const double (&sc)[3] = F.sc;
    const double (&rho)[6] = F.rho;
    const bool planar = F.planar;
    {
        /* linearised start: the products b_i b_j that involve only the first 1 / 2 / 3 null vectors' leading terms */
        constexpr int ncol[3] = {4, 3, 5};
        constexpr int cols[3][5] = {{0, 1, 3, 6, 0}, {0, 1, 2, 0, 0}, {0, 1, 2, 3, 4}};
        double A[30], x[5], beta[4] = {0, 0, 0, 0};
        if (planar) {
            /* three control points: the distance equations of the pairs (0,1), (0,2), (1,2) = rows 0, 1, 3; start 0 takes the first
             * null vector alone (x = b00), start 1 the first two (x = b00 b01 b11, a square system); there is no third start.
             * Gauss-Newton runs on the unknowns of the start (1 or 2 betas against three equations). */
            if constexpr (variant == 2) {
                return -1.0;
            } else {
                constexpr int rows3[3] = {0, 1, 3}, nb = variant + 1, nc3 = variant == 0 ? 1 : 3;
                double l3[3][3], rho3[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    rho3[p] = rho[rows3[p]];
#pragma unroll
                    for (int j = 0; j < 3; ++j) l3[p][j] = L[(size_t)(10 * rows3[p] + j) * es];
#pragma unroll
                    for (int j = 0; j < nc3; ++j) A[p * nc3 + j] = l3[p][j];
                }
                if (!lsq_rc<3, nc3>(A, rho3, x)) return -1.0;
                const double s = x[0] < 0.0 ? -1.0 : 1.0;
                beta[0] = sqrt(s * x[0]);
                if (variant == 1) {
                    beta[1] = s * x[2] > 0.0 ? sqrt(s * x[2]) : 0.0;
                    if (x[1] < 0.0) beta[0] = -beta[0];
                }
                if (!(beta[0] != 0.0)) return -1.0;
                for (int it = 0; it < 5; ++it) {
                    double J[6], r[3], dx[2];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        const double* l = l3[p];
                        J[nb * p] = 2.0 * l[0] * beta[0] + l[1] * beta[1];
                        if (nb == 2) J[nb * p + 1] = l[1] * beta[0] + 2.0 * l[2] * beta[1];
                        r[p] = rho3[p] - (l[0] * beta[0] * beta[0] + l[1] * beta[0] * beta[1] + l[2] * beta[1] * beta[1]);
                    }
                    if (!lsq_rc<3, nb>(J, r, dx)) break;
#pragma unroll
                    for (int k = 0; k < nb; ++k) beta[k] += dx[k];
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int j = 0; j < 5; ++j)
                    if (j < ncol[variant]) A[p * ncol[variant] + j] = L[(size_t)(10 * p + cols[variant][j]) * es];
            const int solved = variant == 0 ? lsq6<4>(A, rho, x) : (variant == 1 ? lsq6<3>(A, rho, x) : lsq6<5>(A, rho, x));
            if (!solved) return -1.0;
            if (variant == 0) {  /* x = b00 b01 b02 b03 */
                const double s = x[0] < 0.0 ? -1.0 : 1.0;
                beta[0] = sqrt(s * x[0]);
                if (!(beta[0] > 0.0)) return -1.0;
#pragma unroll
                for (int k = 1; k < 4; ++k) beta[k] = s * x[k] / beta[0];
            } else {             /* x = b00 b01 b11 (b02 b12) */
                const double s = x[0] < 0.0 ? -1.0 : 1.0;
                beta[0] = sqrt(s * x[0]);
                beta[1] = s * x[2] > 0.0 ? sqrt(s * x[2]) : 0.0;
                if (x[1] < 0.0) beta[0] = -beta[0];
                if (!(beta[0] != 0.0)) return -1.0;
                if (variant == 2) beta[2] = x[3] / beta[0];
            }
            for (int it = 0; it < 5; ++it) {  /* Gauss-Newton on the six distance equations */
                double J[24], r[6], dx[4];
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    double l[10];
#pragma unroll
                    for (int q = 0; q < 10; ++q) l[q] = L[(size_t)(10 * p + q) * es];
                    J[4 * p + 0] = 2.0 * l[0] * beta[0] + l[1] * beta[1] + l[3] * beta[2] + l[6] * beta[3];
                    J[4 * p + 1] = l[1] * beta[0] + 2.0 * l[2] * beta[1] + l[4] * beta[2] + l[7] * beta[3];
                    J[4 * p + 2] = l[3] * beta[0] + l[4] * beta[1] + 2.0 * l[5] * beta[2] + l[8] * beta[3];
                    J[4 * p + 3] = l[6] * beta[0] + l[7] * beta[1] + l[8] * beta[2] + 2.0 * l[9] * beta[3];
                    r[p] = rho[p] - (l[0] * beta[0] * beta[0] + l[1] * beta[0] * beta[1] + l[2] * beta[1] * beta[1] + l[3] * beta[0] * beta[2] +
                                     l[4] * beta[1] * beta[2] + l[5] * beta[2] * beta[2] + l[6] * beta[0] * beta[3] + l[7] * beta[1] * beta[3] +
                                     l[8] * beta[2] * beta[3] + l[9] * beta[3] * beta[3]);
                }
                if (!lsq6<4>(J, r, dx)) break;
#pragma unroll
                for (int k = 0; k < 4; ++k) beta[k] += dx[k];
            }
        }
        /* control points in the camera frame, sign from the first point's depth */
        double cc[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 3; ++e)
                cc[j][e] = beta[0] * ev[(size_t)(3 * j + e) * es] + beta[1] * ev[(size_t)(12 + 3 * j + e) * es] + beta[2] * ev[(size_t)(24 + 3 * j + e) * es] + beta[3] * ev[(size_t)(36 + 3 * j + e) * es];
        {
            double al[4];
            EPNP_ALPHAS(idx[0], al);
            const double z0 = al[0] * cc[0][2] + al[1] * cc[1][2] + al[2] * cc[2][2] + al[3] * cc[3][2];
            if (z0 < 0.0)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 3; ++e) cc[j][e] = -cc[j][e];
        }
        /* absolute orientation world -> camera (Horn's quaternion form): S = sum pc (pw - c0)^T */
        double Sm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pcm[3] = {0, 0, 0};
        for (int k = lane; k < m; k += kstep) {
            double al[4], pc[3];
            EPNP_ALPHAS(idx[k], al);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                pc[e] = al[0] * cc[0][e] + al[1] * cc[1][e] + al[2] * cc[2][e] + al[3] * cc[3][e];
                pcm[e] += pc[e];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Sm[3 * i + j] += pc[i] * (obj[3 * (size_t)idx[k] + j] - c0[j]);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) Sm[i] = total(Sm[i]);
#pragma unroll
        for (int e = 0; e < 3; ++e) pcm[e] = total(pcm[e]) / (double)m;
        /* Sm[i][j] = sum camera_i world_j; the rotation maximising tr(R^T S) is the top eigenvector of Horn's 4 x 4 matrix
         * written for the map world -> camera (its "left" set is the world points: Sxy = sum world_x camera_y = S[y][x]) */
        const double Sxx = Sm[0], Sxy = Sm[3], Sxz = Sm[6], Syx = Sm[1], Syy = Sm[4], Syz = Sm[7], Szx = Sm[2], Szy = Sm[5], Szz = Sm[8];
        double N[16] = {Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx,
                        Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz,
                        Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy,
                        Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz};
        double V4[16], w4[4];
        jacobi_eig<4>(N, V4, w4);
        double q0 = V4[0], qx = V4[4], qy = V4[8], qz = V4[12], wtop = w4[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (w4[k] > wtop) wtop = w4[k], q0 = V4[k], qx = V4[4 + k], qy = V4[8 + k], qz = V4[12 + k];
        cand[0] = q0 * q0 + qx * qx - qy * qy - qz * qz, cand[1] = 2.0 * (qx * qy - q0 * qz), cand[2] = 2.0 * (qx * qz + q0 * qy);
        cand[3] = 2.0 * (qy * qx + q0 * qz), cand[4] = q0 * q0 - qx * qx + qy * qy - qz * qz, cand[5] = 2.0 * (qy * qz - q0 * qx);
        cand[6] = 2.0 * (qz * qx - q0 * qy), cand[7] = 2.0 * (qz * qy + q0 * qx), cand[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
#pragma unroll
        for (int i = 0; i < 3; ++i) cand[9 + i] = pcm[i] - (cand[3 * i] * c0[0] + cand[3 * i + 1] * c0[1] + cand[3 * i + 2] * c0[2]);
        double err = 0.0;
        for (int k = lane; k < m; k += kstep) {
            const double* X = obj + 3 * (size_t)idx[k];
            const double xc = cand[0] * X[0] + cand[1] * X[1] + cand[2] * X[2] + cand[9];
            const double yc = cand[3] * X[0] + cand[4] * X[1] + cand[5] * X[2] + cand[10];
            const double zc = cand[6] * X[0] + cand[7] * X[1] + cand[8] * X[2] + cand[11];
            const double eu = uc + fu * xc / zc - img[2 * (size_t)idx[k]], evv = vc + fv * yc / zc - img[2 * (size_t)idx[k] + 1];
            err += sqrt(eu * eu + evv * evv);
        }
        err = total(err);
        if (!(err < 1e300)) return -1.0;
        return err;
    }
}
#undef EPNP_ALPHAS

// Samples of at most 64 points (the RANSAC loop's five-point samples) in two launches. Front: ONE WAVE per sample, SOLVE_WAVES samples
// per workgroup (no workgroup barrier anywhere: waves return on their own), leaving the sample's frame — 130 doubles: c0 3, axes 9,
// lengths 3, rho 6, null vectors 48, distance system 60, valid 1 — in the batch's arrays, field-major (element e of sample s at
// frame[e * n_samples + s]: the back half's lanes read neighbouring words). Back: ONE LANE per sample. The back half is scalar work
// with ~380 live registers: run by a whole wave per sample it held the kernel at one wave per SIMD and 64 lanes repeated every
// operation (2.0 ms for 10 000 samples); by lanes, 10 000 samples are 157 waves.
constexpr int PNP_FRAME = 130, PNP_F_EV = 21, PNP_F_L = 69, PNP_F_VALID = 129;

__global__ __launch_bounds__(64 * SOLVE_WAVES) void solve_pnp_front_kernel(const double* __restrict__ obj, const double* __restrict__ img,
                                                                          const double* __restrict__ K, int sample_size, int n_samples,
                                                                          const int* __restrict__ idx, double* __restrict__ frame) {
    __shared__ PnpLds lds[SOLVE_WAVES];
    extern __shared__ double rows_dyn[];   // SOLVE_WAVES x min(sample_size, 64) x 24: the two rows of every point of a wave's sample
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * SOLVE_WAVES + wave;
    if (s >= n_samples) return;
    double* rows = rows_dyn + (size_t)wave * 24 * (sample_size < 64 ? sample_size : 64);
    const double K4[4] = {K[0], K[1], K[2], K[3]};
    PnpFrame F;
    PnpLds& S = lds[wave];
    const int ok = epnp_front<false>(sample_size, idx + (size_t)s * sample_size, obj, img, K4, F, S, rows, nullptr);
    const size_t ns = (size_t)n_samples;
    double* dst = frame + s;
    if (lane == 0) {
        dst[PNP_F_VALID * ns] = ok ? 1.0 : 0.0;
        if (ok) {
#pragma unroll
            for (int e = 0; e < 3; ++e) dst[e * ns] = F.c0[e], dst[(12 + e) * ns] = F.sc[e];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int e = 0; e < 3; ++e) dst[(3 + 3 * k + e) * ns] = F.ax[k][e];
#pragma unroll
            for (int q = 0; q < 6; ++q) dst[(15 + q) * ns] = F.rho[q];
        }
    }
    if (ok) {
        if (lane < 48) dst[(PNP_F_EV + lane) * ns] = S.ev[lane];
        if (lane < 60) dst[(PNP_F_L + lane) * ns] = S.L[lane];
    }
}

// A lane per (sample, linearised start): blockIdx.y is the start (0..2), ONE launch — as one lane per sample with the three starts in
// a row the kernel needed ~380 registers, spilled 122 of them (324 B of scratch per lane) and ran one wave per SIMD; as three launches
// (one instantiation each) the starts waited for one another on the stream: 36 + 32 + 32 us per RANSAC chunk of the incremental loop,
// where a chunk is four waves per start. The starts' errors and poses go to `tmp` ([start][sample][13]); solve_pnp_select_kernel
// takes the first strictly smallest, as the CPU restatement's loop over the starts does.
template <int variant>
__device__ __forceinline__ void solve_pnp_back_body(const double* __restrict__ obj, const double* __restrict__ img,
                                                    const double* __restrict__ K, int sample_size, int n_samples,
                                                    const int* __restrict__ idx, const double* __restrict__ frame,
                                                    double* __restrict__ tmp) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_samples) return;
    const size_t ns = (size_t)n_samples;
    const double* src = frame + s;
    const double K4[4] = {K[0], K[1], K[2], K[3]};
    double cand[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) cand[k] = 0.0;
    double err = -1.0;
    if (src[PNP_F_VALID * ns] != 0.0) {
        PnpFrame F;
#pragma unroll
        for (int e = 0; e < 3; ++e) F.c0[e] = src[e * ns], F.sc[e] = src[(12 + e) * ns];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int e = 0; e < 3; ++e) F.ax[k][e] = src[(3 + 3 * k + e) * ns];
#pragma unroll
        for (int q = 0; q < 6; ++q) F.rho[q] = src[(15 + q) * ns];
        F.planar = F.sc[2] == 0.0;
        const int* rows_idx = idx + (size_t)s * sample_size;
        err = epnp_back_variant<true, variant>(sample_size, rows_idx, obj, img, K4, F, src + PNP_F_EV * ns, src + PNP_F_L * ns, ns, nullptr, cand);
    }
    double* dst = tmp + ((size_t)variant * ns + s) * 13;
    dst[0] = err;
#pragma unroll
    for (int k = 0; k < 12; ++k) dst[1 + k] = cand[k];
}
__global__ __launch_bounds__(64) void solve_pnp_back_kernel(const double* __restrict__ obj, const double* __restrict__ img,
                                                            const double* __restrict__ K, int sample_size, int n_samples,
                                                            const int* __restrict__ idx, const double* __restrict__ frame,
                                                            double* __restrict__ tmp) {
    if (blockIdx.y == 0) solve_pnp_back_body<0>(obj, img, K, sample_size, n_samples, idx, frame, tmp);        // (workgroup-uniform)
    else if (blockIdx.y == 1) solve_pnp_back_body<1>(obj, img, K, sample_size, n_samples, idx, frame, tmp);
    else solve_pnp_back_body<2>(obj, img, K, sample_size, n_samples, idx, frame, tmp);
}
__global__ __launch_bounds__(256) void solve_pnp_select_kernel(int n_samples, const double* __restrict__ tmp, double* __restrict__ models, int* __restrict__ n_models) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_samples) return;
    double best = -1.0;
    int which = -1;
    for (int v = 0; v < 3; ++v) {
        const double err = tmp[((size_t)v * n_samples + s) * 13];
        if (err >= 0.0 && (best < 0.0 || err < best)) best = err, which = v;
    }
    for (int k = 0; k < 12; ++k) models[12 * (size_t)s + k] = which >= 0 ? tmp[((size_t)which * n_samples + s) * 13 + 1 + k] : 0.0;
    n_models[s] = which >= 0 ? 1 : 0;
}

// samples of more than 64 points (the all-inlier refit): one workgroup of three waves per sample. Wave 0 runs the front half (a
// partial M^T M per lane) and leaves the frame, the null vectors and the distance system in LDS; then every wave takes ONE
// linearised start of the back half (its sums over the points spread over the wave's lanes, each wave with its own reduction
// scratch) and thread 0 picks the first strictly smallest error — the order of epnp_back. One wave running the three starts in a row
// was 234 us per refit of the incremental loop.
__global__ __launch_bounds__(192) void solve_pnp_big_kernel(const double* __restrict__ obj, const double* __restrict__ img,
                                                            const double* __restrict__ K, int sample_size, const int* __restrict__ idx,
                                                            double* __restrict__ models, int* __restrict__ n_models) {
    __shared__ PnpLds lds;
    __shared__ double part[78 * 64];
    __shared__ PnpFrame frame;
    __shared__ int front_ok;
    __shared__ double red[3][64], result[3][13];
    const int s = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double K4[4] = {K[0], K[1], K[2], K[3]};
    const int* rows_idx = idx + (size_t)s * sample_size;
    if (wave == 0) {
        PnpFrame F;
        const int n = epnp_front<true>(sample_size, rows_idx, obj, img, K4, F, lds, nullptr, part);
        if (lane == 0) frame = F, front_ok = n;
    }
    __syncthreads();
    if (front_ok) {   // (workgroup-uniform)
        const PnpFrame F = frame;
        double cand[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) cand[k] = 0.0;
        double err;
        if (wave == 0) err = epnp_back_variant<false, 0>(sample_size, rows_idx, obj, img, K4, F, lds.ev, lds.L, 1, red[0], cand);
        else if (wave == 1) err = epnp_back_variant<false, 1>(sample_size, rows_idx, obj, img, K4, F, lds.ev, lds.L, 1, red[1], cand);
        else err = epnp_back_variant<false, 2>(sample_size, rows_idx, obj, img, K4, F, lds.ev, lds.L, 1, red[2], cand);
        if (lane == 0) {
            result[wave][0] = err;
#pragma unroll
            for (int k = 0; k < 12; ++k) result[wave][1 + k] = cand[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double best = -1.0;
        int which = -1;
        if (front_ok)
            for (int v = 0; v < 3; ++v)
                if (result[v][0] >= 0.0 && (best < 0.0 || result[v][0] < best)) best = result[v][0], which = v;
        for (int k = 0; k < 12; ++k) models[12 * (size_t)s + k] = which >= 0 ? result[which][1 + k] : 0.0;
        n_models[s] = which >= 0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(64 * SOLVE_WAVES) void solve_h4_kernel(const double* __restrict__ a, const double* __restrict__ b, int n_samples,
                                                                   const int* __restrict__ idx, double* __restrict__ models, int* __restrict__ n_models) {
    __shared__ double LtL[SOLVE_WAVES][81], V[SOLVE_WAVES][81];
    __shared__ JacRound R[SOLVE_WAVES];
    const int wave = threadIdx.x >> 6;
    const int s = blockIdx.x * SOLVE_WAVES + wave;
    if (s >= n_samples) return;
    double pa[8], pb[8], out[9];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = idx[s * 4 + k];
        pa[2 * k] = a[2 * (size_t)i]; pa[2 * k + 1] = a[2 * (size_t)i + 1];
        pb[2 * k] = b[2 * (size_t)i]; pb[2 * k + 1] = b[2 * (size_t)i + 1];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = 0.0;
    const int n = homography4_wave(pa, pb, out, LtL[wave], V[wave], R[wave]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) models[9 * (size_t)s + k] = out[k];
        n_models[s] = n;
    }
}

__global__ __launch_bounds__(64 * SOLVE_WAVES) void solve_e5_kernel(const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ K,
                                                                   int has_K, int n_samples, const int* __restrict__ idx, double* __restrict__ models,
                                                                   int* __restrict__ n_models) {
    __shared__ E5Lds lds[SOLVE_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * SOLVE_WAVES + wave;
    if (s >= n_samples) return;
    double pa[10], pb[10];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int i = idx[s * 5 + k];
        pa[2 * k] = a[2 * (size_t)i]; pa[2 * k + 1] = a[2 * (size_t)i + 1];
        pb[2 * k] = b[2 * (size_t)i]; pb[2 * k + 1] = b[2 * (size_t)i + 1];
    }
    double fx = 1, fy = 1, cx = 0, cy = 0;
    if (has_K) fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    double* dst = models + (size_t)s * 90;
    for (int k = lane; k < 90; k += 64) dst[k] = 0.0;  // (this wave's own stores below follow in program order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const int n = essential5_wave(pa, pb, has_K != 0, fx, fy, cx, cy, dst, lds[wave]);
    if (lane == 0) n_models[s] = n;
}

}  // namespace
}  // namespace eacham

using namespace eacham;

extern "C" int eacham_solve_minimal(eacham_ctx* ctx, int kind, int n_points, const double* a, const double* b, const double* K,
                                    int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (kind != EACHAM_SOLVE_HOMOGRAPHY4 && kind != EACHAM_SOLVE_ESSENTIAL5) return ctx->fail(EACHAM_ERR_INVALID, "solve_minimal: unknown kind %d", kind);
    if (n_points < 0 || n_samples < 0 || (n_samples > 0 && (!a || !b || !sample_idx || !models || !n_models)))
        return ctx->fail(EACHAM_ERR_INVALID, "solve_minimal: null argument or negative size");
    if (n_samples == 0) return EACHAM_OK;
    const int m = kind == EACHAM_SOLVE_HOMOGRAPHY4 ? 4 : 5, maxm = kind == EACHAM_SOLVE_HOMOGRAPHY4 ? 1 : 10;
    for (long long k = 0; k < (long long)n_samples * m; ++k)
        if (sample_idx[k] < 0 || sample_idx[k] >= n_points)
            return ctx->fail(EACHAM_ERR_INVALID, "solve_minimal: sample index %d of %d points", (int)sample_idx[k], n_points);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_a = io.in<double>(a, 2 * (size_t)n_points), h_b = io.in<double>(b, 2 * (size_t)n_points);
    const auto h_K = io.in<double>(K, 4);
    const auto h_i = io.in<int>(sample_idx, (size_t)n_samples * m);
    const auto h_m = io.out<double>(models, 9 * (size_t)maxm * n_samples);
    const auto h_n = io.out<int>(n_models, (size_t)n_samples);
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        const unsigned grid = (unsigned)((n_samples + SOLVE_WAVES - 1) / SOLVE_WAVES);
        if (kind == EACHAM_SOLVE_HOMOGRAPHY4)
            solve_h4_kernel<<<grid, 64 * SOLVE_WAVES, 0, st>>>(d(h_a), d(h_b), n_samples, d(h_i), d(h_m), d(h_n));
        else
            solve_e5_kernel<<<grid, 64 * SOLVE_WAVES, 0, st>>>(d(h_a), d(h_b), d(h_K), K ? 1 : 0, n_samples, d(h_i), d(h_m), d(h_n));
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}

extern "C" int eacham_solve_pnp(eacham_ctx* ctx, int n_points, const double* object_points, const double* image_points, const double* K,
                                int sample_size, int n_samples, const int32_t* sample_idx, double* models, int32_t* n_models) {
    if (!ctx) return EACHAM_ERR_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (n_points < 0 || n_samples < 0 || (n_samples > 0 && (!object_points || !image_points || !K || !sample_idx || !models || !n_models)))
        return ctx->fail(EACHAM_ERR_INVALID, "solve_pnp: null argument or negative size");
    if (n_samples == 0) return EACHAM_OK;
    if (sample_size < 5) return ctx->fail(EACHAM_ERR_INVALID, "solve_pnp: EPnP needs at least 5 points per sample, got %d", sample_size);
    const long long total = (long long)n_samples * sample_size;
    for (long long k = 0; k < total; ++k)
        if (sample_idx[k] < 0 || sample_idx[k] >= n_points)
            return ctx->fail(EACHAM_ERR_INVALID, "solve_pnp: sample index %d of %d points", (int)sample_idx[k], n_points);
    EACHAM_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IoStage io(ctx, st);
    const auto h_a = io.in<double>(object_points, 3 * (size_t)n_points), h_b = io.in<double>(image_points, 2 * (size_t)n_points);
    const auto h_K = io.in<double>(K, 4);
    const auto h_i = io.in<int>(sample_idx, (size_t)total);
    const auto h_m = io.out<double>(models, 12 * (size_t)n_samples);
    const auto h_n = io.out<int>(n_models, (size_t)n_samples);
    const auto h_f = io.scratch<double>(sample_size <= 64 ? PNP_FRAME * (size_t)n_samples : 0);   // the samples' frames between the two launches
    const auto h_t = io.scratch<double>(sample_size <= 64 ? 3 * 13 * (size_t)n_samples : 0);      // error + pose of the three starts
    IoDev d;
    if (int rc = io.upload(d)) return rc;
    {
        ProfileScope scope(ctx, EACHAM_KERNEL_SCORE);
        // Bit-identical with the CPU restatement either way: samples of at most 64 points — the RANSAC loop's — a wave per sample for the
        // shared front half, a lane per sample for the scalar back half; larger ones — the all-inlier refit — one wave for both.
        if (sample_size <= 64) {
            solve_pnp_front_kernel<<<(unsigned)((n_samples + SOLVE_WAVES - 1) / SOLVE_WAVES), 64 * SOLVE_WAVES,
                                     sizeof(double) * SOLVE_WAVES * 24 * (size_t)std::min(sample_size, 64), st>>>(
                d(h_a), d(h_b), d(h_K), sample_size, n_samples, d(h_i), d(h_f));
            const unsigned gb = (unsigned)((n_samples + 63) / 64);
            solve_pnp_back_kernel<<<dim3(gb, 3), 64, 0, st>>>(d(h_a), d(h_b), d(h_K), sample_size, n_samples, d(h_i), d(h_f), d(h_t));
            solve_pnp_select_kernel<<<(unsigned)((n_samples + 255) / 256), 256, 0, st>>>(n_samples, d(h_t), d(h_m), d(h_n));
        }
        else
            solve_pnp_big_kernel<<<(unsigned)n_samples, 192, 0, st>>>(d(h_a), d(h_b), d(h_K), sample_size, d(h_i), d(h_m), d(h_n));
    }
    EACHAM_HIP_TRY(ctx, hipGetLastError());
    return io.finish();
}
