// A second CPU stand-in for libeacham_hip.so, TEST INFRASTRUCTURE ONLY: where stub_abi.cpp computes nothing, this one
// answers the entry points that include/eacham/TwoViewHip.hpp and PnPHip.hpp call — eacham_ctx_*, eacham_solve_minimal,
// eacham_solve_pnp, eacham_score_hypotheses, eacham_two_view_points — with the CPU oracle (oracle/*.c, the shared object that
// oracle.build() makes; link it next to this file). The GPU tests hold the device library bit for bit to that oracle, so the
// estimator loops of the two headers run here, without a GPU, on the arithmetic they will meet on one: tests/test_estimators.py
// runs one driver and one set of assertions against both. The argument checks follow the device library's. Every other entry
// point is absent: a driver that needs one does not link. Never linked into anything shipped.
#include <cstdint>
#include <string>

#include "eacham_hip.h"

extern "C" {
void oracle_solve_minimal(int kind, const double* a, const double* b, const double* K, int n_samples, const int32_t* idx, double* models,
                          int32_t* n_models);
void oracle_solve_pnp(const double* obj, const double* img, const double* K, int sample_size, int n_samples, const int32_t* idx,
                      double* models, int32_t* n_models);
void oracle_score_hypotheses(int kind, int n, const double* a, const double* b, int nm, const double* models, const double* K,
                             float threshold, float* errors, int32_t* counts, float* medians);
void oracle_two_view_points(int n, const double* uv1, const double* uv2, const double* K, int nt, const double* transforms, float max_err,
                            float min_angle, int angle_strict, double* points, uint8_t* keep, int32_t* counts);
}

struct eacham_ctx {
    std::string err;
};

static int fail(eacham_ctx* c, int code, const char* msg) {
    c->err = msg;
    return code;
}

static bool rows_in_range(const int32_t* idx, long long count, int n) {
    for (long long i = 0; i < count; ++i)
        if (idx[i] < 0 || idx[i] >= n) return false;
    return true;
}

extern "C" {

int eacham_ctx_create(int, eacham_ctx** out) {
    if (!out) return EACHAM_ERR_INVALID;
    *out = new eacham_ctx();
    return EACHAM_OK;
}
void eacham_ctx_destroy(eacham_ctx* c) { delete c; }
const char* eacham_last_error(const eacham_ctx* c) { return c ? c->err.c_str() : "null context"; }
int eacham_ctx_sync(eacham_ctx*) { return EACHAM_OK; }
void* eacham_ctx_stream(eacham_ctx*) { return nullptr; }
const char* eacham_version(void) { return "eacham_hip oracle stand-in (CPU, tests only)"; }

int eacham_solve_minimal(eacham_ctx* c, int kind, int n_points, const double* a, const double* b, const double* K, int n_samples,
                         const int32_t* idx, double* models, int32_t* n_models) {
    if (!c) return EACHAM_ERR_INVALID;
    if (kind != EACHAM_SOLVE_HOMOGRAPHY4 && kind != EACHAM_SOLVE_ESSENTIAL5) return fail(c, EACHAM_ERR_INVALID, "solve_minimal: unknown kind");
    if (n_points < 0 || n_samples < 0 || (n_samples > 0 && (!a || !b || !idx || !models || !n_models)))
        return fail(c, EACHAM_ERR_INVALID, "solve_minimal: null argument or negative size");
    if (n_samples == 0) return EACHAM_OK;
    if (!rows_in_range(idx, (long long)n_samples * (kind == EACHAM_SOLVE_HOMOGRAPHY4 ? 4 : 5), n_points))
        return fail(c, EACHAM_ERR_INVALID, "solve_minimal: sample index out of range");
    oracle_solve_minimal(kind, a, b, K, n_samples, idx, models, n_models);
    return EACHAM_OK;
}

int eacham_solve_pnp(eacham_ctx* c, int n_points, const double* obj, const double* img, const double* K, int sample_size, int n_samples,
                     const int32_t* idx, double* models, int32_t* n_models) {
    if (!c) return EACHAM_ERR_INVALID;
    if (n_points < 0 || n_samples < 0 || (n_samples > 0 && (!obj || !img || !K || !idx || !models || !n_models)))
        return fail(c, EACHAM_ERR_INVALID, "solve_pnp: null argument or negative size");
    if (n_samples == 0) return EACHAM_OK;
    if (sample_size < 5) return fail(c, EACHAM_ERR_INVALID, "solve_pnp: EPnP needs at least 5 points per sample");
    if (!rows_in_range(idx, (long long)n_samples * sample_size, n_points)) return fail(c, EACHAM_ERR_INVALID, "solve_pnp: sample index out of range");
    oracle_solve_pnp(obj, img, K, sample_size, n_samples, idx, models, n_models);
    return EACHAM_OK;
}

int eacham_score_hypotheses(eacham_ctx* c, int kind, int n, const double* a, const double* b, int nm, const double* models, const double* K,
                            float threshold, float* errors, int32_t* counts, float* medians) {
    if (!c) return EACHAM_ERR_INVALID;
    if (kind < EACHAM_SCORE_ESSENTIAL || kind > EACHAM_SCORE_PNP || n < 0 || nm < 0) return fail(c, EACHAM_ERR_INVALID, "score: bad kind or negative size");
    if (nm == 0) return EACHAM_OK;
    if (!models || (n > 0 && (!a || !b)) || (kind == EACHAM_SCORE_PNP && !K)) return fail(c, EACHAM_ERR_INVALID, "score: null array");
    oracle_score_hypotheses(kind, n, a, b, nm, models, K, threshold, errors, counts, medians);
    return EACHAM_OK;
}

int eacham_two_view_points(eacham_ctx* c, int n, const double* uv1, const double* uv2, const double* K, int nt, const double* T,
                           float max_err, float min_angle, int angle_strict, double* points, uint8_t* keep, int32_t* counts) {
    if (!c) return EACHAM_ERR_INVALID;
    if (n < 0 || nt < 0 || !K) return fail(c, EACHAM_ERR_INVALID, "two_view: null argument or negative size");
    if (counts)
        for (int k = 0; k < nt; ++k) counts[k] = 0;
    if ((long long)n * nt == 0) return EACHAM_OK;
    if (!uv1 || !uv2 || !T || !points || !keep || !counts) return fail(c, EACHAM_ERR_INVALID, "two_view: null array");
    oracle_two_view_points(n, uv1, uv2, K, nt, T, max_err, min_angle, angle_strict, points, keep, counts);
    return EACHAM_OK;
}

}  // extern "C"
