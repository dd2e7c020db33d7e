/* CPU reference of the dot-product matcher (eacham_match_pair_dot / _pairs_directed_dot / _all_pairs_dot of
 * include/eacham_hip.h). Test infrastructure: tests/dot_reference.py compiles it with the host compiler.
 *
 *   s(q,t) = a_q . b_t, fp32, the k-ordered fmaf chain from 0 (what v_mfma_f32_32x32x2_f32 produces; the same chain as
 *            dist2_dot_f32 of oracle/match_oracle.c, without the norm step). Nothing is normalised.
 *   directed: t0 = argmax_t s(q,t), lower t on equal similarity; keep iff s(q,t0) > min_score (strict). Every comparison is
 *             a strict '>' against a running best that starts at -inf with no index: NaN (and -inf) never win, never pass.
 *   mutual:   m12, m21 directed; dropped if |m12| < min_dir or |m21| < min_dir; mutual = {(q,t) in m12 : m21[t] == q};
 *             edge iff |mutual| > min_mutual. stats = {|m12|, |m21|, |mutual|, edge}.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static inline float dot_f32(const float* a, const float* b, int dim) {
    float s = 0.0f;
    for (int k = 0; k < dim; ++k) s = fmaf(a[k], b[k], s);
    return s;
}

/* best[q] = argmax_t (or -1), score[q] = its similarity (-inf when there is none) */
static void argmax_rows(const float* A, int n1, const float* B, int n2, int dim, int32_t* best, float* score) {
#pragma omp parallel for schedule(static)
    for (int q = 0; q < n1; ++q) {
        float sb = -INFINITY;
        int32_t tb = -1;
        for (int t = 0; t < n2; ++t) {
            const float s = dot_f32(A + (size_t)q * dim, B + (size_t)t * dim, dim);
            if (s > sb) {
                sb = s;
                tb = t;
            }
        }
        best[q] = tb;
        score[q] = sb;
    }
}

/* the raw row result (for the tests that look at gaps): best index and similarity per row of A */
void dotref_argmax(const float* A, int n1, const float* B, int n2, int dim, int32_t* best, float* score) {
    argmax_rows(A, n1, B, n2, dim, best, score);
}

/* returns the number of matches; q, t, score hold up to n1 entries, sorted by q */
int dotref_match_directed(const float* A, int n1, const float* B, int n2, int dim, float min_score, uint32_t* q, uint32_t* t,
                          float* score) {
    int32_t* best = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n1 > 0 ? n1 : 1));
    float* sc = (float*)malloc(sizeof(float) * (size_t)(n1 > 0 ? n1 : 1));
    argmax_rows(A, n1, B, n2, dim, best, sc);
    int cnt = 0;
    for (int i = 0; i < n1; ++i)
        if (best[i] >= 0 && sc[i] > min_score) {
            q[cnt] = (uint32_t)i;
            t[cnt] = (uint32_t)best[i];
            score[cnt] = sc[i];
            ++cnt;
        }
    free(best);
    free(sc);
    return cnt;
}

/* returns the count the C-ABI reports for the pair (|mutual| for an edge, 0 otherwise); q, t, score hold |mutual| entries
 * whenever the pair is an edge */
int dotref_match_mutual(const float* A, int n1, const float* B, int n2, int dim, float min_score, int min_dir, int min_mutual,
                        uint32_t* q, uint32_t* t, float* score, int32_t* stats) {
    int32_t* b12 = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n1 > 0 ? n1 : 1));
    float* s12 = (float*)malloc(sizeof(float) * (size_t)(n1 > 0 ? n1 : 1));
    int32_t* b21 = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n2 > 0 ? n2 : 1));
    float* s21 = (float*)malloc(sizeof(float) * (size_t)(n2 > 0 ? n2 : 1));
    argmax_rows(A, n1, B, n2, dim, b12, s12);
    argmax_rows(B, n2, A, n1, dim, b21, s21); /* fmaf(a, b, s) == fmaf(b, a, s): the same similarities, seen by column */
    int c12 = 0, c21 = 0, m = 0;
    for (int i = 0; i < n1; ++i) c12 += b12[i] >= 0 && s12[i] > min_score;
    for (int j = 0; j < n2; ++j) c21 += b21[j] >= 0 && s21[j] > min_score;
    for (int i = 0; i < n1; ++i) {
        if (!(b12[i] >= 0 && s12[i] > min_score)) continue;
        const int j = b12[i];
        if (b21[j] == i && s21[j] > min_score) {
            q[m] = (uint32_t)i;
            t[m] = (uint32_t)j;
            score[m] = s12[i];
            ++m;
        }
    }
    const int edge = c12 >= min_dir && c21 >= min_dir && m > min_mutual;
    if (stats) {
        stats[0] = c12;
        stats[1] = c21;
        stats[2] = m;
        stats[3] = edge;
    }
    free(b12);
    free(s12);
    free(b21);
    free(s21);
    return edge ? m : 0;
}
