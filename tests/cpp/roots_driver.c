/* roots_driver.c — the root rules of the three CPU restatements, callable on a polynomial alone (tests/test_essential5_reference.py
 * builds it as a shared library with the host compiler):
 *   degree 10  real_roots10  oracle/solve_oracle.c               (five-point solver)
 *   degree 4   real_roots4   tests/cpp/p3p_reference.c           (P3P)
 *   degree 3   real_roots3   tests/cpp/fundamental_reference.c   (seven-point solver)
 * The three are static in their files: the files are included, nothing of them is restated here.
 * c: degree + 1 coefficients, ascending. roots: room for `degree`. Returns the number of real roots, ascending in `roots`; -1 for another degree. */
#include "../../oracle/solve_oracle.c"
#include "fundamental_reference.c"
#include "p3p_reference.c"

int roots_driver(int degree, const double* c, double* roots) {
    if (degree == 10) return real_roots10(c, roots);
    if (degree == 4) return real_roots4(c[0], c[1], c[2], c[3], c[4], roots);
    if (degree == 3) return real_roots3(c[0], c[1], c[2], c[3], roots);
    return -1;
}
