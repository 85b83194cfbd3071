// imag_host_check.cpp -- stand-alone driver of the imaginary-time host algebra
// (cal_expm_real_col1: dense.cpp + host_api.cpp) for the sanitized build
// (csrc/Makefile `imag-host-san`: g++ -fsanitize=address,undefined; no HIP,
// no GPU).  Fixed inputs.  For a diagonal T the first column is e_1 exactly
// (the shift makes its exponent zero); for a symmetric 2 x 2 the column is
// known in closed form and is checked to the bar of tests/test_imagtime_host.py
// (64 eps max(1, ||tau T||_1), relative to the exponential's norm); larger
// tridiagonals with a padded leading dimension must give finite columns whose
// first entry is positive.  Any out-of-bounds access, leak or undefined
// behaviour aborts the program.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/calanczos_host.h"

static const double kEps = 2.220446049250313e-16;

static int check_diagonal(int m, double tau) {
    std::vector<double> T((size_t)m * m, 0.0), c(m, -1.0);
    for (int i = 0; i < m; ++i) T[i + (size_t)i * m] = 1.5 + i;
    if (cal_expm_real_col1(m, T.data(), m, tau, c.data()) != 0) return 1;
    for (int i = 0; i < m; ++i)
        if (c[i] != (i == 0 ? 1.0 : 0.0)) {
            std::printf("FAIL diagonal m=%d i=%d %g\n", m, i, c[i]);
            return 1;
        }
    return 0;
}

// T = [[a, b], [b, d]]: with h = (d - a)/2 and r = hypot(h, b), the first column of
// expm(-tau (T - a I)) is exp(-tau h) [cosh(tau r) + (h/r) sinh(tau r), -(b/r) sinh(tau r)]
static int check_2x2(double a, double b, double d, double tau) {
    const double T[4] = {a, b, b, d};
    double c[2];
    if (cal_expm_real_col1(2, T, 2, tau, c) != 0) return 1;
    const double h = 0.5 * (d - a), r = std::hypot(h, b);
    const double e0 = std::exp(-tau * h) * (std::cosh(tau * r) + h / r * std::sinh(tau * r));
    const double e1 = -std::exp(-tau * h) * b / r * std::sinh(tau * r);
    const double nrm = std::exp(tau * (r - h));  // the exponential's 2-norm: its largest eigenvalue
    const double n1 = std::fabs(tau) * std::fmax(std::fabs(a) + std::fabs(b), std::fabs(b) + std::fabs(d));
    const double err = std::hypot(c[0] - e0, c[1] - e1) / nrm, bar = 64.0 * kEps * std::fmax(1.0, n1);
    std::printf("2x2 tau=%g ||tau T||_1=%.3g err=%.3e bar=%.3e\n", tau, n1, err, bar);
    if (!(err <= bar)) {
        std::printf("FAIL 2x2\n");
        return 1;
    }
    return 0;
}

static int check_finite(int m, double tau, int ldt) {
    std::vector<double> T((size_t)ldt * m, std::nan("")), c(m);  // the pad rows are never read
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) T[i + (size_t)j * ldt] = 0.0;
    for (int i = 0; i < m; ++i) {
        T[i + (size_t)i * ldt] = 2.0 + std::sin((double)i);
        if (i + 1 < m) {
            const double e = 1.0 / (1.0 + (i % 3));
            T[(i + 1) + (size_t)i * ldt] = e;
            T[i + (size_t)(i + 1) * ldt] = e * (1.0 + 1e-9);  // only nearly symmetric, as the CA loop's T
        }
    }
    if (cal_expm_real_col1(m, T.data(), ldt, tau, c.data()) != 0) return 1;
    for (int i = 0; i < m; ++i)
        if (!std::isfinite(c[i])) {
            std::printf("FAIL finite m=%d\n", m);
            return 1;
        }
    if (!(c[0] > 0.0)) {
        std::printf("FAIL sign m=%d\n", m);
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    bad += check_diagonal(1, 3.0);
    bad += check_diagonal(5, 0.25);
    bad += check_2x2(1.0, 0.5, 2.0, 0.3);
    bad += check_2x2(-0.7, 1.1, -0.9, 40.0);
    bad += check_2x2(3.0, 0.2, 1.0, 100.0);
    bad += check_finite(7, 0.3, 9);
    bad += check_finite(24, 2.5, 24);
    bad += check_finite(48, 10.0, 50);
    bad += check_finite(97, 100.0, 101);
    // error paths: no access to the arrays
    std::vector<double> T(4, 1.0), c(2);
    if (cal_expm_real_col1(0, T.data(), 1, 0.1, c.data()) != CAL_ERR_ARG) bad++;
    if (cal_expm_real_col1(513, T.data(), 513, 0.1, c.data()) != CAL_ERR_ARG) bad++;
    if (cal_expm_real_col1(2, T.data(), 1, 0.1, c.data()) != CAL_ERR_ARG) bad++;
    if (cal_expm_real_col1(2, T.data(), 2, std::nan(""), c.data()) != CAL_ERR_ARG) bad++;
    T[1] = INFINITY;
    if (cal_expm_real_col1(2, T.data(), 2, 0.1, c.data()) != CAL_ERR_NUMERIC) bad++;
    // a NaN that e_1 is not coupled to: blkdiag([1], [NaN])
    const double D[4] = {1.0, 0.0, 0.0, std::nan("")};
    if (cal_expm_real_col1(2, D, 2, 0.1, c.data()) != CAL_ERR_NUMERIC) bad++;
    std::printf(bad ? "FAILED %d\n" : "imag host check ok\n", bad);
    return bad ? 1 : 0;
}
