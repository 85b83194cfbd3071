// prop_host_check.cpp -- stand-alone driver of the propagator's host algebra
// (cal_expm_col1: dense.cpp + host_api.cpp) for the sanitized build
// (csrc/Makefile `prop-host-san`: g++ -fsanitize=address,undefined; no HIP,
// no GPU).  Fixed inputs; for symmetric T the first column of expm(-i dt T)
// has unit 2-norm, which is checked to the bar of tests/test_prop_host.py
// (64 eps max(1, ||dt T||_1)); m = 1 is checked against cos / sin.  Any
// out-of-bounds access, leak or undefined behaviour aborts the program.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/calanczos_host.h"

static int check_unitary(int m, double dt, int ldt) {
    // symmetric tridiagonal: d_i = 2 + sin(i), e_i = 1 / (1 + (i % 3)), stored with ld ldt
    std::vector<double> T((size_t)ldt * m, 0.0);
    for (int i = 0; i < m; ++i) {
        T[i + (size_t)i * ldt] = 2.0 + std::sin((double)i);
        if (i + 1 < m) {
            const double e = 1.0 / (1.0 + (i % 3));
            T[(i + 1) + (size_t)i * ldt] = e;
            T[i + (size_t)(i + 1) * ldt] = e;
        }
    }
    double nrm1 = 0.0;
    for (int j = 0; j < m; ++j) {
        double cs = 0.0;
        for (int i = 0; i < m; ++i) cs += std::fabs(dt * T[i + (size_t)j * ldt]);
        nrm1 = std::fmax(nrm1, cs);
    }
    std::vector<double> cr(m), ci(m);
    const int st = cal_expm_col1(m, T.data(), ldt, dt, cr.data(), ci.data());
    if (st != 0) {
        std::printf("FAIL m=%d dt=%g status %d\n", m, dt, st);
        return 1;
    }
    double n2 = 0.0;
    for (int i = 0; i < m; ++i) n2 += cr[i] * cr[i] + ci[i] * ci[i];
    const double dev = std::fabs(std::sqrt(n2) - 1.0), bar = 64.0 * 2.220446049250313e-16 * std::fmax(1.0, nrm1);
    std::printf("m=%d dt=%g norm1=%.3g |norm-1|=%.3e bar=%.3e\n", m, dt, nrm1, dev, bar);
    if (!(dev <= bar)) {
        std::printf("FAIL unitarity\n");
        return 1;
    }
    if (m == 1) {
        const double x = dt * T[0];
        if (std::fabs(cr[0] - std::cos(x)) > bar || std::fabs(ci[0] + std::sin(x)) > bar) {
            std::printf("FAIL m=1 value\n");
            return 1;
        }
    }
    return 0;
}

int main() {
    int bad = 0;
    bad += check_unitary(1, 0.7, 1);
    bad += check_unitary(2, 0.001, 2);
    bad += check_unitary(7, 0.3, 9);
    bad += check_unitary(24, 2.5, 24);
    bad += check_unitary(48, 10.0, 50);
    bad += check_unitary(121, 0.025, 121);
    // error paths: no access to the arrays
    std::vector<double> T(4, 1.0), c(2);
    if (cal_expm_col1(0, T.data(), 1, 0.1, c.data(), c.data()) != CAL_ERR_ARG) bad++;
    if (cal_expm_col1(513, T.data(), 513, 0.1, c.data(), c.data()) != CAL_ERR_ARG) bad++;
    if (cal_expm_col1(2, T.data(), 1, 0.1, c.data(), c.data()) != CAL_ERR_ARG) bad++;
    if (cal_expm_col1(2, T.data(), 2, std::nan(""), c.data(), c.data()) != CAL_ERR_ARG) bad++;
    std::printf(bad ? "FAILED %d\n" : "prop host check ok\n", bad);
    return bad ? 1 : 0;
}
