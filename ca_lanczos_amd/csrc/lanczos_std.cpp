// lanczos_std.cpp -- the standard (one vector per SpMV) Lanczos of the
// reference, [T,Q,ritz_rnorm,orth_err] = lanczos(A,r,maxiter,orth)
// (lanczos.m:18-311), device-resident: the other half of every experiment
// script's ca_lanczos / lanczos comparison.
//
// One step (lanczos.m:103-110) is three launches:
//   SpMV mode 4   r = A q_j - beta_{j-1} q_{j-1}, block partials of r'q_j
//   k_pro_update  alpha_j = sum of the partials; r -= alpha_j q_j; partials of r'r
//   k_pro_div     beta_j^2 = their sum; q_{j+1} = r / beta_j
// alpha_j and beta_j^2 stay on the device and feed the next kernels; 'local'
// and 'full' enqueue any number of steps without a host round trip.  An SpMV
// grid of more than kInKernelParts blocks (CSR row blocks) is summed by
// k_reduce first.  A matrix on the row-pattern kernels without a fused mode
// (k_spmv_pat, k_spmv_pat_lds) runs SpMV mode 0 + launch_pro_step, the Newton
// prologue's step (info.fused = 0); so does the test build under
// CAL_TEST_LANCZOS_SPLIT.  One rank only.
//
//   local      nothing more.  keep_Q = 0 keeps a ring of three columns.
//   full       one CGS pass of q_{j+1} against Q(:,1:j) (:62-66) on the device
//              (Gram, [-R; 1], apply: the Newton prologue's chain), Q(:,1:j)
//              in blocks of 128 columns whose Grams are all taken before the
//              first update (so it stays CGS).  T is not touched, q_{j+1} is
//              not renormalised, as in the reference.
//   periodic   normest(A), the omega recurrence of lanczos.m:267-311 on the
//              host, and when max|omega(j+1,1:j)| >= sqrt(eps):
//              Q(:,j-5:j+1) = projectAndNormalize({Q(:,1:j-6)}, Q(:,j-5:j+1), true).
//              For j <= 6 the reference indexes out of range; here the window
//              is clamped to start at column 1 and the earlier block is empty.
//   selective  eig(T_j) on the host each step, the count of
//              beta(i)*|Vp(j,i)| < normest(A)*sqrt(eps) (the reference's
//              beta(i), literally), QR = Q(:,1:j)*Vp(:,conv) rebuilt on the
//              device when it grows, and while nritz > 0
//              Q(:,j+1) = projectAndNormalize({QR}, Q(:,j+1), false).
// periodic and selective read alpha_j, beta_j on the host every step.
// Earlier blocks wider than 128 columns are handed to project.m's block loop
// in blocks of 128 (block MGS across them), the one deviation from a literal
// single block.
// Diagnostics (:117-126): rn(j,1:j) by the library's device Ritz-residual
// path, oe(j) = max(Q(:,1:j)'*Q(:,j+1)) (signed); they never feed back.
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "cal_internal.hpp"
#include "comm.hpp"
#include "dense.hpp"

namespace cal {

struct StdLanczosState {
    int64_t n = 0, ld = 0, lpad = 0;
    uint64_t A_gen = 0;
    int m = 0;     // maxiter
    int mode = 0;  // 0 local, 1 full, 2 periodic, 3 selective
    bool keep_Q = true;
    int ncols = 0;          // columns of dQ: m + 1, or the ring's 3
    double* dQ = nullptr;   // the Lanczos vectors
    double* dr = nullptr;   // r, then the 7-column window copy and its work block (periodic / selective)
    double* dQR = nullptr;  // selective: the locked Ritz vectors (m columns, lazily)
    double* d_ab = nullptr;   // alpha [0, m), beta^2 [m, 2m)
    double* d_part = nullptr; // SpMV partials [0, nparts), their sum, alpha / beta^2 partials (2 dot_blocks)
    double* d_cg = nullptr;   // full: per 128-column block the Gram (2048) and M (256)
    double* h_ab = nullptr;   // pinned, 2 m
    int nparts = 0;           // mode 4's partials (0: unfused)
    bool fused = false;
    int j = 0;            // steps enqueued
    int synced = 0;       // steps whose alpha, beta are on the host
    bool broken = false;
    std::vector<double> alpha, beta, rn, oe;
    // periodic
    std::vector<double> omega;  // (m + 2)^2, 1-based accessor below
    // selective
    int nritz = 0;
    cal_std_lanczos_info info{};
    double* col(int jc) const { return dQ + (size_t)(keep_Q ? jc : jc % 3) * ld + lpad; }
    double* r() const { return dr + lpad; }
    double* wcol(int k) const { return dr + (size_t)(1 + k) * ld + lpad; }  // k < 14
    double& om(int i, int k) { return omega[(size_t)(i - 1) + (size_t)(k - 1) * (m + 2)]; }
};

namespace {

constexpr int kInKernelParts = 4096;  // k_pro_update sums up to this many SpMV partials itself
constexpr int kCgsBlock = 128;        // columns per Gram / apply of the CGS pass
constexpr int kWin = 7;               // periodic: the reorthogonalised window (lanczos.m:253)

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void std_free(cal_ctx* c) {
    if (!c || !c->slz) return;
    StdLanczosState* L = c->slz;
    if (L->dQ) hipFree(L->dQ);
    if (L->dr) hipFree(L->dr);
    if (L->dQR) hipFree(L->dQR);
    if (L->d_ab) hipFree(L->d_ab);
    if (L->d_part) hipFree(L->d_part);
    if (L->d_cg) hipFree(L->d_cg);
    if (L->h_ab) hipHostFree(L->h_ab);
    delete L;
    c->slz = nullptr;
}

int parse_orth(const char* orth) {
    std::string o = orth ? orth : "";
    for (auto& ch : o) ch = (char)tolower(ch);
    if (o == "local") return 0;
    if (o == "full") return 1;
    if (o == "periodic") return 2;
    if (o == "selective") return 3;
    return -1;
}

int check_ctx(cal_ctx* c) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    if (!c->has_A) return set_error(c, CAL_ERR_NOMATRIX, "no matrix set on the context");
    if (c->comm && c->comm->nranks > 1)
        return set_error(c, CAL_ERR_UNSUPPORTED, "the standard Lanczos solver runs on one rank");
    return 0;
}

// lanczos.m:103-110 for step j (0-based), enqueued
int recurrence(cal_ctx* c, StdLanczosState& L, int j) {
    const int64_t n = L.n;
    const int m = L.m, nb = dot_blocks(n);
    double* q = L.col(j);
    const double* qprev = j > 0 ? L.col(j - 1) : nullptr;
    const double* pbprev = j > 0 ? L.d_ab + m + j - 1 : nullptr;
    double* qnext = L.col(j + 1);
    double* pa = L.d_part;                      // SpMV partials
    double* ps = L.d_part + L.nparts;           // their sum (large grids)
    double* pab = L.d_part + L.nparts + 8;      // alpha / beta^2 partials of the vector kernels
    if (L.fused) {
        CAL_TRY(spmv_lanczos_dev(c, q, qprev, pbprev, L.r(), pa));
        const double* pin = pa;
        int np = L.nparts;
        if (np > kInKernelParts) {
            CAL_HIP_OTHER(c, launch_reduce(pa, np, 1, ps, c->stream));
            pin = ps;
            np = 1;
        }
        const int t = timer_begin(c, 3, 40.0 * n);
        const hipError_t e =
            launch_pro_tail(L.r(), q, qnext, n, pin, np, pab + nb, L.d_ab + j, L.d_ab + m + j, c->stream);
        timer_end(c, t);
        if (e != hipSuccess) return hip_fail(c, e, "launch_pro_tail");
        return 0;
    }
    CAL_TRY(spmv_dev(c, q, L.r(), 0, 0.0, 0.0, nullptr));
    const int t = timer_begin(c, 3, (j > 0 ? 72.0 : 64.0) * n);
    const hipError_t e = launch_pro_step(L.r(), qprev, pbprev, q, qnext, n, pab, L.d_ab + j, L.d_ab + m + j, c->stream);
    timer_end(c, t);
    if (e != hipSuccess) return hip_fail(c, e, "launch_pro_step");
    return 0;
}

// one CGS pass of q_{j+1} against Q(:,0..j) (lanczos.m:62-66), enqueued
int cgs_pass(cal_ctx* c, StdLanczosState& L, int j) {
    const int64_t n = L.n, ld = L.ld;
    const int w = j + 1, nblk = (w + kCgsBlock - 1) / kCgsBlock;
    double* qn = L.col(j + 1);
    Panel B = panel();
    panel_add(B, qn, ld, 1);
    for (int b = 0; b < nblk; ++b) {  // every Gram before the first update
        const int c0 = b * kCgsBlock, wb = std::min(kCgsBlock, w - c0);
        Panel Qb = panel();
        panel_add(Qb, L.col(c0), ld, wb);
        const GramPlan pl = gram_plan(wb, 1, n);
        CAL_TRY(ensure_partial(c, (size_t)pl.blocks * pl.entries));
        const int t = timer_begin(c, 1, 8.0 * n * (wb + 1));
        CAL_HIP(c, launch_gram(Qb, B, n, pl, c->d_partial, c->stream));
        timer_end(c, t);
        CAL_HIP_OTHER(c, launch_reduce(c->d_partial, pl.blocks, pl.entries, L.d_cg + (size_t)b * 2304, c->stream));
    }
    for (int b = 0; b < nblk; ++b) {
        const int c0 = b * kCgsBlock, wb = std::min(kCgsBlock, w - c0);
        const GramPlan pl = gram_plan(wb, 1, n);
        double* dG = L.d_cg + (size_t)b * 2304;
        double* dM = dG + 2048;
        CAL_HIP_OTHER(c, launch_form_projM(dG, 16 * pl.nta, wb, 1, dM, c->stream));
        Panel W = panel();  // [Q_b | q_{j+1}]: contiguous for the last block
        if (c0 + wb == w) {
            panel_add(W, L.col(c0), ld, wb + 1);
        } else {
            panel_add(W, L.col(c0), ld, wb);
            panel_add(W, qn, ld, 1);
        }
        const ApplyPlan ap = apply_plan(wb + 1, 1, n, false, 0);
        const int t = timer_begin(c, 2, 8.0 * n * (wb + 2));
        CAL_HIP(c, launch_apply(W, dM, wb + 1, 1, panel_out(qn, ld, 1), true, 0, n, ap, c->d_partial, c->stream));
        timer_end(c, t);
    }
    return 0;
}

// alpha, beta of the steps enqueued so far onto the host; the first beta that
// is not finite and positive cuts the run there
int sync_ab(cal_ctx* c, StdLanczosState& L) {
    if (L.synced >= L.j) return 0;
    const int m = L.m;
    CAL_HIP(c, hipMemcpyAsync(L.h_ab, L.d_ab, 2 * (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    for (int j = L.synced; j < L.j && !L.broken; ++j) {
        L.alpha[j] = L.h_ab[j];
        const double b2 = L.h_ab[m + j];
        const double b = std::sqrt(b2);
        if (!std::isfinite(L.alpha[j])) {  // a non-finite matrix or start vector
            L.alpha[j] = 0.0;
            L.beta[j] = 0.0;
            L.broken = true;
            L.info.steps = j;
        } else if (!(b > 0.0) || !std::isfinite(b)) {
            L.beta[j] = 0.0;
            L.broken = true;
            L.info.steps = j + 1;
        } else {
            L.beta[j] = b;
            L.info.steps = j + 1;
        }
    }
    L.synced = L.j;
    L.info.breakdown = L.broken ? 1 : 0;
    return 0;
}

// T_j = tridiag(alpha(1:j), beta(1:j-1)), [Vp, Dp] = eig(T_j) ascending
void eig_Tj(const StdLanczosState& L, int j, std::vector<double>& w, std::vector<double>& V) {
    std::vector<double> T((size_t)j * j, 0.0);
    for (int i = 0; i < j; ++i) {
        T[i + (size_t)i * j] = L.alpha[i];
        if (i + 1 < j) T[i + 1 + (size_t)i * j] = T[i + (size_t)(i + 1) * j] = L.beta[i];
    }
    w.assign(j, 0.0);
    V.assign((size_t)j * j, 0.0);
    dense::eig_symmetric(j, T.data(), j, w.data(), V.data(), j);
}

// projectAndNormalize({Qp(:, 0:wp)}, X, doreorth) -> X, X being nx columns at dX
int pn_inplace(cal_ctx* c, StdLanczosState& L, double* Qp, int wp, double* dX, int nx, bool doreorth) {
    const int64_t n = L.n, ld = L.ld;
    double* Xc = L.wcol(0);       // the copy projectAndNormalize reads
    double* Yw = L.wcol(kWin);    // its work block
    CAL_HIP(c, copy_cols(c, Xc, dX, ld, n, nx));
    std::vector<double*> blocks;
    std::vector<int> widths;
    for (int c0 = 0; c0 < wp; c0 += 128) {
        blocks.push_back(Qp + (size_t)c0 * ld);
        widths.push_back(std::min(128, wp - c0));
    }
    std::vector<std::vector<double>> RZ;
    std::vector<double> R((size_t)nx * nx);
    bool re = false;
    int rank = nx;
    return project_and_normalize_blocks_dev(c, n, ld, (int)blocks.size(), blocks, widths.data(), nx, Xc, doreorth, Yw,
                                            panel_out(dX, ld, nx), RZ, R.data(), &re, &rank);
}

// lanczos.m:267-300 for n = j (1-based), in place in the fixed-size omega
void update_omega(StdLanczosState& L, int n) {
    const double T = std::numeric_limits<double>::epsilon() * L.info.norm_A;
    auto al = [&](int i) { return L.alpha[i - 1]; };
    auto be = [&](int i) { return L.beta[i - 1]; };
    const double binv = 1.0 / be(n);
    if (n == 1) {
        L.om(1, 1) = 1.0;
        L.om(1, 2) = 0.0;
        L.om(2, 1) = binv * T;
        L.om(2, 2) = 1.0;
        return;
    }
    double v = be(2) * L.om(n, 2) + (al(1) - al(n)) * L.om(n, 1) - be(n) * L.om(n - 1, 1);
    L.om(n + 1, 1) = v > 0 ? binv * (v + T) : binv * (v - T);
    for (int k = 2; k <= n - 1; ++k) {
        v = be(k + 1) * L.om(n, k + 1) + (al(k) - al(n)) * L.om(n, k) + be(k) * L.om(n, k - 1) - be(n) * L.om(n - 1, k);
        L.om(n + 1, k) = v > 0 ? binv * (v + T) : binv * (v - T);
    }
    L.om(n + 1, n) = binv * T;
    L.om(n + 1, n + 1) = 1.0;
}

// lanczos.m:302-311: rows n and n + 1
void reset_omega(StdLanczosState& L, int n) {
    const double T = std::numeric_limits<double>::epsilon() * L.info.norm_A;
    for (int k = 1; k <= n; ++k) {
        L.om(n, k) = T;
        L.om(n + 1, k) = T;
    }
    L.om(n, n) = 1.0;
    L.om(n, n + 1) = 0.0;
    L.om(n + 1, n + 1) = 1.0;
}

// lanczos.m:117-126 after step j (1-based): rn(j,1:j), oe(j)
int diagnostics_step(cal_ctx* c, StdLanczosState& L, int j) {
    const int m = L.m;
    std::vector<double> w, V, rnj(j);
    eig_Tj(L, j, w, V);
    CAL_TRY(ritz_rnorm_dev(c, L.col(0), j, V.data(), w.data(), rnj.data()));
    for (int i = 0; i < j; ++i) L.rn[(size_t)(j - 1) + (size_t)i * m] = rnj[i];
    Panel Qj = panel();
    panel_add(Qj, L.col(0), L.ld, j);
    Panel qn = panel();
    panel_add(qn, L.col(j), L.ld, 1);
    std::vector<double> g(j);
    CAL_TRY(gram_host(c, L.n, Qj, qn, g.data()));
    double mx = g[0];  // MATLAB's max: NaN only if every entry is
    for (int i = 1; i < j; ++i)
        if (std::isnan(mx) || g[i] > mx) mx = g[i];
    L.oe[j - 1] = mx;
    return 0;
}

int selective_step(cal_ctx* c, StdLanczosState& L, int j) {
    const int64_t n = L.n, ld = L.ld;
    const double thr = L.info.norm_A * std::sqrt(std::numeric_limits<double>::epsilon());
    std::vector<double> w, V;
    eig_Tj(L, j, w, V);
    std::vector<int> conv;
    for (int i = 0; i < j; ++i)
        if (L.beta[i] * std::fabs(V[(size_t)(j - 1) + (size_t)i * j]) < thr) conv.push_back(i);
    if ((int)conv.size() > L.nritz) {
        L.info.n_orth_breaks++;
        L.nritz = (int)conv.size();
        L.info.n_ritz_locked = L.nritz;
        if (!L.dQR) {
            CAL_HIP(c, hipMalloc((void**)&L.dQR, (size_t)L.m * ld * sizeof(double)));
            CAL_HIP(c, hipMemsetAsync(L.dQR, 0, (size_t)L.m * ld * sizeof(double), c->stream));
        }
        std::vector<double> M((size_t)j * L.nritz);
        for (int k = 0; k < L.nritz; ++k)
            for (int i = 0; i < j; ++i) M[i + (size_t)k * j] = V[i + (size_t)conv[k] * j];
        CAL_TRY(ensure_small(c, M.size()));
        CAL_HIP(c, hipMemcpyAsync(c->d_small, M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        double* QR = L.dQR + L.lpad;
        if (apply_mt_ok(j, L.nritz)) {
            const int t = timer_begin(c, 2, 8.0 * n * (j + L.nritz));
            CAL_HIP(c, launch_apply_mt(L.col(0), ld, c->d_small, j, L.nritz, QR, ld, n, c->stream));
            timer_end(c, t);
        } else {
            Panel Qj = panel();
            panel_add(Qj, L.col(0), ld, j);
            CAL_TRY(apply_dev(c, n, Qj, c->d_small, L.nritz, panel_out(QR, ld, L.nritz)));
        }
        CAL_HIP(c, hipStreamSynchronize(c->stream));  // M is a local
    }
    if (L.nritz > 0) CAL_TRY(pn_inplace(c, L, L.dQR + L.lpad, L.nritz, L.col(j), 1, false));
    return 0;
}

int periodic_step(cal_ctx* c, StdLanczosState& L, int j) {
    update_omega(L, j);
    double err = 0.0;
    for (int k = 1; k <= j; ++k) {
        const double a = std::fabs(L.om(j + 1, k));
        if (std::isnan(a) || a > err) err = a;
    }
    if (!(err >= std::sqrt(std::numeric_limits<double>::epsilon()))) return 0;
    L.info.n_orth_breaks++;
    // 1-based columns j-5 .. j+1, clamped to start at 1; 0-based first = max(j - 6, 0)
    const int first = std::max(j - 6, 0), nx = j + 1 - first;
    CAL_TRY(pn_inplace(c, L, L.col(0), first, L.col(first), nx, true));
    reset_omega(L, j);
    return 0;
}

}  // namespace
}  // namespace cal

using namespace cal;

extern "C" {

void cal_std_lanczos_free_state(cal_ctx* c) { std_free(c); }

static int std_begin(cal_ctx* c, const double* r, int maxiter, const char* orth, int keep_Q) {
    CAL_TRY(check_ctx(c));
    const int mode = parse_orth(orth);
    if (mode < 0)
        return set_error(c, CAL_ERR_ARG, std::string("lanczos: Invalid option value for orth: ") + (orth ? orth : ""));
    const int64_t n = c->A.n_local, ld = c->A.ld;
    if (!r || maxiter < 1 || maxiter > n) return set_error(c, CAL_ERR_ARG, "lanczos: need r and 1 <= maxiter <= n");
    if (!keep_Q && mode != 0) return set_error(c, CAL_ERR_ARG, "lanczos: keep_Q = 0 needs orth = 'local'");
    if (mode >= 2) CAL_TRY(shared_refuses(c, "orth = 'periodic' / 'selective' (normest)"));
    std_free(c);
    StdLanczosState* L = new StdLanczosState();
    c->slz = L;
    L->n = n;
    L->ld = ld;
    L->lpad = c->A.lpad;
    L->A_gen = c->A_gen;
    L->m = maxiter;
    L->mode = mode;
    L->keep_Q = keep_Q != 0;
    L->ncols = L->keep_Q ? maxiter + 1 : 3;
    const int m = maxiter, nb = dot_blocks(n);
    L->alpha.assign(m, 0.0);
    L->beta.assign(m, 0.0);
    L->oe.assign(m, 0.0);
    const int ncr = mode >= 2 ? 1 + 2 * kWin : 1;
    CAL_HIP(c, hipMalloc((void**)&L->dQ, (size_t)L->ncols * ld * sizeof(double)));
    CAL_HIP(c, hipMalloc((void**)&L->dr, (size_t)ncr * ld * sizeof(double)));
    CAL_HIP(c, hipMalloc((void**)&L->d_ab, 2 * (size_t)m * sizeof(double)));
    CAL_HIP(c, hipHostMalloc((void**)&L->h_ab, 2 * (size_t)m * sizeof(double), hipHostMallocDefault));
    // the pad rows of every column stay zero (the plane march reads them)
    CAL_HIP(c, hipMemsetAsync(L->dQ, 0, (size_t)L->ncols * ld * sizeof(double), c->stream));
    CAL_HIP(c, hipMemsetAsync(L->dr, 0, (size_t)ncr * ld * sizeof(double), c->stream));
    CAL_HIP(c, hipMemsetAsync(L->d_ab, 0, 2 * (size_t)m * sizeof(double), c->stream));
    L->nparts = test_switch("CAL_TEST_LANCZOS_SPLIT") ? 0 : spmv_lanczos_parts(c, L->col(0), L->col(1), L->r());
    L->fused = L->nparts > 0;
    L->info.fused = L->fused ? 1 : 0;
    CAL_HIP(c, hipMalloc((void**)&L->d_part, ((size_t)L->nparts + 8 + 2 * (size_t)nb) * sizeof(double)));
    if (mode == 1) {
        const int nblk = (m + kCgsBlock - 1) / kCgsBlock;
        CAL_HIP(c, hipMalloc((void**)&L->d_cg, (size_t)nblk * 2304 * sizeof(double)));
    }
    if (mode == 2) L->omega.assign((size_t)(m + 2) * (m + 2), 0.0);
    if (mode >= 2) CAL_TRY(normest_run(c, &L->info.norm_A));  // lanczos.m:146,219
    // q = r / norm(r) (lanczos.m:47)
    double* q0 = L->col(0);
    CAL_HIP(c, hipMemcpyAsync(q0, r, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CAL_HIP_OTHER(c, launch_dot(q0, q0, n, L->d_part, nb, c->stream));
    CAL_HIP_OTHER(c, launch_reduce(L->d_part, nb, 1, L->d_ab, c->stream));
    CAL_HIP(c, hipMemcpyAsync(L->h_ab, L->d_ab, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    const double nrm = std::sqrt(L->h_ab[0]);
    if (!(nrm > 0.0) || !std::isfinite(nrm))
        return set_error(c, CAL_ERR_ARG, "lanczos: the start vector must be finite and non-zero");
    CAL_HIP_OTHER(c, launch_div(q0, q0, nrm, n, c->stream));
    return 0;
}

int cal_std_lanczos_begin(cal_ctx* c, const double* r, int maxiter, const char* orth, int keep_Q) {
    const int st = std_begin(c, r, maxiter, orth, keep_Q);
    if (st < 0 && c) std_free(c);  // no half-built solver is left behind
    return st;
}

int cal_std_lanczos_step(cal_ctx* c, int nsteps, int diagnostics) {
    if (!c) return CAL_ERR_ARG;
    if (!c->slz) return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_step: no active solver (cal_std_lanczos_begin)");
    CAL_TRY(check_ctx(c));
    StdLanczosState& L = *c->slz;
    if (L.A_gen != c->A_gen)
        return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_step: the context's matrix changed since begin");
    if (nsteps < 0 || L.j + nsteps > L.m)
        return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_step: nsteps runs past maxiter");
    if (diagnostics && !L.keep_Q)
        return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_step: diagnostics need keep_Q");
    if (diagnostics) CAL_TRY(shared_refuses(c, "the Ritz diagnostics' residual"));
    if (diagnostics && L.rn.empty()) L.rn.assign((size_t)L.m * L.m, 0.0);
    const bool host = diagnostics || L.mode >= 2;  // alpha, beta on the host every step
    const double t0 = now_ms();
    double tdiag = 0.0;
    for (int it = 0; it < nsteps && !L.broken; ++it) {
        const int j = L.j;  // 0-based
        CAL_TRY(recurrence(c, L, j));
        L.j = j + 1;
        if (L.mode == 1) CAL_TRY(cgs_pass(c, L, j));
        if (!host) continue;
        CAL_TRY(sync_ab(c, L));
        if (L.broken) break;
        if (L.mode == 3) CAL_TRY(selective_step(c, L, j + 1));
        if (diagnostics) {
            const double td = now_ms();
            CAL_TRY(diagnostics_step(c, L, j + 1));
            tdiag += now_ms() - td;
        }
        if (L.mode == 2) CAL_TRY(periodic_step(c, L, j + 1));
    }
    L.info.diag_ms += tdiag;
    L.info.loop_ms += now_ms() - t0 - tdiag;
    return L.broken ? CAL_WARN_BREAKDOWN : 0;
}

int cal_std_lanczos_get(cal_ctx* c, double* alpha, double* beta, double* rn, double* oe, cal_std_lanczos_info* info) {
    if (!c) return CAL_ERR_ARG;
    if (!c->slz) return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_get: no active solver");
    hipSetDevice(c->device);
    StdLanczosState& L = *c->slz;
    CAL_TRY(sync_ab(c, L));
    const int k = L.info.steps, m = L.m;
    for (int j = 0; j < k; ++j) {
        if (alpha) alpha[j] = L.alpha[j];
        if (beta) beta[j] = L.beta[j];
    }
    if (rn)
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) rn[j + (size_t)i * m] = L.rn.empty() ? 0.0 : L.rn[j + (size_t)i * m];
    if (oe)
        for (int j = 0; j < k; ++j) oe[j] = L.oe[j];
    if (info) *info = L.info;
    return L.broken ? CAL_WARN_BREAKDOWN : 0;
}

int cal_std_lanczos_get_Q(cal_ctx* c, int64_t col0, int ncols, double* Q) {
    if (!c) return CAL_ERR_ARG;
    if (!c->slz) return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_get_Q: no active solver");
    hipSetDevice(c->device);
    StdLanczosState& L = *c->slz;
    if (!L.keep_Q) return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_get_Q: the run keeps no Q (keep_Q = 0)");
    CAL_TRY(sync_ab(c, L));
    if (!Q || col0 < 0 || ncols < 0 || col0 + ncols > L.info.steps)
        return set_error(c, CAL_ERR_ARG, "cal_std_lanczos_get_Q: columns outside the kept steps");
    if (ncols == 0) return 0;
    CAL_HIP(c, hipMemcpy2DAsync(Q, L.n * sizeof(double), L.col((int)col0), L.ld * sizeof(double), L.n * sizeof(double),
                                ncols, hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cal_std_lanczos_end(cal_ctx* c) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    std_free(c);
    return 0;
}

int cal_lanczos(cal_ctx* c, const double* r, int maxiter, const char* orth, int diagnostics, double* T, double* Q,
                double* rn, double* oe, cal_std_lanczos_info* info) {
    if (!c) return CAL_ERR_ARG;
    if (!T) return set_error(c, CAL_ERR_ARG, "cal_lanczos: need T");
    const int mode = parse_orth(orth);
    const int keep = Q || diagnostics || mode != 0;
    CAL_TRY(cal_std_lanczos_begin(c, r, maxiter, orth, keep));
    int status = cal_std_lanczos_step(c, maxiter, diagnostics);
    const int m = maxiter;
    std::vector<double> a(m, 0.0), b(m, 0.0);
    if (status >= 0) {
        cal_std_lanczos_info inf{};
        const int st = cal_std_lanczos_get(c, a.data(), b.data(), rn, oe, &inf);
        status = st < 0 ? st : std::max(status, st);
        if (st >= 0) {
            const int k = inf.steps;
            std::memset(T, 0, (size_t)m * m * sizeof(double));
            for (int j = 0; j < k; ++j) {  // lanczos.m:131
                T[j + (size_t)j * m] = a[j];
                if (j + 1 < k) T[j + 1 + (size_t)j * m] = T[j + (size_t)(j + 1) * m] = b[j];
            }
            if (Q) {
                std::memset(Q, 0, (size_t)c->slz->n * m * sizeof(double));
                const int sq = cal_std_lanczos_get_Q(c, 0, k, Q);
                if (sq < 0) status = sq;
            }
            if (info) *info = inf;
        }
    }
    cal_std_lanczos_end(c);
    return status;
}

int cal_spmv_lanczos(cal_ctx* c, const double* x, const double* xprev, double beta2, double* y, double* dot) {
    CAL_TRY(check_ctx(c));
    if (!x || !y || !dot || (xprev && !(beta2 >= 0.0)))
        return set_error(c, CAL_ERR_ARG, "cal_spmv_lanczos: need x, y, dot and beta2 >= 0");
    const int64_t n = c->A.n_local, ld = c->A.ld;
    CAL_TRY(ensure_scratch(c, 3 * ld));
    CAL_HIP(c, hipMemsetAsync(c->d_scratch, 0, 3 * ld * sizeof(double), c->stream));
    double* dx = vcol(c, c->d_scratch, 0);
    double* dy = vcol(c, c->d_scratch, 1);
    double* dp = vcol(c, c->d_scratch, 2);
    CAL_HIP(c, hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (xprev) CAL_HIP(c, hipMemcpyAsync(dp, xprev, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const int np = spmv_lanczos_parts(c, dx, xprev ? dp : nullptr, dy);
    if (np <= 0) return set_error(c, CAL_ERR_UNSUPPORTED, "cal_spmv_lanczos: this matrix's SpMV kernel has no fused mode");
    CAL_TRY(ensure_partial(c, (size_t)np));
    CAL_TRY(ensure_red(c, 2));
    CAL_HIP(c, hipMemcpyAsync(c->d_red + 1, &beta2, sizeof(double), hipMemcpyHostToDevice, c->stream));
    CAL_TRY(spmv_lanczos_dev(c, dx, xprev ? dp : nullptr, xprev ? c->d_red + 1 : nullptr, dy, c->d_partial));
    CAL_HIP_OTHER(c, launch_reduce(c->d_partial, np, 1, c->d_red, c->stream));
    CAL_HIP(c, hipMemcpyAsync(y, dy, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipMemcpyAsync(dot, c->d_red, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cal_spmv_lanczos_fused(cal_ctx* c, int* fused) {
    CAL_TRY(check_ctx(c));
    if (!fused) return set_error(c, CAL_ERR_ARG, "cal_spmv_lanczos_fused: null output");
    const int64_t ld = c->A.ld;
    CAL_TRY(ensure_scratch(c, 3 * ld));
    *fused = spmv_lanczos_parts(c, vcol(c, c->d_scratch, 0), vcol(c, c->d_scratch, 2), vcol(c, c->d_scratch, 1)) > 0;
    return 0;
}

}  // extern "C"
