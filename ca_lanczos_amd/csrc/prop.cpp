// prop.cpp -- Krylov time propagation psi(t+dt) = exp(-i dt H) psi(t) on the
// CA-Lanczos basis (ca_lanczos_prop.m:3-135 as runLanczos.m:84-131 drives it).
//
// H is real symmetric and psi = u + i v complex.  Hermitian Lanczos on psi
// has real recurrence coefficients, so q_j = p_j(H) u + i p_j(H) v with real
// polynomials p_j: exactly real Lanczos on blkdiag(H, H) from the stacked
// vector [u; v].  The context's matrix is that 2n x 2n embedding
// (cal_set_matrix_csr_stacked), the state one real device vector of 2n rows
// (Re in [0, n), Im in [n, 2n)), and a time step is
//   normalise -> CA blocks ('local', lanczos_step unchanged) -> after block k
//   c = expm(-i dt T(1:ks,1:ks)) e_1 on the host and the reference's residual
//   |dt b(k) c(ks) nrm| (:122-123) -> psi <- nrm Q_c c (prop.hip, which also
//   leaves the new squared norm).
// The state, Q and the norm stay on the device across steps; the Lanczos
// run's Q / V allocation is reused, and the Newton shifts of the first step
// serve every later one (runLanczos.m:93-96 passes eigest the same way).
// A time-dependent potential H(t) = H0 + sum_k f_k(t) diag(W_k)
// (cal_prop_set_drive / cal_prop_step_driven) rewrites the matrix's stored
// diagonal in place before each step (prop.hip k_diag_density without a state,
// through runtime.cpp diag_update_dev): the step itself is unchanged.
// A nonlinear term g |psi|^2 (cal_prop_set_nonlinear; Gross-Pitaevskii) adds
// the state's density to that diagonal on the device (the same kernel with one
// state or two, through diag_density_dev, the drive in the same launch): once
// per step with the density of psi_n ("frozen", first order), or twice
// ("midpoint": a frozen step predicts psi* into a second buffer, then the step
// proper runs from psi_n under the mean of both densities; second order, two
// Krylov builds, no copy of the state).
// An absorbing mask (cal_prop_set_absorber) multiplies the state by a real
// diagonal 0 <= M <= 1 at the end of every step, inside the combine sweep
// (prop.hip's ABS flag), and records the squared norm it removes.
// Imaginary time (cal_prop_set_imaginary_time) keeps the build and the combine
// and changes the host's coefficients: c = expm(-dt (T - T(1,1) I)) e_1, real,
// scaled to the squared norm N the mode started with -- psi <- sqrt(N) exp(-dt
// H[psi]) psi / ||.||, whose fixed point is the ground state.  A real H has a
// real ground state: cal_prop_begin_real runs the same host path on H itself
// (PropState::halves = 1), the state one real vector of n rows, the combine
// and the density the REAL instantiations of k_prop_combine and k_diag_density.
// The host path is written once: combine_launch sizes, times, launches and
// reduces a filled PropCombine for combine_dev (the step's sweep and, as an
// option, the midpoint predictor's) and for combine_host (the five
// cal_prop_combine* exports, stacked and real); krylov_scaled is a build with
// its refusal and scaling; history_rows serves the four cal_prop_get_* getters.
// Every step also records [t_n, N_n, mu_n, E_n, res_n] from the first column
// of its first build's T (cal_prop_get_energetics): no kernel, no sweep.
// The one deliberate difference from ca_lanczos_prop.m: :78 projects with
// doreorth = false, the blocks here apply the library's second-pass rule
// (projectAndNormalize's 'second'), which is at least as orthogonal.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/calanczos_host.h"
#include "cal_internal.hpp"
#include "comm.hpp"
#include "dense.hpp"
#include "leja.hpp"

namespace cal {

struct PropState {
    int64_t n = 0;        // rows of H (the matrix has halves * n)
    int halves = 2;       // 2: the stacked state [Re psi; Im psi]; 1: a real state on H itself (cal_prop_begin_real)
    int s = 0, max_blocks = 0;
    bool newton = false;
    bool have_shifts = false;
    std::vector<double> shifts;  // Leja order
    double* d_psi = nullptr;     // one vector column (A.ld doubles, local origin at +lpad)
    double* d_coef = nullptr;    // a (kPropMaxCols) then b
    double* h_coef = nullptr;    // pinned; [2 kPropMaxCols] on receives the squared norm (then the observables)
    double nrm2 = 0.0;           // psi'psi
    cal_prop_info info{};
    double t = 0.0;              // the accumulated time, sum of dt over the completed steps
    // imaginary time (cal_prop_set_imaginary_time; always on with halves == 1):
    // a step is psi <- sqrt(N0) exp(-dt H) psi / ||.||
    bool imag = false;
    double N0 = 0.0;             // the squared norm every step restores: the state's when the mode went on
    std::vector<double> ehist;   // one row [t_n, N_n, mu_n, E_n, res_n] per completed step since the begin
    // observables (cal_prop_set_observables): reduced in the combine sweep
    int nw = 0, nphi = 0;
    bool energy = false;
    double* d_obs = nullptr;     // W (nw columns), phi_re (nphi), phi_im (nphi); ldo doubles each
    int64_t ldo = 0;             // even, >= n
    double* d_hpsi = nullptr;    // energy: H psi (one vector column, A.ld doubles)
    int eparts = 0;              // energy: mode 4's partials (0: SpMV + dot)
    std::vector<double> hist;    // one row of 3 + nw + 2 nphi per completed step
    // the drive H(t) = H0 + sum_k f_k(t) diag(W_k) (cal_prop_set_drive): H0's
    // diagonal as it stood when the drive was set and the nk operators, both
    // library-owned; the matrix (generation drv_gen) holds whatever the last
    // driven step wrote until the drive goes off, which puts V0 back
    int nk = 0;
    double* d_v0 = nullptr;      // n doubles (the first half's diagonal)
    double* d_drv = nullptr;     // W (nk columns of ldd doubles)
    int64_t ldd = 0;             // roundup(n, 64)
    uint64_t drv_gen = 0;
    // the absorbing mask (cal_prop_set_absorber): a library-owned copy, applied
    // by the combine sweep; one row [t, absorbed] per completed step since the set
    double* d_mask = nullptr;    // ldm doubles
    int64_t ldm = 0;             // roundup(n, 64)
    std::vector<double> ahist;
    // the nonlinear term g |psi|^2 (cal_prop_set_nonlinear): the diagonal is
    // V0 + the drive + the density of the state, rewritten by one
    // k_diag_density launch before every Krylov build.  V0 (d_v0) belongs to
    // the first of {drive, term} set and goes back when the last goes off.
    double g = 0.0;              // 0: off
    bool nl_mid = false;         // "midpoint" (two builds per step); false: "frozen"
    double* d_psi2 = nullptr;    // midpoint's predicted state (A.ld doubles, pad rows zero)
    double* h_coef2 = nullptr;   // pinned; the predictor's coefficients (2 kPropMaxCols)
    double* d_nlpart = nullptr;  // the density kernel's block shares of sum |psi_n|^4 (nl_nb), reduced by the
    int nl_nb = 0;               // step's combine (d_partial is the Lanczos blocks' in between)
    double f_last[kDriveMaxOps] = {0.0, 0.0, 0.0, 0.0};  // the amplitudes of the most recent driven step
    std::vector<double> nhist;   // one row [t_n, sum |psi_n|^4] per completed step since the set
    bool nl_on() const { return g != 0.0; }
    bool obs_on() const { return nw > 0 || nphi > 0 || energy; }
    bool abs_on() const { return d_mask != nullptr; }
    int nq() const { return nw + 2 * nphi; }
    // what a step reduces, in the order combine_dev leaves it in d_red and in
    // h_coef + 2 kPropMaxCols: [psi'psi, the nq sums, the absorbed norm
    // (absorber on), the energy (energy on)]
    int red_absorbed() const { return 1 + nq(); }
    int red_energy() const { return 1 + nq() + (abs_on() ? 1 : 0); }
    int red_count() const { return red_energy() + (energy ? 1 : 0); }
    // the most a step brings back: red_count() at its largest (the norm, nw + 2 nphi sums at their caps, the
    // absorbed norm, the energy) and the nonlinear term's sum after it -- the size of h_coef's tail
    static constexpr int kRedMax = 1 + 3 * kPropMaxObs + 1 + 1 + 1;
    double* psi(const cal_ctx* c) const { return d_psi + c->A.lpad; }
    int64_t rows() const { return halves * n; }  // of the matrix and of the state
};

namespace {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int64_t pad64(int64_t n) { return ((n + 63) / 64) * 64; }

PropObs make_obs(const double* base, int64_t ldo, int nw, int nphi) {
    PropObs o;
    o.W = base;
    o.pr = base + (size_t)nw * ldo;
    o.pi = base + (size_t)(nw + nphi) * ldo;
    o.ld = ldo;
    o.nw = nw;
    o.np = nphi;
    return o;
}

// 0 with a propagator open on c (and, need_matrix, the matrix it was begun on still set)
int active_prop(cal_ctx* c, const std::string& who, bool need_matrix) {
    if (!c || !c->prop) return set_error(c, CAL_ERR_ARG, who + ": no active propagator");
    if (need_matrix && (!c->has_A || c->A.n_local != c->prop->rows()))
        return set_error(c, CAL_ERR_ARG, who + ": the context's matrix changed since cal_prop_begin");
    return 0;
}

// k host columns of n doubles as columns of ld doubles at dst, the pad rows
// zero (src null: all zeros); on the stream
int upload_cols(cal_ctx* c, double* dst, int64_t ld, const double* src, int64_t n, int k) {
    if (k < 1) return 0;
    CAL_HIP(c, hipMemsetAsync(dst, 0, (size_t)k * ld * sizeof(double), c->stream));
    if (src)
        CAL_HIP(c, hipMemcpy2DAsync(dst, ld * sizeof(double), src, n * sizeof(double), n * sizeof(double), k,
                                    hipMemcpyHostToDevice, c->stream));
    return 0;
}

// W, phi_re and phi_im (null: zeros) as columns of ldo doubles at dst, on the stream
int upload_obs(cal_ctx* c, double* dst, int64_t ldo, int64_t n, int nw, const double* W, int nphi,
               const double* phi_re, const double* phi_im) {
    CAL_TRY(upload_cols(c, dst, ldo, W, n, nw));
    CAL_TRY(upload_cols(c, dst + (size_t)nw * ldo, ldo, phi_re, n, nphi));
    return upload_cols(c, dst + (size_t)(nw + nphi) * ldo, ldo, phi_im, n, nphi);
}

void obs_free(PropState& P) {
    if (P.d_obs) hipFree(P.d_obs);
    if (P.d_hpsi) hipFree(P.d_hpsi);
    P.d_obs = P.d_hpsi = nullptr;
    P.nw = P.nphi = P.eparts = 0;
    P.ldo = 0;
    P.energy = false;
    P.hist.clear();
}

// V0 is still the diagonal of the context's matrix underneath what was written
bool v0_current(const cal_ctx* c, const PropState& P) {
    return P.d_v0 && c->has_A && c->A_gen == P.drv_gen && c->A.n_local == P.rows();
}

// V0 + sum_k f[k] W_k (f null: V0 alone) back into the matrix V0 was taken
// from, when that matrix is still the context's; waits for it
int v0_write(cal_ctx* c, PropState& P, const double* f) {
    if (!v0_current(c, P)) return 0;
    int st = f ? diag_update_dev(c, P.d_v0, P.n, P.halves, P.nk, P.d_drv, P.ldd, f)
               : diag_update_dev(c, P.d_v0, P.n, P.halves, 0, nullptr, 0, nullptr);
    if (hipStreamSynchronize(c->stream) != hipSuccess && st == 0) st = CAL_ERR_HIP;
    return st;
}

// the propagator takes the diagonal: V0 <- the matrix's, as it is now (a V0
// taken from a matrix that is no longer the context's is dropped first)
int v0_take(cal_ctx* c, PropState& P) {
    if (P.d_v0 && !v0_current(c, P)) {
        hipFree(P.d_v0);
        P.d_v0 = nullptr;
    }
    if (P.d_v0) return 0;
    CAL_HIP(c, hipMalloc((void**)&P.d_v0, P.n * sizeof(double)));
    int st = diag_gather_dev(c, P.d_v0, P.n);
    if (st == 0 && hipStreamSynchronize(c->stream) != hipSuccess)
        st = set_error(c, CAL_ERR_HIP, "cal_prop: gathering the diagonal failed");
    if (st < 0) {
        hipFree(P.d_v0);
        P.d_v0 = nullptr;
        return st;
    }
    P.drv_gen = c->A_gen;
    return 0;
}

// the drive's operators are freed (the matrix is not touched)
void drive_free(PropState& P) {
    if (P.d_drv) hipFree(P.d_drv);
    P.d_drv = nullptr;
    P.nk = 0;
    P.ldd = 0;
    for (double& f : P.f_last) f = 0.0;
}

// the nonlinear term's buffers are freed (the matrix is not touched)
void nl_free(PropState& P) {
    if (P.d_psi2) hipFree(P.d_psi2);
    if (P.d_nlpart) hipFree(P.d_nlpart);
    if (P.h_coef2) hipHostFree(P.h_coef2);
    P.d_psi2 = P.d_nlpart = P.h_coef2 = nullptr;
    P.nl_nb = 0;
    P.g = 0.0;
    P.nl_mid = false;
    P.nhist.clear();
}

// the last of {drive, nonlinear term} went off: V0 back into the matrix, then it is freed
int v0_release(cal_ctx* c, PropState& P) {
    const int st = v0_write(c, P, nullptr);
    if (P.d_v0) hipFree(P.d_v0);
    P.d_v0 = nullptr;
    return st;
}

// everything that owns the diagonal goes off
int drive_off(cal_ctx* c, PropState& P) {
    const int st = v0_release(c, P);
    drive_free(P);
    nl_free(P);
    return st;
}

void abs_free(PropState& P) {
    if (P.d_mask) hipFree(P.d_mask);
    P.d_mask = nullptr;
    P.ldm = 0;
    P.ahist.clear();
}

void prop_free(cal_ctx* c) {
    if (!c || !c->prop) return;
    drive_off(c, *c->prop);
    obs_free(*c->prop);
    abs_free(*c->prop);
    if (c->prop->d_psi) hipFree(c->prop->d_psi);
    if (c->prop->d_coef) hipFree(c->prop->d_coef);
    if (c->prop->h_coef) hipHostFree(c->prop->h_coef);
    delete c->prop;
    c->prop = nullptr;
}

// One combine sweep from a filled PropCombine (all but its partial): sizes
// d_partial (the sweep's quantities x blocks, then `extra` doubles of the
// caller's) and d_red (nred doubles; 0: nothing is reduced), launches under the
// "apply" timer with the sweep's bytes and reduces the quantities into d_red
int combine_launch(cal_ctx* c, PropCombine& k, size_t extra, int nred) {
    const int nb = prop_combine_blocks(k.n);
    const int nk = prop_combine_quantities(k);
    CAL_TRY(ensure_partial(c, (size_t)nk * nb + extra));
    if (nred > 0) CAL_TRY(ensure_red(c, (size_t)nred));
    k.partial = c->d_partial;
    const double rows = (double)(k.real ? 1 : 2) * k.n;  // of Q's columns and of out
    const int t = timer_begin(c, 2, (rows * k.m + rows + (double)k.n * (nk - 1)) * 8.0);
    const hipError_t e = launch_prop_combine(k, c->stream);
    timer_end(c, t);
    if (e != hipSuccess) return hip_fail(c, e, "launch_prop_combine");
    if (nred > 0) CAL_HIP_OTHER(c, launch_reduce(c->d_partial, nb, nk, c->d_red, c->stream));
    return 0;
}

// psi <- Q(:, 0:m) (a + i b) and nrm2 <- psi'psi (a, b: Re / Im of nrm c, on the host);
// a real state (halves == 1): psi <- Q(:, 0:m) a through k_prop_combine's REAL flag.
// predict: the midpoint predictor's sweep, d_psi2 <- Q(:, 0:m) (a + i b) -- the
// plain sweep (no observables, no mask), nothing reduced and no host wait: the
// corrector's density launch follows it on the stream.  Its coefficients are
// staged in h_coef2: h_coef is the step proper's.
int combine_dev(cal_ctx* c, PropState& P, const double* Q, int64_t ld, int m, const double* a, const double* b,
                bool predict = false) {
    double* hc = predict ? P.h_coef2 : P.h_coef;
    std::memcpy(hc, a, m * sizeof(double));
    std::memcpy(hc + kPropMaxCols, b, m * sizeof(double));
    CAL_HIP_OTHER(c, hipMemcpyAsync(P.d_coef, hc, 2 * kPropMaxCols * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PropCombine k;
    k.Q = Q;
    k.ld = ld;
    k.n = P.n;
    k.m = m;
    k.a = P.d_coef;
    k.b = P.d_coef + kPropMaxCols;
    k.real = P.halves == 1;
    if (predict) {  // the provisional state's norm is not used
        k.out = P.d_psi2 + c->A.lpad;
        return combine_launch(c, k, 0, 0);
    }
    k.out = P.psi(c);
    k.obs = make_obs(P.d_obs, P.ldo, P.nw, P.nphi);
    k.mask = P.d_mask;
    k.ldm = P.ldm;
    const int nd = dot_blocks(P.rows());
    // the energy's partials follow the combine's
    const size_t pe = (size_t)prop_combine_quantities(k) * prop_combine_blocks(P.n);
    const int nred = P.red_count() + (P.nl_on() ? 1 : 0);  // the nonlinear term's sum |psi_n|^4 comes last
    CAL_TRY(combine_launch(c, k, P.energy ? (size_t)std::max(P.eparts, nd) : 0, nred));
    if (P.nl_on()) CAL_HIP_OTHER(c, launch_reduce(P.d_nlpart, P.nl_nb, 1, c->d_red + P.red_count(), c->stream));
    if (P.energy) {
        // <psi'|H|psi'> = y'x over the stacked rows, y = blkdiag(H, H) x: the
        // fused Lanczos mode's dot, reduced as lanczos_std.cpp reduces it
        double* y = P.d_hpsi + c->A.lpad;
        double* part = c->d_partial + pe;
        if (P.eparts > 0) {
            CAL_TRY(spmv_lanczos_dev(c, P.psi(c), nullptr, nullptr, y, part));
            CAL_HIP_OTHER(c, launch_reduce(part, P.eparts, 1, c->d_red + P.red_energy(), c->stream));
        } else {
            CAL_TRY(spmv_dev(c, P.psi(c), y, 0, 0.0, 0.0, nullptr));
            CAL_HIP_OTHER(c, launch_dot(y, P.psi(c), P.rows(), part, nd, c->stream));
            CAL_HIP_OTHER(c, launch_reduce(part, nd, 1, c->d_red + P.red_energy(), c->stream));
        }
    }
    // everything reduced comes back with the squared norm in the one pinned transfer
    double* h = P.h_coef + 2 * kPropMaxCols;
    CAL_HIP_OTHER(c, hipMemcpyAsync(h, c->d_red, (size_t)nred * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    P.nrm2 = h[0];
    return 0;
}

// the diagonal <- V0 + sum_k f[k] W_k + ga |psi_n|^2 (+ gb |B|^2), one launch;
// the blocks' shares of sum |psi_n|^4 stay in d_nlpart for the step's combine
int density_dev(cal_ctx* c, PropState& P, const double* f, double ga, const double* B, double gb) {
    return diag_density_dev(c, P.d_v0, P.n, P.halves, P.nk, P.d_drv, P.ldd, f, P.psi(c), ga, B, gb, P.d_nlpart);
}

// the history row of the step just completed (combine_dev's transfer is in h_coef)
void record_row(PropState& P) {
    const double* h = P.h_coef + 2 * kPropMaxCols;
    P.hist.push_back(P.t);
    P.hist.push_back(h[0]);
    P.hist.push_back(P.energy ? h[P.red_energy()] : std::numeric_limits<double>::quiet_NaN());
    P.hist.insert(P.hist.end(), h + 1, h + 1 + P.nq());
}

// the absorber's row [t, absorbed] of the step just completed
void record_absorbed(PropState& P) {
    P.ahist.push_back(P.t);
    P.ahist.push_back(P.h_coef[2 * kPropMaxCols + P.red_absorbed()]);
}

// One Krylov build from the current state: CA blocks until max_blocks, the
// adaptive stop or a dropped block.  *kuse blocks are usable (0: the first
// block broke down); cre / cim: expm(-i dt T(1:ks,1:ks)) e_1 for ks = s kuse,
// and *scale = nrm: the new state is Q (scale (cre + i cim)).
// Imaginary time: cre = expm(-dt (T - T(1,1) I)) e_1 (real), cim = 0, *scale =
// sqrt(N0) / ||cre||_2 (the sum of squares in ascending order) -- the new state
// has the squared norm N0 -- and the residual is |dt b(k) c(ks)| *scale.
// en non-null: en[0] = T(1,1) = <psi|H|psi>/<psi|psi> and en[1] = ||T(2:ks,1)||_2,
// the eigen-residual of the start state (Q(:,1) is psi / ||psi||).
int krylov(cal_ctx* c, PropState& P, double dt, double tol, int adaptive, int* kuse, std::vector<double>& cre,
           std::vector<double>& cim, double* resid, double* scale, double* en) {
    const int s = P.s;
    const double nrm = std::sqrt(P.nrm2);
    *scale = nrm;
    LanczosBegin in;
    in.r_dev = P.psi(c);
    in.rr = P.nrm2;
    in.prologue_cgs = false;  // lanczos(A,r0,2*s,'local') (ca_lanczos_prop.m:33)
    in.reuse = true;
    if (P.newton && P.have_shifts) {
        in.shifts = P.shifts.data();
        in.nshifts = (int)P.shifts.size();
    }
    CAL_TRY(lanczos_begin(c, in, s, P.max_blocks, P.newton ? "newton" : "monomial", "local"));
    if (P.newton && !P.have_shifts) {  // the prologue's shifts serve every later step
        const LanczosView v = lanczos_view(c);
        P.shifts.assign(v.shifts, v.shifts + std::min(2 * s, 64));
        P.have_shifts = true;
    }
    *kuse = 0;
    std::vector<double> tre((size_t)s * P.max_blocks), tim((size_t)s * P.max_blocks);
    for (int k = 1; k <= P.max_blocks; ++k) {
        const int rd0 = lanczos_view(c).n_rank_deficient;
        const int st = lanczos_step(c, 0);
        if (st < 0) return st;
        const LanczosView v = lanczos_view(c);
        if (st == CAL_WARN_BREAKDOWN) {  // rho_t == 0 or a non-finite T: the block is dropped
            P.info.breakdowns++;
            break;
        }
        // normalize's 'Rank deficient' (svd(R) against 1e-8 s_1): the reference
        // displays it and goes on (normalize.m:21-27), and so does this loop --
        // a smooth state's first block is flagged routinely (the oscillator's
        // Krylov basis has kappa > 1e8) while its T still propagates within
        // the bar; the residual below judges the block
        P.info.rank_deficient += v.n_rank_deficient - rd0;
        const int ks = k * s;
        double r = std::numeric_limits<double>::quiet_NaN();
        double sc = nrm;
        if (P.imag) {
            if (dense::expm_real_col1(ks, v.T, v.ldt, dt, tre.data())) {
                double cc = 0.0;
                for (int j = 0; j < ks; ++j) {
                    cc = cc + tre[j] * tre[j];
                    tim[j] = 0.0;
                }
                sc = std::sqrt(P.N0) / std::sqrt(cc);
                r = std::fabs(dt * v.b[k - 1] * tre[ks - 1]) * sc;
            }
        } else if (dense::expm_col1(ks, v.T, v.ldt, dt, tre.data(), tim.data())) {
            r = std::fabs(dt * v.b[k - 1] * nrm) * std::hypot(tre[ks - 1], tim[ks - 1]);  // :123
        }
        if (!std::isfinite(r)) {  // a non-finite T: the block is dropped like a breakdown
            P.info.breakdowns++;
            break;
        }
        *kuse = k;
        *resid = r;
        *scale = sc;
        if (en) {
            double rr = 0.0;
            for (int i = 1; i < ks; ++i) rr = rr + v.T[i] * v.T[i];
            en[0] = v.T[0];
            en[1] = std::sqrt(rr);
        }
        cre.assign(tre.begin(), tre.begin() + ks);
        cim.assign(tim.begin(), tim.begin() + ks);
        if (adaptive && r < tol && ks >= 3) break;  // :124
    }
    return 0;
}

// krylov with what every caller does next: no usable block is refused with
// CAL_WARN_BREAKDOWN under the caller's message (the state is unchanged);
// otherwise *ks = s kuse and cre / cim are scaled to the combine's
// coefficients, nrm c (imaginary time: sqrt(N0) c / ||c||)
int krylov_scaled(cal_ctx* c, PropState& P, double dt, double tol, int adaptive, const std::string& broke, int* ks,
                  std::vector<double>& cre, std::vector<double>& cim, double* resid, double* en) {
    int kuse = 0;
    double scale = 0.0;
    CAL_TRY(krylov(c, P, dt, tol, adaptive, &kuse, cre, cim, resid, &scale, en));
    if (kuse == 0) return set_error(c, CAL_WARN_BREAKDOWN, broke);
    *ks = kuse * P.s;
    for (int j = 0; j < *ks; ++j) {
        cre[j] = scale * cre[j];
        cim[j] = scale * cim[j];
    }
    return 0;
}

int check_prop_args(cal_ctx* c, int64_t n, int halves, int s, int max_blocks, const char* basis, bool* newton) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    if (!c->has_A) return set_error(c, CAL_ERR_NOMATRIX, "no matrix set on the context");
    if (halves == 1) {
        // the real-state path runs on H itself: what only the stacked propagator takes is refused
        if (c->comm && c->comm->nranks > 1)
            return set_error(c, CAL_ERR_UNSUPPORTED, "cal_prop_begin_real: the real-state path runs on one rank, as "
                                                     "the stacked propagator (cal_prop_begin) does");
        if (c->A.herm)
            return set_error(c, CAL_ERR_UNSUPPORTED, "cal_prop_begin_real: a complex Hermitian matrix has a complex "
                                                     "ground state; use the stacked propagator (cal_prop_begin) "
                                                     "with cal_prop_set_imaginary_time");
        if (c->A.shared)
            return set_error(c, CAL_ERR_UNSUPPORTED, "cal_prop_begin_real: a \"shared\" matrix is blkdiag(H, H); set H "
                                                     "itself (cal_set_matrix_csr) or use the stacked propagator "
                                                     "(cal_prop_begin) with cal_prop_set_imaginary_time");
        if (n >= 1 && c->A.n_local == 2 * n)
            return set_error(c, CAL_ERR_UNSUPPORTED, "cal_prop_begin_real: the matrix has 2n rows, a stacked matrix; "
                                                     "set H itself (cal_set_matrix_csr) or use the stacked "
                                                     "propagator (cal_prop_begin) with cal_prop_set_imaginary_time");
        if (n < 1 || c->A.n_local != n)
            return set_error(c, CAL_ERR_ARG, "cal_prop_begin_real: the matrix must have n rows (cal_set_matrix_csr)");
    } else {
        if (c->comm && c->comm->nranks > 1)
            return set_error(c, CAL_ERR_UNSUPPORTED, "time propagation runs on one rank");
        if (n < 1 || c->A.n_local != 2 * n)
            return set_error(c, CAL_ERR_ARG, "cal_prop: the matrix must have 2n rows (cal_set_matrix_csr_stacked)");
    }
    if (s < 1 || s > 31 || max_blocks < 1 || (int64_t)s * max_blocks > kPropMaxCols)
        return set_error(c, CAL_ERR_ARG, "cal_prop: need 1 <= s <= 31 and s*max_blocks <= 512");
    std::string b = basis ? basis : "";
    for (auto& ch : b) ch = (char)tolower(ch);
    if (b != "monomial" && b != "newton") return set_error(c, CAL_ERR_ARG, "ERROR: Unknown basis type: " + b);
    *newton = b == "newton";
    return 0;
}

bool combine_args_ok(int64_t n, int m, const double* Q, const double* c_re, const double* c_im, const double* out_re,
                     const double* out_im) {
    return n >= 1 && m >= 1 && m <= kPropMaxCols && Q && c_re && c_im && out_re && out_im;
}

bool obs_counts_ok(int nw, const double* W, int nphi, const double* phi_re) {
    return nw >= 0 && nw <= kPropMaxObs && nphi >= 0 && nphi <= kPropMaxObs && (nw == 0 || W) && (nphi == 0 || phi_re);
}

// every value finite and in [0, 1] (NaN fails both comparisons)
bool mask_ok(const double* mask, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!(mask[i] >= 0.0 && mask[i] <= 1.0)) return false;
    return true;
}

// The combine sweep on host data, behind the cal_prop_combine* exports (which
// check the arguments): halves = 2 the stacked sweep (Q of 2n rows, c_re +
// i c_im), halves = 1 the real state's (Q of n rows, c_re alone; no mask, no
// reference states); mask null for none, nw = nphi = 0 for no observables.
// Q has the host leading dimension ldq >= halves n.  ldq == halves n: the
// device copy takes the library's own padded leading dimension (a multiple of
// 64: the 16-byte path, and the stacked lower half misaligned exactly when n is
// odd).  ldq > halves n: the copy keeps ldq, so an odd ldq runs the 8-byte path.
// d_scratch holds [out (ldv) | W and phi (ldo x nq) | the mask (ldo, when
// given) | the coefficients (halves m, rounded up to even) | Q (ld x m)], ldv
// and ldo multiples of 64: every origin is 16-byte aligned.
int combine_host(cal_ctx* c, int64_t n, int halves, int m, const double* Q, int64_t ldq, const double* c_re,
                 const double* c_im, const double* mask, int nw, const double* W, int nphi, const double* phi_re,
                 const double* phi_im, double* out_re, double* out_im, double* norm2, double* absorbed, double* sums) {
    const int nq = nw + 2 * nphi, na = mask ? 1 : 0;
    const int64_t rows = halves * n, ldv = pad64(rows), ldo = pad64(n), ld = ldq == rows ? ldv : ldq;
    const size_t mc = (size_t)halves * m + (halves * m & 1);
    CAL_TRY(ensure_scratch(c, (size_t)ldv + (size_t)ldo * (nq + na) + mc + (size_t)ld * m));
    double* dout = c->d_scratch;
    double* dobs = dout + ldv;
    double* dmask = dobs + (size_t)ldo * nq;
    double* dco = dmask + (size_t)ldo * na;
    double* dq = dco + mc;
    PropCombine k;
    k.Q = dq;
    k.ld = ld;
    k.n = n;
    k.m = m;
    k.a = dco;
    k.b = dco + m;
    k.out = dout;
    k.obs = make_obs(dobs, ldo, nw, nphi);
    k.mask = mask ? dmask : nullptr;
    k.ldm = ldo;
    k.real = halves == 1;
    CAL_HIP(c, hipMemcpy2DAsync(dq, ld * sizeof(double), Q, ldq * sizeof(double), rows * sizeof(double), m,
                                hipMemcpyHostToDevice, c->stream));
    CAL_HIP(c, hipMemcpyAsync(dco, c_re, m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (halves == 2) CAL_HIP(c, hipMemcpyAsync(dco + m, c_im, m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (mask) CAL_HIP(c, hipMemcpyAsync(dmask, mask, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CAL_TRY(upload_obs(c, dobs, ldo, n, nw, W, nphi, phi_re, phi_im));
    const int nk = prop_combine_quantities(k);
    CAL_TRY(combine_launch(c, k, 0, nk));
    CAL_HIP(c, hipMemcpyAsync(out_re, dout, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (halves == 2) CAL_HIP(c, hipMemcpyAsync(out_im, dout + n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    double red[2 + 3 * kPropMaxObs] = {0.0};
    CAL_HIP(c, hipMemcpyAsync(red, c->d_red, (size_t)nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    if (norm2) *norm2 = red[0];
    for (int q = 0; q < nq; ++q) sums[q] = red[1 + q];
    if (mask && absorbed) *absorbed = red[1 + nq];
    return 0;
}

// rows [first, first + count) of a per-step history of nc columns, behind the
// four cal_prop_get_* exports; out null: the row count alone
int history_rows(cal_ctx* c, const std::string& who, const std::vector<double>& hist, int nc, int64_t first,
                 int64_t count, double* out, int64_t* nrows) {
    const int64_t nr = (int64_t)(hist.size() / nc);
    if (nrows) *nrows = nr;
    if (!out) return 0;
    if (first < 0 || count < 0 || first + count > nr)
        return set_error(c, CAL_ERR_ARG, who + ": rows [first, first + count) out of range");
    std::memcpy(out, hist.data() + (size_t)first * nc, (size_t)count * nc * sizeof(double));
    return 0;
}

}  // namespace
}  // namespace cal

using namespace cal;

extern "C" {

void cal_prop_free_state(cal_ctx* c) { prop_free(c); }

int cal_set_matrix_csr_stacked(cal_ctx* c, int64_t n, const int64_t* rowptr, const int32_t* colind,
                               const double* val) {
    if (!c || n < 0 || !rowptr || (n > 0 && rowptr[n] > 0 && (!colind || !val)))
        return set_error(c, CAL_ERR_ARG, "cal_set_matrix_csr_stacked: bad arguments");
    const int64_t nnz = rowptr[n];
    if (c->spmv_format == 4) {
        // the "shared" format: H alone goes up, nothing doubled on the host
        if (c->comm && c->comm->nranks > 1)
            return set_error(c, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_stacked: the \"shared\" format runs on one "
                                                     "rank (the context has a communicator of several ranks)");
        if (nnz < 0 || nnz >= ((int64_t)1 << 31) || 2 * n >= ((int64_t)1 << 31))
            return set_error(c, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_stacked: 2n and nnz(H) must be < 2^31");
        if (n < 1) return set_error(c, CAL_ERR_ARG, "cal_set_matrix_csr_stacked: the \"shared\" format needs n >= 1");
        hipSetDevice(c->device);
        std::vector<int> rp(n + 1), col(nnz);
        for (int64_t i = 0; i <= n; ++i) rp[i] = (int)rowptr[i];
        for (int64_t i = 0; i < n; ++i)
            if (rp[i + 1] < rp[i]) return set_error(c, CAL_ERR_ARG, "row pointers must be non-decreasing");
        if (rp[0] != 0) return set_error(c, CAL_ERR_ARG, "row pointers must start at 0");
        for (int64_t p = 0; p < nnz; ++p) {
            if (colind[p] < 0 || colind[p] >= n) return set_error(c, CAL_ERR_ARG, "column index out of range");
            col[p] = colind[p];
        }
        return upload_matrix_shared(c, n, rp, col, val);
    }
    if (nnz < 0 || 2 * nnz >= ((int64_t)1 << 31) || 2 * n >= ((int64_t)1 << 31))
        return set_error(c, CAL_ERR_UNSUPPORTED, "n and nnz must be < 2^31 per rank");
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return set_error(c, CAL_ERR_ARG, "row pointers must be non-decreasing");
    std::vector<int64_t> rp(2 * n + 1);
    std::vector<int32_t> col(2 * nnz);
    std::vector<double> v(2 * nnz);
    for (int64_t i = 0; i <= n; ++i) rp[i] = rowptr[i];
    for (int64_t i = 1; i <= n; ++i) rp[n + i] = nnz + rowptr[i];
    for (int64_t p = 0; p < nnz; ++p) {
        if (colind[p] < 0 || colind[p] >= n) return set_error(c, CAL_ERR_ARG, "column index out of range");
        col[p] = colind[p];
        col[nnz + p] = (int32_t)(colind[p] + n);
        v[p] = val[p];
        v[nnz + p] = val[p];
    }
    return cal_set_matrix_csr(c, 2 * n, rp.data(), col.data(), v.data());
}

// E(H) = [[A, -B], [B, A]] for the complex Hermitian H = A + iB (val_re, val_im):
// the real symmetric matrix whose SpMV on [Re psi; Im psi] is [Re H psi; Im H psi].
int cal_set_matrix_csr_hermitian(cal_ctx* c, int64_t n, const int64_t* rowptr, const int32_t* colind,
                                 const double* val_re, const double* val_im) {
    // a real H: blkdiag(H, H), cal_set_matrix_csr_stacked's own path and bits
    if (!val_im) return cal_set_matrix_csr_stacked(c, n, rowptr, colind, val_re);
    if (!c || n < 0 || !rowptr || (n > 0 && rowptr[n] > 0 && (!colind || !val_re)))
        return set_error(c, CAL_ERR_ARG, "cal_set_matrix_csr_hermitian: bad arguments");
    const int64_t nnz = rowptr[n];
    const bool shared = c->spmv_format == 4;
    if (shared && c->comm && c->comm->nranks > 1)
        return set_error(c, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_hermitian: the \"shared\" format runs on one "
                                                 "rank (the context has a communicator of several ranks)");
    if (shared && (nnz < 0 || nnz >= ((int64_t)1 << 31) || 2 * n >= ((int64_t)1 << 31)))
        return set_error(c, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_hermitian: 2n and nnz(H) must be < 2^31");
    if (!shared && (nnz < 0 || 4 * nnz >= ((int64_t)1 << 31) || 2 * n >= ((int64_t)1 << 31)))
        return set_error(c, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_hermitian: 2n and 4 nnz(H) must be < 2^31 "
                                                 "(the embedding [[A, -B], [B, A]] stores every nonzero four times)");
    if (shared && n < 1)
        return set_error(c, CAL_ERR_ARG, "cal_set_matrix_csr_hermitian: the \"shared\" format needs n >= 1");
    if (rowptr[0] != 0) return set_error(c, CAL_ERR_ARG, "row pointers must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return set_error(c, CAL_ERR_ARG, "row pointers must be non-decreasing");
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            if (colind[p] < 0 || colind[p] >= n) return set_error(c, CAL_ERR_ARG, "column index out of range");
            if (colind[p] == i && val_im[p] != 0.0)  // NaN too
                return set_error(c, CAL_ERR_ARG, "cal_set_matrix_csr_hermitian: the diagonal of a Hermitian matrix is "
                                                 "real (a stored diagonal entry has a non-zero imaginary part)");
        }
    if (shared) {
        // H alone goes up: rowptr / col / val as for blkdiag(H, H), plus the imaginary parts
        hipSetDevice(c->device);
        std::vector<int> rp(n + 1), col(colind, colind + nnz);
        for (int64_t i = 0; i <= n; ++i) rp[i] = (int)rowptr[i];
        return upload_matrix_shared(c, n, rp, col, val_re, val_im);
    }
    // any other format: the embedding on the host, explicit zeros kept (the
    // pattern does not depend on the values).  Top row i: (c, a) in stored
    // order, then (n + c, -b); bottom row n + i: (c, b), then (n + c, a).
    std::vector<int64_t> rp(2 * n + 1);
    std::vector<int32_t> col(4 * nnz);
    std::vector<double> v(4 * nnz);
    rp[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t p0 = rowptr[i], k = rowptr[i + 1] - p0, t = 2 * p0, b = 2 * nnz + 2 * p0;
        rp[i + 1] = t + 2 * k;
        rp[n + i + 1] = b + 2 * k;
        for (int64_t j = 0; j < k; ++j) {
            const int32_t cj = colind[p0 + j];
            const double ar = val_re[p0 + j], bi = val_im[p0 + j];
            col[t + j] = cj;
            v[t + j] = ar;
            col[t + k + j] = (int32_t)(cj + n);
            v[t + k + j] = -bi;
            col[b + j] = cj;
            v[b + j] = bi;
            col[b + k + j] = (int32_t)(cj + n);
            v[b + k + j] = ar;
        }
    }
    return cal_set_matrix_csr(c, 2 * n, rp.data(), col.data(), v.data());
}

int cal_prop_combine(cal_ctx* c, int64_t n, int m, const double* Q, const double* c_re, const double* c_im,
                     double* out_re, double* out_im, double* norm2) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    if (!combine_args_ok(n, m, Q, c_re, c_im, out_re, out_im))
        return set_error(c, CAL_ERR_ARG, "cal_prop_combine: need n >= 1, 1 <= m <= 512 and non-null arrays");
    return combine_host(c, n, 2, m, Q, 2 * n, c_re, c_im, nullptr, 0, nullptr, 0, nullptr, nullptr, out_re, out_im,
                        norm2, nullptr, nullptr);
}

int cal_prop_combine_obs(cal_ctx* c, int64_t n, int m, const double* Q, const double* c_re, const double* c_im,
                         int nw, const double* W, int nphi, const double* phi_re, const double* phi_im,
                         double* out_re, double* out_im, double* norm2, double* sums) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    if (!combine_args_ok(n, m, Q, c_re, c_im, out_re, out_im))
        return set_error(c, CAL_ERR_ARG, "cal_prop_combine_obs: need n >= 1, 1 <= m <= 512 and non-null arrays");
    if (!obs_counts_ok(nw, W, nphi, phi_re) || (nw + 2 * nphi > 0 && !sums))
        return set_error(c, CAL_ERR_ARG, "cal_prop_combine_obs: need 0 <= nw, nphi <= 4 with their arrays and sums");
    return combine_host(c, n, 2, m, Q, 2 * n, c_re, c_im, nullptr, nw, W, nphi, phi_re, phi_im, out_re, out_im, norm2,
                        nullptr, sums);
}

int cal_prop_combine_real_ld(cal_ctx* c, int64_t n, int m, const double* Q, int64_t ldq, const double* a, int nw,
                             const double* W, double* out, double* norm2, double* sums) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    if (n < 1 || m < 1 || m > kPropMaxCols || !Q || ldq < n || !a || !out)
        return set_error(c, CAL_ERR_ARG,
                         "cal_prop_combine_real: need n >= 1, 1 <= m <= 512, ldq >= n and non-null arrays");
    if (nw < 0 || nw > kPropMaxObs || (nw > 0 && (!W || !sums)))
        return set_error(c, CAL_ERR_ARG, "cal_prop_combine_real: need 0 <= nw <= 4 with W and sums");
    return combine_host(c, n, 1, m, Q, ldq, a, nullptr, nullptr, nw, W, 0, nullptr, nullptr, out, nullptr, norm2,
                        nullptr, sums);
}

int cal_prop_combine_real(cal_ctx* c, int64_t n, int m, const double* Q, const double* a, int nw, const double* W,
                          double* out, double* norm2, double* sums) {
    return cal_prop_combine_real_ld(c, n, m, Q, n, a, nw, W, out, norm2, sums);
}

int cal_prop_set_observables(cal_ctx* c, int nw, const double* W, int nphi, const double* phi_re, const double* phi_im,
                             int energy) {
    CAL_TRY(active_prop(c, "cal_prop_set_observables", true));
    hipSetDevice(c->device);
    PropState& P = *c->prop;
    if (!obs_counts_ok(nw, W, nphi, phi_re))
        return set_error(c, CAL_ERR_ARG, "cal_prop_set_observables: need 0 <= nw, nphi <= 4 with their arrays");
    if (P.halves == 1 && nphi > 0)
        return set_error(c, CAL_ERR_UNSUPPORTED, "cal_prop_set_observables: a real-state propagator "
                                                 "(cal_prop_begin_real) takes W and energy only; reference states "
                                                 "need the stacked propagator (cal_prop_begin)");
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    obs_free(P);
    const int nq = nw + 2 * nphi;
    if (nq > 0) {
        P.ldo = pad64(P.n);
        CAL_HIP(c, hipMalloc((void**)&P.d_obs, (size_t)nq * P.ldo * sizeof(double)));
        const int st = upload_obs(c, P.d_obs, P.ldo, P.n, nw, W, nphi, phi_re, phi_im);
        if (st < 0 || hipStreamSynchronize(c->stream) != hipSuccess) {  // the sources are the caller's
            obs_free(P);
            return st < 0 ? st : set_error(c, CAL_ERR_HIP, "cal_prop_set_observables: upload failed");
        }
    }
    if (energy) {
        const int64_t ld = c->A.ld;
        CAL_HIP(c, hipMalloc((void**)&P.d_hpsi, ld * sizeof(double)));
        CAL_HIP(c, hipMemsetAsync(P.d_hpsi, 0, ld * sizeof(double), c->stream));
        P.eparts = spmv_lanczos_parts(c, P.psi(c), nullptr, P.d_hpsi + c->A.lpad);
    }
    P.nw = nw;
    P.nphi = nphi;
    P.energy = energy != 0;
    return 0;
}

int cal_prop_get_observables(cal_ctx* c, int64_t first, int64_t count, double* out, int64_t* nrows, int* ncols) {
    CAL_TRY(active_prop(c, "cal_prop_get_observables", false));
    const int nc = 3 + c->prop->nq();
    if (ncols) *ncols = nc;
    return history_rows(c, "cal_prop_get_observables", c->prop->hist, nc, first, count, out, nrows);
}

int cal_prop_combine_masked(cal_ctx* c, int64_t n, int m, const double* Q, const double* c_re, const double* c_im,
                            const double* mask, int nw, const double* W, int nphi, const double* phi_re,
                            const double* phi_im, double* out_re, double* out_im, double* norm2, double* absorbed,
                            double* sums) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    if (!combine_args_ok(n, m, Q, c_re, c_im, out_re, out_im) || !mask)
        return set_error(c, CAL_ERR_ARG, "cal_prop_combine_masked: need n >= 1, 1 <= m <= 512 and non-null arrays");
    if (!obs_counts_ok(nw, W, nphi, phi_re) || (nw + 2 * nphi > 0 && !sums))
        return set_error(c, CAL_ERR_ARG,
                         "cal_prop_combine_masked: need 0 <= nw, nphi <= 4 with their arrays and sums");
    if (!mask_ok(mask, n))
        return set_error(c, CAL_ERR_ARG, "cal_prop_combine_masked: the mask must be finite and within [0, 1]");
    return combine_host(c, n, 2, m, Q, 2 * n, c_re, c_im, mask, nw, W, nphi, phi_re, phi_im, out_re, out_im, norm2,
                        absorbed, sums);
}

int cal_prop_set_absorber(cal_ctx* c, const double* mask) {
    CAL_TRY(active_prop(c, "cal_prop_set_absorber", false));
    hipSetDevice(c->device);
    PropState& P = *c->prop;
    if (P.halves == 1)
        return set_error(c, CAL_ERR_UNSUPPORTED, "cal_prop_set_absorber: a real-state propagator "
                                                 "(cal_prop_begin_real) takes no absorber; use the stacked "
                                                 "propagator (cal_prop_begin)");
    if (mask && !mask_ok(mask, P.n))
        return set_error(c, CAL_ERR_ARG, "cal_prop_set_absorber: the mask must be finite and within [0, 1]");
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    if (!mask) {
        abs_free(P);
        return 0;
    }
    // the new copy first: a failure leaves an earlier absorber as it was
    const int64_t ldm = pad64(P.n);
    double* d = nullptr;
    CAL_HIP(c, hipMalloc((void**)&d, ldm * sizeof(double)));
    if (upload_cols(c, d, ldm, mask, P.n, 1) < 0 ||
        hipStreamSynchronize(c->stream) != hipSuccess) {  // the source is the caller's
        hipFree(d);
        return set_error(c, CAL_ERR_HIP, "cal_prop_set_absorber: upload failed");
    }
    abs_free(P);
    P.d_mask = d;
    P.ldm = ldm;
    return 0;
}

int cal_prop_get_absorbed(cal_ctx* c, int64_t first, int64_t count, double* out, int64_t* nrows) {
    CAL_TRY(active_prop(c, "cal_prop_get_absorbed", false));
    return history_rows(c, "cal_prop_get_absorbed", c->prop->ahist, 2, first, count, out, nrows);
}

// halves = 1: the real-state path (psi_im unused)
static int prop_begin(cal_ctx* c, int64_t n, int halves, const double* psi_re, const double* psi_im, int s,
                      int max_blocks, const char* basis, const double* eigest, int neig) {
    bool newton = false;
    CAL_TRY(check_prop_args(c, n, halves, s, max_blocks, basis, &newton));
    if (!psi_re || neig < 0 || (neig > 0 && !eigest))
        return set_error(c, CAL_ERR_ARG, "cal_prop_begin: need psi_re (and eigest when neig > 0)");
    prop_free(c);
    PropState* P = new PropState();
    c->prop = P;
    P->n = n;
    P->halves = halves;
    P->s = s;
    P->max_blocks = max_blocks;
    P->newton = newton;
    if (newton && neig > 0) {
        // basis_shifts = leja(real(eigest)) (ca_lanczos_prop.m:38-40)
        if (neig < s) return set_error(c, CAL_ERR_ARG, "cal_prop_begin: fewer than s eigenvalue estimates");
        std::vector<std::complex<double>> x(neig), y;
        for (int i = 0; i < neig; ++i) {
            if (!std::isfinite(eigest[i])) return set_error(c, CAL_ERR_ARG, "cal_prop_begin: non-finite eigest");
            x[i] = std::complex<double>(eigest[i], 0.0);
        }
        std::vector<int> oi;
        std::string err;
        if (leja::real_leja(x, y, oi, err) != 0) return set_error(c, CAL_ERR_NUMERIC, "leja: " + err);
        if ((int)y.size() < s) return set_error(c, CAL_ERR_ARG, "cal_prop_begin: fewer than s distinct estimates");
        for (const auto& v : y) P->shifts.push_back(v.real());
        P->have_shifts = true;
    }
    const int64_t ld = c->A.ld;
    CAL_HIP(c, hipMalloc((void**)&P->d_psi, ld * sizeof(double)));
    CAL_HIP(c, hipMalloc((void**)&P->d_coef, 2 * kPropMaxCols * sizeof(double)));
    CAL_HIP(c, hipHostMalloc((void**)&P->h_coef, (2 * kPropMaxCols + PropState::kRedMax) * sizeof(double),
                             hipHostMallocDefault));
    std::memset(P->h_coef, 0, (2 * kPropMaxCols + PropState::kRedMax) * sizeof(double));
    CAL_HIP(c, hipMemsetAsync(P->d_psi, 0, ld * sizeof(double), c->stream));
    CAL_HIP(c, hipMemcpyAsync(P->psi(c), psi_re, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (psi_im && halves == 2)
        CAL_HIP(c, hipMemcpyAsync(P->psi(c) + n, psi_im, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // the first norm: one sweep; every later one comes out of the combine
    const int nb = dot_blocks(P->rows());
    CAL_TRY(ensure_partial(c, nb));
    CAL_TRY(ensure_red(c, 1));
    CAL_HIP_OTHER(c, launch_dot(P->psi(c), P->psi(c), P->rows(), c->d_partial, nb, c->stream));
    CAL_HIP_OTHER(c, launch_reduce(c->d_partial, nb, 1, c->d_red, c->stream));
    CAL_HIP(c, hipMemcpyAsync(P->h_coef + 2 * kPropMaxCols, c->d_red, sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    P->nrm2 = P->h_coef[2 * kPropMaxCols];
    if (!(P->nrm2 > 0.0) || !std::isfinite(P->nrm2))
        return set_error(c, CAL_ERR_ARG, "cal_prop_begin: the start state must be finite and non-zero");
    P->info.norm = std::sqrt(P->nrm2);
    if (halves == 1) {  // imaginary time from the start: N = psi'psi
        P->imag = true;
        P->N0 = P->nrm2;
    }
    return 0;
}

int cal_prop_begin(cal_ctx* c, int64_t n, const double* psi_re, const double* psi_im, int s, int max_blocks,
                   const char* basis, const double* eigest, int neig) {
    const int st = prop_begin(c, n, 2, psi_re, psi_im, s, max_blocks, basis, eigest, neig);
    if (st < 0 && c) prop_free(c);  // no half-built propagator is left behind
    return st;
}

int cal_prop_begin_real(cal_ctx* c, int64_t n, const double* psi, int s, int max_blocks, const char* basis,
                        const double* eigest, int neig) {
    // a refusal of the matrix leaves an open propagator as it was (prop_begin frees it only after the checks)
    const bool had = c && c->prop;
    const int st = prop_begin(c, n, 1, psi, nullptr, s, max_blocks, basis, eigest, neig);
    if (st < 0 && c && c->prop && !(had && st == CAL_ERR_UNSUPPORTED)) prop_free(c);
    return st;
}

int cal_prop_set_imaginary_time(cal_ctx* c, int on) {
    CAL_TRY(active_prop(c, "cal_prop_set_imaginary_time", false));
    PropState& P = *c->prop;
    if (!on && P.halves == 1)
        return set_error(c, CAL_ERR_UNSUPPORTED, "cal_prop_set_imaginary_time: a real-state propagator "
                                                 "(cal_prop_begin_real) steps in imaginary time only; real time "
                                                 "needs the stacked propagator (cal_prop_begin)");
    if (on && !P.imag) P.N0 = P.nrm2;  // the squared norm every later step restores
    P.imag = on != 0;
    return 0;
}

int cal_prop_get_energetics(cal_ctx* c, int64_t first, int64_t count, double* out, int64_t* nrows) {
    if (!c) return CAL_ERR_ARG;
    CAL_TRY(active_prop(c, "cal_prop_get_energetics", false));
    return history_rows(c, "cal_prop_get_energetics", c->prop->ehist, 5, first, count, out, nrows);
}

// nsteps time steps; f non-null: before step `it` the diagonal is set to
// V0 + sum_k f[it ldf + k] W_k (one k_diag_density launch without a state,
// enqueued ahead of the step's first kernel on the same stream).  With a
// nonlinear term on, that launch takes the state too (the drive and g |psi|^2
// together, once per Krylov build: twice per step under "midpoint"), and it
// runs for f null too, with the amplitudes of the most recent driven step
// (f_last; zeros before the first)
static int prop_steps(cal_ctx* c, const char* who, double dt, double tol, int adaptive, int nsteps, const double* f,
                      int ldf) {
    const std::string w = who;
    CAL_TRY(active_prop(c, w, true));
    hipSetDevice(c->device);
    PropState& P = *c->prop;
    if (!std::isfinite(dt) || nsteps < 0 || std::isnan(tol))
        return set_error(c, CAL_ERR_ARG, w + ": need a finite dt, a tol and nsteps >= 0");
    if (f) {
        if (P.nk < 1 || !P.d_v0) return set_error(c, CAL_ERR_ARG, w + ": no drive set (cal_prop_set_drive)");
        if (c->A_gen != P.drv_gen)
            return set_error(c, CAL_ERR_ARG, w + ": the context's matrix changed since cal_prop_set_drive");
        if (ldf < P.nk) return set_error(c, CAL_ERR_ARG, w + ": need ldf >= nk");
        for (int it = 0; it < nsteps; ++it)
            for (int k = 0; k < P.nk; ++k)
                if (!std::isfinite(f[(size_t)it * ldf + k]))
                    return set_error(c, CAL_ERR_ARG, w + ": non-finite amplitude in f");
    }
    const double t0 = now_ms();
    std::vector<double> cre, cim;
    int status = 0;
    if (P.nl_on() && (!P.d_v0 || c->A_gen != P.drv_gen))
        return set_error(c, CAL_ERR_ARG, w + ": the context's matrix changed since cal_prop_set_nonlinear");
    for (int it = 0; it < nsteps; ++it) {
        if (f)
            for (int k = 0; k < P.nk; ++k) P.f_last[k] = f[(size_t)it * ldf + k];
        const double nrm2_n = P.nrm2;  // psi_n's: the energetics row's N_n
        int ks = 0;
        double resid = 0.0;
        double en[2] = {0.0, 0.0};  // mu_n and res_n, from the step's first build
        if (P.nl_on()) {
            // the drive and the density of psi_n in one launch; "midpoint" then
            // predicts psi* into d_psi2 (psi_n and its norm stay where they
            // are) and rewrites the diagonal with the mean of both densities
            status = density_dev(c, P, P.f_last, P.g, nullptr, 0.0);
            if (status < 0) break;
            if (P.nl_mid) {
                status = krylov_scaled(c, P, dt, tol, adaptive, w + ": the predictor's first CA block broke down", &ks,
                                       cre, cim, &resid, en);
                if (status != 0) break;
                const LanczosView vp = lanczos_view(c);
                status = combine_dev(c, P, vp.Q, vp.ld, ks, cre.data(), cim.data(), true);
                if (status < 0) break;
                status = density_dev(c, P, P.f_last, 0.5 * P.g, P.d_psi2 + c->A.lpad, 0.5 * P.g);
                if (status < 0) break;
            }
        } else if (f) {
            status = diag_update_dev(c, P.d_v0, P.n, P.halves, P.nk, P.d_drv, P.ldd, f + (size_t)it * ldf);
            if (status < 0) break;
        }
        status = krylov_scaled(c, P, dt, tol, adaptive, w + ": the first CA block broke down", &ks, cre, cim, &resid,
                               P.nl_on() && P.nl_mid ? nullptr : en);
        if (status != 0) break;
        const LanczosView v = lanczos_view(c);
        status = combine_dev(c, P, v.Q, v.ld, ks, cre.data(), cim.data());
        if (status < 0) break;
        if (P.nl_on()) {  // [t_n, sum |psi_n|^4]: the state the step started from
            P.nhist.push_back(P.t);
            P.nhist.push_back(P.h_coef[2 * kPropMaxCols + P.red_count()]);
        }
        {  // [t_n, N_n, mu_n, E_n, res_n]: E_n = N_n mu_n - (g/2) sum |psi_n|^4
            double E = nrm2_n * en[0];
            if (P.nl_on()) E = E - 0.5 * P.g * P.h_coef[2 * kPropMaxCols + P.red_count()];
            const double row[5] = {P.t, nrm2_n, en[0], E, en[1]};
            P.ehist.insert(P.ehist.end(), row, row + 5);
        }
        P.t += dt;
        if (P.obs_on()) record_row(P);
        if (P.abs_on()) record_absorbed(P);
        P.info.steps++;
        P.info.lsteps = ks;
        P.info.lsteps_max = std::max(P.info.lsteps_max, ks);
        P.info.lsteps_sum += ks;
        P.info.residual = resid;
        P.info.residual_max = std::max(P.info.residual_max, resid);
        P.info.norm = std::sqrt(P.nrm2);
    }
    P.info.ms += now_ms() - t0;
    return status;
}

int cal_prop_step(cal_ctx* c, double dt, double tol, int adaptive, int nsteps) {
    return prop_steps(c, "cal_prop_step", dt, tol, adaptive, nsteps, nullptr, 0);
}

int cal_prop_step_driven(cal_ctx* c, double dt, double tol, int adaptive, int nsteps, const double* f, int ldf) {
    if (!c) return CAL_ERR_ARG;
    if (!f && nsteps > 0) return set_error(c, CAL_ERR_ARG, "cal_prop_step_driven: need f (nsteps rows of ldf)");
    return prop_steps(c, "cal_prop_step_driven", dt, tol, adaptive, nsteps, f, ldf);
}

int cal_prop_set_drive(cal_ctx* c, int nk, const double* W) {
    CAL_TRY(active_prop(c, "cal_prop_set_drive", true));
    hipSetDevice(c->device);
    PropState& P = *c->prop;
    if (nk < 0 || nk > kDriveMaxOps || (nk > 0 && !W))
        return set_error(c, CAL_ERR_ARG, "cal_prop_set_drive: need 0 <= nk <= 4 and W (n x nk) when nk > 0");
    for (size_t i = 0; i < (size_t)nk * P.n; ++i)
        if (!std::isfinite(W[i])) return set_error(c, CAL_ERR_ARG, "cal_prop_set_drive: non-finite entry in W");
    CAL_TRY(diag_positions(c));  // refusals leave the matrix and an earlier drive as they are
    // an earlier drive goes off: V0 goes back into the matrix, and stays the
    // propagator's while a nonlinear term is on (the matrix then holds V0 + g
    // rho: gathering it again would take the wrong values)
    int st = P.nl_on() ? v0_write(c, P, nullptr) : v0_release(c, P);
    drive_free(P);
    if (st < 0 || nk == 0) return st;
    CAL_TRY(v0_take(c, P));
    const int64_t ldd = pad64(P.n);
    double* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)nk * ldd * sizeof(double)) != hipSuccess) st = CAL_ERR_HIP;
    if (st == 0 && (upload_cols(c, d, ldd, W, P.n, nk) < 0 ||
                    hipStreamSynchronize(c->stream) != hipSuccess))  // W is the caller's
        st = CAL_ERR_HIP;
    if (st < 0) {  // the matrix holds V0
        if (d) hipFree(d);
        if (!P.nl_on()) v0_release(c, P);
        return set_error(c, CAL_ERR_HIP, "cal_prop_set_drive: upload failed");
    }
    P.d_drv = d;
    P.ldd = ldd;
    P.nk = nk;
    return 0;
}

int cal_prop_set_nonlinear(cal_ctx* c, double g, const char* density) {
    if (!c) return CAL_ERR_ARG;
    CAL_TRY(active_prop(c, "cal_prop_set_nonlinear", true));
    hipSetDevice(c->device);
    PropState& P = *c->prop;
    const std::string dn = density ? density : "";
    if (!std::isfinite(g)) return set_error(c, CAL_ERR_ARG, "cal_prop_set_nonlinear: g must be finite");
    if (dn != "frozen" && dn != "midpoint")
        return set_error(c, CAL_ERR_ARG, "cal_prop_set_nonlinear: density must be \"frozen\" or \"midpoint\"");
    if (g == 0.0) {
        if (!P.nl_on()) return 0;  // nothing was set: nothing to put back
        CAL_HIP(c, hipStreamSynchronize(c->stream));
        nl_free(P);
        // a drive stays: the matrix goes back to whatever H its last step left
        return P.nk > 0 ? v0_write(c, P, P.f_last) : v0_release(c, P);
    }
    CAL_TRY(diag_positions(c));  // refusals leave the matrix and the propagator as they are
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    const bool owned = P.d_v0 != nullptr;
    CAL_TRY(v0_take(c, P));  // the first of {drive, term}: V0 is gathered now
    if (!P.d_psi2) {
        const int64_t ld = c->A.ld;
        const int nb = diag_density_blocks(P.n);
        double *psi2 = nullptr, *part = nullptr, *h2 = nullptr;
        if (hipMalloc((void**)&psi2, ld * sizeof(double)) != hipSuccess ||
            hipMalloc((void**)&part, (size_t)nb * sizeof(double)) != hipSuccess ||
            hipHostMalloc((void**)&h2, 2 * kPropMaxCols * sizeof(double), hipHostMallocDefault) != hipSuccess ||
            hipMemsetAsync(psi2, 0, ld * sizeof(double), c->stream) != hipSuccess ||
            hipMemsetAsync(part, 0, (size_t)nb * sizeof(double), c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) {
            if (psi2) hipFree(psi2);
            if (part) hipFree(part);
            if (h2) hipHostFree(h2);
            if (!owned) v0_release(c, P);  // nothing else was written
            return set_error(c, CAL_ERR_HIP, "cal_prop_set_nonlinear: allocation failed");
        }
        std::memset(h2, 0, 2 * kPropMaxCols * sizeof(double));
        P.d_psi2 = psi2;
        P.d_nlpart = part;
        P.h_coef2 = h2;
        P.nl_nb = nb;
    }
    P.g = g;
    P.nl_mid = dn == "midpoint";
    P.nhist.clear();
    return 0;
}

int cal_prop_get_nonlinear(cal_ctx* c, int64_t first, int64_t count, double* out, int64_t* nrows) {
    if (!c) return CAL_ERR_ARG;
    CAL_TRY(active_prop(c, "cal_prop_get_nonlinear", false));
    return history_rows(c, "cal_prop_get_nonlinear", c->prop->nhist, 2, first, count, out, nrows);
}

int cal_prop_refresh_shifts(cal_ctx* c) {
    CAL_TRY(active_prop(c, "cal_prop_refresh_shifts", false));
    PropState& P = *c->prop;
    if (!P.newton) return 0;
    P.have_shifts = false;
    P.shifts.clear();
    return 0;
}

int cal_prop_get(cal_ctx* c, double* psi_re, double* psi_im, cal_prop_info* info) {
    CAL_TRY(active_prop(c, "cal_prop_get", false));
    hipSetDevice(c->device);
    PropState& P = *c->prop;
    if (psi_re) CAL_HIP(c, hipMemcpyAsync(psi_re, P.psi(c), P.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (psi_im && P.halves == 1) std::memset(psi_im, 0, P.n * sizeof(double));  // a real state
    if (psi_im && P.halves == 2)
        CAL_HIP(c, hipMemcpyAsync(psi_im, P.psi(c) + P.n, P.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (psi_re || psi_im) CAL_HIP(c, hipStreamSynchronize(c->stream));
    if (info) {
        *info = P.info;
        info->nshifts = P.have_shifts ? (int)std::min<size_t>(P.shifts.size(), 64) : 0;
        for (int i = 0; i < 64; ++i) info->shifts[i] = i < info->nshifts ? P.shifts[i] : 0.0;
    }
    return 0;
}

int cal_prop_end(cal_ctx* c) {
    if (!c) return CAL_ERR_ARG;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    prop_free(c);
    cal_lanczos_end(c);
    return 0;
}

int cal_ca_lanczos_prop(cal_ctx* c, int64_t n, const double* r_re, const double* r_im, int s, int m, double dt,
                        double tol, const char* basis, const double* eigest, int neig, int adaptive, double* T,
                        double* Q_re, double* Q_im, int* lsteps) {
    if (!c) return CAL_ERR_ARG;
    if (!T || !lsteps || !std::isfinite(dt) || std::isnan(tol))
        return set_error(c, CAL_ERR_ARG, "cal_ca_lanczos_prop: need T, lsteps, a finite dt and a tol");
    CAL_TRY(cal_prop_begin(c, n, r_re, r_im, s, m, basis, eigest, neig));
    PropState& P = *c->prop;
    std::vector<double> cre, cim;
    int ks = 0;
    double resid = 0.0;
    int status = krylov_scaled(c, P, dt, tol, adaptive, "cal_ca_lanczos_prop: the first CA block broke down", &ks, cre,
                               cim, &resid, nullptr);
    if (status == 0) {
        const LanczosView v = lanczos_view(c);
        *lsteps = ks;
        for (int j = 0; j < ks; ++j)
            for (int i = 0; i < ks; ++i) T[i + (size_t)j * ks] = v.T[i + (size_t)j * v.ldt];
        auto get = [&](double* dst, const double* src) -> int {
            CAL_HIP(c, hipMemcpy2DAsync(dst, n * sizeof(double), src, v.ld * sizeof(double), n * sizeof(double), ks,
                                        hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        if (Q_re) status = get(Q_re, v.Q);
        if (status == 0 && Q_im) status = get(Q_im, v.Q + n);
        if (status == 0) status = hipStreamSynchronize(c->stream) == hipSuccess ? 0 : CAL_ERR_HIP;
    } else {
        *lsteps = 0;
    }
    cal_prop_end(c);
    return status;
}

}  // extern "C"
