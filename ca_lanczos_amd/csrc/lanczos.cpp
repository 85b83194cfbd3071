// lanczos.cpp -- the device-resident CA-Lanczos outer loop (ca_lanczos.m).
//
//   begin():  q = r/sqrt(r'r) (ca_lanczos.m:55); change of basis Bk: monomial
//             (:63-65) or Newton (:66-72: 2s-step Lanczos 'fro' on the GPU,
//             eig + modified Leja + newton_basis_matrix on the host).
//   step():   one outer iteration (:166-237): s fused SpMV+shift launches
//             into V, block orthogonalisation (normalize at k=1,
//             projectAndNormalize against the previous block otherwise, plus
//             the 'fro' pass against all of Q), the host-side T extension
//             (:200-223) and, optionally, the Ritz residuals / orthogonality
//             error diagnostics (:228-236).
// Only (s+1) x s, s x s and (2s+1) x s matrices cross PCIe per iteration.
#include <algorithm>
#include <chrono>
#include <limits>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <string>
#include <system_error>
#include <vector>

#include "../../include/calanczos_host.h"
#include "cal_internal.hpp"
#include "comm.hpp"
#include "dense.hpp"
#include "leja.hpp"

namespace cal {

// block size limit: the k = 1 block has s + 1 <= 32 columns (the TSQR tile)
// and the Newton prologue's 2s shifts fit cal_lanczos_info.shifts[64]
constexpr int kMaxS = 31;

// Ritz pair of T(1:sk,1:sk) (compute_ritz_rnorm, ca_lanczos.m:88-97)
struct RitzPair {
    double lr, li;
    int cr, ci;  // columns of the real / imaginary part in V (ci = -1: real)
};

// The diagnostics of one outer iteration (ca_lanczos.m:227-236), run one
// iteration late: eig(T_k) is solved on the host while the GPU runs step
// k + 1's matrix powers and the previous iteration's diagnostics kernels
// (diagnostics on).
struct DiagJob {
    int k = 0;  // outer iteration described; 0: empty
    std::vector<RitzPair> pairs;  // MATLAB's descending sort
    std::vector<double> V;        // eigenvectors of T_k (sk x sk)
    std::vector<double> Tk;       // T(1:sk,1:sk), the eig's input
    std::future<int> eig;         // the eig on a host worker thread (diag_prepare)
    struct OeChunk {
        int a0, na, b0, nb, ldc;
        size_t off;  // doubles into the result region
    };
    std::vector<OeChunk> oe;
    int wa = 0;
    std::vector<int> sep;  // pairs reduced on their own (row kernel)
    hipEvent_t ev = nullptr;           // the job's results are in pinned memory
    std::vector<hipEvent_t> evc;       // diag_launch: chunk q of X written; [nch]: the job's start
};

struct LanczosState {
    int s = 0, max_outer = 0, k = 0;
    bool newton = false, full = false;
    int mode = 0;  // orth: 0 local, 1 full, 2 periodic, 3 selective (ca_lanczos.m:74-84)
    double norm_A = 0.0;  // normest(A) (periodic / selective)
    std::vector<double> omega;  // periodic: (om_n x om_n), column-major
    int om_n = 0;
    double* dQR = nullptr;  // selective: converged Ritz vectors (orthonormal), ld x qr_cap
    double* dQRy = nullptr;  // selective: their un-normalised form / work
    int qr_cap = 0, nritz = 0;
    // explicit restart (restarted_ca_lanczos.m): the converged vectors Q_conv
    // every new block is also projected against
    bool restart_inner = false;
    double* dExt = nullptr;  // Q_conv columns (not owned), lpad origin
    int next = 0;
    int64_t n = 0, ld = 0;
    double* dQ = nullptr;  // ld x (s*max_outer + 1)
    double* dV = nullptr;  // ld x 2(s+1): the basis block, double-buffered by step parity
    bool powers_ready = false;  // matrix powers of step k+1 already enqueued (prefetch)
    std::vector<double> Bk;  // (s+1) x s
    int Tld = 0;
    std::vector<double> T;  // Tld x Tld
    std::vector<double> b;
    std::vector<int> reorth;
    std::vector<std::vector<double>> rn;
    std::vector<double> oe;
    cal_lanczos_info info{};
    bool breakdown = false;
    // deferred diagnostics: `ready` solved on the host, `pending` on the stream
    DiagJob ready, pending;
    double* d_dres = nullptr;  // results: residual sums (2 sk), then the orth-error Grams
    double* h_dres = nullptr;  // pinned
    size_t dres_cap = 0;
    double* d_din = nullptr;   // inputs: Vp (sk x sk), Ritz values, pair columns / slots
    double* h_din = nullptr;   // pinned
    size_t din_cap = 0;
    double* d_dpart = nullptr;  // block partials of the diagnostics' auxiliary-stream kernels
    size_t dpart_cap = 0;
    // orthogonality errors deferred to the flush ('local' / 'full': Q(:,1:sk+1)
    // is final once written): the iterations still to do, one wide Gram then
    bool oe_defer = false;
    std::vector<int> oe_pend;
    double* d_oe = nullptr;  // the wide Gram's entries
    double* h_oe = nullptr;  // pinned
    size_t oe_cap = 0;
    int64_t lpad = 0;  // local origin inside each column (left halo space)
    double* col(int j) { return dQ + (size_t)j * ld + lpad; }
    double* vcolumn(int j, int par = 0) { return dV + ((size_t)par * (s + 1) + j) * ld + lpad; }
};

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// global dot product x'y of two device n-vectors (allreduced)
static int dot_host(cal_ctx* c, int64_t n, const double* x, const double* y, double* out) {
    const int nb = dot_blocks(n);
    CAL_TRY(ensure_partial(c, nb));
    CAL_TRY(ensure_red(c, 1));
    CAL_HIP_OTHER(c, launch_dot(x, y, n, c->d_partial, nb, c->stream));
    CAL_HIP_OTHER(c, launch_reduce(c->d_partial, nb, 1, c->d_red, c->stream));
    CAL_TRY(allreduce_sum(c, c->d_red, 1));
    CAL_HIP_OTHER(c, hipMemcpyAsync(c->h_red, c->d_red, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    c->small_pending = false;
    *out = c->h_red[0];
    return 0;
}

// matrix powers of step k into the V buffer of parity k & 1 (ca_lanczos.m:
// 110-118); V(:,1) = q is not copied: the panels reference q's column of Q.
static int lanczos_powers(cal_ctx* c, LanczosState& L, const double* q, int par) {
    const int s = L.s;
    std::vector<double*> Y(s);
    std::vector<double> sh(s);
    for (int i = 0; i < s; ++i) {
        Y[i] = L.vcolumn(i + 1, par);
        sh[i] = L.newton ? L.Bk[i + (size_t)i * (s + 1)] : 0.0;
    }
    return powers_dev(c, s, q, Y.data(), L.newton ? sh.data() : nullptr, nullptr, nullptr);
}

static int enqueue_powers(cal_ctx* c, LanczosState& L, int k) {
    return lanczos_powers(c, L, L.col((k - 1) * L.s), k & 1);
}

// ---- normest(A) (MATLAB built-in; ca_lanczos.m:258,370) ---------------------
// Power iteration on A'A = A^2 (A symmetric) from x = sum(abs(A))', until the
// estimate changes by <= tol * e (tol 1e-6, at most 100 iterations).  The
// iterations run in chunks of kNormestChunk with no host round trip: each
// leaves ||x||^2 and ||Sx||^2 in d_red and rescales x by the device-side norm
// (the host's sqrt and division, same bits); the host then replays MATLAB's
// stopping test over the chunk and stops at the same iteration with the same
// e -- extra iterations of the last chunk are discarded.
static int normest_dev(cal_ctx* c, double* out) {
    constexpr int kNormestChunk = 8;
    constexpr size_t kNrm = 4096;  // d_red / h_red offset (orth_device uses [0, 4096))
    CAL_TRY(shared_refuses(c, "normest"));
    const int64_t n = c->A.n_local, ld = c->A.ld;
    CAL_TRY(ensure_work(c, 2, ld));
    CAL_TRY(ensure_red(c, kNrm + 2 * kNormestChunk));
    double* x = work_col(c, 0) + c->A.lpad;
    double* y = work_col(c, 1) + c->A.lpad;
    CAL_HIP_OTHER(c, launch_abs_rowsum(c->A.rowptr + c->A.ext_off, c->A.val, n, x, c->stream));
    double xx = 0.0;
    CAL_TRY(dot_host(c, n, x, x, &xx));
    double e = std::sqrt(xx);
    if (e == 0.0) {
        *out = 0.0;
        return 0;
    }
    CAL_HIP_OTHER(c, launch_div(x, x, e, n, c->stream));
    const int nb = dot_blocks(n);
    CAL_TRY(ensure_partial(c, nb));
    auto dot_dev = [&](const double* a, double* dst) -> int {
        CAL_HIP_OTHER(c, launch_dot(a, a, n, c->d_partial, nb, c->stream));
        CAL_HIP_OTHER(c, launch_reduce(c->d_partial, nb, 1, dst, c->stream));
        return allreduce_sum(c, dst, 1);
    };
    double* d_nrm = c->d_red + kNrm;
    const double* h_nrm = c->h_red + kNrm;
    // one rank: both norms and the rescale in two launches (the same bits);
    // the test build's CAL_TEST_PROLOGUE_SPLIT keeps the separate launches
    const bool fused = !test_switch("CAL_TEST_PROLOGUE_SPLIT") && (!c->comm || c->comm->nranks <= 1);
    if (fused) CAL_TRY(ensure_partial(c, 2 * (size_t)nb));
    // CSR: x is never rescaled in memory -- the next Sx = S*x divides each
    // gathered x_j by the norm (SpMV mode 3): the same quotients, one read
    // and one write of x fewer per iteration
    const bool gather_div = fused && !c->A.use_pat;
    const double* xnrm = nullptr;  // ||x||^2 of the unscaled x (device), after the first iteration
    double e0 = 0.0;
    int cnt = 0;
    for (;;) {
        for (int i = 0; i < kNormestChunk; ++i) {
            CAL_TRY(spmv_dev(c, x, y, xnrm ? 3 : 0, 0.0, 0.0, nullptr, xnrm));  // Sx = S*x
            CAL_TRY(spmv_dev(c, y, x, 0, 0.0, 0.0, nullptr));                  // x = S'*Sx
            if (gather_div) {
                CAL_HIP_OTHER(c, launch_normest_norms_only(x, y, n, c->d_partial, d_nrm + 2 * i, c->stream));
                xnrm = d_nrm + 2 * i;
                continue;
            }
            if (fused) {
                CAL_HIP_OTHER(c, launch_normest_norms(x, y, n, c->d_partial, d_nrm + 2 * i, c->stream));
                continue;
            }
            CAL_TRY(dot_dev(x, d_nrm + 2 * i));
            CAL_TRY(dot_dev(y, d_nrm + 2 * i + 1));
            CAL_HIP_OTHER(c, launch_div_sqrt(x, x, d_nrm + 2 * i, n, c->stream));  // x = x / norm(x)
        }
        CAL_HIP_OTHER(c, hipMemcpyAsync(c->h_red + kNrm, d_nrm, 2 * kNormestChunk * sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream));
        CAL_HIP(c, hipStreamSynchronize(c->stream));
        c->small_pending = false;
        for (int i = 0; i < kNormestChunk; ++i) {
            if (!(std::fabs(e - e0) > 1.0e-6 * e && cnt <= 100)) {
                *out = e;
                return 0;
            }
            e0 = e;
            const double nx = std::sqrt(h_nrm[2 * i]);
            e = nx / std::sqrt(h_nrm[2 * i + 1]);
            ++cnt;
        }
    }
}

int normest_run(cal_ctx* c, double* out) { return normest_dev(c, out); }

// ---- normest on its own stream (one rank) ----------------------------------
// The same iteration as normest_dev -- the same kernels in the same order, so
// the same e to the bit -- enqueued on the context's normest stream in chunks
// of kNestChunk iterations, so that it runs beside whatever the caller
// enqueues next on the solver's stream (the IRL's Newton prologue and first CA
// blocks: normest(A) is needed only at the first convergence test,
// impl_restarted_ca_lanczos.m:37-40,127-143).  The host never waits on it
// until normest_async_finish: normest_async_poll (non-blocking) replays
// MATLAB's stopping test over a finished chunk and enqueues the next one.
// x, Sx and the partials are the normest's own scratch (c->d_nest), nothing
// the solver's stream touches.
namespace {
constexpr int kNestChunk = 16;
struct NormestAsync {
    bool active = false, done = false;
    bool gather_div = false;   // CSR: x rescaled in the next SpMV's gathers (mode 3)
    double e = 0.0, e0 = 0.0;  // MATLAB's e, e0
    int cnt = 0;               // iterations replayed
    int chunk = 0;             // chunks enqueued
    const double* xnrm = nullptr;
    double result = 0.0;
    int timer = -1;  // the span on the normest stream (timer kind "normest")
};
}  // namespace

// One chunk's launches (kNestChunk iterations and the norms' copy to the
// host), xnrm0 the first SpMV's divisor (null: x already rescaled).
static hipError_t normest_chunk_launches(const cal_ctx* c, bool gather_div, const double* xnrm0, hipStream_t st) {
    const int64_t n = c->A.n_local;
    const int nb = dot_blocks(n);
    double* x = c->d_nest;
    double* y = x + n;
    double* part = y + n;
    double* d_nrm = part + 2 * (size_t)nb;  // [0] = x0'x0, then 2 per iteration of the chunk
    const double* xnrm = xnrm0;
    hipError_t e = hipSuccess;
    for (int i = 0; i < kNestChunk && e == hipSuccess; ++i) {
        e = spmv_on_stream(c, x, y, xnrm ? 3 : 0, xnrm, st);     // Sx = S*x
        if (e == hipSuccess) e = spmv_on_stream(c, y, x, 0, nullptr, st);  // x = S'*Sx
        double* dst = d_nrm + 1 + 2 * i;
        if (e != hipSuccess) break;
        if (gather_div) {
            e = launch_normest_norms_only(x, y, n, part, dst, st);
            xnrm = dst;
        } else {
            e = launch_normest_norms(x, y, n, part, dst, st);
        }
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->h_nest, d_nrm, (1 + 2 * kNestChunk) * sizeof(double), hipMemcpyDeviceToHost, st);
    return e;
}

// The chunk as a replayed graph: the ~50 launches cost the host ~0.7 ms per
// chunk, time in which the solver's stream (waiting for its next block's
// launches) ran dry; one graph launch costs tens of us.  The first chunk
// (kind 0) and the later ones (kind 1: the first SpMV divides by the previous
// chunk's last norm) are captured once per context and re-captured when the
// scratch or the matrix change.  Same kernels, same order: same bits.
static int normest_chunk_graph(cal_ctx* c, const NormestAsync& J, int kind, hipStream_t st) {
    const DevMatrix& A = c->A;
    const std::vector<int64_t> key = {(int64_t)(intptr_t)c->d_nest, (int64_t)(intptr_t)A.rowptr,
                                      (int64_t)(intptr_t)A.col,    (int64_t)(intptr_t)A.val,
                                      (int64_t)(intptr_t)A.blk,    (int64_t)A.nblk,
                                      (int64_t)A.nit,              (int64_t)A.use_pat,
                                      (int64_t)A.ext_off,          A.n_local,
                                      (int64_t)A.nnz,              (int64_t)J.gather_div,
                                      (int64_t)c->A_gen};
    if (!c->nest_exec[kind] || c->nest_key[kind] != key) {
        if (c->nest_exec[kind]) CAL_HIP(c, hipGraphExecDestroy(c->nest_exec[kind]));
        c->nest_exec[kind] = nullptr;
        CAL_HIP(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const hipError_t e = normest_chunk_launches(c, J.gather_div, J.xnrm, st);
        hipGraph_t g = nullptr;
        const hipError_t e2 = hipStreamEndCapture(st, &g);
        CAL_HIP(c, e);
        CAL_HIP(c, e2);
        const hipError_t e3 = hipGraphInstantiate(&c->nest_exec[kind], g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        CAL_HIP(c, e3);
        c->nest_key[kind] = key;
    }
    CAL_HIP(c, hipGraphLaunch(c->nest_exec[kind], st));
    return 0;
}

static int normest_async_enqueue_chunk(cal_ctx* c, NormestAsync& J) {
    const int64_t n = c->A.n_local;
    const int nb = dot_blocks(n);
    double* d_nrm = c->d_nest + 2 * n + 2 * (size_t)nb;
    const hipStream_t st = c->nest_stream;
    if (test_switch("CAL_TEST_NEST_DIRECT")) {  // the test build's A/B: the launches themselves
        CAL_HIP(c, normest_chunk_launches(c, J.gather_div, J.xnrm, st));
    } else {
        CAL_TRY(normest_chunk_graph(c, J, J.xnrm ? 1 : 0, st));
    }
    if (J.gather_div) J.xnrm = d_nrm + 1 + 2 * (kNestChunk - 1);
    timer_end_on(c, J.timer, st);  // re-recorded per chunk: the last one ends the span
    CAL_HIP(c, hipEventRecord(c->nest_event, st));
    J.chunk++;
    return 0;
}

static int normest_async_begin(cal_ctx* c, NormestAsync& J) {
    CAL_TRY(shared_refuses(c, "normest"));
    J = NormestAsync();
    const int64_t n = c->A.n_local;
    const int nb = dot_blocks(n);
    const size_t need = 2 * (size_t)n + 2 * (size_t)nb + 1 + 2 * kNestChunk;
    if (!c->nest_stream) CAL_HIP(c, hipStreamCreateWithFlags(&c->nest_stream, hipStreamNonBlocking));
    if (!c->nest_event) CAL_HIP(c, hipEventCreateWithFlags(&c->nest_event, hipEventDisableTiming));
    if (need > c->nest_cap) {
        if (c->d_nest) CAL_HIP(c, hipFree(c->d_nest));
        c->d_nest = nullptr;
        CAL_HIP(c, scratch_malloc((void**)&c->d_nest, need * sizeof(double)));
        if (!c->h_nest)
            CAL_HIP(c, hipHostMalloc((void**)&c->h_nest, (1 + 2 * kNestChunk) * sizeof(double), hipHostMallocDefault));
        c->nest_cap = need;
    }
    double* x = c->d_nest;
    double* part = x + 2 * n;
    double* d_nrm = part + 2 * (size_t)nb;
    const hipStream_t st = c->nest_stream;
    // the matrix must be on the device before the normest stream reads it
    CAL_HIP(c, hipEventRecord(c->nest_event, c->stream));
    CAL_HIP(c, hipStreamWaitEvent(st, c->nest_event, 0));
    J.timer = timer_begin_on(c, 6, st);
    // x = sum(abs(S))', e = norm(x) (kept on the device), x = x/e
    CAL_HIP(c, launch_abs_rowsum(c->A.rowptr + c->A.ext_off, c->A.val, n, x, st));
    CAL_HIP(c, launch_dot(x, x, n, part, nb, st));
    CAL_HIP(c, launch_reduce(part, nb, 1, d_nrm, st));
    CAL_HIP(c, launch_div_sqrt(x, x, d_nrm, n, st));
    J.gather_div = !c->A.use_pat;
    J.active = true;
    return normest_async_enqueue_chunk(c, J);
}

// The finished chunk's norms: MATLAB's stopping test replayed (normest_dev's
// loop); enqueue the next chunk if it did not stop.  wait: block on the chunk.
static int normest_async_poll(cal_ctx* c, NormestAsync& J, bool wait) {
    while (J.active && !J.done) {
        if (wait) CAL_HIP(c, hipEventSynchronize(c->nest_event));
        else {
            const hipError_t q = hipEventQuery(c->nest_event);
            if (q == hipErrorNotReady) return 0;
            CAL_HIP(c, q);
        }
        const double* h = c->h_nest;
        if (J.chunk == 1) {
            J.e = std::sqrt(h[0]);
            if (J.e == 0.0) {  // normest of a zero matrix
                J.result = 0.0;
                J.done = true;
                return 0;
            }
        }
        for (int i = 0; i < kNestChunk; ++i) {
            if (!(std::fabs(J.e - J.e0) > 1.0e-6 * J.e && J.cnt <= 100)) {
                J.result = J.e;
                J.done = true;
                return 0;
            }
            J.e0 = J.e;
            J.e = std::sqrt(h[1 + 2 * i]) / std::sqrt(h[2 + 2 * i]);
            ++J.cnt;
        }
        CAL_TRY(normest_async_enqueue_chunk(c, J));
        if (!wait) return 0;
    }
    return 0;
}

static int normest_async_finish(cal_ctx* c, NormestAsync& J, double* out) {
    CAL_TRY(normest_async_poll(c, J, true));
    J.active = false;
    *out = J.result;
    return 0;
}

// ---- periodic: the omega recurrence (ca_lanczos.m:464-549) -----------------
static void update_omega(LanczosState& L, const std::vector<double>& alpha, const std::vector<double>& beta) {
    const int s = L.s;
    const double Tn = std::numeric_limits<double>::epsilon() * L.norm_A;
    auto al = [&](int i) { return alpha[i - 1]; };  // 1-based as in the reference
    auto be = [&](int i) { return beta[i - 1]; };
    int jlo, jhi, nn;
    std::vector<double> om;
    if (L.om_n == 0) {
        nn = s + 1;
        om.assign((size_t)nn * nn, 0.0);
        auto O = [&](int i, int j) -> double& { return om[(i - 1) + (size_t)(j - 1) * nn]; };
        O(1, 1) = 1.0;
        O(1, 2) = 0.0;
        O(2, 1) = Tn / be(1);
        O(2, 2) = 1.0;
        jlo = 2;
        jhi = s;
    } else {
        const int m = L.om_n - 1;
        nn = (int)alpha.size() + 1;
        om.assign((size_t)nn * nn, 0.0);
        for (int j = 0; j < L.om_n; ++j)
            for (int i = 0; i < L.om_n; ++i) om[i + (size_t)j * nn] = L.omega[i + (size_t)j * L.om_n];
        jlo = m + 1;
        jhi = m + s;
    }
    auto O = [&](int i, int j) -> double& { return om[(i - 1) + (size_t)(j - 1) * nn]; };
    for (int j = jlo; j <= jhi; ++j) {
        const double binv = 1.0 / be(j);
        double v = be(2) * O(j, 2) + (al(1) - al(j)) * O(j, 1) - be(j) * O(j - 1, 1);
        O(j + 1, 1) = v > 0 ? binv * (v + Tn) : binv * (v - Tn);
        for (int k = 2; k <= j - 1; ++k) {
            v = be(k + 1) * O(j, k + 1) + (al(k) - al(j)) * O(j, k) + be(k) * O(j, k - 1) - be(j) * O(j - 1, k);
            O(j + 1, k) = v > 0 ? binv * (v + Tn) : binv * (v - Tn);
        }
        O(j + 1, j) = binv * Tn;
        O(j + 1, j + 1) = 1.0;
    }
    L.omega.swap(om);
    L.om_n = nn;
}

static void reset_omega(LanczosState& L) {
    const int s = L.s, nn = L.om_n, m = nn - s - 1;
    const double Tn = std::numeric_limits<double>::epsilon() * L.norm_A;
    for (int j = m + 1; j <= m + s; ++j) {
        for (int k = 1; k <= j; ++k) L.omega[j + (size_t)(k - 1) * nn] = Tn;  // omega(j+1,k)
        L.omega[j + (size_t)j * nn] = 1.0;                                     // omega(j+1,j+1)
    }
}

// ---- Newton prologue: lanczos(A,q,2s,'full') (lanczos.m:18-134) ----------
static int newton_prologue(cal_ctx* c, LanczosState& L, bool cgs = true) {
    const RoctxRange marker("ca_lanczos newton prologue");
    const int s = L.s, m = 2 * s;
    const int64_t n = c->A.n_local, ld = c->A.ld;
    CAL_TRY(ensure_work(c, m + 2, ld));
    double* r = work_col(c, m + 1) + c->A.lpad;
    auto Qc = [&](int j) { return work_col(c, j) + c->A.lpad; };
    // q = r/norm(r) (lanczos.m:47) of the already normalised start vector
    double nrm2 = 0.0;
    CAL_TRY(dot_host(c, n, L.col(0), L.col(0), &nrm2));
    CAL_HIP_OTHER(c, launch_div(Qc(0), L.col(0), std::sqrt(nrm2), n, c->stream));
    // the 2s steps run without host round trips: alpha_j and beta_j^2 stay
    // on the device (d_red [kAB, kAB + 2m)) and feed the updates directly; the
    // CGS coefficients become [-R; 1] on the device (k_form_projM).  Same
    // kernels and operations as the host-driven loop: same bits.
    constexpr size_t kAB = 4096 + 64;  // above normest's chunk, below the async projection regions
    CAL_TRY(ensure_red(c, kAB + 2 * m + 2048));
    double* d_ab = c->d_red + kAB;      // alpha at [0, m), beta^2 at [m, 2m)
    double* d_cg = d_ab + 2 * m;        // CGS Gram (ld 16 * nta), M at +1024
    const int nbd = dot_blocks(n);
    CAL_TRY(ensure_partial(c, nbd));
    auto dot_dev = [&](const double* a, const double* b, double* dst) -> int {
        CAL_HIP_OTHER(c, launch_dot(a, b, n, c->d_partial, nbd, c->stream));
        CAL_HIP_OTHER(c, launch_reduce(c->d_partial, nbd, 1, dst, c->stream));
        return allreduce_sum(c, dst, 1);
    };
    // one rank: the recurrence in three launches per step (launch_pro_step,
    // the same bits); several ranks all-reduce each dot before its use.
    // the test build's CAL_TEST_PROLOGUE_SPLIT (read per run) keeps the
    // separate launches: the parity test compares both.
    const bool fused = !test_switch("CAL_TEST_PROLOGUE_SPLIT") && (!c->comm || c->comm->nranks <= 1);
    if (fused) CAL_TRY(ensure_partial(c, 2 * (size_t)nbd));
    for (int j = 0; j < m; ++j) {
        CAL_TRY(spmv_dev(c, Qc(j), r, 0, 0.0, 0.0, nullptr));  // :103
        if (fused) {
            CAL_HIP_OTHER(c, launch_pro_step(r, j > 0 ? Qc(j - 1) : nullptr, d_ab + m + j - 1, Qc(j), Qc(j + 1), n,
                                       c->d_partial, d_ab + j, d_ab + m + j, c->stream));  // :105-110
        } else {
            if (j > 0) CAL_HIP_OTHER(c, launch_axpy_sub_dev(r, Qc(j - 1), d_ab + m + j - 1, true, n, c->stream));  // :105
            CAL_TRY(dot_dev(r, Qc(j), d_ab + j));                                                          // :107
            CAL_HIP_OTHER(c, launch_axpy_sub_dev(r, Qc(j), d_ab + j, false, n, c->stream));                      // :108
            CAL_TRY(dot_dev(r, r, d_ab + m + j));                                                          // :109
            CAL_HIP_OTHER(c, launch_div_sqrt(Qc(j + 1), r, d_ab + m + j, n, c->stream));                         // :110
        }
        if (!cgs) continue;  // lanczos(...,'local') (restarted_ca_lanczos.m:65)
        // one CGS pass against Q(:,1:j) (lanczos.m:62-66)
        Panel Qj = panel();
        panel_add(Qj, Qc(0), ld, j + 1);
        Panel qn = panel();
        panel_add(qn, Qc(j + 1), ld, 1);
        const GramPlan pl = gram_plan(j + 1, 1, n);
        CAL_TRY(ensure_partial(c, (size_t)pl.blocks * pl.entries));
        CAL_HIP(c, launch_gram(Qj, qn, n, pl, c->d_partial, c->stream));
        CAL_HIP_OTHER(c, launch_reduce(c->d_partial, pl.blocks, pl.entries, d_cg, c->stream));
        CAL_TRY(allreduce_sum(c, d_cg, pl.entries));
        double* dM = d_cg + 1024;
        CAL_HIP_OTHER(c, launch_form_projM(d_cg, 16 * pl.nta, j + 1, 1, dM, c->stream));
        Panel W = panel();
        panel_add(W, Qc(0), ld, j + 2);  // [Q(:,1:j) | q_{j+1}] contiguous
        const ApplyPlan ap = apply_plan(j + 2, 1, n, false, 0);
        CAL_HIP(c, launch_apply(W, dM, j + 2, 1, panel_out(Qc(j + 1), ld, 1), true, 0, n, ap, c->d_partial,
                                c->stream));
    }
    std::vector<double> alpha(m), beta(m);
    {
        CAL_HIP_OTHER(c, hipMemcpyAsync(c->h_red + kAB, d_ab, 2 * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        CAL_HIP(c, hipStreamSynchronize(c->stream));
        c->small_pending = false;
        for (int j = 0; j < m; ++j) {
            alpha[j] = c->h_red[kAB + j];
            beta[j] = std::sqrt(c->h_red[kAB + m + j]);
            if (!(beta[j] > 0.0) || !std::isfinite(beta[j])) {
                L.breakdown = true;
                return set_error(c, CAL_ERR_NUMERIC, "Lanczos breakdown (beta = 0) in the Newton prologue");
            }
        }
    }
    // eig(T) of the 2s x 2s symmetric tridiagonal (ca_lanczos.m:69): ascending
    std::vector<double> w(m);
    if (!dense::tridiag_eigvals(m, alpha.data(), beta.data(), w.data()))
        return set_error(c, CAL_ERR_NUMERIC, "tridiagonal eigensolver did not converge");
    std::vector<std::complex<double>> x(m), y;
    for (int i = 0; i < m; ++i) x[i] = std::complex<double>(w[i], 0.0);
    std::vector<int> oi;
    std::string err;
    if (leja::real_leja(x, y, oi, err) != 0) return set_error(c, CAL_ERR_NUMERIC, "leja: " + err);  // :70
    for (int i = 0; i < m && i < 64; ++i) {
        L.info.shifts[i] = y[i].real();
        L.info.shifts_im[i] = y[i].imag();
    }
    if (leja::newton_basis_matrix(s, y, 1, L.Bk, err) != 0)  // :71
        return set_error(c, CAL_ERR_NUMERIC, "newton_basis_matrix: " + err);
    return 0;
}

// ---- Ritz diagnostics (compute_ritz_rnorm / compute_orth_err, -----------
// ca_lanczos.m:88-107,227-236), deferred by one outer iteration.
//   diag_prepare(k): eig(T(1:sk,1:sk)) and MATLAB's descending sort, on the
//     host, right after step k's T extension (the GPU meanwhile runs step
//     k + 1's prefetched matrix powers and step k - 1's diagnostics kernels);
//   diag_launch: the orthogonality error's Grams of Q(:,1:sk+1), X = Q(:,1:sk)
//     Vp on the matrix cores, the residual sums of all sk pairs (real pairs on
//     the pair patterns in one launch), one reduction, async copies to pinned
//     memory, an event; enqueued in step k + 1 before anything there rewrites
//     Q(:,1:sk+1) (periodic);
//   diag_collect: reads the results once the event has passed (in step k + 2
//     after the block orthogonalisation's wait, i.e. without waiting).
// The last step (and cal_lanczos_get) flush what is left.
static void matlab_sort_desc(std::vector<RitzPair>& v, bool cplx) {
    std::stable_sort(v.begin(), v.end(), [&](const RitzPair& a, const RitzPair& b) {
        if (!cplx) return a.lr > b.lr;
        const double aa = std::hypot(a.lr, a.li), ab = std::hypot(b.lr, b.li);
        if (aa != ab) return aa > ab;
        return std::atan2(a.li, a.lr) > std::atan2(b.li, b.lr);
    });
}

// [Vp,Dp] = eig(T(1:s*k,1:s*k)) (ca_lanczos.m:229) and the sort, on J's own
// copy of T_k: runs on a host worker thread (touches nothing but J)
static int diag_eig(DiagJob& J, int sk) {
    std::vector<double> wr(sk), wi(sk);
    J.V.assign((size_t)sk * sk, 0.0);
    if (cal_eig(sk, J.Tk.data(), sk, wr.data(), wi.data(), J.V.data()) != 0) return CAL_ERR_NUMERIC;
    J.pairs.clear();
    bool cplx = false;
    for (int j = 0; j < sk; ++j) {
        if (wi[j] != 0.0) {
            cplx = true;
            // V(:,j) + i V(:,j+1) belongs to wr + i|wi|; the conjugate uses the
            // conjugate vector (same residual norm)
            const int jr = wi[j] > 0 ? j : j - 1;
            J.pairs.push_back({wr[j], wi[j], jr, jr + 1});
        } else {
            J.pairs.push_back({wr[j], 0.0, j, -1});
        }
    }
    matlab_sort_desc(J.pairs, cplx);
    return 0;
}

// Step k's job: T_k copied, its eig started on a worker thread.  The eig is
// O((sk)^3) (10 ms at sk = 120 on one core) and used to run on the calling
// thread between two steps, where at large k it outlasted the GPU work queued
// behind it; now it overlaps the next step too, and diag_join waits for it
// right before the job's kernels are launched (one step later).
static int diag_prepare(cal_ctx* c, LanczosState& L, DiagJob& J) {
    (void)c;
    const int sk = L.s * L.k;
    J.Tk.resize((size_t)sk * sk);
    for (int j = 0; j < sk; ++j)
        for (int i = 0; i < sk; ++i) J.Tk[i + (size_t)j * sk] = L.T[i + (size_t)j * L.Tld];
    J.k = L.k;
    DiagJob* jp = &J;
    try {
        J.eig = std::async(std::launch::async, [jp, sk]() { return diag_eig(*jp, sk); });
    } catch (const std::system_error&) {  // no thread to be had: the eig on this thread
        std::promise<int> done;
        done.set_value(diag_eig(J, sk));
        J.eig = done.get_future();
    }
    return 0;
}

// wait for a job's eig (before anything moves or reads J)
static int diag_join(cal_ctx* c, DiagJob& J) {
    if (!J.eig.valid()) return 0;
    if (J.eig.get() != 0) {
        J.k = 0;
        return set_error(c, CAL_ERR_NUMERIC, "eig(T) did not converge");
    }
    return 0;
}

static int grow_pinned(cal_ctx* c, double** d, double** h, size_t* cap, size_t need) {
    if (need <= *cap) return 0;
    if (*d) CAL_HIP(c, hipFree(*d));
    if (*h) CAL_HIP(c, hipHostFree(*h));
    *d = *h = nullptr;
    const size_t n = std::max(need, *cap + *cap / 2);
    CAL_HIP(c, scratch_malloc((void**)d, n * sizeof(double)));
    CAL_HIP(c, hipHostMalloc((void**)h, n * sizeof(double), hipHostMallocDefault));
    *cap = n;
    return 0;
}

static int grow_pinned_dev(cal_ctx* c, double** d, size_t* cap, size_t need) {
    if (need <= *cap) return 0;
    if (*d) CAL_HIP(c, hipFree(*d));
    *d = nullptr;
    const size_t n = std::max(need, *cap + *cap / 2);
    CAL_HIP(c, scratch_malloc((void**)d, n * sizeof(double)));
    *cap = n;
    return 0;
}

// c->stream pointed at another stream for a scope (every launcher and helper
// enqueues on c->stream)
struct StreamScope {
    cal_ctx* c;
    hipStream_t saved;
    StreamScope(cal_ctx* ctx, hipStream_t s) : c(ctx), saved(ctx->stream) { c->stream = s; }
    ~StreamScope() { c->stream = saved; }
};

// The GPU work of one job: the orthogonality-error Grams, the Ritz-vector
// apply (bound by the f64 matrix cores), the residual sums (bound by the
// gather), one reduction and copy, all on the context stream.  (A second
// stream for the Grams and residuals, and the apply in column chunks so a
// chunk's residuals overlap the next chunk's apply, measured slower: lap3d_215,
// 15 iterations, 130.5 outer-it/s on one stream, 125.3 on two, 117-120 with
// two chunks -- the residual blocks take LDS and CU slots from the apply's.)
// the orthogonality-error Gram chunks of an iteration with sk columns
// (compute_orth_err(Q(:,1:sk+1), s): Q(:,1:j-s-1)'Q(:,j-s:j) for j > s+1,
// else Q'Q - I; chunks of 128 x 16 columns, gram_async): wa, the chunks from
// result offset 2 sk on, the result size and the largest partial
static int diag_oe_layout(const LanczosState& L, int64_t n, int sk, std::vector<DiagJob::OeChunk>* oe,
                          size_t* dres_need, size_t* oe_part) {
    const int s = L.s, jq = sk + 1;
    const int wa = jq > s + 1 ? jq - s - 1 : s + 1;
    size_t off = (size_t)2 * sk, part = 0;
    if (oe) oe->clear();
    for (int a0 = 0; a0 < (L.oe_defer ? 0 : wa); a0 += 128)
        for (int b0 = 0; b0 < s + 1; b0 += 16) {
            const int na = std::min(128, wa - a0), nb = std::min(16, s + 1 - b0);
            const GramPlan pl = gram_plan(na, nb, n);
            if (oe) oe->push_back({a0, na, b0, nb, 16 * pl.nta, off});
            off += (size_t)pl.entries;
            part = std::max(part, (size_t)pl.blocks * pl.entries);
        }
    *dres_need = off;
    *oe_part = part;
    return wa;
}

// The job buffers sized once for the last iteration (each growth of a pinned
// buffer frees and allocates: a device synchronisation plus a pinned
// allocation, ~0.5 ms of idle GPU per growth in the early iterations)
static int diag_reserve(cal_ctx* c, LanczosState& L) {
    const int64_t n = c->A.n_local;
    const int skm = L.s * L.max_outer;
    size_t dres = 0, oe_part = 0;
    diag_oe_layout(L, n, skm, nullptr, &dres, &oe_part);
    const size_t din = (size_t)skm * skm + skm + 2 * (size_t)((skm + 1) / 2);
    const int nbp = spmv_resid_pair_multi_blocks(c);
    const int nbr = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256));
    const size_t dpart = (nbp > 0 ? (size_t)2 * skm * nbp : 0) + (size_t)2 * skm * nbr + oe_part;
    CAL_TRY(grow_pinned(c, &L.d_dres, &L.h_dres, &L.dres_cap, dres));
    CAL_TRY(grow_pinned(c, &L.d_din, &L.h_din, &L.din_cap, din));
    CAL_TRY(grow_pinned_dev(c, &L.d_dpart, &L.dpart_cap, dpart));
    return 0;
}

static int diag_launch(cal_ctx* c, LanczosState& L, DiagJob& J) {
    CAL_TRY(shared_refuses(c, "the Ritz residual"));
    const int s = L.s, sk = s * J.k;
    const int64_t n = c->A.n_local, ld = c->A.ld;
    const hipStream_t main = c->stream, aux = c->stream;
    if (L.dres_cap == 0) CAL_TRY(diag_reserve(c, L));
    size_t off = 0, oe_part = 0;
    J.wa = diag_oe_layout(L, n, sk, &J.oe, &off, &oe_part);
    const int jq = sk + 1;
    const int bcol = jq > s + 1 ? J.wa : 0;
    CAL_TRY(grow_pinned(c, &L.d_dres, &L.h_dres, &L.dres_cap, off));
    // the Ritz vectors (one column chunk; the chunked form is kept for the
    // pair grouping below)
    const bool mt = apply_mt_ok(sk, sk);
    const int nch = 1;
    const int cw = nch == 1 ? sk : ((sk + nch * 16 - 1) / (nch * 16)) * 16;
    auto chunk_of = [&](int col) { return std::min(nch - 1, col / cw); };
    // inputs: Vp, then the batched pairs grouped by chunk (Ritz value, column,
    // output slot), offsets per chunk
    const int nbp = spmv_resid_pair_multi_blocks(c);  // 0: no pair path (row kernel for every pair)
    const size_t o_lam = (size_t)sk * sk, o_col = o_lam + sk, o_out = o_col + (sk + 1) / 2;
    CAL_TRY(grow_pinned(c, &L.d_din, &L.h_din, &L.din_cap, o_out + (sk + 1) / 2));
    std::copy(J.V.begin(), J.V.end(), L.h_din);
    double* h_lam = L.h_din + o_lam;
    int* h_col = reinterpret_cast<int*>(L.h_din + o_col);
    int* h_out = reinterpret_cast<int*>(L.h_din + o_out);
    J.sep.clear();
    std::vector<int> cnt(nch + 1, 0);  // batched pairs per chunk, then prefix offsets
    for (int i = 0; i < sk; ++i) {
        if (nbp > 0 && J.pairs[i].ci < 0) cnt[chunk_of(J.pairs[i].cr) + 1]++;
        else J.sep.push_back(i);
    }
    for (int q = 0; q < nch; ++q) cnt[q + 1] += cnt[q];
    {
        std::vector<int> pos(cnt.begin(), cnt.end() - 1);
        for (int i = 0; i < sk; ++i) {
            const RitzPair& p = J.pairs[i];
            if (!(nbp > 0 && p.ci < 0)) continue;
            const int q = pos[chunk_of(p.cr)]++;
            h_lam[q] = p.lr;
            h_col[q] = p.cr;
            h_out[q] = i;
        }
    }
    CAL_HIP(c, hipMemcpyAsync(L.d_din, L.h_din, (o_out + (sk + 1) / 2) * sizeof(double), hipMemcpyHostToDevice,
                              main));
    // sized for the last iteration at once (each growth frees and zeroes)
    CAL_TRY(ensure_work(c, std::max(sk, s * L.max_outer), ld));
    double* X = work_col(c, 0) + c->A.lpad;
    const int nbr = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256));
    const bool batched = nbp > 0;
    const size_t sep0 = batched ? (size_t)2 * sk * nbp : 0;           // row-kernel partials
    const size_t oe0 = sep0 + (size_t)2 * std::max<size_t>(J.sep.size(), batched ? 0 : sk) * nbr;
    CAL_TRY(grow_pinned_dev(c, &L.d_dpart, &L.dpart_cap, oe0 + oe_part));
    if (J.evc.size() < (size_t)nch + 1) {
        const size_t old = J.evc.size();
        J.evc.resize(nch + 1, nullptr);
        for (size_t q = old; q < J.evc.size(); ++q) CAL_HIP(c, hipEventCreateWithFlags(&J.evc[q], hipEventDisableTiming));
    }
    // the aux stream starts behind everything on the context stream so far
    CAL_HIP(c, hipEventRecord(J.evc[nch], main));
    CAL_HIP(c, hipStreamWaitEvent(aux, J.evc[nch], 0));
    {
        StreamScope on_aux(c, aux);
        for (const auto& ch : J.oe) {
            Panel OA = panel(), OB = panel();
            panel_add(OA, L.col(ch.a0), ld, ch.na);
            panel_add(OB, L.col(bcol + ch.b0), ld, ch.nb);
            int ldc = 0;
            CAL_TRY(gram_async(c, n, OA, OB, L.d_dres + ch.off, L.h_dres + ch.off, &ldc, L.d_dpart + oe0));
        }
    }
    for (int q = 0; q < nch; ++q) {
        const int c0 = q * cw, c1 = q + 1 == nch ? sk : std::min(sk, c0 + cw);
        // X(:, c0:c1) = Q(:,1:sk) * Vp(:, c0:c1) (ca_lanczos.m:93)
        if (mt) {
            const int t = timer_begin(c, 2, 8.0 * n * (sk + (c1 - c0)));
            hipError_t e = launch_apply_mt(L.col(0), ld, L.d_din + (size_t)c0 * sk, sk, c1 - c0, X + (int64_t)c0 * ld,
                                           ld, n, main);
            timer_end(c, t);
            if (e != hipSuccess) return hip_fail(c, e, "launch_apply_mt (Ritz vectors)");
        } else {  // sk > 1280: the generic apply in column chunks
            Panel Qp = panel();
            panel_add(Qp, L.col(0), ld, sk);
            CAL_TRY(apply_dev(c, n, Qp, L.d_din, sk, panel_out(X, ld, sk)));
        }
        CAL_HIP(c, hipEventRecord(J.evc[q], main));
        const int npq = cnt[q + 1] - cnt[q];
        if (npq == 0) continue;
        CAL_HIP(c, hipStreamWaitEvent(aux, J.evc[q], 0));
        StreamScope on_aux(c, aux);
        for (int i = cnt[q]; i < cnt[q + 1]; ++i) CAL_TRY(halo_exchange(c, X + (int64_t)h_col[i] * ld));
        // ||A x - l x||^2, ||l x||^2 per pair (ca_lanczos.m:94): entry 2i + e
        const int t = timer_begin(c, 3);
        CAL_TRY(spmv_resid_pair_multi_dev(c, X, ld, reinterpret_cast<const int*>(L.d_din + o_col) + cnt[q],
                                          L.d_din + o_lam + cnt[q], reinterpret_cast<const int*>(L.d_din + o_out) + cnt[q],
                                          npq, L.d_dpart, nbp));
        timer_end(c, t);
    }
    CAL_HIP(c, hipStreamWaitEvent(aux, J.evc[nch - 1], 0));  // every chunk of X written
    {
        StreamScope on_aux(c, aux);
        for (size_t q = 0; q < J.sep.size(); ++q) {
            const RitzPair& p = J.pairs[J.sep[q]];
            double* xr = X + (int64_t)p.cr * ld;
            double* xi = p.ci >= 0 ? X + (int64_t)p.ci * ld : nullptr;
            CAL_TRY(halo_exchange(c, xr));
            if (xi) CAL_TRY(halo_exchange(c, xi));
            SpmvArgs a{};
            a.rowptr = c->A.rowptr + c->A.ext_off;  // local rows of a stored slab
            a.col = c->A.col;
            a.val = c->A.val;
            a.x = xr;
            // no pair path: every pair entry-major at stride nbr (one reduction)
            double* part = L.d_dpart + sep0 + (batched ? q : (size_t)J.sep[q]) * 2 * nbr;
            const int t = timer_begin(c, 3);
            CAL_HIP(c, launch_spmv_resid(a, xi, p.lr, p.li, n, part, nbr, c->stream));
            timer_end(c, t);
        }
        if (batched) {
            if (cnt[nch] > 0) CAL_HIP_OTHER(c, launch_reduce(L.d_dpart, nbp, 2 * sk, L.d_dres, c->stream));
            for (size_t q = 0; q < J.sep.size(); ++q)
                CAL_HIP_OTHER(c, launch_reduce(L.d_dpart + sep0 + q * 2 * nbr, nbr, 2, L.d_dres + 2 * J.sep[q], c->stream));
        } else {
            CAL_HIP_OTHER(c, launch_reduce(L.d_dpart, nbr, 2 * sk, L.d_dres, c->stream));
        }
        CAL_TRY(allreduce_sum(c, L.d_dres, 2 * sk));
        CAL_HIP(c, hipMemcpyAsync(L.h_dres, L.d_dres, 2 * sk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (!J.ev) CAL_HIP(c, hipEventCreateWithFlags(&J.ev, hipEventDisableTiming));
        CAL_HIP(c, hipEventRecord(J.ev, c->stream));
    }
    CAL_HIP(c, hipStreamWaitEvent(main, J.ev, 0));
    return 0;
}

static int diag_collect(cal_ctx* c, LanczosState& L, DiagJob& J) {
    const int s = L.s, k = J.k, sk = s * k;
    CAL_HIP(c, hipEventSynchronize(J.ev));
    std::vector<double> rn(sk);
    for (int i = 0; i < sk; ++i) rn[i] = std::sqrt(L.h_dres[2 * i]) / std::sqrt(L.h_dres[2 * i + 1]);
    double oe = 0.0;
    const bool off_diag = sk + 1 > s + 1;
    for (const auto& ch : J.oe)
        for (int jj = 0; jj < ch.nb; ++jj)
            for (int ii = 0; ii < ch.na; ++ii) {
                double g = L.h_dres[ch.off + ii + (size_t)jj * ch.ldc];
                if (!off_diag && ch.a0 + ii == ch.b0 + jj) g -= 1.0;
                oe = std::max(oe, std::fabs(g));
            }
    if ((int)L.rn.size() < k) L.rn.resize(k);
    if ((int)L.oe.size() < k) L.oe.resize(k, 0.0);
    L.rn[k - 1] = rn;
    if (L.oe_defer) L.oe_pend.push_back(k);
    else L.oe[k - 1] = oe;
    J.k = 0;
    return 0;
}

// The deferred orthogonality errors (compute_orth_err, ca_lanczos.m:99-107)
// of every pending iteration k from one Gram of Q(:,1:sK+1), K the last of
// them: k_gram_wide reads Q once (the per-iteration Grams re-read
// Q(:,1:s(k-1)) every iteration: 77 GB over 15 iterations at n = 9.94 M).
// Entry (i, j), i < j, is the same dot product the per-iteration Gram
// forms (another summation order, i.e. the same value to rounding).
static int oe_flush(cal_ctx* c, LanczosState& L) {
    if (L.oe_pend.empty()) return 0;
    const int s = L.s;
    const int K = *std::max_element(L.oe_pend.begin(), L.oe_pend.end());
    const int w = s * K + 1;
    const int64_t n = c->A.n_local;
    const int nent = gram_wide_entries(w), nb = gram_wide_blocks(n);
    CAL_TRY(grow_pinned_dev(c, &L.d_dpart, &L.dpart_cap, (size_t)nent * nb));
    CAL_TRY(grow_pinned(c, &L.d_oe, &L.h_oe, &L.oe_cap, (size_t)nent));
    CAL_HIP(c, launch_gram_wide(L.col(0), L.ld, w, n, L.d_dpart, c->stream));
    CAL_HIP_OTHER(c, launch_reduce(L.d_dpart, nb, nent, L.d_oe, c->stream));
    CAL_TRY(allreduce_sum(c, L.d_oe, nent));
    CAL_HIP(c, hipMemcpyAsync(L.h_oe, L.d_oe, (size_t)nent * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<double> G((size_t)w * w, 0.0);  // upper tile pairs; diagonal tiles both triangles
    std::vector<char> have((size_t)w * w, 0);
    for (int e = 0; e < nent; ++e) {
        int i, j;
        gram_wide_entry(w, e, &i, &j);
        if (i < w && j < w) {
            G[i + (size_t)j * w] = L.h_oe[e];
            have[i + (size_t)j * w] = 1;
        }
    }
    for (const int k : L.oe_pend) {
        const int jq = s * k + 1;  // Q(:,1:jq)
        double oe = 0.0;
        if (jq > s + 1) {  // max |Q(:,1:jq-s-1)' Q(:,jq-s:jq)|
            for (int j = jq - s - 1; j < jq; ++j)
                for (int i = 0; i < jq - s - 1; ++i) oe = std::max(oe, std::fabs(G[i + (size_t)j * w]));
        } else {  // max |Q(:,1:jq)'Q(:,1:jq) - I|
            for (int j = 0; j < jq; ++j)
                for (int i = 0; i < jq; ++i) {
                    const size_t e = have[i + (size_t)j * w] ? i + (size_t)j * w : j + (size_t)i * w;
                    oe = std::max(oe, std::fabs(G[e] - (i == j ? 1.0 : 0.0)));
                }
        }
        if ((int)L.oe.size() < k) L.oe.resize(k, 0.0);
        L.oe[k - 1] = oe;
    }
    L.oe_pend.clear();
    return 0;
}

// everything still deferred: the stream is drained
static int diag_flush(cal_ctx* c, LanczosState& L) {
    if (L.pending.k) CAL_TRY(diag_collect(c, L, L.pending));
    CAL_TRY(diag_join(c, L.ready));
    if (L.ready.k) {
        std::swap(L.pending, L.ready);
        CAL_TRY(diag_launch(c, L, L.pending));
        CAL_TRY(diag_collect(c, L, L.pending));
    }
    return oe_flush(c, L);
}

static void diag_free(LanczosState& L) {
    for (DiagJob* J : {&L.ready, &L.pending}) {
        if (J->eig.valid()) J->eig.wait();
        if (J->ev) hipEventDestroy(J->ev);
        for (hipEvent_t e : J->evc) hipEventDestroy(e);
    }
    if (L.d_dpart) hipFree(L.d_dpart);
    if (L.d_dres) hipFree(L.d_dres);
    if (L.h_dres) hipHostFree(L.h_dres);
    if (L.d_din) hipFree(L.d_din);
    if (L.h_din) hipHostFree(L.h_din);
    if (L.d_oe) hipFree(L.d_oe);
    if (L.h_oe) hipHostFree(L.h_oe);
}

// ---- T extension (ca_lanczos.m:176-223) -----------------------------------
static int extend_T_first(cal_ctx* c, LanczosState& L, const std::vector<double>& Rk) {
    const int s = L.s, s1 = s + 1;
    // T = Rk*Bk/Rk(1:s,1:s)   ((s+1) x s)
    std::vector<double> RB((size_t)s1 * s), R11((size_t)s * s);
    dense::matmul(s1, s1, s, Rk.data(), s1, L.Bk.data(), s1, RB.data(), s1);
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i) R11[i + (size_t)j * s] = Rk[i + (size_t)j * s1];
    if (R11[(s - 1) + (size_t)(s - 1) * s] == 0.0) {
        L.breakdown = true;
        return CAL_WARN_BREAKDOWN;
    }
    dense::rdiv_upper(s1, s, RB.data(), s1, R11.data(), s);
    for (const double v : RB)
        if (!std::isfinite(v)) {  // the reference divides on (Inf/NaN in T, a MATLAB warning): flagged here
            L.breakdown = true;
            return CAL_WARN_BREAKDOWN;
        }
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s1; ++i) L.T[i + (size_t)j * L.Tld] = RB[i + (size_t)j * s1];
    L.b.assign(1, RB[s + (size_t)(s - 1) * s1]);  // b(1) = T(s+1,s)
    return 0;
}

// Tk (s x s) and the next beta of one block (ca_lanczos.m:200-214) from the
// block's projection coefficients Rkk_s ((s+1) x s) and R factor Rk_s (s x s).
static int block_T(const std::vector<double>& Bk, int s, double bprev, const std::vector<double>& Rkk_s,
                   const std::vector<double>& Rk_s, std::vector<double>& Tk, double* bnew) {
    const int s1 = s + 1;
    // Rk = [e1, [Rkk_s(s+1,1:s); Rk_s]]  ((s+1) x (s+1))
    std::vector<double> Rk((size_t)s1 * s1, 0.0);
    Rk[0] = 1.0;
    for (int j = 1; j <= s; ++j) {
        Rk[0 + (size_t)j * s1] = Rkk_s[s + (size_t)(j - 1) * s1];
        for (int i = 1; i <= s; ++i) Rk[i + (size_t)j * s1] = Rk_s[(i - 1) + (size_t)(j - 1) * s];
    }
    std::vector<double> R11((size_t)s * s), Rkk11((size_t)s * s, 0.0);
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i) R11[i + (size_t)j * s] = Rk[i + (size_t)j * s1];
    // Rkk = [zeros(s,1), Rkk_s(1:s,:)] -> Rkk(1:s,1:s) = [0, Rkk_s(1:s,1:s-1)]
    for (int j = 1; j < s; ++j)
        for (int i = 0; i < s; ++i) Rkk11[i + (size_t)j * s] = Rkk_s[i + (size_t)(j - 1) * s1];
    const double rho = Rk[s + (size_t)s * s1];
    const double rho_t = Rk[(s - 1) + (size_t)(s - 1) * s1];
    const double bk = Bk[s + (size_t)(s - 1) * s1];
    if (rho_t == 0.0) return CAL_WARN_BREAKDOWN;
    // term1 = R11*Bk(1:s,:)/R11
    std::vector<double> B11((size_t)s * s), t1((size_t)s * s), t3((size_t)s * s, 0.0);
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i) B11[i + (size_t)j * s] = Bk[i + (size_t)j * s1];
    dense::matmul(s, s, s, R11.data(), s, B11.data(), s, t1.data(), s);
    dense::rdiv_upper(s, s, t1.data(), s, R11.data(), s);
    // term2 = ((bk/rho_t)*zk)*es'  (last column only)
    const double f = bk / rho_t;
    // term3 = (((b(k-1)*e1)*es')*Rkk(1:s,1:s))/R11  (first row only)
    for (int j = 0; j < s; ++j) t3[0 + (size_t)j * s] = bprev * Rkk11[(s - 1) + (size_t)j * s];
    dense::rdiv_upper(s, s, t3.data(), s, R11.data(), s);
    Tk.assign((size_t)s * s, 0.0);
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i) {
            double v = t1[i + (size_t)j * s];
            if (j == s - 1) v = v + f * Rk[i + (size_t)s * s1];
            v = v - t3[i + (size_t)j * s];
            Tk[i + (size_t)j * s] = v;
        }
    *bnew = bk * (rho / rho_t);  // :214
    return 0;
}

// place block Tk at column m0 of T with the couplings b(k-1) and b(k) (:217-223)
static void place_T(LanczosState& L, int m0, const std::vector<double>& Tk, double bprev, double bnew) {
    const int s = L.s;
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i) L.T[(m0 + i) + (size_t)(m0 + j) * L.Tld] = Tk[i + (size_t)j * s];
    L.T[(m0 - 1) + (size_t)m0 * L.Tld] = bprev;            // T12
    L.T[m0 + (size_t)(m0 - 1) * L.Tld] = bprev;            // T21
    L.T[(m0 + s) + (size_t)(m0 + s - 1) * L.Tld] = bnew;   // T32
}

static int extend_T(cal_ctx* c, LanczosState& L, const std::vector<double>& Rkk_s, const std::vector<double>& Rk_s) {
    (void)c;
    const int k = L.k;
    std::vector<double> Tk;
    double bnew = 0.0;
    const double bprev = L.b[k - 2];
    bool finite = true;
    const int bt = block_T(L.Bk, L.s, bprev, Rkk_s, Rk_s, Tk, &bnew);
    for (const double v : Tk) finite = finite && std::isfinite(v);
    if (bt != 0 || !finite || !std::isfinite(bnew)) {  // non-finite: the reference's Inf/NaN T, flagged
        L.breakdown = true;
        return CAL_WARN_BREAKDOWN;
    }
    L.b.push_back(bnew);
    place_T(L, L.s * (k - 1), Tk, bprev, bnew);
    return 0;
}

#ifdef CAL_TEST_HOOKS  // the test build only (csrc/Makefile libcalanczos_testhooks.so)
// TEST HOOK: R of the last ca_lanczos run's first block ((s+1) x (s+1),
// column-major); returns s + 1, or a negative status when there is none.
extern "C" int cal_test_first_block_R(cal_ctx* c, double* R, int cap) {
    if (!c || !R) return CAL_ERR_ARG;
    const size_t m2 = c->test_R1.size();
    int m = 0;
    while ((size_t)(m + 1) * (m + 1) <= m2) ++m;
    if (m == 0 || (size_t)m * m != m2 || (size_t)cap < m2) return CAL_ERR_ARG;
    std::copy(c->test_R1.begin(), c->test_R1.end(), R);
    return m;
}

// TEST HOOK (CAL_TEST_EIG_PAIR set; tests/test_gpu_parity.py): no converged
// complex Ritz pair arises on the inputs the tests can reach, so the test
// rewrites every all-real eig(T) the way tests/test_oracle.py's hook rewrites
// the oracle's: the two most converged eigenpairs (smallest |V(sk,i)|, unit
// vectors) become one conjugate pair 0.5 (w_i + w_j) +- 1e-3 i with vectors
// (v_i +- i v_j) / sqrt 2.  In this layout the pair is stored as (Re, Im)
// columns at min(i,j), min(i,j)+1; the other columns keep their order.
static void test_eig_pair(int sk, std::vector<double>& wr, std::vector<double>& wi, std::vector<double>& V) {
    if (sk < 2) return;
    for (int j = 0; j < sk; ++j)
        if (wi[j] != 0.0) return;
    std::vector<int> idx(sk);
    for (int j = 0; j < sk; ++j) idx[j] = j;
    auto last = [&](int j) {
        double nv = 0.0;
        for (int i = 0; i < sk; ++i) nv += V[i + (size_t)j * sk] * V[i + (size_t)j * sk];
        return std::fabs(V[(sk - 1) + (size_t)j * sk]) / std::sqrt(nv);
    };
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return last(a) < last(b); });
    const int lo = std::min(idx[0], idx[1]), hi = std::max(idx[0], idx[1]);
    const int i0 = idx[0], j0 = idx[1];
    const double wm = 0.5 * (wr[i0] + wr[j0]), r2 = 1.0 / std::sqrt(2.0);
    double ni = 0.0, nj = 0.0;  // unit v_i, v_j (hqr2's vectors are not normalised)
    for (int r = 0; r < sk; ++r) {
        ni += V[r + (size_t)i0 * sk] * V[r + (size_t)i0 * sk];
        nj += V[r + (size_t)j0 * sk] * V[r + (size_t)j0 * sk];
    }
    ni = r2 / std::sqrt(ni);
    nj = r2 / std::sqrt(nj);
    std::vector<double> re(sk), im(sk);
    for (int r = 0; r < sk; ++r) {
        re[r] = V[r + (size_t)i0 * sk] * ni;
        im[r] = V[r + (size_t)j0 * sk] * nj;
    }
    std::vector<double> wr2, wi2, V2;
    wr2.reserve(sk);
    wi2.reserve(sk);
    V2.reserve((size_t)sk * sk);
    for (int j = 0; j < sk; ++j) {
        if (j == hi) continue;
        if (j == lo) {
            wr2.push_back(wm);
            wi2.push_back(1.0e-3);
            V2.insert(V2.end(), re.begin(), re.end());
            wr2.push_back(wm);
            wi2.push_back(-1.0e-3);
            V2.insert(V2.end(), im.begin(), im.end());
            continue;
        }
        wr2.push_back(wr[j]);
        wi2.push_back(0.0);
        V2.insert(V2.end(), V.begin() + (size_t)j * sk, V.begin() + (size_t)(j + 1) * sk);
    }
    wr.swap(wr2);
    wi.swap(wi2);
    V.swap(V2);
}
#endif

// selective (ca_lanczos.m:321-340): the Ritz pairs of T(1:sk,1:sk) with
// b(k)|Vp(sk,i)| < normest(A) sqrt(eps) (unit-norm eigenvectors, as MATLAB's
// eig returns them); when their count grows, QR = normalize(Q(:,1:sk) Vp(:,conv)).
// A converged complex-conjugate pair (the test is the same for both) enters
// as Q Re(v), Q Im(v): the real span of the reference's complex QR columns
// Q v, Q conj(v), so the count and the projections are the reference's.
static int selective_update(cal_ctx* c, LanczosState& L) {
    const int s = L.s, k = L.k, sk = s * k;
    const int64_t n = c->A.n_local, ld = c->A.ld;
    std::vector<double> Tk((size_t)sk * sk), wr(sk), wi(sk), V((size_t)sk * sk);
    for (int j = 0; j < sk; ++j)
        for (int i = 0; i < sk; ++i) Tk[i + (size_t)j * sk] = L.T[i + (size_t)j * L.Tld];
    if (cal_eig(sk, Tk.data(), sk, wr.data(), wi.data(), V.data()) != 0)
        return set_error(c, CAL_ERR_NUMERIC, "eig(T) did not converge");
#ifdef CAL_TEST_HOOKS
    if (std::getenv("CAL_TEST_EIG_PAIR")) test_eig_pair(sk, wr, wi, V);
#endif
    const double thresh = L.norm_A * std::sqrt(std::numeric_limits<double>::epsilon());
    const double bk = L.b.back();
    std::vector<int> conv;  // columns of V: real pairs, or (Re v, Im v) of a complex pair
    for (int j = 0; j < sk; ++j) {
        if (wi[j] != 0.0) {  // V(:,j) + i V(:,j+1) belongs to wr(j) + i wi(j), wi(j) > 0, and its conjugate
            double nv = 0.0;
            for (int i = 0; i < sk; ++i)
                nv += V[i + (size_t)j * sk] * V[i + (size_t)j * sk] + V[i + (size_t)(j + 1) * sk] * V[i + (size_t)(j + 1) * sk];
            nv = std::sqrt(nv);
            const double last = std::hypot(V[(sk - 1) + (size_t)j * sk], V[(sk - 1) + (size_t)(j + 1) * sk]);
            if (bk * (last / nv) < thresh) {
                conv.push_back(j);
                conv.push_back(j + 1);
            }
            ++j;
            continue;
        }
        double nv = 0.0;
        for (int i = 0; i < sk; ++i) nv += V[i + (size_t)j * sk] * V[i + (size_t)j * sk];
        nv = std::sqrt(nv);
        if (bk * std::fabs(V[(sk - 1) + (size_t)j * sk] / nv) < thresh) conv.push_back(j);
    }
    if ((int)conv.size() <= L.nritz) return 0;
    L.info.n_orth_breaks++;
    const int nr = (int)conv.size();
    L.info.n_ritz_complex = 0;
    for (int q : conv)
        if (wi[q] != 0.0) L.info.n_ritz_complex++;  // both members of a pair carry +-Im
    if (nr > L.qr_cap) {
        if (L.dQR) CAL_HIP(c, hipFree(L.dQR));
        if (L.dQRy) CAL_HIP(c, hipFree(L.dQRy));
        L.dQR = L.dQRy = nullptr;
        L.qr_cap = std::max(nr, 2 * s);
        CAL_HIP(c, hipMalloc((void**)&L.dQR, (size_t)L.qr_cap * ld * sizeof(double)));
        CAL_HIP(c, hipMalloc((void**)&L.dQRy, (size_t)L.qr_cap * ld * sizeof(double)));
    }
    std::vector<double> M((size_t)sk * nr);
    for (int q = 0; q < nr; ++q)
        for (int i = 0; i < sk; ++i) M[i + (size_t)q * sk] = V[i + (size_t)conv[q] * sk];
    Panel Qp = panel();
    panel_add(Qp, L.col(0), ld, sk);
    PanelOut Y = panel_out(L.dQRy + L.lpad, ld, nr);
    CAL_TRY(apply_host(c, n, Qp, M.data(), nr, &Y, nullptr, 0, nullptr));  // y = Q(:,1:ks)*Vp(:,i)
    // halo columns of the Ritz vectors are never read (they only enter Grams
    // and row-local applies), so no exchange is needed
    CAL_TRY(normalize_wide_dev(c, n, ld, L.dQRy + L.lpad, nr, L.dQR + L.lpad, L.dQRy + L.lpad));
    L.nritz = nr;
    L.info.n_ritz_locked = nr;
    return 0;
}

// periodic (ca_lanczos.m:438-453): advance the omega estimate; when it
// reaches sqrt(eps), reorthogonalise Q(:,(k-1)s+1:ks+1) against
// Q(:,1:(k-1)s) (the new columns do not feed back into T).
static int periodic_update(cal_ctx* c, LanczosState& L) {
    const int s = L.s, k = L.k, sk = s * k;
    const int64_t n = c->A.n_local, ld = c->A.ld;
    std::vector<double> alpha(sk), beta(sk);
    for (int i = 0; i < sk; ++i) {
        alpha[i] = L.T[i + (size_t)i * L.Tld];        // diag(T,0)
        beta[i] = L.T[(i + 1) + (size_t)i * L.Tld];   // diag(T,-1)
    }
    update_omega(L, alpha, beta);
    double err = 0.0;
    for (int i = 1; i <= s; ++i) {
        const int row = (k - 1) * s + i;  // omega((k-1)s+i+1, 1:(k-1)s+i), 0-based row
        double row_err = 0.0;
        for (int j = 0; j < row; ++j) row_err = std::max(row_err, std::fabs(L.omega[row + (size_t)j * L.om_n]));
        if (row_err > err) err = row_err;
    }
    if (!(err >= std::sqrt(std::numeric_limits<double>::epsilon()))) return 0;
    L.info.n_orth_breaks++;
    const int w = (k - 1) * s, m = s + 1;
    CAL_TRY(ensure_work(c, m, ld));
    double* dX = work_col(c, 0) + c->A.lpad;
    CAL_HIP(c, copy_cols(c, dX, L.col(w), ld, n, m));
    Panel Qp = panel(), X = panel();
    if (w > 0) panel_add(Qp, L.col(0), ld, w);
    panel_add(X, dX, ld, m);
    std::vector<double> Rq((size_t)std::max(w, 1) * m), R((size_t)m * m);
    PNResult res;
    CAL_TRY(project_and_normalize_dev(c, n, Qp, X, true, panel_out(L.col(w), ld, m), Rq.data(), R.data(), &res));
    reset_omega(L);
    return 0;
}

int lanczos_step(cal_ctx* c, int diagnostics) {
    LanczosState& L = *c->lz;
    if (L.k >= L.max_outer) return set_error(c, CAL_ERR_ARG, "lanczos_step: max_outer iterations reached");
    if (L.breakdown) return set_error(c, CAL_WARN_BREAKDOWN, "lanczos_step: breakdown already hit");
    const double t0 = now_ms();
    const int s = L.s;
    const int64_t n = c->A.n_local, ld = L.ld;
    L.k += 1;
    const int k = L.k;
    char range[48];
    std::snprintf(range, sizeof range, "ca_lanczos outer k=%d", k);
    const RoctxRange marker(range);  // rocprofv3 --marker-trace splits traces by step
    const double* q = L.col((k - 1) * s);  // ca_lanczos.m:171 (k=1: q itself)
    auto Vc = [&](int j) { return L.vcolumn(j, k & 1); };
    if (!L.powers_ready) CAL_TRY(enqueue_powers(c, L, k));
    L.powers_ready = false;
    // Prefetch: the matrix powers of step k+1 need only Q's last column
    // (stream-ordered after this step's pass B) and the fixed shifts, so they
    // are enqueued (into the other V buffer) before the host waits for this
    // step's R: the GPU runs them while the host extends T and returns.
    const bool prefetch = L.mode == 0 && !L.restart_inner && k + 1 <= L.max_outer;
    c->orth_redone = false;
    if (prefetch)
        c->pre_wait = [c, &L, k]() {
            const int st = enqueue_powers(c, L, k + 1);
            if (st == 0) L.powers_ready = true;
            return st;
        };
    struct ClearHook {
        cal_ctx* c;
        ~ClearHook() { c->pre_wait = nullptr; }
    } clear_hook{c};
    int status = 0;
    if (k == 1) {
        Panel X = panel();
        panel_add(X, q, ld, 1);
        panel_add(X, Vc(1), ld, s);
        PanelOut Qo = panel_out(L.col(0), ld, s + 1);
        std::vector<double> Rk((size_t)(s + 1) * (s + 1));
        int rank = 0;
        bool sh = false;
        CAL_TRY(normalize_dev(c, n, X, Qo, Rk.data(), 1.0e-8, &rank, &sh));
        if (rank < s + 1) L.info.n_rank_deficient++;
#ifdef CAL_TEST_HOOKS
        c->test_R1 = Rk;
#endif
        if (L.restart_inner) {
            // [Q(:,1:s+1),R_] = projectAndNormalize({Q_conv},Q_,true) (restarted_ca_lanczos.m:291)
            CAL_TRY(ensure_work(c, s + 1, ld));
            double* dW = work_col(c, 0) + c->A.lpad;
            CAL_HIP(c, copy_cols(c, dW, L.col(0), ld, n, s + 1));
            Panel Qc = panel(), Xw = panel();
            if (L.next > 0) panel_add(Qc, L.dExt, ld, L.next);
            panel_add(Xw, dW, ld, s + 1);
            std::vector<double> Rq((size_t)std::max(L.next, 1) * (s + 1)), R_((size_t)(s + 1) * (s + 1));
            PNResult r_;
            CAL_TRY(project_and_normalize_dev(c, n, Qc, Xw, true, Qo, Rq.data(), R_.data(), &r_));
        }
        L.reorth.push_back(0);
        status = extend_T_first(c, L, Rk);
    } else {
        Panel Qp = panel(), X = panel();
        panel_add(Qp, L.col((k - 2) * s), ld, s + 1);
        panel_add(X, Vc(1), ld, s);
        PanelOut Qo = panel_out(L.col((k - 1) * s + 1), ld, s);
        std::vector<double> Rq((size_t)(s + 1) * s), R((size_t)s * s);
        PNResult res;
        const bool ext_local = L.restart_inner && L.mode == 0 && L.next > 0;
        if ((L.mode == 3 && L.nritz > 0) || ext_local) {
            // projectAndNormalize({Q block, QR(:,1:nritz)}, V(:,2:s+1)) (ca_lanczos.m:287), or
            // against {Q block, Q_conv} (restarted_ca_lanczos.m:301)
            CAL_TRY(ensure_work(c, s, ld));
            std::vector<double*> dQ{L.col((k - 2) * s), ext_local ? L.dExt : L.dQR + L.lpad};
            const int widths[2] = {s + 1, ext_local ? L.next : L.nritz};
            std::vector<std::vector<double>> RZ;
            bool ro = false;
            int rk = s;
            CAL_TRY(project_and_normalize_blocks_dev(c, n, ld, 2, dQ, widths, s, Vc(1), true,
                                                     work_col(c, 0) + c->A.lpad, Qo, RZ, R.data(), &ro, &rk));
            Rq = RZ[0];
            res.reorth = ro;
            res.rank = rk;
        } else {
            // 'full' (ca_lanczos.m:197): this block's pass B also forms the
            // projection's Gram [Q(:,1:(k-1)s+1) | Q_new]' Q_new below, reading
            // only Q(:,1:(k-2)s) beyond its own columns (k_passb_wide)
            if (L.full && !L.restart_inner && k >= 3 && !test_switch("CAL_TEST_PASSB_WIDE_OFF")) {
                c->pbw.want = true;
                c->pbw.qold = panel();
                panel_add(c->pbw.qold, L.col(0), ld, (k - 2) * s);
            }
            c->sweep_x_fresh = true;  // X = V(:,2:s+1), the powers just written
            const int st = project_and_normalize_dev(c, n, Qp, X, true, Qo, Rq.data(), R.data(), &res);
            c->sweep_x_fresh = false;
            c->pbw.want = false;
            CAL_TRY(st);
        }
        L.reorth.push_back(res.reorth ? 1 : 0);
        if (res.reorth) L.info.n_reorth++;
        if (res.reorth && res.rank < s) L.info.n_rank_deficient++;
        if (L.full && L.restart_inner) {
            // Q(:,(k-1)s+2:ks+1) = projectAndNormalize({Q_conv,Q(:,1:(k-2)*s)},Q_,true)
            // (restarted_ca_lanczos.m:309)
            CAL_TRY(ensure_work(c, 2 * s, ld));
            double* dW = work_col(c, 0) + c->A.lpad;
            double* dY = work_col(c, s) + c->A.lpad;
            CAL_HIP(c, copy_cols(c, dW, L.col((k - 1) * s + 1), ld, n, s));
            std::vector<double*> dQ{L.dExt ? L.dExt : L.col(0), L.col(0)};
            const int widths[2] = {L.next, (k - 2) * s};
            std::vector<std::vector<double>> RZ;
            std::vector<double> R2((size_t)s * s);
            bool ro = false;
            int rk = s;
            CAL_TRY(project_and_normalize_blocks_dev(c, n, ld, 2, dQ, widths, s, dW, true, dY, Qo, RZ, R2.data(),
                                                     &ro, &rk));
        } else if (L.full) {  // ca_lanczos.m:197
            Panel Qall = panel(), Xn = panel();
            const int wall = (k - 1) * s + 1;
            panel_add(Qall, L.col(0), ld, wall);
            panel_add(Xn, L.col((k - 1) * s + 1), ld, s);
            std::vector<double> Rq2((size_t)wall * s), R2((size_t)s * s);
            PNResult res2;
            std::vector<double> G1;
            if (c->pbw.ready) {
                // [Qp | Q_new | Qold]' Q_new (k_passb_wide's order) -> [Qall | Q_new]' Q_new
                CAL_HIP(c, hipEventSynchronize(c->pbw.ev));
                const int wold = c->pbw.qold.total, wp = wall + s, lda = 16 * c->pbw.ntw;
                G1.assign((size_t)wp * s, 0.0);
                for (int j = 0; j < s; ++j)
                    for (int a = 0; a < wold + 17; ++a)
                        G1[(a < 17 ? wold + a : a - 17) + (size_t)j * wp] = c->pbw.h[a + (size_t)j * lda];
            }
            c->pbw.ready = false;
            CAL_TRY(project_and_normalize_dev(c, n, Qall, Xn, true, Qo, Rq2.data(), R2.data(), &res2,
                                              G1.empty() ? nullptr : G1.data()));
        }
        status = extend_T(c, L, Rq, R);
    }
    // a block redone on the host path rewrote q after the prefetched powers read it
    if (c->orth_redone && L.powers_ready) CAL_TRY(enqueue_powers(c, L, k + 1));
    if (status == CAL_WARN_BREAKDOWN) {
        L.info.breakdown = 1;
        return set_error(c, CAL_WARN_BREAKDOWN, "CA-Lanczos breakdown: rho_t = Rk(s,s) = 0");
    }
    // deferred diagnostics (see diag_prepare): step k-2's results are in (the
    // wait for this block's R passed their event); step k-1's kernels go on
    // the stream before periodic_update rewrites Q(:,(k-1)s+1:ks+1)
    double td = now_ms();
    if (L.pending.k) CAL_TRY(diag_collect(c, L, L.pending));
    CAL_TRY(diag_join(c, L.ready));
    if (L.ready.k) {
        std::swap(L.pending, L.ready);
        CAL_TRY(diag_launch(c, L, L.pending));
    }
    double tdiag = now_ms() - td;
    if (L.mode == 2) CAL_TRY(periodic_update(c, L));
    if (L.mode == 3) CAL_TRY(selective_update(c, L));
    td = now_ms();
    if (diagnostics) {
        CAL_TRY(diag_prepare(c, L, L.ready));  // eig(T_k) on a host thread, GPU busy
        if (k == L.max_outer) CAL_TRY(diag_flush(c, L));
    }
    const double t2 = now_ms();
    tdiag += t2 - td;
    L.info.loop_ms += t2 - t0;
    L.info.diag_ms += tdiag;
    L.info.t = k;
    return 0;
}

}  // namespace cal

using namespace cal;

extern "C" {

void cal_lanczos_free_state(cal_ctx* c) {
    if (!c || !c->lz) return;
    if (c->lz->dQ) hipFree(c->lz->dQ);
    if (c->lz->dV) hipFree(c->lz->dV);
    if (c->lz->dQR) hipFree(c->lz->dQR);
    if (c->lz->dQRy) hipFree(c->lz->dQRy);
    diag_free(*c->lz);
    delete c->lz;
    c->lz = nullptr;
}

}  // extern "C"

namespace cal {

int lanczos_begin(cal_ctx* c, const LanczosBegin& in, int s, int max_outer, const char* basis, const char* orth) {
    if (!c) return CAL_ERR_ARG;
    if (!c->has_A) return set_error(c, CAL_ERR_NOMATRIX, "no matrix set on the context");
    const bool have_r = in.r_host || in.r_dev;
    if (!have_r || s < 1 || s > kMaxS || max_outer < 1 || !basis)
        return set_error(c, CAL_ERR_ARG, "cal_lanczos_begin: need r, 1 <= s <= 31, max_outer >= 1");
    std::string o = orth ? orth : "local", b = basis;
    for (auto& ch : o) ch = (char)tolower(ch);
    for (auto& ch : b) ch = (char)tolower(ch);
    if (o != "local" && o != "full" && o != "periodic" && o != "selective")
        return set_error(c, CAL_ERR_ARG, "ca_lanczos.m: Invalid option value for orth: " + o);
    if (b != "monomial" && b != "newton") return set_error(c, CAL_ERR_ARG, "ERROR: Unknown basis type: " + b);
    if (in.shifts && in.nshifts < s) return set_error(c, CAL_ERR_ARG, "lanczos_begin: fewer than s Newton shifts");
    // normest: refused before the previous run's state is touched
    if (o == "periodic" || o == "selective") CAL_TRY(shared_refuses(c, ("orth = '" + o + "' (normest)").c_str()));
    hipSetDevice(c->device);
    // the previous run's Q / V buffers, kept when the shapes match
    double *keepQ = nullptr, *keepV = nullptr;
    if (in.reuse && c->lz && c->lz->s == s && c->lz->max_outer == max_outer && c->lz->ld == c->A.ld &&
        c->lz->lpad == c->A.lpad && c->lz->n == c->A.n_local && c->lz->dQ && c->lz->dV) {
        std::swap(keepQ, c->lz->dQ);
        std::swap(keepV, c->lz->dV);
    }
    cal_lanczos_free_state(c);
#ifdef CAL_TEST_HOOKS
    c->test_R1.clear();
#endif
    LanczosState* L = new LanczosState();
    c->lz = L;
    L->s = s;
    L->max_outer = max_outer;
    L->newton = b == "newton";
    L->full = o == "full";
    L->mode = o == "local" ? 0 : (o == "full" ? 1 : (o == "periodic" ? 2 : 3));
    L->n = c->A.n_local;
    L->ld = c->A.ld;
    L->lpad = c->A.lpad;
    L->info.s = s;
    const size_t qcols = (size_t)s * max_outer + 1;
    if (keepQ) {
        L->dQ = keepQ;
        L->dV = keepV;
    } else {
        CAL_HIP(c, hipMalloc((void**)&L->dQ, qcols * L->ld * sizeof(double)));
        CAL_HIP(c, hipMalloc((void**)&L->dV, (size_t)2 * (s + 1) * L->ld * sizeof(double)));
        CAL_HIP(c, hipMemsetAsync(L->dQ, 0, qcols * L->ld * sizeof(double), c->stream));
        CAL_HIP(c, hipMemsetAsync(L->dV, 0, (size_t)2 * (s + 1) * L->ld * sizeof(double), c->stream));
    }
    L->Tld = s * max_outer + 1;
    L->T.assign((size_t)L->Tld * L->Tld, 0.0);
    {
        // CAL_OE_DEFER=0: the orthogonality error's Grams every iteration (read
        // per run: the parity test compares both)
        const char* e = std::getenv("CAL_OE_DEFER");
        const bool defer = !e || std::atoi(e) != 0;
        L->oe_defer = defer && L->mode <= 1 && (int64_t)s * max_outer + 1 <= 128;
    }
    const double t0 = now_ms();
    // q = r/sqrt(r'*r) (ca_lanczos.m:55)
    const double* r = in.r_dev;
    if (in.r_host) {
        CAL_HIP(c, hipMemcpyAsync(L->vcolumn(0), in.r_host, L->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        r = L->vcolumn(0);
    }
    double rr = in.rr;
    if (in.r_host || !(rr >= 0.0)) CAL_TRY(dot_host(c, L->n, r, r, &rr));
    CAL_HIP_OTHER(c, launch_div(L->col(0), r, std::sqrt(rr), L->n, c->stream));
    if (L->newton && in.shifts) {
        // basis_shifts handed over: Bk = newton_basis_matrix(shifts, s, 0) (ca_lanczos_prop.m:38-41)
        std::vector<std::complex<double>> y(in.nshifts);
        for (int i = 0; i < in.nshifts; ++i) y[i] = std::complex<double>(in.shifts[i], 0.0);
        for (int i = 0; i < in.nshifts && i < 64; ++i) L->info.shifts[i] = in.shifts[i];
        std::string err;
        if (leja::newton_basis_matrix(s, y, 0, L->Bk, err) != 0)
            return set_error(c, CAL_ERR_NUMERIC, "newton_basis_matrix: " + err);
    } else if (L->newton) {
        CAL_TRY(newton_prologue(c, *L, in.prologue_cgs));
    } else {  // Bk = I(:,2:s+1) (ca_lanczos.m:63-65)
        L->Bk.assign((size_t)(s + 1) * s, 0.0);
        for (int j = 0; j < s; ++j) L->Bk[(j + 1) + (size_t)j * (s + 1)] = 1.0;
    }
    if (L->mode >= 2) CAL_TRY(normest_dev(c, &L->norm_A));  // ca_lanczos.m:258,370
    L->info.norm_A = L->norm_A;
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    L->info.prologue_ms = now_ms() - t0;
    return 0;
}

LanczosView lanczos_view(cal_ctx* c) {
    LanczosState& L = *c->lz;
    return LanczosView{L.s, L.k, L.Tld, L.T.data(), L.b.data(), L.col(0), L.ld, L.info.n_rank_deficient,
                       L.info.shifts};
}

}  // namespace cal

extern "C" {

int cal_lanczos_begin(cal_ctx* c, const double* r, int s, int max_outer, const char* basis, const char* orth) {
    LanczosBegin in;
    in.r_host = r;
    return lanczos_begin(c, in, s, max_outer, basis, orth);
}

int cal_lanczos_step(cal_ctx* c, int diagnostics) {
    if (!c || !c->lz) return set_error(c, CAL_ERR_ARG, "cal_lanczos_step: no active CA-Lanczos run");
    if (diagnostics) CAL_TRY(shared_refuses(c, "the Ritz diagnostics' residual"));
    hipSetDevice(c->device);
    return lanczos_step(c, diagnostics);
}

int cal_lanczos_state(cal_ctx* c, int* k, int* s, int* reorth_last) {
    if (!c || !c->lz) return CAL_ERR_ARG;
    if (k) *k = c->lz->k;
    if (s) *s = c->lz->s;
    if (reorth_last) *reorth_last = c->lz->reorth.empty() ? 0 : c->lz->reorth.back();
    return 0;
}

int cal_lanczos_get(cal_ctx* c, double* T, int ldt, double* rn, double* oe, int* reorth_flags,
                    cal_lanczos_info* info) {
    if (!c || !c->lz) return CAL_ERR_ARG;
    LanczosState& L = *c->lz;
    const int k = L.k, sk = L.s * L.k;
    if (T && ldt < sk) return set_error(c, CAL_ERR_ARG, "cal_lanczos_get: ldt < s*k");
    if (L.pending.k || L.ready.k || !L.oe_pend.empty()) {  // diagnostics still deferred
        hipSetDevice(c->device);
        CAL_TRY(diag_flush(c, L));
    }
    if (T) {
        for (int j = 0; j < sk; ++j)
            for (int i = 0; i < sk; ++i) T[i + (size_t)j * ldt] = L.T[i + (size_t)j * L.Tld];
    }
    if (rn) {  // k x sk column-major (MATLAB rnorm(1:k,:))
        for (int j = 0; j < sk; ++j)
            for (int i = 0; i < k; ++i) {
                double v = 0.0;
                if (i < (int)L.rn.size() && j < (int)L.rn[i].size()) v = L.rn[i][j];
                rn[i + (size_t)j * k] = v;
            }
    }
    if (oe)
        for (int i = 0; i < k; ++i) oe[i] = i < (int)L.oe.size() ? L.oe[i] : 0.0;
    if (reorth_flags)
        for (int i = 0; i < k; ++i) reorth_flags[i] = L.reorth[i];
    if (info) *info = L.info;
    return 0;
}

int cal_lanczos_get_Q(cal_ctx* c, int64_t col0, int ncols, double* Q) {
    if (!c || !c->lz || !Q || col0 < 0 || ncols < 0) return CAL_ERR_ARG;
    LanczosState& L = *c->lz;
    if (col0 + ncols > (int64_t)L.s * L.max_outer + 1) return set_error(c, CAL_ERR_ARG, "Q column range");
    CAL_HIP(c, hipMemcpy2DAsync(Q, L.n * sizeof(double), L.col((int)col0), L.ld * sizeof(double),
                                L.n * sizeof(double), ncols, hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cal_lanczos_end(cal_ctx* c) {
    if (!c) return CAL_ERR_ARG;
    cal_lanczos_free_state(c);
    return 0;
}

// compute_ritz_rnorm (ca_lanczos.m:88-97) for host Q (n_local x k) and a
// real eigen-decomposition (Vp k x k, d): [d, ix] = sort(d, 'descend'),
// rn(i) = ||A x - l x|| / ||l x|| with x = Q Vp(:, ix(i)), l = d(ix(i)).  The
// device path of the diagnostics: X = Q Vp on the matrix cores, the batched
// residual kernel (the plane march where the matrix takes it), one reduction.
int cal_compute_ritz_rnorm(cal_ctx* c, const double* Q, int k, const double* Vp, const double* d, double* rn) {
    if (!c || !Q || !Vp || !d || !rn || k < 1) return CAL_ERR_ARG;
    if (!c->has_A) return set_error(c, CAL_ERR_NOMATRIX, "no matrix set on the context");
    CAL_TRY(shared_refuses(c, "compute_ritz_rnorm"));
    const int64_t n = c->A.n_local, ld = c->A.ld;
    CAL_TRY(ensure_work(c, 2 * k, ld));
    double* Qd = work_col(c, 0) + c->A.lpad;
    CAL_HIP(c, hipMemcpy2DAsync(Qd, ld * sizeof(double), Q, n * sizeof(double), n * sizeof(double), k,
                                hipMemcpyHostToDevice, c->stream));
    return ritz_rnorm_dev(c, Qd, k, Vp, d, rn);
}

}  // extern "C"

// the same for Q already on the device (k columns at Qd, leading dimension
// A.ld, local origin; not work columns [k, 2k), which hold X)
int cal::ritz_rnorm_dev(cal_ctx* c, const double* Qd, int k, const double* Vp, const double* d, double* rn) {
    CAL_TRY(shared_refuses(c, "compute_ritz_rnorm"));
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(d[i])) return set_error(c, CAL_ERR_ARG, "compute_ritz_rnorm: non-finite eigenvalue");
    const int64_t n = c->A.n_local, ld = c->A.ld;
    std::vector<RitzPair> pairs;
    for (int j = 0; j < k; ++j) pairs.push_back({d[j], 0.0, j, -1});
    matlab_sort_desc(pairs, false);
    CAL_TRY(ensure_work(c, 2 * k, ld));
    double* X = work_col(c, k) + c->A.lpad;
    const int nbp = spmv_resid_pair_multi_blocks(c);
    const int nbr = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256));
    const size_t npart = (size_t)2 * k * std::max(nbp, nbr);
    // inputs: Vp, then per pair (Ritz value, column, output slot)
    const size_t o_lam = (size_t)k * k, o_col = o_lam + k, o_out = o_col + (k + 1) / 2, nin = o_out + (k + 1) / 2;
    std::vector<double> hin(nin, 0.0);
    std::copy(Vp, Vp + (size_t)k * k, hin.begin());
    int* h_col = reinterpret_cast<int*>(hin.data() + o_col);
    int* h_out = reinterpret_cast<int*>(hin.data() + o_out);
    for (int i = 0; i < k; ++i) {
        hin[o_lam + i] = pairs[i].lr;
        h_col[i] = pairs[i].cr;
        h_out[i] = i;
    }
    double *din = nullptr, *dpart = nullptr, *dres = nullptr;
    auto fin = [&](int st) {
        hipFree(din);
        hipFree(dpart);
        hipFree(dres);
        return st;
    };
    if (hipMalloc((void**)&din, nin * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&dpart, npart * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&dres, (size_t)2 * k * sizeof(double)) != hipSuccess)
        return fin(set_error(c, CAL_ERR_HIP, "compute_ritz_rnorm: device allocation failed"));
    auto go = [&]() -> int {
        CAL_HIP(c, hipMemcpyAsync(din, hin.data(), nin * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (apply_mt_ok(k, k)) {
            CAL_HIP(c, launch_apply_mt(Qd, ld, din, k, k, X, ld, n, c->stream));
        } else {
            Panel Qp = panel();
            panel_add(Qp, Qd, ld, k);
            CAL_TRY(apply_dev(c, n, Qp, din, k, panel_out(X, ld, k)));
        }
        for (int i = 0; i < k; ++i) CAL_TRY(halo_exchange(c, X + (int64_t)i * ld));
        if (nbp > 0) {
            CAL_TRY(spmv_resid_pair_multi_dev(c, X, ld, reinterpret_cast<const int*>(din + o_col), din + o_lam,
                                              reinterpret_cast<const int*>(din + o_out), k, dpart, nbp));
            CAL_HIP_OTHER(c, launch_reduce(dpart, nbp, 2 * k, dres, c->stream));
        } else {
            for (int i = 0; i < k; ++i) {
                SpmvArgs a{};
                a.rowptr = c->A.rowptr + c->A.ext_off;
                a.col = c->A.col;
                a.val = c->A.val;
                a.x = X + (int64_t)pairs[i].cr * ld;
                CAL_HIP(c, launch_spmv_resid(a, nullptr, pairs[i].lr, 0.0, n, dpart + (size_t)2 * i * nbr, nbr,
                                             c->stream));
                CAL_HIP_OTHER(c, launch_reduce(dpart + (size_t)2 * i * nbr, nbr, 2, dres + 2 * i, c->stream));
            }
        }
        CAL_TRY(allreduce_sum(c, dres, 2 * k));
        std::vector<double> h(2 * k);
        CAL_HIP(c, hipMemcpyAsync(h.data(), dres, 2 * k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        CAL_HIP(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < k; ++i) rn[i] = std::sqrt(h[2 * i]) / std::sqrt(h[2 * i + 1]);
        return 0;
    };
    return fin(go());
}

extern "C" {

int cal_ca_lanczos(cal_ctx* c, const double* r, int s, int iter, const char* basis, const char* orth,
                   int diagnostics, double* T, double* Q, double* rn, double* oe, int* reorth_flags,
                   cal_lanczos_info* info) {
    if (!c) return CAL_ERR_ARG;
    if (s < 1 || iter < 1) return set_error(c, CAL_ERR_ARG, "cal_ca_lanczos: need s >= 1 and iter >= 1");
    const int t = (iter + s - 1) / s;  // ca_lanczos.m:52
    if (diagnostics) CAL_TRY(shared_refuses(c, "the Ritz diagnostics' residual"));  // before a run is opened
    CAL_TRY(cal_lanczos_begin(c, r, s, t, basis, orth));
    int status = 0;
    for (int k = 0; k < t; ++k) {
        status = cal_lanczos_step(c, diagnostics);
        if (status != 0) break;
    }
    if (status < 0) return status;
    const int k = c->lz->k, sk = s * k;
    CAL_TRY(cal_lanczos_get(c, T, sk, rn, oe, reorth_flags, info));
    if (Q) CAL_TRY(cal_lanczos_get_Q(c, 0, sk, Q));
    cal_lanczos_free_state(c);
    return status;
}

// ---- f2: explicit restart (restarted_ca_lanczos.m) ------------------------
}  // extern "C"

namespace {
// ||A x - l x|| / ||l x|| of one device vector (ld layout, lpad origin)
int rel_residual(cal_ctx* c, double* x, double l, double* out) {
    CAL_TRY(shared_refuses(c, "the Ritz residual"));
    const int64_t n = c->A.n_local;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256));
    CAL_TRY(ensure_partial(c, (size_t)2 * std::max(nb, spmv_resid_pair_blocks(c))));
    CAL_TRY(ensure_red(c, 2));
    CAL_TRY(halo_exchange(c, x));
    int nbk = 0;
    CAL_TRY(spmv_resid_pair_dev(c, x, l, c->d_partial, &nbk));
    if (nbk > 0) {
        CAL_HIP_OTHER(c, launch_reduce(c->d_partial, nbk, 2, c->d_red, c->stream));
    } else {
        SpmvArgs a{};
        a.rowptr = c->A.rowptr + c->A.ext_off;  // local rows of a stored slab
        a.col = c->A.col;
        a.val = c->A.val;
        a.x = x;
        CAL_HIP(c, launch_spmv_resid(a, nullptr, l, 0.0, n, c->d_partial, nb, c->stream));
        CAL_HIP_OTHER(c, launch_reduce(c->d_partial, nb, 2, c->d_red, c->stream));
    }
    CAL_TRY(allreduce_sum(c, c->d_red, 2));
    CAL_HIP_OTHER(c, hipMemcpyAsync(c->h_red, c->d_red, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CAL_HIP(c, hipStreamSynchronize(c->stream));
    c->small_pending = false;
    *out = std::sqrt(c->h_red[0]) / std::sqrt(c->h_red[1]);
    return 0;
}
}  // namespace

extern "C" {

int cal_restarted_ca_lanczos(cal_ctx* c, const double* r, int max_lanczos, int n_wanted, int s, const char* basis,
                             const char* orth, double tol, int diagnostics, double* conv_eigs, double* Q_conv,
                             double* rnorms, double* orth_err, cal_restart_info* info) {
    constexpr int kMaxRestarts = 200;  // restarted_ca_lanczos.m:6
    if (!c || !r || n_wanted < 1 || s < 1 || s > kMaxS || !basis || !orth || !conv_eigs)
        return set_error(c, CAL_ERR_ARG, "restarted_ca_lanczos: bad arguments");
    if (!c->has_A) return set_error(c, CAL_ERR_NOMATRIX, "no matrix set on the context");
    CAL_TRY(shared_refuses(c, "the restart drivers' normest and Ritz residuals"));
    std::string o(orth), b(basis);
    for (auto& ch : o) ch = (char)std::tolower(ch);
    for (auto& ch : b) ch = (char)std::tolower(ch);
    if (o != "local" && o != "full" && o != "periodic" && o != "selective")
        return set_error(c, CAL_ERR_ARG, "lanczos.m: Invalid option value for orth: " + o);
    if (o == "periodic" || o == "selective")  // lanczos_periodic / lanczos_selective are not defined there
        return set_error(c, CAL_ERR_UNSUPPORTED, "restarted_ca_lanczos.m defines no lanczos_" + o);
    if (b != "monomial" && b != "newton") return set_error(c, CAL_ERR_ARG, "ERROR: Unknown basis type: " + b);
    const int iters = max_lanczos / s;  // :86
    if (iters < 1) return set_error(c, CAL_ERR_ARG, "restarted_ca_lanczos: max_lanczos < s");
    hipSetDevice(c->device);
    const double t_start = now_ms();
    const int64_t n = c->A.n_local, ld = c->A.ld;
    cal_lanczos_free_state(c);
    LanczosState* L = new LanczosState();
    c->lz = L;
    L->s = s;
    L->max_outer = iters + 1;  // the inner loop runs iters+1 blocks (:277)
    L->newton = b == "newton";
    L->full = o == "full";
    L->mode = L->full ? 1 : 0;
    L->restart_inner = true;
    L->n = n;
    L->ld = ld;
    L->lpad = c->A.lpad;
    L->info.s = s;
    const size_t qcols = (size_t)s * L->max_outer + 1;
    CAL_HIP(c, hipMalloc((void**)&L->dQ, qcols * ld * sizeof(double)));
    CAL_HIP(c, hipMalloc((void**)&L->dV, (size_t)2 * (s + 1) * ld * sizeof(double)));
    CAL_HIP(c, hipMemsetAsync(L->dQ, 0, qcols * ld * sizeof(double), c->stream));
    CAL_HIP(c, hipMemsetAsync(L->dV, 0, (size_t)2 * (s + 1) * ld * sizeof(double), c->stream));
    L->Tld = s * L->max_outer + 1;
    // converged vectors Q(:,1:nconv) (the reference's Q buffer, :74)
    int qc_cap = n_wanted + s * iters;
    double* dQc = nullptr;
    CAL_HIP(c, hipMalloc((void**)&dQc, (size_t)qc_cap * ld * sizeof(double)));
    struct FreeQc {
        double*& p;
        ~FreeQc() {
            if (p) hipFree(p);
        }
    } free_qc{dQc};
    double norm_A = 0.0;
    // normest(A) (:35) on its own stream beside the prologue and the first
    // inner run (one rank; cal_impl_restarted_ca_lanczos does the same); tol is
    // first used by the first restart's convergence test (:39, :114)
    NormestAsync nest;
    struct NestGuard {
        cal_ctx* c;
        NormestAsync* J;
        ~NestGuard() {
            if (J->active) hipStreamSynchronize(c->nest_stream);
            J->active = false;
        }
    } nest_guard{c, &nest};
    const double tol_rel = tol;
    if ((!c->comm || c->comm->nranks <= 1) && !test_switch("CAL_TEST_NORMEST_SYNC")) {
        CAL_TRY(normest_async_begin(c, nest));
    } else {
        CAL_TRY(normest_dev(c, &norm_A));
        tol = tol_rel * norm_A;
    }
    // q = r/norm(r) (:56)
    CAL_HIP(c, hipMemcpyAsync(L->vcolumn(0), r, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    double rr = 0.0;
    CAL_TRY(dot_host(c, n, L->vcolumn(0), L->vcolumn(0), &rr));
    CAL_HIP_OTHER(c, launch_div(L->col(0), L->vcolumn(0), std::sqrt(rr), n, c->stream));
    if (L->newton) {
        CAL_TRY(newton_prologue(c, *L, false));  // lanczos(A,q,2*s,'local') (:65)
        if (nest.active) CAL_TRY(normest_async_poll(c, nest, false));
    } else {
        L->Bk.assign((size_t)(s + 1) * s, 0.0);
        for (int j = 0; j < s; ++j) L->Bk[(j + 1) + (size_t)j * (s + 1)] = 1.0;
    }
    std::vector<double> ceigs, crn, rn_hist, oe_hist;
    std::vector<double> rn_row(n_wanted, 0.0);
    int nconv = 0, num_restarts = 0;
    bool restart = true;
    const int m = s * iters;
    while (restart && num_restarts < kMaxRestarts) {
        num_restarts++;
        // fresh inner run from q = Q(:,1)
        L->k = 0;
        L->T.assign((size_t)L->Tld * L->Tld, 0.0);
        L->b.clear();
        L->reorth.clear();
        L->breakdown = false;
        L->powers_ready = false;
        L->dExt = dQc + c->A.lpad;
        L->next = nconv;
        for (int it = 0; it <= iters; ++it) {
            if (nest.active) CAL_TRY(normest_async_poll(c, nest, false));
            const int st = lanczos_step(c, 0);
            if (st < 0) return st;
            if (st == CAL_WARN_BREAKDOWN) return set_error(c, CAL_WARN_BREAKDOWN, "restart: inner CA-Lanczos breakdown");
        }
        if (nest.active) {
            CAL_TRY(normest_async_finish(c, nest, &norm_A));
            tol = tol_rel * norm_A;
        }
        // eig(T(1:m,1:m)), beta = T(m+1,m) (:105-107); unit-norm eigenvectors
        std::vector<double> Tm((size_t)m * m), wr(m), wi(m), V((size_t)m * m);
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) Tm[i + (size_t)j * m] = L->T[i + (size_t)j * L->Tld];
        if (cal_eig(m, Tm.data(), m, wr.data(), wi.data(), V.data()) != 0)
            return set_error(c, CAL_ERR_NUMERIC, "eig(T) did not converge");
        const double beta = L->T[m + (size_t)(m - 1) * L->Tld];
        std::vector<double> rnz(m);
        for (int j = 0; j < m; ++j) {
            double nv = 0.0;
            for (int i = 0; i < m; ++i) nv += V[i + (size_t)j * m] * V[i + (size_t)j * m];
            nv = std::sqrt(nv);
            for (int i = 0; i < m; ++i) V[i + (size_t)j * m] /= nv;
            // complex pairs never count as converged (deviation: the reference would
            // carry complex Ritz vectors)
            rnz[j] = wi[j] != 0.0 ? HUGE_VAL : beta * std::fabs(V[(m - 1) + (size_t)j * m]);
        }
        // push converged pairs to the front (:114-126)
        int k = 0;
        for (int i = 0; i < m; ++i)
            if (rnz[i] < tol) {
                std::swap(wr[i], wr[k]);
                std::swap(wi[i], wi[k]);
                std::swap(rnz[i], rnz[k]);
                for (int q = 0; q < m; ++q) std::swap(V[q + (size_t)i * m], V[q + (size_t)k * m]);
                ++k;
            }
        // Q(:,nconv+i) = Q_new*Vp(:,i) (:129-133)
        if (nconv + k > qc_cap) {
            const int cap2 = std::max(nconv + k, 2 * qc_cap);
            double* p2 = nullptr;
            CAL_HIP(c, hipMalloc((void**)&p2, (size_t)cap2 * ld * sizeof(double)));
            CAL_HIP(c, hipMemcpyAsync(p2, dQc, (size_t)nconv * ld * sizeof(double), hipMemcpyDeviceToDevice,
                                      c->stream));
            CAL_HIP(c, hipStreamSynchronize(c->stream));
            hipFree(dQc);
            dQc = p2;
            qc_cap = cap2;
        }
        Panel Qn = panel();
        panel_add(Qn, L->col(0), ld, m);
        if (k > 0) {
            PanelOut Y = panel_out(dQc + c->A.lpad + (size_t)nconv * ld, ld, k);
            CAL_TRY(apply_host(c, n, Qn, V.data(), k, &Y, nullptr, 0, nullptr));
        }
        for (int i = 0; i < k; ++i) {
            ceigs.push_back(wr[i]);
            crn.push_back(rnz[i]);
        }
        if (diagnostics) {  // :140-165
            std::vector<double> row(n_wanted, 0.0);
            for (int i = 0; i < std::min(nconv, n_wanted); ++i) row[i] = rn_row[i];
            for (int i = 0; i < k && nconv + i < n_wanted; ++i)
                CAL_TRY(rel_residual(c, dQc + c->A.lpad + (size_t)(nconv + i) * ld, ceigs[nconv + i],
                                     &row[nconv + i]));
            std::vector<int> ix;
            for (int j = k; j < m; ++j) ix.push_back(j);
            std::stable_sort(ix.begin(), ix.end(), [&](int a, int b2) { return wr[a] > wr[b2]; });
            const int extra = n_wanted - nconv - k;
            if (extra > 0) {
                CAL_TRY(ensure_work(c, 1, ld));
                double* x = work_col(c, 0) + c->A.lpad;
                for (int i = 0; i < extra && i < (int)ix.size(); ++i) {
                    PanelOut X1 = panel_out(x, ld, 1);
                    CAL_TRY(apply_host(c, n, Qn, V.data() + (size_t)ix[i] * m, 1, &X1, nullptr, 0, nullptr));
                    CAL_TRY(rel_residual(c, x, wr[ix[i]], &row[nconv + k + i]));
                }
            }
            rn_row = row;
            rn_hist.insert(rn_hist.end(), row.begin(), row.end());
            // ||I - Q_'Q_||_F, Q_ = [Q_conv Q_new] (:162-165)
            const int wq = nconv + m;
            Panel Aall = panel();
            if (nconv > 0) panel_add(Aall, dQc + c->A.lpad, ld, nconv);
            panel_add(Aall, L->col(0), ld, m);
            double fro = 0.0;
            for (int j0 = 0, nbb = 0; j0 < wq; j0 += nbb) {
                // chunks of <= 16 columns that do not straddle the two blocks
                nbb = std::min(16, (j0 < nconv ? nconv : wq) - j0);
                Panel B2 = panel();
                const double* bp = j0 < nconv ? dQc + c->A.lpad + (size_t)j0 * ld : L->col(j0 - nconv);
                panel_add(B2, bp, ld, nbb);
                std::vector<double> G((size_t)wq * nbb);
                CAL_TRY(gram_host(c, n, Aall, B2, G.data()));
                for (int jj = 0; jj < nbb; ++jj)
                    for (int ii = 0; ii < wq; ++ii) {
                        const double d = (ii == j0 + jj ? 1.0 : 0.0) - G[ii + (size_t)jj * wq];
                        fro += d * d;
                    }
            }
            oe_hist.push_back(std::sqrt(fro));
        }
        nconv += k;
        restart = (int)ceigs.size() < n_wanted;  // check_wanted_eigs (:236-253)
        if (restart) {
            // generateStartVector 'largest' (:200-214): MATLAB '>' compares real parts
            int l = std::min(k, m - 1);
            for (int j = k; j < m; ++j)
                if (wr[j] > wr[l]) l = j;
            CAL_TRY(ensure_work(c, 1, ld));
            double* x = work_col(c, 0) + c->A.lpad;
            PanelOut X1 = panel_out(x, ld, 1);
            CAL_TRY(apply_host(c, n, Qn, V.data() + (size_t)l * m, 1, &X1, nullptr, 0, nullptr));
            double xx = 0.0;
            CAL_TRY(dot_host(c, n, x, x, &xx));
            CAL_HIP_OTHER(c, launch_div(L->col(0), x, std::sqrt(xx), n, c->stream));
        }
    }
    // sort descending, keep n_wanted (or all, if not converged) (:180-196)
    std::vector<int> ix(ceigs.size());
    for (size_t i = 0; i < ix.size(); ++i) ix[i] = (int)i;
    std::stable_sort(ix.begin(), ix.end(), [&](int a, int b2) { return ceigs[a] > ceigs[b2]; });
    const int keep = restart ? nconv : n_wanted;
    for (int i = 0; i < keep; ++i) conv_eigs[i] = ceigs[ix[i]];
    if (Q_conv)
        for (int i = 0; i < keep; ++i)
            CAL_HIP(c, hipMemcpy(Q_conv + (size_t)i * n, dQc + c->A.lpad + (size_t)ix[i] * ld, n * sizeof(double),
                                 hipMemcpyDeviceToHost));
    if (rnorms)
        for (int rI = 0; rI < (int)rn_hist.size() / std::max(n_wanted, 1); ++rI)
            for (int j = 0; j < n_wanted; ++j)
                rnorms[rI + (size_t)j * kMaxRestarts] = rn_hist[(size_t)rI * n_wanted + j];
    if (orth_err)
        for (size_t i = 0; i < oe_hist.size(); ++i) orth_err[i] = oe_hist[i];
    if (info) {
        info->num_restarts = num_restarts;
        info->nconv = keep;
        info->converged = restart ? 0 : 1;
        info->norm_A = norm_A;
        double mx = 0.0;
        for (int i = 0; i < keep; ++i) mx = std::max(mx, crn[ix[i]]);
        info->max_ritz_norm = mx;
        info->ms = now_ms() - t_start;
    }
    cal_lanczos_free_state(c);
    return 0;
}

// ---- f3: implicit restart (impl_restarted_ca_lanczos.m, the intended IRL) --
}  // extern "C"

namespace {
// One CA block of lanczos_basic (impl_restarted_ca_lanczos.m:366-424) starting
// at column nvecs: s matrix powers from Q(:,nvecs+1); at nvecs == 0 the
// first block is normalised (:371-380), otherwise V(:,2:s+1) is projected
// against {Q(:,1:nvecs-s), Q(:,nvecs-s+1:nvecs+1)} ('full', :387-392; doreorth
// true, see oracle/ca_lanczos_ref.irl_lanczos_basic) and T is extended.
// (Prefetching the next block's powers before the host waits for R, as
// lanczos_step does, measured neutral here: 34.5-35.1 vs 34.9-35.4 solves/s,
// the Grams after the prefetched powers lose the Infinity Cache lines of the
// block they project, 6.74 -> 6.95 ms per solve; not kept.)
int irl_block(cal_ctx* c, LanczosState& L, int nvecs, double* bprev) {
    const int s = L.s;
    const int64_t n = c->A.n_local, ld = L.ld;
    const double* q = L.col(nvecs);
    CAL_TRY(lanczos_powers(c, L, q, 0));
    if (nvecs == 0) {
        Panel X = panel();
        panel_add(X, q, ld, 1);
        panel_add(X, L.vcolumn(1), ld, s);
        std::vector<double> Rk((size_t)(s + 1) * (s + 1));
        int rank = 0;
        bool sh = false;
        CAL_TRY(normalize_dev(c, n, X, panel_out(L.col(0), ld, s + 1), Rk.data(), 1.0e-8, &rank, &sh));
        if (rank < s + 1) L.info.n_rank_deficient++;
        if (extend_T_first(c, L, Rk) != 0) return set_error(c, CAL_WARN_BREAKDOWN, "IRL: breakdown in the first block");
        *bprev = L.b[0];
        return 0;
    }
    CAL_TRY(ensure_work(c, s, ld));
    std::vector<double*> dQ;
    std::vector<int> widths;
    if (nvecs - s > 0) {
        dQ.push_back(L.col(0));
        widths.push_back(nvecs - s);
    }
    dQ.push_back(L.col(nvecs - s));
    widths.push_back(s + 1);
    std::vector<std::vector<double>> RZ;
    std::vector<double> R((size_t)s * s);
    bool ro = false;
    int rk = s;
    CAL_TRY(project_and_normalize_blocks_dev(c, n, ld, (int)dQ.size(), dQ, widths.data(), s, L.vcolumn(1), true,
                                             work_col(c, 0) + c->A.lpad, panel_out(L.col(nvecs + 1), ld, s), RZ,
                                             R.data(), &ro, &rk));
    if (ro) L.info.n_reorth++;
    if (ro && rk < s) L.info.n_rank_deficient++;
    std::vector<double> Tk;
    double bnew = 0.0;
    const int bt = block_T(L.Bk, s, *bprev, RZ.back(), R, Tk, &bnew);
    bool finite = std::isfinite(bnew);
    for (const double v : Tk) finite = finite && std::isfinite(v);
    if (bt != 0 || !finite) return set_error(c, CAL_WARN_BREAKDOWN, "IRL: CA-Lanczos breakdown (rho_t = 0)");
    place_T(L, nvecs, Tk, *bprev, bnew);
    *bprev = bnew;
    return 0;
}

// eigen-decomposition of the symmetric part of the leading m x m of T
// (ascending, orthonormal vectors) -- the IRL's Ritz data
// (Y = NULL: the values alone -- the same values, without the vectors' cost)
void irl_sym_eig(const std::vector<double>& T, int ldt, int m, std::vector<double>& w, std::vector<double>* Y) {
    std::vector<double> S((size_t)m * m);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) S[i + (size_t)j * m] = 0.5 * (T[i + (size_t)j * ldt] + T[j + (size_t)i * ldt]);
    w.resize(m);
    if (Y) Y->resize((size_t)m * m);
    dense::eig_symmetric(m, S.data(), m, w.data(), Y ? Y->data() : nullptr, m);
}

// selectShifts 'largest' (impl_restarted_ca_lanczos.m:236-243): by modulus, descending (stable)
std::vector<int> irl_order(const std::vector<double>& w) {
    std::vector<int> ix(w.size());
    for (size_t i = 0; i < ix.size(); ++i) ix[i] = (int)i;
    std::stable_sort(ix.begin(), ix.end(), [&](int a, int b) { return std::fabs(w[a]) > std::fabs(w[b]); });
    return ix;
}

}  // namespace

extern "C" {

int cal_impl_restarted_ca_lanczos(cal_ctx* c, const double* r, int max_lanczos, int n_wanted, int s,
                                  const char* basis, const char* orth, double tol, double* conv_eigs, double* Q_conv,
                                  double* ritz_est, cal_restart_info* info) {
    constexpr int kMaxRestarts = 40;  // impl_restarted_ca_lanczos.m:7
    if (!c) return CAL_ERR_ARG;
    if (!r || n_wanted < 1 || s < 1 || s > kMaxS || !basis || !orth || !conv_eigs)
        return set_error(c, CAL_ERR_ARG, "impl_restarted_ca_lanczos: bad arguments");
    if (!c->has_A) return set_error(c, CAL_ERR_NOMATRIX, "no matrix set on the context");
    CAL_TRY(shared_refuses(c, "the restart drivers' normest and Ritz residuals"));
    std::string o(orth), b(basis);
    for (auto& ch : o) ch = (char)std::tolower(ch);
    for (auto& ch : b) ch = (char)std::tolower(ch);
    if (o != "local" && o != "full" && o != "periodic" && o != "selective")  // :24-33
        return set_error(c, CAL_ERR_ARG, "lanczos.m: Invalid option value for orth: " + o);
    if (o != "full")
        return set_error(c, CAL_ERR_UNSUPPORTED, "impl_restarted_ca_lanczos: only orth 'full' is defined (:381-392)");
    if (b != "monomial" && b != "newton") return set_error(c, CAL_ERR_ARG, "ERROR: Unknown basis type: " + b);
    // k kept, p shifts, m = k + p (:72-74; k >= s)
    const int k = std::max(n_wanted + 4, s);
    const int p = s * ((max_lanczos - k) / s);
    const int m = k + p;
    if (p < s) return set_error(c, CAL_ERR_ARG, "impl_restarted_ca_lanczos: max_lanczos < n_wanted+4+s");
    const int nblk = (m + s - 1) / s;
    hipSetDevice(c->device);
    const double t_start = now_ms();
    const int64_t n = c->A.n_local, ld = c->A.ld;
    cal_lanczos_free_state(c);
    LanczosState* L = new LanczosState();
    c->lz = L;
    L->s = s;
    L->max_outer = nblk;
    L->newton = b == "newton";
    L->full = true;
    L->mode = 1;
    L->n = n;
    L->ld = ld;
    L->lpad = c->A.lpad;
    L->info.s = s;
    const size_t qcols = (size_t)s * nblk + 1;
    CAL_HIP(c, hipMalloc((void**)&L->dQ, qcols * ld * sizeof(double)));
    CAL_HIP(c, hipMalloc((void**)&L->dV, (size_t)2 * (s + 1) * ld * sizeof(double)));
    CAL_HIP(c, hipMemsetAsync(L->dQ, 0, qcols * ld * sizeof(double), c->stream));
    CAL_HIP(c, hipMemsetAsync(L->dV, 0, (size_t)2 * (s + 1) * ld * sizeof(double), c->stream));
    L->Tld = (int)qcols;
    L->T.assign((size_t)L->Tld * L->Tld, 0.0);
    double norm_A = 0.0;
    // normest(A) (:37-40) on its own stream beside the prologue and the first
    // CA blocks (one rank); it is first needed by the convergence test
    NormestAsync nest;
    struct NestGuard {  // an early return leaves no normest running
        cal_ctx* c;
        NormestAsync* J;
        ~NestGuard() {
            if (J->active) hipStreamSynchronize(c->nest_stream);
            J->active = false;
        }
    } nest_guard{c, &nest};
    const double tol_rel = tol;
    if ((!c->comm || c->comm->nranks <= 1) && !test_switch("CAL_TEST_NORMEST_SYNC")) {
        CAL_TRY(normest_async_begin(c, nest));
    } else {
        CAL_TRY(normest_dev(c, &norm_A));
        tol = tol_rel * norm_A;
    }
    CAL_HIP(c, hipMemcpyAsync(L->vcolumn(0), r, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    double rr = 0.0;
    CAL_TRY(dot_host(c, n, L->vcolumn(0), L->vcolumn(0), &rr));
    CAL_HIP_OTHER(c, launch_div(L->col(0), L->vcolumn(0), std::sqrt(rr), n, c->stream));  // :53
    if (L->newton) {
        CAL_TRY(newton_prologue(c, *L, true));  // lanczos(A,q,2*s,'full') (:229-234)
        if (nest.active) CAL_TRY(normest_async_poll(c, nest, false));
    } else {
        L->Bk.assign((size_t)(s + 1) * s, 0.0);
        for (int j = 0; j < s; ++j) L->Bk[(j + 1) + (size_t)j * (s + 1)] = 1.0;
    }
    int it = 0;
    bool converged = false;
    std::vector<double> wk, Yk, est(n_wanted, 0.0);
    std::vector<int> wanted;
    CAL_TRY(ensure_work(c, k + 1, ld));
    while (!converged && it < kMaxRestarts) {
        ++it;
        // extend to m vectors (:85-94)
        double bprev = it == 1 ? 0.0 : L->T[k + (size_t)(k - 1) * L->Tld];
        for (int nv = it == 1 ? 0 : k; nv < m; nv += s) {
            if (nest.active) CAL_TRY(normest_async_poll(c, nest, false));
            CAL_TRY(irl_block(c, *L, nv, &bprev));
        }
        if (nest.active) {
            CAL_TRY(normest_async_finish(c, nest, &norm_A));
            tol = tol_rel * norm_A;
        }
        const double beta_m = L->T[m + (size_t)(m - 1) * L->Tld];
        // exact shifts: the p smallest-modulus Ritz values of T_m (:96-107)
        std::vector<double> H((size_t)m * m), W((size_t)m * m, 0.0), w;
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) H[i + (size_t)j * m] = L->T[i + (size_t)j * L->Tld];
        irl_sym_eig(L->T, L->Tld, m, w, nullptr);  // the shifts need no vectors
        const std::vector<int> u = irl_order(w);
        // T_m is tridiagonal up to rounding: drop the sub-subdiagonal noise the
        // reference's first qrstep clean-up removes (:670-672)
        for (int j = 0; j < m; ++j)
            for (int i = j + 2; i < m; ++i) H[i + (size_t)j * m] = 0.0;
        for (int i = 0; i < m; ++i) W[i + (size_t)i * m] = 1.0;
        std::vector<double> mus;
        for (int j = m; j > k; --j) mus.push_back(w[u[j - 1]]);
        dense::hess_qrsteps(m, H.data(), m, W.data(), m, mus.data(), (int)mus.size());
        // [V_k | r] = [V_m | v_{m+1}] M with r = V_m W(:,k+1) H(k+1,k) + f_m W(m,k)
        std::vector<double> M((size_t)(m + 1) * (k + 1), 0.0);
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < m; ++i) M[i + (size_t)j * (m + 1)] = W[i + (size_t)j * m];
        const double hk = H[k + (size_t)(k - 1) * m];
        for (int i = 0; i < m; ++i) M[i + (size_t)k * (m + 1)] = W[i + (size_t)k * m] * hk;
        M[m + (size_t)k * (m + 1)] = beta_m * W[(m - 1) + (size_t)(k - 1) * m];
        Panel P = panel();
        panel_add(P, L->col(0), ld, m + 1);
        // in place when the apply is one row-parallel launch (<= 256 panel
        // columns, <= 16 outputs: k_apply_stage / k_apply_rows read a row of
        // [V_m | v_{m+1}] whole before writing it): no work panel and no copy
        // back (≈ 58 us per restart).  Wider panels take the MFMA-tile apply
        // and more outputs split into launches that would read what an
        // earlier one wrote: those keep the work panel.
        if (m + 1 <= 256 && k + 1 <= 16 && !test_switch("CAL_TEST_RESTART_COPY")) {
            PanelOut Y = panel_out(L->col(0), ld, k + 1);
            CAL_TRY(apply_host(c, n, P, M.data(), k + 1, &Y, nullptr, 0, nullptr));
        } else {
            double* dW = work_col(c, 0);
            PanelOut Y = panel_out(dW + c->A.lpad, ld, k + 1);
            CAL_TRY(apply_host(c, n, P, M.data(), k + 1, &Y, nullptr, 0, nullptr));
            CAL_HIP(c, hipMemcpyAsync(L->dQ, dW, (size_t)(k + 1) * ld * sizeof(double), hipMemcpyDeviceToDevice,
                                      c->stream));
        }
        double rk2 = 0.0;
        CAL_TRY(dot_host(c, n, L->col(k), L->col(k), &rk2));
        const double bk = std::sqrt(rk2);
        if (!(bk > 0.0) || !std::isfinite(bk)) return set_error(c, CAL_ERR_NUMERIC, "IRL: zero restart residual");
        CAL_HIP_OTHER(c, launch_div(L->col(k), L->col(k), bk, n, c->stream));
        std::fill(L->T.begin(), L->T.end(), 0.0);
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < k; ++i) L->T[i + (size_t)j * L->Tld] = H[i + (size_t)j * m];
        L->T[k + (size_t)(k - 1) * L->Tld] = bk;
        // convergence of the n_wanted largest-modulus Ritz pairs of T_k (:127-143)
        irl_sym_eig(L->T, L->Tld, k, wk, &Yk);
        const std::vector<int> ord = irl_order(wk);
        wanted.assign(ord.begin(), ord.begin() + std::min(n_wanted, k));
        converged = true;
        for (int i = 0; i < (int)wanted.size(); ++i) {
            est[i] = bk * std::fabs(Yk[(k - 1) + (size_t)wanted[i] * k]);
            if (!(est[i] < tol)) converged = false;
            if (ritz_est) ritz_est[(it - 1) + (size_t)i * kMaxRestarts] = est[i];
        }
    }
    // wanted pairs, descending (:218-222)
    std::vector<int> sel(wanted);
    std::stable_sort(sel.begin(), sel.end(), [&](int a, int b2) { return wk[a] > wk[b2]; });
    const int nw = (int)sel.size();
    for (int i = 0; i < nw; ++i) conv_eigs[i] = wk[sel[i]];
    {
        // the Ritz vectors Q_conv = V_k Y_k(:, sel) are formed on the device
        // (work columns 0..nw-1); Q_conv == NULL keeps them there
        std::vector<double> Ms((size_t)k * nw);
        for (int j = 0; j < nw; ++j)
            for (int i = 0; i < k; ++i) Ms[i + (size_t)j * k] = Yk[i + (size_t)sel[j] * k];
        CAL_TRY(ensure_work(c, nw, ld));
        Panel P = panel();
        panel_add(P, L->col(0), ld, k);
        PanelOut Y = panel_out(work_col(c, 0) + c->A.lpad, ld, nw);
        CAL_TRY(apply_host(c, n, P, Ms.data(), nw, &Y, nullptr, 0, nullptr));
        if (Q_conv)
            CAL_HIP(c, hipMemcpy2DAsync(Q_conv, n * sizeof(double), work_col(c, 0) + c->A.lpad, ld * sizeof(double),
                                        n * sizeof(double), nw, hipMemcpyDeviceToHost, c->stream));
        CAL_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (info) {
        info->num_restarts = it;
        info->nconv = nw;
        info->converged = converged ? 1 : 0;
        info->norm_A = norm_A;
        double mx = 0.0;
        for (int i = 0; i < nw; ++i) mx = std::max(mx, est[i]);
        info->max_ritz_norm = mx;
        info->ms = now_ms() - t_start;
    }
    cal_lanczos_free_state(c);
    return 0;
}

}  // extern "C"
