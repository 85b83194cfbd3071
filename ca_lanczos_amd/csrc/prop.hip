// prop.hip -- the half-mixing combine of the Krylov time propagation
// (ca_lanczos_prop.m / runLanczos.m:102-103 on stacked halves):
//
//   psi' = nrm * Q_c * c,   Q_c = Q(1:n,:) + i Q(n+1:2n,:),   nrm c = a + i b
//   out[i]     = sum_j Q[i,j] a_j - Q[i+n,j] b_j
//   out[i + n] = sum_j Q[i,j] b_j + Q[i+n,j] a_j              0 <= i < n
//
// One streaming pass: every Q element is read once ((2n m + 2n) * 8 bytes
// with the store).  A lane owns kPropPairs pairs of adjacent rows and reads
// each pair of either half with one 16-byte load; a half whose origin (or
// whose output's origin) is not 16-byte aligned -- the lower half starts at
// row n, n may be odd, and the columns' local origin may be shifted -- takes
// 8-byte loads instead, and so does the single last row of an odd n.
//
// The summation order is fixed (the build is -ffp-contract=off, so a NumPy
// loop reproduces the bits): accumulators start at +0.0, j ascends, and per j
//   top = top + Qt a_j;  top = top - Qb b_j;  bot = bot + Qt b_j;  bot = bot + Qb a_j
// one chain per output row -- the rows a lane owns give the instruction-level
// parallelism, not split accumulators.  The coefficients are staged in LDS.
// Every block also leaves the sum of its out^2 in partial[block] (per lane in
// row order top then bottom, pair by pair; wave tree; the four waves in
// order): launch_reduce turns them into the next step's squared norm without
// another sweep, deterministically (no atomics).
//
// launch_prop_combine is the one host entry: it picks OBS, ABS and REAL from
// what its PropCombine carries and VT / VB from the alignment of Q and out.
//
// OBS = true (nw + np > 0) also reduces observables of the new
// state in the same sweep: nw real diagonal operators W_k and np reference
// states phi_r = pr + i pi, each streamed once (a lane's two adjacent rows
// with one 16-byte load: the library's own aligned allocation with an even
// leading dimension).  Per output row, t = Re psi'[i], b = Im psi'[i]:
//   W_k  :  d = t*t;  d = d + b*b;  accW[k] = accW[k] + w*d
//   phi_r:  accRe[r] = accRe[r] + pr*t;  accRe[r] = accRe[r] + pi*b
//           accIm[r] = accIm[r] + pr*b;  accIm[r] = accIm[r] - pi*t
// a lane's rows in row order, pair by pair (the nrm chain's order), then the
// nrm chain's wave tree and wave order.  Quantity q's block partial goes to
// partial[q * gridDim.x + block] (launch_reduce's entry-major layout): q = 0
// the squared norm, 1 + k <W_k>, 1 + nw + 2r / + 2r + 1 Re / Im <phi_r|psi'>.
// The counts are kernel arguments; the loops over them are unrolled to the
// cap with wave-uniform guards, so every accumulator is a register.  The nrm
// chain and the stores are those of OBS = false: same state, same norm bits.
//
// ABS = true (a mask is given) multiplies the new state by a real
// diagonal mask 0 <= M <= 1 before it is stored (the absorbing boundary: the
// first-order splitting of a complex absorbing potential -ln(M)/dt) and sums
// what the mask removes.  The mask is streamed once from the library's own
// aligned copy (even leading dimension >= n; a row pair with one 16-byte load,
// the odd last row with an 8-byte load; the pad is never read).  Per row, with
// ut, ub the two accumulators after the j loop and m the row's mask value:
//   d = ut*ut;  d = d + ub*ub;  p = m*m;  g = 1.0 - p;  accA = accA + g*d
//   t = m*ut;   b = m*ub;       store t, b
// and the nrm chain and the observables then run on t, b as written above: they
// are those of the state as stored.  accA takes a lane's rows in row order, pair
// by pair, then the nrm chain's wave tree and wave order; its block partial is
// quantity 1 + nw + 2 np (after the observables; 1 without OBS).  ABS = false
// is the kernel as it was: the mask is an `if constexpr` away.
//
// REAL = true is the combine of a real state (cal_prop_begin_real; an
// imaginary-time step keeps a real state real), out[i] = sum_j Q[i,j] a_j for
// i in [0, n): the same kernel without the lower half -- no loads of it, no b,
// no sb in LDS, VB unused, no mask and no reference states.  Staging, the rows
// per lane and per block, the odd-n tail, the wave sums and the epilogue are
// the ones above; the per-row chains are t = t + x*a_j, then nrm = nrm + t*t
// and with OBS, for k < nw,  d = t*t;  accW[k] = accW[k] + w*d  (no b term, not
// even a zero one).  (n m + n + n nw) 8 bytes.  The stacked instantiations keep
// the statement order they had: the scheduler follows it.
#include "cal_internal.hpp"

namespace cal {

namespace {

typedef double pd2 __attribute__((ext_vector_type(2)));

constexpr int kPropThreads = 256;
constexpr int kPropPairs = 2;                                     // row pairs per lane
constexpr int kPropBlockRows = 2 * kPropPairs * kPropThreads;     // rows of one half per block

__device__ __forceinline__ double prop_wave_sum(double s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
    return s;
}

// two adjacent rows of one half: a 16-byte access when the half is aligned
template <bool VEC>
__device__ __forceinline__ void load2(const double* __restrict__ p, double& x0, double& x1) {
    if (VEC) {
        const pd2 v = *reinterpret_cast<const pd2*>(p);
        x0 = v.x;
        x1 = v.y;
    } else {
        x0 = p[0];
        x1 = p[1];
    }
}
template <bool VEC>
__device__ __forceinline__ void store2(double* __restrict__ p, double x0, double x1) {
    if (VEC) {
        pd2 v;
        v.x = x0;
        v.y = x1;
        *reinterpret_cast<pd2*>(p) = v;
    } else {
        p[0] = x0;
        p[1] = x1;
    }
}

// the OBS / ABS kernels' extra argument; the plain kernel carries an empty one
template <bool OBS, bool ABS>
struct PropObsArg {};
template <>
struct PropObsArg<true, false> {
    PropObs o;
};
template <>
struct PropObsArg<false, true> {
    const double* mask;
};
template <>
struct PropObsArg<true, true> {
    PropObs o;
    const double* mask;
};

struct PropObsAcc {
    double w[kPropMaxObs], re[kPropMaxObs], im[kPropMaxObs];
};

// the observables' wave sums (LDS of the OBS kernels only)
__device__ __forceinline__ double (*obs_wave_sums())[kPropThreads / 64] {
    __shared__ double wo[3 * kPropMaxObs][kPropThreads / 64];
    return wo;
}

// the absorbed norm's wave sums (LDS of the ABS kernels only)
__device__ __forceinline__ double* abs_wave_sums() {
    __shared__ double wa[kPropThreads / 64];
    return wa;
}

// one row under the mask value m: what the mask removes goes to s, the row is scaled
__device__ __forceinline__ void mask_row(double m, double& t, double& b, double& s) {
    double d = t * t;
    d = d + b * b;
    const double p = m * m;
    const double g = 1.0 - p;
    s = s + g * d;
    t = m * t;
    b = m * b;
}

// the observables' terms of the adjacent rows r, r + 1 (PAIR) or of row r alone;
// REAL: d = t*t with no b term, and no reference states
template <bool PAIR, bool REAL>
__device__ __forceinline__ void obs_rows(const PropObs& o, int64_t r, double t0, double t1, double b0, double b1,
                                         PropObsAcc& s) {
#pragma unroll
    for (int k = 0; k < kPropMaxObs; ++k)
        if (k < o.nw) {
            const double* w = o.W + k * o.ld + r;
            double w0, w1 = 0.0;
            if (PAIR) load2<true>(w, w0, w1);
            else w0 = *w;
            double d = t0 * t0;
            if constexpr (!REAL) d = d + b0 * b0;
            s.w[k] = s.w[k] + w0 * d;
            if (PAIR) {
                d = t1 * t1;
                if constexpr (!REAL) d = d + b1 * b1;
                s.w[k] = s.w[k] + w1 * d;
            }
        }
    if constexpr (REAL) return;
#pragma unroll
    for (int k = 0; k < kPropMaxObs; ++k)
        if (k < o.np) {
            const double* pr = o.pr + k * o.ld + r;
            const double* pi = o.pi + k * o.ld + r;
            double r0, r1 = 0.0, i0, i1 = 0.0;
            if (PAIR) {
                load2<true>(pr, r0, r1);
                load2<true>(pi, i0, i1);
            } else {
                r0 = *pr;
                i0 = *pi;
            }
            s.re[k] = s.re[k] + r0 * t0;
            s.re[k] = s.re[k] + i0 * b0;
            s.im[k] = s.im[k] + r0 * b0;
            s.im[k] = s.im[k] - i0 * t0;
            if (PAIR) {
                s.re[k] = s.re[k] + r1 * t1;
                s.re[k] = s.re[k] + i1 * b1;
                s.im[k] = s.im[k] + r1 * b1;
                s.im[k] = s.im[k] - i1 * t1;
            }
        }
}

template <bool VT, bool VB, bool OBS, bool ABS, bool REAL>
__global__ __launch_bounds__(kPropThreads) void k_prop_combine(const double* __restrict__ Q, int64_t ld, int64_t n,
                                                               int m, const double* __restrict__ a,
                                                               const double* __restrict__ b,
                                                               double* __restrict__ out,
                                                               double* __restrict__ partial, PropObsArg<OBS, ABS> obs) {
    static_assert(!REAL || (!VB && !ABS), "a real state has no lower half and takes no mask");
    __shared__ double sa[kPropMaxCols];
    __shared__ double sb[kPropMaxCols];  // REAL: no statement names it, so it takes no LDS
    __shared__ double ws[kPropThreads / 64];
    PropObsAcc acc;
    if constexpr (OBS) {
#pragma unroll
        for (int k = 0; k < kPropMaxObs; ++k) acc.w[k] = acc.re[k] = acc.im[k] = 0.0;
    }
    for (int j = threadIdx.x; j < m; j += kPropThreads) {
        sa[j] = a[j];
        if constexpr (!REAL) sb[j] = b[j];
    }
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * kPropBlockRows;
    double nrm = 0.0;
    double absd = 0.0;
#pragma unroll
    for (int p = 0; p < kPropPairs; ++p) {
        const int64_t r = base + 2 * ((int64_t)p * kPropThreads + threadIdx.x);
        if (r + 1 < n) {
            const double* qt = Q + r;
            const double* qb = REAL ? nullptr : Q + n + r;  // a real state has no lower half
            double t0 = 0.0, t1 = 0.0, b0 = 0.0, b1 = 0.0;
#pragma unroll 4
            for (int j = 0; j < m; ++j) {
                double xt0, xt1, xb0, xb1, bj;  // REAL: the lower half and b are never read
                load2<VT>(qt, xt0, xt1);
                if constexpr (!REAL) load2<VB>(qb, xb0, xb1);
                qt += ld;
                if constexpr (!REAL) qb += ld;
                const double aj = sa[j];
                if constexpr (!REAL) bj = sb[j];
                t0 = t0 + xt0 * aj;
                t1 = t1 + xt1 * aj;
                if constexpr (!REAL) {
                    t0 = t0 - xb0 * bj;
                    t1 = t1 - xb1 * bj;
                    b0 = b0 + xt0 * bj;
                    b1 = b1 + xt1 * bj;
                    b0 = b0 + xb0 * aj;
                    b1 = b1 + xb1 * aj;
                }
            }
            if constexpr (ABS) {
                double m0, m1;
                load2<true>(obs.mask + r, m0, m1);
                mask_row(m0, t0, b0, absd);
                mask_row(m1, t1, b1, absd);
            }
            store2<VT>(out + r, t0, t1);
            if constexpr (!REAL) store2<VB>(out + n + r, b0, b1);
            nrm = nrm + t0 * t0;
            nrm = nrm + t1 * t1;
            if constexpr (!REAL) {
                nrm = nrm + b0 * b0;
                nrm = nrm + b1 * b1;
            }
            if constexpr (OBS) obs_rows<true, REAL>(obs.o, r, t0, t1, b0, b1, acc);
        } else if (r < n) {  // the last row of an odd n
            const double* qt = Q + r;
            const double* qb = REAL ? nullptr : Q + n + r;  // a real state has no lower half
            double t0 = 0.0, b0 = 0.0;
            for (int j = 0; j < m; ++j) {
                double xb0, bj;
                const double xt0 = *qt;
                if constexpr (!REAL) xb0 = *qb;
                qt += ld;
                if constexpr (!REAL) qb += ld;
                const double aj = sa[j];
                if constexpr (!REAL) bj = sb[j];
                t0 = t0 + xt0 * aj;
                if constexpr (!REAL) {
                    t0 = t0 - xb0 * bj;
                    b0 = b0 + xt0 * bj;
                    b0 = b0 + xb0 * aj;
                }
            }
            if constexpr (ABS) mask_row(obs.mask[r], t0, b0, absd);
            out[r] = t0;
            if constexpr (!REAL) out[n + r] = b0;
            nrm = nrm + t0 * t0;
            if constexpr (!REAL) nrm = nrm + b0 * b0;
            if constexpr (OBS) obs_rows<false, REAL>(obs.o, r, t0, 0.0, b0, 0.0, acc);
        }
    }
    nrm = prop_wave_sum(nrm);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) ws[wave] = nrm;
    if constexpr (OBS) {
        double(*wo)[kPropThreads / 64] = obs_wave_sums();
        const int nw = obs.o.nw, np = REAL ? 0 : obs.o.np;
#pragma unroll
        for (int k = 0; k < kPropMaxObs; ++k)
            if (k < nw) {
                const double v = prop_wave_sum(acc.w[k]);
                if (lane == 0) wo[k][wave] = v;
            }
#pragma unroll
        for (int k = 0; k < kPropMaxObs; ++k)
            if (k < np) {
                const double vr = prop_wave_sum(acc.re[k]);
                const double vi = prop_wave_sum(acc.im[k]);
                if (lane == 0) {
                    wo[nw + 2 * k][wave] = vr;
                    wo[nw + 2 * k + 1][wave] = vi;
                }
            }
    }
    if constexpr (ABS) {
        absd = prop_wave_sum(absd);
        if (lane == 0) abs_wave_sums()[wave] = absd;
    }
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    if constexpr (OBS) {  // thread q writes quantity q of this block
        double(*wo)[kPropThreads / 64] = obs_wave_sums();
        const int q = (int)threadIdx.x - 1;
        if (q >= 0 && q < obs.o.nw + 2 * (REAL ? 0 : obs.o.np))
            partial[(int64_t)(q + 1) * gridDim.x + blockIdx.x] = ((wo[q][0] + wo[q][1]) + wo[q][2]) + wo[q][3];
    }
    if constexpr (ABS) {  // after the observables: quantity 1 + nw + 2 np
        const double* wa = abs_wave_sums();
        int q = 1;
        if constexpr (OBS) q = 1 + obs.o.nw + 2 * obs.o.np;
        if (threadIdx.x == 0) partial[(int64_t)q * gridDim.x + blockIdx.x] = ((wa[0] + wa[1]) + wa[2]) + wa[3];
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int prop_combine_blocks(int64_t n) {
    const int64_t b = (n + kPropBlockRows - 1) / kPropBlockRows;
    return (int)(b < 1 ? 1 : b);
}

int prop_combine_quantities(const PropCombine& p) { return 1 + p.obs.nw + 2 * p.obs.np + (p.mask ? 1 : 0); }

// the VT / VB choice: a half takes 16-byte accesses when its rows of every
// column and of the output start 16-byte aligned (even leading dimension);
// a real state (REAL) is the upper half alone, VB unused
template <bool OBS, bool ABS, bool REAL = false>
static hipError_t launch_combine(const PropCombine& p, PropObsArg<OBS, ABS> obs, hipStream_t st) {
    const dim3 grid((unsigned)prop_combine_blocks(p.n)), block(kPropThreads);
    const bool even = (p.ld & 1) == 0;
    const bool vt = even && aligned16(p.Q) && aligned16(p.out);
    auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, grid, block, 0, st, p.Q, p.ld, p.n, p.m, p.a, p.b, p.out, p.partial, obs);
    };
    if constexpr (REAL) {
        if (vt) launch(k_prop_combine<true, false, OBS, ABS, true>);
        else launch(k_prop_combine<false, false, OBS, ABS, true>);
    } else {
        const bool vb = even && aligned16(p.Q + p.n) && aligned16(p.out + p.n);
        if (vt && vb) launch(k_prop_combine<true, true, OBS, ABS, false>);
        else if (vt) launch(k_prop_combine<true, false, OBS, ABS, false>);
        else if (vb) launch(k_prop_combine<false, true, OBS, ABS, false>);
        else launch(k_prop_combine<false, false, OBS, ABS, false>);
    }
    return hipGetLastError();
}

// the observables' counts, arrays and 16-byte loads
static bool obs_arg_ok(const PropObs& o, int64_t n) {
    if (o.nw < 0 || o.nw > kPropMaxObs || o.np < 0 || o.np > kPropMaxObs) return false;
    if ((o.nw > 0 && !o.W) || (o.np > 0 && (!o.pr || !o.pi))) return false;
    // aligned origins, an even leading dimension of at least n rows
    if (o.nw + o.np > 0 && (o.ld < n || (o.ld & 1) != 0)) return false;
    if ((o.nw > 0 && !aligned16(o.W)) || (o.np > 0 && (!aligned16(o.pr) || !aligned16(o.pi)))) return false;
    return true;
}

hipError_t launch_prop_combine(const PropCombine& p, hipStream_t st) {
    if (p.n < 1 || p.m < 1 || p.m > kPropMaxCols || p.ld < (p.real ? 1 : 2) * p.n) return hipErrorInvalidValue;
    if (p.n > ((int64_t)1 << 40)) return hipErrorInvalidValue;
    if (!obs_arg_ok(p.obs, p.n)) return hipErrorInvalidValue;
    if (p.real) {  // no reference states and no mask on a real state
        if (p.obs.np > 0 || p.mask) return hipErrorInvalidValue;
        if (p.obs.nw > 0) return launch_combine<true, false, true>(p, PropObsArg<true, false>{p.obs}, st);
        return launch_combine<false, false, true>(p, PropObsArg<false, false>{}, st);
    }
    // the mask's 16-byte loads: the rules of the observables' columns
    if (p.mask && (!aligned16(p.mask) || p.ldm < p.n || (p.ldm & 1) != 0)) return hipErrorInvalidValue;
    const bool obs = p.obs.nw + p.obs.np > 0;
    if (!obs && !p.mask) return launch_combine(p, PropObsArg<false, false>{}, st);
    if (!p.mask) return launch_combine(p, PropObsArg<true, false>{p.obs}, st);
    if (!obs) return launch_combine(p, PropObsArg<false, true>{p.mask}, st);
    return launch_combine(p, PropObsArg<true, true>{p.obs, p.mask}, st);
}

// ---- the time-dependent diagonal ---------------------------------------------------
// H(t) = H0 + sum_k f_k(t) diag(W_k) rewrites one stored entry per row: the
// slot of val with col == row (and the split format's streamed diagonal).
//
// k_diag_find (once per matrix) looks that slot up: one row per thread in a
// grid-stride loop, a plain scan of the row -- empty rows and rows longer
// than a CSR row block included -- keeping the first hit and counting the
// hits.  Rows with no hit and rows with several are counted per block (exact
// small integers in doubles; wave tree, the four waves in order) so that
// launch_reduce gives the two totals in the fixed order, no atomics.
//
// k_diag_density (once per Krylov build) is one row per lane with 8-byte accesses:
//   d = V0[i];  k ascending:  p = f_k * W_k[i];  d = d + p
// product and sum rounded separately (-ffp-contract=off), the amplitudes
// kernel arguments (wave-uniform) and the loop unrolled to the cap with
// uniform guards, as the OBS combine's; then the same d goes to the row's
// slot of either half.  Vector stores only.  The chain and the stores are
// written once; the template's state count adds the nonlinear term.
namespace {

constexpr int kDiagThreads = 256;

__global__ __launch_bounds__(kDiagThreads) void k_diag_find(const int* __restrict__ rowptr,
                                                            const int* __restrict__ col, int64_t n,
                                                            int* __restrict__ dpos, double* __restrict__ partial) {
    __shared__ double wm[kDiagThreads / 64];
    __shared__ double wd[kDiagThreads / 64];
    double miss = 0.0, dup = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kDiagThreads;
    for (int64_t r = (int64_t)blockIdx.x * kDiagThreads + threadIdx.x; r < n; r += stride) {
        const int p0 = rowptr[r], p1 = rowptr[r + 1];
        int pos = -1, hits = 0;
        for (int p = p0; p < p1; ++p)
            if (col[p] == (int)r) {
                if (hits == 0) pos = p;
                ++hits;
            }
        dpos[r] = pos;
        if (hits == 0) miss = miss + 1.0;
        if (hits > 1) dup = dup + 1.0;
    }
    miss = prop_wave_sum(miss);
    dup = prop_wave_sum(dup);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        wm[wave] = miss;
        wd[wave] = dup;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = ((wm[0] + wm[1]) + wm[2]) + wm[3];
        partial[gridDim.x + blockIdx.x] = ((wd[0] + wd[1]) + wd[2]) + wd[3];
    }
}

// NS: the states whose density g |psi|^2 joins the diagonal.  0: the drive
// alone -- no state load, no q, no LDS, no barrier, partial untouched (null is
// allowed).  1: the nonlinear term of one state A; 2: of two (the midpoint
// rule's average of the densities of psi_n and the predicted psi*), the order
// of cal_internal.hpp's DiagDrive:
//   ra = ua*ua;  ra = ra + va*va;  [rb likewise]  the drive's chain into d;
//   p = ga*ra;  d = d + p;  [p = gb*rb;  d = d + p]  the stores
// and the lane's q = ra*ra (0 past row n) summed as everything else here:
// wave tree, the four waves in order, one partial per block; no lane leaves
// before the barrier.  The lower half of a state starts at row n, which may be
// odd: 8-byte accesses.  REAL: the states are real vectors of n rows
// (cal_prop_begin_real), there is no lower half to load -- ra = ua*ua, rb =
// ub*ub -- and halves is 1; everything else is the same.
template <bool SPLIT, int NS, bool REAL>
__global__ __launch_bounds__(kDiagThreads) void k_diag_density(DiagDrive a) {
    static_assert(NS >= 0 && NS <= 2 && (NS > 0 || !REAL), "REAL describes the states");
    const int64_t n = a.n;
    const int64_t i = (int64_t)blockIdx.x * kDiagThreads + threadIdx.x;
    double acc = 0.0;
    if (i < n) {
        double ra = 0.0, rb = 0.0;
        if constexpr (NS >= 1) {
            const double ua = a.A[i];
            ra = ua * ua;
            if constexpr (!REAL) {
                const double va = a.A[n + i];
                ra = ra + va * va;
            }
        }
        if constexpr (NS == 2) {
            const double ub = a.B[i];
            rb = ub * ub;
            if constexpr (!REAL) {
                const double vb = a.B[n + i];
                rb = rb + vb * vb;
            }
        }
        double d = a.V0[i];
#pragma unroll
        for (int k = 0; k < kDriveMaxOps; ++k)
            if (k < a.nk) {
                const double p = a.f[k] * a.W[k * a.ldw + i];
                d = d + p;
            }
        if constexpr (NS >= 1) {
            const double p = a.ga * ra;
            d = d + p;
        }
        if constexpr (NS == 2) {
            const double p = a.gb * rb;
            d = d + p;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (h < a.halves) {
                const int64_t r = i + h * n;
                a.val[a.dpos[r]] = d;
                if (SPLIT) a.ds_diag[r] = d;
            }
        if constexpr (NS >= 1) {
            const double q = ra * ra;
            acc = acc + q;
        }
    }
    if constexpr (NS >= 1) {
        __shared__ double ws[kDiagThreads / 64];
        acc = prop_wave_sum(acc);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) ws[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) a.partial[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    }
}

}  // namespace

int diag_find_blocks(int64_t n) {
    int64_t b = (n + kDiagThreads - 1) / kDiagThreads;
    if (b > 1024) b = 1024;
    return (int)(b < 1 ? 1 : b);
}

hipError_t launch_diag_find(const int* rowptr, const int* col, int64_t n, int* dpos, double* partial, hipStream_t st) {
    if (n < 1 || n >= ((int64_t)1 << 31) || !rowptr || !col || !dpos || !partial) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_diag_find, dim3((unsigned)diag_find_blocks(n)), dim3(kDiagThreads), 0, st, rowptr, col, n,
                       dpos, partial);
    return hipGetLastError();
}

int diag_density_blocks(int64_t n) {
    const int64_t b = (n + kDiagThreads - 1) / kDiagThreads;
    return (int)(b < 1 ? 1 : b);
}

hipError_t launch_diag_density(const DiagDrive& a, hipStream_t st) {
    if (a.n < 1 || a.n >= ((int64_t)1 << 31) || a.halves < 1 || a.halves > 2 || a.nk < 0 || a.nk > kDriveMaxOps)
        return hipErrorInvalidValue;
    if (!a.V0 || !a.dpos || !a.val || (a.nk > 0 && (!a.W || a.ldw < a.n))) return hipErrorInvalidValue;
    // a state brings its partials; real states are written on one half
    if (a.A ? !a.partial || (a.real && a.halves != 1) : a.B != nullptr) return hipErrorInvalidValue;
    const dim3 grid((unsigned)diag_density_blocks(a.n)), block(kDiagThreads);
    auto launch = [&](auto k) { hipLaunchKernelGGL(k, grid, block, 0, st, a); };
    auto states = [&](auto split) {
        constexpr bool S = decltype(split)::value;
        if (!a.A) launch(k_diag_density<S, 0, false>);
        else if (a.real && a.B) launch(k_diag_density<S, 2, true>);
        else if (a.real) launch(k_diag_density<S, 1, true>);
        else if (a.B) launch(k_diag_density<S, 2, false>);
        else launch(k_diag_density<S, 1, false>);
    };
    if (a.ds_diag) states(std::true_type{});
    else states(std::false_type{});
    return hipGetLastError();
}

}  // namespace cal
