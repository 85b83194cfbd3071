// Probe: does a load policy in the block step's sweeps keep the last matrix
// powers in the Infinity Cache?  The in-loop emulation of stencil_probe.hip
// (n = 215^3: 8 gather powers rotating through 9 vectors, two Gram-like
// 17-column read sweeps, one 17 -> 8 apply sweep writing the new block) with
// a compile-time policy in k_sweep17:
//   RES = -1     all plain loads
//   RES = 0..3   non-temporal loads for columns c < 17 - RES, plain loads for
//                the last RES columns (x(9-RES)..x8 of [Qp(9) | X(8)])
// The apply sweep stores non-temporally (as pass B does); LASTPLAIN stores
// its last output column, the next step's q, plainly.  LOOP is the library's
// Gram shape: 1024 blocks, grid-stride, the next chunk loaded before this
// chunk's arithmetic.  Not part of the library.
//   hipcc -O3 --offload-arch=gfx950 tools/residency_probe.hip -o tools/residency_probe
// One JSON line per variant and pass; the whole list runs PASSES times so the
// spread of RES = -1 within the process is on record.
//   tools/residency_probe coef
// runs, in the library shape at RES = 3 only, the attribution of what the
// library's pass A and pass B do besides loading their 17 columns
// (k_sweep17c: each knob puts back one thing k_rowapply has and k_sweep17
// lacks), twice per process, one JSON line per variant and pass:
//   coef   imm: immediate coefficients; lds: an LDS-staged table read one
//          row per column behind the library's pins (a); glb: uniform loads
//          of a global table behind the same pins (b)
//   gramt  the second sweep with the wave's 64-row LDS transpose, 16
//          v_mfma_f64_16x16x4f64 per chunk and the extra VALU column (c;
//          with coef lds: d, pass A as it is; with coef glb: e)
//   chain  the apply sweep with pass B's 17 + 25 coefficient rows
// The first sweep (P1 has no coefficients) is always k_sweep17's.
// -DSWEEP_COEF_ROWS=r (1..4, default 4): coef glb pins its accumulators every r columns,
// so r uniform row loads are in flight together (k_rowapply's
// CAL_SWEEP_COEF_ROWS).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>

#ifndef SWEEP_COEF_ROWS
#define SWEEP_COEF_ROWS 4
#endif

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

struct Offs { int64_t d[8]; };

// the pair SpMV of stencil_probe.hip (k_pairtab<true, true, true, true>):
// per-pair uint16 id, LDS (offset code, value pair) table staged from global
// memory, centre load
__global__ __launch_bounds__(256) void k_pairtab(const double* __restrict__ x, double* __restrict__ y,
                                                 const uint16_t* __restrict__ ids, int64_t n,
                                                 const int* __restrict__ gtab_off,
                                                 const double2* __restrict__ gtab_v) {
    __shared__ int s_off[256];
    __shared__ double2 s_v[256];
    s_off[threadIdx.x] = gtab_off[threadIdx.x];
    s_v[threadIdx.x] = gtab_v[threadIdx.x];
    __syncthreads();
    const int G = gridDim.x, q = G >> 3, rm = G & 7, xi = blockIdx.x & 7, i = blockIdx.x >> 3;
    const int b = (xi < rm ? xi * (q + 1) : rm * (q + 1) + (xi - rm) * q) + i;
    const int64_t t = (int64_t)b * 256 + threadIdx.x;
    const int64_t r = 2 * t;
    if (r + 1 >= n) return;
    const int base = ids[t];  // 0
    double y0 = 0.0, y1 = 0.0;
    int code[7];
    double2 xv[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        code[e] = s_off[base + e];
        double2 v;
        __builtin_memcpy(&v, x + r + (code[e] >> 2), 16);
        xv[e] = v;
    }
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        const double2 v = s_v[base + e];
        const double t0 = v.x * xv[e].x, t1 = v.y * xv[e].y;
        const double a0 = y0 + t0, a1 = y1 + t1;
        y0 = (code[e] & 1) ? a0 : y0;
        y1 = (code[e] & 2) ? a1 : y1;
    }
    double2 c;
    __builtin_memcpy(&c, x + r, 16);
    y0 -= 0.5 * c.x;
    y1 -= 0.5 * c.y;
    double2 o;
    o.x = y0;
    o.y = y1;
    *reinterpret_cast<double2*>(y + r) = o;
}

struct Col17 { const double* p[17]; };
struct Col8 { double* p[8]; };

typedef double d2 __attribute__((ext_vector_type(2)));
template <int ROWS> struct RowT { typedef double T; };
template <> struct RowT<2> { typedef d2 T; };

template <int RES, int C, typename T>
__device__ __forceinline__ T load_col(const T* p) {
    if constexpr (RES >= 0 && C < 17 - RES) return __builtin_nontemporal_load(p);
    else return *p;
}
template <int RES, typename T, int C = 0>
__device__ __forceinline__ void load17(const Col17& P, int64_t r, T* v) {
    if constexpr (C < 17) {
        v[C] = load_col<RES, C, T>(reinterpret_cast<const T*>(P.p[C] + r));
        load17<RES, T, C + 1>(P, r, v);
    }
}

// ROWS = 2: two rows per lane, every column one 16-B load (the columns are
// 16-B aligned and followed by a halo, so the pair at an odd n's last row is
// readable; its second row is not stored)
template <bool STORE, int RES, bool LASTPLAIN, bool LOOP, int ROWS>
__global__ __launch_bounds__(256) void k_sweep17(Col17 P, Col8 Y, int64_t n) {
    typedef typename RowT<ROWS>::T T;
    constexpr int CH = 256 * ROWS;
    const int64_t nch = (n + CH - 1) / CH;
    const int64_t cstride = LOOP ? (int64_t)gridDim.x : nch;
    const int64_t rlast = (n - 1) / ROWS * ROWS;
    T acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0;
    T pn[17];
    {
        const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) * ROWS;
        load17<RES, T>(P, r < n ? r : rlast, pn);
    }
    for (int64_t ci = blockIdx.x; ci < nch; ci += cstride) {
        const int64_t r = (ci * 256 + threadIdx.x) * ROWS;
        const bool in = r < n;
        T v[17];
#pragma unroll
        for (int c = 0; c < 17; ++c) v[c] = in ? pn[c] : T(0.0);
        if (LOOP && ci + cstride < nch) {
            const int64_t r2 = ((ci + cstride) * 256 + threadIdx.x) * ROWS;
            load17<RES, T>(P, r2 < n ? r2 : rlast, pn);
        }
        if (STORE) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int c = 0; c < 17; ++c) acc[j] += v[c] * (0.01 * (c + j));
        }
        if (STORE && in) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (ROWS == 2) {
                    if (r + 1 < n) {
                        if (LASTPLAIN && j == 7) *reinterpret_cast<d2*>(Y.p[j] + r) = acc[j];
                        else __builtin_nontemporal_store(acc[j], reinterpret_cast<d2*>(Y.p[j] + r));
                    } else {
                        Y.p[j][r] = acc[j][0];
                    }
                } else {
                    if (LASTPLAIN && j == 7) Y.p[j][r] = acc[j];
                    else __builtin_nontemporal_store(acc[j], Y.p[j] + r);
                }
            }
        }
    }
    if constexpr (!STORE) {
        double a0, a1;
        if constexpr (ROWS == 2) { a0 = acc[0][0] + acc[0][1]; a1 = acc[1][0] + acc[1][1]; }
        else { a0 = acc[0]; a1 = acc[1]; }
        if (a0 == 1.2345) Y.p[0][(int64_t)blockIdx.x * 256 + threadIdx.x] = a1;
    }
}

// The attribution variants (RES = 3, one row per lane).  COEF: 0 immediates,
// 1 LDS table, 2 uniform loads of M; the table is k_rowapply's
// [M1 (17 x 8) | M2p (17 x 8) | M2y (8 x 8)], row-major.
typedef double d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int COEF>
__device__ __forceinline__ void coef_row(const double* Mc, int row, double* mrow) {
    if constexpr (COEF == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) mrow[j] = 0.01 * (row % 25 + j);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const d2 t = *reinterpret_cast<const d2*>(&Mc[row * 8 + j]);
            mrow[j] = t[0];
            mrow[j + 1] = t[1];
        }
    }
}
template <int COEF, bool GRAMT, bool STORE, bool CHAIN, bool LOOP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_sweep17c(Col17 P, Col8 Y, const double* __restrict__ M,
                                                  double* __restrict__ partial, int64_t n) {
    constexpr int RES = 3, TLD = 17, MSZ = 17 * 8 * 2 + 64;
    __shared__ double tile[GRAMT ? 256 * TLD : 1];
    __shared__ __attribute__((aligned(16))) double Ms[COEF == 1 ? MSZ : 2];
    const double* const Mc = COEF == 1 ? Ms : M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, g = lane >> 4;
    if (COEF == 1)
        for (int e = tid; e < MSZ; e += 256) Ms[e] = M[e];
    if (GRAMT)
        for (int e = tid; e < 256 * TLD; e += 256) tile[e] = 0.0;
    if (COEF == 1 || GRAMT) __syncthreads();
    const int64_t nch = (n + 255) / 256;
    const int64_t cstride = LOOP ? (int64_t)gridDim.x : nch;
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    double eacc = 0.0;
    double y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = 0.0;
    double pn[17];
    {
        const int64_t r = (int64_t)blockIdx.x * 256 + tid;
        load17<RES, double>(P, r < n ? r : n - 1, pn);
    }
    for (int64_t ci = blockIdx.x; ci < nch; ci += cstride) {
        asm volatile("" ::: "memory");
        const int64_t r = ci * 256 + tid;
        const bool in = r < n;
        double v[17];
#pragma unroll
        for (int c = 0; c < 17; ++c) v[c] = in ? pn[c] : 0.0;
        if (LOOP && ci + cstride < nch) {
            const int64_t r2 = (ci + cstride) * 256 + tid;
            load17<RES, double>(P, r2 < n ? r2 : n - 1, pn);
        }
        if (STORE || GRAMT) {
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = 0.0;
        }
#pragma unroll
        for (int c = 0; c < 17; ++c) {
            if (COEF != 2 || c % SWEEP_COEF_ROWS == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(y[j])::"memory");
            }
            double mrow[8];
            coef_row<COEF>(Mc, c, mrow);
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = __builtin_fma(v[c], mrow[j], y[j]);
        }
        if (CHAIN) {
            double y2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y2[j] = 0.0;
#pragma unroll
            for (int c = 0; c < 25; ++c) {
                if (COEF != 2 || c % SWEEP_COEF_ROWS == 0) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(y2[j])::"memory");
                }
                const double src = c < 17 ? v[c < 17 ? c : 0] : y[c >= 17 ? c - 17 : 0];
                double mrow[8];
                coef_row<COEF>(Mc, 17 + c, mrow);
#pragma unroll
                for (int j = 0; j < 8; ++j) y2[j] = __builtin_fma(src, mrow[j], y2[j]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = y2[j];
        }
        if (STORE && in) {
#pragma unroll
            for (int j = 0; j < 8; ++j) __builtin_nontemporal_store(y[j], Y.p[j] + r);
        }
        if (GRAMT) {
            double* trow = tile + tid * TLD;
#pragma unroll
            for (int c = 0; c < 8; ++c) trow[c] = v[c];
#pragma unroll
            for (int j = 0; j < 8; ++j) trow[8 + j] = y[j];
            trow[16] = v[8];
            wave_lds_sync();
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int row = wave * 64 + 4 * k + g;
                const double a = tile[row * TLD + c16];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
                eacc = eacc + tile[row * TLD + 16] * a;
            }
            wave_lds_sync();
        }
    }
    if constexpr (GRAMT) {  // the block's partials, as k_rowapply writes them (272 entries x gridDim.x)
        double* const red = tile;
        __syncthreads();
        if (wave > 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[((wave - 1) * 64 + lane) * 5 + q] = acc[q];
            red[((wave - 1) * 64 + lane) * 5 + 4] = eacc;
        }
        __syncthreads();
        if (wave == 0) {
            const int64_t nb = gridDim.x;
            double* out = partial + blockIdx.x;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double s = acc[q];
                for (int w = 0; w < 3; ++w) s = s + red[(w * 64 + lane) * 5 + q];
                out[(int64_t)(c16 * 16 + g + 4 * q) * nb] = s;
            }
            double e = eacc;
            for (int w = 0; w < 3; ++w) e = e + red[(w * 64 + lane) * 5 + 4];
            const double e1 = __shfl(e, c16 + 16, 64), e2 = __shfl(e, c16 + 32, 64), e3 = __shfl(e, c16 + 48, 64);
            if (g == 0) out[(int64_t)(256 + c16) * nb] = ((e + e1) + e2) + e3;
        }
    } else if constexpr (!STORE) {
        if (y[0] == 1.2345) Y.p[0][(int64_t)blockIdx.x * 256 + tid] = y[1];
    }
}

// second sweep (1024 blocks, grid-stride) and apply sweep (one row per thread) of one attribution variant
template <int COEF>
static void sweep_c(bool second, bool knob, int grid, const Col17& P, const Col8& Y, const double* M, double* partial,
                    int64_t n) {
    if (second) {
        if (knob) hipLaunchKernelGGL((k_sweep17c<COEF, true, false, false, true>), dim3(grid), dim3(256), 0, 0, P, Y, M, partial, n);
        else hipLaunchKernelGGL((k_sweep17c<COEF, false, false, false, true>), dim3(grid), dim3(256), 0, 0, P, Y, M, partial, n);
    } else {
        if (knob) hipLaunchKernelGGL((k_sweep17c<COEF, false, true, true, false>), dim3(grid), dim3(256), 0, 0, P, Y, M, partial, n);
        else hipLaunchKernelGGL((k_sweep17c<COEF, false, true, false, false>), dim3(grid), dim3(256), 0, 0, P, Y, M, partial, n);
    }
}

template <bool STORE, bool LASTPLAIN, bool LOOP, int ROWS>
static void sweep(int res, int grid, const Col17& P, const Col8& Y, int64_t n) {
    switch (res) {
        case 0: hipLaunchKernelGGL((k_sweep17<STORE, 0, LASTPLAIN, LOOP, ROWS>), dim3(grid), dim3(256), 0, 0, P, Y, n); break;
        case 1: hipLaunchKernelGGL((k_sweep17<STORE, 1, LASTPLAIN, LOOP, ROWS>), dim3(grid), dim3(256), 0, 0, P, Y, n); break;
        case 2: hipLaunchKernelGGL((k_sweep17<STORE, 2, LASTPLAIN, LOOP, ROWS>), dim3(grid), dim3(256), 0, 0, P, Y, n); break;
        case 3: hipLaunchKernelGGL((k_sweep17<STORE, 3, LASTPLAIN, LOOP, ROWS>), dim3(grid), dim3(256), 0, 0, P, Y, n); break;
        default: hipLaunchKernelGGL((k_sweep17<STORE, -1, LASTPLAIN, LOOP, ROWS>), dim3(grid), dim3(256), 0, 0, P, Y, n); break;
    }
}
template <bool STORE, bool LASTPLAIN, bool LOOP>
static void sweep(int rows, int res, int grid, const Col17& P, const Col8& Y, int64_t n) {
    if (rows == 2) sweep<STORE, LASTPLAIN, LOOP, 2>(res, grid, P, Y, n);
    else sweep<STORE, LASTPLAIN, LOOP, 1>(res, grid, P, Y, n);
}

int main(int argc, char** argv) {
    const bool coef_mode = argc > 1 && std::string(argv[1]) == "coef";
    const int N = 215;
    const int64_t n = (int64_t)N * N * N, P = (int64_t)N * N;
    uint16_t* id;
    CK(hipMalloc(&id, n * 2));
    CK(hipMemset(id, 0, n * 2));
    const int g2 = (int)((n / 2 + 255) / 256);
    const int64_t ldv = ((n + 2 * P + 64) + 63) / 64 * 64;
    double* pool;
    CK(hipMalloc(&pool, (size_t)(9 + 17) * ldv * 8));
    CK(hipMemset(pool, 0, (size_t)(9 + 17) * ldv * 8));
    // 256-B aligned origin (the library's columns start on 512 B), halo >= P + 32 rows on both sides;
    // -DRESIDENCY_PROBE_UNALIGNED: stencil_probe.hip's origin, 8 B past a 16-B boundary (one row per lane
    // only), where every non-temporal wave load straddles one more line and the policy gains nothing
#ifdef RESIDENCY_PROBE_UNALIGNED
    const int64_t H = P + 32 + (P & 1 ? 0 : 1);
#else
    const int64_t H = (P + 32 + 31) / 32 * 32;
#endif
    auto V = [&](int j) { return pool + (size_t)j * ldv + H; };
    auto Qc = [&](int j) { return pool + (size_t)(9 + j) * ldv + H; };
    std::vector<int> ho(256, 0);
    std::vector<double2> hv(256, make_double2(0.0, 0.0));
    const int64_t o7[7] = {-P, -N, -1, 0, 1, N, P};
    for (int e = 0; e < 7; ++e) {
        ho[e] = (int)o7[e] * 4 + 3;
        hv[e] = make_double2(e == 3 ? 6.0 : -1.0, e == 3 ? 6.0 : -1.0);
    }
    int* go;
    double2* gv;
    CK(hipMalloc(&go, 256 * 4));
    CK(hipMalloc(&gv, 256 * 16));
    CK(hipMemcpy(go, ho.data(), 256 * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(gv, hv.data(), 256 * 16, hipMemcpyHostToDevice));
    std::vector<hipEvent_t> ev(12);
    for (auto& evk : ev) CK(hipEventCreate(&evk));
    Col17 Pc;
    Col8 Yc;
    for (int c = 0; c < 9; ++c) Pc.p[c] = Qc(c);
    for (int c = 0; c < 8; ++c) Pc.p[9 + c] = V(c + 1);
    for (int c = 0; c < 7; ++c) Yc.p[c] = Qc(9 + c);
    Yc.p[7] = V(0);
    // form 0: one row per thread in all three sweeps; form 1: the Gram sweeps
    // in the library's shape (the library's pass B is one row per thread)
    // rows: rows per lane (1: 8-B loads, 2: 16-B loads)
    struct Variant { int form, rows, res, lastplain; };
    std::vector<Variant> vs;
    for (int form = 0; form < 2; ++form)
#ifdef RESIDENCY_PROBE_UNALIGNED
        for (int rows = 1; rows <= 1; ++rows)
#else
        for (int rows = 1; rows <= 2; ++rows)
#endif
            for (int lp = 0; lp < 2; ++lp)
                for (int res = -1; res <= 3; ++res) vs.push_back({form, rows, res, lp});
    const int PASSES = 4, steps = 6;
    if (coef_mode) {
        // the coefficient table (the emulation's immediates) and the Gram partials
        constexpr int MSZ = 17 * 8 * 2 + 64;
        std::vector<double> hm(MSZ);
        for (int row = 0; row < 42; ++row)
            for (int j = 0; j < 8; ++j) hm[row * 8 + j] = 0.01 * (row % 25 + j);
        double *gm, *gpart;
        CK(hipMalloc(&gm, MSZ * 8));
        CK(hipMemcpy(gm, hm.data(), MSZ * 8, hipMemcpyHostToDevice));
        CK(hipMalloc(&gpart, (size_t)1024 * 272 * 8));
        const int ga = (int)((n + 255) / 256);
        const char* cname[3] = {"imm", "lds", "glb"};
        for (int pass = 0; pass < 2; ++pass) {
            // ref: k_sweep17 in all three sweeps (the line "lib x1 res 3" of the full list)
            for (int vi = -1; vi < 12; ++vi) {
                const int coef = vi < 0 ? 0 : vi / 4, gramt = vi < 0 ? 0 : (vi >> 1) & 1, chain = vi < 0 ? 0 : vi & 1;
                double acc[11] = {0};
                for (int stp = 0; stp < steps; ++stp) {
                    CK(hipEventRecord(ev[0]));
                    for (int j = 0; j < 8; ++j) {
                        hipLaunchKernelGGL(k_pairtab, dim3(g2), dim3(256), 0, 0, V(j), V(j + 1), id, n, go, gv);
                        CK(hipEventRecord(ev[j + 1]));
                    }
                    sweep<false, false, true>(1, 3, 1024, Pc, Yc, n);
                    CK(hipEventRecord(ev[9]));
                    if (vi < 0) sweep<false, false, true>(1, 3, 1024, Pc, Yc, n);
                    else if (coef == 0) sweep_c<0>(true, gramt, 1024, Pc, Yc, gm, gpart, n);
                    else if (coef == 1) sweep_c<1>(true, gramt, 1024, Pc, Yc, gm, gpart, n);
                    else sweep_c<2>(true, gramt, 1024, Pc, Yc, gm, gpart, n);
                    CK(hipEventRecord(ev[10]));
                    if (vi < 0) sweep<true, false, false>(1, 3, ga, Pc, Yc, n);
                    else if (coef == 0) sweep_c<0>(false, chain, ga, Pc, Yc, gm, gpart, n);
                    else if (coef == 1) sweep_c<1>(false, chain, ga, Pc, Yc, gm, gpart, n);
                    else sweep_c<2>(false, chain, ga, Pc, Yc, gm, gpart, n);
                    CK(hipEventRecord(ev[11]));
                    CK(hipEventSynchronize(ev[11]));
                    CK(hipGetLastError());
                    if (stp == 0) continue;
                    for (int k = 0; k < 11; ++k) {
                        float ms;
                        CK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
                        acc[k] += ms * 1e3 / (steps - 1);
                    }
                }
                double tot = 0;
                for (int k = 0; k < 11; ++k) tot += acc[k];
                if (vi < 0) printf("{\"inloop\": \"lib x1 res 3\", \"variant\": \"ref\", ");
                else printf("{\"inloop\": \"lib x1 res 3 coef %s%s%s\", \"variant\": \"sweep17c\", \"coef\": \"%s\", \"gramt\": %d, \"chain\": %d, ",
                            cname[coef], gramt ? " gramt" : "", chain ? " chain" : "", cname[coef], gramt, chain);
                printf("\"pass\": %d, \"spmv_us\": [", pass);
                for (int k = 0; k < 8; ++k) printf("%.1f%s", acc[k], k < 7 ? ", " : "");
                printf("], \"gram_us\": %.1f, \"gram2_us\": %.1f, \"apply_us\": %.1f, \"total_us\": %.1f}\n", acc[8], acc[9],
                       acc[10], tot);
                fflush(stdout);
            }
        }
        CK(hipDeviceSynchronize());
        return 0;
    }
    for (int pass = 0; pass < PASSES; ++pass) {
        for (const Variant& vr : vs) {
            double acc[11] = {0};
            const int ga = (int)((n + 256 * vr.rows - 1) / (256 * vr.rows));
            for (int stp = 0; stp < steps; ++stp) {
                CK(hipEventRecord(ev[0]));
                for (int j = 0; j < 8; ++j) {
                    hipLaunchKernelGGL(k_pairtab, dim3(g2), dim3(256), 0, 0, V(j), V(j + 1), id, n, go, gv);
                    CK(hipEventRecord(ev[j + 1]));
                }
                for (int k = 0; k < 2; ++k) {
                    if (vr.form) sweep<false, false, true>(vr.rows, vr.res, 1024, Pc, Yc, n);
                    else sweep<false, false, false>(vr.rows, vr.res, ga, Pc, Yc, n);
                    CK(hipEventRecord(ev[9 + k]));
                }
                if (vr.lastplain) sweep<true, true, false>(vr.rows, vr.res, ga, Pc, Yc, n);
                else sweep<true, false, false>(vr.rows, vr.res, ga, Pc, Yc, n);
                CK(hipEventRecord(ev[11]));
                CK(hipEventSynchronize(ev[11]));
                CK(hipGetLastError());
                if (stp == 0) continue;
                for (int k = 0; k < 11; ++k) {
                    float ms;
                    CK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
                    acc[k] += ms * 1e3 / (steps - 1);
                }
            }
            double tot = 0;
            for (int k = 0; k < 11; ++k) tot += acc[k];
            printf("{\"inloop\": \"%s x%d res %d%s\", \"form\": \"%s\", \"rows\": %d, \"res\": %d, \"last_plain\": %d, \"pass\": %d, \"spmv_us\": [",
                   vr.form ? "lib" : "row", vr.rows, vr.res, vr.lastplain ? " lastplain" : "", vr.form ? "lib" : "row", vr.rows,
                   vr.res, vr.lastplain, pass);
            for (int k = 0; k < 8; ++k) printf("%.1f%s", acc[k], k < 7 ? ", " : "");
            printf("], \"gram_us\": %.1f, \"gram2_us\": %.1f, \"apply_us\": %.1f, \"total_us\": %.1f}\n", acc[8], acc[9],
                   acc[10], tot);
            fflush(stdout);
        }
    }
    CK(hipDeviceSynchronize());
    return 0;
}
