/*
 * calanczos.h -- C ABI of the MI355X-native CA-Lanczos hot path.
 *
 * Drop-in boundary for the MATLAB reference (magnusgrandin/ca-lanczos).  The
 * reference resolves every hot-path function by file name, so a MEX file of
 * the same name shadows the .m file.  Each entry point below
 * is what such a MEX shim binds; the comment on each cites
 * the reference interface it replaces.
 *
 * Conventions
 *  - Dense matrices are column-major double (MATLAB layout).  Host-pointer
 *    entry points take leading dimension == rows.
 *  - A is the n x n sparse symmetric matrix.  It is handed over once per
 *    context (cal_set_matrix_*), kept resident in HBM and reused by every
 *    call, as the SURVEY §8b "two tiers" design prescribes.
 *  - Every function returns an int status: 0 ok, < 0 error, > 0 warning.
 *    cal_last_error(ctx) holds the message of the last non-zero status.
 *  - Calls are synchronous (outputs valid on return) and a context may be
 *    used by one host thread at a time, like mexFunction.
 *  - Cell arrays of blocks ({Q1,Q2,...}) are passed as (nblocks, const
 *    double* const* blocks, const int* widths); a block of width 0 is the
 *    MATLAB empty matrix [].
 */
#ifndef CALANCZOS_H
#define CALANCZOS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAL_OK 0
#define CAL_ERR_ARG (-1)          /* bad argument (reference: disp()+return)        */
#define CAL_ERR_HIP (-2)          /* HIP runtime failure                            */
#define CAL_ERR_NOMATRIX (-3)     /* no matrix set on the context                   */
#define CAL_ERR_NUMERIC (-4)      /* NaN/Inf, Leja error() cases                    */
#define CAL_ERR_COMM (-5)         /* collective / halo failure                      */
#define CAL_ERR_UNSUPPORTED (-6)  /* option outside the built scope                 */
#define CAL_WARN_RANK_DEFICIENT 1 /* reference: disp('Rank deficient'), continues   */
#define CAL_WARN_BREAKDOWN 2      /* rho_t == 0 or beta == 0 (reference divides)    */

typedef struct cal_ctx cal_ctx;

/* ---- context lifecycle ------------------------------------------------- */
int cal_version(void);
int cal_device_count(int* count);
/* Create a context on HIP device `device` with its own stream. */
int cal_create(int device, cal_ctx** out);
void cal_destroy(cal_ctx* ctx);
const char* cal_last_error(const cal_ctx* ctx);
int cal_synchronize(cal_ctx* ctx);
/* Kernel-duration timer (HIP events on the context stream).  kind: "spmv",
 * "gram", "apply", "other", "allreduce", "halo" (the RCCL calls), "normest"
 * (the span of the implicit restart's normest on its own stream), "drive"
 * (the kernel that rewrites the diagonal: cal_set_diagonal, one launch per
 * driven time step), "all".
 * Returns the number of launches timed and their summed duration since the
 * last reset. */
int cal_timer_enable(cal_ctx* ctx, int on);
int cal_timer_read(cal_ctx* ctx, const char* kind, int64_t* count, double* total_ms);
/* The algorithmic HBM bytes of the timed launches of a kind
 * since the last reset (the roofline's numerator; 0 for launches that state
 * none). */
int cal_timer_bytes(cal_ctx* ctx, const char* kind, double* bytes);
int cal_timer_reset(cal_ctx* ctx);

/* ---- the sparse matrix A ------------------------------------------------ */
/* MATLAB mxArray sparse storage (CSC: jc colptr, ir rowidx, pr values, all
 * mwIndex = int64), transposed into CSR on the host, so the device holds A
 * (not A') for any A; rows keep ascending columns, MATLAB's accumulation
 * order.  Replaces the `A` argument of SpMV.m:6, ca_lanczos.m:24. */
int cal_set_matrix_csc(cal_ctx* ctx, int64_t n, const int64_t* jc, const int64_t* ir, const double* pr);
/* CSR with int64 row pointers and int32 column indices (SciPy layout). */
int cal_set_matrix_csr(cal_ctx* ctx, int64_t n, const int64_t* rowptr, const int32_t* colind, const double* val);
/* The 2n x 2n matrix blkdiag(H, H) of an n x n CSR H, built on the host and
 * handed to cal_set_matrix_csr: the real form of a complex problem whose
 * vectors are stacked, Re in rows [0, n), Im in rows [n, 2n) (the time
 * propagator, cal_prop_*).  Each half keeps H's rows, column offsets and row
 * patterns; the values are stored twice.  cal_matrix_info reports 2n.
 * With the "shared" format selected (cal_set_spmv_format) H alone is uploaded
 * and nothing is doubled: one copy of rowptr / col / val serves both halves
 * (2n < 2^31 and nnz(H) < 2^31; one rank).  cal_matrix_info still reports the
 * logical matrix, 2n rows and 2 nnz(H); cal_spmv_shared_info what is stored. */
int cal_set_matrix_csr_stacked(cal_ctx* ctx, int64_t n, const int64_t* rowptr, const int32_t* colind,
                               const double* val);
/* A complex Hermitian n x n CSR matrix H = A + iB (val_re, val_im; A real
 * symmetric, B real antisymmetric) as the real symmetric 2n x 2n matrix
 *     E(H) = [[A, -B], [B, A]]
 * on the same stacked vectors: E(H) [Re psi; Im psi] = [Re H psi; Im H psi],
 * so the time propagator (cal_prop_begin(ctx, n, ...)) and everything else that
 * takes cal_set_matrix_csr_stacked's matrix take this one (magnetic fields,
 * velocity gauge, rotating frames).  val_im == NULL is
 * cal_set_matrix_csr_stacked(ctx, n, rowptr, colind, val_re): same code, same
 * bits.  An all-zero val_im is not detected.
 * The imaginary part of every stored diagonal entry must be exactly 0
 * (CAL_ERR_ARG otherwise).  Hermiticity of the off-diagonal entries -- entry
 * (j, i) stored as the conjugate of entry (i, j) -- is the caller's contract
 * and is not checked, as symmetry is not for cal_set_matrix_csr.  Row pointers
 * and column indices are checked as cal_set_matrix_csr_stacked checks them.
 * With the "shared" format selected H is stored once: rowptr / col / val_re as
 * for blkdiag(H, H) plus one array of nnz(H) imaginary parts, 20 bytes per
 * nonzero of H (2n < 2^31, nnz(H) < 2^31, one rank).  Its SpMV forms, per stored
 * nonzero (a, b) with x0 = x[c], x1 = x[n + c], the top half's term
 * a*x0 - b*x1 and the bottom half's b*x0 + a*x1 (each product and the
 * difference / sum rounded separately) and sums each row's terms in stored
 * order from +0.0.  Such a matrix is a "shared" matrix in every other respect:
 * cal_spmv_shared_info, cal_set_diagonal / cal_get_diagonal (the real diagonal;
 * d[i] == d[n + i]) and the same CAL_ERR_UNSUPPORTED for normest, the Ritz
 * residuals and the restart drivers; cal_matrix_info reports 2n rows and
 * 4 nnz(H).
 * With any other format E(H) is built on the host and handed to
 * cal_set_matrix_csr (4 nnz(H) < 2^31): top row i lists H's row i as (c, a) in
 * stored order, then (n + c, -b) in stored order; bottom row n + i lists
 * (c, b), then (n + c, a); zeros are kept, so the pattern does not depend on
 * the values.  That matrix runs everything the library has.
 * Every eigenvalue of E(H) is double ([u; v] and [-v; u]): see DESIGN.md §4b
 * before running a long eigen-solve on it. */
int cal_set_matrix_csr_hermitian(cal_ctx* ctx, int64_t n, const int64_t* rowptr, const int32_t* colind,
                                 const double* val_re, const double* val_im);
/* *on = 1 when the resident matrix is a Hermitian H stored once (the "shared"
 * format with a non-NULL val_im), with H's row count and stored nonzeros;
 * zeros otherwise (the host-built embedding included). */
int cal_spmv_hermitian_info(cal_ctx* ctx, int* on, int64_t* n, int64_t* nnz_stored);
/* Row-slab of a distributed matrix: rows [row0, row0+nlocal) of the global
 * n_global x n_global matrix, global column indices.  Requires a communicator
 * (cal_comm_*) when nranks > 1. */
int cal_set_matrix_csr_dist(cal_ctx* ctx, int64_t n_global, int64_t row0, int64_t nlocal,
                            const int64_t* rowptr, const int64_t* colind_global, const double* val);
int cal_matrix_info(cal_ctx* ctx, int64_t* n_local, int64_t* nnz_local, int64_t* n_global, int64_t* nghost);
/* Rewrite / read the stored diagonal of the resident matrix in place: no new
 * upload, no new format analysis, every device pointer unchanged.  n must
 * equal n_local; d has one entry per row (the entry with col == row).  The
 * positions are looked up on the device at the first call on a matrix (one
 * host wait), later calls only enqueue.  cal_set_diagonal takes effect for
 * every later call on the context.
 * CAL_ERR_UNSUPPORTED (nothing is written, the message names the cause): a
 * communicator of several ranks or a slab of a distributed matrix; a matrix on
 * the row-pattern format (its values live in pattern tables: select "csr" or
 * "split" with cal_set_spmv_format before the matrix is set -- under "auto"
 * that includes the plain Laplacians, which need "split"); a row that stores
 * no diagonal entry, or more than one (an explicit 0.0 counts as stored).
 * CAL_ERR_ARG: a non-finite d, a wrong n, or a cal_lanczos_begin /
 * cal_std_lanczos_begin run open on the context; cal_set_diagonal also while
 * a propagator is open (it owns the diagonal; cal_get_diagonal is allowed
 * there and reads the 2n entries of blkdiag(H, H) as the last step left them). */
int cal_set_diagonal(cal_ctx* ctx, int64_t n, const double* d);
int cal_get_diagonal(cal_ctx* ctx, int64_t n, double* d);
/* CA matrix-powers kernel of a distributed banded matrix (window halo layout,
 * row-pattern format): each slab also stores the rows of its (depth-1)-band
 * deep ghost zone, so the s <= depth powers of matrix_powers_* / one
 * CA-Lanczos outer iteration need ONE halo exchange of q's s-band deep ghost
 * zone instead of s (the reference's SpMV.m / matrix_powers_*.m
 * are serial, the powers are bit-identical either way).  Applies at the next
 * cal_set_matrix_csr_dist; depth 1 turns it off; default 8.  mpk_info reports
 * the active depth (1 = off), the global band and the stored row count. */
int cal_set_mpk_depth(cal_ctx* ctx, int depth);
int cal_mpk_info(cal_ctx* ctx, int* depth, int64_t* band_l, int64_t* band_r, int64_t* n_rows);
/* Schedule the last matrix-powers call took: 0 one halo exchange per SpMV,
 * 1 one deep exchange, 2 one deep exchange on the RCCL stream overlapped
 * with the interior powers, 3 the split schedule without an exchange (one
 * rank, CAL_MPK_FAKE_BAND), 4 the host-staged twin of 2 (the exchange's
 * copies on the communicator's stream, its callbacks on a comm thread, the
 * same ev_q / ev_halo event graph); -1 before the first call. */
int cal_mpk_schedule(cal_ctx* ctx, int* schedule);
/* SpMV-class kernel launches the last matrix-powers call made on this rank
 * (one per power: split schedules count their powers, not their two-range
 * pieces); 0 before the first call. */
int cal_powers_launches(cal_ctx* ctx, int* launches);
/* Device storage of A, chosen at the next cal_set_matrix_*: "auto" (default:
 * row patterns when A has <= 65535 distinct rows of <= 32 entries, else
 * CSR), "csr", "pattern", "split" or "shared".  All are lossless and give bit-identical
 * SpMV results (same per-row summation order).
 * "split" forces the diagonal-split format for grid Hamiltonians H = K +
 * diag(V): a uniform 5- or 7-slot stencil K (offsets -P .. -1, 0, +1 .. +P, P
 * >= 256, in-plane reach <= 256, rows of at most 8 entries, a whole single
 * slab) on the plane-march kernel and the per-row diagonal as one streamed
 * vector; cal_set_matrix_* returns CAL_ERR_UNSUPPORTED for a matrix that does
 * not qualify.  "auto" takes it for a qualifying matrix that would otherwise
 * run on CSR or on the row / pair kernels; "csr" never does.  Everything but
 * the SpMV (residuals, normest's rescale) runs on the matrix's CSR copy, and
 * cal_spmv_format keeps reporting CSR for it.
 * "shared" (opt-in, never chosen by "auto") is the stacked matrix blkdiag(H, H)
 * of cal_set_matrix_csr_stacked with H stored once: its SpMV (modes 0, 1, 2 and
 * the fused Lanczos step) loads every col / val entry once and applies it to
 * both halves, each row summed in the stacked CSR kernel's order -- y is
 * bit-identical to the stacked "csr" context.  With it selected every other
 * cal_set_matrix_* but cal_set_matrix_csr_hermitian (which stores a complex
 * Hermitian H once in the same way) and a communicator of several ranks return
 * CAL_ERR_UNSUPPORTED (the message names cal_set_matrix_csr_stacked); it never
 * falls back to another storage.  On a shared matrix whatever reads the CSR
 * rows of the whole matrix returns CAL_ERR_UNSUPPORTED and names "csr" as the
 * way to get it: normest (orth 'periodic' / 'selective'), the Ritz residuals
 * (diagnostics, cal_compute_ritz_rnorm) and the restart drivers.
 * cal_set_diagonal needs d[i] == d[n + i] there (CAL_ERR_ARG otherwise: the
 * halves share one slot).  cal_spmv_format reports CSR for it. */
int cal_set_spmv_format(cal_ctx* ctx, const char* fmt);
/* The shared stacked format of the resident matrix: *on = 1 when H is stored
 * once, with H's row count and stored nonzeros; zeros otherwise. */
int cal_spmv_shared_info(cal_ctx* ctx, int* on, int64_t* n_half, int64_t* nnz_stored);
/* The diagonal-split format of the resident matrix: *on = 1 when its SpMV
 * runs there, with the plane stride P, the in-plane reach H and *neg1 = 1
 * when every off-diagonal is -1; zeros otherwise. */
int cal_spmv_split_info(cal_ctx* ctx, int* on, int64_t* P, int* H, int* neg1);
int cal_spmv_format(cal_ctx* ctx, int* is_pattern, int* npatterns, int* nentries);
/* Pair patterns of the row-pattern format (two rows per lane): number of
 * merged pair patterns, their table entries, and pairs on the per-row path. */
int cal_spmv_pair_info(cal_ctx* ctx, int* npairpatterns, int* nentries, int64_t* nsplit);
/* The plane march of the row-pattern format (k_spmv_planes, k_resid_planes:
 * a single slab whose canonical slots are -P .. +P with P >= 256 and the
 * other slots within 256 rows): the plane stride P, the in-plane reach H and
 * the key mode (0: uniform slot values keyed by slot-mask bytes, 1 / 2: 1-
 * or 2-byte pattern ids); P = 0, key_mode = -1 when it is not in use. */
int cal_spmv_plane_info(cal_ctx* ctx, int64_t* plane_P, int* plane_H, int* key_mode);
/* Where the s x s algebra between the block-orthogonalisation sweeps runs:
 * "device" (default: one kernel, no host round trip inside a block) or
 * "host".  Both give bit-identical results; "host" exists for testing. */
int cal_set_orth_coef(cal_ctx* ctx, const char* where);
/* Backend of normalize (tsqr.m) on the device: "auto" (default: Householder
 * TSQR for the host-pointer calls cal_tsqr / cal_normalize /
 * cal_project_and_normalize; CholQR2 fused into the CA-Lanczos sweeps, with
 * Householder TSQR whenever its Cholesky fails, i.e. kappa > ~1e8), "tsqr"
 * (Householder TSQR everywhere, the reference's algorithm; multi-GPU: the
 * local trees' roots are all-gathered over RCCL), "cholqr2" (CholQR2
 * everywhere, shifted CholQR3 when its Cholesky fails).  cal_tsqr is always
 * Householder TSQR.  get: 0 auto, 1 tsqr, 2 cholqr2. */
int cal_set_normalize(cal_ctx* ctx, const char* kind);
int cal_get_normalize(cal_ctx* ctx, int* kind);
/* Counters of the fused TSQR projectAndNormalize (Householder TSQR of Y with
 * the second projection folded into the R factor; blockorth.cpp
 * pn_tsqr_fold): blocks run, blocks declined (the explicit-Z TSQR path was
 * taken because the fold's loss-of-orthogonality estimate exceeded 1e-14),
 * and the last block's estimate.  Any pointer may be null. */
int cal_tsqr_fold_stats(cal_ctx* ctx, long long* runs, long long* declined, double* last_est);
/* The fused TSQR's acceptance threshold on its loss-of-orthogonality estimate
 * (default 1e-14, also the maximum): a block whose estimate exceeds it is
 * declined and redone on the explicit-Z path (projectAndNormalize.m:63-64
 * literally), so lowering it keeps the results within the bars.  0 declines
 * every block that takes the second projection, a negative tol every block
 * (the fallback's test hooks); NaN or a tol above 1e-14 (which would accept
 * folds the default declines) is an error. */
int cal_set_tsqr_fold_tol(cal_ctx* ctx, double tol);
/* Device-resident SpMV timing: `reps` launches of y = (A - shift I) x on
 * HBM-resident vectors (x = ones), HIP events around each launch on the
 * context stream; returns the mean and the minimum kernel time. */
int cal_bench_spmv(cal_ctx* ctx, int reps, double shift, double* mean_ms, double* min_ms);

/* ---- a1-a4: SpMV and the s-step matrix-powers kernel -------------------- */
/* Av = SpMV(A,v)                                       SpMV.m:6-8           */
int cal_spmv(cal_ctx* ctx, const double* v, double* Av);
/* V = matrix_powers_monomial(A,q,s); V is n x s        matrix_powers_monomial.m:6-12 */
int cal_matrix_powers_monomial(cal_ctx* ctx, const double* q, int s, double* V);
/* V = matrix_powers_newton(A,v,s,lambda,modifiedp); V is n x (s+1).
 * lambda = lambda_re + i*lambda_im (lambda_im may be NULL: real shifts).
 *                                                      matrix_powers_newton.m:15-54 */
int cal_matrix_powers_newton(cal_ctx* ctx, const double* v, int s, const double* lambda_re,
                             const double* lambda_im, int modifiedp, double* V);

/* ---- a5-a9: tall-skinny block orthogonalisation ------------------------- */
/* [Q,R] = tsqr(A): A n x m -> Q n x m, R m x m upper, diag(R) >= 0.   tsqr.m:7-12
 * Householder TSQR (LAPACK reflectors per tile, reduction tree), m <= 32, n >= m. */
int cal_tsqr(cal_ctx* ctx, int64_t n, int m, const double* A, double* Q, double* R);
/* [Q,R] = cholqr(X): G = X'X, R = chol(G), Q = X/R.                  cholqr.m:3-8 */
int cal_cholqr(cal_ctx* ctx, int64_t n, int m, const double* X, double* Q, double* R);
/* [X,R] = project(Q,X,doreorth); Xout may alias X; R[i] is widths[i] x m.  project.m:7-58 */
int cal_project(cal_ctx* ctx, int64_t n, int nblocks, const double* const* Q, const int* widths,
                int m, const double* X, int doreorth, double* Xout, double* const* R);
/* [Q,R,rank] = normalize(X,'None',tol).                               normalize.m:3-36 */
int cal_normalize(cal_ctx* ctx, int64_t n, int m, const double* X, double tol, double* Q, double* R,
                  int* rank);
/* [Q,R,rank] = normalize(X,opt,tol), opt "None" or "randomizeNullSpace"
 * (normalize.m:28-31,38-51: when rank < m, R = S*W' and Q = Q*U from svd(R),
 * then the null-space columns are replaced by rand (a fresh MT19937 stream,
 * seed 5489 -- cal_matlab_rand), projected against Q(:,1:rank) and tsqr'd).
 * Returns CAL_WARN_RANK_DEFICIENT when rank < m.  m <= 32. */
int cal_normalize_opt(cal_ctx* ctx, int64_t n, int m, const double* X, const char* opt, double tol, double* Q,
                      double* R, int* rank);
/* [QZ,RZ] = projectAndNormalize(Q,X,doreorth); RZ has nblocks+1 entries:
 * RZ[i] widths[i] x m, RZ[nblocks] m x m.  *reorth = 1 when the reference
 * would disp('second').                                    projectAndNormalize.m:3-90 */
int cal_project_and_normalize(cal_ctx* ctx, int64_t n, int nblocks, const double* const* Q,
                              const int* widths, int m, const double* X, int doreorth, double* QZ,
                              double* const* RZ, int* reorth, int* rank);

/* ---- a10-a14: the CA-Lanczos driver ------------------------------------- */
typedef struct cal_lanczos_info {
    int t;              /* outer iterations run                                 */
    int s;
    int n_reorth;       /* projectAndNormalize second passes ('second')         */
    int n_rank_deficient;
    int breakdown;      /* 1 if rho_t == 0 / beta == 0 was hit                  */
    double shifts[64];  /* Newton shifts (first 2s, Leja order; re part)        */
    double shifts_im[64];
    double prologue_ms; /* Newton prologue wall time                            */
    double loop_ms;     /* outer loop wall time (incl. diagnostics)             */
    double diag_ms;     /* of which diagnostics                                 */
    int n_orth_breaks;  /* periodic: full reorthogonalisations; selective: QR rebuilds */
    int n_ritz_locked;  /* selective: converged Ritz vectors in QR               */
    double norm_A;      /* normest(A) (periodic / selective)                    */
    int n_ritz_complex; /* selective: of n_ritz_locked, members of complex pairs */
} cal_lanczos_info;

/* [T,Q,rn,oe] = ca_lanczos(A,r,s,iter,basis,orth).           ca_lanczos.m:24-86
 * basis in {"monomial","newton"}, orth in {"local","full","periodic","selective"}.
 * Outputs (any may be NULL): T (s*t x s*t), Q (n x s*t), rn (t x s*t),
 * oe (t), reorth_flags (t).  t = ceil(iter/s).  diagnostics=0 skips the
 * per-iteration Ritz residuals / orthogonality error (rn, oe left zero);
 * they never feed back into T or Q (ca_lanczos.m:228-236). */
int cal_ca_lanczos(cal_ctx* ctx, const double* r, int s, int iter, const char* basis, const char* orth,
                   int diagnostics, double* T, double* Q, double* rn, double* oe, int* reorth_flags,
                   cal_lanczos_info* info);

/* rn = compute_ritz_rnorm(A,Q,Vp,Dp) for a real eigen-decomposition.  ca_lanczos.m:88-97
 * Q: n_local x k (host, column-major), Vp: k x k, d: the k eigenvalues
 * diag(Dp).  [d,ix] = sort(d,'descend') (stable); rn(i) = ||A x - l x|| /
 * ||l x|| with x = Q*Vp(:,ix(i)), l = d(ix(i)).  The diagnostics' device
 * path: X = Q*Vp on the matrix cores, then the batched residual kernel. */
int cal_compute_ritz_rnorm(cal_ctx* ctx, const double* Q, int k, const double* Vp, const double* d, double* rn);

/* Step-wise, device-resident form of the same loop (benchmarks, restart
 * drivers).  begin() normalises r and runs the basis set-up (Newton
 * prologue); step() runs one outer iteration (s SpMVs + block orth + T
 * update); get() copies the current T (sk x sk, ldt >= sk) and flags.
 * With diagnostics the iteration's rn / oe are computed late (rn one
 * iteration behind; oe of 'local' / 'full' runs of <= 128 columns at the
 * last step, from one Gram of Q): get() finishes whatever is pending, so
 * its rn / oe are always complete for the iterations run so far.  eig(T) of
 * iteration k runs on a host worker thread and is joined one step later: a
 * non-converging eig(T) is reported (CAL_ERR_NUMERIC) by step k+1 or by get(),
 * after step k+1 has already extended T. */
int cal_lanczos_begin(cal_ctx* ctx, const double* r, int s, int max_outer, const char* basis,
                      const char* orth);
int cal_lanczos_step(cal_ctx* ctx, int diagnostics);
int cal_lanczos_state(cal_ctx* ctx, int* k, int* s, int* reorth_last);
int cal_lanczos_get(cal_ctx* ctx, double* T, int ldt, double* rn, double* oe, int* reorth_flags,
                    cal_lanczos_info* info);
int cal_lanczos_get_Q(cal_ctx* ctx, int64_t col0, int ncols, double* Q);
int cal_lanczos_end(cal_ctx* ctx);

/* ---- f2: explicit restart ------------------------------------------------ */
typedef struct cal_restart_info {
    int num_restarts;      /* restarts run (<= 200)                                */
    int nconv;             /* eigenpairs returned                                  */
    int converged;         /* 1 if n_wanted eigenpairs converged                   */
    double norm_A;         /* normest(A)                                           */
    double max_ritz_norm;  /* largest beta|y_m| estimate among the returned pairs  */
    double ms;             /* wall time                                            */
} cal_restart_info;

/* [E,V,nres,rnorms,orth_err] = restarted_ca_lanczos(A,r,max_lanczos,
 * n_wanted_eigs,s,basis,orth,tol)  (restarted_ca_lanczos.m:4-198, restart
 * strategy 'largest').  orth in {"local","full"} (the reference defines no
 * periodic/selective inner solver).  Outputs: conv_eigs (n_wanted, descending;
 * info->nconv valid), Q_conv (n x n_wanted, may be NULL), rnorms (200 x
 * n_wanted column-major, rows 1..num_restarts, may be NULL; needs
 * diagnostics), orth_err (200, may be NULL; needs diagnostics). */
int cal_restarted_ca_lanczos(cal_ctx* ctx, const double* r, int max_lanczos, int n_wanted, int s, const char* basis,
                             const char* orth, double tol, int diagnostics, double* conv_eigs, double* Q_conv,
                             double* rnorms, double* orth_err, cal_restart_info* info);

/* ---- f3: implicit restart ------------------------------------------------ */
/* [conv_eigs,Q_conv,num_restarts] = impl_restarted_ca_lanczos(A,r,max_lanczos,
 * n_wanted_eigs,s,basis,orth,tol)  (impl_restarted_ca_lanczos.m:4-226).  The
 * reference file does not run; this is the implicit restart it
 * sets out to implement: k = max(n_wanted+4, s) kept vectors, p = s*floor(
 * (max_lanczos-k)/s) exact shifts by qrstep (:623-678) per restart, CA blocks
 * of lanczos_basic (:333-426) with orth 'full' (the only branch that is
 * defined: others return CAL_ERR_UNSUPPORTED), at most 40 restarts (:7).
 * Converged when the n_wanted largest-modulus Ritz pairs of T_k all have
 * ||r_k|||e_k'y| < tol*normest(A).  Outputs: conv_eigs (n_wanted,
 * descending), Q_conv (n x n_wanted, may be NULL), ritz_est (40 x n_wanted
 * column-major: the estimates after each restart, may be NULL).
 * Parity unpinned (no runnable reference): checked against analytic spectra
 * and scipy eigsh. */
int cal_impl_restarted_ca_lanczos(cal_ctx* ctx, const double* r, int max_lanczos, int n_wanted, int s,
                                  const char* basis, const char* orth, double tol, double* conv_eigs,
                                  double* Q_conv, double* ritz_est, cal_restart_info* info);

/* ---- Krylov time propagation psi(t+dt) = exp(-i*dt*H) psi(t) -------------- */
/* ca_lanczos_prop.m:3-135 driven as runLanczos.m:84-131 drives it, for a real
 * symmetric H and a complex psi = u + i v.  Hermitian Lanczos on psi has real
 * recurrence coefficients, so it is real CA-Lanczos on blkdiag(H, H)
 * (cal_set_matrix_csr_stacked) started from the stacked vector [u; v]: same
 * T, complex basis Q(1:n,:) + i Q(n+1:2n,:).  One rank only
 * (CAL_ERR_UNSUPPORTED with a communicator of more ranks). */
typedef struct cal_prop_info {
    int steps;            /* time steps taken                                    */
    int lsteps;           /* Lanczos vectors (k*s) of the last step              */
    int lsteps_max;       /* largest and ...                                     */
    long long lsteps_sum; /* ... summed lsteps over all steps                    */
    double residual;      /* |dt*b(k)*c(k*s)*nrm| of the last step (:123)        */
    double residual_max;  /* its maximum over all steps                          */
    double norm;          /* 2-norm of the current state                         */
    int nshifts;          /* Newton shifts in use (Leja order), 0: monomial      */
    double shifts[64];
    int breakdowns;       /* blocks dropped: breakdown or a non-finite residual  */
    int rank_deficient;   /* blocks normalize flagged 'Rank deficient' (kept, as
                             the reference keeps them: normalize.m:21-27)        */
    double ms;            /* wall time inside cal_prop_step                      */
} cal_prop_info;

/* out = nrm * Q_c * c on stacked halves (the propagator's combine kernel on
 * host data): Q is 2n x m (ld 2n), c = c_re + i c_im (m entries, m <= 512),
 *   out_re = Q(1:n,:) c_re - Q(n+1:2n,:) c_im,
 *   out_im = Q(1:n,:) c_im + Q(n+1:2n,:) c_re,
 * each output row one chain over ascending j, *norm2 (may be
 * NULL) = sum of out_re^2 + out_im^2.  Needs no matrix on the context. */
int cal_prop_combine(cal_ctx* ctx, int64_t n, int m, const double* Q, const double* c_re, const double* c_im,
                     double* out_re, double* out_im, double* norm2);

/* Step-wise propagator.  The context's matrix must have 2n rows (blkdiag(H,
 * H)).  psi_im may be NULL (real start).  1 <= s <= 31, s*max_blocks <= 512;
 * basis "monomial" or "newton".  With eigest (neig >= s values) the Newton
 * shifts are leja(real(eigest)) (:38-41); with none, the first step runs
 * lanczos(A,psi,2s,'local') (:33) and every later step reuses its shifts
 * (runLanczos.m:93-96).  The state, Q and the norm stay on the device. */
int cal_prop_begin(cal_ctx* ctx, int64_t n, const double* psi_re, const double* psi_im, int s, int max_blocks,
                   const char* basis, const double* eigest, int neig);
/* nsteps time steps of size dt.  Each: normalise, CA blocks with orth 'local'
 * (the library's second-pass rule where :78 passes doreorth = false), after
 * block k the residual |dt*b(k)*c(k*s)*nrm| with c = expm(-i*dt*T(1:ks,1:ks))
 * e_1 (:122-123); with adaptive != 0 the step stops at the first k with
 * residual < tol and k*s >= 3 (:124); psi <- nrm*Q_c*c.  A block that breaks
 * down (rho_t == 0, a non-finite T or residual) is dropped with those after
 * it and counted in the info; if it is the first block the call returns
 * CAL_WARN_BREAKDOWN and the state is unchanged.  A block that normalize
 * flags 'Rank deficient' is counted and kept, as the reference keeps it. */
int cal_prop_step(cal_ctx* ctx, double dt, double tol, int adaptive, int nsteps);
/* The state (either pointer may be NULL) and the counters; the only
 * device-to-host copy of the state. */
int cal_prop_get(cal_ctx* ctx, double* psi_re, double* psi_im, cal_prop_info* info);
int cal_prop_end(cal_ctx* ctx);

/* Observables of the state after each later time step, reduced on the device inside the combine sweep.
 * W: n x nw column-major real diagonal operators (0 <= nw <= 4; NULL when nw = 0).  phi_re / phi_im: n x nphi
 * reference states (0 <= nphi <= 4; phi_im may be NULL = real).  energy != 0 also records <psi|H|psi> (one more SpMV
 * per step).  Replaces an earlier set and clears the history; nw = nphi = energy = 0 switches them off.
 * CAL_ERR_ARG without an active propagator or outside the caps. */
int cal_prop_set_observables(cal_ctx* ctx, int nw, const double* W, int nphi, const double* phi_re,
                             const double* phi_im, int energy);
/* Row k (one per completed step since the set): [t, norm2, energy (NaN when off), <W_0>..<W_{nw-1}>,
 * Re<phi_0|psi>, Im<phi_0|psi>, ...], t the time since cal_prop_begin, <W_k> = sum W_k |psi|^2, <phi|psi> =
 * sum conj(phi) psi.  A step that ends in CAL_WARN_BREAKDOWN records no row.  out == NULL: only *nrows / *ncols.
 * Copies rows [first, first+count), row-major with *ncols = 3 + nw + 2 nphi doubles each. */
int cal_prop_get_observables(cal_ctx* ctx, int64_t first, int64_t count, double* out, int64_t* nrows, int* ncols);
/* The OBS kernel on host data, as cal_prop_combine is for the plain one: same out / norm2 (to the bit), plus
 * sums[nw + 2 nphi] in the order of a history row's last columns.  Per output row, t = out_re[i], b = out_im[i]:
 *   W_k  :  d = t*t;  d = d + b*b;  acc = acc + W_k[i]*d
 *   phi_r:  re = re + pr[i]*t;  re = re + pi[i]*b;  im = im + pr[i]*b;  im = im - pi[i]*t
 * summed over the rows in the squared norm's fixed order. */
int cal_prop_combine_obs(cal_ctx* ctx, int64_t n, int m, const double* Q, const double* c_re, const double* c_im,
                         int nw, const double* W, int nphi, const double* phi_re, const double* phi_im,
                         double* out_re, double* out_im, double* norm2, double* sums);

/* ---- an absorbing boundary: a mask applied at the end of every time step ---- */
/* mask: n doubles, 0 <= mask[i] <= 1 (1 in the interior, ramping down towards
 * the edge), copied to the device; NULL switches the absorber off.  From then
 * on every completed time step (each sub-step of a driven scheme is one) ends
 * with, inside the combine sweep,
 *   u = nrm*Q_c*c;  psi' = mask .* u;  absorbed = sum_i (1 - mask[i]^2) |u_i|^2
 * the observables, the energy and the squared norm that normalises the next
 * step are those of psi', the state as stored.  This is the first-order
 * splitting of a complex absorbing potential Gamma = -ln(mask)/dt: the mask
 * belongs to the dt it is stepped with.  Needs an active propagator.
 * CAL_ERR_ARG without one, or when a value is not finite or outside [0, 1];
 * then an earlier absorber stays as it was.  Replaces an earlier mask and
 * clears the absorbed history (not the observables'); cal_prop_end and a new
 * cal_prop_begin drop the absorber. */
int cal_prop_set_absorber(cal_ctx* ctx, const double* mask);
/* One row [t, absorbed] per completed step since the absorber was set, t as in
 * cal_prop_get_observables.  A step that ends in CAL_WARN_BREAKDOWN leaves the
 * state unmasked and records no row.  out == NULL: only *nrows.  Copies rows
 * [first, first+count), two doubles each. */
int cal_prop_get_absorbed(cal_ctx* ctx, int64_t first, int64_t count, double* out, int64_t* nrows);
/* The masked kernel on host data, as cal_prop_combine_obs is for the
 * observables: with ut, ub the two sums of row i as cal_prop_combine leaves
 * them and m = mask[i] (n values, finite, in [0, 1]),
 *   d = ut*ut;  d = d + ub*ub;  p = m*m;  g = 1.0 - p;  acc = acc + g*d
 *   out_re[i] = m*ut;  out_im[i] = m*ub
 * *norm2 and sums[nw + 2 nphi] (cal_prop_combine_obs's, either count may be 0)
 * are those of out; *absorbed (may be NULL) = acc summed in the squared norm's
 * fixed order. */
int cal_prop_combine_masked(cal_ctx* ctx, int64_t n, int m, const double* Q, const double* c_re, const double* c_im,
                            const double* mask, int nw, const double* W, int nphi, const double* phi_re,
                            const double* phi_im, double* out_re, double* out_im, double* norm2, double* absorbed,
                            double* sums);

/* ---- a time-dependent potential H(t) = H0 + sum_k f_k(t) diag(W_k) ---- */
/* W: n x nk column-major real diagonal operators, 0 <= nk <= 4, copied to the
 * device.  H0's diagonal V0 is taken from the context's matrix as it is at
 * this call and kept on the device; from then on the propagator owns the
 * diagonal.  nk = 0 switches the drive off and puts V0 back; cal_prop_end and
 * a new cal_prop_begin do the same, so the matrix is left as the caller set
 * it.  Needs an active propagator (CAL_ERR_ARG without one, or with nk outside
 * the cap or a non-finite W); CAL_ERR_UNSUPPORTED as cal_set_diagonal, with
 * the matrix and an earlier drive untouched. */
int cal_prop_set_drive(cal_ctx* ctx, int nk, const double* W);
/* cal_prop_step under the drive: before time step it = 0 .. nsteps-1 one
 * kernel sets, in both halves of blkdiag(H, H), row i's diagonal to
 *   d = V0[i];  for k = 0 .. nk-1 (ascending):  p = f[it*ldf + k] * W_k[i];  d = d + p
 * (product and sum rounded separately: a NumPy loop reproduces the bits), then
 * the step is exactly cal_prop_step's.  ldf >= nk; a non-finite amplitude in
 * the nsteps rows is CAL_ERR_ARG before anything runs.  The library does not
 * interpret the rows of f: at which times they are sampled is the caller's
 * integration scheme (the midpoint rule takes f(t + dt/2)).  The energy an
 * observables row records is <psi'|H|psi'> with the H of that step.
 * cal_prop_step keeps working while a drive is set: it steps under whatever H
 * the last driven step left (H0 before the first).  The Newton shifts stay
 * those of the first step unless cal_prop_refresh_shifts is called. */
int cal_prop_step_driven(cal_ctx* ctx, double dt, double tol, int adaptive, int nsteps, const double* f, int ldf);
/* Forget the Newton shifts the first step's prologue (or eigest) left: the
 * next step's prologue computes them from the current H and state.  Right
 * after a drive has moved H's spectrum by an amount comparable to its width;
 * unnecessary for a drive small against it.  No-op for the monomial basis. */
int cal_prop_refresh_shifts(cal_ctx* ctx);

/* ---- a nonlinear term: i d/dt psi = (H0 + sum_k f_k(t) diag(W_k) + g |psi|^2) psi ---- */
/* The Gross-Pitaevskii / nonlinear Schroedinger equation.  After this call
 * cal_prop_step and cal_prop_step_driven take nonlinear steps: before a
 * Krylov build one kernel forms the diagonal from the state on the device
 * and writes it, with the drive, in one launch (no copy of the state to the
 * host).  For row i, with A = ua + i va and (two states only) B = ub + i vb,
 * every product and sum rounded separately, so a NumPy loop gives the bits:
 *   ra = ua*ua;  ra = ra + va*va
 *   rb = ub*ub;  rb = rb + vb*vb                                  (two states)
 *   d  = V0[i];  for k ascending:  p = f_k*W_k[i];  d = d + p     (the drive's chain)
 *   p  = ga*ra;  d = d + p
 *   p  = gb*rb;  d = d + p                                        (two states)
 * and d goes to row i's diagonal in both halves of blkdiag(H, H).
 * density "frozen": ga = g, A = psi_n, one state; then the step is
 *   cal_prop_step's.  First order in dt, one Krylov build per step.
 * density "midpoint" (predictor-corrector, second order, two builds per step):
 *   (a) a frozen step from psi_n to a provisional psi* (no observables, no
 *       absorber, no history row; the time and info.steps do not advance);
 *   (b) ga = gb = 0.5*g, A = psi_n, B = psi*;
 *   (c) the step proper from psi_n, with everything that is set.
 *   The same row of amplitudes f serves both passes.
 * If a pass breaks down the call returns CAL_WARN_BREAKDOWN with the state
 * psi_n unchanged.  cal_prop_info under "midpoint": breakdowns and
 * rank_deficient count the blocks of both builds of a step; steps, lsteps,
 * lsteps_max, lsteps_sum, residual and residual_max are the corrector's alone.  Under cal_prop_step the f_k are those of the most recent
 * driven step (zeros before the first).  The propagator owns the diagonal
 * from the first of {cal_prop_set_drive, cal_prop_set_nonlinear} to the last
 * of them that goes off (g = 0, nk = 0, cal_prop_end, a new cal_prop_begin);
 * then H0's diagonal is put back.  g = 0 with nothing set is a no-op.
 * CAL_ERR_ARG for a NULL context, no active propagator, a non-finite g or a
 * density other than the two; CAL_ERR_UNSUPPORTED as cal_prop_set_drive, with
 * the matrix untouched.  Setting the term clears its history.
 * The conserved Gross-Pitaevskii energy is a column of cal_prop_get_energetics
 * (the energy observable stays <psi'|H|psi'> with the H stored in the matrix:
 * under "midpoint" H0 + drive + g (|psi_n|^2 + |psi*|^2)/2).  Not built: more
 * than second order in the nonlinear part (a "cf4" drive's sub-steps are
 * nonlinear steps each). */
int cal_prop_set_nonlinear(cal_ctx* ctx, double g, const char* density);
/* One row [t_n, sum_i |psi_n,i|^4] per completed step since the term was set,
 * psi_n the state the step started from and t_n its time (g/2 times the sum
 * is the interaction energy).  Summed by the density kernel: per row q =
 * ra*ra, the rows of a 256-row block by a wave tree and the four waves in
 * order, the blocks in the library's fixed order.  It arrives with the
 * step's squared norm, in the same transfer.  out == NULL: only *nrows.
 * Copies rows [first, first+count), two doubles each. */
int cal_prop_get_nonlinear(cal_ctx* ctx, int64_t first, int64_t count, double* out, int64_t* nrows);

/* ---- imaginary time: psi <- sqrt(N) exp(-tau H[psi]) psi / ||.||, ground states ---- */
/* on != 0: from now on cal_prop_step and cal_prop_step_driven take dt as the
 * imaginary-time step tau.  The Krylov build is unchanged; after block k
 *   c = expm(-tau (T(1:ks,1:ks) - T(1,1) I)) e_1           (cal_expm_real_col1)
 *   cc = sum_j c_j^2 (j ascending);  sc = sqrt(N) / sqrt(cc)
 * and the coefficients handed to the combine sweep are a = sc*c, b = 0: the
 * kernel is the real-time one, and the new state has the squared norm N up to
 * Q's loss of orthogonality (the measured squared norm still normalises the
 * next start vector).  N is the state's squared norm when the mode went on.
 * The adaptive / reported residual is |tau b(k) c(ks)| sc.  Under
 * cal_prop_set_nonlinear "frozen" and "midpoint" keep their meaning (the
 * predictor's coefficients are normalised the same way); observables, energy,
 * absorber and drive work as in real time, on every matrix cal_prop_begin
 * takes; t accumulates tau.  on = 0 returns to real time
 * (CAL_ERR_UNSUPPORTED on a real-state propagator).  CAL_ERR_ARG without an
 * active propagator. */
int cal_prop_set_imaginary_time(cal_ctx* ctx, int on);
/* One row [t_n, N_n, mu_n, E_n, res_n] per completed step since
 * cal_prop_begin, in real and in imaginary time, of the state psi_n the step
 * started from (N_n its squared norm).  Q(:,1) = psi_n/||psi_n||, so with T
 * of the step's first Krylov build (under "midpoint" the predictor's, whose
 * matrix H0 + drive + g |psi_n|^2 is self-consistent for psi_n):
 *   mu_n  = T(1,1)              = <psi_n|H[psi_n]|psi_n>/N_n   (the chemical potential)
 *   res_n = ||T(2:ks,1)||_2     = ||H[psi_n] psi_n - mu_n psi_n|| / sqrt(N_n)
 *   E_n   = N_n mu_n - (g/2) sum_i |psi_n,i|^4                 (N_n mu_n without a nonlinear term)
 * no kernel and no sweep: the sum is the one cal_prop_get_nonlinear records.
 * In real time E_n is the conserved Gross-Pitaevskii energy, at that step's
 * drive amplitudes.  A step that ends in CAL_WARN_BREAKDOWN records no row.
 * out == NULL: only *nrows.  Copies rows [first, first+count), five doubles each. */
int cal_prop_get_energetics(cal_ctx* ctx, int64_t first, int64_t count, double* out, int64_t* nrows);
/* The real-state propagator: imaginary time on H itself.  The ground state of
 * a real symmetric H is real, with or without g |psi|^2, so the state is one
 * real device vector of n rows and the context's matrix the n x n H
 * (cal_set_matrix_csr / _csc, in whatever SpMV format the upload chose): half
 * the rows and half the bytes of every SpMV and sweep of the stacked route.
 * Imaginary time is on from the start (N = psi'psi) and cannot be switched
 * off.  cal_prop_step, _step_driven, _set_drive, _set_nonlinear (both
 * densities; the density kernel's REAL instantiation: ra = ua*ua, rb = ub*ub,
 * the rest of its chain unchanged), _get_nonlinear, _get_energetics,
 * _refresh_shifts, _get (psi_im, when given, is filled with zeros) and _end
 * work as on the stacked propagator; cal_prop_set_observables takes W and
 * energy (nphi > 0: CAL_ERR_UNSUPPORTED), cal_prop_set_absorber is refused.
 * CAL_ERR_UNSUPPORTED, naming the stacked propagator, for a matrix of 2n rows
 * (a stacked matrix), a "shared" or Hermitian matrix, or a communicator of
 * several ranks; then an open propagator stays as it was. */
int cal_prop_begin_real(cal_ctx* ctx, int64_t n, const double* psi, int s, int max_blocks, const char* basis,
                        const double* eigest, int neig);
/* The real state's combine kernel (k_prop_combine, REAL) on host data, as
 * cal_prop_combine_obs is for the stacked kernel: Q is n x m (ld n), a has m
 * entries (m <= 512),
 *   out[i] = sum_j Q[i,j] a_j     t = +0.0; j ascending: t = t + Q[i,j]*a_j
 * *norm2 (may be NULL) = sum out^2 and, for k < nw <= 4, sums[k] = sum_i
 * W_k[i] out[i]^2 (per row d = t*t; acc = acc + W_k[i]*d), both in the squared
 * norm's fixed order.  W: n x nw column-major (NULL when nw = 0).
 * Needs no matrix on the context.  The device copy of Q has the library's own
 * padded leading dimension (16-byte accesses).  cal_prop_combine_real_ld takes
 * Q with a host leading dimension ldq >= n and, when ldq > n, keeps it on the
 * device: an odd ldq runs the kernel's 8-byte accesses. */
int cal_prop_combine_real(cal_ctx* ctx, int64_t n, int m, const double* Q, const double* a, int nw, const double* W,
                          double* out, double* norm2, double* sums);
int cal_prop_combine_real_ld(cal_ctx* ctx, int64_t n, int m, const double* Q, int64_t ldq, const double* a, int nw,
                             const double* W, double* out, double* norm2, double* sums);

/* [T,Q,lsteps] = ca_lanczos_prop(A,r0,s,m,dt,tol,basis,eigest,adaptive)
 * (ca_lanczos_prop.m:3-135) with r0 = r_re + i r_im (r_im may be NULL) on the
 * stacked matrix: T is *lsteps x *lsteps (ld *lsteps; room for s*m squared),
 * Q_re / Q_im n x *lsteps (room for n x s*m; either may be NULL). */
int cal_ca_lanczos_prop(cal_ctx* ctx, int64_t n, const double* r_re, const double* r_im, int s, int m, double dt,
                        double tol, const char* basis, const double* eigest, int neig, int adaptive, double* T,
                        double* Q_re, double* Q_im, int* lsteps);

/* ---- standard Lanczos: [T,Q,ritz_rnorm,orth_err] = lanczos(A,r,maxiter,orth) */
/* lanczos.m:18-311, device-resident, the other half of the reference's
 * ca_lanczos / lanczos comparisons.  orth is "local", "full", "periodic" or
 * "selective" (anything else: CAL_ERR_ARG, as is maxiter < 1 or > n).  One
 * Lanczos step is the fused SpMV mode (y = A q_j - beta_{j-1} q_{j-1} with the
 * block partials of y'q_j) and two vector kernels; alpha and beta^2 stay on the
 * device, so "local" and "full" enqueue their steps without a host round trip.
 * "periodic" and "selective" read alpha_j, beta_j on the host every step.  In
 * "periodic" the reference's window Q(:,j-5:j+1) is clamped to start at column
 * 1 for j <= 6 (the reference indexes out of range there) and the earlier
 * block is then empty.  One rank only (CAL_ERR_UNSUPPORTED with a communicator
 * of more ranks). */
typedef struct cal_std_lanczos_info {
    int steps;           /* Lanczos steps kept (columns of T)                   */
    int breakdown;       /* 1: beta_j == 0 or non-finite; steps is cut before it */
    int fused;           /* 1: the fused SpMV mode ran, 0: MODE 0 + k_pro_dot   */
    int n_orth_breaks;   /* periodic: reorthogonalisations; selective: QR rebuilds */
    int n_ritz_locked;   /* selective                                           */
    double norm_A;       /* normest(A) (periodic / selective)                   */
    double loop_ms, diag_ms;
} cal_std_lanczos_info;

/* One call: T is m x m (ld m, m = maxiter), its leading steps x steps block
 * filled and the rest zero; Q n x m (may be NULL; columns past steps zero); rn
 * m x m, row j = step j (ld m; may be NULL); oe m entries (may be NULL); rn /
 * oe are written with diagnostics != 0 only.  A beta_j that is not finite and
 * positive cuts steps to j and returns CAL_WARN_BREAKDOWN. */
int cal_lanczos(cal_ctx* ctx, const double* r, int maxiter, const char* orth, int diagnostics, double* T, double* Q,
                double* rn, double* oe, cal_std_lanczos_info* info);
/* Step-wise.  keep_Q = 0 ("local" only, else CAL_ERR_ARG) keeps a ring of
 * three columns: O(n) memory, the same T to the bit, no get_Q, no diagnostics. */
int cal_std_lanczos_begin(cal_ctx* ctx, const double* r, int maxiter, const char* orth, int keep_Q);
/* nsteps more steps (CAL_ERR_ARG past maxiter).  "local" / "full" without
 * diagnostics only enqueue: a breakdown shows in cal_std_lanczos_get. */
int cal_std_lanczos_step(cal_ctx* ctx, int nsteps, int diagnostics);
/* alpha, beta (steps entries each; beta_j of a breakdown is stored as 0), rn
 * (ld maxiter), oe; every pointer may be NULL.  Waits for the enqueued steps. */
int cal_std_lanczos_get(cal_ctx* ctx, double* alpha, double* beta, double* rn, double* oe, cal_std_lanczos_info* info);
int cal_std_lanczos_get_Q(cal_ctx* ctx, int64_t col0, int ncols, double* Q);
int cal_std_lanczos_end(cal_ctx* ctx);
/* The fused kernel on host data: y = A x - sqrt(beta2) xprev (xprev may be
 * NULL: y = A x, the bits of cal_spmv), *dot = y'x summed in a fixed order.
 * CAL_ERR_UNSUPPORTED when the matrix sits on an SpMV kernel without the mode. */
int cal_spmv_lanczos(cal_ctx* ctx, const double* x, const double* xprev, double beta2, double* y, double* dot);
/* *fused = 1 when the context's matrix takes the fused mode */
int cal_spmv_lanczos_fused(cal_ctx* ctx, int* fused);

/* ---- multi-GPU (row slabs, RCCL over xGMI) ------------------------------ */
/* 128-byte RCCL unique id; broadcast it out of band (e.g. torch.distributed). */
int cal_comm_unique_id(void* id128);
int cal_comm_init_rccl(cal_ctx* ctx, int nranks, int rank, const void* id128);
/* Communicator statistics since the last reset (reset != 0 zeroes them after
 * reading): stats[0] ranks, [1] kind (0 none, 1 RCCL, 2 host-staged), [2]
 * ncclCommCount (-1 unless RCCL), [3] all-reduces issued, [4] doubles they
 * carried, [5] halo exchanges, [6] doubles exchanged (sent + received), [7]
 * rows computed by SpMV launches (with the CA matrix powers: the slab's rows
 * plus the shrinking ghost-zone ranges).  nstats <= 8.  The timer kinds
 * "allreduce" and "halo" time the RCCL calls (cal_timer_read). */
int cal_comm_stats(cal_ctx* ctx, int64_t* stats, int nstats, int reset);
/* Host-staged communicator (tests, CPU rendezvous): device buffers are
 * staged through pinned host memory and handed to these callbacks.  The
 * callbacks run on the caller's thread, except with the opt-in overlapped
 * matrix-powers schedule (environment CAL_MPK_OVERLAP=1, a rehearsal of the
 * RCCL schedule): there the exchange callback runs on a library-owned thread
 * while the caller's thread enqueues the interior powers, so the transport
 * must allow calls from another thread (MPI_THREAD_MULTIPLE or
 * MPI_THREAD_SERIALIZED with no concurrent use by the caller). */
typedef int (*cal_allreduce_fn)(void* user, double* buf, int64_t count);
typedef int (*cal_exchange_fn)(void* user, int peer, const double* send, int64_t nsend, double* recv,
                               int64_t nrecv);
int cal_comm_init_host(cal_ctx* ctx, int nranks, int rank, cal_allreduce_fn allreduce,
                       cal_exchange_fn exchange, void* user);
int cal_comm_info(cal_ctx* ctx, int* nranks, int* rank, int* kind);

#ifdef __cplusplus
}
#endif
#endif /* CALANCZOS_H */
