"""NumPy references of the Hermitian stored-once SpMV (k_spmv_stacked, HERM true;
test_hermitian_host.py, test_gpu_hermitian.py): y = E(H) x with E(H) =
[[A, -B], [B, A]] for the complex Hermitian CSR H = A + iB on the stacked
vector x = [x0; x1] of 2n rows.

  * herm_chain: the kernel's order contract (include/calanczos.h).  Per stored
    nonzero (a, b) of row i at column c, with x0 = x[c], x1 = x[n + c],
        t0 = a*x0;  t1 = b*x1;  pt = t0 - t1      (the top half's term)
        u0 = b*x0;  u1 = a*x1;  pb = u0 + u1      (the bottom half's term)
    every product, the difference and the sum rounded separately; then
    y[i] = the pt of the row, y[n + i] = its pb, each summed sequentially in
    stored order from +0.0.
  * rowsum_chain: the CSR kernel's arithmetic on any real CSR matrix (rounded
    products, each row summed in stored order from +0.0) -- the stacked "csr"
    context on blkdiag(A, A) or on E(H), and "shared" on A.
  * row_bar: the project's summation bar per row (tests/prop_obs_ref.py): a
    float sum of N products whose absolute values sum to S is within (N + 8)
    eps S of the exact sum in any order.  A row of k nonzeros has N = 2k
    products per half and S = sum_j (|a_j| + |b_j|)(|x0_j| + |x1_j|), which
    bounds either half's sum of absolute products.
  * epilogue / lanczos_epilogue: the shift epilogues of modes 1 and 2 and the
    fused Lanczos step's subtraction, in the kernels' rounding order.
"""
import numpy as np

EPS = np.finfo(float).eps


def _parts(H):
    a = np.ascontiguousarray(H.data.real, dtype=np.float64)
    b = np.ascontiguousarray(H.data.imag, dtype=np.float64) if np.iscomplexobj(H.data) else np.zeros(len(a))
    return a, b


def _rowsums(indptr, terms):
    """Each row's terms summed sequentially in stored order from +0.0."""
    lens = np.diff(indptr)
    start = np.asarray(indptr[:-1], dtype=np.int64)
    y = np.zeros(len(lens))
    for j in range(int(lens.max()) if len(lens) else 0):
        m = lens > j
        y[m] = y[m] + terms[start[m] + j]
    return y


def herm_chain(H, x, val_im=None):
    """y = E(H) x in k_spmv_stacked's order (HERM true).  val_im replaces H's imaginary parts
    (e.g. zeros: the Hermitian path on a real matrix)."""
    n = H.shape[0]
    a, b = _parts(H)
    if val_im is not None:
        b = np.asarray(val_im, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    x0, x1 = x[:n][H.indices], x[n:][H.indices]
    t0 = a * x0
    t1 = b * x1
    pt = t0 - t1
    u0 = b * x0
    u1 = a * x1
    pb = u0 + u1
    return np.concatenate([_rowsums(H.indptr, pt), _rowsums(H.indptr, pb)])


def rowsum_chain(A, x):
    """y = A x as the CSR kernel sums it (any real CSR A)."""
    return _rowsums(A.indptr, np.asarray(A.data, dtype=np.float64) * np.asarray(x, dtype=np.float64)[A.indices])


def shared_chain(A, x):
    """The "shared" / stacked kernels on blkdiag(A, A)."""
    n = A.shape[0]
    return np.concatenate([rowsum_chain(A, x[:n]), rowsum_chain(A, x[n:])])


def row_bar(H, x):
    """(2k + 8) eps S per row of H, tiled to both halves."""
    n = H.shape[0]
    a, b = _parts(H)
    x = np.abs(np.asarray(x, dtype=np.float64))
    w = (np.abs(a) + np.abs(b)) * (x[:n][H.indices] + x[n:][H.indices])
    S = np.zeros(n)
    np.add.at(S, np.repeat(np.arange(n), np.diff(H.indptr)), w)
    k = np.diff(H.indptr)
    return np.tile((2 * k + 8) * EPS * S, 2)


def exact_product(H, x):
    """[Re(H psi); Im(H psi)] in complex128 (scipy's product)."""
    n = H.shape[0]
    z = H @ (np.asarray(x[:n], dtype=np.float64) + 1j * np.asarray(x[n:], dtype=np.float64))
    return np.concatenate([z.real, z.imag])


def epilogue(s, x, shift=None, im2=None, xprev=None):
    """spmv_epilogue: y = s - shift*x (mode 1), + im2*xprev (mode 2)."""
    if shift is None:
        return s
    t = np.float64(shift) * x
    y = s - t
    if xprev is not None:
        u = np.float64(im2) * xprev
        y = y + u
    return y


def lanczos_epilogue(s, xprev=None, b2=0.0):
    """lz_sub: y = s - sqrt(b2) * xprev; without xprev the subtrahend is +0.0."""
    if xprev is None:
        return s - 0.0
    t = np.sqrt(np.float64(b2)) * xprev
    return s - t
