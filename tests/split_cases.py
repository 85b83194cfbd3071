"""Matrices of the diagonal-split tests (test_split_host.py, test_gpu_split.py):
grid Hamiltonians K + diag(V) with a potential that differs in every row."""
import numpy as np
import scipy.sparse as sp


def potential(dims):
    """0.5 |x - x0|^2 about the grid centre plus index * 2^-27: every value
    is an exact binary fraction and no two are equal (0.5 |x - x0|^2 is a
    multiple of 1/8, the index term stays below 1/16 for n < 2^23)."""
    dims = tuple(int(d) for d in dims)
    n = int(np.prod(dims))
    assert n < 2 ** 23
    idx = np.arange(n, dtype=np.int64)
    r2 = np.zeros(n)
    stride = 1
    for d in dims:  # the first dimension is the fastest, as in matrices._stencil_csr
        x = (idx // stride) % d - (d - 1) / 2.0
        r2 += x * x
        stride *= d
    V = 0.5 * r2 + idx * 2.0 ** -27
    assert len(np.unique(V)) == n
    return V


def with_potential(L, dims):
    """Laplacian L (diagonal 2d, off-diagonals -1) + diag(V): canonical CSR, int32 columns."""
    A = (L + sp.diags(potential(dims))).tocsr()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    return A


def lap3d_v(cal, N):
    return with_potential(cal.matrices.laplacian_3d(N), (N, N, N))


def hamiltonian_2d(cal, N):
    """5-point, off-diagonals -1/(2 h^2) = -8: not the -1 of the Laplacians."""
    return cal.matrices.grid_hamiltonian((N, N), potential((N, N)), h=0.25)


def drop_diagonal(A, rows):
    """A with the diagonal entries of `rows` structurally absent."""
    C = A.tocoo()
    keep = ~((C.row == C.col) & np.isin(C.row, np.asarray(rows)))
    B = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=A.shape)
    B.sort_indices()
    B.indices = B.indices.astype(np.int32)
    assert B.nnz == A.nnz - len(rows)
    return B
