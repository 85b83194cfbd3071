"""The host analysis of the diagonal-split SpMV format (cal_split_analyze,
DESIGN.md §3): a uniform 5- / 7-point stencil plus a per-row diagonal, H = K +
diag(V).  It is the analysis the upload runs; no GPU is needed."""
import ctypes
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_cases import drop_diagonal, hamiltonian_2d, lap3d_v, potential  # noqa: E402


def test_library_exports_the_split_symbols(cal):
    lib = ctypes.CDLL(cal.LIB_PATH)
    for s in ("cal_split_analyze", "cal_spmv_split_info", "cal_set_spmv_format"):
        assert hasattr(lib, s), s
    from ca_lanczos_amd import _lib
    bound = {s[0] for s in _lib.SIGNATURES}
    assert {"cal_split_analyze", "cal_spmv_split_info"} <= bound


def test_accepts_laplacian_plus_potential(cal):
    A = lap3d_v(cal, 17)
    assert len(np.unique(A.diagonal())) == A.shape[0]
    assert cal.split_analyze(A) == (289, 18, True)


def test_accepts_grid_hamiltonian_with_other_off_diagonals(cal):
    A = hamiltonian_2d(cal, 300)
    assert A.indices.dtype == np.int32 and A.has_sorted_indices
    off = A.data[A.indices != np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))]
    assert np.all(off == -8.0)
    assert cal.split_analyze(A) == (300, 2, False)


def test_grid_hamiltonian_is_scaled_laplacian_plus_potential(cal):
    for dims, L in (((19, 23), None), ((7, 9, 11), None), ((12, 12, 12), cal.matrices.laplacian_3d(12))):
        V = potential(dims)
        A = cal.matrices.grid_hamiltonian(dims, V, h=0.5, mass=2.0)
        n = int(np.prod(dims))
        assert A.shape == (n, n) and A.indices.dtype == np.int32 and A.has_sorted_indices
        t = 1.0 / (2.0 * 2.0 * 0.25)
        assert np.array_equal(A.diagonal(), t * 2 * len(dims) + V)
        assert abs(A - A.T).nnz == 0
        if L is not None:
            assert abs(A - (t * L + sp.diags(V))).max() == 0.0
    A1 = cal.matrices.grid_hamiltonian((16, 16, 16), np.zeros(16 ** 3), h=1.0, mass=0.5)
    assert abs(A1 - cal.matrices.laplacian_3d(16)).nnz == 0


def test_accepts_the_stacked_matrix(cal):
    A = lap3d_v(cal, 17)
    S = sp.block_diag((A, A), format="csr")
    assert cal.split_analyze(S) == (289, 18, True)


def test_accepts_structurally_absent_diagonal_entries(cal):
    A = lap3d_v(cal, 17)
    n = A.shape[0]
    B = drop_diagonal(A, [0, 5, 288, 289, n // 2, n - 1])
    assert cal.split_analyze(B) == (289, 18, True)


def test_rejects_small_plane_stride(cal):
    assert cal.split_analyze(cal.matrices.laplacian_2d(37)) is None  # P = 37 < 256


def test_rejects_irregular_matrix(cal):
    assert cal.split_analyze(cal.matrices.circuit_like(60)) is None


def test_rejects_one_perturbed_off_diagonal(cal):
    A = lap3d_v(cal, 17).copy()
    r = A.shape[0] // 2
    p = A.indptr[r]  # the row's first entry: offset -P
    assert A.indices[p] == r - 289
    A.data[p] = -1.0 - 2.0 ** -30
    assert cal.split_analyze(A) is None


def test_rejects_nine_diagonal_band(cal):
    n = 3000
    offs = [-300, -3, -2, -1, 0, 1, 2, 3, 300]
    A = sp.diags([np.full(n - abs(o), -1.0) if o else 9.0 + np.arange(n) * 2.0 ** -12 for o in offs], offs,
                 format="csr")
    assert cal.split_analyze(A) is None


def test_rejects_rows_longer_than_eight(cal):
    A = lap3d_v(cal, 17).tolil()
    r = A.shape[0] // 2
    A[r, r + 2] = -1.0
    A[r, r - 2] = -1.0  # 9 entries in row r
    A = A.tocsr()
    assert np.diff(A.indptr).max() == 9
    assert cal.split_analyze(A) is None
