"""Complex Hermitian H on the CPU: matrices.hermitian_embedding,
matrices.peierls_hamiltonian, the NumPy order contract of the Hermitian
stored-once SpMV (tests/herm_ref.py herm_chain) and the C ABI of
cal_set_matrix_csr_hermitian / cal_spmv_hermitian_info.  No GPU.

Bars: the project's summation bar per row, (N + 8) eps S with N = 2k products
and S = sum_j (|a_j| + |b_j|)(|x0_j| + |x1_j|) (herm_ref.row_bar), between any
two orders of a row's sum and against the complex128 product; bits where the
contract says bits.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import herm_ref  # noqa: E402
from herm_cases import band_herm, rand_herm, signed_zero_vec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 63, 257)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- hermitian_embedding -------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_embedding_is_symmetric_and_in_the_documented_row_order(cal, n):
    H = rand_herm(n)
    E = cal.matrices.hermitian_embedding(H)
    assert E.shape == (2 * n, 2 * n) and E.nnz == 4 * H.nnz and E.dtype == np.float64
    assert (E - E.T).nnz == 0 or np.max(np.abs((E - E.T).data)) == 0.0
    a, b = H.data.real, H.data.imag
    for i in range(n):
        p0, p1 = H.indptr[i], H.indptr[i + 1]
        c = H.indices[p0:p1]
        t0, t1 = E.indptr[i], E.indptr[i + 1]
        assert np.array_equal(E.indices[t0:t1], np.concatenate([c, c + n]))
        assert np.array_equal(bits(E.data[t0:t1]), bits(np.concatenate([a[p0:p1], -b[p0:p1]])))
        b0, b1 = E.indptr[n + i], E.indptr[n + i + 1]
        assert np.array_equal(E.indices[b0:b1], np.concatenate([c, c + n]))
        assert np.array_equal(bits(E.data[b0:b1]), bits(np.concatenate([b[p0:p1], a[p0:p1]])))


def test_embedding_keeps_explicit_zeros(cal):
    H = rand_herm(63)
    Z = sp.csr_matrix((H.data.real + 0j, H.indices, H.indptr), shape=H.shape)
    E, EZ = cal.matrices.hermitian_embedding(H), cal.matrices.hermitian_embedding(Z)
    assert np.array_equal(E.indptr, EZ.indptr) and np.array_equal(E.indices, EZ.indices)
    R = cal.matrices.hermitian_embedding(sp.csr_matrix(H.real))  # a real dtype: B = 0
    assert np.array_equal(R.indices, E.indices) and np.array_equal(R.data, EZ.data)


@pytest.mark.parametrize("n", SIZES)
def test_embedding_product_is_the_complex_product(cal, n):
    H = rand_herm(n)
    E = cal.matrices.hermitian_embedding(H)
    x = signed_zero_vec(2 * n, 3)
    y = herm_ref.rowsum_chain(E, x)
    exact = herm_ref.exact_product(H, x)
    bar = herm_ref.row_bar(H, x)
    assert np.all(np.abs(y - exact) <= bar)
    assert np.all(np.abs(E @ x - exact) <= bar)


def test_embedding_eigenvalues_are_those_of_h_twice(cal):
    H = rand_herm(40, full_diag=True)
    w = np.linalg.eigvalsh(H.toarray())
    we = np.linalg.eigvalsh(cal.matrices.hermitian_embedding(H).toarray())
    normH = np.max(np.abs(w))
    assert np.max(np.abs(we - np.repeat(w, 2))) <= 80 * 8 * np.finfo(float).eps * normH  # 2n x a few ulp of |H|


# ---- peierls_hamiltonian ---------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(8, 8), (7, 5), (5, 4, 3)])
def test_peierls_is_hermitian_to_the_bit_with_a_real_diagonal(cal, dims):
    n = int(np.prod(dims))
    V = np.random.RandomState(1).randn(n)
    H = cal.matrices.peierls_hamiltonian(dims, V, 1.0 / 7.0, h=0.5, mass=2.0)
    assert np.iscomplexobj(H.data) and H.has_sorted_indices
    Hc = H.conj().T.tocsr()
    Hc.sort_indices()
    assert np.array_equal(Hc.indptr, H.indptr) and np.array_equal(Hc.indices, H.indices)
    assert np.array_equal(bits(Hc.data.real), bits(H.data.real))
    assert np.array_equal(bits(Hc.data.imag + 0.0), bits(H.data.imag + 0.0))
    rows = np.repeat(np.arange(n), np.diff(H.indptr))
    assert np.all(H.data.imag[H.indices == rows] == 0.0) and np.count_nonzero(H.indices == rows) == n
    assert np.any(H.data.imag != 0.0)
    G = cal.matrices.grid_hamiltonian(dims, V, h=0.5, mass=2.0)
    assert np.array_equal(G.indptr, H.indptr) and np.array_equal(G.indices, H.indices)


@pytest.mark.parametrize("dims", [(8, 8), (5, 4, 3)])
def test_peierls_without_flux_is_the_grid_hamiltonian(cal, dims):
    n = int(np.prod(dims))
    V = np.random.RandomState(2).randn(n)
    H = cal.matrices.peierls_hamiltonian(dims, V, 0.0, h=0.7)
    G = cal.matrices.grid_hamiltonian(dims, V, h=0.7)
    assert np.array_equal(G.indptr, H.indptr) and np.array_equal(G.indices, H.indices)
    assert np.array_equal(bits(H.data.real), bits(G.data))
    assert H.nnz == G.nnz and np.array_equal(bits(H.data.imag), bits(np.zeros(H.nnz)))


def test_peierls_against_a_dense_construction(cal):
    """8 x 8, first axis fastest: site (x0, x1) is row x0 + 8 x1.  Hops along
    axis 0 are -t; the hop from (x0, x1 + 1) to (x0, x1), entry H[r, r + 8],
    is -t exp(-2 pi i flux x0) and its mirror the conjugate."""
    N, flux, hh, mass = 8, 1.0 / 12.0, 0.5, 1.5
    t = 1.0 / (2.0 * mass * hh * hh)
    V = np.random.RandomState(3).randn(N * N)
    D = np.zeros((N * N, N * N), dtype=complex)
    for x1 in range(N):
        for x0 in range(N):
            r = x0 + N * x1
            D[r, r] = 4.0 * t + V[r]
            if x0 + 1 < N:
                D[r, r + 1] = D[r + 1, r] = -t
            if x1 + 1 < N:
                ph = np.exp(-2j * np.pi * flux * x0)
                D[r, r + N] = -t * ph
                D[r + N, r] = -t * np.conj(ph)
    H = cal.matrices.peierls_hamiltonian((N, N), V, flux, h=hh, mass=mass)
    assert np.max(np.abs(H.toarray() - D)) <= 4 * np.finfo(float).eps * (4.0 * t + np.max(np.abs(V)))
    assert np.array_equal(H.toarray() != 0, D != 0)


# ---- herm_chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_chain_with_zero_imaginary_parts_has_the_shared_chains_bits(n):
    H = rand_herm(n)
    A = sp.csr_matrix((np.ascontiguousarray(H.data.real), H.indices, H.indptr), shape=H.shape)
    for seed in (4, 5):
        x = signed_zero_vec(2 * n, seed)
        y = herm_ref.herm_chain(H, x, val_im=np.zeros(H.nnz))
        assert np.array_equal(bits(y), bits(herm_ref.shared_chain(A, x)))
        ym = herm_ref.herm_chain(H, x, val_im=-np.zeros(H.nnz))  # b = -0.0 as well
        assert np.array_equal(bits(ym), bits(y))


@pytest.mark.parametrize("n", SIZES)
def test_chain_within_the_bar_of_the_embedding_chain_and_the_exact_product(cal, n):
    H = rand_herm(n)
    E = cal.matrices.hermitian_embedding(H)
    worst = 0.0
    for seed in (6, 7):
        x = signed_zero_vec(2 * n, seed)
        y = herm_ref.herm_chain(H, x)
        bar = herm_ref.row_bar(H, x)
        ye = herm_ref.rowsum_chain(E, x)
        ex = herm_ref.exact_product(H, x)
        assert np.all(np.abs(y - ye) <= bar) and np.all(np.abs(y - ex) <= bar)
        nz = bar > 0
        if nz.any():
            worst = max(worst, float(np.max(np.abs(y - ye)[nz] / bar[nz])), float(np.max(np.abs(y - ex)[nz] / bar[nz])))
        assert np.all(y[~nz] == 0.0) and not np.any(np.signbit(y[~nz]))
    print("n=%d: largest |difference| / bar %.3f" % (n, worst))


def test_chain_on_a_band_matrix_within_the_bar(cal):
    H = band_herm()
    x = signed_zero_vec(2 * H.shape[0], 8)
    y, bar = herm_ref.herm_chain(H, x), herm_ref.row_bar(H, x)
    assert np.all(np.abs(y - herm_ref.rowsum_chain(cal.matrices.hermitian_embedding(H), x)) <= bar)
    assert np.all(np.abs(y - herm_ref.exact_product(H, x)) <= bar)


# ---- the ABI ----------------------------------------------------------------------------------------
NAMES = ("cal_set_matrix_csr_hermitian", "cal_spmv_hermitian_info")


def test_library_exports_the_symbols(cal):
    lib = ctypes.CDLL(cal.LIB_PATH)
    from ca_lanczos_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name)
        assert name in {s[0] for s in _lib.SIGNATURES}
    assert hasattr(cal.Context, "set_matrix_hermitian") and hasattr(cal.Context, "spmv_hermitian_info")
    assert hasattr(cal.matrices, "hermitian_embedding") and hasattr(cal.matrices, "peierls_hamiltonian")


def test_header_declares_them_and_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "calanczos.h")).read()
    assert re.search(r"int\s+cal_set_matrix_csr_hermitian\(cal_ctx\*\s*ctx,\s*int64_t\s+n,\s*const\s+int64_t\*\s*rowptr,"
                     r"\s*const\s+int32_t\*\s*colind,\s*const\s+double\*\s*val_re,\s*const\s+double\*\s*val_im\);", hdr)
    assert re.search(r"int\s+cal_spmv_hermitian_info\(cal_ctx\*\s*ctx,\s*int\*\s*on,\s*int64_t\*\s*n,\s*"
                     r"int64_t\*\s*nnz_stored\);", hdr)
    assert "caller's contract" in hdr and "[[A, -B], [B, A]]" in hdr


def test_mex_shims_still_compile_against_the_header():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "mex"), "check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
