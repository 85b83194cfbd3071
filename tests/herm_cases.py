"""Random complex Hermitian CSR matrices of the Hermitian SpMV tests
(test_hermitian_host.py, test_gpu_hermitian.py): the patterns of
tests/test_gpu_shared.py's generators, every upper entry with a complex value
of its own (distinct moduli, all four sign combinations), the mirror its
conjugate, the stored diagonal real."""
import numpy as np
import scipy.sparse as sp


def canon(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    return A


def herm_from_upper(n, i, j, seed):
    rng = np.random.RandomState(seed)
    key = np.unique(np.asarray(i, dtype=np.int64) * n + np.asarray(j, dtype=np.int64))
    i, j = key // n, key % n
    m = len(key)
    re = (1.0 + (rng.permutation(m) + 1.0) / (m + 1.0)) * rng.choice([-1.0, 1.0], m)
    im = (0.5 + (rng.permutation(m) + 1.0) / (m + 1.0)) * rng.choice([-1.0, 1.0], m)
    off = i != j
    v = re + 1j * np.where(off, im, 0.0)
    rows = np.concatenate([i, j[off]])
    cols = np.concatenate([j, i[off]])
    vals = np.concatenate([v, np.conj(v[off])])
    H = canon(sp.coo_matrix((vals, (rows, cols)), shape=(n, n)))
    assert np.iscomplexobj(H.data)
    return H


def rand_herm(n, seed=0, full_diag=False):
    """Rows of 0..12 entries, empty rows, rows without a stored diagonal."""
    rng = np.random.RandomState(1000 + n + seed)
    i, j = [], []
    for _ in range(6):  # six permutations: at most 12 off-diagonals per row
        p = rng.permutation(n)
        keep = rng.rand(n) < 0.6
        a, b = np.arange(n)[keep], p[keep]
        i.append(np.minimum(a, b))
        j.append(np.maximum(a, b))
    i, j = np.concatenate(i), np.concatenate(j)
    ok = i != j
    i, j = i[ok], j[ok]
    empty = rng.rand(n) < 0.05 if n > 3 else np.zeros(n, dtype=bool)
    if full_diag:
        empty[:] = False
    ok = ~(empty[i] | empty[j])
    i, j = i[ok], j[ok]
    deg = np.bincount(np.concatenate([i, j]), minlength=n)
    diag = (deg < 12) & ~empty & ((rng.rand(n) < 0.67) | full_diag)
    if n <= 3:
        diag[0] = True
    d = np.nonzero(diag)[0]
    H = herm_from_upper(n, np.concatenate([i, d]), np.concatenate([j, d]), seed + n)
    lens = np.diff(H.indptr)
    assert lens.max() <= 12
    if n >= 255 and not full_diag:
        stored_diag = np.zeros(n, dtype=bool)
        rows = np.repeat(np.arange(n), lens)
        stored_diag[rows[H.indices == rows]] = True
        assert lens.min() == 0 and np.any(~stored_diag & (lens > 0))
    return H


def band_herm(n=600, half=150):
    """About 300 nonzeros per row: the 2048-nonzero limit cuts the row blocks at 6 rows."""
    i = np.repeat(np.arange(n), half + 1)
    j = i + np.tile(np.arange(half + 1), n)
    ok = j < n
    H = herm_from_upper(n, i[ok], j[ok], 77)
    assert np.diff(H.indptr).max() == 2 * half + 1 and 7 * (2 * half + 1) > 2048 >= 6 * (2 * half + 1)
    return H


def long_row_herm(n=4100, k=1000):
    """Row k and its mirror column hold n - 1 off-diagonals, every diagonal is
    stored: row k has n = 2 * 2048 + 4 nonzeros, two full chunks and a remainder."""
    o = np.delete(np.arange(n), k)
    i = np.concatenate([np.minimum(o, k), np.arange(n)])
    j = np.concatenate([np.maximum(o, k), np.arange(n)])
    H = herm_from_upper(n, i, j, 31 + k)
    assert H.indptr[k + 1] - H.indptr[k] == n and 2 * 2048 < n < 3 * 2048
    return H


def signed_zero_vec(n2, seed):
    """A stacked vector with +0.0 and -0.0 entries among the random ones."""
    rng = np.random.RandomState(seed)
    x = rng.randn(n2)
    if n2 >= 8:
        x[rng.rand(n2) < 0.1] = 0.0
        x[rng.rand(n2) < 0.1] = -0.0
    else:
        x[0] = -0.0
    return x
