"""NumPy references of the time-dependent potential H(t) = H0 + sum_k f_k(t)
diag(W_k) (test_drive_host.py, test_gpu_drive.py).

  * chain: the drive kernel's order contract (include/calanczos.h),
      d = V0;  for k ascending:  p = f_k * W_k;  d = d + p
    with product and sum rounded separately, elementwise.
  * dense_driven: the product of dense eigh exponentials exp(-i sub H_j) of the
    Hamiltonians H_j = H0 + diag(sum_k rows[j, k] W_k) -- the reference of a
    run with the same amplitude rows, so only the Krylov error is judged.
  * propagate_driven_numpy: the same steps by real Lanczos on blkdiag(H_j, H_j)
    (m = 24 with full reorthogonalisation, tests/prop_obs_ref.py).
  * oracle_driven: the same steps by the CPU oracle's ca_lanczos ('local') on
    blkdiag(H_j, H_j), then expm -- the yardstick the device is held next to.
The problems are those of tests/test_gpu_prop.py: the oscillator comes from
tests/prop_obs_ref.py, packet_2d is restated here.
"""
import functools
import os
import sys

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prop_obs_ref as pref  # noqa: E402

oscillator = pref.oscillator  # (H csr, psi0, x, ew, U)


@functools.lru_cache(maxsize=None)
def packet_2d():
    """laplacian_2d(40), a Gaussian packet times exp(i(0.7x + 0.3y)) and the
    grid coordinates x, y (tests/test_gpu_prop.py's packet_2d)."""
    from ca_lanczos_amd import matrices
    N = 40
    H = matrices.laplacian_2d(N)
    y, x = np.divmod(np.arange(N * N), N)
    psi = np.exp(-((x - 19.5) ** 2 + (y - 19.5) ** 2) / (2 * 4.0 ** 2)) * np.exp(1j * (0.7 * x + 0.3 * y))
    return H, psi, x.astype(float), y.astype(float)


def chain(V0, W, f):
    """The diagonal a driven step writes: W is a list of columns, f their amplitudes."""
    d = np.array(V0, dtype=np.float64, copy=True)
    for k in range(len(W)):
        p = np.float64(f[k]) * np.asarray(W[k], dtype=np.float64)
        d = d + p
    return d


def _wcols(W, n):
    return np.asarray(W, dtype=float).reshape(len(W), n)


def dense_driven(H, W, psi0, rows, sub):
    """psi after len(rows) steps of size sub, each the dense exponential of its own H_j."""
    Hd = H.toarray() if sp.issparse(H) else np.asarray(H)
    Wc = _wcols(W, Hd.shape[0])
    psi = np.asarray(psi0, dtype=complex)
    for r in np.asarray(rows, dtype=float).reshape(len(rows), -1):
        ew, U = np.linalg.eigh(Hd + np.diag(r @ Wc))
        psi = U @ (np.exp(-1j * sub * ew) * (U.T @ psi))
    return psi


def propagate_driven_numpy(H, W, psi0, rows, sub, m=24):
    """The same steps by stacked real Lanczos (m vectors, full reorthogonalisation)."""
    H = sp.csr_matrix(H)
    N = H.shape[0]
    Wc = _wcols(W, N)
    psi0 = np.asarray(psi0, dtype=complex)
    x = np.concatenate([psi0.real, psi0.imag]).astype(float)
    for r in np.asarray(rows, dtype=float).reshape(len(rows), -1):
        Hj = H + sp.diags(r @ Wc)
        H2 = sp.block_diag([Hj, Hj], format="csr")
        T, Q = pref.lanczos_full(H2, x, m)
        c = sl.expm(-1j * sub * T)[:, 0] * np.linalg.norm(x)
        p = (Q[:N] + 1j * Q[N:]) @ c
        x = np.concatenate([p.real, p.imag])
    return x[:N] + 1j * x[N:]


def oracle_driven(H, W, psi0, rows, sub, s, blocks, basis):
    """The same steps by the CPU oracle's CA-Lanczos on blkdiag(H_j, H_j); returns
    (psi, the largest | ||psi_j|| - ||psi0|| | over the steps)."""
    from oracle import ca_lanczos_ref as ref
    H = sp.csr_matrix(H)
    N = H.shape[0]
    Wc = _wcols(W, N)
    psi0 = np.asarray(psi0, dtype=complex)
    n0 = np.linalg.norm(psi0)
    x = np.concatenate([psi0.real, psi0.imag]).astype(float)
    drift = 0.0
    for r in np.asarray(rows, dtype=float).reshape(len(rows), -1):
        Hj = (H + sp.diags(r @ Wc)).tocsr()
        A2 = sp.block_diag([Hj, Hj], format="csr")
        nrm = np.linalg.norm(x)
        res = ref.ca_lanczos(A2, x, s, s * blocks, basis, "local", diagnostics=False)
        c = sl.expm(-1j * sub * res.T)[:, 0] * nrm
        out = (res.Q[:N] + 1j * res.Q[N:]) @ c
        x = np.concatenate([out.real, out.imag])
        drift = max(drift, abs(np.linalg.norm(x) - n0))
    return x[:N] + 1j * x[N:], drift


def f_one(t):
    """The single-operator drive of the tests: 2 sin 3t on x."""
    return np.array([2.0 * np.sin(3.0 * t)])


def f_two(t):
    """The two-operator drive: (2 sin 3t, 0.25 cos 2t) on (x, x^2)."""
    return np.array([2.0 * np.sin(3.0 * t), 0.25 * np.cos(2.0 * t)])
