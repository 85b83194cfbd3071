"""NumPy references of the nonlinear term g |psi|^2 (test_nonlinear_host.py,
test_gpu_nonlinear.py): i d/dt psi = (H0 + sum_k f_k(t) diag(W_k) + g |psi|^2) psi.

  * density_chain: the density kernel's order contract (include/calanczos.h),
      ra = ua*ua;  ra = ra + va*va;  [rb likewise from B]
      d = V0;  for k ascending:  p = f_k * W_k;  d = d + p
      p = ga*ra;  d = d + p;  [p = gb*rb;  d = d + p]
    with every product and sum rounded separately, elementwise.
  * the two schemes, one step of size sub under the amplitudes r:
      "frozen":    psi' = exp(-i sub (H_r + g diag|psi|^2)) psi
      "midpoint":  psi* = the frozen step;  psi' = exp(-i sub (H_r + g diag(|psi|^2 + |psi*|^2)/2)) psi
    (H_r = H0 + diag(sum_k r_k W_k); an absorbing mask multiplies psi' only).
    dense_nonlinear takes every exponential by a dense eigh, so that against a
    run with the same rows only the Krylov error is judged;
    lanczos_nonlinear takes them by stacked real Lanczos (m = 24, full
    reorthogonalisation, tests/prop_obs_ref.py); oracle_nonlinear by the CPU
    oracle's ca_lanczos ('local') then expm, as tests/drive_ref.py
    oracle_driven does.
"""
import os
import sys

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prop_obs_ref as pref  # noqa: E402

oscillator = pref.oscillator


def density_chain(V0, W, f, ga, A, gb=None, B=None):
    """The diagonal a nonlinear step writes: W a list of columns, f their
    amplitudes, A (and B) complex states."""
    A = np.asarray(A, dtype=complex)
    ua, va = A.real.astype(np.float64), A.imag.astype(np.float64)
    ra = ua * ua
    ra = ra + va * va
    if B is not None:
        B = np.asarray(B, dtype=complex)
        ub, vb = B.real.astype(np.float64), B.imag.astype(np.float64)
        rb = ub * ub
        rb = rb + vb * vb
    d = np.array(V0, dtype=np.float64, copy=True)
    for k in range(len(W)):
        p = np.float64(f[k]) * np.asarray(W[k], dtype=np.float64)
        d = d + p
    p = np.float64(ga) * ra
    d = d + p
    if B is not None:
        p = np.float64(gb) * rb
        d = d + p
    return d


def _rows(rows):
    r = np.asarray(rows, dtype=float)
    return r.reshape(len(r), -1)


def _wcols(W, n):
    return np.asarray(W, dtype=float).reshape(len(W), n) if len(W) else np.zeros((0, n))


def nonlinear_steps(expo, n, W, psi0, rows, sub, g, density, mask=None, history=False):
    """The scheme with expo(extra, psi) = exp(-i sub (H0 + diag(extra))) psi.
    Returns psi, or with history (states after each step, the diagonal
    additions `extra` of each step's last exponential)."""
    if density not in ("frozen", "midpoint"):
        raise ValueError(density)
    Wc = _wcols(W, n)
    psi = np.asarray(psi0, dtype=complex)
    states, extras = [], []
    for r in _rows(rows):
        lin = r @ Wc if Wc.shape[0] else np.zeros(n)
        rho = np.abs(psi) ** 2
        extra = lin + g * rho
        if density == "midpoint":
            star = expo(extra, psi)
            extra = lin + 0.5 * g * (rho + np.abs(star) ** 2)
        psi = expo(extra, psi)
        if mask is not None:
            psi = np.asarray(mask, dtype=float) * psi
        states.append(psi)
        extras.append(extra)
    return (states, extras) if history else psi


def dense_nonlinear(H, W, psi0, rows, sub, g, density, mask=None, history=False):
    """Every exponential by a dense eigh ("midpoint": both passes)."""
    Hd = H.toarray() if sp.issparse(H) else np.asarray(H, dtype=float)

    def expo(extra, psi):
        ew, U = np.linalg.eigh(Hd + np.diag(extra))
        return U @ (np.exp(-1j * sub * ew) * (U.T @ psi))
    return nonlinear_steps(expo, Hd.shape[0], W, psi0, rows, sub, g, density, mask, history)


def lanczos_nonlinear(H, W, psi0, rows, sub, g, density, m=24):
    """Every exponential by stacked real Lanczos (m vectors, full reorthogonalisation)."""
    H = sp.csr_matrix(H)
    N = H.shape[0]

    def expo(extra, psi):
        Hj = H + sp.diags(extra)
        H2 = sp.block_diag([Hj, Hj], format="csr")
        x = np.concatenate([psi.real, psi.imag]).astype(float)
        T, Q = pref.lanczos_full(H2, x, m)
        c = sl.expm(-1j * sub * T)[:, 0] * np.linalg.norm(x)
        return (Q[:N] + 1j * Q[N:]) @ c
    return nonlinear_steps(expo, N, W, psi0, rows, sub, g, density)


def oracle_nonlinear(H, W, psi0, rows, sub, g, density, s, blocks, basis):
    """Every exponential by the CPU oracle's CA-Lanczos on blkdiag(H_j, H_j);
    returns (psi, the largest | ||psi_j|| - ||psi0|| | over the steps)."""
    from oracle import ca_lanczos_ref as ref
    H = sp.csr_matrix(H)
    N = H.shape[0]

    def expo(extra, psi):
        Hj = (H + sp.diags(extra)).tocsr()
        A2 = sp.block_diag([Hj, Hj], format="csr")
        x = np.concatenate([psi.real, psi.imag]).astype(float)
        res = ref.ca_lanczos(A2, x, s, s * blocks, basis, "local", diagnostics=False)
        c = sl.expm(-1j * sub * res.T)[:, 0] * np.linalg.norm(x)
        return (res.Q[:N] + 1j * res.Q[N:]) @ c
    states, _ = nonlinear_steps(expo, N, W, psi0, rows, sub, g, density, history=True)
    n0 = np.linalg.norm(psi0)
    drift = max(abs(np.linalg.norm(p) - n0) for p in states)
    return states[-1], drift


def quartic(psi):
    """(sum_i |psi_i|^4, its rounding bar (N + 8) eps S of tests/prop_obs_ref.py)."""
    psi = np.asarray(psi, dtype=complex)
    d = psi.real ** 2 + psi.imag ** 2
    S = float(np.sum(d * d))
    return S, (len(psi) + 8) * pref.EPS * S
