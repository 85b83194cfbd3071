"""NumPy references of imaginary-time propagation (test_imagtime_host.py,
test_gpu_imagtime.py):  psi <- sqrt(N) exp(-tau H[psi]) psi / ||.||,
H[psi] = H0 + diag(sum_k f_k W_k) + g diag|psi|^2, N = ||psi_0||^2.

  * dense_imag: the scheme with every exponential by a dense eigh, applied as
    exp(-tau (w - w_0)) (w_0 the lowest eigenvalue: no overflow, and only the
    direction is used), then renormalised to N.  "frozen" takes the density of
    psi_n; "midpoint" predicts psi* with a frozen step (renormalised the same
    way) and steps from psi_n under g (|psi_n|^2 + |psi*|^2)/2.
  * oracle_imag: the same scheme with the CPU oracle's CA-Lanczos ('local'),
    stacked on blkdiag(H_j, H_j) from [Re; Im] or on H_j itself from a real
    state, the coefficients c = expm(-tau (T - T11 I)) e_1 by SciPy, the new
    state sqrt(N) Q c / ||c||_2 -- what the device build does.
  * combine_real_ref: the real combine kernel's chain (k_prop_combine, REAL).
  * energetics: mu, E_GP and the eigen-residual of a state from the true
    Rayleigh quotient, with the rounding bar of mu.
"""
import os
import sys

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prop_obs_ref as pref  # noqa: E402

EPS = pref.EPS
oscillator = pref.oscillator


def combine_real_ref(Q, a):
    """out = Q a in the kernel's order: one chain per row from +0.0, j ascending, no contraction."""
    out = np.zeros(Q.shape[0])
    for j in range(Q.shape[1]):
        out = out + Q[:, j] * a[j]
    return out


def imag_coefficients(c, N):
    """a = sqrt(N)/||c||_2 * c as the library forms it: the sum of squares in
    ascending order, two square roots, one division, one product per entry."""
    cc = 0.0
    for x in c:
        cc = cc + x * x
    sc = np.sqrt(N) / np.sqrt(cc)
    return sc * np.asarray(c, dtype=float)


def _lin(W, r, n):
    Wc = np.asarray(W, dtype=float).reshape(len(W), n) if len(W) else np.zeros((0, n))
    return np.asarray(r, dtype=float) @ Wc if Wc.shape[0] else np.zeros(n)


def imag_steps(expo, n, W, psi0, rows, g, density, history=False):
    """The scheme with expo(extra, psi) = a vector along exp(-tau (H0 +
    diag(extra))) psi; every result is renormalised to N = ||psi0||^2.
    Returns the last state, or with history the list of states (psi_0 first)."""
    if density not in ("frozen", "midpoint"):
        raise ValueError(density)
    psi = np.asarray(psi0)
    n0 = np.linalg.norm(psi)

    def renorm(v):
        return v * (n0 / np.linalg.norm(v))
    states = [psi]
    for r in np.asarray(rows, dtype=float).reshape(len(rows), -1):
        lin = _lin(W, r, n)
        rho = np.abs(psi) ** 2
        extra = lin + g * rho
        if density == "midpoint":
            star = renorm(expo(extra, psi))
            extra = lin + 0.5 * g * (rho + np.abs(star) ** 2)
        psi = renorm(expo(extra, psi))
        states.append(psi)
    return states if history else psi


def dense_imag(H, W, psi0, rows, tau, g, density, history=False):
    Hd = H.toarray() if sp.issparse(H) else np.asarray(H)

    def expo(extra, psi):
        ew, U = np.linalg.eigh(Hd + np.diag(extra))
        return U @ (np.exp(-tau * (ew - ew[0])) * (U.conj().T @ psi))
    return imag_steps(expo, Hd.shape[0], W, psi0, rows, g, density, history)


def oracle_imag(H, W, psi0, rows, tau, g, density, s, blocks, basis, stacked, history=False):
    """The oracle route; stacked: real CA-Lanczos on blkdiag(H_j, H_j) from
    [Re psi; Im psi], else on H_j from the real psi."""
    from oracle import ca_lanczos_ref as ref
    H = sp.csr_matrix(H)
    N = H.shape[0]

    def expo(extra, psi):
        Hj = (H + sp.diags(extra)).tocsr()
        if stacked:
            A = sp.block_diag([Hj, Hj], format="csr")
            x = np.concatenate([psi.real, psi.imag]).astype(float)
        else:
            A, x = Hj, np.asarray(psi.real, dtype=float)
        res = ref.ca_lanczos(A, x, s, s * blocks, basis, "local", diagnostics=False)
        T = res.T
        c = sl.expm(-tau * (T - T[0, 0] * np.eye(T.shape[0])))[:, 0]
        Q = res.Q[:, :T.shape[0]]
        return (Q[:N] + 1j * Q[N:]) @ c if stacked else Q @ c
    return imag_steps(expo, N, W, psi0, rows, g, density, history)


def oracle_first_column(H, psi, g, s, blocks, basis, stacked, extra=None):
    """(T(1,1), ||T(2:,1)||_2) of the oracle's CA-Lanczos on H[psi] started
    from psi: what the library's energetics rows read off the device build."""
    from oracle import ca_lanczos_ref as ref
    psi = np.asarray(psi)
    d = g * np.abs(psi) ** 2 + (0.0 if extra is None else np.asarray(extra, dtype=float))
    Hj = (sp.csr_matrix(H) + sp.diags(d)).tocsr()
    if stacked:
        A = sp.block_diag([Hj, Hj], format="csr")
        x = np.concatenate([psi.real, psi.imag]).astype(float)
    else:
        A, x = Hj, np.asarray(psi.real, dtype=float)
    T = ref.ca_lanczos(A, x, s, s * blocks, basis, "local", diagnostics=False).T
    return T[0, 0], float(np.linalg.norm(T[1:, 0]))


def energetics(H, psi, g=0.0, extra=None):
    """(mu, E_GP, res, bar_mu) of the state psi under H[psi] = H + diag(extra)
    + g diag|psi|^2:  mu = <psi|H[psi]|psi>/N, E_GP = N mu - (g/2) sum|psi|^4,
    res = ||H[psi] psi - mu psi|| / sqrt(N).  bar_mu = 1.4 eps ||H[psi]||_inf,
    the size of the rounding in the Lanczos recurrence's first coefficient."""
    H = sp.csr_matrix(H)
    psi = np.asarray(psi)
    rho = np.abs(psi) ** 2
    d = g * rho + (0.0 if extra is None else np.asarray(extra, dtype=float))
    Hp = H @ psi + d * psi
    N = float(np.sum(rho))
    mu = float(np.real(np.vdot(psi, Hp))) / N
    E = N * mu - 0.5 * g * float(np.sum(rho * rho))
    res = float(np.linalg.norm(Hp - mu * psi)) / np.sqrt(N)
    hinf = float(np.max(abs(H).sum(axis=1).A1 + np.abs(d)))
    return mu, E, res, 1.4 * EPS * hinf
