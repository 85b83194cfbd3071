"""NumPy references and rounding bars for the propagator's device-side
observables (test_prop_observables_host.py, test_gpu_prop_observables.py).

Definitions (include/calanczos.h), psi = t + i b, phi = pr + i pi:
  <W>       = sum_i W[i] (t[i]^2 + b[i]^2)
  <phi|psi> = sum_i conj(phi[i]) psi[i] = sum (pr t + pi b) + i sum (pr b - pi t)
  E         = x' blkdiag(H, H) x over the stacked x = [t; b]

Rounding bar, derived and not measured: a quantity that is a sum of N
products whose absolute values sum to S stays within (N + 8) eps S of the
exact sum in any summation order (N - 1 additions, each at most eps of the
running sum <= S, to first order; the 8 covers the few roundings inside a
term -- t*t + b*b and its product with W are three -- and the second order).
  <W_k>: N = n;  each overlap component: N = 2n;
  energy: N = nnz(blkdiag(H, H)) + 2n, S = |x|' |A| |x|.
"""
import functools

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

EPS = np.finfo(float).eps


# ---- the combine sweep's chain -----------------------------------------------------
def combine_ref(Q, c):
    """(Re, Im) of Q_c c on stacked halves in the kernel's order: one chain
    per output row, j ascending, no contraction (k_prop_combine)."""
    n = Q.shape[0] // 2
    a, b = c.real, c.imag
    top, bot = np.zeros(n), np.zeros(n)
    for j in range(Q.shape[1]):
        qt, qb = Q[:n, j], Q[n:, j]
        top = top + qt * a[j]
        top = top - qb * b[j]
        bot = bot + qt * b[j]
        bot = bot + qb * a[j]
    return top, bot


# ---- the reference values and their bars -----------------------------------------
def w_ref(W, psi):
    """(<W_k> for every column of W (n x nw), the rounding bars)."""
    W = np.asarray(W, dtype=float).reshape(len(psi), -1)
    d = psi.real ** 2 + psi.imag ** 2
    n = len(psi)
    return W.T @ d, (n + 8) * EPS * (np.abs(W).T @ d)


def overlap_ref(phi, psi):
    """(<phi_r|psi> for every column of phi (n x nphi), the bars of Re, of Im)."""
    phi = np.asarray(phi, dtype=complex).reshape(len(psi), -1)
    n = len(psi)
    pr, pi, t, b = np.abs(phi.real), np.abs(phi.imag), np.abs(psi.real), np.abs(psi.imag)
    bar_re = (2 * n + 8) * EPS * (pr.T @ t + pi.T @ b)
    bar_im = (2 * n + 8) * EPS * (pr.T @ b + pi.T @ t)
    return phi.conj().T @ psi, bar_re, bar_im


def energy_ref(H, psi):
    """(<psi|H|psi> as the stacked real form computes it, its bar)."""
    H = sp.csr_matrix(H)
    n = H.shape[0]
    t, b = psi.real, psi.imag
    E = t @ (H @ t) + b @ (H @ b)
    A = abs(H)
    S = np.abs(t) @ (A @ np.abs(t)) + np.abs(b) @ (A @ np.abs(b))
    return E, (2 * H.nnz + 2 * n + 8) * EPS * S


def check_row(row, H, psi, W, phi, energy=True):
    """One history row [t, norm2, E, <W>.., Re, Im, ..] against the state psi
    it belongs to; returns the list of (name, |difference|, bar) and asserts."""
    W = np.asarray(W, dtype=float).reshape(len(psi), -1)
    phi = np.asarray(phi, dtype=complex).reshape(len(psi), -1)
    nw, nphi = W.shape[1], phi.shape[1]
    assert len(row) == 3 + nw + 2 * nphi
    out = []
    if energy:
        E, bar = energy_ref(H, psi)
        out.append(("energy", abs(row[2] - E), bar))
    else:
        assert np.isnan(row[2])
    wv, wbar = w_ref(W, psi)
    for k in range(nw):
        out.append(("W%d" % k, abs(row[3 + k] - wv[k]), wbar[k]))
    ov, bre, bim = overlap_ref(phi, psi)
    for r in range(nphi):
        out.append(("Re%d" % r, abs(row[3 + nw + 2 * r] - ov[r].real), bre[r]))
        out.append(("Im%d" % r, abs(row[4 + nw + 2 * r] - ov[r].imag), bim[r]))
    for name, d, bar in out:
        print("%s: |diff| %.3e bar %.3e" % (name, d, bar))
        assert d <= bar, (name, d, bar)
    return out


# ---- the oscillator of tests/test_gpu_prop.py ----------------------------------------
@functools.lru_cache(maxsize=None)
def oscillator(N):
    """H (CSR), psi0, the grid x and the dense eigh of H (runLanczos.m:5-21)."""
    lo, hi = -10.0, 10.0
    h = (hi - lo) / N
    x = lo + h / 2 + h * np.arange(N)
    i = np.arange(N)
    L = np.zeros((N, N))
    L[i, (i + 1) % N] += 4.0 / 3
    L[i, (i + 2) % N] -= 1.0 / 12
    L = L + L.T - 2.5 * np.eye(N)
    H = -L / (2 * h * h) + np.diag(0.5 * x * x)
    w, displ = 0.5, 4.0
    psi = (1 / (np.pi * w * w)) ** 0.25 * np.exp(-0.5 * ((x - displ) / w) ** 2)
    ew, U = np.linalg.eigh(H)
    return sp.csr_matrix(H), psi, x, ew, U


def exact(ew, U, psi0, t):
    return U @ (np.exp(-1j * t * ew) * (U.T @ psi0))


def exact_observables(N, W, phi, t):
    """(<W_k>, <phi_r|psi>, E) of exp(-i t H) psi0 from the dense eigh."""
    _, psi0, _, ew, U = oscillator(N)
    p = exact(ew, U, psi0, t)
    W = np.asarray(W, dtype=float).reshape(N, -1)
    phi = np.asarray(phi, dtype=complex).reshape(N, -1)
    c = U.T @ psi0
    return W.T @ (np.abs(p) ** 2), phi.conj().T @ p, float(np.sum(ew * c * c))


def physics_bars(N, W, phi, k):
    """The bars of a state within e_k = k 1e-10 (2-norm) of the exact one:
    | <W> - exact | <= 2 max|W| ||psi0|| e_k, | <phi|psi> - exact | <= ||phi|| e_k,
    | E - exact | <= 2 ||H||_2 ||psi0|| e_k (first order in e_k)."""
    _, psi0, _, ew, _ = oscillator(N)
    W = np.asarray(W, dtype=float).reshape(N, -1)
    phi = np.asarray(phi, dtype=complex).reshape(N, -1)
    e, n0 = k * 1e-10, np.linalg.norm(psi0)
    return (2 * np.max(np.abs(W), axis=0) * n0 * e, np.linalg.norm(phi, axis=0) * e,
            2 * np.max(np.abs(ew)) * n0 * e)


# ---- NumPy propagation: stacked real Lanczos (tests/test_prop_host.py) -------------------
def lanczos_full(A, r, m):
    """m-step Lanczos with two passes of full reorthogonalisation; stops
    early when the Krylov space is exhausted."""
    n = len(r)
    Q = np.zeros((n, m), dtype=r.dtype)
    T = np.zeros((m, m))
    Q[:, 0] = r / np.linalg.norm(r)
    for j in range(m):
        v = A @ Q[:, j]
        T[j, j] = np.real(np.vdot(Q[:, j], v))
        for _ in range(2):
            v = v - Q[:, : j + 1] @ (Q[:, : j + 1].conj().T @ v)
        beta = np.linalg.norm(v)
        if j + 1 == m or beta < 1e-12:
            return T[: j + 1, : j + 1], Q[:, : j + 1]
        T[j + 1, j] = T[j, j + 1] = beta
        Q[:, j + 1] = v / beta


def propagate_numpy(H, psi0, dt, steps, m=24):
    """The states after 1..steps time steps, by real Lanczos on blkdiag(H, H)."""
    N = H.shape[0]
    H2 = sp.block_diag([H, H], format="csr")
    x = np.concatenate([psi0.real, psi0.imag]).astype(float)
    out = []
    for _ in range(steps):
        T, Q = lanczos_full(H2, x, m)
        c = sl.expm(-1j * dt * T)[:, 0] * np.linalg.norm(x)
        p = (Q[:N] + 1j * Q[N:]) @ c
        x = np.concatenate([p.real, p.imag])
        out.append(p)
    return out
