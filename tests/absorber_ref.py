"""NumPy references for the propagator's absorbing mask
(test_absorber_host.py, test_gpu_absorber.py).

The scheme, per completed time step (include/calanczos.h):
  u = nrm Q_c c;  psi' = M .* u;  absorbed = sum_i (1 - M_i^2) |u_i|^2
the kernel's chain per row, with ut, ub the two sums of the row and m = M_i:
  d = ut*ut;  d = d + ub*ub;  p = m*m;  g = 1.0 - p;  acc = acc + g*d
  t = m*ut;   b = m*ub

Rounding bars: those of tests/prop_obs_ref.py -- a sum of N products whose
absolute values sum to S is within (N + 8) eps S of the exact sum.
  absorbed: N = n,  S = sum (1 - M^2) |u|^2;   norm2: N = 2n, S = norm2.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prop_obs_ref as pref  # noqa: E402
from prop_obs_ref import combine_ref  # noqa: E402,F401  (the plain combine's chain)

EPS = np.finfo(float).eps


def masked_ref(top, bot, M):
    """(M * top, M * bot, the terms (1 - M^2)(top^2 + bot^2) in the kernel's
    order of operations): the stored halves to the bit, the terms of absorbed."""
    d = top * top
    d = d + bot * bot
    p = M * M
    g = 1.0 - p
    return M * top, M * bot, g * d


def absorbed_bar(terms):
    return (len(terms) + 8) * EPS * np.sum(np.abs(terms))


def norm2_ref(t, b):
    """(sum t^2 + b^2, its bar)."""
    v = np.sum(t * t) + np.sum(b * b)
    return v, (2 * len(t) + 8) * EPS * v


def oscillator_mask(x):
    """The mask of the oscillator tests: 1 for |x| <= 3, ramping down to the box's edge at 10."""
    return np.cos(0.5 * np.pi * np.clip((np.abs(x) - 3.0) / 7.0, 0.0, 1.0)) ** 0.125


def dense_scheme(N, M, dt, steps):
    """psi <- M .* U exp(-i dt E) U' psi on prop_obs_ref.oscillator(N):
    (the states after 1..steps steps, the unmasked u of every step, absorbed per step)."""
    _, psi0, _, ew, U = pref.oscillator(N)
    ph = np.exp(-1j * dt * ew)
    psi = psi0.astype(complex)
    states, us, ab = [], [], []
    for _ in range(steps):
        u = U @ (ph * (U.T @ psi))
        ab.append(float(np.sum((1.0 - M * M) * np.abs(u) ** 2)))
        psi = M * u
        us.append(u)
        states.append(psi)
    return states, us, np.array(ab)


def propagate_numpy_masked(H, psi0, M, dt, steps, m=24):
    """prop_obs_ref.propagate_numpy with the mask after every step:
    (the states, absorbed per step)."""
    import scipy.linalg as sl
    import scipy.sparse as sp
    N = H.shape[0]
    H2 = sp.block_diag([H, H], format="csr")
    x = np.concatenate([psi0.real, psi0.imag]).astype(float)
    out, ab = [], []
    for _ in range(steps):
        T, Q = pref.lanczos_full(H2, x, m)
        c = sl.expm(-1j * dt * T)[:, 0] * np.linalg.norm(x)
        u = (Q[:N] + 1j * Q[N:]) @ c
        t, b, terms = masked_ref(u.real, u.imag, M)
        ab.append(float(np.sum(terms)))
        x = np.concatenate([t, b])
        out.append(t + 1j * b)
    return out, np.array(ab)
