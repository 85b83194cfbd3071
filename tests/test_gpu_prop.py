"""Krylov time propagation psi(t+dt) = exp(-i dt H) psi(t) on the device
(cal_prop_*, ca_lanczos_prop.m as runLanczos.m:84-131 drives it).

Bars:
  * the combine kernel (k_prop_combine) is bit-exact against a NumPy loop in
    its documented order (one chain per output row, j ascending; the build
    does not contract a*b+c); its squared norm is within 2n eps (relative) of
    np.sum(out**2), the worst case for any summation order of non-negative
    terms; two runs give identical bits.
  * propagation: 2-norm error against the dense eigh exponential at most
    steps * 1e-10 -- the reference's default tol = 1e-10 bounds each step's
    residual estimate and unitary steps add their errors.  The CPU oracle
    (oracle.ca_lanczos_ref.ca_lanczos on the stacked matrix, 'local', then
    the same propagation in NumPy) is held to the same bar.  The norm is
    conserved to the same bar at every step.
"""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prop_obs_ref import combine_ref  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


# ---- problems ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oscillator(N):
    """H (CSR) and psi of runLanczos.m:5-21, with the dense eigh of H."""
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
    return sp.csr_matrix(H), psi, ew, U


@functools.lru_cache(maxsize=None)
def packet_2d():
    """laplacian_2d(40) and a Gaussian packet times exp(i(0.7x + 0.3y))."""
    from ca_lanczos_amd import matrices
    N = 40
    H = matrices.laplacian_2d(N)
    y, x = np.divmod(np.arange(N * N), N)
    psi = np.exp(-((x - 19.5) ** 2 + (y - 19.5) ** 2) / (2 * 4.0 ** 2)) * np.exp(1j * (0.7 * x + 0.3 * y))
    ew, U = np.linalg.eigh(H.toarray())
    return H, psi, ew, U


def exact(ew, U, psi0, t):
    return U @ (np.exp(-1j * t * ew) * (U.T @ psi0))


@functools.lru_cache(maxsize=None)
def oracle_error(N, s, blocks, basis, dt, steps):
    """The CPU oracle's propagation error on the oscillator."""
    from oracle import ca_lanczos_ref as ref
    H, psi0, ew, U = oscillator(N)
    A2 = sp.block_diag([H, H], format="csr")
    x = np.concatenate([psi0, np.zeros(N)])
    for _ in range(steps):
        nrm = np.linalg.norm(x)
        res = ref.ca_lanczos(A2, x, s, s * blocks, basis, "local", diagnostics=False)
        c = sl.expm(-1j * dt * res.T)[:, 0] * nrm
        out = (res.Q[:N] + 1j * res.Q[N:]) @ c
        x = np.concatenate([out.real, out.imag])
    return np.linalg.norm(x[:N] + 1j * x[N:] - exact(ew, U, psi0, steps * dt))


# ---- 1. the combine kernel (its NumPy chain: prop_obs_ref.combine_ref) ------------------
@pytest.fixture(scope="module")
def ctx(cal):
    c = cal.Context()
    yield c
    c.close()


@pytest.mark.parametrize("m", [1, 6, 24, 97])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 20001])
def test_combine_bit_exact(ctx, n, m):
    rng = np.random.RandomState(1000 * m + n)
    Q = np.asfortranarray(rng.randn(2 * n, m))
    c = rng.randn(m) + 1j * rng.randn(m)
    out, n2 = ctx.prop_combine(Q, c)
    top, bot = combine_ref(Q, c)
    assert np.array_equal(out.real, top)
    assert np.array_equal(out.imag, bot)
    ref2 = np.sum(top ** 2) + np.sum(bot ** 2)
    assert abs(n2 - ref2) <= 2 * n * EPS * ref2, (n2, ref2)
    out_b, n2_b = ctx.prop_combine(Q, c)
    assert np.array_equal(out, out_b) and n2 == n2_b


# ---- 2. / 3. the harmonic oscillator ---------------------------------------------------
def run_oscillator(cal, N, s, blocks, basis, steps, dt, adaptive=False, tol=1e-10):
    H, psi0, ew, U = oscillator(N)
    P = cal.Propagator(H, psi0, s, blocks, basis=basis)
    try:
        n0 = np.linalg.norm(psi0)
        lsteps, drift = [], 0.0
        for _ in range(steps):
            assert P.step(dt, 1, tol=tol, adaptive=adaptive) == 0
            i = P.info()
            lsteps.append(i["lsteps"])
            drift = max(drift, abs(i["norm"] - n0))
        psi, info = P.state(), P.info()
    finally:
        P.close()
    err = np.linalg.norm(psi - exact(ew, U, psi0, steps * dt))
    assert abs(np.linalg.norm(psi) - info["norm"]) <= 1e-13 * n0
    return err, drift, lsteps, info


@pytest.mark.parametrize("s,blocks", [(6, 4), (4, 6)])
@pytest.mark.parametrize("basis", ["newton", "monomial"])
@pytest.mark.parametrize("N", [256, 255])
def test_oscillator(cal, N, basis, s, blocks):
    steps, dt = 8, 0.025
    bar = steps * 1e-10
    err, drift, lsteps, info = run_oscillator(cal, N, s, blocks, basis, steps, dt)
    e_or = oracle_error(N, s, blocks, basis, dt, steps)
    print("N=%d %s s=%d blocks=%d: err %.3e, oracle err %.3e, norm drift %.3e, breakdowns %d, residual_max %.3e"
          % (N, basis, s, blocks, err, e_or, drift, info["breakdowns"], info["residual_max"]))
    assert e_or <= bar, e_or
    assert err <= bar, err
    assert drift <= bar, drift
    assert info["steps"] == steps and lsteps == [s * blocks] * steps
    assert info["lsteps_sum"] == steps * s * blocks and info["lsteps_max"] == s * blocks


@pytest.mark.parametrize("s,blocks,expect", [(6, 4, 12), (4, 6, 12)])
def test_adaptive_stopping(cal, s, blocks, expect):
    steps, dt, tol = 8, 0.025, 1e-9
    err, drift, lsteps, info = run_oscillator(cal, 256, s, blocks, "newton", steps, dt, adaptive=True, tol=tol)
    print("adaptive s=%d: lsteps %s, err %.3e, residual_max %.3e" % (s, lsteps, err, info["residual_max"]))
    assert lsteps == [expect] * steps
    assert err <= steps * 1e-10 and drift <= steps * 1e-10
    assert info["residual_max"] < tol


# ---- 4. complex start, pattern-format matrix ---------------------------------------------
@pytest.mark.parametrize("dt,s,blocks", [(0.5, 6, 4), (1.0, 8, 3)])
@pytest.mark.parametrize("basis", ["newton", "monomial"])
def test_complex_start_pattern_matrix(cal, basis, dt, s, blocks):
    H, psi0, ew, U = packet_2d()
    assert 0.92 <= np.max(psi0.imag) < 0.93  # a start state that is truly complex
    steps = 4
    P = cal.Propagator(H, psi0, s, blocks, basis=basis)
    try:
        fmt, npat, _ = P.ctx.spmv_format()
        alone = cal.Context().set_matrix(H)
        fmt1, npat1, _ = alone.spmv_format()
        alone.close()
        assert fmt == "pattern" and fmt1 == "pattern" and npat == npat1
        assert P.ctx.matrix_info()["n_local"] == 2 * H.shape[0]
        assert P.step(dt, steps) == 0
        psi = P.state()
    finally:
        P.close()
    err = np.linalg.norm(psi - exact(ew, U, psi0, steps * dt))
    print("lap2d_40 %s dt=%g s=%d blocks=%d: err %.3e" % (basis, dt, s, blocks, err))
    assert err <= steps * 1e-10


def test_complex_start_csr_format(cal):
    H, psi0, ew, U = packet_2d()
    steps, dt = 4, 0.5
    c = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, 6, 4, ctx=c)
        assert c.spmv_format()[0] == "csr"
        assert P.step(dt, steps) == 0
        psi = P.state()
        P.close()
    finally:
        c.close()
    err = np.linalg.norm(psi - exact(ew, U, psi0, steps * dt))
    print("lap2d_40 csr: err %.3e" % err)
    assert err <= steps * 1e-10


# ---- 5. the one-shot mirror of ca_lanczos_prop ----------------------------------------------
def test_one_shot_matches_a_step(cal):
    H, psi0, _, _ = packet_2d()
    n, s, m, dt = H.shape[0], 6, 4, 0.5
    T, Q, lsteps = cal.ca_lanczos_prop(H, psi0, s, m, dt)
    assert lsteps == s * m and T.shape == (lsteps, lsteps) and Q.shape == (n, lsteps) and np.iscomplexobj(Q)
    G = Q[:, :s].conj().T @ Q[:, :s]
    assert np.max(np.abs(G - np.eye(s))) < 1e-10
    nrm = np.linalg.norm(psi0)
    mine = Q @ (sl.expm(-1j * dt * T)[:, 0] * nrm)
    P = cal.Propagator(H, psi0, s, m)
    try:
        assert P.step(dt) == 0
        step = P.state()
    finally:
        P.close()
    d = np.linalg.norm(mine - step)
    print("one-shot vs step: %.3e (bar %.3e)" % (d, 1e-13 * nrm))
    assert d <= 1e-13 * nrm


# ---- 6. residency ---------------------------------------------------------------------------
def test_state_stays_resident(cal, ref):
    H, psi0, _, _ = oscillator(256)
    c = cal.Context()
    try:
        P = cal.Propagator(H, psi0, 6, 4, ctx=c)
        P.step(0.025, 5)
        mid = P.state()  # the copy back does not disturb the run
        P.step(0.025, 5)
        a = P.state()
        assert P.info()["steps"] == 10 and not np.array_equal(mid, a)
        P.close()
        P = cal.Propagator(H, psi0, 6, 4, ctx=c)
        P.step(0.025, 10)
        b = P.state()
        P.close()
        assert np.array_equal(a, b)
        # the context still serves cal_lanczos_begin-based calls
        A = cal.matrices.laplacian_2d(24)
        r = ref.matlab_rand(24 * 24)
        c.set_matrix(A)
        out = cal.ca_lanczos_ex(A, r, 8, 24, "newton", "local", diagnostics=False, ctx=c)
        fresh = cal.Context().set_matrix(A)
        exp = cal.ca_lanczos_ex(A, r, 8, 24, "newton", "local", diagnostics=False, ctx=fresh)
        fresh.close()
        assert np.array_equal(out.T, exp.T) and np.array_equal(out.Q, exp.Q)
    finally:
        c.close()


# ---- 7. errors -------------------------------------------------------------------------------
def test_bad_arguments(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    H, psi0, _, _ = oscillator(256)
    n = H.shape[0]
    re = np.ascontiguousarray(psi0)
    c = cal.Context()
    try:
        c.set_matrix(H)  # n rows instead of 2n
        assert lib.cal_prop_begin(c.h, n, ptr(re), None, 6, 4, b"newton", None, 0) == CAL_ERR_ARG
        c.set_matrix_stacked(H)
        assert lib.cal_prop_begin(c.h, n, ptr(re), None, 32, 1, b"newton", None, 0) == CAL_ERR_ARG
        assert lib.cal_prop_begin(c.h, n, ptr(re), None, 27, 19, b"newton", None, 0) == CAL_ERR_ARG  # 513
        assert lib.cal_prop_begin(c.h, n, ptr(re), None, 6, 4, b"chebyshev", None, 0) == CAL_ERR_ARG
        assert lib.cal_prop_step(c.h, 0.025, 1e-10, 0, 1) == CAL_ERR_ARG  # no propagator was left behind
        assert lib.cal_prop_begin(c.h, n, ptr(re), None, 6, 4, b"newton", None, 0) == 0
        assert lib.cal_prop_step(c.h, float("nan"), 1e-10, 0, 1) == CAL_ERR_ARG
        assert lib.cal_prop_step(c.h, 0.025, 1e-10, 0, 1) == 0
        assert lib.cal_prop_end(c.h) == 0
    finally:
        c.close()
