"""Host side of the Krylov time propagation (CPU only, no GPU needed).

  * cal_expm_col1 (c = expm(-i dt T) e_1, scaling and squaring in complex
    arithmetic) against independent evaluations: V exp(-i dt w) V' e_1 from
    numpy.linalg.eigh for symmetric T, scipy.linalg.expm for non-symmetric T.
    Bar: ||c - c_ref||_2 <= 64 eps max(1, ||dt T||_1) -- the number of
    squarings grows with log2 ||dt T|| and each roughly doubles the
    accumulated rounding, so the error scales with the norm.  For symmetric T
    the same bar holds for | ||c||_2 - 1 | (unitarity).
  * the claim the feature rests on, in NumPy alone: Hermitian Lanczos on a
    complex start vector psi = u + i v of a real symmetric H is real Lanczos
    on blkdiag(H, H) from [u; v]; both propagate the reference's harmonic
    oscillator (runLanczos.m:5-21) to the dense exponential's answer.
  * a stand-alone program (tests/native/prop_host_check.cpp) of the same host
    code under g++ -fsanitize=address,undefined (csrc/Makefile
    `prop-host-san`); nothing is preloaded, nothing is loaded into Python.
"""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ca_lanczos_amd", "csrc")
EPS = np.finfo(float).eps
SIZES = (1, 2, 7, 24, 48, 121)
NORMS = (1e-3, 0.3, 1.0, 7.0, 50.0)  # ||dt T||_1


def _bar(T, dt):
    return 64 * EPS * max(1.0, np.linalg.norm(dt * T, 1))


def _sym_tridiag(m, rng):
    d, e = rng.randn(m), rng.rand(max(m - 1, 0)) + 0.1
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


@pytest.mark.parametrize("m", SIZES)
def test_expm_col1_symmetric_vs_eigh(cal, m):
    rng = np.random.RandomState(100 + m)
    T = _sym_tridiag(m, rng)
    w, V = np.linalg.eigh(T)
    for target in NORMS:
        dt = target / np.linalg.norm(T, 1)
        c = cal.expm_col1(T, dt)
        c_ref = V @ (np.exp(-1j * dt * w) * V[0, :])
        err, uni, bar = np.linalg.norm(c - c_ref), abs(np.linalg.norm(c) - 1.0), _bar(T, dt)
        print("m=%d ||dt T||=%g err=%.3e unitarity=%.3e bar=%.3e" % (m, target, err, uni, bar))
        assert err <= bar, (m, target, err, bar)
        assert uni <= bar, (m, target, uni, bar)


@pytest.mark.parametrize("m", SIZES)
def test_expm_col1_nonsymmetric_vs_scipy(cal, m):
    """Random tridiagonals plus a 1e-3 non-symmetric perturbation (the CA
    loop's T is only nearly symmetric and is exponentiated as it comes)."""
    rng = np.random.RandomState(200 + m)
    T = _sym_tridiag(m, rng) + 1e-3 * np.triu(np.tril(rng.randn(m, m), 3), -1)
    assert m == 1 or np.max(np.abs(T - T.T)) > 1e-5
    for target in NORMS:
        dt = target / np.linalg.norm(T, 1)
        c = cal.expm_col1(T, dt)
        c_ref = sl.expm(-1j * dt * T)[:, 0]
        err, bar = np.linalg.norm(c - c_ref), _bar(T, dt)
        print("m=%d ||dt T||=%g err=%.3e bar=%.3e" % (m, target, err, bar))
        assert err <= bar, (m, target, err, bar)


def test_expm_col1_on_ca_lanczos_T(cal):
    """The T of a CA-Lanczos run (Newton basis, 'local'), not symmetrised."""
    T = np.load(os.path.join(ROOT, "tests", "golden", "lap2d_32_s8_newton_local.npz"))["T"]
    assert T.shape[0] == T.shape[1] and not np.array_equal(T, T.T)
    for target in NORMS:
        dt = target / np.linalg.norm(T, 1)
        c = cal.expm_col1(T, dt)
        c_ref = sl.expm(-1j * dt * T)[:, 0]
        err, bar = np.linalg.norm(c - c_ref), _bar(T, dt)
        print("golden T m=%d ||dt T||=%g err=%.3e bar=%.3e" % (T.shape[0], target, err, bar))
        assert err <= bar, (target, err, bar)


def test_expm_col1_leading_dimension_and_errors(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    rng = np.random.RandomState(3)
    T = _sym_tridiag(7, rng)
    big = np.asfortranarray(np.full((11, 7), np.nan))
    big[:7, :] = T
    cre, cim = np.zeros(7), np.zeros(7)
    assert lib.cal_expm_col1(7, ptr(big), 11, 0.4, ptr(cre), ptr(cim)) == 0
    assert np.array_equal(cre + 1j * cim, cal.expm_col1(T, 0.4))
    one = np.ones(1)
    assert lib.cal_expm_col1(0, ptr(one), 1, 0.1, ptr(cre), ptr(cim)) == CAL_ERR_ARG
    assert lib.cal_expm_col1(513, ptr(one), 513, 0.1, ptr(cre), ptr(cim)) == CAL_ERR_ARG
    assert lib.cal_expm_col1(7, ptr(big), 11, float("nan"), ptr(cre), ptr(cim)) == CAL_ERR_ARG


# ---- the stacked equivalence, NumPy only -------------------------------------
def oscillator(N):
    """H and psi of runLanczos.m:5-21 (dense; H is real symmetric, periodic
    fourth-order Laplacian plus the harmonic potential)."""
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
    return H, psi


def _lanczos_full(A, r, m):
    """m-step Lanczos with two passes of full reorthogonalisation (real or
    complex start); stops early when the Krylov space is exhausted."""
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


def test_stacked_real_lanczos_equals_complex_lanczos():
    N, steps, dt, m = 256, 8, 0.025, 24
    H, psi0 = oscillator(N)
    w, U = np.linalg.eigh(H)
    exact = U @ (np.exp(-1j * steps * dt * w) * (U.T @ psi0))
    H2 = np.block([[H, np.zeros((N, N))], [np.zeros((N, N)), H]])
    pc = psi0.astype(complex)
    ps = np.concatenate([psi0, np.zeros(N)])
    for _ in range(steps):
        T, Q = _lanczos_full(H, pc, m)
        pc = Q @ (sl.expm(-1j * dt * T)[:, 0] * np.linalg.norm(pc))
        T, Q = _lanczos_full(H2, ps, m)
        c = sl.expm(-1j * dt * T)[:, 0] * np.linalg.norm(ps)
        out = (Q[:N] + 1j * Q[N:]) @ c
        ps = np.concatenate([out.real, out.imag])
    e_c = np.linalg.norm(pc - exact)
    e_s = np.linalg.norm(ps[:N] + 1j * ps[N:] - exact)
    print("complex Lanczos err %.3e, stacked real Lanczos err %.3e" % (e_c, e_s))
    assert e_c <= steps * 1e-10 and e_s <= steps * 1e-10


# ---- the sanitized stand-alone program ---------------------------------------
def test_prop_host_check_sanitized():
    p = subprocess.run(["make", "-C", CSRC, "prop-host-san"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(CSRC, "build", "prop_host_check_san")], capture_output=True, text=True, env=env,
                       timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, \
        p.stdout + p.stderr[-3000:]
    assert "prop host check ok" in p.stdout
