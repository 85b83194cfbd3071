"""Host side of imaginary-time propagation (CPU only, no GPU needed).

  * cal_expm_real_col1 (c = expm(-tau (T - T11 I)) e_1, scaling and squaring in
    real arithmetic) against V exp(-tau (w - T11)) V' e_1 from numpy.linalg.eigh
    for symmetric T and scipy.linalg.expm for non-symmetric T.  Bar, taken from
    tests/test_prop_host.py: ||c - c_ref||_2 <= 64 eps max(1, ||tau T||_1)
    relative to ||expm(-tau (T - T11 I))||_2 (the exponential is not unitary
    here: its norm is exp(tau (T11 - w_min)), up to 1e200 in these cases).
    The bar holds as it stands in every case but one, and there it is the
    reference that misses it: m = 2, non-symmetric, tau ||T||_1 = 100, where
    scipy.linalg.expm is 2.98e-12 from a 50-digit evaluation (mpmath) and the
    library 6.2e-15 (bar 1.42e-12).  A case that misses the bar against SciPy
    is therefore held to the same bar against the 50-digit value, and against
    SciPy to the bar plus SciPy's own measured error; nothing else is widened.
  * the schemes of tests/imagtime_ref.py themselves: the linear iteration
    converges to the eigh ground state, the Gross-Pitaevskii energy of the
    frozen-density iteration does not increase, and its fixed point does not
    depend on tau.  The reference (dense eigh) is asserted first, then the
    oracle route (CA-Lanczos on H itself).
  * the stopping rule of ground_state, with a stub stepping function.
  * a stand-alone program (tests/native/imag_host_check.cpp) of the same host
    code under g++ -fsanitize=address,undefined (csrc/Makefile
    `imag-host-san`); nothing is preloaded, nothing is loaded into Python.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ca_lanczos_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imagtime_ref as iref  # noqa: E402

EPS = np.finfo(float).eps
SIZES = (1, 2, 3, 24, 48, 97)
NORMS = (0.1, 1.0, 10.0, 100.0, 500.0)  # tau ||T||_1


def _sym_tridiag(m, rng):
    d, e = rng.randn(m), rng.rand(max(m - 1, 0)) + 0.1
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def _norm2(E):
    """||E||_2 of a matrix whose entries may reach 1e200 (the SVD would overflow)."""
    mx = np.max(np.abs(E))
    return mx * np.linalg.norm(E / mx, 2)


def _rel(d, E):
    """||d||_2 / ||E||_2 without overflow."""
    mx = np.max(np.abs(E))
    return np.linalg.norm(d / mx) * mx / _norm2(E)


def _mp_col1(T, tau):
    """expm(-tau (T - T11 I)) e_1 in 50-digit arithmetic (mpmath, which comes
    with sympy and so with torch; README, "Tests")."""
    try:
        import mpmath as mp
    except ImportError:
        pytest.fail("this case needs the package mpmath for its 50-digit reference (a missing package, "
                    "not a numeric miss)")
    with mp.workdps(50):
        m = T.shape[0]
        A = -mp.mpf(float(tau)) * (mp.matrix(T.tolist()) - mp.mpf(float(T[0, 0])) * mp.eye(m))
        E = mp.expm(A)
        return np.array([float(E[i, 0]) for i in range(m)])


def _check(cal, T, E_of, label):
    worst = 0.0
    for target in NORMS:
        tau = target / np.linalg.norm(T, 1)
        c = cal.expm_real_col1(T, tau)
        E = E_of(tau)
        err = _rel(c - E[:, 0], E)
        bar = 64 * EPS * max(1.0, np.linalg.norm(tau * T, 1))
        print("%s m=%d tau||T||=%g err=%.3e bar=%.3e ||E||=%.3e" % (label, T.shape[0], target, err, bar, _norm2(E)))
        if err > bar and T.shape[0] <= 24:
            # the reference's own error: the same bar against a 50-digit exponential, and
            # against the reference the bar plus what the reference itself is off by
            ref = _mp_col1(T, tau)
            e_ref, e_mp = _rel(E[:, 0] - ref, E), _rel(c - ref, E)
            print("  the reference is off by %.3e from the 50-digit value, the library by %.3e" % (e_ref, e_mp))
            assert e_mp <= bar, (label, T.shape[0], target, e_mp, bar)
            bar = bar + e_ref
        assert err <= bar, (label, T.shape[0], target, err, bar)
        worst = max(worst, err / bar)
    return worst


@pytest.mark.parametrize("m", SIZES)
def test_expm_real_col1_symmetric_vs_eigh(cal, m):
    T = _sym_tridiag(m, np.random.RandomState(100 + m))
    w, V = np.linalg.eigh(T)
    _check(cal, T, lambda tau: (V * np.exp(-tau * (w - T[0, 0]))) @ V.T, "symmetric")


@pytest.mark.parametrize("m", SIZES)
def test_expm_real_col1_nonsymmetric_vs_scipy(cal, m):
    """Random tridiagonals plus a 1e-3 non-symmetric perturbation: T is taken as it comes."""
    rng = np.random.RandomState(200 + m)
    T = _sym_tridiag(m, rng) + 1e-3 * np.triu(np.tril(rng.randn(m, m), 3), -1)
    assert m == 1 or np.max(np.abs(T - T.T)) > 1e-5
    _check(cal, T, lambda tau: sl.expm(-tau * (T - T[0, 0] * np.eye(m))), "nonsymmetric")


def test_expm_real_col1_on_ca_lanczos_T(cal):
    """The T of the oracle's CA-Lanczos on the oscillator (Newton basis, 'local'), not symmetrised."""
    from oracle import ca_lanczos_ref as ref
    H, psi0, _, _, _ = iref.oscillator(256)
    T = ref.ca_lanczos(H, psi0, 6, 24, "newton", "local", diagnostics=False).T
    assert T.shape == (24, 24) and not np.array_equal(T, T.T)
    _check(cal, T, lambda tau: sl.expm(-tau * (T - T[0, 0] * np.eye(24))), "oracle T")


def test_expm_real_col1_leading_dimension_and_errors(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, CAL_ERR_NUMERIC, lib, ptr
    T = _sym_tridiag(7, np.random.RandomState(3))
    big = np.asfortranarray(np.full((11, 7), np.nan))
    big[:7, :] = T
    c = np.zeros(7)
    assert lib.cal_expm_real_col1(7, ptr(big), 11, 0.4, ptr(c)) == 0
    assert np.array_equal(c, cal.expm_real_col1(T, 0.4))
    assert cal.expm_real_col1(T, 0.0)[0] == 1.0 and not np.any(cal.expm_real_col1(T, 0.0)[1:])
    assert np.array_equal(cal.expm_real_col1(np.array([[3.5]]), 2.0), [1.0])  # the shift: exp(0)
    one = np.ones(1)
    assert lib.cal_expm_real_col1(0, ptr(one), 1, 0.1, ptr(c)) == CAL_ERR_ARG
    assert lib.cal_expm_real_col1(513, ptr(one), 513, 0.1, ptr(c)) == CAL_ERR_ARG
    assert lib.cal_expm_real_col1(7, ptr(big), 6, 0.1, ptr(c)) == CAL_ERR_ARG
    assert lib.cal_expm_real_col1(7, ptr(big), 11, float("nan"), ptr(c)) == CAL_ERR_ARG
    assert lib.cal_expm_real_col1(7, ptr(big), 11, float("inf"), ptr(c)) == CAL_ERR_ARG
    for v in (np.inf, np.nan):
        bad = T.copy(order="F")
        bad[3, 2] = v
        with pytest.raises(cal.CalError) as e:
            cal.expm_real_col1(bad, 0.1)
        assert e.value.status == CAL_ERR_NUMERIC
    # a NaN in a block that is not coupled to e_1 never reaches the first column: refused all the same
    blk = np.zeros((4, 4), order="F")
    blk[:2, :2] = [[1.0, 0.5], [0.5, 2.0]]
    blk[2:, 2:] = [[1.0, np.nan], [0.25, 3.0]]
    with pytest.raises(cal.CalError) as e:
        cal.expm_real_col1(blk, 0.1)
    assert e.value.status == CAL_ERR_NUMERIC
    blk[2, 3] = 0.25
    assert np.all(np.isfinite(cal.expm_real_col1(blk, 0.1)))


# ---- the schemes ---------------------------------------------------------------------------------------
N, TAU, S, BLOCKS = 256, 0.2, 6, 4


def run_until(step_states, H, g, tol, max_steps=400):
    """Step a scheme (a function psi -> next psi) until the state it starts a
    step from meets residual <= tol max(1, |mu|), as ground_state does;
    returns (the states psi_0 .., the energetics rows of each but the last)."""
    states, rows = [step_states[0]], []
    for _ in range(max_steps):
        mu, E, res, _ = iref.energetics(H, states[-1], g)
        rows.append((mu, E, res))
        states.append(step_states[1](states[-1]))
        if res <= tol * max(1.0, abs(mu)):
            break
    return states, np.array(rows)


def dense_step(H, g, tau):
    return lambda psi: iref.dense_imag(H, [], psi, np.zeros((1, 0)), tau, g, "frozen")


def oracle_step(H, g, tau):
    return lambda psi: iref.oracle_imag(H, [], psi, np.zeros((1, 0)), tau, g, "frozen", S, BLOCKS, "newton", False)


@pytest.mark.parametrize("route", ["dense", "oracle"])
def test_linear_converges_to_the_ground_state(route):
    H, psi0, _, ew, U = iref.oscillator(N)
    step = dense_step(H, 0.0, TAU) if route == "dense" else oracle_step(H, 0.0, TAU)
    states, rows = run_until((psi0, step), H, 0.0, 1e-10)
    psi = states[-1]
    n0 = np.linalg.norm(psi0)
    overlap = abs(U[:, 0] @ psi) / n0
    mu = iref.energetics(H, psi)[0]
    print("%s: %d steps, 1 - overlap %.3e, mu - ew0 %.3e, residual %.3e" % (route, len(rows), 1 - overlap, mu - ew[0],
                                                                            rows[-1, 2]))
    assert len(rows) < 400 and rows[-1, 2] <= 1e-10 * max(1.0, abs(rows[-1, 0]))
    assert 1.0 - overlap <= 1e-12
    assert abs(mu - ew[0]) <= 1e-10
    assert abs(np.linalg.norm(psi) - n0) <= 1e-12


@pytest.mark.parametrize("g", [1.0, 5.0])
def test_gp_energy_does_not_increase(g):
    """E_n of the frozen-density iteration, from the true Rayleigh quotient.
    The slack is the rounding of two such energies: each is N mu with mu
    rounded to 1.4 eps ||H[psi]||_inf (imagtime_ref.energetics)."""
    H, psi0, _, _, _ = iref.oscillator(N)
    n2 = float(psi0 @ psi0)
    out = {}
    for route, step in (("dense", dense_step(H, g, TAU)), ("oracle", oracle_step(H, g, TAU))):
        states, rows = run_until((psi0, step), H, g, 1e-8)
        slack = 2 * n2 * max(iref.energetics(H, p, g)[3] for p in states[:3])
        worst = np.max(np.diff(rows[:, 1]))
        print("g=%g %s: %d steps, E %.12f -> %.12f, largest increase %.3e (slack %.3e)"
              % (g, route, len(rows), rows[0, 1], rows[-1, 1], worst, slack))
        assert len(rows) < 400 and rows[-1, 2] <= 1e-8 * max(1.0, abs(rows[-1, 0])), route
        assert worst <= slack, (route, worst, slack)
        out[route] = rows[-1]
    assert abs(out["dense"][0] - out["oracle"][0]) <= 1e-8 * max(1.0, abs(out["dense"][0]))


@pytest.mark.parametrize("g", [0.0, 1.0])
def test_fixed_point_does_not_depend_on_tau(g):
    """A state converged at tau = 0.2 is an eigenvector of H[psi] to the
    tolerance; a step at another tau leaves it one (frozen density)."""
    tol = 1e-9
    H, psi0, _, _, _ = iref.oscillator(N)
    states, rows = run_until((psi0, dense_step(H, g, TAU)), H, g, tol)
    psi = states[-1]
    mu, _, res, _ = iref.energetics(H, psi, g)
    assert res <= tol * max(1.0, abs(mu))
    for tau in (0.05, 0.5):
        for step in (dense_step(H, g, tau), oracle_step(H, g, tau)):
            nxt = step(psi)
            mu2, _, res2, _ = iref.energetics(H, nxt, g)
            print("g=%g tau=%g: residual %.3e -> %.3e, mu %.12f -> %.12f" % (g, tau, res, res2, mu, mu2))
            assert res2 <= tol * max(1.0, abs(mu2))
            assert abs(mu2 - mu) <= tol


# ---- the driver's stopping rule ------------------------------------------------------------------------
class Stub:
    """Residuals halve every step; an optional breakdown at step `bd`."""

    def __init__(self, bd=None, r0=1.0):
        self.k, self.bd, self.r0, self.rows = 0, bd, r0, []

    def step(self):
        from ca_lanczos_amd._lib import CAL_WARN_BREAKDOWN
        if self.bd is not None and self.k == self.bd:
            return CAL_WARN_BREAKDOWN  # no row, the state unchanged
        self.rows.append((0.1 * self.k, 1.0, -3.0, -3.0, self.r0 * 0.5 ** self.k))
        self.k += 1
        return 0

    def last(self):
        r = np.array(self.rows).reshape(-1, 5)
        return dict(t=r[:, 0], norm2=r[:, 1], mu=r[:, 2], energy=r[:, 3], residual=r[:, 4])

    def state(self):
        return np.full(3, float(self.k))


def test_ground_state_stopping_rule(cal):
    # the criterion is relative to max(1, |mu|) = 3: 0.5^k <= 3e-3 first at k = 9, seen after 10 steps
    s = Stub()
    out = cal.api._ground_state_loop(s.step, s.last, s.state, 1e-3, 100)
    assert out["converged"] and out["steps"] == 10 and out["residual"] == 0.5 ** 9 and out["mu"] == -3.0
    assert out["psi"][0] == 10.0 and len(out["history"]["mu"]) == 10
    # max_steps runs out first
    s = Stub()
    out = cal.api._ground_state_loop(s.step, s.last, s.state, 1e-3, 4)
    assert not out["converged"] and out["steps"] == 4 and out["residual"] == 0.5 ** 3
    # a breakdown whose last row meets the criterion: converged; the state is the unchanged one
    s = Stub(bd=0)
    s.rows.append((0.0, 1.0, -3.0, -3.0, 1e-6))
    out = cal.api._ground_state_loop(s.step, s.last, s.state, 1e-3, 100)
    assert out["converged"] and out["steps"] == 0 and out["residual"] == 1e-6 and out["psi"][0] == 0.0
    s = Stub(bd=3, r0=1.0)
    out = cal.api._ground_state_loop(s.step, s.last, s.state, 1e-3, 100)
    assert not out["converged"] and out["steps"] == 3 and out["residual"] == 0.25
    # a breakdown before any row
    s = Stub(bd=0)
    out = cal.api._ground_state_loop(s.step, s.last, s.state, 1e-3, 100)
    assert not out["converged"] and out["steps"] == 0 and np.isnan(out["mu"])


# ---- the sanitized stand-alone program ------------------------------------------------------------------
def test_imag_host_check_sanitized():
    p = subprocess.run(["make", "-C", CSRC, "imag-host-san"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(CSRC, "build", "imag_host_check_san")], capture_output=True, text=True, env=env,
                       timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, \
        p.stdout + p.stderr[-3000:]
    assert "imag host check ok" in p.stdout
