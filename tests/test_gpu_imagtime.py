"""Imaginary-time propagation on the device: cal_prop_set_imaginary_time, the
real-state path (cal_prop_begin_real, kernels k_prop_combine<.., REAL> and
k_diag_density<.., REAL>), the energetics rows and ground_state.

Bars:
  * k_prop_combine<.., REAL>'s out is the NumPy chain of tests/imagtime_ref.py
    combine_real_ref to the bit; norm2 and <W_k> within the derived rounding
    bar (N + 8) eps S of tests/prop_obs_ref.py.  The real density's diagonal is
    tests/nonlinear_ref.py density_chain with real states to the bit.
  * a stacked imaginary-time step is the untouched k_prop_combine with the
    real coefficients a = sqrt(N) c / ||c||_2, b = 0: combine_ref's bits.
  * propagation: 2-norm error against the same scheme with dense eigh
    exponentials at most builds * 1e-10 (8 steps of tau = 0.025: 8 builds
    "frozen", 16 "midpoint"), the same for |norm2 - N|; the CPU oracle route is
    held to the same bar next to the device (tests/test_gpu_nonlinear.py).
  * energetics: mu_n against the true Rayleigh quotient of P.state().  Measured
    on the CPU, the oracle's T(1,1) is within 1.49e-13 of it over these cases
    (0.99 of 1.4 eps ||H[psi]||_inf, ||H||_inf = 486), its ||T(2:,1)|| within
    1.0e-14 of the true residual.  The device sums in another order and is
    allowed 8 x 1.5e-13 = 1.2e-12 for mu and for the residual; the energy
    N mu - (g/2) sum|psi|^4 gets N times that plus (|g|/2) times the bar of
    the quartic sum.  The oracle is held to the same bars next to the device.
  * the driver: at most the dense scheme's step count + 5; |mu - ew[0]| <=
    1e-10, 1 - overlap <= 1e-12; the real and the stacked route give the same
    mu within the energetics' bar of 1.2e-12 (measured: 1.7e-13).  In real
    time the drift of E_n is held to the dense scheme's own drift plus the
    energy's bar, once.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imagtime_ref as iref  # noqa: E402
import nonlinear_ref as nref  # noqa: E402
from split_cases import lap3d_v  # noqa: E402

pref = nref.pref
EPS = pref.EPS
pytestmark = pytest.mark.gpu
G = 0.75
MU_BAR = 8 * 1.5e-13


@pytest.fixture(scope="module")
def ctx(cal):
    c = cal.Context()
    yield c
    c.close()


# ---- 1. the real combine kernel's bits -----------------------------------------------------------------
def _check_combine(ctx, Q, a, W):
    n = Q.shape[0]
    out, n2, wv = ctx.prop_combine_real(Q, a, W if len(W) else None)
    expect = iref.combine_real_ref(np.asarray(Q), a)
    assert np.array_equal(out, expect)
    S = float(np.sum(expect * expect))
    assert abs(n2 - S) <= (n + 8) * EPS * S, (n2, S)
    assert len(wv) == len(W)
    for k, w in enumerate(W):
        ref, bar = float(w @ (expect * expect)), (n + 8) * EPS * float(np.abs(w) @ (expect * expect))
        assert abs(wv[k] - ref) <= bar, (k, wv[k], ref, bar)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 20001])
def test_combine_real_bits(ctx, n):
    rng = np.random.RandomState(n)
    for m in (1, 6, 24, 97):
        Q = np.asfortranarray(rng.randn(n, m))
        a = rng.randn(m)
        for nw in (0, 1, 4):
            _check_combine(ctx, Q, a, [rng.randn(n) for _ in range(nw)])
    # an odd leading dimension: the 8-byte path
    ldq = n + 1 if n % 2 == 0 else n + 2
    for m in (6, 97):
        big = np.asfortranarray(np.full((ldq, m), np.nan))
        big[:n, :] = rng.randn(n, m)
        Q = big[:n, :]
        assert Q.strides[1] == ldq * 8 and ldq % 2 == 1
        a = rng.randn(m)
        for nw in (0, 4):
            _check_combine(ctx, Q, a, [rng.randn(n) for _ in range(nw)])


def test_combine_real_argument_errors(cal, ctx):
    Q = np.asfortranarray(np.ones((4, 3)))
    with pytest.raises(ValueError):
        ctx.prop_combine_real(Q, np.ones(2))
    with pytest.raises(cal.CalError):
        ctx.prop_combine_real(np.ones((2, 513), order="F"), np.ones(513))
    with pytest.raises(cal.CalError):
        ctx.prop_combine_real(Q, np.ones(3), [np.ones(4)] * 5)


# ---- 2. the real density's bits --------------------------------------------------------------------------
def canon(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    return A


def tridiag(n, seed):
    rng = np.random.RandomState(seed)
    e = rng.randn(n - 1)
    return canon(sp.diags([e, rng.randn(n) + 3.0, e], [-1, 0, 1], format="csr"))


def problem(cal, fmt, n):
    H = lap3d_v(cal, 17) if fmt == "split" else tridiag(n, 11 + n)
    assert H.shape[0] == n
    rng = np.random.RandomState(n)
    psi = rng.randn(n)
    return H, psi / np.linalg.norm(psi), [rng.randn(n), 10.0 * rng.rand(n)], rng.randn(2)


def open_real(cal, fmt, H, psi0, s=4, blocks=2):
    c = cal.Context(spmv_format=fmt)
    try:
        P = cal.Propagator(H, psi0, s, blocks, ctx=c, real=True)
    except Exception:
        c.close()
        raise
    assert c.spmv_split_info()[0] == (fmt == "split")
    return c, P


def one_step(P, W, f, nk, tau=0.01):
    if nk:
        P.set_drive(W[:nk])
        return P.step(tau, 1, drive=[f[:nk]])
    return P.step(tau, 1)


@pytest.mark.parametrize("nk", [0, 2])
@pytest.mark.parametrize("fmt,n", [("csr", 17), ("csr", 255), ("csr", 256), ("csr", 257), ("csr", 1025),
                                   ("split", 4913)])
def test_real_density_bits(cal, fmt, n, nk):
    H, psi0, W, f = problem(cal, fmt, n)
    V0 = H.diagonal()
    c, P = open_real(cal, fmt, H, psi0)
    try:
        P.set_nonlinear(G, "frozen")
        assert one_step(P, W, f, nk) == 0
        expect = nref.density_chain(V0, W[:nk], f[:nk], G, psi0)
        assert np.array_equal(c.get_diagonal(), expect)
        assert not np.array_equal(expect, V0)
        rows = P.nonlinear()
        S, bar = nref.quartic(psi0)
        assert rows.shape == (1, 2) and rows[0, 0] == 0.0 and abs(rows[0, 1] - S) <= bar
        star = P.state()
        assert not np.any(star.imag) and abs(np.linalg.norm(star) - 1.0) <= 1e-10
        P.close()
        assert np.array_equal(c.get_diagonal(), V0)
        P = cal.Propagator(H, psi0, 4, 2, ctx=c, real=True)
        P.set_nonlinear(G, "midpoint")
        assert one_step(P, W, f, nk) == 0
        expect = nref.density_chain(V0, W[:nk], f[:nk], 0.5 * G, psi0, 0.5 * G, star.real)
        assert np.array_equal(c.get_diagonal(), expect)
        rows = P.nonlinear()
        assert rows.shape == (1, 2) and abs(rows[0, 1] - S) <= bar
        assert P.info()["steps"] == 1 and not np.array_equal(P.state(), star)
        P.close()
    finally:
        c.close()


# ---- 3. stacked imaginary time leaves the kernel alone -------------------------------------------------------
def test_stacked_imaginary_step_is_the_existing_combine(cal):
    N, s, blocks, tau = 257, 6, 4, 0.05
    H, psi0, x, _, _ = iref.oscillator(N)
    psi0 = psi0 * np.exp(0.7j * x)
    c = cal.Context(spmv_format="csr")
    try:
        T, Q, k = cal.ca_lanczos_prop(H, psi0, s, blocks, tau, basis="newton", ctx=c)
        assert k == s * blocks
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=c)
        P.set_imaginary_time(True)
        assert P.step(tau, 1) == 0
        en = P.energetics()
        a = iref.imag_coefficients(cal.expm_real_col1(T, tau), en["norm2"][0])
        top, bot = pref.combine_ref(np.vstack([Q.real, Q.imag]), a + 0j)
        got = P.state()
        assert np.array_equal(got.real, top) and np.array_equal(got.imag, bot)
        rr = 0.0
        for t in T[1:, 0]:
            rr = rr + t * t
        assert en["mu"][0] == T[0, 0] and en["residual"][0] == np.sqrt(rr)
        assert abs(P.info()["norm"] ** 2 - en["norm2"][0]) <= 1e-10
        P.close()
        # back to real time: the bits of a propagator that never left it
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=c)
        assert P.step(0.025, 2) == 0
        want = P.state()
        P.close()
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=c)
        P.set_imaginary_time(True)
        P.set_imaginary_time(False)
        assert P.step(0.025, 2) == 0
        assert np.array_equal(P.state(), want)
        P.close()
    finally:
        c.close()


# ---- 4. accuracy against the dense scheme -------------------------------------------------------------------
STEPS, TAU = 8, 0.025
ACC = [(g, d) for g in (1.0, -0.5) for d in ("frozen", "midpoint")] + [(0.0, "frozen")]


def start(N, stacked):
    H, psi0, x, _, _ = iref.oscillator(N)
    return H, (psi0 * np.exp(0.7j * x) if stacked else psi0)


@pytest.mark.parametrize("stacked", [True, False])
@pytest.mark.parametrize("g,density", ACC)
@pytest.mark.parametrize("s,blocks", [(6, 4), (4, 6)])
@pytest.mark.parametrize("N", [256, 255])
def test_imaginary_time_oscillator(cal, N, s, blocks, g, density, stacked):
    builds = STEPS * (2 if density == "midpoint" else 1)
    bar = builds * 1e-10
    H, psi0 = start(N, stacked)
    rows = np.zeros((STEPS, 0))
    exact = iref.dense_imag(H, [], psi0, rows, TAU, g, density)
    n2 = float(np.vdot(psi0, psi0).real)
    c = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=c, real=not stacked)
        if stacked:
            P.set_imaginary_time(True)
        if g != 0.0:
            P.set_nonlinear(g, density)
        assert P.step(TAU, STEPS) == 0
        psi, info, en = P.state(), P.info(), P.energetics()
        P.close()
    finally:
        c.close()
    err, drift = np.linalg.norm(psi - exact), abs(info["norm"] ** 2 - n2)
    psi_or = iref.oracle_imag(H, [], psi0, rows, TAU, g, density, s, blocks, "newton", stacked)
    e_or, d_or = np.linalg.norm(psi_or - exact), abs(float(np.vdot(psi_or, psi_or).real) - n2)
    print("N=%d s=%d blocks=%d g=%g %s stacked=%s: err %.3e |norm2 - N| %.3e, oracle err %.3e %.3e"
          % (N, s, blocks, g, density, stacked, err, drift, e_or, d_or))
    assert e_or <= bar and d_or <= bar, (e_or, d_or)
    assert err <= bar, err
    assert drift <= bar, drift
    assert info["steps"] == STEPS and info["breakdowns"] == 0 and abs(P.t - STEPS * TAU) < 1e-15
    assert len(en["t"]) == STEPS and np.allclose(en["t"], TAU * np.arange(STEPS), rtol=0, atol=1e-15)
    if not stacked:
        assert not np.any(psi.imag)


# ---- 5. energetics ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,g,density", [("imag-real", 0.0, "frozen"), ("imag-real", 1.0, "frozen"),
                                            ("imag-real", 1.0, "midpoint"), ("imag-stacked", 1.0, "frozen"),
                                            ("imag-stacked", 1.0, "midpoint"), ("real-stacked", 0.0, "frozen"),
                                            ("real-stacked", 1.0, "frozen"), ("real-stacked", 1.0, "midpoint")])
def test_energetics_rows(cal, mode, g, density):
    N, s, blocks = 256, 6, 4
    stacked = mode != "imag-real"
    H, psi0 = start(N, stacked)
    c = cal.Context(spmv_format="csr")
    states = []
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=c, real=not stacked)
        if mode == "imag-stacked":
            P.set_imaginary_time(True)
        if g != 0.0:
            P.set_nonlinear(g, density)
        for _ in range(STEPS):
            states.append(P.state())
            assert P.step(TAU, 1) == 0
        en = P.energetics()
        quart = P.nonlinear()[:, 1] if g != 0.0 else np.zeros(STEPS)
        P.close()
    finally:
        c.close()
    assert all(len(en[k]) == STEPS for k in ("t", "norm2", "mu", "energy", "residual"))
    worst = 0.0
    for j, p in enumerate(states):
        mu, E, res, _ = iref.energetics(H, p, g)
        mu_or, res_or = iref.oracle_first_column(H, p, g, s, blocks, "newton", stacked)
        n2 = float(np.vdot(p, p).real)
        S, qbar = nref.quartic(p)
        ebar = n2 * MU_BAR + 0.5 * abs(g) * qbar + (N + 8) * EPS * n2 * abs(mu)  # N_n itself is a rounded sum
        d = (abs(en["mu"][j] - mu), abs(en["residual"][j] - res), abs(en["energy"][j] - E))
        worst = max(worst, d[0])
        print("%s g=%g %s step %d: mu %.12f |dmu| %.2e (oracle %.2e) |dres| %.2e (oracle %.2e) |dE| %.2e (bar %.2e)"
              % (mode, g, density, j, mu, d[0], abs(mu_or - mu), d[1], abs(res_or - res), d[2], ebar))
        assert abs(mu_or - mu) <= MU_BAR and abs(res_or - res) <= MU_BAR
        assert d[0] <= MU_BAR and d[1] <= MU_BAR and d[2] <= ebar, d
        assert abs(en["norm2"][j] - n2) <= (N + 8) * EPS * n2
        assert en["energy"][j] == en["norm2"][j] * en["mu"][j] - (0.5 * g * quart[j] if g != 0.0 else 0.0)
    if mode == "real-stacked" and g == 1.0 and density == "midpoint":
        # the conserved energy: the device's drift is the dense scheme's own plus the rounding bar
        dense = [psi0] + nref.dense_nonlinear(H, [], psi0, np.zeros((STEPS, 0)), TAU, g, density, history=True)[0]
        Ed = np.array([iref.energetics(H, p, g)[1] for p in dense[:STEPS]])
        dd, dv = np.max(np.abs(Ed - Ed[0])), np.max(np.abs(en["energy"] - en["energy"][0]))
        print("E_GP drift over %d steps: device %.3e, dense scheme %.3e" % (STEPS, dv, dd))
        assert dv <= dd + ebar


# ---- 6. the driver ---------------------------------------------------------------------------------------------
def dense_steps(H, psi0, g, tol, tau):
    """The dense scheme stepped as ground_state steps: (steps taken, the last judged mu and energy)."""
    psi, k = psi0, 0
    while k < 400:
        mu, E, res, _ = iref.energetics(H, psi, g)
        psi = iref.dense_imag(H, [], psi, np.zeros((1, 0)), tau, g, "frozen")
        k += 1
        if res <= tol * max(1.0, abs(mu)):
            break
    return k, mu, E


def test_ground_state_linear(cal):
    N, tau, tol = 256, 0.2, 1e-10
    H, psi0, x, ew, U = iref.oscillator(N)
    out = {}
    for real in (True, False):
        p0 = psi0 if real else psi0 * np.exp(0.7j * x)
        kd, _, _ = dense_steps(H, p0, 0.0, tol, tau)
        r = cal.ground_state(H, p0, tau, 6, 4, tol=tol, real=real, ctx=None)
        overlap = abs(np.vdot(U[:, 0], r["psi"])) / np.linalg.norm(p0)
        print("real=%s: %d steps (dense %d), mu - ew0 %.3e, 1 - overlap %.3e, residual %.3e"
              % (real, r["steps"], kd, r["mu"] - ew[0], 1 - overlap, r["residual"]))
        assert kd <= 395 and r["converged"] and r["steps"] <= kd + 5
        assert abs(r["mu"] - ew[0]) <= 1e-10 and 1.0 - overlap <= 1e-12
        assert len(r["history"]["mu"]) == r["steps"] and r["energy"] == r["history"]["energy"][-1]
        assert (r["psi"].dtype == np.float64) == real
        out[real] = r
    n2 = float(psi0 @ psi0)
    print("mu real - mu stacked %.3e (bar %.2e)" % (out[True]["mu"] - out[False]["mu"], MU_BAR))
    assert abs(out[True]["mu"] - out[False]["mu"]) <= MU_BAR
    assert abs(out[True]["energy"] - out[False]["energy"]) <= 2 * n2 * MU_BAR + 4 * (N + 8) * EPS * n2 * abs(ew[0])


def test_ground_state_gp(cal):
    """g = 1, tol = 1e-8 against the dense scheme run to the same tolerance.
    Both end states have an eigen-residual below r = tol max(1, |mu|); the gap
    of the oscillator is 1, so each is within about r of the fixed point, and
    mu moves by at most (1 + 2 g max|psi|^2) <= 3 times that (max|psi|^2 < 1):
    two states, 10 r with room for the second order."""
    N, tau, tol, g = 256, 0.2, 1e-8, 1.0
    H, psi0, _, _, _ = iref.oscillator(N)
    kd, mud, Ed = dense_steps(H, psi0, g, tol, tau)
    for real in (True, False):
        c = cal.Context(spmv_format="csr")  # the nonlinear term rewrites a stored diagonal
        try:
            r = cal.ground_state(H, psi0, tau, 6, 4, g=g, density="frozen", tol=tol, real=real, ctx=c)
        finally:
            c.close()
        print("g=1 real=%s: %d steps (dense %d), mu %.12f (dense %.12f), E %.12f (dense %.12f)"
              % (real, r["steps"], kd, r["mu"], mud, r["energy"], Ed))
        bar = 10 * tol * max(1.0, abs(mud))
        assert r["converged"] and r["steps"] <= kd + 5
        assert abs(r["mu"] - mud) <= bar and abs(r["energy"] - Ed) <= bar * float(psi0 @ psi0)
        assert abs(np.linalg.norm(r["psi"]) - np.linalg.norm(psi0)) <= 1e-10


def test_ground_state_hermitian_shared(cal):
    """A complex Hermitian H (Peierls phases) on the stored-once format, against eigh."""
    d = 12
    r2 = np.add.outer((np.arange(d) - 5.5) ** 2, (np.arange(d) - 5.5) ** 2).ravel()
    H = cal.matrices.peierls_hamiltonian((d, d), 0.5 * 0.36 * r2, 0.08)
    assert np.iscomplexobj(H)
    ew, U = np.linalg.eigh(H.toarray())
    rng = np.random.RandomState(5)
    psi0 = rng.randn(d * d) + 1j * rng.randn(d * d)
    psi0 /= np.linalg.norm(psi0)
    c = cal.Context(spmv_format="shared")
    try:
        r = cal.ground_state(H, psi0, 0.5, 6, 4, tol=1e-10, ctx=c)
        assert c.spmv_hermitian_info()[0]
    finally:
        c.close()
    overlap = abs(np.vdot(U[:, 0], r["psi"]))
    print("hermitian shared: %d steps, mu - ew0 %.3e, 1 - overlap %.3e" % (r["steps"], r["mu"] - ew[0], 1 - overlap))
    assert r["converged"] and r["steps"] <= 400
    assert abs(r["mu"] - ew[0]) <= 1e-10 and 1.0 - overlap <= 1e-12


# ---- 7. refusals and bookkeeping ----------------------------------------------------------------------------------
def test_real_path_refusals(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, CAL_ERR_UNSUPPORTED, lib, ptr
    N = 64
    H, psi0, x, _, _ = iref.oscillator(N)
    with pytest.raises(ValueError):
        cal.Propagator(H, psi0 + 0j, 4, 2, real=True)
    with pytest.raises(ValueError):
        cal.Propagator(H.astype(complex), psi0, 4, 2, real=True)
    # a stacked matrix, and a "shared" one
    for fmt in ("csr", "shared"):
        c = cal.Context(spmv_format=fmt)
        try:
            c.set_matrix_stacked(H)
            st = lib.cal_prop_begin_real(c.h, N, ptr(psi0), 4, 2, b"newton", None, 0)
            msg = lib.cal_last_error(c.h).decode()
            assert st == CAL_ERR_UNSUPPORTED and "stacked propagator" in msg, (fmt, st, msg)
            assert lib.cal_prop_get(c.h, None, None, None) == CAL_ERR_ARG  # nothing was opened
            if fmt == "shared":
                with pytest.raises(cal.CalError):  # the format takes no H alone
                    cal.Propagator(H, psi0, 4, 2, ctx=c, real=True)
        finally:
            c.close()
    c = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, 4, 2, ctx=c, real=True)
        assert P.step(0.05, 2) == 0
        before, rows = P.state(), P.energetics()
        for call in (lambda: P.set_observables(phi=[psi0 + 0j]), lambda: P.set_absorber(np.ones(N)),
                     lambda: P.set_imaginary_time(False)):
            with pytest.raises(cal.CalError) as e:
                call()
            assert e.value.status == CAL_ERR_UNSUPPORTED and "stacked propagator" in str(e.value)
        for tau in (float("nan"), float("inf")):
            with pytest.raises(cal.CalError) as e:
                P.step(tau, 1)
            assert e.value.status == CAL_ERR_ARG
        assert np.array_equal(P.state(), before) and len(P.energetics()["t"]) == len(rows["t"]) == 2
        P.set_imaginary_time(True)  # a no-op
        # W and the energy are taken
        P.set_observables(W=[x * x], energy=True)
        assert P.step(0.05, 1) == 0
        ob, psi = P.observables(), P.state()
        assert not np.any(psi.imag)
        pref.check_row(np.concatenate([[ob["t"][0], ob["norm2"][0], ob["energy"][0]], ob["W"][0]]), H, psi,
                       (x * x).reshape(N, 1), np.zeros((N, 0)))
        P.close()
    finally:
        c.close()


def test_energetics_bookkeeping(cal):
    N = 128
    H, psi0, x, _, _ = iref.oscillator(N)
    c = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0 * np.exp(0.3j * x), 4, 3, ctx=c)
        assert len(P.energetics()["t"]) == 0
        P.set_drive([x])
        P.set_nonlinear(0.5, "midpoint")
        assert P.step(0.02, 3, drive=lambda t: [0.1 * np.sin(t)], scheme="cf4") == 0
        en = P.energetics()
        assert len(en["t"]) == 6 and P.info()["steps"] == 6  # one row per sub-step, one per "midpoint" step
        assert np.allclose(en["t"], 0.01 * np.arange(6), rtol=0, atol=1e-15)
        part = P.energetics(2, 3)
        for k in en:
            assert np.array_equal(part[k], en[k][2:5])
        assert len(P.energetics(6, 0)["t"]) == 0
        with pytest.raises(cal.CalError):
            P.energetics(4, 3)
        with pytest.raises(cal.CalError):
            P.energetics(-1, 1)
        P.close()
    finally:
        c.close()
