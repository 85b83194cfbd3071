"""The nonlinear term g |psi|^2 on the device: cal_prop_set_nonlinear,
cal_prop_get_nonlinear (kernel k_diag_density, prop.hip).

Bars:
  * the diagonal a nonlinear step writes is the NumPy chain of
    tests/nonlinear_ref.py density_chain to the bit (array_equal), on "csr",
    "split" and "shared", for one state ("frozen") and for two ("midpoint",
    whose predictor is the frozen step to the bit); the history's sum |psi|^4
    within the derived rounding bar (N + 8) eps S of tests/prop_obs_ref.py.
  * propagation: 2-norm error against the same scheme with dense eigh
    exponentials at most builds * 1e-10 (8 steps: 8 builds "frozen", 16
    "midpoint"), and the same for the absolute norm drift -- the bars of
    tests/test_gpu_drive.py, for the same reason.  The CPU oracle variant is
    held to the same bar next to the device.
  * the refusals of cal_prop_set_drive apply; the case "several ranks" cannot be
    reached here: cal_prop_begin itself refuses a context of several ranks, so
    no propagator is ever open on one.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import absorber_ref as aref  # noqa: E402
import drive_ref as dref  # noqa: E402
import nonlinear_ref as nref  # noqa: E402
from split_cases import drop_diagonal, hamiltonian_2d, lap3d_v  # noqa: E402

pref = nref.pref
EPS = pref.EPS
pytestmark = pytest.mark.gpu
G = 0.75


# ---- problems -----------------------------------------------------------------------------
def canon(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    return A


def tridiag(n, seed):
    """Random symmetric tridiagonal, every diagonal entry stored."""
    rng = np.random.RandomState(seed)
    e = rng.randn(n - 1)
    return canon(sp.diags([e, rng.randn(n) + 3.0, e], [-1, 0, 1], format="csr"))


def rand_state(n, seed):
    rng = np.random.RandomState(seed)
    psi = rng.randn(n) + 1j * rng.randn(n)
    return psi / np.linalg.norm(psi)


def problem(cal, fmt, n):
    """(H, psi0, W (two columns), f (two amplitudes)) of the bit tests; "split"
    takes the grid Hamiltonians of tests/split_cases.py, named by n."""
    if fmt == "split":
        H = lap3d_v(cal, 17) if n == 4913 else hamiltonian_2d(cal, 257)
        assert H.shape[0] == n
    else:
        H = tridiag(n, 11 + n)
    rng = np.random.RandomState(n)
    return H, rand_state(n, 2 * n + 1), [rng.randn(n), 10.0 * rng.rand(n)], rng.randn(2)


BIT_CASES = [(fmt, n) for fmt in ("csr", "shared") for n in (16, 17, 255, 256, 257, 513, 1025)] + \
    [("split", 4913), ("split", 66049)]


def open_prop(cal, fmt, H, psi0, s=4, blocks=2, basis="newton"):
    ctx = cal.Context(spmv_format=fmt)
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis=basis, ctx=ctx)
    except Exception:
        ctx.close()
        raise
    assert ctx.spmv_split_info()[0] == (fmt == "split")
    assert ctx.spmv_shared_info()[0] == (fmt == "shared")
    return ctx, P


def one_step(P, W, f, nk, dt=0.01):
    if nk:
        P.set_drive(W[:nk])
        return P.step(dt, 1, drive=[f[:nk]])
    return P.step(dt, 1)


# ---- 1. the kernel's bits, "frozen" ------------------------------------------------------------
@pytest.mark.parametrize("nk", [0, 2])
@pytest.mark.parametrize("fmt,n", BIT_CASES)
def test_frozen_diagonal_bits(cal, fmt, n, nk):
    H, psi0, W, f = problem(cal, fmt, n)
    V0 = H.diagonal()
    expect = nref.density_chain(V0, W[:nk], f[:nk], G, psi0)
    assert not np.array_equal(expect, dref.chain(V0, W[:nk], f[:nk]))  # the density is in it
    ctx, P = open_prop(cal, fmt, H, psi0)
    try:
        P.set_nonlinear(G, "frozen")
        assert P.nonlinear().shape == (0, 2)
        assert one_step(P, W, f, nk) == 0
        assert np.array_equal(ctx.get_diagonal(), np.tile(expect, 2))
        rows = P.nonlinear()
        S, bar = nref.quartic(psi0)
        print("%s n=%d nk=%d: sum|psi|^4 %.15e (NumPy %.15e, bar %.2e)" % (fmt, n, nk, rows[0, 1], S, bar))
        assert rows.shape == (1, 2) and rows[0, 0] == 0.0
        assert abs(rows[0, 1] - S) <= bar
        assert P.info()["steps"] == 1
        P.close()
        assert np.array_equal(ctx.get_diagonal(), np.tile(V0, 2))
    finally:
        ctx.close()


# ---- 2. the predictor is the frozen step, and "midpoint"'s bits -----------------------------------
@pytest.mark.parametrize("nk", [0, 2])
@pytest.mark.parametrize("fmt,n", [(fmt, n) for fmt in ("csr", "shared") for n in (17, 256, 1025)] + [("split", 4913)])
def test_midpoint_diagonal_bits(cal, fmt, n, nk):
    H, psi0, W, f = problem(cal, fmt, n)
    V0 = H.diagonal()
    ctx, P = open_prop(cal, fmt, H, psi0)
    try:
        P.set_nonlinear(G, "frozen")
        assert one_step(P, W, f, nk) == 0
        star = P.state()
        P.close()
        P = cal.Propagator(H, psi0, 4, 2, ctx=ctx)
        P.set_nonlinear(G, "midpoint")
        assert one_step(P, W, f, nk) == 0
        expect = nref.density_chain(V0, W[:nk], f[:nk], 0.5 * G, psi0, 0.5 * G, star)
        assert np.array_equal(ctx.get_diagonal(), np.tile(expect, 2))
        assert not np.array_equal(expect, nref.density_chain(V0, W[:nk], f[:nk], G, psi0))
        rows = P.nonlinear()
        S, bar = nref.quartic(psi0)
        assert rows.shape == (1, 2) and rows[0, 0] == 0.0 and abs(rows[0, 1] - S) <= bar
        assert P.info()["steps"] == 1 and not np.array_equal(P.state(), star)
        P.close()
    finally:
        ctx.close()


def test_formats_agree(cal):
    """lap3d_v(17), driven, "midpoint", 3 steps: "split" (whose streamed diagonal
    the kernel writes too) and "shared" (one written half) give the bits of "csr"."""
    H, psi0, W, f = problem(cal, "split", 4913)
    out = {}
    for fmt in ("csr", "split", "shared"):
        ctx, P = open_prop(cal, fmt, H, psi0, 4, 3)
        try:
            P.set_drive(W[:1])
            P.set_nonlinear(G, "midpoint")
            assert P.step(0.02, 3, drive=np.array([[0.3], [-0.2], [0.1]])) == 0
            out[fmt] = (P.state(), P.info()["norm"], P.nonlinear(), ctx.get_diagonal())
            P.close()
        finally:
            ctx.close()
    for fmt in ("split", "shared"):
        for a, b in zip(out["csr"], out[fmt]):
            assert np.array_equal(a, b), fmt
    assert out["csr"][2].shape == (3, 2)


# ---- 3. accuracy against the same scheme done densely -------------------------------------------------
STEPS, DT = 8, 0.025


def _rows(driven):
    return np.array([dref.f_one((j + 0.5) * DT) for j in range(STEPS)]) if driven else np.zeros((STEPS, 0))


@functools.lru_cache(maxsize=None)
def oscillator_reference(N, g, density, driven):
    H, psi0, x, _, _ = nref.oscillator(N)
    return nref.dense_nonlinear(H, [x] if driven else [], psi0, _rows(driven), DT, g, density)


@pytest.mark.parametrize("driven", [False, True])
@pytest.mark.parametrize("density", ["frozen", "midpoint"])
@pytest.mark.parametrize("g", [1.0, -0.5])
@pytest.mark.parametrize("s,blocks", [(6, 4), (4, 6)])
@pytest.mark.parametrize("N", [256, 255])
def test_nonlinear_oscillator(cal, N, s, blocks, g, density, driven):
    builds = STEPS * (2 if density == "midpoint" else 1)
    bar = builds * 1e-10
    H, psi0, x, _, _ = nref.oscillator(N)
    W, rows = ([x] if driven else []), _rows(driven)
    exact = oscillator_reference(N, g, density, driven)
    n0 = np.linalg.norm(psi0)
    ctx = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=ctx)
        if driven:
            P.set_drive(W)
        P.set_nonlinear(g, density)
        drift = 0.0
        for j in range(STEPS):
            assert (P.step(DT, 1, drive=rows[j:j + 1]) if driven else P.step(DT, 1)) == 0
            drift = max(drift, abs(P.info()["norm"] - n0))
        psi, info, hist = P.state(), P.info(), P.nonlinear()
        P.close()
    finally:
        ctx.close()
    err = np.linalg.norm(psi - exact)
    psi_or, drift_or = nref.oracle_nonlinear(H, W, psi0, rows, DT, g, density, s, blocks, "newton")
    e_or = np.linalg.norm(psi_or - exact)
    print("N=%d s=%d blocks=%d g=%g %s driven=%s: err %.3e drift %.3e, oracle err %.3e drift %.3e, residual_max %.3e"
          % (N, s, blocks, g, density, driven, err, drift, e_or, drift_or, info["residual_max"]))
    assert e_or <= bar and drift_or <= bar, (e_or, drift_or)
    assert err <= bar, err
    assert drift <= bar, drift
    assert info["steps"] == STEPS and info["breakdowns"] == 0 and abs(P.t - STEPS * DT) < 1e-15
    assert hist.shape == (STEPS, 2)
    assert np.allclose(hist[:, 0], DT * np.arange(STEPS), rtol=0, atol=1e-15)
    assert hist[0, 1] == pytest.approx(nref.quartic(psi0)[0], abs=nref.quartic(psi0)[1])


def test_nonlinear_packet_2d(cal):
    """laplacian_2d(40) with the complex packet of drive_ref.packet_2d, g = 0.5,
    "midpoint", 4 steps of dt = 0.5 on "csr": 8 builds, bar 8e-10.  The scheme's
    own CPU variants (NumPy Lanczos, the CPU oracle with s = 6, 4 blocks) are
    inside that bar against the dense exponentials at dt = 0.5, so the step
    size is kept."""
    H, psi0, _, _ = dref.packet_2d()
    steps, dt, s, blocks, g = 4, 0.5, 6, 4, 0.5
    bar = 2 * steps * 1e-10
    rows = np.zeros((steps, 0))
    exact = nref.dense_nonlinear(H, [], psi0, rows, dt, g, "midpoint")
    ctx = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=ctx)
        P.set_nonlinear(g)  # the default density is "midpoint"
        assert P.step(dt, steps) == 0
        psi, info = P.state(), P.info()
        P.close()
    finally:
        ctx.close()
    n0 = np.linalg.norm(psi0)
    err, drift = np.linalg.norm(psi - exact), abs(info["norm"] - n0)
    psi_or, drift_or = nref.oracle_nonlinear(H, [], psi0, rows, dt, g, "midpoint", s, blocks, "newton")
    e_or = np.linalg.norm(psi_or - exact)
    print("packet midpoint: err %.3e drift %.3e, oracle err %.3e drift %.3e" % (err, drift, e_or, drift_or))
    assert e_or <= bar and drift_or <= bar, (e_or, drift_or)
    assert err <= bar and drift <= bar, (err, drift)
    assert info["steps"] == steps
    # the term matters here: the linear state is far away
    lin = dref.dense_driven(H, [], psi0, rows, dt)
    assert np.linalg.norm(lin - exact) > 1e-3


# ---- 4. nothing changes when nothing is set -------------------------------------------------------------
def test_zero_g_is_a_no_op(cal):
    H, psi0, _, _, _ = nref.oscillator(256)
    out = []
    for call in (True, False):
        ctx = cal.Context(spmv_format="csr")
        try:
            P = cal.Propagator(H, psi0, 6, 4, ctx=ctx)
            if call:
                P.set_nonlinear(0.0)
                P.set_nonlinear(0.0, "frozen")
            assert P.step(DT, 8) == 0
            info = P.info()
            info.pop("ms")  # wall time
            out.append((P.state(), info, P.nonlinear(), ctx.get_diagonal()))
            P.close()
        finally:
            ctx.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
    assert a[1].keys() == b[1].keys()
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k
    assert a[2].shape == (0, 2) and b[2].shape == (0, 2)


# ---- 5. ownership of the diagonal ---------------------------------------------------------------------------
@pytest.mark.parametrize("density", ["frozen", "midpoint"])
@pytest.mark.parametrize("fmt", ["csr", "split", "shared"])
def test_diagonal_ownership(cal, fmt, density):
    n = 4913 if fmt == "split" else 257
    H, psi0, W, f = problem(cal, fmt, n)
    V0 = np.tile(H.diagonal(), 2)
    ctx, P = open_prop(cal, fmt, H, psi0)
    try:
        assert np.array_equal(ctx.get_diagonal(), V0)
        P.set_nonlinear(G, density)
        assert P.step(0.01, 1) == 0
        assert not np.array_equal(ctx.get_diagonal(), V0)
        P.set_drive(W)  # must not take V0 + g rho for H0's diagonal
        assert P.step(0.01, 1, drive=[f]) == 0
        P.set_drive(None)
        assert P.step(0.01, 1) == 0
        # without the drive the step wrote V0 + g rho alone
        assert P.nonlinear().shape == (3, 2)
        P.set_nonlinear(0.0)
        assert np.array_equal(ctx.get_diagonal(), V0)
        # the other order: the drive first, the term goes off while the drive stays
        P.set_drive(W)
        P.set_nonlinear(-G, density)
        assert P.step(0.01, 1, drive=[f]) == 0
        P.set_nonlinear(0.0)  # whatever H the last driven step left
        assert np.array_equal(ctx.get_diagonal(), np.tile(dref.chain(H.diagonal(), W, f), 2))
        P.set_drive(None)
        assert np.array_equal(ctx.get_diagonal(), V0)
        # and close() with both on
        P.set_nonlinear(G, density)
        assert P.step(0.01, 1) == 0
        P.set_drive(W)
        assert P.step(0.01, 1, drive=[f]) == 0
        P.close()
        assert np.array_equal(ctx.get_diagonal(), V0)
        # a new propagator starts without the term
        P = cal.Propagator(H, psi0, 4, 2, ctx=ctx)
        assert P.step(0.01, 1) == 0 and P.nonlinear().shape == (0, 2)
        assert np.array_equal(ctx.get_diagonal(), V0)
        P.close()
    finally:
        ctx.close()


def test_undriven_step_uses_the_last_amplitudes(cal):
    """cal_prop_step while a drive is set: the linear part is that of the most
    recent driven step, zeros before the first."""
    H, psi0, W, f = problem(cal, "csr", 257)
    V0 = H.diagonal()
    ctx, P = open_prop(cal, "csr", H, psi0)
    try:
        P.set_drive(W)
        P.set_nonlinear(G, "frozen")
        assert P.step(0.01, 1) == 0
        assert np.array_equal(ctx.get_diagonal(), np.tile(nref.density_chain(V0, W, [0.0, 0.0], G, psi0), 2))
        assert P.step(0.01, 1, drive=[f]) == 0
        psi = P.state()
        assert P.step(0.01, 1) == 0
        assert np.array_equal(ctx.get_diagonal(), np.tile(nref.density_chain(V0, W, f, G, psi), 2))
        P.close()
    finally:
        ctx.close()


# ---- 6. one row per step under "midpoint" ---------------------------------------------------------------------
def test_midpoint_records_one_row_per_step(cal):
    N, steps, g = 256, 5, 1.0
    H, psi0, x, ew, _ = nref.oscillator(N)
    M = aref.oscillator_mask(x)
    W, phi = [x, x * x], [psi0]
    rows = np.zeros((steps, 0))
    states, extras = nref.dense_nonlinear(H, [], psi0, rows, DT, g, "midpoint", mask=M, history=True)
    ctx = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, 6, 4, ctx=ctx)
        P.set_observables(W=W, phi=phi, energy=True)
        P.set_absorber(M)
        P.set_nonlinear(g, "midpoint")
        assert P.step(DT, steps) == 0
        o, ab, nl, info = P.observables(), P.absorbed(), P.nonlinear(), P.info()
        P.close()
    finally:
        ctx.close()
    assert o["t"].shape == (steps,) and ab["t"].shape == (steps,) and nl.shape == (steps, 2)
    assert info["steps"] == steps
    assert np.all(np.abs(o["t"] - DT * np.arange(1, steps + 1)) <= 8 * EPS * DT * steps)
    assert np.array_equal(ab["t"], o["t"])
    assert np.all(np.abs(nl[:, 0] - DT * np.arange(steps)) <= 8 * EPS * DT * steps)
    n0 = np.linalg.norm(psi0)
    Wm = np.column_stack(W)
    before = [np.asarray(psi0, dtype=complex)] + states[:-1]
    for j in range(steps):
        k = 2 * (j + 1)  # builds so far: the state is within k 1e-10 of the dense scheme's
        e = k * 1e-10
        psi = states[j]
        wv, wbar = pref.w_ref(Wm, psi)
        ov, bre, bim = pref.overlap_ref(np.column_stack(phi), psi)
        # a state within e (2-norm): the first-order bars of tests/prop_obs_ref.py physics_bars
        for q in range(2):
            assert abs(o["W"][j, q] - wv[q]) <= wbar[q] + 2 * np.max(np.abs(Wm[:, q])) * n0 * e, (j, q)
        assert abs(o["overlap"][j, 0].real - ov[0].real) <= bre[0] + np.linalg.norm(psi0) * e
        assert abs(o["overlap"][j, 0].imag - ov[0].imag) <= bim[0] + np.linalg.norm(psi0) * e
        # the energy is <psi'|H|psi'> with the H stored in the matrix: H0 + g (rho_n + rho*)/2
        Hs = H + sp.diags(extras[j])
        E, ebar = pref.energy_ref(Hs, psi)
        # (||H|| <= max|ew| + max|extra|; the stored density itself moves by at most |g| 2 max|psi| e)
        hn = np.max(np.abs(ew)) + np.max(np.abs(extras[j]))
        dh = abs(g) * 2 * np.max(np.abs(before[j])) * e
        assert abs(o["energy"][j] - E) <= ebar + 2 * hn * n0 * e + dh * n0 * n0, (j, o["energy"][j], E)
        n2, n2bar = aref.norm2_ref(psi.real, psi.imag)
        assert abs(o["norm2"][j] - n2) <= n2bar + 2 * n0 * e
        S, sbar = nref.quartic(before[j])
        # |psi|^4 of a state within e_prev: d(sum rho^2) <= 4 max(rho) ||psi|| e_prev
        e_prev = 2 * j * 1e-10
        assert abs(nl[j, 1] - S) <= sbar + 4 * np.max(np.abs(before[j]) ** 2) * n0 * e_prev, (j, nl[j, 1], S)
    assert ab["absorbed"].shape == (steps,) and np.all(ab["absorbed"] >= 0.0)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def _refused_unsupported(cal, fmt, H, word):
    from ca_lanczos_amd._lib import CAL_ERR_UNSUPPORTED, lib
    n = H.shape[0]
    x = np.random.RandomState(3).randn(2 * n)
    ctx = cal.Context(spmv_format=fmt)
    try:
        ctx.set_matrix_stacked(H)
        y0 = ctx.spmv(x)
        P = cal.Propagator(H, rand_state(n, 5), 4, 2, ctx=ctx)
        assert ctx.spmv_format()[0] == ("pattern" if fmt == "pattern" else "csr")
        for density in (b"frozen", b"midpoint"):
            assert lib.cal_prop_set_nonlinear(ctx.h, 1.0, density) == CAL_ERR_UNSUPPORTED
            msg = lib.cal_last_error(ctx.h).decode()
            assert word in msg, msg
        assert P.nonlinear().shape == (0, 2)
        assert P.step(0.01, 1) == 0  # the propagator goes on, linear
        P.close()
        assert np.array_equal(ctx.spmv(x), y0)
    finally:
        ctx.close()


def test_refuses_pattern_format(cal):
    _refused_unsupported(cal, "pattern", cal.matrices.laplacian_3d(20), "cal_set_spmv_format")


def test_refuses_missing_diagonal(cal):
    _refused_unsupported(cal, "csr", drop_diagonal(lap3d_v(cal, 17), [0, 2456, 4912]),
                         "6 row(s) store no diagonal entry")


def test_refuses_duplicate_diagonal(cal):
    """Two stored entries with col == row in one row (raw arrays: SciPy would sum them)."""
    from ca_lanczos_amd._lib import CAL_ERR_UNSUPPORTED, check, lib, ptr
    rowptr = np.array([0, 2, 5, 7], dtype=np.int64)
    col = np.array([0, 1, 0, 1, 1, 1, 2], dtype=np.int32)
    val = np.array([2.0, -1.0, -1.0, 1.5, 0.5, -1.0, 2.0])
    re, im = np.array([1.0, 0.5, -0.25]), np.array([0.0, 0.25, 0.5])
    x = np.random.RandomState(1).randn(6)
    ctx = cal.Context(spmv_format="csr")
    try:
        check(ctx.h, lib.cal_set_matrix_csr_stacked(ctx.h, 3, rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                    col.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ptr(val)))
        y0 = ctx.spmv(x)
        check(ctx.h, lib.cal_prop_begin(ctx.h, 3, ptr(re), ptr(im), 1, 2, b"monomial", None, 0))
        assert lib.cal_prop_set_nonlinear(ctx.h, 1.0, b"midpoint") == CAL_ERR_UNSUPPORTED
        assert "2 row(s) store more than one diagonal entry" in lib.cal_last_error(ctx.h).decode()
        check(ctx.h, lib.cal_prop_end(ctx.h))
        assert np.array_equal(ctx.spmv(x), y0)
    finally:
        ctx.close()


def test_refuses_bad_arguments(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    H, psi0, _, _, _ = nref.oscillator(256)
    V0 = np.tile(H.diagonal(), 2)
    nr = ctypes.c_int64()
    out = np.zeros(8)
    ctx = cal.Context(spmv_format="csr")
    try:
        ctx.set_matrix_stacked(H)
        # no open propagator
        assert lib.cal_prop_set_nonlinear(ctx.h, 1.0, b"midpoint") == CAL_ERR_ARG
        assert lib.cal_prop_get_nonlinear(ctx.h, 0, 0, None, ctypes.byref(nr)) == CAL_ERR_ARG
        P = cal.Propagator(H, psi0, 6, 4, ctx=ctx)
        for bad in (np.nan, np.inf, -np.inf):
            assert lib.cal_prop_set_nonlinear(ctx.h, bad, b"midpoint") == CAL_ERR_ARG
        for density in (b"", b"Midpoint", b"exact", None):
            assert lib.cal_prop_set_nonlinear(ctx.h, 1.0, density) == CAL_ERR_ARG
            assert lib.cal_prop_set_nonlinear(ctx.h, 0.0, density) == CAL_ERR_ARG
        with pytest.raises(cal.CalError):
            P.set_nonlinear(1.0, "rk4")
        assert np.array_equal(ctx.get_diagonal(), V0)
        assert P.step(DT, 1) == 0 and P.nonlinear().shape == (0, 2)  # nothing was set
        assert np.array_equal(ctx.get_diagonal(), V0)
        P.set_nonlinear(1.0)
        assert P.step(DT, 2) == 0
        assert lib.cal_prop_get_nonlinear(ctx.h, 1, 2, ptr(out), ctypes.byref(nr)) == CAL_ERR_ARG  # rows out of range
        assert nr.value == 2
        assert np.array_equal(P.nonlinear(first=1, count=1), P.nonlinear()[1:2])
        P.set_nonlinear(2.0, "frozen")  # setting the term again clears its history
        assert P.nonlinear().shape == (0, 2)
        P.close()
        assert np.array_equal(ctx.get_diagonal(), V0)
    finally:
        ctx.close()
