"""The time-dependent potential H(t) = H0 + sum_k f_k(t) diag(W_k) on the device:
cal_set_diagonal / cal_get_diagonal, cal_prop_set_drive, cal_prop_step_driven,
cal_prop_refresh_shifts (kernels k_diag_find / k_diag_density without a state, prop.hip).

Bars:
  * rewriting the diagonal is bit-exact: a context whose diagonal was rewritten
    computes what a fresh context set with the new values computes
    (array_equal), on CSR and on the diagonal-split format, and the diagonal a
    driven step leaves is the NumPy chain of tests/drive_ref.py to the bit.
  * driven propagation: 2-norm error against the product of the dense eigh
    exponentials of the same per-step Hamiltonians at most steps * 1e-10, and
    the same for the norm drift -- the bars of tests/test_gpu_prop.py, for the
    same reason (tol = 1e-10 bounds each step's residual estimate, unitary
    steps add their errors).  The CPU oracle (ca_lanczos on blkdiag(H_j, H_j),
    'local', then expm) is held to the same bar next to the device.
"""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drive_ref as dref  # noqa: E402
from split_cases import drop_diagonal, hamiltonian_2d, lap3d_v  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- matrices ------------------------------------------------------------------------
def canon(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    return A


def rand_sym(n, seed):
    """Random sparse symmetric matrix, about 6 off-diagonals per row, every diagonal entry stored."""
    rng = np.random.RandomState(seed)
    m = min(3 * n, n * (n - 1) // 2)
    i, j = rng.randint(0, n, m), rng.randint(0, n, m)
    keep = i != j
    U = sp.coo_matrix((rng.randn(int(keep.sum())), (i[keep], j[keep])), shape=(n, n))
    return canon(U + U.T + sp.diags(rng.randn(n) + 3.0))


def arrow(n, seed):
    """Dense first row and column (a row longer than a CSR row block) plus the diagonal."""
    rng = np.random.RandomState(seed)
    v = rng.randn(n - 1)
    r = np.concatenate([np.zeros(n - 1, dtype=int), np.arange(1, n)])
    c = np.concatenate([np.arange(1, n), np.zeros(n - 1, dtype=int)])
    return canon(sp.coo_matrix((np.concatenate([v, v]), (r, c)), shape=(n, n)) + sp.diags(rng.randn(n) + 2.0))


def diag_positions(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    pos = np.nonzero(rows == A.indices)[0]
    assert len(pos) == A.shape[0]
    return pos


def with_diag(A, d):
    """A's structure with the diagonal values d (explicit zeros stay stored)."""
    B = A.copy()
    B.data = B.data.copy()
    B.data[diag_positions(A)] = d
    assert B.nnz == A.nnz
    return B


def new_diag(n, seed):
    d = np.random.RandomState(seed).randn(n)
    d[:: 3] = 0.0  # exact +0.0 entries: the slots stay stored
    return d


def csr_cases(cal):
    out = [("rand%d" % n, rand_sym(n, 100 + n)) for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)]
    out.append(("arrow3000", arrow(3000, 7)))
    out.append(("circuit200", canon(cal.matrices.circuit_like(200))))
    return out


CSR_NAMES = ["rand%d" % n for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)] + ["arrow3000", "circuit200"]


# ---- 4. set_diagonal on CSR -------------------------------------------------------------
@pytest.mark.parametrize("name", CSR_NAMES)
def test_set_diagonal_csr_bit_exact(cal, name):
    A = dict(csr_cases(cal))[name]
    n = A.shape[0]
    if name == "arrow3000":
        assert A.indptr[1] - A.indptr[0] > 2048
    d0 = A.diagonal()
    d = new_diag(n, n)
    x = np.random.RandomState(n + 1).randn(n)
    ctx = cal.Context(spmv_format="csr").set_matrix(A)
    fresh = cal.Context(spmv_format="csr").set_matrix(with_diag(A, d))
    try:
        assert ctx.spmv_format()[0] == "csr"
        y0 = ctx.spmv(x)
        assert np.array_equal(ctx.get_diagonal(), d0)
        ctx.set_diagonal(d)
        got = ctx.get_diagonal()
        assert np.array_equal(got, d) and not np.any(np.signbit(got[::3]))
        assert np.array_equal(ctx.spmv(x), fresh.spmv(x))
        assert ctx.matrix_info()["nnz_local"] == A.nnz
        ctx.set_diagonal(d0)
        assert np.array_equal(ctx.get_diagonal(), d0)
        assert np.array_equal(ctx.spmv(x), y0)
    finally:
        ctx.close()
        fresh.close()


# ---- 5. set_diagonal on the split format ----------------------------------------------------
@pytest.mark.parametrize("which", ["lap3d_v17", "ham2d_257"])
def test_set_diagonal_split_bit_exact(cal, ref, which):
    A = lap3d_v(cal, 17) if which == "lap3d_v17" else hamiltonian_2d(cal, 257)
    n = A.shape[0]
    assert n == 4913 or n > 65535
    d = new_diag(n, 5) + 0.25 * np.arange(n) / n
    B = with_diag(A, d)
    rng = np.random.RandomState(9)
    x, xprev = rng.randn(n), rng.randn(n)
    lam = np.array([7.0, 3 + 0.5j, 3 - 0.5j])
    r = ref.matlab_rand(n)
    ctx = cal.Context(spmv_format="split").set_matrix(A)
    fs = cal.Context(spmv_format="split").set_matrix(B)
    fc = cal.Context(spmv_format="csr").set_matrix(B)
    try:
        on, P, _, neg1 = ctx.spmv_split_info()
        assert on and (P == 289 if which == "lap3d_v17" else not neg1)
        ctx.set_diagonal(d)
        assert ctx.spmv_split_info()[0] and fs.spmv_split_info()[0] and not fc.spmv_split_info()[0]
        assert np.array_equal(ctx.get_diagonal(), d)
        for other in (fs, fc):
            assert np.array_equal(ctx.spmv(x), other.spmv(x))
            assert np.array_equal(cal.matrix_powers_newton(B, x, 3, lam, 1, ctx=ctx),
                                  cal.matrix_powers_newton(B, x, 3, lam, 1, ctx=other))
            ya, da = ctx.spmv_lanczos(x, xprev, 0.7)
            yb, db = other.spmv_lanczos(x, xprev, 0.7)
            assert np.array_equal(ya, yb) and da == db
        # whole runs: one outer block (iter = 3 < s) and three (iter = 12)
        for it in (3, 12):
            a = cal.ca_lanczos_ex(B, r, 4, it, "newton", "local", ctx=ctx)
            b = cal.ca_lanczos_ex(B, r, 4, it, "newton", "local", ctx=fc)
            assert np.array_equal(a.T, b.T) and np.array_equal(a.Q, b.Q) and np.array_equal(a.shifts, b.shifts)
            assert np.array_equal(a.ritz_rnorm, b.ritz_rnorm)
    finally:
        ctx.close()
        fs.close()
        fc.close()


# ---- 6. refusals -----------------------------------------------------------------------------
def _refused(cal, ctx, n, status, word):
    from ca_lanczos_amd._lib import lib, ptr
    x = np.random.RandomState(3).randn(n)
    y0 = ctx.spmv(x)
    d = np.ones(n)
    out = np.zeros(n)
    assert lib.cal_set_diagonal(ctx.h, n, ptr(d)) == status
    msg = lib.cal_last_error(ctx.h).decode()
    assert word in msg, msg
    assert lib.cal_get_diagonal(ctx.h, n, ptr(out)) == status
    assert lib.cal_set_diagonal(ctx.h, n, ptr(d)) == status  # the cached verdict answers the same
    assert np.array_equal(ctx.spmv(x), y0)


@pytest.mark.parametrize("fmt", ["csr", "split"])
def test_refuses_missing_diagonal(cal, fmt):
    from ca_lanczos_amd._lib import CAL_ERR_UNSUPPORTED
    A = drop_diagonal(lap3d_v(cal, 17), [0, 2456, 4912])
    ctx = cal.Context(spmv_format=fmt).set_matrix(A)
    try:
        assert ctx.spmv_split_info()[0] == (fmt == "split")
        _refused(cal, ctx, A.shape[0], CAL_ERR_UNSUPPORTED, "3 row(s) store no diagonal entry")
    finally:
        ctx.close()


def test_refuses_empty_row(cal):
    from ca_lanczos_amd._lib import CAL_ERR_UNSUPPORTED
    A = rand_sym(100, 4).tolil()
    A[37, :] = 0.0
    A[:, 37] = 0.0
    A = canon(A.tocsr())
    A.eliminate_zeros()
    assert A.indptr[38] == A.indptr[37]
    ctx = cal.Context(spmv_format="csr").set_matrix(A)
    try:
        _refused(cal, ctx, 100, CAL_ERR_UNSUPPORTED, "1 row(s) store no diagonal entry")
    finally:
        ctx.close()


def test_refuses_duplicate_diagonal(cal):
    """Two stored entries with col == row in one row (raw arrays: SciPy would sum them)."""
    import ctypes
    from ca_lanczos_amd._lib import CAL_ERR_UNSUPPORTED, check, lib, ptr
    rowptr = np.array([0, 2, 5, 7], dtype=np.int64)
    col = np.array([0, 1, 0, 1, 1, 1, 2], dtype=np.int32)
    val = np.array([2.0, -1.0, -1.0, 1.5, 0.5, -1.0, 2.0])
    ctx = cal.Context(spmv_format="csr")
    try:
        check(ctx.h, lib.cal_set_matrix_csr(ctx.h, 3, rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                            col.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ptr(val)))
        _refused(cal, ctx, 3, CAL_ERR_UNSUPPORTED, "1 row(s) store more than one diagonal entry")
    finally:
        ctx.close()


def test_refuses_pattern_format(cal):
    from ca_lanczos_amd._lib import CAL_ERR_UNSUPPORTED
    A = cal.matrices.laplacian_3d(20)
    ctx = cal.Context(spmv_format="pattern").set_matrix(A)
    try:
        assert ctx.spmv_format()[0] == "pattern"
        _refused(cal, ctx, A.shape[0], CAL_ERR_UNSUPPORTED, "cal_set_spmv_format")
    finally:
        ctx.close()


def test_refuses_bad_arguments_and_open_runs(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    A = rand_sym(257, 1)
    n = A.shape[0]
    x = np.random.RandomState(2).randn(n)
    ctx = cal.Context(spmv_format="csr").set_matrix(A)
    try:
        y0 = ctx.spmv(x)
        for bad in (np.nan, np.inf, -np.inf):
            d = np.ones(n)
            d[n // 2] = bad
            assert lib.cal_set_diagonal(ctx.h, n, ptr(d)) == CAL_ERR_ARG
        assert lib.cal_set_diagonal(ctx.h, n - 1, ptr(np.ones(n))) == CAL_ERR_ARG
        assert lib.cal_set_diagonal(ctx.h, n, None) == CAL_ERR_ARG
        assert np.array_equal(ctx.spmv(x), y0)
        ctx.lanczos_begin(x, 4, 3, "newton", "local")
        assert lib.cal_set_diagonal(ctx.h, n, ptr(np.ones(n))) == CAL_ERR_ARG
        assert lib.cal_get_diagonal(ctx.h, n, ptr(np.ones(n))) == CAL_ERR_ARG
        ctx.lanczos_end()
        assert np.array_equal(ctx.get_diagonal(), A.diagonal())
        assert np.array_equal(ctx.spmv(x), y0)
        # a propagator owns the diagonal while it is open; the drive's own argument checks
        H, psi0, xg, _, _ = dref.oscillator(256)
        P = cal.Propagator(H, psi0, 6, 4, ctx=ctx)
        assert lib.cal_set_diagonal(ctx.h, 512, ptr(np.ones(512))) == CAL_ERR_ARG
        one = np.ones((256, 5), order="F")
        assert lib.cal_prop_set_drive(ctx.h, 5, ptr(one)) == CAL_ERR_ARG
        assert lib.cal_prop_set_drive(ctx.h, -1, ptr(one)) == CAL_ERR_ARG
        f = np.zeros(4)
        assert lib.cal_prop_step_driven(ctx.h, 0.025, 1e-10, 0, 1, ptr(f), 1) == CAL_ERR_ARG  # no drive set
        P.set_drive([xg, xg * xg])
        assert lib.cal_prop_step_driven(ctx.h, 0.025, 1e-10, 0, 1, ptr(f), 1) == CAL_ERR_ARG  # ldf < nk
        f[3] = np.nan
        assert lib.cal_prop_step_driven(ctx.h, 0.025, 1e-10, 0, 2, ptr(f), 2) == CAL_ERR_ARG  # nothing ran
        assert P.info()["steps"] == 0
        assert np.array_equal(ctx.get_diagonal(), np.tile(H.diagonal(), 2))
        P.close()
    finally:
        ctx.close()


# ---- 7. the drive kernel's order contract ---------------------------------------------------------
def _order_setup(cal, which):
    if which == "lap3d_v17":
        H = lap3d_v(cal, 17)
        n = H.shape[0]
        i = np.arange(n)
        psi0 = np.exp(-((i % 17 - 8.0) ** 2 + ((i // 17) % 17 - 8.0) ** 2 + (i // 289 - 8.0) ** 2) / 18.0) * \
            np.exp(0.7j * (i % 17))
        return H, psi0 / np.linalg.norm(psi0), "split", 0.05
    H, psi0, _, _, _ = dref.oscillator(int(which))
    return H, psi0.astype(complex), "csr", 0.025


@pytest.mark.parametrize("which", ["255", "256", "lap3d_v17"])
def test_drive_order_contract(cal, which):
    H, psi0, fmt, dt = _order_setup(cal, which)
    n = H.shape[0]
    rng = np.random.RandomState(n)
    W = [rng.randn(n), rng.randn(n) * 100.0, rng.rand(n) * 1e-3]
    f = rng.randn(3)
    V0 = H.diagonal()
    expect = dref.chain(V0, W, f)
    assert not np.array_equal(expect, V0 + (f[0] * W[0] + f[1] * W[1] + f[2] * W[2]))  # the order is observable
    ctx = cal.Context(spmv_format=fmt)
    try:
        P = cal.Propagator(H, psi0, 4, 3, ctx=ctx)
        assert ctx.spmv_split_info()[0] == (fmt == "split")
        P.set_drive(W)
        assert np.array_equal(ctx.get_diagonal(), np.tile(V0, 2))
        P.step(dt, 1, drive=[f])
        assert np.array_equal(ctx.get_diagonal(), np.tile(expect, 2))
        P.set_drive(None)
        assert np.array_equal(ctx.get_diagonal(), np.tile(V0, 2))
        P.set_drive(W[:2])
        P.step(dt, 1, drive=np.array([f[:2]]))
        assert np.array_equal(ctx.get_diagonal(), np.tile(dref.chain(V0, W[:2], f[:2]), 2))
        P.close()  # the caller's context keeps its matrix, as the caller set it
        assert np.array_equal(ctx.get_diagonal(), np.tile(V0, 2))
        x = rng.randn(2 * n)
        fresh = cal.Context(spmv_format=fmt).set_matrix_stacked(H)
        y = fresh.spmv(x)
        fresh.close()
        assert np.array_equal(ctx.spmv(x), y)
    finally:
        ctx.close()


# ---- 8. / 11. / 13. bit identities on lap3d_v(17) ------------------------------------------------
def _lap_run(cal, fmt, rows, drive_on=True, s=4, blocks=3, dt=0.05):
    H, psi0, _, _ = _order_setup(cal, "lap3d_v17")
    n = H.shape[0]
    i = np.arange(n)
    W = [i % 17 - 8.0, ((i // 17) % 17 - 8.0) ** 2]
    ctx = cal.Context(spmv_format=fmt)
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=ctx)
        assert ctx.spmv_split_info()[0] == (fmt == "split")
        P.set_observables(W=[W[0]], phi=[psi0], energy=True)
        if drive_on:
            P.set_drive(W)
            assert P.step(dt, len(rows), drive=rows) == 0
        else:
            assert P.step(dt, len(rows)) == 0
        o = P.observables()
        out = (P.state(), P.info()["norm"], np.column_stack([o["t"], o["norm2"], o["energy"], o["W"],
                                                            o["overlap"].real, o["overlap"].imag]))
        P.close()
        return out
    finally:
        ctx.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.fixture(scope="module")
def lap_rows():
    t = 0.05 * (np.arange(4) + 0.5)
    return np.column_stack([0.3 * np.sin(3 * t), 0.02 * np.cos(2 * t)])


@pytest.fixture(scope="module")
def lap_driven(cal, lap_rows):
    return {fmt: _lap_run(cal, fmt, lap_rows) for fmt in ("split", "csr")}


@pytest.mark.parametrize("fmt", ["split", "csr"])
def test_zero_amplitudes_change_nothing(cal, fmt):
    driven = _lap_run(cal, fmt, np.zeros((4, 2)))
    plain = _lap_run(cal, fmt, np.zeros((4, 2)), drive_on=False)
    assert driven[2].shape == (4, 6) and np.all(np.isfinite(driven[2]))
    assert _same(driven, plain)


def test_formats_agree_under_the_drive(cal, lap_driven, lap_rows):
    a, b = lap_driven["split"], lap_driven["csr"]
    assert a[2].shape == (4, 6) and np.all(np.isfinite(a[2])) and np.all(np.isfinite(a[0].view(float)))
    assert _same(a, b)
    # and the drive does something
    plain = _lap_run(cal, "csr", lap_rows, drive_on=False)
    assert not np.array_equal(a[0], plain[0])


def test_driven_runs_repeat_to_the_bit(cal, lap_driven, lap_rows):
    for fmt in ("split", "csr"):
        assert _same(lap_driven[fmt], _lap_run(cal, fmt, lap_rows))


# ---- 9. accuracy -------------------------------------------------------------------------------------
def _ops(N, nops):
    _, _, x, _, _ = dref.oscillator(N)
    return ([x], dref.f_one) if nops == 1 else ([x, x * x], dref.f_two)


@functools.lru_cache(maxsize=None)
def oscillator_reference(N, nops, dt, steps):
    H, psi0, _, _, _ = dref.oscillator(N)
    W, f = _ops(N, nops)
    rows = np.array([f((j + 0.5) * dt) for j in range(steps)])
    return rows, dref.dense_driven(H, W, psi0, rows, dt)


@pytest.mark.parametrize("nops", [1, 2])
@pytest.mark.parametrize("s,blocks", [(6, 4), (4, 6)])
@pytest.mark.parametrize("basis", ["newton", "monomial"])
@pytest.mark.parametrize("N", [256, 255])
def test_driven_oscillator(cal, N, basis, s, blocks, nops):
    steps, dt = 8, 0.025
    bar = steps * 1e-10
    H, psi0, _, _, _ = dref.oscillator(N)
    W, f = _ops(N, nops)
    rows, exact = oscillator_reference(N, nops, dt, steps)
    got, sub = cal.drive_rows(f, 0.0, dt, steps, "midpoint")
    assert sub == dt and np.allclose(got, rows, rtol=0, atol=1e-15)
    n0 = np.linalg.norm(psi0)
    ctx = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis=basis, ctx=ctx)
        P.set_drive(W)
        drift = 0.0
        for j in range(steps):
            assert P.step(dt, 1, drive=rows[j:j + 1]) == 0
            drift = max(drift, abs(P.info()["norm"] - n0))
        psi, info = P.state(), P.info()
        P.close()
    finally:
        ctx.close()
    err = np.linalg.norm(psi - exact)
    psi_or, drift_or = dref.oracle_driven(H, W, psi0, rows, dt, s, blocks, basis)
    e_or = np.linalg.norm(psi_or - exact)
    print("N=%d %s s=%d blocks=%d nops=%d: err %.3e drift %.3e, oracle err %.3e drift %.3e, residual_max %.3e"
          % (N, basis, s, blocks, nops, err, drift, e_or, drift_or, info["residual_max"]))
    assert e_or <= bar and drift_or <= bar, (e_or, drift_or)
    assert err <= bar, err
    assert drift <= bar, drift
    assert info["steps"] == steps and abs(P.t - steps * dt) < 1e-15


def packet_drive(t):
    return np.array([0.05 * np.sin(3.0 * t), 0.02 * np.cos(2.0 * t)])


def test_driven_packet_cf4(cal):
    """The commutator-free fourth-order rule through a callable drive: 4 steps
    of dt = 0.5 are 8 sub-steps of 0.25, each with its own amplitudes; the
    dense reference takes the same sub-steps, so the bar is 8 x 1e-10."""
    H, psi0, x, y = dref.packet_2d()
    steps, dt, s, blocks = 4, 0.5, 6, 4
    rows, sub = cal.drive_rows(packet_drive, 0.0, dt, steps, "cf4")
    assert rows.shape == (2 * steps, 2) and sub == 0.25
    bar = 2 * steps * 1e-10
    exact = dref.dense_driven(H, [x, y], psi0, rows, sub)
    ctx = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis="newton", ctx=ctx)
        assert ctx.spmv_format()[0] == "csr"
        P.set_observables(energy=True)
        P.set_drive([x, y])
        assert P.step(dt, steps, drive=packet_drive, scheme="cf4") == 0
        psi, info, o = P.state(), P.info(), P.observables()
        P.close()
    finally:
        ctx.close()
    n0 = np.linalg.norm(psi0)
    err, drift = np.linalg.norm(psi - exact), np.max(np.abs(np.sqrt(o["norm2"]) - n0))
    psi_or, drift_or = dref.oracle_driven(H, [x, y], psi0, rows, sub, s, blocks, "newton")
    e_or = np.linalg.norm(psi_or - exact)
    print("packet cf4: err %.3e drift %.3e, oracle err %.3e drift %.3e" % (err, drift, e_or, drift_or))
    assert e_or <= bar and drift_or <= bar, (e_or, drift_or)
    assert err <= bar and drift <= bar, (err, drift)
    # the clock: two sub-steps per step, their sum in P.t and in the history's t column
    assert info["steps"] == 2 * steps and abs(P.t - steps * dt) < 1e-15
    assert np.allclose(o["t"], sub * np.arange(1, 2 * steps + 1), rtol=0, atol=1e-15)
    # the energy of the last row is <psi|H|psi> with the H of the last sub-step
    Hl = H + sp.diags(rows[-1, 0] * x + rows[-1, 1] * y)
    E, ebar = dref.pref.energy_ref(Hl, psi)  # the rounding bar of tests/prop_obs_ref.py
    assert abs(o["energy"][-1] - E) <= ebar, (o["energy"][-1], E, ebar)


# ---- 10. global phase ---------------------------------------------------------------------------------
def test_constant_shift_is_a_global_phase(cal):
    H, psi0, _, _, _ = dref.oscillator(256)
    steps, dt = 8, 0.025
    out = []
    for driven in (True, False):
        ctx = cal.Context(spmv_format="csr")
        try:
            P = cal.Propagator(H, psi0, 6, 4, basis="newton", ctx=ctx)
            if driven:
                P.set_drive([np.ones(256)])
                assert P.step(dt, steps, drive=lambda t: [3.0]) == 0
            else:
                assert P.step(dt, steps) == 0
            out.append(P.state())
            P.close()
        finally:
            ctx.close()
    d = np.linalg.norm(out[0] - np.exp(-3j * steps * dt) * out[1])
    print("global phase: %.3e (bar %.3e)" % (d, 2 * steps * 1e-10))
    assert d <= 2 * steps * 1e-10
    assert np.linalg.norm(out[0] - out[1]) > 0.1  # the phase is there


# ---- 12. refresh_shifts -----------------------------------------------------------------------------------
def test_refresh_shifts(cal):
    H, psi0, _, ew, _ = dref.oscillator(256)
    lo, hi = ew[0], ew[-1]
    c = 2.0 * (hi - lo)
    tolr = 1e-9 * max(abs(lo), abs(hi))
    ctx = cal.Context(spmv_format="csr")
    try:
        P = cal.Propagator(H, psi0, 6, 4, basis="newton", ctx=ctx)
        P.set_drive([np.ones(256)])
        assert P.step(0.025, 1, drive=[[0.0]]) == 0
        S0 = P.info()["shifts"]
        assert len(S0) >= 6 and np.all(S0 >= lo - tolr) and np.all(S0 <= hi + tolr)
        P.step(0.025, 1, drive=[[c]])
        assert np.array_equal(P.info()["shifts"], S0)
        P.refresh_shifts()
        P.step(0.025, 1, drive=[[c]])
        S1 = P.info()["shifts"]
        print("shifts before [%.3f, %.3f], after the refresh [%.3f, %.3f], c = %.3f"
              % (S0.min(), S0.max(), S1.min(), S1.max(), c))
        assert len(S1) == len(S0)
        assert np.all(S1 >= lo + c - tolr) and np.all(S1 <= hi + c + tolr)
        assert S1.min() > S0.max()
        P.close()
        # the monomial basis has no shifts to forget
        P = cal.Propagator(H, psi0, 6, 4, basis="monomial", ctx=ctx)
        P.refresh_shifts()
        assert P.step(0.025, 1) == 0 and len(P.info()["shifts"]) == 0
        P.close()
    finally:
        ctx.close()
