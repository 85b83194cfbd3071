"""The propagator's absorbing mask on the device (cal_prop_set_absorber /
cal_prop_get_absorbed / cal_prop_combine_masked; k_prop_combine's ABS flag).

Bars (tests/absorber_ref.py, tests/prop_obs_ref.py): the stored state is held
to the bits of the NumPy chain combine_ref, then M * top and M * bot; a sum of
N products whose absolute values sum to S is within (N + 8) eps S of the exact
sum -- absorbed: N = n, S = sum (1 - M^2) |u|^2; norm2: N = 2n, S = norm2; the
observables' bars are prop_obs_ref's, on the masked state.  Against the dense
scheme psi <- M .* U exp(-i dt E) U' psi the state's bar is that of
tests/test_gpu_prop.py, k 1e-10 after k steps (a mask <= 1 amplifies no step's
error), and a step's absorbed norm is within 2 ||u|| k 1e-10 plus its rounding
bar of the dense one (measured on an MI355X, N = 256 and 255: states within
3.5e-13 - 6.6e-13 at every step, the NumPy Lanczos oracle on the same input
2e-14 - 1.2e-13; absorbed rows within 2e-14).  With a mask of ones, and after the absorber is switched
off, runs are held to the bits of runs that never had one.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import absorber_ref as aref  # noqa: E402
import prop_obs_ref as pref  # noqa: E402
from split_cases import lap3d_v  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def ctx(cal):
    c = cal.Context()
    yield c
    c.close()


def _inputs(n, m, nw, nphi):
    rng = np.random.RandomState(100000 * nw + 10000 * nphi + 1000 * m + n)
    Q = np.asfortranarray(rng.randn(2 * n, m))
    c = rng.randn(m) + 1j * rng.randn(m)
    W = rng.randn(n, nw)
    phi = rng.randn(n, nphi) + 1j * rng.randn(n, nphi)
    return rng, Q, c, W, phi


# ---- 1. the kernel through prop_combine_masked ----------------------------------------------
@pytest.mark.parametrize("nw,nphi", [(0, 0), (2, 1), (4, 4)])
@pytest.mark.parametrize("m", [1, 24])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 20001])
def test_combine_masked_kernel(ctx, n, m, nw, nphi):
    rng, Q, c, W, phi = _inputs(n, m, nw, nphi)
    M = rng.rand(n)
    M[rng.randint(n)] = 1.0
    M[rng.randint(n)] = 0.0
    out, n2, ab, wv, ov = ctx.prop_combine_masked(Q, c, M, W, phi)
    top, bot = aref.combine_ref(Q, c)
    t, b, terms = aref.masked_ref(top, bot, M)
    assert np.array_equal(out.real, t) and np.array_equal(out.imag, b)
    assert wv.shape == (nw,) and ov.shape == (nphi,)
    ab_ref, ab_bar = np.sum(terms), aref.absorbed_bar(terms)
    n2_ref, n2_bar = aref.norm2_ref(t, b)
    wr, wbar = pref.w_ref(W, out)
    orf, bre, bim = pref.overlap_ref(phi, out)
    print("n=%d m=%d nw=%d nphi=%d: absorbed %.3e / %.3e, norm2 %.3e / %.3e, W %s / %s, Re %s / %s, Im %s / %s"
          % (n, m, nw, nphi, abs(ab - ab_ref), ab_bar, abs(n2 - n2_ref), n2_bar, np.abs(wv - wr), wbar,
             np.abs(ov.real - orf.real), bre, np.abs(ov.imag - orf.imag), bim))
    assert abs(ab - ab_ref) <= ab_bar
    assert abs(n2 - n2_ref) <= n2_bar
    assert np.all(np.abs(wv - wr) <= wbar)
    assert np.all(np.abs(ov.real - orf.real) <= bre)
    assert np.all(np.abs(ov.imag - orf.imag) <= bim)
    out_b, n2_b, ab_b, wv_b, ov_b = ctx.prop_combine_masked(Q, c, M, W, phi)
    assert np.array_equal(out, out_b) and n2 == n2_b and ab == ab_b
    assert np.array_equal(wv, wv_b) and np.array_equal(ov, ov_b)


# ---- 2. a mask of ones -----------------------------------------------------------------------
@pytest.mark.parametrize("nw,nphi", [(0, 0), (2, 1), (4, 4)])
@pytest.mark.parametrize("m", [1, 24])
@pytest.mark.parametrize("n", [1, 2, 3, 257, 1024, 1025, 20001])
def test_mask_of_ones_is_the_plain_kernel(ctx, n, m, nw, nphi):
    _, Q, c, W, phi = _inputs(n, m, nw, nphi)
    out, n2, ab, wv, ov = ctx.prop_combine_masked(Q, c, np.ones(n), W, phi)
    plain, n2p = ctx.prop_combine(Q, c)
    obs, n2o, wvo, ovo = ctx.prop_combine_obs(Q, c, W, phi)
    assert np.array_equal(out, plain) and n2 == n2p
    assert np.array_equal(out, obs) and n2 == n2o and np.array_equal(wv, wvo) and np.array_equal(ov, ovo)
    assert ab == 0.0


# ---- 3. a 0/1 mask ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 24])
@pytest.mark.parametrize("n", [2, 3, 257, 1025, 20001])
def test_zero_one_mask(ctx, n, m):
    rng, Q, c, _, _ = _inputs(n, m, 0, 0)
    M = (rng.rand(n) < 0.5).astype(float)
    M[0], M[-1] = 0.0, 1.0
    out, n2, ab, _, _ = ctx.prop_combine_masked(Q, c, M)
    plain, _ = ctx.prop_combine(Q, c)
    gone = M == 0.0
    assert not out[gone].any()
    assert np.array_equal(out[~gone], plain[~gone])
    terms = np.abs(plain[gone]) ** 2
    bar = (n + 8) * EPS * np.sum(terms)
    print("n=%d m=%d: absorbed %.17g, sum |u|^2 over the masked rows %.17g, bar %.3e" % (n, m, ab, np.sum(terms), bar))
    assert abs(ab - np.sum(terms)) <= bar
    n2_ref, n2_bar = aref.norm2_ref(out.real, out.imag)
    assert abs(n2 - n2_ref) <= n2_bar


# ---- 4. arguments ----------------------------------------------------------------------------
S, BLOCKS, STEPS, DT = 6, 4, 8, 0.025


def test_bad_masks_leave_the_absorber_in_place(cal):
    N = 255
    H, psi0, x, _, _ = pref.oscillator(N)
    M = aref.oscillator_mask(x)
    P = cal.Propagator(H, psi0, S, BLOCKS)
    R = cal.Propagator(H, psi0, S, BLOCKS)
    try:
        P.set_absorber(M)
        R.set_absorber(M)
        assert P.step(DT, 1) == 0
        for bad in (np.nan, -0.1, 1.5, np.inf):
            Mb = M.copy()
            Mb[N // 2] = bad
            with pytest.raises(cal.CalError) as e:
                P.set_absorber(Mb)
            assert e.value.status == cal._lib.CAL_ERR_ARG
        with pytest.raises(ValueError):
            P.set_absorber(M[:-1])
        assert P.absorbed()["t"].size == 1  # the refusals did not clear the history
        assert P.step(DT, 1) == 0
        assert R.step(DT, 2) == 0
        a, r = P.absorbed(), R.absorbed()
        assert a["t"].size == 2 and np.all(a["absorbed"] > 0.0)
        assert np.array_equal(a["absorbed"], r["absorbed"]) and np.array_equal(P.state(), R.state())
    finally:
        P.close()
        R.close()
    with pytest.raises(cal.CalError):
        P.set_absorber(M)


def test_no_propagator_is_an_argument_error(cal, ctx):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    one = np.ones(4)
    nr = ctypes.c_int64()
    assert lib.cal_prop_set_absorber(ctx.h, ptr(one)) == CAL_ERR_ARG
    assert lib.cal_prop_set_absorber(ctx.h, None) == CAL_ERR_ARG
    assert lib.cal_prop_get_absorbed(ctx.h, 0, 0, None, ctypes.byref(nr)) == CAL_ERR_ARG
    n, m = 5, 2
    rng = np.random.RandomState(0)
    Q, c = np.asfortranarray(rng.randn(2 * n, m)), rng.randn(m) + 1j * rng.randn(m)
    for bad in (np.nan, -0.1, 1.5):
        M = np.ones(n)
        M[3] = bad
        with pytest.raises(cal.CalError):
            ctx.prop_combine_masked(Q, c, M)
    with pytest.raises(ValueError):
        ctx.prop_combine_masked(Q, c, np.ones(n + 1))
    with pytest.raises(cal.CalError):
        ctx.prop_combine_masked(Q, c, np.ones(n), rng.randn(n, 5), None)


def test_history_bookkeeping(cal):
    N = 256
    H, psi0, x, _, _ = pref.oscillator(N)
    M = aref.oscillator_mask(x)
    c = cal.Context()
    try:
        P = cal.Propagator(H, psi0, S, BLOCKS, ctx=c)
        assert P.absorbed()["t"].size == 0
        P.set_observables(W=[x])
        P.step(DT, 1)
        assert P.absorbed()["t"].size == 0  # nothing set: no rows
        P.set_absorber(M)
        P.step(DT, 3)
        P.step(DT, 2)
        a = P.absorbed()
        assert a["t"].shape == (5,) and a["absorbed"].shape == (5,)
        # t counts from the start of the propagation: one step was taken before the set
        assert np.all(np.abs(a["t"] - DT * np.arange(2, 7)) <= 8 * EPS * DT * 6)
        assert np.array_equal(a["t"], P.observables()["t"][1:])
        part = P.absorbed(first=1, count=3)
        assert np.array_equal(part["t"], a["t"][1:4]) and np.array_equal(part["absorbed"], a["absorbed"][1:4])
        with pytest.raises(cal.CalError):
            P.absorbed(first=3, count=3)
        P.set_absorber(M * M)  # again: the absorbed history is cleared, the observables' is not
        assert P.absorbed()["t"].size == 0 and P.observables()["t"].size == 6
        P.step(DT, 1)
        assert P.absorbed()["t"].size == 1 and P.observables()["t"].size == 7
        P.set_observables(W=[x])  # and the other way round
        assert P.absorbed()["t"].size == 1 and P.observables()["t"].size == 0
        P.set_absorber(None)
        P.step(DT, 1)
        assert P.absorbed()["t"].size == 0
        P.set_absorber(M)
        P.close()
        # a new propagator on the same context starts without an absorber
        P = cal.Propagator(H, psi0, S, BLOCKS, ctx=c)
        P.step(DT, 2)
        assert P.absorbed()["t"].size == 0
        n0 = np.linalg.norm(psi0)
        assert abs(P.info()["norm"] - n0) <= 2 * 1e-10
        P.close()
    finally:
        c.close()


# ---- 5. the oscillator against the dense scheme ------------------------------------------------
@pytest.mark.parametrize("N", [256, 255])
def test_oscillator_against_the_dense_scheme(cal, N):
    H, psi0, x, _, _ = pref.oscillator(N)
    M = aref.oscillator_mask(x)
    dense, us, dab = aref.dense_scheme(N, M, DT, STEPS)
    oracle, _ = aref.propagate_numpy_masked(H, psi0.astype(complex), M, DT, STEPS, m=S * BLOCKS)
    P = cal.Propagator(H, psi0, S, BLOCKS, basis="newton")
    try:
        P.set_absorber(M)
        states = []
        for _ in range(STEPS):
            assert P.step(DT, 1) == 0
            states.append(P.state())
        ab, info = P.absorbed(), P.info()
    finally:
        P.close()
    assert ab["t"].shape == (STEPS,)
    assert np.all(np.abs(ab["t"] - DT * np.arange(1, STEPS + 1)) <= 8 * EPS * DT * STEPS)
    worst = []
    for k in range(1, STEPS + 1):
        err = np.linalg.norm(states[k - 1] - dense[k - 1])
        e_or = np.linalg.norm(oracle[k - 1] - dense[k - 1])
        u = us[k - 1]
        terms = (1.0 - M * M) * np.abs(u) ** 2
        abar = 2 * np.linalg.norm(u) * k * 1e-10 + aref.absorbed_bar(terms)
        d_ab = abs(ab["absorbed"][k - 1] - dab[k - 1])
        print("N=%d step %d: err %.3e (NumPy oracle %.3e, bar %.1e), |absorbed - dense| %.3e (bar %.3e), absorbed %.6e"
              % (N, k, err, e_or, k * 1e-10, d_ab, abar, ab["absorbed"][k - 1]))
        worst.append((err <= k * 1e-10, d_ab <= abar))
    assert all(a for a, _ in worst), "state outside k 1e-10 (the figures are printed)"
    assert all(b for _, b in worst), "absorbed outside its bar (the figures are printed)"
    last = states[-1]
    n2_ref, n2_bar = aref.norm2_ref(last.real, last.imag)
    assert abs(info["norm"] ** 2 - n2_ref) <= n2_bar + 4 * EPS * n2_ref
    assert info["steps"] == STEPS and info["breakdowns"] == 0
    # the mask is no no-op here: about 5 % of the squared norm is gone
    assert 0.93 <= n2_ref / np.sum(psi0 ** 2) <= 0.97


# ---- 6. do not disturb ------------------------------------------------------------------------------
def _osc_run(cal, N, plan, observables=True):
    """plan: a list of (mask or None or "keep", steps); returns state, info, histories."""
    H, psi0, x, _, _ = pref.oscillator(N)
    P = cal.Propagator(H, psi0, S, BLOCKS, basis="newton")
    try:
        if observables:
            P.set_observables(W=[x, x * x], phi=[psi0], energy=True)
        for mask, steps in plan:
            if not isinstance(mask, str):
                P.set_absorber(mask)
            assert P.step(DT, steps) == 0
        info = P.info()
        info.pop("ms")  # wall time
        return dict(state=P.state(), info=info, hist=P.observables(), absorbed=P.absorbed())
    finally:
        P.close()


def _same_run(a, b):
    assert np.array_equal(a["state"], b["state"])
    assert a["info"].keys() == b["info"].keys()
    for k in a["info"]:
        assert np.array_equal(a["info"][k], b["info"][k]), k
    assert a["hist"].keys() == b["hist"].keys()
    for k in a["hist"]:
        assert np.array_equal(a["hist"][k], b["hist"][k], equal_nan=True), k


@pytest.mark.parametrize("observables", [True, False])
@pytest.mark.parametrize("N", [256, 255])
def test_mask_of_ones_does_not_disturb_the_run(cal, N, observables):
    ones = _osc_run(cal, N, [(np.ones(N), STEPS)], observables)
    plain = _osc_run(cal, N, [("keep", STEPS)], observables)
    _same_run(ones, plain)
    assert ones["info"]["steps"] == STEPS and ones["hist"]["t"].size == (STEPS if observables else 0)
    assert ones["absorbed"]["t"].shape == (STEPS,) and not ones["absorbed"]["absorbed"].any()
    assert plain["absorbed"]["t"].size == 0
    if observables:
        assert np.array_equal(ones["absorbed"]["t"], ones["hist"]["t"])


@pytest.mark.parametrize("N", [256, 255])
def test_switching_off_continues_as_never_masked(cal, N):
    _, _, x, _, _ = pref.oscillator(N)
    M = aref.oscillator_mask(x)
    # ones for 3 steps (the bits of no absorber, above), off, 2 more steps: 5 steps that never had one
    off = _osc_run(cal, N, [(np.ones(N), 3), (None, 2)])
    never = _osc_run(cal, N, [("keep", 5)])
    _same_run(off, never)
    assert off["absorbed"]["t"].size == 0
    # from a truly masked state: off continues as the masked kernel with a mask of ones does
    a = _osc_run(cal, N, [(M, 3), (None, 2)])
    b = _osc_run(cal, N, [(M, 3), (np.ones(N), 2)])
    _same_run(a, b)
    assert b["absorbed"]["t"].size == 2 and not b["absorbed"]["absorbed"].any()
    assert not np.array_equal(a["state"], never["state"])
    assert a["info"]["norm"] < 0.99 * never["info"]["norm"]


# ---- 7. with the drive and observables on lap3d_v(17) --------------------------------------------
def _lap_drive(t):
    return [0.3 * np.sin(3 * t), 0.02 * np.cos(2 * t)]


def _lap_run(cal, fmt, scheme, steps=3, dt=0.05):
    N = 17
    H = lap3d_v(cal, N)
    n = H.shape[0]
    i = np.arange(n)
    psi0 = np.exp(-((i % N - 8.0) ** 2 + ((i // N) % N - 8.0) ** 2 + (i // N ** 2 - 8.0) ** 2) / 18.0) * \
        np.exp(0.7j * (i % N))
    psi0 = psi0 / np.linalg.norm(psi0)
    W = [i % N - 8.0, ((i // N) % N - 8.0) ** 2]
    M = cal.matrices.absorber_mask((N, N, N), 4)
    c = cal.Context(spmv_format=fmt)
    try:
        P = cal.Propagator(H, psi0, 4, 3, basis="newton", ctx=c)
        assert c.spmv_split_info()[0] == (fmt == "split")
        P.set_observables(W=[W[0]], phi=[psi0], energy=True)
        P.set_drive(W)
        P.set_absorber(M)
        assert P.step(dt, steps, drive=_lap_drive, scheme=scheme) == 0
        o, a = P.observables(), P.absorbed()
        out = dict(state=P.state(), norm=P.info()["norm"], absorbed=np.column_stack([a["t"], a["absorbed"]]),
                   hist=np.column_stack([o["t"], o["norm2"], o["energy"], o["W"], o["overlap"].real,
                                         o["overlap"].imag]), M=M, H=H, W=W, psi0=psi0)
        P.close()
        return out
    finally:
        c.close()


def _same_lap(a, b):
    return (np.array_equal(a["state"], b["state"]) and a["norm"] == b["norm"]
            and np.array_equal(a["absorbed"], b["absorbed"]) and np.array_equal(a["hist"], b["hist"]))


@pytest.fixture(scope="module")
def lap_runs(cal):
    return {(fmt, sch): _lap_run(cal, fmt, sch) for fmt in ("split", "csr") for sch in ("midpoint", "cf4")}


@pytest.mark.parametrize("scheme", ["midpoint", "cf4"])
def test_formats_agree_with_drive_observables_and_mask(cal, lap_runs, scheme):
    a, b = lap_runs[("split", scheme)], lap_runs[("csr", scheme)]
    rows = 3 * (2 if scheme == "cf4" else 1)
    assert a["absorbed"].shape == (rows, 2) and a["hist"].shape == (rows, 6)
    assert np.all(np.isfinite(a["hist"])) and np.all(np.isfinite(a["state"].view(float)))
    assert _same_lap(a, b)
    assert np.all(a["absorbed"][:, 1] > 0.0)  # the packet's tail reaches the ramp
    # the last row's observables and norm are those of the stored (masked) state
    n2_ref, n2_bar = aref.norm2_ref(a["state"].real, a["state"].imag)
    assert abs(a["hist"][-1, 1] - n2_ref) <= n2_bar
    wr, wbar = pref.w_ref(a["W"][0].reshape(-1, 1), a["state"])
    orf, bre, bim = pref.overlap_ref(a["psi0"].reshape(-1, 1), a["state"])
    assert abs(a["hist"][-1, 3] - wr[0]) <= wbar[0]
    assert abs(a["hist"][-1, 4] - orf[0].real) <= bre[0] and abs(a["hist"][-1, 5] - orf[0].imag) <= bim[0]
    # what the norm loses against what the mask took (1 at the start); printed, the steps' own drift is in it
    print("%s: norm lost %.6e, absorbed in all %.6e" % (scheme, 1.0 - a["hist"][-1, 1], np.sum(a["absorbed"][:, 1])))


@pytest.mark.parametrize("scheme", ["midpoint", "cf4"])
def test_masked_driven_runs_repeat_to_the_bit(cal, lap_runs, scheme):
    for fmt in ("split", "csr"):
        assert _same_lap(lap_runs[(fmt, scheme)], _lap_run(cal, fmt, scheme))


def test_cf4_records_two_absorbed_rows_per_step(cal, lap_runs):
    dt = 0.05
    a = lap_runs[("split", "cf4")]
    t = a["absorbed"][:, 0]
    assert t.shape == (6,)
    assert np.all(np.abs(t - 0.5 * dt * np.arange(1, 7)) <= 8 * EPS * 6 * dt)
    assert np.array_equal(t, a["hist"][:, 0])
    m = lap_runs[("split", "midpoint")]["absorbed"][:, 0]
    assert np.all(np.abs(m - dt * np.arange(1, 4)) <= 8 * EPS * 3 * dt)
