"""Device-side observables of the time propagator (cal_prop_set_observables /
cal_prop_get_observables / cal_prop_combine_obs; k_prop_combine's OBS flag).

Bars (tests/prop_obs_ref.py): a sum of N products whose absolute values sum
to S is within (N + 8) eps S of the exact sum in any order -- N = n for a
diagonal operator, 2n for an overlap component, nnz(blkdiag(H, H)) + 2n for
the energy with S = |x|' |A| |x|.  Against the exact solution the state's own
bar of tests/test_gpu_prop.py (k 1e-10 after k steps) is carried through each
observable (prop_obs_ref.physics_bars) and the rounding bar added.  State,
norm and counters with observables set are held to the bits of a run without.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prop_obs_ref as pref  # noqa: E402
from prop_obs_ref import combine_ref  # noqa: E402
from split_cases import lap3d_v, potential  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def ctx(cal):
    c = cal.Context()
    yield c
    c.close()


# ---- 1. the kernel through prop_combine_obs ----------------------------------------------
@pytest.mark.parametrize("nw,nphi", [(1, 0), (0, 1), (2, 1), (4, 4)])
@pytest.mark.parametrize("m", [1, 24])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 20001])
def test_combine_obs_kernel(ctx, n, m, nw, nphi):
    rng = np.random.RandomState(100000 * nw + 10000 * nphi + 1000 * m + n)
    Q = np.asfortranarray(rng.randn(2 * n, m))
    c = rng.randn(m) + 1j * rng.randn(m)
    W = rng.randn(n, nw)
    phi = rng.randn(n, nphi) + 1j * rng.randn(n, nphi)
    out, n2, wv, ov = ctx.prop_combine_obs(Q, c, W, phi)
    plain, n2p = ctx.prop_combine(Q, c)
    top, bot = combine_ref(Q, c)
    assert np.array_equal(out, plain) and n2 == n2p
    assert np.array_equal(out.real, top) and np.array_equal(out.imag, bot)
    assert wv.shape == (nw,) and ov.shape == (nphi,)
    wr, wbar = pref.w_ref(W, out)
    orf, bre, bim = pref.overlap_ref(phi, out)
    print("n=%d m=%d nw=%d nphi=%d: W %s / %s, Re %s / %s, Im %s / %s"
          % (n, m, nw, nphi, np.abs(wv - wr), wbar, np.abs(ov.real - orf.real), bre, np.abs(ov.imag - orf.imag), bim))
    assert np.all(np.abs(wv - wr) <= wbar)
    assert np.all(np.abs(ov.real - orf.real) <= bre)
    assert np.all(np.abs(ov.imag - orf.imag) <= bim)
    out_b, n2_b, wv_b, ov_b = ctx.prop_combine_obs(Q, c, W, phi)
    assert np.array_equal(out, out_b) and n2 == n2_b and np.array_equal(wv, wv_b) and np.array_equal(ov, ov_b)


def test_combine_obs_caps(cal, ctx):
    n, m = 257, 3
    rng = np.random.RandomState(5)
    Q, c = np.asfortranarray(rng.randn(2 * n, m)), rng.randn(m) + 1j * rng.randn(m)
    with pytest.raises(cal.CalError):
        ctx.prop_combine_obs(Q, c, rng.randn(n, 5), None)
    with pytest.raises(cal.CalError):
        ctx.prop_combine_obs(Q, c, None, rng.randn(n, 5) + 0j)
    out, n2, wv, ov = ctx.prop_combine_obs(Q, c, None, None)  # nothing set: the plain results
    plain, n2p = ctx.prop_combine(Q, c)
    assert np.array_equal(out, plain) and n2 == n2p and wv.size == 0 and ov.size == 0


@pytest.mark.parametrize("m", [1, 24])
@pytest.mark.parametrize("n", [1, 2, 3, 257, 1025])
def test_combine_obs_without_observables_is_the_plain_kernel(ctx, n, m):
    """No W and no phi: the sweep takes the kernel without observables, and
    out and norm2 are the plain entry's to the bit (the odd last row, the
    unaligned lower half, more than one block)."""
    rng = np.random.RandomState(7000 * m + n)
    Q = np.asfortranarray(rng.randn(2 * n, m))
    c = rng.randn(m) + 1j * rng.randn(m)
    out, n2, wv, ov = ctx.prop_combine_obs(Q, c)
    plain, n2p = ctx.prop_combine(Q, c)
    assert np.array_equal(out, plain) and n2 == n2p
    assert wv.shape == (0,) and ov.shape == (0,)


# ---- 2. - 4. the oscillator: one run with observables, one without -------------------------
S, BLOCKS, STEPS, DT = 6, 4, 8, 0.025
_runs = {}


def oscillator_runs(cal, N):
    if N in _runs:
        return _runs[N]
    H, psi0, x, _, _ = pref.oscillator(N)
    W = np.column_stack([x, x * x])
    phi = psi0.astype(complex).reshape(-1, 1)
    res = {}
    for name in ("obs", "plain"):
        P = cal.Propagator(H, psi0, S, BLOCKS, basis="newton")
        try:
            if name == "obs":
                P.set_observables(W=[x, x * x], phi=[psi0], energy=True)
            assert P.step(DT, STEPS) == 0
            info = P.info()
            info.pop("ms")  # wall time
            res[name] = dict(state=P.state(), info=info, hist=P.observables())
        finally:
            P.close()
    res.update(H=H, psi0=psi0, W=W, phi=phi)
    _runs[N] = res
    return res


def rows(hist):
    """The history dict as the C rows [t, norm2, E, W.., Re, Im, ..]."""
    ov = hist["overlap"]
    ri = np.empty((ov.shape[0], 2 * ov.shape[1]))
    ri[:, 0::2], ri[:, 1::2] = ov.real, ov.imag
    return np.column_stack([hist["t"], hist["norm2"], hist["energy"], hist["W"], ri])


@pytest.mark.parametrize("N", [256, 255])
def test_observables_do_not_disturb_the_run(cal, N):
    r = oscillator_runs(cal, N)
    assert np.array_equal(r["obs"]["state"], r["plain"]["state"])
    a, b = r["obs"]["info"], r["plain"]["info"]
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["steps"] == STEPS
    assert r["plain"]["hist"]["t"].size == 0  # nothing set: no rows


@pytest.mark.parametrize("N", [256, 255])
def test_values_against_the_device_state(cal, N):
    r = oscillator_runs(cal, N)
    h = r["obs"]["hist"]
    assert h["t"].shape == (STEPS,) and h["W"].shape == (STEPS, 2) and h["overlap"].shape == (STEPS, 1)
    pref.check_row(rows(h)[-1], r["H"], r["obs"]["state"], r["W"], r["phi"])
    nrm = r["obs"]["info"]["norm"]
    assert abs(h["norm2"][-1] - nrm ** 2) <= 4 * EPS * nrm ** 2
    assert abs(h["t"][-1] - STEPS * DT) <= 8 * EPS * STEPS * DT


@pytest.mark.parametrize("N", [256, 255])
def test_values_against_the_exact_solution(cal, N):
    r = oscillator_runs(cal, N)
    h = r["obs"]["hist"]
    H, W, phi = r["H"], r["W"], r["phi"]
    _, psi0, _, ew, U = pref.oscillator(N)
    ebars = []
    for k in range(1, STEPS + 1):
        we, oe, Ee = pref.exact_observables(N, W, phi, k * DT)
        pw, po, pe = pref.physics_bars(N, W, phi, k)
        pk = pref.exact(ew, U, psi0, k * DT)  # the rounding bars' S: from the exact state
        _, wbar = pref.w_ref(W, pk)
        _, bre, bim = pref.overlap_ref(phi, pk)
        _, ebar = pref.energy_ref(H, pk)
        dw = np.abs(h["W"][k - 1] - we)
        do = h["overlap"][k - 1, 0] - oe[0]
        dE = abs(h["energy"][k - 1] - Ee)
        print("N=%d step %d: |dW| %s (bar %s), |d overlap| %.3e, %.3e (bar %.3e), |dE| %.3e (bar %.3e)"
              % (N, k, dw, pw + wbar, abs(do.real), abs(do.imag), po[0] + bre[0], dE, pe + ebar))
        assert np.all(dw <= pw + wbar)
        assert abs(do.real) <= po[0] + bre[0] and abs(do.imag) <= po[0] + bim[0]
        assert dE <= pe + ebar
        ebars.append(pe + ebar)
    assert np.max(h["energy"]) - np.min(h["energy"]) <= 2 * max(ebars)


@pytest.mark.parametrize("N", [256, 255])
def test_energy_alone_does_not_disturb_the_run(cal, N):
    """set_observables(energy=True) alone: the combine is the plain kernel's,
    so the state has the bits of a run without observables, and every row
    holds to the derived bars with no W and no phi."""
    H, psi0, _, _, _ = pref.oscillator(N)
    none = np.zeros((N, 0))
    states = {}
    for name in ("energy", "plain"):
        P = cal.Propagator(H, psi0, S, BLOCKS, basis="newton")
        try:
            if name == "energy":
                P.set_observables(energy=True)
            states[name] = []
            for _ in range(3):
                assert P.step(DT, 1) == 0
                states[name].append(P.state())
            hist = P.observables()
        finally:
            P.close()
        if name == "energy":
            h = rows(hist)
    assert h.shape == (3, 3)
    for k in range(3):
        assert np.array_equal(states["energy"][k], states["plain"][k])
        pref.check_row(h[k], H, states["energy"][k], none, none, energy=True)


# ---- 5. split-format Hamiltonian, complex state --------------------------------------------
def test_split_format_complex_state(cal):
    N = 17
    H = lap3d_v(cal, N)
    n = H.shape[0]
    V = potential((N, N, N))
    idx = np.arange(n)
    coords = [(idx // N ** d) % N for d in range(3)]
    r2 = sum((c - 0.5 * (N - 1)) ** 2 for c in coords)
    psi0 = np.exp(-r2 / (2 * 3.0 ** 2)) * np.exp(1j * (0.7 * coords[0] + 0.3 * coords[1] + 0.2 * coords[2]))
    assert np.max(np.abs(psi0.imag)) > 0.5
    hist, last = {}, {}
    for fmt in ("split", "csr"):
        c = cal.Context(spmv_format=fmt)
        try:
            P = cal.Propagator(H, psi0, 6, 4, ctx=c)
            assert c.spmv_split_info()[0] is (fmt == "split")
            P.set_observables(W=[V], phi=[psi0], energy=True)
            assert P.step(0.02, 4) == 0
            hist[fmt], last[fmt] = rows(P.observables()), P.state()
            P.close()
        finally:
            c.close()
    assert hist["split"].shape == (4, 6)
    assert np.array_equal(hist["split"], hist["csr"])
    assert np.array_equal(last["split"], last["csr"])
    pref.check_row(hist["split"][-1], H, last["split"], V.reshape(-1, 1), psi0.reshape(-1, 1))


# ---- 6. history bookkeeping -------------------------------------------------------------------
def test_history_bookkeeping(cal):
    N, dt = 256, 0.025
    H, psi0, x, _, _ = pref.oscillator(N)
    P = cal.Propagator(H, psi0, S, BLOCKS)
    try:
        h = P.observables()
        assert h["t"].size == 0 and h["W"].shape == (0, 0) and h["overlap"].shape == (0, 0)
        P.step(dt, 1)
        assert P.observables()["t"].size == 0  # nothing set: no rows
        P.set_observables(W=[x], phi=[psi0, 1j * psi0], energy=False)
        P.step(dt, 3)
        P.step(dt, 2)
        h = P.observables()
        assert h["t"].shape == (5,) and h["W"].shape == (5, 1) and h["overlap"].shape == (5, 2)
        # t counts from the start of the propagation: one step was taken before the set
        assert np.all(np.abs(h["t"] - dt * np.arange(2, 7)) <= 8 * EPS * dt * 6)
        assert np.all(np.isnan(h["energy"]))
        assert np.array_equal(h["overlap"][:, 1], -1j * h["overlap"][:, 0])  # <i phi|psi> = -i <phi|psi>
        part = P.observables(first=1, count=3)
        for k in ("t", "norm2", "W", "overlap"):
            assert np.array_equal(part[k], h[k][1:4]), k
        with pytest.raises(cal.CalError):
            P.observables(first=3, count=3)
        P.set_observables(W=[x], energy=True)  # again: the history is cleared
        assert P.observables()["t"].size == 0
        P.step(dt, 1)
        h = P.observables()
        assert h["t"].size == 1 and np.isfinite(h["energy"][0]) and h["overlap"].shape == (1, 0)
        P.set_observables()  # off
        P.step(dt, 1)
        assert P.observables()["t"].size == 0
        with pytest.raises(cal.CalError):
            P.set_observables(W=[x] * 5)
        with pytest.raises(cal.CalError):
            P.set_observables(phi=[psi0] * 5)
    finally:
        P.close()
    with pytest.raises(cal.CalError):
        P.set_observables(W=[x])


def test_history_starts_at_dt(cal):
    N, dt = 255, 0.025
    H, psi0, x, _, _ = pref.oscillator(N)
    P = cal.Propagator(H, psi0, S, BLOCKS)
    try:
        P.set_observables(W=[x])
        P.step(dt, 3)
        P.step(dt, 2)
        t = P.observables()["t"]
        assert t.shape == (5,) and np.all(np.abs(t - dt * np.arange(1, 6)) <= 8 * EPS * dt * 5)
    finally:
        P.close()


# ---- 7. an unfused format: the energy's SpMV + dot fallback -------------------------------------
def test_energy_on_an_unfused_format(cal):
    """Nine entries per row in the row-pattern format (test_gpu_lanczos_std.py):
    the row kernels have no fused Lanczos mode."""
    n = 1003
    offs = [-4, -3, -2, -1, 0, 1, 2, 3, 4]
    H = sp.diags([[-1.0] * (n - abs(o)) if o else [9.0] * n for o in offs], offs, format="csr")
    i = np.arange(n)
    psi0 = np.exp(-((i - 500.0) / 40.0) ** 2) * np.exp(0.3j * i)
    V = 0.01 * (i - 500.0)
    c = cal.Context(spmv_format="pattern")
    try:
        P = cal.Propagator(H, psi0, 6, 4, ctx=c)
        assert c.spmv_format()[0] == "pattern" and c.spmv_lanczos_fused() is False
        P.set_observables(W=[V], phi=[psi0], energy=True)
        assert P.step(0.05, 4) == 0
        h, psi = rows(P.observables()), P.state()
        P.close()
    finally:
        c.close()
    assert h.shape == (4, 6)
    pref.check_row(h[-1], H, psi, V.reshape(-1, 1), psi0.reshape(-1, 1))
