"""Host side of the nonlinear term g |psi|^2 (CPU only).

  * cal_prop_set_nonlinear and cal_prop_get_nonlinear are exported by the built
    library and bound in _lib.py, Propagator.set_nonlinear / nonlinear exist,
    and both entries return CAL_ERR_ARG for a null context.
  * the order of the two schemes (tests/nonlinear_ref.py, dense exponentials) on
    the oscillator (N = 256) over T = 0.2: the reference is the midpoint scheme
    at dt = 0.05/32, the error ratios are taken between dt = 0.05, 0.025 and
    0.0125, for g = 1.0 and g = -0.5, each with and without the drive
    2 sin(3t) x sampled at the step's midpoint.  "frozen" is first order (ratio
    2, asserted in [1.6, 2.4]); "midpoint" second (ratio 4, asserted in
    [3.4, 4.6]).  The margins are what the measured ratios (1.90 - 2.01 and
    3.95 - 4.06) leave towards the neighbouring order.
  * the NumPy Lanczos variant of the reference (m = 24) follows the dense one
    far below the bars of the GPU tests.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drive_ref as dref  # noqa: E402
import nonlinear_ref as nref  # noqa: E402

NAMES = ("cal_prop_set_nonlinear", "cal_prop_get_nonlinear")


def test_entry_points_exported_and_bound(cal):
    from ca_lanczos_amd import _lib
    image = ctypes.CDLL(cal.LIB_PATH)
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(image, name), name
        assert name in bound, name
    for name in ("set_nonlinear", "nonlinear"):
        assert callable(getattr(cal.Propagator, name, None)), name


def test_no_context_is_an_argument_error(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    out = np.zeros(2)
    nr = ctypes.c_int64()
    assert lib.cal_prop_set_nonlinear(None, 1.0, b"midpoint") == CAL_ERR_ARG
    assert lib.cal_prop_set_nonlinear(None, 0.0, b"frozen") == CAL_ERR_ARG
    assert lib.cal_prop_get_nonlinear(None, 0, 0, ptr(out), ctypes.byref(nr)) == CAL_ERR_ARG


def test_density_chain_order_is_observable():
    rng = np.random.RandomState(3)
    n = 257
    V0, W, f = rng.randn(n), [rng.randn(n), 100.0 * rng.randn(n)], rng.randn(2)
    A, B = rng.randn(n) + 1j * rng.randn(n), rng.randn(n) + 1j * rng.randn(n)
    one = nref.density_chain(V0, W, f, 0.75, A)
    two = nref.density_chain(V0, W, f, 0.375, A, 0.375, B)
    assert np.allclose(one, V0 + f[0] * W[0] + f[1] * W[1] + 0.75 * np.abs(A) ** 2, rtol=1e-13, atol=1e-13)
    assert np.allclose(two, V0 + f[0] * W[0] + f[1] * W[1] + 0.375 * (np.abs(A) ** 2 + np.abs(B) ** 2),
                       rtol=1e-13, atol=1e-13)
    assert not np.array_equal(two, V0 + (f[0] * W[0] + f[1] * W[1]) + 0.375 * (np.abs(A) ** 2 + np.abs(B) ** 2))
    assert np.array_equal(nref.density_chain(V0, [], [], 0.0, A), V0 + 0.0)


# ---- the order of the schemes -------------------------------------------------------------
T_END = 0.2


def _rows(dt, driven):
    n = int(round(T_END / dt))
    if not driven:
        return np.zeros((n, 0))
    return np.array([dref.f_one((j + 0.5) * dt) for j in range(n)])


@functools.lru_cache(maxsize=None)
def _fine(g, driven):
    H, psi0, x, _, _ = nref.oscillator(256)
    dt = 0.05 / 32
    return nref.dense_nonlinear(H, [x] if driven else [], psi0, _rows(dt, driven), dt, g, "midpoint")


def _errors(g, driven, density):
    H, psi0, x, _, _ = nref.oscillator(256)
    ref = _fine(g, driven)
    out = []
    for dt in (0.05, 0.025, 0.0125):
        psi = nref.dense_nonlinear(H, [x] if driven else [], psi0, _rows(dt, driven), dt, g, density)
        out.append(np.linalg.norm(psi - ref))
    return out


@pytest.mark.parametrize("driven", [False, True])
@pytest.mark.parametrize("g", [1.0, -0.5])
def test_order_of_the_schemes(g, driven):
    for density, lo, hi in (("frozen", 1.6, 2.4), ("midpoint", 3.4, 4.6)):
        e = _errors(g, driven, density)
        r1, r2 = e[0] / e[1], e[1] / e[2]
        print("g=%g driven=%s %s: errors %.3e %.3e %.3e, ratios %.2f %.2f" % (g, driven, density, e[0], e[1], e[2], r1, r2))
        assert lo <= r1 <= hi and lo <= r2 <= hi, (density, r1, r2)


def test_the_term_is_not_a_perturbation():
    """With g = 1 the state at T = 0.2 differs from the linear one by about 0.55
    in the 2-norm: the ratios above are those of the nonlinear part."""
    H, psi0, _, ew, U = nref.oscillator(256)
    d = np.linalg.norm(_fine(1.0, False) - nref.pref.exact(ew, U, psi0, T_END))
    print("||psi_g=1 - psi_linear|| at T = 0.2: %.3f" % d)
    assert d > 0.3


@pytest.mark.parametrize("density", ["frozen", "midpoint"])
def test_numpy_lanczos_follows_the_dense_scheme(density):
    """The stacked-real-Lanczos variant (m = 24) against the dense one on the
    GPU tests' run (dt = 0.025, 8 steps, driven, g = 1): within a hundredth of
    the GPU tests' smallest bar, 8 builds x 1e-10, in error and in norm drift."""
    H, psi0, x, _, _ = nref.oscillator(256)
    rows = np.array([dref.f_one((j + 0.5) * 0.025) for j in range(8)])
    a = nref.dense_nonlinear(H, [x], psi0, rows, 0.025, 1.0, density)
    b = nref.lanczos_nonlinear(H, [x], psi0, rows, 0.025, 1.0, density)
    err, drift = np.linalg.norm(a - b), abs(np.linalg.norm(b) - np.linalg.norm(psi0))
    print("%s: NumPy Lanczos vs dense %.3e, drift %.3e" % (density, err, drift))
    assert err <= 8e-12 and drift <= 8e-12
