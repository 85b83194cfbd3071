"""Host side of the propagator's device-side observables (CPU only).

  * the three entry points (cal_prop_set_observables, cal_prop_get_observables,
    cal_prop_combine_obs) are exported by the built library and bound in
    _lib.py, Propagator has set_observables / observables, Context has
    prop_combine_obs; without a context the entries return CAL_ERR_ARG.
  * the NumPy references of tests/prop_obs_ref.py (the GPU tests' yardstick)
    against dense formulas: the oscillator of tests/test_gpu_prop.py (N = 256
    and 255, dt = 0.025, 8 steps) is propagated in NumPy by stacked real
    Lanczos (m = 24, tests/test_prop_host.py); after every step the helpers'
    <x>, <x^2>, <psi0|psi> and E of that state are held to the exact values
    from the dense eigh within the physics bars of a state 1e-10 per step
    away plus the helpers' rounding bars.  The NumPy propagation itself is
    within 1e-13 of the exact state, four orders inside those bars.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prop_obs_ref as pref  # noqa: E402

NAMES = ("cal_prop_set_observables", "cal_prop_get_observables", "cal_prop_combine_obs")


def test_entry_points_exported_and_bound(cal):
    from ca_lanczos_amd import _lib
    image = ctypes.CDLL(cal.LIB_PATH)
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(image, name), name
        assert name in bound, name
    assert callable(getattr(cal.Propagator, "set_observables", None))
    assert callable(getattr(cal.Propagator, "observables", None))
    assert callable(getattr(cal.Context, "prop_combine_obs", None))


def test_no_context_is_an_argument_error(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    one = np.ones(2)
    assert lib.cal_prop_set_observables(None, 0, None, 0, None, None, 0) == CAL_ERR_ARG
    assert lib.cal_prop_set_observables(None, 1, ptr(one), 0, None, None, 1) == CAL_ERR_ARG
    nr, nc = ctypes.c_int64(), ctypes.c_int()
    assert lib.cal_prop_get_observables(None, 0, 0, None, ctypes.byref(nr), ctypes.byref(nc)) == CAL_ERR_ARG
    assert lib.cal_prop_combine_obs(None, 1, 1, ptr(one), ptr(one), ptr(one), 0, None, 0, None, None, ptr(one),
                                    ptr(one), None, None) == CAL_ERR_ARG


def test_obs_arrays_shapes(cal):
    from ca_lanczos_amd.api import _obs_arrays
    n = 5
    x = np.arange(n, dtype=float)
    W, pr, pi = _obs_arrays(n, [x, x * x], [x + 2j * x])
    assert W.shape == (n, 2) and W.flags.f_contiguous and np.array_equal(W[:, 1], x * x)
    assert pr.shape == (n, 1) and np.array_equal(pr[:, 0], x) and np.array_equal(pi[:, 0], 2 * x)
    W, pr, pi = _obs_arrays(n, None, np.ones((n, 3)))
    assert W.shape == (n, 0) and pr.shape == (n, 3) and not pi.any()
    W, pr, pi = _obs_arrays(n, x, None)
    assert W.shape == (n, 1) and pr.shape == (n, 0) and pi.shape == (n, 0)
    with pytest.raises(ValueError):
        _obs_arrays(n, [np.ones(n + 1)], None)


@pytest.mark.parametrize("N", [256, 255])
def test_helpers_against_dense_formulas(N):
    steps, dt = 8, 0.025
    H, psi0, x, ew, U = pref.oscillator(N)
    W = np.column_stack([x, x * x])
    phi = psi0.astype(complex).reshape(-1, 1)
    states = pref.propagate_numpy(H, psi0.astype(complex), dt, steps, m=24)
    err = np.linalg.norm(states[-1] - pref.exact(ew, U, psi0, steps * dt))
    print("N=%d NumPy propagation error %.3e" % (N, err))
    assert err <= 1e-12
    for k, psi in enumerate(states, start=1):
        wv, wbar = pref.w_ref(W, psi)
        ov, bre, bim = pref.overlap_ref(phi, psi)
        E, ebar = pref.energy_ref(H, psi)
        we, oe, Ee = pref.exact_observables(N, W, phi, k * dt)
        pw, po, pe = pref.physics_bars(N, W, phi, k)
        # the dense formulas, written independently of the helpers
        Hd = H.toarray()
        assert abs(E - np.real(np.vdot(psi, Hd @ psi))) <= ebar
        assert np.all(np.abs(wv - np.array([np.vdot(psi, x * psi).real, np.vdot(psi, x * x * psi).real])) <= wbar)
        assert abs(ov[0] - np.vdot(psi0, psi)) <= bre[0] + bim[0]
        assert np.all(np.abs(wv - we) <= pw + wbar), (k, wv, we)
        assert abs(ov[0].real - oe[0].real) <= po[0] + bre[0] and abs(ov[0].imag - oe[0].imag) <= po[0] + bim[0]
        assert abs(E - Ee) <= pe + ebar, (k, E, Ee)
    # sanity of the definitions: <x>(t) of the packet displaced by 4 in the harmonic well is 4 cos t in the
    # continuum; the fourth-order stencil at h = 20 / N is within h^4 ~ 4e-5 of it per unit frequency
    # (psi0 is normalised in the continuum, so the grid sums carry 1 / h: take the ratio)
    mean_x = pref.w_ref(W, states[-1])[0][0] / np.sum(np.abs(states[-1]) ** 2)
    assert abs(mean_x - 4.0 * np.cos(steps * dt)) < 1e-3
