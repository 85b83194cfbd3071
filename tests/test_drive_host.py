"""Host side of the time-dependent potential H(t) = H0 + sum_k f_k(t) diag(W_k)
(CPU only).

  * the five entry points (cal_set_diagonal, cal_get_diagonal,
    cal_prop_set_drive, cal_prop_step_driven, cal_prop_refresh_shifts) are
    exported by the built library and bound in _lib.py, the Python methods
    exist, and every entry returns CAL_ERR_ARG for a null context.
  * the schemes of Propagator.step (api.drive_rows: which amplitudes a callable
    drive is sampled to) converge at their order.  The rows drive the NumPy
    stacked-real-Lanczos propagator of tests/drive_ref.py (m = 24) on the
    oscillator (N = 256, W = [x], f(t) = 2 sin 3t) over T = 0.2; each scheme is
    held against the dense exponentials of the same rule at dt / 8.
  * Context.set_diagonal on a context handed out by context_for(A) is refused:
    that cache pairs the device copy with the SciPy object.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drive_ref as dref  # noqa: E402

NAMES = ("cal_set_diagonal", "cal_get_diagonal", "cal_prop_set_drive", "cal_prop_step_driven",
         "cal_prop_refresh_shifts")


def test_entry_points_exported_and_bound(cal):
    from ca_lanczos_amd import _lib
    image = ctypes.CDLL(cal.LIB_PATH)
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(image, name), name
        assert name in bound, name
    for name in ("set_diagonal", "get_diagonal"):
        assert callable(getattr(cal.Context, name, None)), name
    for name in ("set_drive", "refresh_shifts", "step"):
        assert callable(getattr(cal.Propagator, name, None)), name


def test_no_context_is_an_argument_error(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    one = np.ones(2)
    assert lib.cal_set_diagonal(None, 2, ptr(one)) == CAL_ERR_ARG
    assert lib.cal_get_diagonal(None, 2, ptr(one)) == CAL_ERR_ARG
    assert lib.cal_prop_set_drive(None, 1, ptr(one)) == CAL_ERR_ARG
    assert lib.cal_prop_set_drive(None, 0, None) == CAL_ERR_ARG
    assert lib.cal_prop_step_driven(None, 0.1, 1e-10, 0, 1, ptr(one), 1) == CAL_ERR_ARG
    assert lib.cal_prop_refresh_shifts(None) == CAL_ERR_ARG


# ---- the schemes ---------------------------------------------------------------------
def test_drive_rows_shapes_and_coefficients(cal):
    r3 = np.sqrt(3.0)
    rows, sub = cal.drive_rows(np.arange(6.0).reshape(3, 2), 0.0, 0.1, 3)
    assert sub == 0.1 and np.array_equal(rows, np.arange(6.0).reshape(3, 2)) and rows.flags.c_contiguous
    rows, sub = cal.drive_rows(lambda t: [t, 2 * t], 1.0, 0.1, 3, "midpoint")
    assert sub == 0.1 and rows.shape == (3, 2)
    assert np.allclose(rows[:, 0], [1.05, 1.15, 1.25], rtol=0, atol=1e-15) and np.array_equal(rows[:, 1], 2 * rows[:, 0])
    rows, sub = cal.drive_rows(lambda t: t, 1.0, 0.1, 2, "cf4")
    assert sub == 0.05 and rows.shape == (4, 1)
    # a linear f: both factors' amplitudes are f at their own combination of the Gauss points
    t1, t2 = 1.0 + (0.5 - r3 / 6) * 0.1, 1.0 + (0.5 + r3 / 6) * 0.1
    a1, a2 = 0.5 + r3 / 3, 0.5 - r3 / 3
    assert np.allclose(rows[:2, 0], [a1 * t1 + a2 * t2, a2 * t1 + a1 * t2], rtol=0, atol=1e-15)
    assert abs(rows[0, 0] + rows[1, 0] - 2 * 1.05) < 1e-15  # the two factors average to the midpoint
    with pytest.raises(ValueError):
        cal.drive_rows(lambda t: t, 0.0, 0.1, 2, "rk4")
    with pytest.raises(ValueError):
        cal.drive_rows(np.zeros((2, 1)), 0.0, 0.1, 3)


def _scheme_error(cal, scheme, dt, T):
    H, psi0, x, _, _ = dref.oscillator(256)
    n = int(round(T / dt))
    rows, sub = cal.drive_rows(dref.f_one, 0.0, dt, n, scheme)
    psi = dref.propagate_driven_numpy(H, [x], psi0, rows, sub, m=24)
    fine, fsub = cal.drive_rows(dref.f_one, 0.0, dt / 8, 8 * n, scheme)
    ref = dref.dense_driven(H, [x], psi0, fine, fsub)
    # the Krylov floor of these very rows, for the docstring's claim
    floor = np.linalg.norm(psi - dref.dense_driven(H, [x], psi0, rows, sub))
    return np.linalg.norm(psi - ref), floor


def test_midpoint_is_second_order(cal):
    """Error against the same rule at dt / 8, over T = 0.2: the ratio between
    dt = 0.05 and dt = 0.025 lies in [3, 5] (second order: 4)."""
    e1, fl1 = _scheme_error(cal, "midpoint", 0.05, 0.2)
    e2, fl2 = _scheme_error(cal, "midpoint", 0.025, 0.2)
    print("midpoint: err(0.05) %.3e, err(0.025) %.3e, ratio %.2f; Krylov floors %.1e %.1e" % (e1, e2, e1 / e2, fl1, fl2))
    assert max(fl1, fl2) < 1e-3 * e2
    assert 3.0 <= e1 / e2 <= 5.0


def test_cf4_is_fourth_order(cal):
    """The same for the commutator-free fourth-order rule: the ratio is at
    least 10 (fourth order: 16).  At dt = 0.05 and 0.025 the errors (printed)
    stand well above the NumPy propagator's Krylov and rounding floor (printed
    too, and asserted to be below a hundredth of the smaller error), so the
    issue's step sizes are kept."""
    e1, fl1 = _scheme_error(cal, "cf4", 0.05, 0.2)
    e2, fl2 = _scheme_error(cal, "cf4", 0.025, 0.2)
    print("cf4: err(0.05) %.3e, err(0.025) %.3e, ratio %.2f; Krylov floors %.1e %.1e" % (e1, e2, e1 / e2, fl1, fl2))
    assert max(fl1, fl2) < 1e-2 * e2
    assert e1 / e2 >= 10.0


# ---- the context_for cache -------------------------------------------------------------
def test_set_diagonal_refused_on_a_cached_context(cal, monkeypatch):
    """context_for marks the contexts it hands out and set_diagonal refuses
    them before anything reaches the library (no device is needed: the
    Context is a stand-in without a handle)."""
    from ca_lanczos_amd import api

    class Stub(api.Context):
        def __init__(self):
            self.h = None

        def set_matrix(self, A):
            return self

        def close(self):
            pass

    monkeypatch.setattr(api, "Context", Stub)
    monkeypatch.setattr(api, "_matrix_ctx", {})
    A = cal.matrices.laplacian_2d(4)
    ctx = api.context_for(A)
    assert api.context_for(A) is ctx
    with pytest.raises(cal.CalError) as e:
        ctx.set_diagonal(np.ones(16))
    assert e.value.status == api._lib.CAL_ERR_ARG and "explicit Context" in str(e.value)
    # an explicit context is not marked
    assert not getattr(Stub(), "_cached_for_matrix", False)
