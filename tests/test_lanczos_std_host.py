"""Host-side checks of the standard Lanczos work (lanczos.m): the NumPy
restatement of the periodic / selective modes that the GPU tests compare
against, and the Python wrappers' argument checks.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lanczos_std_ref as href  # noqa: E402

EPS = np.finfo(float).eps


@pytest.mark.parametrize("orth", ["periodic", "selective"])
def test_restatement_is_local_when_no_event_fires(ref, orth):
    """lap2d_37, m = 48: neither mode fires, and the restatement's recurrence
    is the oracle's, so T and Q are ref.lanczos(..., 'local') bit for bit."""
    A = ref.laplacian_2d(37)
    r = np.random.default_rng(0).standard_normal(37 * 37)
    out = href.lanczos(A, r, 48, orth)
    Q, T, _, _ = ref.lanczos(A, r, 48, "local")
    assert out.events == []
    assert np.array_equal(out.T, T) and np.array_equal(out.Q, Q)


def test_restatement_events_on_the_diagonal_matrix():
    """The event lists the GPU test asserts (periodic: steps; selective:
    (step, locked vectors)) and how far the nearest decision is from its
    threshold."""
    A = href.diag_test_matrix()
    r = np.random.default_rng(0).standard_normal(A.shape[0])
    p = href.lanczos(A, r, 48, "periodic")
    assert p.events == [14, 21, 28, 35, 42]
    assert max(m for m in p.margins if m < 1.0) < 0.85
    s = href.lanczos(A, r, 48, "selective")
    assert s.events == [(13, 1), (15, 2), (16, 3), (17, 4)]
    assert min(s.margins) > 0.05


def test_update_omega_hand_computed():
    """lanczos.m:276-299 by hand: the 2 x 2 start, then n = 2 (3 x 3), where
    the k loop is empty and omega(3,1) takes the +T / -T branch by sign."""
    anorm = 8.0
    T = EPS * anorm
    alpha = np.array([2.0, 3.0, 1.0])
    beta = np.array([0.5, 0.25, 2.0])
    om2 = href.update_omega(None, 1, alpha, beta, anorm)
    assert np.array_equal(om2, np.array([[1.0, 0.0], [T / 0.5, 1.0]]))
    om3 = href.update_omega(om2, 2, alpha, beta, anorm)
    # omega(3,1) = beta(2)*omega(2,2) + (alpha(1)-alpha(2))*omega(2,1) - beta(2)*omega(1,1)
    v = 0.25 * 1.0 + (2.0 - 3.0) * (T / 0.5) - 0.25 * 1.0
    assert v < 0
    exp = np.zeros((3, 3))
    exp[:2, :2] = om2
    exp[2, 0] = (1.0 / 0.25) * (v - T)
    exp[2, 1] = (1.0 / 0.25) * T
    exp[2, 2] = 1.0
    assert np.array_equal(om3, exp)
    # the positive branch: alpha(1) < alpha(2) reversed
    om3p = href.update_omega(om2, 2, np.array([3.0, 2.0, 1.0]), beta, anorm)
    vp = 0.25 * 1.0 + (3.0 - 2.0) * (T / 0.5) - 0.25 * 1.0
    assert vp > 0 and om3p[2, 0] == (1.0 / 0.25) * (vp + T)
    # reset_omega rewrites rows n and n + 1
    rs = href.reset_omega(om3, 2, anorm)
    assert np.array_equal(rs, np.array([[1.0, 0.0, 0.0], [T, 1.0, 0.0], [T, T, 1.0]]))


def test_wrappers_reject_bad_orth_before_the_library(cal, monkeypatch):
    """lanczos / lanczos_ex / Context.std_lanczos_begin raise ValueError on an
    unknown orth without a context or a library call, as ca_lanczos does."""
    from ca_lanczos_amd import api

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(api, "context_for", boom)
    A = cal.matrices.laplacian_2d(4)
    r = np.ones(16)
    for bad in ("fro", "", "Localx", 3):
        with pytest.raises(ValueError):
            cal.lanczos(A, r, 4, bad)
        with pytest.raises(ValueError):
            cal.lanczos_ex(A, r, 4, bad)
    ctx = object.__new__(api.Context)  # no device: the check comes first
    ctx.h = None
    with pytest.raises(ValueError):
        api.Context.std_lanczos_begin(ctx, r, 4, "nope")


def test_new_symbols_are_exported_and_bound(cal):
    from ca_lanczos_amd import _lib

    bound = {s[0] for s in _lib.SIGNATURES}
    for name in ("cal_lanczos", "cal_std_lanczos_begin", "cal_std_lanczos_step", "cal_std_lanczos_get",
                 "cal_std_lanczos_get_Q", "cal_std_lanczos_end", "cal_spmv_lanczos"):
        assert name in bound and hasattr(_lib.lib, name)
    assert callable(cal.lanczos) and callable(cal.lanczos_ex)
    assert math.isclose(_lib.CAL_WARN_BREAKDOWN, 2)
