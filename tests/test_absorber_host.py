"""Host side of the propagator's absorbing mask (CPU only).

  * matrices.absorber_mask: values in [0, 1], exactly 1.0 in the interior,
    symmetric, in the row order of matrices.grid_hamiltonian.
  * the scheme psi <- M .* exp(-i dt H) psi as tests/absorber_ref.py states it:
    stacked real Lanczos in NumPy (prop_obs_ref.lanczos_full, m = 24) with the
    mask after every step against the dense scheme on the oscillator, bar
    k 1e-10 after k steps (tests/test_gpu_prop.py's: the mask is <= 1 and
    amplifies no step's error).  Measured: below 6e-14 at every step.  The mask
    removes 0.6 - 0.7 % of the squared norm per step here, about 5 % in all.
  * the three entry points are exported and bound.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import absorber_ref as aref  # noqa: E402
import prop_obs_ref as pref  # noqa: E402

NAMES = ("cal_prop_set_absorber", "cal_prop_get_absorbed", "cal_prop_combine_masked")


def test_entry_points_exported_and_bound(cal):
    from ca_lanczos_amd import _lib
    image = ctypes.CDLL(cal.LIB_PATH)
    bound = {s[0] for s in _lib.SIGNATURES}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "calanczos.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert hasattr(image, name), name
        assert name in bound, name
    assert callable(getattr(cal.Propagator, "set_absorber", None))
    assert callable(getattr(cal.Propagator, "absorbed", None))
    assert callable(getattr(cal.Context, "prop_combine_masked", None))
    assert callable(getattr(cal.matrices, "absorber_mask", None))


def test_no_context_is_an_argument_error(cal):
    from ca_lanczos_amd._lib import CAL_ERR_ARG, lib, ptr
    one = np.ones(2)
    assert lib.cal_prop_set_absorber(None, None) == CAL_ERR_ARG
    assert lib.cal_prop_set_absorber(None, ptr(one)) == CAL_ERR_ARG
    nr = ctypes.c_int64()
    assert lib.cal_prop_get_absorbed(None, 0, 0, None, ctypes.byref(nr)) == CAL_ERR_ARG
    assert lib.cal_prop_combine_masked(None, 1, 1, ptr(one), ptr(one), ptr(one), ptr(one), 0, None, 0, None, None,
                                       ptr(one), ptr(one), None, None, None) == CAL_ERR_ARG


# ---- absorber_mask ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims,width", [((9,), 3), ((8, 7), 2), ((5, 4, 3), 1), ((12, 9, 10), 4), ((6, 6), 0),
                                        ((5, 5), 9)])
def test_mask_range_interior_symmetry(cal, dims, width):
    M = cal.matrices.absorber_mask(dims, width)
    assert M.shape == (int(np.prod(dims)),) and M.dtype == np.float64
    assert np.all(M >= 0.0) and np.all(M <= 1.0)
    G = M.reshape(dims, order="F")  # the first dimension is the fastest
    inner = tuple(slice(width, d - width) for d in dims)
    if all(d > 2 * width for d in dims):
        assert G[inner].size > 0 and np.all(G[inner] == 1.0)  # exactly
        edge = np.ones(dims, dtype=bool)
        edge[inner] = False
        assert np.all(G[edge] < 1.0)
    for ax in range(len(dims)):
        assert np.array_equal(G, np.flip(G, axis=ax))
    assert np.array_equal(M, M[::-1])


def test_mask_profile(cal):
    """One axis: cos(pi/2 r)^power with r = (width - e)/width, e the distance to the nearer end."""
    M = cal.matrices.absorber_mask((11,), 4, power=0.25)
    r = np.array([1.0, 0.75, 0.5, 0.25, 0, 0, 0, 0.25, 0.5, 0.75, 1.0])
    exp = np.cos(0.5 * np.pi * r) ** 0.25
    assert np.max(np.abs(M - exp)) <= 4 * np.finfo(float).eps
    assert M[0] < 0.02 and np.all(np.diff(M[:5]) > 0)
    M2 = cal.matrices.absorber_mask((11, 6), 4, power=0.25)
    m6 = cal.matrices.absorber_mask((6,), 4, power=0.25)
    assert np.array_equal(M2.reshape((11, 6), order="F"), np.multiply.outer(M, m6))
    with pytest.raises(ValueError):
        cal.matrices.absorber_mask((5, 5), -1)


def test_mask_ordering_matches_grid_hamiltonian(cal):
    """On a non-cubic grid: with width 1 the mask is below 1 exactly on the
    points that lack a neighbour in grid_hamiltonian's Dirichlet stencil, and
    the points it damps along axis k alone are those that lack the neighbour
    at the column offset of axis k."""
    dims = (5, 4, 3)
    n = int(np.prod(dims))
    H = cal.matrices.grid_hamiltonian(dims, np.zeros(n))
    M = cal.matrices.absorber_mask(dims, 1)
    full = np.diff(H.indptr) == 2 * len(dims) + 1
    assert 0 < full.sum() < n
    assert np.array_equal(M == 1.0, full)
    D = H.toarray() != 0
    i = np.arange(n)
    stride = 1
    for k, d in enumerate(dims):
        lower = np.array([r - stride < 0 or not D[r, r - stride] for r in i])
        upper = np.array([r + stride >= n or not D[r, r + stride] for r in i])
        one = [1] * len(dims)
        one[k] = d
        axis_only = cal.matrices.absorber_mask((d,), 1)  # the factor of axis k
        Mk = np.ones(dims)
        Mk *= axis_only.reshape(one)
        assert np.array_equal(Mk.ravel(order="F") < 1.0, lower | upper), k
        stride *= d


# ---- the scheme in NumPy against the dense scheme --------------------------------------------------
@pytest.mark.parametrize("N", [256, 255])
def test_numpy_lanczos_with_mask_against_dense_scheme(N):
    steps, dt = 8, 0.025
    H, psi0, x, _, _ = pref.oscillator(N)
    M = aref.oscillator_mask(x)
    assert np.all(M >= 0.0) and np.all(M <= 1.0) and np.all(M[np.abs(x) <= 3.0] == 1.0) and M.min() < 0.6
    states, ab = aref.propagate_numpy_masked(H, psi0.astype(complex), M, dt, steps, m=24)
    dense, us, dab = aref.dense_scheme(N, M, dt, steps)
    n2 = np.sum(np.abs(psi0) ** 2)
    for k in range(1, steps + 1):
        err = np.linalg.norm(states[k - 1] - dense[k - 1])
        frac = dab[k - 1] / np.sum(np.abs(us[k - 1]) ** 2)
        print("N=%d step %d: |numpy - dense| %.3e (bar %.1e), absorbed %.6e (dense %.6e), fraction %.4f"
              % (N, k, err, k * 1e-10, ab[k - 1], dab[k - 1], frac))
        assert err <= k * 1e-10
        # a state within e of the dense one: |absorbed - dense| <= 2 ||u|| e, plus the sum's rounding
        u = us[k - 1]
        terms = (1.0 - M * M) * np.abs(u) ** 2
        assert abs(ab[k - 1] - dab[k - 1]) <= 2 * np.linalg.norm(u) * k * 1e-10 + aref.absorbed_bar(terms)
        assert 0.004 <= frac <= 0.01  # the mask is no no-op on this input
    left = np.sum(np.abs(dense[-1]) ** 2) / n2
    assert 0.93 <= left <= 0.97
    # what the mask removes is what the norm loses (unitary steps)
    assert abs(n2 - np.sum(np.abs(dense[-1]) ** 2) - np.sum(dab)) <= 1e-12 * n2


def test_masked_ref_chain():
    """The chain of absorber_ref.masked_ref: ones change nothing and absorb nothing, zeros remove the row."""
    rng = np.random.RandomState(3)
    top, bot = rng.randn(33), rng.randn(33)
    t, b, terms = aref.masked_ref(top, bot, np.ones(33))
    assert np.array_equal(t, top) and np.array_equal(b, bot) and not terms.any()
    M = (rng.rand(33) < 0.5).astype(float)
    t, b, terms = aref.masked_ref(top, bot, M)
    assert not t[M == 0].any() and np.array_equal(t[M == 1], top[M == 1])
    assert np.array_equal(terms[M == 0], (top * top + bot * bot)[M == 0]) and not terms[M == 1].any()
