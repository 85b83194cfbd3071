"""The shared stacked SpMV format (``spmv_format="shared"``, kernel k_spmv_stacked, HERM false):
blkdiag(H, H) with H stored once.

Everything here compares a "shared" context against a "csr" context given the
same H through ``set_matrix_stacked``; the SpMV is also compared against the
NumPy emulation of the CSR kernel's arithmetic (products rounded, then each row
summed sequentially from +0.0 in stored order).

Bars:
  * y of every SpMV mode: ``array_equal`` (the order contract: each half's rows
    are summed as the stacked CSR kernel sums them).
  * the fused Lanczos dot: the two contexts agree to the bit where the stacked
    CSR row blocks do not straddle row n (the Hamiltonian of 1024 rows: four
    seam-aligned blocks per half).  Elsewhere the block partials are cut at
    other rows, so the dot is held to the project's summation bar: a float sum
    of N products whose absolute values sum to S is within (N + 8) eps S of the
    exact sum in any order (tests/prop_obs_ref.py); N = 2n, the exact sum is
    math.fsum of the device's own y .* x.
  * the propagator: bit-identical state, norm, observables and absorbed rows on
    the Hamiltonian; on the periodic oscillator of the reference's
    runLanczos.m the state is within 5e-14 of the csr context's (the bar of
    tests/test_prop_host.py against the dense exponential, applied between the
    two contexts).
"""
import math
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_cases import hamiltonian_2d, lap3d_v  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
CAL_ERR_ARG = -1
CAL_ERR_UNSUPPORTED = -6


# ---- matrices: symmetric, all values distinct ------------------------------------------
def canon(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    return A


def sym_from_upper(n, i, j, seed):
    """Symmetric CSR with the entries (i, j), i <= j, and their mirrors; every
    upper entry gets a value of its own (distinct absolute values)."""
    rng = np.random.RandomState(seed)
    key = np.unique(np.asarray(i, dtype=np.int64) * n + np.asarray(j, dtype=np.int64))
    i, j = key // n, key % n
    m = len(key)
    v = (1.0 + (rng.permutation(m) + 1.0) / (m + 1.0)) * rng.choice([-1.0, 1.0], m)
    off = i != j
    rows = np.concatenate([i, j[off]])
    cols = np.concatenate([j, i[off]])
    vals = np.concatenate([v, v[off]])
    return canon(sp.coo_matrix((vals, (rows, cols)), shape=(n, n)))


def rand_sparse(n, seed=0, full_diag=False):
    """(a): rows of 0..12 entries, empty rows, rows without a stored diagonal."""
    rng = np.random.RandomState(1000 + n + seed)
    i, j = [], []
    for _ in range(6):  # six permutations: at most 12 off-diagonals per row
        p = rng.permutation(n)
        keep = rng.rand(n) < 0.6
        a, b = np.arange(n)[keep], p[keep]
        i.append(np.minimum(a, b))
        j.append(np.maximum(a, b))
    i, j = np.concatenate(i), np.concatenate(j)
    ok = i != j
    i, j = i[ok], j[ok]
    empty = rng.rand(n) < 0.05 if n > 3 else np.zeros(n, dtype=bool)
    if full_diag:
        empty[:] = False
    ok = ~(empty[i] | empty[j])
    i, j = i[ok], j[ok]
    deg = np.bincount(np.concatenate([i, j]), minlength=n)
    diag = (deg < 12) & ~empty & ((rng.rand(n) < 0.67) | full_diag)
    if n <= 3:
        diag[0] = True
    d = np.nonzero(diag)[0]
    H = sym_from_upper(n, np.concatenate([i, d]), np.concatenate([j, d]), seed + n)
    lens = np.diff(H.indptr)
    assert lens.max() <= 12
    if n >= 255 and not full_diag:
        assert lens.min() == 0 and np.any((H.diagonal() == 0.0) & (lens > 0))
    return H


def dense_band(n=600, half=150):
    """(b): about 300 nonzeros per row: the 2048-nonzero limit cuts the row blocks at 6 rows."""
    i = np.repeat(np.arange(n), half + 1)
    j = i + np.tile(np.arange(half + 1), n)
    ok = j < n
    H = sym_from_upper(n, i[ok], j[ok], 77)
    assert np.diff(H.indptr).max() == 2 * half + 1 and 7 * (2 * half + 1) > 2048 >= 6 * (2 * half + 1)
    return H


def long_row(n, k):
    """(c): row k and its mirror column hold n - 1 off-diagonals; every diagonal is stored."""
    o = np.delete(np.arange(n), k)
    i = np.concatenate([np.minimum(o, k), np.arange(n)])
    j = np.concatenate([np.maximum(o, k), np.arange(n)])
    H = sym_from_upper(n, i, j, 31 + k)
    assert H.indptr[k + 1] - H.indptr[k] == n > 2048
    return H


def oscillator(N):
    """The reference's runLanczos.m:15-18 restated: the periodic fourth-order
    second difference on [-10, 10) plus 0.5 x^2, and its displaced Gaussian."""
    h = 20.0 / N
    x = -10.0 + h / 2.0 + h * np.arange(N)
    e, i = np.ones(N), np.arange(N)
    H = sp.csr_matrix((4.0 * e / 3.0, (i, (i + 1) % N)), shape=(N, N)) - \
        sp.csr_matrix((e / 12.0, (i, (i + 2) % N)), shape=(N, N))
    H = (H + H.T) - sp.diags(5.0 * e / 2.0)
    H = -H / (2.0 * h * h)
    H = H + sp.diags(0.5 * x * x)
    w, displ = 0.5, 4.0
    psi = (1.0 / (np.pi * w * w)) ** 0.25 * np.exp(-0.5 * ((x - displ) / w) ** 2)
    return canon(H), psi.astype(complex), x


RAND_N = (1, 2, 3, 255, 256, 257, 513, 2051)
NAMES = ["rand%d" % n for n in RAND_N] + ["band600", "long0", "longlast", "ham2d_32", "lap3d_v41"]


def build(cal, name):
    if name.startswith("rand"):
        return rand_sparse(int(name[4:]))
    if name == "band600":
        return dense_band()
    if name == "long0":
        return long_row(2051, 0)
    if name == "longlast":
        return long_row(2051, 2050)
    if name == "ham2d_32":
        return canon(hamiltonian_2d(cal, 32))
    assert name == "lap3d_v41"
    return canon(lap3d_v(cal, 41))


class Pair:
    def __init__(self, cal, H):
        self.H = H
        self.n = H.shape[0]
        self.shared = cal.Context(spmv_format="shared").set_matrix_stacked(H)
        self.csr = cal.Context(spmv_format="csr").set_matrix_stacked(H)

    def close(self):
        self.shared.close()
        self.csr.close()


@pytest.fixture(scope="module")
def pairs(cal):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pair(cal, build(cal, name))
        return made[name]

    yield get
    for p in made.values():
        p.close()


def vec(n2, seed):
    return np.random.RandomState(seed).randn(n2)


def rowsum_ref(H, x):
    """The CSR kernel's arithmetic in NumPy: rounded products, each row summed in stored order from +0.0."""
    prod = H.data * x[H.indices]
    lens = np.diff(H.indptr)
    y = np.zeros(H.shape[0])
    start = H.indptr[:-1]
    for j in range(int(lens.max()) if len(lens) else 0):
        m = lens > j
        y[m] = y[m] + prod[start[m] + j]
    return y


def stacked_ref(H, x):
    n = H.shape[0]
    return np.concatenate([rowsum_ref(H, x[:n]), rowsum_ref(H, x[n:])])


def refused(cal, code, what, fn):
    with pytest.raises(cal.CalError) as e:
        fn()
    assert e.value.status == code, (e.value.status, str(e.value))
    assert what in str(e.value), str(e.value)


# ---- 1. the format exists (fails without the feature) ---------------------------------------
@pytest.mark.parametrize("name", ["rand257", "ham2d_32"])
def test_shared_context(cal, pairs, name):
    p = pairs(name)
    assert p.shared.spmv_shared_info() == (True, p.n, p.H.nnz)
    assert p.csr.spmv_shared_info() == (False, 0, 0)
    assert p.shared.matrix_info() == p.csr.matrix_info()
    assert p.shared.matrix_info()["n_local"] == 2 * p.n and p.shared.matrix_info()["nnz_local"] == 2 * p.H.nnz
    assert p.shared.spmv_format()[0] == "csr" and p.shared.spmv_split_info()[0] is False
    assert p.shared.spmv_lanczos_fused() is True


def test_shared_takes_only_the_stacked_setter(cal):
    H = rand_sparse(257)
    ctx = cal.Context(spmv_format="shared")
    try:
        refused(cal, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_stacked", lambda: ctx.set_matrix(H))
        refused(cal, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_stacked", lambda: ctx.set_matrix_csc(H))
        refused(cal, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_stacked", lambda: ctx.set_matrix_slab(257, 0, H))
        ctx.set_matrix_stacked(H)
        assert ctx.spmv_shared_info() == (True, 257, H.nnz)
    finally:
        ctx.close()


def test_format_from_the_environment(cal, monkeypatch):
    monkeypatch.setenv("CAL_SPMV_FORMAT", "shared")
    ctx = cal.Context()
    try:
        ctx.set_matrix_stacked(rand_sparse(3))
        assert ctx.spmv_shared_info()[0] is True
    finally:
        ctx.close()


# ---- 2. y to the bit, every mode ------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_spmv_bits(cal, pairs, name):
    p = pairs(name)
    x = vec(2 * p.n, 11)
    y = p.shared.spmv(x)
    assert np.array_equal(y, p.csr.spmv(x))
    assert np.array_equal(y, stacked_ref(p.H, x))
    assert not np.any(np.signbit(y[y == 0.0]))  # an empty row's sum is +0.0


@pytest.mark.parametrize("name", NAMES)
def test_matrix_powers_bits(cal, pairs, name):
    p = pairs(name)
    s = 6
    q = vec(2 * p.n, 12) / 64.0
    real = np.array([0.5, -1.25, 2.0, 0.75, -0.5, 1.5])
    cplx = np.array([0.5, 1.0 + 0.75j, 1.0 - 0.75j, -1.25, 0.25 + 2.0j, 0.25 - 2.0j])
    got = cal.matrix_powers_monomial(None, q, s, ctx=p.shared)
    assert np.array_equal(got, cal.matrix_powers_monomial(None, q, s, ctx=p.csr))
    assert np.array_equal(got[:, 0], stacked_ref(p.H, q))
    for lam, mod in ((real, 0), (real, 1), (cplx, 1)):  # complex shifts exist in the modified (real) basis only
        a = cal.matrix_powers_newton(None, q, s, lam, mod, ctx=p.shared)
        b = cal.matrix_powers_newton(None, q, s, lam, mod, ctx=p.csr)
        assert a.shape == (2 * p.n, s + 1) and np.array_equal(a, b), (name, mod)


# ---- 2. / 3. the fused Lanczos step -----------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_spmv_lanczos_bits_and_dot(cal, pairs, name):
    p = pairs(name)
    x, xp = vec(2 * p.n, 13), vec(2 * p.n, 14)
    for xprev, b2 in ((None, 0.0), (xp, 0.7)):
        y, dot = p.shared.spmv_lanczos(x, xprev, b2)
        yc, dotc = p.csr.spmv_lanczos(x, xprev, b2)
        assert np.array_equal(y, yc)
        if xprev is None:
            assert np.array_equal(y, stacked_ref(p.H, x))
        terms = y * x
        exact, S = math.fsum(terms), float(np.sum(np.abs(terms)))
        bar = (2 * p.n + 8) * EPS * S
        print("%s xprev=%s: dot %.17g csr %.17g fsum %.17g |d| %.3e bar %.3e"
              % (name, xprev is not None, dot, dotc, exact, abs(dot - exact), bar))
        assert abs(dot - exact) <= bar
        if name == "ham2d_32":
            assert dot == dotc


def test_lanczos_runs_agree_to_the_bit(cal, pairs):
    p = pairs("ham2d_32")
    r = vec(2 * p.n, 15)
    for orth in ("local", "full"):
        a = cal.lanczos_ex(None, r, 40, orth, ctx=p.shared)
        b = cal.lanczos_ex(None, r, 40, orth, ctx=p.csr)
        assert a.info["fused"] == b.info["fused"] == 1
        assert np.array_equal(a.T, b.T) and np.array_equal(a.Q, b.Q), orth
        assert np.all(np.isfinite(a.T)) and a.T.shape == (40, 40)
    for orth in ("local", "full"):
        a = cal.ca_lanczos_ex(None, r, 6, 24, "newton", orth, diagnostics=False, ctx=p.shared)
        b = cal.ca_lanczos_ex(None, r, 6, 24, "newton", orth, diagnostics=False, ctx=p.csr)
        assert np.array_equal(a.T, b.T) and np.array_equal(a.Q, b.Q), orth


# ---- 4. confinement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,col", [("rand257", 100), ("long0", 7), ("longlast", 2050), ("band600", 300)])
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_halves_do_not_mix(cal, pairs, name, col, bad):
    p = pairs(name)
    n = p.n
    H = p.H
    hit = np.zeros(n, dtype=bool)
    hit[H.tocsc().indices[H.tocsc().indptr[col]:H.tocsc().indptr[col + 1]]] = True  # rows that reference col
    if not hit.any():
        col = int(np.nonzero(np.diff(H.tocsc().indptr) > 0)[0][0])
        hit[H.tocsc().indices[H.tocsc().indptr[col]:H.tocsc().indptr[col + 1]]] = True
    for half in (0, 1):
        x = vec(2 * n, 16)
        x[half * n + col] = bad
        y = p.shared.spmv(x)
        nf = ~np.isfinite(y)
        expect = np.zeros(2 * n, dtype=bool)
        expect[half * n:(half + 1) * n] = hit
        assert np.array_equal(nf, expect), (name, half)


# ---- 5. the diagonal ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ham2d_32", "randfull257", "long0"])
def test_diagonal(cal, which):
    H = rand_sparse(257, full_diag=True) if which == "randfull257" else build(cal, which)
    n = H.shape[0]
    p = Pair(cal, H)
    try:
        d0 = H.diagonal()
        assert np.array_equal(p.shared.get_diagonal(), np.tile(d0, 2))
        d = np.random.RandomState(5).randn(n)
        d[::3] = 0.0
        x = vec(2 * n, 17)
        y0 = p.shared.spmv(x)
        p.shared.set_diagonal(np.tile(d, 2))
        p.csr.set_diagonal(np.tile(d, 2))
        assert np.array_equal(p.shared.get_diagonal(), np.tile(d, 2))
        y = p.shared.spmv(x)
        assert np.array_equal(y, p.csr.spmv(x)) and not np.array_equal(y, y0)
        bad = np.tile(d, 2)
        bad[n + n // 2] += 1.0
        refused(cal, CAL_ERR_ARG, "d[i] must equal d[n + i]", lambda: p.shared.set_diagonal(bad))
        assert np.array_equal(p.shared.spmv(x), y)  # nothing was written
        p.shared.set_diagonal(np.tile(d0, 2))
        assert np.array_equal(p.shared.spmv(x), y0)
    finally:
        p.close()


def test_missing_diagonal_is_refused(cal, pairs):
    p = pairs("rand257")
    refused(cal, CAL_ERR_UNSUPPORTED, "store no diagonal entry", lambda: p.shared.get_diagonal())
    refused(cal, CAL_ERR_UNSUPPORTED, "store no diagonal entry", lambda: p.shared.set_diagonal(np.zeros(2 * p.n)))
    x = vec(2 * p.n, 18)
    assert np.array_equal(p.shared.spmv(x), p.csr.spmv(x))


# ---- 6. the propagator ------------------------------------------------------------------------------------------
def prop_run(cal, fmt, H, psi0, W, mask, drive=None, scheme="midpoint", steps=8, dt=0.025):
    n = H.shape[0]
    ctx = cal.Context(spmv_format=fmt)
    try:
        P = cal.Propagator(H, psi0, 6, 4, basis="newton", ctx=ctx)
        assert ctx.spmv_shared_info()[0] == (fmt == "shared")
        P.set_observables(W=[W[0]], phi=[psi0], energy=True)
        P.set_absorber(mask)
        if drive is not None:
            P.set_drive(W)
            assert np.array_equal(ctx.get_diagonal(), np.tile(H.diagonal(), 2))
            assert P.step(dt, steps, drive=drive, scheme=scheme) == 0
            assert not np.array_equal(ctx.get_diagonal(), np.tile(H.diagonal(), 2))
        else:
            assert P.step(dt, steps) == 0
        o, ab = P.observables(), P.absorbed()
        out = dict(state=P.state(), norm=P.info()["norm"],
                   obs=np.column_stack([o["t"], o["norm2"], o["energy"], o["W"], o["overlap"].real, o["overlap"].imag]),
                   absorbed=np.column_stack([ab["t"], ab["absorbed"]]))
        P.close()
        out["diag_after"] = ctx.get_diagonal()
        assert len(o["t"]) == len(ab["t"]) and np.all(np.isfinite(out["obs"])) and n == len(out["state"])
        return out
    finally:
        ctx.close()


def same_run(a, b):
    return (np.array_equal(a["state"], b["state"]) and a["norm"] == b["norm"] and np.array_equal(a["obs"], b["obs"])
            and np.array_equal(a["absorbed"], b["absorbed"]))


def ham_setup(cal):
    H = canon(hamiltonian_2d(cal, 32))
    n = H.shape[0]
    i = np.arange(n)
    gx, gy = (i % 32 - 15.5) * 0.25, (i // 32 - 15.5) * 0.25
    psi0 = (np.exp(-0.5 * ((gx - 1.0) ** 2 + gy ** 2)) * np.exp(0.7j * gx)).astype(complex)
    psi0 /= np.linalg.norm(psi0)
    mask = np.minimum(1.0, np.minimum(np.minimum(i % 32, 31 - i % 32), np.minimum(i // 32, 31 - i // 32)) / 4.0 + 0.5)
    return H, psi0, [gx, gy * gy], mask


def test_propagator_bits_on_the_hamiltonian(cal):
    H, psi0, W, mask = ham_setup(cal)
    a = prop_run(cal, "shared", H, psi0, W, mask)
    b = prop_run(cal, "csr", H, psi0, W, mask)
    assert a["obs"].shape == (8, 6) and a["absorbed"].shape == (8, 2) and np.any(a["absorbed"][:, 1] > 0.0)
    assert same_run(a, b)


def test_propagator_on_the_reference_oscillator(cal):
    H, psi0, x = oscillator(256)
    assert np.diff(H.indptr).max() == 5 and H[0, 255] != 0.0 and H[0, 254] != 0.0  # periodic: stays on CSR
    mask = np.ones(256)
    mask[:8] = mask[-8:] = 0.99
    a = prop_run(cal, "shared", H, psi0, [x, x * x], mask)
    b = prop_run(cal, "csr", H, psi0, [x, x * x], mask)
    d = np.linalg.norm(a["state"] - b["state"])
    print("oscillator 256: |shared - csr| = %.3e (bar 5e-14)" % d)
    assert d <= 5e-14


def ham_drive(t):
    return np.array([0.3 * np.sin(3.0 * t), 0.02 * np.cos(2.0 * t)])


@pytest.mark.parametrize("scheme", ["midpoint", "cf4"])
def test_driven_propagator_bits(cal, scheme):
    H, psi0, W, mask = ham_setup(cal)
    a = prop_run(cal, "shared", H, psi0, W, mask, drive=ham_drive, scheme=scheme, steps=4, dt=0.05)
    b = prop_run(cal, "csr", H, psi0, W, mask, drive=ham_drive, scheme=scheme, steps=4, dt=0.05)
    assert same_run(a, b)
    # closing the propagator restores V0 in the one stored copy
    assert np.array_equal(a["diag_after"], np.tile(H.diagonal(), 2))
    assert np.array_equal(b["diag_after"], a["diag_after"])
    plain = prop_run(cal, "shared", H, psi0, W, mask, steps=4, dt=0.05)
    assert not np.array_equal(plain["state"], a["state"])  # the drive does something


# ---- 7. what a shared matrix refuses ---------------------------------------------------------------------------
def test_refusals_name_csr_and_leave_the_context_usable(cal, pairs):
    p = pairs("ham2d_32")
    r, x = vec(2 * p.n, 19), vec(2 * p.n, 20)
    y = p.csr.spmv(x)
    calls = [
        lambda: cal.lanczos_ex(None, r, 20, "periodic", ctx=p.shared),
        lambda: cal.lanczos_ex(None, r, 20, "selective", ctx=p.shared),
        lambda: cal.lanczos_ex(None, r, 20, "local", diagnostics=True, ctx=p.shared),
        lambda: cal.ca_lanczos_ex(None, r, 6, 24, "newton", "periodic", diagnostics=False, ctx=p.shared),
        lambda: cal.ca_lanczos_ex(None, r, 6, 24, "newton", "local", diagnostics=True, ctx=p.shared),
        lambda: cal.impl_restarted_ca_lanczos(None, r, 60, 4, 6, "newton", "full", ctx=p.shared),
        lambda: cal.restarted_ca_lanczos(None, r, 60, 4, 6, "newton", "local", ctx=p.shared),
        lambda: cal.compute_ritz_rnorm(None, np.eye(2 * p.n, 2), np.eye(2), np.array([1.0, 2.0]), ctx=p.shared),
    ]
    for k, fn in enumerate(calls):
        refused(cal, CAL_ERR_UNSUPPORTED, "\"csr\"", fn)
        assert np.array_equal(p.shared.spmv(x), y), k
    # and the csr context runs them
    out = cal.ca_lanczos_ex(None, r, 6, 24, "newton", "local", diagnostics=True, ctx=p.csr)
    assert np.all(np.isfinite(out.ritz_rnorm[-1]))
