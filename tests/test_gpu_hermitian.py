"""Complex Hermitian H on the device: cal_set_matrix_csr_hermitian, the
stored-once kernel k_spmv_stacked with HERM ("shared" selected) and the host-built embedding
E(H) = [[A, -B], [B, A]] on the existing kernels ("csr"), through the SpMV
modes, standard Lanczos and the whole time propagator.

Every pair of contexts here holds the same random Hermitian H (tests/
herm_cases.py): `herm` stores it once, `emb` stores the embedding.

Bars:
  * y of every SpMV mode on `herm`: ``array_equal`` to the NumPy restatement of
    the order contract (tests/herm_ref.py herm_chain, with the epilogues of
    modes 1, 2 and 4 restated there).
  * the fused Lanczos dot: within (2n + 8) eps S of math.fsum of the device's
    own y .* x (the project's summation bar, tests/prop_obs_ref.py).
  * zero imaginary parts: the bits of a "shared" context on A.
  * `herm` against `emb` (another order of the same 2k products per row):
    (2k + 8) eps S per row, S = sum_j (|a_j| + |b_j|)(|x0_j| + |x1_j|).
  * the propagator against dense exponentials of the complex H
    (numpy.linalg.eigh): state error and norm drift at most steps * 1e-10
    (tests/test_gpu_prop.py), builds * 1e-10 with the nonlinear term
    (tests/test_gpu_nonlinear.py), on both contexts; the two contexts agree
    within 5e-14 relative (tests/test_gpu_shared.py's bar between contexts).
    The time step dt = 0.04 was chosen on the CPU: the CPU oracle's CA-Lanczos
    ('local') on the embedding, then expm, is held to the same bar in the test
    (its errors are printed beside the device's).
  * standard Lanczos 'full', 20 vectors: max |H Q_k - Q_k T_k - beta_k q_{k+1}
    e_k'| <= 1e-12 ||H|| and |Q^H Q - I| <= 1e-13 with Q = Q_u + i Q_v, the
    bars tests/test_gpu_lanczos_std.py holds T and |Q'Q - I| to.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import absorber_ref as aref  # noqa: E402
import drive_ref as dref  # noqa: E402
import herm_ref  # noqa: E402
import nonlinear_ref as nref  # noqa: E402
import prop_obs_ref as pref  # noqa: E402
from herm_cases import band_herm, long_row_herm, rand_herm, signed_zero_vec  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
CAL_ERR_ARG = -1
CAL_ERR_UNSUPPORTED = -6

RAND_N = (1, 2, 3, 255, 256, 257, 1025)
NAMES = ["rand%d" % n for n in RAND_N] + ["band600", "long4100"]


@functools.lru_cache(maxsize=None)
def build(name):
    if name.startswith("rand"):
        return rand_herm(int(name[4:]))
    if name == "band600":
        return band_herm()
    assert name == "long4100"
    return long_row_herm()


def real_part(H):
    return sp.csr_matrix((np.ascontiguousarray(H.data.real), H.indices, H.indptr), shape=H.shape)


class Pair:
    def __init__(self, cal, H):
        self.H = H
        self.n = H.shape[0]
        self.herm = cal.Context(spmv_format="shared").set_matrix_hermitian(H)
        self.emb = cal.Context(spmv_format="csr").set_matrix_hermitian(H)

    def close(self):
        self.herm.close()
        self.emb.close()


@pytest.fixture(scope="module")
def pairs(cal):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pair(cal, build(name))
        return made[name]

    yield get
    for p in made.values():
        p.close()


def refused(cal, code, what, fn):
    with pytest.raises(cal.CalError) as e:
        fn()
    assert e.value.status == code, (e.value.status, str(e.value))
    assert what in str(e.value), str(e.value)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 5. what is stored ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rand3", "rand257", "long4100"])
def test_hermitian_info(cal, pairs, name):
    p = pairs(name)
    assert p.herm.spmv_hermitian_info() == (True, p.n, p.H.nnz)
    assert p.herm.spmv_shared_info() == (True, p.n, p.H.nnz)
    assert p.emb.spmv_hermitian_info() == (False, 0, 0) and p.emb.spmv_shared_info() == (False, 0, 0)
    assert p.herm.matrix_info() == p.emb.matrix_info()
    assert p.herm.matrix_info()["n_local"] == 2 * p.n and p.herm.matrix_info()["nnz_local"] == 4 * p.H.nnz
    assert p.herm.spmv_lanczos_fused() is True


@pytest.mark.parametrize("fmt", ["shared", "csr"])
def test_a_real_matrix_takes_the_stacked_path(cal, fmt):
    """val_im = NULL (a real dtype): cal_set_matrix_csr_stacked's matrix and bits."""
    A = real_part(build("rand257"))
    a, b = cal.Context(spmv_format=fmt), cal.Context(spmv_format=fmt)
    try:
        a.set_matrix_hermitian(A)
        b.set_matrix_stacked(A)
        assert a.spmv_hermitian_info() == (False, 0, 0)
        assert a.spmv_shared_info() == b.spmv_shared_info() == ((True, 257, A.nnz) if fmt == "shared" else (False, 0, 0))
        assert a.matrix_info() == b.matrix_info()
        x = signed_zero_vec(514, 21)
        ya, yb = a.spmv(x), b.spmv(x)
        assert np.array_equal(bits(ya), bits(yb)) and np.array_equal(bits(ya), bits(herm_ref.shared_chain(A, x)))
    finally:
        a.close()
        b.close()


# ---- 1. y to the bit, every mode --------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_spmv_bits(cal, pairs, name):
    p = pairs(name)
    for seed in (11, 12):
        x = signed_zero_vec(2 * p.n, seed)
        y = p.herm.spmv(x)
        assert np.array_equal(bits(y), bits(herm_ref.herm_chain(p.H, x))), seed
        assert not np.any(np.signbit(y[y == 0.0]))  # a row sum starts at +0.0 and never becomes -0.0


@pytest.mark.parametrize("name", NAMES)
def test_matrix_powers_bits(cal, pairs, name):
    """s = 3: the monomial basis is mode 0 three times; the modified Newton basis
    with the shifts (0.5, 1 + 0.75i, 1 - 0.75i) is mode 1, mode 1, mode 2; a real
    shift list in the plain basis is mode 1."""
    p = pairs(name)
    H, s = p.H, 3
    q = signed_zero_vec(2 * p.n, 13) / 64.0
    got = cal.matrix_powers_monomial(None, q, s, ctx=p.herm)
    v = q
    for k in range(s):
        v = herm_ref.herm_chain(H, v)
        assert np.array_equal(bits(got[:, k]), bits(v)), k
    lam = np.array([0.5, 1.0 + 0.75j, 1.0 - 0.75j])
    V = cal.matrix_powers_newton(None, q, s, lam, 1, ctx=p.herm)
    assert V.shape == (2 * p.n, s + 1) and np.array_equal(bits(V[:, 0]), bits(q))
    v1 = herm_ref.epilogue(herm_ref.herm_chain(H, q), q, 0.5)
    v2 = herm_ref.epilogue(herm_ref.herm_chain(H, v1), v1, 1.0)
    v3 = herm_ref.epilogue(herm_ref.herm_chain(H, v2), v2, 1.0, 0.75 * 0.75, v1)
    for k, v in enumerate((v1, v2, v3)):
        assert np.array_equal(bits(V[:, k + 1]), bits(v)), k
    real = np.array([0.5, -1.25, 2.0])
    V = cal.matrix_powers_newton(None, q, s, real, 0, ctx=p.herm)
    v = q
    for k in range(s):
        v = herm_ref.epilogue(herm_ref.herm_chain(H, v), v, real[k])
        assert np.array_equal(bits(V[:, k + 1]), bits(v)), k


@pytest.mark.parametrize("name", NAMES)
def test_spmv_lanczos_bits_and_dot(cal, pairs, name):
    p = pairs(name)
    x, xp = signed_zero_vec(2 * p.n, 14), signed_zero_vec(2 * p.n, 15)
    for xprev, b2 in ((None, 0.0), (xp, 0.7)):
        y, dot = p.herm.spmv_lanczos(x, xprev, b2)
        assert np.array_equal(bits(y), bits(herm_ref.lanczos_epilogue(herm_ref.herm_chain(p.H, x), xprev, b2)))
        terms = y * x
        exact, S = math.fsum(terms), float(np.sum(np.abs(terms)))
        bar = (2 * p.n + 8) * EPS * S
        print("%s xprev=%s: dot %.17g fsum %.17g |d| %.3e bar %.3e"
              % (name, xprev is not None, dot, exact, abs(dot - exact), bar))
        assert abs(dot - exact) <= bar


# ---- 3. zero imaginary parts: the bits of "shared" on A --------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_zero_imaginary_parts_give_the_shared_bits(cal, pairs, name):
    H = build(name)
    n = H.shape[0]
    A = real_part(H)
    Z = sp.csr_matrix((H.data.real + 0j, H.indices, H.indptr), shape=H.shape)  # complex dtype, val_im all zeros
    z, a = cal.Context(spmv_format="shared"), cal.Context(spmv_format="shared")
    try:
        z.set_matrix_hermitian(Z)
        a.set_matrix_stacked(A)
        assert z.spmv_hermitian_info() == (True, n, H.nnz)  # not detected: the Hermitian kernel runs
        assert a.spmv_hermitian_info() == (False, 0, 0) and a.spmv_shared_info() == (True, n, H.nnz)
        x, xp = signed_zero_vec(2 * n, 16), signed_zero_vec(2 * n, 17)
        assert np.array_equal(bits(z.spmv(x)), bits(a.spmv(x)))
        for xprev, b2 in ((None, 0.0), (xp, 0.7)):
            yz, dz = z.spmv_lanczos(x, xprev, b2)
            ya, da = a.spmv_lanczos(x, xprev, b2)
            assert np.array_equal(bits(yz), bits(ya)) and dz == da
    finally:
        z.close()
        a.close()


# ---- 4. stored once against the embedding on the existing kernels -------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_stored_once_against_the_embedding(cal, pairs, name):
    p = pairs(name)
    E = cal.matrices.hermitian_embedding(p.H)
    worst = 0.0
    for seed in (18, 19):
        x = signed_zero_vec(2 * p.n, seed)
        y, ye = p.herm.spmv(x), p.emb.spmv(x)
        assert np.array_equal(bits(ye), bits(herm_ref.rowsum_chain(E, x)))  # the host builds the documented rows
        bar = herm_ref.row_bar(p.H, x)
        d = np.abs(y - ye)
        assert np.all(d <= bar)
        assert np.all(np.abs(y - herm_ref.exact_product(p.H, x)) <= bar)
        if np.any(bar > 0):
            worst = max(worst, float(np.max(d[bar > 0] / bar[bar > 0])))
    print("%s: largest |herm - emb| / bar %.3f" % (name, worst))


# ---- 6. a non-finite x entry reaches both halves of the rows that store its column -------------------------------
@pytest.mark.parametrize("name,col", [("rand257", 100), ("long4100", 7), ("long4100", 2000), ("band600", 300)])
def test_an_inf_reaches_both_halves(cal, pairs, name, col):
    p = pairs(name)
    n, Hc = p.n, p.H.tocsc()
    if Hc.indptr[col + 1] == Hc.indptr[col]:
        col = int(np.nonzero(np.diff(Hc.indptr) > 0)[0][0])
    hit = np.zeros(n, dtype=bool)
    hit[Hc.indices[Hc.indptr[col]:Hc.indptr[col + 1]]] = True  # the rows that store column col
    assert hit.any() and not hit.all()
    for half in (0, 1):
        x = np.random.RandomState(20).randn(2 * n)
        x[half * n + col] = np.inf
        for ctx in (p.herm, p.emb):
            nf = ~np.isfinite(ctx.spmv(x))
            assert np.array_equal(nf, np.tile(hit, 2)), (name, half, ctx is p.herm)


# ---- 7. refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["shared", "csr"])
def test_an_imaginary_diagonal_is_refused(cal, fmt):
    H = rand_herm(257, full_diag=True).copy()
    rows = np.repeat(np.arange(257), np.diff(H.indptr))
    d = np.nonzero(H.indices == rows)[0]
    H.data[d[100]] += 1e-300j
    ctx = cal.Context(spmv_format=fmt)
    try:
        refused(cal, CAL_ERR_ARG, "diagonal", lambda: ctx.set_matrix_hermitian(H))
        H.data[d[100]] = H.data[d[100]].real
        ctx.set_matrix_hermitian(H)  # the context goes on working
        assert ctx.spmv_hermitian_info()[0] == (fmt == "shared")
    finally:
        ctx.close()


def test_the_stored_once_matrix_refuses_what_shared_refuses(cal, pairs):
    p = pairs("rand257")
    r, x = signed_zero_vec(2 * p.n, 22) + 0.5, signed_zero_vec(2 * p.n, 23)
    y = p.herm.spmv(x)
    calls = [
        lambda: cal.lanczos_ex(None, r, 20, "periodic", ctx=p.herm),
        lambda: cal.ca_lanczos_ex(None, r, 6, 24, "newton", "periodic", diagnostics=False, ctx=p.herm),
        lambda: cal.lanczos_ex(None, r, 20, "local", diagnostics=True, ctx=p.herm),
        lambda: cal.ca_lanczos_ex(None, r, 6, 24, "newton", "local", diagnostics=True, ctx=p.herm),
        lambda: cal.restarted_ca_lanczos(None, r, 60, 4, 6, "newton", "local", ctx=p.herm),
        lambda: cal.impl_restarted_ca_lanczos(None, r, 60, 4, 6, "newton", "full", ctx=p.herm),
    ]
    for k, fn in enumerate(calls):
        refused(cal, CAL_ERR_UNSUPPORTED, "cal_set_matrix_csr_hermitian", fn)
        assert np.array_equal(bits(p.herm.spmv(x)), bits(y)), k
    # the embedding runs what the stored-once matrix refuses
    out = cal.ca_lanczos_ex(None, r, 6, 24, "newton", "local", diagnostics=True, ctx=p.emb)
    assert np.all(np.isfinite(out.ritz_rnorm[-1]))


def test_the_diagonal_is_the_real_one_of_both_halves(cal):
    H = rand_herm(257, full_diag=True)
    n = 257
    p = Pair(cal, H)
    try:
        d0 = H.diagonal().real
        assert np.array_equal(p.herm.get_diagonal(), np.tile(d0, 2))
        d = np.random.RandomState(5).randn(n)
        d[::3] = 0.0
        x = signed_zero_vec(2 * n, 24)
        y0 = p.herm.spmv(x)
        bad = np.tile(d, 2)
        bad[n + n // 2] += 1.0
        refused(cal, CAL_ERR_ARG, "d[i] must equal d[n + i]", lambda: p.herm.set_diagonal(bad))
        assert np.array_equal(bits(p.herm.spmv(x)), bits(y0))  # nothing was written
        p.herm.set_diagonal(np.tile(d, 2))
        assert np.array_equal(p.herm.get_diagonal(), np.tile(d, 2))
        Hd = H.copy()
        rows = np.repeat(np.arange(n), np.diff(H.indptr))
        Hd.data[H.indices == rows] = d
        y = p.herm.spmv(x)
        assert np.array_equal(bits(y), bits(herm_ref.herm_chain(Hd, x))) and not np.array_equal(y, y0)
        p.herm.set_diagonal(np.tile(d0, 2))
        assert np.array_equal(bits(p.herm.spmv(x)), bits(y0))
    finally:
        p.close()


def test_a_missing_diagonal_is_refused(cal, pairs):
    p = pairs("rand257")
    refused(cal, CAL_ERR_UNSUPPORTED, "store no diagonal entry", lambda: p.herm.get_diagonal())


# ---- 8. the propagator against dense exponentials ------------------------------------------------------------
N2, FLUX, HX = 24, 1.0 / 12.0, 0.5
STEPS, DT = 8, 0.04


@functools.lru_cache(maxsize=None)
def peierls_problem():
    """peierls_hamiltonian((24, 24), harmonic V, flux 1/12) on a mesh of width
    0.5, a Gaussian packet with momentum, the grid coordinates and the dense
    eigh of the complex H."""
    from ca_lanczos_amd import matrices
    i = np.arange(N2 * N2)
    gx, gy = (i % N2 - 0.5 * (N2 - 1)) * HX, (i // N2 - 0.5 * (N2 - 1)) * HX
    V = 0.5 * (gx * gx + gy * gy)
    H = matrices.peierls_hamiltonian((N2, N2), V, FLUX, h=HX)
    psi0 = np.exp(-0.5 * ((gx + 1.5) ** 2 + gy ** 2)) * np.exp(1j * (1.0 * gx + 0.5 * gy))
    psi0 = psi0 / np.linalg.norm(psi0)
    ew, U = np.linalg.eigh(H.toarray())
    return H, psi0, gx, gy, ew, U


def expo_dense(Hd, extra, sub, psi):
    ew, U = np.linalg.eigh(Hd + np.diag(extra))
    return U @ (np.exp(-1j * sub * ew) * (U.conj().T @ psi))


def exact(ew, U, psi0, t):
    return U @ (np.exp(-1j * t * ew) * (U.conj().T @ psi0))


@functools.lru_cache(maxsize=None)
def oracle_error(s, blocks, basis):
    """The CPU oracle's CA-Lanczos ('local') on the embedding, then expm: the run dt was chosen with."""
    from ca_lanczos_amd import matrices
    from oracle import ca_lanczos_ref as ref
    H, psi0, _, _, ew, U = peierls_problem()
    n = H.shape[0]
    E = matrices.hermitian_embedding(H)
    x = np.concatenate([psi0.real, psi0.imag])
    drift = 0.0
    for _ in range(STEPS):
        nrm = np.linalg.norm(x)
        res = ref.ca_lanczos(E, x, s, s * blocks, basis, "local", diagnostics=False)
        c = sl.expm(-1j * DT * res.T)[:, 0] * nrm
        out = (res.Q[:n] + 1j * res.Q[n:]) @ c
        x = np.concatenate([out.real, out.imag])
        drift = max(drift, abs(np.linalg.norm(x) - 1.0))
    return np.linalg.norm(x[:n] + 1j * x[n:] - exact(ew, U, psi0, STEPS * DT)), drift


def run_peierls(cal, fmt, s, blocks, basis):
    H, psi0, _, _, ew, U = peierls_problem()
    ctx = cal.Context(spmv_format=fmt)
    try:
        P = cal.Propagator(H, psi0, s, blocks, basis=basis, ctx=ctx)
        assert ctx.spmv_hermitian_info()[0] == (fmt == "shared")
        drift = 0.0
        for _ in range(STEPS):
            assert P.step(DT, 1) == 0
            drift = max(drift, abs(P.info()["norm"] - 1.0))
        psi, info = P.state(), P.info()
        P.close()
    finally:
        ctx.close()
    assert info["steps"] == STEPS and info["breakdowns"] == 0
    return psi, np.linalg.norm(psi - exact(ew, U, psi0, STEPS * DT)), drift


@pytest.mark.parametrize("s,blocks", [(6, 4), (4, 6)])
@pytest.mark.parametrize("basis", ["newton", "monomial"])
def test_propagator_in_a_magnetic_field(cal, basis, s, blocks):
    H, psi0, _, _, _, _ = peierls_problem()
    assert np.iscomplexobj(H.data) and np.max(np.abs(H.data.imag)) > 0.5
    bar = STEPS * 1e-10
    e_or, d_or = oracle_error(s, blocks, basis)
    pe, err_e, drift_e = run_peierls(cal, "csr", s, blocks, basis)
    ph, err_h, drift_h = run_peierls(cal, "shared", s, blocks, basis)
    between = np.linalg.norm(ph - pe) / np.linalg.norm(pe)
    print("%s s=%d blocks=%d: oracle err %.3e drift %.3e; embedding err %.3e drift %.3e; stored once err %.3e "
          "drift %.3e; between the contexts %.3e (bar 5e-14)"
          % (basis, s, blocks, e_or, d_or, err_e, drift_e, err_h, drift_h, between))
    assert e_or <= bar and d_or <= bar
    assert err_e <= bar and drift_e <= bar
    assert err_h <= bar and drift_h <= bar
    assert between <= 5e-14


# ---- 9. the rest of the propagator on the stored-once matrix -----------------------------------------------------
def open_herm(cal, s=6, blocks=4):
    H, psi0, _, _, _, _ = peierls_problem()
    ctx = cal.Context(spmv_format="shared")
    try:
        P = cal.Propagator(H, psi0, s, blocks, ctx=ctx)
    except Exception:
        ctx.close()
        raise
    assert ctx.spmv_hermitian_info() == (True, H.shape[0], H.nnz)
    return ctx, P


def test_energy_and_a_diagonal_operator(cal):
    from ca_lanczos_amd import matrices
    H, psi0, gx, _, _, _ = peierls_problem()
    n = H.shape[0]
    E = matrices.hermitian_embedding(H)
    ctx, P = open_herm(cal)
    try:
        P.set_observables(W=[gx], energy=True)
        for k in range(3):
            assert P.step(DT, 1) == 0
            psi = P.state()
            row = P.observables()
            x = np.concatenate([psi.real, psi.imag])
            e_ref = float(np.real(np.vdot(psi, H @ psi)))
            e_bar = (E.nnz + 2 * n + 8) * EPS * float(np.abs(x) @ (abs(E) @ np.abs(x)))
            w_ref, w_bar = pref.w_ref(gx, psi)
            print("step %d: |dE| %.3e (bar %.3e), |d<x>| %.3e (bar %.3e)"
                  % (k + 1, abs(row["energy"][k] - e_ref), e_bar, abs(row["W"][k, 0] - w_ref[0]), w_bar[0]))
            assert abs(row["energy"][k] - e_ref) <= e_bar
            assert abs(row["W"][k, 0] - w_ref[0]) <= w_bar[0]
        P.close()
    finally:
        ctx.close()


def test_absorber_rows(cal):
    H, psi0, _, _, ew, U = peierls_problem()
    from ca_lanczos_amd import matrices
    M = matrices.absorber_mask((N2, N2), 6)
    ph = np.exp(-1j * DT * ew)
    psi, us, ab = psi0.astype(complex), [], []
    for _ in range(4):  # the dense scheme psi <- M .* U exp(-i dt E) U^H psi
        u = U @ (ph * (U.conj().T @ psi))
        ab.append(float(np.sum((1.0 - M * M) * np.abs(u) ** 2)))
        us.append(u)
        psi = M * u
    ctx, P = open_herm(cal)
    try:
        P.set_absorber(M)
        assert P.step(DT, 4) == 0
        got, a = P.state(), P.absorbed()
        P.close()
    finally:
        ctx.close()
    err = np.linalg.norm(got - psi)
    print("absorber: state err %.3e (bar %.1e)" % (err, 4e-10))
    assert err <= 4 * 1e-10
    assert a["absorbed"].shape == (4,) and np.all(a["absorbed"] > 0.0)
    for k in range(1, 5):
        _, _, terms = aref.masked_ref(us[k - 1].real, us[k - 1].imag, M)
        bar = 2 * np.linalg.norm(us[k - 1]) * k * 1e-10 + aref.absorbed_bar(terms)
        d = abs(a["absorbed"][k - 1] - ab[k - 1])
        print("step %d: absorbed %.6e, |absorbed - dense| %.3e (bar %.3e)" % (k, a["absorbed"][k - 1], d, bar))
        assert d <= bar


def column_of(ctx, n, c):
    """Column c of E(H) read through a SpMV of the unit vector: (Re, Im) of H[:, c]."""
    e = np.zeros(2 * n)
    e[c] = 1.0
    y = ctx.spmv(e)
    return y[:n], y[n:]


def test_drive_midpoint_and_the_diagonal_it_leaves(cal):
    """2 sin(3t) x under "midpoint" against the dense exponentials of H + f_j
    diag(x); the diagonal a driven step leaves is the drive chain to the bit and
    the imaginary parts are those of the upload."""
    H, psi0, gx, _, _, _ = peierls_problem()
    n = H.shape[0]
    Hd, V0 = H.toarray(), H.diagonal().real
    rows = np.array([dref.f_one((j + 0.5) * DT) for j in range(STEPS)])
    psi = psi0.astype(complex)
    for r in rows:
        psi = expo_dense(Hd, r[0] * gx, DT, psi)
    ctx, P = open_herm(cal)
    try:
        P.set_drive([gx])
        assert P.step(DT, 1, drive=dref.f_one, scheme="midpoint") == 0
        assert np.array_equal(bits(ctx.get_diagonal()), bits(np.tile(dref.chain(V0, [gx], rows[0]), 2)))
        assert P.step(DT, STEPS - 1, drive=dref.f_one, scheme="midpoint") == 0
        assert np.array_equal(bits(ctx.get_diagonal()), bits(np.tile(dref.chain(V0, [gx], rows[-1]), 2)))
        got, info = P.state(), P.info()
        P.close()
        assert np.array_equal(bits(ctx.get_diagonal()), bits(np.tile(V0, 2)))  # closing restores V0
        for c in range(0, n, 37):  # vim untouched, val touched on the diagonal only
            re, im = column_of(ctx, n, c)
            assert np.array_equal(re, Hd[:, c].real) and np.array_equal(im, Hd[:, c].imag), c
    finally:
        ctx.close()
    err, drift = np.linalg.norm(got - psi), abs(info["norm"] - 1.0)
    print("driven: err %.3e drift %.3e (bar %.1e)" % (err, drift, STEPS * 1e-10))
    assert err <= STEPS * 1e-10 and drift <= STEPS * 1e-10


def test_nonlinear_midpoint_and_the_density_diagonal(cal):
    H, psi0, gx, _, _, _ = peierls_problem()
    n, g = H.shape[0], 0.5
    Hd, V0 = H.toarray(), H.diagonal().real
    builds = 2 * STEPS
    ref_psi = nref.nonlinear_steps(lambda extra, psi: expo_dense(Hd, extra, DT, psi), n, [], psi0,
                                   np.zeros((STEPS, 0)), DT, g, "midpoint")
    ctx, P = open_herm(cal)
    try:
        P.set_nonlinear(g, "midpoint")
        drift = 0.0
        for _ in range(STEPS):
            assert P.step(DT, 1) == 0
            drift = max(drift, abs(P.info()["norm"] - 1.0))
        got = P.state()
        P.close()
        # one driven "frozen" step: the diagonal it leaves is density_chain's
        P = cal.Propagator(H, psi0, 6, 4, ctx=ctx)
        P.set_drive([gx])
        P.set_nonlinear(g, "frozen")
        assert P.step(DT, 1, drive=[[0.3]]) == 0
        expect = nref.density_chain(V0, [gx], [0.3], g, psi0)
        assert not np.array_equal(expect, dref.chain(V0, [gx], [0.3]))
        assert np.array_equal(bits(ctx.get_diagonal()), bits(np.tile(expect, 2)))
        P.close()
        assert np.array_equal(bits(ctx.get_diagonal()), bits(np.tile(V0, 2)))
        for c in range(5, n, 41):
            re, im = column_of(ctx, n, c)
            assert np.array_equal(re, Hd[:, c].real) and np.array_equal(im, Hd[:, c].imag), c
    finally:
        ctx.close()
    err = np.linalg.norm(got - ref_psi)
    print("nonlinear midpoint: err %.3e drift %.3e (bar %.1e)" % (err, drift, builds * 1e-10))
    assert err <= builds * 1e-10 and drift <= builds * 1e-10


# ---- 10. standard Lanczos 'full' -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["herm", "emb"])
def test_standard_lanczos_full(cal, pairs, which):
    p = pairs("rand257")
    n, m = p.n, 20
    ctx = p.herm if which == "herm" else p.emb
    r = np.random.RandomState(25).randn(2 * n)
    out = cal.lanczos_ex(None, r, m, "full", ctx=ctx)
    assert out.info["steps"] == m and out.info["breakdown"] == 0 and out.info["fused"] == 1
    Q = out.Q[:n] + 1j * out.Q[n:]
    Hd = p.H.toarray()
    normH = float(np.max(np.abs(np.linalg.eigvalsh(Hd))))
    k = m - 1  # Q_k, T_k and q_{k+1}: 20 vectors in all
    R = Hd @ Q[:, :k] - Q[:, :k] @ out.T[:k, :k]
    R[:, k - 1] -= out.T[k, k - 1] * Q[:, k]
    res = float(np.max(np.abs(R)))
    oq = float(np.max(np.abs(Q.conj().T @ Q - np.eye(m))))
    oq_real = float(np.max(np.abs(out.Q.T @ out.Q - np.eye(m))))
    print("%s: residual / |H| %.3e (bar 1e-12), |Q^H Q - I| %.3e (bar 1e-13; the real inner product alone %.3e)"
          % (which, res / normH, oq, oq_real))
    assert res <= 1e-12 * normH
    assert oq <= 1e-13
