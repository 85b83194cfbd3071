"""The diagonal-split SpMV format (k_spmv_planes with DG; a
uniform 5- / 7-point stencil on the plane march plus the per-row diagonal as
one streamed vector, H = K + diag(V)) against the oracle and against the same
matrix on a "csr" context.

Bar: the bits of the sequential CSR row sum (k_spmv) in every mode the format
takes (0, the Newton modes 1 and 2, the fused Lanczos step 4), inf / nan
confinement included; whole CA-Lanczos, standard Lanczos and propagator runs
do not depend on the format.  Every potential is all-distinct (split_cases.
potential), so each row has a diagonal value of its own.

Geometries: lap3d_17 (P = 289 odd, one partial block per plane), lap3d_23 (P
= 529 odd, 2 blocks per plane), lap3d_41 (n = 68,921 > 65,535 rows: more row
patterns than the pattern format holds), 5-point Hamiltonians with
off-diagonals -8 (not NEG1) at P = 300 and P = 257 (odd), lap3d_17 with some
diagonal entries structurally absent, and lap3d_164 (1113 blocks of 8 planes:
the Z = 8 kernel; every smaller grid marches 2 planes per block)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_cases import drop_diagonal, hamiltonian_2d, lap3d_v  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
CAL_ERR_UNSUPPORTED = -6


def _nodiag_rows(n, N, P):
    return [0, N - 1, P, n // 2 + N - 1, n // 2 + N, n - P, n - 1]


def _lap3d_17_nodiag(cal):
    A = lap3d_v(cal, 17)
    return drop_diagonal(A, _nodiag_rows(A.shape[0], 17, 289))


CASES = [
    # (name, builder, P, H, neg1, in-plane stride N)
    ("lap3d_17_V", lambda cal: lap3d_v(cal, 17), 289, 18, True, 17),
    ("lap3d_23_V", lambda cal: lap3d_v(cal, 23), 529, 24, True, 23),
    ("lap3d_41_V", lambda cal: lap3d_v(cal, 41), 1681, 42, True, 41),
    ("ham2d_300", lambda cal: hamiltonian_2d(cal, 300), 300, 2, False, 300),
    ("ham2d_257", lambda cal: hamiltonian_2d(cal, 257), 257, 2, False, 257),
    ("lap3d_17_V_nodiag", _lap3d_17_nodiag, 289, 18, True, 17),
    ("lap3d_164_V_z8", lambda cal: lap3d_v(cal, 164), 164 * 164, 164, True, 164),
]


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, cal):
    name, build, P, H, neg1, N = request.param
    A = build(cal)
    split = cal.Context(spmv_format="split").set_matrix(A)
    csr = cal.Context(spmv_format="csr").set_matrix(A)
    yield dict(name=name, A=A, split=split, csr=csr, P=P, H=H, neg1=neg1, N=N)
    split.close()
    csr.close()


def _many_diagonals(cal, N, M):
    """test_gpu_planes._many_diagonals: 306 row patterns, on the plane march with 2-B keys."""
    A = cal.matrices.laplacian_2d(N).tolil()
    n = A.shape[0]
    A.setdiag(4.0 + (np.arange(n) % M) * 2.0 ** -10)
    A = A.tocsr()
    A.sort_indices()
    return A


# ---- the format taken ------------------------------------------------------
def test_split_format_taken(case, cal):
    c = case
    assert c["split"].spmv_split_info() == (True, c["P"], c["H"], c["neg1"]), c["name"]
    assert c["split"].spmv_format()[0] == "csr"
    assert c["split"].spmv_plane_info() == (0, 0, -1)
    assert c["csr"].spmv_split_info() == (False, 0, 0, False)
    if c["name"].endswith("z8"):
        n = c["A"].shape[0]
        assert ((c["P"] + 511) // 512) * ((-(-n // c["P"]) + 7) // 8) == 1113  # >= 1024 blocks: Z = 8
    auto = cal.Context(spmv_format="auto").set_matrix(c["A"])
    try:
        assert auto.spmv_split_info() == (True, c["P"], c["H"], c["neg1"]), c["name"]
        assert auto.spmv_format()[0] == "csr"
    finally:
        auto.close()


def test_split_refuses_what_does_not_qualify(cal):
    for A in (cal.matrices.circuit_like(200), cal.matrices.laplacian_2d(37)):
        ctx = cal.Context(spmv_format="split")
        try:
            with pytest.raises(cal.CalError) as e:
                ctx.set_matrix(A)
            assert e.value.status == CAL_ERR_UNSUPPORTED
            assert "diagonal-split" in str(e.value)
        finally:
            ctx.close()


def test_auto_leaves_other_matrices_alone(cal):
    for A, fmt, plane in ((cal.matrices.circuit_like(200), None, False), (_many_diagonals(cal, 300, 100), "pattern", True),
                          (cal.matrices.laplacian_3d(20), "pattern", True)):
        ctx = cal.Context(spmv_format="auto").set_matrix(A)
        try:
            assert ctx.spmv_split_info() == (False, 0, 0, False)
            if fmt:
                assert ctx.spmv_format()[0] == fmt
            assert (ctx.spmv_plane_info()[0] > 0) == plane
        finally:
            ctx.close()


# ---- mode 0 ----------------------------------------------------------------
def test_split_spmv_bitexact(case, ref):
    c = case
    A, n = c["A"], c["A"].shape[0]
    rng = np.random.RandomState(11)
    vecs = (ref.matlab_rand(n, seed=3) - 0.5, rng.randn(n) * 1e3, np.ones(n))
    for v in vecs:
        got = c["split"].spmv(v)
        assert np.array_equal(got, ref.SpMV(A, v)), c["name"]
        assert np.array_equal(got, c["csr"].spmv(v)), c["name"]


def test_split_spmv_inf_does_not_leak(case, ref):
    """The positions of test_plane_spmv_inf_does_not_leak; in the case without
    some diagonal entries, several of them are rows that lack theirs: such a
    row does not reference its own x and must stay finite."""
    c = case
    A, n, P, N = c["A"], c["A"].shape[0], c["P"], c["N"]
    rng = np.random.RandomState(5)
    pos_list = (0, N - 1, N, P - 1, P, n - 1, n // 2 + N - 1, n - P)
    if c["name"].endswith("nodiag"):
        absent = [r for r in pos_list if A[r, r] == 0.0 and r not in A[r].indices]
        assert len(absent) >= 5
    for pos in pos_list:
        v = rng.randn(n)
        v[pos] = np.inf if pos % 2 else np.nan
        got, exp = c["split"].spmv(v), ref.SpMV(A, v)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), (c["name"], pos)
        assert np.array_equal(np.isinf(got), np.isinf(exp)), (c["name"], pos)
        fin = np.isfinite(exp)
        assert np.array_equal(got[fin], exp[fin]), (c["name"], pos)
        if c["name"].endswith("nodiag") and pos in absent:
            assert np.isfinite(got[pos]), (c["name"], pos)


# ---- modes 1 and 2, monomial -----------------------------------------------
def test_split_newton_and_monomial_powers_bitexact(case, cal, ref):
    c = case
    A, n, ctx = c["A"], c["A"].shape[0], c["split"]
    v = ref.matlab_rand(n)
    lamc = np.array([7.0, 3 + 0.5j, 3 - 0.5j, 1.0])
    assert np.array_equal(cal.matrix_powers_newton(A, v, 4, lamc, 1, ctx=ctx),
                          ref.matrix_powers_newton(A, v, 4, lamc, 1)), c["name"]
    lam = np.array([11.5, 0.3, 6.1, 2.2, 9.0, 4.4, 1.1, 7.7])
    for modifiedp in (0, 1):
        assert np.array_equal(cal.matrix_powers_newton(A, v, 8, lam, modifiedp, ctx=ctx),
                              ref.matrix_powers_newton(A, v, 8, lam, modifiedp)), c["name"]
    assert np.array_equal(cal.matrix_powers_monomial(A, v, 8, ctx=ctx), ref.matrix_powers_monomial(A, v, 8)), c["name"]


# ---- mode 4 ----------------------------------------------------------------
def test_split_fused_lanczos_step(case):
    c = case
    n, ctx = c["A"].shape[0], c["split"]
    assert ctx.spmv_lanczos_fused() is True
    rng = np.random.default_rng(11)
    x, xprev = rng.standard_normal(n), rng.standard_normal(n)
    beta2 = 0.7
    y0, d0 = ctx.spmv_lanczos(x, None, 0.0)
    assert np.array_equal(y0, ctx.spmv(x)), c["name"]
    y, d = ctx.spmv_lanczos(x, xprev, beta2)
    y2, d2 = ctx.spmv_lanczos(x, xprev, beta2)
    assert np.array_equal(y, y2) and d == d2, c["name"]
    yc0, dc0 = c["csr"].spmv_lanczos(x, None, 0.0)
    yc, dc = c["csr"].spmv_lanczos(x, xprev, beta2)
    assert np.array_equal(y0, yc0) and np.array_equal(y, yc), c["name"]
    assert d0 == dc0 and d == dc, c["name"]  # the dot is summed in the CSR kernel's order
    for yy, dd in ((y0, d0), (y, d)):
        prod = yy * x
        exact_dot = math.fsum(prod.tolist())
        lim = n * EPS * float(np.sum(np.abs(prod)))
        print("%s: |dot - fsum| = %.3e (bound %.3e)" % (c["name"], abs(dd - exact_dot), lim))
        assert abs(dd - exact_dot) <= lim


# ---- whole runs do not depend on the format ---------------------------------
@pytest.fixture(scope="module")
def pair17(cal):
    A = lap3d_v(cal, 17)
    split = cal.Context(spmv_format="split").set_matrix(A)
    csr = cal.Context(spmv_format="csr").set_matrix(A)
    yield A, split, csr
    split.close()
    csr.close()


@pytest.mark.parametrize("diagnostics", [False, True], ids=["plain", "diagnostics"])
def test_ca_lanczos_run_is_format_invariant(pair17, cal, ref, diagnostics):
    """With diagnostics the Ritz residuals run on the CSR residual kernel of
    either context (the split format has no residual kernel of its own)."""
    A, split, csr = pair17
    r = ref.matlab_rand(A.shape[0])
    a = cal.ca_lanczos_ex(A, r, 8, 40, "newton", "local", diagnostics=diagnostics, ctx=split)
    b = cal.ca_lanczos_ex(A, r, 8, 40, "newton", "local", diagnostics=diagnostics, ctx=csr)
    assert split.spmv_split_info()[0] and not csr.spmv_split_info()[0]
    assert a.T.shape == (40, 40)
    assert np.array_equal(a.T, b.T) and np.array_equal(a.Q, b.Q)
    assert np.array_equal(a.shifts, b.shifts) and np.array_equal(a.reorth, b.reorth)
    if diagnostics:
        assert np.array_equal(a.ritz_rnorm, b.ritz_rnorm) and np.array_equal(a.orth_err, b.orth_err)
        assert np.all(np.isfinite(a.ritz_rnorm))


def test_propagator_is_format_invariant(cal):
    N = 17
    H = lap3d_v(cal, N)
    n = H.shape[0]
    i = np.arange(n)
    x, y, z = i % N - 8.0, (i // N) % N - 8.0, i // (N * N) - 8.0
    psi0 = np.exp(-(x * x + y * y + z * z) / 18.0) * np.exp(1j * (0.7 * x - 0.4 * y + 0.2 * z))
    psi0 /= np.linalg.norm(psi0)
    out = {}
    for fmt in ("split", "csr"):
        c = cal.Context(spmv_format=fmt)
        try:
            P = cal.Propagator(H, psi0, 6, 4, ctx=c)
            on, sP, sH, ng = c.spmv_split_info()
            if fmt == "split":  # the stacked blkdiag(H, H) splits with the stride and reach of H alone
                assert (on, sP, sH, ng) == (True, 289, 18, True)
                assert c.matrix_info()["n_local"] == 2 * n
            else:
                assert not on
            assert P.step(0.05, 3) == 0
            out[fmt] = P.state()
            P.close()
        finally:
            c.close()
    assert np.all(np.isfinite(out["split"].view(float)))
    assert np.array_equal(out["split"], out["csr"])


def test_standard_lanczos_run_is_format_invariant(pair17, cal, ref):
    """y has the same bits in both formats, and the split kernel sums y'x in
    the CSR kernel's order (64-row wave sums, four per 256-row block), so alpha
    and with it the whole run are bit-identical."""
    A, split, csr = pair17
    r = ref.matlab_rand(A.shape[0])
    a = cal.lanczos_ex(A, r, 24, "local", ctx=split)
    b = cal.lanczos_ex(A, r, 24, "local", ctx=csr)
    assert a.info["fused"] == 1
    print("lanczos split vs csr: max |d alpha| %.3e, |d beta| %.3e, max |dQ| %.3e"
          % (np.max(np.abs(a.alpha - b.alpha)), np.max(np.abs(a.beta - b.beta)), np.max(np.abs(a.Q - b.Q))))
    assert np.array_equal(a.T, b.T) and np.array_equal(a.Q, b.Q)
