"""GPU tests of the device-resident standard Lanczos (lanczos.m:18-311): the
fused Lanczos mode of the SpMV kernels in every instantiation, the four
orthogonalisations against the oracle (local, full) and against a NumPy
restatement of lanczos.m:136-311 (periodic, selective; tests/lanczos_std_ref.py),
the O(n) eigenvalue-only run, chunked stepping, breakdown, diagnostics, bad
arguments, and the fused step against the split one on the test build."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lanczos_std_ref as href  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


def arrow_matrix(n=3000):
    """diagonal 4, first row and first column dense (-1): row 0 has n entries
    and takes the CSR kernel's chunked long-row branch (> 2048 nonzeros)."""
    A = sp.lil_matrix((n, n))
    A.setdiag(4.0)
    A[0, 1:] = -1.0
    A[1:, 0] = -1.0
    return A.tocsr()


# name -> (matrix builder, spmv_format, expected path)
KERNEL_CASES = {
    "lap2d_37_pattern": (lambda cal: cal.matrices.laplacian_2d(37), "pattern", "pair"),
    "lap2d_257_planes_z2": (lambda cal: cal.matrices.laplacian_2d(257), "pattern", "planes"),
    "lap3d_17_planes": (lambda cal: cal.matrices.laplacian_3d(17), "pattern", "planes"),
    "lap3d_164_planes_z8": (lambda cal: cal.matrices.laplacian_3d(164), "pattern", "planes"),
    "lap2d_37_csr": (lambda cal: cal.matrices.laplacian_2d(37), "csr", "csr"),
    "arrow_3000_csr": (lambda cal: arrow_matrix(3000), "csr", "csr"),
}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_fused_kernel_every_instantiation(cal, name):
    build, fmt, path = KERNEL_CASES[name]
    A = build(cal).tocsr()
    n = A.shape[0]
    ctx = cal.Context(spmv_format=fmt).set_matrix(A)
    try:
        kind = ctx.spmv_format()[0]
        P, H, _ = ctx.spmv_plane_info()
        if path == "planes":
            assert kind == "pattern" and P >= 256, (kind, P)
            blocks8 = ((P + 511) // 512) * ((-(-n // P) + 7) // 8)  # the grid at 8 planes per block
            if name.endswith("z8"):  # it reaches CAL_SPMV_PLANES_MIN_BLOCKS: the headline's Z = 8 kernel
                assert blocks8 == 1113
            else:
                assert blocks8 < 1024
        elif path == "pair":
            assert kind == "pattern" and P == 0 and ctx.spmv_pair_info()[0] > 0
        else:
            assert kind == "csr"
        assert ctx.spmv_lanczos_fused() is True
        rng = np.random.default_rng(11)
        x, xprev = rng.standard_normal(n), rng.standard_normal(n)
        beta2 = 0.7
        b = math.sqrt(beta2)
        # without xprev: the bits of cal_spmv
        y0, d0 = ctx.spmv_lanczos(x, None, 0.0)
        assert np.array_equal(y0, ctx.spmv(x))
        y, d = ctx.spmv_lanczos(x, xprev, beta2)
        y2, d2 = ctx.spmv_lanczos(x, xprev, beta2)
        assert np.array_equal(y, y2) and d == d2  # fixed summation order
        # row-wise bound against an extended-precision reference
        Al = A.astype(np.longdouble)
        exact = Al @ x.astype(np.longdouble) - np.longdouble(b) * xprev.astype(np.longdouble)
        mag = np.asarray(abs(A) @ np.abs(x)) + np.abs(b * xprev)
        nnz_row = np.diff(A.indptr)
        err = np.abs((y.astype(np.longdouble) - exact).astype(np.float64))
        bound = (nnz_row + 2) * EPS * mag
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print("%s: max err / bound = %.3f" % (name, worst))
        assert np.all(err <= bound)
        for yy, dd in ((y0, d0), (y, d)):
            prod = yy * x
            exact_dot = math.fsum(prod.tolist())
            lim = n * EPS * float(np.sum(np.abs(prod)))
            print("%s: |dot - fsum| = %.3e (bound %.3e)" % (name, abs(dd - exact_dot), lim))
            assert abs(dd - exact_dot) <= lim
    finally:
        ctx.close()


# --------------------------------------------------------------------------
# local / full against the oracle
# --------------------------------------------------------------------------
MATS = {"lap2d_37": (lambda cal: cal.matrices.laplacian_2d(37), 8.0),
        "lap3d_17": (lambda cal: cal.matrices.laplacian_3d(17), 12.0)}
_oracle_cache = {}


def oracle_run(ref, cal, mat, seed, m, orth, diagnostics=False):
    key = (mat, seed, m, orth, diagnostics)
    if key not in _oracle_cache:
        A = MATS[mat][0](cal)
        r = np.random.default_rng(seed).standard_normal(A.shape[0])
        _oracle_cache[key] = (A, r) + tuple(ref.lanczos(A, r, m, orth, diagnostics))
    return _oracle_cache[key]


@pytest.mark.parametrize("mat", list(MATS))
@pytest.mark.parametrize("orth,m", [("local", 16), ("local", 24), ("local", 40), ("full", 24), ("full", 72)])
def test_local_and_full_against_the_oracle(cal, ref, mat, orth, m):
    normA = MATS[mat][1]
    for seed in (0, 1, 2):
        A, r, Qr, Tr, _, _ = oracle_run(ref, cal, mat, seed, m, orth)
        out = cal.lanczos_ex(A, r, m, orth)
        assert out.info["steps"] == m and out.info["breakdown"] == 0 and out.info["fused"] == 1
        dT = float(np.max(np.abs(out.T - Tr)))
        dQ = float(np.max(np.abs(out.Q - Qr)))
        print("%s %s m=%d seed %d: dT/|A| %.2e dQ %.2e" % (mat, orth, m, seed, dT / normA, dQ))
        assert dT <= 1e-12 * normA
        assert dQ <= 1e-11
        if orth == "full":
            oq = float(np.max(np.abs(out.Q.T @ out.Q - np.eye(m))))
            print("   |Q'Q - I| %.2e" % oq)
            assert oq <= 1e-13


def test_full_past_128_columns_splits_the_cgs_pass(cal, ref):
    """'full' at m = 136 on lap2d_37: from step 129 on Q(:,1:j) is projected
    in two blocks of columns (the Grams of both before the first update).
    T and |Q'Q - I| keep the bars of the shorter runs (the oracle: 8.9e-16).  Q
    itself is not compared here: the oracle's own Q moves by 2e-11 at this
    length when r is perturbed by one ulp, its T by 6e-15."""
    m = 136
    A, r, Qr, Tr, _, _ = oracle_run(ref, cal, "lap2d_37", 0, m, "full")
    out = cal.lanczos_ex(A, r, m, "full")
    assert out.info["steps"] == m and out.info["breakdown"] == 0
    dT = float(np.max(np.abs(out.T - Tr)))
    oq = float(np.max(np.abs(out.Q.T @ out.Q - np.eye(m))))
    print("full m=136: dT/|A| %.2e, |Q'Q - I| %.2e, dQ %.2e" % (dT / 8.0, oq, float(np.max(np.abs(out.Q - Qr)))))
    assert dT <= 1e-12 * 8.0
    assert oq <= 1e-13


def test_unfused_row_pattern_matrix_takes_the_split_step(cal, ref):
    """Nine entries per row in the row-pattern format: the pair kernel (rows of
    at most 8 entries) does not apply, the row kernels have no fused mode, so
    the solver runs SpMV mode 0 + the prologue's step and says so."""
    n = 1003
    offs = [-4, -3, -2, -1, 0, 1, 2, 3, 4]
    A = sp.diags([[-1.0] * (n - abs(o)) if o else [9.0] * n for o in offs], offs, format="csr")
    r = np.random.default_rng(3).standard_normal(n)
    ctx = cal.Context(spmv_format="pattern").set_matrix(A)
    try:
        assert ctx.spmv_format()[0] == "pattern" and ctx.spmv_plane_info()[0] == 0
        assert ctx.spmv_lanczos_fused() is False
        with pytest.raises(cal.CalError) as ei:
            ctx.spmv_lanczos(r, None, 0.0)
        assert ei.value.status == -6
        out = cal.lanczos_ex(A, r, 24, "local", ctx=ctx)
    finally:
        ctx.close()
    assert out.info["fused"] == 0 and out.info["steps"] == 24
    Qr, Tr, _, _ = ref.lanczos(A, r, 24, "local")
    normA = 17.0  # Gershgorin: 9 + 8
    assert float(np.max(np.abs(out.T - Tr))) <= 1e-12 * normA
    assert float(np.max(np.abs(out.Q - Qr))) <= 1e-11


def test_keep_q_0_same_bits_and_no_get_q(cal):
    A = cal.matrices.laplacian_3d(17)
    r = np.random.default_rng(0).standard_normal(A.shape[0])
    ctx = cal.Context().set_matrix(A)
    try:
        res = []
        for keep in (True, False):
            ctx.std_lanczos_begin(r, 40, "local", keep_Q=keep)
            ctx.std_lanczos_step(40)
            al, be, _, _, info = ctx.std_lanczos_get()
            res.append((al, be))
            if not keep:
                with pytest.raises(cal.CalError) as ei:
                    ctx.std_lanczos_get_Q(0, 1)
                assert ei.value.status == -1
            ctx.std_lanczos_end()
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert len(res[0][0]) == 40
    finally:
        ctx.close()


def test_step_chunking_gives_identical_bits(cal):
    A = cal.matrices.laplacian_3d(17)
    r = np.random.default_rng(0).standard_normal(A.shape[0])
    ctx = cal.Context().set_matrix(A)
    try:
        res = []
        for chunks in ([1] * 40, [10] * 4, [40]):
            ctx.std_lanczos_begin(r, 40, "local")
            for c in chunks:
                ctx.std_lanczos_step(c)
            al, be, _, _, _ = ctx.std_lanczos_get()
            res.append((al, be, ctx.std_lanczos_get_Q(0, 40)))
            ctx.std_lanczos_end()
        for other in res[1:]:
            for a, b in zip(res[0], other):
                assert np.array_equal(a, b)
    finally:
        ctx.close()


# --------------------------------------------------------------------------
# periodic / selective against the restatement of lanczos.m:136-311
# --------------------------------------------------------------------------
@pytest.mark.parametrize("orth", ["periodic", "selective"])
def test_periodic_selective_on_the_diagonal_matrix(cal, orth):
    A = href.diag_test_matrix()
    n, m, normA = A.shape[0], 48, 4.0
    r = np.random.default_rng(0).standard_normal(n)
    exp = href.lanczos(A, r, m, orth)
    ctx = cal.Context().set_matrix(A)
    try:
        ctx.std_lanczos_begin(r, m, orth)
        events, breaks = [], 0
        for j in range(1, m + 1):
            ctx.std_lanczos_step(1)
            info = ctx.std_lanczos_get()[4]
            if info["n_orth_breaks"] > breaks:
                breaks = info["n_orth_breaks"]
                events.append(j if orth == "periodic" else (j, info["n_ritz_locked"]))
        al, be, _, _, info = ctx.std_lanczos_get()
        Q = ctx.std_lanczos_get_Q(0, m)
        ctx.std_lanczos_end()
    finally:
        ctx.close()
    T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
    if orth == "periodic":
        assert exp.events == [14, 21, 28, 35, 42]
        assert info["n_orth_breaks"] == 5
    else:
        assert exp.events == [(13, 1), (15, 2), (16, 3), (17, 4)]
        assert info["n_orth_breaks"] == 4 and info["n_ritz_locked"] == 4
    assert events == exp.events
    assert abs(info["norm_A"] - exp.norm_A) <= 1e-12 * normA
    dT = float(np.max(np.abs(T - exp.T)))
    own = float(np.max(np.abs(exp.Q.T @ exp.Q - np.eye(m))))
    oq = float(np.max(np.abs(Q.T @ Q - np.eye(m))))
    print("%s: dT/|A| %.2e, |Q'Q - I| %.2e (restatement %.2e)" % (orth, dT / normA, oq, own))
    assert dT <= 1e-12 * normA
    assert oq <= 10.0 * own


@pytest.mark.parametrize("orth", ["periodic", "selective"])
def test_periodic_selective_without_events_are_local(cal, orth):
    A = cal.matrices.laplacian_2d(37)
    r = np.random.default_rng(0).standard_normal(A.shape[0])
    loc = cal.lanczos_ex(A, r, 48, "local")
    out = cal.lanczos_ex(A, r, 48, orth)
    assert out.info["n_orth_breaks"] == 0 and out.info["n_ritz_locked"] == 0
    assert out.info["steps"] == 48
    assert float(np.max(np.abs(out.T - loc.T))) <= 1e-12 * 8.0


def test_breakdown_on_an_exact_invariant_vector(cal):
    """A e_1 = 0 exactly on the diagonal matrix: beta_1 = 0."""
    A = href.diag_test_matrix()
    n = A.shape[0]
    r = np.zeros(n)
    r[0] = 1.0
    ctx = cal.Context().set_matrix(A)
    try:
        ctx.std_lanczos_begin(r, 8, "local")
        ctx.std_lanczos_step(8)
        al, be, rn, oe, info = ctx.std_lanczos_get()
        assert info["status"] == 2 and info["breakdown"] == 1 and info["steps"] == 1
        Q = ctx.std_lanczos_get_Q(0, 1)
        ctx.std_lanczos_end()
    finally:
        ctx.close()
    out = cal.lanczos_ex(A, r, 8, "local")
    assert out.info["status"] == 2 and out.info["steps"] == 1
    assert out.T.shape == (1, 1) and out.T[0, 0] == 0.0
    for a in (al, be, rn, oe, Q, out.T, out.Q, out.alpha, out.beta, out.ritz_rnorm, out.orth_err):
        assert np.all(np.isfinite(a))
    assert np.array_equal(out.Q[:, 0], r)


def test_diagnostics_against_the_oracle(cal, ref):
    A, r, Qr, Tr, rn_ref, oe_ref = oracle_run(ref, cal, "lap2d_37", 0, 12, "full", True)
    out = cal.lanczos_ex(A, r, 12, "full", diagnostics=True)
    assert out.ritz_rnorm.shape == (12, 12) and out.orth_err.shape == (12,)
    err = np.abs(out.ritz_rnorm - rn_ref)
    lim = 1e-9 * np.maximum(rn_ref, 1e-6)
    print("rn: max err / bound %.3e; oe: max err %.3e" % (float(np.max(err / lim)), float(np.max(np.abs(out.orth_err - oe_ref)))))
    assert np.all(err <= lim)
    assert np.all(np.abs(out.orth_err - oe_ref) <= 1e-14)
    # the diagnostics never feed back
    plain = cal.lanczos_ex(A, r, 12, "full")
    assert np.array_equal(plain.T, out.T) and np.array_equal(plain.Q, out.Q)
    T4, Q4, rn4, oe4 = cal.lanczos(A, r, 12, "full")
    assert np.array_equal(T4, out.T) and np.array_equal(rn4, out.ritz_rnorm)


def test_bad_arguments(cal):
    from ca_lanczos_amd import _lib

    A = cal.matrices.laplacian_2d(12)
    n = A.shape[0]
    r = np.ones(n)
    ctx = cal.Context().set_matrix(A)
    try:
        lib, p = _lib.lib, _lib.ptr
        assert lib.cal_std_lanczos_begin(ctx.h, p(r), 8, b"fro", 1) == _lib.CAL_ERR_ARG  # unknown orth
        assert lib.cal_std_lanczos_begin(ctx.h, p(r), 0, b"local", 1) == _lib.CAL_ERR_ARG
        assert lib.cal_std_lanczos_begin(ctx.h, p(r), n + 1, b"local", 1) == _lib.CAL_ERR_ARG
        assert lib.cal_std_lanczos_begin(ctx.h, p(r), 8, b"full", 0) == _lib.CAL_ERR_ARG  # keep_Q = 0 needs local
        assert lib.cal_std_lanczos_step(ctx.h, 1, 0) == _lib.CAL_ERR_ARG  # step before begin
        T = np.zeros((8, 8), order="F")
        assert lib.cal_lanczos(ctx.h, p(r), 8, b"nope", 0, p(T), None, None, None, None) == _lib.CAL_ERR_ARG
        # the context still works
        x = np.arange(n, dtype=float)
        assert np.array_equal(ctx.spmv(x), A @ x)
        out = cal.lanczos_ex(A, r + x, 8, "local", ctx=ctx)
        assert out.info["steps"] == 8
        ctx.std_lanczos_begin(r + x, 4, "local")
        with pytest.raises(cal.CalError):
            ctx.std_lanczos_step(5)  # past maxiter
        ctx.std_lanczos_end()
    finally:
        ctx.close()


# --------------------------------------------------------------------------
# fused against split, on the test build (a fresh child process each)
# --------------------------------------------------------------------------
CHILD = r"""
import sys, os, json, numpy as np
sys.path.insert(0, %r)
import ca_lanczos_amd as cal
from ca_lanczos_amd import _lib
assert _lib.LIB_PATH.endswith('/libcalanczos_testhooks.so')
A = cal.matrices.laplacian_3d(17)
r = np.random.default_rng(0).standard_normal(A.shape[0])
out = cal.lanczos_ex(A, r, 40, 'local')
np.save(sys.argv[1], np.column_stack([out.Q[:, 0], out.Q[:, 1]]))
print(json.dumps(dict(fused=out.info['fused'], steps=out.info['steps'], alpha=out.alpha.tolist(),
                      beta=out.beta.tolist())))
""" % ROOT


def run_child(tmp_path, tag, **env):
    e = dict(os.environ, CAL_LIBRARY="testhooks")
    e.pop("CAL_TEST_LANCZOS_SPLIT", None)
    e.update(env)
    qfile = str(tmp_path / ("q_%s.npy" % tag))
    p = subprocess.run([sys.executable, "-c", CHILD, qfile], env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    row = json.loads(p.stdout.strip().splitlines()[-1])
    return row, np.load(qfile)


def test_fused_against_split_on_the_test_build(tmp_path):
    """lap3d_17, local, m = 40, with and without CAL_TEST_LANCZOS_SPLIT."""
    fu, qf = run_child(tmp_path, "fused")
    sp_, qs = run_child(tmp_path, "split", CAL_TEST_LANCZOS_SPLIT="1")
    assert fu["fused"] == 1 and sp_["fused"] == 0
    assert fu["steps"] == 40 and sp_["steps"] == 40
    da = float(np.max(np.abs(np.array(fu["alpha"]) - np.array(sp_["alpha"]))))
    db = float(np.max(np.abs(np.array(fu["beta"]) - np.array(sp_["beta"]))))
    print("fused vs split: max |d alpha| %.3e, |d beta| %.3e; Q(:,1:2) differing entries %d"
          % (da, db, int(np.count_nonzero(qf != qs))))
    assert max(da, db) <= 1e-13 * 12.0
    assert np.array_equal(qf, qs)
