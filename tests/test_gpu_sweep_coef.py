"""The coefficient source of the block step's pass A and pass B (kernels.hip
k_rowapply COEF, chosen by launch_rowapply): the block-uniform matrix M read
from an LDS-staged table, or by uniform loads of the argument itself.  The
products, their order and the sums are the same, so with the source switched
to LDS (CAL_TEST_SWEEP_COEF_LDS) and to uniform loads
(CAL_TEST_SWEEP_COEF_SCALAR) every result has the same bits.

The GPU cases run in child processes on the test build
(libcalanczos_testhooks.so), which alone reads the two switches and exports
cal_test_sweep_coef (the source of the last device block orthogonalisation:
0 LDS, 1 uniform loads).  Each child prints one JSON line.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRELUDE = ("import sys, os, json, ctypes, numpy as np, scipy.sparse as sp; sys.path.insert(0, %r)\n"
           "import ca_lanczos_amd as cal\n"
           "from ca_lanczos_amd import _lib\n"
           "assert _lib.LIB_PATH.endswith('/libcalanczos_testhooks.so')\n"
           "from oracle import ca_lanczos_ref as ref\n"
           "lib = _lib.lib\n"
           "for f in (lib.cal_test_sweep_coef, lib.cal_test_sweep_policy):\n"
           "    f.restype = ctypes.c_int\n"
           "    f.argtypes = [ctypes.c_void_p]\n"
           "def switch(mode):\n"
           "    os.environ.pop('CAL_TEST_SWEEP_COEF_LDS', None)\n"
           "    os.environ.pop('CAL_TEST_SWEEP_COEF_SCALAR', None)\n"
           "    if mode: os.environ['CAL_TEST_SWEEP_COEF_' + mode] = '1'\n" % ROOT)

SWITCHES = ["CAL_TEST_SWEEP_COEF_LDS", "CAL_TEST_SWEEP_COEF_SCALAR", "cal_test_sweep_coef"]
STREAM = ["CAL_TEST_SWEEP_STREAM_ON", "CAL_TEST_SWEEP_STREAM_OFF"]


def run_testhooks(body, stream_on=False, timeout=240):
    e = dict(os.environ, CAL_LIBRARY="testhooks")
    for name in SWITCHES[:2] + STREAM:
        e.pop(name, None)
    if stream_on:
        e["CAL_TEST_SWEEP_STREAM_ON"] = "1"
    p = subprocess.run([sys.executable, "-c", PRELUDE + body], env=e, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


# projectAndNormalize on the device CholQR2 path (orth_device: P1, pass A,
# pass B): the inputs and oracle tolerances of tests/test_gpu_sweep_policy.py
# (tests/test_gpu_parity.py test_project_and_normalize_one_block, frac = 0.9)
BLOCK_STEP = r"""
n, w, m = %d, %d, %d
rng = np.random.RandomState(11)
Qp, _ = np.linalg.qr(rng.randn(n, w))
X = 0.9 * Qp @ rng.randn(w, m) + 0.1 * rng.randn(n, m) / np.sqrt(n) * 3
QZr, RZr, info = ref.projectAndNormalize_ex([Qp], X)
ctx = cal.Context()
ctx.set_normalize("cholqr2")
res, out = {}, dict(coef_before=int(lib.cal_test_sweep_coef(ctx.h)))
for mode in ("LDS", "SCALAR"):
    switch(mode)
    QZ, RZ, re, rank = cal.projectAndNormalize_ex([Qp], X, ctx=ctx)
    res[mode] = (QZ, RZ[0], RZ[1], re)
    out["coef_" + mode] = int(lib.cal_test_sweep_coef(ctx.h))
    out["policy_" + mode] = int(lib.cal_test_sweep_policy(ctx.h))
    out["oracle_" + mode] = dict(flag=bool(re == info.reorth), RY=float(np.max(np.abs(RZ[0] - RZr[0]))),
                                 R=float(np.max(np.abs(RZ[1] - RZr[1]))), Q=float(np.max(np.abs(QZ - QZr))),
                                 QtQp=float(np.max(np.abs(QZ.T @ Qp))))
a, b = res["LDS"], res["SCALAR"]
out.update(Q=bool(np.array_equal(a[0], b[0])), RY=bool(np.array_equal(a[1], b[1])),
           R=bool(np.array_equal(a[2], b[2])), flag=bool(a[3] == b[3]), finite=bool(np.isfinite(b[0]).all()))
ctx.close()
print(json.dumps(out))
"""


def check_block_step(out, policy):
    assert out["coef_before"] == -2
    assert out["coef_LDS"] == 0 and out["coef_SCALAR"] == 1, out
    assert out["policy_LDS"] == policy and out["policy_SCALAR"] == policy, out
    assert out["Q"] and out["R"] and out["RY"] and out["flag"] and out["finite"], out
    for mode in ("LDS", "SCALAR"):
        o = out["oracle_" + mode]
        assert o["flag"], out
        assert o["RY"] < 1e-12 and o["R"] < 1e-11 and o["Q"] < 1e-10 and o["QtQp"] < 1e-13, out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [200, 256, 257, 1000, 70001, 300001])
def test_block_step_coef_bitwise(n):
    """w = 9, m = 8 at less than a 256-row chunk, exactly one, a one-row tail,
    ragged, many blocks with a tail (70 001 rows) and several grid-stride
    rounds with a tail (300 001 rows): Q, R, RY and the reorth flag of the
    scalar-fed run equal the LDS-fed run's bit for bit, both are within the
    oracle tolerances of the parity test for the same call, and the getter
    shows each source was taken.  The load policy is off at these sizes, so
    the RES = -1 kernels (pass B storing plainly) are the ones compared."""
    out = run_testhooks(BLOCK_STEP % (n, 9, 8))
    print(json.dumps(out))
    check_block_step(out, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("w,m", [(9, 5), (3, 8)])
@pytest.mark.parametrize("n", [200, 256, 257, 1000, 70001, 300001])
def test_block_step_coef_bitwise_padded_shapes(n, w, m):
    """Shapes that reach the 17 x 8 instantiation through padding (14 and 11
    panel columns, 5 and 8 outputs; (9, 8) is the case above): the padded
    coefficient rows and columns are read from either source alike."""
    out = run_testhooks(BLOCK_STEP % (n, w, m))
    print(json.dumps(out))
    check_block_step(out, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [200, 256, 257, 1000, 70001, 300001])
def test_block_step_coef_bitwise_with_load_policy(n):
    """With CAL_TEST_SWEEP_STREAM_ON as well the sweeps are the load policy's
    (RES = 3, pass B storing non-temporally): the bench's kernels, LDS-fed
    against scalar-fed."""
    out = run_testhooks(BLOCK_STEP % (n, 9, 8), stream_on=True)
    print(json.dumps(out))
    check_block_step(out, 3)


SHORT_RUN = r"""
A = cal.matrices.%s
r = ref.matlab_rand(A.shape[0])
res, out = {}, {}
for mode in ("LDS", "SCALAR", ""):
    switch(mode)
    ctx = cal.Context()
    ctx.set_matrix(A)
    o = cal.ca_lanczos_ex(A, r, 8, 40, "newton", "local", diagnostics=False, ctx=ctx)
    res[mode] = o
    out["coef_" + (mode or "none")] = int(lib.cal_test_sweep_coef(ctx.h))
    ctx.close()
a, b = res["LDS"], res["SCALAR"]
out.update(T=bool(np.array_equal(a.T, b.T)), flags=bool(list(a.reorth) == list(b.reorth)),
           Q=bool(np.array_equal(a.Q, b.Q)), t=int(b.info["t"]), finite=bool(np.isfinite(b.Q).all()),
           nonzero=bool(np.any(b.Q[:, -1] != 0.0)))
print(json.dumps(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", ["laplacian_3d(12)", "laplacian_2d(40)"])
def test_short_run_coef_bitwise(matrix):
    """ca_lanczos, s = 8, Newton, 'local', 40 vectors (5 outer iterations): T,
    the reorth flags and Q of the scalar-fed run are the LDS-fed run's bits.
    Without a switch the launcher keeps LDS at these sizes: it takes the
    scalar source only for sweeps that stream from memory."""
    out = run_testhooks(SHORT_RUN % matrix)
    print(json.dumps(out))
    assert out["t"] == 5 and out["finite"] and out["nonzero"], out
    assert out["T"] and out["flags"] and out["Q"], out
    assert out["coef_LDS"] == 0 and out["coef_SCALAR"] == 1 and out["coef_none"] == 0, out


def test_production_library_carries_no_coef_switches():
    """The two switches and the getter live in the test build only."""
    prod = open(os.path.join(ROOT, "ca_lanczos_amd", "libcalanczos.so"), "rb").read()
    test = open(os.path.join(ROOT, "ca_lanczos_amd", "libcalanczos_testhooks.so"), "rb").read()
    present = [h for h in SWITCHES if h.encode() in prod]
    assert not present, present
    for h in SWITCHES:
        assert h.encode() in test, h
