"""The load policy of the block step's three sweeps (blockorth.cpp
sweep_policy, kernels.hip k_rowapply RES): non-temporal loads for every
column but the last R of X.  A load's cache policy changes no arithmetic, so
with the policy on (CAL_TEST_SWEEP_STREAM_ON: the chooser's R at any n) and
off (CAL_TEST_SWEEP_STREAM_OFF) every result has the same bits.

The GPU cases run in child processes on the test build
(libcalanczos_testhooks.so), which alone reads the two switches and exports
cal_test_sweep_policy (the policy of the last device block orthogonalisation:
-1 off, 0..3 resident columns).  Each child prints one JSON line.
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
           "lib.cal_test_sweep_policy.restype = ctypes.c_int\n"
           "lib.cal_test_sweep_policy.argtypes = [ctypes.c_void_p]\n"
           "def switch(mode):\n"
           "    os.environ.pop('CAL_TEST_SWEEP_STREAM_ON', None)\n"
           "    os.environ.pop('CAL_TEST_SWEEP_STREAM_OFF', None)\n"
           "    if mode: os.environ['CAL_TEST_SWEEP_STREAM_' + mode] = '1'\n" % ROOT)

SWITCHES = ["CAL_TEST_SWEEP_STREAM_ON", "CAL_TEST_SWEEP_STREAM_OFF", "cal_test_sweep_policy"]


def run_testhooks(body, timeout=240):
    e = dict(os.environ, CAL_LIBRARY="testhooks")
    for name in SWITCHES[:2]:
        e.pop(name, None)
    p = subprocess.run([sys.executable, "-c", PRELUDE + body], env=e, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


# projectAndNormalize on the device CholQR2 path (orth_device: P1, pass A,
# pass B) with w = 9, m = 8: the inputs and oracle tolerances of
# tests/test_gpu_parity.py test_project_and_normalize_one_block (frac = 0.9)
BLOCK_STEP = r"""
n, w, m = %d, 9, 8
rng = np.random.RandomState(11)
Qp, _ = np.linalg.qr(rng.randn(n, w))
X = 0.9 * Qp @ rng.randn(w, m) + 0.1 * rng.randn(n, m) / np.sqrt(n) * 3
QZr, RZr, info = ref.projectAndNormalize_ex([Qp], X)
ctx = cal.Context()
ctx.set_normalize("cholqr2")
res, out = {}, dict(policy_before=int(lib.cal_test_sweep_policy(ctx.h)))
for mode in ("OFF", "ON", ""):
    switch(mode)
    QZ, RZ, re, rank = cal.projectAndNormalize_ex([Qp], X, ctx=ctx)
    res[mode] = (QZ, RZ[0], RZ[1], re)
    out["policy_" + (mode or "none")] = int(lib.cal_test_sweep_policy(ctx.h))
    if mode:
        out["oracle_" + mode] = dict(flag=bool(re == info.reorth), RY=float(np.max(np.abs(RZ[0] - RZr[0]))),
                                     R=float(np.max(np.abs(RZ[1] - RZr[1]))), Q=float(np.max(np.abs(QZ - QZr))),
                                     QtQp=float(np.max(np.abs(QZ.T @ Qp))))
a, b = res["OFF"], res["ON"]
out.update(Q=bool(np.array_equal(a[0], b[0])), RY=bool(np.array_equal(a[1], b[1])),
           R=bool(np.array_equal(a[2], b[2])), flag=bool(a[3] == b[3]), finite=bool(np.isfinite(b[0]).all()))
ctx.close()
print(json.dumps(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("n", [200, 256, 257, 1000, 70001, 300001])
def test_block_step_policy_bitwise(n):
    """Less than a 256-row chunk, exactly one, a one-row tail, ragged, many
    blocks with a tail (70 001 rows = 274 chunks, one per block of the Gram
    sweeps) and several grid-stride rounds with a tail (300 001 rows = 1172
    chunks on the Gram sweeps' 512 blocks, so the prefetched next chunk is
    loaded under the policy too): Q, R, RY and the reorth flag of the switched-on
    run equal the switched-off run's bit for bit, and both are within the
    oracle tolerances of the parity test for the same call.  The getter shows
    the switched-on run took R = 3, the switched-off one and the one without
    a switch none (the chooser is off at these sizes).  Switched on, pass B
    is the policy's kernel, which also stores non-temporally; switched off it
    is the plain one: the stores' policy changes no bits either."""
    out = run_testhooks(BLOCK_STEP % n)
    print(json.dumps(out))
    assert out["policy_before"] == -2
    assert out["policy_OFF"] == -1 and out["policy_ON"] == 3 and out["policy_none"] == -1, out
    assert out["Q"] and out["R"] and out["RY"] and out["flag"] and out["finite"], out
    for mode in ("OFF", "ON"):
        o = out["oracle_" + mode]
        assert o["flag"], out
        assert o["RY"] < 1e-12 and o["R"] < 1e-11 and o["Q"] < 1e-10 and o["QtQp"] < 1e-13, out


SHORT_RUN = r"""
A = cal.matrices.%s
r = ref.matlab_rand(A.shape[0])
res, out = {}, {}
for mode in ("OFF", "ON", ""):
    switch(mode)
    ctx = cal.Context()
    ctx.set_matrix(A)
    o = cal.ca_lanczos_ex(A, r, 8, 40, "newton", "local", diagnostics=False, ctx=ctx)
    res[mode] = o
    out["policy_" + (mode or "none")] = int(lib.cal_test_sweep_policy(ctx.h))
    ctx.close()
a, b = res["OFF"], res["ON"]
out.update(T=bool(np.array_equal(a.T, b.T)), flags=bool(list(a.reorth) == list(b.reorth)),
           Q=bool(np.array_equal(a.Q, b.Q)), t=int(b.info["t"]), finite=bool(np.isfinite(b.Q).all()),
           nonzero=bool(np.any(b.Q[:, -1] != 0.0)))
print(json.dumps(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", ["laplacian_3d(12)", "laplacian_2d(40)"])
def test_short_run_policy_bitwise(matrix):
    """ca_lanczos, s = 8, Newton, 'local', 5 outer iterations: T, the reorth
    flags and Q with the policy switched on are the switched-off run's bits.
    Without a switch the policy is off at these sizes: the bench-size chooser
    does not reach small problems."""
    out = run_testhooks(SHORT_RUN % matrix)
    print(json.dumps(out))
    assert out["t"] == 5 and out["finite"] and out["nonzero"], out
    assert out["T"] and out["flags"] and out["Q"], out
    assert out["policy_OFF"] == -1 and out["policy_ON"] == 3 and out["policy_none"] == -1, out


def test_production_library_carries_no_sweep_switches():
    """The two switches and the getter live in the test build only."""
    prod = open(os.path.join(ROOT, "ca_lanczos_amd", "libcalanczos.so"), "rb").read()
    test = open(os.path.join(ROOT, "ca_lanczos_amd", "libcalanczos_testhooks.so"), "rb").read()
    present = [h for h in SWITCHES if h.encode() in prod]
    assert not present, present
    for h in SWITCHES:
        assert h.encode() in test, h
