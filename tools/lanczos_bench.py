#!/usr/bin/env python
"""Lanczos vectors/s of the standard Lanczos step on one GPU, fused against
split, beside the CA loop's figure of the same session.

  python tools/lanczos_bench.py [--workload lap3d_215] [--steps 200] [--repeats 5]
                                [--warmup 50] [--rounds 2] [--no-ca]
                                [--out profiles/lanczos/NAME.json]

Workload: lanczos(A, r, m, 'local') with keep_Q = 0 (three columns on the
device), r = default_rng(0).standard_normal(n).  Each measurement runs in a
fresh child process (the library is chosen at import):
  fused   the production library: SpMV mode 4 + k_pro_update + k_pro_div;
  split   the test build with CAL_TEST_LANCZOS_SPLIT=1: SpMV mode 0 +
          k_pro_dot + k_pro_update + k_pro_div;
alternating, --rounds times each.  A child warms up --warmup steps, then
times --repeats windows of step(--steps) with cal_synchronize around each
(median, min, max), then runs 20 steps with the library's HIP-event timers on
(per-kind kernel time and stated bytes per vector).  Last, unless --no-ca,
`bench.py --gpus 1 --steps 20 --warmup 3` runs in its own process: its
headline (outer iterations/s) x s = 8 is the CA loop's vectors/s.
Prints one JSON line; --out also writes it to a file.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload_matrix(cal, name):
    kind, N = name.split("_")
    return cal.matrices.laplacian_3d(int(N)) if kind == "lap3d" else cal.matrices.laplacian_2d(int(N))


def child(a):
    import numpy as np

    import ca_lanczos_amd as cal
    from ca_lanczos_amd import _lib

    A = workload_matrix(cal, a.workload)
    n = A.shape[0]
    r = np.random.default_rng(0).standard_normal(n)
    ctx = cal.Context().set_matrix(A)
    timed = 20
    ctx.std_lanczos_begin(r, a.warmup + a.repeats * a.steps + timed, "local", keep_Q=False)
    ctx.std_lanczos_step(a.warmup)
    ctx.synchronize()
    ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ctx.std_lanczos_step(a.steps)
        ctx.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    ctx.timer_enable(True)
    ctx.timer_reset()
    ctx.std_lanczos_step(timed)
    ctx.synchronize()
    kinds = {k: ctx.timer_read(k) for k in ("spmv", "other")}
    kbytes = {k: ctx.timer_bytes(k) for k in ("spmv", "other")}
    ctx.timer_enable(False)
    al, be, _, _, info = ctx.std_lanczos_get()
    ctx.std_lanczos_end()
    med = statistics.median(ms)
    out = dict(library=os.path.basename(_lib.LIB_PATH), split_switch=bool(os.environ.get("CAL_TEST_LANCZOS_SPLIT")),
               fused=info["fused"], n=n, steps=a.steps, repeats=a.repeats, warmup=a.warmup,
               window_ms=ms, median_ms=med, min_ms=min(ms), max_ms=max(ms),
               vectors_per_s=a.steps / (med * 1e-3), us_per_vector=1e3 * med / a.steps,
               spmv_format=ctx.spmv_format(), plane_info=ctx.spmv_plane_info(),
               kernel_us_per_vector={k: 1e3 * v[1] / timed for k, v in kinds.items()},
               launches_per_vector={k: v[0] / timed for k, v in kinds.items()},
               stated_bytes_per_vector_over_n={k: v / timed / n for k, v in kbytes.items()},
               steps_kept=info["steps"], breakdown=info["breakdown"],
               alpha_last=float(al[-1]), beta_last=float(be[-1]))
    ctx.close()
    print(json.dumps(out))


def run_child(a, split):
    env = dict(os.environ)
    env.pop("CAL_TEST_LANCZOS_SPLIT", None)
    env.pop("CAL_LIBRARY", None)
    if split:
        env["CAL_LIBRARY"] = "testhooks"
        env["CAL_TEST_LANCZOS_SPLIT"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--steps", str(a.steps),
           "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="lap3d_215")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-ca", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    if a.child:
        return child(a)

    res = dict(workload=a.workload, steps=a.steps, repeats=a.repeats, warmup=a.warmup, rounds=a.rounds,
               fused_runs=[], split_runs=[])
    for _ in range(a.rounds):  # alternating, each in a fresh process
        res["fused_runs"].append(run_child(a, False))
        res["split_runs"].append(run_child(a, True))

    def summary(runs):
        w = [x for r in runs for x in r["window_ms"]]
        med = statistics.median(w)
        return dict(median_ms=med, min_ms=min(w), max_ms=max(w), spread=(max(w) - min(w)) / med,
                    vectors_per_s=a.steps / (med * 1e-3), us_per_vector=1e3 * med / a.steps)

    res["fused"], res["split"] = summary(res["fused_runs"]), summary(res["split_runs"])
    res["fused_over_split"] = res["split"]["median_ms"] / res["fused"]["median_ms"]
    # faster by more than the run-to-run spread of the two: the windows do not overlap
    res["fused_faster_beyond_spread"] = bool(res["fused"]["max_ms"] < res["split"]["min_ms"])
    if not a.no_ca:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20",
                            "--warmup", "3"], capture_output=True, text=True, timeout=900)
        line = None
        for ln in p.stdout.strip().splitlines():
            if ln.startswith("{"):
                line = ln
        if p.returncode != 0 or line is None:
            raise RuntimeError("bench.py failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
        b = json.loads(line)
        res["ca"] = dict(metric=b.get("metric"), outer_it_per_s=b.get("value"), s=8,
                         vectors_per_s=None if b.get("value") is None else 8.0 * b["value"])
        if res["ca"]["vectors_per_s"]:
            res["fused_over_ca"] = res["fused"]["vectors_per_s"] / res["ca"]["vectors_per_s"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
