#!/usr/bin/env python
"""Time steps/s of the Krylov time propagator on a stacked Laplacian.

  python tools/prop_bench.py [--workload lap3d_215] [--s 8] [--blocks 3]
                             [--steps 50] [--warmup 5] [--out profiles/prop/NAME.json]

Workload: psi <- exp(-i dt H) psi with H = lap3d_N (or lap2d_N), embedded as
blkdiag(H, H) (2n rows), Newton basis, a complex Gaussian packet as the start
state.  Measured, in runs of their own:
  1. wall time of --steps time steps after --warmup (timers off): steps/s;
  2. the same steps with the library's HIP-event timers on: per-kind kernel
     time per time step;
  3. the steady-state outer iteration of a plain CA-Lanczos loop on the same
     stacked matrix (3 warm-up iterations, 12 timed), the yardstick "blocks x
     the per-outer-iteration time at twice the rows";
  4. the combine kernel alone through cal_prop_combine (the library timer
     brackets the kernel only): mean time and rate over (2n m + 2n) 8 bytes;
  5. cal_expm_col1 on T's of s, 2s, ... s*blocks rows on the host.
Also records what cal_spmv_plane_info / cal_spmv_format report for the
stacked matrix and for H alone, whether the stacked SpMV equals H applied to
each half bit for bit, and the norm drift over the run (unitarity).
Prints one JSON line; --out also writes it to a file.

  python tools/prop_bench.py --windows 5 [--window-steps 4] [--observables NW,NPHI[,energy]]...
                             [--absorber] [--copyback] [--combine-kernel] [--package-root DIR]

The window mode (instead of 1.-5.): every leg is a fresh Propagator on one
context, 2 warm-up steps, then --windows host-clock windows of --window-steps
synchronised time steps (the counts of tools/hamiltonian_bench.py), and a run
of --timed-steps steps with the library's timers on (kernel time per class
and step; class "spmv" also with its launch count).  Legs:
  plain          no observables set;
  obs_NW_NPHI[_energy]
                 per --observables: NW diagonal operators (coordinates, r^2)
                 and NPHI reference states (shifted copies of the start
                 state) reduced on the device inside the combine sweep;
  copyback_...   (--copyback) what that replaces: the same steps with
                 P.state() copied back after every step and the same sums
                 done in NumPy;
  absorber       (--absorber) matrices.absorber_mask (width N/8) set with
                 set_absorber: the mask applied and the absorbed norm summed
                 inside the combine sweep;
  copyback_absorber
                 (--absorber --copyback) what that replaces: after every step
                 the state is copied back, multiplied by the mask in NumPy and
                 handed to a new Propagator.
--combine-kernel adds the combine kernel alone with each --observables set
through cal_prop_combine_obs, bytes (2n m + 2n + n NW + 2n NPHI) 8, next to
the plain one, and with --absorber the masked kernel alone through
cal_prop_combine_masked, bytes (2n m + 3n) 8.  --package-root imports ca_lanczos_amd from another checkout
(its built library), e.g. the parent commit's for an A/B in alternating
fresh processes; such a checkout need not know the observables.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="lap3d_215")
    ap.add_argument("--s", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timed-steps", type=int, default=10, help="time steps of the run with the timers on")
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--start", default="packet", choices=("packet", "random"),
                    help="start state: a smooth complex Gaussian packet, or random (a well-conditioned Krylov basis)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=0, help="window mode: timed windows per leg (0: the default report)")
    ap.add_argument("--window-steps", type=int, default=4)
    ap.add_argument("--observables", action="append", default=[], metavar="NW,NPHI[,energy]")
    ap.add_argument("--combine-kernel", action="store_true")
    ap.add_argument("--absorber", action="store_true", help="window mode: also the leg with an absorbing mask set")
    ap.add_argument("--copyback", action="store_true", help="window mode: also the copy-back leg of every --observables")
    ap.add_argument("--package-root", default=None, help="import ca_lanczos_amd from this checkout")
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))

    import ca_lanczos_amd as cal
    kind, N = a.workload.split("_")
    N = int(N)
    dim = 3 if kind == "lap3d" else 2
    H = cal.matrices.laplacian_3d(N) if dim == 3 else cal.matrices.laplacian_2d(N)
    n = H.shape[0]
    idx = np.arange(n)
    coords = [(idx // N ** d) % N for d in range(dim)]
    r2 = sum((c - 0.5 * (N - 1)) ** 2 for c in coords)
    phase = sum(k * c for k, c in zip((0.7, 0.3, 0.2), coords))
    psi0 = np.exp(-r2 / (2 * (N / 8.0) ** 2)) * np.exp(1j * phase)
    del idx, coords, r2, phase
    if a.start == "random":
        rng = np.random.RandomState(1)
        psi0 = rng.randn(n) + 1j * rng.randn(n)

    res = dict(workload=a.workload, start=a.start, n=n, rows=2 * n, s=a.s, blocks=a.blocks, m=a.s * a.blocks, dt=a.dt,
               steps=a.steps, warmup=a.warmup)
    if a.windows > 0:
        res.update(windows=a.windows, window_steps=a.window_steps, package=os.path.dirname(cal.__file__),
                   library=os.path.basename(cal.LIB_PATH))
        del res["steps"], res["warmup"]
        window_mode(cal, a, H, psi0, N, dim, res)
        return emit(res, a.out)
    alone = cal.Context().set_matrix(H)
    res["H_alone"] = dict(spmv_format=alone.spmv_format(), plane_info=alone.spmv_plane_info())
    half_re, half_im = alone.spmv(psi0.real), alone.spmv(psi0.imag)
    alone.close()

    ctx = cal.Context()
    P = cal.Propagator(H, psi0, a.s, a.blocks, basis="newton", ctx=ctx)
    res["stacked"] = dict(spmv_format=ctx.spmv_format(), plane_info=ctx.spmv_plane_info(),
                          pair_info=ctx.spmv_pair_info(), matrix_info=ctx.matrix_info())
    # the stacked SpMV is H on each half, bit for bit (also across the seam at row n)
    y = ctx.spmv(np.concatenate([psi0.real, psi0.imag]))
    res["spmv_stacked_equals_halves"] = bool(np.array_equal(y[:n], half_re) and np.array_equal(y[n:], half_im))
    del y, half_re, half_im
    n0 = P.info()["norm"]
    P.step(a.dt, a.warmup)
    ctx.synchronize()
    t0 = time.perf_counter()
    P.step(a.dt, a.steps)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    info = P.info()
    res.update(steps_per_s=a.steps / wall, ms_per_step=1e3 * wall / a.steps, norm_drift=abs(info["norm"] - n0),
               lsteps=info["lsteps"], breakdowns=info["breakdowns"], rank_deficient=info["rank_deficient"],
               residual_max=info["residual_max"], tsqr_fold_stats=ctx.tsqr_fold_stats(),
               normalize=ctx.normalize_backend())

    # 2. the kernel classes of a time step
    ctx.timer_enable(True)
    ctx.timer_reset()
    P.step(a.dt, a.timed_steps)
    ctx.synchronize()
    prop_t = {k: ctx.timer_read(k) for k in ("spmv", "gram", "apply", "other")}
    prop_b = ctx.timer_bytes("apply")
    ctx.timer_enable(False)
    res["kernel_ms_per_step"] = {k: v[1] / a.timed_steps for k, v in prop_t.items()}
    P.close()

    # 3. the steady-state outer iteration of the plain CA-Lanczos loop on the
    # same matrix (bench.py's measure: warm-up iterations, then timed ones)
    x0 = np.concatenate([psi0.real, psi0.imag])
    wu, it = 3, 12
    ctx.lanczos_begin(x0, a.s, wu + it, "newton", "local")
    for _ in range(wu):
        ctx.lanczos_step(False)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(it):
        ctx.lanczos_step(False)
    ctx.synchronize()
    res["outer_iteration_ms"] = 1e3 * (time.perf_counter() - t0) / it
    ctx.lanczos_end()

    # the combine kernel alone, through the host-pointer entry (its timer
    # brackets the kernel only): one untimed launch, then three timed ones
    Q = np.ones((2 * n, a.s * a.blocks), order="F")
    c = np.exp(1j * np.arange(a.s * a.blocks)) / np.sqrt(a.s * a.blocks)
    ctx.prop_combine(Q, c)
    ctx.timer_enable(True)
    ctx.timer_reset()
    for _ in range(3):
        ctx.prop_combine(Q, c)
    cnt, cms = ctx.timer_read("apply")
    cbytes = ctx.timer_bytes("apply")
    ctx.timer_enable(False)
    del Q
    comb_ms = cms / cnt
    res["combine"] = dict(launches=cnt, ms=comb_ms, bytes=cbytes / cnt,
                          expected_bytes=(2.0 * n * a.s * a.blocks + 2.0 * n) * 8,
                          tb_per_s=cbytes / (cms * 1e-3) / 1e12)
    ctx.close()

    # 4. the host exponential of one time step (after every block)
    rng = np.random.RandomState(0)
    tex = 0.0
    for k in range(1, a.blocks + 1):
        m = k * a.s
        T = np.diag(3 + rng.rand(m)) + np.diag(rng.rand(m - 1), 1)
        T = T + np.triu(T, 1).T
        t0 = time.perf_counter()
        for _ in range(20):
            cal.expm_col1(T, a.dt)
        tex += (time.perf_counter() - t0) / 20
    res["expm_ms_per_step"] = 1e3 * tex
    ms = res["ms_per_step"]
    loop = a.blocks * res["outer_iteration_ms"]
    # blocks x the steady outer iteration, the combine, the host exponential;
    # the rest is the begin (normalise, T reset) and what the first block
    # (normalize of s + 1 columns) costs beyond a steady one
    res["share"] = dict(blocks_x_outer_iteration=loop / ms, combine=comb_ms / ms,
                        expm=res["expm_ms_per_step"] / ms,
                        begin_first_block_and_rest=1.0 - (loop + comb_ms + res["expm_ms_per_step"]) / ms)
    emit(res, a.out)


def emit(res, out):
    line = json.dumps(res, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def parse_observables(spec):
    p = spec.split(",")
    if len(p) not in (2, 3) or (len(p) == 3 and p[2] != "energy"):
        raise SystemExit("--observables takes NW,NPHI[,energy], not %r" % spec)
    return int(p[0]), int(p[1]), len(p) == 3


def observable_set(n, N, dim, psi0, nw, nphi):
    """nw real diagonal operators (the coordinates about the centre, then
    r^2) and nphi reference states (the start state shifted by r rows)."""
    idx = np.arange(n)
    coords = [(idx // N ** d) % N - 0.5 * (N - 1) for d in range(dim)]
    ops = coords + [sum(c * c for c in coords)]
    W = [ops[k % len(ops)] * (1.0 + k // len(ops)) for k in range(nw)]
    phi = [np.roll(psi0, r) for r in range(nphi)]
    return W, phi


def window_mode(cal, a, H, psi0, N, dim, res):
    n = H.shape[0]
    ctx = cal.Context()

    def leg(setup, after_step):
        """ms per step of every window, then the timers' kernel classes over --timed-steps steps."""
        P = cal.Propagator(H, psi0, a.s, a.blocks, basis="newton", ctx=ctx)
        setup(P)
        sums = []

        def steps(k):
            if after_step is None:
                P.step(a.dt, k)
            else:
                for _ in range(k):
                    P.step(a.dt, 1)
                    sums.append(after_step(P))
            ctx.synchronize()

        steps(2)
        ms = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            steps(a.window_steps)
            ms.append(1e3 * (time.perf_counter() - t0) / a.window_steps)
        ctx.timer_enable(True)
        ctx.timer_reset()
        steps(a.timed_steps)
        t = {k: ctx.timer_read(k) for k in ("spmv", "gram", "apply", "other")}
        ctx.timer_enable(False)
        info = P.info()
        out = dict(ms_per_step=ms, kernel_ms_per_step={k: v[1] / a.timed_steps for k, v in t.items()},
                   spmv_launches_per_step=t["spmv"][0] / a.timed_steps, lsteps=info["lsteps"],
                   breakdowns=info["breakdowns"], residual_max=info["residual_max"])
        last = P.observables() if hasattr(P, "observables") else None
        P.close()
        return out, last, sums

    legs = {}
    legs["plain"], _, _ = leg(lambda P: None, None)
    for spec in a.observables:
        nw, nphi, energy = parse_observables(spec)
        W, phi = observable_set(n, N, dim, psi0, nw, nphi)
        name = "%d_%d%s" % (nw, nphi, "_energy" if energy else "")
        legs["obs_" + name], hist, _ = leg(lambda P: P.set_observables(W=W, phi=phi, energy=energy), None)
        legs["obs_" + name]["expected_combine_bytes"] = (2.0 * n * a.s * a.blocks + 2.0 * n + n * nw + 2.0 * n * nphi) * 8
        Wm = np.column_stack(W) if nw else np.zeros((n, 0))
        Pm = np.column_stack(phi) if nphi else np.zeros((n, 0), dtype=complex)

        def numpy_sums(P):
            psi = P.state()
            d = psi.real ** 2 + psi.imag ** 2
            E = float(psi.real @ (H @ psi.real) + psi.imag @ (H @ psi.imag)) if energy else float("nan")
            return float(np.sum(d)), E, Wm.T @ d, Pm.conj().T @ psi

        if not a.copyback:
            continue
        legs["copyback_" + name], _, sums = leg(lambda P: None, numpy_sums)
        # the two legs take the same steps from the same start: their last sums agree to rounding
        n2, E, wv, ov = sums[-1]
        legs["copyback_" + name]["last_vs_device"] = dict(
            norm2=abs(n2 - hist["norm2"][-1]) / n2, energy=abs(E - hist["energy"][-1]) / abs(E) if energy else None,
            W=float(np.max(np.abs(wv - hist["W"][-1]) / (np.abs(Wm).T @ np.abs(psi0) ** 2))) if nw else None,
            overlap=float(np.max(np.abs(ov - hist["overlap"][-1]))) / n2 if nphi else None)
    mask = cal.matrices.absorber_mask((N,) * dim, max(N // 8, 1)) if a.absorber else None
    if a.absorber:
        legs["absorber"], _, _ = leg(lambda P: P.set_absorber(mask), None)
        legs["absorber"]["expected_combine_bytes"] = (2.0 * n * a.s * a.blocks + 3.0 * n) * 8
    if a.absorber and a.copyback:
        # a new propagator per step: the state goes back, is masked in NumPy and uploaded again
        def masked_steps(psi, k):
            for _ in range(k):
                P = cal.Propagator(H, psi, a.s, a.blocks, basis="newton", ctx=ctx)
                P.step(a.dt, 1)
                psi = mask * P.state()
                P.close()
            return psi

        psi = masked_steps(psi0, 2)
        ms = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            psi = masked_steps(psi, a.window_steps)
            ms.append(1e3 * (time.perf_counter() - t0) / a.window_steps)
        legs["copyback_absorber"] = dict(ms_per_step=ms, norm2_left=float(np.sum(np.abs(psi) ** 2) /
                                                                          np.sum(np.abs(psi0) ** 2)))
    res["legs"] = legs

    if a.combine_kernel:
        m = a.s * a.blocks
        Q = np.ones((2 * n, m), order="F")
        c = np.exp(1j * np.arange(m)) / np.sqrt(m)

        def timed(call, expected):
            call()
            ctx.timer_enable(True)
            ctx.timer_reset()
            for _ in range(3):
                call()
            cnt, cms = ctx.timer_read("apply")
            cbytes = ctx.timer_bytes("apply")
            ctx.timer_enable(False)
            return dict(launches=cnt, ms=cms / cnt, bytes=cbytes / cnt, expected_bytes=expected,
                        tb_per_s=cbytes / (cms * 1e-3) / 1e12)

        base = (2.0 * n * m + 2.0 * n) * 8
        ck = dict(plain=timed(lambda: ctx.prop_combine(Q, c), base))
        for spec in a.observables:
            nw, nphi, _ = parse_observables(spec)
            W, phi = observable_set(n, N, dim, psi0, nw, nphi)
            r = timed(lambda: ctx.prop_combine_obs(Q, c, W, phi), base + (n * nw + 2.0 * n * nphi) * 8)
            r["expected_ms_from_byte_ratio"] = ck["plain"]["ms"] * r["expected_bytes"] / base
            ck["obs_%d_%d" % (nw, nphi)] = r
        if a.absorber:
            r = timed(lambda: ctx.prop_combine_masked(Q, c, mask), base + n * 8.0)
            r["expected_ms_from_byte_ratio"] = ck["plain"]["ms"] * r["expected_bytes"] / base
            ck["absorber"] = r
        res["combine_kernel"] = ck
    ctx.close()


if __name__ == "__main__":
    main()
