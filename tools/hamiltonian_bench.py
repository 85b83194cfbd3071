#!/usr/bin/env python
"""The diagonal-split SpMV format on a grid Hamiltonian K + diag(V), against
the same matrix on CSR and against the plain Laplacian's plane march.

  python tools/hamiltonian_bench.py [--N 215] [--rounds 2] [--windows 5]
                                    [--only spmv,ca,lanczos,prop]
                                    [--library NAME] [--out profiles/dsplit/NAME.json]
                                    [--drive LIST] [--package-root DIR]
                                    [--imaginary stacked,real]

Matrix: grid_hamiltonian((N, N, N), V) with the harmonic potential V = 0.5 w^2
|x - x0|^2 (w = 0.02: V of the size of the kinetic term), h = mass = 1, so the
off-diagonals are -1/2 (the general uniform-value kernel, not NEG1).  Variants,
each in a fresh child process, alternating, --rounds times each:
  split  Context(spmv_format="split")
  csr    Context(spmv_format="csr")         the A/B partner
  lap    laplacian_3d(N), format "auto"     the plane march, the yardstick
  shared Context(spmv_format="shared").set_matrix_stacked(H): blkdiag(H, H) with
         H stored once -- every leg (spmv, lanczos, prop; no ca) on the 2n rows
  csr2   Context(spmv_format="csr").set_matrix_stacked(H): the stacked CSR
         matrix, shared's A/B partner, same legs on the same 2n rows
  herm   Context(spmv_format="shared").set_matrix_hermitian(H) with H =
         peierls_hamiltonian on N^3 (the same potential, flux 1/16 per
         plaquette): the complex Hermitian H stored once (k_spmv_stacked, HERM true), the
         stacked legs on the 2n rows of [[A, -B], [B, A]]
  herm_csr  the same H with spmv_format="csr": the host-built embedding on the
         existing CSR kernel, herm's A/B partner ("herm_vs_herm_csr"; "herm_vs_shared"
         holds herm against the real shared leg)
A child measures, in --windows (>= 5) windows each after a warm-up:
  spmv     mode 0 back to back, 50 launches per window, each bracketed by the
           library's device events (cal_bench_spmv): mean us per launch;
  ca       the CA loop (s = 8, Newton, 'local'), 10 outer iterations per
           window, host clock around synchronised windows as bench.py;
  lanczos  fused standard Lanczos, keep_Q = 0, 100 steps per window, as
           tools/lanczos_bench.py;
  prop     the propagator on blkdiag(H, H), s = 8, 3 blocks, 4 time steps per
           window, as tools/prop_bench.py.
--drive LIST (comma separated, default 0) runs the prop leg once per entry, each
in a child of its own ("VARIANT+driveK"): 0 undriven; NK = 1 .. 4 under the
drive H(t) = H0 + sum_k f_k(t) diag(W_k) with NK operators (the coordinates
about the centre, then r^2; midpoint amplitudes 1e-3 sin((k + 1) t)), where the
child also reports the drive kernel's own time (the library's "drive" timer
class over 10 driven steps) and its rate over the bytes the library counts,
(8 (1 + NK) + 4 * 2) n in + 16 * 2 * n out (8 * 2 * n on CSR); "reupload"
is what the drive replaces, set_matrix_stacked of the new H (the diagonal
rewritten in the host's CSR copy) before every step, 2 steps per window.
--nonlinear LIST (comma separated, e.g. frozen,midpoint,copyback) adds prop legs
under the Gross-Pitaevskii term g |psi|^2 (g = 0.05; the start state's largest
|psi|^2 is 1), each in a child of its own ("VARIANT+nlNAME"), undriven:
"frozen" and "midpoint" are Propagator.set_nonlinear's two densities, where the
child also reports the density kernel's own time (the "drive" timer class over
10 steps: one launch per step "frozen", two "midpoint"); "copyback" is the
route they replace -- state() back to the host, |psi|^2 and the new diagonal in
NumPy, and a new Propagator on the rewritten matrix, every step (the frozen
scheme; 2 steps per window).
--imaginary LIST (stacked, real) adds prop legs in imaginary time, tau = --dt,
each in a child of its own ("VARIANT+imstacked", "VARIANT+imreal"), and with
--nonlinear frozen also under g |psi|^2 ("...+nlfrozen"): "stacked" is
Propagator.set_imaginary_time on blkdiag(H, H), "real" is Propagator(...,
real=True) on H itself.  Both start from the packet's real envelope |psi0| (a
step's cost follows the state, so the two legs must relax the same one; the
stacked leg's imaginary half then stays zero, which is the work the real path
saves).  The summary's "imaginary_real_vs_stacked" has the ratio of the
medians and, window class by window class, of the fastest and of the slowest
windows.  The
variant "auto" (format "auto") is there for the real leg: whatever the upload
picks for H alone.  An imaginary child also times its combine kernel alone
through the host-data entry (cal_prop_combine_real, n x 24, bytes (24 n + n) 8;
cal_prop_combine, 2n x 24, bytes (48 n + 2n) 8; the library's "apply" timer
brackets the kernel, three launches after a warm-up).
--package-root DIR adds the undriven prop leg from another checkout's built
package ("VARIANT@root", e.g. the parent commit's, to show it unchanged); for
csr2 it adds every leg (the parent's stacked CSR, which shared is held against:
"shared_vs_parent" says whether shared's median lies below the parent leg's
fastest window), and none for shared, which the parent does not have.
The summary has median, min and max over all windows of a variant and, for
split against csr, whether split is faster beyond the spread of both (split's
slowest window under csr's fastest).  --library runs the children on another
build of the library (CAL_LIBRARY), e.g. a kernel variant.  Prints one JSON
line; --out also writes it to a file.  Needs a GPU.
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

S, BLOCKS = 8, 3
HERM = ("herm", "herm_csr")  # the complex Hermitian H (set_matrix_hermitian)
STACKED = ("shared", "csr2") + HERM  # variants whose spmv / lanczos legs run on the stacked 2n rows
FLUX = 1.0 / 16.0
SPMV_PER_WINDOW, CA_PER_WINDOW, LZ_PER_WINDOW, PROP_PER_WINDOW = 50, 10, 100, 4
G_NL = 0.05  # the --nonlinear legs' coupling


def build(cal, np, variant, N):
    if variant == "lap":
        return cal.matrices.laplacian_3d(N)
    idx = np.arange(N ** 3, dtype=np.int64)
    r2 = np.zeros(N ** 3)
    for d in range(3):
        x = (idx // N ** d) % N - 0.5 * (N - 1)
        r2 += x * x
    if variant in HERM:
        return cal.matrices.peierls_hamiltonian((N, N, N), 0.5 * 0.02 ** 2 * r2, FLUX)
    return cal.matrices.grid_hamiltonian((N, N, N), 0.5 * 0.02 ** 2 * r2)


def child(a):
    import numpy as np

    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import ca_lanczos_amd as cal
    from ca_lanczos_amd import _lib

    N, W = a.N, a.windows
    A = build(cal, np, a.variant, N)
    n = A.shape[0]
    fmt = {"split": "split", "csr": "csr", "lap": "auto", "auto": "auto", "shared": "shared", "csr2": "csr",
           "herm": "shared", "herm_csr": "csr"}[a.variant]
    stacked = a.variant in STACKED
    ctx = cal.Context(spmv_format=fmt)
    if a.variant in HERM:
        ctx.set_matrix_hermitian(A)
        n = 2 * n
    elif stacked:
        ctx.set_matrix_stacked(A)
        n = 2 * n  # the legs below run on the stacked problem
    else:
        ctx.set_matrix(A)
    out = dict(variant=a.variant, library=os.path.basename(_lib.LIB_PATH), package=os.path.relpath(os.path.dirname(cal.__file__), ROOT),
               drive=a.drive, nonlinear=a.nonlinear, imaginary=a.imaginary, n=n, nnz=int(A.nnz),
               spmv_format=ctx.spmv_format(), plane_info=ctx.spmv_plane_info(), split_info=ctx.spmv_split_info())
    if hasattr(ctx, "spmv_shared_info"):
        out["shared_info"] = ctx.spmv_shared_info()
    if hasattr(ctx, "spmv_hermitian_info"):
        out["hermitian_info"] = ctx.spmv_hermitian_info()
    only = a.only.split(",")
    if "spmv" in only:
        ctx.bench_spmv(20)
        out["spmv_us"] = [1e3 * ctx.bench_spmv(SPMV_PER_WINDOW)[0] for _ in range(W)]
        out["spmv_launches"] = W * SPMV_PER_WINDOW
    r = np.random.default_rng(0).standard_normal(n)
    if "ca" in only and not stacked:
        wu = 3
        ctx.lanczos_begin(r, S, wu + W * CA_PER_WINDOW + 1, "newton", "local")
        for _ in range(wu):
            ctx.lanczos_step(False)
        ctx.synchronize()
        ms = []
        for _ in range(W):
            t0 = time.perf_counter()
            for _ in range(CA_PER_WINDOW):
                ctx.lanczos_step(False)
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / CA_PER_WINDOW)
        info = ctx.lanczos_get()[4]
        ctx.lanczos_end()
        out["ca_ms_per_outer"] = ms
        out["ca_flags"] = dict(n_reorth=info.n_reorth, breakdown=info.breakdown, n_rank_deficient=info.n_rank_deficient)
    if "lanczos" in only:
        wu = 50
        ctx.std_lanczos_begin(r, wu + W * LZ_PER_WINDOW, "local", keep_Q=False)
        ctx.std_lanczos_step(wu)
        ctx.synchronize()
        ms = []
        for _ in range(W):
            t0 = time.perf_counter()
            ctx.std_lanczos_step(LZ_PER_WINDOW)
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / LZ_PER_WINDOW)
        info = ctx.std_lanczos_get()[4]
        ctx.std_lanczos_end()
        out["lanczos_ms_per_vector"] = ms
        out["lanczos_fused"] = info["fused"]
    ctx.close()
    if "prop" in only:
        n = A.shape[0]
        idx = np.arange(n)
        coords = [(idx // N ** d) % N for d in range(3)]
        r2 = sum((c - 0.5 * (N - 1)) ** 2 for c in coords)
        phase = sum(k * c for k, c in zip((0.7, 0.3, 0.2), coords))
        psi0 = np.exp(-r2 / (2 * (N / 8.0) ** 2)) * np.exp(1j * phase)
        del idx, coords, r2, phase
        ctx = cal.Context(spmv_format=fmt)
        if a.imaginary != "0":  # both imaginary legs relax the same state: the packet's real envelope
            psi0 = np.abs(psi0)
        if a.imaginary == "real":  # on H itself
            P = cal.Propagator(A, psi0, S, BLOCKS, basis="newton", ctx=ctx, real=True)
            out["real_spmv_format"] = ctx.spmv_format()
        else:
            P = cal.Propagator(A, psi0, S, BLOCKS, basis="newton", ctx=ctx)
            if a.imaginary == "stacked":
                P.set_imaginary_time(True)
        out["stacked_split_info"] = ctx.spmv_split_info()
        out["stacked_plane_info"] = ctx.spmv_plane_info()
        nk = int(a.drive) if a.drive.isdigit() else 0
        per_window = PROP_PER_WINDOW
        if nk > 0 or a.drive == "reupload":
            idx = np.arange(n)
            cc = [(idx // N ** d) % N - 0.5 * (N - 1) for d in range(3)]
            ops = (cc + [sum(c * c for c in cc)])[:max(nk, 1)]
            del idx, cc

            def amp(t):
                return np.array([1e-3 * np.sin((k + 1) * t) for k in range(len(ops))])
        if nk > 0:
            P.set_drive(ops)

            def steps(k):
                P.step(a.dt, k, drive=amp)
        elif a.drive == "reupload":
            per_window = 2
            rows = np.repeat(np.arange(n), np.diff(A.indptr))
            dpos = np.nonzero(rows == A.indices)[0]
            del rows
            d0 = A.data[dpos].copy()
            Hn = A.copy()

            def steps(k):
                for _ in range(k):
                    Hn.data[dpos] = d0 + amp(P.t + 0.5 * a.dt)[0] * ops[0]
                    ctx.set_matrix_stacked(Hn)
                    P.step(a.dt, 1)
        elif a.nonlinear in ("frozen", "midpoint"):
            P.set_nonlinear(G_NL, a.nonlinear)

            def steps(k):
                P.step(a.dt, k)
        elif a.nonlinear == "copyback":
            per_window = 2
            rows = np.repeat(np.arange(n), np.diff(A.indptr))
            dpos = np.nonzero(rows == A.indices)[0]
            del rows
            d0 = A.data[dpos].copy()
            Hn = A.copy()

            def steps(k):
                nonlocal P
                for _ in range(k):
                    psi = P.state()
                    P.close()
                    Hn.data[dpos] = d0 + G_NL * (psi.real ** 2 + psi.imag ** 2)
                    P = cal.Propagator(Hn, psi, S, BLOCKS, basis="newton", ctx=ctx)
                    P.step(a.dt, 1)
        else:
            def steps(k):
                P.step(a.dt, k)
        steps(2)
        ctx.synchronize()
        ms = []
        for _ in range(W):
            t0 = time.perf_counter()
            steps(per_window)
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / per_window)
        if nk > 0 or a.nonlinear in ("frozen", "midpoint"):  # the diagonal's kernel alone: its own timer class over 10 steps
            K = 10
            ctx.timer_enable(True)
            ctx.timer_reset()
            steps(K)
            ctx.synchronize()
            cnt, tot = ctx.timer_read("drive")
            bytes_counted = ctx.timer_bytes("drive")
            ctx.timer_enable(False)
            us = 1e3 * tot / cnt
            out["drive_kernel"] = dict(us=us, launches_per_step=cnt / K, bytes=bytes_counted / cnt,
                                       TBps=bytes_counted / cnt / (us * 1e-6) / 1e12)
        if a.imaginary != "0":
            en = P.energetics()
            out["energetics_last"] = {k: float(v[-1]) for k, v in en.items()}
        info = P.info()
        out["prop_ms_per_step"] = ms
        out["prop_lsteps"] = info["lsteps"]
        out["prop_residual_max"] = info["residual_max"]
        # what a step's cost depends on besides the kernels' rates: the Lanczos vectors taken
        # (dropped blocks shorten a step) and the blocks' orthogonalisation path
        out["prop_info"] = {k: info[k] for k in ("steps", "lsteps_sum", "lsteps_max", "breakdowns", "rank_deficient")}
        out["prop_tsqr_fold_stats"] = ctx.tsqr_fold_stats()
        P.close()
        if a.imaginary != "0":  # the combine kernel alone, on host data
            m = S * BLOCKS
            rows = n if a.imaginary == "real" else 2 * n
            Q = np.empty((rows, m), order="F")
            Q[:] = 1.0 / np.arange(1, m + 1)
            co = np.cos(np.arange(m))
            if a.imaginary == "real":
                call, nbytes = (lambda: ctx.prop_combine_real(Q, co)), (n * m + n) * 8.0
            else:
                call, nbytes = (lambda: ctx.prop_combine(Q, co + 0.5j * co)), (2.0 * n * m + 2.0 * n) * 8.0
            call()
            ctx.timer_enable(True)
            ctx.timer_reset()
            for _ in range(3):
                call()
            cnt, tot = ctx.timer_read("apply")
            ctx.timer_enable(False)
            us = 1e3 * tot / cnt
            out["combine_kernel"] = dict(us=us, launches=cnt, bytes=nbytes, TBps=nbytes / (us * 1e-6) / 1e12)
            del Q
        ctx.close()
    print(json.dumps(out))


def run_child(a, variant, drive="0", root=None, nonlinear="0", imaginary="0"):
    env = dict(os.environ)
    env.pop("CAL_LIBRARY", None)
    env.pop("CAL_SPMV_FORMAT", None)
    if a.library:
        env["CAL_LIBRARY"] = a.library
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", variant, "--N", str(a.N),
           "--windows", str(a.windows), "--only",
           a.only if drive == "0" and nonlinear == "0" and imaginary == "0" and (not root or variant in STACKED)
           else "prop",
           "--dt", str(a.dt),
           "--drive", drive, "--nonlinear", nonlinear, "--imaginary", imaginary]
    if root:
        cmd += ["--package-root", root]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError("child %s drive %s nonlinear %s imaginary %s failed (%d): %s"
                           % (variant, drive, nonlinear, imaginary, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=215)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="spmv,ca,lanczos,prop")
    ap.add_argument("--variants", default="split,csr,lap")
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--library", default=None)
    ap.add_argument("--drive", default="0", help="prop leg: comma list of 0, 1..4 (operators) or reupload")
    ap.add_argument("--nonlinear", default="0", help="prop leg: comma list of frozen, midpoint, copyback")
    ap.add_argument("--imaginary", default="0", help="prop leg in imaginary time: comma list of stacked, real")
    ap.add_argument("--package-root", default=None, help="also the undriven prop leg from this checkout's package")
    ap.add_argument("--child-timeout", type=int, default=500)
    ap.add_argument("--variant", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.windows < 5:
        ap.error("--windows must be at least 5")
    if a.child:
        return child(a)

    variants = a.variants.split(",")
    drives = a.drive.split(",")
    for d in drives:
        if d not in ("0", "1", "2", "3", "4", "reupload"):
            ap.error("--drive takes 0, 1..4 or reupload")
    nls = [x for x in a.nonlinear.split(",") if x != "0"]
    for x in nls:
        if x not in ("frozen", "midpoint", "copyback"):
            ap.error("--nonlinear takes frozen, midpoint or copyback")
    ims = [x for x in a.imaginary.split(",") if x != "0"]
    for x in ims:
        if x not in ("stacked", "real"):
            ap.error("--imaginary takes stacked or real")
    # the real-time legs; "auto" exists for the real imaginary leg alone
    legs = [(v, v, "0", None, "0", "0") for v in variants if v != "auto"] if "0" in drives else []
    legs += [("%s+drive%s" % (v, d), v, d, None, "0", "0") for v in variants if v not in ("lap", "auto")
             for d in drives if d != "0"]
    legs += [("%s+nl%s" % (v, x), v, "0", None, x, "0") for v in variants if v not in ("lap", "auto") for x in nls]
    for v in variants:
        for im in ims:
            if v == "lap" or (im == "real" and v in STACKED) or (im == "stacked" and v == "auto"):
                continue
            legs.append(("%s+im%s" % (v, im), v, "0", None, "0", im))
            if "frozen" in nls and v != "auto":  # the density kernel rewrites a stored diagonal ("csr" / "split")
                legs.append(("%s+im%s+nlfrozen" % (v, im), v, "0", None, "frozen", im))
    if a.package_root:
        legs += [("%s@root" % v, v, "0", a.package_root, "0", "0") for v in variants
                 if v not in ("shared", "auto") and v not in HERM]
    variants = [l[0] for l in legs]
    res = dict(N=a.N, n=a.N ** 3, rounds=a.rounds, windows=a.windows, only=a.only, library=a.library or "production",
               s=S, blocks=BLOCKS, runs={v: [] for v in variants})
    for i in range(a.rounds):  # alternating, each in a fresh process
        for name, v, d, root, nl, im in legs:
            res["runs"][name].append(run_child(a, v, d, root, nl, im))
            print("round %d: %s done" % (i + 1, name), file=sys.stderr, flush=True)

    keys = dict(spmv="spmv_us", ca="ca_ms_per_outer", lanczos="lanczos_ms_per_vector", prop="prop_ms_per_step")
    summ = {}
    for v in variants:
        summ[v] = {}
        for k, field in keys.items():
            w = [x for r in res["runs"][v] for x in r.get(field, [])]
            if w:
                med = statistics.median(w)
                summ[v][k] = dict(median=med, min=min(w), max=max(w), windows=len(w), per_s=1e3 / med if k != "spmv" else None)
    for v in variants:
        dk = [r["drive_kernel"] for r in res["runs"][v] if "drive_kernel" in r]
        if dk:
            summ[v]["drive_kernel"] = dict(us=statistics.median(x["us"] for x in dk), us_all=[x["us"] for x in dk],
                                           bytes=dk[0]["bytes"], launches_per_step=dk[0]["launches_per_step"],
                                           TBps=dk[0]["bytes"] / (statistics.median(x["us"] for x in dk) * 1e-6) / 1e12)
        ck = [r["combine_kernel"] for r in res["runs"][v] if "combine_kernel" in r]
        if ck:
            us = statistics.median(x["us"] for x in ck)
            summ[v]["combine_kernel"] = dict(us=us, us_all=[x["us"] for x in ck], bytes=ck[0]["bytes"],
                                             TBps=ck[0]["bytes"] / (us * 1e-6) / 1e12)
    res["summary"] = summ
    # the real path against the stacked one, leg by leg: the byte ratio says 2
    res["imaginary_real_vs_stacked"] = {}
    for v in variants:
        if "+imreal" in v and "prop" in summ[v]:
            other = v.replace("+imreal", "+imstacked")
            if other.startswith("auto+"):
                other = "split+" + other.split("+", 1)[1]
            if other in summ and "prop" in summ[other]:
                res["imaginary_real_vs_stacked"][v] = dict(
                    against=other, ratio=summ[other]["prop"]["median"] / summ[v]["prop"]["median"],
                    ratio_fastest_windows=summ[other]["prop"]["min"] / summ[v]["prop"]["min"],
                    ratio_slowest_windows=summ[other]["prop"]["max"] / summ[v]["prop"]["max"],
                    slowest_real_beats_fastest_stacked=bool(summ[v]["prop"]["max"] < summ[other]["prop"]["min"]))
    n = a.N ** 3
    for v in variants:
        if "spmv" in summ[v]:
            per_row = 33.0 if v == "split" else 25.0  # algorithmic bytes per row of the marches
            nnz = res["runs"][v][0]["nnz"]
            b = per_row * n if v != "csr" else 12.0 * nnz + 20.0 * n
            if v.split("@")[0] == "csr2":
                b = 2.0 * (12.0 * nnz + 20.0 * n)
            if v == "shared":
                b = 12.0 * nnz + 4.0 * (n + 1) + 32.0 * n
            if v == "herm":
                b = 20.0 * nnz + 4.0 * (n + 1) + 32.0 * n
            if v == "herm_csr":  # the embedding's 4 nnz entries and 2n rows on the CSR kernel
                b = 2.0 * (24.0 * nnz + 20.0 * n)
            summ[v]["spmv"]["algorithmic_TBps"] = b / (summ[v]["spmv"]["median"] * 1e-6) / 1e12
    if "split" in summ and "csr" in summ:
        res["split_vs_csr"] = {
            k: dict(ratio=summ["csr"][k]["median"] / summ["split"][k]["median"],
                    beyond_spread=bool(summ["split"][k]["max"] < summ["csr"][k]["min"]))
            for k in summ["split"] if k in summ["csr"]}
    for name, other in (("shared_vs_csr2", "csr2"), ("shared_vs_parent", "csr2@root"),
                        ("shared_vs_csr2_driven", "csr2+drive1"), ("herm_vs_herm_csr", "herm_csr"),
                        ("herm_vs_shared", "shared")):
        mine = "shared+drive1" if other.endswith("drive1") else "herm" if name.startswith("herm") else "shared"
        if mine in summ and other in summ:
            res[name] = {
                k: dict(ratio=summ[other][k]["median"] / summ[mine][k]["median"],
                        median_below_fastest_window=bool(summ[mine][k]["median"] < summ[other][k]["min"]))
                for k in ("spmv", "lanczos", "prop") if k in summ[mine] and k in summ[other]}
    if "split" in summ and "lap" in summ:
        res["split_over_lap_time"] = {k: summ["split"][k]["median"] / summ["lap"][k]["median"]
                                      for k in summ["split"] if k in summ["lap"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
