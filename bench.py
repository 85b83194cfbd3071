"""CA-Lanczos outer-iterations/s + SpMV HBM GB/s on MI355X (BASELINE.json).

A "step" is one CA-Lanczos outer iteration (ca_lanczos.m:166-237): s = 8
fused SpMV+Newton-shift launches, the block orthogonalisation against the
previous block (projectAndNormalize), and the host T extension; diagnostics
(Ritz residuals) off, as SURVEY §8d prescribes.  Inputs (A, r, Q, V) are
resident in HBM before the timed region.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload lap3d_215]
  python bench.py --full                                    # + legs, roofline, CPU baselines
  python bench.py --dump-outputs DIR                        # + DIR/<name>.npy of the last timed step
  python bench.py --workload circuit_1259 --driver irl      # BASELINE config 5
  python bench.py --matrix G3_circuit.mtx --driver irl      # a SuiteSparse file

Workloads: lap2d_N / lap3d_N (Dirichlet Laplacians), circuit_N (the
G3_circuit stand-in, matrices.circuit_like) or --matrix FILE (.mtx/.mat).
N > 1 runs one rank per GPU (torch.distributed.run): contiguous row slabs
(z-slabs for the Laplacians) of the same matrix, one deep RCCL halo exchange
per outer iteration (CA matrix powers, overlapped with the interior powers)
and RCCL allreduce of the Gram blocks (strong scaling, whole-job rate).
--driver irl times whole impl_restarted_ca_lanczos solves instead of
ca_lanczos outer iterations (a secondary line; the default is the headline).

A plain run sets up, warms up, times the K steps and prints the headline line
(metric, value, unit, ms_per_step, the configuration).  --full adds everything
else the benchmark measures, each in runs of its own after the timed steps:
the per-kernel HIP-event timers and the roofline, the secondary legs (TSQR
normalize, CSR format, 'full' orthogonalisation, the other workloads, the
IRL), the back-to-back SpMV kernels, the diagnostics-on rate and the CPU
baselines (--no-legs / --no-cpu-baseline trim a --full run).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md: 8.0 TB/s)
MFMA_F64_PEAK_TF = 78.6  # MI355X FP64 matrix peak (AMD spec sheet; the guide lists no f64 row)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")),
                   help="ranks (one per GPU); without a launcher bench.py starts torch.distributed.run itself")
    p.add_argument("--steps", type=int, default=None,
                   help="timed steps (default 15 outer iterations; --driver irl: 5 solves)")
    p.add_argument("--warmup", type=int, default=None,
                   help="untimed steps before them (default 2; --driver irl: 1 solve)")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the per-kernel timers / roofline, the secondary legs, "
                        "the diagnostics-on run and the CPU baselines (a plain run prints the headline only)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="write what the last timed step computed as DIR/<name>.npy (float64; large arrays as a "
                        "fixed seeded row sample, at most 64 MB in all)")
    p.add_argument("--workload", default="lap3d_215", help="lap2d_N | lap3d_N | circuit_N")
    p.add_argument("--matrix", default=None, help="matrix file (.mtx[.gz] or SuiteSparse .mat); overrides --workload")
    p.add_argument("--driver", default="lanczos", choices=["lanczos", "irl"])
    p.add_argument("--irl", default="64,8", help="impl_restarted_ca_lanczos max_lanczos,n_wanted_eigs")
    p.add_argument("--irl-tol", type=float, default=1.0e-8)
    p.add_argument("--s", type=int, default=8)
    p.add_argument("--basis", default="newton")
    p.add_argument("--orth", default="local")
    p.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines")
    p.add_argument("--basis-gb", type=float, default=200.0,
                   help="per-GPU budget for the Krylov basis Q; longer runs continue in restarted epochs")
    p.add_argument("--cpu-iters", type=int, default=15, help="outer iterations of the C/OpenMP CPU sample")
    p.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "spmv_traffic.json"))
    p.add_argument("--mpk-depth", type=int, default=8,
                   help="N > 1: ghost depth of the CA matrix-powers kernel (1 = one halo exchange per SpMV)")
    p.add_argument("--normalize", default="auto", choices=["auto", "tsqr", "cholqr2"],
                   help="normalize (tsqr.m) backend of the headline: auto = CholQR2 fused into the sweeps "
                        "(Householder TSQR when its Cholesky fails), tsqr = Householder TSQR tree")
    p.add_argument("--no-legs", action="store_true", help="--full without the secondary TSQR / CSR legs")
    p.add_argument("--comm", default="rccl", choices=["rccl", "host"],
                   help="N > 1 transport: RCCL (default) or host-staged gloo callbacks (rehearsal of the "
                        "distributed bench with several ranks on one GPU)")
    args = p.parse_args()
    irl = args.driver == "irl"
    if args.steps is None:
        args.steps = 5 if irl else 15
    if args.warmup is None:
        args.warmup = 1 if irl else 2
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    return args


class Workload:
    """The benchmark matrix: rows(r0, r1) -> local CSR slab (global int32
    columns), full() -> the whole matrix (CPU baseline, CSR comparison)."""

    def __init__(self, name, path=None):
        self.name = name
        self._A = None
        if path:
            from ca_lanczos_amd.matrices import load_matrix
            self._A = load_matrix(path)
            self.name = "file:" + os.path.basename(path)
            self.kind, self.dim, self.N = "file", 0, 0
            self.n = self._A.shape[0]
            self.plane = 1
            self.desc = "%s, n=%%d, nnz=%%d" % self.name
            self.data = "file %s (symmetric sparse, r = MATLAB rand(n,1) seed 5489)" % os.path.basename(path)
            return
        kind, N = name.split("_")
        self.kind, self.N = kind, int(N)
        if kind in ("lap2d", "lap3d"):
            self.dim = 2 if kind == "lap2d" else 3
            self.n = self.N ** self.dim
            self.plane = self.N ** (self.dim - 1)
            st = "7-pt 3-D" if self.dim == 3 else "5-pt 2-D"
            self.desc = "%s: %s %dx..., n=%%d, nnz=%%d" % (name, st, self.N)
            self.data = "synthetic (%s Dirichlet Laplacian, r = MATLAB rand(n,1) seed 5489)" % st[:4]
        elif kind == "circuit":
            from ca_lanczos_amd.matrices import circuit_like
            self.dim = 0
            self._A = circuit_like(self.N)
            self.n = self._A.shape[0]
            self.plane = 1
            self.desc = ("%s: G3_circuit stand-in (random SPD resistor network on a %dx%d grid), n=%%d, nnz=%%d"
                         % (name, self.N, self.N))
            self.data = "synthetic (matrices.circuit_like seed 0; G3_circuit itself is not in the image)"
        else:
            raise ValueError("unknown workload %s" % name)

    def rows(self, r0, r1):
        if self._A is None:
            from ca_lanczos_amd.matrices import laplacian_rows
            return laplacian_rows(self.dim, self.N, r0, r1)
        A = self._A
        rp = A.indptr[r0:r1 + 1].astype(np.int64)
        lo, hi = int(rp[0]), int(rp[-1])
        return rp - lo, A.indices[lo:hi].astype(np.int32), A.data[lo:hi]

    def full(self):
        import scipy.sparse as sp
        if self._A is not None:
            return self._A
        rowptr, col, val = self.rows(0, self.n)
        return sp.csr_matrix((val, col.astype(np.int32), rowptr), shape=(self.n, self.n))


def host_info():
    """CPU model (lscpu's 'Model name' from /proc/cpuinfo), the host cores this
    process may use and the ROCm release of the image (BASELINE.md's line)."""
    model = "?"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    rocm = "?"
    for p in ("/opt/rocm/.info/version", "/opt/rocm/.info/version-dev"):
        try:
            rocm = open(p).read().strip()
            break
        except OSError:
            pass
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        cores = os.cpu_count()
    import torch
    return {"cpu_model": model, "cpu_cores_visible": cores, "rocm": rocm, "torch": torch.__version__}


def _blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return max([d.get("num_threads", 1) for d in threadpool_info()] or [1])
    except Exception:  # pragma: no cover
        return 1


def usable_cpus():
    """The CPUs this process may actually run on: the affinity mask, capped by
    the cgroup CPU quota (v2 cpu.max, v1 cfs_quota_us / cfs_period_us), with
    OMP_NUM_THREADS as found in the environment (reported, not trusted)."""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        aff = os.cpu_count() or 1
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(period)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / period
        except (OSError, ValueError):
            pass
    usable = aff if quota is None else max(1, min(aff, int(math.floor(quota + 1e-9))))
    return {"affinity_cpus": aff, "cgroup_quota_cpus": quota, "usable": usable,
            "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS")}


def cpu_baseline(wl, s, iters, basis="newton", reps=3):
    """The C/OpenMP restatement (oracle/c/ca_lanczos_omp.c) timed on this host
    with one thread per usable CPU (affinity and cgroup quota, usable_cpus();
    SURVEY §8d "OMP_NUM_THREADS = nproc"): Newton prologue excluded, `iters`
    outer iterations of ca_lanczos_basic 'local' (k = 1..iters, diagnostics
    off) on the same matrix and start vector (SURVEY §8d CPU baseline (2)).
    When more than 16 CPUs are usable, 16 threads (the box's per-GPU CPU
    share) are timed too and reported beside it."""
    from oracle import ca_lanczos_ref as ref
    from oracle import omp
    A = wl.full()
    r = ref.matlab_rand(wl.n)
    q = r / math.sqrt(r @ r)
    Bk, _, _ = ref.newton_change_of_basis(A, q, s)
    omp.lib()
    cpus = usable_cpus()

    def timed(th):
        omp.set_threads(th)
        t0 = time.perf_counter()
        omp.ca_lanczos_local(A, q, Bk, s, iters, basis == "newton")
        return omp.loop_seconds(), time.perf_counter() - t0, omp.threads()

    # three runs, the median reported (box-to-box and run-to-run spread of
    # a shared host: VERDICT r04 weak #7)
    runs = [timed(cpus["usable"]) for _ in range(reps)]
    rates = sorted(iters / r[0] for r in runs)
    dt, dt_call, th = sorted(runs)[len(runs) // 2]
    out = {"value": rates[len(rates) // 2], "unit": "outer-iters/s", "cores": th, "kind": "port",
           "runs": len(runs), "min": rates[0], "max": rates[-1],
           "sample": "oracle/c/ca_lanczos_omp.c (C/OpenMP, %d threads = the usable CPUs): %d outer iterations "
                     "(k=1..%d, s=%d, Newton, 'local', Householder TSQR normalize, diagnostics off) on the same "
                     "%s matrix, %d runs, the median reported; outer loop %.1f s (buffers allocated and "
                     "first-touched in parallel before it, as the GPU's are resident; whole call %.1f s)"
                     % (th, iters, iters, s, wl.name, len(runs), dt, dt_call),
           "cpus": cpus}
    if cpus["usable"] > 16:
        dt16, _, th16 = timed(16)
        out["value_16_threads"] = iters / dt16
        out["sample"] += "; with 16 threads: %.1f s" % dt16
    return out


def cpu_baseline_numpy(wl, s, iters, basis="newton"):
    """The NumPy restatement (oracle/ca_lanczos_ref.py) on the same sample:
    SciPy's CSR SpMV is single-threaded, LAPACK QR uses the BLAS threads."""
    from oracle import ca_lanczos_ref as ref
    blas_threads = _blas_threads()
    A = wl.full()
    r = ref.matlab_rand(wl.n)
    q = r / math.sqrt(r @ r)
    Bk, _, _ = ref.newton_change_of_basis(A, q, s)
    t0 = time.perf_counter()
    ref.ca_lanczos_basic(A, q, Bk, iters, s, basis, "local", diagnostics=False)
    dt = time.perf_counter() - t0
    return {"value": iters / dt, "unit": "outer-iters/s", "cores": int(blas_threads), "kind": "port",
            "sample": "oracle/ca_lanczos_ref.py ca_lanczos_basic, %d outer iterations on the same %s matrix; "
                      "SciPy CSR SpMV single-threaded, LAPACK QR %d threads; %.1f s"
                      % (iters, wl.name, blas_threads, dt)}


def cpu_baseline_irl(wl, s, max_lanczos, nw):
    """The oracle's implicit restart, first pass only (ceil(m/s) CA blocks to
    m vectors plus one compression; a whole solve is ~50 s at G3 size):
    CA blocks/s, the unit of the GPU line's blocks_per_s."""
    from oracle import ca_lanczos_ref as ref
    A = wl.full()
    n = wl.n
    k, p, m = ref.irl_sizes(max_lanczos, nw, s)
    ncols = s * (-(-m // s)) + 1
    Q = np.zeros((n, ncols))
    T = np.zeros((ncols, ncols - 1))
    r = ref.matlab_rand(n)
    Q[:, 0] = r / math.sqrt(r @ r)
    Bk, _, _ = ref.newton_change_of_basis(A, Q[:, 0].copy(), s, "full")
    t0 = time.perf_counter()
    nb = -(-m // s)
    ref.irl_lanczos_basic(A, Q, T, Bk, m, 0, s, "newton", "full", 0.0)
    H = T[:m, :m].copy()
    w = ref._sym_eig(H)[0]
    u = [w[i] for i in ref._wanted_order(w)]
    W = np.eye(m)
    for j in range(m, k, -1):
        W, H = ref.qrstep(W, H, u[j - 1], 0, m - 1)
    Q[:, : k + 1] = Q[:, : m + 1] @ np.vstack([W[:, : k + 1], np.zeros((1, k + 1))])
    dt = time.perf_counter() - t0
    return {"value": nb / dt, "unit": "CA blocks/s", "cores": int(_blas_threads()), "kind": "port",
            "sample": "oracle/ca_lanczos_ref.py implicit restart, first pass (%d CA blocks of s=%d, Newton, "
                      "'full', to m=%d vectors) + qrstep shifts + compression on the same %s matrix; %.1f s"
                      % (nb, s, m, wl.name, dt)}


def rank_comm(cal, ctx, args, world, rank, dist):
    """The rank's communicator on ctx: the host-staged gloo callbacks
    (--comm host) or RCCL, whose unique id rank 0 broadcasts over the gloo
    group (every context of a rank gets a communicator of its own)."""
    import torch
    if args.comm == "host":
        def allreduce(a):
            t = torch.from_numpy(a)
            dist.all_reduce(t)

        hang = os.environ.get("CAL_BENCH_TEST_HANG_RANK")

        def exchange(peer, send, recv):
            if hang is not None and int(hang) == rank:  # tests: a rank whose exchange never returns
                while True:
                    time.sleep(3600)
            reqs = []
            if send.size:
                reqs.append(dist.isend(torch.from_numpy(np.ascontiguousarray(send)), peer))
            rt = torch.zeros(recv.size, dtype=torch.float64)
            if recv.size:
                reqs.append(dist.irecv(rt, peer))
            for q in reqs:
                q.wait()
            if recv.size:
                recv[:] = rt.numpy()

        ctx.comm_init_host(world, rank, allreduce, exchange)
        return
    if os.environ.get("CAL_RCCL_HOSTID_PER_RANK") == "1":
        # one-GPU rehearsal of the RCCL line: RCCL refuses two ranks on one
        # device of one host, so each rank states a host of its own and the
        # ranks connect over sockets (tests/test_gpu_rccl_multirank.py)
        os.environ["NCCL_HOSTID"] = "cal-rank-%d" % rank
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_IB_DISABLE", "1")
    uid = bytearray(128)
    if rank == 0:
        buf = ctypes.create_string_buffer(128)
        cal._lib.check(None, cal._lib.lib.cal_comm_unique_id(buf))
        uid = bytearray(buf.raw)
    t = torch.tensor(list(uid), dtype=torch.uint8)
    dist.broadcast(t, 0)
    ctx.comm_init_rccl(world, rank, bytes(t.tolist()))


def setup(args, wd=None):
    """Ranks, context, communicator and the resident matrix slab (each stage
    under the watchdog wd of a multi-rank run)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))

    def stage(name):
        if wd is not None:
            wd.enter(name, stage_limit(name))
    wl = Workload(args.workload, args.matrix)
    n = wl.n

    import ca_lanczos_amd as cal
    from ca_lanczos_amd.matrices import slab_bounds

    dist = None
    if world > 1:
        import torch.distributed as dist
        stage("init_process_group")
        dist.init_process_group("gloo", init_method="env://")
        stage("comm_init")

    ndev = ctypes.c_int(0)
    cal._lib.lib.cal_device_count(ctypes.byref(ndev))
    ctx = cal.Context(device=local % max(ndev.value, 1), mpk_depth=args.mpk_depth, normalize=args.normalize)
    bounds = slab_bounds(n, world, wl.plane)
    r0, r1 = bounds[rank], bounds[rank + 1]
    rowptr, col, val = wl.rows(r0, r1)
    nnz_local = int(rowptr[-1])
    if world > 1:
        rank_comm(cal, ctx, args, world, rank, dist)
    import scipy.sparse as sp
    if world > 1:
        stage("matrix_setup")
        Aloc = sp.csr_matrix((val, col, rowptr), shape=(r1 - r0, n))
        ctx.set_matrix_slab(n, r0, Aloc)
    else:
        ctx.set_matrix(sp.csr_matrix((val, col.astype(np.int32), rowptr), shape=(n, n)))
    del rowptr, col, val
    nnz_total = nnz_local
    if dist is not None:
        import torch
        tt = torch.tensor([float(nnz_local)], dtype=torch.float64)
        dist.all_reduce(tt)
        nnz_total = int(tt.item())
    return dict(world=world, rank=rank, local=local, wl=wl, cal=cal, dist=dist, ctx=ctx, r0=r0, r1=r1,
                nnz_local=nnz_local, nnz_total=nnz_total)


def max_over_ranks(dist, vals):
    if dist is None:
        return vals
    import torch
    tt = torch.tensor(vals, dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    return [float(x) for x in tt]


MFMA_PMC_JSON = os.path.join(ROOT, "profiles", "r05", "pmc", "mfma_summary.json")
PERSISTENT_JSON = os.path.join(ROOT, "profiles", "r06", "config2", "persistent_powers_probe.json")


BOUNDARY_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r05", "graph_powers",
                             "summary.json")


def launch_boundaries(leg):
    """Config 2's launch boundaries.  At ~16 launches
    of 6-35 us per step the HIP-event timers' own cost could make the timed
    kernels' sum exceed the step (with default events, which fence the
    caches at record, the SpMV averaged 11.4 us timed against 7.1 us back to
    back); the library's timing events now skip that fence (5.9 vs 5.5 us,
    kernel share 0.88 against rocprof's 0.87-0.89 busy share, on one box;
    7.7-12.8 us on others), and the share is withheld whenever the timed SpMV
    exceeds 1.3x its back-to-back time.  The busy share comes from a rocprofv3 kernel trace of the timed
    steps and the HIP-graph A/B of the matrix powers
    (profiles/r05/graph_powers/summary.json; round 5's command files are in
    git history), and the persistent-launch A/B of round 6: the eight powers
    as one launch with grid barriers between them against eight launches
    (profiles/r06/config2/persistent_powers_probe.json,
    tools/persistent_powers_probe.hip)."""
    out = {}
    b2b = leg.get("spmv_kernel_back_to_back", {}).get("avg_us")
    timed = leg.get("kernel_avg_launch_us", {}).get("spmv")
    if b2b and timed and timed > 1.3 * b2b:
        out["timer_distortion"] = {"spmv_timed_avg_us": timed, "spmv_back_to_back_us": b2b}
        out["kernel_share_timed"] = leg.get("kernel_share")
        leg["kernel_share"] = None
    try:
        sm = json.load(open(BOUNDARY_JSON))
        out["rocprof_busy_share"] = sm["rocprof_busy_share"]
        out["hip_graph_powers"] = {"graph_outer_it_s": sm["hip_graph_powers_outer_it_s"].get("lap2d_1000"),
                                   "direct_outer_it_s": sm["direct_outer_it_s"].get("lap2d_1000"),
                                   "kept": False}
        out["source"] = "profiles/r05/graph_powers/summary.json"
    except (OSError, ValueError, KeyError):
        pass
    try:
        for ln in open(PERSISTENT_JSON):
            d = json.loads(ln)
            if d.get("N") == 1000:
                out["persistent_powers"] = {
                    "eight_launches_us": d["eight_launches_us"],
                    "one_persistent_launch_us": min(d[k] for k in d if k.startswith("persistent_")),
                    "grid_barrier_us": d["barriers_only_1percu_us"] / 7.0,
                    "kept": False, "source": "profiles/r06/config2/persistent_powers_probe.json"}
    except (OSError, ValueError, KeyError):
        pass
    return out


def gram_mfma(n_loc, gram_avg_ms, b_gram, wname, world):
    """MFMA utilisation of the Gram step (BASELINE north_star): 512 n f64
    flops per sweep of n rows over the live HIP-event average, against the
    f64 matrix peak, with the counter evidence of the current kernels
    (profiles/r05/pmc/mfma_summary.json, tools/pmc_mfma.sh: rocprofv3
    SQ_INSTS_VALU_MFMA_MOPS_F64 x 512 and SQ_VALU_MFMA_BUSY_CYCLES per
    launch of P1 and pass A on lap3d_215) when this is that workload."""
    flops = 512.0 * n_loc
    out = {"flops_per_launch": flops, "tflops": flops / (gram_avg_ms * 1e-3) / 1e12, "peak_tflops": MFMA_F64_PEAK_TF,
           "frac": flops / (gram_avg_ms * 1e-3) / 1e12 / MFMA_F64_PEAK_TF,
           "bound_by_hbm_tflops": 512.0 / b_gram * n_loc * 6.29}
    try:
        pm = json.load(open(MFMA_PMC_JSON))
        if wname == "lap3d_215" and world == 1:
            ev = {}
            for k, d in pm.items():
                if k.startswith("void cal::k_rowapply<17, 4, true") or k.startswith("void cal::k_rowapply<17, 8, true"):
                    ev["P1" if "<17, 4," in k else "pass_A"] = {
                        "pmc_flops_per_launch": d["mfma_f64_flops_per_launch"],
                        "mfma_busy_share": d.get("mfma_busy_share"), "launches_counted": d["launches"]}
            out["pmc"] = dict(ev, source="profiles/r05/pmc/mfma_summary.json")
    except (OSError, ValueError, KeyError):
        pass
    return out


def traffic_for(args, wl, world, cls):
    if not os.path.exists(args.traffic_json):
        return None
    try:
        tj = json.load(open(args.traffic_json))
        if tj.get("workload") == wl.name and tj.get("n_gpus", 1) == world:
            return tj.get("classes", {}).get(cls)
    except Exception:
        return None
    return None


_JSON_FD = None


def _quiet_stdout():
    """Send everything written to fd 1 (gloo's connection banners, HIP/RCCL
    messages, from every rank) to stderr; emit() writes the one JSON line to
    the original stdout."""
    global _JSON_FD
    sys.stdout.flush()
    _JSON_FD = os.dup(1)
    os.dup2(2, 1)


def emit(line):
    data = (json.dumps(line) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(data.decode())
        sys.stdout.flush()
    else:
        os.write(_JSON_FD, data)


class Watchdog:
    """Per-rank stage watchdog of a multi-rank run (the first 8-GPU SCALE
    run is the first RCCL run with more than one rank): every stage has a
    time limit; when one is exceeded the rank prints its rank and stage to
    stderr, rank 0 also emits the JSON line with "error" and "stage", and the
    process leaves with os._exit(3) (no re-exec, no cleanup that could block
    on the hung collective).  enter() starts a stage, done() stops watching."""

    def __init__(self, rank, world, enabled=True, poll=0.5):
        import threading
        self.rank, self.world = rank, world
        self.stage, self.limit, self.t0 = "start", None, time.monotonic()
        self.history = []
        self.fallback = None  # the headline line (rank 0) once it is measured: what a stuck leg leaves
        self._lock = threading.Lock()
        self._stop = threading.Event()
        self._poll = poll
        if enabled:
            self._th = threading.Thread(target=self._run, daemon=True)
            self._th.start()

    def enter(self, stage, limit_s):
        with self._lock:
            now = time.monotonic()
            if self.limit is not None:
                self.history.append((self.stage, round(now - self.t0, 3)))
            self.stage, self.limit, self.t0 = stage, float(limit_s), now

    def done(self):
        self._stop.set()

    def _run(self):
        while not self._stop.wait(self._poll):
            with self._lock:
                stage, limit, el = self.stage, self.limit, time.monotonic() - self.t0
            if limit is not None and el > limit:
                msg = "bench.py rank %d/%d: stage '%s' exceeded %.0f s (%.1f s)" % (self.rank, self.world, stage,
                                                                                 limit, el)
                sys.stderr.write(msg + "\n")
                try:  # where every thread of the rank stands
                    import faulthandler
                    faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
                except Exception:  # pragma: no cover
                    pass
                sys.stderr.flush()
                if stage == "legs" and self.fallback is not None:
                    # the headline was measured and reduced over ranks before
                    # the secondary legs began: it stands, the legs are lost
                    if self.rank == 0:
                        try:
                            emit(dict(self.fallback, legs_error=msg, stages_done_s=self.history))
                        except Exception:  # pragma: no cover
                            pass
                    os._exit(0)
                if self.rank == 0:
                    try:
                        emit({"metric": "CA-Lanczos outer-iters/sec (n~10M, s=8)", "value": None,
                              "error": msg, "stage": stage, "rank": self.rank, "n_gpus": self.world,
                              "stages_done_s": self.history})
                    except Exception:  # pragma: no cover
                        pass
                os._exit(3)


# per-stage limits (s) of a multi-rank run; the driver's own limit is 600 s
STAGE_LIMITS = {"init_process_group": 120, "comm_init": 120, "matrix_setup": 240, "lanczos_begin": 120,
                "first_outer_step": 60, "warmup": 120, "timed": 240, "legs": 240, "finalize": 60}


IRL_MAX_ALLREDUCE_US = 1000.0


def stage_limit(name):
    """STAGE_LIMITS, or every stage CAL_BENCH_STAGE_LIMIT seconds (tests)."""
    v = os.environ.get("CAL_BENCH_STAGE_LIMIT")
    return float(v) if v else STAGE_LIMITS[name]


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args):
    """`bench.py --gpus N` without a launcher: start N ranks (one process per
    GPU) under torch.distributed.run as a CHILD process -- this process has
    not touched the GPU and is not replaced -- relay the rank-0 JSON line and
    return the child's exit code."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "1")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE)
    sys.stdout.write(proc.stdout.decode())
    sys.stdout.flush()
    return proc.returncode


DUMP_Q_BYTES = 48 * 1000 * 1000  # of --dump-outputs' 64 MB: the row sample of the last block of Q
DUMP_T_ORDER = 1024  # T's trailing corner (8 MB at most)
DUMP_SEED = 5489


def _save(dirpath, name, a):
    np.save(os.path.join(dirpath, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def dump_lanczos(ctx, dirpath):
    """--dump-outputs of the CA-Lanczos driver: what a caller of the timed
    path receives after its last step.  T (its trailing DUMP_T_ORDER corner
    when larger), the reorthogonalisation flags, and the s basis vectors the
    last step appended to Q (this rank's rows; beyond DUMP_Q_BYTES a sorted
    row sample drawn with a fixed seed, the rows stored beside it)."""
    os.makedirs(dirpath, exist_ok=True)
    k, s, _ = ctx.lanczos_state()
    T, _, _, flags, _ = ctx.lanczos_get()
    m = min(T.shape[0], DUMP_T_ORDER)
    _save(dirpath, "T", T[T.shape[0] - m:, T.shape[1] - m:])
    _save(dirpath, "reorth_flags", flags)
    n = ctx.n
    cap = DUMP_Q_BYTES // (8 * s)
    rows = np.arange(n) if n <= cap else np.sort(np.random.RandomState(DUMP_SEED).choice(n, cap, replace=False))
    Q = np.empty((len(rows), s))
    for j in range(s):  # a column at a time: the whole block is 0.6 GB at n = 10M
        Q[:, j] = ctx.lanczos_get_Q(s * (k - 1) + 1 + j, 1)[rows, 0]
    _save(dirpath, "Q_last_block", Q)
    _save(dirpath, "Q_last_block_rows", rows)


def dump_irl(out, dirpath):
    """--dump-outputs of the IRL driver: the last timed solve's eigenvalues
    and per-restart Ritz estimates (Q_conv stays on the device in the timed
    solves) and its restart count."""
    os.makedirs(dirpath, exist_ok=True)
    _save(dirpath, "conv_eigs", out["conv_eigs"])
    _save(dirpath, "ritz_est", out["ritz_est"])
    _save(dirpath, "num_restarts", np.array([out["num_restarts"]]))


def main():
    args = parse()
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        return launch_ranks(args)
    if world_env is not None and int(world_env) != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%s\n" % (args.gpus, world_env))
        return 2
    _quiet_stdout()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    wd = Watchdog(int(os.environ.get("RANK", "0")), world) if world > 1 else None

    def stage(name):
        if wd is not None:
            wd.enter(name, stage_limit(name))

    if args.driver == "irl":
        return main_irl(args, wd)
    E = setup(args, wd)
    world, rank, local, wl, cal, dist, ctx = (E[k] for k in ("world", "rank", "local", "wl", "cal", "dist", "ctx"))
    r0, r1, nnz_local, nnz_total = E["r0"], E["r1"], E["nnz_local"], E["nnz_total"]
    n = wl.n
    s = args.s
    r_full = np.random.RandomState(5489).random_sample(n)  # MATLAB rand(n,1), fresh session

    K, W = args.steps, args.warmup
    # K timed steps run without per-kernel events (an event pair around each
    # launch adds ~6 us per kernel boundary); KT more steps then run with the
    # HIP-event kernel timers for the per-kernel figures and the roofline.
    KT = max(1, min(K, 5))
    # Q holds s*t + 1 columns of the local slab.  A run longer than a 200 GB
    # basis (about 300 outer iterations of lap3d_215 on one GPU) continues in
    # epochs: a new epoch restarts the Krylov space from the same vector, and
    # its Newton prologue is timed when it falls inside the timed region.
    # (+1: the run's last step prefetches no matrix powers, so one step more
    # keeps the KT window at one powers call per step, as the timed K steps are)
    t_epoch = min(W + K + KT + 1, max(4, int(args.basis_gb * 1e9 / ((r1 - r0) * 8.0 * (s + 1)))))
    ep = {"left": 0, "flags": []}

    def step():
        if ep["left"] == 0:
            if ep.get("begun"):
                ep["flags"] += list(ctx.lanczos_get()[3])
            ctx.lanczos_begin(r_full[r0:r1], s, t_epoch, args.basis, args.orth)
            ep["left"], ep["begun"] = t_epoch, True
        ctx.lanczos_step(False)
        ep["left"] -= 1

    # the first begin (normest / Newton prologue: the first RCCL all-reduces)
    # and the first outer step (the first deep halo exchange) under their own
    # watchdog stages, synchronised so that a hang is seen where it happens
    stage("lanczos_begin")
    ctx.lanczos_begin(r_full[r0:r1], s, t_epoch, args.basis, args.orth)
    ep["left"], ep["begun"] = t_epoch, True
    ctx.synchronize()
    stage("first_outer_step")
    if W > 0:
        step()
        ctx.synchronize()
    stage("warmup")
    for _ in range(max(W - 1, 0)):
        step()
    ctx.synchronize()
    if dist is not None:
        dist.barrier()
    ctx.synchronize()
    stage("timed")
    t0 = time.perf_counter()
    for _ in range(K):
        step()
    ctx.synchronize()
    t1 = time.perf_counter()
    if dist is not None:
        dist.barrier()
    elapsed = t1 - t0
    if args.dump_outputs and rank == 0:
        dump_lanczos(ctx, args.dump_outputs)
    if not args.full:
        return finish_plain(args, E, wd, elapsed, list(ep["flags"]) + list(ctx.lanczos_get()[3]))
    ctx.timer_enable(True)
    ctx.timer_reset()
    ctx.comm_stats(reset=True)
    for _ in range(KT):
        step()
    ctx.synchronize()
    spmv_cnt, spmv_ms = ctx.timer_read("spmv")
    gram_cnt, gram_ms = ctx.timer_read("gram")
    apply_cnt, apply_ms = ctx.timer_read("apply")
    ar_cnt, ar_ms = ctx.timer_read("allreduce")
    halo_cnt, halo_ms = ctx.timer_read("halo")
    cstats = ctx.comm_stats(reset=True)
    ctx.timer_enable(False)
    stage("legs")
    T, _, _, flags, info = ctx.lanczos_get()
    flags = np.concatenate([np.asarray(ep["flags"], dtype=flags.dtype), flags])
    elapsed, spmv_avg_ms = max_over_ranks(dist, [elapsed, spmv_ms / max(spmv_cnt, 1)])

    fmt, npat, nent = ctx.spmv_format()
    npairpat, npent, nsplit = ctx.spmv_pair_info()
    mpk = ctx.mpk_info()
    sched = ctx.mpk_schedule()  # what the last timed step's matrix powers actually did
    if wd is not None:
        # a secondary leg that hangs or overruns its stage limit leaves this line
        wd.fallback = {
            "metric": "CA-Lanczos outer-iters/sec (n~10M, s=8)", "value": K / elapsed, "unit": "outer-iters/s",
            "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": 1e3 * elapsed / K, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": wl.data,
            "config": {"workload": wl.desc % (n, nnz_total), "s": s, "basis": args.basis, "orth": args.orth,
                       "parallelism": "row-slab x%d" % world, "normalize": args.normalize, "comm": args.comm,
                       "halo": "%s (CA matrix powers depth %d, band %d rows)"
                               % (ctx.MPK_SCHEDULES.get(sched, "?"), mpk["depth"], mpk["band_l"])}}
    apply_avg_ms = apply_ms / max(apply_cnt, 1)
    gram_avg_ms = gram_ms / max(gram_cnt, 1)
    csr_spmv = None
    host_rt_ms = None
    pat_spmv = None
    csr_leg = None
    lap2d_leg = None
    cfg2_leg = None
    full_leg = None
    irl_leg = None
    # the same outer iteration with the Householder TSQR normalize (tsqr.m,
    # BASELINE configs 3/4: "TSQR" / "RCCL TSQR tree"), every rank
    tsqr_leg = None
    if args.normalize != "tsqr" and not args.no_legs:
        ctx.set_normalize("tsqr")
        try:  # a secondary leg: a failure is reported in the line, the headline stands
            f0 = ctx.tsqr_fold_stats()
            tsqr_leg = timed_leg(ctx, r_full[r0:r1], s, min(K, 10), min(W, 2), args.basis, args.orth, dist)
            f1 = ctx.tsqr_fold_stats()
            tsqr_leg["fold"] = {"blocks": f1["runs"] - f0["runs"], "declined": f1["declined"] - f0["declined"],
                                "last_loss_estimate": f1["last_est"]}
        except cal.CalError as e:
            tsqr_leg = {"error": str(e)}
            try:
                ctx.lanczos_end()
            except cal.CalError:
                pass
        ctx.set_normalize(args.normalize)
    if world > 1 and not args.no_legs and args.comm == "rccl" and args.orth == "local":
        # BASELINE config 5 names 8 GPUs: the implicit restart on every rank's
        # row slab of the G3_circuit stand-in (compact halo, RCCL).  A solve
        # takes ~700 collectives, so it is skipped when the timed steps saw
        # all-reduces slower than IRL_MAX_ALLREDUCE_US (ranks sharing one GPU
        # over sockets: ~55 ms per all-reduce at 8 ranks, 37 s per solve)
        ar_us = max_over_ranks(dist, [ar_ms / max(ar_cnt, 1) * 1e3])[0]
        if ar_us > IRL_MAX_ALLREDUCE_US:
            irl_leg = {"skipped": "all-reduce %.0f us per call in the timed steps (> %.0f us: ranks sharing a GPU "
                                  "over sockets)" % (ar_us, IRL_MAX_ALLREDUCE_US)}
        else:
            try:
                irl_leg = irl_workload_leg(cal, ctx.device, "circuit_1259", s, args.basis, dist=dist, args=args)
            except cal.CalError as e:
                irl_leg = {"error": str(e)}
    if world == 1 and not args.no_legs and args.orth == "local":
        # ca_lanczos.m:191-197 'full': the new block projected against all of Q
        # (one wide Gram and one wide apply sweep per step, f1)
        try:
            # k = 2 .. 15 timed (k = 1 is the warm-up): the cost per step grows with k
            full_leg = timed_leg(ctx, r_full[r0:r1], s, 14, 1, args.basis, "full", dist)
            full_leg["what"] = "outer iterations k = 2..15 of ca_lanczos 'full' (k = 1 untimed)"
            fmt0, _, _ = ctx.spmv_format()
            leg_roofline(full_leg, fmt0, ctx.spmv_pair_info()[0], r1 - r0, nnz_local, s)
        except cal.CalError as e:
            full_leg = {"error": str(e)}
    if world == 1 and rank == 0 and ctx.spmv_format()[0] == "pattern":
        # the bench's own SpMV kernel back to back on one x / y pair (the
        # Infinity Cache holds both): the kernel's rate outside the loop
        pat_spmv = ctx.bench_spmv(20, 1.0)
    if world == 1 and rank == 0:
        # the same SpMV in plain CSR (12 B/nonzero), device-resident, for reference
        ctx2 = cal.Context(device=local, spmv_format="csr")
        ctx2.set_matrix(wl.full())
        csr_spmv = ctx2.bench_spmv(20, 1.0)
        if not args.no_legs:
            # the whole outer iteration with A in plain CSR (12 B / nonzero):
            # SURVEY §8d's 619 / 691 outer-it/s bound is for this format
            csr_leg = timed_leg(ctx2, r_full[r0:r1], s, min(K, 10), min(W, 2), args.basis, args.orth, None)
        ctx2.close()
        if not args.no_legs:
            # north_star's literal target (a ~10M-row 5-pt Laplacian at s = 8)
            # and BASELINE config 5's driver on the G3_circuit stand-in
            if wl.name != "lap2d_3162":
                try:
                    lap2d_leg = workload_leg(cal, local, "lap2d_3162", s, min(K, 15), min(W, 2), args.basis)
                except cal.CalError as e:
                    lap2d_leg = {"error": str(e)}
            # BASELINE config 2 (lap2d_1000, n = 1e6, CholQR): a step of ~0.17 ms,
            # so 100 timed steps, and the timed kernels' share of the step (the
            # rest is launch boundaries and small kernels: SURVEY §8d's
            # cache-resident caveat)
            if wl.name != "lap2d_1000":
                try:
                    cfg2_leg = workload_leg(cal, local, "lap2d_1000", s, 100, 5, args.basis)
                    cfg2_leg["normalize"] = "CholQR2 fused into the sweeps (the CholQR of config 2)"
                    cfg2_leg["launch_boundaries"] = launch_boundaries(cfg2_leg)
                except cal.CalError as e:
                    cfg2_leg = {"error": str(e)}
            try:
                irl_leg = irl_workload_leg(cal, local, "circuit_1259", s, args.basis)
            except cal.CalError as e:
                irl_leg = {"error": str(e)}
        # tier-1 host-pointer SpMV (MATLAB-boundary semantics: PCIe in and out)
        v = np.ones(n)
        ctx.spmv(v)
        t_h = time.perf_counter()
        for _ in range(3):
            ctx.spmv(v)
        host_rt_ms = (time.perf_counter() - t_h) / 3 * 1e3
        del v
    # per-rank communication figures of the KT timed steps (max over ranks)
    comm_line = None
    if world > 1:
        red_rows = cstats["spmv_rows"] / KT - s * (r1 - r0)
        mx = max_over_ranks(dist, [ar_ms / KT * 1e3, ar_cnt / KT, halo_ms / KT * 1e3, halo_cnt / KT, red_rows,
                                   cstats["halo_doubles"] * 8.0 / KT])
        comm_line = {"allreduce_us_per_step": mx[0], "allreduces_per_step": mx[1],
                     "halo_us_per_step": mx[2], "halo_exchanges_per_step": mx[3],
                     "mpk_redundant_rows_per_step": mx[4], "halo_bytes_per_step": mx[5],
                     "rccl_comm_count": cstats["rccl_count"], "comm_kind": {0: "none", 1: "rccl", 2: "host"}.get(
                         cstats["kind"], "?"),
                     "what": "max over ranks of the KT event-timed steps: RCCL all-reduce and halo-exchange time "
                             "(timed on the streams they run on; the halo overlaps the interior powers), counts, "
                             "SpMV rows computed beyond the slab (CA matrix-powers ghost zone)"}
    stage("finalize")
    if rank != 0:
        dist.barrier()
        if wd is not None:
            wd.done()
        return

    n_loc = r1 - r0
    # per-launch algorithmic bytes:
    #   SpMV CSR: 12 nnz + 20 n + 4; row-pattern: 2 n (ids) + 8 n (x) + 8 n (y);
    #   apply (pass B, chained): (w + m) * 8 read + m * 8 written per row (w = s+1, m = s)
    #   Gram sweeps (P1 and pass A): (w + m) * 8 read per row
    b_csr = 12 * nnz_local + 20 * n_loc + 4
    #   pair patterns: 1 B of id per row (one 2-B id per row pair)
    b_spmv1 = (17 if npairpat else 18) * n_loc if fmt == "pattern" else b_csr
    lpp = max(1, ctx.powers_launches())  # SpMV-class launches per outer iteration
    b_spmv_launch = spmv_launch_bytes(fmt, npairpat, n_loc, s, lpp, b_csr)
    b_apply = (2 * s + 1 + s) * 8 * n_loc
    b_gram = (2 * s + 1) * 8 * n_loc
    spmv_gbps = b_spmv_launch / (spmv_avg_ms * 1e-3) / 1e9
    # (the first timed step's powers were prefetched untimed: SpMV = avg launch x s)
    per_step = {"spmv": spmv_avg_ms * lpp, "gram": gram_ms / KT, "apply": apply_ms / KT}
    dominant = max(per_step, key=per_step.get)
    dom = {"spmv": (b_spmv_launch, spmv_avg_ms,
                    ("k_spmv_planes / k_spmv_pair (row-pattern SpMV + Newton shift)"
                     if npairpat else "k_spmv_pat_lds (row-pattern SpMV + Newton shift)")
                    if fmt == "pattern" else "k_spmv (CSR-stream SpMV + Newton shift)"),
           "gram": (b_gram, gram_avg_ms, "k_rowapply Gram sweeps ([Qp|X]'X and pass A, MFMA tile Gram, no store)"),
           "apply": (b_apply, apply_avg_ms, "k_rowapply<17,8,chained> (block orthogonalisation pass B)")}[dominant]
    achieved = dom[0] / (dom[1] * 1e-3) / 1e9
    traffic = traffic_for(args, wl, world, dominant)
    n_reorth = int(np.sum(flags[W:W + K]))
    # whole-step algorithmic HBM bytes of this implementation:
    # s SpMVs + P1 + pass A (Gram sweeps) + pass B (chained apply), per rank
    b_step = lpp * b_spmv_launch + 2 * b_gram + b_apply
    b_outer = s * (12 * nnz_total + 20 * n + 4) + 8 * n * (5 * s + 2)
    line = {
        "metric": "CA-Lanczos outer-iters/sec (n~10M, s=8)",
        "value": K / elapsed,
        "unit": "outer-iters/s",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": 1e3 * elapsed / K,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": wl.data,
        "config": {"workload": wl.desc % (n, nnz_total),
                   "s": s, "basis": args.basis, "orth": args.orth, "parallelism": "row-slab x%d" % world,
                   "normalize": {"auto": "CholQR2 fused into the block-orthogonalisation sweeps (Householder TSQR "
                                         "when its Cholesky fails; tsqr_step times the TSQR leg)",
                                 "cholqr2": "CholQR2 (shifted CholQR3 fallback)",
                                 "tsqr": "Householder TSQR tree"}[args.normalize],
                   "comm": (args.comm if world > 1 else "none"),
                   "halo": ("%s (CA matrix powers depth %d, band %d rows)"
                            % (ctx.MPK_SCHEDULES.get(sched, "?"), mpk["depth"], mpk["band_l"]))
                           if world > 1 else "none"},
        "spmv_format": ("%s (%d row patterns, %d entries; %d pair patterns, %d entries, %d split pairs)"
                        % (fmt, npat, nent, npairpat, npent, nsplit)) if fmt == "pattern" else fmt,
        "spmv_gbps": spmv_gbps,
        "spmv_avg_us": spmv_avg_ms * 1e3,
        "spmv_launches_per_step": lpp,
        "spmv_bytes_per_launch": b_spmv_launch,
        "reorth_passes": "%d/%d" % (n_reorth, K),
        "csr_outer_algorithmic_GB": b_outer / 1e9,
        "kernel_ms_per_step": per_step,
        "step_hbm": {"algorithmic_GB_per_rank": b_step / 1e9,
                     "achieved_GBps_per_rank": b_step / (elapsed / K) / 1e9,
                     "frac": b_step / (elapsed / K) / 1e9 / HBM_PEAK_GBS},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                     "kernel": dom[2], "bytes_per_launch": dom[0], "avg_launch_us": dom[1] * 1e3},
        # the Gram sweeps' matrix-core work: one 16x16 f64 tile Gram per 4
        # rows (v_mfma_f64_16x16x4f64), 512 n flops per launch
        "gram_mfma": gram_mfma(n_loc, gram_avg_ms, b_gram, wl.name, world),
    }
    if pat_spmv is not None:
        line["spmv_kernel_back_to_back"] = {"avg_us": pat_spmv[0] * 1e3, "min_us": pat_spmv[1] * 1e3,
                                            "gbps": b_spmv1 / (pat_spmv[0] * 1e-3) / 1e9,
                                            "bytes_per_launch": b_spmv1}
    if tsqr_leg is not None and "error" not in tsqr_leg:
        # per step: P1 Gram + pass-A projection Gram + TSQR up (leaf sweep
        # "gram") + TSQR down (leaf sweep "apply") + tree levels ("other")
        tsqr_leg["normalize"] = "Householder TSQR (tile QR per wave, stacked-R tree%s)" % (
            ", RCCL allgather of the rank roots" if world > 1 else "")
        line["tsqr_step"] = tsqr_leg
    elif tsqr_leg is not None:
        line["tsqr_step"] = tsqr_leg
    if csr_leg is not None:
        csr_leg["spmv_format"] = "csr"
        csr_leg["spmv_avg_us"] = csr_leg["kernel_avg_launch_us"]["spmv"]
        csr_leg["spmv_gbps"] = b_csr / (csr_leg["spmv_avg_us"] * 1e-6) / 1e9
        csr_leg["spmv_frac"] = csr_leg["spmv_gbps"] / HBM_PEAK_GBS
        csr_leg["survey_bound_outer_iters_per_s"] = HBM_PEAK_GBS * 1e9 / (b_outer + 8 * n * (2 * s + 1))
        line["csr_step"] = csr_leg
    if lap2d_leg is not None:
        line["lap2d_3162_step"] = lap2d_leg
    if cfg2_leg is not None:
        line["lap2d_1000_step"] = cfg2_leg
    if full_leg is not None:
        line["full_step"] = full_leg
    if irl_leg is not None:
        line["irl"] = irl_leg
    if csr_spmv is not None:
        line["spmv_csr_kernel"] = {"avg_us": csr_spmv[0] * 1e3, "min_us": csr_spmv[1] * 1e3,
                                   "gbps": b_csr / (csr_spmv[0] * 1e-3) / 1e9, "bytes_per_launch": b_csr}
    if host_rt_ms is not None:
        line["spmv_host_roundtrip_ms"] = host_rt_ms
    if comm_line is not None:
        line["comm"] = comm_line
    line["host"] = host_info()
    if world == 1 and args.orth == "local":
        line["diagnostics_on"] = diagnostics_run(ctx, r_full[r0:r1], s, args)
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(wl, s, args.cpu_iters, args.basis)
        line["cpu_baseline_numpy"] = cpu_baseline_numpy(wl, s, 2, args.basis)
    emit(line)
    if dist is not None:
        dist.barrier()
    if wd is not None:
        wd.done()


def finish_plain(args, E, wd, elapsed, flags):
    """The line of a plain run (no --full): the headline of the K timed steps
    (max over ranks) and what describes them without a further run."""
    world, rank, wl, dist, ctx = (E[k] for k in ("world", "rank", "wl", "dist", "ctx"))
    K, W, s = args.steps, args.warmup, args.s
    elapsed = max_over_ranks(dist, [elapsed])[0]
    if wd is not None:
        wd.enter("finalize", stage_limit("finalize"))
    if rank == 0:
        fmt, npat, nent = ctx.spmv_format()
        npairpat, npent, nsplit = ctx.spmv_pair_info()
        mpk = ctx.mpk_info()
        emit({
            "metric": "CA-Lanczos outer-iters/sec (n~10M, s=8)",
            "value": K / elapsed,
            "unit": "outer-iters/s",
            "n_gpus": world,
            "steps": K,
            "warmup": W,
            "ms_per_step": 1e3 * elapsed / K,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": wl.data,
            "config": {"workload": wl.desc % (wl.n, E["nnz_total"]),
                       "s": s, "basis": args.basis, "orth": args.orth, "parallelism": "row-slab x%d" % world,
                       "normalize": args.normalize, "comm": (args.comm if world > 1 else "none"),
                       "halo": ("%s (CA matrix powers depth %d, band %d rows)"
                                % (ctx.MPK_SCHEDULES.get(ctx.mpk_schedule(), "?"), mpk["depth"], mpk["band_l"]))
                               if world > 1 else "none"},
            "spmv_format": ("%s (%d row patterns, %d entries; %d pair patterns, %d entries, %d split pairs)"
                            % (fmt, npat, nent, npairpat, npent, nsplit)) if fmt == "pattern" else fmt,
            "reorth_passes": "%d/%d" % (int(np.sum(flags[W:W + K])), K),
        })
    if dist is not None:
        dist.barrier()
    if wd is not None:
        wd.done()


def timed_leg(ctx, r, s, K, W, basis, orth, dist):
    """A secondary leg on the same workload: a fresh run, W warm-up and K
    timed outer iterations (barrier + synchronize on both sides, max over
    ranks), then one more with the per-kernel HIP-event timers."""
    KT = 3
    # (+1: the run's last step prefetches no matrix powers; one step more keeps
    # the timed window at one powers call per step)
    ctx.lanczos_begin(r, s, W + K + KT + 1, basis, orth)
    for _ in range(W):
        ctx.lanczos_step(False)
    ctx.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(K):
        ctx.lanczos_step(False)
    ctx.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    ctx.timer_enable(True)
    ctx.timer_reset()
    for _ in range(KT):
        ctx.lanczos_step(False)
    ctx.synchronize()
    tm = {k: ctx.timer_read(k) for k in ("spmv", "gram", "apply", "other")}
    tb = {k: ctx.timer_bytes(k) for k in ("spmv", "gram", "apply")}
    ctx.timer_enable(False)
    flags = ctx.lanczos_get()[3]
    ctx.lanczos_end()
    elapsed = max_over_ranks(dist, [elapsed])[0]
    # the first timed step's matrix powers were prefetched by the untimed step
    # before it: SpMV per step = average launch x s
    per = {k: v[1] / KT for k, v in tm.items()}
    lpp = max(1, ctx.powers_launches())
    per["spmv"] = tm["spmv"][1] / max(tm["spmv"][0], 1) * lpp
    return {"outer_iters_per_s": K / elapsed, "ms_per_step": 1e3 * elapsed / K, "steps": K,
            "reorth_passes": "%d/%d" % (int(np.sum(flags[W:W + K])), K),
            "kernel_ms_per_step": per,
            "kernel_avg_launch_us": {k: 1e3 * v[1] / max(v[0], 1) for k, v in tm.items()},
            "kernel_launches": {k: v[0] for k, v in tm.items()},
            # algorithmic bytes of the timed launches / their summed duration
            # (the library states each launch's bytes, cal_timer_bytes)
            "kernel_gbps": {k: tb[k] / (tm[k][1] * 1e-3) / 1e9 if tm[k][1] > 0 else None for k in tb},
            # the timed kernels' share of the step (the rest: launch boundaries,
            # small untimed kernels, host time the GPU waits on); fixed-shape
            # steps only ('full' projects against a growing Q)
            "kernel_share": (sum(per.values()) / (1e3 * elapsed / K)) if orth in ("local", "periodic") else None,
            "spmv_launches_per_step": lpp}


def spmv_launch_bytes(fmt, npairpat, n_loc, s, lpp, b_csr):
    """Algorithmic HBM bytes per SpMV-class launch when an outer iteration's
    s powers take lpp launches: a row-pattern SpMV reads x and the row's key
    (1 B per row with pair patterns / plane-march mask keys, 2 B otherwise) and
    stores y (a launch that computed several powers would read x and the keys
    once for its s / lpp stored powers)."""
    if fmt != "pattern":
        return b_csr
    kb = 1 if npairpat else 2
    return ((8 + kb) * lpp + 8 * s) * n_loc / lpp


def leg_roofline(leg, fmt, npairpat, n_loc, nnz_loc, s):
    """SpMV GB/s and the roofline of the leg's dominant kernel class: the
    algorithmic bytes the library states for that class's timed launches
    (cal_timer_bytes) over their summed HIP-event durations,
    i.e. bytes per launch / average launch time for fixed-shape launches
    ('local'), and the right average for the growing widths of 'full'."""
    lpp = leg["spmv_launches_per_step"]
    b_spmv = spmv_launch_bytes(fmt, npairpat, n_loc, s, lpp, 12 * nnz_loc + 20 * n_loc + 4)
    avg = leg["kernel_avg_launch_us"]
    per = {k: leg["kernel_ms_per_step"][k] for k in ("spmv", "gram", "apply")}
    dom = max(per, key=per.get)
    leg["spmv_gbps"] = b_spmv / (avg["spmv"] * 1e-6) / 1e9
    leg["spmv_frac"] = leg["spmv_gbps"] / HBM_PEAK_GBS
    ach = leg["kernel_gbps"][dom]
    nl = max(leg["kernel_launches"][dom], 1)
    leg["roofline"] = {"bound": "hbm", "kernel_class": dom, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": ach / HBM_PEAK_GBS, "bytes_per_launch": ach * 1e9 * avg[dom] * 1e-6,
                       "avg_launch_us": avg[dom], "launches": nl}
    return leg


def workload_leg(cal, local, name, s, K, W, basis):
    """The headline's outer iteration (same s, basis, 'local', default
    normalize) on another resident workload, one GPU: outer-it/s, SpMV GB/s
    and the dominant kernel class's roofline fraction."""
    wl2 = Workload(name)
    c = cal.Context(device=local)
    try:
        c.set_matrix(wl2.full())
        r = np.random.RandomState(5489).random_sample(wl2.n)
        leg = timed_leg(c, r, s, K, W, basis, "local", None)
        fmt, npat, nent = c.spmv_format()
        npairpat, npent, nsplit = c.spmv_pair_info()
        nnz = c.matrix_info()["nnz_local"]
        leg["workload"] = wl2.desc % (wl2.n, nnz)
        leg["spmv_format"] = ("%s (%d pair patterns, %d split pairs)" % (fmt, npairpat, nsplit)
                              if fmt == "pattern" else fmt)
        pP, pH, pmode = c.spmv_plane_info()
        if pP > 0:
            leg["spmv_format"] = "pattern (plane march: plane stride %d, in-plane reach %d, key mode %d)" % (
                pP, pH, pmode)
        leg_roofline(leg, fmt, npairpat, wl2.n, nnz, s)
        if fmt == "pattern":
            b2b = c.bench_spmv(20, 1.0)
            leg["spmv_kernel_back_to_back"] = {"avg_us": b2b[0] * 1e3,
                                               "gbps": (17 if npairpat else 18) * wl2.n / (b2b[0] * 1e-3) / 1e9}
    finally:
        c.close()
    return leg


def irl_workload_leg(cal, local, name, s, basis, ml=64, nw=8, tol=1.0e-8, dist=None, args=None):
    """BASELINE config 5's driver as a leg of the default line: whole
    impl_restarted_ca_lanczos solves on the resident G3_circuit stand-in
    (CSR SpMV), solves/s and the SpMV's roofline inside the solve.  With
    dist (a multi-rank line: config 5 names 8 GPUs) every rank holds a row
    slab of the matrix on a context with a communicator of its own; the
    solve time is the max over ranks, the SpMV figures are rank 0's."""
    wl2 = Workload(name)
    world = dist.get_world_size() if dist is not None else 1
    rank = dist.get_rank() if dist is not None else 0
    c = cal.Context(device=local)
    try:
        r = np.random.RandomState(5489).random_sample(wl2.n)
        if world > 1:
            from ca_lanczos_amd.matrices import slab_bounds
            import scipy.sparse as sp
            rank_comm(cal, c, args, world, rank, dist)
            b = slab_bounds(wl2.n, world, wl2.plane)
            r0, r1 = b[rank], b[rank + 1]
            rowptr, col, val = wl2.rows(r0, r1)
            c.set_matrix_slab(wl2.n, r0, sp.csr_matrix((val, col, rowptr), shape=(r1 - r0, wl2.n)))
            r = r[r0:r1]
        else:
            r0, r1 = 0, wl2.n
            c.set_matrix(wl2.full())
        M = irl_measure(cal, c, r, ml, nw, s, basis, tol, 3, 1, dist)
        fmt = c.spmv_format()[0]
        nnz = c.matrix_info()["nnz_local"]
    finally:
        c.close()
    n_loc = r1 - r0
    b_spmv = (12 * nnz + 20 * n_loc + 4) if fmt == "csr" else 18 * n_loc
    ach = b_spmv / (M["spmv_avg_ms"] * 1e-3) / 1e9
    t = M["timers"]
    return {"solves_per_s": M["K"] / M["elapsed"], "ms_per_solve": 1e3 * M["elapsed"] / M["K"], "solves": M["K"],
            "n_ranks": world, "workload": wl2.desc % (wl2.n, wl2.full().nnz), "driver": "impl_restarted_ca_lanczos",
            "max_lanczos": ml, "n_wanted_eigs": nw, "m": M["m"], "s": s, "orth": "full", "tol": tol,
            "num_restarts": M["out"]["num_restarts"], "converged": M["out"]["converged"],
            "blocks_per_s": M["blocks"] / M["elapsed"], "spmv_format": fmt,
            "kernel_ms_per_solve": {"spmv": t[1], "gram": t[3], "apply": t[5], "other": M["other_ms"]},
            "kernel_launches_per_solve": {"spmv": t[0], "gram": t[2], "apply": t[4]},
            "roofline": irl_roofline(M)[0], "time_split": irl_roofline(M)[1],
            "spmv_roofline": {"bound": "hbm", "kernel": "SpMV (%s) inside the solve" % fmt, "achieved": ach,
                              "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                              "bytes_per_launch": b_spmv, "avg_launch_us": M["spmv_avg_ms"] * 1e3}}


def diagnostics_run(ctx, r, s, args, t=15):
    """The reference-faithful cost: ca_lanczos.m computes the
    Ritz residual norms and the orthogonality error at every outer iteration
    (compute_ritz_rnorm / compute_orth_err, ca_lanczos.m:88-107,229-235).
    t outer iterations with both on; the Newton prologue (in begin) excluded.
    One untimed run of the same t first (as the main loop's warm-up steps: the
    first launches of the diagnostics' kernels and its Ritz-vector buffers;
    measured 166 -> 182 outer-it/s from the first run to the next)."""
    def run():
        ctx.lanczos_begin(r, s, t, args.basis, args.orth)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(t):
            ctx.lanczos_step(True)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        info = ctx.lanczos_get()[4]
        ctx.lanczos_end()
        return dt, info

    run()  # warm-up (untimed)
    dt, info = run()
    return {"outer_iters": t, "ms": dt * 1e3, "outer_iters_per_s": t / dt, "diag_ms": info.diag_ms,
            "warmup_runs": 1,
            "what": "Ritz residual norms of all s*k Ritz pairs (eig of T, x = Q*Vp(:,i), ||Ax - lx||) and "
                    "the orthogonality error after every outer iteration, as the reference always runs"}


def irl_measure(cal, ctx, r_loc, ml, nw, s, basis, tol, K, W, dist, full=True):
    """Time K whole impl_restarted_ca_lanczos solves after W warm-up solves
    (barrier + synchronize on both sides, max over ranks), then (full) one
    solve with the per-kernel HIP-event timers and one that downloads Q_conv."""
    # k kept, p shifts, m = k + p (impl_restarted_ca_lanczos.m:72-74, k >= s; include/calanczos.h)
    k = max(nw + 4, s)
    p = s * ((ml - k) // s)
    m = k + p

    def solve(return_Q=False):
        # timed solves leave the Ritz vectors Q_conv on the device (the bench's
        # inputs and outputs are HBM-resident); one more solve below returns
        # them over PCIe and is reported beside the line
        return cal.impl_restarted_ca_lanczos(None, r_loc, ml, nw, s, basis, "full", tol, ctx=ctx,
                                             return_Q=return_Q)

    for _ in range(W):
        solve()
    ctx.synchronize()
    if dist is not None:
        dist.barrier()
    blocks = 0
    t0 = time.perf_counter()
    for _ in range(K):
        out = solve()
        blocks += -(-m // s) + (out["num_restarts"] - 1) * (p // s)
    ctx.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    if not full:
        return {"k": k, "p": p, "m": m, "out": out, "elapsed": max_over_ranks(dist, [elapsed])[0],
                "blocks": blocks, "K": K}
    last = out
    ctx.timer_enable(True)
    ctx.timer_reset()
    out = solve()
    timers = []
    for kind in ("spmv", "gram", "apply"):
        timers += list(ctx.timer_read(kind))
    other_ms = ctx.timer_read("other")[1]
    normest_ms = ctx.timer_read("normest")[1]  # on its own stream, beside the timed classes
    tbytes = {k: ctx.timer_bytes(k) for k in ("spmv", "gram", "apply")}
    ctx.timer_enable(False)
    t_q = time.perf_counter()
    solve(return_Q=True)
    solve_q_ms = (time.perf_counter() - t_q) * 1e3
    elapsed, spmv_avg_ms = max_over_ranks(dist, [elapsed, timers[1] / max(timers[0], 1)])
    return {"k": k, "p": p, "m": m, "out": out, "elapsed": elapsed, "spmv_avg_ms": spmv_avg_ms,
            "timers": timers, "other_ms": other_ms, "normest_ms": normest_ms, "bytes": tbytes, "blocks": blocks, "solve_q_ms": solve_q_ms,
            "K": K, "last_timed_out": last}


def irl_roofline(M):
    """The IRL solve's dominant kernel class (by time per solve) and its
    roofline: the library's algorithmic bytes of that class's launches
    (cal_timer_bytes: (a + b) 8 n per Gram of a x b columns, (p + y) 8 n per
    apply, 12 nnz + 20 n + 4 per CSR SpMV) over their summed duration; and
    the share of the solve the timed kernels do not cover (host work and
    the GPU's waits on it, launch boundaries, the small untimed kernels)."""
    t = M["timers"]
    ms = {"spmv": t[1], "gram": t[3], "apply": t[5]}
    dom = max(ms, key=ms.get)
    ach = M["bytes"][dom] / (ms[dom] * 1e-3) / 1e9
    solve_ms = 1e3 * M["elapsed"] / M["K"]
    kern = t[1] + t[3] + t[5] + M["other_ms"]
    return ({"bound": "hbm", "kernel_class": dom, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": ach / HBM_PEAK_GBS, "bytes_per_solve": M["bytes"][dom], "ms_per_solve": ms[dom],
             "gbps_by_class": {k: M["bytes"][k] / (ms[k] * 1e-3) / 1e9 if ms[k] > 0 else None for k in ms}},
            {"kernel_ms_per_solve": kern, "solve_ms": solve_ms, "untimed_share": max(0.0, 1.0 - kern / solve_ms),
             # normest(A) runs on its own stream beside the prologue and the
             # first CA blocks (one rank): its span overlaps the timed kernels
             # and is not in kernel_ms_per_solve
             "normest_concurrent_span_ms": M.get("normest_ms", 0.0)})


def main_irl(args, wd=None):
    """BASELINE config 5: whole impl_restarted_ca_lanczos solves (normest,
    Newton prologue, CA blocks, shifts, compression) on resident A."""
    E = setup(args, wd)
    if wd is not None:
        wd.enter("timed", stage_limit("timed"))
    world, rank, wl, cal, dist, ctx = (E[k] for k in ("world", "rank", "wl", "cal", "dist", "ctx"))
    r0, r1, nnz_local, nnz_total = E["r0"], E["r1"], E["nnz_local"], E["nnz_total"]
    n = wl.n
    s = args.s
    ml, nw = (int(x) for x in args.irl.split(","))
    r_full = np.random.RandomState(5489).random_sample(n)
    K, W = args.steps, args.warmup
    M = irl_measure(cal, ctx, r_full[r0:r1], ml, nw, s, args.basis, args.irl_tol, K, W, dist, full=args.full)
    k, m, out = M["k"], M["m"], M["out"]
    elapsed, blocks = M["elapsed"], M["blocks"]
    if args.dump_outputs and rank == 0:
        dump_irl(M.get("last_timed_out", out), args.dump_outputs)
    if wd is not None:
        wd.enter("finalize", stage_limit("finalize"))
    if rank != 0:
        dist.barrier()
        if wd is not None:
            wd.done()
        return
    fmt, _, _ = ctx.spmv_format()
    line = {
        "metric": "impl_restarted_ca_lanczos solves/sec (BASELINE config 5)",
        "value": K / elapsed,
        "unit": "solves/s",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": 1e3 * elapsed / K,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": wl.data,
        "config": {"workload": wl.desc % (n, nnz_total), "driver": "impl_restarted_ca_lanczos",
                   "max_lanczos": ml, "n_wanted_eigs": nw, "k": k, "m": m, "s": s, "basis": args.basis,
                   "orth": "full", "tol": args.irl_tol, "parallelism": "row-slab x%d" % world,
                   "comm": (args.comm if world > 1 else "none")},
        "num_restarts": out["num_restarts"],
        "converged": out["converged"],
        "top_eigs": [float(x) for x in out["conv_eigs"][:3]],
        "blocks_per_s": blocks / elapsed,
        "spmv_format": fmt,
    }
    if args.full:
        full_irl_line(args, E, M, line)
    emit(line)
    if dist is not None:
        dist.barrier()
    if wd is not None:
        wd.done()


def full_irl_line(args, E, M, line):
    """--full of the IRL driver: the event-timed solve's per-kernel figures
    and rooflines, the solve that downloads Q_conv and the CPU baseline."""
    world, wl = E["world"], E["wl"]
    nnz_local, n_loc = E["nnz_local"], E["r1"] - E["r0"]
    ml, nw = (int(x) for x in args.irl.split(","))
    spmv_avg_ms = M["spmv_avg_ms"]
    spmv_cnt, spmv_ms, gram_cnt, gram_ms, apply_cnt, apply_ms = M["timers"]
    fmt = line["spmv_format"]
    b_spmv = (12 * nnz_local + 20 * n_loc + 4) if fmt == "csr" else 18 * n_loc
    achieved = b_spmv / (spmv_avg_ms * 1e-3) / 1e9
    line.update({
        "solve_with_q_conv_download_ms": M["solve_q_ms"],
        "kernel_ms_per_solve": {"spmv": spmv_ms, "gram": gram_ms, "apply": apply_ms, "other": M["other_ms"]},
        "kernel_launches_per_solve": {"spmv": spmv_cnt, "gram": gram_cnt, "apply": apply_cnt},
        "roofline": dict(irl_roofline(M)[0], traffic=None),
        "time_split": irl_roofline(M)[1],
        "spmv_roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "frac": achieved / HBM_PEAK_GBS, "traffic": traffic_for(args, wl, world, "spmv"),
                          "kernel": "SpMV (%s) inside the IRL" % fmt, "bytes_per_launch": b_spmv,
                          "avg_launch_us": spmv_avg_ms * 1e3},
    })
    line["host"] = host_info()
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_irl(wl, args.s, ml, nw)


if __name__ == "__main__":
    sys.exit(main() or 0)
