"""MATLAB-named host mirror of the reference hot path over the C ABI.

Each function keeps the reference's name, argument meaning, defaults and
error behaviour (file:line cited per function) and calls the HIP library; a
sparse ``A`` is uploaded once and kept resident in HBM for every later call
with the same matrix object (the "two tiers" boundary of SURVEY §8b).
"""
from __future__ import annotations

import ctypes
import math
import os
import weakref
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import CalError, check, dp, f64, iptr, lib, ptr
from .matrices import to_csr


class Context:
    """A device context (``cal_ctx``): one HIP stream, the resident matrix and
    the device-resident CA-Lanczos state.

    ``spmv_format`` (cal_set_spmv_format; default ``CAL_SPMV_FORMAT`` or
    "auto") is "auto", "csr", "pattern", "split" or "shared".  "shared" is
    opt-in and takes ``set_matrix_stacked`` (blkdiag(H, H) with H stored
    once, ``spmv_shared_info``) and ``set_matrix_hermitian`` (a complex
    Hermitian H stored once, ``spmv_hermitian_info``) only."""

    def __init__(self, device: int | None = None, spmv_format: str | None = None, orth_coef: str | None = None,
                 mpk_depth: int | None = None, normalize: str | None = None):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        h = ctypes.c_void_p()
        st = lib.cal_create(device, ctypes.byref(h))
        if st != 0:
            raise CalError(st, "cal_create(device=%d) failed: no usable HIP device" % device)
        self.h = h
        self.device = device
        self.n = None
        self._keep = []
        fmt = spmv_format or os.environ.get("CAL_SPMV_FORMAT", "auto")
        check(self.h, lib.cal_set_spmv_format(self.h, fmt.encode()), "spmv format")
        if orth_coef:
            self.set_orth_coef(orth_coef)
        if mpk_depth is not None:
            self.set_mpk_depth(mpk_depth)
        if normalize or os.environ.get("CAL_NORMALIZE"):
            self.set_normalize(normalize or os.environ["CAL_NORMALIZE"])

    def set_normalize(self, kind: str):
        """normalize (tsqr.m) backend: "auto", "tsqr" (Householder TSQR
        everywhere) or "cholqr2" (cal_set_normalize)."""
        check(self.h, lib.cal_set_normalize(self.h, kind.encode()), "normalize backend")
        return self

    def normalize_backend(self):
        v = ctypes.c_int()
        check(self.h, lib.cal_get_normalize(self.h, ctypes.byref(v)))
        return ("auto", "tsqr", "cholqr2")[v.value]

    def set_mpk_depth(self, depth: int):
        """Ghost depth of the distributed CA matrix-powers kernel (next
        set_matrix_slab; 1 = one halo exchange per SpMV)."""
        check(self.h, lib.cal_set_mpk_depth(self.h, int(depth)), "mpk depth")
        return self

    def mpk_info(self):
        """{'depth': active depth (1 = off), 'band_l', 'band_r', 'n_rows' (stored rows)}."""
        d, bl, br, nr = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(self.h, lib.cal_mpk_info(self.h, ctypes.byref(d), ctypes.byref(bl), ctypes.byref(br), ctypes.byref(nr)))
        return dict(depth=d.value, band_l=bl.value, band_r=br.value, n_rows=nr.value)

    MPK_SCHEDULES = {-1: "none", 0: "one exchange per SpMV", 1: "one deep exchange",
                     2: "one deep exchange overlapped with the interior powers",
                     3: "split schedule, no exchange (single-rank stand-in band)",
                     4: "one deep exchange on the host-staged comm thread overlapped with the interior powers"}

    def mpk_schedule(self):
        """Schedule the last matrix-powers call took (cal_mpk_schedule)."""
        v = ctypes.c_int()
        check(self.h, lib.cal_mpk_schedule(self.h, ctypes.byref(v)))
        return v.value

    def powers_launches(self):
        """SpMV-class launches of the last matrix-powers call (cal_powers_launches)."""
        v = ctypes.c_int()
        check(self.h, lib.cal_powers_launches(self.h, ctypes.byref(v)))
        return v.value

    def tsqr_fold_stats(self):
        """Fused-TSQR projectAndNormalize counters (cal_tsqr_fold_stats):
        blocks run, blocks declined (explicit-Z path), last estimate."""
        r, d, e = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
        check(self.h, lib.cal_tsqr_fold_stats(self.h, ctypes.byref(r), ctypes.byref(d), ctypes.byref(e)))
        return dict(runs=r.value, declined=d.value, last_est=e.value)

    def set_tsqr_fold_tol(self, tol: float):
        """The fused TSQR's loss-of-orthogonality acceptance threshold
        (cal_set_tsqr_fold_tol; default 1e-14, 0 declines every block that
        takes the second projection, a negative value every block)."""
        check(self.h, lib.cal_set_tsqr_fold_tol(self.h, float(tol)), "tsqr fold tol")
        return self

    def set_orth_coef(self, where: str):
        """Run the block-orthogonalisation s x s algebra on the "device"
        (default) or on the "host" (same bits; for testing)."""
        check(self.h, lib.cal_set_orth_coef(self.h, where.encode()), "orth coef")
        return self

    def bench_spmv(self, reps=20, shift=0.0):
        """Mean and min SpMV kernel time (ms) on HBM-resident vectors."""
        a, b = ctypes.c_double(), ctypes.c_double()
        check(self.h, lib.cal_bench_spmv(self.h, reps, shift, ctypes.byref(a), ctypes.byref(b)), "bench_spmv")
        return a.value, b.value

    def spmv(self, v):
        v = f64(v).ravel()
        out = np.empty_like(v)
        check(self.h, lib.cal_spmv(self.h, ptr(v), ptr(out)), "SpMV")
        return out

    def spmv_format(self):
        """('pattern'|'csr', number of row patterns, table entries)."""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(self.h, lib.cal_spmv_format(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return ("pattern" if a.value else "csr", b.value, c.value)

    def spmv_pair_info(self):
        """(pair patterns, their table entries, pairs on the per-row path);
        zeros when the two-rows-per-lane kernel is not in use."""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        check(self.h, lib.cal_spmv_pair_info(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def spmv_plane_info(self):
        """(plane stride P, in-plane reach H, key mode) of the plane-march
        kernels; (0, 0, -1) when the matrix does not take them."""
        a, b, c = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
        check(self.h, lib.cal_spmv_plane_info(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def spmv_split_info(self):
        """(on, plane stride P, in-plane reach H, neg1) of the diagonal-split
        format (``spmv_format="split"``, or "auto" on a grid Hamiltonian K +
        diag(V)); (False, 0, 0, False) when the matrix does not run there.
        ``spmv_format()`` reports "csr" for such a matrix: only its SpMV takes
        the split kernels."""
        on, P, H, ng = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
        check(self.h, lib.cal_spmv_split_info(self.h, ctypes.byref(on), ctypes.byref(P), ctypes.byref(H),
                                              ctypes.byref(ng)))
        return bool(on.value), P.value, H.value, bool(ng.value)

    def spmv_shared_info(self):
        """(on, n, nnz stored) of the shared stacked format
        (``spmv_format="shared"`` with ``set_matrix_stacked``): blkdiag(H, H)
        with the n x n H stored once; (False, 0, 0) for any other matrix.
        ``spmv_format()`` reports "csr" and ``matrix_info()`` the logical 2n
        rows and 2 nnz(H) for such a matrix."""
        on, n, nz = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        check(self.h, lib.cal_spmv_shared_info(self.h, ctypes.byref(on), ctypes.byref(n), ctypes.byref(nz)))
        return bool(on.value), n.value, nz.value

    def close(self):
        if self.h:
            lib.cal_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- matrix ---------------------------------------------------------------
    def set_matrix(self, A):
        A = to_csr(A)
        if A.shape[0] != A.shape[1]:
            raise ValueError("A must be square")
        rowptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        col = np.ascontiguousarray(A.indices, dtype=np.int32)
        val = np.ascontiguousarray(A.data, dtype=np.float64)
        check(self.h, lib.cal_set_matrix_csr(self.h, A.shape[0], rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                             col.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ptr(val)),
              "set_matrix")
        self.n = A.shape[0]
        return self

    def set_matrix_stacked(self, H):
        """blkdiag(H, H) through cal_set_matrix_csr_stacked: the real form of
        a complex problem on stacked vectors [Re; Im] (the time propagator).
        On a ``spmv_format="shared"`` context H is stored once and serves both
        halves (same bits as the stacked "csr" context); that format takes no
        other way of setting a matrix but ``set_matrix_hermitian``."""
        H = to_csr(H)
        if H.shape[0] != H.shape[1]:
            raise ValueError("H must be square")
        rowptr = np.ascontiguousarray(H.indptr, dtype=np.int64)
        col = np.ascontiguousarray(H.indices, dtype=np.int32)
        val = np.ascontiguousarray(H.data, dtype=np.float64)
        check(self.h, lib.cal_set_matrix_csr_stacked(
            self.h, H.shape[0], rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            col.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ptr(val)), "set_matrix_stacked")
        self.n = 2 * H.shape[0]
        return self

    def set_matrix_hermitian(self, H):
        """A complex Hermitian sparse H = A + iB through
        cal_set_matrix_csr_hermitian: the real symmetric 2n x 2n matrix
        E(H) = [[A, -B], [B, A]] on stacked vectors [Re; Im]
        (``matrices.hermitian_embedding``), which the time propagator takes
        as it takes ``set_matrix_stacked``'s.  ``H.data.real`` and
        ``H.data.imag`` go down; a real dtype passes no imaginary part and is
        ``set_matrix_stacked(H)``.  The stored diagonal must be real, and
        Hermiticity of the rest is the caller's contract.  On a
        ``spmv_format="shared"`` context H is stored once (20 bytes per
        nonzero, ``spmv_hermitian_info``); any other format stores the
        embedding, four entries per nonzero of H."""
        H = to_csr(H)
        if H.shape[0] != H.shape[1]:
            raise ValueError("H must be square")
        rowptr = np.ascontiguousarray(H.indptr, dtype=np.int64)
        col = np.ascontiguousarray(H.indices, dtype=np.int32)
        re = np.ascontiguousarray(H.data.real, dtype=np.float64)
        im = np.ascontiguousarray(H.data.imag, dtype=np.float64) if np.iscomplexobj(H.data) else None
        check(self.h, lib.cal_set_matrix_csr_hermitian(
            self.h, H.shape[0], rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            col.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ptr(re), ptr(im)), "set_matrix_hermitian")
        self.n = 2 * H.shape[0]
        return self

    def spmv_hermitian_info(self):
        """(on, n, nnz stored) of the Hermitian stored-once format
        (``spmv_format="shared"`` with ``set_matrix_hermitian`` of a complex
        H); (False, 0, 0) for any other matrix, the host-built embedding of
        the other formats included."""
        on, n, nz = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        check(self.h, lib.cal_spmv_hermitian_info(self.h, ctypes.byref(on), ctypes.byref(n), ctypes.byref(nz)))
        return bool(on.value), n.value, nz.value

    def _prop_combine(self, Q, c, mask, W, phi, entry):
        """The marshalling of the three host-data combine entries; ``entry``
        names the one to call ("prop_combine": no observables, no mask;
        "prop_combine_obs": no mask; "prop_combine_masked").  Returns (out,
        norm2, absorbed, <W_k>, <phi_r|out>)."""
        Q = f64(Q)
        n, m = Q.shape[0] // 2, Q.shape[1]
        c = np.asarray(c, dtype=np.complex128).ravel()
        cre, cim = np.ascontiguousarray(c.real), np.ascontiguousarray(c.imag)
        args = [self.h, n, m, ptr(Q), ptr(cre), ptr(cim)]
        if entry == "prop_combine_masked":
            mk = np.ascontiguousarray(mask, dtype=np.float64).ravel()
            if mk.shape[0] != n:
                raise ValueError("the mask needs n entries")
            args.append(ptr(mk))
        Wm, pre, pim = _obs_arrays(n, W, phi)
        nw, nphi = Wm.shape[1], pre.shape[1]
        ore, oim = np.zeros(n), np.zeros(n)
        sums = np.zeros(max(nw + 2 * nphi, 1))
        n2, ab = ctypes.c_double(), ctypes.c_double()
        if entry != "prop_combine":
            args += [nw, ptr(Wm) if nw else None, nphi, ptr(pre) if nphi else None, ptr(pim) if nphi else None]
        args += [ptr(ore), ptr(oim), ctypes.cast(ctypes.byref(n2), dp)]
        if entry == "prop_combine_masked":
            args.append(ctypes.cast(ctypes.byref(ab), dp))
        if entry != "prop_combine":
            args.append(ptr(sums))
        check(self.h, getattr(lib, "cal_" + entry)(*args), entry)
        ov = sums[nw:nw + 2 * nphi]
        return ore + 1j * oim, n2.value, ab.value, sums[:nw].copy(), ov[0::2] + 1j * ov[1::2]

    def prop_combine(self, Q, c):
        """``nrm * Q_c * c`` on stacked halves (cal_prop_combine): Q is
        2n x m real, c complex with m entries; returns (complex n-vector,
        sum |out|^2 as the kernel's block partials reduce it)."""
        return self._prop_combine(Q, c, None, None, None, "prop_combine")[:2]

    def prop_combine_obs(self, Q, c, W=None, phi=None):
        """``prop_combine`` through the kernel that also reduces observables
        (cal_prop_combine_obs): W real diagonal operators (a list or n x nw),
        phi complex reference states (a list or n x nphi), at most 4 each.
        Returns (out, norm2, <W_k> = sum W_k |out|^2 (nw), <phi_r|out> (nphi,
        complex)); out and norm2 have the bits of ``prop_combine``."""
        out, n2, _, wv, ov = self._prop_combine(Q, c, None, W, phi, "prop_combine_obs")
        return out, n2, wv, ov

    def prop_combine_masked(self, Q, c, mask, W=None, phi=None):
        """``prop_combine_obs`` through the kernel that multiplies the result
        by a real mask in [0, 1] before it is stored (cal_prop_combine_masked):
        with u = ``prop_combine(Q, c)``, out = mask * u.  Returns (out, norm2,
        absorbed = sum (1 - mask^2) |u|^2, <W_k>, <phi_r|out>); norm2 and the
        observables are those of out."""
        return self._prop_combine(Q, c, mask, W, phi, "prop_combine_masked")

    def prop_combine_real(self, Q, a, W=None):
        """The real state's combine sweep on host data
        (cal_prop_combine_real): Q is n x m real, a real with m entries;
        ``out[i] = sum_j Q[i, j] a_j`` as one chain per row over ascending j.
        W: real diagonal operators (a list or n x nw, at most 4).  Returns
        (out, norm2 = sum out^2, <W_k> = sum W_k out^2 (nw)).  A Q that is a
        column-major view with a column stride above n (``big[:n, :]``) keeps
        that leading dimension on the device: an odd one runs the kernel's
        8-byte path."""
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim != 2:
            raise ValueError("Q must be n x m")
        n, m = Q.shape
        it = Q.itemsize
        if not (n >= 1 and Q.strides[0] == it and Q.strides[1] >= n * it and Q.strides[1] % it == 0):
            Q = f64(Q)
        ldq = Q.strides[1] // it if m > 1 or Q.strides[1] >= n * it else n
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if a.shape[0] != m:
            raise ValueError("a needs one entry per column of Q")
        Wm = _obs_arrays(n, W, None)[0]
        nw = Wm.shape[1]
        out, sums, n2 = np.zeros(n), np.zeros(max(nw, 1)), ctypes.c_double()
        check(self.h, lib.cal_prop_combine_real_ld(self.h, n, m, ptr(Q), ldq, ptr(a), nw, ptr(Wm) if nw else None,
                                                   ptr(out), ctypes.cast(ctypes.byref(n2), dp), ptr(sums)),
              "prop_combine_real")
        return out, n2.value, sums[:nw].copy()

    def set_diagonal(self, d):
        """Rewrite the stored diagonal of the resident matrix in place
        (cal_set_diagonal): one entry per row, no new upload or analysis.
        Needs a "csr" or "split" matrix with exactly one stored diagonal
        entry in every row; refused (CalError, nothing written) otherwise,
        while a Lanczos run or a propagator is open, and on a context handed
        out by ``context_for(A)`` -- that cache pairs the device copy with
        the SciPy object, so ``set_diagonal`` wants an explicit ``Context``."""
        if getattr(self, "_cached_for_matrix", False):
            raise CalError(_lib.CAL_ERR_ARG, "set_diagonal: this context is the cached device copy of a SciPy matrix "
                                             "(context_for); set_diagonal wants an explicit Context")
        d = np.ascontiguousarray(d, dtype=np.float64).ravel()
        check(self.h, lib.cal_set_diagonal(self.h, d.shape[0], ptr(d)), "set_diagonal")
        return self

    def get_diagonal(self):
        """The stored diagonal of the resident matrix (cal_get_diagonal;
        the 2n entries of blkdiag(H, H) while a propagator is open)."""
        n = self.matrix_info()["n_local"]
        d = np.zeros(n)
        check(self.h, lib.cal_get_diagonal(self.h, n, ptr(d)), "get_diagonal")
        return d

    def set_matrix_csc(self, A):
        """MATLAB's sparse storage (mxGetJc / mxGetIr / mxGetPr: CSC with int64
        mwIndex arrays) through cal_set_matrix_csc, the entry a MEX shim uses."""
        A = sp.csc_matrix(A)
        A.sort_indices()
        jc = np.ascontiguousarray(A.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(A.indices, dtype=np.int64)
        pr = np.ascontiguousarray(A.data, dtype=np.float64)
        check(self.h, lib.cal_set_matrix_csc(self.h, A.shape[0], jc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                             ir.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ptr(pr)),
              "set_matrix_csc")
        self.n = A.shape[0]
        return self

    def set_matrix_slab(self, n_global, row0, A_rows):
        """Distributed: rows [row0, row0+nlocal) of A (global column ids)."""
        A_rows = sp.csr_matrix(A_rows)
        A_rows.sort_indices()
        rowptr = np.ascontiguousarray(A_rows.indptr, dtype=np.int64)
        col = np.ascontiguousarray(A_rows.indices, dtype=np.int64)
        val = np.ascontiguousarray(A_rows.data, dtype=np.float64)
        check(self.h, lib.cal_set_matrix_csr_dist(
            self.h, n_global, row0, A_rows.shape[0], rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            col.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ptr(val)), "set_matrix_slab")
        self.n = A_rows.shape[0]
        return self

    def matrix_info(self):
        v = [ctypes.c_int64() for _ in range(4)]
        check(self.h, lib.cal_matrix_info(self.h, *[ctypes.byref(x) for x in v]))
        return dict(n_local=v[0].value, nnz_local=v[1].value, n_global=v[2].value, nghost=v[3].value)

    # -- timers ---------------------------------------------------------------
    def timer_enable(self, on=True):
        check(self.h, lib.cal_timer_enable(self.h, 1 if on else 0))

    def timer_reset(self):
        check(self.h, lib.cal_timer_reset(self.h))

    def comm_stats(self, reset=False):
        """Communicator counters (cal_comm_stats): ranks, kind, RCCL comm
        count, all-reduces and their doubles, halo exchanges and their
        doubles, SpMV rows computed."""
        v = (ctypes.c_int64 * 8)()
        check(self.h, lib.cal_comm_stats(self.h, v, 8, 1 if reset else 0))
        keys = ("nranks", "kind", "rccl_count", "allreduce_calls", "allreduce_doubles", "halo_calls",
                "halo_doubles", "spmv_rows")
        return dict(zip(keys, [int(x) for x in v]))

    def timer_bytes(self, kind="spmv"):
        """Algorithmic HBM bytes of the timed launches of `kind`."""
        b = ctypes.c_double()
        check(self.h, lib.cal_timer_bytes(self.h, kind.encode(), ctypes.byref(b)))
        return b.value

    def timer_read(self, kind="spmv"):
        cnt = ctypes.c_int64()
        tot = ctypes.c_double()
        check(self.h, lib.cal_timer_read(self.h, kind.encode(), ctypes.byref(cnt), ctypes.byref(tot)))
        return cnt.value, tot.value

    def synchronize(self):
        check(self.h, lib.cal_synchronize(self.h))

    # -- communicators ----------------------------------------------------------
    def comm_init_rccl(self, nranks, rank, uid: bytes):
        buf = ctypes.create_string_buffer(uid, 128)
        check(self.h, lib.cal_comm_init_rccl(self.h, nranks, rank, buf), "comm_init_rccl")

    def comm_init_host(self, nranks, rank, allreduce, exchange):
        """allreduce(np.ndarray) sums in place; exchange(peer, send, recv) fills recv."""
        def _ar(user, buf, count):
            try:
                a = np.ctypeslib.as_array(buf, shape=(count,))
                allreduce(a)
                return 0
            except Exception:  # pragma: no cover - reported as CAL_ERR_COMM
                return -1

        def _ex(user, peer, send, ns, recv, nr):
            try:
                s = np.ctypeslib.as_array(send, shape=(ns,)) if ns > 0 else np.zeros(0)
                r = np.ctypeslib.as_array(recv, shape=(nr,)) if nr > 0 else np.zeros(0)
                exchange(peer, s, r)
                return 0
            except Exception:  # pragma: no cover
                return -1

        cb = (_lib.ALLREDUCE_FN(_ar), _lib.EXCHANGE_FN(_ex))
        self._keep.append(cb)
        check(self.h, lib.cal_comm_init_host(self.h, nranks, rank, cb[0], cb[1], None), "comm_init_host")

    # -- step-wise CA-Lanczos ---------------------------------------------------
    def lanczos_begin(self, r, s, max_outer, basis="newton", orth="local"):
        r = f64(r)
        check(self.h, lib.cal_lanczos_begin(self.h, ptr(r), s, max_outer, basis.encode(), orth.encode()),
              "lanczos_begin")
        self._lz = dict(s=s, max_outer=max_outer)

    def lanczos_step(self, diagnostics=False):
        return check(self.h, lib.cal_lanczos_step(self.h, 1 if diagnostics else 0), "lanczos_step")

    def lanczos_state(self):
        k, s, re = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(self.h, lib.cal_lanczos_state(self.h, ctypes.byref(k), ctypes.byref(s), ctypes.byref(re)))
        return k.value, s.value, re.value

    def lanczos_get(self):
        k, s, _ = self.lanczos_state()
        sk = s * k
        T = np.zeros((sk, sk), order="F")
        rn = np.zeros((k, sk), order="F")
        oe = np.zeros(k)
        fl = np.zeros(k, dtype=np.int32)
        info = _lib.LanczosInfo()
        check(self.h, lib.cal_lanczos_get(self.h, ptr(T), max(sk, 1), ptr(rn), ptr(oe), iptr(fl),
                                          ctypes.byref(info)))
        return T, rn, oe, fl, info

    def lanczos_get_Q(self, col0, ncols):
        Q = np.zeros((self.n, ncols), order="F")
        check(self.h, lib.cal_lanczos_get_Q(self.h, col0, ncols, ptr(Q)))
        return Q

    def lanczos_end(self):
        check(self.h, lib.cal_lanczos_end(self.h))

    # -- step-wise standard Lanczos (lanczos.m) -----------------------------------
    def std_lanczos_begin(self, r, maxiter, orth="local", keep_Q=True):
        r = f64(r).ravel()
        check(self.h, lib.cal_std_lanczos_begin(self.h, ptr(r), int(maxiter), _std_orth(orth).encode(),
                                                1 if keep_Q else 0), "std_lanczos_begin")
        self._slz = int(maxiter)

    def std_lanczos_step(self, nsteps=1, diagnostics=False):
        """Enqueue nsteps more steps; returns the status (CAL_WARN_BREAKDOWN = 2 once a beta_j broke down)."""
        return check(self.h, lib.cal_std_lanczos_step(self.h, int(nsteps), 1 if diagnostics else 0), "std_lanczos_step")

    def std_lanczos_get(self):
        """(alpha, beta, ritz_rnorm, orth_err, info dict) of the steps kept so far."""
        m = self._slz
        al, be, oe = np.zeros(m), np.zeros(m), np.zeros(m)
        rn = np.zeros((m, m), order="F")
        info = _lib.StdLanczosInfo()
        st = check(self.h, lib.cal_std_lanczos_get(self.h, ptr(al), ptr(be), ptr(rn), ptr(oe), ctypes.byref(info)),
                   "std_lanczos_get")
        k = info.steps
        return al[:k].copy(), be[:k].copy(), np.array(rn[:k, :k]), oe[:k].copy(), _std_info(info, st)

    def std_lanczos_get_Q(self, col0, ncols):
        Q = np.zeros((self.n, ncols), order="F")
        check(self.h, lib.cal_std_lanczos_get_Q(self.h, col0, ncols, ptr(Q)), "std_lanczos_get_Q")
        return Q

    def std_lanczos_end(self):
        check(self.h, lib.cal_std_lanczos_end(self.h))

    def spmv_lanczos(self, x, xprev=None, beta2=0.0):
        """The fused Lanczos SpMV on host data: (y, dot) with y = A x - sqrt(beta2) xprev, dot = y'x."""
        x = f64(x).ravel()
        xp = None if xprev is None else f64(xprev).ravel()
        y = np.zeros(self.n)
        dot = np.zeros(1)
        check(self.h, lib.cal_spmv_lanczos(self.h, ptr(x), ptr(xp), float(beta2), ptr(y), ptr(dot)), "spmv_lanczos")
        return y, float(dot[0])

    def spmv_lanczos_fused(self):
        """Whether the context's matrix takes the fused Lanczos SpMV mode."""
        f = ctypes.c_int()
        check(self.h, lib.cal_spmv_lanczos_fused(self.h, ctypes.byref(f)), "spmv_lanczos_fused")
        return bool(f.value)


def split_analyze(A):
    """Whether A qualifies for the diagonal-split SpMV format (a uniform 5- or
    7-point stencil plus a per-row diagonal, ``grid_hamiltonian``): ``(P, H,
    neg1)`` (plane stride, in-plane reach, every off-diagonal is -1) or
    ``None``.  Host only (cal_split_analyze: the upload's own analysis)."""
    A = to_csr(A)
    if A.shape[0] != A.shape[1]:
        raise ValueError("A must be square")
    rowptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
    col = np.ascontiguousarray(A.indices, dtype=np.int32)
    val = np.ascontiguousarray(A.data, dtype=np.float64)
    P, H, ng = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    ok = lib.cal_split_analyze(A.shape[0], rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                               col.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ptr(val), ctypes.byref(P),
                               ctypes.byref(H), ctypes.byref(ng))
    return (P.value, H.value, bool(ng.value)) if ok else None


def _std_orth(orth):
    """lanczos.m:20-32: the option check (a numeric orth is num2str'ed there)."""
    o = orth.lower() if isinstance(orth, str) else str(orth)
    if o not in ("local", "full", "selective", "periodic"):
        raise ValueError("lanczos.m: Invalid option value for orth: %s" % orth)
    return o


def _std_info(info, status):
    return dict(steps=info.steps, breakdown=info.breakdown, fused=info.fused, n_orth_breaks=info.n_orth_breaks,
                n_ritz_locked=info.n_ritz_locked, norm_A=info.norm_A, loop_ms=info.loop_ms, diag_ms=info.diag_ms,
                status=status)


# ---------------------------------------------------------------------------
# context cache: one resident copy per matrix object (MATLAB passes A by value
# on every call; the device copy is the "persistent state" of SURVEY §8b)
# ---------------------------------------------------------------------------
_default_ctx: Context | None = None
_matrix_ctx: dict = {}


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def _evict(key, ref) -> None:
    """Close the context of a matrix that died (its weakref's callback):
    the device copy of A and the work buffers go with it."""
    hit = _matrix_ctx.get(key)
    if hit is not None and hit[0] is ref:
        del _matrix_ctx[key]
        hit[1].close()


def context_for(A) -> Context:
    key = id(A)
    hit = _matrix_ctx.get(key)
    if hit is not None and hit[0]() is A:
        return hit[1]
    if hit is not None:  # a dead matrix's id, reused before its callback ran
        _evict(key, hit[0])
    ctx = Context().set_matrix(A)
    ctx._cached_for_matrix = True  # Context.set_diagonal refuses: the cache pairs the device copy with A
    try:
        ref = weakref.ref(A, lambda r, key=key: _evict(key, r))
    except TypeError:  # pragma: no cover  (not weak-referenceable: kept for the process)
        ref = lambda: A  # noqa: E731
    _matrix_ctx[key] = (ref, ctx)
    return ctx


# ---------------------------------------------------------------------------
# a1-a4
# ---------------------------------------------------------------------------
def SpMV(A, v):
    """``Av = SpMV(A,v)`` -- SpMV.m:6-8."""
    ctx = context_for(A)
    v = f64(v).ravel()
    out = np.empty_like(v)
    check(ctx.h, lib.cal_spmv(ctx.h, ptr(v), ptr(out)), "SpMV")
    return out


def matrix_powers_monomial(A, q, s, ctx=None):
    """``V = matrix_powers_monomial(A,q,s)`` (n x s) -- matrix_powers_monomial.m:6-12."""
    ctx = ctx or context_for(A)
    q = f64(q).ravel()
    V = np.zeros((len(q), s), order="F")
    check(ctx.h, lib.cal_matrix_powers_monomial(ctx.h, ptr(q), s, ptr(V)), "matrix_powers_monomial")
    return V


def matrix_powers_newton(A, v, s, lam, modifiedp=0, ctx=None):
    """``V = matrix_powers_newton(A,v,s,lambda,modifiedp)`` (n x (s+1)) -- matrix_powers_newton.m:15-54."""
    ctx = ctx or context_for(A)
    v = f64(v).ravel()
    lam = np.asarray(lam)
    lre = f64(np.real(lam)).ravel()
    lim = f64(np.imag(lam)).ravel() if np.iscomplexobj(lam) else None
    V = np.zeros((len(v), s + 1), order="F")
    check(ctx.h, lib.cal_matrix_powers_newton(ctx.h, ptr(v), s, ptr(lre), ptr(lim), int(modifiedp), ptr(V)),
          "matrix_powers_newton")
    return V


# ---------------------------------------------------------------------------
# a5-a9
# ---------------------------------------------------------------------------
def tsqr(A):
    """``[Q,R] = tsqr(A)`` -- tsqr.m:7-12 (R upper, diag(R) >= 0)."""
    ctx = default_context()
    A = f64(A)
    n, m = A.shape
    Q = np.zeros((n, m), order="F")
    R = np.zeros((m, m), order="F")
    check(ctx.h, lib.cal_tsqr(ctx.h, n, m, ptr(A), ptr(Q), ptr(R)), "tsqr")
    return Q, R


def cholqr(X):
    """``[Q,R] = cholqr(X)`` -- cholqr.m:3-8 (one Cholesky-QR pass)."""
    ctx = default_context()
    X = f64(X)
    n, m = X.shape
    Q = np.zeros((n, m), order="F")
    R = np.zeros((m, m), order="F")
    check(ctx.h, lib.cal_cholqr(ctx.h, n, m, ptr(X), ptr(Q), ptr(R)), "cholqr")
    return Q, R


def _blocks(Q):
    if not isinstance(Q, (list, tuple)):
        raise TypeError("Input Q (arg 1) to project() must be cell (block) array.")
    blocks = [f64(b) if (b is not None and np.size(b) > 0) else None for b in Q]
    widths = np.array([0 if b is None else b.shape[1] for b in blocks], dtype=np.int32)
    arr = (dp * max(len(blocks), 1))(*[ptr(b) if b is not None else None for b in blocks])
    return blocks, widths, arr


def project(Q, X, doreorth=False, ctx=None):
    """``[X,R] = project(Q,X,doreorth)`` -- project.m:7-58."""
    if isinstance(X, (list, tuple)):
        raise TypeError("Input X (arg 2) project() must be a column matrix.")
    if len(Q) == 0:
        return np.array(X, dtype=np.float64), []
    ctx = ctx or default_context()
    X = f64(X)
    n, m = X.shape
    blocks, widths, arr = _blocks(Q)
    R = [np.zeros((int(w), m), order="F") for w in widths]
    Rarr = (dp * len(R))(*[ptr(r) for r in R])
    Xout = np.zeros((n, m), order="F")
    check(ctx.h, lib.cal_project(ctx.h, n, len(blocks), arr, iptr(widths), m, ptr(X), 1 if doreorth else 0,
                                 ptr(Xout), Rarr), "project")
    return Xout, R


def normalize(X, opt="None", tol=1.0e-8, ctx=None):
    """``[Q,R,rank] = normalize(X,opt,tol)`` -- normalize.m:3-36; opt
    'randomizeNullSpace' runs normalize.m:28-31,38-51 (the null-space
    columns drawn from a fresh MATLAB rand stream, seed 5489)."""
    ctx = ctx or default_context()
    X = f64(X)
    n, m = X.shape
    Q = np.zeros((n, m), order="F")
    R = np.zeros((m, m), order="F")
    rank = ctypes.c_int()
    check(ctx.h, lib.cal_normalize_opt(ctx.h, n, m, ptr(X), str(opt).encode(), tol, ptr(Q), ptr(R),
                                       ctypes.byref(rank)), "normalize")
    return Q, R, rank.value


def matlab_rand(count, seed=5489):
    """MATLAB ``rand`` of a fresh session (rng(seed,'twister')): cal_matlab_rand."""
    out = np.zeros(int(count))
    check(None, lib.cal_matlab_rand(int(count), int(seed), ptr(out)), "matlab_rand")
    return out


def projectAndNormalize_ex(Q, X, doreorth=True, ctx=None):
    """projectAndNormalize.m:3-90, also returning (reorth flag, rank).  With
    a distributed context, Q / X are this rank's local rows."""
    ctx = ctx or default_context()
    X = f64(X)
    n, m = X.shape
    blocks, widths, arr = _blocks(Q)
    RZ = [np.zeros((int(w), m), order="F") for w in widths] + [np.zeros((m, m), order="F")]
    RZarr = (dp * len(RZ))(*[ptr(r) for r in RZ])
    QZ = np.zeros((n, m), order="F")
    re, rk = ctypes.c_int(), ctypes.c_int()
    check(ctx.h, lib.cal_project_and_normalize(ctx.h, n, len(blocks), arr, iptr(widths), m, ptr(X),
                                               1 if doreorth else 0, ptr(QZ), RZarr, ctypes.byref(re),
                                               ctypes.byref(rk)), "projectAndNormalize")
    return QZ, RZ, bool(re.value), rk.value


def projectAndNormalize(Q, X, doreorth=True):
    """``[QZ,RZ] = projectAndNormalize(Q,X,doreorth)`` -- projectAndNormalize.m:3-90."""
    QZ, RZ, _, _ = projectAndNormalize_ex(Q, X, doreorth)
    return QZ, RZ


# ---------------------------------------------------------------------------
# a13 host routines
# ---------------------------------------------------------------------------
def leja(x, which=None):
    """``[y,idx] = leja(x,'nonmodified')`` -> real_leja -> modified_leja (leja.m:23-31)."""
    if which is None:
        raise NotImplementedError("nonmodified_leja is not on the ca_lanczos path")
    x = np.asarray(x).ravel()
    n = len(x)
    xr = f64(np.real(x))
    xi = f64(np.imag(x)) if np.iscomplexobj(x) else None
    yr, yi = np.zeros(n), np.zeros(n)
    idx = np.zeros(n, dtype=np.int32)
    st = lib.cal_leja(n, ptr(xr), ptr(xi), ptr(yr), ptr(yi), iptr(idx))
    if st != 0:
        raise CalError(st, "leja: modified Leja ordering failed")
    y = yr + 1j * yi if np.any(yi != 0) else yr
    return y, idx.astype(np.int64)


def newton_basis_matrix(lam, s, modifiedp=0):
    """``B_ = newton_basis_matrix(lambda,s,modifiedp)`` -- newton_basis_matrix.m:13-60."""
    lam = np.asarray(lam)
    lr = f64(np.real(lam)).ravel()
    li = f64(np.imag(lam)).ravel() if np.iscomplexobj(lam) else None
    B = np.zeros((s + 1, s), order="F")
    st = lib.cal_newton_basis_matrix(s, ptr(lr), ptr(li), int(modifiedp), ptr(B))
    if st != 0:
        raise CalError(st, "newton_basis_matrix failed")
    return B


def eig(T):
    """``[V,D] = eig(T)`` as used by ca_lanczos.m:229 -> (w complex/real, V)."""
    T = f64(T)
    n = T.shape[0]
    wr, wi = np.zeros(n), np.zeros(n)
    V = np.zeros((n, n), order="F")
    st = lib.cal_eig(n, ptr(T), n, ptr(wr), ptr(wi), ptr(V))
    if st != 0:
        raise CalError(st, "eig did not converge")
    if np.any(wi != 0):
        Vc = V.astype(complex)
        j = 0
        while j < n:
            if wi[j] > 0:
                Vc[:, j] = V[:, j] + 1j * V[:, j + 1]
                Vc[:, j + 1] = V[:, j] - 1j * V[:, j + 1]
                j += 2
            else:
                j += 1
        return wr + 1j * wi, Vc
    return wr, V


# ---------------------------------------------------------------------------
# a14: the driver
# ---------------------------------------------------------------------------
def compute_ritz_rnorm(A, Q, Vp, Dp, ctx=None):
    """``ritz_rnorm = compute_ritz_rnorm(A,Q,Vp,Dp)`` -- ca_lanczos.m:88-97 (real
    Dp: a vector of eigenvalues or the diagonal matrix).  The Ritz vectors
    x = Q*Vp(:,i) are formed on the device; the values are sorted descending
    as the reference does."""
    ctx = ctx or context_for(A)
    Q = np.asfortranarray(f64(Q))
    Vp = np.asfortranarray(f64(Vp))
    d = f64(np.diag(Dp) if np.ndim(Dp) == 2 else Dp).ravel().copy()
    k = Vp.shape[1]
    if Q.shape[1] != k or Vp.shape[0] != k or d.size != k:
        raise ValueError("compute_ritz_rnorm: Q is n x k, Vp k x k, Dp k values")
    rn = np.zeros(k)
    check(ctx.h, lib.cal_compute_ritz_rnorm(ctx.h, ptr(Q), k, ptr(Vp), ptr(d), ptr(rn)), "compute_ritz_rnorm")
    return rn


@dataclass
class CALanczosOutput:
    T: np.ndarray
    Q: np.ndarray | None
    ritz_rnorm: np.ndarray
    orth_err: np.ndarray
    reorth: np.ndarray
    shifts: np.ndarray
    info: dict = field(default_factory=dict)


def ca_lanczos_ex(A, r, s, iter, basis, orth="local", diagnostics=True, return_Q=True, ctx=None):
    """ca_lanczos.m:24-86 with the extra outputs (flags, shifts, timings)."""
    o = orth.lower() if isinstance(orth, str) else str(orth)
    if o not in ("local", "full", "selective", "periodic"):
        raise ValueError("ca_lanczos.m: Invalid option value for orth: %s" % orth)
    ctx = ctx or context_for(A)
    r = f64(r).ravel()
    t = int(math.ceil(iter / s))
    n = len(r)
    T = np.zeros((s * t, s * t), order="F")
    Q = np.zeros((n, s * t), order="F") if return_Q else None
    rn = np.zeros((t, s * t), order="F")
    oe = np.zeros(t)
    fl = np.zeros(t, dtype=np.int32)
    info = _lib.LanczosInfo()
    st = lib.cal_ca_lanczos(ctx.h, ptr(r), s, iter, basis.encode(), orth.encode(), 1 if diagnostics else 0,
                            ptr(T), ptr(Q), ptr(rn), ptr(oe), iptr(fl), ctypes.byref(info))
    check(ctx.h, st, "ca_lanczos")
    k = info.t
    sk = s * k
    shifts = np.array(info.shifts[: 2 * s]) if basis.lower() == "newton" else np.zeros(0)
    if np.any(np.array(info.shifts_im[: 2 * s]) != 0):
        shifts = shifts + 1j * np.array(info.shifts_im[: 2 * s])
    return CALanczosOutput(
        T=np.array(T[:sk, :sk]), Q=None if Q is None else np.array(Q[:, :sk]),
        ritz_rnorm=np.array(rn[:k, :sk]), orth_err=oe[:k].copy(), reorth=fl[:k].copy(), shifts=shifts,
        info=dict(t=k, n_reorth=info.n_reorth, n_rank_deficient=info.n_rank_deficient,
                  breakdown=info.breakdown, prologue_ms=info.prologue_ms, loop_ms=info.loop_ms,
                  diag_ms=info.diag_ms, status=st, n_orth_breaks=info.n_orth_breaks,
                  n_ritz_locked=info.n_ritz_locked, norm_A=info.norm_A,
                  n_ritz_complex=info.n_ritz_complex))


def ca_lanczos(A, r, s, iter, basis, orth="local"):
    """``[T,Q,ritz_rnorm,orth_err] = ca_lanczos(A,r,s,iter,basis,orth)`` -- ca_lanczos.m:24-86."""
    out = ca_lanczos_ex(A, r, s, iter, basis, orth, diagnostics=True, return_Q=True)
    return out.T, out.Q, out.ritz_rnorm, out.orth_err


# ---------------------------------------------------------------------------
# standard Lanczos (lanczos.m), the other half of the reference's comparisons
# ---------------------------------------------------------------------------
@dataclass
class LanczosOutput:
    T: np.ndarray
    Q: np.ndarray | None
    alpha: np.ndarray
    beta: np.ndarray
    ritz_rnorm: np.ndarray
    orth_err: np.ndarray
    info: dict = field(default_factory=dict)


def lanczos_ex(A, r, maxiter, orth="local", diagnostics=False, return_Q=True, ctx=None):
    """lanczos.m:18-60 with alpha, beta and the counters.  return_Q = False
    with orth 'local' and no diagnostics keeps three columns on the device."""
    o = _std_orth(orth)
    ctx = ctx or context_for(A)
    keep = bool(return_Q or diagnostics or o != "local")
    ctx.std_lanczos_begin(r, maxiter, o, keep_Q=keep)
    try:
        ctx.std_lanczos_step(int(maxiter), diagnostics)
        al, be, rn, oe, info = ctx.std_lanczos_get()
        k = info["steps"]
        Q = ctx.std_lanczos_get_Q(0, k) if return_Q else None
    finally:
        ctx.std_lanczos_end()
    T = np.diag(al) + np.diag(be[: max(k - 1, 0)], 1) + np.diag(be[: max(k - 1, 0)], -1)  # lanczos.m:131
    return LanczosOutput(T=T, Q=Q, alpha=al, beta=be, ritz_rnorm=rn, orth_err=oe, info=info)


def lanczos(A, r, maxiter, orth="local"):
    """``[T,Q,ritz_rnorm,orth_err] = lanczos(A,r,maxiter,orth)`` -- lanczos.m:18-60."""
    out = lanczos_ex(A, r, maxiter, orth, diagnostics=True, return_Q=True)
    return out.T, out.Q, out.ritz_rnorm, out.orth_err


# ---------------------------------------------------------------------------
# f2: explicit restart
# ---------------------------------------------------------------------------
MAX_RESTARTS = 200  # restarted_ca_lanczos.m:6


def restarted_ca_lanczos(A, r, max_lanczos, n_wanted_eigs=10, s=6, basis="newton", orth="local", tol=1.0e-8,
                         diagnostics=True, ctx=None):
    """``[E,V,nres,rnorms,orth_err] = restarted_ca_lanczos(A,r,max_lanczos,
    n_wanted_eigs,s,basis,orth,tol)`` -- restarted_ca_lanczos.m:4-198.

    Returns a dict: conv_eigs (descending), Q_conv (n x nconv), num_restarts,
    rnorms (num_restarts x n_wanted_eigs), orth_err (num_restarts),
    converged, norm_A."""
    ctx = ctx or context_for(A)
    r = f64(r).ravel()
    n = len(r)
    E = np.zeros(n_wanted_eigs)
    V = np.zeros((n, n_wanted_eigs), order="F")
    rn = np.zeros((MAX_RESTARTS, n_wanted_eigs), order="F")
    oe = np.zeros(MAX_RESTARTS)
    info = _lib.RestartInfo()
    st = lib.cal_restarted_ca_lanczos(ctx.h, ptr(r), int(max_lanczos), int(n_wanted_eigs), int(s), basis.encode(),
                                      orth.encode(), float(tol), 1 if diagnostics else 0, ptr(E), ptr(V), ptr(rn),
                                      ptr(oe), ctypes.byref(info))
    check(ctx.h, st, "restarted_ca_lanczos")
    k, nr = info.nconv, info.num_restarts
    return dict(conv_eigs=E[:k].copy(), Q_conv=V[:, :k].copy(), num_restarts=nr, rnorms=rn[:nr].copy(),
                orth_err=oe[:nr].copy(), converged=bool(info.converged), norm_A=info.norm_A, ms=info.ms)


IMPL_MAX_RESTARTS = 40  # impl_restarted_ca_lanczos.m:7


def impl_restarted_ca_lanczos(A, r, max_lanczos, n_wanted_eigs=10, s=6, basis="newton", orth="full", tol=1.0e-6,
                              ctx=None, return_Q=True):
    """``[conv_eigs,Q_conv,num_restarts] = impl_restarted_ca_lanczos(A,r,
    max_lanczos,n_wanted_eigs,s,basis,orth,tol)`` -- the implicit restart
    impl_restarted_ca_lanczos.m:4-226 sets out to implement (the file itself
    does not run).  Only orth 'full' is defined.

    Returns a dict: conv_eigs (n_wanted_eigs, descending), Q_conv
    (n x n_wanted_eigs; None with return_Q=False: the Ritz vectors are formed
    on the device but not copied to the host), num_restarts, converged,
    ritz_est (num_restarts x n_wanted_eigs), norm_A."""
    ctx = ctx or context_for(A)
    r = f64(r).ravel()
    n = len(r)
    E = np.zeros(n_wanted_eigs)
    V = np.zeros((n, n_wanted_eigs), order="F") if return_Q else None
    est = np.zeros((IMPL_MAX_RESTARTS, n_wanted_eigs), order="F")
    info = _lib.RestartInfo()
    st = lib.cal_impl_restarted_ca_lanczos(ctx.h, ptr(r), int(max_lanczos), int(n_wanted_eigs), int(s),
                                           basis.encode(), orth.encode(), float(tol), ptr(E),
                                           ptr(V) if return_Q else None, ptr(est),
                                           ctypes.byref(info))
    check(ctx.h, st, "impl_restarted_ca_lanczos")
    k, nr = info.nconv, info.num_restarts
    return dict(conv_eigs=E[:k].copy(), Q_conv=V[:, :k].copy() if return_Q else None, num_restarts=nr,
                ritz_est=est[:nr].copy(),
                converged=bool(info.converged), norm_A=info.norm_A, ms=info.ms)


# ---------------------------------------------------------------------------
# Krylov time propagation psi(t+dt) = exp(-i dt H) psi(t)
# ---------------------------------------------------------------------------
def expm_col1(T, dt):
    """``expm(-1i*dt*T)(:,1)`` for a general real square T (cal_expm_col1:
    host only, ca_lanczos_prop.m:122)."""
    T = f64(T)
    m = T.shape[0]
    cre, cim = np.zeros(max(m, 1)), np.zeros(max(m, 1))
    st = lib.cal_expm_col1(m, ptr(T), max(m, 1), float(dt), ptr(cre), ptr(cim))
    if st != 0:
        raise CalError(st, "cal_expm_col1")
    return cre[:m] + 1j * cim[:m]


def expm_real_col1(T, tau):
    """``expm(-tau*(T - T(1,1)*I))(:,1)`` for a general real square T
    (cal_expm_real_col1: host only; the coefficients of an imaginary-time
    step, which uses their direction only)."""
    T = f64(T)
    m = T.shape[0]
    c = np.zeros(max(m, 1))
    st = lib.cal_expm_real_col1(m, ptr(T), max(m, 1), float(tau), ptr(c))
    if st != 0:
        raise CalError(st, "cal_expm_real_col1")
    return c[:m]


def _split(psi):
    psi = np.asarray(psi)
    re = np.ascontiguousarray(psi.real, dtype=np.float64).ravel()
    im = np.ascontiguousarray(psi.imag, dtype=np.float64).ravel() if np.iscomplexobj(psi) else None
    return re, im


def _eigest(eigest):
    if eigest is None or len(eigest) == 0:
        return None, 0
    e = np.ascontiguousarray(np.real(np.asarray(eigest)), dtype=np.float64).ravel()
    return e, len(e)


def _obs_arrays(n, W, phi):
    """(W n x nw, Re phi n x nphi, Im phi n x nphi), column-major float64, from lists or 2-D arrays."""
    def cols(a, dtype):
        if a is None or len(a) == 0:
            return np.zeros((n, 0), dtype=dtype)
        a = np.asarray(a, dtype=dtype) if not isinstance(a, (list, tuple)) else np.column_stack(
            [np.asarray(x, dtype=dtype).ravel() for x in a])
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim != 2 or a.shape[0] != n:
            raise ValueError("observables need n rows (one column per operator or reference state)")
        return a
    Wm = f64(cols(W, np.float64))
    p = cols(phi, np.complex128)
    return Wm, f64(p.real), f64(p.imag)


def drive_rows(drive, t0, dt, nsteps, scheme="midpoint"):
    """The amplitude rows ``Propagator.step`` hands to cal_prop_step_driven
    and the size of the (sub-)step each row is taken with: (rows (nrows x nk,
    C order), sub).  An array drive is taken as it is (nsteps rows, sub = dt);
    a callable is sampled by the scheme (see ``Propagator.step``)."""
    if not callable(drive):
        rows = np.ascontiguousarray(np.asarray(drive, dtype=np.float64))
        if rows.ndim == 1:
            rows = rows.reshape(nsteps, -1)
        if rows.ndim != 2 or rows.shape[0] != nsteps:
            raise ValueError("drive needs one row of amplitudes per step")
        return rows, dt

    def f(t):
        return np.atleast_1d(np.asarray(drive(t), dtype=np.float64)).ravel()
    if scheme == "midpoint":
        rows = [f(t0 + j * dt + 0.5 * dt) for j in range(nsteps)]
        sub = dt
    elif scheme == "cf4":
        r3 = math.sqrt(3.0)
        a1, a2 = 0.5 + r3 / 3.0, 0.5 - r3 / 3.0
        rows = []
        for j in range(nsteps):
            f1 = f(t0 + j * dt + (0.5 - r3 / 6.0) * dt)
            f2 = f(t0 + j * dt + (0.5 + r3 / 6.0) * dt)
            rows.append(a1 * f1 + a2 * f2)  # the right factor acts first
            rows.append(a2 * f1 + a1 * f2)
        sub = 0.5 * dt
    else:
        raise ValueError("scheme must be \"midpoint\" or \"cf4\"")
    nk = len(rows[0]) if rows else 0
    return np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(len(rows), nk)), sub


class Propagator:
    """Time stepper ``psi <- exp(-i dt H) psi`` for a real symmetric or complex
    Hermitian sparse H and a complex state (cal_prop_*; ca_lanczos_prop.m as
    runLanczos.m:84-131 drives it).  A real H is embedded as blkdiag(H, H)
    (``set_matrix_stacked``), a complex-dtype H = A + iB as [[A, -B], [B, A]]
    (``set_matrix_hermitian``: magnetic fields, velocity gauge, rotating
    frames); the state lives on the device as [Re psi; Im psi].  Observables,
    energy, absorber, drive and the nonlinear term touch only the real
    diagonal and work on either.  ``state()`` is the only copy back of the
    state, ``set_observables`` / ``observables`` watch it from the device.

    ``set_imaginary_time`` turns the stepper into ``psi <- sqrt(N) exp(-tau
    H[psi]) psi / ||.||`` (ground states; ``ground_state`` drives it), and
    ``energetics`` gives mu, the Gross-Pitaevskii energy and the
    eigen-residual of every step's start state in either mode.
    ``real=True`` (a real H and a real psi0) is the real-state path
    (cal_prop_begin_real): imaginary time only, on the n x n H itself through
    ``Context.set_matrix`` in any SpMV format, the state a real vector of n
    rows -- half the bytes of every SpMV and sweep.  It takes the drive, the
    nonlinear term, W observables and the energy; reference states, an
    absorber and real time are refused and need the stacked propagator."""

    def __init__(self, H, psi0, s, max_blocks, basis="newton", eigest=None, ctx=None, real=False):
        self.n = H.shape[0]
        self.real = bool(real)
        if self.real and (np.iscomplexobj(H) or np.iscomplexobj(psi0)):
            raise ValueError("real=True needs a real H and a real psi0 (the stacked propagator takes complex ones)")
        self._nw = 0
        self._nk = 0
        self.t = 0.0  # the propagator's clock: the sum of the (sub-)steps taken through step()
        self._own = ctx is None
        self.ctx = ctx or Context()
        try:
            if self.real:
                self.ctx.set_matrix(H)
            elif np.iscomplexobj(H):
                self.ctx.set_matrix_hermitian(H)
            else:
                self.ctx.set_matrix_stacked(H)
            re, im = _split(psi0)
            if re.shape[0] != self.n:
                raise ValueError("psi0 must have H.shape[0] entries")
            e, ne = _eigest(eigest)
            if self.real:
                check(self.ctx.h, lib.cal_prop_begin_real(self.ctx.h, self.n, ptr(re), s, max_blocks, basis.encode(),
                                                          ptr(e), ne), "prop_begin_real")
            else:
                check(self.ctx.h, lib.cal_prop_begin(self.ctx.h, self.n, ptr(re), ptr(im), s, max_blocks,
                                                     basis.encode(), ptr(e), ne), "prop_begin")
        except Exception:
            if self._own:
                self.ctx.close()
            raise
        self._open = True

    def step(self, dt, nsteps=1, tol=1.0e-10, adaptive=False, drive=None, scheme="midpoint"):
        """nsteps time steps of size dt; returns the status (0, or
        CAL_WARN_BREAKDOWN when a step's first block broke down).

        ``drive`` (after ``set_drive``) steps under H(t) = H0 + sum_k f_k(t)
        diag(W_k).  An array (nsteps, nk) is used row by row, one row of
        amplitudes per step.  A callable ``t -> nk amplitudes`` is sampled by
        ``scheme``: "midpoint" takes ``drive(t_j + dt/2)`` for step j (the
        exponential midpoint rule, second order); "cf4" is the commutator-free
        fourth-order rule, two sub-steps of dt/2 per step,
        ``exp(-i dt/2 (a2 A1 + a1 A2)) exp(-i dt/2 (a1 A1 + a2 A2))`` (right
        factor first) with ``A_i = H(t_j + (1/2 -+ sqrt(3)/6) dt)`` and
        ``a_{1,2} = 1/2 +- sqrt(3)/3`` -- two rows of amplitudes (and two
        history rows of the observables) per step through the same call.
        ``self.t`` advances by the sub-steps' sum.  ``drive=None`` is the
        undriven call: it steps under whatever H the last driven step left.

        After ``set_nonlinear`` every (sub-)step is a nonlinear step.
        ``scheme`` keeps its meaning for the drive: under "cf4" each of the
        two sub-steps is a nonlinear step of its own, so the drive is treated
        to fourth order while the nonlinear part stays second order
        ("midpoint" density) or first ("frozen")."""
        if drive is None:
            st = check(self.ctx.h, lib.cal_prop_step(self.ctx.h, float(dt), float(tol), 1 if adaptive else 0,
                                                     int(nsteps)), "prop_step")
            self.t += float(dt) * int(nsteps)
            return st
        rows, sub = drive_rows(drive, self.t, float(dt), int(nsteps), scheme)
        if rows.shape[1] != self._nk:
            raise ValueError("drive has %d amplitudes per step, set_drive has %d operators" % (rows.shape[1], self._nk))
        st = check(self.ctx.h, lib.cal_prop_step_driven(self.ctx.h, sub, float(tol), 1 if adaptive else 0,
                                                        rows.shape[0], ptr(rows), max(rows.shape[1], 1)),
                   "prop_step_driven")
        self.t += sub * rows.shape[0]
        return st

    def set_drive(self, W):
        """The operators of the drive H(t) = H0 + sum_k f_k(t) diag(W_k): real
        diagonal operators W (a list or n x nk, at most 4), copied to the
        device; H0 is the matrix as it is now.  ``None`` switches the drive off
        and restores H0's diagonal, as ``close()`` does.  Needs a "csr" or
        "split" context (``Context.set_diagonal``'s conditions)."""
        if not getattr(self, "_open", False):
            raise CalError(_lib.CAL_ERR_ARG, "set_drive: the propagator is closed")
        Wm = _obs_arrays(self.n, W, None)[0]
        nk = Wm.shape[1]
        check(self.ctx.h, lib.cal_prop_set_drive(self.ctx.h, nk, ptr(Wm) if nk else None), "prop_set_drive")
        self._nk = nk
        return self

    def set_nonlinear(self, g, density="midpoint"):
        """The Gross-Pitaevskii term: from now on ``step`` propagates
        ``i d/dt psi = (H0 + drive + g |psi|^2) psi``.  The diagonal is formed
        from the state on the device before each Krylov build (one launch
        with the drive; no copy back).  ``density="frozen"`` uses
        ``|psi_n|^2`` for the whole step (first order, one build per step);
        ``"midpoint"`` predicts ``psi*`` with a frozen step and then steps
        from ``psi_n`` under ``g (|psi_n|^2 + |psi*|^2)/2`` (second order, two
        builds per step).  ``g = 0`` switches the term off; H0's diagonal goes
        back when neither the term nor a drive is set.  Clears ``nonlinear()``.
        The conserved Gross-Pitaevskii energy is a column of
        ``energetics()`` (the ``energy`` observable stays ``<psi|H|psi>``
        with the H stored in the matrix).  Not built: more than second order
        in the nonlinear part."""
        if not getattr(self, "_open", False):
            raise CalError(_lib.CAL_ERR_ARG, "set_nonlinear: the propagator is closed")
        check(self.ctx.h, lib.cal_prop_set_nonlinear(self.ctx.h, float(g), str(density).encode()),
              "prop_set_nonlinear")
        return self

    def _history(self, getter, name, first, count, ncols=None):
        """Rows [first, first + count) (count None: all from first) of one of
        the per-step histories: a first call for the row count (and, with
        ``ncols`` None, the column count the getter reports), a second for
        the rows."""
        nr, nc = ctypes.c_int64(), ctypes.c_int()
        tail = (ctypes.byref(nr),) if ncols is not None else (ctypes.byref(nr), ctypes.byref(nc))
        check(self.ctx.h, getter(self.ctx.h, 0, 0, None, *tail), name)
        count = nr.value - first if count is None else count
        rows = np.zeros((max(count, 0), nc.value if ncols is None else ncols))
        check(self.ctx.h, getter(self.ctx.h, int(first), int(count), ptr(rows), *tail), name)
        return rows

    def nonlinear(self, first=0, count=None):
        """One row ``[t_n, sum_i |psi_n,i|^4]`` per completed step since
        ``set_nonlinear`` (rows [first, first + count); default all), psi_n
        the state the step started from: ``g/2`` times the second column is
        the interaction energy.  Shape (rows, 2)."""
        return self._history(lib.cal_prop_get_nonlinear, "prop_get_nonlinear", first, count, 2)

    def set_imaginary_time(self, on=True):
        """From now on ``step`` takes ``dt`` as an imaginary-time step tau:
        ``psi <- sqrt(N) exp(-tau H[psi]) psi / ||.||`` with N the squared
        norm of the state at this call -- the iteration whose fixed point is
        the ground state (of the Gross-Pitaevskii functional under
        ``set_nonlinear``).  Everything else (drive, nonlinear densities,
        observables, absorber) keeps its meaning.  ``on=False`` returns to
        real time; a ``real=True`` propagator refuses that."""
        check(self.ctx.h, lib.cal_prop_set_imaginary_time(self.ctx.h, 1 if on else 0), "prop_set_imaginary_time")
        return self

    def energetics(self, first=0, count=None):
        """One entry per completed step since the propagator was opened (rows
        [first, first + count); default all), of the state psi_n the step
        started from: dict of ``t``, ``norm2`` (N_n), ``mu`` (the Rayleigh
        quotient ``<psi_n|H[psi_n]|psi_n>/N_n``, the chemical potential),
        ``energy`` (``N_n mu - (g/2) sum |psi_n|^4``, the Gross-Pitaevskii
        energy: conserved in real time) and ``residual``
        (``||H[psi_n] psi_n - mu psi_n|| / sqrt(N_n)``).  They are read off
        the first column of the step's Krylov matrix: no kernel, no sweep."""
        rows = self._history(lib.cal_prop_get_energetics, "prop_get_energetics", first, count, 5)
        return dict(t=rows[:, 0].copy(), norm2=rows[:, 1].copy(), mu=rows[:, 2].copy(), energy=rows[:, 3].copy(),
                    residual=rows[:, 4].copy())

    def refresh_shifts(self):
        """Forget the Newton shifts of the first step: the next step computes
        them from the current H and state (cal_prop_refresh_shifts; for a
        drive that moves H's spectrum by about its width or more)."""
        check(self.ctx.h, lib.cal_prop_refresh_shifts(self.ctx.h), "prop_refresh_shifts")
        return self

    def state(self):
        re, im = np.zeros(self.n), np.zeros(self.n)
        check(self.ctx.h, lib.cal_prop_get(self.ctx.h, ptr(re), ptr(im), None), "prop_get")
        return re + 1j * im

    def info(self):
        i = _lib.PropInfo()
        check(self.ctx.h, lib.cal_prop_get(self.ctx.h, None, None, ctypes.byref(i)), "prop_get")
        return dict(steps=i.steps, lsteps=i.lsteps, lsteps_max=i.lsteps_max, lsteps_sum=i.lsteps_sum,
                    residual=i.residual, residual_max=i.residual_max, norm=i.norm,
                    shifts=np.array(i.shifts[:i.nshifts]), breakdowns=i.breakdowns, rank_deficient=i.rank_deficient, ms=i.ms)

    def set_observables(self, W=None, phi=None, energy=False):
        """Record, after every later time step and without copying the state
        back: ``sum W_k |psi|^2`` for real diagonal operators W (a list or
        n x nw, at most 4), ``<phi_r|psi>`` for complex reference states phi
        (a list or n x nphi, at most 4) and, with ``energy``, ``<psi|H|psi>``
        (one more SpMV per step).  Replaces an earlier set and clears the
        history; no arguments switch the observables off."""
        if not getattr(self, "_open", False):
            raise CalError(_lib.CAL_ERR_ARG, "set_observables: the propagator is closed")
        Wm, pre, pim = _obs_arrays(self.n, W, phi)
        nw, nphi = Wm.shape[1], pre.shape[1]
        check(self.ctx.h, lib.cal_prop_set_observables(self.ctx.h, nw, ptr(Wm) if nw else None, nphi,
                                                       ptr(pre) if nphi else None, ptr(pim) if nphi else None,
                                                       1 if energy else 0), "prop_set_observables")
        self._nw = nw
        return self

    def observables(self, first=0, count=None):
        """The history since ``set_observables``, one entry per completed
        step (rows [first, first + count); default all): dict of ``t``,
        ``norm2``, ``energy`` (NaN when off), ``W`` (steps x nw) and
        ``overlap`` (steps x nphi, complex)."""
        rows = self._history(lib.cal_prop_get_observables, "prop_get_observables", first, count)
        nw = self._nw  # the W columns come first, then the (Re, Im) pairs
        ov = rows[:, 3 + nw:]
        return dict(t=rows[:, 0].copy(), norm2=rows[:, 1].copy(), energy=rows[:, 2].copy(),
                    W=rows[:, 3:3 + nw].copy(), overlap=ov[:, 0::2] + 1j * ov[:, 1::2])

    def set_absorber(self, mask):
        """An absorbing boundary: from now on every completed time step (each
        sub-step of ``scheme="cf4"`` too) ends with ``psi <- mask * psi``
        inside the combine sweep, mask real with n values in [0, 1]
        (``matrices.absorber_mask``), and the squared norm it removes,
        ``sum (1 - mask^2) |psi|^2``, is recorded (``absorbed``).  This is the
        first-order splitting of a complex absorbing potential
        ``-ln(mask)/dt``: a mask belongs to the dt it is stepped with.  The
        observables, the energy and ``info()["norm"]`` are those of the masked
        state.  Replaces an earlier mask and clears the absorbed history;
        ``None`` switches the absorber off."""
        if not getattr(self, "_open", False):
            raise CalError(_lib.CAL_ERR_ARG, "set_absorber: the propagator is closed")
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, dtype=np.float64).ravel()
            if mk.shape[0] != self.n:
                raise ValueError("the mask must have H.shape[0] entries")
        check(self.ctx.h, lib.cal_prop_set_absorber(self.ctx.h, ptr(mk)), "prop_set_absorber")
        return self

    def absorbed(self, first=0, count=None):
        """The squared norm the mask removed, one entry per completed step
        since ``set_absorber`` (rows [first, first + count); default all):
        dict of ``t`` and ``absorbed``."""
        rows = self._history(lib.cal_prop_get_absorbed, "prop_get_absorbed", first, count, 2)
        return dict(t=rows[:, 0].copy(), absorbed=rows[:, 1].copy())

    def close(self):
        if getattr(self, "_open", False):
            self._open = False
            if self.ctx.h:
                check(self.ctx.h, lib.cal_prop_end(self.ctx.h), "prop_end")
            if self._own:
                self.ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ground_state_loop(step, last, state, tol, max_steps):
    """The stopping rule of ``ground_state``: ``step()`` takes one
    imaginary-time step and returns its status, ``last()`` the energetics
    rows recorded so far as a dict, ``state()`` the current state.  A step's
    row describes the state it started from, so the loop stops when that
    row's ``residual <= tol * max(1, |mu|)`` -- the state returned is one
    step past the one judged, and no worse.  A CAL_WARN_BREAKDOWN whose last
    recorded row already meets the criterion counts as converged (an
    eigenvector to rounding has a one-dimensional Krylov space)."""
    def met(h):
        return len(h["mu"]) > 0 and h["residual"][-1] <= tol * max(1.0, abs(h["mu"][-1]))
    steps, converged = 0, False
    h = last()
    while steps < max_steps:
        st = step()
        h = last()
        if st == _lib.CAL_WARN_BREAKDOWN:
            converged = met(h)
            break
        steps += 1
        if met(h):
            converged = True
            break
    k = len(h["mu"]) - 1
    nan = float("nan")
    return dict(psi=state(), mu=h["mu"][k] if k >= 0 else nan, energy=h["energy"][k] if k >= 0 else nan,
                residual=h["residual"][k] if k >= 0 else nan, steps=steps, converged=converged, history=h)


def ground_state(H, psi0, tau, s, max_blocks, g=0.0, density="frozen", tol=1e-10, max_steps=1000, real=None,
                 basis="newton", ctx=None):
    """The ground state of H (of the Gross-Pitaevskii functional with
    ``g != 0``) by imaginary-time propagation on the device, normalised to
    ``||psi0||``.  ``real=None`` takes the real-state path exactly when H and
    psi0 are real.  One step at a time until ``residual <= tol * max(1,
    |mu|)`` or ``max_steps``.  Returns a dict: ``psi``, ``mu``, ``energy``,
    ``residual``, ``steps``, ``converged`` and ``history`` (the energetics
    rows; mu, energy and residual are the last row's, of the state before the
    last step).

    The nonlinear term rewrites the matrix's stored diagonal, which only the
    "csr" and "split" formats keep.  On the real path H goes up through
    ``Context.set_matrix``, where "auto" may pick a format without one and
    ``set_nonlinear`` is then refused; so with ``g != 0``, ``real`` and no
    ``ctx`` the context opened here is a "csr" one.  Pass a
    ``Context(spmv_format="split")`` for a grid Hamiltonian that qualifies."""
    if real is None:
        real = not (np.iscomplexobj(H) or np.iscomplexobj(psi0))
    own = None
    if ctx is None and real and g != 0.0:
        ctx = own = Context(spmv_format="csr")
    try:
        P = Propagator(H, psi0, s, max_blocks, basis=basis, ctx=ctx, real=real)
    except Exception:
        if own is not None:
            own.close()
        raise
    try:
        if not real:
            P.set_imaginary_time(True)
        if g != 0.0:
            P.set_nonlinear(g, density)
        out = _ground_state_loop(lambda: P.step(tau), P.energetics, P.state, tol, max_steps)
        if real:
            out["psi"] = out["psi"].real.copy()
        return out
    finally:
        P.close()
        if own is not None:
            own.close()


def ca_lanczos_prop(A, r0, s, m, dt, tol=1.0e-10, basis="newton", eigest=None, adaptive=False, ctx=None):
    """``[T,Q,lsteps] = ca_lanczos_prop(A,r0,s,m,dt,tol,basis,eigest,adaptive)``
    -- ca_lanczos_prop.m:3-135 for a real symmetric A and a real or complex
    r0; Q is complex n x lsteps."""
    n = A.shape[0]
    own = ctx is None
    ctx = ctx or Context()
    try:
        ctx.set_matrix_stacked(A)
        re, im = _split(r0)
        if re.shape[0] != n:
            raise ValueError("r0 must have A.shape[0] entries")
        e, ne = _eigest(eigest)
        cap = max(int(s) * int(m), 1)
        T = np.zeros(cap * cap)
        Qre, Qim = np.zeros((n, cap), order="F"), np.zeros((n, cap), order="F")
        ls = ctypes.c_int()
        check(ctx.h, lib.cal_ca_lanczos_prop(ctx.h, n, ptr(re), ptr(im), s, m, float(dt), float(tol),
                                             basis.encode(), ptr(e), ne, 1 if adaptive else 0, ptr(T), ptr(Qre),
                                             ptr(Qim), ctypes.byref(ls)), "ca_lanczos_prop")
        k = ls.value
        return T[:k * k].reshape(k, k, order="F").copy(), Qre[:, :k] + 1j * Qim[:, :k], k
    finally:
        if own:
            ctx.close()
