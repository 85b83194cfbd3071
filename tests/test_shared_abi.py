"""The C ABI of the shared stacked SpMV format (cal_spmv_shared_info, the
"shared" value of cal_set_spmv_format).  CPU only."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_shared_symbol(cal):
    lib = ctypes.CDLL(cal.LIB_PATH)
    assert hasattr(lib, "cal_spmv_shared_info")
    from ca_lanczos_amd import _lib
    assert "cal_spmv_shared_info" in {s[0] for s in _lib.SIGNATURES}
    assert hasattr(cal.Context, "spmv_shared_info")


def test_header_declares_it_and_documents_the_format():
    hdr = open(os.path.join(ROOT, "include", "calanczos.h")).read()
    assert re.search(r"int\s+cal_spmv_shared_info\(cal_ctx\*\s*ctx,\s*int\*\s*on,\s*int64_t\*\s*n_half,\s*"
                     r"int64_t\*\s*nnz_stored\);", hdr)
    assert '"shared"' in hdr


def test_mex_shims_still_compile_against_the_header():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "mex"), "check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
