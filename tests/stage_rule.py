"""The staging rule of the stream schedule as the header states it: isplib_stream_stage_panel (include/isplib_hip.h) is a static
inline, so it is compiled here into a scrap library (as tests/test_host_owner_exchange.py does for its predicate) and called
through ctypes.  Shared by tests/test_stage_host.py and tests/test_gpu_stage.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, FORCE, AUTO = 0, 1, 2

_SRC = r"""
#include "isplib_hip.h"
extern "C" int stage_panel(unsigned long long y_addr, long long ldy, long long c0, long long k, int streams, long long n, long long nnz,
                           unsigned long long room_bytes, int mode) {
   return isplib_stream_stage_panel(y_addr, ldy, c0, k, streams, n, nnz, room_bytes, mode);
}
"""


def header_constant(name: str) -> int:
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    expr = re.search(rf"^#define\s+ISPLIB_{name}[ \t]+(\S.*?)\s*$", text, flags=re.M).group(1)
    return int(eval(re.sub(r"(?<=[0-9a-fA-F])[uU]\b", "", expr)))


def compile_rule(tmp_dir):
    """-> stage_panel(y_addr, ldy, c0, k, streams, n, nnz, room_bytes, mode) -> bool"""
    src, so = os.path.join(str(tmp_dir), "stage_rule.cpp"), os.path.join(str(tmp_dir), "stage_rule.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", so], check=True, timeout=120)
    L = ctypes.CDLL(so)
    L.stage_panel.argtypes = [ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong,
                              ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int]
    return lambda *a: bool(L.stage_panel(*a))


def old_workspace_bytes(n_parts: int, streams: int) -> int:
    """isplib_spmm_stream_workspace_bytes before the staging area: the partial rows alone."""
    return 256 if n_parts <= 0 else (n_parts * (256 // streams) * 4 + 255) & ~255
