"""RM_RCCL_LIBRARY (csrc/rm_gather.hip, rccl_load) and the loop-back stand-in tests/native/rccl_loopback.cpp, without a
device: the stand-in compiles with g++ and exports what the library resolves; the variable names the ONE library that
is tried (a missing file or a missing symbol is RM_E_RCCL with the path in the message, never a quiet fall-back to
librccl.so.1); unset, the library behaves as before.  rm_comm_unique_id needs no device, and with the stand-in (or a
library that fails to load) it makes no HIP call; in the unset case it is real RCCL's ncclGetUniqueId that runs, and
that does look for a device.  Each check is a fresh process because the library reads the variable and caches the handle once."""
import ctypes
import os
import subprocess
import sys

import pytest

from loopback_stub import LB_SYMBOLS, NCCL_SYMBOLS, build_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_E_RCCL = -7
PROBE = """
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from raymarch_algo_compare_amd import _native
L = _native.load()
ident = ctypes.create_string_buffer(128)
rc = L.rm_comm_unique_id(ident)
print("PROBE", rc, int(any(ident.raw)), L.rm_last_error().decode("utf-8", "replace"))
"""


@pytest.fixture(scope="module")
def stub():
    return build_stub()


def _unique_id(library):
    """(return code, whether the id has a non-zero byte, rm_last_error()) of rm_comm_unique_id in a fresh process with
    RM_RCCL_LIBRARY = `library` (None: unset)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RM_RCCL_LIBRARY", "RM_HIP_LIB")}
    if library is not None:
        env["RM_RCCL_LIBRARY"] = library
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", PROBE, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    _, rc, nonzero, *msg = lines[0].split(" ", 3)
    return int(rc), bool(int(nonzero)), msg[0] if msg else ""


def test_the_stand_in_exports_what_the_library_resolves(stub):
    S = ctypes.CDLL(stub)
    missing = [n for n in NCCL_SYMBOLS + LB_SYMBOLS if not hasattr(S, n)]
    assert not missing, missing
    assert len(NCCL_SYMBOLS) == 9
    S.ncclGetErrorString.restype = ctypes.c_char_p
    S.ncclGetErrorString.argtypes = [ctypes.c_int]
    assert b"invalid usage" in S.ncclGetErrorString(5)          # ncclInvalidUsage: what a refused call returns
    S.lb_pending.restype = ctypes.c_int
    assert S.lb_pending() == 0                                   # host state only: no HIP call


def test_a_named_library_is_the_one_that_is_loaded(stub):
    rc, nonzero, msg = _unique_id(stub)
    assert (rc, nonzero) == (0, True), msg


def test_a_named_library_that_is_missing_is_an_error_naming_it():
    rc, nonzero, msg = _unique_id("/nonexistent.so")
    assert rc == RM_E_RCCL and not nonzero
    assert "/nonexistent.so" in msg and "RM_RCCL_LIBRARY" in msg


def test_a_named_library_without_the_symbols_is_an_error_naming_it():
    rc, nonzero, msg = _unique_id("libm.so.6")                  # loads, and is no RCCL
    assert rc == RM_E_RCCL and not nonzero
    assert "libm.so.6 lacks ncclGetUniqueId" in msg


@pytest.mark.parametrize("value", [None, ""])
def test_without_a_named_library_nothing_changes(value):
    """Unset (or empty), the default names are tried as before this variable existed.  Recorded from the parent commit:
    where ROCm's librccl.so.1 is installed and there is no device, RCCL loads and its ncclGetUniqueId fails ('unhandled
    cuda error'), so the call returns RM_E_RCCL with 'R.GetUniqueId(&u) failed'; with a device it returns RM_OK and an id;
    without RCCL installed it is RM_E_RCCL with 'librccl.so.1 could not be loaded'.  Any of the three is accepted; the
    first is PINNED only where this test can tell, without a HIP call, that it is on such a host: no /dev/kfd and a
    librccl.so.1 under $ROCM_PATH/lib (default /opt/rocm/lib).  That need not be where dlopen finds RCCL, so elsewhere the
    test records the three outcomes and no more."""
    rc, nonzero, msg = _unique_id(value)
    assert "RM_RCCL_LIBRARY" not in msg
    if rc == 0:
        assert nonzero
    else:
        assert rc == RM_E_RCCL and not nonzero
        assert "R.GetUniqueId(&u) failed" in msg or "librccl.so.1 could not be loaded" in msg
    if not os.path.exists("/dev/kfd") and os.path.exists(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "librccl.so.1")):
        assert rc == RM_E_RCCL and "R.GetUniqueId(&u) failed" in msg       # the parent commit's answer on a host without a GPU
