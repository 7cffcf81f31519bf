"""Builds tests/native/rccl_loopback.cpp, the loop-back stand-in for RCCL that RM_RCCL_LIBRARY names to librm_hip.so
(tests/test_gpu_loopback_gather.py, tests/test_loopback_host.py), and declares its test-only exports for ctypes."""
import ctypes
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCCL_SYMBOLS = ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclAllGather", "ncclSend", "ncclRecv",
                "ncclGroupStart", "ncclGroupEnd", "ncclGetErrorString")
LB_SYMBOLS = ("lb_reset", "lb_pending", "lb_last_reason", "lb_fill", "lb_counts", "lb_epoch", "lb_peek")


def rocm_root() -> str:
    """ROCm as csrc/Makefile finds it: where $HIPCC (default: the hipcc on PATH) is installed."""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc:
        return os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    return os.environ.get("ROCM_PATH", "/opt/rocm")


def build_stub() -> str:
    """g++ build of the stand-in (host code only: it links the HIP runtime, it holds no kernel).  Its path."""
    src = os.path.join(ROOT, "tests", "native", "rccl_loopback.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build_rccl_loopback.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        rocm = rocm_root()
        lib = os.path.join(rocm, "lib")
        tmp = f"{out[:-3]}.{os.getpid()}.so"
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                        "-o", tmp, src, "-L" + lib, "-lamdhip64", "-Wl,-rpath," + lib], check=True)
        os.replace(tmp, out)
    return out


def declare(S: ctypes.CDLL) -> ctypes.CDLL:
    """Prototypes of the lb_* exports."""
    S.lb_reset.restype = None
    S.lb_pending.restype = ctypes.c_int
    S.lb_last_reason.restype = ctypes.c_char_p
    S.lb_fill.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    S.lb_fill.restype = ctypes.c_int
    S.lb_counts.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    S.lb_counts.restype = None
    S.lb_epoch.argtypes = [ctypes.c_int]
    S.lb_epoch.restype = None
    S.lb_peek.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    S.lb_peek.restype = ctypes.c_longlong
    return S
