"""The device-math test kernels (raymarch_algo_compare_amd/_build/math_check.o, csrc/rm_math_check.hip) read from the code
object, no GPU needed: one kernel per RmMathFn routine is built, each in the render kernels' workgroup shape, with the
libm tables in LDS, and through the ISA peephole (csrc/rm_peephole.py) like every other object of the library -- so
tests/test_gpu_math_exact.py checks the instructions a frame runs."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

OBJ = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build", "math_check.o")
N_FNS = 15      # RM_MATH_COUNT (include/rm_hip.h)
NO_TABLE = {4, 5}   # RM_MATH_POW_HALF_GUARD, RM_MATH_SQRT: the square root alone


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(OBJ):
        pytest.skip("math_check.o is not in the tree (make -C raymarch_algo_compare_amd/csrc)")
    tool = _tool()
    kernels = [k for k in tool.collect([OBJ]) if "math_check_kernel<" in k["demangled"]]
    dis = {}
    with tempfile.TemporaryDirectory() as td:
        for co in tool.code_objects(OBJ, td):
            text = subprocess.run([os.path.join(tool.LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True,
                                  text=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = m.group(1)
                    dis.setdefault(cur, [])
                elif cur:
                    dis[cur].append(line.strip())
    return kernels, dis


def test_one_kernel_per_routine_with_every_table_in_lds(built):
    kernels, _ = built
    fns = sorted(int(re.search(r"math_check_kernel<(\d+)>", k["demangled"]).group(1)) for k in kernels)
    assert fns == list(range(N_FNS))
    for k in kernels:
        # rm_s_pow_log_tab 512 + rm_s_exp_tab 256 + rm_s_log_tab 256 + rm_s_sincostab 550 + rm_s_asncs 2808 +
        # rm_s_inroot 128 + rm_s_cij 1687 doubles (csrc/rm_tables.h)
        assert k["group_segment_fixed_size"] >= 8 * 6197, k["demangled"]


def test_kernels_went_through_the_peephole(built):
    """No VOP2 v_cndmask_b32 with a VGPR or inline-constant src0 is left (rm_peephole.py re-encodes those as VOP3); the
    routines that use a table read it from LDS (ds_read) as the render kernels do."""
    kernels, dis = built
    vop2 = re.compile(r"\bv_cndmask_b32_e32\s+v\d+,\s*(v\d+|-?\d+(\.\d+)?)\s*,")
    for k in kernels:
        lines = dis.get(k["name"])
        assert lines, ("not disassembled", k["demangled"])
        assert not [ln for ln in lines if vop2.search(ln)], k["demangled"]
        if int(re.search(r"math_check_kernel<(\d+)>", k["demangled"]).group(1)) not in NO_TABLE:
            assert any(re.search(r"\bds_read", ln) for ln in lines), k["demangled"]
