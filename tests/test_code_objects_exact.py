"""The exact first-hit kernels (raymarch_algo_compare_amd/_build/exact.o, csrc/rm_exact.hip) read from the code object's
metadata, no GPU needed: exactly the two kernels, and no per-lane memory -- the walks of csrc/rm_exact.h keep the germ
stack in one word and the saved points in register slots, so nothing may spill or live in scratch."""
import importlib.util
import os

import pytest

from conftest import ROOT

OBJ = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build", "exact.o")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(OBJ), "exact.o is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.collect([OBJ])


def test_exactly_the_two_kernels(kernels):
    names = sorted(k["demangled"].split("(")[0].split("::")[-1] for k in kernels)
    assert names == ["exact_march_kernel", "exact_render_kernel"]


def test_no_spills_and_no_scratch(kernels):
    for k in kernels:
        print(k["demangled"].split("(")[0], {f: k[f] for f in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                                "private_segment_fixed_size", "group_segment_fixed_size")})
        assert k["vgpr_spill_count"] == 0, k["demangled"]
        assert k["private_segment_fixed_size"] == 0, k["demangled"]
