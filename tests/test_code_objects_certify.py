"""The certified first-hit kernels (raymarch_algo_compare_amd/_build/certify.o, csrc/rm_certify.hip) read from the code
object's metadata, no GPU needed: exactly the two kernels, and no per-lane memory -- the two walks of a trip keep their
stacks in register slots, the bracket of the ray lives in registers across them, so nothing may spill or live in scratch."""
import importlib.util
import os

import pytest

from conftest import ROOT

OBJ = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build", "certify.o")


@pytest.fixture(scope="module")
def tool():
    assert os.path.exists(OBJ), "certify.o is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_exactly_the_two_kernels(tool):
    names = sorted(k["demangled"].split("(")[0].split("::")[-1] for k in tool.collect([OBJ]))
    assert names == ["certify_march_kernel", "certify_render_kernel"]


def test_no_spills_and_no_scratch(tool):
    found = tool.matching_instructions(OBJ, r"\b(scratch|buffer)_")
    for k in tool.collect([OBJ]):
        print(k["demangled"].split("(")[0], {f: k[f] for f in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                                "private_segment_fixed_size", "group_segment_fixed_size")})
        assert found.get(k["name"]) == [], (k["demangled"], found.get(k["name"], "not disassembled")[:4])
        assert k["vgpr_spill_count"] == 0, k["demangled"]
        assert k["private_segment_fixed_size"] == 0, k["demangled"]
