"""Register allocation of the scene-program interpreter's kernels (raymarch_algo_compare_amd/_build/scene_prog.o, read
from the code objects' metadata and disassembly by tools/kernel_resources.py; no GPU needed).  The interpreter keeps its
value and point stacks in registers (csrc/rm_scene_program.h): no kernel may touch scratch memory or spill vector
registers.

The resume kernels carry a 20-36 byte private segment that no instruction reads or writes -- a stack frame the
compiler lays out around the parked-ray record, the same size as the catalogue scenes' kernels of the same template
(tools/kernel_resources.py scene_0.o: Sphere 20 / 36) -- so the assertion on memory traffic is made on the instructions
themselves.  Scalar spills go to VGPR lanes (v_writelane / v_readlane), not to memory; the render kernels of the
interpreter hold 58-122 of them (the catalogue's Pillar Forest 62-100)."""
import importlib.util
import os

import pytest

from conftest import ROOT

OBJ = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build", "scene_prog.o")
N_KERNELS = 13


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(OBJ), "scene_prog.o is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    return [k for k in _tool().collect([OBJ]) if "SceneProgram" in k["demangled"]]


@pytest.fixture(scope="module")
def memory_ops():
    """symbol -> scratch / buffer instructions of every function in the code object"""
    return _tool().matching_instructions(OBJ, r"\b(scratch|buffer)_(load|store)")


def test_every_form_is_built(kernels):
    names = [k["demangled"] for k in kernels]
    for form, n in (("render_kernel<", 2 * N_KERNELS), ("resume_kernel<", 2 * N_KERNELS), ("march_rays_kernel<", N_KERNELS),
                    ("sdf_eval_kernel<", 1)):
        assert sum(form in d for d in names) == n, form
    assert not any("team" in d or "pipeline" in d for d in names)


def test_no_scratch_and_no_vector_spills(kernels, memory_ops):
    assert len(memory_ops) >= len(kernels)
    for k in kernels:
        assert memory_ops.get(k["name"]) == [], (k["demangled"], memory_ops.get(k["name"], "not disassembled")[:4])
        assert k["vgpr_spill_count"] == 0, k["demangled"]
        assert k["sgpr_spill_count"] < 128, k["demangled"]
        if "resume_kernel<" not in k["demangled"]:
            assert k["private_segment_fixed_size"] == 0, k["demangled"]
        else:
            assert k["private_segment_fixed_size"] <= 36, k["demangled"]
