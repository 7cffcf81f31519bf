"""Register allocation of the kernels of the interpreter's second instantiation (SceneExtProgram, the one with the four
ops beyond primitives.py: raymarch_algo_compare_amd/_build/scene_progext.o), read from the code object as
tests/test_code_objects_scene_program.py reads scene_prog.o; no GPU needed."""
import importlib.util
import os

from conftest import ROOT


def test_ext_interpreter_kernels_keep_their_stacks_in_registers():
    """scene_progext.o (SceneExtProgram: the kernels of a program with an op beyond primitives.py) is held to what
    tests/test_code_objects_scene_program.py asks of scene_prog.o: every form built, no scratch or buffer instruction, no
    vector spill, fewer than 128 scalar spills; and scene_prog.o itself holds no kernel of it."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    build = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build")
    obj = os.path.join(build, "scene_progext.o")
    assert os.path.exists(obj), "scene_progext.o is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    kernels = [k for k in tool.collect([obj]) if "SceneExtProgram" in k["demangled"]]
    names = [k["demangled"] for k in kernels]
    for form, n in (("render_kernel<", 26), ("resume_kernel<", 26), ("march_rays_kernel<", 13), ("sdf_eval_kernel<", 1)):
        assert sum(form in d for d in names) == n, form
    memory_ops = tool.matching_instructions(obj, r"\b(scratch|buffer)_(load|store)")
    for k in kernels:
        assert memory_ops.get(k["name"]) == [], (k["demangled"], memory_ops.get(k["name"], "not disassembled")[:4])
        assert k["vgpr_spill_count"] == 0, k["demangled"]
        assert k["sgpr_spill_count"] < 128, (k["demangled"], k["sgpr_spill_count"])
        assert k["private_segment_fixed_size"] <= (36 if "resume_kernel<" in k["demangled"] else 0), k["demangled"]
    plain = tool.collect([os.path.join(build, "scene_prog.o")])
    assert not any("SceneExtProgram" in k["demangled"] for k in plain)
