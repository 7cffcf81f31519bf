"""The strategy-program interpreter's code objects (raymarch_algo_compare_amd/_build/strat_*.o, read from their metadata
and disassembly by tools/kernel_resources.py; no GPU needed): exactly three kernels per object, registers in VGPRs and
LDS only -- no scratch or buffer memory instruction, no vector spill, at most 256 VGPRs, no private segment.

The kernel template's frame would otherwise hold a 16-byte slot per rematerialised 128-bit kernel-argument load that no
instruction touches (20 / 36 bytes with the emergency slot, as render_kernel carries for the compiled strategies of the
same scenes); the build of these objects sets a private segment that nothing can reach to 0 (csrc/rm_peephole.py,
--drop-unused-private-segment), and test_no_scratch_or_buffer_instruction is the other half of that statement."""
import glob
import importlib.util
import os

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build")
NAMES = [str(i) for i in range(20)] + ["prog", "progext"]


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def objects():
    objs = [os.path.join(BUILD, f"strat_{n}.o") for n in NAMES]
    missing = [o for o in objs if not os.path.exists(o)]
    assert not missing, f"{missing[0]} is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    assert sorted(glob.glob(os.path.join(BUILD, "strat_*.o"))) == sorted(objs)
    return objs


@pytest.fixture(scope="module")
def kernels(objects):
    tool = _tool()
    return {o: tool.collect([o]) for o in objects}


def test_exactly_three_kernels_per_object(kernels):
    for obj, ks in kernels.items():
        names = sorted(k["demangled"] for k in ks)
        assert len(names) == 3, (obj, names)
        assert all("StratProgram" in n for n in names), (obj, names)
        assert sum("march_rays_kernel<" in n for n in names) == 1, (obj, names)
        assert sum("render_kernel<" in n and "4, false, false>" in n for n in names) == 1, (obj, names)
        assert sum("render_kernel<" in n and "4, false, true>" in n for n in names) == 1, (obj, names)


def test_the_scene_objects_hold_no_interpreter_kernel():
    tool = _tool()
    for n in ("0", "prog"):
        assert not any("StratProgram" in k["demangled"] for k in tool.collect([os.path.join(BUILD, f"scene_{n}.o")]))


def test_no_scratch_or_buffer_instruction(objects, kernels):
    tool = _tool()
    for obj in objects:
        ops = tool.matching_instructions(obj, r"\b(scratch|buffer)_(load|store)")
        for k in kernels[obj]:
            assert ops.get(k["name"]) == [], (k["demangled"], ops.get(k["name"], "not disassembled")[:4])


def test_nothing_can_reach_private_memory(objects, kernels):
    """what the build's zeroed private segment rests on, read from the finished objects: no access, no call or indirect
    jump to code that could make one, no flat-scratch or private-aperture operand"""
    tool = _tool()
    rx = r"\b(scratch_\w+|buffer_(load|store|atomic)\w*|s_swappc_b64|s_setpc_b64|s_call_b64|flat_scratch\w*|src_private_base|src_private_limit)\b"
    for obj in objects:
        ops = tool.matching_instructions(obj, rx)
        for k in kernels[obj]:
            assert ops.get(k["name"]) == [], (k["demangled"], ops.get(k["name"], "not disassembled")[:4])


def test_registers(kernels):
    for ks in kernels.values():
        for k in ks:
            assert k["vgpr_spill_count"] == 0, k["demangled"]
            assert k["vgpr_count"] + k["agpr_count"] <= 256, k["demangled"]
            assert k["group_segment_fixed_size"] <= 160 * 1024, k["demangled"]


def test_no_private_segment(kernels):
    bad = {k["demangled"][:70]: k["private_segment_fixed_size"] for ks in kernels.values() for k in ks
           if k["private_segment_fixed_size"] != 0}
    print(bad)
    assert not bad
