"""Register allocation of the split single launch (csrc/rm_pipeline.h: pipeline_team_kernel, pipeline_producer_kernel),
read from the code objects' metadata like tests/test_code_objects.py.  No GPU needed.

The split form exists because the fused pipeline_kernel serves two roles with one allocation.  What it buys is visible
here: the team kernel keeps no scratch and spills fewer scalar registers than the stand-alone march_rays_team_kernel
built from the same trip code, and the producer kernel spills fewer scalar registers than the fused one.

The producer kernels read their arguments from a copy in LDS as well (pipeline_body): with the arguments left in scalar
registers the four interleaved Mandelbulb / Standard producer kernels kept the fused kernel's 2 ... 4 spilled vector
registers at the 256-register cap."""
import os

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build")

# sgpr_spill_count of pipeline_team_kernel<SceneMandelbulb, StratStandard, false> when this test was written.  The same
# trips in march_rays_team_kernel spill 60; the team kernel reads everything but three knobs from an LDS copy of its
# arguments, so the queue code adds nothing that lives through a trip loop.
TEAM_SGPR_SPILLS_RECORDED = 44


def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    obj = os.path.join(BUILD, "scene_10.o")
    if not os.path.exists(obj):
        pytest.skip("scene objects are not in the tree (make -C raymarch_algo_compare_amd/csrc)")
    return _tool().collect([obj])


def _one(kernels, text):
    ks = [k for k in kernels if text in k["demangled"]]
    assert len(ks) == 1, (text, [k["demangled"] for k in ks])
    return ks[0]


def test_team_kernel_keeps_everything_in_registers(kernels):
    for batch in ("false", "true"):
        k = _one(kernels, f"pipeline_team_kernel<SceneMandelbulb, StratStandard, {batch}>")
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
        assert k["group_segment_fixed_size"] <= 64 * 1024, k
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, k
    k = _one(kernels, "pipeline_team_kernel<SceneMandelbulb, StratStandard, false>")
    alone = _one(kernels, "march_rays_team_kernel<SceneMandelbulb, StratStandard>")
    assert k["sgpr_spill_count"] <= TEAM_SGPR_SPILLS_RECORDED * 1.1, (k["sgpr_spill_count"], TEAM_SGPR_SPILLS_RECORDED)
    assert k["sgpr_spill_count"] <= alone["sgpr_spill_count"], (k["sgpr_spill_count"], alone["sgpr_spill_count"])


def test_producer_kernels_spill_less_than_the_fused_kernel(kernels):
    for tile_h in (1, 4):
        for batch in ("false", "true"):
            args = f"<SceneMandelbulb, StratStandard, {tile_h}, true, {batch}>"
            producer, fused = _one(kernels, "pipeline_producer_kernel" + args), _one(kernels, "pipeline_kernel" + args)
            print(args, "producer sgpr / vgpr spills", producer["sgpr_spill_count"], producer["vgpr_spill_count"],
                  "fused", fused["sgpr_spill_count"], fused["vgpr_spill_count"])
            assert producer["sgpr_spill_count"] < fused["sgpr_spill_count"], (args, producer, fused)
            assert producer["vgpr_count"] + producer.get("agpr_count", 0) <= 256, (args, producer)
            assert producer["vgpr_spill_count"] == 0, (args, producer)
