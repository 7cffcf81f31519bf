#!/usr/bin/env python3
"""Write csrc/rm_interval_catalogue.h: the 14 catalogue scenes that are compositions of primitives.py as RmSceneOp
programs (scene_program.compile_ops(catalogue_expressions()[id])), so the interval ABI takes catalogue ids without
Python.  tests/test_interval_host.py checks the committed table against compile_ops.

Usage:  python tools/gen_interval_catalogue.py
"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from raymarch_algo_compare_amd import scene_program as sp  # noqa: E402

NAMES = {v: k for k, v in sp.OPCODES.items()}
OUT = os.path.join(ROOT, "raymarch_algo_compare_amd", "csrc", "rm_interval_catalogue.h")


def lit(x: float) -> str:
    return "0.0" if x == 0.0 and str(x)[0] != "-" else ("-0.0" if x == 0.0 else float(x).hex())


def main() -> None:
    ex = sp.catalogue_expressions()
    lines = [
        "// rm_interval_catalogue.h -- the catalogue scenes that are compositions of primitives.py, as scene programs:",
        "// scene_program.compile_ops(catalogue_expressions()[id]) for the 14 ids (ids 0-8, 12, 13, 14, 17, 19).",
        "// Written by tools/gen_interval_catalogue.py; tests/test_interval_host.py checks it against compile_ops.",
        "// Constants are hex-float literals: Capped Torus's sc = (math.sin(2.0), math.cos(2.0)) are the ones",
        "// SceneCappedTorus (rm_scenes.h) holds; the device never evaluates trigonometry.",
        "#pragma once",
        "",
        '#include "../../include/rm_hip.h"',
        "",
        "namespace rm {",
        "",
    ]
    ids = sorted(ex)
    for sid in ids:
        ops = sp.compile_ops(ex[sid])
        lines.append(f"// scene {sid}")
        lines.append(f"static const RmSceneOp kIntervalCatalogue{sid}[{len(ops)}] = {{")
        for op, f in ops:
            fs = ", ".join(lit(v) for v in f)
            lines.append(f"    {{ {op}, 0, {{ {fs} }} }},   // {NAMES[op]}" if fs else f"    {{ {op}, 0, {{ 0.0 }} }},   // {NAMES[op]}")
        lines.append("};")
    lines.append("")
    lines.append("// the program of catalogue scene `id`, nullptr for a scene without one (Mandelbulb, Menger, Gyroid, ...)")
    lines.append("inline const RmSceneOp* interval_catalogue_ops(int id, int32_t* nops)")
    lines.append("{")
    lines.append("    switch (id) {")
    for sid in ids:
        lines.append(f"        case {sid}: *nops = (int32_t)(sizeof kIntervalCatalogue{sid} / sizeof(RmSceneOp)); "
                     f"return kIntervalCatalogue{sid};")
    lines.append("    }")
    lines.append("    *nops = 0;")
    lines.append("    return nullptr;")
    lines.append("}")
    lines.append("")
    lines.append("}  // namespace rm")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
