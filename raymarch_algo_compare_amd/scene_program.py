"""User-defined CSG scenes: expressions over the reference's scenes/primitives.py functions, compiled to a scene
program (RmSceneOp[], include/rm_hip.h) that the device interpreter evaluates (csrc/rm_scene_program.h).

    from raymarch_algo_compare_amd.scene_program import *
    info = register_scene("Two Boxes", op_smooth_union(sd_box((1, 1, 1)), op_translate((1.5, 0, 0), sd_sphere(0.7)), 0.3))
    run_once(scene_name="Two Boxes", strategy_name="Segment")

The builder's names and argument orders are the reference's, without the point argument: a point transform takes the
subtree it applies to (`op_translate(offset, child)`, `op_repeat(spacing, child)`), a distance modifier the subtree it
modifies (`op_round(child, radius)`, `op_onion(child, thickness)`).  `sd_cone`'s cos / sin of the angle are computed
here by Python's math (the libm the reference calls).

Four ops go beyond primitives.py, enough to write five more catalogue scenes as programs (catalogue_twins):
`op_scale(child, factor)` multiplies a distance, `op_limited_repeat(spacing, limit, child)` is a finite lattice,
`sd_menger_cross(scale)` is one trip of the Menger sponge's fold and `sd_gyroid(freq, lipschitz)` the gyroid sheet (the
one op whose sin / cos the device evaluates, with the library's exact restatements of libm's).

Three placement builders orient a subtree (PLACEMENT_OPCODES): `op_rotate(angles_rad, child)` turns it about the world x
axis, then y, then z, `op_turn(quarters, child)` does so by exact quarter turns (the same opcode, constants 0 and +-1),
`op_mirror(axes, child)` evaluates it at the absolute value of the flagged coordinates.  One of them is one nested point
transform, of which a program may have MAX_POINTS open at once.

A registered scene is found by registry.get_scene_by_name and accepted by run_once, HipCollector, run_gpu_benchmark,
GPURunner (by its id), the sweep and the _native entry points; get_all_scenes() / SCENES stay the 20 catalogue scenes.
Registration is process-wide; unregister_scene frees the program (its id is never reused).
"""
from __future__ import annotations

import json
import math
import threading
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

from . import registry
from .registry import SceneInfo

# opcodes (RM_SOP_*, include/rm_hip.h)
OPCODES = {
    "sd_sphere": 0, "sd_box": 1, "sd_plane": 2, "sd_cylinder": 3, "sd_torus": 4, "sd_capsule": 5,
    "sd_capped_torus": 6, "sd_cone": 7,
    "op_union": 8, "op_subtract": 9, "op_intersect": 10,
    "op_smooth_union": 11, "op_smooth_subtract": 12, "op_smooth_intersect": 13,
    "op_translate": 14, "op_repeat": 15, "pop_point": 16,
    "op_round": 17, "op_onion": 18,
}
# the four ops that are not primitives.py functions (RM_SOP_SCALE ..)
EXT_OPCODES = {"op_scale": 19, "op_limited_repeat": 20, "sd_menger_cross": 21, "sd_gyroid": 22}
# placement: one op_rotate / op_turn (the same opcode) is a full orientation in one point slot; op_mirror folds space
PLACEMENT_OPCODES = {"op_rotate": 23, "op_turn": 23, "op_mirror": 24}
_ALL_OPCODES = {**OPCODES, **EXT_OPCODES, **PLACEMENT_OPCODES}
MAX_OPS, MAX_VALUES, MAX_POINTS = 256, 8, 4

# op -> (parameters as (name, number of floats), children)
_SPEC: Dict[str, Tuple[Tuple[Tuple[str, int], ...], Tuple[str, ...]]] = {
    "sd_sphere": ((("radius", 1),), ()),
    "sd_box": ((("half_extents", 3),), ()),
    "sd_plane": ((("normal", 3), ("offset", 1)), ()),
    "sd_cylinder": ((("radius", 1), ("half_height", 1)), ()),
    "sd_torus": ((("major_radius", 1), ("minor_radius", 1)), ()),
    "sd_capsule": ((("a", 3), ("b", 3), ("radius", 1)), ()),
    "sd_capped_torus": ((("sc", 2), ("ra", 1), ("rb", 1)), ()),
    "sd_cone": ((("angle_rad", 1), ("height", 1)), ()),
    "op_union": ((), ("a", "b")),
    "op_subtract": ((), ("a", "b")),
    "op_intersect": ((), ("a", "b")),
    "op_smooth_union": ((("k", 1),), ("a", "b")),
    "op_smooth_subtract": ((("k", 1),), ("a", "b")),
    "op_smooth_intersect": ((("k", 1),), ("a", "b")),
    "op_translate": ((("offset", 3),), ("child",)),
    "op_repeat": ((("spacing", 3),), ("child",)),
    "op_round": ((("radius", 1),), ("child",)),
    "op_onion": ((("thickness", 1),), ("child",)),
    "op_scale": ((("factor", 1),), ("child",)),
    "op_limited_repeat": ((("spacing", 3), ("limit", 3)), ("child",)),
    "sd_menger_cross": ((("scale", 1),), ()),
    "sd_gyroid": ((("freq", 1), ("lipschitz", 1)), ()),
    "op_rotate": ((("angles_rad", 3),), ("child",)),
    "op_turn": ((("quarters", 3),), ("child",)),
    "op_mirror": ((("axes", 3),), ("child",)),
}
_POINT_TRANSFORMS = ("op_translate", "op_repeat", "op_limited_repeat", "op_rotate", "op_turn", "op_mirror")
# cos, sin of k quarter turns: exact, where math.cos(math.pi / 2) is 6.1e-17
_QUARTER = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


@dataclass(frozen=True)
class Expr:
    """One node of a scene expression: a primitives.py function, its constants and its subtrees."""
    op: str
    params: Tuple[Tuple[str, object], ...]
    children: Tuple["Expr", ...] = ()

    def param(self, name):
        return dict(self.params)[name]

    def to_json(self) -> dict:
        d = {"op": self.op}
        for k, v in self.params:
            d[k] = list(v) if isinstance(v, tuple) else v
        for k, c in zip(_SPEC[self.op][1], self.children):
            d[k] = c.to_json()
        return d


def _num(name, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a number, not {type(v).__name__}")
    return float(v)


def _make(op: str, values: dict, children: Sequence[Expr]) -> Expr:
    params, kids = _SPEC[op]
    out = []
    for name, n in params:
        v = values[name]
        if n == 1:
            out.append((name, _num(name, v)))
        else:
            vs = tuple(v) if isinstance(v, (list, tuple)) else None
            if vs is None or len(vs) != n:
                raise TypeError(f"{op}: {name} must be a sequence of {n} numbers")
            nums = tuple(_num(name, x) for x in vs)
            if op == "op_turn":
                if any(not math.isfinite(x) or x != math.floor(x) for x in nums):
                    raise ValueError(f"op_turn: quarters must be whole numbers, not {nums}")
                nums = tuple(float(int(x) % 4) for x in nums)
            if op == "op_mirror" and any(x not in (0.0, 1.0) for x in nums):
                raise ValueError(f"op_mirror: axes must be 0 / 1 flags, not {nums}")
            out.append((name, nums))
    for c in children:
        if not isinstance(c, Expr):
            raise TypeError(f"{op}: a subtree must be an expression, not {type(c).__name__}")
    if len(children) != len(kids):
        raise TypeError(f"{op} takes {len(kids)} subtree(s)")
    return Expr(op, tuple(out), tuple(children))


# ---- the builder: the reference's names (scenes/primitives.py) -----------------------------------------------------

def sd_sphere(radius) -> Expr:
    return _make("sd_sphere", {"radius": radius}, ())


def sd_box(half_extents) -> Expr:
    return _make("sd_box", {"half_extents": half_extents}, ())


def sd_plane(normal, offset) -> Expr:
    return _make("sd_plane", {"normal": normal, "offset": offset}, ())


def sd_cylinder(radius, half_height) -> Expr:
    return _make("sd_cylinder", {"radius": radius, "half_height": half_height}, ())


def sd_torus(major_radius, minor_radius) -> Expr:
    return _make("sd_torus", {"major_radius": major_radius, "minor_radius": minor_radius}, ())


def sd_capsule(a, b, radius) -> Expr:
    return _make("sd_capsule", {"a": a, "b": b, "radius": radius}, ())


def sd_capped_torus(sc, ra, rb) -> Expr:
    """sc = (sin(half_angle), cos(half_angle)), as the reference takes it."""
    return _make("sd_capped_torus", {"sc": sc, "ra": ra, "rb": rb}, ())


def sd_cone(angle_rad, height) -> Expr:
    return _make("sd_cone", {"angle_rad": angle_rad, "height": height}, ())


def op_union(a: Expr, b: Expr) -> Expr:
    return _make("op_union", {}, (a, b))


def op_subtract(a: Expr, b: Expr) -> Expr:
    """b subtracted from a."""
    return _make("op_subtract", {}, (a, b))


def op_intersect(a: Expr, b: Expr) -> Expr:
    return _make("op_intersect", {}, (a, b))


def op_smooth_union(a: Expr, b: Expr, k) -> Expr:
    return _make("op_smooth_union", {"k": k}, (a, b))


def op_smooth_subtract(a: Expr, b: Expr, k) -> Expr:
    return _make("op_smooth_subtract", {"k": k}, (a, b))


def op_smooth_intersect(a: Expr, b: Expr, k) -> Expr:
    return _make("op_smooth_intersect", {"k": k}, (a, b))


def op_translate(offset, child: Expr) -> Expr:
    return _make("op_translate", {"offset": offset}, (child,))


def op_repeat(spacing, child: Expr) -> Expr:
    """Infinite repetition; an axis with spacing 0 is untouched."""
    return _make("op_repeat", {"spacing": spacing}, (child,))


def op_round(child: Expr, radius) -> Expr:
    return _make("op_round", {"radius": radius}, (child,))


def op_onion(child: Expr, thickness) -> Expr:
    return _make("op_onion", {"thickness": thickness}, (child,))


def op_scale(child: Expr, factor) -> Expr:
    """child * factor (factor > 0): a distance that is off by a known factor, e.g. Bad Lipschitz Sphere."""
    return _make("op_scale", {"factor": factor}, (child,))


def op_limited_repeat(spacing, limit, child: Expr) -> Expr:
    """A finite lattice: per axis x - c * max(-l, min(l, floor(x / c + 0.5))); an axis with spacing 0 is untouched."""
    return _make("op_limited_repeat", {"spacing": spacing, "limit": limit}, (child,))


def sd_menger_cross(scale) -> Expr:
    """One trip of the Menger sponge's loop (scenes/catalog.py:221-237) at fold scale `scale` (> 0)."""
    return _make("sd_menger_cross", {"scale": scale}, ())


def sd_gyroid(freq, lipschitz) -> Expr:
    """(sin(q.x) cos(q.y) + sin(q.y) cos(q.z) + sin(q.z) cos(q.x)) / lipschitz with q = freq * p (lipschitz > 0)."""
    return _make("sd_gyroid", {"freq": freq, "lipschitz": lipschitz}, ())


def op_rotate(angles_rad, child: Expr) -> Expr:
    """The child turned about the world x axis by angles_rad[0], then about y, then about z (radians, right-handed).  The
    cosines and sines are computed here by Python's math, as sd_cone's are; an angle of exactly 0 leaves its plane untouched."""
    return _make("op_rotate", {"angles_rad": angles_rad}, (child,))


def op_turn(quarters, child: Expr) -> Expr:
    """op_rotate by whole quarter turns (three integers, taken mod 4): the cosines and sines are exactly 0 and +-1, the
    rotation is a permutation of the axes with signs and rounds nothing -- op_turn((0, 0, 1), sd_cylinder(r, h)) is the
    cylinder about x."""
    return _make("op_turn", {"quarters": quarters}, (child,))


def op_mirror(axes, child: Expr) -> Expr:
    """The child evaluated at the point with every flagged coordinate (three 0 / 1 flags) replaced by its absolute value:
    the child's positive side, mirrored.  The value is the mirrored solid's distance only where the child's solid lies
    on the positive side of each mirror plane (elsewhere it is still a 1-Lipschitz bound that is positive outside)."""
    return _make("op_mirror", {"axes": axes}, (child,))


# ---- the catalogue scenes expressible in primitives.py, restated -------------------------------------------------------
# (csrc/rm_scenes.h, scenes/catalog.py; the built-in scene and its program give bit-identical frames)
_CLOUD = [(0.4253, 1.3505, 0.9373, 0.4723), (-0.9343, -0.6794, 1.2701, 0.4257), (-1.6821, 1.0922, 1.0100, 0.3090),
          (-0.1090, -0.6697, -0.7534, 0.4659), (-0.8334, -0.1867, 0.0155, 0.4879), (0.1819, 1.6847, 0.9951, 0.4789),
          (0.4154, 1.6625, -0.9680, 0.4053), (-1.1553, 0.3826, -1.5506, 0.3120), (-1.5787, 0.0506, -0.1149, 0.3223),
          (1.4184, 0.4394, 0.0480, 0.4841), (-0.0106, -0.8584, -1.6599, 0.4015), (-1.0458, 0.6529, -1.0179, 0.3197),
          (-0.4436, -1.6873, 1.1222, 0.4745), (-1.1748, -0.7902, 1.2931, 0.4211), (0.0333, 1.1803, 0.4750, 0.4053),
          (0.8220, -1.3889, 0.1399, 0.3628), (0.0264, 1.2626, -0.4717, 0.3704), (0.3338, -1.4985, -0.3821, 0.3327),
          (-0.6017, -1.1893, 1.0755, 0.2884), (-0.4099, 1.6277, 0.3060, 0.4728), (0.3572, 0.4692, 0.5999, 0.3829),
          (-1.1873, -0.2029, -0.8855, 0.4005), (-0.3315, -1.3712, 1.5906, 0.3509), (-0.9690, 0.5840, -0.6786, 0.4453)]


def catalogue_expressions() -> Dict[int, Expr]:
    """Scene id -> expression for the 14 catalogue scenes that are compositions of primitives.py (0-8, 12, 13, 14,
    17, 19).  Sphere Cloud's `d = 1e10` seed is the first union operand, as sd_plane with a zero normal and offset
    -1e10 (0 - (-1e10) = 1e10 at every finite point)."""
    cloud = sd_plane((0.0, 0.0, 0.0), -1e10)
    for cx, cy, cz, r in _CLOUD:
        cloud = op_union(cloud, op_translate((cx, cy, cz), sd_sphere(r)))
    metaballs = op_translate((0.0, 0.0, 0.0), sd_sphere(0.8))
    for c in ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0)):
        metaballs = op_smooth_union(metaballs, op_translate(c, sd_sphere(0.6)), 0.45)
    return {
        0: sd_sphere(1.0),
        1: sd_plane((0.0, 1.0, 0.0), -0.5),
        2: sd_box((1.0, 1.0, 1.0)),
        3: sd_torus(1.5, 0.05),
        4: sd_cylinder(1.0, 1.5),
        5: op_union(op_translate((-1.01, 0.0, 0.0), sd_sphere(1.0)), op_translate((1.01, 0.0, 0.0), sd_sphere(1.0))),
        6: op_subtract(sd_box((1.0, 1.0, 1.0)), sd_sphere(1.3)),
        7: op_smooth_union(op_translate((-0.5, 0.0, 0.0), sd_sphere(0.8)),
                           op_translate((0.5, 0.0, 0.0), sd_box((0.6, 0.6, 0.6))), 0.5),
        8: op_onion(op_onion(sd_sphere(2.0), 0.1), 0.05),
        12: op_union(op_repeat((2.0, 0.0, 2.0), sd_cylinder(0.15, 3.0)), sd_plane((0.0, 1.0, 0.0), -3.0)),
        13: op_onion(op_repeat((0.0, 0.5, 0.0), sd_plane((0.0, 1.0, 0.0), 0.0)), 0.01),
        14: cloud,
        17: sd_capped_torus((math.sin(2.0), math.cos(2.0)), 1.2, 0.2),
        19: metaballs,
    }


_BUMPS = [(0.3841, 1.4500, 0.0000), (-0.4821, 1.3500, 0.4417), (0.0725, 1.2500, -0.8260), (0.5860, 1.1500, 0.7643),
          (-1.0548, 1.0500, -0.1866), (0.9794, 0.9500, -0.6230), (-0.3209, 0.8500, 1.1935), (-0.5987, 0.7500, -1.1528),
          (1.2698, 0.6500, 0.4637), (-1.2900, 0.5500, 0.5325), (0.6065, 0.4500, -1.2960), (0.4365, 0.3500, 1.3917),
          (-1.2797, 0.2500, -0.7416), (1.4577, 0.1500, -0.3205), (-0.8622, 0.0500, 1.2264), (-0.1927, -0.0500, -1.4867),
          (1.1412, -0.1500, 0.9618), (-1.4778, -0.2500, 0.0611), (1.0339, -0.3500, -1.0289), (-0.0661, -0.4500, 1.4294),
          (-0.8941, -0.5500, -1.0715), (1.3398, -0.6500, 0.1803), (-1.0663, -0.7500, 0.7419), (0.2713, -0.8500, -1.2058),
          (0.5771, -0.9500, 1.0072), (-1.0205, -1.0500, -0.3256), (0.8743, -1.1500, -0.4039), (-0.3201, -1.2500, 0.7649),
          (-0.2213, -1.3500, -0.6152), (0.3400, -1.4500, 0.1787)]


def catalogue_twins() -> Dict[int, Expr]:
    """Scene id -> a program that is bit-identical, as a point function, to a catalogue scene the library holds no
    interval form for: Menger (9), Bad Lipschitz Sphere (11), Bumpy Sphere (15), Gyroid (16), Box Lattice (18).
    Registered (register_twin), such a twin gives its scene the interval oracle, the segment tracer and the affine
    range.  Mandelbulb (10) has none: its estimator is no distance bound."""
    menger = sd_box((1.0, 1.0, 1.0))
    for s in (1.0, 3.0, 9.0):
        menger = op_intersect(menger, sd_menger_cross(s))
    bumpy = sd_sphere(1.4)
    for c in _BUMPS:
        bumpy = op_union(bumpy, op_translate(c, sd_sphere(0.18)))
    return {
        9: menger,
        11: op_scale(sd_sphere(1.0), 2.0),
        15: bumpy,
        16: op_intersect(sd_gyroid(3.0, 3.0 * 2.0 * 3.0 ** 0.5), sd_sphere(2.2)),
        18: op_limited_repeat((1.0, 1.0, 1.0), (2.0, 2.0, 2.0), sd_box((0.3, 0.3, 0.3))),
    }


# ---- JSON ----------------------------------------------------------------------------------------------------------

def expr_from_json(d: dict) -> Expr:
    """The inverse of Expr.to_json: {"op": <name>, <parameter>: value ..., "a" / "b" / "child": {...}}."""
    if not isinstance(d, dict) or d.get("op") not in _SPEC:
        raise ValueError(f"not a scene expression node: {d!r:.120}")
    op = d["op"]
    params, kids = _SPEC[op]
    known = {"op"} | {n for n, _ in params} | set(kids)
    extra = set(d) - known
    if extra:
        raise ValueError(f"{op}: unknown field(s) {sorted(extra)}")
    missing = [n for n, _ in params if n not in d] + [k for k in kids if k not in d]
    if missing:
        raise ValueError(f"{op}: missing field(s) {missing}")
    return _make(op, {n: d[n] for n, _ in params}, tuple(expr_from_json(d[k]) for k in kids))


def dumps(expr: Expr) -> str:
    return json.dumps(expr.to_json())


def loads(text: str) -> Expr:
    return expr_from_json(json.loads(text))


# ---- compilation to RmSceneOp[] --------------------------------------------------------------------------------------

def compile_ops(expr: Expr) -> List[Tuple[int, Tuple[float, ...]]]:
    """Postfix program: [(opcode, constants)], constants in RmSceneOp.f order (the library validates the result)."""
    out: List[Tuple[int, Tuple[float, ...]]] = []

    def flat(e: Expr) -> Tuple[float, ...]:
        if e.op == "sd_cone":     # cos / sin of the angle by the reference's libm (primitives.py:55-56)
            a = e.param("angle_rad")
            return (math.cos(a), math.sin(a), e.param("height"))
        if e.op == "sd_menger_cross":     # `s *= 3.0` before the division (catalog.py:226, :236)
            return (e.param("scale"), e.param("scale") * 3.0)
        if e.op == "op_rotate":           # (cos, sin) per axis by the host's libm; (1.0, 0.0) exactly for an angle of 0
            return tuple(v for a in e.param("angles_rad") for v in ((1.0, 0.0) if a == 0.0 else (math.cos(a), math.sin(a))))
        if e.op == "op_turn":
            return tuple(v for q in e.param("quarters") for v in _QUARTER[int(q) % 4])
        vals: List[float] = []
        for _, v in e.params:
            vals.extend(v if isinstance(v, tuple) else (v,))
        return tuple(vals)

    def emit(e: Expr) -> None:
        kids = _SPEC[e.op][1]
        if kids == ("child",) and e.op in _POINT_TRANSFORMS:
            out.append((_ALL_OPCODES[e.op], flat(e)))
            emit(e.children[0])
            out.append((OPCODES["pop_point"], ()))
            return
        for c in e.children:
            emit(c)
        out.append((_ALL_OPCODES[e.op], flat(e)))

    emit(expr)
    return out


def to_ctypes(expr: Expr):
    """The program as an RmSceneOp array (ctypes) and its length."""
    from ._native import RmSceneOp
    ops = compile_ops(expr)
    arr = (RmSceneOp * len(ops))()
    for i, (op, f) in enumerate(ops):
        arr[i].op, arr[i].arg = op, 0
        for j, v in enumerate(f):
            arr[i].f[j] = v
    return arr, len(ops)


# ---- registration -----------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class _Registered:
    info: SceneInfo
    expr: Expr


_reg_lock = threading.Lock()
_registered: Dict[int, _Registered] = {}


def register_scene(name: str, expr: Expr, *, category: str = "custom", description: str = "", lipschitz: float = 1.0,
                   camera_position: Optional[Sequence[float]] = None,
                   camera_target: Optional[Sequence[float]] = None) -> SceneInfo:
    """Register `expr` under `name` (a new scene program of the library; no GPU needed).  ValueError when the name
    normalises (lower case, spaces removed) to a catalogue scene's or another registered scene's name, or the library
    rejects the program."""
    from . import _native
    if not isinstance(expr, Expr):
        raise TypeError("expr must be a scene expression (scene_program.sd_* / op_*)")
    if not isinstance(name, str) or not name.strip():
        raise ValueError("a scene needs a non-empty name")
    if camera_target is not None and camera_position is None:
        raise ValueError("camera_target needs camera_position")
    arr, n = to_ctypes(expr)
    with _reg_lock:
        registry.check_new_scene_name(name)
        try:
            sid = _native.scene_program_create(arr, n, float(lipschitz))
        except _native.RmError as e:
            if e.code != -6:
                raise
            raise ValueError(f"scene {name!r}: {e}") from None
        info = SceneInfo(sid, name, category, description,
                         tuple(float(v) for v in camera_position) if camera_position is not None else None,
                         tuple(float(v) for v in (camera_target if camera_target is not None else (0.0, 0.0, 0.0)))
                         if camera_position is not None else None,
                         float(lipschitz))
        _registered[sid] = _Registered(info, expr)
        registry.add_program_scene(info)
    return info


def unregister_scene(name: str) -> None:
    """Remove a registered scene (exact name, or its normalised form) and destroy its program.  KeyError if none."""
    from . import _native
    with _reg_lock:
        info = registry.remove_program_scene(name)
        _registered.pop(info.id, None)
        _native.scene_program_destroy(info.id)


def twin_name(scene) -> str:
    """The name a catalogue scene's twin is registered under."""
    return f"{_catalogue_scene(scene).name} (program)"


def _catalogue_scene(scene) -> SceneInfo:
    if isinstance(scene, SceneInfo):
        return scene
    if isinstance(scene, str):
        return registry.get_scene_by_name(scene)
    return registry.SCENES[int(scene)]


def register_twin(scene) -> SceneInfo:
    """Register the twin (catalogue_twins) of a catalogue scene -- its id, name or record -- as "<name> (program)" with
    the scene's Lipschitz bound and suggested camera; returns the record, the existing one if it is registered already.
    KeyError for a scene without a twin."""
    base = _catalogue_scene(scene)
    twins = catalogue_twins()
    if base.id not in twins:
        raise KeyError(f"catalogue scene {base.name!r} has no twin program")
    name = twin_name(base)
    found = registry.find_program_scene(name)
    if found is not None:
        return found
    return register_scene(name, twins[base.id], category=base.category,
                          description=f"program twin of the catalogue scene {base.name}", lipschitz=base.lipschitz,
                          camera_position=base.camera_position, camera_target=base.camera_target)


def registered_scenes() -> List[SceneInfo]:
    with _reg_lock:
        return [r.info for r in _registered.values()]


def expression_of(name: str) -> Expr:
    info = registry.find_program_scene(name)
    if info is None:
        raise KeyError(f"no registered scene {name!r}")
    return _registered[info.id].expr


# ---- scene files -------------------------------------------------------------------------------------------------------
# {"scenes": [{"name": ..., "sdf": <expression>, "category": ..., "description": ..., "lipschitz": ...,
#              "camera_position": [x, y, z], "camera_target": [x, y, z]}, ...]}

def scene_entry(name: str, expr: Expr, **meta) -> dict:
    d = {"name": name, "sdf": expr.to_json()}
    for k in ("category", "description", "lipschitz", "camera_position", "camera_target"):
        if meta.get(k) is not None:
            v = meta[k]
            d[k] = list(v) if isinstance(v, (tuple, list)) else v
    return d


def save_scene_file(path: str, scenes: Iterable) -> None:
    """Write registered scenes (names or SceneInfo records) to a scene file."""
    entries = []
    for s in scenes:
        name = s.name if isinstance(s, SceneInfo) else s
        info = registry.find_program_scene(name)
        if info is None:
            raise KeyError(f"no registered scene {name!r}")
        entries.append(scene_entry(info.name, _registered[info.id].expr, category=info.category,
                                   description=info.description, lipschitz=info.lipschitz,
                                   camera_position=info.camera_position, camera_target=info.camera_target))
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"scenes": entries}, f, indent=1)


def load_scene_file(path: str) -> List[SceneInfo]:
    """Register every scene of a scene file; returns their records."""
    with open(path, encoding="utf-8") as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or not isinstance(doc.get("scenes"), list):
        raise ValueError(f"{path}: a scene file is {{\"scenes\": [...]}}")
    out = []
    for e in doc["scenes"]:
        extra = set(e) - {"name", "sdf", "category", "description", "lipschitz", "camera_position", "camera_target"}
        if extra:
            raise ValueError(f"{path}: scene {e.get('name')!r}: unknown field(s) {sorted(extra)}")
        out.append(register_scene(e["name"], expr_from_json(e["sdf"]), category=e.get("category", "custom"),
                                  description=e.get("description", ""), lipschitz=e.get("lipschitz", 1.0),
                                  camera_position=e.get("camera_position"), camera_target=e.get("camera_target")))
    return out


__all__ = ["Expr", "sd_sphere", "sd_box", "sd_plane", "sd_cylinder", "sd_torus", "sd_capsule", "sd_capped_torus", "sd_cone",
           "op_union", "op_subtract", "op_intersect", "op_smooth_union", "op_smooth_subtract", "op_smooth_intersect",
           "op_translate", "op_repeat", "op_round", "op_onion", "expr_from_json", "dumps", "loads", "compile_ops",
           "register_scene", "unregister_scene", "registered_scenes", "expression_of", "scene_entry", "save_scene_file",
           "load_scene_file", "catalogue_expressions", "op_scale", "op_limited_repeat", "sd_menger_cross", "sd_gyroid",
           "catalogue_twins", "register_twin", "twin_name", "op_rotate", "op_turn", "op_mirror"]
