"""The error contract of the C ABI as a table: an invalid or degenerate call per early return of the host layer
(csrc/rm_capi.hip, the march's host side csrc/rm_frame.hip, the gather csrc/rm_gather.hip and the entry points below the kernels of the other csrc/rm_*.hip), the code it returns and -- where the wording is stable -- a piece of rm_last_error().  Which
check fires FIRST when several would is part of the contract (no device before a bad argument in rm_render, a bad
scene before no device in rm_interval_*), so rows combine faults on purpose.

The rows of CPU_ROWS return before the library looks for a device and run everywhere; NO_DEVICE_ROWS run on hosts
without a GPU; DEVICE_ROWS (marked gpu) sit behind the device check.  Every row returns before a kernel launch and no
row hands the library a pointer it would use on the device."""
import ctypes
import math

import numpy as np
import pytest

from conftest import gpu_count
from raymarch_algo_compare_amd import _native

OK, BAD_SCENE, BAD_STRATEGY, BAD_DIMS, NO_DEVICE, E_HIP, BAD_ARG, E_RCCL = 0, -1, -2, -3, -4, -5, -6, -7
NO_PROGRAM = _native.RM_SCENE_PROGRAM_BASE + 1000000      # an id rm_scene_program_create has not handed out
NO_INTERVAL = 10                                          # Mandelbulb: a catalogue scene without an interval form
vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
ref = ctypes.byref


def _desc(scene=0, strategy=0, w=16, h=8, **kw):
    return _native.make_desc(scene, strategy, [0.0] * 14, w, h, **kw)


def _timing(repeats, warmup=0):
    t = _native.RmTiming()
    t.repeats, t.warmup = repeats, warmup
    return t


class _Bufs:
    """Host arrays big enough for every row that passes one (n <= 16 elements of up to 24 bytes)."""

    def __init__(self):
        self.a = np.zeros(64)
        self.b = np.zeros(64)
        self.c = np.zeros(64)
        self.d = np.zeros(64)

    def p(self, name):
        return getattr(self, name).ctypes.data_as(dp)

    def v(self, name):
        return getattr(self, name).ctypes.data_as(vp)


B = _Bufs()


def _outputs(**kw):
    o = _native.RmOutputs()
    for k, v in kw.items():
        setattr(o, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
    return o


def _three(**kw):
    return _outputs(depth=B.a, iters=B.b, hit=B.c, **kw)


def _sphere_op():
    from raymarch_algo_compare_amd import scene_program as sp
    return sp.to_ctypes(sp.sd_sphere(1.0))


# ---- rows that return before the device check -------------------------------------------------------------------------
# (name, call(L) -> code, expected code, substring of rm_last_error() or None)
def _cpu_rows():
    rows = []
    add = lambda *r: rows.append(r)      # noqa: E731
    for what, scene, text in (("unknown scene", 99, "scene 99 has no interval extension"),
                              ("negative scene", -1, "has no interval extension"),
                              ("no interval form", NO_INTERVAL, "scene 10 has no interval extension"),
                              ("unknown program", NO_PROGRAM, f"scene program {NO_PROGRAM} does not exist")):
        add(f"interval_sdf_eval: {what}", lambda L, s=scene: L.rm_interval_sdf_eval(s, None, None, 4, None, None), BAD_SCENE, text)
        add(f"interval_march_rays: {what}", lambda L, s=scene: L.rm_interval_march_rays(s, None, None, None, 4, None, None, None),
            BAD_SCENE, text)
        add(f"interval_render: {what}",
            lambda L, s=scene: L.rm_interval_render(ref(_desc(s, w=0)), ref(_native.interval_config(tol=-1.0)), None, None, None, None, None),
            BAD_SCENE, text)
    bad_cfgs = [(dict(tol=-1.0), "RmIntervalConfig: tol is negative"), (dict(t_max=math.nan), "RmIntervalConfig: t_max is not finite"),
                (dict(bound_radius=math.inf), "bound_radius is not finite"), (dict(max_steps=-1), "max_steps is negative"),
                (dict(max_steps=_native.RM_INTERVAL_MAX_STEPS + 1), "above the ceiling"), (dict(growth=0.5), "growth must be > 1")]
    for kw, text in bad_cfgs:
        add(f"interval_march_rays: config {kw}",
            lambda L, kw=kw: L.rm_interval_march_rays(0, ref(_native.interval_config(**kw)), None, None, 4, None, None, None), BAD_ARG, text)
        add(f"interval_render: config {kw}",
            lambda L, kw=kw: L.rm_interval_render(ref(_desc(w=0)), ref(_native.interval_config(**kw)), None, None, None, None, None),
            BAD_ARG, text)

    def reserved(L):
        c = _native.interval_config()
        c.reserved = 1
        return L.rm_interval_march_rays(0, ref(c), None, None, 4, None, None, None)
    add("interval_march_rays: reserved set", reserved, BAD_ARG, "reserved must be 0")
    add("interval_render: NULL desc", lambda L: L.rm_interval_render(None, None, None, None, None, None, None), BAD_ARG, "desc is NULL")
    for what, kw in (("zero width", dict(w=0)), ("zero height", dict(h=0)), ("negative row0", dict(row0=-1, rows=1)),
                     ("negative rows", dict(rows=-1)), ("rows beyond height", dict(row0=4, rows=5)),
                     # the interval path takes no band-cyclic slices: rows beyond the height stay an error with bands set
                     ("banded rows beyond height", dict(row0=0, rows=12, band_rows=4, band_stride=3, band_offset=1))):
        add(f"interval_render: {what}", lambda L, kw=kw: L.rm_interval_render(ref(_desc(**kw)), None, None, None, None, None, ref(_timing(0))),
            BAD_DIMS, "bad frame slice")
    add("interval_render: frame too large",
        lambda L: L.rm_interval_render(ref(_desc(w=65536, h=65536, rows=0)), None, None, None, None, None, ref(_timing(0))), BAD_DIMS, "frame too large")
    for what, t in (("repeats 0", _timing(0)), ("repeats above the maximum", _timing(_native.RM_MAX_TIMED + 1)), ("negative warmup", _timing(1, -1))):
        add(f"interval_render: timing {what}", lambda L, t=t: L.rm_interval_render(ref(_desc()), None, None, None, None, None, ref(t)),
            BAD_ARG, "timing: repeats must be 1..256, warmup >= 0")
    add("render_batch_outputs: NULL outputs", lambda L: L.rm_render_batch_outputs(None, -1, None, None, None, None, None), BAD_ARG,
        "outputs record is NULL")
    for field in ("t_raw", "final_sdf", "block_var"):
        add(f"render_batch_outputs: {field} set",
            lambda L, f=field: L.rm_render_batch_outputs(None, -1, None, None, ref(_outputs(**{f: B.a})), None, None), BAD_ARG,
            "batches return depth, iters, hit and evals only")
    sid = ctypes.c_int32(-7)
    ops, nops = _sphere_op()
    add("scene_program_create: NULL id", lambda L: L.rm_scene_program_create(ops, nops, 1.0, None), BAD_ARG, "scene_id is NULL")
    for lip in (0.0, -1.0, math.nan, math.inf):
        add(f"scene_program_create: lipschitz {lip}", lambda L, v=lip: L.rm_scene_program_create(ops, nops, v, ref(sid)), BAD_ARG,
            "lipschitz must be finite and > 0")
    add("scene_program_create: NULL ops", lambda L: L.rm_scene_program_create(None, 1, 1.0, ref(sid)), BAD_ARG, "scene program: ops is NULL")
    add("scene_program_create: no ops", lambda L: L.rm_scene_program_create(ops, 0, 1.0, ref(sid)), BAD_ARG, "scene program: program length 0")

    def bad_opcode(L):
        bad = (_native.RmSceneOp * 1)()
        bad[0].op = 10000
        return L.rm_scene_program_create(bad, 1, 1.0, ref(sid))
    add("scene_program_create: opcode out of range", bad_opcode, BAD_ARG, "opcode 10000 out of range")
    add("scene_program_destroy: unknown program", lambda L: L.rm_scene_program_destroy(NO_PROGRAM), BAD_SCENE,
        f"scene program {NO_PROGRAM} does not exist")
    add("scene_program_destroy: a catalogue id", lambda L: L.rm_scene_program_destroy(0), BAD_SCENE, "scene program 0 does not exist")
    add("set_queue_capacity: negative", lambda L: L.rm_set_queue_capacity(-1), BAD_ARG, "negative queue capacity")
    f = ctypes.c_float()
    add("last_queue_marks: NULL push", lambda L: L.rm_last_queue_marks(None, ref(f)), BAD_ARG, "NULL output")
    add("last_queue_marks: NULL pop", lambda L: L.rm_last_queue_marks(ref(f), None), BAD_ARG, "NULL output")
    add("long_ray_marks: NULL", lambda L: L.rm_long_ray_marks(None), BAD_ARG, "NULL output")
    add("runtime_info: NULL", lambda L: L.rm_runtime_info(None), BAD_ARG, "out is NULL")
    add("comm_destroy: nothing to destroy", lambda L: L.rm_comm_destroy(), OK, None)
    # rm_intrinsic_features: seglen is a length (csrc/rm_features.h); 2 sets of 3 chords, the message names the element
    ts, res = np.linspace(0.0, 1.0, 160), (_native.RmIntrinsicFeatures * 2)()
    for what, i, v in (("NaN", 4, math.nan), ("negative", 5, -1.0), ("-0.0", 0, -0.0), ("-inf", 2, -math.inf)):
        seg = np.ones(6)
        seg[i] = v
        add(f"intrinsic_features: seglen {what}",
            lambda L, seg=seg: L.rm_intrinsic_features(0, 2, 4, B.p("a"), 1e-4, 3, B.p("b"), seg.ctypes.data_as(dp), 160, ts.ctypes.data_as(dp),
                                                       res, None, None, None), BAD_ARG, f"rm_intrinsic_features: seglen[{i}] is NaN or negative")
    return rows


CPU_ROWS = _cpu_rows()


def _run(row):
    name, call, want, text = row
    L = _native.load()
    rc = call(L)
    assert rc == want, (name, rc, L.rm_last_error())
    if text is not None:
        assert text.encode() in L.rm_last_error(), (name, L.rm_last_error())


@pytest.mark.parametrize("row", CPU_ROWS, ids=[r[0] for r in CPU_ROWS])
def test_returns_before_the_device_check(row):
    _run(row)


def test_the_rejected_program_id_was_not_written():
    """a failed rm_scene_program_create leaves *scene_id alone and registers nothing"""
    L = _native.load()
    sid = ctypes.c_int32(-7)
    assert L.rm_scene_program_create(None, 1, 1.0, ref(sid)) == BAD_ARG and sid.value == -7


def test_interval_supported_is_an_answer_not_a_code():
    L = _native.load()
    assert [L.rm_interval_supported(s) for s in (0, NO_INTERVAL, 99, -1, NO_PROGRAM)] == [1, 0, 0, 0, 0]
    ops, nops = _sphere_op()
    sid = ctypes.c_int32(-1)
    assert L.rm_scene_program_create(ops, nops, 1.0, ref(sid)) == OK and sid.value >= _native.RM_SCENE_PROGRAM_BASE
    assert L.rm_interval_supported(sid.value) == 1
    assert L.rm_scene_program_destroy(sid.value) == OK
    assert L.rm_interval_supported(sid.value) == 0
    assert L.rm_scene_program_destroy(sid.value) == BAD_SCENE


# ---- without a device: everything else is RM_E_NO_DEVICE, whatever else is wrong with the call -------------------------
def _no_device_rows():
    d, t, st = _desc(scene=99, strategy=99, w=0), _timing(0), _native.RmStats()
    return [
        ("init", lambda L: L.rm_init(0)),
        ("device_info", lambda L: L.rm_device_info(None)),
        ("sdf_eval", lambda L: L.rm_sdf_eval(99, None, 4, None)),
        ("march_rays", lambda L: L.rm_march_rays(99, 99, None, None, None, 4, None, None, None, None)),
        ("march_rays_team", lambda L: L.rm_march_rays_team(99, 99, None, None, None, 4, None, None, None, None)),
        ("render", lambda L: L.rm_render(ref(d), None, None, None, None, None, None, None, ref(t))),
        ("render: NULL desc", lambda L: L.rm_render(None, None, None, None, None, None, None, None, None)),
        ("render_outputs", lambda L: L.rm_render_outputs(None, None, None, None)),
        ("render_device", lambda L: L.rm_render_device(None, None, None, None, None, None)),
        ("read_stats", lambda L: L.rm_read_stats(None, None, None)),
        ("bench_device", lambda L: L.rm_bench_device(None, None, None, None, None, None)),
        ("render_batch", lambda L: L.rm_render_batch(None, -1, None, None, None, None, None, None, None)),
        ("render_batch_outputs", lambda L: L.rm_render_batch_outputs(None, -1, None, None, ref(_outputs()), ref(st), None)),
        ("comm_init", lambda L: L.rm_comm_init(None, 0, -1)),
        ("assemble_frame", lambda L: L.rm_assemble_frame(0, -1, 0, -1, 0, 3, None, None, None)),
        ("gather_frame", lambda L: L.rm_gather_frame(None, None, None, None, None, None, None, None)),
        ("gather_frame_root", lambda L: L.rm_gather_frame_root(None, None, None, None, None, None, None, -1, None)),
        ("set_pass_timing", lambda L: L.rm_set_pass_timing(1)),
        ("get_pass_ms", lambda L: L.rm_get_pass_ms(None, None, None)),
        ("alloc_frame", lambda L: L.rm_alloc_frame(0, 0, None, None, None)),
        ("free_frame", lambda L: L.rm_free_frame(None, None, None)),
        ("copy_frame_to_host", lambda L: L.rm_copy_frame_to_host(0, 0, None, None, None, None, None, None)),
        ("debug_poison_queues", lambda L: L.rm_debug_poison_queues(0, ref(ctypes.c_uint32()))),
        ("debug_math_eval", lambda L: L.rm_debug_math_eval(-1, None, None, 4, 0, None, None)),
        ("debug_set_trace", lambda L: L.rm_debug_set_trace(1)),
        ("debug_get_trace", lambda L: L.rm_debug_get_trace(None, 0, None, None, None, 0, None)),
        ("stream_create", lambda L: L.rm_stream_create(None)),
        ("stream_synchronize", lambda L: L.rm_stream_synchronize(None)),
        ("stream_destroy", lambda L: L.rm_stream_destroy(None)),
        ("bench_store_path", lambda L: L.rm_bench_store_path(0, 0, None, None, None, None)),
        # the interval calls look for the device once the scene, the configuration, the slice and the timing are in order
        ("interval_sdf_eval", lambda L: L.rm_interval_sdf_eval(0, None, None, 4, None, None)),
        ("interval_march_rays", lambda L: L.rm_interval_march_rays(0, None, None, None, 4, None, None, None)),
        ("interval_render", lambda L: L.rm_interval_render(ref(_desc()), None, None, None, None, None, ref(_timing(1)))),
        ("interval_render: nothing to do", lambda L: L.rm_interval_render(ref(_desc(rows=0)), None, None, None, None, None, None)),
    ]


NO_DEVICE_ROWS = _no_device_rows()


@pytest.mark.parametrize("row", NO_DEVICE_ROWS, ids=[r[0] for r in NO_DEVICE_ROWS])
def test_every_other_entry_point_reports_no_device(row):
    if gpu_count() > 0:
        pytest.skip("a GPU is present; the no-device behaviour is checked on CPU-only hosts")
    name, call = row
    L = _native.load()
    assert call(L) == NO_DEVICE, (name, L.rm_last_error())
    if name != "init":
        assert b"rm_init" in L.rm_last_error(), name


def test_calls_that_need_no_device_succeed_without_one():
    if gpu_count() > 0:
        pytest.skip("a GPU is present; the no-device behaviour is checked on CPU-only hosts")
    L = _native.load()
    L.rm_shutdown()                                   # nothing to shut down
    f, g4 = ctypes.c_float(-1.0), (ctypes.c_float * 4)(-1.0, -1.0, -1.0, -1.0)
    assert L.rm_last_queue_marks(ref(f), ref(f)) == OK and f.value == 0.0
    assert L.rm_long_ray_marks(g4) == OK and list(g4) == [0.0] * 4
    assert L.rm_set_queue_capacity(0) == OK


# ---- with a device: the argument checks behind the device check --------------------------------------------------------
def _frame(L, w=16, rows=8):
    p = [vp(), vp(), vp()]
    _native.check(L.rm_alloc_frame(w, rows, *[ref(q) for q in p]))
    return p


def _device_rows():
    rows = []
    add = lambda *r: rows.append(r)      # noqa: E731
    cfg = _native.march_config()
    st = _native.RmStats()
    add("device_info: NULL", lambda L, F: L.rm_device_info(None), BAD_ARG, "out is NULL")
    add("init: same device again", lambda L, F: L.rm_init(0), OK, None)
    add("init: another device", lambda L, F: L.rm_init(1), BAD_ARG, "already initialised on device 0")
    # per-point / per-ray calls: scene, strategy, configuration, n == 0 before the buffers, buffers
    add("sdf_eval: scene out of range", lambda L, F: L.rm_sdf_eval(99, None, 0, None), BAD_SCENE, "scene_id 99 out of range")
    add("sdf_eval: negative scene", lambda L, F: L.rm_sdf_eval(-1, None, 0, None), BAD_SCENE, "scene_id -1 out of range")
    add("sdf_eval: unknown program", lambda L, F: L.rm_sdf_eval(NO_PROGRAM, None, 0, None), BAD_SCENE,
        f"scene program {NO_PROGRAM} does not exist (never created, or destroyed)")
    add("sdf_eval: n == 0", lambda L, F: L.rm_sdf_eval(0, None, 0, None), OK, None)
    add("sdf_eval: NULL points", lambda L, F: L.rm_sdf_eval(0, None, 4, B.p("a")), BAD_ARG, "NULL buffer")
    add("sdf_eval: NULL out", lambda L, F: L.rm_sdf_eval(0, B.p("a"), 4, None), BAD_ARG, "NULL buffer")
    for team, fn in ((False, "rm_march_rays"), (True, "rm_march_rays_team")):
        call = lambda L, *a, fn=fn: getattr(L, fn)(*a)      # noqa: E731
        add(f"{fn}: scene out of range", lambda L, F, c=call: c(L, 99, 99, None, None, None, 0, None, None, None, None), BAD_SCENE, "out of range")
        add(f"{fn}: strategy out of range", lambda L, F, c=call: c(L, 10, 13, None, None, None, 0, None, None, None, None), BAD_STRATEGY,
            "strategy_id 13 out of range")
        add(f"{fn}: negative strategy", lambda L, F, c=call: c(L, 10, -1, None, None, None, 0, None, None, None, None), BAD_STRATEGY,
            "strategy_id -1 out of range")
        add(f"{fn}: NULL cfg", lambda L, F, c=call: c(L, 10, 0, None, None, None, 0, None, None, None, None), BAD_ARG, "cfg is NULL")
        add(f"{fn}: n == 0", lambda L, F, c=call: c(L, 10, 0, ref(cfg), None, None, 0, None, None, None, None), OK, None)
        add(f"{fn}: NULL final_sdf", lambda L, F, c=call: c(L, 10, 0, ref(cfg), B.p("a"), B.p("b"), 2, B.v("c"), B.p("c"), B.v("d"), None),
            BAD_ARG, "NULL buffer")
        add(f"{fn}: NULL origins", lambda L, F, c=call: c(L, 10, 0, ref(cfg), None, B.p("b"), 2, B.v("c"), B.p("c"), B.v("d"), B.p("d")),
            BAD_ARG, "NULL buffer")
    add("rm_march_rays_team: scene without a team form", lambda L, F: L.rm_march_rays_team(0, 0, ref(cfg), None, None, 0, None, None, None, None),
        BAD_SCENE, "scene 0 has no wavefront-team form")
    # frames: the descriptor first, then the outputs
    add("render_outputs: NULL desc", lambda L, F: L.rm_render_outputs(None, None, None, None), BAD_ARG, "desc is NULL")
    for what, d, code, text in (
            ("scene out of range", _desc(scene=20, strategy=99), BAD_SCENE, "scene_id 20 out of range"),
            ("unknown program", _desc(scene=NO_PROGRAM), BAD_SCENE, "does not exist"),
            ("strategy out of range", _desc(strategy=13, w=0), BAD_STRATEGY, "strategy_id 13 out of range"),
            ("zero width", _desc(w=0), BAD_DIMS, "bad frame slice"),
            ("zero height", _desc(h=0), BAD_DIMS, "bad frame slice"),
            ("negative row0", _desc(row0=-4, rows=4), BAD_DIMS, "bad frame slice"),
            ("negative rows", _desc(rows=-1), BAD_DIMS, "bad frame slice"),
            ("rows beyond height", _desc(row0=4, rows=8), BAD_DIMS, "bad frame slice: 16x8 rows [4,12)"),
            ("frame too large", _desc(w=65536, h=65536, rows=0), BAD_DIMS, "frame too large"),
            ("tile_rows", _desc(tile_rows=3), BAD_ARG, "tile_rows must be 0, 4 or 1"),
            ("tile_order_mode", _desc(tile_order_mode=5), BAD_ARG, "tile_order_mode must be 0 .. 4"),
            ("eval_mode", _desc(eval_mode=3), BAD_ARG, "eval_mode must be 0, 1 or 2"),
            ("pipeline", _desc(pipeline=3), BAD_ARG, "pipeline must be 0, 1 or 2"),
            ("band row beyond height", _desc(h=48, row0=0, rows=24, band_rows=4, band_stride=3, band_offset=2), BAD_DIMS, "band-cyclic slice maps row"),
            ("band offset", _desc(h=48, row0=0, rows=4, band_rows=4, band_stride=2, band_offset=2), BAD_ARG, "band_offset must be < band_stride")):
        add(f"render_outputs: {what}", lambda L, F, d=d: L.rm_render_outputs(ref(d), None, None, None), code, text)
        add(f"render_device: {what}", lambda L, F, d=d: L.rm_render_device(ref(d), None, None, None, None, None), code, text)
        add(f"bench_device: {what}", lambda L, F, d=d: L.rm_bench_device(ref(d), None, None, None, None, None), code, text)
        add(f"render_batch_outputs: {what}", lambda L, F, d=d: L.rm_render_batch_outputs(ref(d), -1, None, None, ref(_outputs()), None, None), code, text)
        add(f"gather_frame: {what}", lambda L, F, d=d: L.rm_gather_frame(ref(d), None, None, None, None, None, None, None), code, text)
        add(f"gather_frame_root: {what}", lambda L, F, d=d: L.rm_gather_frame_root(ref(d), None, None, None, None, None, None, -1, None), code, text)
    add("render_outputs: NULL outputs", lambda L, F: L.rm_render_outputs(ref(_desc()), None, None, None), BAD_ARG, "depth, iters and hit are required")
    add("render_outputs: NULL hit", lambda L, F: L.rm_render_outputs(ref(_desc()), ref(_outputs(depth=B.a, iters=B.b)), None, None), BAD_ARG,
        "depth, iters and hit are required")
    add("render: NULL maps", lambda L, F: L.rm_render(ref(_desc()), None, None, None, None, None, None, None, None), BAD_ARG,
        "depth, iters and hit are required")
    add("render_outputs: final_sdf without march.full", lambda L, F: L.rm_render_outputs(ref(_desc()), ref(_three(final_sdf=B.d)), None, None),
        BAD_ARG, "final_sdf requires march.full = 1")
    add("render_outputs: block_var with row0 % 4 != 0",
        lambda L, F: L.rm_render_outputs(ref(_desc(row0=2, rows=4)), ref(_three(block_var=B.d)), None, None), BAD_ARG, "block_var requires row0 % 4 == 0")
    for what, t in (("repeats 0", _timing(0)), ("repeats above the maximum", _timing(_native.RM_MAX_TIMED + 1)), ("negative warmup", _timing(1, -1))):
        text = "timing: repeats must be 1..256, warmup >= 0"
        add(f"render_outputs: timing {what}", lambda L, F, t=t: L.rm_render_outputs(ref(_desc(w=4, h=4)), ref(_three()), None, ref(t)), BAD_ARG, text)
        add(f"bench_device: timing {what}", lambda L, F, t=t: L.rm_bench_device(ref(_desc()), F[0], F[1], F[2], ref(st), ref(t)), BAD_ARG, text)
        add(f"bench_store_path: timing {what}", lambda L, F, t=t: L.rm_bench_store_path(16, 8, F[0], F[1], F[2], ref(t)), BAD_ARG, None)
        add(f"interval_render: timing {what}", lambda L, F, t=t: L.rm_interval_render(ref(_desc()), None, None, None, None, None, ref(t)), BAD_ARG, text)
    add("render_device: NULL maps", lambda L, F: L.rm_render_device(ref(_desc()), None, None, None, None, None), BAD_ARG,
        "device output pointers are required")
    add("render_device: NULL hit", lambda L, F: L.rm_render_device(ref(_desc()), F[0], F[1], None, None, None), BAD_ARG,
        "device output pointers are required")
    add("read_stats: NULL out", lambda L, F: L.rm_read_stats(None, None, None), BAD_ARG, "out is NULL")
    add("bench_device: NULL timing", lambda L, F: L.rm_bench_device(ref(_desc()), F[0], F[1], F[2], None, None), BAD_ARG,
        "device outputs and timing are required")
    add("bench_device: NULL maps", lambda L, F: L.rm_bench_device(ref(_desc()), None, None, None, None, ref(_timing(1))), BAD_ARG,
        "device outputs and timing are required")
    # batches
    cams = np.zeros((3, 14))
    cp = cams.ctypes.data_as(dp)
    add("render_batch_outputs: negative nframes", lambda L, F: L.rm_render_batch_outputs(ref(_desc()), -1, cp, None, ref(_three()), None, None),
        BAD_ARG, "bad batch arguments")
    add("render_batch_outputs: NULL cams", lambda L, F: L.rm_render_batch_outputs(ref(_desc()), 2, None, None, ref(_three()), None, None),
        BAD_ARG, "bad batch arguments")
    add("render_batch_outputs: NULL maps", lambda L, F: L.rm_render_batch_outputs(ref(_desc()), 2, cp, None, ref(_outputs()), None, None),
        BAD_ARG, "bad batch arguments")
    add("render_batch: NULL maps", lambda L, F: L.rm_render_batch(ref(_desc()), 2, cp, None, None, None, None, None, None), BAD_ARG,
        "bad batch arguments")
    add("render_batch_outputs: tile_order_mode on a batch",
        lambda L, F: L.rm_render_batch_outputs(ref(_desc(tile_order_mode=2)), 0, None, None, ref(_outputs()), None, None), BAD_ARG,
        "tile_order_mode is not supported for batches")
    add("render_batch_outputs: no frames", lambda L, F: L.rm_render_batch_outputs(ref(_desc()), 0, None, None, ref(_outputs()), None, None), OK, None)

    def mixed_full(L, F):
        cfgs = (_native.RmMarchConfig * 3)(_native.march_config(full=True), _native.march_config(full=True), _native.march_config(full=False))
        return L.rm_render_batch_outputs(ref(_desc(w=4, h=4)), 3, cp, cfgs, ref(_three()), None, None)
    add("render_batch_outputs: mixed march.full", mixed_full, BAD_ARG, "all frames of a batch must share march.full")
    add("render_batch_outputs: batch too large",
        lambda L, F: L.rm_render_batch_outputs(ref(_desc(w=32768, h=32768)), 3, cp, None, ref(_three()), None, None), BAD_DIMS, "batch too large")
    # communicator and shards
    add("comm_init: NULL id", lambda L, F: L.rm_comm_init(None, 1, 0), BAD_ARG, "bad communicator arguments")
    add("comm_init: rank outside the world", lambda L, F: L.rm_comm_init(ctypes.create_string_buffer(128), 2, 2), BAD_ARG, "bad communicator arguments")
    add("assemble_frame: element size", lambda L, F: L.rm_assemble_frame(1, 8, 16, 8, 0, 2, F[0], F[1], None), BAD_ARG, "bad assemble arguments")
    add("assemble_frame: NULL source", lambda L, F: L.rm_assemble_frame(1, 8, 16, 8, 0, 4, None, F[1], None), BAD_ARG, "bad assemble arguments")
    add("assemble_frame: cyclic plan", lambda L, F: L.rm_assemble_frame(2, 12, 16, 6, 1, 4, F[0], F[1], None), BAD_DIMS, "band-cyclic plan needs")
    add("assemble_frame: shards too short", lambda L, F: L.rm_assemble_frame(2, 8, 16, 3, 0, 4, F[0], F[1], None), BAD_DIMS, "the shards do not cover the frame")
    add("gather_frame: NULL buffer", lambda L, F: L.rm_gather_frame(ref(_desc()), F[0], F[1], F[2], F[0], F[1], None, None), BAD_ARG, "NULL buffer")
    add("gather_frame: no communicator", lambda L, F: L.rm_gather_frame(ref(_desc()), F[0], F[1], F[2], F[0], F[1], F[2], None), E_RCCL,
        "no communicator: call rm_comm_init() first")
    add("gather_frame_root: NULL shard", lambda L, F: L.rm_gather_frame_root(ref(_desc()), F[0], F[1], None, None, None, None, 0, None), BAD_ARG,
        "NULL shard buffer")
    add("gather_frame_root: no communicator", lambda L, F: L.rm_gather_frame_root(ref(_desc()), F[0], F[1], F[2], None, None, None, -1, None), E_RCCL,
        "no communicator: call rm_comm_init() first")
    # small state
    n32, f4 = ctypes.c_int32(), (ctypes.c_float * 8)()
    add("get_pass_ms: NULL count", lambda L, F: L.rm_get_pass_ms(None, None, f4), BAD_ARG, "NULL output")
    add("get_pass_ms: NULL times", lambda L, F: L.rm_get_pass_ms(None, ref(n32), None), BAD_ARG, "NULL output")
    add("get_pass_ms: pass timing off", lambda L, F: (L.rm_set_pass_timing(0), L.rm_get_pass_ms(None, ref(n32), f4))[1], BAD_ARG,
        "pass timing is off (rm_set_pass_timing)")
    q = [vp(), vp(), vp()]
    add("alloc_frame: zero width", lambda L, F: L.rm_alloc_frame(0, 8, ref(q[0]), ref(q[1]), ref(q[2])), BAD_ARG, "bad arguments")
    add("alloc_frame: NULL result", lambda L, F: L.rm_alloc_frame(16, 8, ref(q[0]), ref(q[1]), None), BAD_ARG, "bad arguments")
    add("free_frame: nothing", lambda L, F: L.rm_free_frame(None, None, None), OK, None)
    add("debug_math_eval: fn out of range", lambda L, F: L.rm_debug_math_eval(len(_native.MATH_FNS), None, None, 0, 0, None, None), BAD_ARG,
        "fn 15 out of range [0, 15)")
    add("debug_math_eval: negative fn", lambda L, F: L.rm_debug_math_eval(-1, None, None, 0, 0, None, None), BAD_ARG, "fn -1 out of range")
    add("debug_math_eval: no live lane", lambda L, F: L.rm_debug_math_eval(0, None, None, 0, 0, None, None), BAD_ARG, "lane_mask is 0: no live lane")
    add("debug_math_eval: n == 0", lambda L, F: L.rm_debug_math_eval(0, None, None, 0, 1, None, None), OK, None)
    add("debug_math_eval: NULL a", lambda L, F: L.rm_debug_math_eval(_native.MATH_FNS["LOG"], None, None, 4, 1, B.p("b"), None), BAD_ARG, "NULL buffer")
    add("debug_math_eval: NULL second input", lambda L, F: L.rm_debug_math_eval(_native.MATH_FNS["POW"], B.p("a"), None, 4, 1, B.p("b"), None),
        BAD_ARG, "NULL buffer")
    add("debug_math_eval: NULL second output", lambda L, F: L.rm_debug_math_eval(_native.MATH_FNS["SINCOS"], B.p("a"), None, 4, 1, B.p("b"), None),
        BAD_ARG, "NULL buffer")
    add("debug_get_trace: NULL count", lambda L, F: L.rm_debug_get_trace(None, 0, None, None, None, 0, None), BAD_ARG, "nrecords is NULL")
    add("stream_create: NULL", lambda L, F: L.rm_stream_create(None), BAD_ARG, "stream is NULL")
    add("stream_destroy: NULL", lambda L, F: L.rm_stream_destroy(None), OK, None)
    add("stream_synchronize: the library's stream", lambda L, F: L.rm_stream_synchronize(None), OK, None)
    add("bench_store_path: zero width", lambda L, F: L.rm_bench_store_path(0, 8, F[0], F[1], F[2], ref(_timing(1))), BAD_ARG, "bad arguments")
    add("bench_store_path: NULL timing", lambda L, F: L.rm_bench_store_path(16, 8, F[0], F[1], F[2], None), BAD_ARG, "bad arguments")
    # the interval oracle behind the device check
    add("interval_sdf_eval: n == 0", lambda L, F: L.rm_interval_sdf_eval(0, None, None, 0, None, None), OK, None)
    add("interval_sdf_eval: NULL out_hi", lambda L, F: L.rm_interval_sdf_eval(0, B.p("a"), B.p("b"), 2, B.p("c"), None), BAD_ARG, "NULL buffer")
    add("interval_march_rays: n == 0", lambda L, F: L.rm_interval_march_rays(0, None, None, None, 0, None, None, None), OK, None)
    add("interval_march_rays: NULL t", lambda L, F: L.rm_interval_march_rays(0, None, B.p("a"), B.p("b"), 2, None, B.v("c"), B.v("d")), BAD_ARG,
        "NULL buffer")
    add("interval_render: no rows", lambda L, F: L.rm_interval_render(ref(_desc(rows=0)), None, None, None, None, None, None), OK, None)
    add("interval_render: NULL hit", lambda L, F: L.rm_interval_render(ref(_desc(w=4, h=2)), None, B.v("a"), None, None, None, None), BAD_ARG,
        "depth and hit are required")
    return rows


DEVICE_ROWS = _device_rows()


@pytest.fixture(scope="module")
def frame(hip):
    L = hip.load()
    p = _frame(L)
    yield p
    hip.check(L.rm_free_frame(*p))


@pytest.mark.gpu
@pytest.mark.parametrize("row", DEVICE_ROWS, ids=[r[0] for r in DEVICE_ROWS])
def test_argument_checks_behind_the_device_check(hip, frame, row):
    name, call, want, text = row
    L = hip.load()
    rc = call(L, frame)
    assert rc == want, (name, rc, L.rm_last_error())
    if text is not None:
        assert text.encode() in L.rm_last_error(), (name, L.rm_last_error())


@pytest.mark.gpu
def test_cpu_rows_hold_with_a_device_too(hip):
    """the rows that return before the device check give the same answers once a device is bound"""
    for row in CPU_ROWS:
        _run(row)


@pytest.mark.gpu
def test_shard_checks_on_a_communicator_of_one(hip, frame):
    """a shard descriptor that is not this rank's part of the plan, and the root checks of the gather-to-root form"""
    L = hip.load()
    ident = ctypes.create_string_buffer(128)
    hip.check(L.rm_comm_unique_id(ident))
    hip.check(L.rm_comm_init(ident.raw, 1, 0))
    try:
        F = frame
        assert L.rm_comm_init(ident.raw, 1, 0) == BAD_ARG and b"a communicator exists already" in L.rm_last_error()
        for bad, text in ((_desc(row0=0, rows=4), b"contiguous shard of rank 0 must be rows [0, 8)"),
                          (_desc(row0=4, rows=4), b"contiguous shard of rank 0 must be rows [0, 8)"),
                          (_desc(h=48, row0=0, rows=16, band_rows=4, band_stride=3, band_offset=1), b"band-cyclic shard does not match the communicator")):
            assert L.rm_gather_frame(ref(bad), F[0], F[1], F[2], F[0], F[1], F[2], None) == BAD_DIMS
            assert text in L.rm_last_error()
            assert L.rm_gather_frame_root(ref(bad), F[0], F[1], F[2], F[0], F[1], F[2], 0, None) == BAD_DIMS
            assert text in L.rm_last_error()
        for root in (-1, 1):
            assert L.rm_gather_frame_root(ref(_desc()), F[0], F[1], F[2], F[0], F[1], F[2], root, None) == BAD_ARG
            assert b"outside the communicator of 1" in L.rm_last_error()
        assert L.rm_gather_frame_root(ref(_desc()), F[0], F[1], F[2], F[0], None, F[2], 0, None) == BAD_ARG
        assert b"the root needs the three full-frame buffers" in L.rm_last_error()
    finally:
        hip.check(L.rm_comm_destroy())
