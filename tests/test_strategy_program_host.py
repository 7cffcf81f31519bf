"""Strategy programs without a GPU: csrc/rm_strategy_program.h compiled for the host by g++
(tests/native/strategy_program_check.cpp) against the compiled strategies (tests/native/host_check.cpp), the NumPy
machine (strategy_program.run_host) against the oracle, validation, the builder and the ABI."""
import ctypes

import numpy as np
import pytest

import strategy_program_cases as cases
from oracle import oracle
from raymarch_algo_compare_amd import _native
from raymarch_algo_compare_amd import strategy_program as sp


@pytest.fixture(scope="module")
def L():
    return cases.native()


@pytest.fixture(scope="module")
def LC():
    return cases.host_compiled()


@pytest.fixture(scope="module")
def scene_rays():
    return {s: cases.rays(s) for s in cases.HOST_SCENES}


@pytest.mark.parametrize("scene", cases.HOST_SCENES)
def test_twins_equal_compiled_strategies(L, LC, scene_rays, scene):
    """march_one<Scene, StratProgram> with each twin == march_one<Scene, StratX>, bit for bit"""
    o, d = scene_rays[scene]
    for name, kid, prog, prm in cases.twin_cases():
        cfgs = list(cases.CONFIGS) + [(0, 1e-4, 100.0)]
        if kid == 6:
            cfgs.append((int(prm.get("overstep_bisection_steps", 16)), 1e-4, 100.0))
        for cfg in cfgs:
            for full in (0, 1):
                a = cases.march_program(L, scene, prog, cfg, full, o, d)
                b = cases.march_compiled(LC, scene, kid, prm, cfg, full, o, d)
                assert cases.same_bits(a, b) == [], (name, cfg, full)
                assert int(a["evals"].max()) < sp.budget(cfg[0])


@pytest.mark.parametrize("scene", cases.HOST_SCENES)
def test_run_host_equals_oracle(scene_rays, scene):
    """run_host(twin, oracle.sdf_eval) == oracle.march_rays(compiled id), bit for bit, on the rays of the check above: all
    of them, both configurations, `full` on and off (the oracle always marches with the tail evaluations, so without
    `full` its final_sdf is not compared: hit, t and iterations do not depend on it)"""
    o, d = scene_rays[scene]
    for name, kid, prog, prm in cases.twin_cases():
        for mi, eps, far in cases.CONFIGS:
            hit, t, it, fs = oracle.march_rays(scene, kid, o, d, mi, eps, far, 1.0, prm or None)
            want = {"hit": hit, "t": t, "iters": it, "final_sdf": fs}
            cfg = {"max_iterations": mi, "hit_threshold": eps, "max_distance": far}
            for full in (True, False):
                a = sp.run_host(prog, lambda p: oracle.sdf_eval(scene, p), o, d, cfg, full=full)
                keys = ("hit", "iters", "t", "final_sdf") if full else ("hit", "iters", "t")
                assert cases.same_bits(a, want, keys) == [], (name, mi, eps, full)


@pytest.mark.parametrize("scene", [0, 12])
def test_new_strategy_host_build_equals_run_host(L, scene_rays, scene):
    o, d = scene_rays[scene]
    prog = sp.understep_relax()
    for cfg in cases.CONFIGS:
        for full in (0, 1):
            a = cases.march_program(L, scene, prog, cfg, full, o, d)
            b = sp.run_host(prog, lambda p: oracle.sdf_eval(scene, p), o, d,
                            {"max_iterations": cfg[0], "hit_threshold": cfg[1], "max_distance": cfg[2]}, full=bool(full))
            assert cases.same_bits(a, b, ("hit", "iters", "t", "final_sdf", "evals")) == [], (cfg, full)
    assert a["hit"].any() and not a["hit"].all()


def test_budget_ends_a_program_that_would_not(L, scene_rays):
    """The probe finishes itself as a HIT ten evaluations past the budget: every ray must be a miss at the budget."""
    o, d = scene_rays[0]
    prog = sp.budget_probe(10)
    for mi in (4, 0, -3):
        a = cases.march_program(L, 0, prog, (mi, 1e-4, 100.0), 1, o[:200], d[:200])
        b = sp.run_host(prog, lambda p: oracle.sdf_eval(0, p), o[:200], d[:200], {"max_iterations": mi}, full=True)
        for r in (a, b):
            assert not r["hit"].any()
            assert (r["evals"] == sp.budget(mi)).all()
            assert (r["iters"] == sp.budget(mi)).all()
            assert (r["t"] == 0.0).all()
        assert cases.same_bits(a, b, ("hit", "iters", "t", "final_sdf", "evals")) == []


def test_a_ray_its_program_finishes_at_the_budget_keeps_its_result(L, scene_rays):
    """status 2 under `full` set in the block of the budget-th evaluation: the program has finished the ray by then, so its
    hit stands (final_sdf = s5, no tail evaluation); one evaluation later it would have been a forced miss"""
    o, d = scene_rays[0]
    for late, hit in ((0, 1), (1, 0)):
        b = sp.StrategyBuilder()
        n = b.state("n")
        with b.init():
            b.evaluate(0.0, 0)
        with b.phase(0):
            b.set(n, n + 1)
            with b.when(n >= b.max_iterations * 8.0 + float(64 + late)):
                b.finish(hit=1, t=3.0, final_sdf=7.0, reeval=True)
            b.evaluate(0.0, 0)
        prog = b.program()
        x = cases.march_program(L, 0, prog, (4, 1e-4, 100.0), 1, o[:64], d[:64])
        y = sp.run_host(prog, lambda p: oracle.sdf_eval(0, p), o[:64], d[:64], {"max_iterations": 4}, full=True)
        assert cases.same_bits(x, y, ("hit", "iters", "t", "final_sdf", "evals")) == []
        assert (x["hit"] == hit).all() and (x["evals"] == sp.budget(4)).all()
        if hit:
            assert (x["t"] == 3.0).all() and (x["final_sdf"] == 7.0).all()


def test_budget_is_clamped_to_the_evaluation_count():
    assert sp.budget(2 ** 31 - 1) == 2 ** 31 - 1 and sp.budget(3) == 88 and sp.budget(-5) == 64


# ---- validation ------------------------------------------------------------------------------------------------------------

I, B = sp.BLOCK_INIT, sp.OP_BLOCK
GOOD = [(B, 0, I, 0, 0, 0.0), (sp.OP["MOV"], 3, sp.LITERAL, 0, 0, 1.0)]
REFUSALS = [
    ([(B, 0, I, 0, 0, 0.0), (25, 0, 0, 0, 0, 0.0)], "unknown opcode 25"),
    ([(B, 0, I, 0, 0, 0.0), (sp.OP["ADD"], 0, 40, 0, 0, 0.0)], "operand a = 40 out of range"),
    ([(B, 0, I, 0, 0, 0.0), (sp.OP["ADD"], 32, 0, 0, 0, 0.0)], "destination 32 out of range"),
    ([(B, 0, I, 0, 0, 0.0), (sp.OP["MOV"], 0, 17, 0, 0, 0.0)], "temporary t1 read before it is written in its block"),
    ([(B, 0, I, 0, 0, 0.0), (sp.OP["MOV"], 17, 0, 0, 0, 0.0), (B, 0, 0, 0, 0, 0.0), (sp.OP["MOV"], 0, 17, 0, 0, 0.0)],
     "temporary t1 read before it is written in its block"),
    ([(B, 0, 0, 0, 0, 0.0), (sp.OP["MOV"], 3, sp.LITERAL, 0, 0, 1.0)], "no init block"),
    ([(B, 0, I, 0, 0, 0.0), (B, 0, 8, 0, 0, 0.0)], "phase 8 above 7"),
    ([(B, 0, I, 0, 0, 0.0), (B, 0, 2, 0, 0, 0.0), (B, 0, 2, 0, 0, 0.0)], "duplicate block of phase 2"),
    ([(B, 0, I, 0, 0, 0.0), (B, 0, I, 0, 0, 0.0)], "duplicate init block"),
    ([(B, 0, I, 0, 0, 0.0), (sp.OP["MOV"], 0, sp.LITERAL, 0, 0, float("inf"))], "constant is not finite"),
    ([(B, 0, I, 0, 0, 0.0), (sp.OP["MOV"], 0, sp.LITERAL, 0, 0, float("nan"))], "constant is not finite"),
    ([(B, 0, I, 0, 0, 0.0)] + [(sp.OP["MOV"], 0, 0, 0, 0, 0.0)] * 257, "too many instructions: more than 256"),
    ([(B, 0, I, 0, 0, 0.0)] + [(sp.OP["MOV"], 0, sp.LITERAL, 0, 0, float(i)) for i in range(65)],
     "too many constants: more than 64"),
    ([(B, 0, I, 0, 0, 0.0), (sp.OP["MOV"], 0, sp.IN_D, 0, 0, 0.0)], "the init block has no evaluated value to read"),
    ([(sp.OP["MOV"], 0, 0, 0, 0, 0.0)], "instruction before the first block marker"),
]


def test_validation_refusals_host_build_and_library(L):
    ok = sp.StrategyProgram(GOOD)
    why = ctypes.create_string_buffer(256)
    counts = (ctypes.c_int32 * 2)()
    assert L.rsp_encode(ok.to_ops(), len(ok), why, 256, counts) == 1 and list(counts) == [1, 1]
    sid = _native.strategy_program_create(ok.to_ops(), len(ok))
    _native.strategy_program_destroy(sid)
    for rows, reason in REFUSALS:
        p = sp.StrategyProgram(rows)
        assert L.rsp_encode(p.to_ops(), len(p), why, 256, counts) == 0, reason
        assert reason in why.value.decode(), (reason, why.value)
        with pytest.raises(_native.RmError) as e:
            _native.strategy_program_create(p.to_ops(), len(p))
        assert e.value.code == _native.RM_E_BAD_ARG and reason in str(e.value), (reason, str(e.value))


def test_ids_and_error_texts_without_a_device():
    # ("ids 13 and 1023 keep today's error text" is asserted on the GPU, tests/test_gpu_strategy_program.py::test_lifetime:
    # every entry point that takes a strategy id asks for the device before it looks at the id, today as before.)
    a = _native.strategy_program_create(sp.StrategyProgram(GOOD).to_ops(), 2)
    b = _native.strategy_program_create(sp.StrategyProgram(GOOD).to_ops(), 2)
    assert _native.RM_STRATEGY_PROGRAM_BASE <= a < b            # monotonic
    _native.strategy_program_destroy(a)
    c = _native.strategy_program_create(sp.StrategyProgram(GOOD).to_ops(), 2)
    assert c > b                                                # never reused
    _native.strategy_program_destroy(b)
    _native.strategy_program_destroy(c)
    with pytest.raises(_native.RmError) as e:
        _native.strategy_program_destroy(a)
    assert e.value.code == _native.RM_E_BAD_STRATEGY and "does not exist" in str(e.value)
    L = _native.load()
    assert L.rm_num_strategies() == 11


def test_abi_of_the_op_record(L):
    assert ctypes.sizeof(_native.RmStrategyOp) == 32 == L.rsp_sizeof_op()
    names = ["op", "dst", "a", "b", "c", "reserved", "k"]
    offs = [0, 4, 8, 12, 16, 20, 24]
    for i, (n, off) in enumerate(zip(names, offs)):
        assert getattr(_native.RmStrategyOp, n).offset == off == L.rsp_offsetof_op(i), n


# ---- the builder -------------------------------------------------------------------------------------------------------------

def test_when_otherwise_lower_to_selects():
    b = sp.StrategyBuilder()
    x = b.state("x")
    with b.init():
        b.evaluate(0.0, 0)
    with b.phase(0):
        with b.when(b.d < 0.0):
            b.set(x, 1.0)
        with b.otherwise():
            b.set(x, 2.0)
        b.finish(hit=x)
    rows = b.program().blocks()[0]
    names = [sp.OPS[r[0]] for r in rows]
    assert names[:4] == ["LT", "SELECT", "NOT", "SELECT"]
    assert "SELECT" in names and all(r[0] < len(sp.OPS) for r in rows)          # no jump exists to lower to
    sdf = lambda p: p[:, 0]
    o = np.array([[-1.0, 0, 0], [1.0, 0, 0]])
    r = sp.run_host(b.program(), sdf, o, np.array([[0, 0, 1.0]] * 2), {"max_iterations": 4})
    assert list(r["hit"]) == [1, 1] and list(r["evals"]) == [1, 1]
    with pytest.raises(ValueError, match="otherwise"):
        with b.phase(1):
            with b.otherwise():
                pass


def test_statements_after_finish_reach_only_the_other_rays():
    b = sp.StrategyBuilder()
    with b.init():
        b.evaluate(0.0, 0)
    with b.phase(0):
        with b.when(b.d < 0.0):
            b.finish(hit=1, t=5.0)
        b.finish(hit=0, t=7.0)
    o = np.array([[-1.0, 0, 0], [1.0, 0, 0]])
    r = sp.run_host(b.program(), lambda p: p[:, 0], o, np.array([[0, 0, 1.0]] * 2), {"max_iterations": 4})
    assert list(r["hit"]) == [1, 0] and list(r["t"]) == [5.0, 7.0]


def test_literals_are_told_apart_by_their_bits_and_expressions_have_no_truth_value():
    b = sp.StrategyBuilder()
    with b.init():
        x = b.where(b.max_iterations > 0.0, 0.0, -0.0)
        rows = b.rows[-2:]
        assert [sp.OPS[r[0]] for r in rows] == ["MOV", "SELECT"]            # the second literal went through a temporary
        assert {str(rows[0][5]), str(rows[1][5])} == {"0.0", "-0.0"}
        with pytest.raises(TypeError, match="truth value"):
            if x:
                pass
        with pytest.raises(TypeError, match="truth value"):
            (b.t > 1.0) and (b.t < 2.0)
        b.finish(hit=0)


def test_temporary_exhaustion_is_reported():
    b = sp.StrategyBuilder()
    with pytest.raises(ValueError, match="more than 16 temporaries"):
        with b.init():
            keep = [b.d + float(i) for i in range(17)]
    b = sp.StrategyBuilder()
    with b.init():
        for i in range(40):           # dropped temporaries return to the pool
            b.set(b.t, b.t + float(i))
        b.finish(hit=0)
    assert {r[1] for r in b.program().blocks()[sp.BLOCK_INIT] if r[1] >= 16} == {16}          # 40 sums, one temporary


def test_json_round_trip_and_twin_arguments():
    for name, prog in sp.strategy_twins().items():
        again = sp.StrategyProgram.from_json(prog.to_json())
        assert again == prog, name
    with pytest.raises(ValueError):
        sp.StrategyProgram.from_json('{"format": "other", "ops": []}')
    with pytest.raises(TypeError):
        sp.strategy_twins(Relaxed={"beta": 1.0})
    assert sp.strategy_twins(Relaxed={"omega": 1.6})["Relaxed"] != sp.strategy_twins()["Relaxed"]
