"""User-defined marching strategies: step programs the library's interpreter runs on the GPU (include/rm_hip.h,
"Strategy programs"; csrc/rm_strategy_program.h).

A program is written with StrategyBuilder -- named state registers, expressions, nested when / otherwise blocks that
lower to selects, finish() and evaluate() -- registered under a name with register_strategy(), and from then on resolved
by that name wherever a strategy name is (registry.get_strategy_by_name, run_once, HipCollector, GPURunner, sweep.py).

    b = StrategyBuilder()
    i = b.state("i")
    with b.init():
        with b.when(b.max_iterations <= 0):
            b.finish(hit=0, reeval=True)
        b.evaluate(0.0, phase=0)
    with b.phase(0):
        b.set(b.iterations, i + 1)
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, final_sdf=b.d)
        b.set(b.t, b.t + b.d * 0.6)                 # understep
        with b.when(b.t > b.max_distance):
            b.finish(hit=0, reeval=True)
        b.set(i, i + 1)
        with b.when(i >= b.max_iterations):
            b.finish(hit=0, reeval=True)
        b.evaluate(b.t, phase=0)
    register_strategy("Understep", b.program())

finish() and evaluate() end the block for the rays they apply to, like a `return`: statements after them reach only the
other rays.  Expressions are emitted where they are written (one instruction per operation, in order), so a state
register read after a set() sees the new value; b.copy(x) takes a snapshot.  A temporary belongs to the Python value that
names it and returns to the block's pool of 16 when that value is dropped (CPython's reference count): a value kept in a
variable keeps its temporary, so a long block drops what it no longer needs (`del ratio`) or computes it where it is used.
Holding on to too many only ever ends in the "more than 16 temporaries" error, never in a wrong program.  Python's
`and` / `or` / `not` / `if` cannot see an expression's value while the program is written and raise TypeError: use
`&`, `|`, `~`, when() and where().

run_host() is a NumPy restatement of the machine (same ops, same operand order of pymax / pymin, same budget), and
strategy_twins() restates five compiled strategies as programs: what the device interpreter is tested against.
"""
from __future__ import annotations

import contextlib
import json
import math
import struct
from typing import Callable, Dict, List, Optional

import numpy as np

OPS = ["MOV", "ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQRT", "PYMAX", "PYMIN", "LT", "LE", "GT", "GE", "EQ", "NE",
       "AND", "OR", "NOT", "SELECT"]
OP = {name: i for i, name in enumerate(OPS)}
OP_BLOCK = 32
_ARGS = {"MOV": 1, "NEG": 1, "ABS": 1, "SQRT": 1, "NOT": 1, "SELECT": 3}      # every other op reads two
MAX_OPS, MAX_CONSTANTS, MAX_STATE, MAX_TEMPS, MAX_PHASES = 256, 64, 16, 16, 8
IN_D, IN_TE, IN_HIT_THRESHOLD, IN_MAX_DISTANCE, IN_MAX_ITERATIONS, IN_LIPSCHITZ = 32, 33, 34, 35, 36, 37
LITERAL = 63
BLOCK_INIT = -1
S_T, S_TE, S_PHASE, S_STATUS, S_HIT, S_FINAL_SDF, S_ITERATIONS = range(7)
FORMAT = "rm-strategy-program-1"


def budget(max_iterations: int) -> int:
    """The evaluation at which a ray is force-finished (include/rm_hip.h)."""
    return min(8 * max(int(max_iterations), 0) + 64, 2 ** 31 - 1)


class StrategyProgram:
    """A list of (op, dst, a, b, c, k) rows: instructions and block markers, as RmStrategyOp takes them."""

    def __init__(self, rows):
        self.rows = [(int(o), int(d), int(a), int(b), int(c), float(k)) for o, d, a, b, c, k in rows]

    def __eq__(self, other):
        return isinstance(other, StrategyProgram) and self.rows == other.rows

    def __len__(self):
        return len(self.rows)

    def to_ops(self):
        from . import _native
        arr = (_native.RmStrategyOp * max(1, len(self.rows)))()
        for r, (o, d, a, b, c, k) in zip(arr, self.rows):
            r.op, r.dst, r.a, r.b, r.c, r.reserved, r.k = o, d, a, b, c, 0, k
        return arr

    def to_json(self) -> str:
        rows = [["BLOCK" if o == OP_BLOCK else OPS[o], d, a, b, c, k] for o, d, a, b, c, k in self.rows]
        return json.dumps({"format": FORMAT, "ops": rows})

    @staticmethod
    def from_json(text: str) -> "StrategyProgram":
        doc = json.loads(text)
        if doc.get("format") != FORMAT:
            raise ValueError(f"not a strategy program (format {doc.get('format')!r}, expected {FORMAT!r})")
        rows = []
        for name, d, a, b, c, k in doc["ops"]:
            if name != "BLOCK" and name not in OP:
                raise ValueError(f"unknown op {name!r}")
            rows.append((OP_BLOCK if name == "BLOCK" else OP[name], d, a, b, c, k))
        return StrategyProgram(rows)

    def blocks(self) -> Dict[int, List[tuple]]:
        """{-1 (init) or phase: its instruction rows}"""
        out, cur = {}, None
        for row in self.rows:
            if row[0] == OP_BLOCK:
                cur = out.setdefault(row[2], [])
            elif cur is not None:
                cur.append(row)
        return out


class Expr:
    """An operand: a register, an input or a literal."""

    def __init__(self, b: "StrategyBuilder", code: int, k: float = 0.0):
        self.b, self.code, self.k = b, code, float(k)

    def _bin(self, op, other, swap=False):
        other = self.b.expr(other)
        return self.b.emit(op, other, self) if swap else self.b.emit(op, self, other)

    def __add__(self, o): return self._bin("ADD", o)
    def __radd__(self, o): return self._bin("ADD", o, True)
    def __sub__(self, o): return self._bin("SUB", o)
    def __rsub__(self, o): return self._bin("SUB", o, True)
    def __mul__(self, o): return self._bin("MUL", o)
    def __rmul__(self, o): return self._bin("MUL", o, True)
    def __truediv__(self, o): return self._bin("DIV", o)
    def __rtruediv__(self, o): return self._bin("DIV", o, True)
    def __neg__(self): return self.b.emit("NEG", self)
    def __abs__(self): return self.b.emit("ABS", self)
    def __lt__(self, o): return self._bin("LT", o)
    def __le__(self, o): return self._bin("LE", o)
    def __gt__(self, o): return self._bin("GT", o)
    def __ge__(self, o): return self._bin("GE", o)
    def __and__(self, o): return self._bin("AND", o)
    def __or__(self, o): return self._bin("OR", o)
    def __invert__(self): return self.b.emit("NOT", self)
    def __bool__(self):
        raise TypeError("an expression has no truth value while the program is written: use & | ~ for and / or / not, "
                        "b.when() / b.where() for a condition")

    def eq(self, o): return self._bin("EQ", o)
    def ne(self, o): return self._bin("NE", o)
    __hash__ = object.__hash__


class StrategyBuilder:
    """Writes a strategy program; see the module's text."""

    def __init__(self):
        self.rows: List[tuple] = []
        self._names: Dict[str, int] = {}
        self._block: Optional[int] = None
        self._done_blocks = set()
        self._free_temps: List[int] = []
        self._live: Optional[Expr] = None        # rays the block has not ended yet (None: all)
        self._conds: List[Optional[Expr]] = []   # the open when / otherwise conditions, each already ANDed with its parents
        self._last_when: List[Optional[Expr]] = [None]    # per nesting level: the latest closed when's own condition
        for name, code in (("t", S_T), ("te", S_TE), ("phase_reg", S_PHASE), ("status", S_STATUS), ("hit", S_HIT),
                           ("final_sdf", S_FINAL_SDF), ("iterations", S_ITERATIONS)):
            setattr(self, name, Expr(self, code))
        self.d, self.te_in = Expr(self, IN_D), Expr(self, IN_TE)
        self.hit_threshold, self.max_distance = Expr(self, IN_HIT_THRESHOLD), Expr(self, IN_MAX_DISTANCE)
        self.max_iterations, self.lipschitz = Expr(self, IN_MAX_ITERATIONS), Expr(self, IN_LIPSCHITZ)

    # ---- registers and operands
    def state(self, name: str) -> Expr:
        """A named state register of the program's own (s7 .. s15): persists between evaluations, zero when a ray starts."""
        if name not in self._names:
            code = 7 + len(self._names)
            if code >= MAX_STATE:
                raise ValueError(f"state register {name!r}: a program has {MAX_STATE - 7} state registers of its own")
            self._names[name] = code
        return Expr(self, self._names[name])

    def expr(self, x) -> Expr:
        if isinstance(x, Expr):
            return x
        if isinstance(x, bool):
            x = 1.0 if x else 0.0
        x = float(x)
        if not math.isfinite(x):
            raise ValueError("a literal must be finite")
        return Expr(self, LITERAL, x)

    def _temp(self) -> int:
        if not self._free_temps:
            raise ValueError(f"block {self._block_name()} needs more than {MAX_TEMPS} temporaries at once: split the "
                             "expression, or keep fewer values alive")
        return self._free_temps.pop(0)

    def _free(self, code: int) -> None:
        if code not in self._free_temps:
            self._free_temps.append(code)
            self._free_temps.sort()

    def _block_name(self) -> str:
        return "init" if self._block == BLOCK_INIT else f"phase {self._block}"

    def _row(self, op: str, dst: int, args) -> None:
        if self._block is None:
            raise ValueError("an instruction outside a block: use `with b.init():` or `with b.phase(n):`")
        args = list(args)
        # one literal value per instruction: any further one goes through a temporary
        lit, keep = None, []
        for x in args:
            if x.code == LITERAL:
                if lit is None or struct.pack("<d", lit) == struct.pack("<d", x.k):      # by bits, as the library: 0.0 is not -0.0
                    lit = x.k
                else:
                    x = self.emit("MOV", x)
            keep.append(x)
        codes = [x.code for x in keep] + [0, 0, 0]
        self.rows.append((OP[op], dst, codes[0], codes[1], codes[2], lit if lit is not None else 0.0))

    def emit(self, op: str, *args) -> Expr:
        """dst <- op(args) into a fresh temporary"""
        args = [self.expr(x) for x in args]
        if len(args) != _ARGS.get(op, 2):
            raise ValueError(f"{op} takes {_ARGS.get(op, 2)} operands")
        dst = 16 + self._temp()
        try:
            self._row(op, dst, args)
        except Exception:
            self._free(dst - 16)
            raise
        return _Temp(self, dst)

    def copy(self, x) -> Expr:
        return self.emit("MOV", x)

    var = copy      # a settable local of the block

    def sqrt(self, x): return self.emit("SQRT", x)
    def pymax(self, a, b): return self.emit("PYMAX", a, b)
    def pymin(self, a, b): return self.emit("PYMIN", a, b)
    def where(self, c, a, b): return self.emit("SELECT", c, a, b)

    # ---- blocks and conditions
    @contextlib.contextmanager
    def _open(self, which: int):
        if self._block is not None:
            raise ValueError("blocks do not nest")
        if which in self._done_blocks:
            raise ValueError("duplicate block")
        self._block = which
        self._done_blocks.add(which)
        self._free_temps = list(range(MAX_TEMPS))
        self._live, self._conds, self._last_when = None, [], [None]
        self.rows.append((OP_BLOCK, 0, which, 0, 0, 0.0))
        try:
            yield self
        finally:
            self._live, self._conds, self._last_when = None, [], [None]
            self._block = None

    def init(self):
        return self._open(BLOCK_INIT)

    def phase(self, n: int):
        if not 0 <= int(n) < MAX_PHASES:
            raise ValueError(f"phase {n} outside 0..{MAX_PHASES - 1}")
        return self._open(int(n))

    def _and(self, a: Optional[Expr], b: Optional[Expr]) -> Optional[Expr]:
        if a is None:
            return b
        if b is None:
            return a
        return a & b

    def _cond(self) -> Optional[Expr]:
        """the rays the next statement applies to (None: all)"""
        return self._and(self._live, self._conds[-1] if self._conds else None)

    @contextlib.contextmanager
    def _nested(self, own: Expr):
        self._conds.append(self._and(self._conds[-1] if self._conds else None, own))
        self._last_when.append(None)
        try:
            yield
        finally:
            self._conds.pop()
            self._last_when.pop()
            self._last_when[-1] = own

    def when(self, cond):
        """The statements of the body apply where `cond` (taken now) is non-zero."""
        return self._nested(cond if isinstance(cond, _Temp) else self.copy(cond))

    def otherwise(self):
        """... and these where the `when` just closed at this level did not apply."""
        own = self._last_when[-1]
        if own is None:
            raise ValueError("otherwise() without a when() just before it")
        return self._nested(~own)

    def set(self, reg: Expr, value) -> None:
        """reg <- value for the rays the statement applies to; reg is a state register or a var()"""
        if not 0 <= reg.code < 32:
            raise ValueError("set() needs a state register or a var()")
        value = self.expr(value)
        c = self._cond()
        if c is None:
            self._row("MOV", reg.code, [value])
        else:
            self._row("SELECT", reg.code, [c, value, reg])

    def _end_block_for_current(self) -> None:
        c = self._cond()
        if c is None:
            self._live = self.copy(0.0)
        else:
            self._live = self._and(self._live, ~c)

    def finish(self, hit=None, t=None, final_sdf=None, reeval: bool = False) -> None:
        """The ray is finished: hit, t (default: as it stands), final_sdf (default 0.0).  reeval: a `full` frame
        evaluates once more at t and reports that value as final_sdf."""
        if t is not None:
            self.set(self.t, t)
        self.set(self.hit, 0.0 if hit is None else hit)
        self.set(self.final_sdf, 0.0 if final_sdf is None else final_sdf)
        self.set(self.status, 2.0 if reeval else 1.0)
        self._end_block_for_current()

    def evaluate(self, te, phase: int) -> None:
        """Evaluate the SDF at ray parameter te next and hand the value to the block of `phase`."""
        if not 0 <= int(phase) < MAX_PHASES:
            raise ValueError(f"phase {phase} outside 0..{MAX_PHASES - 1}")
        self.set(self.te, te)
        self.set(self.phase_reg, float(int(phase)))
        self._end_block_for_current()

    def program(self) -> StrategyProgram:
        if BLOCK_INIT not in self._done_blocks:
            raise ValueError("a program needs an init block")
        n = sum(1 for r in self.rows if r[0] != OP_BLOCK)
        if n > MAX_OPS:
            raise ValueError(f"{n} instructions: a program holds at most {MAX_OPS}")
        consts = {np.float64(r[5]).tobytes() for r in self.rows if r[0] != OP_BLOCK and LITERAL in r[2:5]}
        if len(consts) > MAX_CONSTANTS:
            raise ValueError(f"{len(consts)} distinct literals: a program holds at most {MAX_CONSTANTS}")
        return StrategyProgram(self.rows)


class _Temp(Expr):
    """A temporary that goes back to its block's pool when the last reference to it is dropped."""

    def __init__(self, b: "StrategyBuilder", code: int):
        Expr.__init__(self, b, code)
        self.block = b._block

    def __del__(self):
        try:
            if self.b._block == self.block:
                self.b._free(self.code - 16)
        except Exception:
            pass


# ---- the machine in NumPy ----------------------------------------------------------------------------------------------------

def _apply(op: int, a, b, c):
    one = lambda m: np.where(m, 1.0, 0.0)
    if op == OP["MOV"]: return a.copy()
    if op == OP["ADD"]: return a + b
    if op == OP["SUB"]: return a - b
    if op == OP["MUL"]: return a * b
    if op == OP["DIV"]: return a / b
    if op == OP["NEG"]: return -a
    if op == OP["ABS"]: return np.abs(a)
    if op == OP["SQRT"]: return np.sqrt(a)
    if op == OP["PYMAX"]: return np.where(b > a, b, a)
    if op == OP["PYMIN"]: return np.where(b < a, b, a)
    if op == OP["LT"]: return one(a < b)
    if op == OP["LE"]: return one(a <= b)
    if op == OP["GT"]: return one(a > b)
    if op == OP["GE"]: return one(a >= b)
    if op == OP["EQ"]: return one(a == b)
    if op == OP["NE"]: return one(a != b)
    if op == OP["AND"]: return one((a != 0.0) & (b != 0.0))
    if op == OP["OR"]: return one((a != 0.0) | (b != 0.0))
    if op == OP["NOT"]: return one(a == 0.0)
    if op == OP["SELECT"]: return np.where(a != 0.0, b, c)
    raise ValueError(f"unknown op {op}")


def _iterations(x):
    x = np.where(x > 0.0, x, 0.0)                  # NaN -> 0
    return np.minimum(x, 2147483647.0).astype(np.int64).astype(np.int32)


def run_host(program: StrategyProgram, sdf: Callable, origins, dirs, cfg, full: bool = True) -> dict:
    """The machine of include/rm_hip.h over n rays at once.  sdf: (m, 3) points -> (m,) distances.  cfg: a mapping or
    record with max_iterations, hit_threshold, max_distance, lipschitz.  dirs are normalised as Ray.__init__ does.
    Returns hit (uint8), t, iters (int32), final_sdf, evals (int32)."""
    get = (lambda k, dflt: cfg.get(k, dflt)) if isinstance(cfg, dict) else (lambda k, dflt: getattr(cfg, k, dflt))
    max_it = int(get("max_iterations", 512))
    inputs = {IN_HIT_THRESHOLD: float(get("hit_threshold", 1e-4)), IN_MAX_DISTANCE: float(get("max_distance", 100.0)),
              IN_MAX_ITERATIONS: float(max_it), IN_LIPSCHITZ: float(get("lipschitz", 1.0))}
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    dr = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        # Vec3.length is `** 0.5` on a Python float, i.e. libm's pow (NumPy's power takes a square-root shortcut)
        ln = np.array([x ** 0.5 for x in (dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1] + dr[:, 2] * dr[:, 2]).tolist()], np.float64)
        inv = 1.0 / ln
        dr = np.where((ln < 1e-12)[:, None], 0.0, dr * inv[:, None])
    n = len(o)
    blocks = program.blocks()
    R = np.zeros((32, n))
    nev = np.zeros(n, np.int64)
    tail = np.zeros(n, bool)
    done = np.zeros(n, bool)
    blk = np.full(n, MAX_PHASES, np.int64)
    te = np.zeros(n)
    res = {"hit": np.zeros(n, np.uint8), "t": np.zeros(n), "iters": np.zeros(n, np.int32), "final_sdf": np.zeros(n)}
    lim = budget(max_it)

    def run(rows, idx, d, te_in):
        regs = R[:, idx]
        def operand(code, k):
            if code < 32: return regs[code]
            if code == LITERAL: return np.full(len(idx), k)
            if code == IN_D: return d
            if code == IN_TE: return te_in
            return np.full(len(idx), inputs[code])
        for op, dst, a, b, c, k in rows:
            na = _ARGS.get(OPS[op], 2)
            va = operand(a, k)
            vb = operand(b, k) if na >= 2 else None
            vc = operand(c, k) if na >= 3 else None
            regs[dst] = _apply(op, va, vb, vc)
        R[:, idx] = regs

    def after(idx):
        st = R[S_STATUS, idx]
        go = st == 0.0
        gi = idx[go]
        te[gi] = R[S_TE, gi]
        ph = R[S_PHASE, gi]
        ok = (ph >= 0.0) & (ph < float(MAX_PHASES))
        blk[gi] = np.where(ok, np.where(ok, ph, 0.0).astype(np.int64), MAX_PHASES)
        fi = idx[~go]
        res["hit"][fi] = R[S_HIT, fi] != 0.0
        res["t"][fi] = R[S_T, fi]
        res["final_sdf"][fi] = R[S_FINAL_SDF, fi]
        res["iters"][fi] = _iterations(R[S_ITERATIONS, fi])
        re = (R[S_STATUS, fi] == 2.0) & bool(full)
        te[fi[re]] = res["t"][fi[re]]
        tail[fi[re]] = True
        done[fi[~re]] = True

    with np.errstate(all="ignore"):
        allidx = np.arange(n)
        run(blocks.get(BLOCK_INIT, []), allidx, np.zeros(n), np.zeros(n))
        after(allidx)
        while not done.all():
            idx = np.nonzero(~done)[0]
            p = o[idx] + dr[idx] * te[idx][:, None]
            d = np.asarray(sdf(p), np.float64)
            nev[idx] += 1
            tl = tail[idx]
            ti = idx[tl]
            res["final_sdf"][ti] = d[tl]
            done[ti] = True
            tail[ti] = False
            for ph in range(MAX_PHASES):
                sel = (~tl) & (blk[idx] == ph)
                if sel.any() and ph in blocks:
                    run(blocks[ph], idx[sel], d[sel], te[idx][sel].copy())
            after(idx[~tl])
            at_budget = (~done[idx]) & (nev[idx] >= lim)
            force = at_budget & ~tail[idx]          # (a ray its program finished in this step, tail pending, keeps its result)
            fi = idx[force]
            res["hit"][fi] = 0
            res["t"][fi] = R[S_T, fi]
            res["final_sdf"][fi] = d[force]
            res["iters"][fi] = _iterations(R[S_ITERATIONS, fi])
            done[idx[at_budget]] = True
            tail[idx[at_budget]] = False
    res["evals"] = nev.astype(np.int32)
    return res


# ---- twins of compiled strategies -----------------------------------------------------------------------------------------------

def _begin_loop(b):
    with b.when(b.max_iterations <= 0):
        b.finish(hit=0, reeval=True)
    b.evaluate(b.t, 0)


def _next_iter(b, i):
    b.set(i, i + 1)
    with b.when(i >= b.max_iterations):
        b.finish(hit=0, reeval=True)
    b.evaluate(b.t, 0)


def twin_standard() -> StrategyProgram:
    b = StrategyBuilder()
    i = b.state("i")
    with b.init():
        _begin_loop(b)
    with b.phase(0):
        b.set(b.iterations, i + 1)
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, final_sdf=b.d)
        b.set(b.t, b.t + b.d)
        with b.when(b.t > b.max_distance):
            b.finish(hit=0, reeval=True)
        _next_iter(b, i)
    return b.program()


def twin_relaxed(omega: float = 1.2) -> StrategyProgram:
    b = StrategyBuilder()
    i, prev_d, om = b.state("i"), b.state("prev_d"), b.state("omega")
    with b.init():
        b.set(om, omega)
        _begin_loop(b)
    with b.phase(0):
        b.set(b.iterations, i + 1)
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, final_sdf=b.d)
        with b.when(b.d < 0.0):
            b.set(b.t, b.t + b.d)
            b.set(om, 1.0)
            b.set(prev_d, abs(b.d))
            _next_iter(b, i)
        stp = b.var(b.d * om)
        with b.when((i > 0.0) & ((prev_d + b.d) < prev_d * om)):
            b.set(stp, b.d)
            b.set(om, 1.0)
        b.set(b.t, b.t + stp)
        b.set(prev_d, b.d)
        with b.when(b.t > b.max_distance):
            b.finish(hit=0, reeval=True)
        _next_iter(b, i)
    return b.program()


def twin_auto_relaxed(omega_min=1.0, omega_max=2.0, smoothing=0.7, growth_rate=1.05, decay_rate=0.7,
                      ar_omega_init=1.2) -> StrategyProgram:
    b = StrategyBuilder()
    i, prev_d, om, ema = b.state("i"), b.state("prev_d"), b.state("omega"), b.state("ema")
    with b.init():
        b.set(om, ar_omega_init)
        b.set(ema, 1.0)
        # prev_d starts at 0.0 where the compiled strategy holds +inf: its only reader before the first write is
        # `prev_d > 1e-10 and i > 0`, which i = 0 decides (a literal must be finite)
        _begin_loop(b)
    with b.phase(0):
        b.set(b.iterations, i + 1)
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, final_sdf=b.d)
        with b.when((prev_d > 1e-10) & (i > 0.0)):
            ratio = b.d / prev_d
            b.set(ema, smoothing * ema + (1.0 - smoothing) * ratio)
            with b.when(ema < 0.8):
                b.set(om, b.pymax(omega_min, om * decay_rate))
            with b.otherwise():
                with b.when(ema > 1.0):
                    b.set(om, b.pymin(omega_max, om * growth_rate))
            del ratio
        stp = b.d * om
        with b.when(b.d < 0.0):
            b.set(b.t, b.t + b.d)
            b.set(om, omega_min)
            b.set(prev_d, abs(b.d))
            _next_iter(b, i)
        b.set(b.t, b.t + stp)
        b.set(prev_d, b.d)
        with b.when(b.t > b.max_distance):
            b.finish(hit=0, reeval=True)
        _next_iter(b, i)
    return b.program()


def twin_slope(beta: float = 0.3) -> StrategyProgram:
    b = StrategyBuilder()
    i, r, z, m = b.state("i"), b.state("r"), b.state("z"), b.state("m")

    def loop_head():
        with b.when(i >= b.max_iterations):
            b.finish(hit=0, final_sdf=r)                 # no tail evaluation
        b.set(b.iterations, i + 1)
        with b.when(abs(r) < b.hit_threshold):
            b.finish(hit=1, final_sdf=r)
        with b.when(b.t > b.max_distance):
            b.finish(hit=0, final_sdf=r)
        b.evaluate(b.t + z, 1)

    with b.init():
        b.evaluate(0.0, 0)                               # the pre-loop evaluation r = sdf(ray.at(0))
    with b.phase(0):
        b.set(r, b.d)
        b.set(z, r)
        b.set(m, -1.0)
        loop_head()
    with b.phase(1):
        with b.when(z <= r + abs(b.d)):
            denom = b.te_in - b.t
            M = b.where(denom > 1e-12, (b.d - r) / denom, -1.0)
            b.set(m, (1.0 - beta) * m + beta * M)
            b.set(b.t, b.te_in)
            b.set(r, b.d)
            del denom, M
        with b.otherwise():
            b.set(m, -1.0)
        den = b.var(1.0 - m)
        with b.when(den < 1e-6):
            b.set(den, 1e-6)
        b.set(z, (2.0 * r) / den)
        with b.when(z < 0.0):
            b.set(z, r)
        b.set(i, i + 1)
        del den
        loop_head()
    return b.program()


def twin_overstep_bisect(min_step_factor: float = 0.01, bisection_steps: int = 16) -> StrategyProgram:
    b = StrategyBuilder()
    i, t_near, t_far, t_mid, j = b.state("i"), b.state("t_near"), b.state("t_far"), b.state("t_mid"), b.state("j")
    steps = float(int(bisection_steps))

    def finish_miss():
        b.finish(hit=0, reeval=True)

    def bis_head():
        b.set(t_mid, (t_near + t_far) * 0.5)
        with b.when(j >= steps):
            b.evaluate(t_mid, 2)                         # the final midpoint decides the hit
        b.set(b.iterations, b.iterations + 1)
        b.evaluate(t_mid, 1)

    def after_phase1():
        with b.when(t_far > 0.0):
            b.set(j, 0.0)
            bis_head()
        finish_miss()

    with b.init():
        b.set(t_far, -1.0)
        with b.when(b.max_iterations - steps <= 0.0):
            after_phase1()
        b.evaluate(b.t, 0)
    with b.phase(0):
        b.set(b.iterations, i + 1)
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, final_sdf=b.d)
        with b.when(b.d > 0.0):
            b.set(t_near, b.t)
            b.set(b.t, b.t + b.pymax(b.d, min_step_factor))
        with b.otherwise():
            b.set(t_far, b.t)
            after_phase1()
        with b.when(b.t > b.max_distance):
            finish_miss()
        b.set(i, i + 1)
        with b.when(i >= b.max_iterations - steps):
            after_phase1()
        b.evaluate(b.t, 0)
    with b.phase(1):
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, t=t_mid, final_sdf=b.d)
        with b.when(b.d > 0.0):
            b.set(t_near, t_mid)
        with b.otherwise():
            b.set(t_far, t_mid)
        with b.when((t_far - t_near) < b.hit_threshold):
            b.set(t_mid, (t_near + t_far) * 0.5)
            b.finish(hit=1, t=t_mid, reeval=True)
        b.set(j, j + 1)
        bis_head()
    with b.phase(2):
        b.finish(hit=abs(b.d) < b.hit_threshold * 10.0, t=t_mid, final_sdf=b.d)
    return b.program()


# compiled strategy key -> (twin constructor, its keyword arguments as the reference's constructors name them)
_TWINS = {
    "Standard": (twin_standard, ()),
    "Relaxed": (twin_relaxed, ("omega",)),
    "Heuristic-Auto-Relaxed": (twin_auto_relaxed, ("omega_min", "omega_max", "smoothing", "growth_rate", "decay_rate", "ar_omega_init")),
    "Slope-Auto-Relaxed": (twin_slope, ("beta",)),
    "Overstep-Bisect": (twin_overstep_bisect, ("min_step_factor", "bisection_steps")),
}


def strategy_twins(**ctor) -> Dict[str, StrategyProgram]:
    """{compiled strategy key: its restatement as a program}, constructor arguments baked in as constants.  `ctor`:
    {key: {argument: value}} for the twins that take some, e.g. strategy_twins(Relaxed={"omega": 1.6})."""
    out = {}
    for key, (fn, names) in _TWINS.items():
        kw = dict(ctor.pop(key, {}) or {})
        bad = [k for k in kw if k not in names]
        if bad:
            raise TypeError(f"{key}: unexpected constructor argument {bad[0]!r} (accepted: {list(names)})")
        out[key] = fn(**kw)
    if ctor:
        raise KeyError(f"no twin of {sorted(ctor)[0]!r} (twins: {sorted(_TWINS)})")
    return out


def understep_relax(understep: float = 0.6, omega: float = 1.6, decay: float = 0.9) -> StrategyProgram:
    """A strategy no catalogue entry has: understep until d < 10 * hit_threshold, then relaxed steps with a decaying omega."""
    b = StrategyBuilder()
    i, om = b.state("i"), b.state("omega")

    def bottom(phase):
        with b.when(b.t > b.max_distance):
            b.finish(hit=0, reeval=True)
        b.set(i, i + 1)
        with b.when(i >= b.max_iterations):
            b.finish(hit=0, reeval=True)
        b.evaluate(b.t, phase)

    with b.init():
        b.set(om, omega)
        with b.when(b.max_iterations <= 0):
            b.finish(hit=0, reeval=True)
        b.evaluate(0.0, 0)
    with b.phase(0):
        b.set(b.iterations, i + 1)
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, final_sdf=b.d)
        with b.when(b.d < b.hit_threshold * 10.0):
            b.set(b.t, b.t + b.d)
            bottom(1)
        b.set(b.t, b.t + b.d * understep)
        bottom(0)
    with b.phase(1):
        b.set(b.iterations, i + 1)
        with b.when(abs(b.d) < b.hit_threshold):
            b.finish(hit=1, final_sdf=b.d)
        b.set(b.t, b.t + b.d * om)
        b.set(om, b.pymax(1.0, om * decay))
        bottom(1)
    return b.program()


def budget_probe(extra: int = 10) -> StrategyProgram:
    """Counts its evaluations and would finish as a HIT `extra` evaluations past the budget: the machine must have
    force-finished it as a miss by then."""
    b = StrategyBuilder()
    n = b.state("n")
    with b.init():
        b.evaluate(0.0, 0)
    with b.phase(0):
        b.set(n, n + 1)
        b.set(b.iterations, n)
        with b.when(n >= b.pymax(b.max_iterations, 0.0) * 8.0 + float(64 + extra)):
            b.finish(hit=1, final_sdf=b.d)
        b.evaluate(0.0, 0)
    return b.program()


# ---- registration ----------------------------------------------------------------------------------------------------------------

def register_strategy(name: str, program: StrategyProgram):
    """Validates the program (library, on the host), registers it and makes `name` resolvable wherever a strategy name
    is.  Returns its registry.StrategyInfo (id from RM_STRATEGY_PROGRAM_BASE)."""
    from . import _native, registry
    if not isinstance(program, StrategyProgram):
        raise TypeError("program must be a StrategyProgram (StrategyBuilder.program())")
    registry.check_new_strategy_name(name)
    sid = _native.strategy_program_create(program.to_ops(), len(program))
    info = registry.StrategyInfo(sid, name, name, name, False)
    registry.add_program_strategy(info)
    return info


def unregister_strategy(name: str) -> None:
    from . import _native, registry
    info = registry.remove_program_strategy(name)
    _native.strategy_program_destroy(info.id)
