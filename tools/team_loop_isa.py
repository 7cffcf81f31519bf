#!/usr/bin/env python3
"""team_loop_isa.py -- static instruction mix of the wavefront-team trip loops of a kernel.

A team wave's trip loop (rm_kernels.h team_trips, rm_pipeline.h team role) is the innermost loop that holds the
team's exchange barrier (s_barrier).  For every such loop of the named kernels this prints the instruction counts of
one pass: vector (of them fp64 and v_cndmask), LDS, scalar, literal s_mov (64-bit fp constants rebuilt in SGPRs),
branches, s_nop, scratch accesses and SGPR spill lane moves (v_writelane / v_readlane).  The part column is read from
the loop's exchange write; it is meaningful only for per-part loops (Scene::kPartLoops), not for a single loop whose part
is a runtime value.

Input: the assembly the build keeps next to each object with KEEP_ASM=1 (after the rm_peephole.py pass), e.g.

  make -C raymarch_algo_compare_amd/csrc DEV=1 DEVSCENES=10 KEEP_ASM=1
  python tools/team_loop_isa.py raymarch_algo_compare_amd/_build_dev/scene_10.s            # the team kernel of the split
                                                                                           # single launch, the fused bench
                                                                                           # kernel and march_rays_team_kernel,
                                                                                           # then the three side by side
  python tools/team_loop_isa.py scene_10.s --kernel march_rays_team_kernel --kernel resume_team_kernel
  python tools/team_loop_isa.py scene_10.s --json
  python tools/team_loop_isa.py scene_10.s --kernel pipeline_team_kernel --blocks          # the loops block by block
  python tools/team_loop_isa.py scene_10.s --kernel pipeline_team_kernel --without bb.158,bb.162,BB53_169
  python tools/team_loop_isa.py scene_10.s --kernel pipeline_team_kernel --path BB53_227,bb.228,bb.229,...      # executed per trip

The counts are static: one pass through every block of the loop.  The libm forms of a team wave branch on ballots
(rm_band_needed<true>, rm_math_trig.h), so what a wave issues is the blocks its live lanes make it enter.  --blocks lists
a loop's blocks with their counts and branch targets; --without drops the named blocks (the ones a given wave jumps
over, read off that listing) and prints the mix of the path that is left as a second row.  --path is the same from the
other side: it names the blocks a given wave DOES run (for a lone lane in the common bands: the chain of fall-throughs
from the loop header, none of the join's alternatives it cannot reach) and prints their mix as the "executed" row -- the
instructions issued per trip -- with `taken`, the branches on that path whose target is not the next block of the
path (a taken branch costs a lone wave ~47 cycles, one that falls through ~1: tools/ubench/branch_cost.hip).  Block
lists that were used are kept with the listings under profiles/.  A --path that no wave can walk -- a block whose
successors (its branch targets and, unless it ends in s_branch, the next block in layout) do not hold the next block of
the path -- is an error, not a row.  --fallthrough finds the path itself for loops laid out for it: from the header, no
conditional branch taken but the back edge and the one to the latch block that holds it, every unconditional one
followed; a loop in which that walk does not come back to the header gets no row.

A fall-through block is named bb.<n> after the compiler's comment, unique within one kernel only: give --kernel a name
that matches one.  Block names change with every build; a name that matches no block of the reported loops is an error,
not a shorter sum.
"""
from __future__ import annotations

import argparse
import json
import re
import sys

BENCH_KERNEL = "_ZN2rm15pipeline_kernelINS_15SceneMandelbulbENS_13StratStandardELi4ELb1ELb0EEEvNS_10KernelArgsE"
TEAM_KERNEL = "_ZN2rm20pipeline_team_kernelINS_15SceneMandelbulbENS_13StratStandardELb0EEEvNS_10KernelArgsE"
ALONE_KERNEL = "_ZN2rm22march_rays_team_kernelINS_15SceneMandelbulbENS_13StratStandardEEE"      # (a prefix: its arguments follow)
DEFAULT_KERNELS = [TEAM_KERNEL, BENCH_KERNEL, ALONE_KERNEL]
XCH_WRITE = re.compile(r"^\s*ds_write2st64_b64\b.*?(?:offset0:(\d+))?\s+offset1:(\d+)")
LITERAL = re.compile(r"^\s*s_mov_b32\s+s\d+,\s*(0x[0-9a-fA-F]+|-?\d+)\s*$")


def functions(lines):
    """name -> (first line, last line) of every function body in the file"""
    out, name, start = {}, None, 0
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, start = m.group(1), i
        elif name and re.match(r"^\s*\.Lfunc_end\d+:", ln):
            out[name] = (start, i)
            name = None
    return out


def instructions(lines, a, b):
    for ln in lines[a:b + 1]:
        s = ln.split(";", 1)[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        yield s


def is_literal_mov(ins):
    m = LITERAL.match(ins)
    if not m:
        return False
    v = int(m.group(1), 0)
    return not (-16 <= v <= 64)         # inline constants need no literal


def loop_mix(lines, ranges):
    c = dict(static=0, vector=0, fp64=0, cndmask=0, lds=0, scalar=0, literal_s_mov=0, branches=0, s_nop=0,
             scratch=0, spill_lane_moves=0)
    for ins in (x for a, b in ranges for x in instructions(lines, a, b)):
        op = ins.split()[0]
        c["static"] += 1
        if op.startswith("v_"):
            c["vector"] += 1
            if "_f64" in op:
                c["fp64"] += 1
            if op.startswith("v_cndmask"):
                c["cndmask"] += 1
            if op in ("v_writelane_b32", "v_readlane_b32"):
                c["spill_lane_moves"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("scratch_") or (op.startswith("buffer_") and "off" in ins and "s[0:3]" in ins):
            c["scratch"] += 1
        elif op.startswith("s_"):
            c["scalar"] += 1
            if op.startswith("s_branch") or op.startswith("s_cbranch"):
                c["branches"] += 1
            if op == "s_nop":
                c["s_nop"] += 1
            if is_literal_mov(ins):
                c["literal_s_mov"] += 1
    return c


BLOCK = re.compile(r"^(?:\.LBB(\d+_\d+):|; %bb\.(\d+):)(.*)$")
IN_LOOP = re.compile(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r"=>\s*This (Inner )?Loop Header: Depth=(\d+)")


def team_loops(lines, a, b):
    """Innermost loops (the compiler's own loop annotations of the blocks) that hold an s_barrier: the line ranges
    of their blocks, in layout order"""
    blocks = []                 # (first line, last line, innermost loop header or None, is inner header)
    cur = None
    for i in range(a, b + 1):
        m = BLOCK.match(lines[i])
        if not m:
            continue
        if cur:
            blocks.append((cur[0], i - 1, cur[1], cur[2]))
        name = m.group(1) or None
        loop, inner = None, False
        lm = IN_LOOP.search(m.group(3))
        if lm:
            loop = lm.group(1)
        nxt = lines[i + 1] if i + 1 <= b else ""
        hm = HEADER.search(nxt)
        if hm and name:
            loop, inner = name, bool(hm.group(1))
        cur = (i, loop, inner)
    if cur:
        blocks.append((cur[0], b, cur[1], cur[2]))
    inner_headers = {blk[2] for blk in blocks if blk[3]}
    loops = {}
    for lo, hi, loop, _ in blocks:
        if loop in inner_headers:
            loops.setdefault(loop, []).append((lo, hi))
    def has_barrier(ranges):
        return any(re.match(r"^\s*s_barrier\b", lines[k]) for lo, hi in ranges for k in range(lo, hi + 1))

    out = [(h, ranges) for h, ranges in loops.items() if has_barrier(ranges)]
    out += two_entry_loops(lines, [blk for blk in blocks if blk[2] not in inner_headers], has_barrier)
    return sorted(out, key=lambda t: t[1][0][0])


BRANCH = re.compile(r"^\s*s_(c?branch\w*)\s+\.LBB(\d+_\d+)\b")


def two_entry_loops(lines, blocks, has_barrier):
    """Trip loops the compiler does not annotate: a loop whose count sits in its test (the short last trip, rm_kernels.h
    team_trips) comes out with two entries, and the loop comments name natural loops only.  Found from the branches
    themselves: among the blocks that share their innermost annotated loop, that loop's header aside, every cycle (a
    strongly connected component of more than one block, or a block that branches to itself) that holds an s_barrier.
    Named after its first block in layout order."""
    label = {}
    for k, (lo, hi, loop, _) in enumerate(blocks):
        m = BLOCK.match(lines[lo])
        if m.group(1):
            label[m.group(1)] = k
    succ = {k: set() for k in range(len(blocks))}
    for k, (lo, hi, loop, _) in enumerate(blocks):
        falls = True
        for i in range(lo, hi + 1):
            ins = lines[i].split(";", 1)[0]
            m = BRANCH.match(ins)
            if m:
                t = label.get(m.group(2))
                if t is not None and blocks[t][2] == loop and loop is not None and m.group(2) != loop:
                    succ[k].add(t)
                falls = m.group(1) != "branch"
            elif re.match(r"^\s*(s_endpgm|s_setpc_b64)\b", ins):
                falls = False
            elif ins.strip() and not ins.strip().endswith(":") and not ins.strip().startswith("."):
                falls = True
        if falls and k + 1 < len(blocks) and blocks[k + 1][2] == loop and loop is not None and blocks[k + 1][0] == hi + 1:
            m = BLOCK.match(lines[blocks[k + 1][0]])
            if m.group(1) != loop:
                succ[k].add(k + 1)
    # Tarjan, iterative
    index, low, on, stack, comps, n = {}, {}, set(), [], [], [0]
    for root in succ:
        if root in index:
            continue
        work = [(root, iter(sorted(succ[root])))]
        index[root] = low[root] = n[0]; n[0] += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = n[0]; n[0] += 1; stack.append(w); on.add(w)
                    work.append((w, iter(sorted(succ[w]))))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop(); on.discard(w); comp.append(w)
                        if w == v:
                            break
                    comps.append(sorted(comp))
    out = []
    for comp in comps:
        if len(comp) == 1 and comp[0] not in succ[comp[0]]:
            continue
        ranges = [(blocks[k][0], blocks[k][1]) for k in comp]
        if has_barrier(ranges):
            m = BLOCK.match(lines[ranges[0][0]])
            out.append((m.group(1) or f"line{ranges[0][0]}", ranges))
    return out


def resources(lines, name):
    """registers, spills and private segment of the kernel (its .amdhsa_kernel block and code object metadata)"""
    out = {}
    text = "\n".join(lines)
    m = re.search(rf"^\s*\.amdhsa_kernel {re.escape(name)}\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    if m:
        for key in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size"):
            k = re.search(rf"\.amdhsa_{key}\s+(\d+)", m.group(1))
            if k:
                out[key] = int(k.group(1))
    m = re.search(rf"\.name:\s+{re.escape(name)}\n", text)
    if m:
        after = text[m.end():m.end() + 1000]          # the metadata map's keys after .name (alphabetical order)
        for key in ("sgpr_spill_count", "vgpr_spill_count"):
            k = re.search(rf"\.{key}:\s+(\d+)", after)
            if k:
                out[key] = int(k.group(1))
    return out


def block_name(lines, lo):
    """BB<f>_<n> for a labelled block, bb.<n> for one the compiler only comments (; %bb.<n>:)"""
    m = BLOCK.match(lines[lo])
    return f"BB{m.group(1)}" if m.group(1) else f"bb.{m.group(2)}"


def block_rows(lines, ranges):
    """per block of a loop: its name, its mix and the labels its branches name"""
    rows = []
    for lo, hi in ranges:
        targets = [m.group(2) for m in (BRANCH.match(x.split(";", 1)[0]) for x in lines[lo:hi + 1]) if m]
        rows.append((block_name(lines, lo), loop_mix(lines, [(lo, hi)]), ["BB" + t for t in targets]))
    return rows


def fallthrough_path(lines, ranges):
    """the blocks a wave runs from the loop's header if it takes no conditional branch but the one back to the header
    (or to the latch block that holds that branch), and every unconditional one: the way of a lone lane in the common bands through loops laid out for it (the rare
    bodies sit out of line behind branches that are not taken; rm_math_trig.h ONE RARE-PATH TEST PER CALL)"""
    names = [block_name(lines, lo) for lo, hi in ranges]
    header = names[0]

    def latch_targets(k):
        return ["BB" + m.group(2) for m in (BRANCH.match(x.split(";", 1)[0]) for x in lines[ranges[k][0]:ranges[k][1] + 1]) if m]
    path, k = [], 0
    while k is not None and names[k] not in path:
        path.append(names[k])
        lo, hi = ranges[k]
        nxt = k + 1 if k + 1 < len(names) else None
        for x in lines[lo:hi + 1]:
            m = BRANCH.match(x.split(";", 1)[0])
            if not m:
                continue
            t = "BB" + m.group(2)
            if m.group(1) == "branch":
                nxt = names.index(t) if t in names else None
            elif t == header:
                nxt = None
                break
            elif t in names and header in latch_targets(names.index(t)):      # "more trips": on to the latch
                nxt = names.index(t)
                break
        k = nxt
    return set(path)


def taken_branches(lines, ranges, path, strict=True):
    """branches a wave takes when it runs exactly the blocks of `path`, in layout order, round and round: a block whose
    last instruction is an unconditional branch, or one of whose conditional branches names a block of the path other
    than the next one in layout (the loop's back edge among them); conditional branches to blocks off the path fall through"""
    names = [block_name(lines, lo) for lo, hi in ranges]
    on = [n for n in names if n in path]
    taken = 0
    for lo, hi in ranges:
        n = block_name(lines, lo)
        if n not in path:
            continue
        nxt = on[(on.index(n) + 1) % len(on)]
        layout_next = names[names.index(n) + 1] if names.index(n) + 1 < len(names) else None
        targets, falls = [], True
        for x in lines[lo:hi + 1]:
            ins = x.split(";", 1)[0]
            m = BRANCH.match(ins)
            if m:
                targets.append("BB" + m.group(2))
                falls = m.group(1) != "branch"
            elif ins.strip() and not ins.strip().endswith(":") and not ins.strip().startswith("."):
                falls = True
        if nxt in targets and not (falls and nxt == layout_next):
            taken += 1
        elif not (falls and nxt == layout_next):
            if not strict:
                return None
            sys.exit(f"--path cannot be walked: {n} leads to {sorted(set(targets + ([layout_next] if falls and layout_next else [])))}, "
                     f"not to {nxt}, the next block of the path (see --blocks)")
    return taken


def exchange_part(lines, ranges):
    """the team part a loop belongs to, from its exchange write: TeamXch.v[parity][2 * part][lane] and [2 * part + 1],
    one ds_write2st64_b64 whose offsets (units of 64 doubles) are 2 * part and 2 * part + 1"""
    for a, b in ranges:
        for k in range(a, b + 1):
            m = XCH_WRITE.match(lines[k])
            if m:
                o0 = int(m.group(1) or 0)
                if int(m.group(2)) == o0 + 1 and o0 % 2 == 0:
                    return o0 // 2
    return None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help="assembly of a scene object (KEEP_ASM=1 build)")
    ap.add_argument("--kernel", action="append", default=None,
                    help="mangled name or a substring of it (repeatable); default: the split single launch's team kernel, the "
                         "fused bench kernel and march_rays_team_kernel")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    ap.add_argument("--blocks", action="store_true", help="list every loop's blocks: counts and branch targets")
    ap.add_argument("--without", default="", help="comma-separated block names (as --blocks prints them) to leave out: "
                                                  "adds a row with the mix of the remaining path to each loop that holds one")
    ap.add_argument("--path", default="", help="comma-separated block names (as --blocks prints them) that a wave runs: adds an "
                                               "'executed' row with their mix and the branches taken among them to the loop that holds them")
    ap.add_argument("--fallthrough", action="store_true",
                    help="the 'executed' row of every loop for the path that takes no conditional branch but the back edge")
    args = ap.parse_args(argv)
    lines = open(args.asm).read().splitlines()
    funcs = functions(lines)
    wanted = args.kernel or DEFAULT_KERNELS
    without = {w for w in args.without.split(",") if w}
    path = {w for w in args.path.split(",") if w}
    report = {}
    for w in wanted:
        for name, (a, b) in funcs.items():
            if w == name or w in name:
                loops = team_loops(lines, a, b)
                entries = []
                for h, r in loops:
                    L = dict(header="BB" + h, part=exchange_part(lines, r), **loop_mix(lines, r))
                    kept = [(lo, hi) for lo, hi in r if block_name(lines, lo) not in without]
                    if len(kept) < len(r):
                        L["path"] = dict(without=[block_name(lines, lo) for lo, hi in r if (lo, hi) not in kept],
                                         **loop_mix(lines, kept))
                    loop_path = fallthrough_path(lines, r) if args.fallthrough else path
                    on_path = [(lo, hi) for lo, hi in r if block_name(lines, lo) in loop_path]
                    taken = taken_branches(lines, r, loop_path, strict=not args.fallthrough) if on_path else None
                    if taken is not None:       # (--fallthrough: a loop whose fall-through walk does not come back to its header has no such row)
                        L["executed"] = dict(blocks=[block_name(lines, lo) for lo, hi in on_path], taken=taken, **loop_mix(lines, on_path))
                    if args.blocks:
                        L["blocks"] = [dict(name=n, targets=t, **mix) for n, mix, t in block_rows(lines, r)]
                    entries.append(L)
                report[name] = dict(resources=resources(lines, name), loops=entries)
    if not report:
        sys.exit(f"no kernel matches {wanted}")
    # block names change with every build: a name that matches nothing would leave a path row that looks right and is not
    dropped = {n for r in report.values() for L in r["loops"] for n in L.get("path", {}).get("without", [])}
    if without - dropped:
        sys.exit(f"--without names no block of the reported loops: {sorted(without - dropped)} (see --blocks)")
    ran = {n for r in report.values() for L in r["loops"] for n in L.get("executed", {}).get("blocks", [])}
    if path - ran:
        sys.exit(f"--path names no block of the reported loops: {sorted(path - ran)} (see --blocks)")
    if args.json:
        print(json.dumps(report, indent=1))
        return
    cols = ["static", "vector", "fp64", "cndmask", "lds", "scalar", "literal_s_mov", "branches", "s_nop", "scratch",
            "spill_lane_moves"]
    for name, r in report.items():
        print(f"{name}  {r['resources']}")
        print("  loop header    part " + " ".join(f"{c[:8]:>8}" for c in cols))
        for L in r["loops"]:
            part = "?" if L["part"] is None else L["part"]
            print(f"  {L['header']:<13} {part:>4} " + " ".join(f"{L[c]:>8}" for c in cols))
            if "path" in L:
                print(f"  {'  path':<13} {'':>4} " + " ".join(f"{L['path'][c]:>8}" for c in cols) +
                      "   without " + ",".join(L["path"]["without"]))
            if "executed" in L:
                print(f"  {'  executed':<13} {'':>4} " + " ".join(f"{L['executed'][c]:>8}" for c in cols) +
                      f"   taken {L['executed']['taken']}   blocks " + ",".join(L["executed"]["blocks"]))
            for B in L.get("blocks", []):
                print(f"    {B['name']:<11} {'':>4} " + " ".join(f"{B[c]:>8}" for c in cols) + "   -> " + " ".join(B["targets"]))
    if len(report) > 1:
        # side by side, per part: static / scalar / literal s_mov of one pass of each kernel's loop
        short = {name: re.sub(r"^_ZN2rm\d+(\w+?)INS_.*$", r"\1", name) for name in report}
        parts = sorted({L["part"] for r in report.values() for L in r["loops"] if L["part"] is not None})
        print("\nstatic / scalar / literal s_mov per pass   " + "   ".join(f"{short[n]:>24}" for n in report))
        for p in parts:
            cells = []
            for n, r in report.items():
                Ls = [L for L in r["loops"] if L["part"] == p]
                cells.append(" + ".join(f"{L['static']} / {L['scalar']} / {L['literal_s_mov']}" for L in Ls) or "-")
            print(f"  part {p:<35} " + "   ".join(f"{c:>24}" for c in cells))


if __name__ == "__main__":
    main()
