#!/usr/bin/env python3
"""Compare the final gfx950 assembly of two builds kernel by kernel (CPU only).

    KEEP_ASM=1 make -C raymarch_algo_compare_amd/csrc -j16      # in both trees: keeps _build/<object>.s
    python tools/kernel_isa_diff.py [--by-name] <old>/_build <new>/_build

A refactor of the device headers must leave every kernel as it was.  For every <object>.s that either directory
holds, the kernels (symbols with an .amdhsa_kernel block) are cut out: the text from the kernel's label to its
.Lfunc_end, which holds the instructions and the descriptor block (registers, LDS, scratch, kernarg size).  Kernels
are matched by name, not by position, because the order of template instantiations may differ; the only thing
normalised is the function number in the compiler's local labels (.LBB<n>_<m>, also as BB<n>_<m> in its loop comments,
and .Lfunc_end<n>), and with it the padding between such a label and the comment the compiler aligns behind it.  Only
kernels are compared: a __device__ function that is not inlined would have to be added (today every function is a kernel).  Prints every kernel
that exists on one side only or differs in its instructions or its descriptor; exit status 1 if there is any.

--by-name: for a change that moves kernels between translation units.  A kernel that its object holds on one side only is
looked up by name in every object of the other side (an object that exists on one side only is then no finding by
itself); it must be there exactly once.
"""
import pathlib
import re
import sys

_LABEL = re.compile(r"(?<![\w.$])((?:\.L)?BB|\.Lfunc_end)\d+(?=_\d|:|-)")     # whole tokens only, never part of a symbol
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_END = re.compile(r"^\.Lfunc_end\d+:")
_PAD = re.compile(r"^(\.LBB_\d+:)\s+;")


def kernels(path):
    """{kernel name: (instruction lines, descriptor lines)} of one assembly file"""
    lines = path.read_text().splitlines()
    start = {}                      # symbol -> index of its label line
    out = {}
    name = None
    for i, line in enumerate(lines):
        if line[:1] not in ("", "\t", " ", ".", ";") and ":" in line:
            start[line.split(":", 1)[0]] = i
        m = _KERNEL.match(line)
        if m:
            name, desc0 = m.group(1), i
        elif name and _END.match(line):
            block = [_PAD.sub(r"\1 ;", _LABEL.sub(r"\1", x)) for x in lines[start[name]:i]]
            d0 = desc0 - start[name]
            d1 = next(k for k in range(d0, len(block)) if ".end_amdhsa_kernel" in block[k]) + 1
            out[name] = (block[:d0] + block[d1:], block[d0:d1])
            name = None
    return out


def main(argv):
    by_name = "--by-name" in argv
    argv = [x for x in argv if x != "--by-name"]
    if len(argv) != 3:
        sys.exit(__doc__)
    old, new = pathlib.Path(argv[1]), pathlib.Path(argv[2])
    files = sorted({p.name for d in (old, new) for p in d.glob("*.s") if not p.name.endswith(".raw.s")})
    if not files:
        sys.exit(f"no assembly in {old} or {new}: build with KEEP_ASM=1")
    side = {d: {f: kernels(d / f) for f in files if (d / f).exists()} for d in (old, new)}
    bad = total = moved = 0
    for f in files:
        if not by_name and not (f in side[old] and f in side[new]):
            print(f"{f}: only in {old if f in side[old] else new}")
            bad += 1
            continue
        a, b = side[old].get(f, {}), side[new].get(f, {})
        total += len(a)
        for k in sorted(set(a) | set(b)):
            x, y, where = a.get(k), b.get(k), f
            if by_name and y is None:           # left this object: it must be in exactly one other
                homes = [g for g in side[new] if k in side[new][g]]
                if len(homes) == 1:
                    y, where = side[new][homes[0]][k], f"{f} -> {homes[0]}"
                    moved += 1
            elif by_name and x is None and any(k in ks for ks in side[old].values()):
                continue                        # came from another object: compared from there
            if x is None or y is None:
                what = f"only in {old if x is not None else new}"
            else:
                what = ", ".join(w for w, p, q in (("instructions", x[0], y[0]), ("descriptor", x[1], y[1])) if p != q)
            if what:
                print(f"{where}: {k}: {what}")
                bad += 1
    print(f"{len(files)} objects, {total} kernels" + (f", {moved} in another object" if by_name else "") + f", {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
