#!/usr/bin/env python3
"""ISA peephole over the gfx950 assembly hipcc emits for the kernels (csrc/Makefile runs it between -S and the assembler).

v_cndmask_b32 in its short VOP2 encoding (`v_cndmask_b32_e32 vD, src0, vS1, vcc`) is SERIALIZED ACROSS THE WAVEFRONTS OF A
COMPUTE UNIT on gfx950 when such instructions follow one another: measured (tools/ubench/simd_share.hip) 6 cycles per
instruction with one wave, 8 / 12 / 16 with two / three / four waves on DIFFERENT SIMDs, while the same select in the VOP3
encoding (`v_cndmask_b32_e64 ..., vcc` or with an SGPR-pair mask) costs 5.8 at any wave count -- as do v_bfi, v_cmp, fp64
arithmetic and everything else tried.  The exact libm restatements (rm_math_*.h) are branch-free by design: a trip of the
Mandelbulb SDF holds ~170 selects, half of them shrunk to the VOP2 form by the compiler, in runs (a double is two
selects).  This pass re-encodes them as VOP3 wherever that is legal: src0 a VGPR or an inline constant (VOP3 cannot hold a
32-bit literal on gfx9-class targets; those few stay).  Same operation, same operands, same results -- four more bytes.

--drop-unused-private-segment (the strategy-program objects, csrc/Makefile): a second, separate rewrite of the kernel
descriptors.  render_kernel reads its output pointers with 128-bit scalar loads from the kernel arguments; under scalar
register pressure the allocator's spiller reserves a 16-byte stack slot for such a tuple and then rematerialises the load
at every use instead of spilling it (LLVM's InlineSpiller: the slot is assigned before rematerialisation is tried and is
not given back).  The slot is never read or written -- no machine instruction names it from register allocation on --
but it is no "dead" spill slot either, so the frame keeps it, frame finalisation adds a 4-byte emergency slot beside it,
and the kernel descriptor asks the runtime for 20 (one frame) or 36 (batch: two tuples) bytes of scratch per lane that
nothing touches.  With the flag, a file in which no instruction addresses private memory as such -- no scratch_* or buffer
load / store / atomic, no call or indirect jump, no flat-scratch or private-aperture operand, no dynamic stack -- has the
private segment of every kernel descriptor and of the metadata set to 0 and the segment disabled, which is what the
compiler itself writes for a kernel without a frame.  A file with any such instruction is left exactly as it is.
What the scan does NOT prove by itself: the kernels also hold flat_load / flat_store instructions (the render kernels'
result stores), and a flat access goes to whichever aperture its 64-bit address lies in.  They cannot land in the private
segment because a flat address in the private aperture has to be MADE from a stack object -- the frame index plus
src_private_base -- and the scan refuses that operand; every flat address in these kernels is computed from a pointer of
the kernel arguments (global memory).  The frame objects themselves, the other way to name the segment, are the ones the
compiler's own dump shows no instruction using ("Strategy programs")."""
import re
import sys

INLINE_INT = set(str(i) for i in range(-16, 65))
INLINE_FP = {"0.5", "-0.5", "1.0", "-1.0", "2.0", "-2.0", "4.0", "-4.0", "0.15915494", "0"}
PAT = re.compile(r"^(\s*)v_cndmask_b32_e32(\s+)(v\d+),\s*([^,]+),\s*(v\d+),\s*vcc(\s*(?:;.*)?)$")


def legal_src0(tok: str) -> bool:
    tok = tok.strip()
    return bool(re.fullmatch(r"v\d+", tok)) or tok in INLINE_INT or tok in INLINE_FP


def rewrite(lines):
    changed = kept = 0
    out = []
    for line in lines:
        m = PAT.match(line.rstrip("\n"))
        if m and legal_src0(m.group(4)):
            out.append(f"{m.group(1)}v_cndmask_b32_e64{m.group(2)}{m.group(3)}, {m.group(4).strip()}, {m.group(5)}, vcc{m.group(6)}\n")
            changed += 1
        else:
            if "v_cndmask_b32_e32" in line:
                kept += 1
            out.append(line)
    return out, changed, kept


# anything through which an instruction could reach the private segment, or leave the function for code that could
PRIVATE_USE = re.compile(r"\b(scratch_\w+|buffer_(load|store|atomic)\w*|s_swappc_b64|s_setpc_b64|s_call_b64|flat_scratch\w*|"
                         r"src_private_base|src_private_limit|src_flat_scratch_base\w*)\b")
SEGMENT_SIZE = re.compile(r"^(\s*)(\.amdhsa_private_segment_fixed_size|\.private_segment_fixed_size:)(\s+)(\d+)\s*$")
SEGMENT_ON = re.compile(r"^(\s*\.amdhsa_enable_private_segment\s+)1\s*$")


def drop_unused_private_segment(lines):
    """(lines, kernels rewritten, why not); see the module's text"""
    for line in lines:
        code = line.split(";", 1)[0].split("//", 1)[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            if re.match(r"\s*\.amdhsa_uses_dynamic_stack\s+1", line) or re.match(r"\s*\.uses_dynamic_stack:\s+true", line):
                return lines, 0, "a kernel uses a dynamic stack"
            continue
        m = PRIVATE_USE.search(code)
        if m:
            return lines, 0, f"an instruction may reach private memory ({m.group(0)})"
    out, n = [], 0
    for line in lines:
        m = SEGMENT_SIZE.match(line.rstrip("\n"))
        if m and m.group(4) != "0":
            n += m.group(2).startswith(".amdhsa")
            out.append(f"{m.group(1)}{m.group(2)}{m.group(3)}0\n")
            continue
        m = SEGMENT_ON.match(line.rstrip("\n"))
        out.append(f"{m.group(1)}0\n" if m else line)
    return out, n, None


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    if len(args) != 2 or any(f != "--drop-unused-private-segment" for f in flags):
        sys.exit("usage: rm_peephole.py [--drop-unused-private-segment] <in.s> <out.s>")
    src, dst = args
    with open(src) as f:
        lines = f.readlines()
    out, changed, kept = rewrite(lines)
    if flags:
        out, n, why = drop_unused_private_segment(out)
        print(f"rm_peephole: private segment of {n} kernel(s) set to 0 (never accessed)" if why is None
              else f"rm_peephole: private segments kept: {why}", file=sys.stderr)
    with open(dst, "w") as f:
        f.writelines(out)
    print(f"rm_peephole: {changed} v_cndmask_b32 re-encoded as VOP3, {kept} left in VOP2 (literal operand)", file=sys.stderr)


if __name__ == "__main__":
    main()
