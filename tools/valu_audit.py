#!/usr/bin/env python3
"""Instruction mix of one kernel instantiation, from the compiler's assembly (CPU only, no GPU needed).

    python tools/valu_audit.py                         # shape B, fe_frame8_kernel, the benchmark's instantiation
    python tools/valu_audit.py --shape T --flags 0,1,0,0,0,0
    python tools/valu_audit.py --asm /tmp/fe_b.s       # classify an assembly file that is already there
    python tools/valu_audit.py --save-asm /tmp/fe_b.s  # keep the assembly of this run
    python tools/valu_audit.py --obj fastenhancer_amd/csrc/_obj/fe_shape_B.o   # the object of a build that is there: seconds

The shape's translation unit (csrc/fe_shape.hip.in) is compiled with build.py's FLAGS plus `--cuda-device-only -S` (minutes for
a B-type shape), the kernel is picked by name and template flags (for fe_frame8_kernel: DBG, PERSIST, SLOT, HIO, STRM, BANK), and every
instruction is put into a class by its mnemonic's prefix.  The table has one row per barrier segment of the listing (segment i lies
between the i-th and the (i + 1)-th s_barrier in layout order; both wave roles of a phase are in the same segment) and a total.
fp32 MFMAs and the vector ALU share a SIMD's datapath, so the non-MFMA vector columns are what a phase pays on top
of its matrix work.  This is a counter of instruction classes: it neither looks for nor judges particular instructions."""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ["mfma", "int/addr", "cmp/sel", "move", "transc", "float", "ds_rd", "ds_wr", "vmem", "scalar", "s_nop", "wait"]
VALU = ["int/addr", "cmp/sel", "move", "transc", "float"]
BOOKKEEPING = ["int/addr", "cmp/sel", "move"]

_TRANS = ("v_exp_", "v_rcp_", "v_log_", "v_sqrt_", "v_rsq_", "v_sin_", "v_cos_")
_MOVE = ("v_mov_", "v_pk_mov_", "v_accvgpr_", "v_readfirstlane_", "v_readlane_", "v_writelane_", "v_swap_", "v_permlane")
_CMPSEL = ("v_cmp_", "v_cmpx_", "v_cndmask_")
_VMEM = ("buffer_", "global_", "flat_", "scratch_", "tbuffer_")
_FLOAT_RE = re.compile(r"_(f16|f32|f64|bf16)\b|_(f16|f32|f64|bf16)_")


def classify(mn: str):
    """Mnemonic -> class name, or None for what is no instruction of the twelve classes (s_barrier, s_endpgm are handled by the caller)."""
    if mn.startswith("v_mfma_") or mn.startswith("v_smfmac_"):
        return "mfma"
    if mn.startswith("v_"):
        if mn.startswith(_TRANS):
            return "transc"
        if mn.startswith(_MOVE):
            return "move"
        if mn.startswith(_CMPSEL):
            return "cmp/sel"
        if _FLOAT_RE.search(mn):
            return "float"
        return "int/addr"
    if mn.startswith("ds_"):
        return "ds_wr" if mn.startswith(("ds_write", "ds_store")) else "ds_rd"
    if mn.startswith(_VMEM):
        return "vmem"
    if mn == "s_nop":
        return "s_nop"
    if mn.startswith("s_waitcnt"):
        return "wait"
    if mn.startswith("s_"):
        return "scalar"
    return None


def compile_asm(shape: str, out: str) -> None:
    from fastenhancer_amd import build as fb
    args = dict(fb.shapes()).get(shape)
    if args is None:
        raise SystemExit(f"shape {shape!r} is not in csrc/fe_shapes.def (known: {', '.join(n for n, _ in fb.shapes())})")
    cmd = [fb._hipcc()] + fb.FLAGS + [f"-DFE_SHAPE_NAME={shape}", f"-DFE_SHAPE_ARGS={args}", "--cuda-device-only", "-S",
                                      "-x", "hip", os.path.join(fb.CSRC, "fe_shape.hip.in"), "-o", out]
    subprocess.check_call(cmd)


def disassemble(obj: str, out: str) -> None:
    """An object of csrc/_obj* (a build that is already there) -> a listing in the shape of the compiler's assembly: seconds, not minutes."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tmp = tempfile.mkdtemp(prefix="valu_audit_")
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "k.co")
    subprocess.check_call(["objcopy", f"--dump-section=.hip_fatbin={fat}", obj])
    subprocess.check_call([f"{llvm}/clang-offload-bundler", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--output={co}", "--unbundle"])
    dis = subprocess.check_output([f"{llvm}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    notes = subprocess.check_output([f"{llvm}/llvm-readelf", "--notes", co], text=True)
    # the kernels' metadata maps: keys in alphabetical order, .vgpr_count after .name (an argument's .name comes before the kernel's)
    res, ent = {}, {}
    for ln in notes.splitlines():
        m = re.match(r"[\s-]*\.(\w+):\s*(\S+)", ln)
        if m:
            ent[m.group(1)] = m.group(2)
            if m.group(1) == "vgpr_count":
                res[ent.get("name")], ent = ent, {}

    def footer(f, name):
        r = res.get(name, {})
        f.write(".Lfunc_end:\n")
        f.write(f"; NumVgprs: {r.get('vgpr_count', 0)}\n; NumAgprs: {r.get('agpr_count', 0)}\n; NumSgprs: {r.get('sgpr_count', 0)}\n"
                f"; ScratchSize: {r.get('private_segment_fixed_size', 0)}\n; LDSByteSize: {r.get('group_segment_fixed_size', 0)}\n")

    with open(out, "w") as f:
        cur = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\w+)>:", ln)
            if m and m.group(1).startswith("_Z"):
                if cur:
                    footer(f, cur)
                cur = m.group(1)
                f.write(f"{cur}:\n")
            elif cur and not m and ln.startswith(("\t", " ")) and ln.strip():
                f.write("\t" + ln.split("//")[0].strip() + "\n")
        if cur:
            footer(f, cur)


def pick_kernel(lines, kernel: str, flags):
    """-> (mangled name, first line, one past the last line) of the instantiation whose trailing bool template arguments are `flags`."""
    want = "".join(f"Lb{int(f)}E" for f in flags)
    cands = []
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and kernel in m.group(1):
            cands.append((m.group(1), i))
    hits = [(n, i) for n, i in cands if re.search(re.escape(kernel) + r"I.*E" + want + r"EEv", n)]
    if len(hits) != 1:
        raise SystemExit(f"{len(hits)} instantiations of {kernel} with flags {flags}; candidates:\n  " + "\n  ".join(n for n, _ in cands))
    name, start = hits[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return name, start, end


def audit(lines, start, end):
    segs = [dict.fromkeys(CLASSES, 0)]
    mnems = {}
    barriers = 0
    for ln in lines[start + 1:end]:
        s = ln.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        mn = s.split()[0]
        if mn == "s_barrier":
            barriers += 1
            segs.append(dict.fromkeys(CLASSES, 0))
            continue
        c = classify(mn)
        if c is None:
            continue
        segs[-1][c] += 1
        mnems.setdefault(c, {}).setdefault(mn, 0)
        mnems[c][mn] += 1
    return segs, mnems, barriers


def resources(lines, name, end):
    """The figures the compiler prints behind the kernel's body."""
    out = {}
    for ln in lines[end:end + 400]:
        m = re.match(r"^;\s*(NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", ln)
        if m and m.group(1) not in out:
            out[m.group(1)] = int(m.group(2))
        if re.match(r"^_Z\w+:", ln):
            break
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="B")
    ap.add_argument("--kernel", default="fe_frame8_kernel")
    ap.add_argument("--flags", default="0,0,0,0,0,0", help="the instantiation's trailing bool template arguments")
    ap.add_argument("--asm", help="classify this assembly file instead of compiling")
    ap.add_argument("--obj", help="disassemble this object of a build that is there (csrc/_obj*/fe_shape_<shape>.o) instead of compiling")
    ap.add_argument("--save-asm", help="keep the compiled assembly here")
    a = ap.parse_args()
    flags = [int(x) for x in a.flags.split(",") if x != ""]
    if a.asm:
        path = a.asm
    elif a.obj:
        path = a.save_asm or os.path.join(tempfile.mkdtemp(prefix="valu_audit_"), "listing.s")
        disassemble(a.obj, path)
    else:
        path = a.save_asm or os.path.join(tempfile.mkdtemp(prefix="valu_audit_"), f"fe_shape_{a.shape}.s")
        compile_asm(a.shape, path)
    lines = open(path).read().splitlines()
    name, start, end = pick_kernel(lines, a.kernel, flags)
    segs, mnems, barriers = audit(lines, start, end)
    tot = {c: sum(s[c] for s in segs) for c in CLASSES}
    res = resources(lines, name, end)

    print(f"kernel   {a.kernel} [shape {a.shape}] flags {','.join(str(f) for f in flags)}")
    print(f"symbol   {name}")
    print("resources " + "  ".join(f"{k}={v}" for k, v in res.items()) + f"  s_barrier={barriers}")
    print()
    nv = sum(tot[c] for c in VALU)
    print(f"{'class (static count, all wave roles)':<44}{'instructions':>12}")
    print(f"{'MFMA':<44}{tot['mfma']:>12}")
    print(f"{'vector, not MFMA':<44}{nv:>12}")
    for c, label in (("int/addr", "integer / address"), ("cmp/sel", "compares / selects"), ("move", "moves"),
                     ("transc", "transcendental"), ("float", "float add / mul / fma / cvt")):
        top = sorted(mnems.get(c, {}).items(), key=lambda kv: -kv[1])[:7]
        print(f"{'  - ' + label:<44}{tot[c]:>12}   " + ", ".join(f"{m} {n}" for m, n in top))
    print(f"{'integer/address + compare/select + move':<44}{sum(tot[c] for c in BOOKKEEPING):>12}")
    print()
    print("per barrier segment (layout order):")
    print(f"{'seg':>4}" + "".join(f"{c:>9}" for c in CLASSES))
    for i, s in enumerate(segs):
        print(f"{i:>4}" + "".join(f"{s[c]:>9}" for c in CLASSES))
    print(f"{'all':>4}" + "".join(f"{tot[c]:>9}" for c in CLASSES))


if __name__ == "__main__":
    main()
