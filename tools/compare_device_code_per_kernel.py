#!/usr/bin/env python3
"""tools/compare_device_code.sh, function by function: which gfx950 functions of two builds differ?  (no GPU needed)
   python tools/compare_device_code_per_kernel.py <parent csrc/_obj> <changed csrc/_obj> [--allow REGEX] [--removed REGEX] [--added REGEX] [--kernarg REGEX] [--renamed 'REGEX=>REPL'] > profiles/<name>_device_code.txt
For every *.o of both directories the gfx950 code object is unbundled and split into its functions; of each function the disassembly
(without addresses and encodings) and the kernel's note metadata (registers, spills, LDS, scratch, kernarg layout) are compared.
--allow: a regular expression on the name (demangled where a demangler is installed, and mangled) of the functions that are meant to change; any other difference is an error (exit
status 1).  A change that is confined to some instantiations of a kernel template reports every other function as identical.
--removed: the functions that are meant to disappear (in the parent only); without it a function of one build only is an error.
--added: the functions that are meant to be new (in the changed build only): listed with their resource figures.
--kernarg: the functions whose argument block is meant to change and nothing else: their disassembly and every note field but the kernarg
layout (.kernarg_segment_size, the .args list) must be identical.  One thing in the code follows the layout: the hidden arguments (grid size,
...) lie behind the explicit ones, so a kernel that reads one addresses it through an immediate that moves with the block's size.  Such a line
may differ in that one immediate, by exactly the change of .kernarg_segment_size, in a scalar load or scalar add; the lines are counted.
--renamed 'REGEX=>REPL' (needs a demangler): a kernel template that gained a defaulted parameter gives every old instantiation a new name.  A function of
the changed build only whose demangled name, after re.sub(REGEX, REPL), is that of a function of the parent only is compared with that one (its
own mangled name inside its disassembly counts as the parent's); the pairs are counted and, where they differ, reported under the parent's name."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
FILT = next((p for p in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if p and os.path.exists(p)), None)


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def functions(obj, tmp):
    """{mangled name: (disassembly, notes)} of the gfx950 code in obj; {} if there is none"""
    fat, co = os.path.join(tmp, "x.fat"), os.path.join(tmp, "x.co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    if subprocess.run(["objcopy", f"--dump-section=.hip_fatbin={fat}", obj], capture_output=True).returncode != 0:
        return {}
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}",
                    "--unbundle"], capture_output=True)
    if not os.path.exists(co) or os.path.getsize(co) == 0:
        return {}
    code, name = {}, None
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            name = m.group(1)
            code[name] = []
        elif name is not None:
            code[name].append(re.sub(r"\s*// [0-9A-Fa-f]*:.*$", "", line))
    notes = {}
    for block in re.split(r"\n(?=\s*- \.agpr_count|\s*- \.args)", run(f"{LLVM}/llvm-readelf", "--notes", co)):
        m = re.search(r"\.name:\s+(\S+)", block)
        if m:
            # (the list's last block runs on into the note's footer - amdhsa.target, amdhsa.version - which is no kernel's)
            notes[m.group(1)] = re.sub(r"\.(symbol|name):\s+\S+", "", re.split(r"\n\s*amdhsa\.target:", block)[0])
    # (the padding between one function's end and the next one's alignment - "..." and blank lines - belongs to neither: a function
    #  added behind another one must not make that one look changed)
    for v in code.values():
        while v and v[-1].strip() in ("", "..."):
            v.pop()
    return {k: ("\n".join(v), notes.get(k, "")) for k, v in code.items()}


def without_kernarg(notes):
    """the note block without .kernarg_segment_size and the .args list (the lines indented deeper than the .args key)"""
    out, col = [], None
    for line in notes.splitlines():
        if col is not None and (not line.strip() or len(line) - len(line.lstrip()) > col):
            continue
        col = line.index(".args:") if line.strip() in (".args:", "- .args:") else None
        if col is None and ".kernarg_segment_size:" not in line:
            out.append(line)
    return "\n".join(out)


def kernarg_size(notes):
    m = re.search(r"\.kernarg_segment_size:\s+(\d+)", notes)
    return int(m.group(1)) if m else None


def kernarg_offset_lines(a, b):
    """number of lines in which the disassemblies a (parent) and b differ, if each of them is one scalar load / add whose only difference is
    an immediate moved by the change of the kernarg size; None if the functions differ in any other way"""
    ca, cb = a[0].splitlines(), b[0].splitlines()
    sa, sb = kernarg_size(a[1]), kernarg_size(b[1])
    if len(ca) != len(cb) or sa is None or sb is None:
        return None
    n = 0
    for la, lb in zip(ca, cb):
        if la == lb:
            continue
        ta, tb = la.replace(",", " ").split(), lb.replace(",", " ").split()
        d = [i for i in range(len(ta)) if i >= len(tb) or ta[i] != tb[i]]
        if len(ta) != len(tb) or len(d) != 1 or d[0] == 0 or not re.match(r"s_(load_dword|add_u32|add_i32)", ta[0]):
            return None
        try:
            if int(ta[d[0]], 0) - int(tb[d[0]], 0) != sa - sb:
                return None
        except ValueError:
            return None
        n += 1
    return n


def figures(notes):
    g = lambda key: (re.search(r"\.%s:\s+(\d+)" % key, notes) or [None, "-"])[1]
    return (f"vgpr {g('vgpr_count')} agpr {g('agpr_count')} sgpr {g('sgpr_count')} sgpr-spill {g('sgpr_spill_count')} vgpr-spill {g('vgpr_spill_count')} "
            f"lds {g('group_segment_fixed_size')} scratch {g('private_segment_fixed_size')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("changed")
    ap.add_argument("--allow", default=None)
    ap.add_argument("--removed", default=None)
    ap.add_argument("--added", default=None)
    ap.add_argument("--kernarg", default=None)
    ap.add_argument("--renamed", default=None)
    args = ap.parse_args()
    allow, removed, kernarg, added = (re.compile(r) if r else None for r in (args.allow, args.removed, args.kernarg, args.added))
    hit = lambda rx, dem, k: rx is not None and (rx.search(dem) or rx.search(k)) is not None
    names = sorted(set(f for d in (args.parent, args.changed) for f in os.listdir(d) if f.endswith(".o")))
    bad = total = same = allowed = gone = args_only = new = renamed = 0
    ren_rx, _, ren_to = (args.renamed or "=>").partition("=>")
    demangle = lambda ks: dict(zip(ks, run(FILT, *ks).splitlines())) if ks and FILT else {k: k for k in ks}
    print(f"{'object':<30} {'functions':>9} {'identical':>9} {'changed':>8}")
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            pa, pb = os.path.join(args.parent, n), os.path.join(args.changed, n)
            if not (os.path.exists(pa) and os.path.exists(pb)):
                print(f"{n:<30} only in one build")
                bad += 1
                continue
            fa, fb = functions(pa, tmp), functions(pb, tmp)
            if not fa and not fb:
                continue
            if args.renamed:
                only_a, only_b = demangle(sorted(set(fa) - set(fb))), demangle(sorted(set(fb) - set(fa)))
                by_dem = {d: k for k, d in only_a.items()}
                for kb, d in only_b.items():
                    ka = by_dem.get(re.sub(ren_rx, ren_to, d))
                    if ka is not None and d != only_a[ka]:
                        fb[ka] = (fb[kb][0].replace(kb, ka), fb.pop(kb)[1])
                        renamed += 1
            diff = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
            total += len(fb)
            same += len(fb) - len([k for k in diff if k in fb])
            print(f"{n:<30} {len(fb):>9} {len(fb) - len([k for k in diff if k in fb]):>9} {len(diff):>8}")
            for k in diff:
                dem = run(FILT, k).strip() if FILT else k
                if k in fa and k not in fb and hit(removed, dem, k):
                    gone += 1
                    print(f"    removed (meant to): {dem}")
                    continue
                if k in fb and k not in fa and hit(added, dem, k):
                    new += 1
                    print(f"    added (meant to): {dem}")
                    print(f"        change: {figures(fb[k][1])}, {fb[k][0].count(chr(10)) + 1} lines")
                    continue
                moved = kernarg_offset_lines(fa[k], fb[k]) if k in fa and k in fb and hit(kernarg, dem, k) else None
                if moved is not None and without_kernarg(fa[k][1]) == without_kernarg(fb[k][1]):
                    args_only += 1
                    code = "code identical" if moved == 0 else f"code identical but for {moved} immediate(s) that address hidden arguments"
                    print(f"    kernarg layout only (meant to): {dem}: {code}, the other notes identical, kernarg bytes {kernarg_size(fa[k][1])} -> {kernarg_size(fb[k][1])}")
                    continue
                ok = hit(allow, dem, k) and k in fa and k in fb
                allowed += ok
                bad += not ok
                print(f"    {'changed (meant to)' if ok else 'CHANGED'}: {dem}")
                for side, f in (("parent", fa), ("change", fb)):
                    if k in f:
                        print(f"        {side}: {figures(f[k][1])}, {f[k][0].count(chr(10)) + 1} lines")
    print()
    print(f"{total} functions: {same} identical in code and notes, {args_only} with another kernarg layout only, {allowed} changed as meant to, "
          f"{gone} removed as meant to, {new} added as meant to, {bad} other differences"
          + (f"; {renamed} compared under their parent's name (--renamed)" if args.renamed else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
