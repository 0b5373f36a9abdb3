#!/bin/bash
# Is the gfx950 device code of two builds the same, object by object?  (no GPU needed)
#   tools/compare_device_code.sh <parent csrc/_obj> <changed csrc/_obj> > profiles/<name>_device_code.txt
# For every *.o of either directory the gfx950 code object is unbundled (as tools/kernel_resources.sh does) and three things are compared:
#   symbols   every defined symbol (kernels, their descriptors, device functions and variables) with its type, except
#             __hip_cuid_<hash>: the compiler's id of the translation unit, a hash that includes the host-side source text
#   code      the disassembly without addresses and encodings (symbol-stripped: labels are kept, nothing else names a symbol)
#   notes     the note metadata of every kernel (VGPR / AGPR / SGPR counts, spills, LDS and scratch bytes, kernarg layout)
# A host-side refactor must report "identical" on all three for every object.  Exit status 1 if anything differs.
set -u
A=${1:?parent object directory}; B=${2:?changed object directory}
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
T=$(mktemp -d); trap 'rm -rf $T' EXIT

extract() {   # <object> <out prefix>: prefix.sym / .asm / .notes; returns 1 if the object holds no gfx950 code
    rm -f $2.fat $2.co $2.sym $2.asm $2.notes
    objcopy --dump-section .hip_fatbin=$2.fat "$1" 2>/dev/null || return 1
    $LLVM/clang-offload-bundler --type=o --input=$2.fat --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$2.co --unbundle 2>/dev/null || return 1
    [ -s $2.co ] || return 1
    $LLVM/llvm-readelf --symbols --wide $2.co | awk '$1 ~ /^[0-9]+:$/ && $7 != "UND" && $8 != "" {print $4, $8}' | grep -v " __hip_cuid_" | sort > $2.sym
    $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $2.co | grep -v "file format" | sed -e 's/[[:space:]]*\/\/ [0-9A-Fa-f]*:.*$//' > $2.asm
    $LLVM/llvm-readelf --notes $2.co > $2.notes
}

same() { cmp -s "$1" "$2" && echo identical || echo DIFFERENT; }

bad=0; n=0; kernels=0
printf "%-34s %8s %10s %-10s %-10s %-10s\n" object functions asm-lines symbols code notes
for name in $( (cd "$A" && ls *.o; cd "$B" && ls *.o) 2>/dev/null | sort -u); do
    if [ ! -f "$A/$name" ] || [ ! -f "$B/$name" ]; then
        printf "%-34s only in %s\n" "$name" "$([ -f "$A/$name" ] && echo parent || echo change)"; bad=1; continue
    fi
    extract "$A/$name" $T/a; ra=$?
    extract "$B/$name" $T/b; rb=$?
    if [ $ra -ne 0 ] && [ $rb -ne 0 ]; then printf "%-34s %8s (no gfx950 code in either)\n" "$name" 0; continue; fi
    if [ $ra -ne $rb ]; then printf "%-34s gfx950 code in one build only\n" "$name"; bad=1; continue; fi
    s=$(same $T/a.sym $T/b.sym); c=$(same $T/a.asm $T/b.asm); m=$(same $T/a.notes $T/b.notes)
    k=$(grep -c "^FUNC " $T/b.sym); kernels=$((kernels + k)); n=$((n + 1))
    printf "%-34s %8d %10d %-10s %-10s %-10s\n" "$name" "$k" "$(wc -l < $T/b.asm)" "$s" "$c" "$m"
    if [ "$s$c$m" != identicalidenticalidentical ]; then
        bad=1
        [ $s = DIFFERENT ] && diff $T/a.sym $T/b.sym | head -20 | sed -e 's/^/    symbols: /'
        [ $c = DIFFERENT ] && diff $T/a.asm $T/b.asm | head -20 | sed -e 's/^/    code: /'
        [ $m = DIFFERENT ] && diff $T/a.notes $T/b.notes | head -20 | sed -e 's/^/    notes: /'
    fi
done
echo
if [ $bad -eq 0 ]; then echo "$n objects with gfx950 code, $kernels function symbols: symbols, code and notes identical in every object"
else echo "DIFFERENCES FOUND (see above)"; fi
exit $bad
