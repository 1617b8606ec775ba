#!/bin/bash
# tools/device_code_diff.sh <old.so> <new.so> : diff of the gfx950 ISA of two library builds; exit status 0 when it is the same.
# The code objects come out as in tools/kernel_regs.sh (fat binary section -> bundles -> unbundle), in translation-unit order.
[ $# -eq 2 ] || { echo "usage: $0 <old.so> <new.so>" >&2; exit 2; }
LLVM=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
disassemble() { # <lib.so> <name>: the disassembly of every code object into $T/<name>.s
  mkdir -p "$T/$2"
  $LLVM/llvm-objcopy -O binary --only-section=.hip_fatbin "$1" "$T/$2/fat" || exit 2
  python3 - "$T/$2" <<'PY' || exit 2
import sys
d=sys.argv[1]; b=open(d+'/fat','rb').read(); magic=b'__CLANG_OFFLOAD_BUNDLE__'
pos=[]; i=b.find(magic)
while i>=0: pos.append(i); i=b.find(magic,i+1)
for k,p in enumerate(pos):
    open('%s/fat%03d'%(d,k),'wb').write(b[p:(pos[k+1] if k+1<len(pos) else len(b))])
PY
  for f in "$T/$2"/fat[0-9]*; do
    $LLVM/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$f" --output="$f.co" --unbundle 2>/dev/null || continue
    echo "== code object ${f##*/fat}"
    $LLVM/llvm-objdump -d "$f.co" | grep -v 'file format'
  done > "$T/$2.s"
  [ -s "$T/$2.s" ] || { echo "$1: no gfx950 code object" >&2; exit 2; }
}
disassemble "$1" old
disassemble "$2" new
if diff "$T/old.s" "$T/new.s"; then
  echo "device code identical: $(grep -c '^== code object' "$T/new.s") code objects, $(grep -c '^[0-9a-f]* <.*>:$' "$T/new.s") functions, $(wc -l < "$T/new.s") lines of disassembly"
else
  echo "device code DIFFERS" >&2
  exit 1
fi
