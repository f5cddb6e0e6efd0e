#!/bin/sh
# Diff of the gfx950 device code of two builds of one object, addresses stripped: checks that a source change
# leaves existing kernels' machine code alone.  usage: tools/disasm_diff.sh old.o new.o   (no GPU needed)
# An object without device code (dqp_dispatch.o) is compared by its host code and relocations instead.
L=/opt/rocm/lib/llvm/bin
out=$(mktemp -d)
i=0
for o in "$1" "$2"; do
  i=$((i + 1))
  d=$(mktemp -d)
  if $L/llvm-readelf -S "$o" | grep -q '\.hip_fatbin'; then
    $L/llvm-objcopy --dump-section .hip_fatbin=$d/fat "$o"
    $L/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$d/fat --output=$d/co
    $L/llvm-objdump -d --no-show-raw-insn --no-leading-addr $d/co | grep -v 'file format' |
      sed -E 's@ *//.*$@@; s@<[^>]*\+0x[0-9a-f]+>@@' > "$out/$i.dis"
  else
    $L/llvm-objdump -d -r --no-show-raw-insn --no-leading-addr "$o" | grep -v 'file format' > "$out/$i.dis"
  fi
  rm -rf $d
done
diff "$out/1.dis" "$out/2.dis" > /dev/null && echo "identical: $(grep -c '^<' "$out/1.dis") kernels / functions"
diff "$out/1.dis" "$out/2.dis"
rc=$?
rm -rf "$out"
exit $rc
