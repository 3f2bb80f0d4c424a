#!/bin/bash
# Compare the gfx950 code of two builds function by function: over all objects of each build directory, every function
# symbol's disassembly text and, for kernels, its metadata entry (VGPRs, SGPRs, AGPRs, LDS, scratch, spill counts,
# kernarg size, workgroup size).  Prints the symbols that differ or exist on one side only; exit status 1 if there are
# any.  A plain diff: which object of a build holds a function does not matter; a symbol that two objects of one build
# define (internal linkage allows it) is reported too, since only one of the two could be compared.
# usage: tools/co_diff.sh A_BUILD_DIR B_BUILD_DIR     (VERBOSE=1: also the differing lines)
set -eu
[ $# -eq 2 ] || { echo "usage: $0 A_BUILD_DIR B_BUILD_DIR" >&2; exit 2; }
LLVM=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf $tmp' EXIT

# dump BUILD_DIR OUT_DIR: one file per function symbol in OUT_DIR (each object by itself in OUT_DIR.obj first)
dump() {
  mkdir -p "$2"
  for obj in "$1"/*.o; do
    rm -rf "$2.obj"; mkdir "$2.obj"
    objcopy -O binary --only-section=.hip_fatbin "$obj" $tmp/fat.bin
    [ -s $tmp/fat.bin ] || continue  # host-only object
    $LLVM/clang-offload-bundler --unbundle --type=o --input=$tmp/fat.bin \
      --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/k.co
    $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $tmp/k.co |
      awk -v out="$2.obj" '
        # the comment of a line holds its address and encoding (dropped) and a branch'"'"'s target label (kept); the
        # s_nop / s_code_end padding after a function'"'"'s last instruction is not part of it
        /^<[^>]+>:$/ { if (f) close(f); f = out "/" substr($0, 2, length($0) - 3); print "== code" > f; pad = ""; next }
        !f || !NF { next }
        { sub(/ *\/\/ [0-9A-F]+: [0-9A-F ]*[0-9A-F]/, "") }
        /^[ \t]*(s_nop 0|s_code_end|\.\.\.)[ \t]*$/ { pad = pad $0 "\n"; next }
        { printf "%s", pad >> f; pad = ""; print >> f }'
    $LLVM/llvm-readelf --notes $tmp/k.co |
      awk -v out="$2.obj" '
        function flush(   i) { if (name != "") { f = out "/" name; print "== metadata" >> f; for (i = 0; i < n; i++) print keep[i] >> f; close(f) } n = 0; name = "" }
        /^ +- +\./ { flush() }
        /^ *\.\.\.$|^ +amdhsa\.(target|version)/ { flush() }
        { sub(/^ +(- +)?/, "") }
        /^\.name:/ { name = $2 }
        /^\.(vgpr_count|sgpr_count|agpr_count|group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|kernarg_segment_size|max_flat_workgroup_size|uses_dynamic_stack):/ { keep[n++] = $0 }
        END { flush() }'
    for f in "$2.obj"/*; do
      [ -e "$f" ] || continue
      s=$(basename "$f")
      if [ -e "$2/$s" ]; then echo "twice in $1 (again in $(basename "$obj")): $s"; echo "$s" >> $tmp/twice; else mv "$f" "$2/$s"; fi
    done
  done
}
dump "$1" $tmp/a
dump "$2" $tmp/b

na=$(ls $tmp/a | wc -l); nb=$(ls $tmp/b | wc -l)
ka=$(grep -l "^== metadata" $tmp/a/* | wc -l); kb=$(grep -l "^== metadata" $tmp/b/* | wc -l)
echo "A: $na functions ($ka kernels)   B: $nb functions ($kb kernels)"
bad=$(cat $tmp/twice 2>/dev/null | wc -l)
for s in $(ls $tmp/a $tmp/b | grep -v ':$' | sort -u); do
  [ -n "$s" ] || continue
  if [ ! -e $tmp/a/$s ]; then echo "only in B: $s"; bad=$((bad + 1)); continue; fi
  if [ ! -e $tmp/b/$s ]; then echo "only in A: $s"; bad=$((bad + 1)); continue; fi
  if ! cmp -s $tmp/a/$s $tmp/b/$s; then
    echo "differs:   $s"
    bad=$((bad + 1))
    [ -z "${VERBOSE:-}" ] || diff $tmp/a/$s $tmp/b/$s | head -${VERBOSE_LINES:-40}
  fi
done
echo "$bad symbols differ, are missing on one side or are defined twice"
[ $bad -eq 0 ]
