#!/usr/bin/env bash
# Is the DEVICE code of two trees the same?  usage: tools/device_asm_diff.sh <tree A> <tree B> [jobs]
# Compiles every unit of ringsnark_amd/csrc of both trees to gfx950 assembly (device side only, each tree's own Makefile
# flags; no GPU, about two library builds of time) and compares them PER KERNEL SYMBOL across all the units of a tree, so the
# two trees may cut their units differently.  A kernel's text runs from its label to the end of its .amdhsa_kernel block; the
# compiler's local label numbers (.LBB<n>_<k>, .Ltmp<n>: they count the functions of the unit) are normalised, and comments
# (which repeat them) and the lines naming __hip_cuid_<hash>, a hash of the unit's source text, dropped.  Prints the symbols
# only one tree has, the symbols more than one unit of a tree defines, and one line per kernel whose text differs; exit
# status 1 if there is any of those.  A kernel may differ only because of the unit it is compiled in (hipcc internalises
# device helpers per unit): compare its tools/kernel_resources.py lines then.
set -euo pipefail
A=$(realpath "$1") B=$(realpath "$2") JOBS=${3:-6}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
for side in A B; do
  tree=${!side}/ringsnark_amd/csrc
  cmd=$(make -s -C "$tree" --eval='print-device-cmd: ; @echo $(HIPCC) $(FLAGS)' print-device-cmd)
  mkdir -p "$OUT/$side"
  for f in $(make -s -C "$tree" --eval='print-srcs: ; @echo $(SRCS)' print-srcs); do
    echo "cd $tree && $cmd --offload-device-only -S $f -o $OUT/$side/${f%.hip}.s 2> $OUT/$side/${f%.hip}.log || { cat $OUT/$side/${f%.hip}.log; exit 255; }"
  done
done | xargs -P "$JOBS" -I{} sh -c {}
status=0
for side in A B; do  # $side.txt: "<symbol> <unit> <checksum> <length>" per kernel definition
  for s in "$OUT/$side"/*.s; do
    grep -v __hip_cuid_ "$s" | sed -E 's/[ \t]*;.*$//; s/\.L(BB|JTI)[0-9]+_/.L\1_/g; s/\.L(tmp|func_begin|func_end)[0-9]+/.L\1/g' |
      awk -v unit="$(basename "$s" .s)" '
        /^[A-Za-z_][A-Za-z0-9_$.]*:/ { sym = $1; sub(/:.*/, "", sym); n = 0 }
        sym != "" { text[n++] = $0 }
        /^[ \t]*\.end_amdhsa_kernel/ { cmd = "echo \047" sym "\047 " unit " $(cksum)"; for (i = 0; i < n; i++) print text[i] | cmd; close(cmd); sym = "" }'
  done | LC_ALL=C sort > "$OUT/$side.txt"
  awk '{ print $1, $3, $4 }' "$OUT/$side.txt" | uniq > "$OUT/$side.sum"
  cut -d' ' -f1 "$OUT/$side.txt" | uniq -d | sed "s/^/tree $side, in more than one unit: /" | grep . && status=1
done
LC_ALL=C comm -3 <(cut -d' ' -f1 "$OUT/A.sum" | uniq) <(cut -d' ' -f1 "$OUT/B.sum" | uniq) | sed -E 's/^\t/only in B: /; t; s/^/only in A: /' | grep . && status=1
LC_ALL=C join "$OUT/A.sum" "$OUT/B.sum" | awk '$2 != $4 || $3 != $5 { print "text differs: " $1 }' | grep . && status=1
echo "$(cut -d' ' -f1 "$OUT/A.sum" | uniq | wc -l) kernels in A, $(cut -d' ' -f1 "$OUT/B.sum" | uniq | wc -l) in B: $([ $status = 0 ] && echo identical || echo DIFFERENT)"
exit $status
