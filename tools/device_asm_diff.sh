#!/usr/bin/env bash
# Is the DEVICE code of two trees the same?  usage: tools/device_asm_diff.sh <tree A> <tree B> [jobs]
# Compiles every unit of ringsnark_amd/csrc of both trees to gfx950 assembly (device side only, each tree's own Makefile
# flags; no GPU, about two library builds of time) and compares them without the lines naming __hip_cuid_<hash>, a hash of the
# unit's source text.  A host-only change must print "identical" six times; exit status 1 on any difference.
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
for s in "$OUT"/A/*.s; do
  u=$(basename "$s")
  diff <(grep -v __hip_cuid_ "$s") <(grep -v __hip_cuid_ "$OUT/B/$u") > "$OUT/$u.diff" && echo "$u: identical ($(grep -vc __hip_cuid_ "$s") lines)" ||
    { echo "$u: DIFFERENT"; head -20 "$OUT/$u.diff"; status=1; }
done
exit $status
