#!/bin/bash
# Round-end records on the GPU box, one gpurun call:  gpurun --timeout 3600 -- 'bash tools/round_end.sh <tag> [suite]'
#   the full -m gpu suite (when "suite" is given) + smoke, the bench line with --full, and every rocprofv3 record the line's
#   rooflines are recomputed from (tools/collect_profiles.sh).  Logs and the bench line under $OUT (default out/), the
#   profiles where tools/collect_profiles.sh writes them; copy what is kept into profiles/.
TAG=${1:-r06}
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
mkdir -p "$OUT"
if [[ "${2:-}" == suite ]]; then
  python -m pytest tests -q -m gpu --durations=8 > "$OUT/${TAG}_gpu_suite.log" 2>&1; tail -14 "$OUT/${TAG}_gpu_suite.log"
  python -c "import __graft_entry__ as g; g.smoke()" >> "$OUT/${TAG}_gpu_suite.log" 2>&1; tail -1 "$OUT/${TAG}_gpu_suite.log"
fi
python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"; echo bench rc=$?
bash tools/collect_profiles.sh ${TAG} C3 > "$OUT/${TAG}_collect.log" 2>&1; tail -3 "$OUT/${TAG}_collect.log"
