#!/usr/bin/env bash
# The builder's end-of-round check on one MI355X box (through gpurun, from the repo root):
#   GIT_HEAD=$(git rev-parse --short HEAD); gpurun --timeout 1200 -- "GIT_HEAD=$GIT_HEAD bash scripts/gpu_round_checks.sh r03"
# gpu-marked tests, smoke(), the round's profile set (scripts/profile_all.sh, with an output folder of its own) and the bench line with
# --full.  The test log and the bench line land under $OUT_DIR (default build/round_checks/).
set -euo pipefail
TAG=${1:-r05}
cd "${GRAFT_REPO_ROOT:-$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)}"
OUT=${OUT_DIR:-build/round_checks}
mkdir -p "$OUT"
timeout -k 10 1100 python -m pytest tests -x -q -m gpu > "$OUT/${TAG}_gpu_tests.log" 2>&1 || { tail -40 "$OUT/${TAG}_gpu_tests.log"; exit 1; }
tail -3 "$OUT/${TAG}_gpu_tests.log"
python -c "import __graft_entry__ as g; g.smoke()"
bash scripts/profile_all.sh "$TAG" 2>&1 | tail -12
timeout -k 10 900 python bench.py --full > "$OUT/${TAG}_bench_full.json" 2> "$OUT/${TAG}_bench_full.err"
python - <<PY
import json
d = json.load(open("$OUT/${TAG}_bench_full.json"))
r = d["roofline"]
print(d["ms_per_step"], d["value"], {k: r[k] for k in ("achieved", "peak", "frac", "traffic", "avg_launch_ms")}, d["cpp_api"], d["kernels_ms"])
PY
