# PMC passes over the K1 sparse kernels beside the dense ones (tools/k1_sparse_bench.py, 2 % density, few windows);
# one counter set per run, each under its own time limit, and nothing more is started once a run fails.
# Summarised per kernel and grid size (the tool runs two shapes) by tools/pmc_by_grid.py.
#   bash tools/pmc_k1_sparse.sh [OUT_DIR]      (default: a directory under $TMPDIR or /tmp)
set -o pipefail
OUT=${1:-${TMPDIR:-/tmp}/pmc_k1_sparse}
mkdir -p "$OUT"
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU" "GRBM_GUI_ACTIVE SQ_INSTS_VALU SQ_ACTIVE_INST_VMEM SQ_WAVES" "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum" "TCP_TCC_READ_REQ_LATENCY_sum TCP_TCC_READ_REQ_sum"; do
  i=$((i+1))
  timeout -k 10 150 rocprofv3 --pmc $set --kernel-trace --output-format csv -d "$OUT" -o p$i -- python3 tools/k1_sparse_bench.py --densities 0.02 --reps 2 --chunks '' --out "$OUT/bench_$i.jsonl" > "$OUT/pass_$i.log" 2>&1 || { echo "pass $i failed: stopping"; exit 1; }
done
python3 tools/pmc_by_grid.py "$OUT" > "$OUT/summary.json" && cat "$OUT/summary.json"
