#!/bin/bash
# Regenerate mjx_amd/tuning/gfx950_tunableop.csv: PyTorch TunableOp tunes every GEMM shape the
# workloads run (the bench legs of bench.py --full: C3 PPO, return curve, C4 APG; the update at 2048
# envs; the C5 per-rank 8,192-row shard), each process reading and extending the same results file.
# Run on the GPU box; then copy <out-dir>/tunableop_results0.csv into mujoco-mjx-lab_amd/mjx_amd/tuning/.
# Usage: tools/tune_gemms.sh [out-dir]   (default tune_out)
O=${1:-tune_out}
mkdir -p "$O"
rm -f "$O/tunableop_results0.csv"
export PYTORCH_TUNABLEOP_ENABLED=1 PYTORCH_TUNABLEOP_TUNING=1
export PYTORCH_TUNABLEOP_FILENAME=$O/tunableop_results%d.csv
timeout -k 10 500 python -u bench.py --full --no-cpu > "$O/bench.json" 2> "$O/bench.err" || exit $?
timeout -k 10 300 python -u tools/ppo_update_probe.py graph 2048 > "$O/upd.txt" 2>&1 || exit $?
timeout -k 10 300 python -u tools/ppo_update_probe.py shard > "$O/shard.txt" 2>&1 || exit $?
wc -l "$O/tunableop_results0.csv"
