#!/bin/bash
# Heuristic baselines with the reference's scripts/run_baselines.sh arguments on MI355X.
# The reference's script fans (baseline, root seed) pairs out over SLURM workers that each call
# src/experiments/run_baselines.py --mode single; here every sweep is one GPU handle, so the same
# flags go straight to marlsc.baselines (all arguments are passed through):
#   --mode single|all-seeds --env-config --storage-dir --experiment-name --baseline --baselines
#   --root-seed --n-seeds --eval-seed --eval-episodes
# ENV_CONFIG is used when no --env-config is given.
set -euo pipefail
cd "$(dirname "$0")/.."
export PYTHONPATH="$(pwd)/marl-sc_amd${PYTHONPATH:+:$PYTHONPATH}"
export PYTHONUNBUFFERED=1
export PYTHONHASHSEED=0

ENV_CONFIG=${ENV_CONFIG:-./config_files/environments/env_c3_8wh64r5sku.yaml}
for a in "$@"; do
  if [ "$a" = "--env-config" ]; then ENV_CONFIG=""; fi
done

if [ -n "$ENV_CONFIG" ]; then
  python -m marlsc.baselines --env-config "${ENV_CONFIG}" "$@"
else
  python -m marlsc.baselines "$@"
fi
