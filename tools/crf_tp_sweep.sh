#!/bin/bash
# GPU box: DenseCRF update tile size (pixels per workgroup tile) against the mean-field time of a bench config (DEV library).
export PNP_HIP_LIB=$PWD/pnp-ovss_amd/pnp_ovss/libpnp_hip_dev.so
# The bench lines go to $OUT (default: $TMPDIR/crf_tp_sweep).
CFG=${1:-coco80}
OUT=${OUT:-${TMPDIR:-/tmp}/crf_tp_sweep}
mkdir -p $OUT
for tp in ${TPS:-256 128 64 32}; do
  PNP_CRF_TP=$tp python bench.py --full --config $CFG --no-other-modes --no-other-configs --no-cpu-baseline --no-noise12 --pipelines 1 --steps 3 --warmup 1 2> $OUT/tp_$tp.err > $OUT/tp_$tp.json || { echo "bench failed for tp $tp:"; tail -5 $OUT/tp_$tp.err; exit 1; }
  python -c "import json; d=json.load(open('$OUT/tp_$tp.json')); print('$CFG tp', $tp, 'img/s', round(d['value'],2), 'crf ms', round(d['crf']['ms_per_step'],1))"
done
