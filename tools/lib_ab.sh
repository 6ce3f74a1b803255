#!/bin/bash
# A/B of two builds of libmaxk_hip.so on the default plans (tooling): the candidate in-tree
# library vs a base build, alternating processes, forward and backward at each k; one JSON line
# per run with "lib". The base is tools/ab/libmaxk_hip_base.so (MAXK_HIP_LIB) or, when the base
# lacks a symbol this tree's binding needs, a whole checkout of the base commit with its library
# built in it (AB_BASE_TREE=dir: the same tools are run from that tree).
#   bash tools/lib_ab.sh [ks] [rounds]
#   AB_DATASET=ogbn-proteins AB_BENCH=1 AB_BASE_TREE=../base bash tools/lib_ab.sh 16 5
# AB_VALUES=gcn: GCN edge values in the forward tool (not constant per row). AB_BENCH=1 adds
# bench.py --gpus 1 (ms_per_step) per k, round and build; AB_BWD=0 skips the backward tool.
set -o pipefail
KS=${1:-"8 16 32 64"}
R=${2:-3}
DS=${AB_DATASET:-reddit}
HERE="$(cd "$(dirname "$0")/.." && pwd)"
tag() { sed "s/^{/{\"lib\": \"$1\", \"dataset\": \"$DS\", \"round\": $2, /"; }
for r in $(seq 1 $R); do
  for lib in base cand; do
    for k in $KS; do
      tree="$HERE"
      unset MAXK_HIP_LIB
      if [ $lib = base ]; then
        if [ -n "$AB_BASE_TREE" ]; then tree="$(cd "$AB_BASE_TREE" && pwd)"; else export MAXK_HIP_LIB="$HERE/tools/ab/libmaxk_hip_base.so"; fi
      fi
      cd "$tree" || exit 1
      if [ "${AB_BWD:-1}" = 1 ]; then
        timeout -k 10 120 python -u tools/bwd_opts.py --dataset $DS --k $k --rounds 1 --opts '[{}]' | tag $lib $r || exit 1
      fi
      timeout -k 10 120 python -u tools/fwd_opts_sweep.py --dataset $DS --k $k --rounds 1 --opts '[{}]' \
        ${AB_VALUES:+--values $AB_VALUES} | tag $lib $r || exit 1
      if [ "${AB_BENCH:-0}" = 1 ]; then
        timeout -k 10 180 python -u bench.py --gpus 1 --steps 50 --warmup 10 --dataset $DS --k $k \
          --no-cpu-baseline --no-comparator --k-sweep '' 2>/dev/null | grep '^{' | tag $lib $r || exit 1
      fi
    done
  done
done
