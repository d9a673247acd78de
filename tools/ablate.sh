#!/bin/bash
# Ablation of the streaming scan kernel on the real bench workload: builds variants of
# libmrx_hip.so with pieces of k_stream_findall switched off (MRX_ABLATE, see mrx_kernels.hip)
# and prints the scan kernel's time for each.  Variant results are wrong by design; only the
# timings mean anything.
#   tools/ablate.sh build    (cross-compiles: no GPU needed)
#   tools/ablate.sh run      (on a machine with the GPU)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$R/tools/ablate_libs
VARIANTS="0 1 2 3 4 5 7 16 18 23"
if [ "$1" = build ]; then
  mkdir -p $OUT
  for v in $VARIANTS; do   # (one after the other: build_library compiles a variant's units a few at a time)
    (cd $R && python3 -c 'import sys, __graft_entry__ as g; g.build_library(extra_flags=sys.argv[2:], out=sys.argv[1])' \
      $OUT/libmrx_hip_$v.so -DMRX_ABLATE=$v) || exit 1
  done
  ls -la $OUT
else
  for v in $VARIANTS; do
    line=$(MRX_LIB=$OUT/libmrx_hip_$v.so python3 $R/bench.py --no-cpu-baseline --steps 20 --warmup 3 2>/dev/null | tail -1)
    echo "ablate=$v $(echo "$line" | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print("kernel_ms=%.4f step_ms=%.4f" % (d["roofline"]["kernel_ms"], d["ms_per_step"]))')"
  done
fi
