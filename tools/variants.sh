#!/bin/bash
# Build variants of libmrx_hip.so with extra -D flags and time the bench step with each.
#   VARIANTS="base: b16:-DMRX_DECODE_BATCH=16" tools/variants.sh build     (cross-compiles: no GPU needed)
#   tools/variants.sh run                                                    (on a machine with the GPU)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$R/tools/variant_libs
if [ "$1" = build ]; then
  rm -rf $OUT; mkdir -p $OUT
  for v in $VARIANTS; do   # (one after the other: build_library compiles a variant's units a few at a time)
    name=${v%%:*}; flags=${v#*:}; flags=${flags//,/ }
    (cd $R && python3 -c 'import sys, __graft_entry__ as g; g.build_library(extra_flags=sys.argv[2:], out=sys.argv[1])' \
      $OUT/libmrx_hip_$name.so $flags) || exit 1
  done
  ls -la $OUT
elif [ "$1" = cmd ]; then
  # tools/variants.sh cmd <command...>: run the command once per variant with MRX_LIB set
  shift
  for lib in $OUT/libmrx_hip_*.so; do
    echo "== $(basename $lib)"
    MRX_LIB=$lib "$@" 2>/dev/null | tail -3
  done
else
  for lib in $OUT/libmrx_hip_*.so; do
    line=$(MRX_LIB=$lib python3 $R/bench.py --no-cpu-baseline --steps 20 --warmup 3 2>/dev/null | tail -1)
    echo "$(basename $lib) $(echo "$line" | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print("kernel_ms=%.4f step_ms=%.4f" % (d["roofline"]["kernel_ms"], d["ms_per_step"]))')"
  done
fi
