#!/bin/bash
# same-box A/B of one environment switch: tools/ab_bench.sh VAR [extra bench args]  -> $AB_OUT/VAR_{0,1}.log (+ per-shape GEMM tables);
# AB_OUT defaults to bench_logs/ab
V=$1; shift
out=${AB_OUT:-bench_logs/ab}
mkdir -p "$out"
for val in 1 0 1 0; do
  env $V=$val AVAMD_PROBE_SHAPES="$out/${V}_${val}_shapes.txt" timeout -k 10 300 python bench.py --full --no-cpu-baseline --single-variant "$@" > "$out/${V}_${val}.log" 2>&1 || exit 1
  python - "$out/${V}_${val}.log" "$V" "$val" <<'PY'
import json, sys
l = [x for x in open(sys.argv[1]) if x.startswith("{")][-1]
d = json.loads(l)
r = d.get("roofline") or {}
print(sys.argv[2], "=", sys.argv[3], d["value"], "utt/s", d["ms_per_step"], "ms; roofline", r.get("achieved"), "TF/s", r.get("avg_launch_us"), "us", flush=True)
PY
done
