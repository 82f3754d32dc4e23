#!/bin/bash
# bench_box.sh tag [dir]: the driver's bench command with --full on this box -> <dir>/<tag>.json (default dir: boxes/ under $TMPDIR or /tmp)
# + a one-line summary
OUT=${2:-${TMPDIR:-/tmp}/boxes}
mkdir -p "$OUT"
python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/$1.json" 2> "$OUT/$1.err"
python3 - "$OUT/$1.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().split("\n")[-1])
r, p, a = d["roofline"], d.get("power_clock") or {}, d["aspp_t_step"]
print("BOX", d["value"], d["ms_per_step"], "frac", r["frac"], "launch_us", r["avg_launch_us"], "traffic", r["traffic"], "mfma_busy", r.get("mfma_busy"),
      "aspp", a["gemm_frac_of_peak"], a["whole_step_frac"], "h2d", (d.get("h2d_inclusive") or {}).get("value"), p)
PY
