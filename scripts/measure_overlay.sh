#!/bin/bash
# usage: bash scripts/measure_overlay.sh   -- one GPU visit for profiles/overlay_kernel.txt: the event timings of
# scripts/time_overlay.py (k_overlay_u8 in its three modes beside k_compare_u8, alternating, profiler off), then ONE run under
# rocprofv3 --kernel-trace --stats of its own (--kernel: a few calls of every variant).  Each step has its own time limit and the
# second runs only if the first ended well.  Output: $MEASURE_OUT (default measure_out/) overlay_time.txt, overlay_stats.txt
OUT=${MEASURE_OUT:-measure_out}
mkdir -p "$OUT"
cd "$(dirname "$0")/.." || exit 1
timeout -k 10 300 python scripts/time_overlay.py > "$OUT/overlay_time.txt" 2>&1 || { tail -20 "$OUT/overlay_time.txt"; exit 1; }
cat "$OUT/overlay_time.txt"
rm -rf "$OUT/overlay_prof"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/overlay_prof" -- python scripts/time_overlay.py --kernel \
    > "$OUT/overlay_prof.log" 2>&1 || { tail -20 "$OUT/overlay_prof.log"; exit 1; }
python - "$OUT" <<'PY' | tee "$OUT/overlay_stats.txt"
import csv, glob, sys
rows = {}
for f in glob.glob(sys.argv[1] + "/overlay_prof/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"]
        if "k_overlay_u8" in k or "k_compare_u8" in k:
            key = (k, int(r["Grid_Size_Y"]))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (k, gy), t in sorted(rows.items()):
    t.sort()
    print("%-60s grid.y %5d: %3d launches, median %8.1f us, min %8.1f us" % (k[:60], gy, len(t), t[len(t) // 2], t[0]))
PY
rm -rf "$OUT/overlay_prof"
