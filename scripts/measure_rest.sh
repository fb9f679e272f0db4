#!/bin/bash
# The rest of a round's measurement set (run after scripts/measure_round.sh TAG all cfg3 / cfg2 / cfg5 / cfg3 --mip).
#   usage: bash scripts/measure_rest.sh TAG      -> $OUT/TAG_* (default measure_out/; copy what is to be judged into profiles/)
TAG=${1:-rXX}
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
OUT=${MEASURE_OUT:-measure_out}
mkdir -p "$OUT"
E=$OUT/${TAG}_rest.err; : > $E
python bench.py --full --workload cfg5 --frames-per-gpu 32 --no-cpu-baseline --steps 20 > $OUT/${TAG}_bench_cfg5_32frames.json 2>> $E && echo cfg5-32
python bench.py --full --channels 3 --no-cpu-baseline --no-reference-shaped-step > $OUT/${TAG}_bench_cfg3_c3.json 2>> $E && echo c3
python scripts/coverage_sweep.py > $OUT/${TAG}_coverage_sweep.json 2>> $E && echo sweep
rocprofv3 --kernel-trace --output-format csv -d $OUT/tl -- python3 scripts/prof_objective.py --ops 0 > /dev/null 2>> $E; python scripts/step_timeline.py $OUT/tl --all > $OUT/${TAG}_step_timeline.txt; rm -rf $OUT/tl
rocprofv3 --kernel-trace --output-format csv -d $OUT/tl -- python3 scripts/prof_objective.py --ops 0 --frames-per-step 1 --views-per-step 1 --workload ref --graph 1 --steps 12 > /dev/null 2>> $E; python scripts/step_timeline.py $OUT/tl --all > $OUT/${TAG}_ref_step_timeline_graph.txt; rm -rf $OUT/tl
# wave-cycles of k_shade by phase: a -DFPCDR_OPROF build of objective.hip (scripts/build_obj_variant.sh oprof -DFPCDR_OPROF, built in the container)
if [ -f fpc_diffrend_amd/libfpcdr_oprof.so ]; then
  FPCDR_LIB_PATH=$PWD/fpc_diffrend_amd/libfpcdr_oprof.so python scripts/prof_phases.py > $OUT/${TAG}_shade_phase_cycles.txt 2>> $E && echo oprof
fi
echo done
