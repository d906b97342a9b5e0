#!/bin/bash
# A/B of one environment switch of the TUNING build of the library (make -C csrc tuning; through gpurun, from the repository root):
#     bash tools/ab_env.sh gpurun_out/<dir> SWITCH [bench arguments]        e.g. PHOVO_GN_NO_SOLO --thresholds shipped --workload cfg3
# bench.py through tools/bench_with.py with the tuning build, without and with SWITCH=1, interleaved twice.
set -o pipefail
O=$1; SW=${2:?switch}; shift 2
L=$(realpath photoconsistency-visual-odometry_amd/csrc/build_tuning/libphovo_hip_tuning.so)
mkdir -p $O
for rep in 1 2; do
  timeout -k 10 300 python3 tools/bench_with.py $L --full --no-cpu-baseline "$@" > $O/off.$rep.json 2> $O/off.$rep.err
  python3 tools/benchsum.py $O/off.$rep.json off.$rep || tail -3 $O/off.$rep.err
  env $SW=1 timeout -k 10 300 python3 tools/bench_with.py $L --full --no-cpu-baseline "$@" > $O/on.$rep.json 2> $O/on.$rep.err
  python3 tools/benchsum.py $O/on.$rep.json on.$rep || tail -3 $O/on.$rep.err
done
