#!/bin/bash
# same-call A/B of SMR_MP_SIDE_STEADY=0 (the parent's path) against the default, then the profiles of both
set -o pipefail
OUT=${SIDE_AB_OUT:-bench_outputs}   # where the record goes
mkdir -p $OUT
R=$PWD
T=${1:-side_steady}
O=$OUT/$T
DRV="--gpus 1 --steps 20 --warmup 5"
: > ${O}_ab.log
run() {  # name, env value, bench args
  if [ "$2" = off ]; then SMR_MP_SIDE_STEADY=0 timeout -k 10 240 python bench.py $3 > ${O}_$1.json 2>> ${O}_bench.err || return 1
  else timeout -k 10 240 python bench.py $3 > ${O}_$1.json 2>> ${O}_bench.err || return 1; fi
  python -c "
import json,sys
d=json.loads(open('${O}_$1.json').read().strip().splitlines()[-1]); print('$1', d['ms_per_step'], d['value'])" | tee -a ${O}_ab.log
}
for i in 1 2 3 4 5; do
  run drv_off_$i off "$DRV" && run drv_on_$i on "$DRV" || exit 4
done
for i in 1 2 3 4 5; do
  run def_off_$i off "" && run def_on_$i on "" || exit 5
done
timeout -k 10 120 python tools/side_steady_share.py 2>&1 | tail -1 | tee -a ${O}_ab.log || exit 6
cd /tmp && export TMPDIR=/tmp
SMR_MP_SIDE_STEADY=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $R/${O}_prof_off -- python $R/bench.py $DRV > $R/${O}_under_rocprof_off.json 2> /dev/null || exit 7
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $R/${O}_prof_on -- python $R/bench.py $DRV > $R/${O}_under_rocprof_on.json 2> /dev/null || exit 8
cd $R
for a in off on; do
  python tools/rocpd_summary.py ${O}_prof_$a --only mp_straggler_batch > ${O}_kernel_stats_$a.txt 2>&1
  python tools/rocpd_timeline.py ${O}_prof_$a mp_ --only mp_straggler_batch --limit 4000 > ${O}_timeline_full_$a.txt 2>&1
  grep -v "at::native" ${O}_kernel_stats_$a.txt | head -12 | cut -c1-140
done
cd /tmp
for a in off on; do
  for c in FETCH_SIZE WRITE_SIZE; do
    if [ $a = off ]; then SMR_MP_SIDE_STEADY=0 timeout -k 10 200 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $R/${O}_pmc_${c}_$a -- python $R/tools/pmc_probe.py > /dev/null 2>&1 || exit 9
    else timeout -k 10 200 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $R/${O}_pmc_${c}_$a -- python $R/tools/pmc_probe.py > /dev/null 2>&1 || exit 9; fi
  done
  ( cd $R && python tools/pmc_traffic.py ${O}_pmc_FETCH_SIZE_$a ${O}_pmc_WRITE_SIZE_$a "tools/pmc_probe.py, SMR_MP_SIDE_STEADY $a" > ${O}_pmc_traffic_$a.json 2>> ${O}_pmc.err
    python -c "
import json; d=json.load(open('${O}_pmc_traffic_$a.json'))['kernels']
for k,v in d.items():
    if 'mp_' in k: print('$a', k[:50], v['launches'], round(v['hbm_bytes_per_launch']/1e6,2), 'MB')" | tee -a ${O}_ab.log )
done
cd $R
rm -rf ${O}_prof_off ${O}_prof_on ${O}_pmc_FETCH* ${O}_pmc_WRITE*
