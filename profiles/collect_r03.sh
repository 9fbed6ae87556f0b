#!/bin/bash
# Round-3 artefacts for profiles/ from ONE box:  bash profiles/collect_r03.sh   (run through gpurun; outputs under gpurun_out/r03z)
cd "$(dirname "$0")/.."
R=$PWD
export TMPDIR=/tmp
O=$R/gpurun_out/r03z
mkdir -p $O
# 1. the driver's default command
( time python bench.py --full > $O/bench.json 2> $O/bench.err ) 2> $O/bench.time; tail -3 $O/bench.time
# 2. rocprofv3 kernel summary of the raster legs of the same command
rm -rf /tmp/prof_bench
( cd /tmp && rocprofv3 --kernel-trace --stats -d /tmp/prof_bench -o b -- python $R/bench.py --no-full-step --no-cpu-baseline --no-stress > $O/bench_profiled.json 2> /dev/null )
db=$(find /tmp/prof_bench -name "*.db" | head -1)
python profiles/summarize_rocprof.py "$db" $O/bench_kernel_stats.csv | head -10 | cut -c1-150
# 3. one-stream per-kernel breakdown
python bench.py --full --breakdown --no-full-step --no-cpu-baseline --no-stress --steps 400 --warmup 100 > $O/raster_breakdown.json 2> /dev/null
# 4. HBM traffic per launch: two PMC passes (one counter each), calibrated on a 256-MiB copy of the same run
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/pmc_$c
  ( cd /tmp && rocprofv3 --pmc $c --kernel-trace -d /tmp/pmc_$c -o p --output-format csv -- python $R/profiles/traffic_probe.py > /dev/null 2>&1 )
done
python profiles/traffic_summarize.py /tmp/pmc_FETCH_SIZE /tmp/pmc_WRITE_SIZE $O/traffic.json > /dev/null 2>&1; python - <<PY
import json
t=json.load(open("$O/traffic.json"))
print({k.split("::")[-1][:28]: v["hbm_bytes"] for k,v in t["kernels"].items()})
PY
# 5. DualStyleUNet passes under rocprofv3
rm -rf /tmp/prof_su
( cd /tmp && rocprofv3 --kernel-trace --stats -d /tmp/prof_su -o su -- python $R/profiles/styleunet_bench.py 4 > $O/styleunet_bench.log 2>&1 )
db=$(find /tmp/prof_su -name "*.db" | head -1)
python profiles/summarize_rocprof.py "$db" $O/styleunet_kernel_stats.csv | head -8 | cut -c1-150
grep -E "^fwd" $O/styleunet_bench.log
# 6. host issue time against GPU time
python profiles/host_vs_gpu.py 2>&1 | grep -v amdgpu.ids | tee $O/host_vs_gpu.txt
