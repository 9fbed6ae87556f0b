set -x
O=${AB_OUT:-build/r06a}; mkdir -p "$O"
timeout 900 python -m pytest tests/test_raster_gpu.py -x -q -m gpu 2>&1 | tail -15 > $O/raster_tests.txt
timeout 120 python profiles/bwd_px_stats.py 0 2 5 > $O/px_stats.txt 2>&1
for k in pixel wave pixel wave; do
  AG_BWD_KERNEL=$k timeout 200 python bench.py --full --steps 400 --warmup 100 --no-cpu-baseline --no-full-step --no-stress > "$O/bench_$k.json" 2> "$O/bench_$k.err"
  python - "$O" $k <<'PY'
import json, sys
d=json.loads(open(f"{sys.argv[1]}/bench_{sys.argv[2]}.json").read().strip().splitlines()[-1])
print(f"{sys.argv[2]:8s} value {d['value']:8.1f}  seq {d['sequential']['views_per_s']:7.1f}  bwd us (1 stream) {d['sequential']['blend_backward_avg_launch_us']:6.1f}  overlapped {d['roofline']['avg_launch_us']:6.1f}")
PY
done > $O/ab.txt 2>&1
cat $O/raster_tests.txt $O/px_stats.txt $O/ab.txt
