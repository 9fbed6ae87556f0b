#!/bin/bash
# Round artefacts for profiles/ from ONE box:  profiles/collect_round.sh <tag>    (outputs under $OUT, default build/round)
#   <tag>_bench.json                 python bench.py --full (the headline with every other leg)
#   <tag>_bench_kernel_stats.csv     rocprofv3 --kernel-trace --stats of the same command, summarised per kernel
#   <tag>_conv_layers.csv            per-layer forward / dgrad / wgrad table of the DualStyleUNet convolutions
#   <tag>_styleunet_kernel_stats.csv rocprofv3 summary of DualStyleUNet forward and forward + backward passes
#   <tag>_conv_math_ab.txt           interleaved A/B of the three convolution arithmetic modes (network pass, training step)
#   <tag>_host_vs_gpu.txt            host issue time against GPU time of the network pass and the training step
cd "$(dirname "$0")/.."
tag=${1:-rXX}
O=${OUT:-build/round}; mkdir -p "$O"
T=$(mktemp -d)
python bench.py --full > "$O"/${tag}_bench.json 2> "$O"/${tag}_bench.err
tail -c 600 "$O"/${tag}_bench.json; echo
rocprofv3 --kernel-trace --stats -d "$T/prof_bench" -o b -- python bench.py --full > "$O"/${tag}_bench_profiled.json 2> /dev/null
db=$(find "$T/prof_bench" -name "*.db" | head -1)
python profiles/summarize_rocprof.py "$db" "$O"/${tag}_bench_kernel_stats.csv | head -14 | cut -c1-140
python profiles/conv_layers.py "$O"/${tag}_conv_layers.csv | tail -1
rocprofv3 --kernel-trace --stats -d "$T/prof_su" -o su -- python profiles/styleunet_bench.py 4 > "$O"/${tag}_styleunet_bench.log 2>&1
db=$(find "$T/prof_su" -name "*.db" | head -1)
python profiles/summarize_rocprof.py "$db" "$O"/${tag}_styleunet_kernel_stats.csv | head -8 | cut -c1-140
grep -E "^fwd" "$O"/${tag}_styleunet_bench.log
python profiles/conv_math_ab.py 3 > "$O"/${tag}_conv_math_ab.txt 2>&1; tail -3 "$O"/${tag}_conv_math_ab.txt
python profiles/host_vs_gpu.py > "$O"/${tag}_host_vs_gpu.txt 2>&1; tail -3 "$O"/${tag}_host_vs_gpu.txt
