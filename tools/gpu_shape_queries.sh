#!/bin/bash
# The measurements of the batched shape queries (docs/KERNEL_NOTES.md, "Batched shape queries"): call times on the two
# settled BASELINE worlds, b2hip_step of another build and this one in alternating processes, then the kernel times from a
# separate rocprofv3 run. Every GPU step runs under its own time limit; the chain stops at the first failure.
#   bash tools/gpu_shape_queries.sh <libb2amd_harness.so of the build to compare with> <output directory>
set -o pipefail
other=$1
out=${2:-shape_queries_out}
mkdir -p "$out"
timeout -k 10 900 python tools/gpu_shape_queries.py queries --out "$out/shape_queries_results.json" > "$out/shape_queries_results.txt" &&
timeout -k 10 600 python tools/gpu_queries.py steps --harness "$other" --label "other build" > "$out/shape_queries_step_ab.txt" &&
timeout -k 10 600 python tools/gpu_queries.py steps --label "this build" >> "$out/shape_queries_step_ab.txt" &&
timeout -k 10 600 python tools/gpu_queries.py steps --harness "$other" --label "other build" >> "$out/shape_queries_step_ab.txt" &&
timeout -k 10 600 python tools/gpu_queries.py steps --label "this build" >> "$out/shape_queries_step_ab.txt" &&
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$out/rocprof" -o shape_queries -- python tools/gpu_shape_queries.py queries --quick --reps 2 > "$out/rocprof.log" 2>&1 &&
python tools/gpu_shape_queries.py kernels "$out/rocprof" > "$out/shape_queries_kernel_stats.txt"
