#!/bin/bash
# cross-compiles act_norm_bench into scripts/ubench/build/ and links it with the product's own objects (llama_box_amd/build/*.o: run the package build first)
set -e
cd "$(dirname "$0")"; mkdir -p build
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DGGML_MAX_NAME=128 -I../../include -I../../llama_box_amd/csrc -c act_norm_bench.hip -o build/act_norm_bench.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 build/act_norm_bench.o ../../llama_box_amd/build/*.o -ldl -o build/act_norm_bench
ls -la build/act_norm_bench
