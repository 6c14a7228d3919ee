#!/bin/bash
# Build the working-tree sources into tools/abx/<name>.so with extra hipcc flags, out of tree (same-box A/B of library builds through
# CCDM_LIB; *.so stays out of git).
#   tools/build_variant.sh <name> [hipcc flags...]      e.g.  tools/build_variant.sh new   |   tools/build_variant.sh ilp -mllvm -amdgpu-sched-strategy=max-ilp
set -e
cd "$(dirname "$0")/.."
NAME=${1:?name}; shift
mkdir -p tools/abx
cd ccdm_stochastic_segmentation_amd/csrc
ls *.hip | xargs -P 8 -I{} hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form=1 -fPIC "$@" -I../../include -c {} -o /tmp/variant_${NAME}_{}.o
hipcc --offload-arch=gfx950 -shared -fPIC /tmp/variant_${NAME}_*.o -o ../../tools/abx/$NAME.so
rm -f /tmp/variant_${NAME}_*.o
ls -la ../../tools/abx/$NAME.so
