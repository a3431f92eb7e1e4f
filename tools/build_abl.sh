#!/bin/bash
# Builds dealii-stfem_amd/libstfem_abl.so: the product library with the Q4 fp64 tile kernels compiled
# with -DSTFEM_ABLATION (timing experiments via STFEM_EXP; results are wrong when it is nonzero).
# Extra flags for the two ablation objects: tools/build_abl.sh -DFOO ...
set -e
cd "$(dirname "$0")/../dealii-stfem_amd/csrc"
mkdir -p build_abl
FL="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -ffp-contract=fast ${ABL--DSTFEM_ABLATION} $@"
/opt/rocm/bin/hipcc $FL -DSTFEM_TILE_P=4 -c -o build_abl/stfem_tile_p4.o stfem_tile.hip &
/opt/rocm/bin/hipcc $FL -c -o build_abl/stfem_tile.o stfem_tile.hip &
wait
OBJS=$(ls *.o | grep -v -e "^stfem_tile.o$" -e "^stfem_tile_p4.o$" | tr '\n' ' ')
/opt/rocm/bin/hipcc -shared -fPIC -o ../libstfem_abl.so $OBJS build_abl/stfem_tile.o build_abl/stfem_tile_p4.o -ldl
