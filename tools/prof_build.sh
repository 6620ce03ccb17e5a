#!/bin/bash
# Profiling build for tools/phase_timers.py: ONE launch configuration of the tiled kernel (a row of csrc/das_tile_cfg.h CFGS that has a translation
# unit) compiled with -DQDAS_PROF=1 (in-kernel phase timers, tile_hooks.h), linked with the product's other objects into tools/abl/libqdas_prof.so
# (scratch, git-ignored).
#   tools/prof_build.sh 2       (fp16 general; then: python tools/phase_timers.py c5)
#   tools/prof_build.sh 17      (C3: folded data, lateral mirror, 128-sample windows)
# Run `make -C qups_amd/csrc` first; plans must use the prebuilt kernels (no QDAS_PLAN_JIT).
set -e
CFG=${1:-0}
cd "$(dirname "$0")/../qups_amd/csrc"
mkdir -p ../../tools/abl
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast -DQDAS_PROF=1 -DQDAS_TILE_CFG=$CFG $EXTRA -c das_tile_inst.hip -o ../../tools/abl/das_tile_cfg${CFG}_prof.o
OBJS=$(ls *.o | grep -v "^das_tile_cfg$CFG.o$" | tr '\n' ' ')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/abl/libqdas_prof.so $OBJS ../../tools/abl/das_tile_cfg${CFG}_prof.o -L/opt/rocm/lib -lhipfft -ldl -Wl,-rpath,/opt/rocm/lib
echo "tools/abl/libqdas_prof.so: launch configuration $CFG instrumented"
