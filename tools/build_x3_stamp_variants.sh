#!/bin/bash
# Diagnostic library with the in-kernel clock stamps of the bf16x3 kernels (-DRNNT_STAMPS): build_variants/x3/lib_stamps.so
#   python3 tools/exp_x3_clock.py x3    (on the GPU box)
set -e
cd "$(dirname "$0")/.."
mkdir -p build_variants/x3
make -C rnnt_amd/csrc -j6 -s librnnt_engine.so
others=$(ls rnnt_amd/csrc/*.o | grep -v -E "/(x3|engine)\.o")
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -DRNNT_STAMPS -Irnnt_amd/csrc"
/opt/rocm/bin/hipcc $F -c rnnt_amd/csrc/engine.hip -o build_variants/x3/engine_stamps.o &
/opt/rocm/bin/hipcc $F -c rnnt_amd/csrc/x3.hip -o build_variants/x3/x3_stamps.o &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_variants/x3/lib_stamps.so $others build_variants/x3/engine_stamps.o build_variants/x3/x3_stamps.o
ls -la build_variants/x3/lib_stamps.so
