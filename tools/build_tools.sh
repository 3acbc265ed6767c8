#!/bin/bash
# Builds the stand-alone GPU tools against the in-tree library (run from the repo root; hipcc cross-compiles without a GPU):
#   tools/prof_driver       torch-free frame loop for rocprofv3 (PMC passes, tools/pmc_passes.sh)
#   tools/exact_math_probe  exhaustive check of the exact rcp / sqrt / inverse-length sequences against their definitions
#   tools/valu_rate         VALU issue-rate microbenchmark
set -e
cd "$(dirname "$0")/.."
R=$(pwd)
/opt/rocm/bin/hipcc -O2 -std=c++17 -x c++ -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/prof_driver.cpp \
  -L crychic_renderer_amd -lcrychic_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,"$R/crychic_renderer_amd" -o tools/prof_driver
# the probe sweeps devmath.hpp's sequences as the product compiles them: the product's flag set without -shared, read off the
# build module (tests/devmath_dev_lib.py build_probe does the same for the tests)
PROBE_FLAGS=$(python3 -c "
import importlib.util as u
s = u.spec_from_file_location('b', 'crychic_renderer_amd/build.py'); b = u.module_from_spec(s); s.loader.exec_module(b)
print(' '.join(f for f in b.FLAGS if f != '-shared'))")
/opt/rocm/bin/hipcc $PROBE_FLAGS tools/exact_math_probe.hip -o tools/exact_math_probe
[ -x tools/valu_rate ] && [ tools/valu_rate -nt tools/valu_rate.hip ] || /opt/rocm/bin/hipcc -O2 --offload-arch=gfx950 tools/valu_rate.hip -o tools/valu_rate
