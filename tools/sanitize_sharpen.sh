#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host build of the sharpening kernels' bodies (csrc/sharpen_core.hpp) against
# the checker (tests/sharpen_ref): a stand-alone program linked with the sanitizers' runtimes, so it needs no preload
# (tests/sharpen_host/sharpen_san_main.cpp).  CPU only.
# Usage (from the repo root): tools/sanitize_sharpen.sh
set -euo pipefail
cd "$(dirname "$0")/.."
export ASAN_OPTIONS=detect_leaks=0:abort_on_error=1:halt_on_error=1
export UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1
CLANG=/opt/rocm/lib/llvm/bin/clang
SAN_DIR=$(mktemp -d)
trap 'rm -rf "$SAN_DIR"' EXIT
"$CLANG" -O1 -g -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/sharpen_ref/sharpen_ref.c -o "$SAN_DIR/sharpen_ref.o"
"$CLANG"++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
    -I crychic_renderer_amd/csrc tests/sharpen_host/sharpen_san_main.cpp tests/sharpen_host/sharpen_host.cpp "$SAN_DIR/sharpen_ref.o" -o "$SAN_DIR/sharpen_san"
"$SAN_DIR/sharpen_san"
