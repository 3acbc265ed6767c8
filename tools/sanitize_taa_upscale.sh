#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host build of the temporal upsampling's kernel body
# (csrc/taa_upscale_core.hpp) against its checker (tests/taa_upscale_ref): a stand-alone program linked with the sanitizers' runtimes,
# so it needs no preload (tests/taa_upscale_host/taa_upscale_san_main.cpp).  CPU only.  Usage (from the repo root):
# tools/sanitize_taa_upscale.sh
set -euo pipefail
cd "$(dirname "$0")/.."
export ASAN_OPTIONS=detect_leaks=0:abort_on_error=1:halt_on_error=1
export UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1
CLANG=/opt/rocm/lib/llvm/bin/clang
SAN_DIR=$(mktemp -d)
trap 'rm -rf "$SAN_DIR"' EXIT
"$CLANG" -O1 -g -std=c99 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/taa_upscale_ref/taa_upscale_ref.c -o "$SAN_DIR/taa_upscale_ref.o"
"$CLANG"++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
    -I crychic_renderer_amd/csrc tests/taa_upscale_host/taa_upscale_san_main.cpp tests/taa_upscale_host/taa_upscale_host.cpp "$SAN_DIR/taa_upscale_ref.o" -lm \
    -o "$SAN_DIR/taa_upscale_san"
"$SAN_DIR/taa_upscale_san"
