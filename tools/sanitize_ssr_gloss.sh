#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host build of the glossy screen-space reflections' kernel bodies
# (csrc/ssr_pyramid_core.hpp, csrc/ssr_gloss_core.hpp) against their checker (tests/ssr_gloss_ref): a stand-alone program linked with the
# sanitizers' runtimes, so it needs no preload (tests/ssr_gloss_host/ssr_gloss_san_main.cpp).  CPU only.  Usage (from the repo root):
# tools/sanitize_ssr_gloss.sh
set -euo pipefail
cd "$(dirname "$0")/.."
export ASAN_OPTIONS=detect_leaks=0:abort_on_error=1:halt_on_error=1
export UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1
CLANG=/opt/rocm/lib/llvm/bin/clang
SAN_DIR=$(mktemp -d)
trap 'rm -rf "$SAN_DIR"' EXIT
"$CLANG" -O1 -g -std=c99 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/ssr_gloss_ref/ssr_gloss_ref.c -o "$SAN_DIR/ssr_gloss_ref.o"
"$CLANG"++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -I include \
    -I crychic_renderer_amd/csrc tests/ssr_gloss_host/ssr_gloss_san_main.cpp tests/ssr_gloss_host/ssr_gloss_host.cpp "$SAN_DIR/ssr_gloss_ref.o" -lm -o "$SAN_DIR/ssr_gloss_san"
"$SAN_DIR/ssr_gloss_san"
