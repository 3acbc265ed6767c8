#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host build of the colour grade's kernel body and table builder
# (csrc/grade_core.hpp) against its checker (tests/grade_ref), and over the .cube loader (csrc/host_textures.cpp) on hostile files: a
# stand-alone program linked with the sanitizers' runtimes, so it needs no preload (tests/grade_host/grade_san_main.cpp).  CPU only.
# Usage (from the repo root): tools/sanitize_grade.sh
set -euo pipefail
cd "$(dirname "$0")/.."
export ASAN_OPTIONS=detect_leaks=0:abort_on_error=1:halt_on_error=1
export UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1
CLANG=/opt/rocm/lib/llvm/bin/clang
SAN_DIR=$(mktemp -d)
trap 'rm -rf "$SAN_DIR"' EXIT
"$CLANG" -O1 -g -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/grade_ref/grade_ref.c -o "$SAN_DIR/grade_ref.o"
"$CLANG"++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -I include \
    -I crychic_renderer_amd/csrc tests/grade_host/grade_san_main.cpp tests/grade_host/grade_host.cpp crychic_renderer_amd/csrc/host_textures.cpp \
    "$SAN_DIR/grade_ref.o" -o "$SAN_DIR/grade_san"
mkdir "$SAN_DIR/files"
"$SAN_DIR/grade_san" "$SAN_DIR/files"
