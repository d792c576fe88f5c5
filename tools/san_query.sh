#!/bin/bash
# The host side of tmpt_scene_hit_device, tmpt_query_keys and tmpt_query_plan under ASan + UBSan:
# tools/san_query.cpp, a program of its own linked against the SAN=1 library (host code
# instrumented, device code unchanged).  CPU only; no device call is made.
# Usage: tools/san_query.sh   (exit status 0 = clean)
set -o pipefail
cd "$(dirname "$0")/.."
make -s -C toymeshpathtracer_amd/csrc SAN=1 -j8 >/dev/null || exit 1
mkdir -p tools/_bin
L=$PWD/toymeshpathtracer_amd/_lib_san
/opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
    -Iinclude -o tools/_bin/san_query tools/san_query.cpp -L$L -ltmpt -Wl,-rpath,$L \
    -Wl,-rpath,$(dirname $(/opt/rocm/lib/llvm/bin/clang++ -print-file-name=libclang_rt.asan-x86_64.so)) || exit 1
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 tools/_bin/san_query
