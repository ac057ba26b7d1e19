#!/bin/bash
# ASan + UBSan over the host-only code paths (no GPU): scenes, cameras, scene records, BVH builder/verifier, oracle.
# pt_host.cpp and pt_bvh_check.cpp are the part of the C ABI that needs no device: they take float4 from the HIP headers and link no HIP library.
set -e
cd "$(dirname "$0")/../.."
OUT=${1:-/tmp/pt_san_driver}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
HIPINC="-D__HIP_PLATFORM_AMD__ -I/opt/rocm/include"
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 $SAN $HIPINC -Wno-unused-value -x c++ \
    tests/tools/san_driver.cpp pathtrace_amd/csrc/pt_bvh.cpp pathtrace_amd/csrc/pt_scenes.cpp pathtrace_amd/csrc/pt_host.cpp pathtrace_amd/csrc/pt_bvh_check.cpp \
    -x c++ oracle/oracle_capi.cpp -ffp-contract=off -lpthread -o "$OUT"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1 "$OUT"
