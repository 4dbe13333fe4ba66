#!/bin/bash
# AddressSanitizer + UBSan over the CPU side of the blob bookkeeping, as a stand-alone program (nothing is loaded into python):
#   oracle/c/prune.c and csrc/blobprune_host.hip (the host instantiation of csrc/blobprune.h, compiled as plain C++) linked with
#   profiles/asan_blob_book.cpp, run on every case of tests/blob_book_cases.py.
# usage: bash profiles/asan_blob_book.sh      exit code 0 = no sanitizer report and oracle == host on every case
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
OUT=oracle/_build_asan
mkdir -p $OUT
PYTHONPATH="$PWD" python tests/blob_book_cases.py $OUT/blob_book_cases.bin
gcc $SAN -c -std=c11 -ffp-contract=off -fno-fast-math -D_GNU_SOURCE oracle/c/prune.c -o $OUT/prune_asan.o
g++ $SAN -std=c++17 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wno-unused-result \
    profiles/asan_blob_book.cpp -x c++ radarslampy_amd/csrc/blobprune_host.hip -x none $OUT/prune_asan.o -o $OUT/asan_blob_book -lm
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $OUT/asan_blob_book $OUT/blob_book_cases.bin
