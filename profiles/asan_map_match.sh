#!/bin/bash
# AddressSanitizer + UBSan over the host half of the map matching, as a stand-alone program (nothing is loaded into python):
# radarslampy_amd/csrc/map_match.h - the smear table, the angle table and the argument checks, plain C++ - compiled into
# profiles/asan_map_match.cpp and run on the CPU.
# usage: bash profiles/asan_map_match.sh      exit code 0 = no sanitizer report and every check passed
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
OUT=oracle/_build_asan
mkdir -p $OUT
g++ $SAN -std=c++17 -ffp-contract=off -Wall -Wextra -Wno-format-truncation profiles/asan_map_match.cpp -o $OUT/asan_map_match -lm
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $OUT/asan_map_match
