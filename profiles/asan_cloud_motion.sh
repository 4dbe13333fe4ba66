#!/bin/bash
# AddressSanitizer + UBSan over the host half of the peak clouds' motion compensation, as a stand-alone program (nothing is loaded
# into python): radarslampy_amd/csrc/cloud_motion.h - the velocity checks of the adds and the motion table, plain C++ - compiled into
# profiles/asan_cloud_motion.cpp and run on the CPU.
# usage: bash profiles/asan_cloud_motion.sh      exit code 0 = no sanitizer report and every check passed
set -eu
cd "$(dirname "$0")/.."
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
OUT=oracle/_build_asan
mkdir -p $OUT
g++ $SAN -std=c++17 -ffp-contract=off -Wall -Wextra -Wno-format-truncation profiles/asan_cloud_motion.cpp -o $OUT/asan_cloud_motion -lm
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $OUT/asan_cloud_motion
