#!/bin/bash
# Sanitizer run of the host side of the Fourier-Mellin passes: profiles/asan_auto_prior.cpp and the translation units that hold the code
# it calls (fmt.hip: the argument checks, the size arithmetic and the carve; fft.hip: the optimal DFT size; phasecorr.hip: the pairs per
# chunk, the Hanning factors; warppolar.hip: the warpPolar tables; the other three resolve fmt.hip's references) compiled with the
# HOST side instrumented (-Xarch_host -fsanitize=address,undefined) into one stand-alone program.  It initialises no GPU, needs none, and loads nothing into Python.
# usage: bash profiles/asan_auto_prior.sh      exit code 0 = no report and every check passed
set -eu
cd "$(dirname "$0")/.."
mkdir -p variants
C=radarslampy_amd/csrc
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer"
${HIPCC:-/opt/rocm/bin/hipcc} -O1 -g --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fno-fast-math $SAN -fsanitize=address,undefined \
    profiles/asan_auto_prior.cpp $C/fmt.hip $C/fft.hip $C/phasecorr.hip $C/warppolar.hip $C/fmt_batch.hip $C/fmt_register.hip $C/warpaffine.hip -o variants/asan_auto_prior
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1:exitcode=66 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1:exitcode=66 variants/asan_auto_prior
