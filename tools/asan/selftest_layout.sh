#!/bin/bash
# AddressSanitizer + UBSan over the host side of the self-tests (tools/asan/selftest_layout.cpp):
# api_selftest.cpp and circuit.cpp are compiled with the sanitizers (host side only) and linked
# with the other objects of a finished `make` into a stand-alone program.  CPU only; no device is
# opened.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
PKG=../../plonky2-verifier_amd
OUT=${OUT:-/tmp/p2v_asan}
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined"
mkdir -p $OUT
XSAN=$(for f in $SAN; do printf -- '-Xarch_host %s ' $f; done)
$HIPCC -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-result $XSAN -x hip -c -o $OUT/api_selftest.o $PKG/csrc/api_selftest.cpp
$HIPCC -O1 -g -std=c++17 -fPIC $SAN -c -o $OUT/circuit.o $PKG/csrc/circuit.cpp
$HIPCC -O1 -g -std=c++17 $SAN -c -o $OUT/selftest_layout.o selftest_layout.cpp
OBJS=$(ls $PKG/build/*.o | grep -v -e '/api_selftest\.o$' -e '/circuit\.o$')
$HIPCC --offload-arch=gfx950 $SAN -o $OUT/selftest_layout $OUT/selftest_layout.o $OUT/api_selftest.o $OUT/circuit.o $OBJS
ASAN_OPTIONS=detect_leaks=1 $OUT/selftest_layout
