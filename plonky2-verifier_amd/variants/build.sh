#!/bin/bash
# Measurement / isolation builds of libp2v with extra compile flags, loaded through P2V_LIB:
#   variants/build.sh <name> "<flags>"   ->   variants/libp2v_<name>.so
#   w7:    -DP2V_MERKLE_WAVES=7   (k_merkle at a forced 7 waves per SIMD)
# Built by the Makefile's own rules into variants/build_<name>, so a variant always holds the
# units the library does.
set -e
cd "$(dirname "$0")/.."
NAME=$1; EXTRA=$2
make -j16 BUILD=variants/build_$NAME LIB=variants/libp2v_$NAME.so EXTRA_HIPFLAGS="$EXTRA" variants/libp2v_$NAME.so
