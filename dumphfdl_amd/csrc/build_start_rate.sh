#!/bin/bash
# TEST-ONLY pair of builds (never shipped, never loaded by default) with the timing loop's start rate overridden at compile time
# (-DHFDL_DM_SS_RATE0=<rate>, demod_logic.h): the product's sources as they are, and the strict build with every fast form on
# (tests/hostsim/strict_demod_kernels.hip, -DHFDL_DM_STRICT_FAST=15), every object of both compiled with the same flag.  With a start
# rate of about 1 the timing-recovery wave produces 0, 1 or 2 outputs per input sample: tests/test_gpu_demod_search_run.py compares the
# two word for word.  Output: build/start_rate/libhfdl_gpu_rate.so and libhfdl_gpu_rate_strict.so at the repository root.
set -e
cd "$(dirname "$0")"
. ./objects.sh
RATE=${1:-1.0f}
OUTDIR=../../build/start_rate
mkdir -p $OUTDIR
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
HFDL_OUT=$OUTDIR/libhfdl_gpu_rate.so HFDL_BUILD_DIR=$OUTDIR/obj HFDL_EXTRA_FLAGS="-DHFDL_DM_SS_RATE0=$RATE" bash build.sh > /dev/null
objs=""
for o in $KERNEL_OBJS $SHIM_OBJS; do
	if [ $o = demod_kernels ]; then objs="$objs $OUTDIR/demod_kernels_strict.o"; else objs="$objs $OUTDIR/obj/$o.o"; fi
done
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=off -DHFDL_DM_STRICT_FAST=15 -DHFDL_DM_SS_RATE0=$RATE -I. \
	-c ../../tests/hostsim/strict_demod_kernels.hip -o $OUTDIR/demod_kernels_strict.o
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -o $OUTDIR/libhfdl_gpu_rate_strict.so $objs
ls -la $OUTDIR/*.so
