#!/bin/bash
# Build libhfdl_gpu.so for gfx950 (cross-compiles without a GPU).  Output lands next to the package (in-tree).
#   build.sh          the product library: the tilings the front end can pick, no probes, no A/B switches
#   build.sh lab      libhfdl_gpu_lab.so from the same sources with -DHFDL_LAB: + the tiling sweep, the probes of
#                     include/hfdl_gpu_lab.h and the A/B environment switches (profiles/*.py, bench.py's stream-read probe)
set -e
cd "$(dirname "$0")"
. ./objects.sh
if [ "$1" = "lab" ]; then
	OUT=${HFDL_OUT:-../libhfdl_gpu_lab.so}
	BUILD=${HFDL_BUILD_DIR:-../build/lab}
	HFDL_EXTRA_FLAGS="-DHFDL_LAB ${HFDL_EXTRA_FLAGS:-}"
else
	OUT=${HFDL_OUT:-../libhfdl_gpu.so}          # HFDL_OUT / HFDL_EXTRA_FLAGS: side-by-side builds for A/B measurements
	BUILD=${HFDL_BUILD_DIR:-../build}
fi
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# The HOST half of every object is compiled without exception and unwind tables: the shim has no try, catch or throw, an uncaught C++
# exception ends the process at the C ABI either way, and the tables were 25 KB of a library whose size is pinned
# (tests/test_host_logic_cpu.py).  The device pass never sees the flags.
NO_UNWIND="-Xarch_host -fno-exceptions -Xarch_host -fno-asynchronous-unwind-tables -Xarch_host -fno-unwind-tables"
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $NO_UNWIND ${HFDL_EXTRA_FLAGS:-}"
mkdir -p $BUILD
pids=""
objs=""
for o in $KERNEL_OBJS; do
	case " $NO_CONTRACT_OBJS " in *" $o "*) contract=-ffp-contract=off ;; *) contract= ;; esac
	riders=INCLUDED_$o; included=""
	for r in ${!riders}; do included="$included --include=$r.hip"; done
	$HIPCC $COMMON $contract $included -c $o.hip -o $BUILD/$o.o & pids="$pids $!"
	objs="$objs $BUILD/$o.o"
done
# The shim's HOST code is compiled for size (-Xarch_host -Os: launch bookkeeping, checks and copies, nothing a block's time depends on);
# the device pass keeps -O3, and the library's device code is byte for byte what it is without the flag.  The
# library's size is pinned (tests/test_host_logic_cpu.py).
for o in $SHIM_OBJS; do
	$HIPCC $COMMON -Xarch_host -Os -x hip -c $o.cpp -o $BUILD/$o.o & pids="$pids $!"
	objs="$objs $BUILD/$o.o"
done
for p in $pids; do wait $p; done          # set -e: a failed compile stops the build here instead of linking stale objects
# -Bsymbolic: calls between the library's own entry points stay inside THIS library when the product and the laboratory build
# are loaded into one process.  The product library is linked without a static symbol table (-s; the dynamic one, which is what a
# caller binds to, stays): a change to the link alone, every object file is what it was.  The laboratory build keeps its table for
# profiles and backtraces.  exports.map: only the public entry points are dynamic symbols (a change to the link alone as well).
[ "$1" = "lab" ] && STRIP= || STRIP=-Wl,-s
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -Wl,--version-script=exports.map $STRIP -o $OUT $objs
echo "built $(readlink -f $OUT)"
