# The objects of libhfdl_gpu.so, in ONE place: build.sh compiles and links them, build_strict.sh links the same list with its own
# demodulator object.  Kernel objects come from <name>.hip, the shim's from <name>.cpp.  demod_host (the owner of a front end's
# demodulator state), stages (the one-shot stage entry points) and lab are the shim's: they meet the demodulator's kernels through
# demod_launch.h alone, so the strict builds' kernel object links with them as the product's does.
KERNEL_OBJS="fft_kernels fold_kernels demod_kernels spectrum_kernels"
SHIM_OBJS="hfdl_gpu frontend_create frontend_query demod_host stages lab"
# demodulator and spectrum monitor: no FMA contraction, so the fp32 recurrences round exactly like the plain-C oracle's and the
# monitor's fp32 sums are what tests/spectrum_f64.py emulates term for term
NO_CONTRACT_OBJS="demod_kernels spectrum_kernels"
