# The objects of libhfdl_gpu.so, in ONE place: build.sh compiles and links them, build_strict.sh links the same list with its own
# demodulator object.  Kernel objects come from <name>.hip, the shim's from <name>.cpp.  demod_host (the owner of a front end's
# demodulator state), stages (the one-shot stage entry points) and lab are the shim's: they meet the demodulator's kernels through
# demod_launch.h alone, so the strict builds' kernel object links with them as the product's does.
KERNEL_OBJS="fft_kernels fold_kernels demod_kernels spectrum_kernels"
SHIM_OBJS="hfdl_gpu frontend_create frontend_query frontend_options frontend_quality demod_host stages lab"
# Kernel files compiled INTO another file's object (hipcc --include=<name>.hip: in front of it): the opt-in features share ONE code object
# -- the library's count of code objects and its size are pinned (tests/test_retune_device_cpu.py, tests/test_host_logic_cpu.py), and a
# code object of its own costs 14 KB of headers and padding around 6 KB of code.  INCLUDED_<object>="<names>".
INCLUDED_spectrum_kernels="quality_kernels blanker_kernels iqbal_kernels notch_kernels"
# real-sampled input's two kernels ride with the forward FFT they sit behind; that object is compiled WITH contraction, so real_kernels
# and real_input.h switch it off inside their own functions (a file-wide switch would reach the FFT passes behind the include)
INCLUDED_fft_kernels="real_kernels"
# demodulator, spectrum monitor and frame quality: no FMA contraction, so the fp32 recurrences round exactly like the plain-C oracle's,
# the monitor's fp32 sums are what tests/spectrum_f64.py emulates term for term, and the quality figures are what the host build of
# quality.h computes (quality_kernels rides in spectrum_kernels' object); the blanker's block power is what the host build of blanker.h adds
# up (blanker_kernels rides there too), the carrier canceller's recurrence rounds like the host build of notch.h (notch_kernels as well), and
# the I/Q corrector's sums, state and output are the host build of iqbal.h's word for word (iqbal_kernels, behind blanker_kernels, whose loads it shares)
NO_CONTRACT_OBJS="demod_kernels spectrum_kernels"
