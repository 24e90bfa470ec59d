// retune_launch.h -- internal: the launcher of the retune's channelizer-side kernel (fft_kernels.hip, beside the rider workgroups that own
// the arrays it writes), for the shim (hfdl_gpu.cpp hfdl_gpu_frontend_retune_channel).  The demodulator's side is in demod_launch.h.
#pragma once
#include "kernels.h"

namespace hfdl {

// cc[c] = k, chain[c] and cont[c] as create left them (zero); `done` (optional) rides on the dispatch
void launch_retune_channelizer(ChanConst *cc, NcoState *chain, float2 *cont, int c, const ChanConst &k, hipStream_t st, hipEvent_t done = nullptr);

}  // namespace hfdl
