// stages.cpp -- the one-shot stage entry points of include/hfdl_gpu.h: one kernel (or one short chain) on caller-supplied data, no
// front end.  Stage parity tests and the benches of single stages call them.
#include <cmath>
#include "frontend.h"

using namespace hfdl;

// kernel time of the last stage-level entry point called by this thread (HIP events around its launches, copies excluded)
static thread_local double g_stage_ms = 0.0;
extern "C" double hfdl_gpu_last_stage_ms(void) { return g_stage_ms; }

// the arguments have been checked: select the device, run the stage (demod_kernels.hip; a failure leaves its own text)
template <typename Call> static int run_stage(int device, Call call)
{
	const int rc = select_device(device);
	return rc ? rc : call();
}

extern "C" int hfdl_gpu_fft_forward(int device, const float *in, float *out, int32_t n, int shifted)
{
	if (!in || !out) return fail(HFDL_GPU_EINVAL, "null argument");
	int rc = select_device(device);
	if (rc) return rc;
	HostFftPlan plan;
	if ((rc = plan.build(n))) return rc;
	DevBuf d_in, d_work, d_out;
	const size_t bytes = sizeof(float2) * (size_t)n;
	HIP_TRY(d_in.alloc(bytes));
	HIP_TRY(d_work.alloc(bytes));
	HIP_TRY(d_out.alloc(bytes));
	HIP_TRY(hipMemcpy(d_in.p, in, bytes, hipMemcpyHostToDevice));
	StageTimer tm;
	launch_fft_forward(plan.p, nullptr, d_in.p, SFMT_CF32, 0, nullptr, d_work.as<float2>(), d_out.as<float2>(), shifted != 0, nullptr);
	g_stage_ms = tm.stop();
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpy(out, d_out.p, bytes, hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int hfdl_gpu_viterbi27(int device, const uint8_t *soft, int32_t nbits, int32_t nframes, uint8_t *out)
{
	if (!soft || !out || nbits <= 0 || nframes <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	return run_stage(device, [&] { g_stage_ms = 0.0; return demod_viterbi_batch(soft, nbits, nframes, out, &g_stage_ms); });
}

extern "C" int hfdl_gpu_burst_decode(int device, const float *symbols, const int32_t *modes, const int32_t *bitmask_lsb,
		int32_t nframes, uint8_t *octets, int32_t *lens)
{
	if (!symbols || !modes || !bitmask_lsb || !octets || !lens || nframes <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	for (int i = 0; i < nframes; i++) if (modes[i] < 0 || modes[i] > 7) return fail(HFDL_GPU_EINVAL, "mode out of range");
	return run_stage(device, [&] { g_stage_ms = 0.0; return demod_burst_decode_batch(symbols, modes, bitmask_lsb, nframes, octets, lens, &g_stage_ms); });
}

// decimating_shift_addition_init + decimating_shift_addition_cc (src/libcsdr_gpl.c:26-74) on the device: the NCO / decimator
// tail of the channelizer kernel as a stage of its own, state carried by the caller exactly like the reference's status struct
extern "C" int hfdl_gpu_nco_decimate(int device, const float *in, int32_t input_size, float rate, int32_t decimation,
		int32_t *decimation_remain, float *starting_phase, float *out, int32_t *output_size)
{
	if (!in || !decimation_remain || !starting_phase || !out || !output_size || input_size <= 0 || decimation <= 0 || *decimation_remain < 0)
		return fail(HFDL_GPU_EINVAL, "bad arguments");
	int rc = select_device(device);
	if (rc) return rc;
	float r = rate * (float)decimation;        // decimating_shift_addition_init -> shift_addition_init, fp32 products as written there
	r *= 2;
	const float sd = (float)std::sin(r * M_PI), cd = (float)std::cos(r * M_PI);
	NcoState st{};
	st.decimation_remain = *decimation_remain; st.starting_phase = *starting_phase;
	const size_t max_out = ((size_t)input_size + (size_t)decimation - 1) / (size_t)decimation;
	DevBuf d_in, d_out, d_ph, d_st;
	HIP_TRY(d_in.alloc(sizeof(float2) * (size_t)input_size));
	HIP_TRY(d_out.alloc(sizeof(float2) * max_out));
	HIP_TRY(d_ph.alloc(sizeof(float2) * max_out));
	HIP_TRY(d_st.alloc(sizeof(NcoState)));
	HIP_TRY(hipMemcpy(d_in.p, in, sizeof(float2) * (size_t)input_size, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_st.p, &st, sizeof(st), hipMemcpyHostToDevice));
	launch_nco_decimate(d_in.as<const float2>(), input_size, cd, sd, r, decimation, d_st.as<NcoState>(), d_ph.as<float2>(), d_out.as<float2>(), nullptr);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpy(&st, d_st.p, sizeof(st), hipMemcpyDeviceToHost));
	if (st.output_size > 0) HIP_TRY(hipMemcpy(out, d_out.p, sizeof(float2) * (size_t)st.output_size, hipMemcpyDeviceToHost));
	*decimation_remain = st.decimation_remain; *starting_phase = st.starting_phase; *output_size = st.output_size;
	return 0;
}

extern "C" int hfdl_gpu_crc16_ccitt(int device, const uint8_t *data, uint32_t len, uint16_t crc_init, uint16_t *crc)
{
	if (!crc || (!data && len)) return fail(HFDL_GPU_EINVAL, "bad arguments");
	return run_stage(device, [&] { return demod_crc16(data, len, crc_init, crc); });
}

// PDUs of a batch: at least one, each 1 .. stride octets long
static int check_pdu_lens(const int32_t *lens, int32_t npdus, int32_t stride)
{
	for (int i = 0; i < npdus; i++) if (lens[i] < 1 || lens[i] > stride) return fail(HFDL_GPU_EINVAL, "PDU %d: length %d outside 1..%d", i, lens[i], stride);
	return 0;
}

extern "C" int hfdl_gpu_pdu_triage(int device, const uint8_t *octets, const int32_t *lens, int32_t npdus, int32_t stride,
		uint8_t *fcs_status, uint8_t *pdu_kind, uint16_t *hdr_len)
{
	if (!octets || !lens || !fcs_status || !pdu_kind || !hdr_len || npdus <= 0 || stride <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	if (int rc = check_pdu_lens(lens, npdus, stride)) return rc;
	return run_stage(device, [&] { return demod_pdu_triage_batch(octets, lens, npdus, stride, fcs_status, pdu_kind, hdr_len); });
}

extern "C" int hfdl_gpu_lpdu_walk(int device, const uint8_t *octets, const int32_t *lens, int32_t npdus, int32_t stride, uint8_t *counts)
{
	if (!octets || !lens || !counts || npdus <= 0 || stride <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	if (int rc = check_pdu_lens(lens, npdus, stride)) return rc;
	return run_stage(device, [&] { return demod_lpdu_walk_batch(octets, lens, npdus, stride, counts); });
}

extern "C" int hfdl_gpu_psk_slice(int device, int32_t arity, const float *xy, int32_t n, uint32_t *sym, float *phase_error)
{
	if (!xy || !sym || !phase_error || n <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	if (arity < 1 || arity > 3) return fail(HFDL_GPU_EINVAL, "arity %d: HFDL uses BPSK, QPSK and 8-PSK (1..3 bits per symbol)", arity);
	return run_stage(device, [&] { return demod_psk_slice_batch(arity, xy, n, sym, phase_error); });
}
