// stages.cpp -- the one-shot stage entry points of include/hfdl_gpu.h, whole: one kernel (or one short chain) on caller-supplied data,
// no front end.  Each checks its arguments, selects the device, uploads its inputs (DevBuf::upload / zeroed, kernels.h), launches through
// the kernels' own launchers on the null stream (kernels.h, demod_launch.h), waits (finish_stage) and fetches its outputs.  Stage parity
// tests and the benches of single stages call them.
#include <cmath>
#include <cstring>
#include <vector>
#include "frontend.h"
#include "demod_launch.h"
#include "demod_tables.h"
#include "quality.h"

using namespace hfdl;

// kernel time of the last stage-level entry point called by this thread (HIP events around its launches, copies excluded)
static thread_local double g_stage_ms = 0.0;
extern "C" double hfdl_gpu_last_stage_ms(void) { return g_stage_ms; }

int hfdl::finish_stage()
{
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipGetLastError());
	return 0;
}

int StageFrames::upload(const float *symbols, const int32_t *modes, const int32_t *bitmask_lsb, int32_t nframes)
{
	DemodTables h;
	build_demod_tables(h, 0.6912f);
	std::vector<FrameRec> fr((size_t)nframes);
	std::vector<cf> sym((size_t)nframes * 2 * MAX_DATA_SYMBOLS);
	size_t off = 0;
	for (int i = 0; i < nframes; i++) {
		const size_t nsym = (size_t)mode_params(modes[i]).segments * 30;
		std::memcpy(&sym[(size_t)i * 2 * MAX_DATA_SYMBOLS], symbols + 2 * off, sizeof(cf) * nsym);
		off += nsym;
		FrameRec &f = fr[(size_t)i];
		std::memset(&f, 0, sizeof(f));
		f.channel = i; f.slot = 0; f.mode = modes[i]; f.bitmask_lsb = bitmask_lsb[i] & 1;
		f.signal_level = 1.0f; f.noise_floor = 1.0f;
		f.sample_index = (uint64_t)i;
	}
	HIP_TRY(scrambler.upload(h.scrambler, DEC_CONST_BYTES));
	HIP_TRY(frames.upload(fr.data(), sizeof(FrameRec) * fr.size()));
	HIP_TRY(data.upload(sym.data(), sizeof(cf) * sym.size()));
	return 0;
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
	HIP_TRY(d_in.upload(in, bytes));
	HIP_TRY(d_work.alloc(bytes));
	HIP_TRY(d_out.alloc(bytes));
	StageTimer tm;
	launch_fft_forward(plan.p, nullptr, d_in.p, SFMT_CF32, 0, nullptr, d_work.as<float2>(), d_out.as<float2>(), shifted != 0, nullptr);
	g_stage_ms = tm.stop();
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_out.fetch(out, bytes));
	return 0;
}

extern "C" int hfdl_gpu_viterbi27(int device, const uint8_t *soft, int32_t nbits, int32_t nframes, uint8_t *out)
{
	if (!soft || !out || nbits <= 0 || nframes <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	int rc = select_device(device);
	if (rc) return rc;
	g_stage_ms = 0.0;
	if ((rc = prepare_viterbi_batch(nbits))) return rc;
	const size_t out_bytes = (size_t)nframes * ((nbits + 7) / 8);
	DevBuf d_in, d_out;
	HIP_TRY(d_in.upload(soft, (size_t)nframes * 2 * nbits));
	HIP_TRY(d_out.zeroed(out_bytes));
	StageTimer tm;
	launch_viterbi_batch(d_in.as<const uint8_t>(), nbits, nframes, d_out.as<uint8_t>(), nullptr);
	g_stage_ms = tm.stop();
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_out.fetch(out, out_bytes));
	return 0;
}

extern "C" int hfdl_gpu_burst_decode(int device, const float *symbols, const int32_t *modes, const int32_t *bitmask_lsb,
		int32_t nframes, uint8_t *octets, int32_t *lens)
{
	if (!symbols || !modes || !bitmask_lsb || !octets || !lens || nframes <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	for (int i = 0; i < nframes; i++) if (modes[i] < 0 || modes[i] > 7) return fail(HFDL_GPU_EINVAL, "mode out of range");
	int rc = select_device(device);
	if (rc) return rc;
	g_stage_ms = 0.0;
	StageFrames in;
	if ((rc = in.upload(symbols, modes, bitmask_lsb, nframes))) return rc;
	// K5 as the pipeline launches it: a frame queue of `nframes` entries, all of them filled (counts[4]), a PDU ring with a slot for each
	const int counts[8] = { 0, 0, 0, 0, nframes, 0, 0, 0 };
	DevBuf d_counts, d_freqs, d_pdus;
	HIP_TRY(d_counts.upload(counts, sizeof(counts)));
	HIP_TRY(d_freqs.zeroed(sizeof(int32_t) * (size_t)nframes));
	HIP_TRY(d_pdus.alloc(sizeof(hfdl_gpu_pdu) * (size_t)nframes));
	if ((rc = prepare_burst_decode())) return rc;
	StageTimer tm;
	launch_burst_decode(in.frames.as<const FrameRec>(), d_counts.as<int>(), d_counts.as<int>() + 4, nullptr, nframes, in.data.as<const cf>(), 2,
			in.scrambler.as<const uint8_t>(), d_freqs.as<const int32_t>(), d_pdus.as<hfdl_gpu_pdu>(), nframes, nullptr, nullptr, nullptr);
	g_stage_ms = tm.stop();
	if ((rc = finish_stage())) return rc;
	std::vector<hfdl_gpu_pdu> pdus((size_t)nframes);
	HIP_TRY(d_pdus.fetch(pdus.data(), sizeof(hfdl_gpu_pdu) * pdus.size()));
	for (int i = 0; i < nframes; i++) lens[i] = 0;
	for (auto &p : pdus) {      // PDU slots are claimed in completion order: route by channel (= frame index)
		if (p.channel < 0 || p.channel >= nframes) continue;
		lens[p.channel] = p.len;
		std::memcpy(octets + (size_t)p.channel * HFDL_GPU_PDU_MAX_OCTETS, p.octets, (size_t)p.len);
	}
	return 0;
}

// the blanker's two launches as enqueue_fft queues them, on one block of one receiver
extern "C" int hfdl_gpu_blank_block(int device, const void *raw, int32_t n, int sample_format, float threshold_db,
		float *out, float *power, uint64_t *blanked)
{
	if (!raw || !out || !power || !blanked || n < 1 || n > BLANK_N_MAX || sample_format < SFMT_CF32 || sample_format > SFMT_CU8
			|| !(threshold_db >= BLANK_DB_MIN && threshold_db <= BLANK_DB_MAX))
		return fail(HFDL_GPU_EINVAL, "bad arguments");
	int rc = select_device(device);
	if (rc) return rc;
	DevBuf d_in, d_out, d_part, d_rec;
	hipError_t e = d_in.upload(raw, sample_bytes(sample_format) * (size_t)n);
	if (e == hipSuccess) e = d_out.alloc(sizeof(float2) * (size_t)n);
	if (e == hipSuccess) e = d_part.alloc(sizeof(float) * (size_t)blank_chunks(n));
	if (e == hipSuccess) e = d_rec.zeroed(sizeof(BlankRecord));
	HIP_TRY(e);
	BlankJob j;
	j.fresh[0] = d_in.p; j.out = d_out.as<float2>(); j.out_stride = n; j.partial = d_part.as<float>(); j.rec = d_rec.as<BlankRecord>();
	j.n = n; j.nrx = 1; j.fmt = sample_format; j.k2 = blank_k2(threshold_db);
	StageTimer tm;
	launch_blanker(j, nullptr);
	g_stage_ms = tm.stop();
	if ((rc = finish_stage())) return rc;
	BlankRecord rec;
	e = d_rec.fetch(&rec, sizeof(rec));
	if (e == hipSuccess) e = d_out.fetch(out, sizeof(float2) * (size_t)n);
	HIP_TRY(e);
	*power = rec.power;
	*blanked = rec.blanked;
	return 0;
}

// the I/Q corrector's launch as enqueue_fft queues it, on nblocks consecutive blocks of one receiver from a fresh enable (and a seed)
extern "C" int hfdl_gpu_iqbal_blocks(int device, const void *raw, int32_t n, int32_t nblocks, int sample_format, float alpha,
		const float *seed, int hold, float *out, hfdl_gpu_iqbal_stats *records)
{
	if (!raw || !out || !records || n < 1 || n > BLANK_N_MAX || nblocks < 1 || nblocks > IQBAL_BLOCKS_MAX || sample_format < SFMT_CF32 || sample_format > SFMT_CU8
			|| !iqbal_alpha_valid(alpha) || alpha == 0.f || (hold != 0 && hold != 1) || (!seed && hold) || (seed && !iqbal_seed_valid(seed[0], seed[1], seed[2], seed[3])))
		return fail(HFDL_GPU_EINVAL, "bad arguments");
	int rc = select_device(device);
	if (rc) return rc;
	const size_t N = (size_t)n, B = (size_t)nblocks, G = (size_t)blank_chunks(n);
	IqbalSeed sd = {};
	if (seed) { sd.k_re = seed[0]; sd.k_im = seed[1]; sd.m_re = seed[2]; sd.m_im = seed[3]; sd.gen = 1; sd.hold = (uint32_t)hold; }
	// block b reads state and chunk sums b and writes b + 1: the two slots of the pipeline, laid out as a row so every record is kept
	DevBuf d_in, d_out, d_part, d_state, d_seed;
	hipError_t e = d_in.upload(raw, sample_bytes(sample_format) * N * B);
	if (e == hipSuccess) e = d_out.alloc(sizeof(float2) * N * B);
	if (e == hipSuccess) e = d_part.alloc(sizeof(float) * (B + 1) * 5 * G);
	if (e == hipSuccess) e = d_state.zeroed(sizeof(IqbalState) * (B + 1));
	if (e == hipSuccess) e = d_seed.upload(&sd, sizeof(sd));
	HIP_TRY(e);
	StageTimer tm;
	for (size_t b = 0; b < B; b++) {
		IqbalJob j;
		j.fresh[0] = d_in.as<char>() + sample_bytes(sample_format) * N * b; j.alpha[0] = alpha;
		j.out = d_out.as<float2>() + N * b; j.out_stride = n;
		j.partial = d_part.as<float>() + b * 5 * G; j.state = d_state.as<IqbalState>() + b; j.seed = d_seed.as<IqbalSeed>();
		j.restart = b == 0; j.n = n; j.nrx = 1; j.fmt = sample_format; j.slot = 1;
		launch_iqbal(j, nullptr);
	}
	g_stage_ms = tm.stop();
	if ((rc = finish_stage())) return rc;
	std::vector<IqbalState> rec(B + 1);
	e = d_state.fetch(rec.data(), sizeof(IqbalState) * (B + 1));
	if (e == hipSuccess) e = d_out.fetch(out, sizeof(float2) * N * B);
	HIP_TRY(e);
	for (size_t b = 0; b < B; b++) iqbal_stats_of(rec[b + 1], records + b);
	return 0;
}

// the carrier canceller as the pipeline launches it in a half's hand-over: one "block" of nch rows of n samples each, every channel selected
extern "C" int hfdl_gpu_notch_rows(int device, const float *x, int32_t nch, int32_t n, float mu, float *state, float *y)
{
	if (!x || !y || nch < 1 || n < 1 || (int64_t)nch * n > ((int64_t)1 << 27) || !notch_mu_valid(mu)) return fail(HFDL_GPU_EINVAL, "bad arguments");
	int rc = select_device(device);
	if (rc) return rc;
	const size_t row_bytes = sizeof(float2) * (size_t)nch * (size_t)n, state_bytes = sizeof(float) * NOTCH_STATE_FLOATS * (size_t)nch;
	DevBuf d_in, d_out, d_state, d_rec;
	hipError_t e = d_in.upload(x, row_bytes);
	if (e == hipSuccess) e = d_out.alloc(row_bytes);
	if (e == hipSuccess) e = state ? d_state.upload(state, state_bytes) : d_state.zeroed(state_bytes);
	if (e == hipSuccess) e = d_rec.zeroed(sizeof(NotchRecord) * (size_t)nch);
	HIP_TRY(e);
	NotchJob j;
	j.in = d_in.as<const float2>(); j.out = d_out.as<float2>(); j.state = d_state.as<float>(); j.rec = d_rec.as<NotchRecord>();
	j.nch = nch; j.outs = n; j.nblk = 1; j.nsel = nch; j.mu = mu;
	StageTimer tm;
	launch_notch(j, nullptr);
	g_stage_ms = tm.stop();
	if ((rc = finish_stage())) return rc;
	e = d_out.fetch(y, row_bytes);
	if (e == hipSuccess && state) e = d_state.fetch(state, state_bytes);
	HIP_TRY(e);
	return 0;
}

// frame_quality_kernel as the pipeline launches it behind K5, on K5's staged frames, without a ring: frame i writes record i
extern "C" int hfdl_gpu_frame_quality_batch(int device, const float *symbols, const int32_t *modes, int32_t nframes, hfdl_gpu_frame_quality *out)
{
	if (!symbols || !modes || !out || nframes <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	for (int i = 0; i < nframes; i++) if (modes[i] < 0 || modes[i] > 7) return fail(HFDL_GPU_EINVAL, "mode out of range");
	int rc = select_device(device);
	if (rc) return rc;
	g_stage_ms = 0.0;
	StageFrames in;
	const std::vector<int32_t> masks((size_t)nframes, 0);
	if ((rc = in.upload(symbols, modes, masks.data(), nframes))) return rc;
	DevBuf d_count, d_recs;
	HIP_TRY(d_count.upload(&nframes, sizeof(nframes)));
	HIP_TRY(d_recs.zeroed(sizeof(hfdl_gpu_frame_quality) * (size_t)nframes));
	StageTimer tm;
	launch_frame_quality(in.frames.as<const FrameRec>(), d_count.as<const int>(), nframes, in.data.as<const cf>(), 2,
			(const float *)(in.scrambler.as<const uint8_t>() + DEC_PSK_OFFSET), nullptr, nullptr, d_recs.as<hfdl_gpu_frame_quality>(), nullptr, 0, nullptr);
	g_stage_ms = tm.stop();
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_recs.fetch(out, sizeof(hfdl_gpu_frame_quality) * (size_t)nframes));
	for (int i = 0; i < nframes; i++) {        // what only a front end knows (StageFrames numbers its frames; unit levels are 0 dB already)
		out[i].sample_index = 0;
		out[i].channel = 0;
	}
	return 0;
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
	HIP_TRY(d_in.upload(in, sizeof(float2) * (size_t)input_size));
	HIP_TRY(d_out.alloc(sizeof(float2) * max_out));
	HIP_TRY(d_ph.alloc(sizeof(float2) * max_out));
	HIP_TRY(d_st.upload(&st, sizeof(st)));
	launch_nco_decimate(d_in.as<const float2>(), input_size, cd, sd, r, decimation, d_st.as<NcoState>(), d_ph.as<float2>(), d_out.as<float2>(), nullptr);
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_st.fetch(&st, sizeof(st)));
	if (st.output_size > 0) HIP_TRY(d_out.fetch(out, sizeof(float2) * (size_t)st.output_size));
	*decimation_remain = st.decimation_remain; *starting_phase = st.starting_phase; *output_size = st.output_size;
	return 0;
}

extern "C" int hfdl_gpu_crc16_ccitt(int device, const uint8_t *data, uint32_t len, uint16_t crc_init, uint16_t *crc)
{
	if (!crc || (!data && len)) return fail(HFDL_GPU_EINVAL, "bad arguments");
	int rc = select_device(device);
	if (rc) return rc;
	DevBuf d_in, d_out;
	HIP_TRY(d_in.upload(data, len));         // len = 0: one byte nobody reads (DevBuf::alloc)
	HIP_TRY(d_out.alloc(sizeof(uint32_t)));
	launch_crc16(d_in.as<const uint8_t>(), len, crc_init, d_out.as<uint32_t>(), nullptr);
	if ((rc = finish_stage())) return rc;
	uint32_t v = 0;
	HIP_TRY(d_out.fetch(&v, sizeof(v)));
	*crc = (uint16_t)v;
	return 0;
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
	int rc = check_pdu_lens(lens, npdus, stride);
	if (rc || (rc = select_device(device))) return rc;
	const size_t n = (size_t)npdus;
	DevBuf d_oct, d_lens, d_fcs, d_kind, d_hl;
	HIP_TRY(d_oct.upload(octets, n * (size_t)stride));
	HIP_TRY(d_lens.upload(lens, n * sizeof(int32_t)));
	HIP_TRY(d_fcs.alloc(n));
	HIP_TRY(d_kind.alloc(n));
	HIP_TRY(d_hl.alloc(n * sizeof(uint16_t)));
	launch_pdu_triage(d_oct.as<const uint8_t>(), d_lens.as<const int32_t>(), npdus, stride, d_fcs.as<uint8_t>(), d_kind.as<uint8_t>(), d_hl.as<uint16_t>(), nullptr);
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_fcs.fetch(fcs_status, n));
	HIP_TRY(d_kind.fetch(pdu_kind, n));
	HIP_TRY(d_hl.fetch(hdr_len, n * sizeof(uint16_t)));
	return 0;
}

extern "C" int hfdl_gpu_lpdu_walk(int device, const uint8_t *octets, const int32_t *lens, int32_t npdus, int32_t stride, uint8_t *counts)
{
	if (!octets || !lens || !counts || npdus <= 0 || stride <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	int rc = check_pdu_lens(lens, npdus, stride);
	if (rc || (rc = select_device(device))) return rc;
	const size_t n = (size_t)npdus;
	DevBuf d_oct, d_lens, d_cnt;
	HIP_TRY(d_oct.upload(octets, n * (size_t)stride));
	HIP_TRY(d_lens.upload(lens, n * sizeof(int32_t)));
	HIP_TRY(d_cnt.alloc(n * 5));
	launch_lpdu_walk(d_oct.as<const uint8_t>(), d_lens.as<const int32_t>(), npdus, stride, d_cnt.as<uint8_t>(), nullptr);
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_cnt.fetch(counts, n * 5));
	return 0;
}

extern "C" int hfdl_gpu_psk_slice(int device, int32_t arity, const float *xy, int32_t n, uint32_t *sym, float *phase_error)
{
	if (!xy || !sym || !phase_error || n <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	if (arity < 1 || arity > 3) return fail(HFDL_GPU_EINVAL, "arity %d: HFDL uses BPSK, QPSK and 8-PSK (1..3 bits per symbol)", arity);
	int rc = select_device(device);
	if (rc) return rc;
	DemodTables h;
	build_demod_tables(h, 0.6912f);
	DevBuf d_x, d_pts, d_sym, d_err;
	HIP_TRY(d_x.upload(xy, sizeof(cf) * (size_t)n));
	HIP_TRY(d_pts.upload(h.psk_pts, sizeof(h.psk_pts)));
	HIP_TRY(d_sym.alloc(sizeof(uint32_t) * (size_t)n));
	HIP_TRY(d_err.alloc(sizeof(float) * (size_t)n));
	launch_psk_slice(arity, d_x.as<const cf>(), n, d_pts.as<const float>(), d_sym.as<uint32_t>(), d_err.as<float>(), nullptr);
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_sym.fetch(sym, sizeof(uint32_t) * (size_t)n));
	HIP_TRY(d_err.fetch(phase_error, sizeof(float) * (size_t)n));
	return 0;
}
