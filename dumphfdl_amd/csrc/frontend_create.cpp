// frontend_create.cpp -- builds and destroys a front end: argument checks, geometry, streams and events, allocation, the filter taps.
#include <atomic>
#include <cmath>
#include <complex>
#include <cstring>
#include <thread>
#include "frontend.h"

using namespace hfdl;

extern "C" int hfdl_gpu_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int hfdl::select_device(int device)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
		return fail(HFDL_GPU_ENODEV, "no HIP device visible: the HFDL front end has no CPU fallback");
	if (device < 0 || device >= n) return fail(HFDL_GPU_EINVAL, "device %d out of range (%d visible)", device, n);
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(HFDL_GPU_ENODEV, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
	return 0;
}

// ---------------------------------------------------------------- FFT plan

int hfdl::upload_twiddles(int r, DevBuf &out)
{
	std::vector<float2> h((size_t)r);
	for (int t = 0; t < r; t++) {
		double a = -2.0 * M_PI * (double)t / (double)r;
		h[t] = make_float2((float)std::cos(a), (float)std::sin(a));
	}
	HIP_TRY(out.alloc(sizeof(float2) * (size_t)r));
	HIP_TRY(hipMemcpy(out.p, h.data(), sizeof(float2) * (size_t)r, hipMemcpyHostToDevice));
	return 0;
}

int HostFftPlan::build(int n)
{
	int logn = ilog2(n);
	if ((1 << logn) != n || logn < 9 || logn > 24) return fail(HFDL_GPU_ERANGE, "fft size %d unsupported (need 2^9..2^24)", n);
	// balanced split, largest radix last-but-one; every radix <= 256 so a 16-column tile fits 32 KiB of LDS
	int l1 = (logn + 2) / 3, l2 = (logn - l1 + 1) / 2, l3 = logn - l1 - l2;
	p.n = n; p.logn = logn;
	p.l1 = l1; p.l2 = l2; p.l3 = l3;
	p.r1 = 1 << l1; p.r2 = 1 << l2; p.r3 = 1 << l3;
	const int radix[3] = { p.r1, p.r2, p.r3 };
	for (int i = 0; i < 3; i++) if (int rc = upload_twiddles(radix[i], tw[i])) return rc;
	p.tw1 = tw[0].as<float2>(); p.tw2 = tw[1].as<float2>(); p.tw3 = tw[2].as<float2>();
	return 0;
}

// ---------------------------------------------------------------- create-time configuration

// From the environment (include/hfdl_gpu.h documents every name).  Read at every create and never cached: there is no function-local
// static to race on when front ends are created from several threads.
long hfdl::env_long(const char *name, long lo, long hi, long otherwise)
{
	const char *e = getenv(name);
	if (!e || !*e) return otherwise;
	char *end = nullptr;
	const long v = strtol(e, &end, 10);
	return (end != e && v >= lo && v <= hi) ? v : otherwise;
}

static double env_double(const char *name, double lo, double hi, double otherwise)
{
	const char *e = getenv(name);
	if (!e || !*e) return otherwise;
	char *end = nullptr;
	const double v = strtod(e, &end);
	return (end != e && v >= lo && v <= hi) ? v : otherwise;
}

// The pruned fold: the energy of the taps per (alias row, slot) from the device, the windows from planner.h fold_row_windows
static int build_fold_windows(hfdl_gpu_frontend *fe)
{
	Geometry &g = fe->geo;
	DevBuf d_en;
	std::vector<float> en((size_t)g.pre * (size_t)g.nch_pad);
	HIP_TRY(d_en.alloc(sizeof(float) * en.size()));
	HIP_TRY(hipMemsetAsync(d_en.p, 0, sizeof(float) * en.size(), fe->stream));
	launch_tap_row_energy(fe->d_taps, g, d_en.as<float>(), fe->stream);
	HIP_TRY(hipMemcpyAsync(en.data(), d_en.p, sizeof(float) * en.size(), hipMemcpyDeviceToHost, fe->stream));
	HIP_TRY(hipStreamSynchronize(fe->stream));
	const std::vector<RowWindow> w = fold_row_windows(en, g.pre, g.nch_pad, g.nch, fe->prune_tol, &fe->fold_rows_max);
	static_assert(sizeof(RowWindow) == sizeof(int2), "a window is what the fold kernels load as an int2 { first quad, count }");
	HIP_TRY(fe->alloc(fe->d_win, w.size()));
	HIP_TRY(hipMemcpy(fe->d_win, w.data(), sizeof(int2) * w.size(), hipMemcpyHostToDevice));
	g.fold_win = fe->d_win;
	return 0;
}

bool design_channel(const hfdl_gpu_frontend *fe, int rx, int32_t freq, ChanConst &k, std::complex<float> *taps, std::vector<float> &lp, float &lp_cut)
{
	// src/hfdl.c:476: shift relative to the SSB carrier 1440 Hz above the channel frequency -- from the centre of ITS receiver
	float shift = (float)(fe->rx_center[(size_t)rx] - (freq + 1440)) / (float)fe->sample_rate;
	if (fe->real_rate) shift = real_shift(fe->real_rate, fe->rx_base[(size_t)rx], freq);      // the equivalent stream's, its centre taken exactly
	Plan cp;
	if (!plan_block(cp, fe->tbw, fe->decimation, shift)) return false;
	k = ChanConst{};
	k.offsetbin = cp.offsetbin;
	k.nco_sindelta = cp.sindelta; k.nco_cosdelta = cp.cosdelta; k.nco_rate = cp.rate;
	k.frequency = freq;
	if (taps == nullptr) return true;          // the constants alone
	if (fe->real_rate) {
		// designed at the REAL rate, 2 overlap' + 1 taps, then split into the even and the odd ones (real_input.h)
		// -- the one function the host build calls too, so the words are that build's by construction
		std::vector<std::complex<float>> h((size_t)real_taps_length(fe->plan.taps_length));
		real_design_taps(fe->real_rate, fe->rx_base[(size_t)rx], freq, fe->decimation, fe->plan.taps_length, h.data(), taps, lp, lp_cut);
		return true;
	}
	float half_bw = 0.5f / fe->decimation;
	design_bandpass(taps, fe->plan.taps_length, (-shift) - half_bw, (-shift) + half_bw, lp, lp_cut);
	return true;
}

int queue_real_taps(hfdl_gpu_frontend *fe, const float2 *host, float2 *pad, float2 *work, float2 *eo, int slot, hipStream_t st, hipEvent_t staged)
{
	const size_t T = (size_t)fe->plan.taps_length, n = (size_t)fe->plan.n;
	for (int half = 0; half < 2; half++) {
		HIP_TRY(hipMemcpyAsync(pad, host + (size_t)half * T, sizeof(float2) * T, hipMemcpyHostToDevice, st));
		launch_fft_forward(fe->fft.p, nullptr, pad, SFMT_CF32, 0, nullptr, work, eo + (size_t)half * n, false, st, FftOutLayout(), nullptr, NcoJob(), half ? staged : nullptr);
	}
	RealTapJob j;
	j.e = eo; j.o = eo + n; j.taps = (float *)fe->d_taps; j.rs_f = (size_t)fe->geo.tap_row_stride * 2;
	j.n = fe->plan.n; j.logn = ilog2(fe->plan.n); j.m_log = ilog2(fe->plan.m); j.kind = fe->geo.tap_layout; j.slot = slot;
	launch_real_tap_combine(j, st);
	return 0;
}

static int build_taps(hfdl_gpu_frontend *fe)
{
	const Plan &pl = fe->plan;
	const int nch = (int)fe->freqs.size();
	const size_t n = (size_t)pl.n;
	// time-domain taps on the host (exact reference arithmetic), one worker per hardware thread
	const size_t per = fe->taps_host_len();
	std::vector<std::complex<float>> host((size_t)nch * per);
	fe->cc.resize((size_t)nch);
	unsigned nthreads = std::max(1u, std::min((unsigned)nch, std::thread::hardware_concurrency()));
	// several front ends created at once on one host (one process per GPU): share the cores
	nthreads = std::min(nthreads, (unsigned)env_long("HFDL_GPU_HOST_THREADS", 1, 1 << 16, (long)nthreads));
	std::atomic<int> next{0};
	std::atomic<int> bad{0};
	auto work = [&]() {
		std::vector<float> lp;
		float lp_cut = -1.f;
		for (;;) {
			int c = next.fetch_add(1);
			if (c >= nch) break;
			if (!design_channel(fe, fe->rx_of[(size_t)c], fe->freqs[c], fe->cc[c], host.data() + (size_t)c * per, lp, lp_cut)) bad++;
		}
	};
	std::vector<std::thread> pool;
	for (unsigned t = 1; t < nthreads; t++) pool.emplace_back(work);
	work();
	for (auto &t : pool) t.join();
	if (bad) return fail(HFDL_GPU_EINVAL, "fastddc planning failed for %d channel(s)", (int)bad);

	// frequency-domain taps on the device: zero-pad to N, forward FFT, fftshift (src/fastddc.c:231-240)
	DevBuf pad;
	HIP_TRY(pad.alloc(sizeof(float2) * n));
	float2 *d_pad = pad.as<float2>();
	HIP_TRY(hipMemsetAsync(d_pad, 0, sizeof(float2) * n, fe->stream));
	if (fe->geo.nch_pad > nch)          // the slots that fill each receiver's last group of the interleaved layout up: all-zero taps
		HIP_TRY(hipMemsetAsync(fe->d_taps, 0, sizeof(float2) * n * (size_t)fe->geo.nch_pad, fe->stream));
	DevBuf eo;
	if (fe->real_rate) HIP_TRY(eo.alloc(sizeof(float2) * 2 * n));
	for (int c = 0; c < nch; c++) {
		if (fe->real_rate) {
			// real input: the transforms of the even and the odd taps, combined into the slot
			if (int rc = queue_real_taps(fe, (const float2 *)(host.data() + (size_t)c * per), d_pad, fe->d_work, eo.as<float2>(), fe->slot_of(c), fe->stream, nullptr)) return rc;
			continue;
		}
		HIP_TRY(hipMemcpyAsync(d_pad, host.data() + (size_t)c * pl.taps_length, sizeof(float2) * (size_t)pl.taps_length,
				hipMemcpyHostToDevice, fe->stream));
		// the last pass writes the channel's filter straight into the matrix-operand layout (kernels.h tap_index_f), at its padded slot
		const int slot = fe->slot_of(c);
		FftOutLayout lay = fe->tap_layout;
		lay.chan = slot;
		float2 *dst = lay.kind == TAPL_PLAIN ? fe->d_taps + (size_t)slot * (size_t)fe->geo.tap_chan_stride : fe->d_taps;
		if (fe->geo.mix_l1) {
			// the mixed domain: passes 1 and 2, then R3 T[k1, k2, -n3] into the same layout at (row rho, bin j')
			FftVariant v;
			v.passes = FFT_PASSES_12;
			launch_fft_forward(fe->fft.p, nullptr, d_pad, SFMT_CF32, 0, nullptr, fe->d_work, nullptr, true, fe->stream, FftOutLayout(), nullptr, NcoJob(), nullptr, nullptr, v);
			launch_mixed_tap_pack(fe->fft.p, fe->geo, fe->d_work, fe->d_taps, slot, fe->stream);
		} else launch_fft_forward(fe->fft.p, nullptr, d_pad, SFMT_CF32, 0, nullptr, fe->d_work, dst, true, fe->stream, lay);
	}
	HIP_TRY(hipStreamSynchronize(fe->stream));
	HIP_TRY(hipGetLastError());
	return 0;
}

// span check of src/main.c:214-226, against the channel's own receiver
int hfdl::check_channel_span(int32_t sample_rate, int32_t nrx, int c, int32_t freq, int r, int32_t centre)
{
	if (std::abs((int64_t)centre - freq) < sample_rate / 2) return 0;
	return nrx == 1 ? fail(HFDL_GPU_EINVAL, "channel %d Hz outside +-fs/2 of centre %d", freq, centre)
	                : fail(HFDL_GPU_EINVAL, "channel %d (%d Hz) outside +-fs/2 of the centre %d of its receiver %d", c, freq, centre, r);
}

// Every argument is checked here, before a device is selected (the checks need no GPU)
static int check_create_args(hfdl_gpu_frontend **out, int32_t sample_rate, int32_t nrx, const int32_t *centerfreqs, const int32_t *freqs,
		const int32_t *nch_per_rx)
{
	if (!out || !centerfreqs || !freqs || !nch_per_rx) return fail(HFDL_GPU_EINVAL, "bad arguments: null pointer");
	*out = nullptr;
	if (nrx < 1 || nrx > HFDL_GPU_RECEIVERS_MAX) return fail(HFDL_GPU_EINVAL, "bad arguments: %d receivers (1 .. %d)", nrx, HFDL_GPU_RECEIVERS_MAX);
	for (int r = 0; r < nrx; r++)
		if (nch_per_rx[r] <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments: receiver %d has %d channels", r, nch_per_rx[r]);
	if (sample_rate < 5400) return fail(HFDL_GPU_EINVAL, "sample rate must be >= 5400 (src/main.c:638-641)");
	for (int r = 0, c = 0; r < nrx; r++)
		for (int i = 0; i < nch_per_rx[r]; i++, c++)
			if (int rc = check_channel_span(sample_rate, nrx, c, freqs[c], r, centerfreqs[r])) return rc;
	return 0;
}

extern "C" int hfdl_gpu_frontend_create(hfdl_gpu_frontend **out, int device, int32_t sample_rate, int32_t centerfreq,
		const int32_t *freqs, int32_t nch)
{
	if (!out || !freqs || nch <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	return hfdl_gpu_frontend_create_multi(out, device, sample_rate, 1, &centerfreq, freqs, &nch);
}

// The streams: plain non-blocking ones (stream priority and CU-masking of stream A alone change nothing beyond run-to-run noise,
// profiles/r01_experiments.md).  The laboratory build can bind the demodulator's stream and the channelizer's to disjoint sets of CUs
// where the fold bounds the block (planner.h plan_cu_partition); the forward FFTs then get a stream of their own.  Measured slower than
// the plain streams on cfg3 (profiles/r09_experiments.md section 2): not the product's path.
// Order of creation: the runtime hands its hardware queues (four by default) to streams in turn, and two streams on one queue run in
// turn -- A, B, D (and the laboratory's F) come first, the input stream C after them: the fourth stream of the product, as it has been.
static int create_streams(hfdl_gpu_frontend *fe, const LabConfig &lab)
{
	CuPartition part = plan_cu_partition((int)fe->freqs.size(), Demod::workgroup_lds(), fe->fold_bound);
	if (!lab.cu_partition || lab.cu_split) part.on = false;
	if (part.on) {
		const hipError_t ea = fe->stream.create_on_cus(part.mask_fold), eb = fe->stream_b.create_on_cus(part.mask_demod);
		if (ea != hipSuccess || eb != hipSuccess) {
			// the runtime refuses CU masks: plain streams, and the text says so (not an error)
			fe->stream.reset(); fe->stream_b.reset();
			(void)hipGetLastError();
			(void)fail(0, "CU-masked streams refused (%s): the demodulators share the fold's CUs", hipGetErrorString(ea != hipSuccess ? ea : eb));
			part.on = false;
		}
	}
	fe->cu_partitioned = part.on;
	if (part.on) {
		// A and B are made
	} else if (lab.cu_split) {
		// Laboratory A/B: does a demodulator launch still execute twice the cycles while a fold runs, when no fold wave shares its SIMD?
		// CU i belongs to the demodulator iff ((i >> 3) + i) % k == 0: an equal share of every XCD whether the mask counts XCD-major or
		// XCD-interleaved.
		uint32_t mask_a[8] = {}, mask_b[8] = {};
		for (int i = 0; i < 256; i++)
			((((i >> 3) + i) % lab.cu_split) == 0 ? mask_b : mask_a)[i >> 5] |= 1u << (i & 31);
		CREATE_TRY(fe->stream.create_on_cus(mask_a));
		CREATE_TRY(fe->stream_b.create_on_cus(mask_b));
	} else {
		CREATE_TRY(fe->stream.create());
		CREATE_TRY(fe->stream_b.create());
	}
	// The burst decoder of launch k only hands PDUs to the host; the demodulator of launch k+1 does not need it, and a long frame
	// ending in a block puts 0.3 - 1.2 ms of Viterbi in front of it: the decoder has its own stream (cfg2: +25 % in round 2; at 256
	// channels the round-4 timeline shows a 1.18 ms decoder launch serially ahead of a half's first demodulator).
	if (lab.decode_stream) CREATE_TRY(fe->stream_d.create());
	else fe->stream_d.alias(fe->stream_b);
	fe->demod.order.own_decode = fe->own_decode_stream();
	// Forward FFTs of the half being filled beside the fold of the half before (two sets of spectra / phasor tables / state snapshots).
	// The product decides per push by where the block lies (planner.h FftRule): a device-resident block's FFT runs on the input stream C,
	// which carries no copy for such a block; an uploaded block's stays in front of the fold on stream A (a stream of their own for ALL
	// forward FFTs gained 2 - 4 % on cfg3 and 8 % on cfg4 from device-resident input and lost 16 % with host input,
	// profiles/r09_experiments.md section 2).  The laboratory's switch puts every FFT on stream A or on a stream F of their own, and the
	// CU partition, where stream A alone would be serial, goes with the latter.
	if (lab.fft_stream < 0 ? part.on : lab.fft_stream != 0) {
		if (part.on) CREATE_TRY(fe->stream_f.create_on_cus(part.mask_fold));
		else CREATE_TRY(fe->stream_f.create());
		fe->fft_rule = FFT_RULE_OWN;
	} else if (lab.fft_stream == 0) fe->fft_rule = FFT_RULE_SERIAL;
	CREATE_TRY(fe->stream_c.create());
	return 0;
}

static int create_frontend(hfdl_gpu_frontend *fe, int32_t nrx, const int32_t *nch_per_rx)
{
	const int nch = (int)fe->freqs.size();
	const LabConfig lab = read_lab_config();
	if (!plan_block(fe->plan, fe->tbw, fe->decimation, 0.f)) return fail(HFDL_GPU_EINVAL, "fastddc planning failed");
	const Plan &pl = fe->plan;
	Geometry &g = fe->geo;
	g.n = pl.n; g.m = pl.m; g.pre = pl.pre; g.post = pl.post; g.scrap = pl.scrap; g.post_input_size = pl.post_input_size;
	g.overlap = pl.overlap; g.input_size = pl.input_size; g.outs = (pl.post_input_size + pl.post - 1) / pl.post + 1;
	g.nch = nch;
	// Filter taps row-major over channels: alias row r of every channel sits in one nch*M run, so the workgroups of all
	// channels, which walk the rows together, stream through a few moving windows of HBM instead of nch windows 8N bytes
	// apart (fold kernel 2.58 -> 2.48 ms on cfg3 and a tighter run-to-run spread, profiles/r01_experiments.md)
	g.tap_layout = (pl.m % 16) == 0 && (pl.pre % 8) == 0 ? TAPL_OCTET : TAPL_PLAIN;       // the matrix-pipe fold walks the alias rows four at a time, two such quads in flight
	// each receiver's channels padded to whole groups of the layout on their own (one receiver: nch rounded up, as always)
	g.nch_pad = plan_receiver_slots(nch_per_rx, nrx, tap_layout_group(g.tap_layout), fe->rx_span);
	for (const RxSpan &r : fe->rx_span) fe->rx_host.push_back(make_int4(r.slot0, r.slots, r.chan0, r.nch));
	g.nrx = nrx;
	g.spec_rx_stride = pl.n;
	g.rx_host = fe->rx_host.data();
	g.tap_chan_stride = pl.m; g.tap_row_stride = (int64_t)g.nch_pad * pl.m;
	g.fold_tile = lab.fold_tile;
	fe->tap_layout.kind = g.tap_layout;
	fe->tap_layout.row_log = ilog2(pl.m); fe->tap_layout.row_stride = g.tap_row_stride;
	// HFDL_GPU_FOLD_PRUNE=tol (0 < tol <= 1e-3; unset: every alias row is folded, the reference's sum term for term): fold only the
	// rows around each channel's pass band (build_fold_windows) -- one slice, the windows are the parallelism
	// (the pruned fold's windows are per octet of ONE receiver's taps: off with several receivers)
	// (and per octet of taps whose spectrum is stored: a real front end ignores it, and HFDL_GPU_FOLD_SPECTRUM=0 below, as well)
	fe->prune_tol = g.tap_layout == TAPL_OCTET && nrx == 1 && !fe->real_rate ? env_double("HFDL_GPU_FOLD_PRUNE", 1e-12, 1e-3, 0.0) : 0.0;
	// fold_bound: with many channels the fold bounds the block; the demodulator launches of a half are then held back until the next
	// half's forward FFTs are queued (launch_demod) instead of starting at once.
	fe->fold_bound = lab.fold_bound < 0 ? nch >= 128 : lab.fold_bound != 0;
	const float resamp_rate = (float)(1800 * 3) / ((float)fe->sample_rate / (float)fe->decimation);
	BatchOverrides ov;
	ov.demod_batch = (int)env_long("HFDL_GPU_DEMOD_BATCH", 1, hfdl_gpu_frontend::MAX_HALF, 0);
	ov.fold_batch = (int)env_long("HFDL_GPU_FOLD_BATCH", 1, hfdl_gpu_frontend::MAX_HALF, 0);
	ov.pruned = fe->prune_tol > 0;
	ov.fold_slices = lab.fold_slices;
	ov.no_ramp = !lab.fold_ramp;
	const BatchPlan bp = plan_batches(nch, nrx, pl.n, pl.input_size, fe->sample_rate, pl.pre, fe->fold_bound,
			[&](int want) { return Demod::fit_batch(g.outs, resamp_rate, want); }, ov);
	g.slices = bp.slices;
	g.rows_per_slice = pl.pre / g.slices;
	if (pl.m > 8192 || pl.m < 16) return fail(HFDL_GPU_ERANGE, "inverse FFT size %d unsupported", pl.m);

	if (int rc = create_streams(fe, lab)) return rc;
	for (int i = 0; i < 2; i++) {
		CREATE_TRY(fe->spec[i].own.create(EV_NO_TIMING));
		CREATE_TRY(fe->chan[i].own.create(EV_NO_TIMING));
	}
	CREATE_TRY(fe->fft_done.own.create(EV_NO_TIMING));
	CREATE_TRY(fe->ev_switch.create(EV_NO_TIMING));
	if (int rc = fe->fft.build(pl.n)) return rc;
	{
		// HFDL_GPU_FOLD_SPECTRUM=0: the fold in the mixed domain (fold_domain.h) wherever the geometry allows it -- the
		// forward FFT stops after pass 2.  Unset or 1, the fold reads spectra: all three passes, the taps' full transform.  Opt-in, because
		// under out-of-band signals 60 dB above the channel the mixed-domain sums cancel in the accumulator and the channelizer output
		// lands 2.8 x further from the float64 model (2.4 Msps x 130 channels: 1.57e-4 against 5.6e-5 relative RMS at worst) -- past the
		// gate of tests/test_gpu_channelizer_f64.py at one (block, channel) of 1392.
		const FftPlan &fp = fe->fft.p;
		if (!fe->real_rate && g.tap_layout == TAPL_OCTET && mixed_fold_fits(fp.l1, fp.l2, fp.l3, ilog2(pl.m), fe->prune_tol > 0) && env_long("HFDL_GPU_FOLD_SPECTRUM", 0, 1, 1) == 0) {
			g.mix_l1 = fp.l1; g.mix_q = ilog2(pl.m) - fp.l1;
			g.spec_row_stride = 16; g.spec_group_stride = 16 * (int64_t)pl.pre;
		}
	}
	const size_t n = (size_t)pl.n;
	const size_t K = (size_t)nrx;
	for (int i = 0; i < 2; i++) {      // overlap history, ping-pong: block k reads [k&1] and leaves the next one in [(k+1)&1]; one per receiver
		CREATE_TRY(fe->alloc(fe->d_hist[i], (size_t)pl.overlap * K));
		CREATE_TRY(hipMemsetAsync(fe->d_hist[i], 0, sizeof(float2) * (size_t)pl.overlap * K, fe->stream));   // calloc'ed history, src/fft.c:79
	}
	CREATE_TRY(fe->alloc(fe->d_work, n * K));
	if (fe->real_rate) CREATE_TRY(fe->alloc(fe->d_real, n * K));
	CREATE_TRY(fe->alloc(fe->d_rx, K));
	CREATE_TRY(hipMemcpy(fe->d_rx, fe->rx_host.data(), sizeof(int4) * K, hipMemcpyHostToDevice));
	g.rx_tab = fe->d_rx;
	if (g.tap_layout == TAPL_OCTET) {
		static_assert(sizeof(FoldGroup) == sizeof(int4), "a FoldGroup entry is what the fold kernels load as an int4");
		const std::vector<FoldGroup> t = fold_group_tables(fe->rx_span, g.nch_pad / 8, FOLD_GROUP_MAX);
		CREATE_TRY(fe->alloc(fe->d_grp, t.size()));
		CREATE_TRY(hipMemcpy(fe->d_grp, t.data(), sizeof(int4) * t.size(), hipMemcpyHostToDevice));
		g.grp_tab = fe->d_grp;
	}
	CREATE_TRY(fe->alloc(fe->d_taps, n * (size_t)g.nch_pad));
	CREATE_TRY(fe->alloc(fe->d_nco, (size_t)nch));
	CREATE_TRY(hipMemsetAsync(fe->d_nco, 0, sizeof(NcoState) * (size_t)nch, fe->stream));
	CREATE_TRY(fe->alloc(fe->d_ph_cont, (size_t)nch));
	CREATE_TRY(hipMemsetAsync(fe->d_ph_cont, 0, sizeof(float2) * (size_t)nch, fe->stream));      // (written before it is read; zero so that a retune can put it back)
	CREATE_TRY(fe->alloc(fe->d_cc, (size_t)nch));
	fe->mem.emplace_back();
	if (int rc = upload_twiddles(pl.m, fe->mem.back())) return rc;
	fe->d_tw_m = fe->mem.back().as<float2>();
	if (prepare_ifft_nco(pl.m) != hipSuccess)
		return fail(HFDL_GPU_EHIP, "inverse FFT of %d points: LDS attribute refused: %s", pl.m, hipGetErrorString(hipGetLastError()));
	if (int rc = build_taps(fe)) return rc;
	if (fe->prune_tol > 0 && g.tap_layout == TAPL_OCTET)
		if (int rc = build_fold_windows(fe)) return rc;
	CREATE_TRY(hipMemcpy(fe->d_cc, fe->cc.data(), sizeof(ChanConst) * (size_t)nch, hipMemcpyHostToDevice));
	fe->fold_nb = bp.fold_nb;
	if (int rc = fe->demod.init(nch, g.outs, resamp_rate, fe->freqs.data(), fe->stream, bp.batch_want)) return rc;
	fe->batch = fe->demod.batch;
	fe->half_blocks = bp.half_blocks;
	fe->half_first = fe->half_target = bp.half_first;
	fe->n_stage = bp.n_stage;
	for (int i = 0; i < fe->n_stage; i++) {
		CREATE_TRY(fe->ev_stage_ready[i].create(EV_NO_TIMING));
		CREATE_TRY(fe->ev_stage_free[i].create(EV_NO_TIMING));
	}
	const size_t hb = (size_t)fe->half_blocks;
	CREATE_TRY(fe->alloc(fe->d_spec, fe->spec_stride() * 2 * hb));
	CREATE_TRY(fe->alloc(fe->d_partial, fe->partial_stride() * hb));
	CREATE_TRY(fe->alloc(fe->d_ph, fe->ph_stride() * 2 * hb));
	CREATE_TRY(fe->alloc(fe->d_nco_snap, (size_t)nch * 2 * hb));
	CREATE_TRY(fe->alloc(fe->d_chan_all, 2 * hb * (size_t)nch * g.outs));
	CREATE_TRY(fe->alloc(fe->d_cnt_all, 2 * hb * (size_t)nch));
	CREATE_TRY(hipMemsetAsync(fe->d_cnt_all, 0, sizeof(int) * 2 * hb * (size_t)nch, fe->stream));
	CREATE_TRY(hipStreamSynchronize(fe->stream));
	return 0;
}

// real_rate / bases: a real front end (hfdl_gpu_frontend_create_real), whose sample_rate and centerfreqs are the equivalent stream's
static int create_any(hfdl_gpu_frontend **out, int device, int32_t sample_rate, int32_t nrx, const int32_t *centerfreqs, const int32_t *freqs,
		const int32_t *nch_per_rx, int32_t real_rate, const int32_t *bases)
{
	int rc = check_create_args(out, sample_rate, nrx, centerfreqs, freqs, nch_per_rx);
	if (rc || (rc = select_device(device))) return rc;
	int32_t nch = 0;
	for (int r = 0; r < nrx; r++) nch += nch_per_rx[r];
	auto fe = std::make_unique<hfdl_gpu_frontend>();
	fe->device = device;
	fe->sample_rate = sample_rate;
	fe->decimation = fft_decimation_rate(sample_rate, 1800 * 3);
	fe->tbw = relative_transition_bw(sample_rate, 250);
	fe->freqs.assign(freqs, freqs + nch);
	fe->nrx = nrx;
	fe->rx_center.assign(centerfreqs, centerfreqs + nrx);
	fe->real_rate = real_rate;
	if (real_rate) fe->rx_base.assign(bases, bases + nrx);
	for (int r = 0; r < nrx; r++) fe->rx_of.insert(fe->rx_of.end(), (size_t)nch_per_rx[r], r);
	if ((rc = create_frontend(fe.get(), nrx, nch_per_rx))) return rc;       // (the destructor releases what a failed create got as far as)
	*out = fe.release();
	return 0;
}

extern "C" int hfdl_gpu_frontend_create_multi(hfdl_gpu_frontend **out, int device, int32_t sample_rate, int32_t nrx,
		const int32_t *centerfreqs, const int32_t *freqs, const int32_t *nch_per_rx)
{
	return create_any(out, device, sample_rate, nrx, centerfreqs, freqs, nch_per_rx, 0, nullptr);
}

// Real-sampled receivers: planned as the equivalent complex streams (real_input.h), checked like them
extern "C" int hfdl_gpu_frontend_create_real(hfdl_gpu_frontend **out, int device, int32_t sample_rate_real, int32_t nrx,
		const int32_t *base_freqs, const int32_t *freqs, const int32_t *nch_per_rx)
{
	if (out) *out = nullptr;
	if (!base_freqs || !freqs || !nch_per_rx || nrx < 1 || nrx > HFDL_GPU_RECEIVERS_MAX) return fail(HFDL_GPU_EINVAL, "bad arguments: null pointer, or %d receivers", nrx);
	if (sample_rate_real < REAL_RATE_MIN || (sample_rate_real & 1)) return fail(HFDL_GPU_EINVAL, "real sample rate %d: even and >= %d", sample_rate_real, REAL_RATE_MIN);
	int32_t centres[HFDL_GPU_RECEIVERS_MAX];
	for (int r = 0; r < nrx; r++) {
		if (!real_base_valid(sample_rate_real, base_freqs[r])) return fail(HFDL_GPU_EINVAL, "receiver %d: base %d Hz out of range", r, base_freqs[r]);
		centres[r] = real_equiv_centre(sample_rate_real, base_freqs[r]);
	}
	return create_any(out, device, real_equiv_rate(sample_rate_real), nrx, centres, freqs, nch_per_rx, sample_rate_real, base_freqs);
}

// The order, explicitly: every owned stream (the demodulator's collection stream too) and the monitor's event are synchronised; then
// the members go in reverse order of declaration -- events, memory, streams (frontend.h)
hfdl_gpu_frontend::~hfdl_gpu_frontend()
{
	(void)hipSetDevice(device);
	for (const hfdl::Stream *s : { &stream, &stream_b, &stream_d, &stream_c, &stream_f, &demod.st_collect }) (void)s->sync();
	if (mon) (void)hipEventSynchronize(mon->newest());
}

extern "C" void hfdl_gpu_frontend_destroy(hfdl_gpu_frontend *fe) { delete fe; }
