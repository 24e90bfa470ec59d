// frontend_options.cpp -- the opt-in stages of a front end, each in one place: its switch, the hook the pipeline (hfdl_gpu.cpp) calls in
// one line, and its reader.  The input chain (impulse-noise blanker, I/Q corrector), the spectrum monitor and its history of interval
// rows, the carrier canceller, the channel baseband export.  What each stage is and owns: frontend.h.
#include <algorithm>
#include <cstring>
#include "frontend.h"

using namespace hfdl;

// an enable's allocations that do not fit are HFDL_GPU_ENOMEM, as at create
#define ALLOC_FAIL(e, what) fail_hip(e, true, what " buffers", __FILE__, __LINE__)

static int check_receiver(const hfdl_gpu_frontend *fe, int32_t rx)
{
	if (rx < 0 || rx >= fe->nrx) return fail(HFDL_GPU_EINVAL, "receiver %d out of range (%d receivers)", rx, fe->nrx);
	return 0;
}

// channels[0 .. nsel): each inside 0 .. nch - 1 and listed once -- marked in seen[nch] -- or the index of the first that is not; -1: all are
static int check_channel_list(int nch, const int32_t *channels, int32_t nsel, std::vector<bool> &seen)
{
	for (int i = 0; i < nsel; i++) {
		if (channels[i] < 0 || channels[i] >= nch || seen[(size_t)channels[i]]) return i;
		seen[(size_t)channels[i]] = true;
	}
	return -1;
}

// Read one record behind the newest launch of a stage: the collection stream waits for the event that rode on that launch's dispatch
// and copies beside the kernels in flight -- no packet on the stage's own stream, no wait for anything behind the launch.
static int read_record(hfdl_gpu_frontend *fe, hipEvent_t newest, const void *src, void *host, size_t bytes)
{
	hipStream_t st = fe->demod.st_collect;
	hipError_t e = hipSetDevice(fe->device);
	if (e == hipSuccess) e = hipStreamWaitEvent(st, newest, 0);
	if (e == hipSuccess) e = hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	HIP_TRY(e);
	return 0;
}

// ---------------------------------------------------------------- the input chain: impulse-noise blanker, I/Q corrector

// the chain's scratch, [nrx][input_size] cf32: allocated by the first enable of either stage, kept until the front end goes
static hipError_t chain_scratch(hfdl_gpu_frontend *fe)
{
	return fe->chain_scratch.p ? hipSuccess : fe->chain_scratch.alloc(sizeof(float2) * (size_t)fe->nrx * (size_t)fe->geo.input_size);
}

extern "C" int hfdl_gpu_frontend_blanker_enable(hfdl_gpu_frontend *fe, float threshold_db)
{
	if (!(threshold_db == 0.f || (threshold_db >= BLANK_DB_MIN && threshold_db <= BLANK_DB_MAX))) return fail(HFDL_GPU_EINVAL, "blanker threshold %g dB", (double)threshold_db);
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	if (!fe->blank) {
		if (threshold_db == 0.f) return 0;
		HIP_TRY(hipSetDevice(fe->device));
		const size_t K = (size_t)fe->nrx;
		auto b = std::make_unique<Blanker>();
		hipError_t e = chain_scratch(fe);
		if (e == hipSuccess) e = b->partial.alloc(sizeof(float) * K * (size_t)blank_chunks(fe->geo.input_size));
		if (e == hipSuccess) e = b->rec.zeroed(sizeof(BlankRecord) * K);
		if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // the clearing runs on the null stream, which the front end's streams do not follow
		if (e == hipSuccess) e = b->host.alloc(1);
		if (e == hipSuccess) e = b->ev.create(EV_NO_TIMING);
		if (e != hipSuccess) return ALLOC_FAIL(e, "blanker");
		fe->blank = std::move(b);
	}
	fe->blank->k2 = threshold_db == 0.f ? 0.f : blank_k2(threshold_db);
	return 0;
}

extern "C" int hfdl_gpu_frontend_blanker_stats(hfdl_gpu_frontend *fe, int32_t rx, hfdl_gpu_blanker_stats *out)
{
	if (!fe || !out) return fail(HFDL_GPU_EINVAL, "null argument");
	Blanker *b = fe->blank.get();
	if (!b) return fail(HFDL_GPU_EINVAL, "the blanker was never enabled");
	if (int rc = check_receiver(fe, rx)) return rc;
	memset(out, 0, sizeof(*out));
	if (b->blocks == 0) return 0;
	if (int rc = read_record(fe, b->ev, b->rec.as<BlankRecord>() + rx, b->host.p, sizeof(BlankRecord))) return rc;
	out->blocks = b->blocks; out->samples_blanked = b->host.p->blanked;
	out->last_power = b->host.p->power; out->last_threshold = b->host.p->threshold;
	return 0;
}

// rx = -1: every receiver
static bool iqbal_targets(const hfdl_gpu_frontend *fe, int32_t rx, int &r0, int &r1)
{
	if (rx < -1 || rx >= fe->nrx || fe->real_rate) return false;       // (real samples: there is no I/Q to balance)
	r0 = rx < 0 ? 0 : rx;
	r1 = rx < 0 ? fe->nrx : rx + 1;
	return true;
}

extern "C" int hfdl_gpu_frontend_iqbal_enable(hfdl_gpu_frontend *fe, int32_t rx, float alpha)
{
	if (!iqbal_alpha_valid(alpha)) return fail(HFDL_GPU_EINVAL, "I/Q corrector alpha %g", (double)alpha);
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	int r0, r1;
	if (!iqbal_targets(fe, rx, r0, r1)) return fail(HFDL_GPU_EINVAL, "receiver %d out of range (%d receivers), or a front end for real input", rx, fe->nrx);
	if (!fe->iqbal) {
		if (alpha == 0.f) return 0;
		HIP_TRY(hipSetDevice(fe->device));
		const size_t K = (size_t)fe->nrx;
		auto q = std::make_unique<Iqbal>();
		q->alpha.assign(K, 0.f);
		hipError_t e = chain_scratch(fe);
		if (e == hipSuccess) e = q->partial.alloc(sizeof(float) * 2 * K * 5 * (size_t)blank_chunks(fe->geo.input_size));
		if (e == hipSuccess) e = q->state.zeroed(sizeof(IqbalState) * 2 * K);
		if (e == hipSuccess) e = q->seed.zeroed(sizeof(IqbalSeed) * K);
		if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // the clearing runs on the null stream, which the front end's streams do not follow
		if (e == hipSuccess) e = q->host.alloc(1);
		if (e == hipSuccess) e = q->ev.create(EV_NO_TIMING);
		if (e != hipSuccess) return ALLOC_FAIL(e, "I/Q corrector");
		fe->iqbal = std::move(q);
	}
	Iqbal *q = fe->iqbal.get();
	for (int r = r0; r < r1; r++) {
		if (alpha > 0.f && q->alpha[(size_t)r] == 0.f) {
			// on again: the estimate starts afresh with the next block, and a seed from before the switch is forgotten (the one wait of
			// this call, and only where a seed was ever given: for the launch that may still be reading it)
			q->restart |= (uint64_t)1 << r;
			if (q->seeds) {
				HIP_TRY(hipSetDevice(fe->device));
				if (q->step) HIP_TRY(hipEventSynchronize(q->ev));
				const IqbalSeed none = {};
				HIP_TRY(hipMemcpy(q->seed.as<IqbalSeed>() + r, &none, sizeof(none), hipMemcpyHostToDevice));
			}
		}
		q->alpha[(size_t)r] = alpha;
	}
	q->any_on = false;
	for (float a : q->alpha) q->any_on = q->any_on || a > 0.f;
	return 0;
}

extern "C" int hfdl_gpu_frontend_iqbal_seed(hfdl_gpu_frontend *fe, int32_t rx, float kappa_re, float kappa_im, float dc_re, float dc_im, int hold)
{
	if (!iqbal_seed_valid(kappa_re, kappa_im, dc_re, dc_im) || (hold != 0 && hold != 1)) return fail(HFDL_GPU_EINVAL, "I/Q corrector seed: |kappa| above 0.25, a value that is not finite, or hold %d", hold);
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	Iqbal *q = fe->iqbal.get();
	int r0, r1;
	// (the receiver and the kind of front end first: a real front end says so, whatever else is wrong -- its corrector can never have been enabled)
	if (!iqbal_targets(fe, rx, r0, r1)) return fail(HFDL_GPU_EINVAL, "receiver %d out of range (%d receivers), or a front end for real input", rx, fe->nrx);
	if (!q) return fail(HFDL_GPU_EINVAL, "the I/Q corrector was never enabled");
	for (int r = r0; r < r1; r++) if (q->alpha[(size_t)r] == 0.f) return fail(HFDL_GPU_EINVAL, "the I/Q corrector of receiver %d is off", r);
	HIP_TRY(hipSetDevice(fe->device));
	if (q->step) HIP_TRY(hipEventSynchronize(q->ev));       // the newest launch may still be reading the slot
	IqbalSeed sd = {};
	sd.k_re = kappa_re; sd.k_im = kappa_im; sd.m_re = dc_re; sd.m_im = dc_im; sd.gen = ++q->seeds; sd.hold = (uint32_t)hold;
	for (int r = r0; r < r1; r++) HIP_TRY(hipMemcpy(q->seed.as<IqbalSeed>() + r, &sd, sizeof(sd), hipMemcpyHostToDevice));
	return 0;
}

extern "C" int hfdl_gpu_frontend_iqbal_stats(hfdl_gpu_frontend *fe, int32_t rx, hfdl_gpu_iqbal_stats *out)
{
	if (!fe || !out) return fail(HFDL_GPU_EINVAL, "null argument");
	Iqbal *q = fe->iqbal.get();
	if (!q) return fail(HFDL_GPU_EINVAL, "the I/Q corrector was never enabled");
	if (int rc = check_receiver(fe, rx)) return rc;
	memset(out, 0, sizeof(*out));
	if (q->step == 0) return 0;
	if (int rc = read_record(fe, q->ev, q->state.as<IqbalState>() + ((q->step - 1) & 1) * (size_t)fe->nrx + (size_t)rx, q->host.p, sizeof(IqbalState))) return rc;
	iqbal_stats_of(*q->host.p, out);
	return 0;
}

// The input chain, in front of the forward FFT's first pass on that block's FFT stream.  ONE rule:
//   - the first stage that is on for this block reads the block where it lies, in its own sample format, and writes the chain's scratch;
//   - every later stage works on the scratch in place, as cf32;
//   - if any stage ran, the first pass reads the scratch as cf32 (in.fresh and fmt say so on return);
//   - the order is fixed: blanker (two launches), then corrector (one).
// One scratch serves every block: forward FFTs run one after the other whichever stream they are on (they share d_work and the overlap
// history: planner.h FftOrder), so the chain of block i + 1 is behind the first pass that read block i's.  The timed pair and every event
// other streams wait for stay on the passes; the staging buffer's input_read event still rides on pass 1, which runs behind the chain's
// last read of the input; each stage's `ev` rides on its own last launch.
void condition_input(hfdl_gpu_frontend *fe, FftInputs &in, int &fmt, hipStream_t st)
{
	const int n = fe->geo.input_size;
	float2 *scratch = fe->chain_scratch.as<float2>();
	bool ran = false;
	if (Blanker *b = fe->blank.get(); b && b->k2 > 0.f) {
		BlankJob j;
		for (int r = 0; r < fe->nrx; r++) j.fresh[r] = in.fresh[r];
		j.out = scratch; j.out_stride = n; j.partial = b->partial.as<float>(); j.rec = b->rec.as<BlankRecord>();
		j.n = n; j.nrx = fe->nrx; j.fmt = fmt; j.k2 = b->k2;
		launch_blanker(j, st, b->ev);
		b->blocks++;
		ran = true;
	}
	if (Iqbal *q = fe->iqbal.get(); q && q->any_on) {
		IqbalJob j;
		for (int r = 0; r < fe->nrx; r++) { j.fresh[r] = ran ? scratch + (size_t)r * (size_t)n : in.fresh[r]; j.alpha[r] = q->alpha[(size_t)r]; }
		j.out = scratch; j.out_stride = n;
		j.partial = q->partial.as<float>(); j.state = q->state.as<IqbalState>(); j.seed = q->seed.as<IqbalSeed>();
		j.restart = q->restart; j.n = n; j.nrx = fe->nrx; j.fmt = ran ? SFMT_CF32 : fmt; j.slot = (int)(q->step & 1);
		launch_iqbal(j, st, q->ev);
		q->restart = 0;
		q->step++;
		ran = true;
	}
	if (!ran) return;
	for (int r = 0; r < fe->nrx; r++) in.fresh[r] = scratch + (size_t)r * (size_t)n;
	fmt = SFMT_CF32;
}

// ---------------------------------------------------------------- spectrum monitor

static_assert(HFDL_GPU_SPECTRUM_HANN == SPECMON_HANN && HFDL_GPU_SPECTRUM_MAXHOLD == SPECMON_MAXHOLD, "include/hfdl_gpu.h and spectrum.h name the same flags");
static_assert(HFDL_GPU_RECEIVERS_MAX <= 64, "SpecmonJob::fresh is one bit per receiver");

extern "C" int hfdl_gpu_frontend_spectrum_enable(hfdl_gpu_frontend *fe, int32_t bins, uint32_t flags)
{
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	if (flags & ~(HFDL_GPU_SPECTRUM_HANN | HFDL_GPU_SPECTRUM_MAXHOLD)) return fail(HFDL_GPU_EINVAL, "unknown spectrum flags 0x%x", flags);
	if (bins != 0 && (bins < 16 || (bins & (bins - 1)) != 0)) return fail(HFDL_GPU_EINVAL, "spectrum bins %d: a power of two >= 16 (or 0 = off)", bins);
	if (bins > fe->geo.n / 16) return fail(HFDL_GPU_ERANGE, "spectrum bins %d: at most fft_size / 16 = %d", bins, fe->geo.n / 16);
	HIP_TRY(hipSetDevice(fe->device));
	// the old monitor's buffers go once nothing queued uses them any more: wait for the monitor launches queued so far, nothing else
	if (fe->mon) (void)hipEventSynchronize(fe->mon->newest());
	fe->mon.reset();                       // (and the history of interval rows with it)
	if (bins == 0) return 0;
	const size_t nb = (size_t)bins, K = (size_t)fe->nrx;
	auto mon = std::make_unique<SpectrumMonitor>();
	hipError_t e = mon->acc.alloc(sizeof(float2) * nb * K);
	if (e == hipSuccess && (flags & HFDL_GPU_SPECTRUM_MAXHOLD)) e = mon->peak.alloc(sizeof(float) * nb * K);
	if (e == hipSuccess) e = mon->host.alloc(3 * nb);
	if (e == hipSuccess && fe->geo.mix_l1) e = mon->scratch.alloc(sizeof(float2) * K * (size_t)fe->geo.n);
	if (e == hipSuccess) e = mon->ev.create(EV_NO_TIMING);
	if (e != hipSuccess) return ALLOC_FAIL(e, "spectrum monitor");
	mon->bins = bins;
	mon->flags = flags;
	mon->fresh = ~(uint64_t)0;             // every receiver starts over with the next block: nothing to clear on the device
	mon->blocks.assign(K, 0);
	mon->first.assign(K, 0);
	fe->mon = std::move(mon);
	return 0;
}

// behind the forward FFT's last launch on `st`, which left the step's spectra in `spectrum` and keeps the timed pair and the events other streams wait for
void launch_monitor(hfdl_gpu_frontend *fe, const float2 *spectrum, hipStream_t st)
{
	SpectrumMonitor *mon = fe->mon.get();
	if (!mon) return;
	const Geometry &g = fe->geo;
	SpecmonJob m;
	m.spec = spectrum; m.rx_stride = g.n; m.n = g.n; m.bins = mon->bins; m.nrx = fe->nrx; m.flags = mon->flags;
	m.scale = (float)(1.0 / ((double)g.n * (double)g.n * ((mon->flags & SPECMON_HANN) ? 0.375 : 1.0)));
	m.fresh = mon->fresh; m.acc = mon->acc.as<float2>(); m.peak = mon->peak.as<float>();
	SpectrumHistory *h = mon->hist.get();
	hipEvent_t done = mon->ev;
	if (h) {
		// The open row's slot is the launch's second target and its event the one this dispatch carries: row i + rows overwrites
		// the slot of row i in stream order.  One thread drives a front end (include/hfdl_gpu.h), and a collection returns only
		// when its copies are done, so no copy of a slot is in flight while a push re-targets it.
		const size_t slot = (size_t)(h->open % (uint64_t)h->rows), set = (size_t)fe->nrx * (size_t)mon->bins;
		m.row_acc = h->acc.as<float2>() + slot * set;
		if (mon->flags & SPECMON_MAXHOLD) m.row_peak = h->peak.as<float>() + slot * set;
		m.row_fresh = h->open_blocks == 0;
		done = h->ev[slot];
	}
	launch_spectrum_monitor(m, st, done);
	mon->last = done;
	for (int r = 0; r < fe->nrx; r++) {
		if ((mon->fresh >> r) & 1) { mon->blocks[(size_t)r] = 0; mon->first[(size_t)r] = fe->blocks; }
		mon->blocks[(size_t)r]++;
	}
	if (h) {
		if (h->open_blocks++ == 0) h->open_first = fe->blocks;
		if (h->interval > 0 && h->open_blocks == (uint32_t)h->interval) h->close();
	}
	mon->fresh = 0;
}

// what the device's Kahan pair becomes on the host, for a read and for a row alike: the compensation holds what the sum has gained too much
static void mean_of(const float *h, size_t nb, uint64_t T, float *mean)
{
	for (size_t b = 0; b < nb; b++) mean[b] = (float)(((double)h[2 * b] - (double)h[2 * b + 1]) / (double)T);
}

extern "C" int hfdl_gpu_frontend_spectrum_read(hfdl_gpu_frontend *fe, int32_t rx, float *mean, float *peak, int32_t cap,
		uint64_t *blocks, uint64_t *first_block, int reset)
{
	if (!fe || !mean || !blocks || !first_block) return fail(HFDL_GPU_EINVAL, "null argument");
	SpectrumMonitor *mon = fe->mon.get();
	if (!mon) return fail(HFDL_GPU_EINVAL, "the spectrum monitor is off: hfdl_gpu_frontend_spectrum_enable() first");
	if (int rc = check_receiver(fe, rx)) return rc;
	if (peak && !(mon->flags & HFDL_GPU_SPECTRUM_MAXHOLD)) return fail(HFDL_GPU_EINVAL, "peak asked for, but the monitor was enabled without HFDL_GPU_SPECTRUM_MAXHOLD");
	if (cap < mon->bins) return fail(HFDL_GPU_ERANGE, "%d bands, buffer holds %d", mon->bins, cap);
	const bool pending = (mon->fresh >> rx) & 1;      // reset (or just enabled) and no block since
	const uint64_t T = pending ? 0 : mon->blocks[(size_t)rx];
	*blocks = T;
	*first_block = pending ? fe->blocks : mon->first[(size_t)rx];
	if (T == 0) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	// as read_record, with a second copy where a peak is asked for
	const size_t nb = (size_t)mon->bins;
	float *h = mon->host.p;
	hipStream_t st = fe->demod.st_collect;
	HIP_TRY(hipStreamWaitEvent(st, mon->newest(), 0));
	HIP_TRY(hipMemcpyAsync(h, mon->acc.as<float2>() + (size_t)rx * nb, sizeof(float2) * nb, hipMemcpyDeviceToHost, st));
	if (peak) HIP_TRY(hipMemcpyAsync(h + 2 * nb, mon->peak.as<float>() + (size_t)rx * nb, sizeof(float) * nb, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	mean_of(h, nb, T, mean);
	if (peak) memcpy(peak, h + 2 * nb, sizeof(float) * nb);
	if (reset) mon->fresh |= (uint64_t)1 << rx;
	return 0;
}

// ---------------------------------------------------------------- spectrum monitor: history of interval rows

extern "C" int hfdl_gpu_frontend_spectrum_history(hfdl_gpu_frontend *fe, int32_t rows, int32_t interval_blocks)
{
	if (rows != 0 && (rows < 2 || rows > HFDL_GPU_SPECTRUM_ROWS_MAX)) return fail(HFDL_GPU_EINVAL, "spectrum history rows %d: 2 .. %d (or 0 = off)", rows, HFDL_GPU_SPECTRUM_ROWS_MAX);
	if (interval_blocks < 0) return fail(HFDL_GPU_EINVAL, "spectrum history interval of %d blocks", interval_blocks);
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	SpectrumMonitor *mon = fe->mon.get();
	if (!mon) return fail(HFDL_GPU_EINVAL, "the spectrum monitor is off: hfdl_gpu_frontend_spectrum_enable() first");
	const size_t set = (size_t)fe->nrx * (size_t)mon->bins, R = (size_t)rows;
	if (R * set * 12 > ((size_t)1 << 30)) return fail(HFDL_GPU_ERANGE, "spectrum history of %d rows x %d receivers x %d bands: more than 1 GiB", rows, fe->nrx, mon->bins);
	HIP_TRY(hipSetDevice(fe->device));
	// the old ring goes once nothing queued writes into it any more: wait for the monitor launches queued so far, nothing else
	if (mon->hist) {
		(void)hipEventSynchronize(mon->newest());
		mon->last = nullptr;
		mon->hist.reset();
	}
	if (rows == 0) return 0;
	auto h = std::make_unique<SpectrumHistory>();
	hipError_t e = h->acc.alloc(sizeof(float2) * R * set);
	if (e == hipSuccess && (mon->flags & HFDL_GPU_SPECTRUM_MAXHOLD)) e = h->peak.alloc(sizeof(float) * R * set);
	if (e == hipSuccess) e = h->host.alloc((size_t)SpectrumHistory::CHUNK * 3 * (size_t)mon->bins);
	h->ev.resize(R);
	for (size_t i = 0; i < R && e == hipSuccess; i++) e = h->ev[i].create(EV_NO_TIMING);
	if (e != hipSuccess) return ALLOC_FAIL(e, "spectrum history");
	h->rows = rows;
	h->interval = interval_blocks;
	h->info.resize(R);
	mon->hist = std::move(h);              // the first block opens row 0: "start over" is set, nothing to clear on the device
	return 0;
}

extern "C" int hfdl_gpu_frontend_spectrum_row_close(hfdl_gpu_frontend *fe, uint64_t *row)
{
	if (!fe || !row) return fail(HFDL_GPU_EINVAL, "null argument");
	SpectrumHistory *h = fe->mon ? fe->mon->hist.get() : nullptr;
	if (!h) return fail(HFDL_GPU_EINVAL, "the spectrum history is off: hfdl_gpu_frontend_spectrum_history() first");
	*row = h->open;
	if (h->open_blocks) h->close();
	return 0;
}

extern "C" int hfdl_gpu_frontend_spectrum_rows(hfdl_gpu_frontend *fe, int32_t rx, uint64_t from_row, int32_t max_rows,
		float *mean, float *peak, hfdl_gpu_spectrum_row *info, int32_t *n, uint64_t *next_row, int wait)
{
	if (!fe || !n || !next_row) return fail(HFDL_GPU_EINVAL, "null argument");
	SpectrumMonitor *mon = fe->mon.get();
	SpectrumHistory *h = mon ? mon->hist.get() : nullptr;
	if (!h) return fail(HFDL_GPU_EINVAL, "the spectrum history is off: hfdl_gpu_frontend_spectrum_history() first");
	if (int rc = check_receiver(fe, rx)) return rc;
	if (max_rows < 0) return fail(HFDL_GPU_EINVAL, "max_rows %d", max_rows);
	if (max_rows > 0 && (!mean || !info)) return fail(HFDL_GPU_EINVAL, "null argument");
	if (peak && !(mon->flags & HFDL_GPU_SPECTRUM_MAXHOLD)) return fail(HFDL_GPU_EINVAL, "peak asked for, but the monitor was enabled without HFDL_GPU_SPECTRUM_MAXHOLD");
	const uint64_t R = (uint64_t)h->rows;
	uint64_t from = std::min(std::max(from_row, h->oldest()), h->open);
	uint64_t end = std::min(h->open, from + (uint64_t)max_rows);
	*n = 0;
	*next_row = from;
	if (end == from) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	// Finished = the slot's event has fired (it rode on the row's last launch).  Launches run in order, so the rows finished are a prefix.
	if (wait) HIP_TRY(hipEventSynchronize(h->ev[(end - 1) % R]));
	else for (uint64_t r = from; r < end; r++) {
		const hipError_t e = hipEventQuery(h->ev[r % R]);
		if (e == hipSuccess) continue;
		if (e != hipErrorNotReady) return fail(HFDL_GPU_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
		(void)hipGetLastError();           // "not yet" is an answer, as in hfdl_gpu_frontend_input_copied()
		end = r;
	}
	// the collection stream has nothing to wait for: it copies beside the kernels in flight, CHUNK rows per wait
	const size_t nb = (size_t)mon->bins, K = (size_t)fe->nrx;
	hipStream_t st = fe->demod.st_collect;
	for (uint64_t r0 = from; r0 < end; r0 += SpectrumHistory::CHUNK) {
		const size_t cnt = (size_t)std::min<uint64_t>(SpectrumHistory::CHUNK, end - r0);
		for (size_t i = 0; i < cnt; i++) {
			const size_t at = ((size_t)((r0 + i) % R) * K + (size_t)rx) * nb;
			float *hb = h->host.p + i * 3 * nb;
			HIP_TRY(hipMemcpyAsync(hb, h->acc.as<float2>() + at, sizeof(float2) * nb, hipMemcpyDeviceToHost, st));
			if (peak) HIP_TRY(hipMemcpyAsync(hb + 2 * nb, h->peak.as<float>() + at, sizeof(float) * nb, hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(hipStreamSynchronize(st));
		for (size_t i = 0; i < cnt; i++) {
			const size_t o = (size_t)(r0 + i - from);
			const float *hb = h->host.p + i * 3 * nb;
			info[o] = h->info[(size_t)((r0 + i) % R)];
			mean_of(hb, nb, info[o].blocks, mean + o * nb);
			if (peak) memcpy(peak + o * nb, hb + 2 * nb, sizeof(float) * nb);
		}
	}
	*n = (int32_t)(end - from);
	*next_row = end;
	return 0;
}

// ---------------------------------------------------------------- carrier canceller

static_assert(HFDL_GPU_NOTCH_STATE_FLOATS == NOTCH_STATE_FLOATS, "include/hfdl_gpu.h and notch.h name the same state");

// From this call on the selected channels are cancelled with step `mu`, each from zero state; blocks pushed before it are handed over
// as they would have been.  The half being filled is closed as a retune closes it; the new selection and the cleared state follow the
// closed half's canceller and demodulators on stream B.  Everything is checked and allocated before the first launch.
extern "C" int hfdl_gpu_frontend_notch_enable(hfdl_gpu_frontend *fe, const int32_t *channels, int32_t nsel, float mu)
{
	if (!(mu == 0.f || notch_mu_valid(mu))) return fail(HFDL_GPU_EINVAL, "canceller step %g: 0 (off) or %g .. %g", (double)mu, (double)NOTCH_MU_MIN, (double)NOTCH_MU_MAX);
	if (!fe || nsel < 0 || (nsel > 0 && !channels)) return fail(HFDL_GPU_EINVAL, "null argument");
	const int nch = fe->geo.nch;
	std::vector<int32_t> sel(channels, channels + nsel);
	std::vector<bool> seen((size_t)nch, nsel == 0);             // none listed: every channel
	if (const int bad = check_channel_list(nch, channels, nsel, seen); bad >= 0) return fail(HFDL_GPU_EINVAL, "canceller: channel %d out of range or listed twice", channels[bad]);
	for (int c = 0; nsel == 0 && c < nch; c++) sel.push_back(c);
	if (!fe->notch && mu == 0.f) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	if (!fe->notch) {
		auto n = std::make_unique<Notch>();
		hipError_t e = n->out.alloc(sizeof(float2) * 2 * (size_t)fe->half_blocks * (size_t)nch * (size_t)fe->geo.outs);
		if (e == hipSuccess) e = n->sel.alloc(sizeof(int32_t) * (size_t)nch);
		if (e == hipSuccess) e = n->state.alloc(sizeof(float) * NOTCH_STATE_FLOATS * (size_t)nch);
		if (e == hipSuccess) e = n->rec.alloc(sizeof(NotchRecord) * (size_t)nch);
		if (e == hipSuccess) e = n->host.alloc(1);
		if (e == hipSuccess) e = n->host_sel.alloc((size_t)nch);
		if (e == hipSuccess) e = n->staged.create(EV_NO_TIMING);
		if (e == hipSuccess) e = n->ev.create(EV_NO_TIMING);
		if (e != hipSuccess) return ALLOC_FAIL(e, "canceller");
		fe->notch = std::move(n);
	}
	// the boundary: what was pushed so far goes to the demodulator under the old setting
	if (int rc = close_boundary(fe)) return rc;
	Notch &n = *fe->notch;
	n.mu = mu;
	if (mu == 0.f) return 0;
	if (n.staging) HIP_TRY(hipEventSynchronize(n.staged));       // the upload of the enable before this one has read the page-locked list
	std::copy(sel.begin(), sel.end(), n.host_sel.p);
	HIP_TRY(hipMemcpyAsync(n.sel.p, n.host_sel.p, sizeof(int32_t) * sel.size(), hipMemcpyHostToDevice, fe->stream_b));
	HIP_TRY(hipEventRecord(n.staged, fe->stream_b));
	n.staging = true;
	HIP_TRY(hipMemsetAsync(n.state.p, 0, sizeof(float) * NOTCH_STATE_FLOATS * (size_t)nch, fe->stream_b));
	HIP_TRY(hipMemsetAsync(n.rec.p, 0, sizeof(NotchRecord) * (size_t)nch, fe->stream_b));
	n.nsel = (int)sel.size();
	n.selected = seen;
	n.launched = false;
	return 0;
}

// A half's hand-over to the demodulator: stream B waits for the half (`ready`, may be null) here, and the demodulators read the rows
// returned -- the selected channels' cancelled, the others' word for word -- behind the canceller on the stream.  Null: the canceller is
// off, nothing was queued.  A HIP call that fails ends the hook; the caller finds it with hipGetLastError(), as it finds a failed launch.
const float2 *launch_canceller(hfdl_gpu_frontend *fe, int slot0, int nblk, hipEvent_t ready)
{
	Notch *n = fe->notch.get();
	if (!n || !(n->mu > 0.f)) return nullptr;
	const Geometry &g = fe->geo;
	const size_t at = (size_t)slot0 * (size_t)g.nch * (size_t)g.outs;
	float2 *out = n->out.as<float2>() + at;
	if (ready && hipStreamWaitEvent(fe->stream_b, ready, 0) != hipSuccess) return out;
	if (n->nsel < g.nch && hipMemcpyAsync(out, fe->chan_slot(slot0), sizeof(float2) * (size_t)nblk * (size_t)g.nch * (size_t)g.outs, hipMemcpyDeviceToDevice, fe->stream_b) != hipSuccess) return out;
	NotchJob j;
	j.in = fe->chan_slot(slot0); j.out = out; j.cnt = fe->cnt_slot(slot0); j.sel = n->sel.as<int32_t>();
	j.state = n->state.as<float>(); j.rec = n->rec.as<NotchRecord>();
	j.nch = g.nch; j.outs = g.outs; j.nblk = nblk; j.nsel = n->nsel; j.mu = n->mu;
	launch_notch(j, fe->stream_b, n->ev);
	n->launched = true;
	return out;
}

// a retuned channel meets a fresh canceller: its taps and delay line go where its demodulator state goes, behind the closed half on B
int canceller_retuned(hfdl_gpu_frontend *fe, int channel)
{
	if (Notch *n = fe->notch.get()) HIP_TRY(hipMemsetAsync(n->state.as<float>() + (size_t)channel * NOTCH_STATE_FLOATS, 0, sizeof(float) * NOTCH_STATE_FLOATS, fe->stream_b));
	return 0;
}

extern "C" int hfdl_gpu_frontend_notch_stats(hfdl_gpu_frontend *fe, int32_t channel, hfdl_gpu_notch_stats *out)
{
	if (!fe || !out) return fail(HFDL_GPU_EINVAL, "null argument");
	Notch *n = fe->notch.get();
	if (!n) return fail(HFDL_GPU_EINVAL, "the canceller was never enabled");
	if (channel < 0 || channel >= fe->geo.nch || !n->selected[(size_t)channel]) return fail(HFDL_GPU_EINVAL, "channel %d is out of range or not selected", channel);
	memset(out, 0, sizeof(*out));
	if (!n->launched) return 0;
	if (int rc = read_record(fe, n->ev, n->rec.as<NotchRecord>() + channel, n->host.p, sizeof(NotchRecord))) return rc;
	const NotchRecord &r = *n->host.p;
	out->blocks = r.blocks; out->resets = r.resets;
	out->last_in_power = r.in_power; out->last_out_power = r.out_power; out->tap_energy = r.tap_energy;
	return 0;
}

// ---------------------------------------------------------------- channel baseband export

static_assert(HFDL_GPU_EXPORT_CF32 == EXPORT_CF32 && HFDL_GPU_EXPORT_CS16 == EXPORT_CS16, "include/hfdl_gpu.h and spectrum.h name the same formats");

extern "C" int hfdl_gpu_frontend_export_enable(hfdl_gpu_frontend *fe, const int32_t *channels, int32_t nsel, int format, float scale, int32_t ring_blocks)
{
	if (!fe || (!channels && nsel > 0)) return fail(HFDL_GPU_EINVAL, "null argument");
	const size_t S = (size_t)nsel, R = (size_t)ring_blocks, P = (size_t)fe->geo.outs - 1;
	const size_t es = format == HFDL_GPU_EXPORT_CS16 ? sizeof(short2) : sizeof(float2);
	if (nsel > 0) {
		std::vector<bool> seen((size_t)fe->geo.nch);
		const bool ok = nsel <= fe->geo.nch && (format == HFDL_GPU_EXPORT_CF32 || format == HFDL_GPU_EXPORT_CS16) && ring_blocks >= 2 && ring_blocks <= HFDL_GPU_EXPORT_RING_MAX
			&& (format == HFDL_GPU_EXPORT_CF32 || (scale > 0.f && scale <= 3.402823466e38f)) && check_channel_list(fe->geo.nch, channels, nsel, seen) < 0;
		if (!ok) return fail(HFDL_GPU_EINVAL, "export: bad channels, format, scale or ring");
		if (R * S * (P * es + 12) > ((size_t)1 << 30)) return fail(HFDL_GPU_ERANGE, "export ring above 1 GiB");
	} else if (nsel < 0) return fail(HFDL_GPU_EINVAL, "export: nsel %d", nsel);
	HIP_TRY(hipSetDevice(fe->device));
	std::unique_ptr<ChannelExport> x;
	if (nsel > 0) {
		x = std::make_unique<ChannelExport>();
		// a collection copies up to 4 MiB of samples per wait on its stream, a block at least
		x->chunk = std::max<size_t>(1, std::min(R, ((size_t)4 << 20) / (S * P * es)));
		hipError_t e = x->channels.alloc(sizeof(int32_t) * S);
		if (e == hipSuccess) e = x->samples.alloc(R * S * P * es);
		if (e == hipSuccess) e = x->counts.alloc(R * S * 4);
		if (e == hipSuccess) e = x->power.alloc(R * S * 4);
		if (e == hipSuccess) e = x->clipped.alloc(R * S * 4);
		if (e == hipSuccess) e = x->host.alloc(x->chunk * S * (P * es + 12));
		x->ev.resize(R);
		for (size_t i = 0; i < R && e == hipSuccess; i++) e = x->ev[i].create(EV_NO_TIMING);
		if (e == hipSuccess) e = hipMemcpy(x->channels.p, channels, sizeof(int32_t) * S, hipMemcpyHostToDevice);
		if (e != hipSuccess) return ALLOC_FAIL(e, "export");
		x->nsel = nsel; x->format = format; x->scale = scale;
		x->last_of.resize(R);
		x->ring.start((uint32_t)ring_blocks, fe->blocks);      // a block waiting in the half being filled is older: the hook leaves it out
	}
	// the old ring goes once nothing queued writes into it any more: wait for the export launches queued so far, nothing else
	if (fe->exp && fe->exp->newest) (void)hipEventSynchronize(fe->exp->newest);
	fe->exp = std::move(x);
	return 0;
}

// behind the half's inverse FFT on stream A, whose timed pair and done event stay where they are; the next inverse FFT into this half is
// behind it on the stream, which is all that makes its read safe.  The half's blocks are the newest nblk.
void launch_export(hfdl_gpu_frontend *fe, int slot0, int nblk)
{
	ChannelExport *x = fe->exp.get();
	if (!x) return;
	const Geometry &g = fe->geo;
	const uint32_t skip = x->ring.skip_of_half(fe->blocks - (uint64_t)nblk, (uint32_t)nblk);
	if (skip >= (uint32_t)nblk) return;
	ExportJob e;
	e.chan = fe->chan_slot(slot0 + (int)skip); e.cnt = fe->cnt_slot(slot0 + (int)skip); e.channels = x->channels.as<int32_t>();
	e.nch = g.nch; e.outs = g.outs; e.P = g.outs - 1; e.nsel = x->nsel; e.nblk = nblk - (int)skip; e.format = x->format; e.scale = x->scale;
	e.slot0 = x->ring.slot(fe->blocks - (uint64_t)e.nblk); e.R = x->ring.R;
	e.samples = x->samples.p; e.counts = x->counts.as<int32_t>(); e.power = x->power.as<float>(); e.clipped = x->clipped.as<uint32_t>();
	x->newest = x->ev[x->ring.push_launch(x->last_of.data(), fe->blocks - 1)];
	launch_export_pack(e, fe->stream, x->newest);
}

extern "C" int hfdl_gpu_frontend_export_read(hfdl_gpu_frontend *fe, uint64_t from_block, int32_t max_blocks, void *samples, int32_t *counts,
		float *power, uint32_t *clipped, hfdl_gpu_export_block *info, int32_t *n, uint64_t *next_block, int wait)
{
	if (!fe || !n || !next_block) return fail(HFDL_GPU_EINVAL, "null argument");
	ChannelExport *x = fe->exp.get();
	if (!x || max_blocks < 0 || (max_blocks > 0 && (!samples || !counts || !info))) return fail(HFDL_GPU_EINVAL, "export off, or bad arguments");
	HIP_TRY(hipSetDevice(fe->device));
	ExportRing &ring = x->ring;
	// Finished = the event that rode on the block's launch has fired.  wait: for the newest launch queued -- nothing is closed for it.
	if (wait && x->newest) HIP_TRY(hipEventSynchronize(x->newest));
	hipError_t bad = hipSuccess;
	ring.settle(x->last_of.data(), [&](uint32_t at) {
		const hipError_t e = hipEventQuery(x->ev[at]);
		if (e == hipSuccess) return true;
		if (e == hipErrorNotReady) (void)hipGetLastError(); else bad = e;       // "not yet" is an answer, as in hfdl_gpu_frontend_input_copied()
		return false;
	});
	if (bad != hipSuccess) return fail(HFDL_GPU_EHIP, "hipEventQuery: %s", hipGetErrorString(bad));
	uint64_t from = 0, end = 0;
	ring.range(from_block, (uint64_t)max_blocks, from, end);
	// the collection stream has nothing to wait for: it copies beside the kernels in flight, a run of consecutive slots per wait
	const size_t S = (size_t)x->nsel, row = S * ((size_t)fe->geo.outs - 1) * (x->format == HFDL_GPU_EXPORT_CS16 ? sizeof(short2) : sizeof(float2));
	hipStream_t st = fe->demod.st_collect;
	for (uint64_t b = from, run = 0; b < end; b += run) {
		const size_t slot = ring.slot(b), o = (size_t)(b - from);
		run = std::min<uint64_t>(std::min<uint64_t>(x->chunk, end - b), ring.R - slot);
		char *h = x->host.p, *meta = h + x->chunk * row;
		const void *src[3] = { x->counts.p, power ? x->power.p : nullptr, clipped ? x->clipped.p : nullptr };
		void *dst[3] = { counts + o * S, power ? power + o * S : nullptr, clipped ? clipped + o * S : nullptr };
		HIP_TRY(hipMemcpyAsync(h, (const char *)x->samples.p + slot * row, run * row, hipMemcpyDeviceToHost, st));
		for (int k = 0; k < 3; k++)
			if (src[k]) HIP_TRY(hipMemcpyAsync(meta + k * x->chunk * S * 4, (const char *)src[k] + slot * S * 4, run * S * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		memcpy((char *)samples + o * row, h, run * row);
		for (int k = 0; k < 3; k++)
			if (src[k]) memcpy(dst[k], meta + k * x->chunk * S * 4, run * S * 4);
		for (uint64_t i = 0; i < run; i++) info[o + i].block = b + i;
	}
	*n = (int32_t)(end - from);
	*next_block = end;
	return 0;
}
