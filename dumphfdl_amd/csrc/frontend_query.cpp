// frontend_query.cpp -- what a caller reads from a front end: the error text, geometry, input-done queries, timers, statistics, stage
// taps, counters, the spectrum monitor, the blanker's and the I/Q corrector's switches and records; and the page-locked allocator.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include "frontend.h"
#include "demod_lds.h"

using namespace hfdl;

static thread_local char g_err[512] = "";

int hfdl::fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return code;
}

int hfdl::fail_hip(hipError_t e, bool alloc, const char *expr, const char *file, int line)
{
	return fail(alloc && e == hipErrorOutOfMemory ? HFDL_GPU_ENOMEM : HFDL_GPU_EHIP, "%s: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
}

extern "C" const char *hfdl_gpu_last_error(void) { return g_err; }

// ---------------------------------------------------------------- geometry

static void fill_block_geometry(const Plan &p, hfdl_gpu_geometry *g)
{
	g->pre_decimation = p.pre; g->post_decimation = p.post;
	g->taps_length = p.taps_length; g->overlap_length = p.overlap;
	g->fft_size = p.n; g->fft_inv_size = p.m; g->input_size = p.input_size;
	g->post_input_size = p.post_input_size; g->scrap = p.scrap;
	g->outputs_per_block = p.post_input_size / p.post;
	g->max_outputs_per_block = (p.post_input_size + p.post - 1) / p.post;
}

extern "C" int hfdl_gpu_frontend_geometry(const hfdl_gpu_frontend *fe, hfdl_gpu_geometry *g)
{
	if (!fe || !g) return fail(HFDL_GPU_EINVAL, "null argument");
	fill_block_geometry(fe->plan, g);
	g->sample_rate = fe->sample_rate; g->decimation = fe->decimation;
	g->channels = fe->geo.nch; g->fold_slices = fe->geo.slices;
	g->demod_batch = fe->batch;
	g->fold_batch = fe->fold_nb;
	g->prefetch_depth = fe->n_stage - 1;
	g->fold_rows = fe->fold_rows_max ? fe->fold_rows_max : fe->plan.pre;
	g->transition_bw = fe->tbw;
	g->resamp_rate = (float)(1800 * 3) / ((float)fe->sample_rate / (float)fe->decimation);
	return 0;
}

extern "C" int hfdl_gpu_plan_geometry(int32_t decimation, float transition_bw, hfdl_gpu_geometry *g)
{
	if (!g || decimation < 1 || !(transition_bw > 0.f)) return fail(HFDL_GPU_EINVAL, "bad arguments");
	Plan p;
	if (!plan_block(p, transition_bw, decimation, 0.f)) return fail(HFDL_GPU_EINVAL, "fastddc planning failed");
	memset(g, 0, sizeof(*g));
	fill_block_geometry(p, g);
	g->decimation = decimation;
	g->transition_bw = transition_bw;
	return 0;
}

extern "C" int hfdl_gpu_frontend_channel_receiver(const hfdl_gpu_frontend *fe, int32_t channel, int32_t *rx, int32_t *centerfreq)
{
	if (!fe || !rx || !centerfreq) return fail(HFDL_GPU_EINVAL, "null argument");
	if (channel < 0 || channel >= fe->geo.nch) return fail(HFDL_GPU_EINVAL, "channel %d out of range (%d channels)", channel, fe->geo.nch);
	*rx = fe->rx_of[(size_t)channel];
	*centerfreq = fe->rx_center[(size_t)*rx];
	return 0;
}

extern "C" int hfdl_gpu_frontend_real_input(const hfdl_gpu_frontend *fe, int32_t *is_real, int32_t *real_rate)
{
	if (!fe || !is_real || !real_rate) return fail(HFDL_GPU_EINVAL, "null argument");
	*is_real = fe->real_rate != 0;
	*real_rate = fe->real_rate;
	return 0;
}

// ---------------------------------------------------------------- page-locked host memory

// page-locked ranges handed out by hfdl_gpu_host_alloc(): only these are left to the DMA engine after push_block returns
static std::mutex g_pinned_lock;
static std::vector<std::pair<const char *, size_t>> g_pinned;

bool hfdl::is_library_pinned(const void *p, size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_pinned_lock);
	for (auto &r : g_pinned)
		if ((const char *)p >= r.first && (const char *)p + bytes <= r.first + r.second) return true;
	return false;
}

extern "C" int hfdl_gpu_host_alloc(void **ptr, size_t bytes)
{
	if (!ptr || !bytes) return fail(HFDL_GPU_EINVAL, "bad arguments");
	HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
	std::lock_guard<std::mutex> lk(g_pinned_lock);
	g_pinned.emplace_back((const char *)*ptr, bytes);
	return 0;
}

extern "C" void hfdl_gpu_host_free(void *ptr)
{
	if (!ptr) return;
	{
		std::lock_guard<std::mutex> lk(g_pinned_lock);
		for (size_t i = 0; i < g_pinned.size(); i++)
			if (g_pinned[i].first == (const char *)ptr) { g_pinned.erase(g_pinned.begin() + (long)i); break; }
	}
	(void)hipHostFree(ptr);         // the caller's memory by contract: the one release outside the handle types
}

// ---------------------------------------------------------------- input-done queries

extern "C" int hfdl_gpu_frontend_input_done(hfdl_gpu_frontend *fe)
{
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(fe->device));
	// the newest copy's event, not the stream: the input stream also carries the forward FFTs of device-resident blocks
	if (fe->host_blocks) HIP_TRY(hipEventSynchronize(fe->input_event(fe->host_blocks - 1)));
	return 0;
}

static int check_host_block(const hfdl_gpu_frontend *fe, uint64_t host_block)
{
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	if (host_block >= fe->host_blocks) return fail(HFDL_GPU_EINVAL, "host block %llu has not been pushed (%llu so far)", (unsigned long long)host_block, (unsigned long long)fe->host_blocks);
	HIP_TRY(hipSetDevice(fe->device));
	return 0;
}

extern "C" int hfdl_gpu_frontend_input_done_upto(hfdl_gpu_frontend *fe, uint64_t host_block)
{
	if (int rc = check_host_block(fe, host_block)) return rc;
	HIP_TRY(hipEventSynchronize(fe->input_event(host_block)));
	return 0;
}

extern "C" int hfdl_gpu_frontend_input_copied(hfdl_gpu_frontend *fe, uint64_t host_block)
{
	if (int rc = check_host_block(fe, host_block)) return rc;
	const hipError_t e = hipEventQuery(fe->input_event(host_block));
	if (e == hipSuccess) return 1;
	if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }       // "not yet" is an answer, not an error to be found by a later check
	return fail(HFDL_GPU_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
}

// ---------------------------------------------------------------- timers

// what every getter below starts with: finish everything queued (a sync reads the timed launches back), then read
static int sync_to_read(hfdl_gpu_frontend *fe, bool args_ok = true)
{
	if (!fe || !args_ok) return fail(HFDL_GPU_EINVAL, "null argument");
	return hfdl_gpu_frontend_sync(fe);
}

extern "C" int hfdl_gpu_frontend_reset_timers(hfdl_gpu_frontend *fe, int enable)
{
	if (int rc = sync_to_read(fe)) return rc;
	return fe->timers.reset(enable != 0);
}

static int stage_totals(hfdl_gpu_frontend *fe, Stage s, double *ms, int64_t *launches, int64_t *blocks)
{
	if (int rc = sync_to_read(fe)) return rc;
	const LaunchTimers::Totals &t = fe->timers.stage[s];
	if (ms) *ms = t.ms;
	if (launches) *launches = t.launches;
	if (blocks) *blocks = t.blocks;
	return 0;
}

extern "C" int hfdl_gpu_frontend_fold_time_ms(hfdl_gpu_frontend *fe, double *total_ms, int64_t *launches) { return stage_totals(fe, ST_FOLD, total_ms, launches, nullptr); }

extern "C" int hfdl_gpu_frontend_fold_blocks(hfdl_gpu_frontend *fe, int64_t *blocks)
{
	if (!blocks) return fail(HFDL_GPU_EINVAL, "null argument");
	return stage_totals(fe, ST_FOLD, nullptr, nullptr, blocks);
}

extern "C" int hfdl_gpu_frontend_demod_time_ms(hfdl_gpu_frontend *fe, double *total_ms, int64_t *launches, int64_t *blocks) { return stage_totals(fe, ST_DEMOD, total_ms, launches, blocks); }

extern "C" int hfdl_gpu_frontend_fold_launch_shapes(hfdl_gpu_frontend *fe, int64_t counts[HFDL_GPU_FOLD_BATCH_MAX + 1], double ms[HFDL_GPU_FOLD_BATCH_MAX + 1])
{
	if (int rc = sync_to_read(fe, counts)) return rc;
	for (int i = 0; i <= FOLD_MAX_BLOCKS; i++) counts[i] = fe->timers.fold_shapes[i];
	if (ms) for (int i = 0; i <= FOLD_MAX_BLOCKS; i++) ms[i] = fe->timers.fold_shape_ms[i];
	return 0;
}

extern "C" int hfdl_gpu_frontend_stage_times(hfdl_gpu_frontend *fe, double ms[5], int64_t launches[5])
{
	if (int rc = sync_to_read(fe, ms && launches)) return rc;
	for (int s = 0; s < ST_N; s++) { ms[s] = fe->timers.stage[s].ms; launches[s] = fe->timers.stage[s].launches; }
	return 0;
}

extern "C" int hfdl_gpu_frontend_step_period_ms(hfdl_gpu_frontend *fe, double *period_ms)
{
	if (int rc = sync_to_read(fe, period_ms)) return rc;
	// first timed fold start -> last timed fold start covers every timed block but the last launch's; per BLOCK
	const LaunchTimers &t = fe->timers;
	const int64_t covered = t.stage[ST_FOLD].blocks - t.fold_last_blocks;
	*period_ms = (t.stage[ST_FOLD].launches > 1 && covered > 0) ? t.span_ms / (double)covered : 0.0;
	return 0;
}

// ---------------------------------------------------------------- statistics, counters, stage taps

extern "C" int hfdl_gpu_frontend_all_channel_stats(hfdl_gpu_frontend *fe, hfdl_gpu_channel_stats *out, int32_t cap, int32_t *n)
{
	if (!fe || !out || !n) return fail(HFDL_GPU_EINVAL, "null argument");
	if (cap < fe->geo.nch) return fail(HFDL_GPU_ERANGE, "%d channels, buffer holds %d", fe->geo.nch, cap);
	HIP_TRY(hipSetDevice(fe->device));
	memset(out, 0, sizeof(*out) * (size_t)fe->geo.nch);
	if (int rc = fe->demod.stats_all(out, fe->geo.nch)) return rc;
	for (int i = 0; i < fe->geo.nch; i++) out[i].freq = fe->freqs[(size_t)i];
	*n = fe->geo.nch;
	return 0;
}

extern "C" int hfdl_gpu_frontend_channel_stats(hfdl_gpu_frontend *fe, int32_t channel, hfdl_gpu_channel_stats *out)
{
	if (!fe || !out) return fail(HFDL_GPU_EINVAL, "null argument");
	if (channel < 0 || channel >= fe->geo.nch) return fail(HFDL_GPU_EINVAL, "channel out of range");
	int rc = hfdl_gpu_frontend_sync(fe);
	if (rc) return rc;
	memset(out, 0, sizeof(*out));
	out->freq = fe->freqs[(size_t)channel];
	return fe->demod.stats(channel, out);
}

extern "C" int hfdl_gpu_frontend_counters(hfdl_gpu_frontend *fe, hfdl_gpu_frontend_counters_t *out)
{
	if (!fe || !out) return fail(HFDL_GPU_EINVAL, "null argument");
	memset(out, 0, sizeof(*out));
	out->blocks = fe->blocks;
	out->pdus_taken = fe->demod.taken;
	out->pdus_dropped = fe->demod.dropped;
	out->pdu_ring_capacity = (uint32_t)fe->demod.pdu_cap;
	return 0;
}

extern "C" int hfdl_gpu_frontend_enable_taps(hfdl_gpu_frontend *fe, int enable)
{
	if (int rc = sync_to_read(fe)) return rc;
	fe->demod.taps_enabled = enable != 0;
	return 0;
}

extern "C" int hfdl_gpu_frontend_read_tap_block(hfdl_gpu_frontend *fe, int what, int32_t channel, int32_t back, float *dst, size_t cap, size_t *n_floats)
{
	if (int rc = sync_to_read(fe, dst && n_floats)) return rc;
	const Geometry &g = fe->geo;
	// the channelizer's own buffers hold every block of the newest half: `back` blocks before the newest one
	if (back < 0 || back > fe->last_index) return fail(HFDL_GPU_ERANGE, "block %d back is not held any more (%d are)", back, fe->last_index);
	if (back && what != HFDL_GPU_TAP_SPECTRUM && what != HFDL_GPU_TAP_CHAN_OUT && what != HFDL_GPU_TAP_NCO_PHASORS && what != HFDL_GPU_TAP_NOTCH_OUT)
		return fail(HFDL_GPU_EINVAL, "tap %d holds the last launch only", what);
	const int slot = fe->last_slot - back, index = fe->last_index - back;
	// (the spectrum tap of a one-receiver front end ignores `channel`; with several receivers it selects the channel's receiver)
	if ((what != HFDL_GPU_TAP_SPECTRUM || fe->nrx > 1) && (channel < 0 || channel >= g.nch)) return fail(HFDL_GPU_EINVAL, "channel out of range");
	const void *src = nullptr;
	size_t nf = 0;
	switch (what) {
	case HFDL_GPU_TAP_SPECTRUM:
		src = fe->spec_slot(fe->last_set, index) + (fe->nrx > 1 ? (size_t)fe->rx_of[(size_t)channel] * (size_t)g.n : 0);
		nf = 2 * (size_t)g.n;
		if (!g.mix_l1) break;
		[[fallthrough]];                       // the mixed domain: the slot holds pass 2's output -- the spectrum is made here, by the pass 3 the pipeline left out
	case HFDL_GPU_TAP_FILTER: {
		// the taps lie in matrix-operand order (kernels.h tap_index_f): a kernel gathers the channel into plain cf32[N].  In the mixed
		// domain both taps go back to pass 2's own order and through pass 3: the words the three-pass transform leaves
		if (2 * (size_t)g.n > cap) return fail(HFDL_GPU_ERANGE, "tap needs %zu floats, buffer holds %zu", 2 * (size_t)g.n, cap);
		DevBuf plain, mid;
		HIP_TRY(plain.alloc(sizeof(float2) * (size_t)g.n));
		if (g.mix_l1) {
			HIP_TRY(mid.alloc(sizeof(float2) * (size_t)g.n));
			if (what == HFDL_GPU_TAP_SPECTRUM) launch_mixed_block_unpack(fe->fft.p, g, (const float2 *)src, mid.as<float2>(), fe->stream);
			else launch_mixed_tap_unpack(fe->fft.p, g, fe->d_taps, fe->slot_of(channel), mid.as<float2>(), fe->stream);
			FftVariant v;
			v.passes = FFT_PASS_3;
			launch_fft_forward(fe->fft.p, nullptr, (const void *)nullptr, SFMT_CF32, 0, nullptr, mid.as<float2>(), plain.as<float2>(), true, fe->stream, FftOutLayout(), nullptr, NcoJob(), nullptr, nullptr, v);
		} else launch_tap_extract(fe->d_taps, g, fe->slot_of(channel), plain.as<float2>(), fe->stream);
		HIP_TRY(hipStreamSynchronize(fe->stream));
		HIP_TRY(hipMemcpy(dst, plain.p, sizeof(float2) * (size_t)g.n, hipMemcpyDeviceToHost));
		*n_floats = 2 * (size_t)g.n;
		return 0; }
	case HFDL_GPU_TAP_CHAN_OUT:
	case HFDL_GPU_TAP_NOTCH_OUT: {
		// the channelizer's own row, or the same row of the canceller's buffer: what the demodulator read
		const Notch *nt = fe->notch.get();
		if (what == HFDL_GPU_TAP_NOTCH_OUT && !(nt && nt->mu > 0.f)) return fail(HFDL_GPU_EINVAL, "tap %d: the canceller is off", what);
		int cnt = 0;
		HIP_TRY(hipMemcpy(&cnt, fe->cnt_slot(slot) + channel, sizeof(cnt), hipMemcpyDeviceToHost));
		src = (what == HFDL_GPU_TAP_CHAN_OUT ? fe->chan_slot(slot) : nt->out.as<float2>() + (size_t)slot * (size_t)g.nch * (size_t)g.outs) + (size_t)channel * g.outs;
		nf = 2 * (size_t)cnt; break; }
	case HFDL_GPU_TAP_NCO_PHASORS: {
		int cnt = 0;
		HIP_TRY(hipMemcpy(&cnt, fe->cnt_slot(slot) + channel, sizeof(cnt), hipMemcpyDeviceToHost));
		if (2 * (size_t)cnt > cap) return fail(HFDL_GPU_ERANGE, "tap needs %zu floats, buffer holds %zu", 2 * (size_t)cnt, cap);
		// column `channel` of the [outs][nch] table
		if (cnt) HIP_TRY(hipMemcpy2D(dst, sizeof(float2), fe->ph_slot(fe->last_set, index) + channel, sizeof(float2) * (size_t)g.nch, sizeof(float2), (size_t)cnt, hipMemcpyDeviceToHost));
		*n_floats = 2 * (size_t)cnt;
		return 0; }
	case HFDL_GPU_TAP_PHASE_CYCLES: src = fe->demod.d_tap_lvl + (size_t)channel * fe->demod.cap + phase_slot(fe->demod.cap, PHASE_AHEAD); nf = DM_PHASE_SLOTS; break;
	default:
		if (int rc = fe->demod.tap(what, channel, &src, &nf)) return rc;
	}
	if (nf > cap) return fail(HFDL_GPU_ERANGE, "tap needs %zu floats, buffer holds %zu", nf, cap);
	if (nf) HIP_TRY(hipMemcpy(dst, src, sizeof(float) * nf, hipMemcpyDeviceToHost));
	*n_floats = nf;
	return 0;
}

extern "C" int hfdl_gpu_frontend_read_tap(hfdl_gpu_frontend *fe, int what, int32_t channel, float *dst, size_t cap, size_t *n_floats)
{
	return hfdl_gpu_frontend_read_tap_block(fe, what, channel, 0, dst, cap, n_floats);
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
	if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? HFDL_GPU_ENOMEM : HFDL_GPU_EHIP, "spectrum monitor buffers: %s", hipGetErrorString(e));
	mon->bins = bins;
	mon->flags = flags;
	mon->fresh = ~(uint64_t)0;             // every receiver starts over with the next block: nothing to clear on the device
	mon->blocks.assign(K, 0);
	mon->first.assign(K, 0);
	fe->mon = std::move(mon);
	return 0;
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
	if (rx < 0 || rx >= fe->nrx) return fail(HFDL_GPU_EINVAL, "receiver %d out of range (%d receivers)", rx, fe->nrx);
	if (peak && !(mon->flags & HFDL_GPU_SPECTRUM_MAXHOLD)) return fail(HFDL_GPU_EINVAL, "peak asked for, but the monitor was enabled without HFDL_GPU_SPECTRUM_MAXHOLD");
	if (cap < mon->bins) return fail(HFDL_GPU_ERANGE, "%d bands, buffer holds %d", mon->bins, cap);
	const bool pending = (mon->fresh >> rx) & 1;      // reset (or just enabled) and no block since
	const uint64_t T = pending ? 0 : mon->blocks[(size_t)rx];
	*blocks = T;
	*first_block = pending ? fe->blocks : mon->first[(size_t)rx];
	if (T == 0) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	// the collection stream waits for the newest monitor launch (its event rode on the dispatch) and copies beside the kernels in flight
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
	if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? HFDL_GPU_ENOMEM : HFDL_GPU_EHIP, "spectrum history buffers: %s", hipGetErrorString(e));
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
	if (rx < 0 || rx >= fe->nrx) return fail(HFDL_GPU_EINVAL, "receiver %d out of range (%d receivers)", rx, fe->nrx);
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

// ---------------------------------------------------------------- impulse-noise blanker

extern "C" int hfdl_gpu_frontend_blanker_enable(hfdl_gpu_frontend *fe, float threshold_db)
{
	if (!(threshold_db == 0.f || (threshold_db >= BLANK_DB_MIN && threshold_db <= BLANK_DB_MAX))) return fail(HFDL_GPU_EINVAL, "blanker threshold %g dB", (double)threshold_db);
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	if (!fe->blank) {
		if (threshold_db == 0.f) return 0;
		HIP_TRY(hipSetDevice(fe->device));
		const size_t K = (size_t)fe->nrx, n = (size_t)fe->geo.input_size;
		auto b = std::make_unique<Blanker>();
		hipError_t e = b->scratch.alloc(sizeof(float2) * K * n);
		if (e == hipSuccess) e = b->partial.alloc(sizeof(float) * K * (size_t)blank_chunks((int)n));
		if (e == hipSuccess) e = b->rec.zeroed(sizeof(BlankRecord) * K);
		if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // the clearing runs on the null stream, which the front end's streams do not follow
		if (e == hipSuccess) e = b->host.alloc(1);
		if (e == hipSuccess) e = b->ev.create(EV_NO_TIMING);
		if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? HFDL_GPU_ENOMEM : HFDL_GPU_EHIP, "blanker buffers: %s", hipGetErrorString(e));
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
	if (rx < 0 || rx >= fe->nrx) return fail(HFDL_GPU_EINVAL, "receiver %d out of range (%d receivers)", rx, fe->nrx);
	memset(out, 0, sizeof(*out));
	if (b->blocks == 0) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	// the collection stream waits for the newest blanker launch (its event rode on the dispatch) and copies beside the kernels in flight
	hipStream_t st = fe->demod.st_collect;
	hipError_t e = hipStreamWaitEvent(st, b->ev, 0);
	if (e == hipSuccess) e = hipMemcpyAsync(b->host.p, b->rec.as<BlankRecord>() + rx, sizeof(BlankRecord), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	HIP_TRY(e);
	out->blocks = b->blocks;
	out->samples_blanked = b->host.p->blanked;
	out->last_power = b->host.p->power;
	out->last_threshold = b->host.p->threshold;
	return 0;
}

// ---------------------------------------------------------------- I/Q imbalance and DC corrector

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
		const size_t K = (size_t)fe->nrx, n = (size_t)fe->geo.input_size;
		auto q = std::make_unique<Iqbal>();
		q->alpha.assign(K, 0.f);
		hipError_t e = q->scratch.alloc(sizeof(float2) * K * n);
		if (e == hipSuccess) e = q->partial.alloc(sizeof(float) * 2 * K * 5 * (size_t)blank_chunks((int)n));
		if (e == hipSuccess) e = q->state.zeroed(sizeof(IqbalState) * 2 * K);
		if (e == hipSuccess) e = q->seed.zeroed(sizeof(IqbalSeed) * K);
		if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // the clearing runs on the null stream, which the front end's streams do not follow
		if (e == hipSuccess) e = q->host.alloc(1);
		if (e == hipSuccess) e = q->ev.create(EV_NO_TIMING);
		if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? HFDL_GPU_ENOMEM : HFDL_GPU_EHIP, "I/Q corrector buffers: %s", hipGetErrorString(e));
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
	if (rx < 0 || rx >= fe->nrx) return fail(HFDL_GPU_EINVAL, "receiver %d out of range (%d receivers)", rx, fe->nrx);
	memset(out, 0, sizeof(*out));
	if (q->step == 0) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	// the collection stream waits for the newest corrector launch (its event rode on the dispatch) and copies beside the kernels in flight
	hipStream_t st = fe->demod.st_collect;
	hipError_t e = hipStreamWaitEvent(st, q->ev, 0);
	if (e == hipSuccess) e = hipMemcpyAsync(q->host.p, q->state.as<IqbalState>() + ((q->step - 1) & 1) * (size_t)fe->nrx + (size_t)rx, sizeof(IqbalState), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	HIP_TRY(e);
	iqbal_stats_of(*q->host.p, out);
	return 0;
}

// ---------------------------------------------------------------- carrier canceller (its switch is the pipeline's: hfdl_gpu.cpp)

static_assert(HFDL_GPU_NOTCH_STATE_FLOATS == NOTCH_STATE_FLOATS, "include/hfdl_gpu.h and notch.h name the same state");

extern "C" int hfdl_gpu_frontend_notch_stats(hfdl_gpu_frontend *fe, int32_t channel, hfdl_gpu_notch_stats *out)
{
	if (!fe || !out) return fail(HFDL_GPU_EINVAL, "null argument");
	Notch *n = fe->notch.get();
	if (!n) return fail(HFDL_GPU_EINVAL, "the canceller was never enabled");
	if (channel < 0 || channel >= fe->geo.nch || !n->selected[(size_t)channel]) return fail(HFDL_GPU_EINVAL, "channel %d is out of range or not selected", channel);
	memset(out, 0, sizeof(*out));
	if (!n->launched) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	// the collection stream waits for the newest canceller launch (its event rode on the dispatch) and copies beside the kernels in flight
	hipStream_t st = fe->demod.st_collect;
	hipError_t e = hipStreamWaitEvent(st, n->ev, 0);
	if (e == hipSuccess) e = hipMemcpyAsync(n->host.p, n->rec.as<NotchRecord>() + channel, sizeof(NotchRecord), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	HIP_TRY(e);
	out->blocks = n->host.p->blocks;
	out->resets = n->host.p->resets;
	out->last_in_power = n->host.p->in_power;
	out->last_out_power = n->host.p->out_power;
	out->tap_energy = n->host.p->tap_energy;
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
		bool ok = nsel <= fe->geo.nch && (format == HFDL_GPU_EXPORT_CF32 || format == HFDL_GPU_EXPORT_CS16) && ring_blocks >= 2 && ring_blocks <= HFDL_GPU_EXPORT_RING_MAX
			&& (format == HFDL_GPU_EXPORT_CF32 || (scale > 0.f && scale <= 3.402823466e38f));
		std::vector<bool> seen((size_t)fe->geo.nch);
		for (size_t i = 0; ok && i < S; i++) {
			ok = channels[i] >= 0 && channels[i] < fe->geo.nch && !seen[(size_t)channels[i]];
			if (ok) seen[(size_t)channels[i]] = true;
		}
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
		if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? HFDL_GPU_ENOMEM : HFDL_GPU_EHIP, "export buffers: %s", hipGetErrorString(e));
		x->nsel = nsel; x->format = format; x->scale = scale;
		x->last_of.resize(R);
		x->ring.start((uint32_t)ring_blocks, fe->blocks);      // a block waiting in the half being filled is older: the hook leaves it out
	}
	// the old ring goes once nothing queued writes into it any more: wait for the export launches queued so far, nothing else
	if (fe->exp && fe->exp->newest) (void)hipEventSynchronize(fe->exp->newest);
	fe->exp = std::move(x);
	return 0;
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
