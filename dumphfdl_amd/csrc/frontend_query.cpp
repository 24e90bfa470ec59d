// frontend_query.cpp -- what a caller reads from a front end: the error text, geometry, input-done queries, timers, statistics, stage
// taps, counters; and the page-locked allocator.  (What the opt-in stages report is read beside their switches: frontend_options.cpp.)
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
