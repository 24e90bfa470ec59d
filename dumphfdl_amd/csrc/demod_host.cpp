// demod_host.cpp -- Demod: the host-side owner of the per-channel demodulator / burst decoder state (K4 + K5) of a front end -- its
// device memory, the launches of a closed half and what orders them (planner.h DemodOrder has the rule), the PDU ring's host logic,
// the statistics read-back.  The kernels and their launchers are demod_kernels.hip's (demod_launch.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "demod.h"
#include "demod_launch.h"
#include "demod_lds.h"
#include "demod_tables.h"
#include "planner.h"
#include "quality.h"

namespace hfdl {

struct DemodImage { DemodTables h; DevTables t; };

Demod::Demod() = default;
Demod::~Demod() = default;

static DevTables resolve_tables(const void *d_img, const DemodTables &h)
{
	const unsigned char *base = (const unsigned char *)d_img;
	auto at = [&](const void *field) { return base + ((const unsigned char *)field - (const unsigned char *)&h); };
	DevTables t;
	t.c.rs_h = (const float *)at(h.rs_h);
	t.c.rs_step = h.rs_step;
	t.c.mf = (const float *)at(h.mf);
	t.c.ss_mf = (const float *)at(h.ss_mf);
	t.c.ss_dmf = (const float *)at(h.ss_dmf);
	t.c.lf_b0 = h.lf_b0; t.c.lf_a1 = h.lf_a1; t.c.ss_rate_adj = h.ss_rate_adj;
	t.c.eq_h0 = (const float *)at(h.eq_h0);
	t.c.a_hi = h.a_hi; t.c.a_lo = h.a_lo;
	t.c.m1_hi = (const uint64_t *)at(h.m1_hi);
	t.c.m1_lo = (const uint64_t *)at(h.m1_lo);
	t.scrambler = (const uint8_t *)at(h.scrambler);
	t.c.corr_tab = (const float *)at(h.corr_tab);
	t.c.psk_pts = (const float *)at(h.psk_pts);
	t.c.a1_lo = h.a1_lo; t.c.a1_hi = h.a1_hi; t.c.a2_lo = h.a2_lo; t.c.a2_hi = h.a2_hi; t.c.pos_min = h.pos_min;
	return t;
}

size_t Demod::workgroup_lds() { return demod_workgroup_lds(0); }

static_assert(DM_MAX_BLOCKS == PLAN_MAX_HALF, "a half that closes full is one demodulator launch");

// blocks a launch can take at most, `want` or fewer: what the kernel's block table holds, a workgroup's LDS (no bound for the product,
// whose per-sample arrays are rings, demod_lds.h; the test-only strict build keeps whole-launch arrays) and output counts that fit 16
// bits (cum[] in LDS: cfg3's 32 blocks make 2 x 31 734).  The frames a channel can finish in the launch are no bound: init() sizes the
// frame queue and the data slots from the launch's signal time.
int Demod::fit_batch(int outs, float resamp_rate, int want)
{
	int batch = fit_output_counts(outs, resamp_rate, want);
	while (batch > 1 && demod_workgroup_lds(demod_launch_samples(outs, batch, resamp_rate)) > 160 * 1024) batch--;
	return batch;
}

int Demod::init(int nch_, int outs_, float resamp_rate, const int32_t *freqs, hipStream_t st, int batch_want)
{
	nch = nch_; outs = outs_;
	if (resamp_rate <= 0.5f || resamp_rate > 1.0f) return fail(HFDL_GPU_ERANGE, "resampling rate %g outside (0.5, 1]", (double)resamp_rate);   // one arbitrary stage, no half-band stages
	// blocks per launch
	batch = fit_batch(outs, resamp_rate, batch_want);
	cap = demod_launch_samples(outs, batch, resamp_rate);
	// a launch covers at most cap samples at 5400 sps: frame records per channel and set, data slots per channel
	const FrameSlots fs = plan_frame_slots((double)cap / 5400.0);
	frames_per_chan = fs.per_channel; data_slots = fs.data_slots;
	img = std::make_unique<DemodImage>();
	build_demod_tables(img->h, resamp_rate);
	CREATE_TRY(d_tables.alloc(sizeof(DemodTables)));
	CREATE_TRY(hipMemcpyAsync(d_tables.p, &img->h, sizeof(DemodTables), hipMemcpyHostToDevice, st));
	img->t = resolve_tables(d_tables.p, img->h);

	std::vector<ChanState> init((size_t)nch);
	for (auto &s : init) chan_state_init(s, img->h.eq_h0);
	CREATE_TRY(d_states.alloc((size_t)nch));
	CREATE_TRY(hipMemcpy(d_states, init.data(), sizeof(ChanState) * (size_t)nch, hipMemcpyHostToDevice));
	CREATE_TRY(d_data.alloc((size_t)nch * data_slots * MAX_DATA_SYMBOLS));
	CREATE_TRY(hipMemsetAsync(d_data, 0, sizeof(float2) * (size_t)nch * data_slots * MAX_DATA_SYMBOLS, st));
	CREATE_TRY(d_frames.alloc(2 * (size_t)nch * frames_per_chan));
	CREATE_TRY(d_counts.alloc(8));
	CREATE_TRY(hipMemsetAsync(d_counts, 0, sizeof(int) * 8, st));
	CREATE_TRY(h_snap.alloc(8));
	std::memset(h_snap.p, 0, sizeof(int) * 8);
	taken = 0; dropped = 0;
	pdu_cap = std::max(4096, 64 * nch);       // ~1 KiB each; polled by the host at least once per few seconds of signal
	if (const char *e = getenv("HFDL_GPU_PDU_RING")) {       // test / tuning knob (include/hfdl_gpu.h)
		const long v = strtol(e, nullptr, 10);
		if (v >= 1 && v <= (1 << 20)) pdu_cap = (int)v;
	}
	CREATE_TRY(d_pdus.alloc((size_t)pdu_cap));
	CREATE_TRY(st_collect.create());
	bounce_cap = pdu_cap < 512 ? pdu_cap : 512;
	CREATE_TRY(h_pdu_bounce.alloc((size_t)bounce_cap));
	CREATE_TRY(h_stats_bounce.alloc((size_t)nch));
	CREATE_TRY(d_freqs.alloc((size_t)nch));
	CREATE_TRY(hipMemcpyAsync(d_freqs, freqs, sizeof(int32_t) * (size_t)nch, hipMemcpyHostToDevice, st));
	for (Event &e : ev_demod) CREATE_TRY(e.create(EV_NO_TIMING));
	for (auto &half : dm) for (DoneEvent &d : half) CREATE_TRY(d.own.create(EV_NO_TIMING));
	if (taps_on) {
		CREATE_TRY(d_tap_rs.alloc((size_t)nch * cap));
		CREATE_TRY(d_tap_mf.alloc((size_t)nch * cap));
		CREATE_TRY(d_tap_sym.alloc((size_t)nch * cap));
		CREATE_TRY(d_tap_lvl.alloc((size_t)nch * cap));
		CREATE_TRY(d_tap_counts.alloc(2 * (size_t)nch));
		CREATE_TRY(hipMemsetAsync(d_tap_counts, 0, sizeof(int) * 2 * (size_t)nch, st));
	}
	lds_bytes = demod_workgroup_lds(cap);
	if (lds_bytes > 160 * 1024) return fail(HFDL_GPU_ERANGE, "a demodulator launch of %d samples needs %zu bytes of LDS", cap, lds_bytes);
	return prepare_demod_kernels(lds_bytes);
}

// A half of `nblk` blocks is demodulated `batch` blocks per launch, each launch followed by its burst decoder.  One launch index serves
// both kernels of a launch: planner.h DemodOrder says which frame queue and counters they share, what the demodulator waits for and
// which of the half's done events it carries.
int Demod::launch_half(const float2 *chan_out, const int *out_count, int nblk, int half, hipEvent_t ready, hipStream_t st_b, hipStream_t st_d, LaunchTimers &timers)
{
	if (!img || nblk < 1 || batch > DM_MAX_BLOCKS)       // (the kernel's block table holds DM_MAX_BLOCKS)
		return fail(HFDL_GPU_EINVAL, "demodulator launches of %d blocks, up to %d each, before init or past the block table", nblk, batch);
	if (ready) HIP_TRY(hipStreamWaitEvent(st_b, ready, 0));
	const int k = (nblk + batch - 1) / batch;
	for (int j0 = 0, l = 0; j0 < nblk; j0 += batch, l++) {
		const int take = std::min(batch, nblk - j0);
		const DemodLaunch p = order.launch(l, k);
		// the done event rides on the kernel's dispatch; with the decoder on its own stream the channelizer may have waited for the frame
		// queue already (frames_free_event), so on the demodulator-bound geometries ONE barrier packet separates consecutive demodulators
		DoneEvent &done = dm[half][p.done_event];
		hipEvent_t t_start = nullptr;
		if (int rc = timers.arm(ST_DEMOD, take, done, t_start)) return rc;
		if (int rc = enqueue_demod(p, chan_out + (size_t)j0 * nch * outs, out_count + (size_t)j0 * nch, take, st_b, done.event(), t_start)) return rc;
		if (order.own_decode) HIP_TRY(hipStreamWaitEvent(st_d, done.event(), 0));
		hipEvent_t k5_start = nullptr, k5_stop = nullptr;
		if (int rc = timers.arm(ST_DECODE, take, k5_start, k5_stop)) return rc;
		if (int rc = enqueue_decode(p, half, st_d, k5_start, k5_stop)) return rc;
	}
	HIP_TRY(hipEventRecord(ev_demod[order.decoded_event(0)], st_d));      // (launches follow their hand-over: this half is the newest)
	halves_launched = order.halves;
	return 0;
}

int Demod::enqueue_demod(const DemodLaunch &p, const float2 *chan_out, const int *out_count, int nblk, hipStream_t st, hipEvent_t done, hipEvent_t start)
{
	DemodBuffers B;
	// the decoder of two launches ago has read this frame queue.  Every wait or record is a barrier packet of its own in the queue
	// (~5 us of idle stream each): on the demodulator-bound geometries the front end moves this one to the channelizer's stream
	if (p.wait_decoder) HIP_TRY(hipStreamWaitEvent(st, ev_dec[p.set], 0));
	B.states = d_states; B.data = (cf *)d_data.p; B.data_slots = data_slots; B.frames = d_frames + (size_t)p.set * nch * frames_per_chan; B.counts = d_counts;
	B.frame_count = d_counts + 4 + p.counter; B.frame_cap = nch * frames_per_chan;
	const bool tw = taps_on && taps_enabled;
	B.tap_rs = tw ? (cf *)d_tap_rs.p : nullptr; B.tap_mf = (cf *)d_tap_mf.p; B.tap_sym = (cf *)d_tap_sym.p; B.tap_lvl = d_tap_lvl; B.tap_counts = d_tap_counts;
	B.cap = cap;
	launch_demod(tw, img->t, B, (const cf *)chan_out, out_count, outs, nblk, nch, lds_bytes, st, start, done);
	HIP_TRY(hipGetLastError());
	return 0;
}

int Demod::enqueue_decode(const DemodLaunch &p, int half, hipStream_t st, hipEvent_t start, hipEvent_t stop)
{
	launch_burst_decode(d_frames + (size_t)p.set * nch * frames_per_chan, d_counts, d_counts + 4 + p.counter, d_counts + 4 + p.zeroed, nch * frames_per_chan,
			(const cf *)d_data.p, data_slots, img->t.scrambler, d_freqs, d_pdus, pdu_cap, st, start, stop);
	// the frame quality records of the same frame queue: part of "the decoder of launch i" for DemodOrder's hazards 1 and 4 -- behind
	// the burst decoder, in front of ev_dec and of the half's decoded event, so the queue, its counter and the data slots are guarded
	// for it exactly as for the decoder's own reads; its ring's counts ride behind it as the PDU ring's do
	if (FrameQuality *q = quality.get()) {
		launch_frame_quality(d_frames + (size_t)p.set * nch * frames_per_chan, d_counts + 4 + p.counter, nch * frames_per_chan, (const cf *)d_data.p, data_slots,
				img->t.c.psk_pts, d_freqs, q->d_counts, q->d_recs, (cf *)q->d_syms.p, q->ring, st);
		HIP_TRY(hipMemcpyAsync(q->h_snap.p + 4 * half, q->d_counts, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipEventRecord(q->ev_last, st));
		q->launched = true;
	}
	// what the ring holds once this launch is done, for a host that collects without draining the pipeline
	HIP_TRY(hipMemcpyAsync(h_snap.p + 4 * half, d_counts, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
	if (order.own_decode) {
		if (!ev_dec[p.set]) HIP_TRY(ev_dec[p.set].create(EV_NO_TIMING));
		HIP_TRY(hipEventRecord(ev_dec[p.set], st));
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

int Demod::prepare_retune(hipStream_t st_b)
{
	if (d_state_image.p) return 0;
	DevArray<ChanState> d;
	PinnedBuf<ChanState> h;
	Event ev;
	CREATE_TRY(d.alloc(1));
	CREATE_TRY(h.alloc(1));
	CREATE_TRY(ev.create(EV_NO_TIMING));
	chan_state_init(*h.p, img->h.eq_h0);
	HIP_TRY(hipMemcpyAsync(d.p, h.p, sizeof(ChanState), hipMemcpyHostToDevice, st_b));
	std::swap(d_state_image.p, d.p);
	std::swap(h_state_image.p, h.p);
	ev_retuned = std::move(ev);
	return 0;
}

void Demod::enqueue_retune(int c, int32_t freq, hipStream_t st_b, hipStream_t st_d)
{
	launch_retune_demod(d_states, d_state_image, c, st_b, ev_retuned);
	launch_retune_freq(d_freqs, c, freq, st_d);
	retuned.push_back(c);
}

// copy ring entries [taken, produced) to the host, at most `max`; every entry below `produced` is complete.
// `produced` may be an OLDER snapshot than `taken` (a draining poll followed by a snapshot poll with no push in between):
// the difference is taken as signed, so a stale snapshot yields nothing instead of wrapping.
int Demod::take(unsigned produced, hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st)
{
	*n = 0;
	const int32_t avail = (int32_t)(produced - taken);
	if (avail <= 0 || max <= 0) return 0;
	if (!out) return fail(HFDL_GPU_EINVAL, "null PDU buffer");              // a NULL buffer never discards PDUs
	unsigned have = (unsigned)avail;
	if (have > (unsigned)pdu_cap) have = (unsigned)pdu_cap;
	const unsigned cnt = have < (unsigned)max ? have : (unsigned)max;
	// ring entries [taken, taken + cnt) in pieces that neither wrap nor exceed the bounce buffer; each piece is copied on the
	// collection stream (beside whatever kernels are running) and waited for on that stream alone
	for (unsigned done = 0; done < cnt;) {
		const unsigned first = (taken + done) % (unsigned)pdu_cap;
		unsigned n1 = cnt - done;
		if (n1 > (unsigned)pdu_cap - first) n1 = (unsigned)pdu_cap - first;
		if (n1 > (unsigned)bounce_cap) n1 = (unsigned)bounce_cap;
		HIP_TRY(hipMemcpyAsync(h_pdu_bounce.p, d_pdus + first, sizeof(hfdl_gpu_pdu) * n1, hipMemcpyDeviceToHost, st_collect));
		HIP_TRY(hipStreamSynchronize(st_collect));
		std::memcpy(out + done, h_pdu_bounce.p, sizeof(hfdl_gpu_pdu) * n1);
		done += n1;
	}
	taken += cnt;
	HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(d_counts + 3), (int)taken, 1, st));    // ordered after the blocks already queued
	*n = (int32_t)cnt;
	return 0;
}

int Demod::collect(hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st)
{
	int counts[4];
	HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	dropped = (uint32_t)counts[2];
	return take((unsigned)counts[1], out, max, n, st);
}

// Leave the newest half running: wait for the last DEMODULATOR of the half before it -- that is the flow control: the caller may
// queue the next blocks, the demodulator stream will not run dry -- and take what the PDU ring is known to hold: the snapshot
// written after that half's last burst decoder if it has finished too, else the one written a half earlier (a stale snapshot
// yields nothing new; those PDUs come with the next call).  Waiting for the burst decoder here (0.3 ms when a long frame ended)
// left the demodulator idle for as long on the demodulator-bound geometries (profiles/r03_experiments.md).
int Demod::collect_ready(bool wait, hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st)
{
	const int half = order.poll_half();
	if (half < 0) return 0;                             // fewer than two halves: nothing is known to be done
	const hipEvent_t ev = dm[half][0].event();          // the last demodulator launch of that half
	if (!wait) {
		// no waiting at all: a caller whose flow control is elsewhere (the C host: the page-locked ring slots it leases to the
		// uploads) only takes what is complete, and comes back
		const hipError_t q = hipEventQuery(ev);
		if (q == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
		if (q != hipSuccess) return fail(HFDL_GPU_EHIP, "hipEventQuery: %s", hipGetErrorString(q));
	} else {
		HIP_TRY(hipEventSynchronize(ev));
	}
	const bool newer = decoded(1);
	const int slot = order.snapshot_slot(newer, !newer && decoded(2));
	return slot < 0 ? 0 : collect_snapshot(slot, out, max, n, st);
}

// A snapshot slot is written by its half's burst decoders' 16-byte copies: read only once the last of them is known to be done
// (ev_demod is recorded behind it).  "Not ready" is an answer, not an error to be found by a later check.
bool Demod::decoded(int back)
{
	const int e = order.decoded_event(back);
	const bool yes = e >= 0 && hipEventQuery(ev_demod[e]) == hipSuccess;
	if (!yes) (void)hipGetLastError();
	return yes;
}

int Demod::collect_snapshot(int slot, hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st)
{
	const volatile int *snap = h_snap.p + 4 * slot;
	const uint32_t d = (uint32_t)snap[2];
	if ((int32_t)(d - dropped) > 0) dropped = d;       // monotone: an older snapshot never takes the count back
	return take((unsigned)snap[1], out, max, n, st);
}

// ---------------------------------------------------------------- frame quality records

int Demod::quality_enable(int ring, bool symbols)
{
	std::unique_ptr<FrameQuality> q;
	if (ring > 0) {
		q = std::make_unique<FrameQuality>();
		const size_t chunk = (size_t)std::min(ring, FrameQuality::CHUNK);
		CREATE_TRY(q->d_recs.alloc((size_t)ring));
		if (symbols) CREATE_TRY(q->d_syms.alloc((size_t)ring * MAX_DATA_SYMBOLS));
		CREATE_TRY(q->d_counts.alloc(4));
		CREATE_TRY(q->h_snap.alloc(8));
		CREATE_TRY(q->h_recs.alloc(chunk));
		if (symbols) CREATE_TRY(q->h_syms.alloc(chunk * MAX_DATA_SYMBOLS));
		CREATE_TRY(q->ev_last.create(EV_NO_TIMING));
		CREATE_TRY(hipMemsetAsync(q->d_counts, 0, sizeof(int) * 4, st_collect));
		CREATE_TRY(hipStreamSynchronize(st_collect));
		std::memset(q->h_snap.p, 0, sizeof(int) * 8);
		q->ring = ring;
	}
	// the old ring goes once nothing queued writes into it any more: wait for the quality launches queued so far, nothing else
	if (quality && quality->launched) (void)hipEventSynchronize(quality->ev_last);
	quality = std::move(q);
	return 0;
}

int Demod::quality_read(hfdl_gpu_frame_quality *out, float *symbols, int32_t max, int32_t *n, uint32_t *dropped_out, hipStream_t st)
{
	FrameQuality &q = *quality;
	*n = 0;
	// Which snapshot may be believed: the newest half's own if its last decoder has been queued and is found done (after a sync, a
	// draining poll: everything); else what a poll that leaves the pipeline running reads (DemodOrder::snapshot_slot).  A slot no
	// quality launch has written holds zeros.
	int slot;
	if (order.newest >= 0 && halves_launched == order.halves && decoded(0)) slot = order.newest;
	else {
		const bool newer = decoded(1);
		slot = order.snapshot_slot(newer, !newer && decoded(2));
	}
	if (slot >= 0) {
		const volatile int *snap = q.h_snap.p + 4 * slot;
		const uint32_t d = (uint32_t)snap[2];
		if ((int32_t)(d - q.dropped) > 0) q.dropped = d;      // monotone: an older snapshot never takes the count back
		const int32_t avail = (int32_t)((unsigned)snap[1] - q.taken);      // signed: a stale snapshot yields nothing
		const unsigned cnt = avail <= 0 || max <= 0 ? 0u : (unsigned)std::min(std::min(avail, q.ring), max);
		// ring entries [taken, taken + cnt) in pieces that neither wrap nor exceed the bounce buffers, copied on the collection stream
		// beside whatever kernels are running
		for (unsigned done = 0; done < cnt;) {
			const unsigned first = (q.taken + done) % (unsigned)q.ring;
			const unsigned n1 = std::min(std::min(cnt - done, (unsigned)q.ring - first), (unsigned)FrameQuality::CHUNK);
			HIP_TRY(hipMemcpyAsync(q.h_recs.p, q.d_recs + first, sizeof(hfdl_gpu_frame_quality) * n1, hipMemcpyDeviceToHost, st_collect));
			if (symbols) HIP_TRY(hipMemcpyAsync(q.h_syms.p, q.d_syms + (size_t)first * MAX_DATA_SYMBOLS, sizeof(float2) * MAX_DATA_SYMBOLS * n1, hipMemcpyDeviceToHost, st_collect));
			HIP_TRY(hipStreamSynchronize(st_collect));
			std::memcpy(out + done, q.h_recs.p, sizeof(hfdl_gpu_frame_quality) * n1);
			if (symbols) std::memcpy(symbols + (size_t)done * 2 * MAX_DATA_SYMBOLS, q.h_syms.p, sizeof(float2) * MAX_DATA_SYMBOLS * n1);
			done += n1;
		}
		if (cnt) {
			q.taken += cnt;
			HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(q.d_counts + 3), (int)q.taken, 1, st));    // ordered after the launches already queued
		}
		*n = (int32_t)cnt;
	}
	if (dropped_out) *dropped_out = q.dropped;
	return 0;
}

int Demod::tap(int what, int channel, const void **src, size_t *nfloats)
{
	if (!taps_on || !taps_enabled) return fail(HFDL_GPU_EINVAL, "the stage taps are off");
	int counts[2];
	HIP_TRY(hipMemcpy(counts, d_tap_counts + 2 * channel, sizeof(counts), hipMemcpyDeviceToHost));
	switch (what) {
	case HFDL_GPU_TAP_RESAMPLED: *src = d_tap_rs + (size_t)channel * cap; *nfloats = 2 * (size_t)counts[0]; return 0;
	case HFDL_GPU_TAP_MF_OUT: *src = d_tap_mf + (size_t)channel * cap; *nfloats = 2 * (size_t)counts[0]; return 0;
	case HFDL_GPU_TAP_SYMBOLS: *src = d_tap_sym + (size_t)channel * cap; *nfloats = 2 * (size_t)counts[1]; return 0;
	case HFDL_GPU_TAP_AGC_LEVEL: *src = d_tap_lvl + (size_t)channel * cap; *nfloats = (size_t)counts[0]; return 0;
	default: return fail(HFDL_GPU_EINVAL, "unknown tap %d", what);
	}
}

static void fill_stats(const ChanScalars &sc, hfdl_gpu_channel_stats *out)
{
	out->a2_found = sc.cnt_a2_found; out->m1_found = sc.cnt_m1_found; out->m1_not_found = sc.cnt_m1_not_found; out->frames = sc.cnt_frames;
	out->noise_floor_db = 20.0f * log10f(sc.noise_floor);
	out->agc_level = 1.0f / sc.agc_g;
	out->costas_dphi = sc.dphi;
	out->framer_state = sc.fr_state;
	out->sample_cnt = sc.sample_cnt; out->symbol_cnt = sc.symbol_cnt;
	out->a1_found = sc.cnt_a1_found;
	out->a1_corr_avg = sc.cnt_a1_found ? (float)sc.sum_a1_dev / 127.0f / (float)sc.cnt_a1_found : 0.f;
	out->a2_corr_avg = sc.cnt_a2_found ? (float)sc.sum_a2_dev / 127.0f / (float)sc.cnt_a2_found : 0.f;
	out->m1_corr_avg = sc.cnt_m1_found ? (float)sc.sum_m1_dev / 127.0f / (float)sc.cnt_m1_found : 0.f;
	out->train_bits_bad = sc.cum_train_bad; out->train_bits_total = sc.cum_train_total;
}

int Demod::stats(int channel, hfdl_gpu_channel_stats *out)
{
	ChanScalars sc;
	HIP_TRY(hipMemcpy(&sc, &d_states[channel].s, sizeof(sc), hipMemcpyDeviceToHost));
	fill_stats(sc, out);
	return 0;
}

// all channels in one strided copy; does not wait for blocks in flight (each field is read whole, the set may straddle a block)
int Demod::stats_all(hfdl_gpu_channel_stats *out, int n)
{
	if (n > nch) return fail(HFDL_GPU_EINVAL, "statistics of %d channels asked for, %d exist", n, nch);
	ChanScalars *sc = h_stats_bounce.p;
	// asked BEFORE the copy: if the newest state reset has run, the copy sees every reset
	if (!retuned.empty() && hipEventQuery(ev_retuned) == hipSuccess) retuned.clear();
	(void)hipGetLastError();              // "not ready" is an answer
	HIP_TRY(hipMemcpy2DAsync(sc, sizeof(ChanScalars), &d_states[0].s, sizeof(ChanState), sizeof(ChanScalars), (size_t)n, hipMemcpyDeviceToHost, st_collect));
	HIP_TRY(hipStreamSynchronize(st_collect));
	// a channel whose reset is still queued is a fresh channel already: the image's scalars, the stream position it has reached
	for (int c : retuned)
		if (c < n) { const uint64_t at = sc[c].sample_cnt; sc[c] = h_state_image.p->s; sc[c].sample_cnt = at; }
	for (int i = 0; i < n; i++) fill_stats(sc[i], out + i);
	return 0;
}

// the DemodTables image resident on the device and the device's own evaluation of hfdl_constants()
int Demod::read_constants(void *tables, size_t tables_bytes, void *constants, size_t constants_bytes)
{
	if (tables_bytes != sizeof(DemodTables) || constants_bytes != sizeof(HfdlConstants) || !d_tables.p)
		return fail(HFDL_GPU_EINVAL, "constants read-back: sizes %zu / %zu, this build's are %zu / %zu", tables_bytes, constants_bytes, sizeof(DemodTables), sizeof(HfdlConstants));
	if (int rc = read_device_constants(constants)) return rc;
	HIP_TRY(hipMemcpy(tables, d_tables.p, sizeof(DemodTables), hipMemcpyDeviceToHost));
	return 0;
}

}  // namespace hfdl
