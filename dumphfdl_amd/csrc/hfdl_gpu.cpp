// hfdl_gpu.cpp -- C-ABI shim of libhfdl_gpu.so, the pipeline: input staging, the forward FFT of a pushed block, the fold / inverse FFT
// of a closed half, the demodulator launches, retune, sync and poll.  The opt-in stages (input chain, spectrum monitor, carrier canceller,
// channel export) are frontend_options.cpp's: the pipeline calls each through one hook.  (frontend.h names the other translation units of the shim.)
// The only C++ a C host ever sees is through include/hfdl_gpu.h (extern "C", plain pointers).
#include "frontend.h"

using namespace hfdl;

// ---------------------------------------------------------------- launch timing

int LaunchTimers::arm(Stage s, int blocks, hipEvent_t &start, hipEvent_t &stop)
{
	if (!on) return 0;
	Timed t;
	if (!pool.empty()) {
		t = std::move(pool.back());
		pool.pop_back();
	} else {
		HIP_TRY(t.start.create(EV_TIMING));
		HIP_TRY(t.stop.create(EV_TIMING));
	}
	t.blocks = blocks;
	start = t.start;
	stop = t.stop;
	stage[s].pending.push_back(std::move(t));
	return 0;
}

int LaunchTimers::drain()
{
	for (int s = 0; s < ST_N; s++) {
		for (Timed &t : stage[s].pending) {
			float ms = 0;
			HIP_TRY(hipEventElapsedTime(&ms, t.start, t.stop));
			stage[s].ms += ms;
			stage[s].launches++;
			stage[s].blocks += t.blocks;
			if (s == ST_FOLD) {
				fold_last_blocks = t.blocks;
				if (t.blocks >= 1 && t.blocks <= FOLD_MAX_BLOCKS) { fold_shapes[t.blocks]++; fold_shape_ms[t.blocks] += ms; }
				if (!first_fold) {
					first_fold = std::move(t.start);           // kept until the next reset
					HIP_TRY(t.start.create(EV_TIMING));
				} else {
					HIP_TRY(hipEventElapsedTime(&ms, first_fold, t.start));
					span_ms = ms;
				}
			}
			pool.push_back(std::move(t));
		}
		stage[s].pending.clear();
	}
	return 0;
}

int LaunchTimers::reset(bool enable)
{
	on = enable;
	for (Totals &t : stage) { t.ms = 0; t.launches = 0; t.blocks = 0; }
	for (auto &c : fold_shapes) c = 0;
	for (auto &c : fold_shape_ms) c = 0;
	first_fold = Event();
	span_ms = 0;
	fold_last_blocks = 0;
	while (enable && pool.size() < 1280) {
		Timed t;
		HIP_TRY(t.start.create(EV_TIMING));
		HIP_TRY(t.stop.create(EV_TIMING));
		pool.push_back(std::move(t));
	}
	return 0;
}

int hfdl_gpu_frontend::settle_events()
{
	if (int rc = timers.drain()) return rc;
	// everything is complete: the pooled events may be reused
	demod.settle();
	for (DoneEvent *d : { &chan[0], &chan[1], &fft_done, &spec[0], &spec[1] }) d->settle();
	return 0;
}

// ---------------------------------------------------------------- input staging

extern "C" void *hfdl_gpu_frontend_stream(hfdl_gpu_frontend *fe) { return fe ? (void *)fe->fft_stream(fe->side_of(true)) : nullptr; }      // the stream that reads device input

// a block of input: a known sample format, exactly input_size samples.  A real front end takes the real formats alone, 2 input_size
// samples a block, and from here on they are what they are to the forward FFT's loads: input_size pairs of the complex format of that
// width (real_input.h)
static int check_block(const hfdl_gpu_frontend *fe, size_t &nsamples, int &fmt)
{
	const bool real_fmt = fmt == HFDL_GPU_SFMT_RS16 || fmt == HFDL_GPU_SFMT_RF32;
	if (real_fmt != (fe->real_rate != 0)) return fail(HFDL_GPU_EINVAL, "sample format %d on a front end for %s input", fmt, fe->real_rate ? "real" : "complex");
	if (real_fmt) {
		if (nsamples != 2 * (size_t)fe->plan.input_size)
			return fail(HFDL_GPU_EINVAL, "a block is exactly %d real samples (got %zu)", 2 * fe->plan.input_size, nsamples);
		fmt = fmt == HFDL_GPU_SFMT_RS16 ? SFMT_CS16 : SFMT_CF32;
		nsamples /= 2;
	}
	if (fmt != SFMT_CF32 && fmt != SFMT_CS16 && fmt != SFMT_CU8) return fail(HFDL_GPU_EINVAL, "unknown sample format %d", fmt);
	if (nsamples != (size_t)fe->plan.input_size)
		return fail(HFDL_GPU_EINVAL, "a block is exactly %d samples (got %zu)", fe->plan.input_size, nsamples);
	return 0;
}

// queue the host -> device copy of the next host block -- one block of every receiver, iq[0 .. nrx - 1] -- on stream C into staging
// buffer host_blocks % n_stage (receiver r at r * nsamples samples)
static int queue_input_copy(hfdl_gpu_frontend *fe, const void *const *iq, size_t nsamples, int fmt, int *sb_out)
{
	// buffer j % n_stage is freed by the forward FFT of host block j - n_stage: that block must have been pushed
	if (fe->host_blocks - fe->host_pushed >= (uint64_t)fe->n_stage)
		return fail(HFDL_GPU_ERANGE, "%d uploads are queued ahead of their blocks: push the oldest first", fe->n_stage);
	const uint64_t j = fe->host_blocks;
	const int sb = (int)(j % (uint64_t)fe->n_stage);
	const size_t need = nsamples * (size_t)fe->nrx;
	if (fe->stage_cap[sb] < need) {
		HIP_TRY(hipStreamSynchronize(fe->stream_c));
		HIP_TRY(hipStreamSynchronize(fe->fft_stream(fe->side_of(false))));
		fe->stage_cap[sb] = 0;
		fe->d_stage[sb] = std::make_unique<DevBuf>();
		HIP_TRY(fe->d_stage[sb]->alloc(sizeof(float2) * need));
		fe->stage_cap[sb] = need;
	}
	HIP_TRY(hipStreamWaitEvent(fe->stream_c, fe->ev_stage_free[sb], 0));     // the forward FFT that read this buffer last is past its first pass
	// (one hipMemcpyAsync per block: cutting a block in 2 or 4 pieces on as many streams was measured and is slower, profiles/r03_experiments.md)
	const size_t bytes = sample_bytes(fmt) * nsamples;
	bool pinned = true;
	for (int r = 0; r < fe->nrx; r++) {
		HIP_TRY(hipMemcpyAsync(fe->d_stage[sb]->as<char>() + (size_t)r * bytes, iq[r], bytes, hipMemcpyHostToDevice, fe->stream_c));
		pinned = pinned && is_library_pinned(iq[r], bytes);
	}
	HIP_TRY(hipEventRecord(fe->ev_stage_ready[sb], fe->stream_c));
	fe->host_blocks = j + 1;
	// a buffer this library did not allocate may be reused by the caller as soon as we return (include/hfdl_gpu.h): do not
	// rely on the runtime staging pageable memory synchronously -- wait for the copy (the kernels of the previous block keep running)
	if (!pinned) HIP_TRY(hipEventSynchronize(fe->ev_stage_ready[sb]));
	*sb_out = sb;
	return 0;
}

// Host input is staged in HBM: the copies (stream C) run up to n_stage - 1 blocks ahead of the blocks that compute (stream A).  Device
// input is read where it lies, by a forward FFT on stream C itself (enqueue_fft).
// iq[0 .. nrx - 1]: one block of every receiver; in.fresh[] receives where the forward FFT reads them.
// *stage_idx = staging buffer used (-1 for device input): the forward FFT's first pass signals ev_stage_free when it has read it.
static int stage_input(hfdl_gpu_frontend *fe, const void *const *iq, size_t nsamples, int &fmt, int on_device, FftInputs &in, int *stage_idx)
{
	*stage_idx = -1;
	if (!fe || !iq) return fail(HFDL_GPU_EINVAL, "null argument");
	for (int r = 0; r < fe->nrx; r++) if (!iq[r]) return fail(HFDL_GPU_EINVAL, "null argument: the block of receiver %d", r);
	if (int rc = check_block(fe, nsamples, fmt)) return rc;
	HIP_TRY(hipSetDevice(fe->device));
	const bool queued = fe->host_pushed < fe->host_blocks;      // prefetched blocks are waiting
	if (on_device) {
		// the prefetched host blocks are numbered and staged: a device block slipped in front of them would be processed out of order
		if (queued) return fail(HFDL_GPU_EINVAL, "a prefetched block is pending: push it or call hfdl_gpu_frontend_prefetch_cancel()");
		for (int r = 0; r < fe->nrx; r++) in.fresh[r] = iq[r];
		return 0;
	}
	int sb;
	if (queued) {
		// the copy of this block was queued ahead by hfdl_gpu_frontend_prefetch_block_raw() (one receiver only): blocks are pushed in the order they were prefetched
		sb = (int)(fe->host_pushed % (uint64_t)fe->n_stage);
		if (fe->pf_ptr[sb] != iq[0] || fe->pf_fmt[sb] != fmt) return fail(HFDL_GPU_EINVAL, "the block pushed after a prefetch must be the (oldest) prefetched one");
	} else {
		int rc = queue_input_copy(fe, iq, nsamples, fmt, &sb);
		if (rc) return rc;
	}
	fe->host_pushed++;
	HIP_TRY(hipStreamWaitEvent(fe->fft_stream(fe->side_of(false)), fe->ev_stage_ready[sb], 0));
	for (int r = 0; r < fe->nrx; r++) in.fresh[r] = fe->d_stage[sb]->as<const char>() + (size_t)r * sample_bytes(fmt) * nsamples;
	*stage_idx = sb;
	return 0;
}

// the entry points that take ONE stream's block: a front end of several receivers needs a block of every receiver per step
static int single_receiver_only(const hfdl_gpu_frontend *fe, const char *what)
{
	if (fe && fe->nrx > 1)
		return fail(HFDL_GPU_EINVAL, "%s: this front end has %d receivers -- push a block of every receiver with hfdl_gpu_frontend_push_blocks_raw()", what, fe->nrx);
	return 0;
}

extern "C" int hfdl_gpu_frontend_prefetch_block_raw(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int sample_format)
{
	if (!fe || !raw) return fail(HFDL_GPU_EINVAL, "null argument");
	if (int rc = single_receiver_only(fe, "hfdl_gpu_frontend_prefetch_block_raw")) return rc;
	if (int rc = check_block(fe, nsamples, sample_format)) return rc;
	if (fe->host_blocks - fe->host_pushed >= (uint64_t)(fe->n_stage - 1))
		return fail(HFDL_GPU_ERANGE, "%d blocks are prefetched already (geometry.prefetch_depth): push the oldest first", fe->n_stage - 1);
	if (!is_library_pinned(raw, sample_bytes(sample_format) * nsamples)) return fail(HFDL_GPU_EINVAL, "only buffers from hfdl_gpu_host_alloc() can be prefetched");
	HIP_TRY(hipSetDevice(fe->device));
	int sb = -1;
	const void *one[1] = { raw };
	int rc = queue_input_copy(fe, one, nsamples, sample_format, &sb);
	if (rc) return rc;
	fe->pf_ptr[sb] = raw; fe->pf_fmt[sb] = sample_format;
	return 0;
}

extern "C" int hfdl_gpu_frontend_prefetch_cancel(hfdl_gpu_frontend *fe)
{
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	if (int rc = single_receiver_only(fe, "hfdl_gpu_frontend_prefetch_cancel")) return rc;
	if (fe->host_pushed == fe->host_blocks) return 0;
	HIP_TRY(hipSetDevice(fe->device));
	// the copies are in flight on stream C: let the newest finish (the caller gets its buffers back), then forget the blocks.  They keep
	// their host block numbers -- input_done_upto() of those numbers returns at once.  Their staging buffers are refilled by later
	// copies, which wait for ev_stage_free as last recorded by the blocks that used the buffers BEFORE the cancelled ones: long done.
	HIP_TRY(hipEventSynchronize(fe->input_event(fe->host_blocks - 1)));
	fe->host_pushed = fe->host_blocks;
	return 0;
}

// ---------------------------------------------------------------- the halves

// Where the demodulator's 256 single-wave workgroups land decides how much they disturb the fold kernel they run beside.
// Launched the moment the channelizer of a half is done, they race the next blocks' forward-FFT workgroups for LDS and
// the outcome depends on details as small as the FFT's LDS footprint: measured on MI355X, the same fold kernel took
// 2.56 ms or 2.87 ms per launch (profiles/r01_experiments.md).  So the demodulator launches of a half are held back until the
// forward FFTs of the NEXT half have been queued on stream A: the workgroups then arrive while only the LDS-free fold kernel is resident, spread
// evenly, and the fold time is the good one every time.  A sync / poll launches held-back demodulators at once.
// The launches themselves, their burst decoders and what orders them are Demod::launch_half's.
static int launch_demod(hfdl_gpu_frontend *fe, int buf, int nblk, hipEvent_t ready)
{
	const int slot0 = buf * fe->half_blocks;
	const float2 *rows = launch_canceller(fe, slot0, nblk, ready);
	if (rows) {
		HIP_TRY(hipGetLastError());
		ready = nullptr;                    // the demodulators follow the canceller on stream B, and it has waited
	} else rows = fe->chan_slot(slot0);
	return fe->demod.launch_half(rows, fe->cnt_slot(slot0), nblk, buf, ready, fe->stream_b, fe->stream_d, fe->timers);
}

// The half being filled is left with `nblk` blocks in it: its last block is the newest channelized one, the other half is filled next.
// with_demod: the half goes to the demodulator (launched now or held back).
static void leave_half(hfdl_gpu_frontend *fe, int nblk, bool with_demod)
{
	const int half = fe->cur_half;
	fe->last_slot = half * fe->half_blocks + nblk - 1;
	fe->last_index = nblk - 1;              // (one block: nothing further back to read, read_tap_block)
	fe->cur_half ^= 1;
	if (with_demod) fe->demod.order.hand_over(half);      // what poll_pdus_ready(.., 1) waits for: the half before the newest one
}

static int flush_pending_demod(hfdl_gpu_frontend *fe, bool after_fft)
{
	if (fe->pending_demod_buf < 0) return 0;
	const int buf = fe->pending_demod_buf, nblk = fe->pending_demod_nblk;
	fe->pending_demod_buf = -1;
	// the forward FFTs of the next half follow this half's inverse FFT on stream A, so their event covers the half's own too
	return launch_demod(fe, buf, nblk, after_fft ? fe->fft_done.event() : fe->chan[buf].event());
}

// When a block is pushed: its forward FFT into the next spectrum slot of the half being filled (the block's NCO phasor table and carried
// state ride on the three pass launches) -- on stream A for an uploaded block, on the input stream, beside the fold of the half before,
// for a device-resident one (planner.h FftOrder has the rules).  Nothing else happens until the half is closed.
static int enqueue_fft(hfdl_gpu_frontend *fe, FftInputs &in, int fmt, int stage_idx, int on_device)
{
	const Geometry &g = fe->geo;
	const int i = fe->batch_fill, set = fe->cur_half;
	const FftPushPlan plan = fe->order.push(fe->side_of(on_device != 0), i, fe->half_target, fe->pending_demod_buf >= 0);
	const hipStream_t st = fe->fft_stream(plan.side);
	// a forward FFT beside the fold carries nothing the held-back demodulators of the half before could wait for: launched now, as a sync would
	if (plan.flush_before)
		if (int rc = flush_pending_demod(fe, false)) return rc;
	if (plan.wait_switch) {
		// the forward FFT before this one ran on the other stream (mixed input: rare): behind everything queued there so far
		HIP_TRY(hipEventRecord(fe->ev_switch, fe->fft_stream(plan.side ^ 1)));
		HIP_TRY(hipStreamWaitEvent(st, fe->ev_switch, 0));
	}
	// beside the fold: this set of spectra / phasor tables / snapshots was last read by the fold and inverse FFT two halves ago
	if (plan.wait_set_free && fe->chan[set].pending()) HIP_TRY(hipStreamWaitEvent(st, fe->chan[set].event(), 0));
	// ... and the first fold after a drain is left alone: behind the inverse FFT of the half just closed, as on stream A
	if (plan.wait_first_fold) HIP_TRY(hipStreamWaitEvent(st, fe->chan[set ^ 1].event(), 0));
	// ... and behind the retune that rewrote a channel's constants and carried NCO state on stream A since the forward FFT before
	if (plan.wait_retune) HIP_TRY(hipStreamWaitEvent(st, fe->retune->done.event(), 0));
	// The events other streams (and the bench's fold timer) wait for ride on the kernel dispatches themselves
	// (hipExtLaunchKernelGGL start / stop events): a separate hipEventRecord is one more barrier packet in the queue, ~5 us
	// of idle machine each (profiles/r01_experiments.md).
	NcoJob job;
	job.cc = fe->d_cc; job.chain = fe->d_nco; job.snap = fe->snap_slot(set, i);
	job.ph = fe->ph_slot(set, i); job.cont = fe->d_ph_cont;
	job.nch = g.nch; job.outs = g.outs; job.post_input_size = g.post_input_size; job.post = g.post;
	// timed: the first pass' start and the last pass' stop ride on their dispatches; the stop event doubles as "this forward FFT is done":
	// what the half's fold waits for (beside the fold), what the held-back demodulators of the half before follow (the LAST forward
	// FFT of a half on stream A, launch_demod)
	hipEvent_t fft_start = nullptr, fft_done = nullptr;
	if (plan.side == FFT_BESIDE || plan.hold_after) {
		DoneEvent &done = plan.side == FFT_BESIDE ? fe->spec[set] : fe->fft_done;
		if (int rc = fe->timers.arm(ST_FFT, 1, done, fft_start)) return rc;
		fft_done = done.event();
	} else if (int rc = fe->timers.arm(ST_FFT, 1, fft_start, fft_done)) return rc;
	condition_input(fe, in, fmt, st);           // the opt-in input chain: what it leaves is what pass 1 reads
	// one three-pass sequence for every receiver of the step (kernels.h FftInputs)
	in.nrx = fe->nrx; in.hist_stride = g.overlap; in.out_stride = g.n;
	// The mixed domain: pass 2 leaves the fold's operand in the block's slot and carries fft_done; pass 3 runs for the spectrum monitor
	// alone, behind it, into the monitor's one-block scratch (forward FFTs run one after the other: one scratch serves them all)
	FftVariant var;
	float2 *spectrum = fe->spec_slot(set, i);
	if (g.mix_l1) {
		var.mix_out = spectrum; var.mix_q = g.mix_q; var.mix_rx_stride = g.n;
		spectrum = fe->monitor_scratch();
		var.passes = spectrum ? FFT_PASSES_ALL : FFT_PASSES_12;
	}
	// Real input: the block's pairs are transformed as they are, pass 3 stores unshifted into the scratch, and one more launch untangles
	// that into the slot, in natural order -- the equivalent stream's shifted order (real_input.h).  `done` and the timed stop ride on
	// that launch, as they moved to pass 2 for the mixed domain; input_read, the timed start and the riders stay on the passes.
	const bool real = fe->real_rate != 0;
	launch_fft_forward(fe->fft.p, fe->d_hist[fe->blocks & 1], in, fmt, g.overlap, fe->d_hist[(fe->blocks + 1) & 1], fe->d_work, real ? fe->d_real : spectrum, !real, st,
			FftOutLayout(), real ? nullptr : fft_done, job,
			stage_idx >= 0 ? fe->ev_stage_free[stage_idx].e : nullptr,      // input consumed once pass 1 is done: the copy stream may refill the buffer
			fft_start, var);
	if (real) {
		RealUntangleJob u;
		u.in = fe->d_real; u.out = spectrum; u.in_stride = u.out_stride = g.n; u.n = g.n; u.logn = fe->fft.p.logn; u.nrx = fe->nrx;
		launch_real_untangle(u, st, fft_done);
	}
	launch_monitor(fe, spectrum, st);
	if (plan.hold_after)
		if (int rc = flush_pending_demod(fe, true)) return rc;
	HIP_TRY(hipGetLastError());
	fe->blocks++;
	fe->batch_fill++;
	return 0;
}

// Stream A, when a half is closed (full, or as a sync / poll finds it): ONE pass over the filter taps per `fold_nb` spectra, then the
// inverse FFT / NCO of every block of the half in one launch.  A's inverse FFT may not overwrite a half before the demodulator
// launches that read it last (two halves ago) are done; B may not start before A has filled what it is given.
// with_demod: hand the half to the demodulator (now, or held back until the next half's forward FFTs are queued).
static int close_half(hfdl_gpu_frontend *fe, bool launch_now, bool with_demod = true)
{
	const int nblk = fe->batch_fill;
	if (nblk == 0) return 0;
	const Geometry &g = fe->geo;
	const int half = fe->cur_half;
	const HalfClosePlan plan = fe->order.close(launch_now);
	if (plan.wait_input) HIP_TRY(hipStreamWaitEvent(fe->stream, fe->spec[half].event(), 0));      // the newest forward FFT of this half beside the fold (stream C / F)
	// launches of up to `fold_nb` blocks (fold_launch_blocks), each timed and counted as the launch it is: the shape the bench prices is a
	// launch that happened
	for (int done = 0, take = 0; done < nblk; done += take) {
		take = fold_launch_blocks(g, nblk - done, fe->fold_nb);
		hipEvent_t start = nullptr, stop = nullptr;
		if (int rc = fe->timers.arm(ST_FOLD, take, start, stop)) return rc;
		if (launch_fold(g, fe->d_taps, fe->spec_slot(half, done), fe->spec_stride(), fe->d_partial + (size_t)done * fe->partial_stride(), fe->partial_stride(),
				take, fe->stream, start, stop) < 0)
			return fail(HFDL_GPU_EINVAL, "no fold launch of %d blocks on this geometry", take);
	}
	// this half is free once the demodulator launches that read it last (two halves ago) are done
	if (hipEvent_t e = fe->demod.half_read_event(half)) HIP_TRY(hipStreamWaitEvent(fe->stream, e, 0));
	if (with_demod && fe->own_decode_stream() && !fe->fold_bound) {
		// this half's first demodulator (launched right after this kernel, on stream B) reuses the frame queue the decoder of two
		// launches ago read: on the demodulator-bound geometries wait for it HERE, where the stream has slack, instead of in front of
		// the demodulator.  (Where the fold bounds the block stream A is the critical one and must not wait for a burst decoder:
		// measured, a 4.3 ms hole in front of every inverse FFT.  There the demodulator waits itself, planner.h DemodOrder.)
		if (hipEvent_t e = fe->demod.frames_free_event()) HIP_TRY(hipStreamWaitEvent(fe->stream, e, 0));
	}
	const int slot0 = half * fe->half_blocks;
	hipEvent_t ifft_start = nullptr;
	if (int rc = fe->timers.arm(ST_IFFT, nblk, fe->chan[half], ifft_start)) return rc;
	launch_ifft_nco(g, fe->d_partial, fe->partial_stride(), fe->d_cc, fe->snap_slot(half, 0), fe->ph_slot(half, 0), fe->ph_stride(), fe->d_tw_m,
			fe->chan_slot(slot0), fe->cnt_slot(slot0), nblk, fe->stream, fe->chan[half].event(), ifft_start);
	launch_export(fe, slot0, nblk);
	HIP_TRY(hipGetLastError());
	fe->last_set = half;
	fe->batch_fill = 0;
	leave_half(fe, nblk, with_demod);
	if (!with_demod) return 0;                   // channelize-only: the half is simply left behind
	// (forward FFTs beside the fold run beside everything anyway: there is no quiet moment to hold the demodulators back for)
	if (!plan.hold_back) return launch_demod(fe, half, nblk, fe->chan[half].event());
	fe->pending_demod_buf = half;
	fe->pending_demod_nblk = nblk;
	return 0;
}

// The boundary in front of a change of setting: everything pushed so far goes on under the old one -- a held-back half is launched, the half
// being filled is closed as a sync closes it, without the sync's waits.
int close_boundary(hfdl_gpu_frontend *fe)
{
	if (int rc = flush_pending_demod(fe, false)) return rc;
	return close_half(fe, true);
}

extern "C" int hfdl_gpu_frontend_channelize_block(hfdl_gpu_frontend *fe, const float *iq, size_t nsamples, int on_device)
{
	FftInputs in;
	int sidx = -1;
	int rc = single_receiver_only(fe, "hfdl_gpu_frontend_channelize_block");
	if (rc) return rc;
	const void *one[1] = { iq };
	int fmt = SFMT_CF32;                                    // (cf32 I/Q: a real front end refuses it)
	if ((rc = stage_input(fe, one, nsamples, fmt, on_device, in, &sidx))) return rc;
	if ((rc = close_boundary(fe))) return rc;               // blocks pushed for the demodulator and not yet handed to it
	if ((rc = enqueue_fft(fe, in, SFMT_CF32, sidx, on_device))) return rc;
	return close_half(fe, false, false);                    // this block is never demodulated
}

// The demodulator / burst-decoder stage alone: one block of channelizer OUTPUT from the host (what fastddc_inv_cc hands to
// hfdl_decoder_thread's loop body, src/hfdl.c:676) goes through K4 + K5 with the channel state carried as usual.  Stage parity:
// fed with the oracle's own channelizer output, the device demodulator is compared with the oracle's without the two channelizers'
// different fp32 roundings in between (tests/test_gpu_parity.py, profiles/strict_study.py).
extern "C" int hfdl_gpu_frontend_push_baseband(hfdl_gpu_frontend *fe, const float *chan_out, const int32_t *counts)
{
	if (!fe || !chan_out || !counts) return fail(HFDL_GPU_EINVAL, "null argument");
	const Geometry &g = fe->geo;
	for (int c = 0; c < g.nch; c++)
		if (counts[c] < 0 || counts[c] > g.outs) return fail(HFDL_GPU_ERANGE, "channel %d: %d samples, a block holds at most %d", c, counts[c], g.outs);
	int rc = hfdl_gpu_frontend_sync(fe);                    // a stage-test entry point: everything pushed before is finished first
	if (rc) return rc;
	const int half = fe->cur_half, slot0 = half * fe->half_blocks;
	HIP_TRY(hipMemcpy(fe->chan_slot(slot0), chan_out, sizeof(float2) * (size_t)g.nch * (size_t)g.outs, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(fe->cnt_slot(slot0), counts, sizeof(int32_t) * (size_t)g.nch, hipMemcpyHostToDevice));
	leave_half(fe, 1, true);
	return launch_demod(fe, half, 1, nullptr);               // no inverse FFT filled this half: the copies above are done, there is no event to wait for
}

// one step: raw[0 .. nrx - 1] = a block of every receiver
static int push_any(hfdl_gpu_frontend *fe, const void *const *raw, size_t nsamples, int fmt, int on_device)
{
	FftInputs in;
	int sidx = -1;
	int rc = stage_input(fe, raw, nsamples, fmt, on_device, in, &sidx);
	if (rc) return rc;
	if ((rc = enqueue_fft(fe, in, fmt, sidx, on_device))) return rc;
	if (fe->batch_fill < fe->half_target) return 0;         // the half is still filling
	// demodulator-bound geometry (few channels): the fold is short, there is nothing to place the demodulator under, and
	// holding it back until the NEXT half's forward FFTs would put those blocks' host -> device copies on the demodulator's
	// critical path (cfg2 fed from host memory: 0.56 -> 0.33 ms per block): launched at once.  Otherwise held back (launch_demod).
	rc = close_half(fe, !fe->fold_bound);
	fe->half_target = fe->half_blocks;                      // closed by filling: the caller runs ahead of the collection, the next halves take every slot
	return rc;
}

extern "C" int hfdl_gpu_frontend_push_block(hfdl_gpu_frontend *fe, const float *iq, size_t nsamples, int on_device)
{
	if (int rc = single_receiver_only(fe, "hfdl_gpu_frontend_push_block")) return rc;
	const void *one[1] = { iq };
	return push_any(fe, one, nsamples, SFMT_CF32, on_device);
}

extern "C" int hfdl_gpu_frontend_push_block_raw(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int sample_format, int on_device)
{
	if (int rc = single_receiver_only(fe, "hfdl_gpu_frontend_push_block_raw")) return rc;
	const void *one[1] = { raw };
	return push_any(fe, one, nsamples, sample_format, on_device);
}

extern "C" int hfdl_gpu_frontend_push_blocks_raw(hfdl_gpu_frontend *fe, const void *const *raw, size_t nsamples, int sample_format, int on_device)
{
	if (!fe || !raw) return fail(HFDL_GPU_EINVAL, "null argument");
	return push_any(fe, raw, nsamples, sample_format, on_device);
}

// ---------------------------------------------------------------- retune

// From this call on channel `channel` is a freshly created channel on new_freq_hz; blocks pushed before it run on the old frequency.  The
// half being filled is closed as a sync closes it, without the sync's waits, and each piece of the change is queued behind the last
// kernel that uses the old value and in front of the first that must see the new one:
//   A: new time-domain taps -> pad -> forward FFT into the channel's tap slot -> retune_channelizer_kernel (d_cc, d_nco, d_ph_cont).
//      The closed half's fold is behind every forward FFT queued so far wherever it ran, so stream A is too; the next forward FFT is
//      behind the kernel by stream order (A) or by the event the kernel carries (beside the fold: planner.h FftOrder::retune)
//   B: retune_demod_kernel behind the closed half's demodulators;  D: retune_freq_kernel behind its burst decoders
// Everything is checked, designed and allocated before the first launch: a refusal leaves the front end as it was.
extern "C" int hfdl_gpu_frontend_retune_channel(hfdl_gpu_frontend *fe, int32_t channel, int32_t new_freq_hz)
{
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	const int nch = fe->geo.nch;
	if (channel < 0 || channel >= nch) return fail(HFDL_GPU_EINVAL, "channel %d out of range (%d channels)", channel, nch);
	if (fe->prune_tol > 0) return fail(HFDL_GPU_EINVAL, "retune refused: HFDL_GPU_FOLD_PRUNE is set, and the pruned fold's row windows depend on the pass bands");
	const int rx = fe->rx_of[(size_t)channel];
	if (int rc = check_channel_span(fe->sample_rate, fe->nrx, channel, new_freq_hz, rx, fe->rx_center[(size_t)rx])) return rc;
	for (int c = 0; c < nch; c++)
		if (c != channel && fe->rx_of[(size_t)c] == rx && fe->freqs[(size_t)c] == new_freq_hz)
			return fail(HFDL_GPU_EINVAL, "channel %d of receiver %d already listens on %d Hz", c, rx, new_freq_hz);
	const size_t ntaps = fe->taps_host_len(), n = (size_t)fe->plan.n;
	ChanConst k;
	{
		std::vector<float> none;
		float cut = -1.f;
		if (!design_channel(fe, rx, new_freq_hz, k, nullptr, none, cut)) return fail(HFDL_GPU_EINVAL, "fastddc planning failed for %d channel(s)", 1);
	}
	HIP_TRY(hipSetDevice(fe->device));
	if (!fe->retune) {
		auto r = std::make_unique<Retune>();
		CREATE_TRY(r->pad.alloc(sizeof(float2) * n));
		CREATE_TRY(r->work.alloc(sizeof(float2) * n));
		if (fe->real_rate) CREATE_TRY(r->eo.alloc(sizeof(float2) * 2 * n));
		for (int i = 0; i < 2; i++) {
			CREATE_TRY(r->stage[i].alloc(ntaps));
			CREATE_TRY(r->staged[i].create(EV_NO_TIMING));
		}
		CREATE_TRY(r->done.own.create(EV_NO_TIMING));
		if (int rc = fe->demod.prepare_retune(fe->stream_b)) return rc;
		HIP_TRY(hipMemsetAsync(r->pad.p, 0, sizeof(float2) * n, fe->stream));
		fe->retune = std::move(r);
	}
	Retune &r = *fe->retune;
	const int sb = (int)(r.calls & 1);
	if (r.calls >= 2) HIP_TRY(hipEventSynchronize(r.staged[sb]));       // the tap FFT of two calls ago has read what was copied out of this buffer
	// the time-domain taps, designed on the host (exact reference arithmetic) straight into the page-locked buffer the copy reads
	static_assert(sizeof(std::complex<float>) == sizeof(float2), "taps are copied as cf32");
	design_channel(fe, rx, new_freq_hz, k, (std::complex<float> *)r.stage[sb].p, r.lp, r.lp_cut);
	// the boundary: what was pushed so far is folded and demodulated on the old frequency
	if (int rc = close_boundary(fe)) return rc;
	const int slot = fe->slot_of(channel);
	if (!fe->real_rate) HIP_TRY(hipMemcpyAsync(r.pad.p, r.stage[sb].p, sizeof(float2) * ntaps, hipMemcpyHostToDevice, fe->stream));
	FftOutLayout lay = fe->tap_layout;
	lay.chan = slot;
	float2 *dst = lay.kind == TAPL_PLAIN ? fe->d_taps + (size_t)slot * (size_t)fe->geo.tap_chan_stride : fe->d_taps;
	if (fe->real_rate) {
		// real input: the function build_taps() went through, so the words are a fresh create's
		if (int rc = queue_real_taps(fe, r.stage[sb].p, r.pad.as<float2>(), r.work.as<float2>(), r.eo.as<float2>(), slot, fe->stream, r.staged[sb])) return rc;
	} else if (fe->geo.mix_l1) {
		FftVariant v;
		v.passes = FFT_PASSES_12;
		launch_fft_forward(fe->fft.p, nullptr, r.pad.p, SFMT_CF32, 0, nullptr, r.work.as<float2>(), nullptr, true, fe->stream, FftOutLayout(), nullptr, NcoJob(), r.staged[sb], nullptr, v);
		launch_mixed_tap_pack(fe->fft.p, fe->geo, r.work.as<float2>(), fe->d_taps, slot, fe->stream);
	} else launch_fft_forward(fe->fft.p, nullptr, r.pad.p, SFMT_CF32, 0, nullptr, r.work.as<float2>(), dst, true, fe->stream, lay, nullptr, NcoJob(), r.staged[sb]);
	launch_retune_channelizer(fe->d_cc, fe->d_nco, fe->d_ph_cont, channel, k, fe->stream, r.done.signal());
	fe->demod.enqueue_retune(channel, new_freq_hz, fe->stream_b, fe->stream_d);
	if (int rc = canceller_retuned(fe, channel)) return rc;
	HIP_TRY(hipGetLastError());
	fe->order.retune();
	fe->freqs[(size_t)channel] = new_freq_hz;
	fe->cc[(size_t)channel] = k;
	r.calls++;
	return 0;
}

// ---------------------------------------------------------------- sync and poll

extern "C" int hfdl_gpu_frontend_sync(hfdl_gpu_frontend *fe)
{
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(fe->device));
	if (int rc = close_boundary(fe)) return rc;                     // blocks waiting for their half to fill: folded and demodulated now
	fe->half_target = fe->half_first;                               // a drain: the pipeline starts over with a short first half
	for (const Stream *s : { &fe->stream_c, &fe->stream_f, &fe->stream, &fe->stream_b, &fe->stream_d }) HIP_TRY(s->sync());      // (an alias is its owner's to synchronise)
	fe->order.drained();
	HIP_TRY(hipGetLastError());
	return fe->settle_events();
}

static int check_poll_args(const hfdl_gpu_frontend *fe, const hfdl_gpu_pdu *out, int32_t max, const int32_t *n)
{
	if (!fe || !n) return fail(HFDL_GPU_EINVAL, "null argument");
	if (!out && max > 0) return fail(HFDL_GPU_EINVAL, "null PDU buffer with max = %d", max);
	return 0;
}

extern "C" int hfdl_gpu_frontend_poll_pdus(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n)
{
	int rc = check_poll_args(fe, out, max, n);
	if (rc || (rc = hfdl_gpu_frontend_sync(fe))) return rc;
	return fe->demod.collect(out, max, n, fe->stream_d);
}

extern "C" int hfdl_gpu_frontend_poll_pdus_ready(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n, int32_t max_in_flight)
{
	if (max_in_flight <= 0) return hfdl_gpu_frontend_poll_pdus(fe, out, max, n);
	if (int rc = check_poll_args(fe, out, max, n)) return rc;
	*n = 0;
	// the newest half is left running (Demod::collect_ready): max_in_flight 1 waits for the demodulators of the half before it, 2 and more
	// wait for nothing
	HIP_TRY(hipSetDevice(fe->device));
	return fe->demod.collect_ready(max_in_flight < 2, out, max, n, fe->stream_d);
}
