/*
 * hfdl_gpu.h -- C ABI of the MI355X (gfx950) HFDL front end: libhfdl_gpu.so
 *
 * Drop-in boundary for dumphfdl's hot path.  Plain C types only: the host
 * program stays C (block / input-common / hfdl_channel API in include/hfdl_host.h) and binds these
 * entry points; they replace, for ALL channels of one receiver at once:
 *
 *   reference interface (file:line)                               -> entry point here
 *   ---------------------------------------------------------------------------------------------
 *   fft_create(decimation, transition_bw)          src/fft.h:31,  src/fft.c:70-86      \
 *   hfdl_channel_create(fs, decim, tbw, cf, freq)  src/hfdl.h:11, src/hfdl.c:468-534    } hfdl_gpu_frontend_create
 *   fft_channelizer_create(...)                    src/fastddc.h:42, src/fastddc.c:217 /
 *   fft_thread loop body: overlap + csdr_fft_execute + fft_swap_sides   src/fft.c:49-59 \
 *   hfdl_decoder_thread loop body: fastddc_inv_cc .. decode_user_data   src/hfdl.c:662-891 } hfdl_gpu_frontend_push_block
 *   dispatch_pdu -> pdu_decoder_queue_push(metadata, octet_string, 0)   src/hfdl.c:1058-1080 -> hfdl_gpu_frontend_poll_pdus
 *   fft_destroy / hfdl_channel_destroy             src/fft.h:32, src/hfdl.h:13          -> hfdl_gpu_frontend_destroy
 *   csdr_fft_execute(fwd)+fft_swap_sides           src/fft_fftw.c:39-41, src/fastddc.c:102 -> hfdl_gpu_fft_forward
 *   update_viterbi27_blk + chainback_viterbi27     src/libfec/fec.h:19-20               -> hfdl_gpu_burst_decode / hfdl_gpu_viterbi27
 *   decimating_shift_addition_init / _cc           src/libcsdr_gpl.h:43-44, src/libcsdr_gpl.c:26-74 -> hfdl_gpu_nco_decimate
 *   crc16_ccitt                                    src/crc.h, src/crc.c:4-47            -> hfdl_gpu_crc16_ccitt
 *   hfdl_pdu_fcs_check + header length rules       src/pdu.c:68-79, src/mpdu.c:56-79, src/spdu.c:55-62 -> hfdl_gpu_pdu_triage
 *   modem_demodulate + phase error (liquid PSK)    src/hfdl.c:737-741                   -> hfdl_gpu_psk_slice (the carrier loop's slicer)
 *   parse_lpdu_list + lpdu_parse's FCS check       src/mpdu.c:92-158, src/lpdu.c:136-149 -> hfdl_gpu_lpdu_walk (and hfdl_gpu_pdu.lpdus_*)
 *
 * All functions return 0 on success or a negative HFDL_GPU_E* code (the reference's constructors
 * return NULL / -1 and xcalloc failure _exit()s: src/util.c:25-33); hfdl_gpu_last_error() gives text.
 * There is no CPU fallback: if no gfx950 device is usable every call fails with HFDL_GPU_ENODEV.
 *
 * Threading: a front end is driven by ONE thread at a time (the reference's fft_thread; src/fft.c:30-66); different front
 * ends -- one per GPU -- are independent.  hfdl_gpu_last_error() is per calling thread.
 */
#ifndef HFDL_GPU_H
#define HFDL_GPU_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HFDL_GPU_EINVAL   (-1)
#define HFDL_GPU_ENODEV   (-2)
#define HFDL_GPU_ENOMEM   (-3)
#define HFDL_GPU_EHIP     (-4)
#define HFDL_GPU_ERANGE   (-5)

#define HFDL_GPU_PDU_MAX_OCTETS 960

/* on-device header triage of a decoded PDU (what mpdu_parse / spdu_parse do first: src/mpdu.c:56-89, src/spdu.c:55-62) */
#define HFDL_GPU_FCS_GOOD      0
#define HFDL_GPU_FCS_BAD       1
#define HFDL_GPU_FCS_TOO_SHORT 2
#define HFDL_GPU_KIND_SPDU          0
#define HFDL_GPU_KIND_MPDU_DOWNLINK 1
#define HFDL_GPU_KIND_MPDU_UPLINK   2

typedef struct hfdl_gpu_frontend hfdl_gpu_frontend;

/* block geometry: the fields of the reference's fastddc_t (src/fastddc.h:8-27) for shift = 0 */
typedef struct {
	int32_t sample_rate, decimation;
	int32_t pre_decimation, post_decimation;
	int32_t taps_length, overlap_length;
	int32_t fft_size, fft_inv_size, input_size, post_input_size, scrap;
	int32_t outputs_per_block;       /* post_input_size / post_decimation */
	int32_t channels;
	int32_t fold_slices;             /* alias-row slices per channel in the fold kernel */
	float   transition_bw;
	float   resamp_rate;             /* 5400 / (fs / decimation) */
	int32_t max_outputs_per_block;   /* ceil(post_input_size / post_decimation): what a block can emit when the carried
	                                    decimation remainder is non-zero (post_input_size not a multiple of post_decimation);
	                                    size HFDL_GPU_TAP_CHAN_OUT buffers from this */
	int32_t demod_batch;             /* blocks one demodulator launch takes when they are pushed faster than they are collected (a half that
	                                    closes full is one launch, cut down where a launch's output counts would not fit 16 bits: 32 at 40 Msps, 8 on
	                                    the small geometries).  Results do not
	                                    depend on it; a poll / sync always demodulates what has been pushed.  HFDL_GPU_DEMOD_BATCH=1..32 overrides
	                                    the default at create time.  0 from hfdl_gpu_plan_geometry() */
	int32_t fold_batch;              /* blocks whose spectra one fold launch multiplies against ONE pass over the per-channel filter taps when
	                                    they are pushed faster than they are collected (src/fastddc.c:123-150 run for that many blocks; the taps are
	                                    > 99 % of a block's bytes on the 256-channel geometries).  Every block's result is bit-identical to a launch
	                                    of its own; a poll / sync always folds what has been pushed.  HFDL_GPU_FOLD_BATCH=1..32 overrides the default
	                                    (32 from 128 channels up, where the fold bounds the block -- the first half after a drain closes at 16 --; 8 below) at create time.  0 from hfdl_gpu_plan_geometry() */
	int32_t prefetch_depth;          /* host blocks whose upload hfdl_gpu_frontend_prefetch_block_raw() may queue ahead of their push
	                                    (half + 1, for a staging ring of half + 2 buffers in HBM, where a half = the blocks between two fold / inverse-FFT
	                                    phases = fold_batch rounded up to hold at least demod_batch blocks); at most HFDL_GPU_PREFETCH_MAX (a 32-block
	                                    half is not uploaded a whole half ahead: 17 blocks of link time cover its fold several times over).
	                                    0 from hfdl_gpu_plan_geometry() */
	int32_t fold_rows;               /* alias rows a fold workgroup adds up at most: pre_decimation (all of them, the reference's sum term for
	                                    term) unless HFDL_GPU_FOLD_PRUNE is set.  0 from hfdl_gpu_plan_geometry() */
} hfdl_gpu_geometry;
#define HFDL_GPU_PREFETCH_MAX 17
#define HFDL_GPU_FOLD_BATCH_MAX 32   /* blocks one fold launch takes at most: two column groups of the sixteen-column matrix instruction */

/* Create-time configuration read from the environment by hfdl_gpu_frontend_create() (every create reads it afresh; nothing is cached):
 *   HFDL_GPU_FOLD_BATCH   1..32  blocks per fold launch (geometry.fold_batch)
 *   HFDL_GPU_DEMOD_BATCH  1..32  blocks per demodulator launch (geometry.demod_batch)
 *   HFDL_GPU_HOST_THREADS >= 1   host threads that design the filter taps (default: one per core; set to cores / processes when several
 *                                front ends are created at once on one host)
 *   HFDL_GPU_PDU_RING     >= 1   capacity of the device PDU ring (default max(4096, 64 per channel))
 *   HFDL_GPU_FOLD_PRUNE   tol    (default unset: off) the pruned fold: a channel's filter is a band-pass with a windowed-sinc stop band, and
 *                                of the N / M alias rows the reference adds up (src/fastddc.c:123-150) all but the few around the pass band hold
 *                                taps at the level of their own rounding noise.  With tol set (1e-12 .. 1e-3) a workgroup folds only
 *                                the rows outside which its channels' filters hold less than tol^2 of their energy (geometry.fold_rows of
 *                                pre_decimation): the channelizer output moves by ~tol relative RMS and the fold's time by the ratio of the
 *                                rows.  The stored taps carry the rounding noise of the fp32 transform that made them (2.1e-7 of their energy
 *                                as an amplitude ratio at N = 2^23) in EVERY row: a tolerance below that keeps every row.  Off, every row is
 *                                folded -- the reference's sum, term for term.  Ignored by a front end of several receivers
 *                                (hfdl_gpu_frontend_create_multi with nrx > 1): there geometry.fold_rows = pre_decimation
 *   HFDL_GPU_FOLD_SPECTRUM 0 / 1 (default 1) 1: the fold reads full spectra -- all three passes of the forward FFT -- on every geometry.
 *                                0: a geometry whose forward FFT runs the register-resident passes (fft_size >= 2^18) with at least
 *                                sixteen bins of fft_inv_size per first-pass index and no pruned fold stops the transform after its second
 *                                pass and folds there: the third pass is a plain DFT, and the fold's sum over its outputs equals the sum
 *                                over its inputs against the taps' second-pass transform, index-reversed and scaled by the radix
 *                                (DESIGN.md section 4.2): 5 % more samples per second at 40 Msps x 256 channels.  Every tap still meets
 *                                every sample in fp32, but what the filter rejects is then rejected by cancellation inside the fp32
 *                                accumulator, not by small taps: out-of-band signals 60 dB above a channel leave its output up to 1.6e-4
 *                                (relative RMS) from the exact convolution instead of 0.6e-4, in proportion to their level.  Hence opt-in.
 *                                HFDL_GPU_TAP_SPECTRUM and HFDL_GPU_TAP_FILTER read the same words either way
 * The A/B switches of the measurement scripts (stream placement, tiling sweeps, probes) are in the laboratory build only:
 * include/hfdl_gpu_lab.h, libhfdl_gpu_lab.so. */

/* one decoded PDU: what dispatch_pdu() hands to pdu_decoder_queue_push (src/hfdl.c:1058-1080,
 * struct hfdl_pdu_metadata src/pdu.h:8-17).  The wall-clock rx_timestamp of the reference is
 * replaced by the 5400-sps sample index at A2 detection (reproducible on file input). */
typedef struct {
	int32_t  channel;                /* index into the freqs[] given at create */
	int32_t  freq;                   /* Hz */
	int32_t  mode;                   /* M1 index 0..7 */
	int32_t  bit_rate;
	int32_t  len;                    /* octets */
	float    freq_err_hz, rssi_db, noise_floor_db;
	char     slot;                   /* 'S' / 'D' */
	uint8_t  fcs_status;             /* HFDL_GPU_FCS_*: header FCS checked on the device (src/pdu.c:68-79) */
	uint8_t  pdu_kind;               /* HFDL_GPU_KIND_*: SPDU / MPDU direction triage (src/pdu.c:124-128, src/mpdu.c:56-74) */
	uint16_t hdr_len;                /* octets covered by the FCS */
	uint64_t sample_index;
	int32_t  train_bits_bad, train_bits_total;
	/* MPDUs with a good header FCS: the LPDU list walked on the device (parse_lpdu_list, src/mpdu.c:136-158) with every LPDU's own
	 * FCS checked (lpdu_parse, src/lpdu.c:136-149) -- the reference's lpdus.processed / lpdus.good / lpdu.errors.bad_fcs /
	 * lpdu.errors.too_short events of this PDU; lpdus_truncated = an announced LPDU runs past the PDU.  All 0 otherwise. */
	uint8_t  lpdus_processed, lpdus_good, lpdus_bad_fcs, lpdus_too_short, lpdus_truncated, lpdu_pad[3];
	uint8_t  octets[HFDL_GPU_PDU_MAX_OCTETS];
} hfdl_gpu_pdu;

/* ---- planning (host only, no device needed) ---- */

/* fastddc_init(.., shift = 0) as fft_create() runs it (src/fft.c:70-86, src/fastddc.c:46-80): block geometry for a
 * decimation / relative transition bandwidth pair.  channels / fold_slices / sample_rate / resamp_rate are left 0. */
int  hfdl_gpu_plan_geometry(int32_t decimation, float transition_bw, hfdl_gpu_geometry *g);

/* page-locked host memory for block staging (the role of the reference's ring read pointer, src/fft.c:50-53) */
int  hfdl_gpu_host_alloc(void **ptr, size_t bytes);
void hfdl_gpu_host_free(void *ptr);

/* ---- whole front end ---- */

/* frequencies in Hz as in hfdl_channel_create(); decimation / transition_bw are derived exactly as
 * main() does (src/main.c:699-704): compute_fft_decimation_rate(fs, 5400), 250 Hz / fs.
 * sample_rate >= 5400, as the reference's main() asks.  A receiver below 10 800 sps (decimation 1) is accepted as the reference
 * accepts it and, there as here, decodes nothing: with pre_decimation = post_decimation = 1 the reference's bin arithmetic leaves
 * its channel half the channel's own sample rate off (the output times (-1)^k), which this library reproduces (oracle/PINNING.md
 * section 3).  From 10 800 sps up channels decode. */
int  hfdl_gpu_frontend_create(hfdl_gpu_frontend **out, int device, int32_t sample_rate, int32_t centerfreq,
		const int32_t *freqs, int32_t nch);
void hfdl_gpu_frontend_destroy(hfdl_gpu_frontend *fe);

/* ---- several receivers in one front end ----
 * nrx receivers at one sample rate: receiver r is centred on centerfreqs[r] and carries nch_per_rx[r] channels.
 * freqs[] lists them receiver-major (receiver 0's channels first), so a channel index -- hfdl_gpu_pdu.channel, the
 * channel argument of stats / taps -- is global over the front end.  Each channel must lie within +-fs/2 of ITS receiver's centre.
 * One pipeline carries them all: per step ONE batched forward-FFT sequence transforms every receiver's block, one fold launch (per
 * tiling, as for one receiver) multiplies every channel of every receiver against one pass over the filter taps, and one inverse-FFT /
 * NCO, demodulator and burst-decoder launch covers all channels.  hfdl_gpu_frontend_create(..) IS this call with nrx = 1 (the same
 * code path, the same results).
 * Rules:
 *   - every argument is checked before a device is selected: null pointers, nrx outside 1 .. HFDL_GPU_RECEIVERS_MAX, a channel count
 *     <= 0, the span of each channel against its own receiver's centre, the sample rate (HFDL_GPU_EINVAL)
 *   - with nrx > 1, hfdl_gpu_frontend_push_block, _push_block_raw, _channelize_block, _prefetch_block_raw and _prefetch_cancel return
 *     HFDL_GPU_EINVAL and enqueue nothing: a step takes a block of every receiver (hfdl_gpu_frontend_push_blocks_raw); prefetching is
 *     for one receiver only
 *   - host blocks (hfdl_gpu_frontend_input_done_upto / _input_copied) count steps: one hfdl_gpu_frontend_push_blocks_raw call = one host block
 *   - HFDL_GPU_TAP_SPECTRUM (read_tap / read_tap_block): with nrx > 1 `channel` selects the spectrum of that channel's receiver and
 *     must be in range; with nrx = 1 it is ignored
 *   - geometry.channels = all channels of all receivers; fold_batch, demod_batch and prefetch_depth report what was chosen: the
 *     per-block buffers of the forward FFT scale with nrx, and a front end of nrx > 1 receivers keeps nrx x (blocks per half) x fft_size
 *     <= 32 x 2^23 (spectra, staging ring, history): where that binds, fold_batch shrinks (never below one block) and demod_batch
 *     with it.  A create that still cannot allocate fails with HFDL_GPU_ENOMEM and leaks nothing
 *   - HFDL_GPU_FOLD_PRUNE is ignored with nrx > 1 (geometry.fold_rows = pre_decimation)
 *   - the receivers are assumed to be clocked alike (one sample rate); pacing, drift and dropouts of live sources are the caller's business */
#define HFDL_GPU_RECEIVERS_MAX 64
int  hfdl_gpu_frontend_create_multi(hfdl_gpu_frontend **out, int device, int32_t sample_rate, int32_t nrx,
		const int32_t *centerfreqs, const int32_t *freqs, const int32_t *nch_per_rx);
/* One block of EVERY receiver: raw[r] holds geometry.input_size samples of receiver r, all in one sample format (HFDL_GPU_SFMT_*);
 * on_device / host-buffer rules as hfdl_gpu_frontend_push_block_raw (page-locked buffers reusable after input_done / sync / poll).
 * Works on any front end, nrx = 1 included. */
int  hfdl_gpu_frontend_push_blocks_raw(hfdl_gpu_frontend *fe, const void *const *raw, size_t nsamples, int sample_format, int on_device);
/* ---- real-sampled input: direct-sampling receivers ----
 * nrx receivers that deliver REAL samples at sample_rate_real; base_freqs[r] is the RF frequency that appears at 0 Hz in receiver r's
 * samples (0 for direct sampling), so receiver r covers base .. base + sample_rate_real / 2.  The call mirrors
 * hfdl_gpu_frontend_create_multi (nrx = 1 is the ordinary case) and the front end is that call's for the EQUIVALENT COMPLEX STREAM of
 * half the rate: sample rate sample_rate_real / 2, centre base + sample_rate_real / 4.  hfdl_gpu_frontend_geometry() and
 * hfdl_gpu_frontend_channel_receiver() report that stream; hfdl_gpu_frontend_real_input() says the rest.  A block of 2 fft_size real
 * samples goes through the fft_size-point complex transform of its sample pairs and one small launch behind it, the channel filters are
 * designed at the real rate with 2 overlap_length + 1 taps and stored for the non-negative frequencies alone (half the taps, half the
 * fold's work of a zero-imaginary stream): what a channel receives is (h * x_a) / 2 with x_a the block's analytic signal -- the mirror
 * image is rejected outright, not through the filter's stop band.
 * Checked before a device is selected (HFDL_GPU_EINVAL): null pointers, sample_rate_real even and >= 21 600, every base >= -2^30 with its
 * span base .. base + sample_rate_real / 2 + 1440 inside an int32 of hertz (checked in 64 bits before the centre is formed), every channel within +- a quarter of
 * sample_rate_real of its receiver's base + sample_rate_real / 4, the rest as hfdl_gpu_frontend_create_multi.
 * Rules:
 *   - input: hfdl_gpu_frontend_push_block_raw, _push_blocks_raw and _prefetch_block_raw with HFDL_GPU_SFMT_RS16 (int16, the full scale
 *     of CS16) or HFDL_GPU_SFMT_RF32 (float32) and nsamples = 2 * geometry.input_size real samples.  A complex format on a real front
 *     end, or a real one on a complex front end, is HFDL_GPU_EINVAL and enqueues nothing; hfdl_gpu_frontend_push_block and
 *     _channelize_block (cf32 I/Q) are therefore refused.  hfdl_gpu_frontend_push_baseband works: it starts behind the channelizer
 *   - the spectrum monitor works unchanged on the equivalent stream: its bands span base .. base + sample_rate_real / 2
 *   - the blanker works unchanged, on the PAIRS it reads: a pair (x[2n], x[2n + 1]) whose power x[2n]^2 + x[2n + 1]^2 exceeds the
 *     threshold goes as a whole, and the mean is over pairs
 *   - hfdl_gpu_frontend_iqbal_enable and _iqbal_seed are HFDL_GPU_EINVAL: there is no I/Q to balance
 *   - carrier canceller, export, frame quality records and retune are per channel and unchanged; a retuned channel's filter is a
 *     fresh create's, bit for bit
 *   - HFDL_GPU_FOLD_SPECTRUM=0 and HFDL_GPU_FOLD_PRUNE are ignored, as the prune is with nrx > 1
 *   - HFDL_GPU_TAP_SPECTRUM returns the fft_size bins of the block's 2 fft_size-point real transform from 0 Hz up (bin k is
 *     base + k sample_rate_real / (2 fft_size)); HFDL_GPU_TAP_FILTER the stored words, the factor 1/2 included */
#define HFDL_GPU_SFMT_RS16 3
#define HFDL_GPU_SFMT_RF32 4
int  hfdl_gpu_frontend_create_real(hfdl_gpu_frontend **out, int device, int32_t sample_rate_real, int32_t nrx,
		const int32_t *base_freqs, const int32_t *freqs, const int32_t *nch_per_rx);
/* *is_real = 1 and *real_rate = sample_rate_real for a front end made by hfdl_gpu_frontend_create_real, 0 and 0 otherwise */
int  hfdl_gpu_frontend_real_input(const hfdl_gpu_frontend *fe, int32_t *is_real, int32_t *real_rate);
/* receiver and centre frequency of a channel */
int  hfdl_gpu_frontend_channel_receiver(const hfdl_gpu_frontend *fe, int32_t channel, int32_t *rx, int32_t *centerfreq);
int  hfdl_gpu_frontend_geometry(const hfdl_gpu_frontend *fe, hfdl_gpu_geometry *g);

/* Enqueue one block: exactly geometry.input_size new complex samples (interleaved I,Q float32).  Asynchronous: the block's forward
 * FFT is queued at once; fold, inverse FFT, demodulator and burst decoder follow when geometry.fold_batch blocks are waiting or the
 * caller syncs / polls, whichever comes first (the results do not depend on which).
 * on_device != 0: `iq` is a device pointer that stays valid until the next sync; its forward FFT runs on the input stream
 *   (hfdl_gpu_frontend_stream()), beside the fold of the blocks before.  Host and device blocks may be mixed freely.
 * on_device == 0: the host -> device copy runs on its own stream into a ring of geometry.prefetch_depth + 1 staging buffers, so the copies
 *   run up to a whole half (fold_batch blocks, or more where demod_batch is larger) ahead of the kernels.  A buffer from hfdl_gpu_host_alloc() (page-locked) is read by DMA after the call
 *   returns: reuse it only after hfdl_gpu_frontend_input_done() / _sync() / _poll_pdus().  Any other host buffer (pageable,
 *   or registered by the caller) is waited for inside the call and may be reused as soon as it returns. */
int  hfdl_gpu_frontend_push_block(hfdl_gpu_frontend *fe, const float *iq, size_t nsamples, int on_device);
/* wait until every host -> device input copy enqueued so far has finished (the kernels keep running, the forward FFTs of device
 * blocks on the same stream included) */
int  hfdl_gpu_frontend_input_done(hfdl_gpu_frontend *fe);
/* wait until the copy of host block number `host_block` (0 = the first block pushed with on_device == 0) has finished, WITHOUT
 * waiting for the blocks pushed after it: a caller that leases two page-locked buffers pushes block k+1, then waits for block k and
 * reuses its buffer -- the copy engine never idles on the host thread */
int  hfdl_gpu_frontend_input_done_upto(hfdl_gpu_frontend *fe, uint64_t host_block);
/* the same question without waiting: 1 = the copy of that host block has finished, 0 = not yet, negative = error */
int  hfdl_gpu_frontend_input_copied(hfdl_gpu_frontend *fe, uint64_t host_block);
/* Queue the host -> device copy of a block that will be pushed LATER (a buffer from hfdl_gpu_host_alloc(), host pointer) without
 * pushing it: the copy then runs beside the blocks still computing -- the fold of a 40 Msps x 256-channel half takes 3 ms, five blocks
 * of PCIe time -- and the following hfdl_gpu_frontend_push_block_raw() of the same pointer and format only queues kernels.  Up to
 * geometry.prefetch_depth blocks may wait this way (HFDL_GPU_ERANGE beyond); they must be pushed in the order they were prefetched.
 * A prefetched block counts as a host block for hfdl_gpu_frontend_input_done_upto() from this call on. */
int  hfdl_gpu_frontend_prefetch_block_raw(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int sample_format);
/* Forget the prefetched blocks (a caller that hit an error between a prefetch and its push): waits for the copies, after which the
 * buffers are the caller's again and any block may be pushed next.  The blocks keep their host block numbers.  No-op without a prefetch.
 * While a prefetch is pending, a push of anything but the oldest prefetched block -- another pointer, another format, a device block --
 * is HFDL_GPU_EINVAL and leaves the queue in place. */
int  hfdl_gpu_frontend_prefetch_cancel(hfdl_gpu_frontend *fe);
/* Same, for raw recorder / SDR samples converted on the device inside the overlap-assembly load of the forward FFT
 * (convert_cs16 / convert_cu8 / convert_cf32, src/input-helpers.c:10-78): interleaved I,Q int16 (full scale 32767.5),
 * uint8 (offset 63.5, full scale 127) or float32.  Halves / quarters the host->device bytes per sample. */
#define HFDL_GPU_SFMT_CF32 0
#define HFDL_GPU_SFMT_CS16 1
#define HFDL_GPU_SFMT_CU8  2
int  hfdl_gpu_frontend_push_block_raw(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int sample_format, int on_device);
/* the demodulator + burst decoder stage alone (for stage parity): one block of channelizer OUTPUT from host memory -- chan_out[channels]
 * [max_outputs_per_block + 1] complex samples (interleaved re, im; rows of that length whatever counts[] says), counts[c] of them valid
 * for channel c -- through the same kernels and carried channel state as a pushed block's (hfdl_decoder_thread's loop body after
 * fastddc_inv_cc, src/hfdl.c:676-892).  Syncs first; collect with hfdl_gpu_frontend_poll_pdus(). */
int  hfdl_gpu_frontend_push_baseband(hfdl_gpu_frontend *fe, const float *chan_out, const int32_t *counts);
/* run only the channelizer part of a block (forward FFT + fold + inverse FFT + NCO); for stage parity/bench */
int  hfdl_gpu_frontend_channelize_block(hfdl_gpu_frontend *fe, const float *iq, size_t nsamples, int on_device);
int  hfdl_gpu_frontend_sync(hfdl_gpu_frontend *fe);
/* Collect PDUs produced by all blocks enqueued so far (implies a sync). Returns count in *n.  `out` must hold `max`
 * entries; out == NULL with max > 0 is HFDL_GPU_EINVAL (nothing is discarded), max == 0 just syncs. */
int  hfdl_gpu_frontend_poll_pdus(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n);
/* Same without draining the pipeline: with max_in_flight = 1 whatever was pushed since the last half filled keeps filling, the newest
 * CLOSED half (geometry.fold_batch blocks, or max(fold_batch, demod_batch)) keeps running; the call waits only for the demodulators of the
 * half before it and returns the PDUs known to be complete at that moment -- those of that half if its burst decoders have finished too,
 * otherwise they come with the next call (nothing until two halves were closed).  max_in_flight = 0 is hfdl_gpu_frontend_poll_pdus();
 * max_in_flight >= 2 does not wait at all: if those demodulators are still running the call returns no PDUs (for a caller that bounds
 * what it queues by other means -- the C host program by the ring slots it leases to the uploads).
 * A file replay pushes block k+1, then collects this way, so copies, channelizer, demodulator and burst decoder of consecutive halves
 * overlap and the fold shares its pass over the filter taps between the blocks of a half; a live receiver that has no further input
 * queued uses 0 and gets its PDUs at once. */
int  hfdl_gpu_frontend_poll_pdus_ready(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n, int32_t max_in_flight);
/* PDUs wait in a device ring of pdu_ring_capacity entries; one that finds the ring full is dropped and counted
 * (the reference's GAsyncQueue is unbounded, src/pdu.c:37-43: poll at least once per few seconds of signal).
 * Capacity: max(4096, 64 per channel); the environment variable HFDL_GPU_PDU_RING overrides it at create time. */
typedef struct {
	uint64_t blocks;                 /* blocks pushed so far */
	uint32_t pdus_taken;             /* PDUs handed to the host so far (mod 2^32) */
	uint32_t pdus_dropped;           /* as of the last poll */
	uint32_t pdu_ring_capacity;
} hfdl_gpu_frontend_counters_t;
int  hfdl_gpu_frontend_counters(hfdl_gpu_frontend *fe, hfdl_gpu_frontend_counters_t *out);
/* the HIP stream that reads device-resident input (hipStream_t as void*): the front end's input stream, on which the forward FFT of a
 * block pushed with on_device != 0 is launched -- beside the fold of the blocks before, which runs on a stream of its own -- and which
 * carries the host -> device copies of the other blocks.  Device input handed to push_block must be complete on, or synchronised with,
 * this stream: a block produced ON it (a kernel or a device-side copy queued there before the push) needs no synchronisation at all.
 * The push contract is unchanged: the pointer stays valid until the next sync, the forward FFT is queued at once */
void *hfdl_gpu_frontend_stream(hfdl_gpu_frontend *fe);

/* per-channel observability: the hot-path StatsD counters and the noise-floor gauge of the reference
 * (src/hfdl.c:818-840, 1082-1105; doc/STATSD_METRICS.md), read from the device-resident channel state */
typedef struct {
	int32_t  freq;
	uint32_t a2_found, m1_found, m1_not_found, frames;
	float    noise_floor_db;         /* 20 log10(noise_floor), what noise_floor_stats_thread reports */
	float    agc_level, costas_dphi;
	int32_t  framer_state;           /* 1 = A1 search ... 7 = DATA_2 (src/hfdl.c:54-62) */
	uint64_t sample_cnt, symbol_cnt;
	/* the reference's debug summary (hfdl_print_summary, src/hfdl.c:563-573), per channel: A1 detections, mean |correlation| at the
	 * A1 / A2 / M1 detections (0 when there were none), training bits of all frames received */
	uint32_t a1_found;
	float    a1_corr_avg, a2_corr_avg, m1_corr_avg;
	uint32_t train_bits_bad, train_bits_total;
} hfdl_gpu_channel_stats;
int  hfdl_gpu_frontend_channel_stats(hfdl_gpu_frontend *fe, int32_t channel, hfdl_gpu_channel_stats *out);
/* every channel in one strided device read, WITHOUT waiting for blocks in flight: each field is read whole, the set may
 * straddle a block boundary (what a periodic gauge needs: noise_floor_stats_thread, src/hfdl.c:1082-1105) */
int  hfdl_gpu_frontend_all_channel_stats(hfdl_gpu_frontend *fe, hfdl_gpu_channel_stats *out, int32_t cap, int32_t *n);

/* Spectrum monitor (off by default): band powers of every receiver from the forward FFT's own spectra, accumulated on the device.
 * For receiver r and block t let X[s], s = 0 .. N - 1 (N = geometry.fft_size) be the fftshifted spectrum of the block's overlap-and-
 * scrap window [history, new]; shifted index s is the frequency centerfreq_r + (s - N/2) fs/N.  With bins = B and G = N / B:
 *   window RECT (flags 0): Xw[s] = X[s], wpow = 1;
 *   window HANN:           Xw[s] = 0.5 X[s] - 0.25 X[(s - 1) mod N] - 0.25 X[(s + 1) mod N], wpow = 0.375 -- the periodic Hann window
 *                          w[n] = 0.5 - 0.5 cos(2 pi n / N) applied in the frequency domain, exactly FFT(w x);
 *   band power of a block: p_t[b] = sum_{s = bG}^{(b+1)G - 1} |Xw[s]|^2 / (N^2 wpow): a full-scale tone (|x| = 1) adds 1.0 (0 dBFS) to
 *                          the band(s) it falls in; with RECT the bands of a block sum to the mean |x|^2 of its window (Parseval);
 *   read back:             mean[b] = (1/T) sum_t p_t[b] over the T blocks since the last reset and, with MAXHOLD, peak[b] = max_t p_t[b];
 *                          linear power, fp32.
 * Band b spans centerfreq_r + (bG - N/2 - 0.5) fs/N .. that + G fs/N.  Consecutive windows overlap by geometry.overlap_length
 * samples: a Welch estimate with that fixed overlap.  The result for a given input, bins and flags is bit-identical from run to run
 * and does not depend on how the caller polls or on fold / demodulator batching.  A block = one push (of every receiver) or one
 * channelize_block; push_baseband is none. */
#define HFDL_GPU_SPECTRUM_HANN    1u
#define HFDL_GPU_SPECTRUM_MAXHOLD 2u
/* bins: a power of two, 16 <= bins <= fft_size / 16; 0 turns the monitor off and frees its buffers.  Takes effect with the next
 * pushed block; calling it again resets the accumulators of every receiver.  HFDL_GPU_EINVAL (null handle, unknown flag, bins no
 * power of two or below 16) / HFDL_GPU_ERANGE (bins > fft_size / 16) are checked before any device work. */
int  hfdl_gpu_frontend_spectrum_enable(hfdl_gpu_frontend *fe, int32_t bins, uint32_t flags);
/* mean[bins] (and peak[bins]; may be NULL, HFDL_GPU_EINVAL if asked for without MAXHOLD) of receiver rx over the blocks accumulated
 * since the last reset; cap = floats each array holds (HFDL_GPU_ERANGE below bins).  *blocks = T (0: nothing yet, the arrays are
 * left untouched), *first_block = index of the first of them in the numbering of hfdl_gpu_frontend_counters().blocks.  reset != 0
 * starts a new average for THIS receiver after the read.  The call queues nothing on the kernels' streams: no half is closed, no
 * fold launched, the PDU stream is what it is without the read.  It BLOCKS until the newest forward FFT (and its monitor launch)
 * has run.  The forward FFTs share a stream with the folds and inverse FFTs of the halves closed before them, and an inverse FFT
 * waits for the demodulators that read its buffer last, so the caller in effect waits for the device to catch up to the newest
 * pushed block (everything but the newest half's fold and demodulators): read every second of signal, not every block. */
int  hfdl_gpu_frontend_spectrum_read(hfdl_gpu_frontend *fe, int32_t rx, float *mean, float *peak, int32_t cap,
		uint64_t *blocks, uint64_t *first_block, int reset);

/* History of interval rows (off by default; needs the monitor on): the device keeps the newest `rows` finished rows, a row being the
 * mean (and, with MAXHOLD, the max-hold) over the blocks of one interval -- what a waterfall or an rtl_power line is made of.  The
 * caller closes intervals with a call that touches no device and collects finished rows whenever it likes, with a read that never
 * waits for a kernel stream; an interval is not lost because it was not read at its boundary.  There is no copy on the device: the
 * monitor's launch adds every block's band powers into the open row's slot of a ring in HBM as well as into the accumulators of
 * hfdl_gpu_frontend_spectrum_read() (8 .. 12 more bytes per band and block, no launch of its own), and closing a row moves a host
 * index: the next block starts the next slot over.
 *   Rows are numbered from 0 at every hfdl_gpu_frontend_spectrum_history() call; row i covers the blocks pushed between close i - 1
 *   and close i ("block" as for the monitor: channelize_block counts, push_baseband does not), the same blocks for every receiver.
 *   A row's mean and peak are BIT-IDENTICAL to what hfdl_gpu_frontend_spectrum_read(rx, reset = 1) returns for the same blocks: the
 *   same compensated sums on the device, the same division on the host.
 *   The two are independent: spectrum_read() and its per-receiver reset behave exactly as without the history, closing a row does
 *   not touch the read's accumulators, a read's reset does not touch the open row.
 *   A row is finished when the monitor launch of its last block has run.  Row i + rows overwrites row i from its first block on; a
 *   row overwritten before it was collected is gone, and the caller sees it by info[0].row > from_row -- nothing fails.
 *   hfdl_gpu_frontend_spectrum_enable() called again (bins = 0 included) drops the history: call spectrum_history() again after it.
 * One thread drives a front end, as everywhere in this header: no collection runs while a push re-targets a slot. */
#define HFDL_GPU_SPECTRUM_ROWS_MAX 1024
typedef struct {
	uint64_t row;                    /* index of the row */
	uint64_t first_block;            /* its first block, in the numbering of hfdl_gpu_frontend_counters().blocks */
	uint32_t blocks;                 /* T: the blocks it covers (>= 1) */
	uint32_t pad;
} hfdl_gpu_spectrum_row;
/* rows = 0: history off, its buffers freed.  rows = 2 .. HFDL_GPU_SPECTRUM_ROWS_MAX: keep the newest `rows` rows (the newest rows - 1
 * once the open row has a block: it lives in the ring too).  interval_blocks > 0: a row closes by itself after that many blocks;
 * 0: only hfdl_gpu_frontend_spectrum_row_close() closes rows.  Calling it again starts over at row 0 with an empty ring (it waits for
 * the monitor launches queued so far before the old ring goes).  HFDL_GPU_EINVAL (rows outside 0, 2 .. 1024, interval_blocks < 0,
 * null handle, monitor off) / HFDL_GPU_ERANGE (rows x receivers x bins x 12 bytes above 1 GiB) are checked before any device work;
 * HFDL_GPU_ENOMEM leaves the history off and the monitor as it was. */
int  hfdl_gpu_frontend_spectrum_history(hfdl_gpu_frontend *fe, int32_t rows, int32_t interval_blocks);
/* End the open row: host bookkeeping only, no device call, no wait.  *row = the open row's index, which is the index of the row this
 * call finishes.  An open row without a block stays open: the call makes no row, and the next close returns the same index. */
int  hfdl_gpu_frontend_spectrum_row_close(hfdl_gpu_frontend *fe, uint64_t *row);
/* Consecutive finished rows of receiver rx from max(from_row, oldest row kept) on, at most max_rows of them: mean[i * bins + b], peak
 * likewise (may be NULL; HFDL_GPU_EINVAL if asked for without MAXHOLD) and info[i] of the i-th row returned; *n = rows written,
 * *next_row = what to pass as from_row next time.  max_rows = 0 writes nothing and reports *next_row, *n = 0.
 * wait = 0: only rows whose last launch has already run -- the call asks (hipEventQuery) and never waits for a kernel stream; the open
 * row and closed rows still in flight come with a later call.  wait != 0: waits for every closed row it returns (like
 * spectrum_read(), for the device to catch up to that row's last block).  The rows are copied on the collection stream through a
 * page-locked buffer beside the kernels in flight; the call returns when that copy is done.  HFDL_GPU_EINVAL (null handle, n or
 * next_row, history off, rx out of range, max_rows < 0, mean or info null with max_rows > 0) is checked before any device work. */
int  hfdl_gpu_frontend_spectrum_rows(hfdl_gpu_frontend *fe, int32_t rx, uint64_t from_row, int32_t max_rows,
		float *mean, float *peak, hfdl_gpu_spectrum_row *info, int32_t *n, uint64_t *next_row, int wait);

/* Channel baseband export (off by default: nothing is allocated or launched): the channelizer's output of SELECTED channels, every
 * sample of it, as a stream the caller collects without waiting -- for recording a channel, feeding another decoder, or looking at a
 * constellation.  Behind the inverse FFT / NCO launch of every closed half, one launch packs the selected channels' rows of the half's
 * blocks into a ring of ring_blocks blocks in HBM; block b (in the numbering of hfdl_gpu_frontend_counters().blocks; "block" as for the
 * spectrum monitor: a push or a channelize_block, not push_baseband) lives in slot b mod ring_blocks, so a block not collected
 * within ring_blocks blocks is overwritten, and a half larger than the ring overwrites its own oldest blocks.  Per block and selected
 * channel s (channel channels[s], P = geometry.max_outputs_per_block):
 *   samples[s][0 .. P)   the counts[s] valid samples -- bit for bit what HFDL_GPU_TAP_CHAN_OUT reads -- then zeros.  CF32: float re, im.
 *                        CS16: int16 re, im; per component r = rintf(v * scale) (one fp32 multiply, round half to even), |r| > 32767
 *                        stored as +-32767, NaN stored as 0, both counted in clipped[s];
 *   power[s]             mean of re^2 + im^2 over the valid samples in fp32 (0 without any), summed in a fixed order: bit-identical
 *                        from run to run and independent of how the caller pushes, polls or batches. */
#define HFDL_GPU_EXPORT_CF32 0
#define HFDL_GPU_EXPORT_CS16 1
#define HFDL_GPU_EXPORT_RING_MAX 4096
typedef struct { uint64_t block; } hfdl_gpu_export_block;      /* index in the numbering of counters().blocks */
/* channels[nsel]: distinct global channel indices in any order -- the order of the exported rows; nsel = 0 turns the export off and
 * frees its buffers.  ring_blocks: 2 .. HFDL_GPU_EXPORT_RING_MAX.  scale: CS16 only, finite and > 0.  The first exported block is the
 * first one pushed after the call (a block already waiting in the half being filled is not exported; no half is closed).  Calling it
 * again starts over with an empty ring (it waits for the export launches queued so far before the old ring goes).  HFDL_GPU_EINVAL
 * (null handle, null channels with nsel > 0, nsel < 0 or above the channel count, a channel out of range or repeated, unknown
 * format, bad scale, ring_blocks out of range) / HFDL_GPU_ERANGE (ring above 1 GiB) are checked before any device work;
 * HFDL_GPU_ENOMEM leaves the export as it was. */
int  hfdl_gpu_frontend_export_enable(hfdl_gpu_frontend *fe, const int32_t *channels, int32_t nsel,
		int format, float scale, int32_t ring_blocks);
/* Consecutive finished blocks from max(from_block, oldest block kept) on, at most max_blocks: samples[i][s][P] elements of the enabled
 * format, counts[i * nsel + s], power and clipped likewise (each may be NULL), info[i].block; *n = blocks written, *next_block = what
 * to pass as from_block next time.  A block overwritten before it was collected shows as info[0].block > from_block -- nothing fails.
 * max_blocks = 0 writes nothing and reports *next_block, *n = 0.  A block is finished when the export launch of its half has run.
 * wait = 0: only such blocks -- the call asks (hipEventQuery) and never waits for a kernel stream.  wait != 0: waits for the newest
 * export launch ALREADY QUEUED; it closes nothing, so blocks still in the half being filled come with a later call (after a sync, a
 * poll, or the push that fills the half).  The copy runs on the collection stream through a page-locked buffer beside the kernels in
 * flight; the call returns when it is done.  One thread drives a front end: no copy of a slot is in flight while a push re-targets
 * it.  HFDL_GPU_EINVAL (null handle, n or next_block, export off, max_blocks < 0, samples, counts or info null with max_blocks > 0)
 * is checked before any device work. */
int  hfdl_gpu_frontend_export_read(hfdl_gpu_frontend *fe, uint64_t from_block, int32_t max_blocks,
		void *samples, int32_t *counts, float *power, uint32_t *clipped, hfdl_gpu_export_block *info,
		int32_t *n, uint64_t *next_block, int wait);

/* Retune one channel of a running front end (HFDL ground stations change their active frequencies every few hours): blocks pushed
 * before the call are channelized, demodulated and labelled with the old frequency, blocks pushed after it with new_freq_hz -- a frame
 * that finished before the call keeps the old `freq` however late it is polled.  From the call on, `channel` is a freshly created
 * channel: filter taps and channelizer constants are what a create with new_freq_hz in its place computes, bit for bit; NCO, AGC,
 * timing, carrier, equaliser, framer and the per-channel counters (symbol_cnt included) start over.  Only sample_cnt goes on -- a PDU's
 * sample_index stays the position in the stream.  Every other channel, the spectrum monitor and the export are untouched, bit for bit;
 * an exported channel keeps exporting, on the new frequency.  The call closes the half being filled (as a sync does) but drains
 * nothing and waits for no kernel: its only wait is for one of two page-locked tap buffers, i.e. for the retune two calls ago.  The
 * first call also allocates -- two buffers of fft_size cf32 (cfg3: 128 MiB), kept -- which may take what an allocation takes; a front
 * end that is never retuned allocates and launches nothing for it.  hfdl_gpu_frontend_all_channel_stats(), which waits for nothing,
 * reports the channel's counters as a fresh channel's from the call on (never the old ones first: the device's own reset runs
 * behind the demodulators in flight), sample_cnt as it goes on.  HFDL_GPU_EINVAL -- null handle, channel out of range, new_freq_hz outside +-fs/2 of the centre of the
 * channel's own receiver, a frequency another channel of that receiver listens on, a shift the planner refuses, a front end created
 * with HFDL_GPU_FOLD_PRUNE (its row windows depend on the pass bands) -- is checked before any device work, and a refusal, like an
 * HFDL_GPU_ENOMEM of the first call, leaves the front end as it was.  One channel per call. */
int  hfdl_gpu_frontend_retune_channel(hfdl_gpu_frontend *fe, int32_t channel, int32_t new_freq_hz);

/* Frame quality records (off by default: nothing is allocated or launched): how well a frame was received, measured on the equalised
 * data symbols the burst decoder sliced -- rssi_db, noise_floor_db and freq_err_hz of a PDU describe the channel in front of the
 * equaliser.  Behind the burst decoder of every demodulator launch, on its stream, one more kernel makes a record for every frame
 * of the launch's frame queue -- also for a frame whose PDU was dropped from a full PDU ring -- in a ring of ring_frames records in HBM.  A
 * record belongs to the PDU with the same (channel, sample_index); the order of the records of one launch is unspecified.  With
 * p[i] the constellation point nearest to data symbol x[i] (the decoder's own slicer and table) and e[i] = x[i] - p[i], in fp32:
 *   seg_err_power[s]   mean |e|^2 over the 30 symbols of data segment s, s < segments; +0.0 above (a frame lasts 2.3 - 4.2 s and fades)
 *   err_power          mean of seg_err_power[0 .. segments); MER in dB = -10 log10(err_power)
 *   err_max            max |e|^2;   sym_power   mean |x|^2;   gain_re + j gain_im   mean x conj(p)
 * summed in a fixed order (dumphfdl_amd/csrc/quality.h): bit-identical from run to run and independent of how the caller pushes,
 * polls or batches.  The figures are DECISION-DIRECTED: below about the SNR where the slicer starts to err, a wrong decision counts
 * the distance to the wrong, nearer point, err_power saturates and overstates the quality.  sym_power - |gain|^2 is the gain- and
 * phase-corrected error power for who wants it.  The symbols are taken as stored, in front of the descrambler: descrambler and
 * bitmask_lsb multiply a symbol by +-1, which maps every HFDL constellation onto itself and changes none of the figures. */
#define HFDL_GPU_QUALITY_SYMBOLS       1u     /* keep each frame's data symbols too */
#define HFDL_GPU_QUALITY_SEGMENTS_MAX  168
#define HFDL_GPU_QUALITY_SYMBOLS_MAX   5040
#define HFDL_GPU_QUALITY_RING_MAX      65536
typedef struct {
	uint64_t sample_index;                  /* = the PDU's */
	int32_t  channel, freq, mode, bitmask_lsb;
	int32_t  nsym, segments;
	int32_t  train_bits_bad, train_bits_total;
	float    freq_err_hz, rssi_db, noise_floor_db;    /* bit for bit the PDU's */
	float    sym_power, err_power, err_max, gain_re, gain_im;
	float    seg_err_power[HFDL_GPU_QUALITY_SEGMENTS_MAX];
} hfdl_gpu_frame_quality;                   /* 744 bytes */
/* ring_frames = 0: off, the buffers freed.  ring_frames = 2 .. HFDL_GPU_QUALITY_RING_MAX: on, from the next demodulator launch
 * QUEUED (frames of halves handed to the demodulator before the call get no record); the call closes no half and drains nothing.
 * flags: HFDL_GPU_QUALITY_SYMBOLS adds a second ring of ring_frames x 5040 cf32 (40 320 bytes a frame).  A frame that finds the ring
 * full is dropped and counted, never left half-written, and leaves no hole; reading makes room.  Calling it again starts over with
 * an empty ring and a dropped count of 0 (it waits for the quality launches queued so far before the old ring goes).
 * HFDL_GPU_EINVAL (null handle, unknown flag, ring_frames outside 0, 2 .. 65536) / HFDL_GPU_ERANGE (rings above 1 GiB) are checked
 * before any device work; HFDL_GPU_ENOMEM leaves the feature as it was. */
int  hfdl_gpu_frontend_quality_enable(hfdl_gpu_frontend *fe, int32_t ring_frames, uint32_t flags);
/* The oldest records not read yet, at most max_frames: out[i], and with `symbols` (may be NULL; HFDL_GPU_EINVAL if given without
 * HFDL_GPU_QUALITY_SYMBOLS) the frame's data symbols at symbols[i * 2 * 5040 ..], re, im, zeros past nsym; *n = records written,
 * *dropped (may be NULL) = frames dropped since the enable.  wait = 0: only records known to be complete -- those of launches whose
 * burst decoders are known to be done, as for hfdl_gpu_frontend_poll_pdus_ready(.., 2); the call asks (hipEventQuery) and never
 * waits for a kernel stream.  After a sync or a draining poll that is every record of every frame decoded so far.  wait != 0: first
 * does what hfdl_gpu_frontend_sync() does.  The records are copied on the collection stream through a page-locked buffer beside
 * the kernels in flight.  HFDL_GPU_EINVAL for a null n, max_frames < 0 or a null out with max_frames > 0 is returned before the
 * handle is looked at and nothing is written; a null handle, the feature off or `symbols` without the flag likewise before any
 * device work. */
int  hfdl_gpu_frontend_quality_read(hfdl_gpu_frontend *fe, hfdl_gpu_frame_quality *out, float *symbols,
		int32_t max_frames, int32_t *n, uint32_t *dropped, int wait);

/* Wideband impulse-noise blanker (off by default: nothing is allocated or launched, and the block path is the one it is without it).
 * Lightning static, power lines and switching supplies put microsecond impulses 30 - 50 dB above everything else into the raw samples; a
 * channel filter of up to 2^20 + 1 taps stretches each over tens of symbols of every channel at once, so the one place to fight them is
 * in front of the forward FFT.  The rule is stateless per block and per receiver (dumphfdl_amd/csrc/blanker.h): with P the mean of
 * |x|^2 over the input_size NEW samples of a receiver's block, after the sample-format conversion, in fp32 and in one fixed order, and
 * T = k2 P, k2 = (float)10^(threshold_db / 10), a sample with |x|^2 > T enters the transform as (0, 0).  Every sample is judged once,
 * when it is new (the overlap history holds blanked values); at most a fraction 1 / k2 of a block can be blanked (Markov: 4 % at 14 dB,
 * 25 % at 6 dB), so a level jump never blanks a whole block and nothing can get stuck; a block whose P is NaN or Inf is not blanked.
 * Results do not depend on how blocks are pushed, polled or batched.  The spectrum monitor and tap 1 see the blanked spectra; retune,
 * export and quality records are untouched.  It works with every entry point that takes wideband input (push_block, push_block_raw,
 * push_blocks_raw, channelize_block, prefetched blocks; host and device-resident input); push_baseband has no wideband input.
 * Cost: two launches per step in front of the forward FFT, on its stream -- the block is read twice in its own format and written and
 * read once more as cf32.
 * threshold_db: 0 = off; 6 .. 60 = on from the next pushed block, for every receiver.  The first enable allocates (nrx x input_size
 * cf32, kept until the front end is destroyed) and may take what an allocation takes; later calls change the threshold alone and wait
 * for nothing.  HFDL_GPU_EINVAL (any other threshold_db, NaN included; null handle) is returned before any device work. */
int  hfdl_gpu_frontend_blanker_enable(hfdl_gpu_frontend *fe, float threshold_db);
typedef struct {
	uint64_t blocks, samples_blanked;       /* blocks blanked and samples zeroed of this receiver since the first enable */
	float    last_power, last_threshold;    /* P and T of its newest blanked block */
} hfdl_gpu_blanker_stats;
/* Receiver rx's record.  Waits as hfdl_gpu_frontend_spectrum_read() does -- for the blanker launches queued so far, on the collection
 * stream -- and queues nothing on the kernels' streams.  No block blanked yet: all zero.  HFDL_GPU_EINVAL: null argument, rx out of
 * range, or a front end whose blanker was never enabled. */
int  hfdl_gpu_frontend_blanker_stats(hfdl_gpu_frontend *fe, int32_t rx, hfdl_gpu_blanker_stats *out);

/* Wideband I/Q imbalance and DC corrector (off by default: nothing is allocated or launched, and the block path differs by one host
 * branch).  A zero-IF receiver whose I and Q arms differ in gain and phase delivers x = s + kappa conj(s) + m: every signal at +f leaves
 * an image at -f, 25 to 40 dB down, and a spike at 0 Hz.  Behind a channel filter the image of a broadcast station is in-band signal on
 * an HFDL channel; in front of the forward FFT, removing it is one complex multiply per sample.  The rule (dumphfdl_amd/csrc/iqbal.h)
 * is per receiver and feed-forward: running averages, with weight alpha per block (the cumulative mean before that), of the means of x,
 * x^2 and |x|^2 over the input_size NEW samples of each block -- after the sample-format conversion and after the blanker -- give
 * m, C = E (x - m)^2 and P = E |x - m|^2; kappa = C / (P + sqrt(P^2 - |C|^2)), exact for a proper s; block b enters the transform as
 * d - kappa conj(d), d = x - m, with the estimate from the blocks BEFORE b.  A block without an estimate -- the first after an enable,
 * P not positive or not finite, or |C| > 0.5 P: a real-valued stream, which the rule must never cancel against itself -- is copied word for
 * word and counted as refused.  A block whose sums are not all finite leaves the estimate as it was.  fp32, in one fixed order: results do
 * not depend on how blocks are pushed, polled or batched.  The spectrum monitor and tap 1 see the corrected spectra; retune, export,
 * quality records and the carrier canceller are untouched.  It works with every entry point that takes wideband input.
 * One complex kappa per receiver corrects the part of the imbalance that is flat over the band.
 *
 * alpha 2^-10 .. 1 turns receiver rx (-1: every receiver) on from the next pushed block, 0 off; turned on again, the estimate starts
 * afresh.  1/8 is the tested value: kappa within 1 % after one block of the tested scenario.  The first enabling call allocates (one
 * block of cf32 per receiver, kept until the front end is destroyed); later calls wait for nothing, except that turning a receiver on
 * again after a seed waits for the corrector launches queued so far.  HFDL_GPU_EINVAL (any other alpha, NaN included; null handle; rx out
 * of range) is returned before any device work. */
int  hfdl_gpu_frontend_iqbal_enable(hfdl_gpu_frontend *fe, int32_t rx, float alpha);
/* Presets (kappa, DC) of receiver rx (-1: every receiver) from its next pushed block.  hold = 1: a fixed, calibrated correction that no
 * block changes; hold = 0: the estimator starts from them as if one block had been seen.  Waits for the corrector launches queued so far.
 * HFDL_GPU_EINVAL, before any device work: |kappa| > 0.25, a value that is not finite, hold not 0 or 1, null handle, rx out of range, a
 * corrector that was never enabled or is off for the receiver. */
int  hfdl_gpu_frontend_iqbal_seed(hfdl_gpu_frontend *fe, int32_t rx, float kappa_re, float kappa_im, float dc_re, float dc_im, int hold);
typedef struct {
	uint64_t blocks, refused;               /* blocks of this receiver that went through the corrector since the first enable; those copied */
	float    kappa_re, kappa_im;            /* what its newest block was corrected with (valid), else 0 */
	float    dc_re, dc_im;
	float    power;                         /* P of that estimate (0 under a seed or a hold) */
	float    image_rejection_db;            /* -20 log10 |kappa|: how far below its signal the uncorrected image lies (valid; kappa = 0: +Inf) */
	uint32_t valid, hold;                   /* the newest block was corrected; with a held preset */
} hfdl_gpu_iqbal_stats;
/* Receiver rx's record.  Waits as hfdl_gpu_frontend_blanker_stats() does -- for the corrector launches queued so far, on the collection
 * stream -- and queues nothing on the kernels' streams.  No block yet: all zero.  HFDL_GPU_EINVAL: null argument, rx out of range, or a
 * front end whose corrector was never enabled. */
int  hfdl_gpu_frontend_iqbal_stats(hfdl_gpu_frontend *fe, int32_t rx, hfdl_gpu_iqbal_stats *out);

/* Adaptive carrier canceller per channel (off by default: nothing is allocated or launched, and the block path differs by one host
 * branch).  Steady carriers inside a channel's 2.4 kHz passband -- broadcast and utility carriers, CW, receiver birdies -- pass the
 * channel filter, and a tone a few dB above the burst defeats the preamble search and the slicer.  Between the channelizer's output and
 * the demodulator, a selected channel runs a normalised-LMS line canceller (dumphfdl_amd/csrc/notch.h): 32 complex taps predict the
 * sample from the channel's own past 24 samples back, the prediction is taken away, and the taps follow with step mu / (power in the
 * delay line).  fp32 in one fixed order; the state is carried sample by sample across blocks, so results do not depend on how blocks
 * are pushed, polled or batched.  A sample that is not finite never reaches the taps; taps whose energy is not finite or exceeds 4 at
 * the end of a block are set to zero and the event is counted: nothing can stay stuck.  One such reset is to be expected where a
 * channel's samples begin out of nothing: enabled before a front end's first block, the canceller meets the channel filter's start-up
 * ramp (some 60 samples rising from 1e-9 to the signal's level), the normalised step runs away on it, that block's row is spoilt and
 * the reset at its end puts the channel right.
 * What sees what: the channel export and HFDL_GPU_TAP_CHAN_OUT read the raw channel (the canceller writes a buffer of its own, of
 * the channelizer output's size: 224 MiB at 40 Msps / 256 channels); the spectrum monitor sees nothing of it; demodulator, burst decoder,
 * HFDL_GPU_TAP_NOTCH_OUT and the frame quality records see the cancelled samples.  An unselected channel's samples reach the demodulator
 * word for word.  It applies to every half that goes to the demodulator, hfdl_gpu_frontend_push_baseband()'s included.  A retuned channel
 * meets a fresh canceller.  Cost: one launch per half on the demodulator's stream.
 * mu: 0 = off; 1e-5 .. 0.05 = on.  channels NULL / nsel 0 = every channel.  Every call replaces the selection and restarts every selected
 * channel from zero state; like a retune it closes the half being filled: blocks pushed before the call are untouched, blocks pushed
 * after it meet the new setting.  The first enable allocates.  HFDL_GPU_EINVAL (any other mu, NaN included; a null handle; a channel out
 * of range or listed twice) is returned before any device work. */
#define HFDL_GPU_NOTCH_STATE_FLOATS 174      /* 32 taps (re, im), then the last 55 inputs (re, im), newest first */
int  hfdl_gpu_frontend_notch_enable(hfdl_gpu_frontend *fe, const int32_t *channels, int32_t nsel, float mu);
typedef struct {
	uint64_t blocks, resets;                                  /* rows cancelled, tap resets, since the enable */
	float    last_in_power, last_out_power, tap_energy;       /* sum |x|^2, sum |y|^2 (sample order, fp32) and sum |w|^2 of the newest row */
} hfdl_gpu_notch_stats;
/* A selected channel's record.  Waits as hfdl_gpu_frontend_blanker_stats() does -- for the canceller launches queued so far, on the
 * collection stream -- and queues nothing on the kernels' streams.  Nothing cancelled since the enable: all zero.  HFDL_GPU_EINVAL: null
 * argument, channel out of range or not selected, or a front end whose canceller was never enabled. */
int  hfdl_gpu_frontend_notch_stats(hfdl_gpu_frontend *fe, int32_t channel, hfdl_gpu_notch_stats *out);

/* stage taps -- the DATADUMPS analogue (src/hfdl.c:616-644): copy an intermediate buffer to host */
enum {
	HFDL_GPU_TAP_SPECTRUM = 1,       /* cf32[fft_size], fftshifted forward FFT (shared.buf after src/fft.c:59) */
	HFDL_GPU_TAP_FILTER = 2,         /* cf32[fft_size], filtertaps_fft of `channel` */
	HFDL_GPU_TAP_CHAN_OUT = 3,       /* cf32[<= max_outputs_per_block], fastddc_inv_cc output of `channel` */
	HFDL_GPU_TAP_RESAMPLED = 4,      /* cf32[n], msresamp output of the last block */
	HFDL_GPU_TAP_MF_OUT = 5,         /* cf32[n], AGC + matched filter output of the last block */
	HFDL_GPU_TAP_SYMBOLS = 6,        /* cf32[n], equalised on-time symbols of the last block */
	HFDL_GPU_TAP_AGC_LEVEL = 7,      /* f32[n], agc signal level per 5400-sps sample */
	HFDL_GPU_TAP_NCO_PHASORS = 9,    /* cf32[n]: the NCO phasors (cos phi_k, sin phi_k) that multiplied the last block's outputs of `channel`
	                                    (decimating_shift_addition_cc's recurrence, src/libcsdr_gpl.c:48-66; bit-exact vs the reference) */
	HFDL_GPU_TAP_NOTCH_OUT = 10,     /* cf32[<= max_outputs_per_block]: the row of `channel` the demodulator read with the carrier canceller on (a selected
	                                    channel: cancelled; another: tap 3's words); `back` as for tap 3.  HFDL_GPU_EINVAL while the canceller is off */
	HFDL_GPU_TAP_PHASE_CYCLES = 8    /* f32[4]: shader cycles of the last demod launch: resampler phase, the whole four-wave pipelined phase (wall),
	                                    busy cycles of the timing-recovery wave, busy cycles of the carrier / equaliser / framer wave */
};
/* Stage taps 4..8 make the demodulator write its intermediate samples to HBM every launch; on by default (tests), a
 * production caller / the bench turns them off.  Taps 1..3 are always available (they are the kernels' own buffers).  Taps 4..8 hold
 * the LAST demodulator launch: one block when the caller syncs / polls after every push, up to geometry.demod_batch blocks otherwise
 * (size buffers for demod_batch * (post_input_size + 64) complex samples); tap 3 and tap 9 hold the last block. */
int  hfdl_gpu_frontend_enable_taps(hfdl_gpu_frontend *fe, int enable);
/* dst holds `cap` floats; *n_floats receives the number written */
int  hfdl_gpu_frontend_read_tap(hfdl_gpu_frontend *fe, int what, int32_t channel, float *dst, size_t cap, size_t *n_floats);
/* taps 1, 3 and 9 of the block `back` blocks before the newest one (0 = read_tap): the channelizer keeps the blocks of the newest half
 * -- what was pushed since the half before it filled (geometry.fold_batch blocks, or max(fold_batch, demod_batch)) or since the last
 * sync / poll; HFDL_GPU_ERANGE beyond that */
int  hfdl_gpu_frontend_read_tap_block(hfdl_gpu_frontend *fe, int what, int32_t channel, int32_t back, float *dst, size_t cap, size_t *n_floats);

/* timing of the dominant kernel (fold) measured with HIP events on the front end's stream; a launch folds up to geometry.fold_batch
 * blocks: hfdl_gpu_frontend_fold_blocks() = the blocks the timed launches covered */
int  hfdl_gpu_frontend_fold_time_ms(hfdl_gpu_frontend *fe, double *total_ms, int64_t *launches);
int  hfdl_gpu_frontend_fold_blocks(hfdl_gpu_frontend *fe, int64_t *blocks);
/* timed fold launches by block count: counts[nb] = launches that folded nb blocks (nb = 1 .. HFDL_GPU_FOLD_BATCH_MAX; counts[0] unused)
 * since the timers were reset, ms[nb] (may be NULL) = their kernel time -- what a caller needs to price the launches it timed (a launch
 * of up to 4 blocks runs the four-column form of the kernel and is bound by the HBM reads of the taps, one of 5 .. 16 the sixteen-column
 * form, one of 17 .. 32 the thirty-two-column form: every loaded tap operand multiplies two spectrum operands) */
int  hfdl_gpu_frontend_fold_launch_shapes(hfdl_gpu_frontend *fe, int64_t counts[HFDL_GPU_FOLD_BATCH_MAX + 1], double ms[HFDL_GPU_FOLD_BATCH_MAX + 1]);
int  hfdl_gpu_frontend_reset_timers(hfdl_gpu_frontend *fe, int enable);
/* the same for the demodulator kernel (the kernel that bounds the small geometries), from its dispatch's own start / stop events;
 * *blocks = the blocks those launches covered (a launch takes up to geometry.demod_batch blocks) */
int  hfdl_gpu_frontend_demod_time_ms(hfdl_gpu_frontend *fe, double *total_ms, int64_t *launches, int64_t *blocks);
/* kernel time by stage since the timers were reset, from start / stop events that ride on the dispatches themselves:
 * ms / launches [0] forward FFTs (first pass start -> last pass stop, one per block), [1] fold launches, [2] inverse FFT / NCO launches
 * (one per half) -- together the channelizer's stream; [3] demodulator launches -- their own stream; [4] burst decoder launches -- theirs.
 * Kernels of different streams overlap: the sums say which stream bounds a half, not what a block costs. */
int  hfdl_gpu_frontend_stage_times(hfdl_gpu_frontend *fe, double ms[5], int64_t launches[5]);
/* steady-state period of one block: (start of the last timed fold launch - start of the first) / (blocks folded by all timed launches
 * but the last), free of the pipeline fill before the first block and the demodulator / burst-decoder drain after the last */
int  hfdl_gpu_frontend_step_period_ms(hfdl_gpu_frontend *fe, double *period_ms);
/* ---- stage-level entry points (host pointers; allocate / copy / free internally) ---- */

/* out[(k + n/2) mod n] = sum_t in[t] e^{-2 pi i k t / n} when shifted != 0 (plain order otherwise); n = power of two >= 512 */
int  hfdl_gpu_fft_forward(int device, const float *in, float *out, int32_t n, int shifted);
/* K=7 r=1/2 Viterbi on `nframes` frames of equal size: soft = nframes * 2*nbits bytes; out = nframes * ceil(nbits/8) */
int  hfdl_gpu_viterbi27(int device, const uint8_t *soft, int32_t nbits, int32_t nframes, uint8_t *out);
/* decode_user_data for a batch: symbols = nframes * (segments*30) equalised data symbols (cf32), one mode and
 * bitmask bit per frame; octets = nframes * HFDL_GPU_PDU_MAX_OCTETS, lens[nframes] */
int  hfdl_gpu_burst_decode(int device, const float *symbols, const int32_t *modes, const int32_t *bitmask_lsb,
		int32_t nframes, uint8_t *octets, int32_t *lens);
/* the blanker (hfdl_gpu_frontend_blanker_enable above) alone, by the device functions of the front end: raw = n samples
 * (1 .. 2^24) of sample_format; out = the n cf32 samples as they would enter the transform, *power = P, *blanked = samples zeroed.
 * threshold_db 6 .. 60.  Every argument is checked before a device is selected. */
int  hfdl_gpu_blank_block(int device, const void *raw, int32_t n, int sample_format, float threshold_db,
		float *out, float *power, uint64_t *blanked);
/* the I/Q corrector (hfdl_gpu_frontend_iqbal_enable above) alone, by the kernel of the front end, on nblocks (1 .. 64) consecutive
 * blocks of n samples (1 .. 2^24) of one receiver from a fresh enable: raw = nblocks * n samples of sample_format; alpha 2^-10 .. 1;
 * seed = NULL, or kappa_re, kappa_im, dc_re, dc_im given before the first block (hold as above; 0 without a seed).  out = the
 * nblocks * n cf32 samples as they would enter the transform, records[b] = the record after block b.  Every argument is checked before a
 * device is selected. */
int  hfdl_gpu_iqbal_blocks(int device, const void *raw, int32_t n, int32_t nblocks, int sample_format, float alpha,
		const float *seed, int hold, float *out, hfdl_gpu_iqbal_stats *records);
/* the carrier canceller (hfdl_gpu_frontend_notch_enable above) alone, by the kernel of the front end: x, y = [nch][n] cf32, every row a
 * channel's next n samples; state = [nch][HFDL_GPU_NOTCH_STATE_FLOATS], in and out, NULL = fresh and discarded.  mu 1e-5 .. 0.05.
 * Every argument is checked before a device is selected. */
int  hfdl_gpu_notch_rows(int device, const float *x, int32_t nch, int32_t n, float mu, float *state, float *y);
/* the frame quality figures (hfdl_gpu_frame_quality above) of a batch, by the device function of the front end's records: symbols
 * and modes as for hfdl_gpu_burst_decode; out[nframes].  mode, nsym, segments and the five figures with seg_err_power are filled;
 * what only a front end knows (sample_index, channel, freq, bitmask_lsb, the training counts, the three channel fields) is 0. */
int  hfdl_gpu_frame_quality_batch(int device, const float *symbols, const int32_t *modes, int32_t nframes,
		hfdl_gpu_frame_quality *out);

/* decimating_shift_addition_cc(input, output, input_size, decimating_shift_addition_init(rate, decimation), decimation, status)
 * (src/libcsdr_gpl.c:26-74): out[k] = in[remain + decimation k] e^{j phi_k} with the reference's fp32 phasor recurrence; the
 * status fields (*decimation_remain, *starting_phase) are read and updated, *output_size receives k.  `out` holds
 * ceil(input_size / decimation) complex samples.  This is the device code the channelizer runs after its inverse FFT. */
int  hfdl_gpu_nco_decimate(int device, const float *in, int32_t input_size, float rate, int32_t decimation,
		int32_t *decimation_remain, float *starting_phase, float *out, int32_t *output_size);
/* crc16_ccitt(data, len, crc_init) of src/crc.c:4-47, computed by the device function the burst decoder checks every FCS with */
int  hfdl_gpu_crc16_ccitt(int device, const uint8_t *data, uint32_t len, uint16_t crc_init, uint16_t *crc);
/* header triage of `npdus` decoded PDUs, PDU i = octets[i * stride .. + lens[i]): fcs_status[i] = HFDL_GPU_FCS_*,
 * pdu_kind[i] = HFDL_GPU_KIND_*, hdr_len[i] = octets covered by the FCS (what burst decoding fills into hfdl_gpu_pdu) */
int  hfdl_gpu_pdu_triage(int device, const uint8_t *octets, const int32_t *lens, int32_t npdus, int32_t stride,
		uint8_t *fcs_status, uint8_t *pdu_kind, uint16_t *hdr_len);

/* the LPDU list walk of `npdus` PDUs (must be MPDUs or SPDUs as they come out of the decoder): counts[i * 5 + 0..4] = lpdus processed,
 * good, bad FCS, too short, truncated flag -- zeros when the header triage of PDU i is not "FCS good" */
int  hfdl_gpu_lpdu_walk(int device, const uint8_t *octets, const int32_t *lens, int32_t npdus, int32_t stride, uint8_t *counts);

/* The carrier loop's slicer on `n` equalised symbols (interleaved re, im): modem_demodulate of liquid's PSK modem (arity 1..3 bits
 * per symbol: the Gray-coded symbol) and its demodulator phase error Im(x conj(x_hat)), src/hfdl.c:737-741.  The device decides by
 * the nearest constellation point (largest Re(x conj(p))), which is what arg() + the reference ladder computes; the two can differ
 * only for x within rounding of a decision boundary. */
int  hfdl_gpu_psk_slice(int device, int32_t arity, const float *xy, int32_t n, uint32_t *sym, float *phase_error);

/* kernel time in ms of the last hfdl_gpu_fft_forward / _viterbi27 / _burst_decode call made by this thread (HIP events
 * around the launch; allocation and host <-> device copies excluded) */
double hfdl_gpu_last_stage_ms(void);

const char *hfdl_gpu_last_error(void);
int  hfdl_gpu_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
