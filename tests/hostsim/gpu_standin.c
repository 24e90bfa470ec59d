/* gpu_standin.c -- a host-memory stand-in for libhfdl_gpu.so, for running the host library's front-end thread (host/frontend.c)
 * on a CPU: exactly the hfdl_gpu_* entry points the host library references, plain C11, no device, no threads of its own.
 *
 * It models what the thread's bookkeeping can get wrong, not the signal path:
 *   - pinned memory is malloc plus a registry; a prefetch of memory outside the registry is refused, and a push behind a prefetch
 *     must name the oldest prefetched pointer;
 *   - the copy engine reads LATE: a queued copy looks at the caller's memory only when it is first reported complete
 *     (input_copied after HFDL_STANDIN_COPY_LAG "not yet" answers, input_done / input_done_upto, a draining poll), and then hashes
 *     the block (FNV-1a 64).  A ring slot handed back to the producer too early is hashed with the producer's newer bytes in it;
 *   - every pushed block yields one 16-octet PDU on channel 0: host block number, then that hash (both little endian), with
 *     sample_index = block number x block length, marked as an MPDU of two LPDUs, one good and one with a bad FCS.
 *     poll_pdus_ready delivers only blocks whose copy is complete.  The number is the HOST block number (copies queued, pushed or
 *     prefetched), not a count of pushes: blocks dropped by prefetch_cancel keep theirs, so later PDUs show a gap, as with the real library;
 *   - a closed spectrum row and an exported block are "finished" one push later: wait = 0 right after the push that made them
 *     returns nothing, wait = 1 returns everything;
 *   - destroy aborts, with one line on stderr, if a prefetched block was left unpushed without a cancel or the front end is not a
 *     live one; host_free aborts likewise on memory it does not own.
 *
 * Read from the environment at create:
 *   HFDL_STANDIN_PREFETCH     0 .. HFDL_GPU_PREFETCH_MAX: geometry.prefetch_depth (default 0)
 *   HFDL_STANDIN_COPY_LAG     L >= 0: input_copied says "not yet" the first L times it is asked about a block (default 0)
 *   HFDL_STANDIN_FAIL_PUSH    k >= 1: the k-th push fails with HFDL_STANDIN_FAIL_TEXT in hfdl_gpu_last_error()
 *   HFDL_STANDIN_FAIL_CREATE  text: create fails with it */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hfdl_gpu.h"

#define BLOCK_SAMPLES 3072
#define FFT_SIZE 4096
#define OUT_PER_BLOCK 6

static _Thread_local char g_error[256] = "";
static int set_error(int code, const char *text)
{
	snprintf(g_error, sizeof(g_error), "%s", text);
	return code;
}
const char *hfdl_gpu_last_error(void) { return g_error; }

static void violation(const char *text)
{
	fprintf(stderr, "gpu stand-in: %s\n", text);
	abort();
}

/* ---- pinned memory ---- */

#define ALLOCS_MAX 64
static struct { char *p; size_t bytes; } g_allocs[ALLOCS_MAX];

int hfdl_gpu_host_alloc(void **ptr, size_t bytes)
{
	if (ptr == NULL) return set_error(HFDL_GPU_EINVAL, "host_alloc: null pointer");
	for (int i = 0; i < ALLOCS_MAX; i++)
		if (g_allocs[i].p == NULL) {
			if ((g_allocs[i].p = malloc(bytes ? bytes : 1)) == NULL) return set_error(HFDL_GPU_ENOMEM, "host_alloc: out of memory");
			g_allocs[i].bytes = bytes;
			*ptr = g_allocs[i].p;
			return 0;
		}
	return set_error(HFDL_GPU_ENOMEM, "host_alloc: registry full");
}

void hfdl_gpu_host_free(void *ptr)
{
	if (ptr == NULL) return;
	for (int i = 0; i < ALLOCS_MAX; i++)
		if (g_allocs[i].p == ptr) {
			free(ptr);
			g_allocs[i].p = NULL;
			return;
		}
	violation("host_free of memory that is not allocated (freed twice?)");
}

static int is_pinned(const void *p, size_t bytes)
{
	for (int i = 0; i < ALLOCS_MAX; i++)
		if (g_allocs[i].p != NULL && (const char *)p >= g_allocs[i].p && (const char *)p + bytes <= g_allocs[i].p + g_allocs[i].bytes) return 1;
	return 0;
}

/* ---- the front end ---- */

struct host_block {
	const void *src;
	size_t bytes;
	int format;
	int asked;                       /* input_copied questions answered "not yet" */
	int copied, pushed;
	uint64_t hash;
};

struct closed_row { uint64_t first_block; uint32_t blocks; uint64_t closed_at; };     /* closed_at: pushes when it was closed */

struct hfdl_gpu_frontend {
	hfdl_gpu_geometry geo;
	int32_t freq0;
	int copy_lag;
	long fail_push;
	char fail_text[128];
	struct host_block *blk;          /* host blocks in the order their copies were queued */
	uint64_t nblk, cap, copied_upto, pushes, delivered;   /* blocks [0, copied_upto) are copied; [0, pushes) pushed; [0, delivered) polled */
	uint64_t prefetched;             /* queued ahead and not pushed yet: host blocks [pushes, pushes + prefetched) */
	int32_t spec_bins, spec_rows;
	struct closed_row *rows;         /* every closed row (the ring is modelled by the oldest index kept) */
	uint64_t nrows, rows_cap, open_first;
	uint32_t open_blocks;
	int32_t x_nsel, x_ring, x_format;
	uint64_t x_first;                /* the first exported block */
};

#define LIVE_MAX 8
static hfdl_gpu_frontend *g_live[LIVE_MAX];

static int bytes_per_sample(int format) { return format == HFDL_GPU_SFMT_CS16 ? 4 : format == HFDL_GPU_SFMT_CU8 ? 2 : format == HFDL_GPU_SFMT_CF32 ? 8 : 0; }

int hfdl_gpu_plan_geometry(int32_t decimation, float transition_bw, hfdl_gpu_geometry *g)
{
	if (g == NULL || decimation < 1) return set_error(HFDL_GPU_EINVAL, "plan_geometry: bad argument");
	memset(g, 0, sizeof(*g));
	g->decimation = decimation;
	g->transition_bw = transition_bw;
	g->pre_decimation = g->post_decimation = 1;
	g->fft_size = FFT_SIZE;
	g->input_size = BLOCK_SAMPLES;
	g->overlap_length = FFT_SIZE - BLOCK_SAMPLES;
	g->taps_length = g->overlap_length + 1;
	g->fft_inv_size = g->post_input_size = OUT_PER_BLOCK;
	g->outputs_per_block = g->max_outputs_per_block = OUT_PER_BLOCK;
	return 0;
}

int hfdl_gpu_frontend_create(hfdl_gpu_frontend **out, int device, int32_t sample_rate, int32_t centerfreq, const int32_t *freqs, int32_t nch)
{
	(void)device; (void)centerfreq;
	if (out == NULL || freqs == NULL || nch < 1 || sample_rate < 1) return set_error(HFDL_GPU_EINVAL, "create: bad argument");
	const char *e = getenv("HFDL_STANDIN_FAIL_CREATE");
	if (e != NULL) return set_error(HFDL_GPU_ENODEV, e);
	hfdl_gpu_frontend *fe = calloc(1, sizeof(*fe));
	if (fe == NULL) return set_error(HFDL_GPU_ENOMEM, "create: out of memory");
	hfdl_gpu_plan_geometry(1, 0.f, &fe->geo);
	fe->geo.sample_rate = sample_rate;
	fe->geo.channels = nch;
	fe->geo.fold_batch = fe->geo.demod_batch = 1;
	if ((e = getenv("HFDL_STANDIN_PREFETCH")) != NULL) fe->geo.prefetch_depth = atoi(e);
	if (fe->geo.prefetch_depth < 0 || fe->geo.prefetch_depth > HFDL_GPU_PREFETCH_MAX) { free(fe); return set_error(HFDL_GPU_EINVAL, "create: HFDL_STANDIN_PREFETCH out of range"); }
	if ((e = getenv("HFDL_STANDIN_COPY_LAG")) != NULL) fe->copy_lag = atoi(e);
	if ((e = getenv("HFDL_STANDIN_FAIL_PUSH")) != NULL) fe->fail_push = atol(e);
	snprintf(fe->fail_text, sizeof(fe->fail_text), "%s", getenv("HFDL_STANDIN_FAIL_TEXT") ? getenv("HFDL_STANDIN_FAIL_TEXT") : "injected push failure");
	fe->freq0 = freqs[0];
	int slot = 0;
	while (slot < LIVE_MAX && g_live[slot] != NULL) slot++;
	if (slot == LIVE_MAX) { free(fe); return set_error(HFDL_GPU_ENOMEM, "create: too many front ends"); }
	g_live[slot] = fe;
	*out = fe;
	return 0;
}

void hfdl_gpu_frontend_destroy(hfdl_gpu_frontend *fe)
{
	if (fe == NULL) return;
	int slot = 0;
	while (slot < LIVE_MAX && g_live[slot] != fe) slot++;
	if (slot == LIVE_MAX) violation("destroy of a front end that is not live (destroyed twice?)");
	if (fe->prefetched > 0) violation("destroy with a prefetched block neither pushed nor cancelled");
	g_live[slot] = NULL;
	free(fe->blk);
	free(fe->rows);
	free(fe);
}

int hfdl_gpu_frontend_geometry(const hfdl_gpu_frontend *fe, hfdl_gpu_geometry *g)
{
	if (fe == NULL || g == NULL) return set_error(HFDL_GPU_EINVAL, "geometry: null pointer");
	*g = fe->geo;
	return 0;
}

int hfdl_gpu_frontend_enable_taps(hfdl_gpu_frontend *fe, int enable)
{
	(void)enable;
	return fe ? 0 : set_error(HFDL_GPU_EINVAL, "enable_taps: null handle");
}

/* ---- uploads: the late-reading copy engine ---- */

static uint64_t fnv1a64(const void *p, size_t n)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
	return h;
}

/* the copies of host blocks [.., upto) finish now: this is when the caller's memory is read */
static void complete_upto(hfdl_gpu_frontend *fe, uint64_t upto)
{
	if (upto > fe->nblk) upto = fe->nblk;
	for (; fe->copied_upto < upto; fe->copied_upto++) {
		struct host_block *b = &fe->blk[fe->copied_upto];
		b->hash = fnv1a64(b->src, b->bytes);
		b->copied = 1;
	}
}

static int queue_copy(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int format)
{
	if (fe->nblk == fe->cap) {
		fe->cap = fe->cap ? 2 * fe->cap : 64;
		struct host_block *grown = realloc(fe->blk, fe->cap * sizeof(*grown));
		if (grown == NULL) return set_error(HFDL_GPU_ENOMEM, "out of memory");
		fe->blk = grown;
	}
	struct host_block *b = &fe->blk[fe->nblk++];
	memset(b, 0, sizeof(*b));
	b->src = raw;
	b->bytes = nsamples * (size_t)bytes_per_sample(format);
	b->format = format;
	/* pageable memory is waited for inside the call, as the real library does */
	if (!is_pinned(raw, b->bytes)) complete_upto(fe, fe->nblk);
	return 0;
}

int hfdl_gpu_frontend_prefetch_block_raw(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int sample_format)
{
	if (fe == NULL || raw == NULL || nsamples != (size_t)fe->geo.input_size || bytes_per_sample(sample_format) == 0)
		return set_error(HFDL_GPU_EINVAL, "prefetch: bad argument");
	if (!is_pinned(raw, nsamples * (size_t)bytes_per_sample(sample_format))) return set_error(HFDL_GPU_EINVAL, "prefetch: the block is not in page-locked memory");
	if (fe->prefetched >= (uint64_t)fe->geo.prefetch_depth) return set_error(HFDL_GPU_ERANGE, "prefetch: more than prefetch_depth blocks waiting");
	int rc = queue_copy(fe, raw, nsamples, sample_format);
	if (rc == 0) fe->prefetched++;
	return rc;
}

int hfdl_gpu_frontend_prefetch_cancel(hfdl_gpu_frontend *fe)
{
	if (fe == NULL) return set_error(HFDL_GPU_EINVAL, "prefetch_cancel: null handle");
	complete_upto(fe, fe->nblk);
	/* the cancelled blocks keep their host block numbers but are never pushed: take them out of the pushed range by marking them */
	for (uint64_t i = 0; i < fe->prefetched; i++) fe->blk[fe->nblk - 1 - i].pushed = -1;
	fe->prefetched = 0;
	return 0;
}

static void open_row_add(hfdl_gpu_frontend *fe);

int hfdl_gpu_frontend_push_block_raw(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int sample_format, int on_device)
{
	if (fe == NULL || raw == NULL || on_device || nsamples != (size_t)fe->geo.input_size || bytes_per_sample(sample_format) == 0)
		return set_error(HFDL_GPU_EINVAL, "push: bad argument");
	if (fe->fail_push > 0 && --fe->fail_push == 0) return set_error(HFDL_GPU_EHIP, fe->fail_text);
	struct host_block *b = NULL;
	if (fe->prefetched > 0) {
		b = &fe->blk[fe->nblk - fe->prefetched];
		if (b->src != raw || b->format != sample_format) return set_error(HFDL_GPU_EINVAL, "push: not the oldest prefetched block");
		fe->prefetched--;
	} else {
		int rc = queue_copy(fe, raw, nsamples, sample_format);
		if (rc != 0) return rc;
		b = &fe->blk[fe->nblk - 1];
	}
	b->pushed = 1;
	fe->pushes++;
	open_row_add(fe);
	return 0;
}

int hfdl_gpu_frontend_input_done(hfdl_gpu_frontend *fe)
{
	if (fe == NULL) return set_error(HFDL_GPU_EINVAL, "input_done: null handle");
	complete_upto(fe, fe->nblk);
	return 0;
}

int hfdl_gpu_frontend_input_done_upto(hfdl_gpu_frontend *fe, uint64_t host_block)
{
	if (fe == NULL || host_block >= fe->nblk) return set_error(HFDL_GPU_EINVAL, "input_done_upto: no such host block");
	complete_upto(fe, host_block + 1);
	return 0;
}

int hfdl_gpu_frontend_input_copied(hfdl_gpu_frontend *fe, uint64_t host_block)
{
	if (fe == NULL || host_block >= fe->nblk) return set_error(HFDL_GPU_EINVAL, "input_copied: no such host block");
	struct host_block *b = &fe->blk[host_block];
	if (!b->copied && b->asked++ >= fe->copy_lag) complete_upto(fe, host_block + 1);
	return b->copied;
}

/* ---- PDUs ---- */

static int deliver(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n, int only_copied)
{
	if (fe == NULL || n == NULL || max < 0 || (out == NULL && max > 0)) return set_error(HFDL_GPU_EINVAL, "poll: bad argument");
	*n = 0;
	for (; *n < max && fe->delivered < fe->nblk; fe->delivered++) {
		const struct host_block *b = &fe->blk[fe->delivered];
		if (b->pushed < 0) continue;                             /* cancelled */
		if (b->pushed == 0 || (only_copied && !b->copied)) break;
		hfdl_gpu_pdu *p = &out[(*n)++];
		memset(p, 0, sizeof(*p));
		p->freq = fe->freq0;
		p->bit_rate = 300;
		p->slot = 'S';
		p->fcs_status = HFDL_GPU_FCS_GOOD;
		p->pdu_kind = HFDL_GPU_KIND_MPDU_DOWNLINK;
		p->lpdus_processed = 2; p->lpdus_good = 1; p->lpdus_bad_fcs = 1;       /* per PDU, so the run statistics' LPDU walk is checkable */
		p->len = 16;
		for (int i = 0; i < 8; i++) {
			p->octets[i] = (uint8_t)(fe->delivered >> (8 * i));
			p->octets[8 + i] = (uint8_t)(b->hash >> (8 * i));
		}
		p->sample_index = fe->delivered * (uint64_t)fe->geo.input_size;
	}
	return 0;
}

int hfdl_gpu_frontend_poll_pdus(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n)
{
	if (fe != NULL) complete_upto(fe, fe->nblk - fe->prefetched);       /* a sync: every pushed block's copy has run */
	return deliver(fe, out, max, n, 0);
}

int hfdl_gpu_frontend_poll_pdus_ready(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n, int32_t max_in_flight)
{
	if (max_in_flight == 0) return hfdl_gpu_frontend_poll_pdus(fe, out, max, n);
	return deliver(fe, out, max, n, 1);
}

int hfdl_gpu_frontend_all_channel_stats(hfdl_gpu_frontend *fe, hfdl_gpu_channel_stats *out, int32_t cap, int32_t *n)
{
	if (fe == NULL || out == NULL || n == NULL || cap < fe->geo.channels) return set_error(HFDL_GPU_EINVAL, "all_channel_stats: bad argument");
	memset(out, 0, sizeof(*out) * (size_t)fe->geo.channels);
	out[0].freq = fe->freq0;
	*n = fe->geo.channels;
	return 0;
}

/* ---- spectrum history: row r holds mean[b] = standin_row_power(r, b) ---- */

static float row_power(uint64_t row, int32_t b) { return (float)(1 + (row * 31 + (uint64_t)b) % 97) / 128.f; }

static void open_row_add(hfdl_gpu_frontend *fe)
{
	if (fe->spec_rows == 0) return;
	if (fe->open_blocks++ == 0) fe->open_first = fe->pushes - 1;
}

int hfdl_gpu_frontend_spectrum_enable(hfdl_gpu_frontend *fe, int32_t bins, uint32_t flags)
{
	if (fe == NULL || (flags & ~3u) || bins < 0 || (bins & (bins - 1)) || (bins > 0 && bins < 16)) return set_error(HFDL_GPU_EINVAL, "spectrum_enable: bad argument");
	if (bins > fe->geo.fft_size / 16) return set_error(HFDL_GPU_ERANGE, "spectrum_enable: more than fft_size / 16 bins");
	fe->spec_bins = bins;
	fe->spec_rows = 0;
	return 0;
}

int hfdl_gpu_frontend_spectrum_history(hfdl_gpu_frontend *fe, int32_t rows, int32_t interval_blocks)
{
	if (fe == NULL || fe->spec_bins == 0 || interval_blocks != 0 || rows == 1 || rows < 0 || rows > HFDL_GPU_SPECTRUM_ROWS_MAX)
		return set_error(HFDL_GPU_EINVAL, "spectrum_history: bad argument");
	fe->spec_rows = rows;
	fe->nrows = 0;
	fe->open_blocks = 0;
	return 0;
}

int hfdl_gpu_frontend_spectrum_row_close(hfdl_gpu_frontend *fe, uint64_t *row)
{
	if (fe == NULL || fe->spec_rows == 0) return set_error(HFDL_GPU_EINVAL, "spectrum_row_close: history off");
	if (row != NULL) *row = fe->nrows;
	if (fe->open_blocks == 0) return 0;
	if (fe->nrows == fe->rows_cap) {
		fe->rows_cap = fe->rows_cap ? 2 * fe->rows_cap : 64;
		struct closed_row *grown = realloc(fe->rows, fe->rows_cap * sizeof(*grown));
		if (grown == NULL) return set_error(HFDL_GPU_ENOMEM, "out of memory");
		fe->rows = grown;
	}
	fe->rows[fe->nrows++] = (struct closed_row){ fe->open_first, fe->open_blocks, fe->pushes };
	fe->open_blocks = 0;
	return 0;
}

int hfdl_gpu_frontend_spectrum_rows(hfdl_gpu_frontend *fe, int32_t rx, uint64_t from_row, int32_t max_rows,
		float *mean, float *peak, hfdl_gpu_spectrum_row *info, int32_t *n, uint64_t *next_row, int wait)
{
	if (fe == NULL || n == NULL || next_row == NULL || fe->spec_rows == 0 || rx != 0 || max_rows < 0 || peak != NULL
			|| (max_rows > 0 && (mean == NULL || info == NULL))) return set_error(HFDL_GPU_EINVAL, "spectrum_rows: bad argument");
	const uint64_t held = fe->nrows + (fe->open_blocks > 0), oldest = held > (uint64_t)fe->spec_rows ? held - (uint64_t)fe->spec_rows : 0;
	uint64_t r = from_row > oldest ? from_row : oldest;
	*n = 0;
	for (; *n < max_rows && r < fe->nrows && (wait || fe->rows[r].closed_at < fe->pushes); r++, (*n)++) {
		info[*n] = (hfdl_gpu_spectrum_row){ r, fe->rows[r].first_block, fe->rows[r].blocks, 0 };
		for (int32_t b = 0; b < fe->spec_bins; b++) mean[(size_t)*n * (size_t)fe->spec_bins + (size_t)b] = row_power(r, b);
	}
	*next_row = r;
	return 0;
}

/* ---- export ring: block b gives selected channel s export_count(b, s) samples; a channel's samples count 0, 1, 2, ... through the
 * blocks from the first exported one on (re = that counter, im = s) ---- */

static int32_t export_count(uint64_t block, int32_t s) { return 1 + (int32_t)((block * 7 + (uint64_t)s * 3) % OUT_PER_BLOCK); }

int hfdl_gpu_frontend_export_enable(hfdl_gpu_frontend *fe, const int32_t *channels, int32_t nsel, int format, float scale, int32_t ring_blocks)
{
	(void)scale;
	if (fe == NULL || nsel < 0 || nsel > fe->geo.channels || (nsel > 0 && channels == NULL) || (format != HFDL_GPU_EXPORT_CF32 && format != HFDL_GPU_EXPORT_CS16)
			|| ring_blocks < 2 || ring_blocks > HFDL_GPU_EXPORT_RING_MAX) return set_error(HFDL_GPU_EINVAL, "export_enable: bad argument");
	fe->x_nsel = nsel;
	fe->x_ring = ring_blocks;
	fe->x_format = format;
	fe->x_first = fe->pushes;
	return 0;
}

int hfdl_gpu_frontend_export_read(hfdl_gpu_frontend *fe, uint64_t from_block, int32_t max_blocks,
		void *samples, int32_t *counts, float *power, uint32_t *clipped, hfdl_gpu_export_block *info,
		int32_t *n, uint64_t *next_block, int wait)
{
	if (fe == NULL || n == NULL || next_block == NULL || fe->x_nsel == 0 || max_blocks < 0 || power != NULL || clipped != NULL
			|| (max_blocks > 0 && (samples == NULL || counts == NULL || info == NULL))) return set_error(HFDL_GPU_EINVAL, "export_read: bad argument");
	const uint64_t finished = wait ? fe->pushes : fe->pushes > 0 ? fe->pushes - 1 : 0;       /* blocks [.., finished) can be read */
	uint64_t oldest = fe->pushes > (uint64_t)fe->x_ring ? fe->pushes - (uint64_t)fe->x_ring : 0;
	if (oldest < fe->x_first) oldest = fe->x_first;
	uint64_t b = from_block > oldest ? from_block : oldest;
	const size_t es = fe->x_format == HFDL_GPU_EXPORT_CS16 ? 2 * sizeof(int16_t) : 2 * sizeof(float);
	if (max_blocks > 0) memset(samples, 0, (size_t)max_blocks * (size_t)fe->x_nsel * OUT_PER_BLOCK * es);
	*n = 0;
	for (; *n < max_blocks && b < finished; b++, (*n)++) {
		info[*n].block = b;
		for (int32_t s = 0; s < fe->x_nsel; s++) {
			uint64_t at = 0;
			for (uint64_t k = fe->x_first; k < b; k++) at += (uint64_t)export_count(k, s);
			const size_t r = (size_t)*n * (size_t)fe->x_nsel + (size_t)s;
			counts[r] = export_count(b, s);
			for (int32_t i = 0; i < counts[r]; i++) {
				if (fe->x_format == HFDL_GPU_EXPORT_CS16) {
					int16_t *v = (int16_t *)samples + 2 * (r * OUT_PER_BLOCK + (size_t)i);
					v[0] = (int16_t)((at + (uint64_t)i) % 32768); v[1] = (int16_t)s;
				} else {
					float *v = (float *)samples + 2 * (r * OUT_PER_BLOCK + (size_t)i);
					v[0] = (float)(at + (uint64_t)i); v[1] = (float)s;
				}
			}
		}
	}
	*next_block = b;
	return 0;
}
