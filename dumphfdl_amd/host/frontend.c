/* frontend.c -- the block that replaces dumphfdl's fft block AND all of its channel threads (src/fft.c, src/hfdl.c):
 * it drains the input ring exactly like fft_thread (src/fft.c:38-54), hands each block of input_size samples to the
 * GPU front end (include/hfdl_gpu.h) and turns the PDUs that come back into pdu_decoder_queue_push() calls the way
 * dispatch_pdu does (src/hfdl.c:1058-1080). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdbool.h>
#include <unistd.h>
#include <pthread.h>
#include <time.h>
#include "hfdl_host.h"
#include "hfdl_gpu.h"
#include "host_internal.h"
#include "retune_requests.h"

/* A GPU library without the entry point (the CPU stand-in of the tests, an older build) leaves the symbol null: it cannot retune, and a
 * request is refused. */
#pragma weak hfdl_gpu_frontend_retune_channel
/* ... and the frame quality records likewise: a frame log asked of such a library is refused when the front end is created */
#pragma weak hfdl_gpu_frontend_quality_enable
#pragma weak hfdl_gpu_frontend_quality_read
/* ... and the impulse-noise blanker: asked of such a library, fft_create() refuses */
#pragma weak hfdl_gpu_frontend_blanker_enable
#pragma weak hfdl_gpu_frontend_blanker_stats
/* ... and the I/Q imbalance and DC corrector likewise */
#pragma weak hfdl_gpu_frontend_iqbal_enable
#pragma weak hfdl_gpu_frontend_iqbal_stats
/* ... and the adaptive carrier canceller likewise */
#pragma weak hfdl_gpu_frontend_notch_enable
#pragma weak hfdl_gpu_frontend_notch_stats
/* ... and real-sampled input likewise */
#pragma weak hfdl_gpu_frontend_create_real

/* The optional outputs of a front end.  Each is set for the NEXT front end by its setter and copied into the block when
 * fft_create() runs; every copy owns its memory (one deep copy, one free for all of them). */
struct spectrum_settings { const char *path; int32_t bins, interval_s; int hann; };                         /* path NULL = off */
struct iq_export_settings { const char *dir; const int32_t *freqs; int32_t nfreqs; int format; float scale; };  /* dir NULL = off */

static struct spectrum_settings spectrum_settings_copy(const struct spectrum_settings *s)
{
	struct spectrum_settings c = *s;
	c.path = s->path ? strdup(s->path) : NULL;
	return c;
}

static void spectrum_settings_free(struct spectrum_settings *s) { free((char *)s->path); }

static struct iq_export_settings iq_export_settings_copy(const struct iq_export_settings *s)
{
	struct iq_export_settings c = *s;
	c.dir = s->dir ? strdup(s->dir) : NULL;
	c.nfreqs = s->dir ? s->nfreqs : 0;
	int32_t *freqs = s->dir ? hfdl_xcalloc(c.nfreqs > 0 ? (size_t)c.nfreqs : 1, sizeof(int32_t)) : NULL;
	if (c.nfreqs > 0) memcpy(freqs, s->freqs, (size_t)c.nfreqs * sizeof(int32_t));
	c.freqs = freqs;
	return c;
}

static void iq_export_settings_free(struct iq_export_settings *s)
{
	free((char *)s->dir);
	free((int32_t *)s->freqs);
}

struct notch_settings { float mu; int32_t *freqs_khz; int32_t nfreqs; };                                   /* nfreqs 0 = every channel */

static struct notch_settings notch_settings_copy(const struct notch_settings *s)
{
	struct notch_settings c = *s;
	c.freqs_khz = s->nfreqs > 0 ? hfdl_xcalloc((size_t)s->nfreqs, sizeof(int32_t)) : NULL;
	if (s->nfreqs > 0) memcpy(c.freqs_khz, s->freqs_khz, (size_t)s->nfreqs * sizeof(int32_t));
	return c;
}

struct gpu_fft_block {
	struct block block;
	int32_t decimation;
	float transition_bw;
	int device;
	hfdl_gpu_geometry geo;
	struct spectrum_settings spectrum;       /* as set when fft_create() ran */
	struct iq_export_settings iqx;
	char *frame_log;                         /* path, NULL = off */
	float blanker_db;                        /* 0 = off */
	float iq_alpha;                          /* 0 = off */
	struct notch_settings notch;             /* mu 0 = off */
	int32_t real_base_khz;                   /* -1 = off: the ring holds I/Q */
};

static int g_device = 0;
void hfdl_frontend_set_device(int device) { g_device = device; }

static struct spectrum_settings g_spectrum;
int hfdl_frontend_set_spectrum(const char *path, int32_t bins, int32_t interval_s, int hann)
{
	if (path != NULL && (bins < 16 || bins > 4096 || (bins & (bins - 1)) != 0 || interval_s < 1)) return -1;
	const struct spectrum_settings given = { path, bins, interval_s, hann };
	spectrum_settings_free(&g_spectrum);
	g_spectrum = spectrum_settings_copy(&given);
	return 0;
}

static struct iq_export_settings g_iqx;
int hfdl_frontend_set_iq_export(const char *dir, const int32_t *freqs, int32_t nfreqs, int format, float scale)
{
	if (dir != NULL && (nfreqs < 0 || (nfreqs > 0 && freqs == NULL) || (format != HFDL_GPU_EXPORT_CF32 && format != HFDL_GPU_EXPORT_CS16)
			|| (format == HFDL_GPU_EXPORT_CS16 && !(scale > 0.f && isfinite(scale))))) return -1;
	const struct iq_export_settings given = { dir, freqs, nfreqs, format, scale };
	iq_export_settings_free(&g_iqx);
	g_iqx = iq_export_settings_copy(&given);
	return 0;
}

static char *g_frame_log;
int hfdl_frontend_set_frame_log(const char *path)
{
	free(g_frame_log);
	g_frame_log = path ? strdup(path) : NULL;
	return 0;
}

static float g_blanker_db;
int hfdl_frontend_set_blanker(float threshold_db)
{
	if (!(threshold_db == 0.f || (threshold_db >= 6.f && threshold_db <= 60.f))) return -1;
	g_blanker_db = threshold_db;
	return 0;
}

static float g_iq_alpha;
int hfdl_frontend_set_iq_correction(float alpha)
{
	if (!(alpha == 0.f || (alpha >= 1.f / 1024.f && alpha <= 1.f))) return -1;
	g_iq_alpha = alpha;
	return 0;
}

static int32_t g_real_base_khz = -1;
int hfdl_frontend_set_real_input(int32_t base_khz)
{
	if (base_khz < -1 || base_khz > 2000000) return -1;
	g_real_base_khz = base_khz;
	return 0;
}

static struct notch_settings g_notch;
int hfdl_frontend_set_notch(float mu, const int32_t *freqs_khz, int n)
{
	if (!(mu == 0.f || (mu >= 1e-5f && mu <= 0.05f)) || n < 0 || n > 4096 || (n > 0 && freqs_khz == NULL)) return -1;
	const struct notch_settings given = { mu, (int32_t *)freqs_khz, n };
	const struct notch_settings copy = notch_settings_copy(&given);
	free(g_notch.freqs_khz);
	g_notch = copy;
	return 0;
}

/* the canceller of a new front end: the listed frequencies become channel indices.  0, or -1 with the reason in *why */
static int notch_start(hfdl_gpu_frontend *fe, const struct notch_settings *s, const int32_t *freqs, size_t nch, const char **why)
{
	static char text[96];
	int32_t *sel = hfdl_xcalloc(s->nfreqs > 0 ? (size_t)s->nfreqs : 1, sizeof(int32_t));
	int rc = 0;
	for (int32_t i = 0; i < s->nfreqs && rc == 0; i++) {
		size_t c = 0;
		while (c < nch && freqs[c] != s->freqs_khz[i] * 1000) c++;
		if (c == nch) {
			snprintf(text, sizeof(text), "notch: %d kHz is not a channel of this front end", s->freqs_khz[i]);
			*why = text;
			rc = -1;
		}
		sel[i] = (int32_t)c;
	}
	if (rc == 0 && hfdl_gpu_frontend_notch_enable(fe, s->nfreqs > 0 ? sel : NULL, s->nfreqs, s->mu) != 0) {
		*why = hfdl_gpu_last_error();
		rc = -1;
	}
	free(sel);
	return rc;
}

/* ---- spectrum monitor: one rtl_power-compatible CSV line from a row of band powers (plain C, no device call; kept in this file
 * because the test builds of the host library compile a fixed list of sources):
 *   date, time, Hz low, Hz high, Hz step, samples, dB, dB, ...
 * date / time: UTC of `t_unix` (the stream-start convention of the PDU timestamps: wall clock at start + signal time); Hz low / high:
 * lower edge of the first and upper edge of the last band; Hz step: width of a band; samples: blocks averaged; one value per band,
 * dB = 10 log10(mean) -- dBFS, a full-scale tone reads 0 -- with a floor of -200 for an empty band. ---- */

int hfdl_spectrum_csv_line(char *buf, size_t cap, double t_unix, double hz_low, double hz_step, uint64_t samples, const float *mean, int32_t bins)
{
	if (buf == NULL || mean == NULL || bins < 1 || cap == 0) return -1;
	time_t sec = (time_t)floor(t_unix);
	struct tm tm;
	if (gmtime_r(&sec, &tm) == NULL) return -1;
	size_t n = strftime(buf, cap, "%Y-%m-%d, %H:%M:%S", &tm);
	if (n == 0) return -1;
	int k = snprintf(buf + n, cap - n, ", %.0f, %.0f, %.4f, %llu", hz_low, hz_low + hz_step * (double)bins, hz_step, (unsigned long long)samples);
	if (k < 0 || (size_t)k >= cap - n) return -1;
	n += (size_t)k;
	for (int32_t b = 0; b < bins; b++) {
		double db = mean[b] > 0.f ? 10.0 * log10((double)mean[b]) : -200.0;
		if (!(db > -200.0)) db = -200.0;
		k = snprintf(buf + n, cap - n, ", %.2f", db);
		if (k < 0 || (size_t)k >= cap - n) return -1;
		n += (size_t)k;
	}
	if (n + 2 > cap) return -1;
	buf[n++] = '\n';
	buf[n] = '\0';
	return (int)n;
}

/* ---- libcsdr helpers main() needs (src/libcsdr.c:135-144) ---- */

int32_t compute_fft_decimation_rate(int32_t sample_rate, int32_t target_rate)
{
	int32_t whole = (int32_t)floorf((float)sample_rate / (float)target_rate);
	for (int i = 0; i < 31; i++) if (whole < (1 << i)) return (1 << i) / 2;
	return -1;
}

float compute_filter_relative_transition_bw(int32_t sample_rate, int32_t transition_bw_hz)
{
	return (float)transition_bw_hz / (float)sample_rate;
}

/* ---- channel slots ---- */

#define MAX_SLOTS 4096
static struct hfdl_channel_slot *g_slots[MAX_SLOTS];
static size_t g_slot_cnt;
static pthread_mutex_t g_slot_lock = PTHREAD_MUTEX_INITIALIZER;

void hfdl_init_globals(void) { /* preamble sequences and filter tables live in libhfdl_gpu.so (built at create time) */ }

static void *channel_idle_thread(void *ctx)
{
	struct block *block = ctx;
	struct shared_buffer *in = &block->consumer.in->shared_buffer;
	pthread_barrier_wait(in->consumers_ready);      /* "all consumers initialised", src/hfdl.c:663 / src/fft.c:36 */
	pthread_barrier_wait(in->data_ready);           /* released once, by block_connection_one2many_shutdown() */
	block->running = false;
	return NULL;
}

struct block *hfdl_channel_create(int32_t sample_rate, int32_t pre_decimation_rate, float transition_bw,
		int32_t centerfreq, int32_t frequency)
{
	if (sample_rate <= 0 || pre_decimation_rate <= 0) return NULL;
	struct hfdl_channel_slot *s = hfdl_xcalloc(1, sizeof(*s));
	s->sample_rate = sample_rate; s->pre_decimation_rate = pre_decimation_rate; s->transition_bw = transition_bw;
	s->centerfreq = centerfreq; s->frequency = frequency;
	s->block.producer.type = PRODUCER_NONE;
	s->block.consumer.type = CONSUMER_MULTI;
	s->block.consumer.min_ru = 0;
	s->block.thread_routine = channel_idle_thread;
	pthread_mutex_lock(&g_slot_lock);
	if (g_slot_cnt == MAX_SLOTS) { pthread_mutex_unlock(&g_slot_lock); free(s); return NULL; }
	g_slots[g_slot_cnt++] = s;
	pthread_mutex_unlock(&g_slot_lock);
	return &s->block;
}

void hfdl_channel_destroy(struct block *channel_block)
{
	if (channel_block == NULL) return;
	struct hfdl_channel_slot *s = container_of(channel_block, struct hfdl_channel_slot, block);
	pthread_mutex_lock(&g_slot_lock);
	for (size_t i = 0; i < g_slot_cnt; i++) if (g_slots[i] == s) { g_slots[i] = g_slots[--g_slot_cnt]; break; }
	pthread_mutex_unlock(&g_slot_lock);
	free(s);
}

size_t hfdl_channels_on_connection(struct block_connection *conn, struct hfdl_channel_slot **out, size_t max)
{
	size_t n = 0;
	pthread_mutex_lock(&g_slot_lock);
	for (size_t i = 0; i < g_slot_cnt && n < max; i++) if (g_slots[i]->block.consumer.in == conn) out[n++] = g_slots[i];
	pthread_mutex_unlock(&g_slot_lock);
	return n;
}

/* ---- retune requests (retune_requests.h): hfdl_frontend_retune() from any thread, hfdl_frontend_schedule_retune() on the sample clock;
 * the front-end thread applies them between two pushes.  One mutex guards both lists AND the application of a request, so a request
 * is always checked against the frequencies the channels will listen on once everything accepted before it has been applied.  Lock
 * order: g_retune_lock, then g_slot_lock. ---- */

static pthread_mutex_t g_retune_lock = PTHREAD_MUTEX_INITIALIZER;
static struct retune_list g_retune;
static struct { double seconds; struct retune_request r; } g_retune_at[HFDL_RETUNE_LIST_MAX];
static int32_t g_retune_at_cnt;

/* g_retune_lock held */
static int retune_add_locked(int32_t old_freq, int32_t new_freq)
{
	int32_t freqs[MAX_SLOTS];
	pthread_mutex_lock(&g_slot_lock);
	const int32_t n = (int32_t)g_slot_cnt;
	for (int32_t i = 0; i < n; i++) freqs[i] = g_slots[i]->frequency;
	pthread_mutex_unlock(&g_slot_lock);
	return retune_list_add(&g_retune, freqs, n, old_freq, new_freq);
}

int hfdl_frontend_retune(int32_t old_freq, int32_t new_freq)
{
	pthread_mutex_lock(&g_retune_lock);
	const int rc = retune_add_locked(old_freq, new_freq);
	pthread_mutex_unlock(&g_retune_lock);
	return rc;
}

int hfdl_frontend_schedule_retune(double seconds, int32_t old_freq, int32_t new_freq)
{
	int rc = -1;
	pthread_mutex_lock(&g_retune_lock);
	if (seconds >= 0 && isfinite(seconds) && g_retune_at_cnt < HFDL_RETUNE_LIST_MAX) {
		g_retune_at[g_retune_at_cnt].seconds = seconds;
		g_retune_at[g_retune_at_cnt].r = (struct retune_request){ old_freq, new_freq };
		g_retune_at_cnt++;
		rc = 0;
	}
	pthread_mutex_unlock(&g_retune_lock);
	return rc;
}

/* ---- StatsD-style observability (src/hfdl.c:818-840, 1082-1105): fed from the device-resident channel state ---- */

__attribute__((weak)) void statsd_counter_per_channel_increment(int32_t freq, char *counter) { (void)freq; (void)counter; }
__attribute__((weak)) void statsd_gauge_per_channel_set(int32_t freq, char *gauge, size_t value) { (void)freq; (void)gauge; (void)value; }

static struct {
	pthread_mutex_t lock;
	hfdl_gpu_channel_stats *last;       /* newest snapshot, one entry per channel of the front end */
	int32_t cnt;
	uint64_t a2, m1, m1_missing, frames; /* totals over all channels */
} g_obs = { .lock = PTHREAD_MUTEX_INITIALIZER };

static int32_t g_nf_interval;
void hfdl_nf_stats_set_interval(int32_t seconds) { g_nf_interval = seconds; }

/* one strided device read per block; emits one increment per new event, like the per-symbol calls of the reference */
static void publish_counters(hfdl_gpu_frontend *fe, hfdl_gpu_channel_stats *now, int32_t nch)
{
	int32_t n = 0;
	if (hfdl_gpu_frontend_all_channel_stats(fe, now, nch, &n) != 0 || n != nch) return;
	pthread_mutex_lock(&g_obs.lock);
	if (g_obs.last == NULL || g_obs.cnt != nch) {
		free(g_obs.last);
		g_obs.last = hfdl_xcalloc((size_t)nch, sizeof(*g_obs.last));
		g_obs.cnt = nch;
	}
	for (int32_t i = 0; i < nch; i++) {
		/* A channel's counters only grow, except that a retune starts them over (the library reports a retuned channel's as a fresh
		 * channel's from the call on, and apply_retune() zeroes the snapshot with them).  Should one be found BELOW the snapshot all
		 * the same, the channel has started over since: counted from zero, never "up" through 2^32. */
		static const hfdl_gpu_channel_stats fresh;
		const hfdl_gpu_channel_stats *o = &g_obs.last[i];
		if (now[i].a2_found < o->a2_found || now[i].m1_found < o->m1_found || now[i].m1_not_found < o->m1_not_found || now[i].frames < o->frames) o = &fresh;
		for (uint32_t k = o->a2_found; k != now[i].a2_found; k++) statsd_counter_per_channel_increment(now[i].freq, "demod.preamble.A2_found");
		for (uint32_t k = o->m1_found; k != now[i].m1_found; k++) statsd_counter_per_channel_increment(now[i].freq, "demod.preamble.M1_found");
		for (uint32_t k = o->m1_not_found; k != now[i].m1_not_found; k++) statsd_counter_per_channel_increment(now[i].freq, "demod.preamble.errors.M1_not_found");
		g_obs.a2 += now[i].a2_found - o->a2_found;
		g_obs.m1 += now[i].m1_found - o->m1_found;
		g_obs.m1_missing += now[i].m1_not_found - o->m1_not_found;
		g_obs.frames += now[i].frames - o->frames;
	}
	memcpy(g_obs.last, now, sizeof(*now) * (size_t)nch);
	pthread_mutex_unlock(&g_obs.lock);
}

/* the reference's debug summary, same lines (src/hfdl.c:563-573): totals over all channels from the newest device snapshot; the
 * correlation averages are weighted by each channel's detection count, as one global S.A1_corr_total / S.A1_found is */
void hfdl_print_summary(void)
{
#ifdef DEBUG
	pthread_mutex_lock(&g_obs.lock);
	uint64_t a1 = 0, a2 = 0, m1 = 0, bad = 0, total = 0;
	double c1 = 0, c2 = 0, cm = 0;
	for (int32_t i = 0; i < g_obs.cnt; i++) {
		const hfdl_gpu_channel_stats *s = &g_obs.last[i];
		a1 += s->a1_found; a2 += s->a2_found; m1 += s->m1_found;
		c1 += (double)s->a1_corr_avg * s->a1_found; c2 += (double)s->a2_corr_avg * s->a2_found; cm += (double)s->m1_corr_avg * s->m1_found;
		bad += s->train_bits_bad; total += s->train_bits_total;
	}
	fprintf(stderr, "A1_found:\t\t%llu\nA2_found:\t\t%llu\nM1_found:\t\t%llu\n", (unsigned long long)a1, (unsigned long long)a2, (unsigned long long)m1);
	fprintf(stderr, "A1_corr_avg:\t\t%4.3f\n", a1 > 0 ? c1 / (double)a1 : 0.0);
	fprintf(stderr, "A2_corr_avg:\t\t%4.3f\n", a2 > 0 ? c2 / (double)a2 : 0.0);
	fprintf(stderr, "M1_corr_avg:\t\t%4.3f\n", m1 > 0 ? cm / (double)m1 : 0.0);
	fprintf(stderr, "train_bits_bad/total:\t%llu/%llu (%f%%)\n", (unsigned long long)bad, (unsigned long long)total,
			(float)bad / (float)total * 100.f);
	pthread_mutex_unlock(&g_obs.lock);
#endif
}

static void *noise_floor_stats_thread(void *ctx)
{
	(void)ctx;
	for (;;) {
		sleep((unsigned)g_nf_interval);
		pthread_mutex_lock(&g_obs.lock);
		for (int32_t i = 0; i < g_obs.cnt; i++) {
			/* tenths of dBFS, positive: a StatsD gauge takes neither floats nor negative values (src/hfdl.c:1093-1101) */
			float nf = g_obs.last[i].noise_floor_db;
			if (nf <= 0.f) statsd_gauge_per_channel_set(g_obs.last[i].freq, "noise_floor", (size_t)fabsf(roundf(nf * 10.f)));
		}
		pthread_mutex_unlock(&g_obs.lock);
	}
	return NULL;
}

int32_t hfdl_nf_stats_thread_start(struct block **channel_block_list, int32_t channel_cnt)
{
	(void)channel_block_list; (void)channel_cnt;     /* every channel of the front end reports; the list is implicit */
	if (g_nf_interval <= 0) return 0;
	pthread_t th;
	pthread_attr_t attr;
	pthread_attr_init(&attr);
	pthread_attr_setdetachstate(&attr, PTHREAD_CREATE_DETACHED);    /* start_thread() detaches, src/util.c:45-63 */
	int ret = pthread_create(&th, &attr, noise_floor_stats_thread, NULL);
	pthread_attr_destroy(&attr);
	return ret == 0 ? 0 : -1;
}

/* ---- the front-end thread ---- */

#define PDU_BATCH 1024

/* Blocks that can be pushed before a launch has run and the thread has looked again: the blocks of two halves and the uploads ahead
 * of them, and as many again.  The spectrum history (were every block a row of its own) and the export ring hold that many. */
#define UNCOLLECTED_BLOCKS_MAX (2 * (2 * HFDL_GPU_FOLD_BATCH_MAX + HFDL_GPU_PREFETCH_MAX + 2))

/* Upload bookkeeping.  The GPU library numbers host blocks in the order their copies were queued, pushed directly or uploaded ahead
 * of their push.  The ring slots of the newest `leased` of them may still be read by the DMA engine; they lie at the ring's head,
 * oldest first, so the next block to take lies right behind them.  A block that went through the bounce buffer is a host block
 * but leases no slot. */
struct uploads {
	uint64_t count;                  /* host blocks whose copy has been queued */
	size_t leased;
	size_t depth;                    /* uploads that may wait for their push */
	const void *queued[HFDL_GPU_PREFETCH_MAX + 1];      /* uploads not pushed yet, oldest at q_head */
	size_t q_head, q_len;
};

static size_t uploads_next_offset(const struct uploads *u, size_t need) { return u->leased * need; }
static uint64_t uploads_oldest_leased(const struct uploads *u) { return u->count - u->leased; }
static void uploads_slot_returned(struct uploads *u) { u->leased--; }
static void uploads_forget(struct uploads *u) { u->leased = 0; u->q_len = 0; }

static void uploads_pushed_direct(struct uploads *u, bool from_ring)
{
	u->count++;
	if (from_ring) u->leased++;
}

static void uploads_queued_ahead(struct uploads *u, const void *blk)
{
	u->queued[(u->q_head + u->q_len) % (HFDL_GPU_PREFETCH_MAX + 1)] = blk;
	u->q_len++;
	u->count++;
	u->leased++;
}

/* its slot was leased when the copy was queued */
static void uploads_pushed_queued(struct uploads *u)
{
	u->q_head = (u->q_head + 1) % (HFDL_GPU_PREFETCH_MAX + 1);
	u->q_len--;
}

/* spectrum monitor: one CSV line per interval of SIGNAL (blocks pushed x block length / sample rate): a row of the device's history */
struct spectrum_csv {
	FILE *file;                      /* NULL = off */
	int32_t bins;
	char *line;
	size_t line_cap;
	float *mean;
	uint64_t closed, next;           /* intervals closed so far; the first row not written yet */
};

/* Channel baseband export: one file per selected channel; finished blocks are collected IQX_CHUNK at a time (wait = 0: never waits for
 * a kernel stream; wait = 1, at the end of a run: everything queued) and each block's valid samples appended to its channel's file. */
#define IQX_CHUNK 4
struct iq_export {
	int32_t nsel, row;               /* selected channels; samples a row holds (geometry.max_outputs_per_block) */
	size_t es;                       /* bytes per sample */
	FILE **files;                    /* NULL = off */
	int32_t *sel;                    /* [nsel] the channel of each file */
	char *samples;
	int32_t *counts;
	hfdl_gpu_export_block info[IQX_CHUNK];
	uint64_t next;                   /* the first block not written yet */
	uint64_t lost;                   /* blocks the ring overwrote before they could be written: named once, counted, the total reported at the end */
};

/* Frame log: one text line per frame from the device's frame quality records, collected FLOG_CHUNK at a time (wait = 0 after every
 * collection of PDUs: never waits for a kernel stream; wait = 1 at shutdown: everything). */
#define FLOG_CHUNK 16
#define FLOG_RING 4096
struct frame_log {
	FILE *file;                      /* NULL = off */
	hfdl_gpu_frame_quality *recs;    /* [FLOG_CHUNK] */
	uint32_t dropped;                /* frames the device's ring dropped because the log fell behind */
};

struct fe_thread {
	struct block *block;
	struct gpu_fft_block *fb;
	struct circ_buffer *ring;        /* the page-locked input ring in front of this block */
	hfdl_gpu_frontend *fe;
	bool ok;                         /* false once the run has failed: what arrives is dropped until the producer shuts down */
	size_t nch;
	int32_t *freqs;
	struct hfdl_channel_slot **slots; /* [nch] the registered channels, in the front end's channel order */
	double fs, centerfreq;           /* of the receiver */
	size_t need;                     /* samples of a block */
	int gfmt;                        /* HFDL_GPU_SFMT_* of the ring's samples */
	int bounce_fmt;                  /* ... and of the bounce buffer's: cf32, or with real input the same words as rf32 */
	size_t push_n;                   /* what a push calls a block's samples: `need`, or with real input twice that (an element is two real samples) */
	struct timeval t0;               /* wall clock at stream start */
	hfdl_gpu_pdu *pdus;
	hfdl_gpu_channel_stats *stats;
	struct uploads up;
	void *bounce;                    /* only for a ring whose blocks are not contiguous (never one made by this library) */
	uint64_t undelivered;            /* blocks pushed since the pipeline was last drained */
	struct timespec last_push;       /* when the newest block was taken from the ring and pushed (CLOCK_REALTIME: pthread_cond_timedwait's clock) */
	double grace;
	struct spectrum_csv csv;
	struct iq_export iqx;
	struct frame_log flog;
	double t_first;
	struct hfdl_run_stats rs;        /* where this thread's time went and what it moved; published once, at shutdown */
};

static void fail(struct fe_thread *t, const char *text)
{
	fprintf(stderr, "GPU front end: %s\n", text);
	do_exit = 1;
	t->ok = false;
}

/* start of frame = A2 detection - (prekey + 2 A) symbols (src/hfdl.c:657-660), on the stream's sample clock: a PDU's timestamp and
 * the time of its frame's line in the frame log */
static struct timeval frame_time(const struct fe_thread *t, uint64_t sample_index)
{
	const double ts = (double)t->t0.tv_sec + 1e-6 * (double)t->t0.tv_usec + (double)sample_index / (HFDL_SYMBOL_RATE * SPS)
		- (448.0 + 2 * 127.0) / HFDL_SYMBOL_RATE;
	struct timeval tv;
	tv.tv_sec = (time_t)floor(ts);
	tv.tv_usec = (suseconds_t)((ts - floor(ts)) * 1e6);
	return tv;
}

static void push_pdu(struct fe_thread *t, const hfdl_gpu_pdu *p)
{
	if (p->fcs_status == HFDL_GPU_FCS_GOOD && p->pdu_kind != HFDL_GPU_KIND_SPDU) {
		t->rs.mpdus_walked++; t->rs.lpdus_processed += p->lpdus_processed; t->rs.lpdus_good += p->lpdus_good; t->rs.lpdus_bad_fcs += p->lpdus_bad_fcs;
	}
	struct metadata *m = hfdl_pdu_metadata_create();
	struct hfdl_pdu_metadata *hm = container_of(m, struct hfdl_pdu_metadata, metadata);
	hm->version = 1;
	hm->freq = p->freq;
	hm->freq_err_hz = p->freq_err_hz;
	hm->rssi = p->rssi_db;
	hm->noise_floor = p->noise_floor_db;
	hm->bit_rate = p->bit_rate;
	hm->slot = p->slot;
	m->rx_timestamp = frame_time(t, p->sample_index);
	uint8_t *copy = hfdl_xcalloc((size_t)p->len ? (size_t)p->len : 1, 1);
	memcpy(copy, p->octets, (size_t)p->len);
	pdu_decoder_queue_push(m, octet_string_new(copy, (size_t)p->len), 0);
}

/* The poll -> push_pdu loop.  draining: everything pushed so far is folded, demodulated and delivered (the half being filled is
 * closed as it is).  Otherwise only what is known to be complete, without draining anything and WITHOUT waiting: what this thread may
 * queue ahead is bounded by the ring slots it leases to the uploads (it sleeps in release_copied() when the ring has nothing new and
 * the oldest upload is still running), and slots can only go back to the producer while this thread is not blocked elsewhere.
 * Ring mutex: not held (calls the device library and the downstream queue). */
static void deliver_pdus(struct fe_thread *t, bool draining)
{
	int32_t n = 0;
	do {
		if ((draining ? hfdl_gpu_frontend_poll_pdus(t->fe, t->pdus, PDU_BATCH, &n)
				: hfdl_gpu_frontend_poll_pdus_ready(t->fe, t->pdus, PDU_BATCH, &n, 2)) != 0) break;
		for (int32_t i = 0; i < n; i++) push_pdu(t, &t->pdus[i]);
		t->rs.pdus += (uint64_t)n;
	} while (n == PDU_BATCH);
}

static struct hfdl_run_stats g_run;
static pthread_mutex_t g_run_lock = PTHREAD_MUTEX_INITIALIZER;

void hfdl_frontend_run_stats(struct hfdl_run_stats *out)
{
	pthread_mutex_lock(&g_run_lock);
	*out = g_run;
	pthread_mutex_unlock(&g_run_lock);
}

static double now_s(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int gpu_format_of(int ring_fmt)
{
	return ring_fmt == SFMT_CS16 ? HFDL_GPU_SFMT_CS16 : ring_fmt == SFMT_CU8 ? HFDL_GPU_SFMT_CU8 : HFDL_GPU_SFMT_CF32;
}

/* give ring slots back to the producer, oldest first, as the DMA engine finishes reading them.  wait_for_one: block until at least
 * the oldest copy is done (the caller is about to sleep and the producer may be waiting for room); otherwise only what is done
 * already.  If the state of a copy cannot be established the run fails and the slot is kept: the producer must never overwrite
 * memory the DMA engine may still read.
 * Ring mutex: not held on entry or on return; taken only around the drop. */
static void release_copied(struct fe_thread *t, bool wait_for_one)
{
	while (t->up.leased > 0) {
		const uint64_t oldest = uploads_oldest_leased(&t->up);
		int done;                        /* 1 = the oldest copy has finished, 0 = not yet, negative = unknown */
		if (wait_for_one) {
			done = hfdl_gpu_frontend_input_done_upto(t->fe, oldest) == 0 || hfdl_gpu_frontend_input_done(t->fe) == 0 ? 1 : -1;
			wait_for_one = false;
		} else {
			done = hfdl_gpu_frontend_input_copied(t->fe, oldest);
		}
		if (done < 0) { fail(t, hfdl_gpu_last_error()); return; }
		if (done == 0) break;
		pthread_mutex_lock(t->ring->mutex);
		hfdl_ring_drop(t->ring->buf, t->need);
		pthread_mutex_unlock(t->ring->mutex);
		pthread_cond_signal(t->ring->cond);
		uploads_slot_returned(&t->up);
	}
}

/* Rows of the spectrum history the device has finished (wait = 0: never waits for a kernel stream; wait = 1, at the end of a run: every
 * closed row), one rtl_power line each, in row order, from row x->next on.  A row the ring has overwritten before it was written is
 * named on stderr. */
static void spectrum_csv_write_rows(struct fe_thread *t, int wait)
{
	struct spectrum_csv *x = &t->csv;
	const hfdl_gpu_geometry *geo = &t->fb->geo;
	const double step = (double)(geo->fft_size / x->bins) * t->fs / (double)geo->fft_size;
	const double low = t->centerfreq - (0.5 * (double)geo->fft_size + 0.5) * t->fs / (double)geo->fft_size;
	for (;;) {
		hfdl_gpu_spectrum_row info;
		int32_t n = 0;
		uint64_t after = x->next;
		if (hfdl_gpu_frontend_spectrum_rows(t->fe, 0, x->next, 1, x->mean, NULL, &info, &n, &after, wait) != 0) {
			fprintf(stderr, "spectrum monitor: %s\n", hfdl_gpu_last_error());
			return;
		}
		if (n == 0) { x->next = after; return; }
		for (uint64_t lost = x->next; lost < info.row; lost++)
			fprintf(stderr, "spectrum monitor: interval %llu has no line: its row was overwritten before it could be written\n", (unsigned long long)lost);
		x->next = after;
		/* stamped like the PDUs: wall clock at stream start + the signal time of the first block averaged */
		const double ts = (double)t->t0.tv_sec + 1e-6 * (double)t->t0.tv_usec + (double)info.first_block * (double)geo->input_size / t->fs;
		if (hfdl_spectrum_csv_line(x->line, x->line_cap, ts, low, step, info.blocks, x->mean, x->bins) > 0) {
			fputs(x->line, x->file);
			fflush(x->file);
		} else {
			fprintf(stderr, "spectrum monitor: interval %llu has no line: it does not fit the line buffer\n", (unsigned long long)info.row);
		}
	}
}

/* opens the file and turns the monitor and its history on; 0, or -1 with the reason on stderr and nothing left open */
static int spectrum_csv_open(struct fe_thread *t)
{
	struct spectrum_csv *x = &t->csv;
	const struct spectrum_settings *set = &t->fb->spectrum;
	x->bins = set->bins;
	while (x->bins > t->fb->geo.fft_size / 16) x->bins /= 2;
	x->file = fopen(set->path, "w");       /* a run writes its own file: nothing of an earlier run stays in front of it */
	if (x->file == NULL || hfdl_gpu_frontend_spectrum_enable(t->fe, x->bins, set->hann ? HFDL_GPU_SPECTRUM_HANN : 0u) != 0
			|| hfdl_gpu_frontend_spectrum_history(t->fe, UNCOLLECTED_BLOCKS_MAX, 0) != 0) {
		fprintf(stderr, "spectrum monitor: %s\n", x->file ? hfdl_gpu_last_error() : "cannot open the spectrum file");
		if (x->file) fclose(x->file);
		x->file = NULL;
		return -1;
	}
	x->mean = hfdl_xcalloc((size_t)x->bins, sizeof(float));
	x->line_cap = 64 + 12 * (size_t)x->bins;
	x->line = hfdl_xcalloc(x->line_cap, 1);
	return 0;
}

/* after a push: an interval boundary closes the open row (no device call); finished rows are written as they are found, without waiting */
static void spectrum_csv_step(struct fe_thread *t)
{
	struct spectrum_csv *x = &t->csv;
	if ((double)t->rs.blocks * (double)t->need / t->fs >= (double)(x->closed + 1) * (double)t->fb->spectrum.interval_s) {
		uint64_t row = 0;
		if (hfdl_gpu_frontend_spectrum_row_close(t->fe, &row) != 0)
			fprintf(stderr, "spectrum monitor: interval %llu has no line: %s\n", (unsigned long long)x->closed, hfdl_gpu_last_error());
		x->closed++;
	}
	spectrum_csv_write_rows(t, 0);
}

/* at the end of a run, while the front end still exists: every closed row not written yet, then the file is closed */
static void spectrum_csv_close(struct fe_thread *t)
{
	struct spectrum_csv *x = &t->csv;
	if (x->file != NULL) {
		spectrum_csv_write_rows(t, 1);
		fclose(x->file);
	}
	free(x->mean);
	free(x->line);
	memset(x, 0, sizeof(*x));
}

static void write_iq_export(hfdl_gpu_frontend *fe, struct iq_export *x, int wait)
{
	for (;;) {
		int32_t n = 0;
		uint64_t after = x->next;
		if (hfdl_gpu_frontend_export_read(fe, x->next, IQX_CHUNK, x->samples, x->counts, NULL, NULL, x->info, &n, &after, wait) != 0) {
			fprintf(stderr, "iq export: %s\n", hfdl_gpu_last_error());
			return;
		}
		const uint64_t first = n > 0 ? x->info[0].block : after;
		if (first > x->next) {
			if (x->lost == 0)
				fprintf(stderr, "iq export: blocks from block %llu on were overwritten before they could be written; the files continue, the count follows at the end\n", (unsigned long long)x->next);
			x->lost += first - x->next;
		}
		for (int32_t i = 0; i < n; i++)
			for (int32_t s = 0; s < x->nsel; s++) {
				const size_t r = (size_t)i * (size_t)x->nsel + (size_t)s, cnt = (size_t)x->counts[r];
				if (fwrite(x->samples + r * (size_t)x->row * x->es, x->es, cnt, x->files[s]) != cnt) fprintf(stderr, "iq export: short write\n");
			}
		x->next = after;
		if (n < IQX_CHUNK) return;
	}
}

/* One line per frame: time of the frame's start (the PDU's timestamp), frequency, mode, slot, MER = -10 log10(err_power) in dB, mean
 * symbol power, |gain|, the gain's phase in degrees, the worst data segment and its MER.  The figures are decision-directed
 * (include/hfdl_gpu.h): at low SNR they overstate the quality. */
static void write_frame_log(struct fe_thread *t, int wait)
{
	struct frame_log *g = &t->flog;
	int32_t n = 0;
	do {
		if (hfdl_gpu_frontend_quality_read(t->fe, g->recs, NULL, FLOG_CHUNK, &n, &g->dropped, wait) != 0) {
			fprintf(stderr, "frame log: %s\n", hfdl_gpu_last_error());
			return;
		}
		for (int32_t i = 0; i < n; i++) {
			const hfdl_gpu_frame_quality *q = &g->recs[i];
			const struct timeval tv = frame_time(t, q->sample_index);
			int32_t worst = 0;
			for (int32_t s = 1; s < q->segments && s < HFDL_GPU_QUALITY_SEGMENTS_MAX; s++)
				if (q->seg_err_power[s] > q->seg_err_power[worst]) worst = s;
			fprintf(g->file, "FRAME ts=%ld.%06ld freq=%d mode=%d slot=%c mer_db=%.2f sym_power=%.4f gain=%.4f gain_phase_deg=%.2f worst_segment=%d worst_mer_db=%.2f\n",
					(long)tv.tv_sec, (long)tv.tv_usec, q->freq, q->mode, q->segments == 72 ? 'S' : 'D', -10.0 * log10((double)q->err_power),
					(double)q->sym_power, hypot((double)q->gain_re, (double)q->gain_im), atan2((double)q->gain_im, (double)q->gain_re) * (180.0 / M_PI),
					worst, -10.0 * log10((double)q->seg_err_power[worst]));
		}
		wait = 0;                                /* the sync has been done */
	} while (n == FLOG_CHUNK);
	fflush(g->file);
}

static void frame_log_close(struct frame_log *g)
{
	if (g->dropped > 0) fprintf(stderr, "frame log: %u frames have no line (the log fell behind the device's ring)\n", g->dropped);
	if (g->file != NULL) fclose(g->file);
	free(g->recs);
	memset(g, 0, sizeof(*g));
}

static int frame_log_open(struct fe_thread *t)
{
	struct frame_log *g = &t->flog;
	if ((g->file = fopen(t->fb->frame_log, "w")) == NULL) { fprintf(stderr, "frame log: cannot open %s\n", t->fb->frame_log); return -1; }
	g->recs = hfdl_xcalloc(FLOG_CHUNK, sizeof(*g->recs));
	if (hfdl_gpu_frontend_quality_enable(t->fe, FLOG_RING, 0) != 0) {
		fprintf(stderr, "frame log: %s\n", hfdl_gpu_last_error());
		frame_log_close(g);
		return -1;
	}
	return 0;
}

static void iq_export_close(struct iq_export *x)
{
	if (x->lost > 0) fprintf(stderr, "iq export: %llu blocks lost\n", (unsigned long long)x->lost);
	for (int32_t s = 0; x->files != NULL && s < x->nsel; s++)
		if (x->files[s] != NULL) fclose(x->files[s]);
	free(x->files);
	free(x->sel);
	free(x->samples);
	free(x->counts);
	memset(x, 0, sizeof(*x));
}

/* selects the channels, opens their files and turns the export on; 0, or -1 with the reason on stderr and nothing left open */
static int iq_export_open(hfdl_gpu_frontend *fe, const struct gpu_fft_block *fb, struct hfdl_channel_slot **slots, size_t nch, struct iq_export *x)
{
	const struct iq_export_settings *set = &fb->iqx;
	const int32_t nsel = set->nfreqs > 0 ? set->nfreqs : (int32_t)nch;
	int32_t *sel = hfdl_xcalloc((size_t)nsel, sizeof(int32_t));
	int rc = 0;
	for (int32_t s = 0; s < nsel && rc == 0; s++) {
		size_t c = set->nfreqs > 0 ? 0 : (size_t)s;
		while (set->nfreqs > 0 && c < nch && slots[c]->frequency != set->freqs[s]) c++;
		if (c == nch) { fprintf(stderr, "iq export: %d Hz is not a registered channel\n", set->freqs[s]); rc = -1; }
		sel[s] = (int32_t)c;
	}
	x->nsel = nsel;
	x->row = fb->geo.max_outputs_per_block;
	x->es = set->format == HFDL_GPU_EXPORT_CS16 ? 2 * sizeof(int16_t) : 2 * sizeof(float);
	x->files = hfdl_xcalloc((size_t)nsel, sizeof(FILE *));
	x->samples = hfdl_xcalloc((size_t)IQX_CHUNK * (size_t)nsel * (size_t)x->row, x->es);
	x->counts = hfdl_xcalloc((size_t)IQX_CHUNK * (size_t)nsel, sizeof(int32_t));
	for (int32_t s = 0; s < nsel && rc == 0; s++) {
		const size_t cap = strlen(set->dir) + 32;
		char *path = hfdl_xcalloc(cap, 1);
		snprintf(path, cap, "%s/%d.%s", set->dir, slots[sel[s]]->frequency, set->format == HFDL_GPU_EXPORT_CS16 ? "cs16" : "cf32");
		if ((x->files[s] = fopen(path, "wb")) == NULL) { fprintf(stderr, "iq export: cannot open %s\n", path); rc = -1; }
		free(path);
	}
	/* the ring is halved until it fits the library's cap on a ring */
	int32_t ring = UNCOLLECTED_BLOCKS_MAX;
	if (rc == 0) {
		while ((rc = hfdl_gpu_frontend_export_enable(fe, sel, nsel, set->format, set->scale, ring)) == HFDL_GPU_ERANGE && ring > 2) ring /= 2;
		if (rc != 0) fprintf(stderr, "iq export: %s\n", hfdl_gpu_last_error());
	}
	x->sel = sel;
	if (rc != 0) iq_export_close(x);
	return rc == 0 ? 0 : -1;
}

/* One accepted request.  The GPU call closes the half being filled and drains nothing: blocks pushed so far keep the old frequency in
 * their PDUs however late they are polled, so nothing is collected here.  What the host keeps by frequency follows: the PDU hand-off
 * takes the frequency from the PDU itself; the slot (and with it t->freqs, the StatsD names -- publish_counters() reads the frequency
 * from the device library's statistics) changes here.  The counters: what the device has counted up to the call is published first,
 * under the old frequency; from the call on the library reports the channel's counters as a fresh channel's (zero, then what the new
 * frequency counts -- never the old values, although the device's own reset runs later, behind the demodulators in flight), so the
 * thread's snapshot is zeroed with them and publish_counters() never sees one run backwards.  (Events of the blocks still in flight
 * at the call are in no count: the reset wipes them.)  An exported channel's blocks from before the boundary go to
 * the old file (they are waited for: the only wait, and only for an exported channel), then a new <freq> file starts.
 * g_retune_lock: held.  Ring mutex: not held. */
static void apply_retune(struct fe_thread *t, const struct retune_request *r)
{
	size_t c = 0;
	while (c < t->nch && t->freqs[c] != r->old_freq) c++;
	const char *why = NULL;
	if (c == t->nch) why = "no channel of this front end listens there";
	else if (hfdl_gpu_frontend_retune_channel == NULL) why = "this GPU library cannot retune";
	else {
		publish_counters(t->fe, t->stats, (int32_t)t->nch);
		if (hfdl_gpu_frontend_retune_channel(t->fe, (int32_t)c, r->new_freq) != 0) why = hfdl_gpu_last_error();
	}
	if (why != NULL) {
		fprintf(stderr, "retune %d -> %d Hz refused: %s\n", r->old_freq, r->new_freq, why);
		return;
	}
	t->freqs[c] = r->new_freq;
	pthread_mutex_lock(&g_slot_lock);
	t->slots[c]->frequency = r->new_freq;
	pthread_mutex_unlock(&g_slot_lock);
	pthread_mutex_lock(&g_obs.lock);
	if (g_obs.last != NULL && (size_t)g_obs.cnt == t->nch) memset(&g_obs.last[c], 0, sizeof(g_obs.last[c]));
	pthread_mutex_unlock(&g_obs.lock);
	struct iq_export *x = &t->iqx;
	for (int32_t s = 0; x->files != NULL && s < x->nsel; s++) {
		if (x->sel[s] != (int32_t)c) continue;
		write_iq_export(t->fe, x, 1);
		const struct iq_export_settings *set = &t->fb->iqx;
		const size_t cap = strlen(set->dir) + 32;
		char *path = hfdl_xcalloc(cap, 1);
		snprintf(path, cap, "%s/%d.%s", set->dir, r->new_freq, set->format == HFDL_GPU_EXPORT_CS16 ? "cs16" : "cf32");
		FILE *f = fopen(path, "wb");
		if (f == NULL) fprintf(stderr, "iq export: cannot open %s; the channel's samples stay in the old file\n", path);
		else { fclose(x->files[s]); x->files[s] = f; }
		free(path);
	}
	t->rs.retunes++;
}

/* Between two pushes: the scheduled requests whose time has come -- the next block's first sample lies at or after it -- join the list
 * as a call of hfdl_frontend_retune() at this moment would, then the list is applied, oldest first.  A request that fails is named
 * once on stderr and the stream goes on.
 * Ring mutex: not held. */
static void retune_step(struct fe_thread *t)
{
	pthread_mutex_lock(&g_retune_lock);
	const double now = (double)t->rs.blocks * (double)t->need / t->fs;
	int32_t kept = 0;
	for (int32_t i = 0; i < g_retune_at_cnt; i++) {
		if (g_retune_at[i].seconds > now) { g_retune_at[kept++] = g_retune_at[i]; continue; }
		const struct retune_request *r = &g_retune_at[i].r;
		if (retune_add_locked(r->old_freq, r->new_freq) != 0)
			fprintf(stderr, "retune %d -> %d Hz refused: no channel listens on the old frequency, or one already listens on the new\n", r->old_freq, r->new_freq);
	}
	g_retune_at_cnt = kept;
	struct retune_request todo[HFDL_RETUNE_LIST_MAX];
	const int32_t n = retune_list_take(&g_retune, todo);
	for (int32_t i = 0; i < n; i++) apply_retune(t, &todo[i]);
	pthread_mutex_unlock(&g_retune_lock);
}

/* Ring mutex: held. */
static bool next_block_is_there(const struct fe_thread *t)
{
	return hfdl_ring_size(t->ring->buf) >= uploads_next_offset(&t->up, t->need) + t->need;
}

/* The ring is empty: a live source, or a reader catching its breath?  Wait the grace period, then deliver.  The grace period counts
 * from the moment the newest block was PUSHED, not from here (the wait for its upload lies in between): a live block's PDUs leave
 * grace after its arrival, whatever the copy took.
 * Ring mutex: held on entry and on return; dropped around the draining collection. */
static void grace_then_drain(struct fe_thread *t)
{
	struct block_connection *in = t->block->consumer.in;
	struct timespec until = t->last_push;
	until.tv_nsec += (long)(t->grace * 1e9);
	while (until.tv_nsec >= 1000000000) { until.tv_sec++; until.tv_nsec -= 1000000000; }
	const double tg = now_s();
	int rc = 0;
	while (rc == 0 && !next_block_is_there(t) && !block_connection_is_shutdown_signaled(in))
		rc = pthread_cond_timedwait(t->ring->cond, t->ring->mutex, &until);
	t->rs.grace_s += now_s() - tg;
	if (next_block_is_there(t) || block_connection_is_shutdown_signaled(in)) return;
	pthread_mutex_unlock(t->ring->mutex);
	deliver_pdus(t, true);
	t->rs.drains++;
	t->undelivered = 0;
	pthread_mutex_lock(t->ring->mutex);
}

/* A block that wraps around the end of a ring this library did not size: one copy.  The blocks still leased to the DMA engine sit
 * in front of it; they go back to the producer first.  Only a cf32 ring can be copied out of.
 * Ring mutex: held on entry and on return; dropped while the leased slots go back. */
static const void *bounce_block(struct fe_thread *t)
{
	pthread_mutex_unlock(t->ring->mutex);
	while (t->ok && t->up.leased > 0) release_copied(t, true);
	pthread_mutex_lock(t->ring->mutex);
	if (t->ok && t->bounce == NULL) t->bounce = hfdl_xcalloc(t->need, sizeof(float complex));
	if (t->ok && hfdl_ring_read(t->ring->buf, t->bounce, t->need) != t->need)
		fail(t, "input ring holds raw samples in blocks that are not contiguous");
	return t->bounce;
}

/* The next block to push: one uploaded ahead if there is one, else the next whole block of the ring, waited for.
 * TOOK_NOTHING: the run has failed; what the ring held was dropped, go round again (until the producer shuts down).
 * Ring mutex: not held on entry, not held on return. */
enum took { TOOK_BLOCK, TOOK_SHUTDOWN, TOOK_NOTHING };
static enum took take_block(struct fe_thread *t, const void **blk, bool *from_bounce)
{
	struct circ_buffer *ring = t->ring;
	*from_bounce = false;
	if (t->up.q_len > 0) {
		*blk = t->up.queued[t->up.q_head];            /* uploaded ahead: only its kernels remain to be queued */
		return TOOK_BLOCK;
	}
	bool waited_grace = false;
	pthread_mutex_lock(ring->mutex);
	/* shutdown is honoured only when there is not a whole block left, so buffered samples are flushed (src/fft.c:39-48) */
	while (!next_block_is_there(t)) {
		if (block_connection_is_shutdown_signaled(t->block->consumer.in)) {
			pthread_mutex_unlock(ring->mutex);
			return TOOK_SHUTDOWN;
		}
		if (t->ok && t->up.leased > 0) {
			/* the producer may be out of room: slots whose upload is done go back before this thread sleeps */
			pthread_mutex_unlock(ring->mutex);
			const double tr = now_s();
			release_copied(t, true);
			t->rs.release_s += now_s() - tr;
			pthread_mutex_lock(ring->mutex);
		} else if (t->ok && t->undelivered > 0 && !waited_grace) {
			grace_then_drain(t);
			waited_grace = true;
		} else {
			pthread_cond_wait(ring->cond, ring->mutex);
		}
	}
	*blk = t->ok ? hfdl_ring_peek(ring->buf, uploads_next_offset(&t->up, t->need), t->need) : NULL;
	if (t->ok && *blk == NULL) {
		*blk = bounce_block(t);
		*from_bounce = true;
	}
	if (!t->ok) hfdl_ring_drop(ring->buf, hfdl_ring_size(ring->buf));
	pthread_mutex_unlock(ring->mutex);
	if (!t->ok) {
		pthread_cond_signal(ring->cond);
		return TOOK_NOTHING;
	}
	return TOOK_BLOCK;
}

/* Push the block take_block() gave.  On failure nothing of ours may stay with the DMA engine: the queued copies are let finish, then
 * every slot is given up (the ring is emptied by the next take_block()).
 * Ring mutex: not held. */
static bool push_block(struct fe_thread *t, const void *blk, bool from_bounce)
{
	if (hfdl_gpu_frontend_push_block_raw(t->fe, blk, t->push_n, from_bounce ? t->bounce_fmt : t->gfmt, 0) != 0) {
		fail(t, hfdl_gpu_last_error());
		(void)hfdl_gpu_frontend_prefetch_cancel(t->fe);
		(void)hfdl_gpu_frontend_input_done(t->fe);
		uploads_forget(&t->up);
		return false;
	}
	t->rs.blocks++;
	t->undelivered++;
	if (t->up.q_len > 0) uploads_pushed_queued(&t->up);
	else uploads_pushed_direct(&t->up, !from_bounce);
	return true;
}

/* queue the uploads of every further whole block the ring holds already: they run beside the blocks still computing.
 * Ring mutex: not held; taken only to look at the ring. */
static void upload_ahead(struct fe_thread *t)
{
	while (t->up.q_len < t->up.depth) {
		pthread_mutex_lock(t->ring->mutex);
		const void *next = next_block_is_there(t) ? hfdl_ring_peek(t->ring->buf, uploads_next_offset(&t->up, t->need), t->need) : NULL;
		pthread_mutex_unlock(t->ring->mutex);
		if (next == NULL || hfdl_gpu_frontend_prefetch_block_raw(t->fe, next, t->push_n, t->gfmt) != 0) break;
		uploads_queued_ahead(&t->up, next);
	}
}

/* creates the front end for the channels registered on the connection, meets the channels at the start barrier (whether or not the
 * create worked) and opens the optional outputs; on any failure t->ok is false and do_exit is set */
static void frontend_setup(struct fe_thread *t, struct block *block)
{
	memset(t, 0, sizeof(*t));
	t->block = block;
	t->fb = container_of(block, struct gpu_fft_block, block);
	t->ring = &block->consumer.in->circ_buffer;
	struct gpu_fft_block *fb = t->fb;
	struct block_connection *down = block->producer.out;
	struct hfdl_channel_slot *slots[MAX_SLOTS];
	t->nch = hfdl_channels_on_connection(down, slots, MAX_SLOTS);
	t->freqs = hfdl_xcalloc(t->nch ? t->nch : 1, sizeof(int32_t));
	t->slots = hfdl_xcalloc(t->nch ? t->nch : 1, sizeof(*t->slots));
	for (size_t i = 0; i < t->nch; i++) { t->freqs[i] = slots[i]->frequency; t->slots[i] = slots[i]; }
	t->ok = true;
	if (t->nch == 0) {
		fail(t, "no channels connected");
	} else if (fb->real_base_khz >= 0 && hfdl_ring_format(t->ring->buf) == SFMT_CU8) {
		fail(t, "real input: CS16 or CF32 samples only");
	} else if (fb->real_base_khz >= 0
			/* the blocks around this one are wired for the equivalent complex stream (include/hfdl_host.h): the receiver's rate is twice theirs */
			? hfdl_gpu_frontend_create_real(&t->fe, fb->device, 2 * slots[0]->sample_rate, 1, &(int32_t){ 1000 * fb->real_base_khz }, t->freqs, &(int32_t){ (int32_t)t->nch }) != 0
			: hfdl_gpu_frontend_create(&t->fe, fb->device, slots[0]->sample_rate, slots[0]->centerfreq, t->freqs, (int32_t)t->nch) != 0) {
		fail(t, hfdl_gpu_last_error());
	} else {
		hfdl_gpu_frontend_geometry(t->fe, &fb->geo);
		hfdl_gpu_frontend_enable_taps(t->fe, 0);
		t->pdus = hfdl_xcalloc(PDU_BATCH, sizeof(*t->pdus));
		t->stats = hfdl_xcalloc(t->nch, sizeof(*t->stats));
		t->fs = (double)slots[0]->sample_rate;
		t->centerfreq = (double)slots[0]->centerfreq;
		if (fb->blanker_db != 0.f && hfdl_gpu_frontend_blanker_enable(t->fe, fb->blanker_db) != 0) fail(t, hfdl_gpu_last_error());
		if (t->ok && fb->iq_alpha != 0.f && hfdl_gpu_frontend_iqbal_enable(t->fe, -1, fb->iq_alpha) != 0) fail(t, hfdl_gpu_last_error());
		const char *why = NULL;
		if (t->ok && fb->notch.mu != 0.f && notch_start(t->fe, &fb->notch, t->freqs, t->nch, &why) != 0) fail(t, why);
	}
	pthread_barrier_wait(down->shared_buffer.consumers_ready);
	gettimeofday(&t->t0, NULL);
	t->need = t->ok ? (size_t)fb->geo.input_size : 1;
	t->gfmt = gpu_format_of(hfdl_ring_format(t->ring->buf));
	t->bounce_fmt = HFDL_GPU_SFMT_CF32;
	t->push_n = t->need;
	if (fb->real_base_khz >= 0) {
		t->gfmt = t->gfmt == HFDL_GPU_SFMT_CS16 ? HFDL_GPU_SFMT_RS16 : HFDL_GPU_SFMT_RF32;
		t->bounce_fmt = HFDL_GPU_SFMT_RF32;
		t->push_n = 2 * t->need;
	}
	if (t->ok && ((fb->spectrum.path != NULL && spectrum_csv_open(t) != 0)
			|| (fb->iqx.dir != NULL && iq_export_open(t->fe, fb, slots, t->nch, &t->iqx) != 0)
			|| (fb->frame_log != NULL && frame_log_open(t) != 0))) {
		do_exit = 1;
		t->ok = false;
	}
	if (t->ok) {
		/* uploads ahead of the pushes: what the library allows, and what the ring can hold beside the block being pushed and room
		 * for the producer to write into */
		const size_t ring_blocks = hfdl_ring_capacity(t->ring->buf) / t->need;
		size_t depth = (size_t)fb->geo.prefetch_depth;
		if (depth > HFDL_GPU_PREFETCH_MAX) depth = HFDL_GPU_PREFETCH_MAX;
		if (ring_blocks < 4) depth = 0; else if (depth > ring_blocks - 3) depth = ring_blocks - 3;
		t->up.depth = depth;
		t->grace = 0.25 * (double)t->need / t->fs;
	}
	if (t->grace > 0.020) t->grace = 0.020;
	if (t->grace < 0.0005) t->grace = 0.0005;
	clock_gettime(CLOCK_REALTIME, &t->last_push);
}

/* delivers what is still in the pipeline, finishes the optional outputs, publishes the run statistics (only a run that had a front
 * end has any), passes the shutdown on to the channels and frees everything */
static void frontend_teardown(struct fe_thread *t)
{
	if (t->fe) {
		deliver_pdus(t, true);                   /* what the lagging collection left behind */
		const double t_last = now_s();
		spectrum_csv_close(t);
		if (t->iqx.files != NULL) write_iq_export(t->fe, &t->iqx, 1);
		if (t->flog.file != NULL && t->flog.recs != NULL) write_frame_log(t, 1);
		hfdl_gpu_blanker_stats bs;
		if (t->fb->blanker_db != 0.f && hfdl_gpu_frontend_blanker_stats(t->fe, 0, &bs) == 0)
			fprintf(stderr, "blanker: receiver 0: %llu samples blanked in %llu blocks (%g dB)\n", (unsigned long long)bs.samples_blanked,
					(unsigned long long)bs.blocks, (double)t->fb->blanker_db);
		/* one line per receiver (a receiver the front end does not have has no record: its call fails and ends the list) */
		for (int32_t r = 0; t->fb->iq_alpha != 0.f && r < 64; r++) {
			hfdl_gpu_iqbal_stats is;
			if (hfdl_gpu_frontend_iqbal_stats(t->fe, r, &is) != 0) break;
			fprintf(stderr, "iq-correct: receiver %d: kappa %+.6f%+.6fj (image %.1f dB down), dc %+.6f%+.6fj, %llu of %llu blocks refused (alpha %g)\n", (int)r,
					(double)is.kappa_re, (double)is.kappa_im, (double)is.image_rejection_db, (double)is.dc_re, (double)is.dc_im,
					(unsigned long long)is.refused, (unsigned long long)is.blocks, (double)t->fb->iq_alpha);
		}
		/* one line per cancelled channel (a channel that was not selected has no record: its call fails and prints nothing) */
		for (size_t c = 0; t->fb->notch.mu != 0.f && c < t->nch; c++) {
			hfdl_gpu_notch_stats ns;
			if (hfdl_gpu_frontend_notch_stats(t->fe, (int32_t)c, &ns) == 0)
				fprintf(stderr, "notch: %d Hz: %llu blocks, %llu tap resets, last block %.4g -> %.4g, tap energy %.4g (mu %g)\n", t->freqs[c],
						(unsigned long long)ns.blocks, (unsigned long long)ns.resets, (double)ns.last_in_power, (double)ns.last_out_power,
						(double)ns.tap_energy, (double)t->fb->notch.mu);
		}
		publish_counters(t->fe, t->stats, (int32_t)t->nch);
		/* requests that never came due, or came in after the last push, are not the next front end's */
		pthread_mutex_lock(&g_retune_lock);
		g_retune.n = 0;
		g_retune_at_cnt = 0;
		pthread_mutex_unlock(&g_retune_lock);
		t->rs.samples = t->rs.blocks * (uint64_t)t->need;
		t->rs.seconds = t->rs.blocks ? t_last - t->t_first : 0.0;
		t->rs.bytes_per_sample = (int32_t)hfdl_ring_elem_size(t->ring->buf);
		t->rs.channels = (int32_t)t->nch;
		t->rs.block_samples = (int32_t)t->need;
		t->rs.zero_copy = hfdl_ring_is_pinned(t->ring->buf);
		pthread_mutex_lock(&g_run_lock);
		g_run = t->rs;
		pthread_mutex_unlock(&g_run_lock);
	}
	block_connection_one2many_shutdown(t->block->producer.out);
	if (t->fe) hfdl_gpu_frontend_destroy(t->fe);
	iq_export_close(&t->iqx);
	frame_log_close(&t->flog);
	free(t->bounce);
	free(t->pdus);
	free(t->stats);
	free(t->freqs);
	free(t->slots);
	t->block->running = false;
}

/* The front-end thread.  A block never gets copied on the host: the ring in front of this block is page-locked and a whole
 * number of blocks long (block_connect_one2one), so each block is handed to the GPU where it lies -- raw cs16 / cu8 samples
 * included, which the device converts -- and its slot goes back to the producer once the DMA has read it.
 *
 * Uploads run AHEAD of the blocks that compute: whatever whole blocks the ring holds beyond the one being pushed are queued for
 * upload at once (hfdl_gpu_frontend_prefetch_block_raw, up to geometry.prefetch_depth of them), so the copy engine keeps working
 * while this thread waits for the GPU in the collection call -- the fold of a 40 Msps x 256-channel half takes 3 ms, five blocks
 * of PCIe time.
 *
 * Live source or replay?  The pipeline is drained (everything pushed so far folded, demodulated and delivered at once) only when
 * the ring has run EMPTY and the source has stayed silent for a grace period of a quarter of a block's own duration (at most
 * 20 ms), counted from the arrival of the newest block: a live radio delivers a block every block duration and gets its PDUs
 * within that grace; a file reader that hiccups for a millisecond beside a GPU about as fast as itself never drains a filled
 * pipeline (round 4's fixed 0.5 ms grace did, five times in a run, for 19 % of the rate).
 *
 * The ring's mutex is never held across a call into the device library or a PDU delivery; every helper below says how it expects
 * and leaves the mutex. */
static void *frontend_thread(void *ctx)
{
	struct fe_thread t;
	frontend_setup(&t, ctx);
	double t_published = 0;
	for (;;) {
		const double tw0 = now_s();
		const void *blk = NULL;
		bool from_bounce = false;
		const enum took took = take_block(&t, &blk, &from_bounce);
		if (took == TOOK_SHUTDOWN) break;
		if (took == TOOK_NOTHING) continue;
		const double tw1 = now_s();
		clock_gettime(CLOCK_REALTIME, &t.last_push);
		if (t.rs.blocks == 0) t.t_first = tw1; else t.rs.wait_input_s += tw1 - tw0;
		retune_step(&t);
		if (!push_block(&t, blk, from_bounce)) continue;
		if (!from_bounce) upload_ahead(&t);
		if (t.csv.file != NULL) spectrum_csv_step(&t);
		if (t.iqx.files != NULL) write_iq_export(t.fe, &t.iqx, 0);
		const double tw2 = now_s();
		t.rs.push_s += tw2 - tw1;
		deliver_pdus(&t, false);
		if (t.flog.file != NULL) write_frame_log(&t, 0);
		const double tw3 = now_s();
		t.rs.collect_s += tw3 - tw2;
		release_copied(&t, false);               /* nothing is waited for here */
		t.rs.release_s += now_s() - tw3;
		/* the StatsD counters / gauges are read from the device every 50 ms of wall time at most: one strided device read per
		 * block would cost more than a block of a small geometry takes (a block is decoded in ~0.3 ms) */
		const double now = now_s();
		if (now - t_published >= 0.05) { publish_counters(t.fe, t.stats, (int32_t)t.nch); t_published = now; }
	}
	frontend_teardown(&t);
	return NULL;
}

size_t hfdl_frontend_block_samples(const struct block *sink)
{
	if (sink == NULL || sink->thread_routine != frontend_thread) return 0;
	return (size_t)container_of(sink, struct gpu_fft_block, block)->geo.input_size;
}

struct block *fft_create(int32_t decimation, float transition_bw)
{
	struct gpu_fft_block *fb = hfdl_xcalloc(1, sizeof(*fb));
	if (hfdl_gpu_plan_geometry(decimation, transition_bw, &fb->geo) != 0) {
		fprintf(stderr, "Error in fastddc_init()");
		free(fb);
		return NULL;
	}
	if (g_frame_log != NULL && (hfdl_gpu_frontend_quality_enable == NULL || hfdl_gpu_frontend_quality_read == NULL)) {
		fprintf(stderr, "frame log: this GPU library has no frame quality records\n");
		free(fb);
		return NULL;
	}
	if (g_blanker_db != 0.f && (hfdl_gpu_frontend_blanker_enable == NULL || hfdl_gpu_frontend_blanker_stats == NULL)) {
		fprintf(stderr, "blanker: this GPU library has no impulse-noise blanker\n");
		free(fb);
		return NULL;
	}
	if (g_iq_alpha != 0.f && (hfdl_gpu_frontend_iqbal_enable == NULL || hfdl_gpu_frontend_iqbal_stats == NULL)) {
		fprintf(stderr, "iq-correct: this GPU library has no I/Q imbalance corrector\n");
		free(fb);
		return NULL;
	}
	if (g_notch.mu != 0.f && (hfdl_gpu_frontend_notch_enable == NULL || hfdl_gpu_frontend_notch_stats == NULL)) {
		fprintf(stderr, "notch: this GPU library has no carrier canceller\n");
		free(fb);
		return NULL;
	}
	if (g_real_base_khz >= 0 && (hfdl_gpu_frontend_create_real == NULL || g_iq_alpha != 0.f)) {
		fputs(hfdl_gpu_frontend_create_real == NULL ? "real-input: this GPU library has no real-sampled input\n"
		                                            : "real-input: real samples have no I/Q to correct (iq-correct)\n", stderr);
		free(fb);
		return NULL;
	}
	fb->real_base_khz = g_real_base_khz;
	fb->blanker_db = g_blanker_db;
	fb->iq_alpha = g_iq_alpha;
	fb->notch = notch_settings_copy(&g_notch);
	fb->frame_log = g_frame_log ? strdup(g_frame_log) : NULL;
	fb->decimation = decimation;
	fb->transition_bw = transition_bw;
	fb->device = g_device;
	fb->spectrum = spectrum_settings_copy(&g_spectrum);
	fb->iqx = iq_export_settings_copy(&g_iqx);
	fb->block.producer.type = PRODUCER_MULTI;
	fb->block.producer.max_tu = (size_t)fb->geo.fft_size;
	fb->block.consumer.type = CONSUMER_SINGLE;
	fb->block.consumer.min_ru = (size_t)fb->geo.fft_size;
	fb->block.thread_routine = frontend_thread;
	return &fb->block;
}

void fft_destroy(struct block *fft_block)
{
	if (fft_block == NULL) return;
	struct gpu_fft_block *fb = container_of(fft_block, struct gpu_fft_block, block);
	spectrum_settings_free(&fb->spectrum);
	iq_export_settings_free(&fb->iqx);
	free(fb->frame_log);
	free(fb->notch.freqs_khz);
	free(fb);
}
