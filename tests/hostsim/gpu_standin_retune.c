/* gpu_standin_retune.c -- gpu_standin.c plus hfdl_gpu_frontend_retune_channel(), for running the host library's retune path
 * (host/frontend.c retune_step) on a CPU.  The plain stand-in has no such entry point: linked with it, the host library finds the weak
 * symbol null and refuses every request.
 *
 * What it models: the boundary.  A PDU carries the frequency its channel listened on when its block was PUSHED, however late it is
 * polled -- the stand-in makes its PDUs when they are polled, labelled with fe->freq0, so the two poll entry points are wrapped here and
 * put the frequency of the PDU's host block back (every stand-in PDU is channel 0's and names its host block in its first eight
 * octets).  A retune of channel 0 records the boundary (the next host block to be queued -- blocks uploaded ahead of their push lie
 * behind it, as they do in the library) and sets fe->freq0, which the statistics report; other channels only count.
 *
 * The boundary rule is therefore THIS FILE's model (first_block = the next host block to be queued; relabelling at poll time), not
 * frontend.c's: what a run against it checks of frontend.c is where retune_step() sits relative to push_block() and the uploads ahead,
 * that every request reaches the entry point once and in order, and what the thread does with a refusal.
 *
 * Statistics: channel 0 counts one A2 detection per pushed block.  As the library does, the stand-in reports a retuned channel's
 * counters as a fresh channel's from the call on (pushes since the boundary).  HFDL_STANDIN_STATS_LAG = L > 0 models a library that
 * does NOT: for L more pushes (or until a draining poll) the old counter is still what the statistics show, and then it drops -- the
 * host must neither count "up" to the smaller value nor hang.
 *
 * Read from the environment at every call:
 *   HFDL_STANDIN_FAIL_RETUNE  k >= 1: the k-th call fails with HFDL_STANDIN_FAIL_TEXT in hfdl_gpu_last_error() and changes nothing
 *   HFDL_STANDIN_STATS_LAG    L >= 0: see above (default 0)
 *   HFDL_STANDIN_RETUNE_COUNT path: rewritten at every call with the number of calls so far (refused ones included) */
#include "hfdl_gpu.h"
#define hfdl_gpu_frontend_poll_pdus standin_poll_pdus
#define hfdl_gpu_frontend_poll_pdus_ready standin_poll_pdus_ready
#define hfdl_gpu_frontend_all_channel_stats standin_all_channel_stats
#include "gpu_standin.c"
#undef hfdl_gpu_frontend_poll_pdus
#undef hfdl_gpu_frontend_poll_pdus_ready
#undef hfdl_gpu_frontend_all_channel_stats

#define BOUNDARIES_MAX 64
static struct { uint64_t first_block; int32_t freq; } g_bounds[BOUNDARIES_MAX];      /* one front end at a time uses this file */
static int g_nbounds;
static long g_retune_calls;
static uint64_t g_count_from;            /* channel 0's counter = pushes - this */
static uint64_t g_count_from_next;       /* pushes at the newest boundary: becomes g_count_from when the reset "runs" ... */
static uint64_t g_reset_at;              /* ... once this many blocks have been pushed (a lagging library) or a draining poll has run */
static int g_reset_pending;
static void reset_runs(void) { g_count_from = g_count_from_next; g_reset_pending = 0; }

int hfdl_gpu_frontend_retune_channel(hfdl_gpu_frontend *fe, int32_t channel, int32_t new_freq_hz)
{
	g_retune_calls++;
	const char *e = getenv("HFDL_STANDIN_RETUNE_COUNT");
	if (e != NULL) {
		FILE *f = fopen(e, "w");
		if (f != NULL) { fprintf(f, "%ld\n", g_retune_calls); fclose(f); }
	}
	if (fe == NULL || channel < 0 || channel >= fe->geo.channels) return set_error(HFDL_GPU_EINVAL, "retune: bad argument");
	if ((e = getenv("HFDL_STANDIN_FAIL_RETUNE")) != NULL && atol(e) == g_retune_calls)
		return set_error(HFDL_GPU_EINVAL, getenv("HFDL_STANDIN_FAIL_TEXT") ? getenv("HFDL_STANDIN_FAIL_TEXT") : "injected retune failure");
	if (channel != 0) return 0;
	if (g_nbounds == BOUNDARIES_MAX) return set_error(HFDL_GPU_ENOMEM, "retune: too many boundaries for the stand-in");
	if (g_nbounds == 0) { g_bounds[0].first_block = 0; g_bounds[0].freq = fe->freq0; g_nbounds = 1; }
	/* the blocks uploaded ahead have not been pushed: they come after the boundary although their host block numbers are taken */
	g_bounds[g_nbounds].first_block = fe->nblk - fe->prefetched;
	g_bounds[g_nbounds].freq = new_freq_hz;
	g_nbounds++;
	fe->freq0 = new_freq_hz;
	e = getenv("HFDL_STANDIN_STATS_LAG");
	g_reset_at = fe->pushes + (uint64_t)(e != NULL ? atol(e) : 0);
	g_count_from_next = fe->pushes;
	g_reset_pending = 1;
	if (fe->pushes >= g_reset_at) reset_runs();
	return 0;
}

int hfdl_gpu_frontend_all_channel_stats(hfdl_gpu_frontend *fe, hfdl_gpu_channel_stats *out, int32_t cap, int32_t *n)
{
	const int rc = standin_all_channel_stats(fe, out, cap, n);
	if (rc != 0) return rc;
	if (g_reset_pending && fe->pushes >= g_reset_at) reset_runs();
	out[0].a2_found = (uint32_t)(fe->pushes - g_count_from);
	return 0;
}

static void relabel(hfdl_gpu_pdu *out, int32_t n)
{
	for (int32_t i = 0; g_nbounds > 0 && i < n; i++) {
		uint64_t block = 0;
		for (int b = 0; b < 8; b++) block |= (uint64_t)out[i].octets[b] << (8 * b);
		for (int k = 0; k < g_nbounds; k++) if (g_bounds[k].first_block <= block) out[i].freq = g_bounds[k].freq;
	}
}

int hfdl_gpu_frontend_poll_pdus(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n)
{
	const int rc = standin_poll_pdus(fe, out, max, n);
	if (g_reset_pending) reset_runs();      /* a drain: every queued reset has run */
	if (rc == 0) relabel(out, *n);
	return rc;
}

int hfdl_gpu_frontend_poll_pdus_ready(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n, int32_t max_in_flight)
{
	/* (the stand-in's own max_in_flight == 0 case calls the draining poll above through its renamed name: relabelled here either way) */
	const int rc = standin_poll_pdus_ready(fe, out, max, n, max_in_flight);
	if (rc == 0) relabel(out, *n);
	return rc;
}
