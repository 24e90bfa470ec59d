/* gpu_standin_quality.c -- gpu_standin.c plus hfdl_gpu_frontend_quality_enable() / _quality_read(), for running the host library's frame
 * log (host/frontend.c write_frame_log) on a CPU.  The plain stand-in has no such entry points: linked with it, the host library finds
 * the weak symbols null and fft_create() refuses a frame log.
 *
 * What it models: one record per PDU, complete no earlier than its PDU -- the stand-in makes its PDUs when they are polled, so the two
 * poll entry points are wrapped here and queue a record for every PDU they hand out: same channel, frequency and sample index, a
 * single-slot BPSK frame with err_power 0.01 (MER 20 dB), unit power, gain 0.6 + 0.8j and segment 5 the worst at 0.1 (10 dB).  What a run
 * against it checks of frontend.c: where the reads sit, that every record becomes one line with its PDU's time and frequency, and that
 * the read at shutdown waits. */
#include "hfdl_gpu.h"
#define hfdl_gpu_frontend_poll_pdus standin_poll_pdus
#define hfdl_gpu_frontend_poll_pdus_ready standin_poll_pdus_ready
#include "gpu_standin.c"
#undef hfdl_gpu_frontend_poll_pdus
#undef hfdl_gpu_frontend_poll_pdus_ready

#define QUEUE_MAX 65536
static struct { uint64_t sample_index; int32_t channel, freq; } g_queue[QUEUE_MAX];      /* one front end at a time uses this file */
static uint32_t g_made, g_read, g_dropped;
static int32_t g_ring;

static void record(const hfdl_gpu_pdu *out, int32_t n)
{
	for (int32_t i = 0; g_ring > 0 && i < n; i++) {
		if (g_made - g_read >= (uint32_t)g_ring) { g_dropped++; continue; }
		g_queue[g_made % QUEUE_MAX].sample_index = out[i].sample_index;
		g_queue[g_made % QUEUE_MAX].channel = out[i].channel;
		g_queue[g_made % QUEUE_MAX].freq = out[i].freq;
		g_made++;
	}
}

int hfdl_gpu_frontend_poll_pdus(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n)
{
	const int rc = standin_poll_pdus(fe, out, max, n);
	if (rc == 0) record(out, *n);
	return rc;
}

int hfdl_gpu_frontend_poll_pdus_ready(hfdl_gpu_frontend *fe, hfdl_gpu_pdu *out, int32_t max, int32_t *n, int32_t max_in_flight)
{
	/* (the stand-in's own max_in_flight == 0 case calls the draining poll above through its renamed name: recorded here either way) */
	const int rc = standin_poll_pdus_ready(fe, out, max, n, max_in_flight);
	if (rc == 0) record(out, *n);
	return rc;
}

int hfdl_gpu_frontend_quality_enable(hfdl_gpu_frontend *fe, int32_t ring_frames, uint32_t flags)
{
	if (fe == NULL || (flags & ~HFDL_GPU_QUALITY_SYMBOLS) != 0 || (ring_frames != 0 && (ring_frames < 2 || ring_frames > HFDL_GPU_QUALITY_RING_MAX)))
		return set_error(HFDL_GPU_EINVAL, "quality_enable: bad argument");
	g_ring = ring_frames;
	g_made = g_read = g_dropped = 0;
	return 0;
}

int hfdl_gpu_frontend_quality_read(hfdl_gpu_frontend *fe, hfdl_gpu_frame_quality *out, float *symbols, int32_t max_frames, int32_t *n,
		uint32_t *dropped, int wait)
{
	(void)wait;
	if (n == NULL || max_frames < 0 || (out == NULL && max_frames > 0) || fe == NULL || g_ring == 0 || symbols != NULL)
		return set_error(HFDL_GPU_EINVAL, "quality_read: bad argument");
	*n = 0;
	for (; *n < max_frames && g_read != g_made; g_read++, (*n)++) {
		hfdl_gpu_frame_quality *q = &out[*n];
		memset(q, 0, sizeof(*q));
		q->sample_index = g_queue[g_read % QUEUE_MAX].sample_index;
		q->channel = g_queue[g_read % QUEUE_MAX].channel;
		q->freq = g_queue[g_read % QUEUE_MAX].freq;
		q->mode = 0; q->nsym = 2160; q->segments = 72;
		q->sym_power = 1.0f; q->err_power = 0.01f; q->err_max = 0.2f; q->gain_re = 0.6f; q->gain_im = 0.8f;
		for (int s = 0; s < 72; s++) q->seg_err_power[s] = s == 5 ? 0.1f : 0.00875f;
	}
	if (dropped != NULL) *dropped = g_dropped;
	return 0;
}
