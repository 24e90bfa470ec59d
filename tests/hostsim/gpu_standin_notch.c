/* gpu_standin_notch.c -- gpu_standin.c plus hfdl_gpu_frontend_notch_enable() / _notch_stats(), for running the host library's carrier
 * canceller switch (host/frontend.c notch_start, hfdl_replay --notch) on a CPU.  The plain stand-in has no such entry points: linked with
 * it, the host library finds the weak symbols null and fft_create() refuses.
 *
 * What it models: the call's arguments, kept and printed -- one line "STANDIN notch_enable mu=MU nsel=N channels=a,b,..." on stderr --
 * and a record per selected channel whose `blocks` is the number of blocks pushed.  What a run against it checks of frontend.c and
 * hfdl_replay.c: that the step and the selection arrive, frequencies turned into channel indices, and that every selected channel and
 * no other gets its line at the end. */
#include <stdio.h>
#include "hfdl_gpu.h"
#define hfdl_gpu_frontend_push_block_raw standin_push_block_raw
#include "gpu_standin.c"
#undef hfdl_gpu_frontend_push_block_raw

#define NOTCH_CH_MAX 4096
static unsigned char g_selected[NOTCH_CH_MAX];       /* one front end at a time uses this file */
static int g_all, g_on;
static uint64_t g_blocks;

int hfdl_gpu_frontend_push_block_raw(hfdl_gpu_frontend *fe, const void *raw, size_t nsamples, int sample_format, int on_device)
{
	const int rc = standin_push_block_raw(fe, raw, nsamples, sample_format, on_device);
	if (rc == 0 && g_on) g_blocks++;
	return rc;
}

int hfdl_gpu_frontend_notch_enable(hfdl_gpu_frontend *fe, const int32_t *channels, int32_t nsel, float mu)
{
	if (!(mu == 0.f || (mu >= 1e-5f && mu <= 0.05f)) || fe == NULL || nsel < 0 || nsel > NOTCH_CH_MAX || (nsel > 0 && channels == NULL))
		return set_error(HFDL_GPU_EINVAL, "notch_enable: bad argument");
	memset(g_selected, 0, sizeof(g_selected));
	for (int32_t i = 0; i < nsel; i++) {
		if (channels[i] < 0 || channels[i] >= NOTCH_CH_MAX || g_selected[channels[i]]) return set_error(HFDL_GPU_EINVAL, "notch_enable: channel out of range or listed twice");
		g_selected[channels[i]] = 1;
	}
	g_all = nsel == 0;
	g_on = mu != 0.f;
	g_blocks = 0;
	fprintf(stderr, "STANDIN notch_enable mu=%g nsel=%d channels=", (double)mu, nsel);
	for (int32_t i = 0; i < nsel; i++) fprintf(stderr, "%s%d", i ? "," : "", channels[i]);
	fprintf(stderr, "\n");
	return 0;
}

int hfdl_gpu_frontend_notch_stats(hfdl_gpu_frontend *fe, int32_t channel, hfdl_gpu_notch_stats *out)
{
	if (fe == NULL || out == NULL || channel < 0 || channel >= NOTCH_CH_MAX || !g_on || !(g_all || g_selected[channel]))
		return set_error(HFDL_GPU_EINVAL, "notch_stats: bad argument, or the channel is not selected");
	memset(out, 0, sizeof(*out));
	out->blocks = g_blocks;
	out->last_in_power = 2.f;
	out->last_out_power = 1.f;
	out->tap_energy = 0.03125f;
	return 0;
}
