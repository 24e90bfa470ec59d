/* frontend_wrap_check.c -- the front-end thread in front of a ring the host library did NOT size: a page-locked cf32 ring that is
 * no whole number of blocks long, connected by hand, so that blocks wrap around the end of the storage and go through the thread's
 * bounce copy while earlier blocks are still leased to the uploads.  Linked with the host sources and gpu_standin.c; prints the PDUs
 * through the library's default pdu_decoder_queue_push().
 *
 *   frontend_wrap_check FILE.cf32 RING_SAMPLES */
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include "hfdl_host.h"
#include "host_internal.h"

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (f == NULL) return 2;
	fseek(f, 0, SEEK_END);
	const size_t nsamples = (size_t)ftell(f) / sizeof(float complex);
	rewind(f);
	float complex *samples = calloc(nsamples ? nsamples : 1, sizeof(*samples));
	if (samples == NULL || fread(samples, sizeof(*samples), nsamples, f) != nsamples) return 2;
	fclose(f);

	const int32_t fs = 250000, centerfreq = 10000000;
	int32_t decimation = compute_fft_decimation_rate(fs, HFDL_SYMBOL_RATE * SPS);
	float tbw = compute_filter_relative_transition_bw(fs, HFDL_CHANNEL_TRANSITION_BW_HZ);
	struct block *fft = fft_create(decimation, tbw);
	struct block *channels[2] = { hfdl_channel_create(fs, decimation, tbw, centerfreq, 10010000), hfdl_channel_create(fs, decimation, tbw, centerfreq, 10020000) };
	if (fft == NULL || channels[0] == NULL || channels[1] == NULL) return 2;

	/* what block_connect_one2one() makes, but for the ring's length */
	pthread_cond_t cond = PTHREAD_COND_INITIALIZER;
	pthread_mutex_t mutex = PTHREAD_MUTEX_INITIALIZER;
	struct block_connection conn = { .circ_buffer = { hfdl_ring_create_ex((size_t)atol(argv[2]), SFMT_CF32, 1), &cond, &mutex } };
	fft->consumer.in = &conn;
	if (block_connect_one2many(fft, 2, channels) != 2 || block_set_start(2, channels) != 2 || block_start(fft) != 1) return 2;

	/* the producer: whatever fits, as soon as it fits; never more than there is room for */
	size_t sent = 0;
	while (sent < nsamples && !do_exit) {
		pthread_mutex_lock(&mutex);
		size_t room = hfdl_ring_space_available(conn.circ_buffer.buf);
		pthread_mutex_unlock(&mutex);
		if (room > nsamples - sent) room = nsamples - sent;
		if (room > 0) complex_samples_produce(&conn.circ_buffer, samples + sent, room);
		else usleep(200);
		sent += room;
	}
	block_connection_one2one_shutdown(&conn);
	while (block_is_running(fft) || block_set_is_any_running(2, channels)) usleep(1000);

	block_disconnect_one2many(fft, 2, channels);
	hfdl_ring_destroy(conn.circ_buffer.buf);
	hfdl_channel_destroy(channels[0]);
	hfdl_channel_destroy(channels[1]);
	fft_destroy(fft);
	free(samples);
	return do_exit ? 1 : 0;
}
