/* retune_requests.h -- the pure parts of retuning a channel from the host: the list of requests that waits for
 * the front-end thread, and the parser of a "SECONDS:OLD_KHZ:NEW_KHZ" option.  No locking, no device, no allocation: whoever shares a
 * list between threads guards it with a mutex.  tests/hostsim/retune_requests_check.cpp runs both under the sanitizers.  Plain C that a
 * C++ compiler takes as well.  frontend.c keeps the list (hfdl_frontend_retune), hfdl_replay.c parses the option. */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define HFDL_RETUNE_LIST_MAX 64

struct retune_request { int32_t old_freq, new_freq; };
struct retune_list { struct retune_request r[HFDL_RETUNE_LIST_MAX]; int32_t n; };

/* where a channel now on `freq` listens once every waiting request has been applied, in order */
static inline int32_t retune_list_resolve(const struct retune_list *l, int32_t freq)
{
	for (int32_t i = 0; i < l->n; i++) if (l->r[i].old_freq == freq) freq = l->r[i].new_freq;
	return freq;
}

/* Queue old_freq -> new_freq.  freqs[nfreqs]: the frequencies the channels listen on now.  old_freq must be what one of them listens on
 * once the waiting requests are applied (so a -> b, b -> c may be queued back to back), and new_freq must not be: two channels never
 * share a frequency, the host's bookkeeping is by frequency.  0, or -1: unknown old_freq, new_freq taken, or the list is full. */
static inline int retune_list_add(struct retune_list *l, const int32_t *freqs, int32_t nfreqs, int32_t old_freq, int32_t new_freq)
{
	int known = 0;
	for (int32_t i = 0; i < nfreqs; i++) {
		const int32_t f = retune_list_resolve(l, freqs[i]);
		if (f == new_freq) return -1;
		if (f == old_freq) known = 1;
	}
	if (!known || l->n == HFDL_RETUNE_LIST_MAX) return -1;
	l->r[l->n].old_freq = old_freq;
	l->r[l->n].new_freq = new_freq;
	l->n++;
	return 0;
}

/* hand every waiting request to the caller, oldest first; returns how many */
static inline int32_t retune_list_take(struct retune_list *l, struct retune_request *out)
{
	const int32_t n = l->n;
	for (int32_t i = 0; i < n; i++) out[i] = l->r[i];
	l->n = 0;
	return n;
}

/* "SECONDS:OLD_KHZ:NEW_KHZ" -> seconds of signal (>= 0, finite) and the two frequencies in Hz (kHz -> Hz as the channel list's are:
 * lround(1e3 * kHz)).  0, or -1 for anything else: a missing or empty field, trailing text, a negative or non-finite time. */
static inline int hfdl_parse_retune(const char *arg, double *seconds, int32_t *old_hz, int32_t *new_hz)
{
	double v[3];
	if (arg == NULL) return -1;
	for (int i = 0; i < 3; i++) {
		char *end = NULL;
		v[i] = strtod(arg, &end);
		if (end == arg || !isfinite(v[i]) || *end != (i < 2 ? ':' : '\0')) return -1;
		arg = end + 1;
	}
	if (v[0] < 0 || fabs(v[1]) > 2e6 || fabs(v[2]) > 2e6) return -1;
	*seconds = v[0];
	*old_hz = (int32_t)lround(1e3 * v[1]);
	*new_hz = (int32_t)lround(1e3 * v[2]);
	return 0;
}
