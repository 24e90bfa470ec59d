"""The demodulator's LDS rings (dumphfdl_amd/csrc/demod_lds.h): results do not depend on where the launches cut the sample stream.

One channel of channelizer output (the oracle's, so that the oracle's PDUs are the reference) holding a 300 bps and an 1800 bps
single-slot burst is pushed through hfdl_gpu_frontend_push_baseband -- the demodulator and burst decoder alone, one launch per call -- cut
in different ways: launches as long as a call takes (a block: the reference cut), launches of R - 1, R, R + 1 and 2 R + 1 resampler outputs
(R = DM_RING = 256, the length of the per-sample rings) and launches of 33 input samples.  A single-slot burst lasts 2.34 s, so the stream
is 5.6 s long and no single launch can hold it (a call takes one block, and a launch less than a second of signal): the longest launches
stand in for "one launch".  Every stage tap, every PDU and every channel statistic must be the same 32 bits for every cut.
"""
import numpy as np
import pytest

import hfdl_synth as synth
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

R = 256                       # demod_lds.h DM_RING
CHUNK = 32                    # demod_lds.h DM_CHUNK
FS, CF, FREQ = 250000, 10_000_000, 10_021_000


@pytest.fixture(scope="module")
def stream(oracle):
    """The oracle's channelizer output of the one channel, end to end, and the oracle's PDUs."""
    rng = np.random.default_rng(29)
    bursts = [dict(freq=FREQ, mode=0, octets=synth.make_pdu(rng, 0), t0=0.20, amp=0.1, cfo=4.0),       # 300 bps, single slot
              dict(freq=FREQ, mode=3, octets=synth.make_pdu(rng, 3), t0=2.95, amp=0.08, cfo=-7.0)]     # 1800 bps, single slot
    dur = 5.6
    x = synth.synth_wideband(FS, CF, int(dur * FS), bursts, noise_sigma=0.004, seed=31)                # > 20 dB in the channel
    ora = oracle.Frontend(FS, CF, [FREQ])
    n, parts = ora.ddc.input_size, []
    for b in range(len(x) // n):
        ora.push_block(x[b * n:(b + 1) * n])
        parts.append(np.array(ora.channel_view(0)["chan_out"], np.complex64))
    pdus = sorted((p["mode"], p["octets"]) for p in ora.pdus)
    ora.close()
    assert [m for m, _ in pdus] == [0, 3], "the oracle decodes both bursts on this input"
    assert [(m, o[:len(b["octets"])]) for (m, o), b in zip(pdus, bursts)] == [(b["mode"], b["octets"]) for b in bursts]
    return np.concatenate(parts), pdus


class Cutter:
    """Input samples per launch for a wanted number of resampler outputs: the device's own 24-bit phase arithmetic (demod_core.h)."""

    def __init__(self, rate):
        self.step = int(round(float(1 << 24) / rate))          # demod_tables.h rs_step
        self.phase = 0

    def outputs(self, n_in):
        total = n_in << 24
        return (total - self.phase + self.step - 1) // self.step if self.phase < total else 0

    def take(self, n_in):
        n_out = self.outputs(n_in)
        self.phase += n_out * self.step - (n_in << 24)
        return n_out

    def inputs_for(self, n_out):
        n_in = max(1, (self.phase + (n_out - 1) * self.step) >> 24)
        while self.outputs(n_in) < n_out:
            n_in += 1
        return n_in


def run(gpu, x, cut):
    """cut(cutter, samples left, launch index) -> input samples of the next launch.  Returns the concatenated taps, the PDUs, the statistics
    and the first output sample of every launch."""
    fe = gpu.Frontend(FS, CF, [FREQ])
    g = fe.geometry
    cutter = Cutter(float(g.resamp_rate))
    taps = {k: [] for k in (F.TAP_RESAMPLED, F.TAP_MF_OUT, F.TAP_SYMBOLS, F.TAP_AGC_LEVEL)}
    pdus, starts, at, done, i = [], [], 0, 0, 0
    while at < len(x):
        n_in = min(cut(cutter, len(x) - at, i), len(x) - at, g.max_outputs_per_block)
        fe.push_baseband([x[at:at + n_in]])
        at += n_in
        i += 1
        n_out = cutter.take(n_in)
        for k in taps:
            taps[k].append(fe.read_tap(k, 0))
        assert len(taps[F.TAP_RESAMPLED][-1]) == n_out == len(taps[F.TAP_MF_OUT][-1]) == len(taps[F.TAP_AGC_LEVEL][-1])
        starts.append(done)
        done += n_out
        pdus += fe.poll_pdus()
    stats = fe.all_channel_stats()
    fe.close()
    bits = {k: np.concatenate(v).view(np.uint32) for k, v in taps.items()}
    return bits, pdus, stats, np.array(starts + [done])


@pytest.fixture(scope="module")
def whole(gpu, stream):
    """The reference cut: every launch as long as a call takes."""
    return run(gpu, stream[0], lambda c, left, i: 1 << 30)


def same(a, b):
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), "tap %d differs" % k
    assert a[1] == b[1], "PDUs differ"
    assert a[2] == b[2], "channel statistics differ"


def test_the_longest_launches_decode_what_the_oracle_decodes(stream, whole):
    assert sorted((p["mode"], p["octets"]) for p in whole[1]) == stream[1]
    assert whole[3][-1] > 14 * R and int(np.max(np.diff(whole[3]))) > 2 * R        # many turns of the rings in all, more than two per launch


@pytest.mark.parametrize("outputs", [R - 1, R, R + 1, 2 * R + 1])
def test_launches_around_the_ring_length_change_nothing(gpu, stream, whole, outputs):
    got = run(gpu, stream[0], lambda c, left, i: c.inputs_for(outputs))
    assert set(np.diff(got[3])[:-1]) == {outputs}
    same(whole, got)
    assert sorted((p["mode"], p["octets"]) for p in got[1]) == stream[1]


def test_launches_of_33_input_samples_change_nothing(gpu, stream, whole):
    same(whole, run(gpu, stream[0], lambda c, left, i: 33))


def test_a_detection_beside_the_ring_wrap_changes_nothing(gpu, stream, whole):
    """The second burst's preamble detection (the PDU's sample_index: the sample that completed A2) is placed within one chunk of a wrap of
    the rings: launches of 2 R + 64 outputs behind a first launch sized so that the detection's index in its launch is a multiple of R,
    a few samples more or less."""
    det = sorted(p["sample_index"] for p in whole[1])[-1]
    length = 2 * R + 64
    first = (det - R - 5) % length or length                    # the detection then sits at index R + 5 of its launch
    got = run(gpu, stream[0], lambda c, left, i: c.inputs_for(first if i == 0 else length))
    same(whole, got)
    starts = got[3]
    at = det - starts[np.searchsorted(starts, det, side="right") - 1]      # the detection's index in its launch, from what was reported
    assert min(at % R, R - at % R) <= CHUNK and at >= R, (det, at)
