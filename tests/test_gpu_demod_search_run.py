"""The demodulator's searching paths (dumphfdl_amd/csrc/demod_core.h): the carrier wave's searching run -- behind a searching symbol that
found nothing, the following ones of the chunk go through one tight loop instead of the general per-output iteration -- and the
timing-recovery wave's straight-line first output per input sample, with the division by three moved from that wave to the carrier wave's
per-chunk load.  What a run can get wrong is where it ends: on a detection (the symbol before it, the symbol itself, the symbol after it),
in front of a carrier run-away's single step, at a chunk's last pair, at a launch's end; and where it starts again: behind a frame, behind
a reset of the timing loop (a restart of wave 1 from the reset state, then its chunks with masked window entries).

Built like tests/test_gpu_demod_frame_active.py.  The stage runs alone (hfdl_gpu_frontend_push_baseband) on the ORACLE's channelizer
output, 250 ksps, two channels, channel 1 noise only.  The reference is the strict build of the same tree (build/strict/
libhfdl_gpu_strict_15.so: the one-lane serial loop of tests/hostsim/serial_demod.h with roundf and x / 3.0f as liquid writes them, which
knows nothing of chunks, runs or waves): every stage tap, every PDU field and every channel statistic of the product build must be the
same 32-bit words, launch for launch; the PDUs must also be the oracle's.  No tolerance anywhere.

Chunk positions: a first launch of o = 1 .. 32 outputs, then launches of 512, puts the sample with stream index g at position
(g - o) mod 32 of its chunk: every event at every position of a chunk once, and on launch boundaries.

Events on channel 0 (event_stream): an A1 detection; a burst cut off inside its second A sequence (the preamble search fails, the framer
resets the timing loop, the search starts again behind the reset); two bursts back to back (search -> frame -> search within a few
chunks); a carrier run-away while searching -- a BPSK-modulated carrier without a preamble whose offset sweeps away at 300 Hz / s, which
the carrier loop follows until |dphi| passes 0.25 (the stream of tests/demod_loops_f64.py stream_c), ADDED to the oracle's channelizer
output of channel 0 at the channel's rate (the wideband synthesiser has no swept carrier).  Every case asserts on the CPU, before anything
runs on the device, that the oracle alone produces the event: the bursts decoded, the failed search counted by the oracle, the run-away
counted by the float64 model (tests/demod_loops_f64.py) on the oracle's matched-filter output of that stretch.

Timing loop off its rate (off_rate_stream): noise plus a burst whose sample clock is off by 1000 ppm, ten times the largest offset of the
float64 model tests' streams: the loop pulls in (the oracle decodes: asserted) with its rate register away from 3 / 2, and input samples
with no output and with one output alternate out of the 1, 1, 0 pattern.  From the reset rate of 3 / 2 no input makes an input sample
yield TWO outputs: that needs del = rate + q_hat below 1, |q_hat| <= b0 / (1 - |a1|) = 0.037, and one loop-filter update moves the rate by
at most rate_adj * 0.037 = 1.8e-5 -- half a unit takes 27 000 updates (15 s) of a timing error saturated at one sign.  The timing-recovery
wave's second to fourth output of a sample is therefore reached through a TEST-ONLY pair of builds whose start rate is 1.0005 instead of
3 / 2 (-DHFDL_DM_SS_RATE0, dumphfdl_amd/csrc/build_start_rate.sh: the product's sources and the strict build, every object of both with
the same flag).  With del around 1 the same stream gives input samples with 0, 1 and 2 outputs (asserted on the CPU with the float64
model started from the same rate), and the product-source build must equal the strict one word for word as everywhere else.  That pair
decodes nothing worth comparing with the oracle, whose loop starts from 3 / 2.

No-frame timeout (timeout_stream): 31 s of noise on both channels; after 13 frames' worth of symbols without a frame the framer re-centres
the loops.  That symbol ends a searching run by its count.  One case: the position in the chunk is whatever it is.  The CPU condition is
the float64 model's symbol counter, which starts again at the timeout."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hfdl_synth as synth
from dumphfdl_amd import frontend as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import demod_loops_f64 as M
from test_gpu_demod_frame_active import Cutter      # input samples per launch for a wanted number of outputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 32                                    # demod_lds.h DM_CHUNK
FS, CF = 250000, 10_000_000
FREQS = [10_021_000, 9_958_000]               # channel 1 carries noise only: it never gets past the preamble search
TAPS = (F.TAP_RESAMPLED, F.TAP_MF_OUT, F.TAP_SYMBOLS, F.TAP_AGC_LEVEL)
PDU_KEY = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
BLOCK = 896                                   # baseband samples per oracle call (the 250 ksps geometry's block)


@pytest.fixture(scope="module")
def strict(gpu):
    """The strict build of this tree with the four fast forms on, loaded beside the product library."""
    lib = os.path.join(ROOT, "build", "strict", "libhfdl_gpu_strict_15.so")
    product = os.path.join(ROOT, "dumphfdl_amd", "libhfdl_gpu.so")
    if not (os.path.exists(lib) and os.path.getmtime(lib) >= os.path.getmtime(product)):
        subprocess.check_call(["bash", os.path.join(ROOT, "dumphfdl_amd", "csrc", "build_strict.sh"), "15"], stdout=subprocess.DEVNULL)
    return F._bind(ctypes.CDLL(lib, mode=ctypes.RTLD_LOCAL))


@pytest.fixture(scope="module")
def start_rate_pair(gpu):
    """The test-only pair with the timing loop's start rate overridden: (the product's sources, the strict build)."""
    d = os.path.join(ROOT, "build", "start_rate")
    libs = [os.path.join(d, "libhfdl_gpu_rate.so"), os.path.join(d, "libhfdl_gpu_rate_strict.so")]
    product = os.path.join(ROOT, "dumphfdl_amd", "libhfdl_gpu.so")
    if not all(os.path.exists(l) and os.path.getmtime(l) >= os.path.getmtime(product) for l in libs):
        subprocess.check_call(["bash", os.path.join(ROOT, "dumphfdl_amd", "csrc", "build_start_rate.sh"), START_RATE], stdout=subprocess.DEVNULL)
    return [F._bind(ctypes.CDLL(l, mode=ctypes.RTLD_LOCAL)) for l in libs]


def channelize(oracle, x):
    """The oracle's channelizer output of both channels, end to end."""
    ora = oracle.Frontend(FS, CF, FREQS)
    size, parts = ora.ddc.input_size, [[], []]
    for b in range(len(x) // size):
        ora.push_block(x[b * size:(b + 1) * size])
        for c in range(2):
            parts[c].append(np.array(ora.channel_view(c)["chan_out"], np.complex64))
    ora.close()
    return [np.concatenate(p) for p in parts]


def oracle_demod(oracle, chan, freq):
    """The oracle's demodulator alone on one channel's baseband: its PDUs, its counters, its matched-filter output and AGC levels."""
    ch = oracle.Channel(FS, CF, freq, want_channelizer=False)
    mf, lvl = [], []
    for i in range(0, len(chan), BLOCK):
        ch.process_baseband(chan[i:i + BLOCK])
        v = ch.view()
        mf.append(v["mf_out"])
        lvl.append(v["agc_level"])
    pdus, summary = list(ch.pdus), ch.summary()
    ch.close()
    return pdus, summary, np.concatenate(mf), np.concatenate(lvl)


def burst(rng, mode, t0, amp=0.1, cfo=4.0):
    return dict(freq=FREQS[0], mode=mode, octets=synth.make_pdu(rng, mode), t0=t0, amp=amp, cfo=cfo)


def sent_and_decoded(pdus, bursts):
    """Every burst comes back, in order, with its mode and its octets."""
    got = sorted(pdus, key=lambda p: p["sample_index"])
    return len(got) == len(bursts) and all(g["mode"] == b["mode"] and g["octets"][:len(b["octets"])] == b["octets"] for g, b in zip(got, bursts))


START_RATE = "1.0005f"                        # the test-only builds' timing loop starts here (module docstring)


class StartRateModel(M.DemodLoopsF64):
    """The float64 model with the timing loop's reset rate of the test-only builds."""

    def ss_reset(self):
        super().ss_reset()
        self.rate = self.delta = float(np.float32(float(START_RATE.rstrip("f"))))


def model_on(mf, lvl, rate, t0, t1, model=M.DemodLoopsF64):
    """The float64 model, started in the search, over the oracle's matched-filter output between t0 and t1 seconds."""
    m = model()
    a, b = int(t0 * rate), int(t1 * rate)
    m.push(mf[a:b], lvl[a:b])
    return m


@pytest.fixture(scope="module")
def event_stream(oracle):
    """Channel 0: an 1800 bps burst, a burst cut off 20 symbols into its second A sequence, a swept carrier that runs the carrier loop
    away, two bursts back to back (300 bps BPSK, 1200 bps QPSK).  Channel 1: noise."""
    rng = np.random.default_rng(77)
    t_cut = 3.0
    cut_off = burst(rng, 1, t_cut)
    t_a2 = t_cut + (448 + 127 + 20) / 1800.0
    t_sw0, t_sw1 = t_a2 + 0.04, t_a2 + 0.64      # behind the cut-off burst, while the AGC still stands at its level (see below)
    t_b2b = 4.3
    first = burst(rng, 0, t_b2b, cfo=-6.0)
    second = burst(rng, 2, t_b2b + synth.burst_symbols_len(0) / 1800.0 + 0.02, amp=0.08, cfo=5.0)
    whole = [burst(rng, 3, 0.2, amp=0.08, cfo=-7.0), first, second]
    dur = second["t0"] + synth.burst_symbols_len(2) / 1800.0 + 0.4
    n = int(dur * FS)
    x = synth.synth_wideband(FS, CF, n, whole, noise_sigma=0.004, seed=83)
    x[:int(t_a2 * FS)] += synth.synth_wideband(FS, CF, n, [cut_off])[:int(t_a2 * FS)]
    chan = channelize(oracle, x)
    # the swept carrier, at the channel's rate and at the level the bursts have there
    rate = FS / (len(x) // len(chan[0]))
    assert abs(rate - M.FS_IN) < 1e-9 and len(x) // len(chan[0]) * len(chan[0]) <= len(x)
    t = np.arange(len(chan[0])) / rate
    level = float(np.sqrt(np.mean(np.abs(chan[0][int(1.0 * rate):int(2.0 * rate)]) ** 2)))      # inside the first burst
    sym = 1.0 - 2.0 * rng.integers(0, 2, int((t_sw1 - t_sw0) * 1800) + 8)
    ph = 2.0 * np.pi * 0.5 * 180.0 / (t_sw1 - t_sw0) * (t - t_sw0) ** 2
    sweep = np.where((t >= t_sw0) & (t < t_sw1), level * synth.shape_burst(sym.astype(np.complex64), rate, t_sw0, len(t)) * np.exp(1j * ph), 0.0)
    chan[0] = (chan[0] + sweep).astype(np.complex64)
    # ---- on the CPU, before anything runs on the device: the oracle alone produces every event
    pdus, summary, mf, lvl = oracle_demod(oracle, chan[0], FREQS[0])
    assert sent_and_decoded(pdus, whole), "the oracle decodes the three whole bursts and nothing of the cut-off one or the sweep"
    assert summary["m1_found"] == 3 and summary["a1_found"] > summary["a2_found"] >= 3, "a preamble search failed and reset the timing loop"
    away = model_on(mf, lvl, 5400.0, 0.0, t_sw1 + 0.05)             # the whole stream up to behind the sweep, from the stream's start
    print("float64 model up to behind the sweep: run-aways %d, counters %s" % (away.resets_runaway, away.cnt))
    assert away.resets_runaway >= 1, "the carrier loop runs away while the framer searches"
    assert away.cnt["frames"] == 1 and away.cnt["a1_found"] > away.cnt["a2_found"] >= 1, "the model's framer went the oracle's way before it"
    idle, _, _, _ = oracle_demod(oracle, chan[1], FREQS[1])
    assert idle == []
    return chan, sorted(PDU_KEY(p) for p in pdus)


@pytest.fixture(scope="module")
def off_rate_stream(oracle):
    """Noise, then a burst whose sample clock runs 1000 ppm fast (module docstring)."""
    rng = np.random.default_rng(91)
    b = burst(rng, 1, 0.5, cfo=3.0)
    dur = b["t0"] + synth.burst_symbols_len(1) / 1800.0 + 0.3
    x = synth.synth_wideband(FS, CF, int(dur * FS), [b], noise_sigma=0.004, seed=92)
    chan = channelize(oracle, x)
    # resampled: sample i of the new stream is the old stream at i * (1 + 1e-3), linear interpolation between neighbours of a stream
    # that is oversampled four times
    for c in range(2):
        at = np.arange(int((len(chan[c]) - 2) / 1.001)) * 1.001
        i0 = at.astype(np.int64)
        f = (at - i0).astype(np.float32)
        chan[c] = ((1 - f) * chan[c][i0] + f * chan[c][i0 + 1]).astype(np.complex64)
    pdus, summary, mf, lvl = oracle_demod(oracle, chan[0], FREQS[0])
    assert sent_and_decoded(pdus, [b]), "the oracle still decodes the resampled burst"
    m = model_on(mf, lvl, 5400.0, 0.0, len(mf) / 5400.0)
    hist = {k: m.outputs.count(k) for k in sorted(set(m.outputs))}
    print("float64 model over the resampled stream: input samples by outputs", hist)
    assert hist.get(0, 0) > 0 and hist.get(1, 0) > 0
    triples = np.array(m.outputs[:len(m.outputs) // 3 * 3]).reshape(-1, 3)
    assert len({tuple(r) for r in triples}) > 1, "the 1, 1, 0 pattern slips: the loop runs off its nominal rate"
    # the same stream through a timing loop that starts from START_RATE: input samples with 0, 1 and 2 outputs all occur
    m = model_on(mf, lvl, 5400.0, 0.0, len(mf) / 5400.0, StartRateModel)
    hist = {k: m.outputs.count(k) for k in sorted(set(m.outputs))}
    print("float64 model from a start rate of %s: input samples by outputs" % START_RATE, hist)
    assert hist.get(0, 0) > 0 and hist.get(1, 0) > 0 and sum(v for k, v in hist.items() if k >= 2) > 0, "0, 1 and >= 2 outputs per input sample"
    return chan, sorted(PDU_KEY(p) for p in pdus)


@pytest.fixture(scope="module")
def timeout_stream(oracle):
    """Noise only, a little longer than 13 single-slot frames."""
    P = M.Protocol()
    dur = P.timeout / 1800.0 + 0.6
    rng = np.random.default_rng(17)
    n = int(dur * FS)
    x = (0.004 * (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32))).astype(np.complex64)
    chan = channelize(oracle, x)
    want = []
    for c in range(2):
        pdus, summary, mf, lvl = oracle_demod(oracle, chan[c], FREQS[c])
        assert pdus == [] and summary["a2_found"] == 0
        m = model_on(mf, lvl, 5400.0, 0.0, len(mf) / 5400.0)
        symbols = len(m.sym_state)
        print("channel %d: %d symbols, the model's counter ends at %d (timeout at %d)" % (c, symbols, m.symbol_cnt, P.timeout))
        # without a frame nothing else starts the counter again (it strikes late where the framer is looking for A2 at that moment)
        assert m.cnt["frames"] == 0 and symbols > P.timeout and m.symbol_cnt <= symbols - P.timeout, "the no-frame timeout strikes"
    return chan, want


def words(v):
    return np.ascontiguousarray(v).view(np.uint32)


def run(gpu, lib, x, cut):
    """cut(launch index, cutter) -> input samples of the next launch (both channels alike).  Returns per launch and channel the taps as
    32-bit words, all PDU fields, the channel statistics after the last launch, and the outputs per launch."""
    fe = gpu.Frontend(FS, CF, FREQS, lib=lib)
    g = fe.geometry
    cutter = Cutter(float(g.resamp_rate))
    taps, pdus, outs, at, i = [], [], [], 0, 0
    n = min(len(x[0]), len(x[1]))
    while at < n:
        n_in = min(cut(i, cutter), n - at, g.max_outputs_per_block)
        fe.push_baseband([x[0][at:at + n_in], x[1][at:at + n_in]])
        at += n_in
        i += 1
        outs.append(cutter.take(n_in))
        taps.append([[words(fe.read_tap(k, c)) for k in TAPS] for c in range(2)])
        assert len(taps[-1][0][0]) == 2 * outs[-1]
        for p in fe.poll_pdus():
            pdus.append({k: (int(words(np.float32(v))[0]) if isinstance(v, float) else v) for k, v in p.items()})
    stats = [{k: (int(words(np.float32(v))[0]) if isinstance(v, float) else v) for k, v in s.items()} for s in fe.all_channel_stats()]
    fe.close()
    return taps, pdus, stats, outs


def same(a, b):
    assert a[3] == b[3]
    for i, (la, lb) in enumerate(zip(a[0], b[0])):
        for c in range(2):
            for k, ta, tb in zip(TAPS, la[c], lb[c]):
                assert np.array_equal(ta, tb), "launch %d channel %d tap %d differs" % (i, c, k)
    assert a[1] == b[1], "PDUs differ"
    assert a[2] == b[2], "channel statistics differ"


def check(gpu, strict, x, want, cut):
    got = run(gpu, None, x, cut)
    same(got, run(gpu, strict, x, cut))
    assert sorted(PDU_KEY(p) for p in got[1]) == want, "PDUs differ from the oracle's"
    assert got[2][1]["a2_found"] == 0 and got[2][1]["frames"] == 0, "the noise channel never gets past the preamble search"
    return got


@pytest.mark.parametrize("first", range(1, CHUNK + 1))
def test_every_event_at_every_position_of_a_chunk(gpu, strict, event_stream, first):
    """A first launch of `first` outputs, then launches of 512: the detections, the symbols around them, the reset after the failed search,
    the run-away's single step and the restarts of the search behind each, at position (g - first) mod 32 of a chunk."""
    x, want = event_stream
    got = check(gpu, strict, x, want, lambda i, c: c.inputs_for(first if i == 0 else 512))
    assert got[3][0] == first and set(got[3][1:-1]) == {512}
    st = got[2][0]
    assert st["frames"] == st["m1_found"] == 3 and st["a1_found"] > st["a2_found"] >= 3, "a preamble search failed and reset the timing loop"


@pytest.mark.parametrize("first", [1, 2, 3, 16, 31, 32])
def test_timing_loop_off_its_rate(gpu, strict, off_rate_stream, first):
    x, want = off_rate_stream
    got = check(gpu, strict, x, want, lambda i, c: c.inputs_for(first if i == 0 else 512))
    assert got[2][0]["frames"] == 1


@pytest.mark.parametrize("first", [1, 2, 3, 16, 31, 32])
def test_two_outputs_from_one_input_sample(gpu, start_rate_pair, off_rate_stream, first):
    """The timing-recovery wave's general loop behind its straight-line first output: the builds whose timing loop starts from about 1."""
    x, _ = off_rate_stream
    cut = lambda i, c: c.inputs_for(first if i == 0 else 512)
    got = run(gpu, start_rate_pair[0], x, cut)
    same(got, run(gpu, start_rate_pair[1], x, cut))
    assert got[3][0] == first and set(got[3][1:-1]) == {512}
    # on the device: more timing-recovery outputs than input samples means some sample gave two (printed, the CPU model is what asserts)
    outputs = sum(len(launch[0][TAPS.index(F.TAP_SYMBOLS)]) for launch in got[0])      # 2 words per symbol, 2 outputs per symbol
    print("channel 0: %d input samples, %d timing-recovery outputs" % (sum(got[3]), outputs))


def test_no_frame_timeout(gpu, strict, timeout_stream):
    x, want = timeout_stream
    got = check(gpu, strict, x, want, lambda i, c: c.inputs_for(7 if i == 0 else 512))
    for c in range(2):
        assert got[2][c]["symbol_cnt"] < 1800, "the symbol counter started again at the timeout"
