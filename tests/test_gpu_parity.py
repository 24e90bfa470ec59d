"""GPU parity tests (run with -m gpu on an MI355X): every call goes through the C ABI of libhfdl_gpu.so and is
checked against the plain-C oracle on the same seeded input."""
import numpy as np
import pytest

import hfdl_synth as synth
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4      # float DSP stages: error RMS / signal RMS


def rel_rms(a, b):
    a = np.asarray(a, np.complex128)
    b = np.asarray(b, np.complex128)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2) / max(np.mean(np.abs(b) ** 2), 1e-300)))


def test_fft_forward_full_size_8mi(gpu):
    """The 2^23-point transform of the 40 Msps geometry: float64 reference, Parseval and a tone landing on its bin."""
    n = 1 << 23
    rng = np.random.default_rng(23)
    x = (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)).astype(np.complex64)
    got = gpu.fft_forward(x, shifted=True)
    want = np.fft.fftshift(np.fft.fft(x.astype(np.complex128)))
    assert rel_rms(got, want) < 3e-6
    assert worst_over_rms(got, want) <= 10 * 3e-6
    assert abs(np.sum(np.abs(got.astype(np.complex128)) ** 2) / (n * np.sum(np.abs(x.astype(np.complex128)) ** 2)) - 1) < 1e-5
    k = 5_000_017
    tone = np.exp(2j * np.pi * ((k * np.arange(n, dtype=np.int64)) % n) / n).astype(np.complex64)
    spec = gpu.fft_forward(tone, shifted=False)
    assert int(np.argmax(np.abs(spec))) == k and abs(abs(spec[k]) / n - 1) < 1e-4


def worst_over_rms(got, want):
    """Worst element error / RMS of the reference.  The gate that goes with an RMS gate G is 10 G: rounding error spread over the
    outputs is near-Gaussian with sigma <= G rms(want); its maximum over n <= 2^24 elements is about sqrt(2 ln n) = 5.8 sigma, 10 leaves
    margin, and one mis-twiddled or misplaced element on Gaussian input errs by about 1 rms(want).  (A single-precision transform
    known to be good stays inside it: tests/test_channelizer_f64_cpu.py::test_oracle_fft_worst_element.)"""
    want = np.asarray(want, np.complex128)
    return float(np.abs(np.asarray(got, np.complex128) - want).max() / np.sqrt(np.mean(np.abs(want) ** 2)))


def fft_rms_gate(n):
    return 3e-6 if n >= 1 << 23 else 2e-6          # the two gates this file has always had: 2^23 and above, and below


@pytest.mark.parametrize("n", [1 << logn for logn in range(9, 24)])
@pytest.mark.parametrize("shifted", [False, True])
def test_fft_forward_vs_float64(gpu, n, shifted):
    """Every size the entry point takes below 2^24 (pass radices (l1, l2, l3) = ((logn + 2) / 3, (logn - l1 + 1) / 2, rest): every
    radix-4 / radix-2 mix of the LDS passes, 2^21 = (7, 7, 7)), RMS and worst element."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    got = gpu.fft_forward(x, shifted=shifted)
    want = np.fft.fft(x.astype(np.complex128))
    if shifted:
        want = np.fft.fftshift(want)
    e, w = rel_rms(got, want), worst_over_rms(got, want)
    print("n 2^%d: rel rms %.3g worst/rms %.3g" % (n.bit_length() - 1, e, w))
    assert e < fft_rms_gate(n)
    assert w <= 10 * fft_rms_gate(n)


@pytest.mark.parametrize("n", [1 << 24])
def test_fft_forward_vs_float64_largest(gpu, n):
    """2^24 = (8, 8, 8): the only size that runs the radix-16 third pass -- the plan of a receiver above 65.536 Msps.  Once, shifted."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)).astype(np.complex64)
    got = gpu.fft_forward(x, shifted=True)
    want = np.fft.fftshift(np.fft.fft(x.astype(np.complex128)))
    e, w = rel_rms(got, want), worst_over_rms(got, want)
    print("n 2^24: rel rms %.3g worst/rms %.3g" % (e, w))
    assert e < fft_rms_gate(n)
    assert w <= 10 * fft_rms_gate(n)


@pytest.mark.parametrize("n,k", [(1 << 21, 0b101010101010101010101), (1 << 24, 0xAAAAAB)])
def test_fft_forward_impulse_and_tone_large(gpu, n, k):
    """What test_fft_forward_impulse_and_tone does at 4096, at (7, 7, 7) and (8, 8, 8): an impulse at an odd index (every output has
    modulus 1 and a known phase: a dropped or duplicated element cannot hide in an average) and a tone on a bin whose index has bits
    set in all three radix fields."""
    idx = 12345
    x = np.zeros(n, np.complex64)
    x[idx] = 1
    got = gpu.fft_forward(x).astype(np.complex128)
    want = np.exp(-2j * np.pi * ((idx * np.arange(n, dtype=np.int64)) % n) / n)
    assert np.abs(np.abs(got) - 1).max() < 1e-5
    assert np.abs(got - want).max() < 1e-5
    del got, want
    tone = np.exp(2j * np.pi * ((k * np.arange(n, dtype=np.int64)) % n) / n).astype(np.complex64)
    spec = gpu.fft_forward(tone, shifted=False)
    assert int(np.argmax(np.abs(spec))) == k and abs(spec[k] / n - 1) < 1e-4
    want = np.zeros(n, np.complex128)
    want[k] = n
    assert rel_rms(spec, want) < fft_rms_gate(n)


@pytest.mark.parametrize("fmt", ["CS16", "CU8"])
@pytest.mark.parametrize("fs,logn", [(48_000, 13), (250_000, 15), (2_400_000, 19), (20_000_000, 22)])
def test_raw_format_spectrum_vs_float64(gpu, fmt, fs, logn):
    """The first FFT pass converts cs16 / cu8 samples as it loads them, one instantiation per format and first-pass radix: l1 = 7
    (N = 2^19) and l1 = 8 (N = 2^22) of the register-resident passes, and below N = 2^18 the LDS passes' fft_pass1<format> (N = 2^13
    at 48 ksps, 2^15 at 250 ksps).  The spectrum of the second block (its history came in through the same path) against numpy
    on the host-side conversion of the same octets, full-scale codes included, RMS and worst element."""
    cf = 30_000_000
    fe = gpu.Frontend(fs, cf, [cf + 100_000, cf - 200_000] if logn >= 18 else [cf + fs // 24, cf - fs // 12])
    g = fe.geometry
    assert g.fft_size == 1 << logn
    if logn >= 18:
        assert (logn + 2) // 3 == (7 if logn == 19 else 8)
    n = fe.input_size
    rng = np.random.default_rng(logn)
    if fmt == "CS16":
        raw = np.clip(np.round(rng.standard_normal(4 * n) * 9000), -32768, 32767).astype(np.int16)
        raw[5:4 * n:4099] = -32768; raw[6:4 * n:4099] = 32767; raw[7:4 * n:4099] = 0
        conv = (raw.astype(np.float64) / float(np.float32(32767.5)))
        code = F.SFMT_CS16
    else:
        # centred on code 63.5, the zero of the conversion: the worst-element gate presumes error spread over the outputs, not a DC bin
        # of half the full scale times N
        raw = np.clip(np.round(rng.standard_normal(4 * n) * 25 + 63.5), 0, 255).astype(np.uint8)
        raw[5:4 * n:4099] = 0; raw[6:4 * n:4099] = 255
        conv = (raw.astype(np.float64) - 63.5) / 127.0
        code = F.SFMT_CU8
    conv = conv.astype(np.float32).astype(np.float64).view(np.complex128)          # the converted sample as an fp32 value
    for b in range(2):
        fe.push_block_raw(raw[2 * b * n:2 * (b + 1) * n], code)
    fe.sync()
    got = fe.read_tap(F.TAP_SPECTRUM)
    fe.close()
    want = np.fft.fftshift(np.fft.fft(conv[2 * n - g.fft_size:]))
    e, w = rel_rms(got, want), worst_over_rms(got, want)
    print("%s N 2^%d: rel rms %.3g worst/rms %.3g" % (fmt, logn, e, w))
    assert e < 5e-6               # the gate of the spectrum tap in this file
    assert w <= 10 * 5e-6


def test_fft_forward_impulse_and_tone(gpu):
    n = 4096
    x = np.zeros(n, np.complex64)
    x[3] = 1
    got = gpu.fft_forward(x)
    want = np.exp(-2j * np.pi * 3 * np.arange(n) / n)
    assert np.abs(got - want).max() < 1e-5
    tone = np.exp(2j * np.pi * 37 * np.arange(n) / n).astype(np.complex64)
    got = gpu.fft_forward(tone, shifted=True)
    assert np.argmax(np.abs(got)) == 37 + n // 2
    assert abs(got[37 + n // 2] - n) < 1e-2 * n


@pytest.mark.parametrize("fs,nch", [(250000, 3), (1000000, 4)])
def test_channelizer_matches_oracle(gpu, oracle, fs, nch):
    cf = 10_000_000
    rng = np.random.default_rng(fs)
    freqs = sorted(int(cf + f) for f in rng.integers(-int(0.4 * fs), int(0.4 * fs), nch))
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    g = fe.geometry
    od = ora.ddc
    for name in ("fft_size", "fft_inv_size", "input_size", "post_input_size", "scrap", "taps_length"):
        assert getattr(g, name) == getattr(od, name), name
    # filter taps in the frequency domain
    for c in range(nch):
        och = oracle.Channel(fs, cf, freqs[c])
        assert rel_rms(fe.read_tap(F.TAP_FILTER, c), och.taps_fft()) < 1e-5
    n = g.input_size
    t = np.arange(4 * n)
    x = np.zeros(4 * n, np.complex128)
    for f in freqs:       # a tone 300 Hz above each carrier plus wideband noise
        x += 0.1 * np.exp(2j * np.pi * (f + 1440 + 300 - cf) / fs * t)
    x += 0.05 * (rng.standard_normal(4 * n) + 1j * rng.standard_normal(4 * n))
    x = x.astype(np.complex64)
    for b in range(4):
        blk = x[b * n:(b + 1) * n]
        fe.channelize_block(blk)
        ora.push_block(blk)
        assert rel_rms(fe.read_tap(F.TAP_SPECTRUM), ora.spectrum()) < 5e-6
        for c in range(nch):
            got = fe.read_tap(F.TAP_CHAN_OUT, c)
            want = ora.channel_view(c)["chan_out"]
            assert len(got) == len(want) == g.outputs_per_block
            assert rel_rms(got, want) < RMS_TOL, (b, c)
    fe.close()


def test_viterbi_bit_exact(gpu, oracle):
    rng = np.random.default_rng(3)
    for mode in range(8):
        nbits = synth.mode_sizes(mode)["nbits"]
        bits = rng.integers(0, 2, (3, nbits)).astype(np.uint8)
        bits[:, -6:] = 0
        soft = []
        for i in range(3):
            coded = synth.conv_encode(bits[i]).astype(float) * 255
            soft.append(np.clip(coded + rng.normal(0, [0, 50, 110][i], len(coded)), 0, 255).astype(np.uint8))
        soft.append(rng.integers(0, 256, 2 * nbits).astype(np.uint8))       # garbage in: still must match bit for bit
        soft = np.stack(soft)
        got = gpu.viterbi27(soft, nbits)
        for i in range(len(soft)):
            assert bytes(got[i]) == bytes(oracle.viterbi27(soft[i], nbits)), (mode, i)


def test_burst_decode_bit_exact(gpu, oracle):
    rng = np.random.default_rng(4)
    syms, modes, masks, want = [], [], [], []
    for mode in list(range(8)) * 2:
        pdu = synth.make_pdu(rng, mode)
        s = synth.encode_data_symbols(pdu, mode).astype(np.complex64)
        mask = int(rng.integers(0, 2))
        s = s * (1 - 2 * mask)
        s = s * np.exp(1j * rng.normal(0, 0.08, len(s))) + 0.12 * (rng.standard_normal(len(s)) + 1j * rng.standard_normal(len(s)))
        s = s.astype(np.complex64)
        syms.append(s); modes.append(mode); masks.append(mask)
        want.append(bytes(oracle.decode_user_data(mode, s, mask)))
        assert want[-1][:len(pdu)] == pdu
    got = gpu.burst_decode(syms, modes, masks)
    assert got == want


def _run_both(gpu, oracle, fs, cf, freqs, x, check_stages=False):
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n = fe.input_size
    worst = dict(resampled=0.0, mf_out=0.0, symbols=[])
    for b in range(len(x) // n):
        blk = x[b * n:(b + 1) * n]
        fe.push_block(blk)
        ora.push_block(blk)
        if check_stages:
            for c in range(len(freqs)):
                v = ora.channel_view(c)
                for name, tap in (("resampled", F.TAP_RESAMPLED), ("mf_out", F.TAP_MF_OUT), ("symbols", F.TAP_SYMBOLS)):
                    got = fe.read_tap(tap, c)
                    assert len(got) == len(v[name]), (name, b, c)
                    if len(got) and name == "symbols":
                        worst[name].append(rel_rms(got, v[name]))
                    elif len(got):
                        worst[name] = max(worst[name], rel_rms(got, v[name]))
    pdus = fe.poll_pdus()
    # hot-path counters and the noise-floor gauge (StatsD analogue) must agree with the oracle's, channel by channel
    for c in range(len(freqs)):
        st, oc = fe.channel_stats(c), ora.channel_counters(c)
        assert (st["a2_found"], st["m1_found"], st["m1_not_found"], st["frames"], st["framer_state"]) == \
            (oc["a2_found"], oc["m1_found"], oc["m1_not_found"], oc["frames"], oc["framer_state"]), c
        assert abs(st["noise_floor_db"] - 20 * np.log10(oc["noise_floor"])) < 0.2
        assert st["freq"] == freqs[c]
    fe.close()
    for p in pdus:                                          # the on-device LPDU walk of every PDU = the oracle's over the same octets
        assert p["lpdus"] == oracle.lpdu_walk(p["octets"]), (p["freq"], p["sample_index"])
    return pdus, ora.pdus, worst


def test_end_to_end_small_matches_oracle(gpu, oracle):
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 10_037_000, 10_081_500]
    dur = 9.0
    bursts = synth.plan_traffic(freqs, dur, seed=3, dense=True)
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=1)
    got, want, worst = _run_both(gpu, oracle, fs, cf, freqs, x, check_stages=True)
    assert worst["resampled"] < RMS_TOL and worst["mf_out"] < RMS_TOL, worst
    # Equalised symbols come out of three nested feedback loops; on noise-only stretches the loops wander and a 1-ulp difference at
    # their INPUT grows: the strict build, whose demodulator arithmetic is the oracle's to the bit (0 of 80519 symbols differ when both
    # are fed the same channelizer output), shows symbol differences of up to 0.07 on such stretches once the device's own channelizer
    # (another FFT factorisation, ~1e-6 relative) is in front of it (profiles/r04/strict_study.md).  So a worst-block bound below
    # that would gate the channelizer's last bits, not the demodulator: the typical block is gated tightly, the worst one loosely, the
    # decoded octets below exactly -- and the demodulator alone in tests/test_gpu_strict.py and the oracle-fed stage test below.
    assert np.median(worst["symbols"]) < 2e-3 and max(worst["symbols"]) < 0.1, (np.median(worst["symbols"]), max(worst["symbols"]))
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert len(got) == 8
    for p in got:
        assert any(p["octets"][:len(b["octets"])] == b["octets"] for b in bursts if b["freq"] == p["freq"]), p["freq"]
    for a, b in zip(sorted(got, key=key), sorted(want, key=key)):
        assert abs(a["freq_err_hz"] - b["freq_err_hz"]) < 0.05
        assert abs(a["rssi_db"] - b["rssi_db"]) < 0.05 and abs(a["noise_floor_db"] - b["noise_floor_db"]) < 0.2
        assert a["slot"] == b["slot"] and a["bit_rate"] == b["bit_rate"]


def test_level_extremes_carrier_offsets_and_adjacent_channels(gpu, oracle):
    """What real bands do to a receiver, GPU against oracle: channels 3 kHz apart (the HFDL raster) transmitting at once with 26 dB
    between them; +-40 Hz of carrier offset (twice what the other tests use); a burst 7 dB above the in-channel noise beside a
    near-full-scale one; a near-full-scale onset out of silence (the AGC swings through ~50 dB inside the prekey: the reference
    chain, as restated, finds A1 and loses A2 -- and so must the device).  The gate is identity: same PDUs, same per-channel event
    counters (checked by _run_both), whatever each burst's fate; nine of the eleven bursts are known to decode."""
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 9_933_000, 10_037_000, 10_040_000, 10_081_000, 10_084_000]
    rng = np.random.default_rng(404)
    bursts = []

    def add(f, mode, t0, amp, cfo):
        bursts.append(dict(freq=f, mode=mode, octets=synth.make_pdu(rng, mode), t0=t0, amp=amp, cfo=cfo))

    add(freqs[0], 3, 0.40, 0.30, +12.0); add(freqs[1], 1, 0.55, 0.015, -8.0)       # 26 dB between neighbours, overlapping in time
    add(freqs[2], 2, 0.30, 0.05, +40.0); add(freqs[3], 0, 0.45, 0.05, -40.0)        # equal levels, opposite carrier offsets
    add(freqs[4], 0, 0.35, 0.006, +3.0); add(freqs[5], 3, 0.50, 0.9, -20.0)         # +7 dB in-channel SNR beside a near-full-scale onset
    add(freqs[0], 5, 3.2, 0.015, -30.0); add(freqs[1], 7, 3.3, 0.30, +30.0)         # levels swapped, double-slot modes
    add(freqs[2], 4, 3.1, 0.006, 40.0); add(freqs[3], 6, 3.25, 0.3, -40.0)
    add(freqs[5], 2, 3.4, 0.2, 0.0)
    dur = 8.4
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=404)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    decoded = {i for p in got for i, b in enumerate(bursts) if b["freq"] == p["freq"] and p["octets"][:len(b["octets"])] == b["octets"]}
    assert decoded == {0, 1, 2, 3, 4, 7, 8, 9, 10}, decoded
    for a, b in zip(sorted(got, key=key), sorted(want, key=key)):
        assert abs(a["freq_err_hz"] - b["freq_err_hz"]) < 0.05 and abs(a["rssi_db"] - b["rssi_db"]) < 0.05


@pytest.mark.parametrize("delay_ms,echo_db,fade_hz,depth", [(0.5, -6, 0.7, 0.4), (2.0, -3, 0.3, 0.3)])
def test_two_path_channel_with_fading(gpu, oracle, delay_ms, echo_db, fade_hz, depth):
    """What the T/2-spaced LMS equaliser is there for (src/hfdl.c:717-733): a second path 0.5 / 2 ms late, 6 / 3 dB down, under a slow
    fade of +-30..40 %.  The equaliser's training steps (two IEEE divisions and a weight update per known symbol) decide every frame here;
    every burst decodes, and the device's PDUs, event counters and carrier / level readings are the oracle's."""
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 9_978_000, 10_037_000, 10_081_500]
    dur = 9.0
    bursts = synth.plan_traffic(freqs, dur, seed=77, dense=True, amp=(0.02, 0.05), cfo_hz=15.0)
    x0 = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.0, seed=77)
    d = int(round(delay_ms * 1e-3 * fs))
    echo = np.zeros_like(x0)
    echo[d:] = x0[:-d]
    t = np.arange(len(x0)) / fs
    fade = 1.0 + depth * np.sin(2 * np.pi * fade_hz * t + 0.7)
    rng = np.random.default_rng(77)
    x = ((x0 + 10 ** (echo_db / 20) * np.exp(1j * 1.1) * echo) * fade
         + rng.normal(0, 0.01, len(x0)) + 1j * rng.normal(0, 0.01, len(x0))).astype(np.complex64)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert len(got) == len(bursts) == 7
    for p in got:
        assert any(p["octets"][:len(b["octets"])] == b["octets"] for b in bursts if b["freq"] == p["freq"]), p["freq"]
    for a, b in zip(sorted(got, key=key), sorted(want, key=key)):
        assert abs(a["freq_err_hz"] - b["freq_err_hz"]) < 0.05 and abs(a["rssi_db"] - b["rssi_db"]) < 0.05


def test_carriers_and_impulses_in_the_band(gpu, oracle):
    """Interference an HF band is full of: a steady carrier 400 Hz beside one channel's own (a few dB under its bursts), a carrier
    sweeping through another channel during its bursts, and 900 full-scale impulses over the nine seconds.  All seven bursts still decode;
    PDUs, counters and readings are the oracle's."""
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 9_978_000, 10_037_000, 10_081_500]
    dur = 9.0
    bursts = synth.plan_traffic(freqs, dur, seed=55, dense=True, amp=(0.02, 0.05), cfo_hz=15.0)
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=55)
    t = np.arange(len(x)) / fs
    rng = np.random.default_rng(55)
    x = x + 0.012 * np.exp(2j * np.pi * (freqs[0] + 1440 + 400 - cf) * t)
    sweep_hz = (freqs[2] + 1440 - cf) - 3000 + 6000 * (t / dur)
    x = x + 0.01 * np.exp(2j * np.pi * np.cumsum(sweep_hz) / fs)
    at = rng.integers(0, len(x), 900)
    x[at] += rng.normal(0, 1.0, len(at)) + 1j * rng.normal(0, 1.0, len(at))
    x = x.astype(np.complex64)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert len(got) == len(bursts) == 7
    for p in got:
        assert any(p["octets"][:len(b["octets"])] == b["octets"] for b in bursts if b["freq"] == p["freq"]), p["freq"]


def test_end_to_end_lpdu_lists(gpu, oracle):
    """MPDUs carrying real LPDU lists (down- and uplink; some LPDUs with a spoiled FCS) through the whole path: every PDU
    record's lpdus_* counts -- parse_lpdu_list + lpdu_parse's checks done by the burst decoder on the device -- equal both
    the oracle's walk of the decoded octets and what was put on the air."""
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 10_037_000, 10_081_500]
    dur = 9.0
    bursts = synth.plan_traffic(freqs, dur, seed=31, dense=True)
    rng = np.random.default_rng(31)
    sent = {}
    for i, b in enumerate(bursts):
        n = synth.mode_sizes(b["mode"])["max_payload"]
        if n < 120:
            continue
        spoil = (0,) if i % 3 == 0 else ()
        b["octets"], cnt = synth.make_mpdu_with_lpdus(rng, n, uplink=bool(i & 1), spoil=spoil)
        sent[b["octets"]] = (cnt, cnt - len(spoil), len(spoil), 0, 0)
    assert len(sent) >= 4
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=31)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    seen = 0
    for p in got:
        for octets, counts in sent.items():                 # the decoder hands over whole interleaver blocks: payload + padding
            if p["octets"][:len(octets)] == octets:
                assert p["lpdus"] == counts and p["fcs_status"] == 0
                seen += 1
    assert seen == len(sent)
    assert any(p["lpdus"][2] for p in got) and any(p["pdu_kind"] == 2 and p["lpdus"][1] for p in got)


def test_end_to_end_cfg2_shape(gpu, oracle):
    """BASELINE.json configs[1] geometry at reduced duration: 8 Msps, 32 channels on a 200 kHz grid."""
    fs, cf = 8_000_000, 10_000_000
    freqs = [int(cf + (i - 16) * 200_000 + 37_000) for i in range(32)]
    dur = 3.3
    bursts = synth.plan_traffic(freqs, dur, seed=2, modes=[0, 1, 2, 3], dense=False, amp=(0.008, 0.03))   # 19..30 dB in-channel SNR
    # pad the stream so the last burst has left the channelizer / demodulator pipeline before the input ends
    x = synth.synth_wideband(fs, cf, int((dur + 0.35) * fs), bursts, noise_sigma=0.02, seed=2)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert len(got) == len(bursts) == 32
    by_freq = {b["freq"]: b["octets"] for b in bursts}
    for p in got:
        assert p["octets"][:len(by_freq[p["freq"]])] == by_freq[p["freq"]]


def test_cfg2_thirty_seconds_through_the_c_host_program(gpu, oracle, tmp_path):
    """BASELINE.json configs[1] at the duration SURVEY.md 8(d) words it with: 8 Msps, 32 channels on a 200 kHz grid, THIRTY seconds of
    burst-dense traffic in all eight modes, as a cs16 file through hfdl_replay (the C host path: file input -> page-locked ring -> GPU
    front end -> pdu_decoder_queue_push), against the oracle on the same converted samples, every channel.  (bench.WORKLOADS["cfg2"]
    keeps 26 blocks = 3 s resident in HBM and replays them: the bench measures rate, this test the thirty seconds.)"""
    import os
    fs, cf = 8_000_000, 10_000_000
    freqs = [int(cf + (i - 16) * 200_000 + 37_000) for i in range(32)]
    dur = 30.0
    bursts = synth.plan_traffic(freqs, dur - 0.4, seed=21, dense=True, amp=(0.008, 0.03))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.02, seed=21)
    raw = np.clip(np.round(x.view(np.float32) * 20000), -32768, 32767).astype(np.int16)
    del x
    got = _replay(tmp_path, raw, "CS16", fs, cf, freqs)
    x_in = (raw.astype(np.float32) / np.float32(32767.5)).view(np.complex64)       # what convert_cs16 produces
    del raw
    threads = max(1, min(64, os.cpu_count() or 1))
    ora = oracle.Frontend(fs, cf, freqs, nthreads=threads)
    n = ora.ddc.input_size
    for b in range(len(x_in) // n):
        ora.push_block(x_in[b * n:(b + 1) * n], nthreads=threads)
    want = [(p["freq"], p["bit_rate"], p["slot"], p["octets"]) for p in ora.pdus]
    assert sorted(got) == sorted(want)
    # the preamble search loses 1 - 3 % of bursts on both sides alike (oracle/PINNING.md); everything else is there, intact
    assert len(got) >= 0.95 * len(bursts) and len(bursts) >= 200
    sent = {}
    for b in bursts:
        sent.setdefault(b["freq"], []).append(b["octets"])
    assert all(any(o[:len(s)] == s for s in sent[f]) for f, _, _, o in got)


def test_no_device_pointer_confusion(gpu):
    with pytest.raises(F.GpuError):
        gpu.Frontend(250000, 10_000_000, [20_000_000])      # outside +-fs/2
    fe = gpu.Frontend(250000, 10_000_000, [10_010_000])
    with pytest.raises(F.GpuError):
        fe.push_block(np.zeros(100, np.complex64))           # not a whole block
    fe.close()


def _replay(tmp_path, x_raw, fmt, fs, cf, freqs, extra=(), want_stderr=False):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dumphfdl_amd", "hfdl_replay")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "dumphfdl_amd", "host")])
    path = tmp_path / ("iq." + fmt.lower())
    x_raw.tofile(path)
    out = subprocess.run([exe, "--iq-file", str(path), "--sample-rate", str(fs), "--sample-format", fmt, "--centerfreq", str(cf / 1e3)]
                         + list(extra) + ["%.3f" % (f / 1e3) for f in freqs], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    pdus = []
    for line in out.stdout.splitlines():
        if line.startswith("PDU "):
            kv = dict(t.split("=") for t in line.split()[1:-1])
            pdus.append((int(kv["freq"]), int(kv["bit_rate"]), kv["slot"], bytes.fromhex(line.split()[-1])))
    return (pdus, out.stderr) if want_stderr else pdus


@pytest.mark.parametrize("fmt", ["CF32", "CS16"])
def test_host_c_program_end_to_end(gpu, oracle, tmp_path, fmt):
    """The C host path: file input -> block ring -> GPU front-end block -> pdu_decoder_queue_push (printing default)."""
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 10_037_000, 10_081_500]
    bursts = synth.plan_traffic(freqs, 6.0, seed=3, dense=True)
    x = synth.synth_wideband(fs, cf, int(6.0 * fs), bursts, noise_sigma=0.01, seed=1)
    if fmt == "CS16":
        raw = np.clip(np.round(x.view(np.float32) * 20000), -32768, 32767).astype(np.int16)
        x_in = (raw.astype(np.float32) / np.float32(32767.5)).view(np.complex64)       # what convert_cs16 produces
    else:
        raw, x_in = x.view(np.float32), x
    got = _replay(tmp_path, raw, fmt, fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n = ora.ddc.input_size
    for b in range(len(x_in) // n):
        ora.push_block(x_in[b * n:(b + 1) * n])
    want = [(p["freq"], p["bit_rate"], p["slot"], p["octets"]) for p in ora.pdus]
    assert sorted(got) == sorted(want) and len(got) == len(bursts)


def test_burst_dense_all_modes_cfg4_shape(gpu, oracle):
    """BASELINE.json configs[3] in miniature: every channel carries back-to-back bursts cycling all 8 modes
    (300/600/1200/1800 bps, single + double slot).  PDU multiset must equal the oracle's, payloads what was sent."""
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000]
    dur = 31.0
    bursts = synth.plan_traffic(freqs, dur, seed=4, dense=True, gap_s=0.12, amp=(0.03, 0.12))
    assert {b["mode"] for b in bursts} == set(range(8))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=4)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["slot"], p["bit_rate"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert len(got) >= len(bursts) - 1
    for p in got:
        assert any(p["octets"][:len(b["octets"])] == b["octets"] and p["mode"] == b["mode"] for b in bursts if b["freq"] == p["freq"])
        assert len(p["octets"]) == synth.mode_sizes(p["mode"])["octets"]
        # on-device FCS / header triage equals the oracle's and (the generator writes valid FCS) says "good"
        assert (p["fcs_status"], p["pdu_kind"], p["hdr_len"]) == oracle.pdu_triage(p["octets"])
        assert p["fcs_status"] == F.FCS_GOOD


def test_degenerate_inputs(gpu, oracle):
    """All-zero input, a single channel at the band edge, full-scale noise: no PDUs, no NaNs, stages still match the oracle."""
    fs, cf = 250000, 10_000_000
    freqs = [cf + 110_000]                              # 0.44 fs from centre
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n = fe.input_size
    rng = np.random.default_rng(0)
    blocks = [np.zeros(n, np.complex64), np.zeros(n, np.complex64),
              (0.7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64),
              np.zeros(n, np.complex64)]
    for blk in blocks:
        fe.push_block(blk)
        ora.push_block(blk)
        got = fe.read_tap(F.TAP_CHAN_OUT, 0)
        want = ora.channel_view(0)["chan_out"]
        assert np.isfinite(got.view(np.float32)).all()
        assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-12) + 1e-12
        lv, lw = fe.read_tap(F.TAP_AGC_LEVEL, 0), ora.channel_view(0)["agc_level"]
        assert len(lv) == len(lw) and np.isfinite(lv).all()
        assert np.allclose(lv, lw, rtol=2e-3, atol=1e-12)
    assert fe.poll_pdus() == [] and ora.pdus == []
    fe.close()


def test_channels_at_the_very_band_edge(gpu, oracle):
    """Channels 1 Hz inside +-fs/2 (the span check of src/main.c:214-226 admits them), whose carrier 1440 Hz above the channel frequency
    and pass-band wrap around the band edge: fastddc's circular bin shift folds them onto the other end of the spectrum, so the channels
    at -fs/2 + 1 and +fs/2 - 1 hear the same signals (2 Hz apart) and both decode the stronger of two overlapping bursts.  Identity with
    the oracle on PDUs and per-channel counters (checked by _run_both) is the gate."""
    fs, cf = 250000, 10_000_000
    freqs = [cf - 124_999, cf - 124_000, cf + 122_000, cf + 124_999]
    rng = np.random.default_rng(5)
    bursts = [dict(freq=f, mode=i % 4, octets=synth.make_pdu(rng, i % 4), t0=0.4 + 0.05 * i, amp=0.05, cfo=float(rng.uniform(-10, 10)))
              for i, f in enumerate(freqs)]
    x = synth.synth_wideband(fs, cf, int(3.4 * fs), bursts, noise_sigma=0.01, seed=5)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert sorted((p["freq"] - cf, p["mode"]) for p in got) == [(-124_999, 3), (-124_000, 1), (122_000, 2), (124_999, 3)]


def test_six_hundred_channels(gpu, oracle):
    """More channels than any BASELINE.json config has (600; every frequency ten times over, as a receiver list with duplicates
    would): the fold's slice count drops to one, the demodulator and burst-decoder grids and the frame queue grow with the channel
    count.  Twenty bursts, each heard by ten channels: 200 PDUs, the oracle's."""
    fs, cf = 250000, 10_000_000
    base = [int(cf + (i - 30) * 4_000 + 500) for i in range(60)]
    freqs = [f for f in base for _ in range(10)]
    rng = np.random.default_rng(9)
    bursts = [dict(freq=f, mode=i % 4, octets=synth.make_pdu(rng, i % 4), t0=0.3 + 0.01 * i, amp=0.02, cfo=float(rng.uniform(-8, 8)))
              for i, f in enumerate(base) if i % 3 == 0]
    x = synth.synth_wideband(fs, cf, int(3.4 * fs), bursts, noise_sigma=0.004, seed=9)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert len(got) == 10 * len(bursts) == 200


def test_constant_payloads_in_every_mode(gpu, oracle):
    """All-zero, all-one and alternating payloads in each of the eight modes (scrambler, interleaver and Viterbi on their least random
    input; none of these is a valid MPDU / SPDU, so the on-device triage sees bad frame checks throughout): the device's PDUs are the
    oracle's, and 23 of the 24 payloads come back octet for octet (the 24th is lost to the preamble search on both sides)."""
    fs, cf = 1_000_000, 10_000_000
    freqs = [int(cf + (i - 12) * 14_000 + 3_000) for i in range(24)]
    bursts = []
    for i, f in enumerate(freqs):
        mode, pat = i % 8, (0x00, 0xFF, 0x55)[i // 8]
        bursts.append(dict(freq=f, mode=mode, octets=bytes([pat]) * synth.mode_sizes(mode)["max_payload"], t0=0.3 + 0.02 * i, amp=0.03,
                           cfo=float((i * 7) % 31 - 15)))
    dur = 0.3 + 0.02 * 24 + synth.burst_symbols_len(7) / 1800 + 0.4
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.02, seed=21)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    good = sum(1 for p in got if any(b["freq"] == p["freq"] and b["mode"] == p["mode"] and p["octets"][:len(b["octets"])] == b["octets"] for b in bursts))
    assert good == len(got) == 23
    for p in got:
        assert (p["fcs_status"], p["pdu_kind"], p["hdr_len"]) == oracle.pdu_triage(p["octets"])


def test_many_frames_in_one_block(gpu, oracle):
    """64 channels whose bursts end inside the same block: the burst-decoder queue takes them all at once."""
    fs, cf = 1_000_000, 10_000_000
    freqs = [int(cf + (i - 32) * 14_000 + 3_000) for i in range(64)]
    rng = np.random.default_rng(12)
    bursts = [dict(freq=f, mode=int(i % 4), octets=synth.make_pdu(rng, int(i % 4)), t0=0.3, amp=0.02, cfo=float(rng.uniform(-8, 8)))
              for i, f in enumerate(freqs)]
    x = synth.synth_wideband(fs, cf, int(3.1 * fs), bursts, noise_sigma=0.004, seed=6)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    assert len(got) >= 60


@pytest.mark.parametrize("fmt", ["CS16", "CU8"])
def test_raw_ingest_converted_on_device(gpu, oracle, fmt):
    """cs16 / cu8 samples converted inside the forward FFT's first load; must equal feeding the
    oracle the reference's host-side conversion (src/input-helpers.c:33-78) of the same octets."""
    fs, cf = 250000, 10_000_000
    freqs = [9_958_000, 10_061_000]
    rng = np.random.default_rng(31)
    bursts = [dict(freq=freqs[0], mode=2, octets=synth.make_pdu(rng, 2), t0=0.3, amp=0.25, cfo=5.0),
              dict(freq=freqs[1], mode=1, octets=synth.make_pdu(rng, 1), t0=0.4, amp=0.3, cfo=-7.0)]
    x = synth.synth_wideband(fs, cf, int(3.3 * fs), bursts, noise_sigma=0.02, seed=3)
    f = x.view(np.float32)
    if fmt == "CS16":
        raw = np.clip(np.round(f * 20000), -32768, 32767).astype(np.int16)
        conv = (raw.astype(np.float32) / np.float32(32767.5)).view(np.complex64)
        code = F.SFMT_CS16
    else:
        raw = np.clip(np.round(f * 100 + 127.5), 0, 255).astype(np.uint8)
        conv = ((raw.astype(np.float32) - np.float32(63.5)) / np.float32(127.0)).view(np.complex64)
        code = F.SFMT_CU8
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n = fe.input_size
    for b in range(len(conv) // n):
        fe.push_block_raw(raw[2 * b * n:2 * (b + 1) * n], code)
        ora.push_block(conv[b * n:(b + 1) * n])
        assert rel_rms(fe.read_tap(F.TAP_SPECTRUM), ora.spectrum()) < 5e-6
    got = sorted((p["freq"], p["octets"]) for p in fe.poll_pdus())
    assert got == sorted((p["freq"], p["octets"]) for p in ora.pdus) and len(got) == 2
    fe.close()


def test_full_size_cfg3_geometry(gpu, oracle):
    """BASELINE.json configs[2] geometry (40 Msps, N = 2^23, M = 4096) with all 256 channels resident.
    Size-independent properties over every channel: encode -> channel -> decode round trip (payload + FCS) and
    linearity of the channelizer; plus oracle parity (channelizer RMS, PDUs, preamble counters) on a 16-channel subset that holds
    every channel whose burst the reference's preamble search loses."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    w = dict(bench.WORKLOADS["cfg3"])
    freqs = bench.channel_plan(w)
    assert len(freqs) == 256
    fe = gpu.Frontend(w["fs"], w["centerfreq"], freqs)
    g = fe.geometry
    assert (g.fft_size, g.fft_inv_size, g.input_size, g.outputs_per_block) == (1 << 23, 4096, 7340032, 1792)
    x, bursts = bench.make_input(w, g.input_size, 0, 1)
    nblk = len(x) // g.input_size
    import json
    row = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg3_oracle_lost_bursts.json")))
    # the oracle runs beside the device on SIXTEEN channels -- the nine whose burst the reference's M1 search loses (the committed table)
    # and seven that decode -- or, on a host large enough, on all 256 (round 5: four channels, none of the nine)
    sub = sorted(set(row["lost_burst_streams"]) | {3, 60, 77, 100, 128, 201, 250})
    assert len(sub) == 16 and len(set(row["lost_burst_streams"])) == 9
    cores = os.cpu_count() or 4
    try:
        ram_gib = os.sysconf("SC_PHYS_PAGES") * os.sysconf("SC_PAGE_SIZE") / 2.0 ** 30
    except (ValueError, OSError):
        ram_gib = 0.0
    if cores >= 32 and ram_gib >= 128:
        # a host with the cores and the memory for it (the GPU boxes: 256 cores, 3 TiB) runs the oracle on ALL 256 channels: 16 GiB of
        # oracle filters, as the reference itself would hold
        sub = list(range(256))
    nthr = max(4, min(128, cores))
    ora = oracle.Frontend(w["fs"], w["centerfreq"], [freqs[c] for c in sub], nthreads=nthr)
    worst = 0.0
    for b in range(nblk):
        blk = x[b * g.input_size:(b + 1) * g.input_size]
        fe.push_block(blk)
        ora.push_block(blk, nthreads=nthr)
        if b in (0, 1, nblk - 1):
            for i, c in enumerate(sub):
                worst = max(worst, rel_rms(fe.read_tap(F.TAP_CHAN_OUT, c), ora.channel_view(i)["chan_out"]))
    assert worst < RMS_TOL, worst
    pdus = fe.poll_pdus()
    sent = {b["freq"]: b for b in bursts}
    # 256 bursts sent; the oracle, run over ALL 256 channels of this very traffic (profiles/variant_study.py, committed table), loses
    # nine of them to the reference's own M1 search (A2_found + M1_not_found): the GPU must lose exactly those nine and no other
    lost = {freqs[i] for i in row["lost_burst_streams"]}
    assert len(lost) == row["m1_not_found"] == 256 - row["pdus"]
    assert {f for f in freqs if not any(p["freq"] == f for p in pdus)} == lost and len(pdus) == row["pdus"] == row["recovered"]
    for p in pdus:
        b = sent[p["freq"]]
        assert p["octets"][:len(b["octets"])] == b["octets"] and p["mode"] == b["mode"] and p["fcs_status"] == F.FCS_GOOD
        assert p["lpdus"] == ((0,) * 5 if b["lpdus"] is None else (b["lpdus"], b["lpdus"], 0, 0, 0))      # the device's LPDU walk = what was sent
    got16 = sorted((p["freq"], p["sample_index"], p["octets"]) for p in pdus if p["channel"] in sub)
    assert got16 == sorted((p["freq"], p["sample_index"], p["octets"]) for p in ora.pdus) and len(got16) == len(sub) - 9      # nine bursts lost by both
    # ... and on the nine the oracle's counters say WHY, the same way the device's do: A2 found, M1 not found
    for i, c in enumerate(sub):
        oc = ora.channel_counters(i)
        st = fe.channel_stats(c)
        assert (st["a2_found"], st["m1_found"], st["m1_not_found"], st["frames"]) == (oc["a2_found"], oc["m1_found"], oc["m1_not_found"], oc["frames"]), (c, st, oc)
        if c in row["lost_burst_streams"]:
            assert st["m1_not_found"] >= 1 and st["frames"] == 0
    fe.close()
    # linearity of the whole channelizer at full size: C(a x + b y) = a C(x) + b C(y), fresh state each time
    rng = np.random.default_rng(9)
    n = g.input_size
    xa = (0.2 * (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32))).astype(np.complex64)
    xb = x[:n]
    outs = []
    for sig in (xa, xb, (np.complex64(0.5) * xa + np.complex64(-1.5) * xb).astype(np.complex64)):
        f2 = gpu.Frontend(w["fs"], w["centerfreq"], freqs[:16])
        f2.channelize_block(sig)
        outs.append(np.stack([f2.read_tap(F.TAP_CHAN_OUT, c) for c in range(16)]))
        f2.close()
    assert rel_rms(outs[2], 0.5 * outs[0] - 1.5 * outs[1]) < 1e-5


def test_marginal_snr_same_pdus_even_when_wrong(gpu, oracle):
    """-6..4 dB in-channel SNR: a third of the dispatched PDUs carry bit errors and some bursts are missed -- the GPU must
    dispatch exactly the PDUs the oracle does (same octets, right or wrong, same detection instant), FCS verdicts included."""
    fs, cf = 1_000_000, 10_000_000
    freqs = [int(cf + (i - 32) * 14_000 + 3_000) for i in range(64)]
    rng = np.random.default_rng(99)
    bursts = []
    for f in freqs:
        t = float(rng.uniform(0.3, 0.9))
        for _ in range(2):
            mode = int(rng.integers(0, 4))
            amp = float(10 ** (rng.uniform(-6, 4) / 20) * 0.0025)        # in-channel noise rms ~ 0.0025
            bursts.append(dict(freq=f, mode=mode, octets=synth.make_pdu(rng, mode), t0=t, amp=amp, cfo=float(rng.uniform(-25, 25))))
            t += synth.burst_symbols_len(mode) / 1800 + 0.4
    dur = max(b["t0"] for b in bursts) + 2.8
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.02, seed=7)
    got, want, _ = _run_both(gpu, oracle, fs, cf, freqs, x)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, want))
    good = [p for p in got if any(p["octets"][:len(b["octets"])] == b["octets"] for b in bursts if b["freq"] == p["freq"])]
    assert 20 < len(good) < len(got) <= len(bursts)          # the regime really is marginal
    for p in got:
        assert (p["fcs_status"], p["pdu_kind"], p["hdr_len"]) == oracle.pdu_triage(p["octets"])
    assert {p["fcs_status"] for p in got} >= {F.FCS_GOOD, F.FCS_BAD}


@pytest.mark.parametrize("fs,offs", [(12_000, [-2_000]), (48_000, [-15_000, 9_000]), (768_000, [-300_000, 5_000, 333_000]),
                                      (2_400_000, [-1_100_000, 1_050_000]), (345_600, [-100_000, 50_000]), (345_599, [-100_000, 50_000])])
def test_other_sample_rates(gpu, oracle, fs, offs):
    """Receiver rates outside BASELINE.json's configs (12 ksps = post_decimation only, Airspy 768 ksps, RTL 2.4 Msps) and the two ends
    of the resampler's range -- 345 600 sps = 5400 x 64: channel rate 5400, resampling rate exactly 1; one sample per second less:
    decimation 32, channel rate 10 799.97, rate 0.500001 (at 0.5 msresamp would grow a half-band stage; the planner cannot reach it):
    geometry, channelizer output and decoded PDUs against the oracle."""
    cf = 10_000_000
    freqs = [cf + o for o in offs]
    rng = np.random.default_rng(fs)
    bursts = [dict(freq=f, mode=int(rng.integers(0, 4)), octets=b"", t0=0.4 + 0.1 * i, amp=0.05, cfo=float(rng.uniform(-10, 10)))
              for i, f in enumerate(freqs)]
    for b in bursts:
        b["octets"] = synth.make_pdu(rng, b["mode"])
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    g, od = fe.geometry, ora.ddc
    for name in ("fft_size", "fft_inv_size", "input_size", "post_input_size", "scrap", "taps_length", "pre_decimation", "post_decimation"):
        assert getattr(g, name) == getattr(od, name), name
    dur = 3.4
    nsamp = (int(dur * fs) // g.input_size + 1) * g.input_size
    dec = g.pre_decimation * g.post_decimation
    x = synth.synth_wideband(fs, cf, nsamp, bursts, noise_sigma=0.01 * np.sqrt(dec / 32.0), seed=3)
    worst = 0.0
    for b in range(nsamp // g.input_size):
        blk = x[b * g.input_size:(b + 1) * g.input_size]
        fe.push_block(blk)
        ora.push_block(blk)
        if b % 7 == 0:
            for c in range(len(freqs)):
                got, want = fe.read_tap(F.TAP_CHAN_OUT, c), ora.channel_view(c)["chan_out"]
                assert len(got) == len(want)
                worst = max(worst, rel_rms(got, want))
    assert worst < RMS_TOL, worst
    got = sorted((p["freq"], p["sample_index"], p["octets"]) for p in fe.poll_pdus())
    assert got == sorted((p["freq"], p["sample_index"], p["octets"]) for p in ora.pdus)
    assert len(got) == len(freqs)
    fe.close()


def test_long_idle_then_burst(gpu, oracle):
    """65 s of noise (twice the 13-frame search timeout that resets the loops, src/hfdl.c:745-752) and then one burst per
    channel.  In noise the timing/carrier loops random-walk, so last-ulp differences between the lane-parallel float
    sums on the device and the serial ones in the oracle decorrelate the two trajectories: the decoded octets, modes and
    event counters must still be identical, the frame position may differ by a fraction of a symbol
    (tolerance: 3 samples at 5400 Hz = one symbol), the noise-floor estimate by 0.5 dB."""
    fs, cf = 250000, 10_000_000
    freqs = [9_924_000, 9_978_000, 10_032_000, 10_086_000]
    dur = 65.0
    rng = np.random.default_rng(65)
    bursts = [dict(freq=f, mode=i, octets=synth.make_pdu(rng, i), t0=dur - 3.0, amp=0.02, cfo=float(rng.uniform(-10, 10)))
              for i, f in enumerate(freqs)]
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs, nthreads=4)
    n = fe.input_size
    total, done, k = int(dur * fs) // n * n, 0, 0
    while done < total:                                  # synthesised in 40-block pieces to bound host memory
        m = min(40 * n, total - done)
        live = [dict(b, t0=b["t0"] - done / fs) for b in bursts if -4 < b["t0"] - done / fs < m / fs + 1]
        x = synth.synth_wideband(fs, cf, m, live, noise_sigma=0.01, seed=650 + k)
        for b in range(m // n):
            fe.push_block(x[b * n:(b + 1) * n])
            ora.push_block(x[b * n:(b + 1) * n], nthreads=4)
        done, k = done + m, k + 1
    got = {p["freq"]: p for p in fe.poll_pdus()}
    want = {p["freq"]: p for p in ora.pdus}
    assert sorted(got) == sorted(want) == sorted(freqs)
    for b in bursts:
        g, w = got[b["freq"]], want[b["freq"]]
        assert g["octets"] == w["octets"] and g["octets"][:len(b["octets"])] == b["octets"]
        assert (g["mode"], g["slot"], g["bit_rate"]) == (w["mode"], w["slot"], w["bit_rate"])
        assert abs(g["sample_index"] - w["sample_index"]) <= 3
        assert abs(g["freq_err_hz"] - w["freq_err_hz"]) < 0.5
    for c in range(len(freqs)):
        sg, so = fe.channel_stats(c), ora.channel_counters(c)
        for key in ("a2_found", "m1_found", "m1_not_found", "frames"):
            if key in sg and key in so:
                assert sg[key] == so[key], key
        assert abs(sg["noise_floor_db"] - 20 * np.log10(so["noise_floor"])) < 0.5
    fe.close()


def test_host_c_program_statsd_counters(gpu, oracle, tmp_path):
    """The C host emits the reference's per-channel StatsD counters (src/hfdl.c:818-840) from device state: a program
    that defines the statsd_* hooks (here hfdl_replay --statsd-print) sees one increment per event, as many as the oracle counts."""
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 10_037_000, 10_081_500]
    bursts = synth.plan_traffic(freqs, 8.0, seed=8, dense=True)
    x = synth.synth_wideband(fs, cf, int(8.0 * fs), bursts, noise_sigma=0.01, seed=8)
    got, err = _replay(tmp_path, x.view(np.float32), "CF32", fs, cf, freqs, extra=["--statsd-print"], want_stderr=True)
    ora = oracle.Frontend(fs, cf, freqs)
    n = ora.ddc.input_size
    for b in range(len(x) // n):
        ora.push_block(x[b * n:(b + 1) * n])
    assert sorted(got) == sorted((p["freq"], p["bit_rate"], p["slot"], p["octets"]) for p in ora.pdus) and len(got) == len(bursts)
    seen = {}
    for line in err.splitlines():
        if line.startswith("STATSD counter "):
            t = line.split()
            seen[int(t[2])] = {k: int(v) for k, v in (kv.split("=") for kv in t[3:])}
    for c, f in enumerate(freqs):
        want = ora.channel_counters(c)
        assert seen[f] == dict(A2_found=want["a2_found"], M1_found=want["m1_found"], M1_not_found=want["m1_not_found"])
    assert sum(v["M1_found"] for v in seen.values()) == len(bursts)


@pytest.mark.parametrize("ring", [0, 3])
def test_collect_without_draining_the_pipeline(gpu, oracle, monkeypatch, ring):
    """hfdl_gpu_frontend_poll_pdus_ready(max_in_flight=1) after every push + one draining poll at the end delivers each
    PDU exactly once; with a 3-entry device ring (HFDL_GPU_PDU_RING) the slots wrap many times without loss -- there with one block
    per fold / demodulator launch, so that what waits in the ring between two collections is a block's PDUs (with 16-block halves
    the three entries would overflow by design: the ring is sized for two halves of traffic, max(4096, 64 per channel) by default)."""
    if ring:
        monkeypatch.setenv("HFDL_GPU_PDU_RING", str(ring))
        monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "1")
        monkeypatch.setenv("HFDL_GPU_DEMOD_BATCH", "1")
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000]
    dur = 14.0
    bursts = synth.plan_traffic(freqs, dur, seed=21, dense=True, gap_s=0.15, amp=(0.03, 0.1))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=21)
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n = fe.input_size
    got, early = [], 0
    for b in range(len(x) // n):
        fe.push_block(x[b * n:(b + 1) * n])
        ora.push_block(x[b * n:(b + 1) * n])
        part = fe.poll_pdus(max_in_flight=1)
        early += len(part)
        got += part
    got += fe.poll_pdus()
    cnt = fe.counters()
    assert cnt["pdus_dropped"] == 0 and cnt["pdus_taken"] == len(got) and cnt["pdu_ring_capacity"] == (ring or 4096)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, ora.pdus)) and len(got) >= len(bursts) - 1
    assert early >= len(got) - len(freqs)                 # all but the last block's worth arrived through the lagging path
    stats = fe.all_channel_stats()
    assert [s["freq"] for s in stats] == freqs
    assert [s["frames"] for s in stats] == [fe.channel_stats(c)["frames"] for c in range(len(freqs))]
    fe.close()


def test_prefetched_uploads_same_pdus(gpu, oracle):
    """hfdl_gpu_frontend_prefetch_block_raw: uploads are queued up to geometry.prefetch_depth blocks ahead of their pushes (page-locked
    buffer, cs16 converted on the device, a ring of fold_batch + 2 staging buffers in HBM), at every distance from 0 (pushed without a
    prefetch) to the full depth; slots are released through input_done_upto() / input_copied().  Same PDUs as the oracle fed the same
    quantised samples; misuse (a block other than the oldest prefetched one pushed, one prefetch too many, a buffer that is not
    page-locked) is refused and leaves the front end usable."""
    import ctypes
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000]
    dur = 10.0
    bursts = synth.plan_traffic(freqs, dur, seed=41, dense=True, gap_s=0.15, amp=(0.03, 0.1))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=41)
    raw = np.clip(np.round(x.view(np.float32) * 20000), -32768, 32767).astype(np.int16)
    xq = (raw.astype(np.float32) / np.float32(32767.5)).view(np.complex64)          # convert_cs16, src/input-helpers.c:56-66
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n = fe.input_size
    nb = len(x) // n
    depth = fe.geometry.prefetch_depth
    assert depth == fe.geometry.fold_batch + 1 == 9 and nb > 3 * depth          # 4 channels: halves of 8 blocks, a staging ring of 10
    hbuf = gpu.host_alloc(raw.nbytes)
    ctypes.memmove(hbuf, raw.ctypes.data, raw.nbytes)
    ptr = lambda b: hbuf + 4 * b * n
    got = []
    for b in range(depth):
        fe.prefetch_host_ptr(ptr(b), F.SFMT_CS16)
    with pytest.raises(gpu.GpuError):
        fe.prefetch_host_ptr(ptr(depth), F.SFMT_CS16)                   # one too many
    with pytest.raises(gpu.GpuError):
        fe.push_host_ptr(ptr(1), F.SFMT_CS16)                           # not the OLDEST prefetched block
    dev_blk = np.zeros(n, np.complex64)
    with pytest.raises(gpu.GpuError):
        fe.push_block(dev_blk)                                          # nor anything else while prefetches are pending ...
    fe.prefetch_cancel()                                                # ... until they are cancelled: the front end takes any block again
    fe.prefetch_cancel()                                                # (no-op without a prefetch)
    fe.input_done_upto(depth - 1)                                       # the cancelled blocks kept their numbers: answers at once
    assert fe.input_copied(0) and fe.input_copied(depth - 1)
    base, q = depth, 0                                                  # stream block b is host block base + b from here on
    for b in range(nb):
        ahead = (b * 7) % (depth + 1)                                   # 0 .. depth uploads queued ahead of this push
        while q < nb and q - b < ahead:
            fe.prefetch_host_ptr(ptr(q), F.SFMT_CS16)
            q += 1
        fe.push_host_ptr(ptr(b), F.SFMT_CS16)                           # the oldest prefetched block, or (ahead == 0) a block uploaded now
        q = max(q, b + 1)
        if b >= 1:
            fe.input_done_upto(base + b - 1)
            assert fe.input_copied(base + b - 1)
        got += fe.poll_pdus(max_in_flight=1)
        ora.push_block(xq[b * n:(b + 1) * n])
    got += fe.poll_pdus()
    with pytest.raises(gpu.GpuError):
        fe.input_done_upto(base + nb + 1)                               # never uploaded
    fe.input_done_upto(0)                                               # long overwritten events: still answers
    pageable = np.zeros(2 * n, np.int16)
    with pytest.raises(gpu.GpuError):
        fe.prefetch_host_ptr(pageable.ctypes.data, F.SFMT_CS16)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, got)) == sorted(map(key, ora.pdus)) and len(got) >= len(bursts) - 1
    fe.close()
    gpu.host_free(hbuf)


def test_demodulator_batching_changes_nothing(gpu, oracle, monkeypatch):
    """On the demodulator-bound geometries one demodulator launch takes several consecutive blocks when they are pushed faster than
    they are collected (hfdl_gpu_geometry.demod_batch).  The per-channel state is carried sample by sample, so every PDU -- octets,
    detection sample, frequency error, levels, training-bit counts -- and every channel's counters equal those of a launch per block
    (HFDL_GPU_DEMOD_BATCH=1), whatever mix of pushes, lagging collections and draining polls cuts the batches."""
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
    dur = 16.0
    bursts = synth.plan_traffic(freqs, dur, seed=77, dense=True, gap_s=0.12, amp=(0.02, 0.1))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.012, seed=77)

    def run(batch_env, pattern):
        if batch_env is None:
            monkeypatch.delenv("HFDL_GPU_DEMOD_BATCH", raising=False)
        else:
            monkeypatch.setenv("HFDL_GPU_DEMOD_BATCH", str(batch_env))
        fe = gpu.Frontend(fs, cf, freqs)
        n, got = fe.input_size, []
        for b in range(len(x) // n):
            fe.push_block(x[b * n:(b + 1) * n])
            if pattern == "lagging":
                got += fe.poll_pdus(max_in_flight=1)
            elif pattern == "ragged" and b % 7 in (2, 3):           # a draining poll every few blocks: batches of 3, 1 and 4 blocks
                got += fe.poll_pdus()
        got += fe.poll_pdus()
        stats = fe.all_channel_stats()
        batch = fe.geometry.demod_batch
        fe.close()
        return sorted(got, key=lambda p: (p["freq"], p["sample_index"])), stats, batch

    ref, ref_stats, b1 = run(1, "end")
    assert b1 == 1 and len(ref) >= len(bursts) - 2
    for pattern in ("end", "lagging", "ragged"):
        got, stats, bn = run(None, pattern)
        assert bn >= 2, "this geometry (0.115 s blocks, 5 channels) batches"
        assert got == ref, pattern                                    # every field of every PDU
        assert stats == ref_stats, pattern
    # and what a launch per block gives is what the oracle gives
    ora = oracle.Frontend(fs, cf, freqs)
    n = ora.ddc.input_size
    for b in range(len(x) // n):
        ora.push_block(x[b * n:(b + 1) * n])
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    assert sorted(map(key, ref)) == sorted(map(key, ora.pdus))
    # the reference's debug summary (hfdl_print_summary, src/hfdl.c:563-573) per channel, from the device state
    for c in range(len(freqs)):
        want, have = ora.channel_summary(c), ref_stats[c]
        assert (have["a1_found"], have["a2_found"], have["m1_found"], have["m1_not_found"]) == (want["a1_found"], want["a2_found"], want["m1_found"], want["m1_not_found"])
        assert (have["train_bits_bad"], have["train_bits_total"]) == (want["train_bits_bad"], want["train_bits_total"])
        for k, cnt in (("a1", "a1_found"), ("a2", "a2_found"), ("m1", "m1_found")):
            if want[cnt]:
                assert have[k + "_corr_avg"] == pytest.approx(want[k + "_corr_total"] / want[cnt], rel=1e-5)


def test_demodulator_stage_fed_with_the_oracles_channelizer_output(gpu, oracle):
    """hfdl_gpu_frontend_push_baseband: the device's demodulator + burst decoder alone, fed block by block with the ORACLE's channelizer
    output (the two channelizers round differently -- other FFT factorisation -- so only this feed compares the demodulators on the same
    input).  Every PDU field and channel counter is the oracle's; the shipped pipeline's symbols stay within 1e-4 of the oracle's in the
    typical block (what is left is the AGC's hardware log / exp and the scan-order sums: profiles/r04/strict_study.md) -- between
    bursts the loops random-walk on noise and the two drift apart in the last bits, which is why the gate is the median block and
    the bit-for-bit comparison is the strict build's (tests/test_gpu_strict.py: 0 of 80519 symbols differ)."""
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000]
    dur = 14.0
    bursts = synth.plan_traffic(freqs, dur, seed=53, dense=True, gap_s=0.12, amp=(0.02, 0.1))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.012, seed=53)
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n, got, errs, nsym = fe.input_size, [], [], 0
    for b in range(len(x) // n):
        ora.push_block(x[b * n:(b + 1) * n])
        fe.push_baseband([ora.channel_view(c)["chan_out"] for c in range(len(freqs))])
        got += fe.poll_pdus()
        for c in range(len(freqs)):
            a, w = fe.read_tap(F.TAP_SYMBOLS, c), ora.channel_view(c)["symbols"]
            assert len(a) == len(w), (b, c)
            if len(w):
                errs.append(rel_rms(a, w))
                nsym += len(w)
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"], p["train_bits_bad"], p["train_bits_total"])
    assert sorted(map(key, got)) == sorted(map(key, ora.pdus)) and len(got) >= len(bursts) - 2
    assert nsym > 80_000 and float(np.median(errs)) < 1e-4, (float(np.median(errs)), max(errs))
    for c in range(len(freqs)):
        want, have = ora.channel_summary(c), fe.channel_stats(c)
        assert (have["a1_found"], have["a2_found"], have["m1_found"], have["m1_not_found"]) == (want["a1_found"], want["a2_found"], want["m1_found"], want["m1_not_found"])
    import ctypes as C                                   # a count beyond what a block holds is refused (HFDL_GPU_ERANGE), nothing is queued
    row = fe.geometry.max_outputs_per_block + 1
    buf, cnt = np.zeros((len(freqs), row), np.complex64), np.full(len(freqs), row + 1, np.int32)
    assert F.load().hfdl_gpu_frontend_push_baseband(fe._h, buf.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)) == -5
    assert fe.poll_pdus() == []
    fe.close()
    ora.close()


@pytest.mark.parametrize("fs,nch", [(250000, 5), (2_400_000, 130)])
def test_fold_batching_changes_nothing(gpu, monkeypatch, fs, nch):
    """One fold launch multiplies the spectra of up to geometry.fold_batch (16) queued blocks against ONE pass over the filter taps on
    the matrix pipe (fold_kernels.hip; src/fastddc.c:123-150 run for that many blocks).  Every bin's sum is the same FMA chain whatever
    the company, so the channelizer output of EVERY block -- read back per block, compared as uint32 -- and every PDU equal those of a
    pass over the taps per block (HFDL_GPU_FOLD_BATCH=1: the four-column form of the kernel, K = 1 products in the order of the K = 4
    instruction), for full batches of 16 / 8 (the sixteen-column form) / 4 / 2 and the ragged batches that draining polls / syncs
    cut (13, 7, 5: columns past the last block computed and dropped; 3, 1: the four-column form) -- and, since round 6, for batches of
    17 .. 32 blocks, which run the thirty-two-column form (two spectrum operands per loaded tap operand).  5 channels: demodulator-bound
    geometry (several blocks per demodulator launch, five channels padded to an octet, only the single-wave workgroups of the
    left-over octets run); 130 channels: fold-bound shape (two 64-channel workgroups + one left-over octet; demodulator launches
    held back behind the next half's forward FFTs)."""
    cf = 10_000_000
    rng = np.random.default_rng(nch)
    if nch == 5:
        freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
        dur = 9.0
        bursts = synth.plan_traffic(freqs, dur, seed=31, dense=True, gap_s=0.12, amp=(0.02, 0.1))
    else:
        freqs = [int(cf + (i - nch // 2) * 15_000 + 4_000) for i in range(nch)]
        dur = 10.2              # 53 blocks (a short first half, a 32-block launch and a ragged one); a single-slot burst lasts 2.5 s
        bursts = [dict(freq=freqs[c], mode=int(rng.integers(0, 4)), octets=b"", t0=float(rng.uniform(0.1, 0.7)), amp=0.03, cfo=float(rng.uniform(-10, 10)))
                  for c in (0, 3, 64, 77, 128, 129)]
        for b in bursts:
            b["octets"] = synth.make_pdu(rng, b["mode"])
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.012, seed=31)
    watch = sorted(set([0, 1, nch // 2, nch - 2, nch - 1]))

    def run(fold_env, cuts, x=x):
        monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", str(fold_env))
        fe = gpu.Frontend(fs, cf, freqs)
        g = fe.geometry
        assert g.fold_batch == fold_env
        n, nblk = fe.input_size, len(x) // fe.input_size
        outs, got, b, i = [], [], 0, 0
        while b < nblk:
            k = min(cuts[i % len(cuts)], nblk - b)
            i += 1
            for j in range(k):
                fe.push_block(x[(b + j) * n:(b + j + 1) * n])
            got += fe.poll_pdus()                 # closes the half as it is: one fold launch for its k blocks
            half = min(32, -(-max(g.fold_batch, g.demod_batch) // g.fold_batch) * g.fold_batch)      # blocks a half holds (planner.h plan_batches, half_blocks)
            # blocks of the newest half: what read_tap(back=...) still reaches.  After a drain the first half closes at 16 blocks where the
            # fold bounds the block (128 channels and more) and a half holds more; the following ones take all `half` slots
            held, target = k, (16 if (nch >= 128 and half > 16) else half)
            while held > target:
                held, target = held - target, half
            for j in range(held):
                outs.append((b + k - held + j, [fe.read_tap(F.TAP_CHAN_OUT, c, back=held - 1 - j).view(np.uint32).copy() for c in watch]))
            b += k
        stats = fe.all_channel_stats()
        fe.close()
        return dict(outs), sorted(got, key=lambda p: (p["freq"], p["sample_index"])), stats

    ref_outs, ref_pdus, ref_stats = run(1, [1])
    assert len(ref_outs) == len(x) // (28672 if fs == 250000 else 458752)
    assert len(ref_pdus) >= len(bursts) - 2
    for fold_env, cuts in ((4, [4]), (4, [3, 1, 2, 4]), (8, [8]), (8, [7, 5, 8, 3]), (2, [2, 1]), (16, [16]), (16, [13, 5, 16, 3, 9]), (32, [32]), (32, [17, 25, 9, 32, 20]), (32, [52, 21])):      # 52 without a poll: 16 (the first half after a drain), 32, then 4
        outs, pdus, stats = run(fold_env, cuts)
        assert outs, (fold_env, cuts)
        for blk, chans in outs.items():
            for c, a in zip(watch, chans):
                assert np.array_equal(a, ref_outs[blk][watch.index(c)]), (fold_env, cuts, blk, c)
        assert pdus == ref_pdus, (fold_env, cuts)       # every field of every PDU
        assert stats == ref_stats, (fold_env, cuts)
    # a second input scale: the same samples times 2^-100 and 2^-115 (products of spectrum and stop-band taps at and below the fp32
    # minimum normal), then a run of exact zeros followed by normal blocks -- the three matrix forms must treat subnormals alike, or a
    # block's output would depend on how many blocks were queued with it
    # (noise only at the low scales: what a demodulator makes of a burst 2^-100 down is not this test's subject)
    n = 28672 if fs == 250000 else 458752
    quiet = synth.synth_wideband(fs, cf, 28 * n, [], noise_sigma=0.012, seed=32)
    tiny = np.concatenate([quiet[:14 * n] * np.float32(2.0 ** -100), quiet[14 * n:] * np.float32(2.0 ** -115), np.zeros(6 * n, np.complex64), x[34 * n:40 * n]])
    ref_outs, ref_pdus, ref_stats = run(1, [1], tiny)
    assert len(ref_outs) == 40
    nonzero = np.mean([np.mean(a != 0) for chans in ref_outs.values() for a in chans])
    print("subnormal-scale stream: share of non-zero output words %.3f" % nonzero)
    assert nonzero > 0.5
    for fold_env, cuts in ((4, [3, 1, 2, 4]), (16, [13, 5, 16, 3, 9]), (32, [17, 25, 9, 32, 20]), (32, [40])):
        outs, pdus, stats = run(fold_env, cuts, tiny)
        assert outs, (fold_env, cuts)
        for blk, chans in outs.items():
            for c, a in zip(watch, chans):
                assert np.array_equal(a, ref_outs[blk][watch.index(c)]), ("tiny", fold_env, cuts, blk, c)
        assert pdus == ref_pdus and stats == ref_stats, ("tiny", fold_env, cuts)


@pytest.mark.parametrize("fs,nch", [(250000, 5), (2_400_000, 130), (1_200_000, 32)])
def test_fold_mfma_equals_fma_chain(gpu, monkeypatch, fs, nch):
    """The fold runs on the fp32 matrix pipe: v_mfma_f32_16x16x4_f32 (per instruction one bin x eight channels' Re / Im rows x FOUR alias
    rows x sixteen blocks; taps in the octet-interleaved layout, four rows per KiB).  One instruction adds its four products to the
    accumulator one after the other, each an exact fmaf (profiles/micro/mfma_k4.hip), so every compiled tiling (the sweep set of the
    laboratory build included) must leave the partial sums of EVERY block count 1 .. 32 (17 .. 32: the thirty-two-column tilings, which
    are also run at 16 and fewer) bit-identical to the plain-VALU reference
    kernel, which spells each bin's sum out as the same chain of fused multiply-adds one thread at a time: the checksum over the bit
    patterns of all partial sums is compared, the buffer poisoned before every kernel.  5 channels: one octet (three channels of zero
    taps), the single-wave workgroups only; 130: two 64-channel workgroups + a left-over octet; 32: single-wave workgroups again."""
    cf = 10_000_000
    lab = F.load_lab()
    freqs = [int(cf + (i - nch // 2) * (15_000 if nch > 5 else 40_000) + 4_000) for i in range(nch)]
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "32")
    fe = gpu.Frontend(fs, cf, freqs, lib=lab)
    g = fe.geometry
    assert g.fold_batch == 32
    rng = np.random.default_rng(nch)
    n = fe.input_size
    for b in range(16):
        fe.channelize_block((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(0.1))
    # channelize_block closes a half per block; fill one half with 32 spectra for the probe.  Three fillings: the normal range; the
    # same kind of noise times 2^-100 and 2^-115 (alternating blocks: spectrum times stop-band taps of ~1e-7 and less puts products and
    # partial sums at and below the fp32 minimum normal -- the matrix instructions' three forms and the VALU chain must treat
    # subnormals alike, or a block's output would depend on its company); sixteen blocks of exact zeros, then sixteen normal ones.
    variants = F.fold_variants()
    assert {nbmax for (_, _, _, _, nbmax, _) in variants} == {4, 16, 32}
    fillings = (("normal", lambda b: np.float32(0.1)),
                ("subnormal products", lambda b: np.float32(0.1) * np.float32(2.0 ** (-100 if b % 2 == 0 else -115))),
                ("zeros, then normal", lambda b: np.float32(0.0 if b < 16 else 0.1)))
    sums = {}
    for name, scale in fillings:
        for b in range(32):
            fe.push_block((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * scale(b))
        fe.sync()
        ran = 0
        for nb in (1, 2, 3, 4, 5, 8, 11, 13, 16, 17, 21, 31, 32):
            ref = fe.fold_variant_probe(-1, nb, 1)[2]
            sums[(name, nb)] = ref
            for v, (p, q, w, d, nbmax, layout) in enumerate(variants):
                if nb > nbmax or layout != 2:
                    continue
                try:
                    chk = fe.fold_variant_probe(v, nb, 1)[2]
                except gpu.GpuError:
                    continue                              # rows per slice not a multiple of the tiling's look-ahead
                assert chk == ref, (name, nb, (p, q, w, d, layout))
                ran += 1
        assert ran >= 13, name
    assert len(set(sums.values())) > 13               # the fillings really differ (a checksum of all-zero sums would agree trivially)
    fe.close()


def test_fft_stream_switch_changes_nothing(gpu, monkeypatch):
    """HFDL_GPU_FFT_STREAM=1 (forward FFTs of the half being filled on a stream of their own, beside the fold of the half before: two
    sets of spectra, phasor tables and state snapshots chained by events) is an A/B switch of the LABORATORY build (measured slower on
    cfg3): it must give the same channelizer output, bit for bit, and the same PDUs -- full halves, ragged cuts,
    lagging collections and channelizer-only blocks in between.  The reference run goes through the product library, which does not
    read the switch at all: the laboratory build's default path is the product's."""
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
    dur = 10.0
    bursts = synth.plan_traffic(freqs, dur, seed=61, dense=True, gap_s=0.12, amp=(0.02, 0.1))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.012, seed=61)

    def run(own_stream):
        monkeypatch.setenv("HFDL_GPU_FFT_STREAM", "1")                 # the product library ignores it
        fe = gpu.Frontend(fs, cf, freqs, lib=F.load_lab() if own_stream else None)
        n, got, outs = fe.input_size, [], []
        for b in range(len(x) // n):
            blk = x[b * n:(b + 1) * n]
            if b == 20:
                fe.channelize_block(blk)               # never demodulated, in both runs
                outs.append(fe.read_tap(F.TAP_CHAN_OUT, 3).view(np.uint32).copy())
                continue
            fe.push_block(blk)
            if b % 11 == 4:
                got += fe.poll_pdus()                  # a draining poll: a ragged half
                outs.append(fe.read_tap(F.TAP_CHAN_OUT, 1).view(np.uint32).copy())
            elif b % 5 == 0:
                got += fe.poll_pdus(max_in_flight=1)
        got += fe.poll_pdus()
        outs.append(fe.read_tap(F.TAP_CHAN_OUT, 4).view(np.uint32).copy())
        stats = fe.all_channel_stats()
        fe.close()
        return sorted(got, key=lambda p: (p["freq"], p["sample_index"])), outs, stats

    ref, ref_outs, ref_stats = run(False)
    got, outs, stats = run(True)
    assert len(ref) >= len(bursts) - 3 and got == ref and stats == ref_stats
    assert len(outs) == len(ref_outs) and all(np.array_equal(a, b) for a, b in zip(outs, ref_outs))


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_call_sequences_equal_a_launch_per_block(gpu, monkeypatch, seed):
    """The batching state machine under random use: after every pushed block one of {nothing, lagging collection, draining poll, sync,
    statistics read, stage-tap read} at random, and now and then a block that only goes through the channelizer (never demodulated, in
    both runs).  Whatever the sequence cuts the batches into, PDUs (every field) and channel statistics equal those of the same sequence
    with one block per launch."""
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000]
    dur = 14.0
    bursts = synth.plan_traffic(freqs, dur, seed=100 + seed, dense=True, gap_s=0.12, amp=(0.02, 0.1))
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.012, seed=100 + seed)
    rng = np.random.default_rng(seed)
    nblk = len(x) // 28672
    script = [(str(rng.choice(["none", "none", "none", "lag", "lag", "drain", "sync", "stats", "tap"])), bool(rng.random() < 0.04)) for _ in range(nblk)]

    def run(batch_env):
        if batch_env is None:
            monkeypatch.delenv("HFDL_GPU_DEMOD_BATCH", raising=False)
        else:
            monkeypatch.setenv("HFDL_GPU_DEMOD_BATCH", str(batch_env))
        fe = gpu.Frontend(fs, cf, freqs)
        n, got = fe.input_size, []
        assert n == 28672
        for b, (act, chan_only) in enumerate(script):
            blk = x[b * n:(b + 1) * n]
            if chan_only:
                fe.channelize_block(blk)
                continue
            fe.push_block(blk)
            if act == "lag":
                got += fe.poll_pdus(max_in_flight=1)
            elif act == "drain":
                got += fe.poll_pdus()
            elif act == "sync":
                fe.sync()
            elif act == "stats":
                fe.all_channel_stats()
            elif act == "tap":
                fe.read_tap(F.TAP_CHAN_OUT, 1)
        got += fe.poll_pdus()
        stats = fe.all_channel_stats()
        cnt = fe.counters()
        fe.close()
        assert cnt["pdus_dropped"] == 0 and cnt["pdus_taken"] == len(got)
        return sorted(got, key=lambda p: (p["freq"], p["sample_index"])), stats

    ref, ref_stats = run(1)
    got, stats = run(None)
    assert len(ref) >= 8
    assert got == ref and stats == ref_stats


def test_random_call_sequences_on_a_fold_bound_geometry(gpu):
    """The same on a geometry with 128 channels, where a block's demodulator launch is held back until the next block's forward FFT
    is queued: whatever is called between the pushes -- lagging collections, draining polls, syncs, statistics and tap reads,
    channelizer-only blocks -- the PDUs and channel statistics are those of plain pushes with one poll at the end."""
    fs, cf = 2_400_000, 10_000_000
    freqs = [int(cf + (i - 64) * 15_000 + 4_000) for i in range(128)]
    rng = np.random.default_rng(5)
    bursts = [dict(freq=freqs[c], mode=int(rng.integers(0, 4)), octets=b"", t0=float(rng.uniform(0.2, 0.8)), amp=0.03, cfo=float(rng.uniform(-10, 10)))
              for c in (3, 40, 77, 101, 126)]
    for b in bursts:
        b["octets"] = synth.make_pdu(rng, b["mode"])
    dur = 3.6
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.01, seed=5)

    def run(script):
        fe = gpu.Frontend(fs, cf, freqs)
        assert fe.geometry.demod_batch >= 2          # 0.19 s blocks: two fit the demodulator's LDS
        n, got = fe.input_size, []
        for b in range(len(x) // n):
            blk = x[b * n:(b + 1) * n]
            act, chan_only = script[b % len(script)]
            if chan_only:
                fe.channelize_block(blk)
                continue
            fe.push_block(blk)
            if act == "lag":
                got += fe.poll_pdus(max_in_flight=1)
            elif act == "drain":
                got += fe.poll_pdus()
            elif act == "sync":
                fe.sync()
            elif act == "stats":
                fe.all_channel_stats()
            elif act == "tap":
                fe.read_tap(F.TAP_CHAN_OUT, 5)
        got += fe.poll_pdus()
        stats = fe.all_channel_stats()
        fe.close()
        return sorted(got, key=lambda p: (p["freq"], p["sample_index"])), stats

    nblk = len(x) // gpu.plan_geometry(256, 250 / fs).input_size
    skip = [bool(rng.random() < 0.05) for _ in range(nblk)]
    skip[:3] = [False] * 3
    plain = [("none", s) for s in skip]
    mixed = [(str(rng.choice(["none", "lag", "lag", "drain", "sync", "stats", "tap"])), s) for s in skip]
    ref, ref_stats = run(plain)
    got, stats = run(mixed)
    assert len(ref) >= 3 and got == ref and stats == ref_stats


def test_full_pdu_ring_drops_and_counts(gpu, oracle, monkeypatch):
    """More frames finishing in one block than the device ring holds: the surplus is dropped and counted, what is
    delivered is intact, and the ring keeps working afterwards."""
    monkeypatch.setenv("HFDL_GPU_PDU_RING", "16")
    fs, cf = 1_000_000, 10_000_000
    freqs = [int(cf + (i - 32) * 14_000 + 3_000) for i in range(64)]
    rng = np.random.default_rng(12)
    bursts = [dict(freq=f, mode=0, octets=synth.make_pdu(rng, 0), t0=0.3, amp=0.02, cfo=0.0) for f in freqs]
    late = dict(freq=freqs[5], mode=1, octets=synth.make_pdu(rng, 1), t0=3.4, amp=0.02, cfo=0.0)
    x = synth.synth_wideband(fs, cf, int(6.5 * fs), bursts + [late], noise_sigma=0.002, seed=12)
    fe = gpu.Frontend(fs, cf, freqs)
    n = fe.input_size
    got = []
    for b in range(len(x) // n):
        fe.push_block(x[b * n:(b + 1) * n])
        got += fe.poll_pdus()
    cnt = fe.counters()
    sent = {b["octets"] for b in bursts}
    first = [p for p in got if p["mode"] == 0]
    assert len(first) == 16 and cnt["pdus_dropped"] == 64 - 16
    assert all(p["octets"][:len(next(iter(sent)))] in sent for p in first)
    assert [p["octets"][:len(late["octets"])] for p in got if p["mode"] == 1] == [late["octets"]]
    fe.close()


def test_host_c_program_live_pipe(gpu, oracle):
    """A source that the front end keeps up with (samples arrive through a pipe, paced at ~4 x real time): the C host then
    drains after every block instead of lagging one block behind, and must deliver the same PDUs."""
    import os
    import subprocess
    import time
    fs, cf = 250000, 10_000_000
    freqs = [9_930_000, 10_037_000, 10_081_500]
    bursts = synth.plan_traffic(freqs, 6.0, seed=13, dense=True)
    x = synth.synth_wideband(fs, cf, int(6.0 * fs), bursts, noise_sigma=0.01, seed=13)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dumphfdl_amd", "hfdl_replay")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "dumphfdl_amd", "host")])
    proc = subprocess.Popen([exe, "--iq-file", "-", "--sample-rate", str(fs), "--sample-format", "CF32", "--centerfreq", str(cf / 1e3),
                             "--statsd-print", "--noise-floor-stats-interval", "1"]
                            + ["%.3f" % (f / 1e3) for f in freqs], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    raw = x.view(np.float32).tobytes()
    step = 8 * 28672                                    # one block of this geometry
    import threading
    arrivals, lines = [], []

    def reader():                                       # every PDU line with the wall time it came out at (the sink flushes per PDU)
        for ln in proc.stdout:
            arrivals.append(time.monotonic())
            lines.append(ln.decode())
    th = threading.Thread(target=reader, daemon=True)
    th.start()
    time.sleep(3.0)                                     # let the front end come up (filter design, 3 channels) before pacing matters
    written = []
    for off in range(0, len(raw), step):
        proc.stdin.write(raw[off:off + step])
        proc.stdin.flush()
        written.append(time.monotonic())
        time.sleep(0.03)
    time.sleep(2.2)                                     # source idle, program still running: the 1 s gauge thread reports the settled values
    t_closed = time.monotonic()
    proc.stdin.close()
    err = proc.stderr.read().decode()
    assert proc.wait(timeout=120) == 0, err
    th.join(timeout=30)
    out = "".join(lines)
    # latency of a paced source: PDUs leave while the source is still feeding -- a block's PDUs are delivered a grace period
    # (a quarter of a block, 29 ms here, counted from the block's arrival) after it, not when the program shuts down
    pdu_t = [t for t, ln in zip(arrivals, lines) if ln.startswith("PDU ")]
    assert pdu_t and max(pdu_t) < written[-1] + 0.5 < t_closed, (max(pdu_t) - written[-1], t_closed - written[-1])
    assert min(pdu_t) < written[len(written) // 2], "no PDU before half of the samples were fed"
    got = []
    for line in out.splitlines():
        if line.startswith("PDU "):
            kv = dict(t.split("=") for t in line.split()[1:-1])
            got.append((int(kv["freq"]), int(kv["bit_rate"]), kv["slot"], bytes.fromhex(line.split()[-1])))
    ora = oracle.Frontend(fs, cf, freqs)
    n = ora.ddc.input_size
    for b in range(len(x) // n):
        ora.push_block(x[b * n:(b + 1) * n])
    assert sorted(got) == sorted((p["freq"], p["bit_rate"], p["slot"], p["octets"]) for p in ora.pdus) and len(got) == len(bursts)
    # the noise-floor gauge thread (hfdl_nf_stats_thread_start, src/hfdl.c:1082-1105) reported every channel at least once,
    # in tenths of -dBFS (with back-to-back bursts the estimate rides between the noise and the burst level)
    gauges = [l.split() for l in err.splitlines() if l.startswith("STATSD gauge ")]
    last = {int(g[2].split(".")[0]): int(g[3]) for g in gauges if g[2].endswith(".noise_floor")}     # before the first samples it is the start value
    assert set(last) == set(freqs), err
    assert all(50 <= v <= 900 for v in last.values()), last


def test_host_c_program_channel_shards(gpu, oracle, tmp_path):
    """hfdl_replay --shard R/W (single stream over W GPUs): every shard reads the same file and decodes channels
    R, R+W, ...; the shards' PDUs are disjoint by channel and their union is what the unsharded program prints."""
    fs, cf = 250000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
    bursts = synth.plan_traffic(freqs, 6.5, seed=17, dense=True)
    x = synth.synth_wideband(fs, cf, int(6.5 * fs), bursts, noise_sigma=0.01, seed=17)
    raw = np.clip(np.round(x.view(np.float32) * 20000), -32768, 32767).astype(np.int16)
    whole = _replay(tmp_path, raw, "CS16", fs, cf, freqs)
    s0 = _replay(tmp_path, raw, "CS16", fs, cf, freqs, extra=["--shard", "0/2"])
    s1 = _replay(tmp_path, raw, "CS16", fs, cf, freqs, extra=["--shard", "1/2"])
    assert {p[0] for p in s0} <= {freqs[0], freqs[2], freqs[4]} and {p[0] for p in s1} <= {freqs[1], freqs[3]}
    assert sorted(s0 + s1) == sorted(whole) and len(whole) >= len(bursts) - 1


def test_long_idle_then_marginal_snr(gpu, oracle):
    """Both hard cases at once: 36 s of noise (past the 13-frame search timeout that resets the loops, src/hfdl.c:745-752) so the
    device's and the oracle's timing / carrier loops have decorrelated in the last ulps, THEN bursts at -3..6 dB in-channel
    SNR, where a frame's fate can hang on one soft decision.  Identical behaviour is not a theorem here (the two float
    trajectories differ); the gate is statistical: nearly every PDU either side dispatches is dispatched by both with the same
    octets and mode, the detection instants agree within one symbol, and the event counters stay close."""
    fs, cf = 250000, 10_000_000
    freqs = [int(cf + (i - 8) * 13_000 + 2_500) for i in range(16)]
    idle = 36.0
    rng = np.random.default_rng(77)
    bursts = []
    for f in freqs:
        t = idle + float(rng.uniform(0.2, 0.6))
        for _ in range(2):
            mode = int(rng.integers(0, 4))
            amp = float(10 ** (rng.uniform(-3, 6) / 20) * 0.0063)          # in-channel noise rms ~ 0.0063 at sigma 0.02
            bursts.append(dict(freq=f, mode=mode, octets=synth.make_pdu(rng, mode), t0=t, amp=amp, cfo=float(rng.uniform(-20, 20))))
            t += synth.burst_symbols_len(mode) / 1800 + 0.4
    dur = max(b["t0"] for b in bursts) + 2.8
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs, nthreads=8)
    n = fe.input_size
    total, done, k = int(dur * fs) // n * n, 0, 0
    while done < total:
        m = min(40 * n, total - done)
        live = [dict(b, t0=b["t0"] - done / fs) for b in bursts if -6 < b["t0"] - done / fs < m / fs + 1]
        x = synth.synth_wideband(fs, cf, m, live, noise_sigma=0.02, seed=770 + k)
        for b in range(m // n):
            fe.push_block(x[b * n:(b + 1) * n])
            ora.push_block(x[b * n:(b + 1) * n], nthreads=8)
        done, k = done + m, k + 1
    got, want = fe.poll_pdus(), ora.pdus
    key = lambda p: (p["freq"], p["mode"], p["octets"])
    A, B = {key(p) for p in got}, {key(p) for p in want}
    assert len(A) == len(got) and len(B) == len(want)
    assert min(len(A), len(B)) >= 12                                  # the bursts are detectable at all
    assert len(A & B) >= 0.9 * max(len(A), len(B)), (len(A), len(B), len(A & B))
    gi = {key(p): p for p in got}
    for p in want:
        if key(p) in gi:
            assert abs(gi[key(p)]["sample_index"] - p["sample_index"]) <= 3
            assert abs(gi[key(p)]["freq_err_hz"] - p["freq_err_hz"]) < 1.0
    sent = [p for p in got if any(p["octets"][:len(b["octets"])] == b["octets"] for b in bursts if b["freq"] == p["freq"])]
    assert 4 <= len(sent) <= len(bursts)                              # marginal: some right, some wrong or missed
    a2g = sum(fe.channel_stats(c)["a2_found"] for c in range(len(freqs)))
    a2o = sum(ora.channel_counters(c)["a2_found"] for c in range(len(freqs)))
    assert abs(a2g - a2o) <= max(2, 0.1 * a2o)
    fe.close()
