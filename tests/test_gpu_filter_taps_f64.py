"""GPU tests: what the device holds for a channel -- its frequency-domain filter (build_taps: upload, zero-pad, forward FFT, the last
pass writing the matrix-operand layout) and the residual NCO it runs -- against tests/ddc_design_f64.py, the plan and taps written from
the definition with nothing of the oracle's or the product's in them; at create, over two receivers, after a retune, and end to end.

The filter: want = the float64 transform of the model's sharp-form taps (fp32 phase register and normalising sum, as the reference
designs them) zero-padded to N, halves swapped.  One gate, e_gpu <= 4 max(e_ora, floor), on relative RMS and on worst element over the
largest |H|: e_ora is the oracle's filter (oracle.Channel.taps_fft) against the same `want`, floor the figure the CPU suite measured
for it (tests/test_ddc_design_f64_cpu.py SPECTRUM_FLOOR, oracle/PINNING.md section 7).  Device and oracle are handed integers (centre,
frequency) only: the 1440 Hz of the carrier, the sign of the shift and the cut-offs are each side's own."""
import time

import numpy as np
import pytest

import ddc_design_f64 as D
import ddc_f64 as M
from dumphfdl_amd import frontend as F
from test_channelizer_f64_cpu import channel_offsets
from test_ddc_design_f64_cpu import SPECTRUM_FLOOR, spectrum_errors
from test_gpu_channelizer_f64 import FLOOR, read_blocks

pytestmark = pytest.mark.gpu

CF = 10_000_000


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def model_filter(fs, centre, freq):
    c = D.channel(fs, centre, freq)
    return np.fft.fftshift(D.spectrum(D.channel_taps(fs, centre, freq)["phase32+sum32"], c.fft_size))


def check_filter(tag, oracle, fs, centre, freq, got, floor):
    """One channel's filter as read from the device against the model of (centre, freq); the oracle's calibrates the gate."""
    want = model_filter(fs, centre, freq)
    assert len(got) == len(want)
    och = oracle.Channel(fs, centre, freq)
    e_ora = spectrum_errors(och.taps_fft(), want)
    och.close()
    e_gpu = spectrum_errors(got, want)
    print("%s, %d Hz (carrier %+d Hz from %d): e_gpu rms %.3g max %.3g | e_ora rms %.3g max %.3g"
          % (tag, freq, freq + 1440 - centre, centre, e_gpu[0], e_gpu[1], e_ora[0], e_ora[1]))
    for i in range(2):
        assert e_gpu[i] <= 4 * max(e_ora[i], floor[i]), (tag, freq, "rms" if i == 0 else "max", e_gpu, e_ora)
    return e_gpu, e_ora


def check_phasors(tag, fs, centre, freq, tables, first_k=0):
    """tables: the NCO phasor tables of consecutive blocks of one channel, the first starting at output number first_k.  Every table
    against exp(j pi nco_rate K) of the model within the bound tests/test_gpu_channelizer_f64.py uses (fp32 start phase, <= 2 ulp(pi) a
    block, + a recurrence of <= 4 roundings a step), and the angle between consecutive phasors of a block against pi nco_rate within
    4 x 2^-23: a step of the recurrence is three roundings of 2^-24 per component (4.3 x 2^-24 as a vector) and the two fp32 words it
    turns by are each 2^-25 off."""
    c = D.channel(fs, centre, freq)
    rate = c.nco_rate32
    k0, worst_tab, worst_step = first_k, 0.0, 0.0
    for b, ph in enumerate(tables):
        ph = ph.astype(np.complex128)
        assert len(ph) == c.post_input_size // c.post_decimation and c.post_input_size % c.post_decimation == 0
        K = k0 + np.arange(len(ph))
        dph = float(np.abs(ph - np.exp(1j * np.pi * rate * K)).max())
        assert dph <= (4 * len(ph) + 4 * (b + 1)) * 2.0 ** -23, (tag, freq, b, dph)
        step = np.angle(ph[1:] * np.conj(ph[:-1]) * np.exp(-1j * np.pi * rate))
        worst_tab, worst_step = max(worst_tab, dph), max(worst_step, float(np.abs(step).max()))
        assert np.abs(step).max() <= 4 * 2.0 ** -23, (tag, freq, b, float(np.abs(step).max()))
        k0 += len(ph)
    print("%s, %d Hz: nco_rate %.9g (pi x rate = %.6f rad a step), tables off the model's phase by <= %.3g, steps by <= %.3g rad"
          % (tag, freq, rate, np.pi * rate, worst_tab, worst_step))


def edge_freqs(fs, cf):
    """Both band edges (the upper one's carrier lies beyond +fs/2), a carrier 37 Hz from the centre, two ordinary ones."""
    half = fs // 2
    return [cf - (half - 1), cf - int(0.3137 * fs) - 1440, cf + 37 - 1440, cf + int(0.2411 * fs), cf + half - 1]


def test_filters_250_ksps_five_channels_with_both_band_edges(gpu, oracle):
    """N = 2^15; one padded octet of the operand layout."""
    fs = 250_000
    freqs = edge_freqs(fs, CF)
    fe = gpu.Frontend(fs, CF, freqs)
    assert fe.geometry.fft_size == 1 << 15
    got = [fe.read_tap(F.TAP_FILTER, c) for c in range(len(freqs))]
    fe.close()
    assert D.channel(fs, CF, freqs[-1]).offsetbin > (1 << 14)
    for c, f in enumerate(freqs):
        check_filter("250 ksps ch %d" % c, oracle, fs, CF, f, got[c], SPECTRUM_FLOOR[fs])


def test_filters_2400_ksps_a_full_octet_and_a_padded_one(gpu, oracle):
    """N = 2^19, nine channels: slots 0 .. 7 fill an octet of the operand layout, channel 8 sits alone in a second, padded one."""
    fs = 2_400_000
    freqs = edge_freqs(fs, CF) + [CF + o for o in (-1_000_000, -333_333, 500_500, 1_100_000)]
    fe = gpu.Frontend(fs, CF, freqs)
    assert fe.geometry.fft_size == 1 << 19 and len(freqs) == 9
    got = [fe.read_tap(F.TAP_FILTER, c) for c in range(len(freqs))]
    fe.close()
    for c, f in enumerate(freqs):
        check_filter("2.4 Msps ch %d" % c, oracle, fs, CF, f, got[c], SPECTRUM_FLOOR[fs])


def test_filters_of_two_receivers_come_from_their_own_centres(gpu, oracle):
    """Receivers of 3 and 9 channels at 250 ksps through create_multi; the same channel frequency appears under both centres, and each
    filter is the model's for ITS receiver's centre (so not for the other's: asserted on the model side)."""
    fs = 250_000
    c0, c1 = CF, CF + 90_000
    shared = CF + 50_000                                    # inside both spans: +50 kHz of receiver 0, -40 kHz of receiver 1
    recv = [(c0, [c0 - 124_999, shared, c0 + 124_999]),
            (c1, [c1 - 124_999, shared] + [c1 + o for o in (-100_100, -61_000, -7, 12_345, 55_555, 99_000)] + [c1 + 124_999])]
    fe = gpu.MultiFrontend(fs, recv)
    assert fe.geometry.channels == 12
    got = [fe.read_tap(F.TAP_FILTER, c) for c in range(12)]
    fe.close()
    a, b = model_filter(fs, c0, shared), model_filter(fs, c1, shared)
    assert spectrum_errors(a, b)[0] > 1.0                   # two different filters: a mixed-up centre cannot pass
    c = 0
    for r, (centre, freqs) in enumerate(recv):
        for f in freqs:
            assert fe.freqs[c] == f
            check_filter("receiver %d (centre %d) ch %d" % (r, centre, c), oracle, fs, centre, f, got[c], SPECTRUM_FLOOR[fs])
            c += 1


def test_filters_40_msps_where_the_phase_register_drifts(gpu, oracle):
    """N = 2^23, 1 048 577 taps: create, read the two filters, close; no block is pushed.  One carrier 600 Hz below +fs/2, one 37 Hz
    from the centre: the channels whose register ends 0.040 and 0.056 rad off (oracle/PINNING.md section 7)."""
    fs, cf = 40_000_000, 100_000_000
    freqs = [cf + fs // 2 - 600 - 1440, cf + 37 - 1440]
    t0 = time.time()
    fe = gpu.Frontend(fs, cf, freqs)
    t_create = time.time() - t0
    assert (fe.geometry.fft_size, fe.geometry.taps_length) == (1 << 23, (1 << 20) + 1)
    got = [fe.read_tap(F.TAP_FILTER, c) for c in range(2)]
    fe.close()
    print("40 Msps x 2 channels: create took %.2f s" % t_create)
    for c, f in enumerate(freqs):
        check_filter("40 Msps ch %d" % c, oracle, fs, cf, f, got[c], SPECTRUM_FLOOR[fs])
        # the bare definition is NOT what the device holds: the drift is the reference's arithmetic and is kept
        d = spectrum_errors(got[c], np.fft.fftshift(D.spectrum(D.channel_taps(fs, cf, f)["definition"], 1 << 23)))
        print("40 Msps ch %d against the float64 definition: rel rms %.3g max %.3g" % (c, d[0], d[1]))
        assert d[0] > 100 * SPECTRUM_FLOOR[fs][0]


def noise_blocks(n, count, seed):
    rng = np.random.default_rng(seed)
    return [(0.01 * (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32))).astype(np.complex64) for _ in range(count)]


def test_the_residual_nco_the_device_runs(gpu):
    """Two blocks at 250 ksps: the phasors that multiplied each channel's outputs turn by pi x the model's nco_rate a step."""
    fs = 250_000
    freqs = edge_freqs(fs, CF)
    fe = gpu.Frontend(fs, CF, freqs)
    tables = [[] for _ in freqs]
    for x in noise_blocks(fe.input_size, 2, 1):
        fe.push_block(x)
        fe.sync()
        for c in range(len(freqs)):
            tables[c].append(fe.read_tap(F.TAP_NCO_PHASORS, c))
    fe.close()
    rates = set()
    for c, f in enumerate(freqs):
        check_phasors("250 ksps ch %d" % c, fs, CF, f, tables[c])
        rates.add(D.channel(fs, CF, f).nco_rate32)
    assert len(rates) == len(freqs)                         # five different residuals: none of them can stand in for another


def test_after_a_retune_filter_and_nco_are_the_new_frequencys(gpu, oracle):
    """The geometry of tests/test_gpu_retune.py (250 ksps x 4 channels, channel 1 moves), one pass: two blocks, a retune to an ordinary
    frequency, two blocks, a retune to a frequency whose carrier lies beyond +fs/2, two blocks.  After each retune the filter read for
    channel 1 meets the create-time gate against the model of the NEW frequency, the other channels' words are what they were, and
    channel 1's phasors start again at output 0 with the new residual rate while channel 0's run on."""
    fs = 250_000
    freqs = [9_930_000, 9_958_000, 10_037_000, 10_081_500]
    ch, moves = 1, [10_003_300, CF + fs // 2 - 500]
    assert D.channel(fs, CF, moves[1]).offsetbin > (1 << 14)
    fe = gpu.Frontend(fs, CF, freqs)
    blocks = noise_blocks(fe.input_size, 6, 2)
    created = [fe.read_tap(F.TAP_FILTER, c) for c in range(4)]
    check_filter("at create, ch %d" % ch, oracle, fs, CF, freqs[ch], created[ch], SPECTRUM_FLOOR[fs])
    other, mine = [], [[], [], []]
    for leg in range(3):
        if leg:
            fe.retune(ch, moves[leg - 1])
            fe.sync()
            now = [fe.read_tap(F.TAP_FILTER, c) for c in range(4)]
            check_filter("after retune %d, ch %d" % (leg, ch), oracle, fs, CF, moves[leg - 1], now[ch], SPECTRUM_FLOOR[fs])
            for c in range(4):
                assert (c == ch) != np.array_equal(u32(now[c]), u32(created[c])), (leg, c)
        for x in blocks[2 * leg:2 * leg + 2]:
            fe.push_block(x)
            fe.sync()
            other.append(fe.read_tap(F.TAP_NCO_PHASORS, 0))
            mine[leg].append(fe.read_tap(F.TAP_NCO_PHASORS, ch))
    fe.close()
    check_phasors("ch 0 across both retunes", fs, CF, freqs[0], other)
    for leg, f in enumerate([freqs[ch]] + moves):
        check_phasors("ch %d, leg %d" % (ch, leg), fs, CF, f, mine[leg])


def test_end_to_end_with_nothing_borrowed(gpu, oracle):
    """250 ksps, three channels (within 1 kHz of +fs/2, on a multiple of v, ordinary), two blocks of ddc_f64.make_signal: device and
    oracle chan_out against ddc_f64.ddc_reference fed the model's plan and sharp-form taps (channel_plan_f64) -- for the device with its own
    phasor tables, as tests/test_gpu_channelizer_f64.py does; the tables are bounded against the model's rate above --, gated
    e_gpu <= 4 max(e_ora, floor) with that module's floor for the rate."""
    fs = 250_000
    g = D.geometry(fs)
    freqs = [CF + o - 1440 for o in channel_offsets(fs, g.overlap_length)]
    fe = gpu.Frontend(fs, CF, freqs)
    n = fe.input_size
    assert n == g.input_size
    x = M.make_signal(fs, CF, freqs, freqs, 2 * n, 11, g.decimation, g.pre_decimation)
    for b in range(2):
        fe.push_block(x[b * n:(b + 1) * n])
    fe.sync()
    dev = {}
    read_blocks(fe, 2, 0, list(range(3)), dev)
    fe.close()
    ora = oracle.Frontend(fs, CF, freqs)
    plans = [M.channel_plan_f64(fs, CF, f) for f in freqs]
    assert plans[1][0].offsetbin * fs == (freqs[1] + 1440 - CF) * g.fft_size and plans[1][0].nco_rate == 0
    st = M.Stream(x, plans[0][0])
    bad = []
    for b in range(2):
        ora.push_block(x[b * n:(b + 1) * n])
        for c, (plan, taps) in enumerate(plans):
            got, ph = dev[b][c]
            want_o = ora.channel_view(c)["chan_out"]
            assert len(got) == len(want_o) == len(ph)
            model = M.ddc_reference(st, taps, plan, nco_phasors=[ph], blocks=[b])[0]
            K = b * len(ph) + np.arange(len(ph))
            model_f64 = model / ph.astype(np.complex128) * np.exp(1j * M.nco_phase(plan, K))      # the calibrating side: the float64 phase
            eg, eo = M.errors(got, model), M.errors(want_o, model_f64)
            print("block %d ch %d (%+d Hz): e_gpu rms %.3g max %.3g | e_ora rms %.3g max %.3g" % (b, c, freqs[c] + 1440 - CF, *eg, *eo))
            for i in range(2):
                if not eg[i] <= 4 * max(eo[i], FLOOR[fs][i]):
                    bad.append((b, c, i, eg, eo))
    ora.close()
    assert not bad, bad
