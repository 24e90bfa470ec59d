"""CPU tests: the float64 direct-form model of the channelizer (tests/ddc_f64.py) and the oracle pinned to each other, with no
fitted rotation and no skipped start-up, at twelve sample rates from 12 ksps to 2.4 Msps (1 .. 128 alias rows); the half-rate shift the
reference's arithmetic leaves below 10 800 sps pinned from both sides, and why 12 ksps escapes it; the model's fast path pinned to
its definition; the oracle's single-precision FFT inside the worst-element gate the GPU FFT tests use."""
import numpy as np
import pytest

import ddc_f64 as M
from dumphfdl_amd import frontend as F

CF = 10_000_000

# Oracle against model, default NCO mode (float64 phase), worst over blocks and channels as measured when this test was written
# (oracle/PINNING.md "Channelizer against the float64 direct form"); the gates are 4 x the worst over the set, rounded up to one
# digit.  The figures are relative to the RMS of the model output, whose in-band level lies 60 dB below the alias-frequency tone.
# That input level is why they sit near 1e-4 and not 1e-7: the fp32 rounding of the strong tone (amplitude 1) is 1e-7 of ITS level,
# which is 1e-4 of the 1e-3 in-band level the error is divided by.
MEASURED = {12_000: (1.8e-5, 6.2e-5), 250_000: (6.3e-5, 1.6e-4), 345_599: (5.0e-5, 1.3e-4), 1_000_000: (2.8e-5, 6.8e-5), 2_400_000: (3.6e-5, 1.3e-4),
            # the geometries of 1 .. 8 alias rows, measured when they were added; the gates below were NOT re-derived from them
            # (the worst, 64 000 sps, uses 0.36 of the RMS gate and 0.45 of the worst-element gate)
            16_000: (3.0e-5, 1.2e-4), 24_000: (6.6e-5, 1.9e-4), 48_000: (9.9e-5, 2.5e-4), 64_000: (1.1e-4, 3.2e-4), 86_399: (9.0e-5, 2.6e-4),
            96_000: (6.2e-5, 1.7e-4), 172_799: (6.9e-5, 1.9e-4)}
# the same against the model times (-1)^K (test_half_rate_shift_below_10800_sps); against the unmodified model: 1.41 .. 1.44
MEASURED_HALF_RATE = {5_400: (1.5e-5, 5.9e-5), 8_000: (9.2e-6, 3.8e-5), 10_799: (3.2e-5, 1.3e-4)}
GATE_RMS, GATE_MAX = 3e-4, 7e-4                # 4 x (6.3e-5, 1.53e-4) = (2.5e-4, 6.1e-4) of the first five rates, rounded up to one digit
# (pre_decimation, post_decimation, inverse FFT size) of the rates below 250 ksps: the geometries of 1 .. 8 alias rows
SMALL_GEOMETRY = {5_400: (1, 1, 1024), 8_000: (1, 1, 2048), 10_799: (1, 1, 2048), 12_000: (1, 2, 2048), 16_000: (1, 2, 4096),
                  24_000: (2, 2, 2048), 32_000: (2, 2, 4096), 48_000: (4, 2, 2048), 64_000: (4, 2, 4096), 86_399: (4, 2, 4096),
                  86_400: (8, 2, 2048), 96_000: (8, 2, 2048), 172_799: (8, 2, 4096)}


channel_offsets = M.channel_offsets             # shared with the device tests (tests/ddc_f64.py)


def run_case(oracle, fs, nblk=4, seed=7):
    _, _, g = oracle.geometry(fs)
    offs = channel_offsets(fs, g.overlap_length)
    freqs = [CF + f - 1440 for f in offs]
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    x = M.make_signal(fs, CF, freqs, freqs, nblk * g.input_size, seed, dec, g.pre_decimation)
    fe = oracle.Frontend(fs, CF, freqs)
    got = [[None] * nblk for _ in freqs]
    for b in range(nblk):
        fe.push_block(x[b * g.input_size:(b + 1) * g.input_size])
        for c in range(len(freqs)):
            got[c][b] = fe.channel_view(c)["chan_out"]
    fe.close()
    return g, freqs, x, got


@pytest.mark.parametrize("fs", [12_000, 16_000, 24_000, 48_000, 64_000, 86_399, 96_000, 172_799, 250_000, 345_599, 1_000_000, 2_400_000])
def test_oracle_channelizer_vs_float64_direct_form(oracle, fs):
    """Four blocks of in-band tones + noise + a tone 60 dB up on an alias of each channel's centre + one on the pass-band edge:
    the oracle's chan_out against ddc_reference per block and channel, nothing fitted, block 0 included.  Below 250 ksps these are
    the geometries of 1, 2, 4 and 8 alias rows (pre_decimation), where every row reaches the output."""
    g, freqs, x, got = run_case(oracle, fs)
    assert (g.pre_decimation, g.post_decimation, g.fft_inv_size) == SMALL_GEOMETRY.get(fs, (g.pre_decimation, g.post_decimation, g.fft_inv_size))
    worst = [0.0, 0.0]
    for c, f in enumerate(freqs):
        plan, taps = M.channel_plan(oracle, fs, CF, f)
        assert plan.offsetbin % plan.v == 0
        if c == 1:
            assert plan.offsetbin * fs == (f + 1440 - CF) * plan.fft_size          # exactly on its bin: nothing left to the NCO
        want = M.ddc_reference(x, taps, plan, fast=fs >= 1_000_000)
        for b in range(len(want)):
            assert len(got[c][b]) == len(want[b])
            e = M.errors(got[c][b], want[b])
            print("fs %d ch %d (%+d Hz, offsetbin %d) block %d: rel rms %.3g  worst/rms %.3g" % (fs, c, f + 1440 - CF, plan.offsetbin, b, e[0], e[1]))
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print("fs %d worst: rel rms %.3g  worst/rms %.3g" % (fs, worst[0], worst[1]))
    assert worst[0] <= GATE_RMS and worst[1] <= GATE_MAX, worst


@pytest.mark.parametrize("fs", [5_400, 8_000, 10_799])
def test_half_rate_shift_below_10800_sps(oracle, fs):
    """pre_decimation = post_decimation = 1 (M = N): the reference's bin arithmetic leaves a shift of N / 2 bins, half the channel's
    own sample rate (oracle/PINNING.md section 3 has the derivation), so its chan_out is the model's times (-1)^K, K the absolute
    output index of the stream.  Both sides of that are asserted: with the factor the oracle is inside the gates of every other rate,
    and against the unmodified model it is off by more than the model's own RMS -- a `corrected` oracle fails here, not silently."""
    g, freqs, x, got = run_case(oracle, fs)
    assert (g.pre_decimation, g.post_decimation, g.fft_inv_size) == SMALL_GEOMETRY[fs] and g.fft_inv_size == g.fft_size
    P = g.post_input_size
    worst, plain = [0.0, 0.0], 10.0
    for c, f in enumerate(freqs):
        plan, taps = M.channel_plan(oracle, fs, CF, f)
        want = M.ddc_reference(x, taps, plan)
        for b in range(len(want)):
            assert len(got[c][b]) == len(want[b]) == P
            e = M.errors(got[c][b], want[b] * M.half_rate_sign(b * P + np.arange(P)))
            e0 = M.errors(got[c][b], want[b])
            print("fs %d ch %d block %d: with (-1)^K rel rms %.3g  worst/rms %.3g | unmodified model rel rms %.3g" % (fs, c, b, e[0], e[1], e0[0]))
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
            plain = min(plain, e0[0])
    print("fs %d worst with (-1)^K: rel rms %.3g  worst/rms %.3g; best against the unmodified model: %.3g" % (fs, worst[0], worst[1], plain))
    assert worst[0] <= GATE_RMS and worst[1] <= GATE_MAX, worst
    assert plain > 1.0, plain


def test_why_12000_sps_escapes_the_half_rate_shift(oracle):
    """12 000 - 21 599 sps have pre_decimation 1 as well, and the same N / 2 bins are left over before the decimator; but
    post_decimation is 2 and post_input_size even, so the decimator starts every block at sample 0 (the oracle's decimation_remain
    is 0 after every block) and keeps the even samples g = 2 K of the stream, where (-1)^g = 1."""
    fs = 12_000
    _, _, g = oracle.geometry(fs)
    assert (g.pre_decimation, g.post_decimation) == (1, 2) and g.fft_inv_size == g.fft_size and g.post_input_size % 2 == 0
    freqs = [CF + f - 1440 for f in channel_offsets(fs, g.overlap_length)]
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    x = M.make_signal(fs, CF, freqs, freqs, 5 * g.input_size, 7, dec, g.pre_decimation)
    fe = oracle.Frontend(fs, CF, freqs)
    for b in range(5):
        fe.push_block(x[b * g.input_size:(b + 1) * g.input_size])
        for c in range(len(freqs)):
            remain, _, n_out = fe.channel_nco(c)
            assert (remain, n_out) == (0, g.post_input_size // 2), (b, c, remain, n_out)
        kept = b * g.post_input_size + np.arange(0, g.post_input_size, 2)       # stream indices the decimator keeps of block b
        assert np.all(M.half_rate_sign(kept) == 1.0)
    fe.close()


def test_model_fast_path_is_the_definition(oracle):
    """ddc_reference(fast=True) (the aliased short inverse transform) against fast=False (the whole linear convolution, then every
    pre-th sample): float64 rounding apart, the same numbers."""
    for fs in (250_000, 345_599):
        g, freqs, x, _ = run_case(oracle, fs, nblk=2)
        for f in freqs:
            plan, taps = M.channel_plan(oracle, fs, CF, f)
            a = M.ddc_reference(x, taps, plan)
            b = M.ddc_reference(x, taps, plan, fast=True)
            for u, v in zip(a, b):
                assert M.errors(v, u)[1] < 1e-12


@pytest.mark.parametrize("fs", [250_000, 2_400_000])
def test_every_alias_row_is_excited_as_far_as_its_taps_reach(oracle, fs):
    """What the channelizer comparisons can and cannot see.  make_signal puts wide-band noise 60 dB above the in-band level into
    EVERY alias row of a channel's filter; one block of the model with one of the `pre` slices of the filtered spectrum left out
    then moves the output by what the filter lets through of that slice; every slice holds its share of the input (asserted).
    How far that is visible is the filter's own depth: the Hamming-window stop band of the
    fp32 taps lies 108 .. 168 dB down at 2.4 Msps, below anything an fp32 evaluation resolves beside the pass band (2^-24 = -144 dB),
    so there only the rows next to the pass band exceed the gates (printed); at 250 ksps (16 rows) the lightest row moves the
    output by 7e-5 of its RMS.  A misreading of a far row is therefore invisible to ANY fp32 comparison of outputs, the product's
    own included; what pins those rows is the bit-exact comparison of the taps (test_tap_design_matches_oracle_bit_for_bit) and of
    the fold's partial sums between kernels."""
    g, freqs, x, _ = run_case(oracle, fs, nblk=2)
    pre = g.pre_decimation
    seen = []
    for f in freqs:
        plan, taps = M.channel_plan(oracle, fs, CF, f)
        st = M.Stream(x, plan)
        X, H = st.spectrum(1).reshape(pre, st.L // pre), M.taps_spectrum(taps, st.L).reshape(pre, st.L // pre)
        cut = slice(plan.scrap, plan.scrap + plan.post_input_size)
        rms = np.sqrt(np.mean(np.abs(np.fft.ifft((X * H).sum(axis=0))[cut]) ** 2))
        w = np.array([np.sqrt(np.mean(np.abs(np.fft.ifft(X[r] * H[r])[cut]) ** 2)) for r in range(pre)]) / rms
        far = np.mean(np.abs(H) ** 2, axis=1) < 1e-6                  # slices without pass band or skirt
        assert far.sum() >= pre - 4 and np.all(np.mean(np.abs(X[far]) ** 2, axis=1) > 0.1 * np.mean(np.abs(X) ** 2))      # input in every one
        seen.append((int((w > GATE_RMS).sum()), float(w.min())))
    print("fs %d: slices whose loss exceeds the RMS gate, lightest slice / output RMS, per channel (of %d):" % (fs, pre), seen)
    # the coverage oracle/PINNING.md section 3 quotes: rows whose loss exceeds the RMS gate, and the lightest row
    assert all(n >= (7 if fs == 250_000 else 3) for n, _ in seen), seen
    assert all(w >= (6e-5 if fs == 250_000 else 1e-7) for _, w in seen), seen


def test_model_is_a_plain_convolution():
    """The model against direct dot products sum_t h[t] x[n - t] on a toy plan (no FFT anywhere on the reference side)."""
    class Plan:
        fft_size, overlap_length, input_size, pre_decimation, post_decimation = 64, 16, 48, 4, 2
        scrap, post_input_size, offsetbin, nco_rate, v = 4, 12, 8, np.float32(0.0371), 4
    rng = np.random.default_rng(1)
    x = rng.standard_normal(3 * 48) + 1j * rng.standard_normal(3 * 48)
    h = rng.standard_normal(17) + 1j * rng.standard_normal(17)
    outs = M.ddc_reference(x, h, Plan)
    K = 0
    for k in range(3):
        for j in range(0, 12, 2):
            n = k * 48 - 16 + 4 * (4 + j)
            y = sum(h[t] * x[n - t] for t in range(17) if n - t >= 0)
            want = y * np.exp(-2j * np.pi * 8 * n / 64) * np.exp(1j * np.pi * float(np.float32(0.0371)) * K)
            assert abs(outs[k][j // 2] - want) < 1e-12
            K += 1


@pytest.mark.parametrize("n", [512, 4096, 1 << 15, 1 << 18, 1 << 21])
def test_oracle_fft_worst_element(oracle, n):
    """A single-precision transform known to be good stays inside the worst-element gate of the GPU FFT tests:
    max |err| <= 10 x (RMS gate 2e-6) x rms(want)."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    want = np.fft.fft(x.astype(np.complex128))
    err = np.abs(oracle.fft(x, -1).astype(np.complex128) - want)
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    print("n %d: rel rms %.3g  worst/rms %.3g" % (n, np.sqrt(np.mean(err ** 2)) / rms, err.max() / rms))
    assert np.sqrt(np.mean(err ** 2)) < 2e-6 * rms
    assert err.max() <= 10 * 2e-6 * rms


def test_80_msps_plans_the_largest_transform():
    """No device needed (the built libhfdl_gpu.so is: build() first, like the other host-library CPU tests): a receiver above 65.536 Msps plans N = 2^24 (the only size whose third FFT pass is the radix-16 one) and an
    inverse transform the front end accepts (16 <= M <= 8192)."""
    from oracle import pyoracle
    dec, tbw, d = pyoracle.geometry(80_000_000)
    g = F.plan_geometry(dec, tbw)
    assert (dec, g.fft_size, g.fft_inv_size, g.pre_decimation, g.taps_length) == (8192, 1 << 24, 4096, 4096, (1 << 21) + 1)
    assert (d.fft_size, d.fft_inv_size, d.taps_length) == (g.fft_size, g.fft_inv_size, g.taps_length)
