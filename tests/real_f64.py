"""Real-sampled input in float64, written from the definition (numpy only; a helper module, not a test).  DESIGN.md section 4.16.

A real front end is planned as the equivalent complex stream of half the rate: fs' = fs_r / 2 centred on base + fs_r / 4, with
N', overlap', input_size', pre, post, M, scrap, offsetbin and the NCO of plan_block(fs').  Block k is the 2 N' real samples
x[2 (k input_size' - overlap') ..] (zeros before the stream begins), and the device computes, per block,

    X[b]  = sum_n x_k[n] exp(-2 pi i b n / 2N'),  b = 0 .. N' - 1      the block's real transform on its non-negative frequencies
    H[b]  = (1/2) sum_t h[t] exp(-2 pi i b t / 2N')                    h: the 2 overlap' + 1 taps designed at the real rate
    y[i]  = (1/N') sum_b H[b] X[b] exp(+2 pi i (b + N'/2) i / N')      the slot holds X in natural order, which the rest of the
                                                                       pipeline reads as the fftshifted order of the equivalent stream

and from there on exactly what tests/ddc_f64.py states for a complex stream: z_k[j] = y[i] exp(-2 pi i offsetbin n / N') at
i = pre (scrap + j), n = k input_size' - overlap' + i, every post-th sample kept and multiplied by the NCO phasor.  That is the
BLOCKWISE definition (real_ddc_reference): y is (h * x_a) / 2 sampled at every second real sample and multiplied by (-1)^i, with x_a
the analytic signal of the BLOCK -- the half-plane projection is circular per block.  global_reference() is the same convolution
on the whole record's analytic signal (or on x itself: the full direct form, images included); the CPU test reports the gap."""
import os
import subprocess

import numpy as np

import ddc_f64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the two identities

def untangle(Z):
    """X[k], k = 0 .. N' - 1, of the 2N'-point DFT of the real block whose pairs z[n] = x[2n] + j x[2n + 1] have the DFT Z."""
    Z = np.asarray(Z, np.complex128)
    n = len(Z)
    k = np.arange(n)
    zm = np.conj(Z[(n - k) % n])
    w = np.exp(-1j * np.pi * k / n)
    return 0.5 * ((Z + zm) - 1j * w * (Z - zm))


def tap_combine(h, n):
    """FFT_N'(h_even) + W^k FFT_N'(h_odd): the 2N'-point transform of the taps h on bins 0 .. N' - 1 (without the stored 1/2)."""
    h = np.asarray(h, np.complex128)
    e, o = np.zeros(n, np.complex128), np.zeros(n, np.complex128)
    e[:len(h[0::2])] = h[0::2]
    o[:len(h[1::2])] = h[1::2]
    return np.fft.fft(e) + np.exp(-1j * np.pi * np.arange(n) / n) * np.fft.fft(o)


def window(x, k, plan):
    """[history | block] of block k: 2 N' real samples, zeros before the stream begins."""
    n, ov, ins = int(plan.fft_size), int(plan.overlap_length), int(plan.input_size)
    lo = 2 * (k * ins - ov)
    w = np.zeros(2 * n, np.float64)
    a = max(lo, 0)
    w[a - lo:] = x[a:lo + 2 * n]
    return w


def block_spectrum(x, k, plan):
    """bins 0 .. N' - 1 of numpy.fft.rfft of block k's window: what HFDL_GPU_TAP_SPECTRUM returns"""
    return np.fft.rfft(window(x, k, plan))[:int(plan.fft_size)]


def stored_filter(taps, plan):
    """what HFDL_GPU_TAP_FILTER returns: the zero-padded 2N' transform of the real-rate taps on bins 0 .. N' - 1, halved"""
    n = int(plan.fft_size)
    h = np.zeros(2 * n, np.complex128)
    h[:len(taps)] = taps
    return 0.5 * np.fft.fft(h)[:n]


# ---------------------------------------------------------------- the blockwise definition

def real_ddc_reference(x, taps, plan, nco_phasors=None, blocks=None, fast=False, taps_fft=None):
    """Per-block channelizer outputs (complex128 arrays) of the REAL stream x (whole blocks of 2 input_size' samples) through the channel
    whose real-rate taps are `taps` and whose planner record (of the equivalent stream) is `plan`; modelled on ddc_f64.ddc_reference.
    fast: the same numbers from a size-M inverse transform of the folded rows.  taps_fft: stored_filter(taps, plan) computed before."""
    x = np.asarray(x, np.float64)
    n, ov, ins = int(plan.fft_size), int(plan.overlap_length), int(plan.input_size)
    pre, post, scrap, P, off = int(plan.pre_decimation), int(plan.post_decimation), int(plan.scrap), int(plan.post_input_size), int(plan.offsetbin)
    assert len(x) % (2 * ins) == 0 and len(taps) == 2 * ov + 1 and pre * scrap == ov
    H = stored_filter(taps, plan) if taps_fft is None else taps_fft
    outs = []
    for k in (range(len(x) // (2 * ins)) if blocks is None else blocks):
        prod = np.fft.ifftshift(H * block_spectrum(x, k, plan))       # slot order (natural) -> the unshifted order the inverse transform sums in
        i = pre * (scrap + np.arange(P, dtype=np.int64))
        if fast:
            y = np.fft.ifft(prod.reshape(pre, n // pre).sum(axis=0))[scrap:scrap + P] / pre
        else:
            y = np.fft.ifft(prod)[i]
        nn = k * ins - ov + i
        z = y * np.exp(-2j * np.pi * ((off * nn) % n) / n)
        g = k * P + np.arange(P, dtype=np.int64)
        keep = (g % post) == 0
        K = g[keep] // post
        ph = np.exp(1j * M.nco_phase(plan, K)) if nco_phasors is None else np.asarray(nco_phasors[len(outs)], np.complex128)
        assert len(ph) == len(K)
        outs.append(z[keep] * ph)
    return outs


def analytic(x):
    """the whole record's analytic signal, float64"""
    x = np.asarray(x, np.float64)
    n = len(x)
    X = np.fft.fft(x)
    X[1:n // 2] *= 2
    X[n // 2 + 1:] = 0
    return np.fft.ifft(X)


def global_reference(x, taps, plan, blocks, images=False):
    """The same outputs from ONE linear convolution over the whole record: (h * x_a) / 2 with x_a the record's analytic signal, or, with
    images, h * x itself -- the full direct form.  Default NCO phase."""
    n, ov, ins = int(plan.fft_size), int(plan.overlap_length), int(plan.input_size)
    pre, post, scrap, P, off = int(plan.pre_decimation), int(plan.post_decimation), int(plan.scrap), int(plan.post_input_size), int(plan.offsetbin)
    src = np.asarray(x, np.float64).astype(np.complex128) if images else 0.5 * analytic(x)
    L = M._pow2_at_least(len(src) + len(taps))
    y = np.fft.ifft(np.fft.fft(src, L) * np.fft.fft(np.asarray(taps, np.complex128), L))
    outs = []
    for k in blocks:
        nn = k * ins - ov + pre * (scrap + np.arange(P, dtype=np.int64))         # equivalent-stream index; the real sample is 2 nn
        z = y[2 * nn] * (1.0 - 2.0 * (nn & 1)) * np.exp(-2j * np.pi * ((off * nn) % n) / n)
        g = k * P + np.arange(P, dtype=np.int64)
        keep = (g % post) == 0
        outs.append(z[keep] * np.exp(1j * M.nco_phase(plan, g[keep] // post)))
    return outs


# ---------------------------------------------------------------- streams

def real_from_equiv(w):
    """2 Re(w_up j^n): the real stream whose equivalent complex stream is w -- w upsampled by two through a zero-padded whole-record
    float64 spectrum and moved up by a quarter of the real rate.  float64, 2 len(w) samples."""
    w = np.asarray(w, np.complex128)
    n = len(w)
    W = np.fft.fft(w)
    U = np.zeros(2 * n, np.complex128)
    U[:n // 2] = W[:n // 2]
    U[2 * n - (n - n // 2):] = W[n // 2:]
    up = np.fft.ifft(U) * 2
    return 2 * np.real(up * (1j ** (np.arange(2 * n) % 4)))


def equiv_from_real(x):
    """The equivalent complex stream of a real record: half its analytic signal (x = Re x_a carries each component at half its
    amplitude; the device's factor 1/2), every second sample, times (-1)^m.  complex128; real_from_equiv's inverse."""
    a = 0.5 * analytic(x)[0::2]
    return a * (1.0 - 2.0 * (np.arange(len(a)) & 1))


def as_rs16(x, scale):
    """int16 samples of x * scale (rounded, |.| <= 32767) and the float64 values the device's conversion makes of them ((float)v / 32767.5f)"""
    v = np.clip(np.rint(np.asarray(x, np.float64) * scale * 32767.5), -32767, 32767).astype(np.int16)
    return v, (v.astype(np.float32) / np.float32(32767.5)).astype(np.float64)


# ---------------------------------------------------------------- plans and taps: the oracle's planner, the host build of real_input.h

def equiv(fs_r, base):
    return fs_r // 2, base + fs_r // 4


def shift32(fs_r, base, freq):
    """real_input.h real_shift in numpy fp32"""
    return np.float32(2 * (base - (freq + 1440)) + fs_r // 2) / np.float32(fs_r)


def band32(fs_r, base, freq, dec):
    c, hb = np.float32(freq + 1440 - base) / np.float32(fs_r), np.float32(0.25) / np.float32(dec)
    return np.float32(c - hb), np.float32(c + hb)


def channel_plan(oracle, fs_r, base, freq):
    """(planner record of the equivalent stream, real-rate taps as complex128) with the oracle's planner and tap design"""
    L = oracle.lib()
    fs = fs_r // 2
    dec, tbw = L.orc_compute_fft_decimation_rate(fs, 5400), L.orc_transition_bw(fs, 250)
    d = oracle.fastddc_init(tbw, dec, float(shift32(fs_r, base, freq)))
    lo, hi = band32(fs_r, base, freq, dec)
    taps = np.zeros(2 * d.taps_length - 1, np.complex64)
    L.orc_firdes_bandpass_c(taps.ctypes.data, len(taps), float(lo), float(hi))
    return d, taps.astype(np.complex128)


def channel_freqs(fs_r, base, overlap_eq):
    """Three channels as ddc_f64.channel_offsets picks them on the equivalent stream (upper edge, on a multiple of v, ordinary) and a
    fourth within 3 kHz of `base`, where the mirror image is adjacent"""
    fs, centre = equiv(fs_r, base)
    return [centre + o - 1440 for o in M.channel_offsets(fs, overlap_eq)] + [base + 2500 - 1440]


def build_host_check(directory, sanitize=False):
    exe = os.path.join(str(directory), "real_input_check" + ("_san" if sanitize else ""))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) +
                          ["-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"), os.path.join(ROOT, "tests", "hostsim", "real_input_check.cpp"), "-o", exe])
    return exe


PLAN_FIELDS = ("fs", "centre", "dec", "tbw", "shift", "n", "overlap", "input_size", "pre", "post", "m", "scrap", "post_input_size", "taps_length", "offsetbin", "taps_real",
               "lowcut", "highcut", "sindelta", "cosdelta", "rate")
PLAN_FLOATS = ("tbw", "shift", "lowcut", "highcut", "sindelta", "cosdelta", "rate")


def host_plan(exe, fs_r, base, freq):
    out = subprocess.run([exe, "plan", str(fs_r), str(base), str(freq)], capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(PLAN_FIELDS)
    return {k: (np.array([int(v, 16)], np.uint32).view(np.float32)[0] if k in PLAN_FLOATS else int(v)) for k, v in zip(PLAN_FIELDS, out)}


def host_taps(exe, directory, fs_r, base, freq):
    """(the L_r real-rate taps, the 2 T words of the even / odd split) of the host build, complex64"""
    path = os.path.join(str(directory), "taps_%d_%d_%d.bin" % (fs_r, base, freq))
    subprocess.check_call([exe, "taps", str(fs_r), str(base), str(freq), path])
    a = np.fromfile(path, np.complex64)
    T = (len(a) + 1) // 4
    return a[:2 * T - 1], a[2 * T - 1:]


# ---------------------------------------------------------------- the decode scene

def decode_scene(oracle):
    """hfdl_synth traffic at (fs' = 250 ksps, centre' = base + fs_r / 4) for fs_r = 500 ksps, base = 5 MHz: three channels, about 6 s, two
    frames each, amplitude 0.05 over noise of sigma 0.004 per component (the smoke run's levels); cut to whole blocks.  w: the complex stream; v16: the real stream
    2 Re(w_up j^n) as RS16; want: the oracle's PDUs on the complex stream, sorted (freq, mode, octets); sent: the bursts."""
    import hfdl_synth as synth
    fs_r, base = 500_000, 5_000_000
    fs, centre = equiv(fs_r, base)
    freqs = [centre - 42_000, centre + 26_000, centre + 83_000]
    _, _, d0 = oracle.geometry(fs)
    rng = np.random.default_rng(77)
    bursts = []
    for i, f in enumerate(freqs):
        for k in range(2):
            mode = int(rng.integers(0, 4))
            bursts.append(dict(freq=f, mode=mode, octets=synth.make_pdu(rng, mode), t0=0.2 + 0.15 * i + 2.9 * k, amp=0.05, cfo=float(rng.uniform(-8, 8))))
    w = synth.synth_wideband(fs, centre, int(6.0 * fs), bursts, noise_sigma=0.004, seed=77)
    nblk = len(w) // d0.input_size
    w = w[:nblk * d0.input_size]
    v16, _ = as_rs16(real_from_equiv(w), 1.0)
    assert np.abs(v16).max() < 32767
    ora = oracle.Frontend(fs, centre, freqs)
    for b in range(nblk):
        ora.push_block(w[b * d0.input_size:(b + 1) * d0.input_size])
    want = sorted((p["freq"], p["mode"], p["octets"]) for p in ora.pdus)
    ora.close()
    return dict(fs_r=fs_r, base=base, fs=fs, centre=centre, freqs=freqs, nblk=nblk, n=d0.input_size, w=w, v16=v16, want=want, sent=bursts)
