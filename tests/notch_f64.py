"""The adaptive carrier canceller (dumphfdl_amd/csrc/notch.h): a float64 model of the rule, the host build of the
fp32 rule (tests/hostsim/notch_check.cpp) behind two Python functions, and the decode scenario the CPU and GPU tests share."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, D = 32, 24
HIST = D + L - 1
STATE_FLOATS = 2 * L + 2 * HIST
RESET = 4.0
MU = 0.002


def model64(x, mu=MU, taps=L, delay=D, row=None):
    """The rule in float64 on one channel's stream x: (y, sum |w|^2 at the end, resets).  The order of the sums is numpy's: at float64
    it does not matter.  row: samples per row for the reset check (None: one check, at the end)."""
    x = np.asarray(x, np.complex128)
    n = len(x)
    pad = np.concatenate([np.zeros(delay + taps - 1, np.complex128), x])
    w = np.zeros(taps, np.complex128)
    y = np.empty(n, np.complex128)
    resets = 0
    for i in range(n):
        # u_k = x[i - delay - k], k = 0 .. taps - 1: pad[i - delay - k + delay + taps - 1] = pad[i + taps - 1 - k]
        u = pad[i:i + taps][::-1]
        yi = x[i] - np.vdot(w, u)
        P = float(np.sum(u.real * u.real + u.imag * u.imag))
        if 0.0 < P < np.inf and np.isfinite(yi.real) and np.isfinite(yi.imag):
            w = w + (mu / P) * np.conj(yi) * u
        y[i] = yi
        if row and (i + 1) % row == 0:
            E = float(np.sum(np.abs(w) ** 2))
            if not E <= RESET:
                w[:] = 0
                resets += 1
    return y, float(np.sum(np.abs(w) ** 2)), resets


# ---- the host build of notch.h

def build_check(out_dir, sanitize=False):
    """compile tests/hostsim/notch_check.cpp into out_dir; returns the program's path"""
    exe = os.path.join(str(out_dir), "notch_check_san" if sanitize else "notch_check")
    if not os.path.exists(exe):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                              ["-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"), os.path.join(ROOT, "tests", "hostsim", "notch_check.cpp"), "-o", exe])
    return exe


def _records(lines):
    out = []
    for ln in lines:
        f = ln.split()
        if f and f[0] == "rec":
            out.append(dict(blocks=int(f[2]), resets=int(f[3]), in_power=int(f[4], 16), out_power=int(f[5], 16), tap_energy=int(f[6], 16)))
    return out


def host_rows(exe, work, x, mu=MU, state=None):
    """notch.h on rows x [nch][n] complex64 (state [nch][STATE_FLOATS] float32 or None = fresh): (y [nch][n], state after, records)"""
    x = np.ascontiguousarray(x, np.complex64)
    nch, n = x.shape
    work = str(work)
    x.tofile(os.path.join(work, "rows_x.cf32"))
    sin = "-"
    if state is not None:
        sin = os.path.join(work, "rows_state_in.f32")
        np.ascontiguousarray(state, np.float32).tofile(sin)
    out = subprocess.run([exe, "rows", os.path.join(work, "rows_x.cf32"), str(nch), str(n), repr(float(mu)), sin,
                          os.path.join(work, "rows_state.f32"), os.path.join(work, "rows_y.cf32")], capture_output=True, text=True, check=True).stdout
    y = np.fromfile(os.path.join(work, "rows_y.cf32"), np.complex64).reshape(nch, n)
    st = np.fromfile(os.path.join(work, "rows_state.f32"), np.float32).reshape(nch, STATE_FLOATS)
    return y, st, _records(out.split("\n"))


def host_stream(exe, work, x, counts, mu=MU, want_y=True):
    """notch.h on one channel's stream x cut into rows: counts = a row length (the last row shorter) or a list of row lengths.
    Returns (y or None, per-row records -- a list of lengths only --, dict(rows, resets, finite, max_tap_energy, tap_energy))."""
    work = str(work)
    x = np.ascontiguousarray(x, np.complex64)
    x.tofile(os.path.join(work, "stream_x.cf32"))
    if isinstance(counts, (int, np.integer)):
        carg = str(int(counts))
    else:
        carg = os.path.join(work, "stream_counts.i32")
        np.ascontiguousarray(counts, np.int32).tofile(carg)
    ypath = os.path.join(work, "stream_y.cf32") if want_y else "-"
    out = subprocess.run([exe, "stream", os.path.join(work, "stream_x.cf32"), repr(float(mu)), carg, ypath], capture_output=True, text=True, check=True).stdout.split("\n")
    tot = [ln.split() for ln in out if ln.startswith("total")][0]
    summary = dict(rows=int(tot[1]), resets=int(tot[2]), finite=tot[3] == "1", max_tap_energy=float(tot[4]), tap_energy=float(tot[5]))
    return (np.fromfile(ypath, np.complex64) if want_y else None), _records(out), summary


# ---- the decode scenario: six frames under one or two carriers, single-channel baseband

RATES = {5468.75: 350_000, 7812.5: 250_000, 9765.625: 40_000_000, 10781.25: 345_000}      # channel rate -> a sample rate that has it
MODES = (3, 0, 6, 5, 1, 7)
AMP, CFO, SIGMA = 0.05, -11.0, 0.002
TONES = {"clean": (), "one tone": ((430.0, 0.15),), "two tones": ((430.0, 0.15), (-900.0, 0.10))}
BLOCK = 896

_inputs = {}


def scenario(rate):
    """dict(case -> complex64 stream at `rate`, read-only) and the sent octets, computed once per process and rate"""
    if rate not in _inputs:
        import hfdl_synth as synth
        rng = np.random.default_rng(7)
        t, bursts = 0.2, []
        for mode in MODES:
            bursts.append(dict(mode=mode, octets=synth.make_pdu(rng, mode), t0=t, amp=AMP, cfo=CFO))
            t += synth.burst_symbols_len(mode) / 1800 + 0.3
        n = int((t + 0.3) * rate)
        base = synth.synth_channel_baseband(rate, n, bursts, noise_sigma=SIGMA, seed=2)
        cases = {}
        for name, tones in TONES.items():
            x = base.astype(np.complex128)
            for f, a in tones:
                x = x + a * np.exp(2j * np.pi * f * np.arange(n) / rate)
            cases[name] = x.astype(np.complex64)
            cases[name].setflags(write=False)
        _inputs[rate] = (cases, [bytes(b["octets"]) for b in bursts])
    return _inputs[rate]


def decoded(pyoracle, rate, x, sent):
    """how many of the sent PDUs the oracle's demodulator decodes from baseband x at `rate`, fed in blocks of BLOCK samples"""
    fs = RATES[rate]
    ch = pyoracle.Channel(fs, 10_000_000, 10_000_000, want_channelizer=False)
    assert fs / ch.dec == rate
    x = np.ascontiguousarray(x, np.complex64)
    for i in range(0, len(x), BLOCK):
        ch.process_baseband(x[i:i + BLOCK])
    got = [bytes(p["octets"]) for p in ch.pdus]
    ch.close()
    n = 0
    for o in sent:
        for i, g in enumerate(got):
            if g[:len(o)] == o:
                n += 1
                del got[i]
                break
    return n


# ---- the pipeline scenario: three channels at 250 ksps, a carrier inside the middle channel's passband

FS, CF = 250000, 10_000_000
FREQS = [9_958_000, 10_012_000, 10_061_000]
MID = 1
N = 28672                                   # geometry.input_size at 250 ksps
PIPE_NOISE = 0.01
PIPE_AMP = 0.006                            # the six frames of the middle channel
PIPE_TONE = (430.0, 0.02)                   # Hz above the middle channel's carrier, amplitude: 10.5 dB above the frames
PIPE_MODES = (3, 0, 2, 1, 3, 1)             # single-slot frames, 2.34 s each: six of them need 15.6 s

_pipeline = None


def pipeline_scenario():
    """dict(clean, tone: complex64 streams at FS, read-only; sent_mid: the six PDUs of the middle channel; sent_other: one PDU on each
    of the two other channels), computed once per process"""
    global _pipeline
    if _pipeline is None:
        import hfdl_synth as synth
        rng = np.random.default_rng(2025)
        bursts, t = [], 0.15
        for i, mode in enumerate(PIPE_MODES):
            bursts.append(dict(freq=FREQS[MID], mode=mode, octets=synth.make_pdu(rng, mode), t0=t, amp=PIPE_AMP, cfo=(-11.0, 7.0)[i & 1]))
            t += synth.burst_symbols_len(mode) / 1800 + 0.25
        others = [dict(freq=FREQS[0], mode=1, octets=synth.make_pdu(rng, 1), t0=0.4, amp=0.007, cfo=4.0),
                  dict(freq=FREQS[2], mode=3, octets=synth.make_pdu(rng, 3), t0=3.1, amp=0.008, cfo=-6.0)]
        n = (int((t + 0.2) * FS) // N + 1) * N
        clean = synth.synth_wideband(FS, CF, n, bursts + others, noise_sigma=PIPE_NOISE, seed=17)
        f = FREQS[MID] + synth.CARRIER_OFFSET_HZ + PIPE_TONE[0] - CF
        tone = (clean + PIPE_TONE[1] * np.exp(2j * np.pi * f * np.arange(n) / FS)).astype(np.complex64)
        for a in (clean, tone):
            a.setflags(write=False)
        _pipeline = dict(clean=clean, tone=tone, sent_mid=[bytes(b["octets"]) for b in bursts], sent_other=[(b["freq"], bytes(b["octets"])) for b in others])
    return _pipeline


def oracle_pdus(pyoracle, x):
    """[(freq, octets)] the oracle's front end decodes from the wideband stream x, in order"""
    ora = pyoracle.Frontend(FS, CF, FREQS)
    for b in range(len(x) // N):
        ora.push_block(x[b * N:(b + 1) * N])
    out = [(p["freq"], bytes(p["octets"])) for p in ora.pdus]
    ora.close()
    return out


def delivered(octets, sent):
    """how many of the sent PDUs appear among the decoded octets (a decoded PDU may carry padding behind the sent octets)"""
    left = list(octets)
    got = 0
    for o in sent:
        for i, g in enumerate(left):
            if g[:len(o)] == o:
                got += 1
                del left[i]
                break
    return got
