"""GPU tests: real-sampled input (hfdl_gpu_frontend_create_real) against float64 (tests/real_f64.py).

Three geometries, the smallest of each class of code path: 96 ksps (equivalent stream 48 ksps: plain tap layout, plain-VALU fold),
500 ksps (250 ksps: N' = 2^15, LDS FFT passes, octet layout, matrix-pipe fold) and 2.8 Msps (1.4 Msps: N' = 2^18, register-resident
passes).  Four channels each: the three ddc_f64.channel_offsets picks on the equivalent stream (within 1 kHz of the upper edge, on a
multiple of v, ordinary) and one within 3 kHz of `base`, where the mirror image is adjacent.  The signal is ddc_f64.make_signal's level
scheme (interferers 60 dB up) on the equivalent stream, made real by real_f64.real_from_equiv.

  spectrum    HFDL_GPU_TAP_SPECTRUM against numpy.fft.rfft of [history | block], bins 0 .. N' - 1: relative RMS 3e-6, worst element 10 x
              that -- the forward-FFT tests' gates; block 0 (zero history) and a middle block, RS16 and RF32
  taps        HFDL_GPU_TAP_FILTER against the float64 transform of the host-designed real-rate taps, the same gates
  channelizer tap 3 per (block, channel) against real_ddc_reference fed the device's own phasor tables (tap 9):
              e_real <= 4 max(e_cal, floor), e_cal = the oracle's error against ddc_reference on the equivalent complex stream of the
              same input (real_f64.equiv_from_real, cast to cf32), floor = tests/test_gpu_channelizer_f64.py FLOOR[fs'] where there is
              one, else the oracle-against-model figure measured the same way and pinned here
and, as comparisons of words: push shape, two receivers against one each, retune against a fresh create; the blanker on pairs, the
refusals, the monitor's bands; the decode end to end."""
import ctypes as C

import numpy as np
import pytest

import ddc_f64 as M
import real_f64 as R
import spectrum_f64 as S
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

SPEC_RMS = 3e-6
# tests/test_gpu_channelizer_f64.py FLOOR[fs'] where it has one; 1.4 Msps has none: the oracle against ddc_reference on the equivalent complex
# stream of this file's input, measured once and written into DESIGN.md section 4.16 -- pinned, so the gate does not move with the run
FLOOR = {48_000: (9.9e-5, 2.5e-4), 250_000: (6.3e-5, 1.6e-4), 1_400_000: (1.9e-5, 5.9e-5)}
GEOS = {96_000: dict(base=0, nblk=6, n=1 << 13, layout="plain"), 500_000: dict(base=5_000_000, nblk=5, n=1 << 15, layout="octet"),
        2_800_000: dict(base=0, nblk=4, n=1 << 18, layout="octet")}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def spectrum_errors(got, want):
    err = np.abs(got.astype(np.complex128) - want)
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    return float(np.sqrt(np.mean(err ** 2)) / rms), float(err.max() / rms)


def make_stream(oracle, fs_r, base, freqs, nblk, seed):
    """(x float32 real stream of nblk blocks, the int16 stream of x / 32 and the float64 values the device makes of it)"""
    fs, centre = R.equiv(fs_r, base)
    dec, _, d0 = oracle.geometry(fs)
    w = M.make_signal(fs, centre, freqs, freqs, nblk * d0.input_size, seed, dec, d0.pre_decimation)
    x = R.real_from_equiv(w).astype(np.float32)
    v16, x16 = R.as_rs16(x, 1.0 / 32)
    assert np.abs(v16).max() < 32767
    return x, v16, x16


@pytest.fixture(scope="module", params=sorted(GEOS))
def run(request, gpu, oracle):
    """One front end per geometry, blocks pushed one by one with a sync after each (RF32; blocks 0 and `mid` once more as RS16 on a second
    front end for the spectrum alone): spectra of block 0 and a middle block, tap 3 and tap 9 of every block and channel, the filters."""
    fs_r = request.param
    geo = GEOS[fs_r]
    base, nblk = geo["base"], geo["nblk"]
    fs, centre = R.equiv(fs_r, base)
    _, _, d0 = oracle.geometry(fs)
    freqs = R.channel_freqs(fs_r, base, d0.overlap_length)
    x, v16, x16 = make_stream(oracle, fs_r, base, freqs, nblk, 1000 + fs_r // 1000)
    fe = gpu.RealFrontend(fs_r, [(base, freqs)])
    g = fe.geometry
    assert (g.sample_rate, g.fft_size, g.input_size) == (fs, geo["n"], d0.input_size) and fe.real_input() == (True, fs_r) and fe.receiver_of(0) == (0, centre)
    assert (g.pre_decimation % 8 == 0 and g.fft_inv_size % 16 == 0) == (geo["layout"] == "octet")
    nb, mid = fe.real_block, nblk // 2
    spec, chan = {}, {}
    for b in range(nblk):
        fe.push_real([x[b * nb:(b + 1) * nb]], F.SFMT_RF32)
        fe.sync()
        if b in (0, mid):
            spec["rf32", b] = fe.read_tap(F.TAP_SPECTRUM)
        chan[b] = [(fe.read_tap(F.TAP_CHAN_OUT, c), fe.read_tap(F.TAP_NCO_PHASORS, c)) for c in range(len(freqs))]
    filters = [fe.read_tap(F.TAP_FILTER, c) for c in range(len(freqs))]
    fe.close()
    fe = gpu.RealFrontend(fs_r, [(base, freqs)])
    for b in range(mid + 1):
        fe.push_real([v16[b * nb:(b + 1) * nb]], F.SFMT_RS16)
        if b in (0, mid):
            spec["rs16", b] = fe.read_tap(F.TAP_SPECTRUM)
    fe.close()
    return dict(fs_r=fs_r, base=base, fs=fs, centre=centre, freqs=freqs, nblk=nblk, mid=mid, plan=d0, x=x.astype(np.float64), x16=x16, spec=spec, chan=chan, filters=filters)


def test_spectrum_against_rfft(run):
    for (fmt, b), got in sorted(run["spec"].items()):
        want = R.block_spectrum(run["x"] if fmt == "rf32" else run["x16"], b, run["plan"])
        assert len(got) == len(want) == run["plan"].fft_size
        e = spectrum_errors(got, want)
        print("fs_r %d %s block %d: spectrum rel rms %.3g worst/rms %.3g" % (run["fs_r"], fmt, b, e[0], e[1]))
        assert e[0] <= SPEC_RMS and e[1] <= 10 * SPEC_RMS, (run["fs_r"], fmt, b, e)


def test_filter_taps_against_float64(run, oracle):
    for c, f in enumerate(run["freqs"]):
        plan, taps = R.channel_plan(oracle, run["fs_r"], run["base"], f)
        e = spectrum_errors(run["filters"][c], R.stored_filter(taps, plan))
        print("fs_r %d channel %d (%d Hz): filter rel rms %.3g worst/rms %.3g" % (run["fs_r"], c, f, e[0], e[1]))
        assert e[0] <= SPEC_RMS and e[1] <= 10 * SPEC_RMS, (run["fs_r"], c, e)


def test_channelizer_against_the_blockwise_definition(run, oracle):
    fs_r, base, fs, centre, freqs, x = (run[k] for k in ("fs_r", "base", "fs", "centre", "freqs", "x"))
    plans = [R.channel_plan(oracle, fs_r, base, f) for f in freqs]
    H = [R.stored_filter(t, p) for p, t in plans]
    # the calibrating side: the oracle on the equivalent complex stream against ddc_reference, float64 phase
    weq = R.equiv_from_real(x).astype(np.complex64)
    cplans = [M.channel_plan(oracle, fs, centre, f) for f in freqs]
    st = M.Stream(weq, cplans[0][0])
    Hc = [M.taps_spectrum(t, st.L) for _, t in cplans]
    ora = oracle.Frontend(fs, centre, freqs)
    n = st.input_size
    rows = []
    for b in range(run["nblk"]):
        ora.push_block(weq[b * n:(b + 1) * n])
        for c in range(len(freqs)):
            got, ph = run["chan"][b][c]
            want_o = ora.channel_view(c)["chan_out"]
            assert len(got) == len(ph) == len(want_o)
            model = R.real_ddc_reference(x, plans[c][1], plans[c][0], nco_phasors=[ph], blocks=[b], fast=True, taps_fft=H[c])[0]
            cal = M.ddc_reference(st, cplans[c][1], cplans[c][0], blocks=[b], fast=True, taps_fft=Hc[c])[0]
            rows.append((b, c, M.errors(got, model), M.errors(want_o, cal)))
        st.forget(b)
    ora.close()
    worst_cal = tuple(max(r[3][i] for r in rows) for i in range(2))
    floor = FLOOR[fs]
    bad = []
    for b, c, eg, ec in rows:
        print("fs_r %d block %d channel %d: e_real rms %.3g max %.3g | e_cal rms %.3g max %.3g" % (fs_r, b, c, eg[0], eg[1], ec[0], ec[1]))
        if not all(eg[i] <= 4 * max(ec[i], floor[i]) for i in range(2)):
            bad.append((b, c, eg, ec))
    print("fs_r %d: floor rms %.3g max %.3g (worst e_cal of the run: rms %.3g max %.3g)" % ((fs_r,) + tuple(floor) + worst_cal))
    assert not bad, (fs_r, bad)


# ---------------------------------------------------------------- comparisons of words

def export_all(fe, nblk):
    samples, counts, _, _, blocks, _ = fe.export_read(0, wait=True)
    assert blocks == list(range(nblk)), blocks
    return u32(samples).copy(), counts.copy()


def pdu_key(p):
    return (p["freq"], p["mode"], p["octets"], p["fcs_status"])


@pytest.fixture(scope="module")
def scene(gpu, oracle):
    """real_f64.decode_scene: hfdl_synth traffic at (fs' = 250 ksps, centre'), three channels, about 6 s, six frames, as RS16.  That the
    oracle decodes 6 of 6 on the complex stream is a condition on the input, asserted by tests/test_real_input_cpu.py."""
    return R.decode_scene(oracle)


def test_end_to_end_decode_equals_the_oracle_and_the_complex_front_end(gpu, scene):
    s = scene
    fe = gpu.Frontend(s["fs"], s["centre"], s["freqs"])
    for b in range(s["nblk"]):
        fe.push_block(s["w"][b * s["n"]:(b + 1) * s["n"]])
    got_c = sorted(pdu_key(p) for p in fe.poll_pdus())
    fe.close()
    assert [k[:3] for k in got_c] == s["want"]
    fe = gpu.RealFrontend(s["fs_r"], [(s["base"], s["freqs"])])
    nb = fe.real_block
    for b in range(s["nblk"]):
        fe.push_real([s["v16"][b * nb:(b + 1) * nb]], F.SFMT_RS16)
    got_r = sorted(pdu_key(p) for p in fe.poll_pdus())
    fe.close()
    assert got_r == got_c, (len(got_r), len(got_c))             # (frequency, mode, octets, header FCS status), as a multiset


def test_replay_real_input_gives_the_same_pdus(gpu, scene, tmp_path):
    """the same RS16 file through hfdl_replay --real-input=BASE_KHZ: the PDUs the oracle decodes on the complex stream"""
    import os
    import re
    import subprocess
    s = scene
    path = tmp_path / "real.cs16"
    s["v16"].tofile(path)
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dumphfdl_amd", "hfdl_replay")
    cmd = [exe, "--iq-file", str(path), "--sample-rate", str(s["fs_r"]), "--sample-format", "CS16", "--real-input=%d" % (s["base"] // 1000)] + ["%.3f" % (f / 1e3) for f in s["freqs"]]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = sorted((int(re.search(r"freq=(-?\d+)", l).group(1)), l.split()[-1]) for l in out.stdout.splitlines() if l.startswith("PDU "))
    assert got == sorted((f, o.hex()) for f, _, o in s["want"]), out.stderr


def test_push_shape_changes_nothing(gpu, scene, monkeypatch):
    """The same stream block by block with a poll after each, in one batch (halves of four blocks: they fill and close on the way), and
    from device memory: channelizer output of every block (the export's words) and PDUs equal, word for word."""
    s = scene
    nblk = s["nblk"]
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "4")
    monkeypatch.setenv("HFDL_GPU_DEMOD_BATCH", "4")
    # the stream in device memory, by the HIP runtime the library itself runs on (loaded with it, RTLD_GLOBAL): no second framework
    # has to start up for one buffer
    hip = C.CDLL(None)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    src = np.ascontiguousarray(s["v16"][:nblk * 2 * s["n"]])
    dev = C.c_void_p()
    gpu.RealFrontend(s["fs_r"], [(s["base"], s["freqs"])]).close()          # (the device is selected)
    assert hip.hipMalloc(C.byref(dev), src.nbytes) == 0 and hip.hipMemcpy(dev, src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0          # 1: host to device, synchronous
    res = []
    for shape in ("poll", "batch", "device"):
        fe = gpu.RealFrontend(s["fs_r"], [(s["base"], s["freqs"])])
        assert fe.geometry.fold_batch == 4
        nb = fe.real_block
        fe.export_enable([0, 1, 2], ring_blocks=64)
        pdus = []
        for b in range(nblk):
            if shape == "device":
                fe.push_real([dev.value + 2 * b * nb], F.SFMT_RS16, on_device=True)
            else:
                fe.push_real([s["v16"][b * nb:(b + 1) * nb]], F.SFMT_RS16)
            if shape == "poll":
                pdus += fe.poll_pdus()
        pdus += fe.poll_pdus()
        res.append((export_all(fe, nblk), sorted((p["freq"], p["sample_index"], p["octets"]) for p in pdus)))
        fe.close()
    assert hip.hipFree(dev) == 0
    (a, ac), pa = res[0]
    assert np.mean(a != 0) > 0.9 and len(pa) == 6 and nblk <= 64
    for (w, wc), p in res[1:]:
        assert np.array_equal(w, a) and np.array_equal(wc, ac) and p == pa


def test_fold_spectrum_0_and_fold_prune_are_ignored(gpu, oracle, monkeypatch):
    """HFDL_GPU_FOLD_SPECTRUM=0 and HFDL_GPU_FOLD_PRUNE on a real front end at 2.8 Msps (N' = 2^18, octet layout: the geometry at which a
    complex front end of the equivalent rate takes both; for the prune that is asserted).  The real front end reports
    every alias row folded, and its filters, its spectrum and its channelizer output are, as uint32, those of a run with neither set."""
    fs_r, base, nblk = 2_800_000, 0, 3
    fs, centre = R.equiv(fs_r, base)
    _, _, d0 = oracle.geometry(fs)
    freqs = R.channel_freqs(fs_r, base, d0.overlap_length)
    v16 = make_stream(oracle, fs_r, base, freqs, nblk, 61)[1]
    res = []
    for env in (None, dict(HFDL_GPU_FOLD_SPECTRUM="0"), dict(HFDL_GPU_FOLD_PRUNE="3e-7"), dict(HFDL_GPU_FOLD_SPECTRUM="0", HFDL_GPU_FOLD_PRUNE="3e-7")):
        for k in ("HFDL_GPU_FOLD_SPECTRUM", "HFDL_GPU_FOLD_PRUNE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        if env == dict(HFDL_GPU_FOLD_PRUNE="3e-7"):
            # the prune bites on a complex front end of the equivalent stream (the mixed domain shows in no geometry field: there the
            # proof is the words below, which a fold reading a layout real_tap_combine_kernel never wrote could not reproduce)
            cfe = gpu.Frontend(fs, centre, freqs)
            assert 0 < cfe.geometry.fold_rows < cfe.geometry.pre_decimation
            cfe.close()
        fe = gpu.RealFrontend(fs_r, [(base, freqs)])
        g = fe.geometry
        assert g.fold_rows == g.pre_decimation and g.fft_size == 1 << 18
        nb = fe.real_block
        fe.export_enable(list(range(len(freqs))), ring_blocks=8)
        for b in range(nblk):
            fe.push_real([v16[b * nb:(b + 1) * nb]], F.SFMT_RS16)
        fe.sync()
        words, counts = export_all(fe, nblk)
        res.append((words, counts, [u32(fe.read_tap(F.TAP_FILTER, c)).copy() for c in range(len(freqs))], u32(fe.read_tap(F.TAP_SPECTRUM)).copy()))
        fe.close()
    assert np.mean(res[0][0] != 0) > 0.9
    for words, counts, fil, spec in res[1:]:
        assert np.array_equal(words, res[0][0]) and np.array_equal(counts, res[0][1]) and np.array_equal(spec, res[0][3])
        assert all(np.array_equal(a, b) for a, b in zip(fil, res[0][2]))


def test_push_baseband_canceller_and_quality_records_on_a_real_front_end(gpu, scene):
    """What the header promises unchanged behind the channelizer.  Run A: the real stream pushed block by block with the carrier canceller
    on every channel and the frame quality records on; its channelizer output collected by the export.  Run B: another real front end,
    same settings, fed that output through push_baseband.  PDUs (every field), quality records (the structs' bytes) and canceller records
    are equal: push_baseband works on a real front end, and canceller and records sit behind the channelizer, per channel, as ever.
    Run C: the complex front end on the complex stream with the same settings decodes the same frames (frequency, mode, octets)."""
    s = scene
    nch = len(s["freqs"])

    def settings(fe):
        fe.notch_enable(0.002)
        fe.quality_enable(ring_frames=64)

    def collect(fe):
        pdus = sorted(fe.poll_pdus(), key=lambda p: (p["channel"], p["sample_index"]))
        recs, _, dropped = fe.quality_read(wait=True)
        st = [fe.notch_stats(c) for c in range(nch)]
        return pdus, sorted(r["raw"] for r in recs), dropped, st

    fe = gpu.RealFrontend(s["fs_r"], [(s["base"], s["freqs"])])
    settings(fe)
    fe.export_enable(list(range(nch)), ring_blocks=64)
    nb = fe.real_block
    for b in range(s["nblk"]):
        fe.push_real([s["v16"][b * nb:(b + 1) * nb]], F.SFMT_RS16)
    a = collect(fe)
    samples, counts, _, _, blocks, _ = fe.export_read(0, wait=True)
    fe.close()
    assert blocks == list(range(s["nblk"]))
    fe = gpu.RealFrontend(s["fs_r"], [(s["base"], s["freqs"])])
    settings(fe)
    for b in range(s["nblk"]):
        fe.push_baseband([samples[b, c, :counts[b, c]] for c in range(nch)])
    bb = collect(fe)
    assert fe.counters()["blocks"] == 0                      # (push_baseband is no wideband block)
    fe.close()
    fe = gpu.Frontend(s["fs"], s["centre"], s["freqs"])
    settings(fe)
    for b in range(s["nblk"]):
        fe.push_block(s["w"][b * s["n"]:(b + 1) * s["n"]])
    c = collect(fe)
    fe.close()
    print("canceller + quality on a real front end: %d PDUs, %d records; complex front end %d PDUs" % (len(a[0]), len(a[1]), len(c[0])))
    assert len(a[0]) >= 1 and len(a[1]) == len(a[0]) and a[2] == 0
    assert bb[0] == a[0] and bb[1] == a[1] and bb[2] == 0
    assert [(t["blocks"], t["resets"]) for t in bb[3]] == [(t["blocks"], t["resets"]) for t in a[3]] and all(t["blocks"] == s["nblk"] for t in a[3])
    assert all(np.array_equal(u32(np.array([x[k] for k in ("last_in_power", "last_out_power", "tap_energy")])), u32(np.array([y[k] for k in ("last_in_power", "last_out_power", "tap_energy")])))
               for x, y in zip(a[3], bb[3]))
    assert sorted((p["freq"], p["mode"], p["octets"]) for p in a[0]) == sorted((p["freq"], p["mode"], p["octets"]) for p in c[0])


def test_two_real_receivers_equal_one_each(gpu, oracle):
    """two receivers with different `base` in one front end at the 500 ksps geometry: each receiver's channelizer output, filters and
    spectrum equal a single-receiver front end's, word for word"""
    fs_r, bases, nblk = 500_000, (5_000_000, 11_000_000), 3
    fs = fs_r // 2
    _, _, d0 = oracle.geometry(fs)
    recv = [(b, R.channel_freqs(fs_r, b, d0.overlap_length)[1 - r:4 - r]) for r, b in enumerate(bases)]
    xs = [make_stream(oracle, fs_r, b, fr, nblk, 40 + r)[1] for r, (b, fr) in enumerate(recv)]

    def run_fe(receivers, streams):
        fe = gpu.RealFrontend(fs_r, receivers)
        nch = fe.geometry.channels
        nb = fe.real_block
        fe.export_enable(list(range(nch)), ring_blocks=16)
        for b in range(nblk):
            fe.push_real([x[b * nb:(b + 1) * nb] for x in streams], F.SFMT_RS16)
        fe.sync()
        words, counts = export_all(fe, nblk)
        fil = [u32(fe.read_tap(F.TAP_FILTER, c)).copy() for c in range(nch)]
        firsts = [sum(len(fr) for _, fr in receivers[:r]) for r in range(len(receivers))]
        spec = [u32(fe.read_tap(F.TAP_SPECTRUM, c)).copy() for c in firsts]
        fe.close()
        return words, counts, fil, spec

    both = run_fe(recv, xs)
    at = 0
    for r in range(2):
        one = run_fe([recv[r]], [xs[r]])
        k = len(recv[r][1])
        assert np.array_equal(both[0][:, at:at + k], one[0]) and np.array_equal(both[1][:, at:at + k], one[1]), r
        assert all(np.array_equal(a, b) for a, b in zip(both[2][at:at + k], one[2])) and np.array_equal(both[3][r], one[3][0]), r
        assert np.mean(one[0] != 0) > 0.9
        at += k


def test_retuned_channel_has_a_fresh_creates_filter(gpu, oracle):
    for fs_r in (96_000, 500_000):
        base = 0
        fs = fs_r // 2
        _, _, d0 = oracle.geometry(fs)
        freqs = R.channel_freqs(fs_r, base, d0.overlap_length)[:3]
        f_new = base + fs_r // 4 + 4_321
        fe = gpu.RealFrontend(fs_r, [(base, freqs)])
        before = [u32(fe.read_tap(F.TAP_FILTER, c)).copy() for c in range(3)]
        fe.retune(1, f_new)
        after = [u32(fe.read_tap(F.TAP_FILTER, c)).copy() for c in range(3)]
        with pytest.raises(F.GpuError):
            fe.retune(1, base + fs_r // 2 + 10)               # outside the span of the equivalent stream
        fe.close()
        fresh = gpu.RealFrontend(fs_r, [(base, [freqs[0], f_new, freqs[2]])])
        want = [u32(fresh.read_tap(F.TAP_FILTER, c)).copy() for c in range(3)]
        fresh.close()
        assert np.array_equal(after[1], want[1]) and not np.array_equal(after[1], before[1]), fs_r
        assert all(np.array_equal(after[c], before[c]) and np.array_equal(after[c], want[c]) for c in (0, 2)), fs_r


def test_blanker_on_pairs_monitor_bands_and_refusals(gpu, oracle):
    """Noise with a few impulses 40 dB up, 96 ksps, blanker at 14 dB.  The model: pair power x[2n]^2 + x[2n + 1]^2 in fp32 against
    k2 times its mean over the block's new pairs; a pair above goes as a whole, and the history holds blanked values.  The spectrum
    equals the model's under the spectrum gates.  The monitor (RECT, 64 bands): band sums of the float64 spectrum of the blanked window
    / N'^2, per band within spectrum_f64.gate(G) (the sums' own fp32 order) + 2 x 3e-6 (|X + e|^2 - |X|^2 <= 2 |X| |e| + |e|^2 with |e| at
    the spectrum gate's RMS bound) of the band's power.  The refusals: iqbal_enable, complex formats, cf32 pushes; a real format on a
    complex front end."""
    fs_r, base = 96_000, 0
    fs, centre = R.equiv(fs_r, base)
    _, _, d0 = oracle.geometry(fs)
    fe = gpu.RealFrontend(fs_r, [(base, [20_000])])
    g = fe.geometry
    nb, nblk, bins = fe.real_block, 3, 64
    rng = np.random.default_rng(9)
    x = (0.05 * rng.standard_normal(nblk * nb)).astype(np.float32)
    hits = rng.choice(nblk * nb, 12, replace=False)
    x[hits] = 5.0
    L = fe._L
    # both refusals name the reason (on a complex front end whose corrector was never enabled the seed is refused too, with another text)
    assert L.hfdl_gpu_frontend_iqbal_enable(fe._h, -1, 0.125) == -1 and b"real input" in L.hfdl_gpu_last_error()
    assert L.hfdl_gpu_frontend_iqbal_seed(fe._h, -1, 0.0, 0.0, 0.0, 0.0, 0) == -1 and b"real input" in L.hfdl_gpu_last_error()
    blk = x[:nb]
    for fmt, ns in ((F.SFMT_CF32, nb // 2), (F.SFMT_CS16, nb // 2), (F.SFMT_CU8, nb // 2), (F.SFMT_RF32, nb // 2), (F.SFMT_RF32, nb + 2), (7, nb)):
        assert L.hfdl_gpu_frontend_push_block_raw(fe._h, blk.ctypes.data_as(C.c_void_p), ns, fmt, 0) == -1, (fmt, ns)
    assert L.hfdl_gpu_frontend_push_block(fe._h, blk.ctypes.data_as(C.c_void_p), nb // 2, 0) == -1
    assert L.hfdl_gpu_frontend_channelize_block(fe._h, blk.ctypes.data_as(C.c_void_p), nb // 2, 0) == -1
    assert fe.counters()["blocks"] == 0
    fe.blanker_enable(14.0)
    fe.spectrum_enable(bins)
    k2 = np.float32(10.0 ** 1.4)
    xb = x.copy()
    blanked = 0
    p64 = []
    for b in range(nblk):
        fe.push_real([x[b * nb:(b + 1) * nb]], F.SFMT_RF32)
        new = xb[b * nb:(b + 1) * nb]
        pw = new[0::2] * new[0::2] + new[1::2] * new[1::2]
        T = float(k2) * float(np.mean(pw.astype(np.float64)))
        assert not np.any(np.abs(pw / T - 1) < 1e-3)             # no pair within the mean's rounding of the threshold
        gone = pw > T
        blanked += int(gone.sum())
        new[0::2][gone] = 0
        new[1::2][gone] = 0
        want = R.block_spectrum(xb.astype(np.float64), b, d0)
        e = spectrum_errors(fe.read_tap(F.TAP_SPECTRUM), want)
        print("blanked block %d: %d pairs gone so far, spectrum rel rms %.3g worst/rms %.3g" % (b, blanked, e[0], e[1]))
        assert e[0] <= SPEC_RMS and e[1] <= 10 * SPEC_RMS
        p64.append((np.abs(want) ** 2).reshape(bins, -1).sum(axis=1) / float(g.fft_size) ** 2)
    st = fe.blanker_stats(0)
    assert st["blocks"] == nblk and st["samples_blanked"] == blanked and 6 <= blanked <= 12
    got = fe.spectrum_read(0)
    G = g.fft_size // bins
    mean64 = np.mean(p64, axis=0)
    err = np.abs(got["mean"].astype(np.float64) - mean64)
    print("monitor: worst band error %.3g of its power (gate %.3g)" % (float((err / mean64).max()), S.gate(G) + 2 * SPEC_RMS))
    assert got["blocks"] == nblk and (err <= (S.gate(G) + 2 * SPEC_RMS) * mean64).all()
    lo, hi = S.band_edges(centre, fs, g.fft_size, bins)
    assert abs(lo[0] - (base - 0.5 * fs / g.fft_size)) < 1e-6 and abs(hi[-1] - (base + fs_r / 2 - 0.5 * fs / g.fft_size)) < 1e-6       # base .. base + fs_r / 2
    assert np.allclose(got["freqs"], (lo + hi) / 2, rtol=0, atol=1e-6)
    fe.close()
    cfe = gpu.Frontend(250_000, 10_000_000, [10_020_000])
    z = np.zeros(4 * cfe.input_size, np.float32)
    for fmt in (F.SFMT_RS16, F.SFMT_RF32):
        assert cfe._L.hfdl_gpu_frontend_push_block_raw(cfe._h, z.ctypes.data_as(C.c_void_p), 2 * cfe.input_size, fmt, 0) == -1
        assert cfe._L.hfdl_gpu_frontend_push_block_raw(cfe._h, z.ctypes.data_as(C.c_void_p), cfe.input_size, fmt, 0) == -1
    assert cfe.counters()["blocks"] == 0 and cfe.real_input() == (False, 0)
    cfe.close()
