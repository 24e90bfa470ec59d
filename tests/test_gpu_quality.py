"""GPU tests of the frame quality records (hfdl_gpu_frontend_quality_enable / _quality_read, hfdl_gpu_frame_quality_batch;
frame_quality_kernel in dumphfdl_amd/csrc/quality_kernels.hip; include/hfdl_gpu.h "Frame quality records").

What a record must be: its PDU's twin by (channel, sample_index), the PDU's own bits where the two share a field, the figures of
tests/quality_f64.py within its derived bound (K = 96 roundings' worth, see there) and -- compared as uint32 -- the same bits however
the frames were batched, pushed or polled.  The captured symbols must be the ones that were decoded: the burst_decode stage entry turns
them back into the PDU's octets.

250 ksps x 4 channels (N = 2^15, the geometry of tests/test_gpu_export.py): one stream of five bursts -- BPSK, QPSK, 8-PSK single-slot
and a double-slot frame on four channels, then a second frame on the first channel -- pushed once per case; one reference pass is
shared."""
import os
import subprocess

import numpy as np
import pytest

import burst_frames
import fec_model as fm
import hfdl_synth as synth
import quality_f64 as Q
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, CF = 250_000, 10_000_000
FREQS = [9_930_000, 9_958_000, 10_037_000, 10_081_500]
DUR = 5.9


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pdu_key(p):
    return (p["freq"], p["sample_index"], p["mode"], p["octets"], p["slot"], p["fcs_status"])


def by_frame(items):
    return {(d["channel"], d["sample_index"]): d for d in items}


def bits(v):
    return np.float32(v).view(np.uint32)


class Stream:
    def __init__(self, gpu):
        fe = gpu.Frontend(FS, CF, FREQS)
        self.n = fe.input_size
        fe.close()
        rng = np.random.default_rng(21)
        self.bursts = [dict(freq=FREQS[0], mode=1, octets=synth.make_pdu(rng, 1), t0=0.15, amp=0.1, cfo=6.0),
                       dict(freq=FREQS[1], mode=2, octets=synth.make_pdu(rng, 2), t0=0.21, amp=0.08, cfo=-4.0),
                       dict(freq=FREQS[2], mode=3, octets=synth.make_pdu(rng, 3), t0=0.18, amp=0.12, cfo=2.0),
                       dict(freq=FREQS[3], mode=6, octets=synth.make_pdu(rng, 6), t0=0.25, amp=0.1, cfo=-7.0),
                       dict(freq=FREQS[0], mode=1, octets=synth.make_pdu(rng, 1), t0=2.95, amp=0.09, cfo=5.0)]
        self.nblk = int(DUR * FS) // self.n
        self.x = synth.synth_wideband(FS, CF, self.nblk * self.n, self.bursts, noise_sigma=0.004, seed=6).astype(np.complex64)
        self.split = int(2.75 * FS) // self.n            # the three single-slot frames have ended, the other two have not

    def push(self, fe, blocks=None, after=None):
        for b in (range(self.nblk) if blocks is None else blocks):
            fe.push_block(self.x[b * self.n:(b + 1) * self.n])
            if after:
                after(b)


@pytest.fixture(scope="module")
def stream(gpu):
    return Stream(gpu)


@pytest.fixture(scope="module")
def ref(gpu, stream):
    """Quality off: the PDUs and statistics of the plain pass.  Quality on with symbols, everything pushed, then a draining poll: the
    records and their symbols."""
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    stream.push(fe)
    off_pdus, off_stats = fe.poll_pdus(), fe.all_channel_stats()
    fe.close()
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    fe.quality_enable(64, symbols=True)
    stream.push(fe)
    pdus = fe.poll_pdus()
    recs, syms, dropped = fe.quality_read(wait=False)            # after a draining poll: everything, without waiting
    stats = fe.all_channel_stats()
    fe.close()
    return dict(off_pdus=off_pdus, off_stats=off_stats, pdus=pdus, recs=recs, syms=syms, dropped=dropped, stats=stats)


# ---------------------------------------------------------------- 1. the stage entry

def test_stage_entry_against_the_model_and_bit_identical(gpu):
    frames = burst_frames.frames()
    for f in frames:
        assert Q.decisions_are_safe(f), (f["mode"], f["mask"], f["kind"])
    sym, modes = [f["symbols"] for f in frames], [f["mode"] for f in frames]
    whole = F.frame_quality(sym, modes)
    again = F.frame_quality(sym, modes)
    assert len(whole) == len(frames)
    for i, (f, r) in enumerate(zip(frames, whole)):
        what = (f["mode"], f["mask"], f["kind"])
        assert (r["mode"], r["channel"], r["freq"], r["sample_index"], r["bitmask_lsb"], r["train_bits_total"]) == (f["mode"], 0, 0, 0, 0, 0), what
        assert (r["freq_err_hz"], r["rssi_db"], r["noise_floor_db"]) == (0, 0, 0), what
        Q.check(r, Q.model(f["symbols"], f["mode"]), what)
        assert r["raw"] == again[i]["raw"], what
        alone = F.frame_quality([f["symbols"]], [f["mode"]])      # nframes = 1: a single-slot (2160) or a double-slot (5040) frame
        assert len(alone) == 1 and np.array_equal(u32(np.frombuffer(alone[0]["raw"], np.uint8)), u32(np.frombuffer(r["raw"], np.uint8))), what
    assert {len(f["symbols"]) for f in frames} == {2160, 5040}


# ---------------------------------------------------------------- 2. end to end

def test_records_are_their_pdus_twins(gpu, stream, ref):
    pdus, recs, syms = ref["pdus"], ref["recs"], ref["syms"]
    assert ref["dropped"] == 0 and len(pdus) == len(stream.bursts) == 5
    assert sorted(p["mode"] for p in pdus) == [1, 1, 2, 3, 6] and sorted(p["channel"] for p in pdus) == [0, 0, 1, 2, 3]
    P, R = by_frame(pdus), by_frame(recs)
    assert len(R) == len(recs) and set(R) == set(P)
    for key, r in R.items():
        p = P[key]
        assert (r["freq"], r["mode"], r["train_bits_bad"], r["train_bits_total"]) == (p["freq"], p["mode"], p["train_bits_bad"], p["train_bits_total"])
        for k in ("freq_err_hz", "rssi_db", "noise_floor_db"):
            assert bits(r[k]) == bits(p[k]), k
        sz = fm.sizes(r["mode"])
        assert (r["nsym"], r["segments"]) == (sz["nsym"], sz["nsym"] // 30) and r["train_bits_total"] > 0
    for i, r in enumerate(recs):
        p = P[(r["channel"], r["sample_index"])]
        x = syms[i, :r["nsym"]]
        # the captured symbols are the ones that were decoded
        assert F.burst_decode([x], [r["mode"]], [r["bitmask_lsb"]]) == [p["octets"]]
        tail = u32(syms[i, r["nsym"]:])
        assert not tail.any()                                    # +0.0, not -0.0
        stage = F.frame_quality([x], [r["mode"]])[0]
        for k in ("sym_power", "err_power", "err_max", "gain_re", "gain_im"):
            assert bits(r[k]) == bits(stage[k]), k
        assert np.array_equal(u32(r["seg_err_power"]), u32(stage["seg_err_power"]))
        Q.check(r, Q.model(x, r["mode"]), (r["channel"], r["mode"]))
        assert r["err_power"] > 0 and r["err_max"] >= r["seg_err_power"].max() >= r["err_power"]


# ---------------------------------------------------------------- 3. independence

def test_records_do_not_depend_on_pushing_and_polling_and_change_no_pdu(gpu, stream, ref):
    want = sorted(r["raw"] for r in ref["recs"])
    assert sorted(map(pdu_key, ref["pdus"])) == sorted(map(pdu_key, ref["off_pdus"])) and ref["stats"] == ref["off_stats"]

    # a sync after every push
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    fe.quality_enable(64)
    got, pdus = [], []
    stream.push(fe, after=lambda b: (fe.sync(), got.extend(fe.quality_read(wait=False)[0])))
    pdus = fe.poll_pdus()
    got += fe.quality_read(wait=False)[0]
    assert sorted(r["raw"] for r in got) == want and sorted(map(pdu_key, pdus)) == sorted(map(pdu_key, ref["off_pdus"]))
    assert fe.all_channel_stats() == ref["off_stats"]
    fe.close()

    # nothing drained while pushing: only what is known to be complete, without waiting
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    fe.quality_enable(64)
    got, pdus = [], []

    def step(b):
        pdus.extend(fe.poll_pdus(max_in_flight=2))
        got.extend(fe.quality_read(wait=False)[0])
    stream.push(fe, after=step)
    pdus += fe.poll_pdus()
    got += fe.quality_read(wait=False)[0]
    assert sorted(r["raw"] for r in got) == want and sorted(map(pdu_key, pdus)) == sorted(map(pdu_key, ref["off_pdus"]))
    assert fe.all_channel_stats() == ref["off_stats"]
    fe.close()


# ---------------------------------------------------------------- 4. a full ring

def test_a_full_ring_drops_whole_frames_and_reading_makes_room(gpu, stream, ref):
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    fe.quality_enable(2, symbols=True)
    stream.push(fe)
    fe.sync()
    recs, syms, dropped = fe.quality_read(wait=False)
    whole = {r["raw"] for r in ref["recs"]}
    assert len(recs) == 2 and dropped == 3 and all(r["raw"] in whole for r in recs) and len({r["raw"] for r in recs}) == 2
    R = {r["raw"]: i for i, r in enumerate(ref["recs"])}
    for i, r in enumerate(recs):
        assert np.array_equal(u32(syms[i]), u32(ref["syms"][R[r["raw"]]]))
    nothing = fe.quality_read(wait=True)
    assert nothing[0] == [] and len(nothing[1]) == 0 and nothing[2] == 3
    # the host has read: the next frames find room again
    stream.push(fe)
    recs2, _, dropped2 = fe.quality_read(wait=True)
    assert len(recs2) == 2 and dropped2 == 6
    assert {r["sample_index"] for r in recs2}.isdisjoint({r["sample_index"] for r in recs})
    assert len(fe.poll_pdus()) == 10
    fe.close()


# ---------------------------------------------------------------- 5. enable mid-stream

def test_enable_mid_stream_again_and_off(gpu, stream, ref):
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    with pytest.raises(F.GpuError):
        fe.quality_read()
    stream.push(fe, range(stream.split))
    early = fe.poll_pdus()                                       # every half so far has been queued, and decoded, without the records
    fe.quality_enable(16)
    stream.push(fe, range(stream.split, stream.nblk))
    late = fe.poll_pdus()
    recs, syms, dropped = fe.quality_read(wait=False)
    assert len(early) == 3 and len(late) == 2 and syms is None and dropped == 0
    assert set(by_frame(recs)) == set(by_frame(late)) and len(recs) == 2
    whole = {r["raw"] for r in ref["recs"]}
    assert all(r["raw"] in whole for r in recs)
    # a second enable empties the ring
    stream.push(fe, range(stream.split))
    fe.sync()
    fe.quality_enable(16)
    assert fe.quality_read(wait=True) == ([], None, 0)
    for bad in (dict(ring_frames=1), dict(ring_frames=F.QUALITY_RING_MAX + 1), dict(ring_frames=-2)):
        with pytest.raises(F.GpuError):
            fe.quality_enable(**bad)
    assert fe._L.hfdl_gpu_frontend_quality_enable(fe._h, 16, 2) == -1        # an unknown flag
    assert fe._L.hfdl_gpu_frontend_quality_enable(fe._h, 65536, 1) == -5     # 65536 x 41 064 bytes: above 1 GiB (HFDL_GPU_ERANGE)
    fe.quality_enable(0)
    with pytest.raises(F.GpuError):
        fe.quality_read()
    fe.close()


# ---------------------------------------------------------------- 6. retune, several receivers

def test_records_carry_their_pdus_frequency_across_a_retune(gpu):
    f_new = 10_010_000
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    n = fe.input_size
    rng = np.random.default_rng(31)
    bursts = [dict(freq=FREQS[0], mode=1, octets=synth.make_pdu(rng, 1), t0=0.15, amp=0.1, cfo=3.0),
              dict(freq=f_new, mode=1, octets=synth.make_pdu(rng, 1), t0=3.0, amp=0.1, cfo=-3.0)]
    nblk = int(5.6 * FS) // n
    k = int(2.75 * FS) // n
    x = synth.synth_wideband(FS, CF, nblk * n, bursts, noise_sigma=0.004, seed=8).astype(np.complex64)
    fe.quality_enable(16)
    for b in range(nblk):
        if b == k:
            fe.retune(0, f_new)
        fe.push_block(x[b * n:(b + 1) * n])
    pdus = fe.poll_pdus()
    recs, _, _ = fe.quality_read(wait=False)
    fe.close()
    P, R = by_frame(pdus), by_frame(recs)
    assert [p["freq"] for p in sorted(pdus, key=lambda p: p["sample_index"])] == [FREQS[0], f_new]
    assert set(P) == set(R) and all(R[key]["freq"] == P[key]["freq"] for key in P)


def test_records_of_several_receivers_carry_global_channels(gpu):
    centres = [10_000_000, 11_000_000]
    freqs = [[9_958_000, 10_037_000], [10_958_000, 11_037_000]]
    fe = gpu.MultiFrontend(FS, list(zip(centres, freqs)))
    fe.enable_taps(False)
    n = fe.input_size
    rng = np.random.default_rng(41)
    nblk = int(2.8 * FS) // n
    xs = []
    for r in range(2):
        b = [dict(freq=freqs[r][1], mode=1 + r, octets=synth.make_pdu(rng, 1 + r), t0=0.15 + 0.05 * r, amp=0.1, cfo=3.0)]
        xs.append(synth.synth_wideband(FS, centres[r], nblk * n, b, noise_sigma=0.004, seed=50 + r).astype(np.complex64))
    fe.quality_enable(16)
    for b in range(nblk):
        fe.push_blocks([x[b * n:(b + 1) * n] for x in xs])
    pdus = fe.poll_pdus()
    recs, _, _ = fe.quality_read(wait=False)
    fe.close()
    assert sorted(p["channel"] for p in pdus) == [1, 3]
    assert set(by_frame(recs)) == set(by_frame(pdus))
    assert {r["channel"]: r["freq"] for r in recs} == {1: freqs[0][1], 3: freqs[1][1]}


# ---------------------------------------------------------------- 7. a physical check

def test_the_stronger_of_two_bursts_has_the_smaller_error(gpu):
    """Two bursts of the same mode in the same noise, 10 dB apart: the order of err_power only, no figure."""
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.enable_taps(False)
    n = fe.input_size
    rng = np.random.default_rng(51)
    bursts = [dict(freq=FREQS[1], mode=2, octets=synth.make_pdu(rng, 2), t0=0.15, amp=0.1, cfo=3.0),
              dict(freq=FREQS[2], mode=2, octets=synth.make_pdu(rng, 2), t0=0.15, amp=0.1 / np.sqrt(10.0), cfo=3.0)]
    nblk = int(2.8 * FS) // n
    x = synth.synth_wideband(FS, CF, nblk * n, bursts, noise_sigma=0.01, seed=9).astype(np.complex64)
    fe.quality_enable(16)
    for b in range(nblk):
        fe.push_block(x[b * n:(b + 1) * n])
    pdus = fe.poll_pdus()
    recs, _, _ = fe.quality_read(wait=False)
    fe.close()
    R = {r["channel"]: r for r in recs}
    assert sorted(R) == [1, 2] and len(pdus) == 2
    for c in (1, 2):
        print("channel %d: MER %.2f dB, gain- and phase-corrected %.2f dB" % (c, -10 * np.log10(R[c]["err_power"]),
              -10 * np.log10(R[c]["sym_power"] - R[c]["gain_re"] ** 2 - R[c]["gain_im"] ** 2)))
    assert R[1]["err_power"] < R[2]["err_power"]


# ---------------------------------------------------------------- 8. the replay program

def test_replay_writes_a_line_per_pdu(gpu, stream, ref, tmp_path):
    """hfdl_replay --frame-log over libhfdl_host.so and the real libhfdl_gpu.so (the weak references resolve): as many lines as PDUs,
    each with a PDU's time and frequency."""
    path, log = tmp_path / "in.cs16", tmp_path / "frames.log"
    np.rint(stream.x.view(np.float32) * 32767.0).astype(np.int16).tofile(path)
    khz = lambda f: "%.1f" % (f / 1e3)
    out = subprocess.run([os.path.join(ROOT, "dumphfdl_amd", "hfdl_replay"), "--iq-file", str(path), "--sample-rate", str(FS), "--sample-format", "CS16",
                          "--centerfreq", khz(CF), "--frame-log", str(log)] + [khz(f) for f in FREQS], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "frame log:" not in out.stderr and "GPU front end" not in out.stderr, out.stderr[-2000:]
    pdus = [dict(kv.split("=") for kv in ln.split()[1:-1]) for ln in out.stdout.splitlines() if ln.startswith("PDU ")]
    lines = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in open(log).read().splitlines()]
    assert len(pdus) == 5 and len(lines) == len(pdus)
    assert sorted((ln["ts"], ln["freq"]) for ln in lines) == sorted((p["ts"], p["freq"]) for p in pdus)
    for ln in lines:
        assert np.isfinite(float(ln["mer_db"])) and 0 <= int(ln["worst_segment"]) < 168 and float(ln["worst_mer_db"]) <= float(ln["mer_db"])
