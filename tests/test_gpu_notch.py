"""GPU tests of the adaptive carrier canceller (hfdl_gpu_frontend_notch_enable / _stats, hfdl_gpu_notch_rows, HFDL_GPU_TAP_NOTCH_OUT;
dumphfdl_amd/csrc/notch_kernels.hip) against the host build of dumphfdl_amd/csrc/notch.h (tests/hostsim/notch_check.cpp), word for word:

  1. the stage alone, y and state as uint32, over the sizes around D and D + L - 1, one to three channels, state carried over calls;
  2. the pipeline at 250 ksps, a carrier in the middle channel: off = the oracle; on = the host model on the device's own channelizer
     rows, block by block, the oracle's demodulator on the model's output, the record;
  3. cuts change nothing;  4. the export is untouched;  5. enable in mid-stream, retune;  6. two receivers;  7. push_baseband.

The pipeline scenario (tests/notch_f64.py): six single-slot frames on the middle channel.  A single-slot frame lasts 2.34 s, so six of
them on one channel take 15.9 s of signal (139 blocks), not six; one more frame on each of the other two channels gives their PDU
comparison something to compare.

The canceller is enabled behind the FIRST block (START = 1) in every pipeline test but the last one.  A front end's first block begins
with the channelizer's start-up ramp -- the channel filter running onto a stream that has no past: some 60 samples rising from 1e-9 to
the signal's level.  A normalised step divides by the power in the delay line, which is 24 samples behind the sample it explains, so
on the ramp the taps are driven far beyond any bound (sum |w|^2 = 188 on this input), the rest of that row is spoilt, and the reset at
the row's end puts the channel right: one reset, in row 0, by the rule as it stands.  test_start_up_ramp_costs_one_reset pins that."""
import numpy as np
import pytest

import notch_f64 as nf
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu
FS, CF, FREQS, MID, N, MU = nf.FS, nf.CF, nf.FREQS, nf.MID, nf.N, nf.MU
TAP_CHAN_OUT, TAP_NOTCH_OUT = F.TAP_CHAN_OUT, F.TAP_NOTCH_OUT
STAGE_N = (1, 23, 24, 25, 55, 56, 57, 897, 1793)
START = 1                     # blocks pushed before the canceller is enabled (the module's text)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return len(a) == len(b) and bool((bits(a) == bits(b)).all())


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("notch")
    return nf.build_check(d), d


# ---------------------------------------------------------------- 1. the stage alone

def stage_input(kind, nch, n):
    rng = np.random.default_rng(100 * nch + n)
    if kind == "zeros":
        return np.zeros((nch, n), np.complex64)
    f = (0.055, -0.115, 0.31)
    x = np.stack([0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + np.exp(2j * np.pi * (f[c] * np.arange(n) + rng.random())) for c in range(nch)])
    scale = {"unit": 1.0, "tiny": 2.0 ** -60, "huge": 2.0 ** 60}[kind]
    return (x * scale).astype(np.complex64)


@pytest.mark.parametrize("kind", ["unit", "tiny", "huge", "zeros"])
@pytest.mark.parametrize("nch", [1, 2, 3])
def test_stage_alone_word_for_word(gpu, exe, kind, nch):
    """nch 1, 2, 3: the second half of a wave empty, full, and the next wave.  Three consecutive calls of 3 n samples in all against the
    host build, the state carried by the caller on both sides."""
    prog, work = exe
    for n in STAGE_N:
        x = stage_input(kind, nch, 3 * n)
        dev_state, host_state = None, None
        for call in range(3):
            part = x[:, call * n:(call + 1) * n]
            y, dev_state = gpu.notch_rows(part, MU, dev_state)
            want, host_state, _ = nf.host_rows(prog, work, part, MU, host_state)
            assert same(y, want), (kind, nch, n, call, int((bits(y) != bits(want)).sum()))
            assert same(dev_state, host_state), (kind, nch, n, call)
        if kind != "zeros" and n >= 897:
            assert np.abs(dev_state[:, :64]).max() > 0          # the taps have moved: the comparison is not one of zeros
    # state NULL = fresh and discarded
    y, _ = gpu.notch_rows(x[:, :57], MU)
    assert same(y, nf.host_rows(prog, work, x[:, :57], MU)[0])


# ---------------------------------------------------------------- 2. the pipeline

def pdu_key(pdus):
    return sorted((p["freq"], p["sample_index"], p["mode"], bytes(p["octets"])) for p in pdus)


def run_blocks(fe, x, nblk, rows_of=(), notch_rows_of=(), first=0):
    """push blocks first .. first + nblk - 1 of x with a read of the asked taps after every block:
    ({channel: [CHAN_OUT row per block]}, {channel: [NOTCH_OUT row per block]})"""
    rows = {c: [] for c in rows_of}
    nrows = {c: [] for c in notch_rows_of}
    for b in range(first, first + nblk):
        fe.push_block(x[b * N:(b + 1) * N])
        for c in rows_of:
            rows[c].append(fe.read_tap(TAP_CHAN_OUT, c))
        for c in notch_rows_of:
            nrows[c].append(fe.read_tap(TAP_NOTCH_OUT, c))
    return rows, nrows


def model_rows(exe, rows, mu=MU):
    """the host model on a channel's rows, state carried across them: ([y row per block], per-row records)"""
    prog, work = exe
    y, recs, s = nf.host_stream(prog, work, np.concatenate(rows), [len(r) for r in rows], mu)
    assert s["resets"] == 0 and s["finite"]
    cuts = np.cumsum([len(r) for r in rows])[:-1]
    return np.split(y, cuts), recs


@pytest.fixture(scope="module")
def runs(gpu, exe):
    """the tone stream through the device, off and on (the middle channel), a read of every row after every block"""
    s = nf.pipeline_scenario()
    nblk = len(s["tone"]) // N
    out = dict(nblk=nblk)
    for name, sel in (("off", None), ("on", [MID])):
        fe = gpu.Frontend(FS, CF, FREQS)
        rows, nrows = run_blocks(fe, s["tone"], START, range(3), ())
        if sel is not None:
            fe.notch_enable(MU, sel)
            assert fe.notch_stats(MID) == dict(blocks=0, resets=0, last_in_power=0, last_out_power=0, tap_energy=0)
        more, nrows = run_blocks(fe, s["tone"], nblk - START, range(3), range(3) if sel is not None else (), first=START)
        rows = {c: rows[c] + more[c] for c in range(3)}
        pdus = fe.poll_pdus()
        out[name] = dict(rows=rows, nrows=nrows, pdus=pdus, stats=fe.notch_stats(MID) if sel is not None else None)
        fe.close()
    # (the model's rows and the device's NOTCH_OUT rows are numbered from block START)
    out["model"] = model_rows(exe, out["on"]["rows"][MID][START:])
    return out


def test_pipeline_off_is_the_oracle(gpu, oracle, runs):
    s = nf.pipeline_scenario()
    want = sorted(nf.oracle_pdus(oracle, s["tone"]))
    got = sorted((p["freq"], bytes(p["octets"])) for p in runs["off"]["pdus"])
    assert got == want
    mid = [o for f, o in got if f == FREQS[MID]]
    assert nf.delivered(mid, s["sent_mid"]) <= 1                # the carrier defeats the middle channel ...
    clean = nf.oracle_pdus(oracle, s["clean"])
    assert nf.delivered([o for f, o in clean if f == FREQS[MID]], s["sent_mid"]) == 6       # ... which decodes all six without it


def test_pipeline_on_is_the_host_model(gpu, oracle, runs):
    s = nf.pipeline_scenario()
    on, off, (model, recs) = runs["on"], runs["off"], runs["model"]
    nblk = runs["nblk"]
    # the canceller leaves the channelizer's output alone
    for c in range(3):
        assert all(same(a, b) for a, b in zip(on["rows"][c], off["rows"][c])), c
    # every block's row the demodulator read: the model's for the middle channel, the channelizer's for the others
    for b in range(nblk - START):
        assert same(on["nrows"][MID][b], model[b]), (b, int((bits(on["nrows"][MID][b]) != bits(model[b])).sum()))
        for c in (0, 2):
            assert same(on["nrows"][c][b], on["rows"][c][START + b]), (b, c)
    assert not same(on["nrows"][MID][-1], on["rows"][MID][-1])
    # the middle channel's PDUs: the oracle's demodulator on the model's output, and all six
    ch = oracle.Channel(FS, CF, FREQS[MID], want_channelizer=False)
    for row in on["rows"][MID][:START] + model:
        ch.process_baseband(row)
    want = [(p["mode"], bytes(p["octets"])) for p in ch.pdus]
    ch.close()
    got = [(p["mode"], bytes(p["octets"])) for p in on["pdus"] if p["freq"] == FREQS[MID]]
    assert got == want and nf.delivered([o for _, o in got], s["sent_mid"]) == 6
    # the other channels' PDUs are those of the off run
    others = lambda pdus: pdu_key(p for p in pdus if p["freq"] != FREQS[MID])
    assert others(on["pdus"]) == others(off["pdus"]) and len(others(on["pdus"])) == 2
    # the record
    st = on["stats"]
    last = recs[-1]
    assert st["blocks"] == nblk - START == last["blocks"] and st["resets"] == 0 == last["resets"]
    assert (f32_bits(st["last_in_power"]), f32_bits(st["last_out_power"]), f32_bits(st["tap_energy"])) == (last["in_power"], last["out_power"], last["tap_energy"])
    assert 0.02 < float(st["tap_energy"]) < 0.06                # one tracked tone: about 1 / L


# ---------------------------------------------------------------- 3. cuts change nothing

def test_cuts_change_nothing(gpu, runs, monkeypatch):
    """polled after every block; pushed with one sync at the end, a demodulator launch per block; the same with the default batching:
    PDUs, frame quality records and the rows of the newest half are identical, and the rows are the model's"""
    s = nf.pipeline_scenario()
    x, nblk = s["tone"], runs["nblk"]
    model = runs["model"][0]
    got = {}
    for name, batch, poll_each in (("polled", None, True), ("batch 1", "1", False), ("default", None, False)):
        if batch is None:
            monkeypatch.delenv("HFDL_GPU_DEMOD_BATCH", raising=False)
        else:
            monkeypatch.setenv("HFDL_GPU_DEMOD_BATCH", batch)
        fe = gpu.Frontend(FS, CF, FREQS)
        fe.quality_enable()
        pdus = []
        for b in range(nblk):
            if b == START:
                fe.notch_enable(MU, [MID])
            fe.push_block(x[b * N:(b + 1) * N])
            if poll_each:
                pdus += fe.poll_pdus()
        pdus += fe.poll_pdus()
        quality = sorted(q["raw"] for q in fe.quality_read(wait=True)[0])       # (the order of the records across channels follows the launches)
        last = fe.read_tap(TAP_NOTCH_OUT, MID)
        assert same(last, model[-1]), name
        if not poll_each:
            # the newest half holds several blocks: one launch walked them all, and every row is the model's
            back = 1
            while True:
                try:
                    row = fe.read_tap(TAP_NOTCH_OUT, MID, back)
                except gpu.GpuError:
                    break
                assert same(row, model[-1 - back]), (name, back)
                back += 1
            assert back > 1, name
        st = fe.notch_stats(MID)
        got[name] = (pdu_key(pdus), quality, bits(last).tobytes(), st)
        fe.close()
    for name in ("batch 1", "default"):
        print("%s against polled: PDUs %s, %d of %d quality records the same, last row %s, record %s" % (
            name, got[name][0] == got["polled"][0], len(set(got[name][1]) & set(got["polled"][1])), len(got["polled"][1]),
            got[name][2] == got["polled"][2], got[name][3] == got["polled"][3]))
    assert got["polled"] == got["batch 1"] == got["default"]
    assert got["polled"][0] == pdu_key(runs["on"]["pdus"]) and len(got["polled"][1]) == len(got["polled"][0]) == 8
    assert got["polled"][3]["blocks"] == nblk - START and got["polled"][3]["resets"] == 0


# ---------------------------------------------------------------- 4. the export is untouched

def test_export_still_reads_the_channelizer(gpu, runs):
    s = nf.pipeline_scenario()
    nblk = 6
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.export_enable([MID], ring_blocks=8)
    first, _ = run_blocks(fe, s["tone"], START, [MID])
    fe.notch_enable(MU, [MID])
    rows, nrows = run_blocks(fe, s["tone"], nblk - START, [MID], [MID], first=START)
    rows = first[MID] + rows[MID]
    samples, counts, _, _, blocks, _ = fe.export_read(0, wait=True)
    assert list(blocks) == list(range(nblk))
    for b in range(nblk):
        assert counts[b, 0] == len(rows[b])
        assert same(samples[b, 0, :counts[b, 0]], rows[b]), b
        assert same(rows[b], runs["on"]["rows"][MID][b]), b
    for b in range(nblk - START):
        assert same(nrows[MID][b], runs["model"][0][b]), b
    assert not same(nrows[MID][-1], rows[-1])
    fe.close()


# ---------------------------------------------------------------- 5. enable in mid-stream, retune

def test_enable_in_mid_stream_and_retune(gpu, exe, runs):
    """enable for channels 1 and 0 after K blocks: the model restarted at block K gives the rows; the blocks before K are the off run's.
    Then the middle channel is retuned before block R: its canceller starts from zero there, channel 0's runs on.  The same calls without
    a sync between the pushes decode the same PDUs: the enable closes the half being filled."""
    s = nf.pipeline_scenario()
    x = s["tone"]
    K, R, nblk = 3, 20, 46
    new_freq = FREQS[MID] + 4000
    fe = gpu.Frontend(FS, CF, FREQS)
    with pytest.raises(gpu.GpuError):
        fe.notch_stats(MID)                                      # never enabled
    fe.notch_enable(0.0)                                         # off before it was ever on: nothing happens
    for bad in dict(mu=0.06), dict(mu=float("nan")), dict(mu=MU, channels=[3]), dict(mu=MU, channels=[-1]), dict(mu=MU, channels=[1, 1]):
        with pytest.raises(gpu.GpuError):
            fe.notch_enable(**bad)
    before, _ = run_blocks(fe, x, K, range(3))
    with pytest.raises(gpu.GpuError):
        fe.read_tap(TAP_NOTCH_OUT, MID)                          # off
    fe.notch_enable(MU, [MID, 0])
    with pytest.raises(gpu.GpuError):
        fe.notch_stats(2)                                        # not selected
    rows1, nrows1 = run_blocks(fe, x, R - K, range(3), range(3), first=K)
    fe.retune(MID, new_freq)
    rows2, nrows2 = run_blocks(fe, x, nblk - R, range(3), range(3), first=R)
    pdus = fe.poll_pdus()
    stats = {c: fe.notch_stats(c) for c in (0, MID)}
    fe.close()
    for c in range(3):
        assert all(same(a, b) for a, b in zip(before[c] + rows1[c], runs["off"]["rows"][c])), c
    ch0, recs0 = model_rows(exe, rows1[0] + rows2[0])
    mid1, _ = model_rows(exe, rows1[MID])
    mid2, recs2 = model_rows(exe, rows2[MID])
    for i, row in enumerate(nrows1[0] + nrows2[0]):
        assert same(row, ch0[i]), i
    for i, row in enumerate(nrows1[MID]):
        assert same(row, mid1[i]), i
    for i, row in enumerate(nrows2[MID]):
        assert same(row, mid2[i]), i
    for i, row in enumerate(nrows1[2] + nrows2[2]):
        assert same(row, (rows1[2] + rows2[2])[i]), i
    assert not same(rows2[MID][-1], runs["off"]["rows"][MID][nblk - 1])                  # the retuned channel is another channel
    # the records count from the enable; a retune restarts the state, not the record
    assert stats[0]["blocks"] == stats[MID]["blocks"] == nblk - K and stats[0]["resets"] == stats[MID]["resets"] == 0
    assert f32_bits(stats[0]["tap_energy"]) == recs0[-1]["tap_energy"] and f32_bits(stats[MID]["tap_energy"]) == recs2[-1]["tap_energy"]
    assert f32_bits(stats[MID]["last_out_power"]) == recs2[-1]["out_power"]
    # the same calls, nothing synced in between
    fe = gpu.Frontend(FS, CF, FREQS)
    for b in range(nblk):
        if b == K:
            fe.notch_enable(MU, [MID, 0])
        if b == R:
            fe.retune(MID, new_freq)
        fe.push_block(x[b * N:(b + 1) * N])
    assert pdu_key(fe.poll_pdus()) == pdu_key(pdus)
    assert same(fe.read_tap(TAP_NOTCH_OUT, MID), mid2[-1]) and same(fe.read_tap(TAP_NOTCH_OUT, 0), ch0[-1])
    # turned off again: the demodulator reads the channelizer's rows, the tap is refused, the record stays
    fe.notch_enable(0.0)
    fe.push_block(x[nblk * N:(nblk + 1) * N])
    with pytest.raises(gpu.GpuError):
        fe.read_tap(TAP_NOTCH_OUT, MID)
    assert fe.notch_stats(0)["blocks"] == nblk - K
    fe.close()


# ---------------------------------------------------------------- 6. two receivers

def test_two_receivers(gpu, runs):
    """two receivers fed the tone stream, the middle channel of each selected (global indices 1 and 4): both decode all six; the
    other four channels' PDUs are those of the same front end with the canceller off"""
    s = nf.pipeline_scenario()
    x, nblk = s["tone"], runs["nblk"]
    rx = [(CF, FREQS), (CF, FREQS)]
    got = {}
    for name, sel in (("off", None), ("on", [MID, 3 + MID])):
        fe = gpu.MultiFrontend(FS, rx)
        for b in range(nblk):
            if sel and b == START:
                fe.notch_enable(MU, sel)
            fe.push_blocks([x[b * N:(b + 1) * N]] * 2)
        got[name] = fe.poll_pdus()
        if sel:
            last = [fe.read_tap(TAP_NOTCH_OUT, c) for c in sel]
            assert same(last[1], last[0]) and not same(last[0], fe.read_tap(TAP_CHAN_OUT, MID))
            st = [fe.notch_stats(c) for c in sel]
            assert st[0] == st[1] and st[0]["blocks"] == nblk - START and st[0]["resets"] == 0
            with pytest.raises(gpu.GpuError):
                fe.notch_stats(0)
        fe.close()
    key = lambda pdus, keep: sorted((p["channel"], p["sample_index"], bytes(p["octets"])) for p in pdus if keep(p["channel"]))
    assert key(got["on"], lambda c: c % 3 != MID) == key(got["off"], lambda c: c % 3 != MID) and len(key(got["on"], lambda c: c % 3 != MID)) == 4
    for c in (MID, 3 + MID):
        assert nf.delivered([bytes(p["octets"]) for p in got["on"] if p["channel"] == c], s["sent_mid"]) == 6
        assert nf.delivered([bytes(p["octets"]) for p in got["off"] if p["channel"] == c], s["sent_mid"]) <= 1


# ---------------------------------------------------------------- 7. push_baseband

def test_push_baseband_goes_through_the_canceller(gpu, runs):
    """the device's own channelizer rows fed back through push_baseband: canceller on = the host model's rows with the canceller off"""
    nblk = 46
    rows, model = {c: r[START:] for c, r in runs["on"]["rows"].items()}, runs["model"][0]
    got = {}
    for name in ("on", "model"):
        fe = gpu.Frontend(FS, CF, FREQS)
        if name == "on":
            fe.notch_enable(MU, [MID])
        for b in range(nblk):
            fe.push_baseband([rows[0][b], rows[MID][b] if name == "on" else model[b], rows[2][b]])
            if name == "on":
                assert same(fe.read_tap(TAP_NOTCH_OUT, MID), model[b]), b
        got[name] = pdu_key(fe.poll_pdus())
        fe.close()
    assert got["on"] == got["model"] and len([p for p in got["on"] if p[0] == FREQS[MID]]) >= 1


# ---------------------------------------------------------------- 8. the first block of a front end

def test_start_up_ramp_costs_one_reset(gpu, exe):
    """enabled before the first block (the module's text): the device is the model's row for row all the same, and both count one
    reset, in row 0, after which the taps settle as they do anywhere else"""
    prog, work = exe
    s = nf.pipeline_scenario()
    nblk = 6
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.notch_enable(MU, [MID])
    rows, nrows = run_blocks(fe, s["tone"], nblk, [MID], [MID])
    st = fe.notch_stats(MID)
    fe.close()
    y, recs, summary = nf.host_stream(prog, work, np.concatenate(rows[MID]), [len(r) for r in rows[MID]], MU)
    cuts = np.cumsum([len(r) for r in rows[MID]])[:-1]
    for b, want in enumerate(np.split(y, cuts)):
        assert same(nrows[MID][b], want), b
    assert [r["resets"] for r in recs] == [1] * nblk and summary["finite"]
    assert np.array([recs[0]["tap_energy"]], np.uint32).view(np.float32)[0] > 4.0
    assert (st["blocks"], st["resets"], f32_bits(st["tap_energy"])) == (nblk, 1, recs[-1]["tap_energy"])
    assert 0.02 < float(st["tap_energy"]) < 0.06
