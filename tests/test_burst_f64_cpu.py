"""CPU tests of the burst decoder's float64 / int64 model (tests/fec_model.py) and of everything that can be compared with it without a
GPU: the reference's compiled libfec (golden files), the oracle's restatement, the product's soft de-mapper compiled for the host
(tests/hostsim), the generator's closed-form interleaver -- and nine wrong variants of the model, each of which the committed frame set
(tests/burst_frames.py) must tell from the right one.  tests/test_gpu_burst_f64.py compares the kernels with the same model on the
same frames."""
import ctypes as C
import os

import numpy as np
import pytest

import burst_frames as bf
import fec_model as fm
import hfdl_synth as synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def frame_set():
    """(frames, model answers).  A condition of every test that uses cleared frames: at most 2 % of their symbols were redrawn."""
    redrawn, total = bf.redraw_share()
    print("redrawn %d of %d symbols (%.3f %%)" % (redrawn, total, 100.0 * redrawn / total))
    assert redrawn <= 0.02 * total
    return bf.frames(), bf.answers()


def _by_size(cases):
    """[(nbits, soft, want)] -> the model's octets (libfec bit order), frames of one size decoded side by side."""
    got = [None] * len(cases)
    for nbits in sorted({c[0] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c[0] == nbits]
        out = fm.viterbi_octets(np.stack([cases[i][1] for i in idx]), nbits)
        for k, i in enumerate(idx):
            got[i] = out[k]
    return got


def test_viterbi_model_equals_reference_libfec():
    """The model's Viterbi decoder against all three golden files (the reference's own viterbi27_port.c, compiled unmodified): the
    eight frame sizes clean, noisy and random; random input at four sizes; and every size 1 .. 130 plus 539, 541, 7559, 7561."""
    cases = []
    z = np.load(os.path.join(GOLD, "viterbi_ref.npz"))
    for mode in range(8):
        i = 0
        while "m%d_c%d_soft" % (mode, i) in z:
            cases.append((fm.sizes(mode)["nbits"], z["m%d_c%d_soft" % (mode, i)], z["m%d_c%d_out" % (mode, i)]))
            i += 1
    z = np.load(os.path.join(GOLD, "viterbi_live_ref.npz"))
    for nbits in (540, 1260, 3240, 7560):
        for i in range(3):
            cases.append((nbits, z["n%d_c%d_soft" % (nbits, i)], z["n%d_c%d_out" % (nbits, i)]))
    ragged = fm.ragged_cases()
    assert len(ragged) == 264 and {c[0] for c in ragged} == set(range(1, 131)) | {539, 541, 7559, 7561}
    cases += ragged
    assert len(cases) >= 18 + 12 + 264
    for c, got in zip(cases, _by_size(cases)):
        assert bytes(got) == bytes(c[2]), c[0]


def test_oracle_viterbi_equals_ragged_golden(oracle):
    for nbits, soft, want in fm.ragged_cases():
        assert bytes(oracle.viterbi27(soft, nbits)) == bytes(want), nbits


def test_interleaver_walk(oracle):
    """The model's cursor walk is a permutation of the table for all 8 modes, equals the oracle's maps, and equals the closed form that
    the kernel and the generator use (hfdl_synth.interleave_maps): row = k mod 40, column = (k div 40 - shift * k) mod columns on the
    way in; row = 9k mod 40, column = k div 40 on the way out."""
    for mode in range(8):
        total = fm.sizes(mode)["coded"]
        push, pop = fm.walk(mode)
        assert np.array_equal(np.sort(push), np.arange(total)) and np.array_equal(np.sort(pop), np.arange(total)), mode
        o_push, o_pop = np.zeros(total, np.int32), np.zeros(total, np.int32)
        oracle.lib().orc_deinterleave_maps(mode, o_push.ctypes.data, o_pop.ctypes.data)
        assert np.array_equal(push, o_push) and np.array_equal(pop, o_pop), mode
        c_push, c_pop = synth.interleave_maps(mode)
        assert np.array_equal(push, c_push) and np.array_equal(pop, c_pop), mode


def test_clean_frames_round_trip():
    """What the generator encodes, the model decodes: all 8 modes, both masks, noiseless symbols exactly on the constellation."""
    rng = np.random.default_rng(31)
    for mode in range(8):
        pdus = [synth.make_pdu(rng, mode) for _ in (0, 1)]
        syms = [synth.encode_data_symbols(p, mode) * (1 - 2 * mask) for mask, p in enumerate(pdus)]
        for p, a in zip(pdus, fm.decode_many(mode, syms, [0, 1])):
            assert a["octets"][:len(p)] == p, mode


def test_frame_set_is_what_it_says(frame_set):
    frames, answers = frame_set
    assert len(frames) == 8 * 2 * 5 + 4 * 2
    for mode in range(8):
        for mask in (0, 1):
            kinds = [f["kind"] for f in frames if f["mode"] == mode and f["mask"] == mask]
            assert kinds == list(bf.KINDS[:5]) + (["zeros"] if fm.sizes(mode)["arity"] == 1 else [])
    for f, a in zip(frames, answers):
        if f["cleared"]:
            assert a["m_int"].min() >= fm.D_INT and a["m_ang"].min() >= fm.D_ANG
        assert f["cleared"] or f["kind"] == "zeros" or (f["kind"] == "tiny" and fm.sizes(f["mode"])["arity"] == 3)
        if f["pdu"] is not None:                                         # clean and noisy frames still carry their PDU
            assert a["octets"][:len(f["pdu"])] == f["pdu"]
    # the set leaves the Viterbi decoder frames it cannot repair (no slack hides a wrong soft byte) and frames with clamped and unclamped bytes
    vin = np.concatenate([a["vin"] for a in answers])
    assert 0.05 < np.mean((vin > 0) & (vin < 255)) < 0.95


def test_oracle_equals_model_on_the_frame_set(frame_set, oracle):
    """orc_user_data_soft and orc_decode_user_data against the model: Viterbi input and octets identical, no exclusions."""
    for f, a in zip(*frame_set):
        if not f["model_exact"]:
            continue
        assert np.array_equal(oracle.user_data_soft(f["mode"], f["symbols"], f["mask"]), a["vin"]), (f["mode"], f["mask"], f["kind"])
        assert bytes(oracle.decode_user_data(f["mode"], f["symbols"], f["mask"])) == a["octets"], (f["mode"], f["mask"], f["kind"])


def test_oracle_split_keeps_decode_user_data(oracle):
    """orc_decode_user_data = orc_user_data_soft + Viterbi + octet reversal, also where the model is not asked (tiny 8-PSK amplitudes)."""
    for f in bf.frames():
        vin = oracle.user_data_soft(f["mode"], f["symbols"], f["mask"])
        nbits = len(vin) // 2
        assert nbits == fm.sizes(f["mode"])["nbits"]
        want = np.packbits(np.unpackbits(oracle.viterbi27(vin, nbits), bitorder="big"), bitorder="little")
        assert bytes(oracle.decode_user_data(f["mode"], f["symbols"], f["mask"])) == bytes(want)


def test_product_soft_demap_on_the_host_equals_model(frame_set):
    """sim_psk_soft -- the product's psk_soft (csrc/demod_logic.h) compiled for the host -- against the model's float64 de-mapper on
    every symbol of the frame set: soft bytes identical, no exclusions."""
    from test_host_logic_cpu import build_sim
    H = build_sim("libhostsim.so", [])
    H.sim_psk_soft_batch.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    for f, a in zip(*frame_set):
        if not f["model_exact"]:
            continue
        sz = fm.sizes(f["mode"])
        flip = ((1.0 - 2.0 * fm.scrambler(sz["nsym"])) * (-1.0 if f["mask"] else 1.0)).astype(np.float32)
        x = np.ascontiguousarray(f["symbols"].view(np.float32).reshape(-1, 2) * flip[:, None])          # the kernel's own fp32 product
        soft = np.zeros((sz["nsym"], sz["arity"]), np.uint8)
        H.sim_psk_soft_batch(sz["arity"], x.ctypes.data, sz["nsym"], soft.ctypes.data)
        assert np.array_equal(soft, a["soft"]), (f["mode"], f["mask"], f["kind"])


@pytest.mark.parametrize("name", list(fm.VARIANTS))
def test_wrong_variant_is_seen(frame_set, name):
    """Each deliberate mistake in the model changes the Viterbi input of the frame set (the two Viterbi mistakes: the octets).  A test
    that compares a kernel with the model on these frames would therefore see the same mistake in the kernel."""
    frames, answers = frame_set
    v = fm.VARIANTS[name]
    if "tie_ge" in v or "lookahead" in v:
        changed = 0
        for mode in range(8):
            idx = [i for i, f in enumerate(frames) if f["mode"] == mode]
            out = fm.viterbi_octets(np.stack([answers[i]["vin"] for i in idx]), fm.sizes(mode)["nbits"], True, v)
            changed += sum(out[k].tobytes() != answers[i]["octets"] for k, i in enumerate(idx))
    else:
        changed = sum(not np.array_equal(fm.soft_stage(f["mode"], f["symbols"], f["mask"], v)[0], a["vin"]) for f, a in zip(frames, answers))
    print("%s: %d of %d frames differ" % (name, changed, len(frames)))
    assert changed > 0
