"""burst_decode_kernel and hfdl_gpu_viterbi27 against the float64 / int64 model of tests/fec_model.py.

What the older tests cannot see: at their noise level the Viterbi decoder repairs what the stages in front of it get wrong, so a
de-interleaver position, a soft magnitude or the rate-1/4 rounding could be off without one octet changing.  Here the kernel's Viterbi
INPUT is read through the laboratory tap hfdl_gpu_lab_burst_soft -- burst_decode_kernel's own device function, stopped in front of the
decoder -- and compared with the model byte for byte, on frames that leave the decoder no slack (tests/burst_frames.py: the same seeded
frames tests/test_burst_f64_cpu.py uses, cleared of symbols where fp32 rounding could decide a byte).  And the Viterbi kernel runs at
sizes no HFDL frame has: every nbits 1 .. 130, both sides of 540 and 7560, many frames per launch, and the LDS limit."""
import numpy as np
import pytest

import burst_frames as bf
import fec_model as fm
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frame_set():
    redrawn, total = bf.redraw_share()
    print("redrawn %d of %d symbols (%.3f %%)" % (redrawn, total, 100.0 * redrawn / total))
    assert redrawn <= 0.02 * total                  # a condition of every test on cleared frames, not a measurement
    return bf.frames(), bf.answers()


def _tag(f):
    return (f["mode"], f["mask"], f["kind"])


def test_lab_tap_equals_model(gpu, oracle, frame_set):
    """The Viterbi input of every frame of the set, one launch: identical to the model's, byte for byte, no exclusions.  (The two
    tiny-amplitude 8-PSK frames per mask, which no draw can clear -- burst_frames.py says why -- are held to the oracle instead.)"""
    frames, answers = frame_set
    got = F.lab_burst_soft([f["symbols"] for f in frames], [f["mode"] for f in frames], [f["mask"] for f in frames])
    wrong = []
    for f, a, g in zip(frames, answers, got):
        want = a["vin"] if f["model_exact"] else oracle.user_data_soft(f["mode"], f["symbols"], f["mask"])
        assert len(g) == len(want), _tag(f)
        if not np.array_equal(g, want):
            wrong.append((_tag(f), int((g != want).sum()), int(np.abs(g.astype(int) - want.astype(int)).max())))
    assert not wrong, "frames whose Viterbi input differs (mode, mask, kind), bytes, largest step: %s" % wrong


def test_product_octets_equal_model_and_oracle(gpu, oracle, frame_set):
    """hfdl_gpu_burst_decode (the product library) on the same frames: octets identical to the model's and to the oracle's."""
    frames, answers = frame_set
    got = gpu.burst_decode([f["symbols"] for f in frames], [f["mode"] for f in frames], [f["mask"] for f in frames])
    for f, a, g in zip(frames, answers, got):
        assert g == bytes(oracle.decode_user_data(f["mode"], f["symbols"], f["mask"])), _tag(f)
        if f["model_exact"]:
            assert g == a["octets"], _tag(f)


def test_many_frames_in_one_launch(gpu, frame_set):
    """200 frames of mixed modes through one launch of each entry point (the older tests stop at 16): every result at its own index.
    The frames are drawn, with repeats, from the set, so the model's answers are already there."""
    frames, answers = frame_set
    exact = [i for i, f in enumerate(frames) if f["model_exact"]]
    pick = np.random.default_rng(8).choice(exact, 200)
    assert len({frames[i]["mode"] for i in pick}) == 8
    syms, modes, masks = [frames[i]["symbols"] for i in pick], [frames[i]["mode"] for i in pick], [frames[i]["mask"] for i in pick]
    octets = gpu.burst_decode(syms, modes, masks)
    vin = F.lab_burst_soft(syms, modes, masks)
    for k, i in enumerate(pick):
        assert octets[k] == answers[i]["octets"], (k, _tag(frames[i]))
        assert np.array_equal(vin[k], answers[i]["vin"]), (k, _tag(frames[i]))


def test_viterbi_ragged_sizes(gpu):
    """Every case of viterbi_ragged_ref.npz (the reference's compiled libfec at nbits 1 .. 130, 539, 541, 7559, 7561) through
    hfdl_gpu_viterbi27, one launch per size, bit-exact: the ragged end of the forward pass, the chainback head at every residue of 48,
    sizes below one 60-step trip and below the 6-step look-ahead, nbits no multiple of 8 or 6."""
    cases = fm.ragged_cases()
    assert len(cases) == 264
    wrong = []
    for nbits in sorted({c[0] for c in cases}):
        mine = [c for c in cases if c[0] == nbits]
        got = gpu.viterbi27(np.stack([c[1] for c in mine]), nbits)
        assert got.shape == (len(mine), (nbits + 7) // 8)
        wrong += [(nbits, k) for k, c in enumerate(mine) if bytes(got[k]) != bytes(c[2])]
    assert not wrong, wrong


def test_viterbi_ragged_many_frames(gpu):
    """nbits = 67 (odd, no multiple of 6 or 8, one full trip and a ragged one), 300 frames in one launch: the entry point's
    soft + f * 2 * nbits and its output stride of ceil(nbits / 8) octets, against the model."""
    rng = np.random.default_rng(67)
    nbits, nframes = 67, 300
    soft = rng.integers(0, 256, (nframes, 2 * nbits)).astype(np.uint8)
    soft[::3] = np.clip(255.0 * rng.integers(0, 2, soft[::3].shape) + rng.normal(0, 60, soft[::3].shape), 0, 255).astype(np.uint8)
    want = fm.viterbi_octets(soft, nbits)
    got = gpu.viterbi27(soft, nbits)
    assert got.shape == want.shape == (nframes, 9)
    assert [k for k in range(nframes) if bytes(got[k]) != bytes(want[k])] == []


def test_viterbi_lds_limit(gpu, oracle):
    """One decision word per step plus eight: 20472 bits fill the 160 KiB of LDS exactly and decode like the model and the oracle;
    20473 are refused with HFDL_GPU_ERANGE before anything is launched, and a valid call straight afterwards succeeds."""
    rng = np.random.default_rng(20472)
    nbits = 20472
    soft = rng.integers(0, 256, (1, 2 * nbits)).astype(np.uint8)
    want = fm.viterbi_octets(soft, nbits)[0]
    assert bytes(oracle.viterbi27(soft[0], nbits)) == bytes(want)
    assert bytes(gpu.viterbi27(soft, nbits)[0]) == bytes(want)
    with pytest.raises(gpu.GpuError, match=r"error -5\b"):
        gpu.viterbi27(np.zeros((1, 2 * (nbits + 1)), np.uint8), nbits + 1)
    assert bytes(gpu.viterbi27(soft[:, :2 * 540], 540)[0]) == bytes(fm.viterbi_octets(soft[:, :2 * 540], 540)[0])
