"""The frame set of tests/test_burst_f64_cpu.py and tests/test_gpu_burst_f64.py (seeded; the same frames in both), and the model's
answers for it, computed once per process.

For every mode and both masks: a clean frame, coded + noise as in test_burst_decode_bit_exact, points anywhere on the plane
(|x| in 0.2 .. 1.6: no slack left for the Viterbi decoder), saturating amplitudes (|x| = 50), tiny amplitudes (1e-20) and, for BPSK,
exact zeros.  Every frame but the ones named below goes through fec_model.clear(), which redraws the symbols that sit where fp32
rounding could decide a byte; `cleared` says so.

Not cleared, because no draw can clear them:
 * exact zeros (BPSK): every soft value is 127 + 0, exactly, in any precision -- compared with the model all the same;
 * tiny amplitudes in 8-PSK: the symbol is 1e-20 from the centre, so the squared distances to the nearest point and its neighbours
   differ by less than the rounding of the fp32 constellation table itself (2 * 0.70710677^2 = 0.99999994 against 1), and the soft values
   of the bits those neighbours decide are 127 +- 1e-5 in fp32: the table's rounding picks 126 or 127.  Those two frames per mask are
   compared with the ORACLE (same fp32 arithmetic, same table), not with the float64 model: `model_exact` is False for them.
"""
import numpy as np

import fec_model as fm
import hfdl_synth as synth

KINDS = ("clean", "noise", "plane", "saturating", "tiny", "zeros")
SEED = 20261018

_frames = None
_answers = None


def _points(rng, n, arity, radius):
    """n points of modulus radius(n), at any angle (BPSK too: the imaginary part must not matter)."""
    return (radius(n) * np.exp(2j * np.pi * rng.random(n))).astype(np.complex64)


def frames():
    """[dict(mode, mask, kind, symbols complex64, cleared, model_exact, redrawn, pdu)], in a fixed order."""
    global _frames
    if _frames is not None:
        return _frames
    rng = np.random.default_rng(SEED)
    out = []
    for mode in range(8):
        sz = fm.sizes(mode)
        n, arity = sz["nsym"], sz["arity"]
        for mask in (0, 1):
            sign = 1 - 2 * mask
            for kind in KINDS:
                pdu = None
                if kind in ("clean", "noise"):
                    pdu = synth.make_pdu(rng, mode)
                    base = synth.encode_data_symbols(pdu, mode).astype(np.complex128) * sign
                    if kind == "clean":        # noiseless at an amplitude of its own per symbol: exactly +-1 would put every BPSK '1' ON the integer 255
                        draw = lambda idx, base=base: base[idx] * rng.uniform(0.6, 0.95, len(idx))
                    else:
                        draw = lambda idx, base=base: base[idx] * np.exp(1j * rng.normal(0, 0.08, len(idx))) + \
                            0.12 * (rng.standard_normal(len(idx)) + 1j * rng.standard_normal(len(idx)))
                elif kind == "plane":
                    draw = lambda idx: _points(rng, len(idx), arity, lambda k: rng.uniform(0.2, 1.6, k))
                elif kind == "saturating":
                    draw = lambda idx: _points(rng, len(idx), arity, lambda k: np.full(k, 50.0))
                elif kind == "tiny":
                    draw = lambda idx: _points(rng, len(idx), arity, lambda k: np.full(k, 1e-20))
                elif arity == 1:
                    draw = lambda idx: np.zeros(len(idx), np.complex64)
                else:
                    continue
                s = np.asarray(draw(np.arange(n)), np.complex64)
                cleared = not (kind == "zeros" or (kind == "tiny" and arity == 3))
                redrawn = fm.clear(s, arity, draw) if cleared else 0
                out.append(dict(mode=mode, mask=mask, kind=kind, symbols=s, cleared=cleared, model_exact=cleared or kind == "zeros",
                                redrawn=redrawn, pdu=pdu))
    _frames = out
    return out


def answers():
    """The model's dict(vin, octets, soft, m_int, m_ang) of every frame, in frames() order (the Viterbi decoder runs once per mode)."""
    global _answers
    if _answers is None:
        fr = frames()
        _answers = [None] * len(fr)
        for mode in range(8):
            idx = [i for i, f in enumerate(fr) if f["mode"] == mode]
            for i, a in zip(idx, fm.decode_many(mode, [fr[i]["symbols"] for i in idx], [fr[i]["mask"] for i in idx])):
                _answers[i] = a
    return _answers


def redraw_share():
    """(symbols redrawn, symbols in cleared frames)."""
    fr = [f for f in frames() if f["cleared"]]
    return sum(f["redrawn"] for f in fr), sum(len(f["symbols"]) for f in fr)
