"""The burst decoder's back end stated plainly: descrambler, soft de-map, 40-row de-interleaver, rate-1/4 combine,
K = 7 Viterbi, octet reversal.  numpy only, float64 / int64 throughout; nothing here comes from the product, the oracle or the
generator -- only the mode parameters and the descrambler's numbers are read from tests/golden/hfdl_constants.json.

It is the reference of tests/test_burst_f64_cpu.py and tests/test_gpu_burst_f64.py: the kernel's Viterbi INPUT and its octets are
compared with this model byte for byte.  A byte-exact comparison of an fp32 kernel with a float64 model is possible because the model
also says how far every input is from a point where rounding decides the byte (the margins below), and the tests draw their inputs
away from those points (clear()).

Every function takes a `v` dictionary of deliberate mistakes (VARIANTS): the CPU tests show that the committed frame set tells each
of them from the right model.
"""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_K = json.load(open(os.path.join(_HERE, "golden", "hfdl_constants.json")))
MODES = [tuple(m) for m in _K["frame_params"]["modes"]]          # (bits per symbol, data segments, code rate 1/r, push column shift)
_SCR = _K["descrambler"]
ROWS, POP_ROW_STEP, SYMBOLS_PER_SEGMENT = 40, 9, 30

D_INT, D_ANG = 2e-3, 1e-4          # clear()'s thresholds: see margins()

# the nine wrong variants of tests/test_burst_f64_cpu.py, as keyword sets for `v`
VARIANTS = {
    "column shift + 1 (mode 2)": dict(shift_delta={2: +1}),
    "column shift - 1 (mode 5)": dict(shift_delta={5: -1}),
    "pop row step 11": dict(pop_step=11),
    "combine rounds up": dict(combine_up=True),
    "8-PSK soft bits reversed": dict(psk8_reversed=True),
    "neighbours at +-2": dict(neighbour=2),
    "scrambler restart at 127": dict(scr_restart=127),
    "BPSK sign": dict(bpsk_sign=+1.0),
    "tie rule >=": dict(tie_ge=True),
    "look-ahead 0": dict(lookahead=0),
}


def sizes(mode):
    arity, segments, rate, shift = MODES[mode]
    nsym = segments * SYMBOLS_PER_SEGMENT
    coded = nsym * arity
    vin = coded // 2 if rate == 4 else coded
    return dict(arity=arity, rate=rate, shift=shift, nsym=nsym, coded=coded, cols=coded // ROWS, vin=vin, nbits=vin // 2)


# ---------------------------------------------------------------- descrambler

def scrambler(n, v=None):
    """Output of the 15-stage shift register with feedback polynomial 1 + D + D^15: b[n] = b[n-1] xor b[n-15] (the delays are the set
    bits of `genpoly`, counted from 1), started from `init` (bit i of it = b[-1-i]) and started again every `seq_len` = 120 symbols."""
    restart = (v or {}).get("scr_restart", _SCR["seq_len"])
    m, poly, init = _SCR["numbits"], _SCR["liquid_1_6_and_later"]["genpoly"], _SCR["liquid_1_6_and_later"]["init"]
    delays = [i + 1 for i in range(m) if (poly >> i) & 1]
    past = [(init >> i) & 1 for i in range(m)]                  # past[i] = b[-1-i]
    period = []
    for _ in range(restart):
        b = 0
        for d in delays:
            b ^= past[d - 1]
        period.append(b)
        past = [b] + past[:-1]
    return np.resize(np.array(period, np.uint8), n)


# ---------------------------------------------------------------- soft de-map

def _ulp32(x):
    """Spacing of float32 at magnitude x (x > 0)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 23)


def _byte(val):
    """float -> soft byte: truncate toward zero, clamp to 0 .. 255."""
    return np.clip(np.trunc(val), 0, 255).astype(np.uint8)


def _int_margin(val, scale):
    """How far `val` is from the integer that decides its byte, in units in which D_INT applies.

    The bytes change at the integers 1 .. 255 (everything below 1 is byte 0, everything from 255 up is byte 255), so the distance is
    taken to the nearest of those.  D_INT = 2e-3 is derived for intermediate values below 1024, whose fp32 spacing is at most 2^-14:
    eight rounded operations on either side of the comparison, times four.  Where the de-mapper's intermediate products are larger
    (`scale`: the squared distances times 16 * gamma at high amplitudes), the fp32 error grows with their spacing, and the distance
    is divided by that growth -- never by less than 1 -- so that one threshold serves every amplitude."""
    near = np.clip(np.rint(val), 1, 255)
    growth = np.maximum(1.0, _ulp32(scale) / 2.0 ** -14)
    return np.abs(val - near) / growth


def demap(x, arity, v=None):
    """x: complex128 symbols, already descrambled.  Returns (soft [n, arity] uint8 with the symbol's MSB first, m_int [n], m_ang [n])."""
    v = v or {}
    x = np.asarray(x, np.complex128)
    n = len(x)
    if arity == 1:
        t = v.get("bpsk_sign", -1.0) * 128.0 * x.real
        val = t + 127.0
        m_int = _int_margin(val, np.maximum(np.abs(t), 127.0))
        # |t| below 2^-20: t + 127 is 127 exactly in fp32 and in float64 alike (half a spacing of fp32 at 127 is 2^-18) -- no rounding decides
        m_int = np.where(np.abs(t) < 2.0 ** -20, 0.5, m_int)
        return _byte(val)[:, None], m_int, np.full(n, np.inf)
    M = 1 << arity
    step = 2 * np.pi / M
    ang = np.angle(x)
    r = np.mod(ang + step / 2, step)
    m_ang = np.minimum(r, step - r)                                  # angular distance from the nearest decision boundary
    lin = np.floor(np.mod(ang + step / 2, 2 * np.pi) / step).astype(np.int64) % M        # nearest constellation point, counted round the circle
    gray = lambda l: l ^ (l >> 1)
    bit = lambda s, k: (s >> (arity - 1 - k)) & 1                      # bit k of a symbol, MSB first
    if arity == 2:
        s = gray(lin)
        soft = np.stack([bit(s, k) * 255 for k in range(arity)], axis=1).astype(np.uint8)
        return soft, np.full(n, np.inf), m_ang
    pts = np.exp(2j * np.pi * np.arange(M) / M)
    gamma, far = 1.2 * M, 4.0
    nb = v.get("neighbour", 1)
    cand = np.stack([lin, (lin - nb) % M, (lin + nb) % M], axis=1)     # the nearest point and its two ring neighbours
    d = np.abs(x[:, None] - pts[cand]) ** 2
    sym = gray(cand)
    soft = np.zeros((n, arity), np.uint8)
    m_int = np.full(n, np.inf)
    for k in range(arity):
        one = bit(sym, k) == 1
        # the nearest point sets the side its bit is on, the other side starts at `far`; then a neighbour may undercut its own side
        d0 = np.where(one[:, 0], far, d[:, 0])
        d1 = np.where(one[:, 0], d[:, 0], far)
        for j in (1, 2):
            d0 = np.where(~one[:, j], np.minimum(d0, d[:, j]), d0)
            d1 = np.where(one[:, j], np.minimum(d1, d[:, j]), d1)
        val = (d0 - d1) * gamma * 16.0 + 127.0
        soft[:, k] = _byte(val)
        m_int = np.minimum(m_int, _int_margin(val, np.maximum(d0, d1) * gamma * 16.0))
    if v.get("psk8_reversed"):
        soft = soft[:, ::-1]
    return soft, m_int, m_ang


def margins(symbols, arity):
    """Per symbol: (m_int, m_ang).  m_int: distance of its unclamped soft values from an integer (see _int_margin); m_ang: angular
    distance from the nearest decision boundary (arity > 1).  Both are the same for x and -x, so the descrambler need not be known.

    Thresholds.  D_INT = 2e-3: a soft value is below 1024 in magnitude, fp32 spacing at most 6.1e-5; about eight rounded operations
    on either side make at most 5e-4; the threshold is four times that.  D_ANG = 1e-4 rad: the device's slicer and atan2f differ by
    about 1e-6 rad."""
    _, m_int, m_ang = demap(np.asarray(symbols, np.complex64).astype(np.complex128), arity)
    return m_int, m_ang


def clear(symbols, arity, redraw, d_int=D_INT, d_ang=D_ANG):
    """Redraw, in place, every symbol of the complex64 array whose margin is below the thresholds, until none is: redraw(idx) returns
    new symbols for the positions idx.  Returns how many symbols were redrawn (a symbol drawn twice counts twice)."""
    assert symbols.dtype == np.complex64
    total = 0
    for _ in range(64):
        m_int, m_ang = margins(symbols, arity)
        bad = np.flatnonzero((m_int < d_int) | (m_ang < d_ang))
        if len(bad) == 0:
            return total
        symbols[bad] = np.asarray(redraw(bad), np.complex64)
        total += len(bad)
    raise RuntimeError("clear(): %d symbols still below the thresholds after 64 rounds" % len(bad))


# ---------------------------------------------------------------- de-interleaver: the stateful walk

_walks = {}


def walk(mode, v=None):
    """(push, pop): table position (row * columns + column) of the k-th byte pushed and of the k-th byte popped, found by WALKING the
    cursor as the receiver does -- push: store, row + 1, after the last row back to row 0 and one column on, then `shift` columns
    back with one conditional wrap; pop: read, row + 9 modulo 40, one column on whenever the row comes back to 0.  Both start at (0, 0)."""
    v = v or {}
    sz = sizes(mode)
    shift = sz["shift"] + v.get("shift_delta", {}).get(mode, 0)
    step = v.get("pop_step", POP_ROW_STEP)
    key = (mode, shift, step)
    if key not in _walks:
        cols, total = sz["cols"], sz["coded"]
        push, pop = np.zeros(total, np.int64), np.zeros(total, np.int64)
        row = col = 0
        for k in range(total):
            push[k] = row * cols + col
            row += 1
            if row == ROWS:
                row = 0
                col += 1
            col -= shift
            if col < 0:
                col += cols
        row = col = 0
        for k in range(total):
            pop[k] = row * cols + (col % cols)          # a wrong row step can run past the last column; the right one never does
            row = (row + step) % ROWS
            if row == 0:
                col += 1
        _walks[key] = (push, pop)
    return _walks[key]


def combine(a, b, v=None):
    """Rate 1/4: every chip was sent twice; the mean of the two soft bytes, rounded down."""
    a, b = a.astype(np.int64), b.astype(np.int64)
    return ((a + b + (1 if (v or {}).get("combine_up") else 0)) // 2).astype(np.uint8)


# ---------------------------------------------------------------- Viterbi, K = 7, rate 1/2, polynomials 0x6d / 0x4f

def _parity(x):
    x = np.asarray(x, np.int64)
    p = np.zeros_like(x)
    while np.any(x):
        p ^= x & 1
        x = x >> 1
    return p


def viterbi(soft, nbits, v=None):
    """soft: uint8 [frames, 2 * nbits] (or one frame).  Returns the decoded bits, uint8 [frames, nbits].

    The textbook decoder with libfec's conventions: state = the last six input bits, newest in bit 0; state 2i and 2i+1 are reached
    from i and i+32; a branch costs (expected ^ received) summed over the two soft bytes, expected being 0 or 255; metrics are int64,
    all 63 at the start except state 0 (0); the path from i+32 wins only when it is STRICTLY cheaper.  Chainback starts in state 0 at
    the end and reads the decision for bit idx from the step `lookahead` = 6 further on -- the step at which bit idx has reached the top
    of the state -- with all-zero decisions past the last step."""
    v = v or {}
    look = v.get("lookahead", 6)
    soft = np.atleast_2d(np.asarray(soft)).astype(np.int64)
    F = soft.shape[0]
    assert soft.shape[1] == 2 * nbits
    i = np.arange(32)
    e0, e1 = 255 * _parity((2 * i) & 0x6d), 255 * _parity((2 * i) & 0x4f)
    metric = np.full((F, 64), 63, np.int64)
    metric[:, 0] = 0
    dec = np.zeros((nbits + look, F, 64), np.uint8)
    for t in range(nbits):
        bm = (e0 ^ soft[:, 2 * t, None]) + (e1 ^ soft[:, 2 * t + 1, None])
        lo, hi = metric[:, :32], metric[:, 32:]
        even_a, even_b = lo + bm, hi + (510 - bm)                      # into state 2i from i / from i+32
        odd_a, odd_b = lo + (510 - bm), hi + bm                        # into state 2i+1
        pick_e = even_a >= even_b if v.get("tie_ge") else even_a > even_b
        pick_o = odd_a >= odd_b if v.get("tie_ge") else odd_a > odd_b
        metric = np.empty_like(metric)
        metric[:, 0::2] = np.where(pick_e, even_b, even_a)
        metric[:, 1::2] = np.where(pick_o, odd_b, odd_a)
        dec[t, :, 0::2] = pick_e
        dec[t, :, 1::2] = pick_o
    bits = np.zeros((F, nbits), np.uint8)
    state = np.zeros(F, np.int64)
    rows = np.arange(F)
    for idx in range(nbits - 1, -1, -1):
        k = dec[idx + look, rows, state]
        state = (state >> 1) | (k.astype(np.int64) << 5)
        bits[:, idx] = k
    return bits


def viterbi_octets(soft, nbits, reverse=False, v=None):
    """ceil(nbits / 8) octets per frame: first decoded bit in the MSB as libfec leaves them, or every octet bit-reversed."""
    bits = viterbi(soft, nbits, v)
    return np.packbits(bits, axis=1, bitorder="little" if reverse else "big")


# ---------------------------------------------------------------- the whole back end

def soft_stage(mode, symbols, bitmask_lsb, v=None):
    """Symbols -> (vin, soft, m_int, m_ang): the bytes the Viterbi decoder is fed, the de-mapper's bytes [nsym, arity] and the margins."""
    sz = sizes(mode)
    x = np.asarray(symbols, np.complex64).astype(np.complex128)
    assert len(x) == sz["nsym"]
    flip = (1.0 - 2.0 * scrambler(sz["nsym"], v)) * (-1.0 if bitmask_lsb else 1.0)
    soft, m_int, m_ang = demap(x * flip, sz["arity"], v)
    push, pop = walk(mode, v)
    table = np.zeros(sz["coded"], np.uint8)
    table[push] = soft.reshape(-1)
    popped = table[pop]
    vin = combine(popped[0::2], popped[1::2], v) if sz["rate"] == 4 else popped
    return vin, soft, m_int, m_ang


def decode(mode, symbols, bitmask_lsb, v=None):
    """One frame: dict(vin, octets, soft, m_int, m_ang); octets as dumphfdl dispatches them (bit-reversed)."""
    return decode_many(mode, [symbols], [bitmask_lsb], v)[0]


def decode_many(mode, symbol_list, masks, v=None):
    """Frames of ONE mode; the Viterbi decoder walks them side by side."""
    stages = [soft_stage(mode, s, m, v) for s, m in zip(symbol_list, masks)]
    octets = viterbi_octets(np.stack([st[0] for st in stages]), sizes(mode)["nbits"], True, v)
    return [dict(vin=st[0], soft=st[1], m_int=st[2], m_ang=st[3], octets=octets[i].tobytes()) for i, st in enumerate(stages)]


def ragged_cases():
    """tests/golden/viterbi_ragged_ref.npz -> [(nbits, soft, octets)]: what the reference's compiled libfec decoded at sizes no frame has."""
    z = np.load(os.path.join(_HERE, "golden", "viterbi_ragged_ref.npz"))
    out, a, b = [], 0, 0
    for nbits in z["nbits"]:
        nbits = int(nbits)
        noct = (nbits + 7) // 8
        out.append((nbits, z["soft"][a:a + 2 * nbits], z["out"][b:b + noct]))
        a += 2 * nbits
        b += noct
    assert a == len(z["soft"]) and b == len(z["out"])
    return out
