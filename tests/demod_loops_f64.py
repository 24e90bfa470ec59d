"""A float64 statement of the demodulator's back half: symbol-timing loop, carrier loop, equaliser, slicer, sampler and framer (numpy
only; a helper module, not a test).  It imports nothing from the product and nothing from oracle/; written from liquid-dsp's published
definitions of symsync_crcf, eqlms_cccf and modem (psk), and from the reference's src/hfdl.c:236-294 (Costas loop) and :696-891, :952-991
(per-sample loop, framer).  Integer logic (counters, bit sequences, the preamble thresholds in the reference's fp32 expression) is exact;
everything else is float64 on the fp32 constants of the reference.

Design (tables=None)
  kaiser(n, fc, As): h[i] = sinc(2 fc t) I0(beta sqrt(1 - (2 t / n)^2)) / I0(beta), t = i - (n - 1) / 2,
                     beta = 0.5842 (As - 21)^0.4 + 0.07886 (As - 21) for 21 < As <= 50 (the window argument 2 t / n as in demod_f64)
  matched bank       symsync_crcf_create_kaiser(k = 3, m = 3, beta, npfb = 16): H = 2 * 0.75 * kaiser(2 * 16 * 3 * 3 + 1, 0.75 / 48, 40);
                     branch b, tap j is H[b + 16 j], j < 18 (H[288] unused)
  derivative bank    dH[i] = H[i + 1] - H[i - 1] (indices mod 289), scaled by 0.06 / max_i |H[i] dH[i]|; same split
  loop filter        set_lf_bw(w = 0.001): alpha = 1 - w, beta = 0.22 w; b0 = beta / (1 - alpha / 2), a1 = -0.495 alpha / (1 - alpha / 2);
                     rate_adj = w / 2
  equaliser          eqlms_cccf_create_lowpass(15, 0.45): h0 = 2 * 0.45 * kaiser(15, 0.45, 40); mu = 0.1

Per matched-filter sample x (symsync_crcf_execute, one input), both 18-sample windows take x (w[0] newest), then
  while b < 16:   m = sum_j mf[b][j] w[j];  output y = m / 3
                  on every second output (a counter that starts at 0 after a reset reads 2): d = sum_j dmf[b][j] wd[j];
                      q = clip(Re(conj(m) d), -1, 1);  v0 = q - a1 v1;  q_hat = b0 v0;  v1 = v0;
                      rate += rate_adj q_hat;  del = rate + q_hat
                  tau += del;  b = round(16 tau) (half away from zero)
  tau -= 1;  b -= 16                      -> 0, 1 or 2 outputs
  reset: the MATCHED window only is cleared; rate = del = 3 / 2; tau = b = q = q_hat = v1 = counter = 0.
Per output y (a counter n of all outputs of the stream, never reset):
  phi += dphi;  phi > pi: phi -= 2 pi;  phi < -pi: phi += 2 pi;  r = y exp(-j phi)
  if |dphi| > 0.25 while searching for A1: phi = dphi = 0, timing loop reset
  equaliser push r (15 newest samples u[0] oldest, s2 = running sum of |u|^2: s2 += |r|^2 - |dropped|^2)
  n even: next output.  n odd, the on-time symbol:
  s = sum_i conj(w_i) u_i;  in training: w_i += mu conj(T - s) u_i / s2 (once 15 samples were pushed since the reset), T the next
  training symbol times the preamble's polarity
  slicer, arity 1: bit = Re s <= 0, point +-1.  Arity a, M = 2^a: theta = arg s - pi (1 - 1 / M) (+ 2 pi below -pi); a ladder of
  references 2^k pi / M, k = a - 1 .. 0: bit = v > 0, v -= or += the reference; point exp(2 pi j index / M), symbol = Gray(index)
  e = Im(s conj(point)) limited to +-1;  phi += alpha e;  dphi += beta e  (alpha = 0.1, beta = 0.047 alpha^2)
  sampler and framer: src/hfdl.c:745-891 (on_symbol below follows it case by case).

The rate register.  `rate` stays within 1e-4 of 3 / 2, where fp32 resolves 1.2e-7, and in lock the loop filter feeds it increments of
rate_adj q_hat ~ 1e-9: a reference in fp32 (liquid's symsync_crcf is float by definition) drops them, and what the integrator picked up
while acquiring stays in it for the rest of the burst.  The proportional path makes up for the difference with a standing timing offset of
1e-2 .. 1e-1 branch: against the all-float64 model an fp32 side takes every branch boundary some dozen outputs early or late, each such
output differing by the signal's slope over 1 / 16 sample.  That one register is the whole difference (measured: oracle/PINNING.md
section 5): with rate_fp32=True the model rounds `rate`, and nothing else, to fp32 after every update, and an fp32 side then follows it
to 1e-6.  Both forms are used: the all-float64 one says how far fp32 is from the loop's equations, the other is sharp enough to see a
dropped tap or a wrong summation order.

The trace holds, besides the symbols, how close every discrete decision was to going the other way (module tests/
test_demod_loops_f64_cpu.py, `decided_within_rounding`)."""
import json
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPFB, SS_TAPS, EQ_LEN = 16, 18, 15
SAMPLER_BITS, SAMPLER_SYMBOLS, SAMPLER_SKIP = 1, 2, 3
FR_A1, FR_A2, FR_M1, FR_M2_SKIP, FR_EQ_TRAIN, FR_DATA_1, FR_DATA_2 = range(1, 8)
MASK127 = (1 << 127) - 1
COUNTERS = ("a1_found", "a2_found", "m1_found", "m1_not_found", "frames", "train_bits_total", "train_bits_bad")


def f32(v):
    return float(np.float32(v))


def kaiser(n, fc, As):
    beta = 0.5842 * (As - 21.0) ** 0.4 + 0.07886 * (As - 21.0)
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    return np.sinc(2.0 * fc * t) * np.i0(beta * np.sqrt(1.0 - (2.0 * t / n) ** 2)) / np.i0(beta)


def design():
    """dict(ss_mf[16][18], ss_dmf[16][18], lf_b0, lf_a1, rate_adj, eq_h0[15]) in float64."""
    n = 2 * NPFB * 3 * 3 + 1
    H = 2.0 * 0.75 * kaiser(n, 0.75 / (3 * NPFB), 40.0)
    dH = np.roll(H, -1) - np.roll(H, 1)
    dH *= 0.06 / np.abs(H * dH).max()
    split = lambda h: np.ascontiguousarray(h[:NPFB * SS_TAPS].reshape(SS_TAPS, NPFB).T)
    w = 0.001
    alpha, beta = 1.0 - w, 0.22 * w
    a0 = 1.0 - 0.5 * alpha
    return dict(ss_mf=split(H), ss_dmf=split(dH), lf_b0=beta / a0, lf_a1=-0.495 * alpha / a0, rate_adj=0.5 * w,
                eq_h0=2.0 * 0.45 * kaiser(EQ_LEN, 0.45, 40.0))


def tables_from(ss_mf, ss_dmf, lf_b0, lf_a1, rate_adj, eq_h0):
    """The fp32 tables of a side under test, as the model takes them."""
    return dict(ss_mf=np.asarray(ss_mf, np.float64).reshape(NPFB, SS_TAPS), ss_dmf=np.asarray(ss_dmf, np.float64).reshape(NPFB, SS_TAPS),
                lf_b0=float(lf_b0), lf_a1=float(lf_a1), rate_adj=float(rate_adj), eq_h0=np.asarray(eq_h0, np.float64).copy())


def round_half_away(v):
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


class Protocol:
    """Preamble sequences, thresholds and frame parameters of tests/golden/hfdl_constants.json."""

    def __init__(self):
        K = json.load(open(os.path.join(GOLD, "hfdl_constants.json")))
        D = K["defines"]
        self.D = D
        abits = [(o >> (7 - i)) & 1 for o in K["A_octets"] for i in range(8)][:D["A_LEN"]]
        self.A = self.pack(abits)
        self.M1 = [self.pack([K["M1_bits"][(K["M_shifts"][m] + j) % D["M1_LEN"]] for j in range(D["M1_LEN"])]) for m in range(8)]
        self.modes = K["frame_params"]["modes"]                    # bits per symbol, segments, code rate, column shift
        self.T = [float(v) for v in K["T_seq"][0]]
        self.T_bits = sum((1 if v < 0 else 0) << (14 - i) for i, v in enumerate(self.T))
        # the correlation of m matching bits in the reference's fp32 expression, 2.0f * m / 127 - 1.0f, against its fp32 thresholds
        m = np.arange(128, dtype=np.float32)
        self.corr = np.float32(2.0) * m / np.float32(D["A_LEN"]) - np.float32(1.0)
        self.over = {k: np.abs(self.corr) > np.float32(D[k]) for k in ("CORR_THRESHOLD_A1", "CORR_THRESHOLD_A2", "CORR_THRESHOLD_M1")}
        co = K["costas"]
        self.alpha = f32(co["alpha"])
        self.beta = float(np.float32(co["beta_over_alpha_squared"]) * np.float32(co["alpha"]) * np.float32(co["alpha"]))
        self.limit, self.runaway = f32(co["limit"]), f32(co["runaway_dphi"])
        self.mu = f32(K["constructors"]["eqlms_bw"])
        dt = K["decoder_thread"]
        self.timeout = dt["max_frames_without_frame"] * D["SINGLE_SLOT_FRAME_LEN"]
        self.nf = (f32(dt["noise_floor_keep"]), f32(dt["noise_floor_take"]), f32(dt["noise_floor_bias"]), dt["noise_floor_clk_mask"])
        self.retries = D["MAX_SEARCH_RETRIES"]
        self.symbol_rate = D["HFDL_SYMBOL_RATE"]

    @staticmethod
    def pack(bits):
        v = 0
        for b in bits:
            v = ((v << 1) | (int(b) & 1)) & MASK127
        return v


def psk_slice(arity, s):
    """(Gray symbol, constellation point, angular margin to the nearest decision boundary in radians -- arity 1: |Re s| / |s|)."""
    mod = abs(s)
    if arity == 1:
        bit = 0 if s.real > 0 else 1
        return bit, complex(-1.0 if bit else 1.0, 0.0), (abs(s.real) / mod if mod > 0 else 0.0)
    M = 1 << arity
    a = math.pi / M
    theta = math.atan2(s.imag, s.real) - math.pi * (1.0 - 1.0 / M)
    if theta < -math.pi:
        theta += 2.0 * math.pi
    idx, v, margin = 0, theta, min(math.pi + theta, math.pi - theta)          # the wrap at theta = +-pi is a boundary as well
    for k in range(arity - 1, -1, -1):
        ref = (1 << k) * a
        margin = min(margin, abs(v))
        idx <<= 1
        if v > 0:
            idx |= 1
            v -= ref
        else:
            v += ref
    ang = idx * 2.0 * a
    return idx ^ (idx >> 1), complex(math.cos(ang), math.sin(ang)), margin


class DemodLoopsF64:
    """One channel.  tables: tables_from(...) of the side under test, or None: the float64 design.  rate_fp32: the timing loop's rate
    register, and it alone, holds fp32 values (module docstring)."""

    def __init__(self, tables=None, rate_fp32=False):
        self.rate_fp32 = rate_fp32
        t = design() if tables is None else tables
        self.mf, self.dmf = t["ss_mf"], t["ss_dmf"]
        self.b0, self.a1, self.rate_adj, self.h0 = t["lf_b0"], t["lf_a1"], t["rate_adj"], t["eq_h0"]
        self.P = Protocol()
        self.win = np.zeros(SS_TAPS, np.complex128)
        self.wind = np.zeros(SS_TAPS, np.complex128)
        self.ss_reset()
        self.phi = self.dphi = 0.0
        self.out_idx = 0
        self.sample_cnt = self.symbol_cnt = 0
        self.noise_floor, self.nf_clk = 1.0, 0
        self.signal_level, self.frame_symbol_cnt, self.freq_err_hz = 0.0, 0.0, 0.0
        self.bits = 0
        self.cnt = dict.fromkeys(COUNTERS, 0)
        self.frames = []                    # dict(mode, bitmask_lsb, freq_err_hz, train_bad, train_total, symbols)
        self.freq_err = []                  # dphi * 1800 / 2 pi at every confirmed second A sequence
        self.framer_reset()
        # ---- the trace, one entry per sample / per symbol of the whole stream
        self.bank_margin = []               # per sample: least distance of 16 tau from a half-integer among its bank decisions
        self.outputs = []                   # per sample: 0, 1 or 2
        self.banks = []                     # the branch of every output
        self.q_trace = []                   # the timing error of every loop-filter update
        self.sym_margin = []                # per symbol: slicer margin
        self.run_margin = []                # per symbol: ||dphi| - 0.25| while searching A1 (inf elsewhere), least of its two outputs
        self.train_margin = []              # per symbol: |Re s| / |s| of a training symbol (inf elsewhere)
        self.sym_bank_margin = []           # per symbol: least bank margin of the decisions that chose its two outputs' branches
        self.sym_state = []                 # per symbol: framer state it arrived in
        self.sym_sample = []                # per symbol: index of the sample that produced it
        self.w_dist = []                    # per symbol: |w - h0| of the equaliser
        self._run_pending = self._sbm = math.inf
        self.resets_runaway = self.resets_failed_search = 0

    # ---------------------------------------------------------------- the objects' resets
    def ss_reset(self):
        self.win[:] = 0.0
        self.rate = self.delta = 1.5
        self.tau, self.b, self.v1, self.decim = 0.0, 0, 0.0, 0
        self._bm_pending = math.inf         # branch 0 after a reset was not chosen by rounding

    def eq_reset(self):
        self.w = self.h0.astype(np.complex128)
        self.buf = np.zeros(EQ_LEN, np.complex128)
        self.x2 = np.zeros(EQ_LEN)
        self.x2_sum, self.eq_count, self.eq_full = 0.0, 0, False

    def framer_reset(self):                                            # src/hfdl.c:968-991
        self.fr_state, self.symbols_wanted, self.search_retries, self.cur_arity = FR_A1, 1, 0, 1
        self.train_total = self.train_bad = 0
        self.T_idx = 0
        self.use_data = False
        self.eq_reset()
        self.data, self.training = [], []
        self.ss_reset()
        self.s_state, self.bitmask = SAMPLER_BITS, 0

    # ---------------------------------------------------------------- one launch
    def push(self, mf_out, level):
        """Matched-filter output samples and AGC levels of one launch -> its on-time equalised symbols."""
        P = self.P
        out = []
        for x, lvl in zip(np.asarray(mf_out, np.complex128), np.asarray(level, np.float64)):
            x, lvl = complex(x), float(lvl)
            if self.fr_state == FR_A1:
                self.nf_clk += 1
                if (self.nf_clk & P.nf[3]) == P.nf[3]:
                    self.noise_floor = P.nf[0] * self.noise_floor + P.nf[1] * min(self.noise_floor, lvl) + P.nf[2]
            # ---- timing loop
            self.win[1:] = self.win[:-1].copy()
            self.win[0] = x
            self.wind[1:] = self.wind[:-1].copy()
            self.wind[0] = x
            ys, bm, bms = [], math.inf, []
            while self.b < NPFB:
                m = complex(np.dot(self.mf[self.b], self.win))
                ys.append(m / 3.0)
                bms.append(self._bm_pending)                           # how close the choice of THIS output's branch was
                self.banks.append(self.b)
                if self.decim == 2:
                    self.decim = 0
                    d = complex(np.dot(self.dmf[self.b], self.wind))
                    q = max(-1.0, min(1.0, m.real * d.real + m.imag * d.imag))
                    self.q_trace.append(q)
                    v0 = q - self.a1 * self.v1
                    q_hat = self.b0 * v0
                    self.v1 = v0
                    self.rate += self.rate_adj * q_hat
                    if self.rate_fp32:
                        self.rate = f32(self.rate)
                    self.delta = self.rate + q_hat
                self.decim += 1
                self.tau += self.delta
                bf = self.tau * NPFB
                self.b = round_half_away(bf)
                self._bm_pending = abs(abs(bf) - math.floor(abs(bf)) - 0.5)
                bm = min(bm, self._bm_pending)
            self.tau -= 1.0
            self.b -= NPFB
            # a sample without an output decided nothing, but the decision that skipped it stands for it
            self.bank_margin.append(bm if ys else self._bm_pending)
            self.outputs.append(len(ys))
            # ---- per output
            for y, ybm in zip(ys, bms):
                self.phi += self.dphi
                if self.phi > math.pi:
                    self.phi -= 2.0 * math.pi
                elif self.phi < -math.pi:
                    self.phi += 2.0 * math.pi
                r = y * complex(math.cos(self.phi), -math.sin(self.phi))
                if self.fr_state == FR_A1:
                    self._run_pending = min(self._run_pending, abs(abs(self.dphi) - P.runaway))
                    if abs(self.dphi) > P.runaway:
                        self.phi = self.dphi = 0.0
                        self.ss_reset()
                        self.resets_runaway += 1
                x2n = r.real * r.real + r.imag * r.imag
                self.x2_sum = self.x2_sum + x2n - self.x2[0]
                self.buf[:-1] = self.buf[1:].copy()
                self.buf[-1] = r
                self.x2[:-1] = self.x2[1:].copy()
                self.x2[-1] = x2n
                self.eq_count += 1
                self._sbm = min(self._sbm, ybm)
                odd = self.out_idx & 1
                self.out_idx += 1
                if not odd:
                    continue
                s = complex(np.dot(np.conj(self.w), self.buf))
                tm = math.inf
                if self.fr_state == FR_EQ_TRAIN:
                    if not self.eq_full and self.eq_count >= EQ_LEN:
                        self.eq_full = True
                    if self.eq_full:
                        tv = P.T[min(self.T_idx, 14)] * (-1.0 if self.bitmask & 1 else 1.0)
                        self.w = self.w + P.mu * np.conj(tv - s) * self.buf / self.x2_sum
                    self.T_idx += 1
                    tm = abs(s.real) / abs(s) if abs(s) > 0 else 0.0
                out.append(s)
                self.sym_state.append(self.fr_state)
                self.sym_sample.append(self.sample_cnt)
                self.train_margin.append(tm)
                self.run_margin.append(self._run_pending)
                self.sym_bank_margin.append(self._sbm)
                self.w_dist.append(float(np.abs(self.w - self.h0).max()))
                self._run_pending, self._sbm = math.inf, math.inf
                self.on_symbol(s, lvl)
            self.sample_cnt += 1
        return np.array(out, np.complex128)

    # ---------------------------------------------------------------- src/hfdl.c:737-891
    def on_symbol(self, s, level):
        P = self.P
        bits, point, margin = psk_slice(self.cur_arity, s)
        self.sym_margin.append(margin)
        perr = (s * point.conjugate()).imag
        e = 0.5 * (abs(perr + P.limit) - abs(perr - P.limit))
        self.phi += P.alpha * e
        self.dphi += P.beta * e
        self.symbol_cnt += 1
        if self.symbol_cnt >= P.timeout and self.fr_state == FR_A1:
            self.symbol_cnt = 0
            self.phi = self.dphi = 0.0
            self.ss_reset()
        if self.s_state == SAMPLER_BITS:
            bits ^= self.bitmask
            for _ in range(self.cur_arity):
                self.bits = ((self.bits << 1) | (bits & 1)) & MASK127
                bits >>= 1
        elif self.s_state == SAMPLER_SYMBOLS:
            (self.data if self.use_data else self.training).append(s)
        if self.fr_state > FR_A1:
            self.signal_level = (self.signal_level * self.frame_symbol_cnt + level) / (self.frame_symbol_cnt + 1.0)
            self.frame_symbol_cnt += 1.0
        if self.symbols_wanted > 1:
            self.symbols_wanted -= 1
            return
        D = P.D
        st = self.fr_state
        if st == FR_A1:
            m = 127 - bin((self.bits ^ P.A) & MASK127).count("1")
            if P.over["CORR_THRESHOLD_A1"][m]:
                self.cnt["a1_found"] += 1
                self.bitmask = 0 if P.corr[m] > 0 else 0xFFFFFFFF
                self.signal_level, self.frame_symbol_cnt = level, 1.0
                self.symbols_wanted, self.search_retries, self.fr_state = D["A_LEN"], 0, FR_A2
        elif st == FR_A2:
            m = 127 - bin((self.bits ^ P.A) & MASK127).count("1")
            if P.over["CORR_THRESHOLD_A2"][m]:
                self.cnt["a2_found"] += 1
                self.freq_err_hz = self.dphi * P.symbol_rate / (2.0 * math.pi)
                self.freq_err.append(self.freq_err_hz)
                self.symbols_wanted, self.search_retries, self.fr_state = D["M1_LEN"], 0, FR_M1
            else:
                self.search_retries += 1
                if self.search_retries >= P.retries:
                    self.resets_failed_search += 1
                    self.framer_reset()
        elif st == FR_M1:
            best, best_idx = np.float32(0.0), -1
            for k in range(8):
                c = abs(P.corr[127 - bin((self.bits ^ P.M1[k]) & MASK127).count("1")])
                if c > best:
                    best, best_idx = c, k
            if best > np.float32(D["CORR_THRESHOLD_M1"]):
                self.cnt["m1_found"] += 1
                self.data_arity, self.data_segment_cnt = P.modes[best_idx][0], P.modes[best_idx][1]
                self.M1 = best_idx
                self.symbols_wanted, self.search_retries, self.fr_state, self.s_state = D["M2_LEN"], 0, FR_M2_SKIP, SAMPLER_SKIP
            else:
                self.cnt["m1_not_found"] += 1
                self.framer_reset()
        elif st == FR_M2_SKIP:
            self.training = []
            self.symbols_wanted, self.eq_train_seq_cnt, self.fr_state, self.s_state = D["T_LEN"], 9, FR_EQ_TRAIN, SAMPLER_SYMBOLS
        elif st == FR_EQ_TRAIN:
            seq = 0
            for v in self.training[:15]:
                seq = (seq << 1) | ((0 if v.real > 0 else 1) ^ (self.bitmask & 1))
            err = bin(seq ^ P.T_bits).count("1")
            self.train_total += 15
            self.train_bad += err
            self.cnt["train_bits_total"] += 15
            self.cnt["train_bits_bad"] += err
            self.training = []
            if self.eq_train_seq_cnt > 1:
                self.eq_train_seq_cnt -= 1
                self.symbols_wanted, self.T_idx = D["T_LEN"], 0
            elif self.data_segment_cnt > 0:
                self.symbols_wanted, self.fr_state, self.cur_arity, self.use_data = D["DATA_FRAME_LEN"] // 2, FR_DATA_1, self.data_arity, True
            else:
                self.frames.append(dict(mode=self.M1, bitmask_lsb=self.bitmask & 1, freq_err_hz=self.freq_err_hz, train_bad=self.train_bad,
                                        train_total=self.train_total, symbols=np.array(self.data, np.complex128)))
                self.cnt["frames"] += 1
                self.framer_reset()
                self.symbol_cnt = 0
        elif st == FR_DATA_1:
            self.symbols_wanted, self.fr_state = D["DATA_FRAME_LEN"] // 2, FR_DATA_2
        elif st == FR_DATA_2:
            self.data_segment_cnt -= 1
            self.cur_arity, self.use_data, self.fr_state, self.eq_train_seq_cnt = 1, False, FR_EQ_TRAIN, 1
            self.symbols_wanted, self.T_idx = D["T_LEN"], 0

    # ---------------------------------------------------------------- what the comparisons leave out
    def decided_within_rounding(self, bank=1e-3, slicer=1e-3, runaway=1e-5):
        """(per symbol, per sample) True where a discrete decision of the model was so close that rounding could take it the other way:
        the branch of one of the symbol's two outputs within `bank` of a branch boundary, the slicer within `slicer` radians (arity 1 and
        training bits: |Re s| / |s|) of a boundary, |dphi| within `runaway` of its limit."""
        sym = (np.array(self.sym_bank_margin) < bank) | (np.array(self.sym_margin) < slicer) | (np.array(self.train_margin) < slicer) | \
            (np.array(self.run_margin) < runaway)
        return sym, np.array(self.bank_margin) < bank


def run_cut(model, mf_out, level, counts):
    """Pushes a stream's taps in launches of counts[i] samples; returns the symbols of every launch."""
    out, at = [], 0
    for n in counts:
        out.append(model.push(mf_out[at:at + n], level[at:at + n]))
        at += n
    return out


# ---------------------------------------------------------------- the edge streams of the tests

FS_IN = 7812.5                     # channelizer output rate at fs 250 000 (resampler rate 0.6912)
RAMP = 0.06                        # seconds; the prekey lasts 0.25
NOISE = 0.0015                     # per component: bursts of amplitude 0.08 .. 0.12 stand 32 .. 36 dB above it in the channel


def _burst(rng, synth, mode, t0, amp, cfo):
    return dict(mode=mode, octets=synth.make_pdu(rng, mode), t0=t0, amp=amp, cfo=cfo)


def _shape(synth, b, n, rate=FS_IN, ppm=0.0, echo=None):
    """One burst on a grid of n samples at `rate`; ppm: the receiver's sample clock runs fast by that much; echo = (delay in symbols,
    complex gain): a second path.  The burst's amplitude rises over its first RAMP seconds (raised cosine): the AGC follows it, where a
    step of 35 dB leaves the first symbols a hundred times too large -- and one branch taken differently among them would be most of
    the stream's error."""
    sym = synth.burst_symbols(b["octets"], b["mode"])
    r = rate * (1.0 + ppm * 1e-6)
    x = synth.shape_burst(sym, r, b["t0"], n)
    if echo:
        x = x + echo[1] * synth.shape_burst(sym, r, b["t0"] + echo[0] / 1800.0, n)
    t = np.arange(n) / r - b["t0"]
    x = x * np.where(t < RAMP, 0.5 - 0.5 * np.cos(np.pi * np.clip(t, 0.0, RAMP) / RAMP), 1.0)
    return b["amp"] * x * np.exp(2j * np.pi * b["cfo"] * np.arange(n) / r)


def _noise(rng, n, sigma):
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


# The sample clock of streams A and C is off by this much on the three channels (stream B: +-100 ppm).  With no offset at all tau stands
# still through a burst, and where it happens to stand within rounding of a branch boundary every symbol of the burst is "decided
# within rounding"; with an offset it passes the boundaries at a walk, as on the air.
PPM = (40.0, -60.0, 50.0)
TAIL = 0.035                       # seconds of noise behind a channel's last burst: its frame is finished, and the stream ends


def _finish(synth, rng, x, last):
    """Noise on x, cut TAIL behind the end of burst `last`: what follows a frame is a search in noise with the loops out of lock, where
    two roundings of the same recurrence part for good -- nothing there can be compared."""
    n = int((last["t0"] + synth.burst_symbols_len(last["mode"]) / 1800.0 + 1.0 / 1800.0 + TAIL) * FS_IN)
    return (x + _noise(rng, len(x), NOISE))[:n].astype(np.complex64)


def stream_a(synth, seed=42):
    """Acquire and track, every arity: per channel idle noise, then one burst -- 300 bps BPSK at +7 Hz, 1200 bps QPSK at -11 Hz, 1800 bps
    8-PSK at +25 Hz (phi turns through +-pi every 70 symbols; the carrier loop's pull-in ends between 30 and 40 Hz: at 30 Hz and above,
    whether the float64 model acquires the burst depends on the noise seed and on the burst's timing phase; at 25 Hz it did for every
    seed and phase tried) -- at high in-channel SNR.  Returns (three cf32 streams, their bursts)."""
    rng = np.random.default_rng(seed)
    n = int(3.0 * FS_IN)
    bursts = [_burst(rng, synth, 0, 0.35, 0.1, 7.0), _burst(rng, synth, 2, 0.30, 0.08, -11.0), _burst(rng, synth, 3, 0.40, 0.12, 25.0)]
    return [_finish(synth, rng, _shape(synth, b, n, ppm=p), b) for b, p in zip(bursts, PPM)], [[b] for b in bursts]


def stream_b(synth, seed=40):
    """Equaliser and timing at work: per channel one burst through a two-path channel (an echo one symbol late, -6 dB, another phase on
    each channel) with the sample clock off by +100, -100 and +100 ppm."""
    rng = np.random.default_rng(seed)
    n = int(3.0 * FS_IN)
    bursts = [_burst(rng, synth, 1, 0.30, 0.1, 3.0), _burst(rng, synth, 0, 0.35, 0.1, -5.0), _burst(rng, synth, 2, 0.30, 0.1, 4.0)]
    paths = [(100.0, (1.0, 0.5)), (-100.0, (1.05, 0.5j)), (100.0, (0.95, -0.5))]
    return [_finish(synth, rng, _shape(synth, b, n, ppm=p, echo=e), b) for b, (p, e) in zip(bursts, paths)], [[b] for b in bursts]


def stream_c(synth, seed=40):
    """Resets.  Channel 0: a burst cut off 20 symbols into its second A sequence (three failed searches, framer reset), a BPSK carrier
    that sweeps away at 300 Hz / s -- the carrier loop follows it -- until |dphi| passes 0.25 while the framer searches, then a clean burst
    that must decode.  Channels 1 and 2: the cut-off burst alone / the sweep alone (downwards, from the stream's start) before a clean
    burst."""
    rng = np.random.default_rng(seed)
    n = int(3.6 * FS_IN)
    t = np.arange(n) / FS_IN
    t_cut = 0.05 + (448 + 127 + 20) / 1800.0

    def cut(b):
        x = _shape(synth, b, n, ppm=PPM[0])
        x[int(t_cut * FS_IN):] = 0.0
        return x

    def sweep(t0, t1, hz, amp=0.1):
        """a BPSK-modulated carrier whose offset grows linearly from 0 to `hz` between t0 and t1"""
        on = (t >= t0) & (t < t1)
        ph = 2.0 * np.pi * 0.5 * hz / (t1 - t0) * (t - t0) ** 2
        sym = 1.0 - 2.0 * rng.integers(0, 2, int((t1 - t0) * 1800) + 8)
        x = synth.shape_burst(sym.astype(np.complex64), FS_IN, t0, n)
        return np.where(on, amp * x * np.exp(1j * ph), 0.0)

    clean = [_burst(rng, synth, 1, 1.10, 0.1, 6.0), _burst(rng, synth, 2, 0.60, 0.1, -4.0), _burst(rng, synth, 0, 0.75, 0.1, 5.0)]
    cut_off = [_burst(rng, synth, 1, 0.05, 0.1, 4.0), _burst(rng, synth, 0, 0.05, 0.1, -3.0)]
    x0 = cut(cut_off[0]) + sweep(0.42, 1.02, 180.0) + _shape(synth, clean[0], n, ppm=PPM[0])
    x1 = cut(cut_off[1]) + _shape(synth, clean[1], n, ppm=PPM[1])
    x2 = sweep(0.05, 0.65, -180.0) + _shape(synth, clean[2], n, ppm=PPM[2])
    return [_finish(synth, rng, x, b) for x, b in zip((x0, x1, x2), clean)], [[b] for b in clean]


STREAMS = dict(A=stream_a, B=stream_b, C=stream_c)
