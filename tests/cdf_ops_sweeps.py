"""Scripts for the CDF-operation interpreters (include/divans_gpu.h: divans_gpu_selftest_cdf_ops_on; oracle/cdf_ops.c:
orc_cdf_ops_run) and the two CPU opinions about what they must answer.

* `oracle_run`   -- the C interpreter: nothing but calls of the oracle's orc_cdf_* / orc_weights_* / state-step functions.
* `Mirror`       -- the same script on the independent Python restatement (ref_restatement), checked against the oracle's
                    functions call by call where it always was.  Slow: it runs the short scripts in full and a thinning of
                    the sweeps.
* the generators -- edge-directed sweeps.  Every sweep is a list of CASES; a case is a self-contained run of ops (it loads
                    the rows / Weights it needs first), so any subset of cases is a valid script and `thin` can keep one
                    case in k.  All deterministic (fixed seeds).

Rows that a blend is applied to take their totals from the ONE trajectory a row's total follows under the speed
(FrequentistCDF16::blend, frequentist_cdf.rs:74-85: from 64, + inc per update, (t + 16) - ((t + 16) >> 2) once it
reached lim); rows that are only read may have any total up to 32767.
"""
import ctypes

import numpy as np

import pyoracle as po
import ref_restatement as rr

Q = 1 << 15
SPECIAL_TOTALS = [16, 64, 255, 256, 16383, 16384, 16385, 32766, 32767]
SPREAD_TOTALS = [23, 100, 700, 3000, 9000, 25000]
# the speeds the GPU tests code streams under (test_gpu_parity.py, test_gpu_reference_unit_tests.py) and four that park a
# row's total at an edge
TEST_SPEEDS = [(16, 8192), (64, 16384), (2, 1024), (128, 16384), (8000, 64), (8100, 16384), (4096, 16384), (8160, 1),
               (1, 16384), (1, 1024), (4, 2048), (8, 4096), (32, 4096), (256, 16384), (1024, 16384),
               (0x30, 0x4000), (0x20, 0x1000), (0x10, 0x2000)]
WEIGHT_LOADS = [1, 1 << 23, (1 << 24) - 1, 1 << 24, 1 << 30, (1 << 31) - 1]
PROB_EDGES = [1, 2, 3, 255, 256, 257, 16383, 16384, 16385, 32766, 32767]
RATES = sorted(set([q << 7 for q in range(257)] + [Q >> 2, Q >> 1, (Q >> 1) + (Q >> 2), 0, Q]))   # what Weights can hand over + operation_test_helper's five


def default_speeds():
    """the literal_adaptation speeds of the two benchmark configurations"""
    out = []
    for cfg in (po.config_simple(), po.config_context_mixing()):
        out += [(int(s.inc), int(s.lim)) for s in cfg.literal_adaptation]
    return out


def all_speeds():
    seen, out = set(), []
    for sp in default_speeds() + TEST_SPEEDS:
        if sp not in seen:
            seen.add(sp); out.append(sp)
    return out


# ---------------------------------------------------------------- the two CPU opinions
def as_ops(ops):
    return np.ascontiguousarray(np.asarray(ops, dtype=np.int64).astype(np.uint32).reshape(-1, 4))


def oracle_run(ops):
    ops = as_ops(ops)
    out = np.zeros((ops.shape[0], 16), dtype=np.int32)
    L = po.lib()
    L.orc_cdf_ops_run.restype = ctypes.c_int
    L.orc_cdf_ops_run.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert L.orc_cdf_ops_run(ops.ctypes.data, ops.shape[0], out.ctypes.data) == 0
    return out.astype(np.int64)


def _u16(v):
    return v & 0xFFFF


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


class Mirror:
    """the same script on the CPU restatements; returns the expected records"""
    def __init__(self):
        self.reset()

    def reset(self):
        self.c = [rr.Cdf(), rr.Cdf()]
        self.o = [po.Cdf16(), po.Cdf16()]
        for x in self.o:
            po.lib().orc_cdf_default(ctypes.byref(x))
        self.w = rr.Weights(); self.w.mixing_param = 2
        self.ow = po.Weights(); po.lib().orc_weights_init(ctypes.byref(self.ow)); self.ow.mixing_param = 2

    def _weights_rec(self):
        return (_i32(self.w.model_weights[0]), _i32(self.w.model_weights[1]), self.w.normalized_weight & 0xFFFF)

    def run(self, ops):
        L = po.lib()
        out = np.zeros((len(ops), 16), dtype=np.int64)
        for k, (kind, a, b, c) in enumerate(ops):
            kind, a, b, c = int(kind), int(a), int(b), int(c)
            if kind in (0, 1, 7):
                i = 1 if kind == 1 else 0
                self.c[i].blend(a, (b, c)); L.orc_cdf_blend(ctypes.byref(self.o[i]), a, po.Speed(b, c))
                assert list(self.o[i].cdf) == self.c[i].cdf
                out[k] = self.c[i].cdf
            elif kind == 2:
                m = self.c[0].average(self.c[1], a)
                om = po.Cdf16(); L.orc_cdf_average(ctypes.byref(self.o[0]), ctypes.byref(self.o[1]), a, ctypes.byref(om))
                assert list(om.cdf) == m.cdf
                out[k] = m.cdf
            elif kind == 3:
                s, f = self.c[0].sym_to_start_and_freq(a)
                out[k, :3] = (_u16(s), _u16(f), a)
            elif kind == 4:
                sym, s, f = self.c[0].cdf_offset_to_sym_start_and_freq(a)
                sf = po.SymStartFreq(); L.orc_cdf_offset_to_sym_start_and_freq(ctypes.byref(self.o[0]), a, ctypes.byref(sf))
                assert (sf.sym, sf.start, sf.freq) == (sym, s, f)
                out[k, :3] = (_u16(s), _u16(f), sym)
            elif kind == 5:
                a, b, c = rr.i16(a), rr.i16(b), rr.i16(c)
                self.w.update([a, b], c)
                probs = (ctypes.c_int16 * 2)(a, b); L.orc_weights_update(ctypes.byref(self.ow), probs, c)
                assert list(self.ow.model_weights) == self.w.model_weights and self.ow.normalized_weight == self.w.normalized_weight
                out[k, :3] = self._weights_rec()
            elif kind == 6:
                self.reset(); out[k] = self.c[0].cdf
            elif kind == 8:
                if a < 2:
                    self.c[a].cdf[b & 15] = rr.i16(c); self.o[a].cdf[b & 15] = rr.i16(c)
                    out[k] = self.c[a].cdf
                else:
                    if b < 2:
                        self.w.model_weights[b] = _i32(c); self.ow.model_weights[b] = _i32(c)
                    else:
                        self.w.normalized_weight = rr.i16(c); self.ow.normalized_weight = rr.i16(c)
                    out[k, :3] = self._weights_rec()
            elif kind == 9:                                   # get_nibble_internal + helper_advance_sym, ans.rs:230-252
                state = a | (b << 32)
                row = self.c[0].average(self.c[1], self.w.norm_weight_as_u16_as_i32()) if c else self.c[0]
                sym, s, f = row.cdf_offset_to_sym_start_and_freq(rr.i16(state & rr.SCALE_MASK))
                x = ((f & rr.M64) * (state >> rr.LOG2_SCALE) + (state & rr.SCALE_MASK) - (s & rr.M64)) & rr.M64
                out[k, :5] = (_u16(s), _u16(f), sym, _i32(x), _i32(x >> 32))
                if c:
                    out[k, 5:8] = (_u16(self.c[0].sym_to_start_and_freq(sym)[1]), _u16(self.c[1].sym_to_start_and_freq(sym)[1]), _u16(f))
            elif kind == 10:                                  # the mixing nibble of code_nibble, literal.rs:230-239
                row = self.c[0].average(self.c[1], self.w.norm_weight_as_u16_as_i32())
                s, f = row.sym_to_start_and_freq(a)
                f0 = self.c[0].sym_to_start_and_freq(a)[1]; f1 = self.c[1].sym_to_start_and_freq(a)[1]
                self.w.update([f0, f1], f)
                out[k, :5] = (_u16(s), _u16(f), a, _u16(f0), _u16(f1))
                out[k, 5:8] = self._weights_rec()
                self.ow.model_weights[0], self.ow.model_weights[1] = self.w.model_weights
                self.ow.normalized_weight = self.w.normalized_weight
            else:
                raise ValueError(kind)
        return out


# ---------------------------------------------------------------- rows
def trajectory(inc, lim):
    """[(total, renormalises)] of a row's total under Speed(inc, lim), from the default row's 64 until it repeats;
    `renormalises`: the update that leaves this total renormalises"""
    out, seen, t = [], set(), 64
    while t not in seen:
        seen.add(t)
        n = t + inc
        ren = n >= lim
        assert n + (16 if ren else 0) <= 32767, (inc, lim, t)  # what divans_gpu_speed_supported promises
        out.append((t, ren))
        t = (n + 16) - ((n + 16) >> 2) if ren else n
    return out


def blend_totals(inc, lim):
    """the totals the Blend sweep puts rows at: every one whose next update renormalises, the ones an update before and
    after it, the trajectory's smallest and largest"""
    tr = trajectory(inc, lim)
    ts = [t for t, _ in tr]
    pick = {min(ts), max(ts)}
    for i, (t, ren) in enumerate(tr):
        if ren:
            pick.add(t)
            if i > 0:
                pick.add(ts[i - 1])
            n = t + inc
            pick.add((n + 16) - ((n + 16) >> 2))
    return sorted(pick)


SHAPES = ["low", "high", "spike", "stairs", "random0", "random1", "random2"]


def make_row(shape, total):
    """16 strictly increasing entries, cdf[0] >= 1, cdf[15] == total"""
    assert 16 <= total <= 32767
    spare = total - 16
    if shape == "low":            # 1, 2, .., 15, T: all the mass on symbol 15
        w = [0] * 15 + [1]
    elif shape == "high":         # T-15, .., T: all of it on symbol 0
        w = [1] + [0] * 15
    elif shape == "spike":
        w = [0] * 7 + [1] + [0] * 8
    elif shape == "stairs":
        w = [1] * 16
    else:
        rng = np.random.default_rng(1000 + int(shape[6:]) * 77 + total)
        w = [float(x) for x in rng.random(16) ** (1 + 3 * int(shape[6:]))]
    sw = sum(w)
    freq = [1 + int(spare * x / sw) for x in w]
    freq[int(np.argmax(w))] += total - sum(freq)
    row = [int(v) for v in np.cumsum(freq)]
    assert row[0] >= 1 and all(b > a for a, b in zip(row, row[1:])) and row[15] == total, (shape, total, row)
    return row


def blended_end_row(sym, speed, n=30000):
    """the row n blends of one symbol end on (common_tests.rs:94-103)"""
    return [int(v) for v in oracle_run([(0, sym, *speed)] * n)[-1]]


def load_row(which, row):
    assert all(b > a for a, b in zip(row, row[1:])) and 1 <= row[0] and row[15] <= 32767
    return [(8, which, i, v) for i, v in enumerate(row)]


def load_weights(w0, w1, norm=None):
    ops = [(8, 2, 0, w0), (8, 2, 1, w1)]
    if norm is not None:
        ops.append((8, 2, 2, norm))
    return ops


def read_rows():
    """(name, row) of the rows the read-only sweeps use: every special total under three shapes (rotating, so every shape
    meets totals from 16 to 32767), a logarithmic spread between, and the rows long runs of one symbol end on"""
    rows = []
    k = 0
    for t in SPECIAL_TOTALS:
        for _ in range(3):
            rows.append((f"{SHAPES[k % len(SHAPES)]}@{t}", make_row(SHAPES[k % len(SHAPES)], t))); k += 1
    for t in SPREAD_TOTALS:
        rows.append((f"{SHAPES[k % len(SHAPES)]}@{t}", make_row(SHAPES[k % len(SHAPES)], t))); k += 1
    rows.append(("default", [4 * (i + 1) for i in range(16)]))
    for speed in default_speeds()[:1] + [(8100, 16384)]:
        for sym in (0, 7, 15):
            rows.append((f"end{sym}@{speed}", blended_end_row(sym, speed)))
    assert len(rows) >= 32 and all(any(n.startswith(s) for n, _ in rows) for s in SHAPES)
    return rows


def row_pairs():
    """ordered pairs (row 0 = context-map row, row 1 = stride row) for the Average sweep, both orders of each: tiny x huge,
    huge x huge, tiny x tiny, and the middle"""
    R = dict(read_rows())
    names = list(R)
    tiny = [n for n in names if R[n][15] <= 256]
    huge = [n for n in names if R[n][15] >= 16383]
    mid = [n for n in names if 256 < R[n][15] < 16383]
    picks = []
    for i in range(10):
        picks.append((tiny[(3 * i) % len(tiny)], huge[(5 * i + 1) % len(huge)]))
        picks.append((huge[(7 * i) % len(huge)], huge[(3 * i + 2) % len(huge)]))
    for i in range(6):
        picks.append((tiny[i % len(tiny)], tiny[(i + 4) % len(tiny)]))
        picks.append((mid[i % len(mid)], huge[(11 * i) % len(huge)]))
    out = []
    for a, b in picks:
        out.append((f"{a} x {b}", R[a], R[b])); out.append((f"{b} x {a}", R[b], R[a]))
    assert len(out) >= 64
    return out


# ---------------------------------------------------------------- the sweeps: lists of cases
def thin(cases, k, phase=0):
    return [c for i, c in enumerate(cases) if i % k == phase % k]


def flatten(cases):
    return [op for c in cases for op in c]


def blend_cases(speeds, forms=(0, 7)):
    """Blend: for every speed, every total of blend_totals, every shape scaled to it and every symbol: a blend (plain and
    known-max form), then a second one of the same symbol; plus the rows long single-symbol runs end on"""
    cases = []
    for speed in speeds:
        inc, lim = speed
        for t in blend_totals(inc, lim):
            shapes = SHAPES if t > 16 else SHAPES[:1]
            for shape in shapes:
                row = make_row(shape, t)
                for sym in range(16):
                    for form in forms:
                        cases.append(load_row(0, row) + [(form, sym, inc, lim)] * 2)
            if t == 64:
                for sym in range(16):
                    cases.append([(6, 0, 0, 0)] + [(0, sym, inc, lim), (7, sym, inc, lim)])
    return cases


def blend_end_cases(speeds):
    cases = []
    for speed in speeds:
        for s0 in (0, 7, 15):
            row = blended_end_row(s0, speed)
            for sym in range(16):
                cases.append(load_row(0, row) + [(0, sym, *speed), (7, sym, *speed)])
                cases.append(load_row(1, row) + [(1, sym, *speed)] * 2)
    return cases


def search_cases(slot_step=1, decode=True):
    """Start/freq and search: per row, all 16 symbols through op 3, the slots through op 4 and (decode) op 9 with a state
    whose upper bits vary with the slot"""
    cases = []
    for name, row in read_rows():
        ops = load_row(0, row) + [(3, s, 0, 0) for s in range(16)]
        slots = range(0, Q, slot_step)
        ops += [(4, off, 0, 0) for off in slots]
        if decode:
            for off in slots:
                state = (((off * 0x9E3779B97F4A7C15) >> 3) & ((1 << 63) - 1) & ~0x7FFF) | (1 << 31) | off
                ops.append((9, state & 0xFFFFFFFF, state >> 32, 0))
        cases.append(ops)
    return cases


def average_cases(rates=RATES):
    """Average: per ordered pair, op 2 at every rate"""
    return [load_row(0, r0) + load_row(1, r1) + [(2, rate, 0, 0) for rate in rates] for _, r0, r1 in row_pairs()]


def _mixed_sf(r0, r1, rate):
    """the oracle's (start, freq) of every symbol under r0.average(r1, rate), freq as i16"""
    L = po.lib()
    a, b, m = po.Cdf16(), po.Cdf16(), po.Cdf16()
    for i in range(16):
        a.cdf[i] = r0[i]; b.cdf[i] = r1[i]
    L.orc_cdf_average(ctypes.byref(a), ctypes.byref(b), rate, ctypes.byref(m))
    out = []
    for s in range(16):
        sf = po.SymStartFreq(); L.orc_cdf_sym_to_start_and_freq(ctypes.byref(m), s, ctypes.byref(sf))
        out.append((int(sf.start), int(sf.freq)))
    return out


def mixed_encode_cases(rates=RATES, pairs=None):
    """op 10 on the pairs of the Average sweep: every rate, every symbol, the Weights loaded with the edge values in turn.
    Where two neighbours of the averaged row are equal the reference's mixed frequency is -1 (huge x huge pairs); such
    records are compared like any other -- Weights::update's wrapping arithmetic is defined there too (weights.rs:110-133)."""
    wl = [(v, 1) for v in WEIGHT_LOADS] + [(1, v) for v in WEIGHT_LOADS[1:]]
    cases, n = [], 0
    for _, r0, r1 in (pairs if pairs is not None else row_pairs()):
        ops = load_row(0, r0) + load_row(1, r1)
        for rate in rates:
            for sym in range(16):
                w0, w1 = wl[n % len(wl)]; n += 1
                ops += load_weights(w0, w1, rate) + [(10, sym, 0, 0)]
        cases.append(ops)
    return cases


STATE_EDGES = [1 << 31, (1 << 31) + 1, (1 << 32) - 1, (1 << 32) + 1, (1 << 47) - 1, (1 << 47) + 1, (1 << 48) - 1, (1 << 48) + 1, 1 << 62, (1 << 63) - 1]


def states():
    rng = np.random.default_rng(99)
    out = list(STATE_EDGES)
    for bits in range(32, 64):
        out.append((1 << (bits - 1)) | int(rng.integers(0, 1 << 62)) & ((1 << (bits - 1)) - 1))
    return out


def _with_slot(state, slot):
    return max((state & ~0x7FFF) | slot, (1 << 31) | slot)     # the decoder refills a state below 2^31 before it uses it


def state_cases():
    """State step: op 9 with the edge states, the low 15 bits set to the symbol's start, start + freq - 1 and a middle slot,
    on rows (plain) and on averaged pairs (mixed) whose every frequency is at least 1"""
    L = po.lib()
    cases = []
    for name, row in read_rows():
        c = po.Cdf16()
        for i in range(16):
            c.cdf[i] = row[i]
        sfs = []
        for s in range(16):
            sf = po.SymStartFreq(); L.orc_cdf_sym_to_start_and_freq(ctypes.byref(c), s, ctypes.byref(sf))
            sfs.append((int(sf.start), int(sf.freq)))
        if min(f for _, f in sfs) < 1:
            continue
        ops = load_row(0, row)
        for st in states():
            for start, freq in sfs:
                for slot in sorted({start, start + freq - 1, start + freq // 2}):
                    x = _with_slot(st, slot)
                    ops.append((9, x & 0xFFFFFFFF, x >> 32, 0))
        cases.append(ops)
    assert len(cases) >= 8
    n_mixed = 0
    for i, (_, r0, r1) in enumerate(row_pairs()):
        rate = RATES[(37 * i) % len(RATES)]
        sfs = _mixed_sf(r0, r1, rate)
        if min(f for _, f in sfs) < 1:
            continue
        n_mixed += 1
        ops = load_row(0, r0) + load_row(1, r1) + load_weights(1, 1, rate)
        for st in states():
            for start, freq in sfs:
                for slot in sorted({start, start + freq - 1, start + freq // 2}):
                    x = _with_slot(st, slot)
                    ops.append((9, x & 0xFFFFFFFF, x >> 32, 1))
        cases.append(ops)
    assert n_mixed >= 8
    return cases


def mixed_decode_cases(n_slots=512):
    """op 9, mixed form, over slots spread across the whole range (every rate of operation_test_helper on every pair):
    search_mix2 / the search on an averaged row"""
    cases = []
    for _, r0, r1 in row_pairs():
        ops = load_row(0, r0) + load_row(1, r1)
        for rate in (Q >> 2, Q >> 1, (Q >> 1) + (Q >> 2), 0, Q):
            ops += load_weights(1, 1, rate)
            for j in range(n_slots):
                slot = (j * Q) // n_slots + (j % 7)
                x = _with_slot((0x5DEECE66D * (j + 1)) << 17, slot & 0x7FFF)
                ops.append((9, x & 0xFFFFFFFF, x >> 32, 1))
        cases.append(ops)
    return cases


def weights_cases():
    """Weights through op 5: the cross product of the edge probabilities from every loaded Weights; and two runs of 20 000
    updates in which one model is always the better one (what drives the normalisation shifts)"""
    cases = []
    wl = [(v, 1) for v in WEIGHT_LOADS] + [(1, v) for v in WEIGHT_LOADS[1:]]
    for w0, w1 in wl:
        ops = []
        for p0 in PROB_EDGES:
            for p1 in PROB_EDGES:
                for pm in PROB_EDGES:
                    ops += load_weights(w0, w1) + [(5, p0, p1, pm)]
        cases.append(ops)
    rng = np.random.default_rng(5)
    for better in (0, 1):
        ops = [(6, 0, 0, 0)]
        for _ in range(20000):
            good, bad = int(rng.integers(20000, 32767)), int(rng.integers(1, 300))
            pm = int(rng.integers(1000, 30000))
            ops.append((5, good, bad, pm) if better == 0 else (5, bad, good, pm))
        cases.append(ops)
    return cases


def check_search_records(ops, rec):
    """the reference's own invariants (common_tests.rs:14-17, 29-39) on the records of a search_cases() case"""
    ops = np.asarray(ops, dtype=np.int64)
    k3 = np.nonzero(ops[:, 0] == 3)[0]
    sf = rec[k3]
    for s in range(1, 16):
        assert sf[s, 0] == 1 + sf[s - 1, 0] + sf[s - 1, 1], ("start chain", s)
    k4 = np.nonzero(ops[:, 0] == 4)[0]
    dec, offs = rec[k4], ops[k4, 1]
    assert (np.diff(dec[:, 2]) >= 0).all() and dec[0, 2] == 0, "symbols not monotone in the slot"
    if offs[-1] == Q - 1:
        assert dec[-1, 2] == 15
    assert ((offs >= dec[:, 0] - 1) & (offs <= dec[:, 0] + dec[:, 1])).all(), "slot outside its symbol's range"


# ---------------------------------------------------------------- the sweeps by name, built once per process
_SWEEPS = {}


def sweep(name):
    """(ops as an (n, 4) uint32 array, expected records from the C interpreter run chunk by chunk, case boundaries) of a named sweep; the
    Python restatement has run a 1-in-k thinning of its cases and agreed record by record"""
    if name in _SWEEPS:
        return _SWEEPS[name]
    if name == "blend":
        cases, k = blend_cases(all_speeds()) + blend_end_cases(all_speeds()), 16
    elif name == "search":
        cases, k = search_cases(), 0
    elif name == "search_encoder":          # for the implementation without a decoder
        cases, k = search_cases(decode=False), 0
    elif name == "average":
        cases, k = average_cases(), 4
    elif name == "mixed_encode":
        cases, k = mixed_encode_cases(), 16
    elif name == "state":
        cases, k = state_cases(), 8
    elif name == "mixed_decode":
        cases, k = mixed_decode_cases(), 8
    elif name == "weights":
        cases, k = weights_cases(), 1
    else:
        raise KeyError(name)
    ops = as_ops(flatten(cases))
    bounds = np.concatenate([[0], np.cumsum([len(c) for c in cases])])
    # an interpreter starts every call from the default rows and Weights, and a load's record shows the whole row: the expected
    # records are computed call by call, over the same whole-case chunks the device is given (chunks())
    exp = np.concatenate([oracle_run(ops[lo:hi]) for lo, hi in chunks(bounds)])
    if name.startswith("search"):           # the cases are too long for the restatement: the same rows, one slot in 61
        thinned = flatten(search_cases(slot_step=61, decode=name == "search"))
    else:
        thinned = thin(cases, k)
        if name in ("mixed_encode", "mixed_decode"):    # and every case in which the reference's mixed frequency is 0 or negative
            col = 1
            for i, c in enumerate(cases):
                rec = exp[bounds[i]:bounds[i + 1]]
                kinds = ops[bounds[i]:bounds[i + 1], 0]
                f = rec[kinds >= 9, col]
                if i % k != 0 and ((f == 0) | (f >= 0x8000)).any():
                    thinned.append(c)
        thinned = flatten(thinned)
    second_opinion(thinned)
    _SWEEPS[name] = (ops, exp, bounds)
    return _SWEEPS[name]


CHUNK = 400_000        # ops per interpreter call (a call's records: 64 bytes per op)


def chunks(bounds):
    """[(lo, hi)] covering all ops, cut at case boundaries, about CHUNK ops each"""
    cuts, last = [0], 0
    for b in bounds[1:]:
        if b - cuts[-1] > CHUNK and last > cuts[-1]:
            cuts.append(last)
        last = int(b)
    cuts.append(int(bounds[-1]))
    return list(zip(cuts, cuts[1:]))


def second_opinion(ops):
    """the C interpreter and the Python restatement must agree on every record of `ops`"""
    a, b = oracle_run(ops), Mirror().run(ops)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, ("C interpreter vs Python restatement", int(bad[0]), tuple(ops[int(bad[0])]), a[bad[0]].tolist(), b[bad[0]].tolist())
    return a


OP_NAMES = {0: "blend row 0", 1: "blend row 1", 2: "average", 3: "sym_to_start_and_freq", 4: "cdf_offset_to_sym_start_and_freq", 5: "Weights::update",
            6: "reset", 7: "blend row 0 (known max)", 8: "load", 9: "decode step", 10: "mixed encode step"}
IMPL_NAMES = {0: "generation 1 (lit_kernels.hip)", 1: "lit_decode2.hip", 2: "bucketed encoder (lit_bucket_dev.h, mix_nibble)", 3: "lit_decode_t.hip"}


def compare(impl, ops, got, exp, what=""):
    got = np.asarray(got, dtype=np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        k = int(bad[0])
        op = tuple(int(v) for v in ops[k])
        raise AssertionError(f"{what}: implementation {impl} = {IMPL_NAMES[impl]}, op index {k}, op {op} ({OP_NAMES.get(op[0], '?')}): "
                             f"got {got[k].tolist()}, expected {exp[k].tolist()}; {bad.size} of {len(ops)} records differ")


# ---- the scripts of the reference's own unit tests (tests/test_gpu_reference_unit_tests.py runs them on the device, tests/test_cdf_ops_oracle_cpu.py on both CPU opinions)
MED, SLOW = (0x30, 0x4000), (0x20, 0x1000)
BUF0 = [0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 5, 5, 5, 5, 5, 6, 7, 8, 8, 9, 9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 11, 12, 12, 12, 13, 13, 13, 14, 15,
        15, 15, 15, 15, 15, 15]
BUF1 = [0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 5, 5, 5, 5, 5]


def script_operation_test_helper():
    Q = 1 << 15
    ops = []
    for s in [3, 3, 9, 14, 0, 15, 7, 7, 7, 2] * 3:       # give row 1 a shape of its own (the reference leaves it at the default)
        ops.append((1, s, *SLOW))
    for s in BUF0:
        ops.append((0, s, *MED))
    ops.append((2, Q >> 2, 0, 0))
    for s in BUF1:
        ops.append((7, s, *MED))                          # the pipelined kernels' blend variant must agree too
    for rate in (Q >> 2, Q >> 1, (Q >> 1) + (Q >> 2), 0, Q):
        ops.append((2, rate, 0, 0))
    return ops


def script_declare_common_tests():
    ops = [(0, (i * 7 + 3) & 15, *MED) for i in range(100)]
    ops += [(3, s, 0, 0) for s in range(16)]
    ops += [(4, off, 0, 0) for off in range(0, 1 << 15, 1)]
    return ops


def script_lcg_sample_run():
    # simple_rand, common_tests.rs:44-48 (seed 1): x = x * 1103515245 + 12345; symbols drawn from a fixed pdf through a prefix table
    x = 1
    pdf = [0.1, 0.01, 0.03, 0.2, 0.02, 0.05, 0.04, 0.15, 0.01, 0.06, 0.03, 0.07, 0.02, 0.1, 0.08, 0.03]
    edges = np.cumsum(pdf)
    ops = []
    for _ in range(60000):
        x = (x * 1103515245 + 12345) & 0xFFFFFFFF
        u = ((x >> 16) & 0x7FFF) / 32768.0
        ops.append((0, int(np.searchsorted(edges, u, side="right").clip(0, 15)), *MED))
    ops += [(0, 15, *MED)] * 30000                         # common_tests.rs:94-103
    return ops


def script_weights_update_sequences():
    rng = np.random.default_rng(7)
    ops = []
    for k in range(30000):
        if k % 5000 == 0:
            ops.append((6, 0, 0, 0))
        mode = (k // 5000) % 3
        if mode == 0:
            p0, p1, pm = (int(v) for v in rng.integers(1, 32767, size=3))
        elif mode == 1:                                    # one model much better than the other: drives the weights to the 2^24 normalisation
            p0, p1 = int(rng.integers(20000, 32767)), int(rng.integers(1, 300)); pm = int(rng.integers(1000, 30000))
        else:
            p0 = p1 = pm = int(rng.integers(1, 32767))
        ops.append((5, p0, p1, pm))
    return ops
