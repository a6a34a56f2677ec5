"""Deterministic configurations and segment lists for the segment entry points (divans_gpu_lit_encode_segments_batch /
_decode_segments_batch), shared by the CPU tier (tests/test_segment_cases_cpu.py: the C oracle against the Python restatement)
and the GPU tier (tests/test_gpu_segment_cases.py: every SEG = true kernel instance against the C oracle).  numpy + ctypes only.

A FAMILY names one (MM, CTXC, MIX) triple of the kernels' dispatch -- MM: the mixing value every reachable entry of the mixing
mask holds (4, 0) or -1 for a table-driven mask; CTXC: the context map is constant; MIX: context_mixing > 1 -- plus the number
of literal block types the codec is given tables for and whether the stream's table is small enough for row caches.

A SHAPE is one (literal bytes, segment list) pair; shapes() returns the batch of a family in a fixed order, the empty stream in
the middle (index EMPTY_AT) so that a group that walks the batch 16 streams apart codes one before and one after it."""
import ctypes

import numpy as np

SEG_DTYPE = np.dtype([("len", "<u4"), ("btype", "<u4"), ("last8", "<u8")])

# mixing values a wire stream can carry, with the strides that look furthest back into last_8_literals: value v >= 4 reads the byte
# min(v ^ 4, 7) places before the previous one (literal.rs:176-183), so 5, 6, 7 reach places 1-3 and 8..12, 15 the oldest byte
MM_GENERIC = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15)
# Value 1 keys the low-nibble rows by the whole context (256 x 256 rows per plane): a mask that holds it has more than 32 766 rows per
# stream, for which no row cache exists.  The cached table-driven families draw from the same values without it.
MM_GENERIC_CACHED = tuple(v for v in MM_GENERIC if v != 1)
GENERIC_SPEEDS = ((16, 8192), (64, 16384), (2, 1024), (128, 16384))
EMPTY_AT = 20
N_STREAMS = 40


class Family:
    def __init__(self, name, mm, ctxc, mix, n_btypes=8, cached=True, seed=0):
        self.name, self.mm, self.ctxc, self.mix, self.n_btypes, self.cached, self.seed = name, mm, ctxc, mix, n_btypes, cached, seed
        self.base = "context_mixing" if not ctxc and mm >= 0 else "simple"      # config_simple() / config_context_mixing() to start from
        self.btype = 0 if n_btypes == 1 else 3                                  # the configuration's own block type (shape S5)

    def __repr__(self):
        return self.name

    def configure(self, cfg):
        """fill a LitConfig (the product's or the oracle's: same layout) that config_<self.base>() initialised"""
        rng = np.random.default_rng(7000 + self.seed)
        cmap = np.zeros(256 * 64, np.uint8)
        if self.ctxc:
            cmap[:] = 7 if self.mm < 0 else 0
        elif self.mm >= 0:
            # config_context_mixing's map (i & 63) for block type 0, another bijection of the 64 contexts for every other type:
            # a context table of the wrong block type changes the coded bytes
            for t in range(8):
                cmap[64 * t:64 * t + 64] = (np.arange(64) * (2 * t + 1)) % 64
        else:
            cmap[:] = rng.integers(0, 32 if self.cached else 48, size=cmap.size, dtype=np.uint8)
        ctypes.memmove(cfg.literal_context_map, cmap.ctypes.data, cmap.size)
        if self.mm >= 0:
            ctypes.memset(cfg.mixing_mask, self.mm, 8192)
        else:
            vals = np.array(MM_GENERIC_CACHED if self.cached else MM_GENERIC, dtype=np.uint8)
            mask = rng.choice(vals, size=8192)
            if self.ctxc:       # one context: 32 entries of the mask (context | nibble << 8 | low << 12) can be reached, and they hold every value
                reach = np.resize(vals, 32); rng.shuffle(reach)
                mask[int(cmap[0]) + 256 * np.arange(32)] = reach
            ctypes.memmove(cfg.mixing_mask, mask.ctypes.data, mask.size)
            cfg.prediction_mode = 2 if self.mix else 3       # UTF8: 4 classes of prev_prev, SIGN: 8
            for i, (inc, lim) in enumerate(GENERIC_SPEEDS):
                cfg.literal_adaptation[i].inc = inc; cfg.literal_adaptation[i].lim = lim
        cfg.context_mixing = 2 if self.mix else 0
        cfg.btype = self.btype
        return cfg

    def pair(self, da, po):
        """(product configuration, oracle configuration) with identical bytes"""
        g = self.configure(getattr(da, "config_" + self.base)())
        o = self.configure(getattr(po, "config_" + self.base)())
        assert bytes(g) == bytes(o)
        return g, o


def families():
    out = []
    seed = 0
    for mm in (4, 0, -1):
        for ctxc in (True, False):
            for mix in (False, True):
                tag = f"mm{mm if mm >= 0 else 'x'}_{'const' if ctxc else 'map'}_{'mix' if mix else 'plain'}"
                out.append(Family(tag, mm, ctxc, mix, seed=seed)); seed += 1
                if mm == 4 and not ctxc:      # one block type: the high-nibble rows laid out by class of prev_prev (LitGeometry::hs_classes)
                    out.append(Family(tag + "_bt1", mm, ctxc, mix, n_btypes=1, seed=seed)); seed += 1
                if mm < 0:                    # every mixing value of MM_GENERIC: three planes, no row cache
                    out.append(Family(tag + "_nocache", mm, ctxc, mix, cached=False, seed=seed)); seed += 1
    return out


FAMILIES = families()
# (family, speed whose row totals leave i16): the launches the library checks for wrapped rows, generation 1 without a cache
WRAP_CASES = [("mm4_map_plain", (0x3000, 0x1000)), ("mmx_map_plain", (8180, 64)), ("mm4_const_plain", (0x7800, 0x7800))]


class _Data:
    """cycles through the corpus, random_then_unicode, shuffle384 and uniform random bytes"""

    def __init__(self, sources, rng):
        self.sources, self.rng, self.k = sources, rng, 0

    def take(self, n):
        kind = self.k % 4; self.k += 1
        if kind == 3:
            return self.rng.integers(0, 256, size=n, dtype=np.uint8)
        src = self.sources[kind]
        if src.size <= n:
            return np.resize(src, n).copy()
        o = int(self.rng.integers(0, src.size - n))
        return src[o:o + n].copy()


def segments(lens, btypes, last8s):
    s = np.zeros(len(lens), dtype=SEG_DTYPE)
    s["len"] = lens; s["btype"] = btypes; s["last8"] = np.asarray(last8s, dtype=np.uint64)
    return s


def _cut(n, cuts):
    """segment lengths of n bytes cut at the given positions (those below n)"""
    edges = [0] + [c for c in cuts if 0 < c < n] + [n]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


Data, cut = _Data, _cut      # public names: tests/caller_stream_cases.py builds its batches with them


def shapes(fam, sources, small=False):
    """[(name, literal bytes, segment list)] of a family: S0..S7 and the random fill, N_STREAMS in all (small: S1-S5 and S7 at the
    lengths the pure-Python restatement can afford, every phase change of the full shapes kept but the chunk seam)"""
    rng = np.random.default_rng(91000 + fam.seed)
    data = _Data(sources, rng)
    nb = fam.n_btypes
    r64 = lambda k: rng.integers(0, 1 << 64, size=k, dtype=np.uint64)
    rbt = lambda k: rng.integers(0, nb, size=k)
    cyc = lambda k, first=0: (np.arange(k) + first) % nb
    fixed = []
    fixed.append(("S1", data.take(1), segments([1], rbt(1), r64(1))))
    n = 150 if small else 600
    fixed.append(("S2", data.take(n), segments([1] * n, rbt(n), r64(n))))
    n = 420 if small else 3000
    lens = _cut(n, [15, 16, 17, 31, 32, 33, 47, 48, 49, 140 if small else 1000])
    fixed.append(("S3", data.take(n), segments(lens, rbt(len(lens)), r64(len(lens)))))
    n = 300 if small else 3000
    lens = [0, n * 2 // 5, 0, 0, n - n * 2 // 5, 0]          # empty segments first, two in a row in the middle, last
    fixed.append(("S4", data.take(n), segments(lens, cyc(len(lens), 1), r64(len(lens)))))
    n = 300 if small else 3000
    fixed.append(("S5", data.take(n), segments([n], [fam.btype], [0])))
    n = 400 if small else 5000
    lens, k = [], 1
    while sum(lens) < n:
        lens.append(min(k, n - sum(lens))); k = k % 200 + 1
    fixed.append(("S7", data.take(n), segments(lens, cyc(len(lens)), r64(len(lens)))))
    if small:
        return fixed
    lens = _cut(40000, [32767, 32768, 32769])                # the 65 536-symbol rANS chunk seam
    s6 = ("S6", data.take(40000), segments(lens, rbt(len(lens)), r64(len(lens))))
    s0 = ("S0", np.zeros(0, np.uint8), segments([], [], []))
    fill = []
    while len(fixed) + len(fill) + 2 < N_STREAMS:
        n = int(rng.integers(1, 4001))
        k = int(rng.integers(1, min(60, n) + 1))
        cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False)).tolist() if k > 1 else []
        lens = _cut(n, cuts)
        fill.append((f"R{len(fill)}", data.take(n), segments(lens, rbt(len(lens)), r64(len(lens)))))
    out = fixed + fill
    out.insert(EMPTY_AT, s0)
    out.append(s6)
    assert len(out) == N_STREAMS and out[EMPTY_AT][0] == "S0"
    return out


def bad_lists(streams):
    """the first 12 streams of a batch with three lists that do not add up to their stream: stream 3's covers 7 bytes too few, stream 5's
    7 too many, stream 9 has bytes but no segments.  Returns (streams, indices of the bad ones)."""
    out = [(name, lit, segs.copy()) for name, lit, segs in streams[:12]]
    for i, d in ((3, -7), (5, 7)):
        segs = out[i][2]
        k = int(np.argmax(segs["len"]))
        assert segs["len"][k] > 7 and out[i][1].size > 7
        segs["len"][k] = int(segs["len"][k]) + d
    assert out[9][1].size > 0
    out[9] = (out[9][0], out[9][1], out[9][2][:0])
    return out, (3, 5, 9)


def short_streams(fam, sources, count):
    """`count` streams of 2..199 bytes in 1..8 segments (for speeds under which only short streams stay clear of a wrapped row)"""
    rng = np.random.default_rng(93000 + fam.seed)
    data = _Data(sources, rng)
    out = []
    for k in range(count):
        n = int(rng.integers(2, 200))
        ns = int(rng.integers(1, min(8, n) + 1))
        cuts = np.sort(rng.choice(np.arange(1, n), size=ns - 1, replace=False)).tolist() if ns > 1 else []
        lens = _cut(n, cuts)
        out.append((f"W{k}", data.take(n), segments(lens, rng.integers(0, fam.n_btypes, size=len(lens)),
                                                    rng.integers(0, 1 << 64, size=len(lens), dtype=np.uint64))))
    return out
