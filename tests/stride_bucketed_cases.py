"""Configurations, shapes and batches for the bucketed one-model encoder pass at the strides 2, 3, 4 and 8 (lit_bucket.hip,
bucket_sort_stride_kernel: mixing values 5, 6, 7, and 8 and above, under a constant context and without mixing), shared by the CPU
tier (tests/test_stride_bucketed_cases_cpu.py) and the GPU tier (tests/test_gpu_stride_bucketed.py).  numpy + ctypes only.

Under a mixing value v >= 4 both rows of a position are chosen by the byte d = 1 + min(7, v ^ 4) places back (literal.rs:184-208):
high row [ctx][b_d], low row [b_d][hi].  With a constant context the bucket key is that byte; a segment's first min(d, len)
positions take it from the segment's last8, at distance d - j for position j.

Families: config_simple() with the whole mask set to 5, 6, 7, 8 and 12, and one whose REACHABLE entries (context | nibble << 8 |
low << 12 of the one context the map holds) alternate between 8 and 12 while the others hold values of other distances.  A batch
without a list holds one stream per length of lengths(d); the batches with lists are bucketed_segment_cases.batch() (in two halves)
and the shapes of stride_shapes()."""
import ctypes

import numpy as np

import bucketed_segment_cases as bc
import segment_cases as sc

PIECE = bc.PIECE
PIECE_BASES = (8192, 57344)
# what "automatic" (encode path 0) runs for a call WITHOUT a segment list on these codecs, as divans_gpu_codec_last_encode_path
# reports it: 2 = the bucketed pass (it measured ahead of the streaming kernels at 16 384 and at 64 streams: DESIGN.md section 7, round 12)
AUTOMATIC_PATH_WITHOUT_A_LIST = 2
BUCKETED_PATH = 2


def distance_of(value):
    """literal.rs:192: stride_offset = min(7, mm_opts ^ 4) << 3 for mm_opts >= 4"""
    assert value >= 4
    return 1 + min(7, value ^ 4)


class StrideFamily:
    """config_simple() under a constant context `ctx` with the mask `fill` everywhere -- or, with `reach`, those values cycling over
    the 32 reachable entries and `fill` in the entries no position can reach.  Has what segment_cases.shapes() asks of a family."""

    def __init__(self, name, fill, seed, reach=None, ctx=0, speeds=None, n_btypes=8):
        self.name, self.fill, self.seed, self.reach, self.ctx, self.speeds, self.n_btypes = name, fill, seed, reach, ctx, speeds, n_btypes
        self.dist = distance_of((reach or (fill,))[0])
        assert all(distance_of(v) == self.dist for v in (reach or (fill,)))
        self.mm, self.ctxc, self.mix, self.cached, self.base = -1, True, False, True, "simple"
        self.btype = 0 if n_btypes == 1 else 3

    def __repr__(self):
        return self.name

    def configure(self, cfg):
        ctypes.memset(cfg.literal_context_map, self.ctx, ctypes.sizeof(cfg.literal_context_map))
        mask = np.full(8192, self.fill, np.uint8)
        if self.reach:
            mask[self.ctx + 256 * np.arange(32)] = np.resize(np.array(self.reach, np.uint8), 32)
        ctypes.memmove(cfg.mixing_mask, mask.ctypes.data, mask.size)
        if self.speeds:
            for i, (inc, lim) in enumerate(self.speeds):
                cfg.literal_adaptation[i].inc = inc; cfg.literal_adaptation[i].lim = lim
        cfg.context_mixing = 0
        cfg.btype = self.btype
        return cfg

    def pair(self, da, po):
        g, o = self.configure(da.config_simple()), self.configure(po.config_simple())
        assert bytes(g) == bytes(o)
        return g, o


FAMILIES = {
    "m5": StrideFamily("m5", 5, 70),
    "m6": StrideFamily("m6", 6, 71, ctx=7),
    "m7": StrideFamily("m7", 7, 72, speeds=sc.GENERIC_SPEEDS),
    "m8": StrideFamily("m8", 8, 73, n_btypes=1),
    "m12": StrideFamily("m12", 12, 74),
    # the entries no position reaches hold a value of distance 2: only the reachable ones decide
    "m8_12": StrideFamily("m8_12", 5, 75, reach=(8, 12), ctx=7),
}
EXPECTED_DISTANCE = {"m5": 2, "m6": 3, "m7": 4, "m8": 8, "m12": 8, "m8_12": 8}


class _Refused:
    def __init__(self, name, base, configure):
        self.name, self.base, self._configure = name, base, configure
        self.n_btypes = 1

    def pair(self, da, po):
        g, o = self._configure(getattr(da, "config_" + self.base)()), self._configure(getattr(po, "config_" + self.base)())
        assert bytes(g) == bytes(o)
        return g, o


def _two_models(cfg):
    ctypes.memset(cfg.mixing_mask, 5, 8192)
    return cfg


def _distances_mixed(cfg):
    """constant context 0, no mixing; the reachable entries alternate between 5 and 6"""
    mask = np.full(8192, 5, np.uint8)
    mask[256 * np.arange(1, 32, 2)] = 6
    ctypes.memmove(cfg.mixing_mask, mask.ctypes.data, mask.size)
    cfg.context_mixing = 0
    return cfg


def _lsb6_map(cfg):
    cfg = bc.LiteralOnly(0, 0).configure(cfg)
    ctypes.memset(cfg.mixing_mask, 5, 8192)
    return cfg


# path 2 is refused and divans_gpu_codec_bucket_stride gives 0: two models; a mask that mixes distances; a context that follows from
# the previous byte (the high row [ctx][b_d] would need two key bytes)
REFUSED = {
    "m5_two_models": _Refused("m5_two_models", "context_mixing", _two_models),
    "m5_m6_mixed": _Refused("m5_m6_mixed", "simple", _distances_mixed),
    "m5_lsb6_map": _Refused("m5_lsb6_map", "context_mixing", _lsb6_map),
}


class _Content:
    """cycles through the corpus, random_then_unicode, shuffle384, uniform random bytes and a constant byte"""

    def __init__(self, sources, rng, first=0):
        self.sources, self.rng, self.k = sources, rng, first

    def take(self, n):
        kind = self.k % 5; self.k += 1
        if kind == 3:
            return self.rng.integers(0, 256, size=n, dtype=np.uint8)
        if kind == 4:
            return np.full(n, int(self.rng.integers(1, 256)), np.uint8)
        src = self.sources[kind]
        if src.size <= n:
            return np.resize(src, n).copy()
        o = int(self.rng.integers(0, src.size - n))
        return src[o:o + n].copy()


def lengths(d):
    """stream lengths around the distance, the 64-position wave step, the piece base (the d bytes in front of it) and the slot"""
    out = [0, 1, d - 1, d, d + 1, 63, 64, 65, 8191, 8192, 8193, 8192 + d - 1, 8192 + d, 16385, 65535, 65536]
    return sorted(set(out))


def plain_streams(fam, sources):
    """one stream per length of lengths(d) and four more around the first piece base, so that every content kind meets it"""
    rng = np.random.default_rng(96000 + fam.seed)
    data = _Content(sources, rng, first=fam.seed)
    out = [data.take(n) for n in lengths(fam.dist)]
    out += [data.take(n) for n in (8192 + fam.dist, 8193, 8192 + fam.dist - 1, 8200)]
    return out


def ragged_layout(blocks):
    """every stream at an ODD offset except stream 0, which starts at offset 0: the piece loader's unaligned path, and a stream with
    nothing in front of its first byte (the first d keys are zero, not whatever precedes the buffer).  -> (buffer, offsets, sizes)"""
    offs, cur = [], 0
    for i, b in enumerate(blocks):
        if i and cur % 2 == 0:
            cur += 1
        offs.append(cur); cur += b.size
    buf = np.full(cur + 64, 0xA5, np.uint8)          # the gaps hold a value no key may pick up
    for o, b in zip(offs, blocks):
        buf[o:o + b.size] = b
    assert offs[0] == 0 and all(o % 2 == 1 for o in offs[1:])
    return buf, np.array(offs, np.int64), np.array([b.size for b in blocks], np.int32)


def base_cuts(d):
    """a segment start at each of base - d .. base + d for the piece bases"""
    return sorted({b + k for b in PIECE_BASES for k in range(-d, d + 1)})


def stride_shapes(fam, sources, small=False):
    """[(name, literal bytes, segment list)] with random 64-bit histories unless named otherwise:
      Y_ones     one-byte segments only: every key comes from a last8, at distance d
      Y_cycle    segments of lengths 1 .. d cycling: segments shorter than d hand nothing on
      Y_empty    empty segments between short ones
      Y_base     a segment start at each of base - d .. base + d for the piece bases 8192 and 57344 (small: the same run of lengths
                 around two cuts of a short stream, for the restatement, which knows no pieces)
      Y_natural  the histories the stream's own bytes give (bucketed_segment_cases.natural_last8): the list changes nothing"""
    d = fam.dist
    rng = np.random.default_rng(94000 + fam.seed)
    data = _Content(sources, rng, first=fam.seed + 2)
    bts = (lambda k: rng.integers(0, fam.n_btypes, size=k)) if fam.n_btypes > 1 else (lambda k: np.full(k, fam.btype))
    r64 = lambda k: rng.integers(0, 1 << 64, size=k, dtype=np.uint64)
    out = []

    def add(name, lit, lens, last8s=None):
        lens = np.asarray(lens, dtype=np.int64)
        assert int(lens.sum()) == lit.size
        out.append((name, lit, sc.segments(lens, bts(len(lens)), r64(len(lens)) if last8s is None else last8s)))

    n = 120 if small else 700
    add("Y_ones", data.take(n), [1] * n)
    n = 300 if small else 3000
    lens, k = [], 1
    while sum(lens) < n:
        lens.append(min(k, n - sum(lens))); k = k % d + 1
    add("Y_cycle", data.take(n), lens)
    unit = [1, 0, 2, 0, 0, d, 0, d - 1, 0, 1, 1, 0, d + 1]
    reps = 8 if small else 60
    add("Y_empty", data.take(sum(unit) * reps), unit * reps)
    if small:
        n, cuts = 400, sorted({b + k for b in (100, 300) for k in range(-d, d + 1)})
    else:
        n, cuts = PIECE_BASES[1] + d + 300, base_cuts(d)
    add("Y_base", data.take(n), sc._cut(n, cuts))
    n = 300 if small else 20000
    cuts = [1, d - 1, d, d + 1, 40, 41] if small else [1, d - 1, d, d + 1, 64, 8191, 8192, 8192 + d, 16384 - 1, 16384 + d - 1]
    cuts = sorted({c for c in cuts if 0 < c < n})
    lit = data.take(n)
    add("Y_natural", lit, sc._cut(n, cuts), [bc.natural_last8(lit, q) for q in [0] + cuts])
    return out


def list_batches(fam, sources):
    """name -> streams: the existing lists of bucketed_segment_cases.batch() in two halves (at most 40 streams per batch) and the
    shapes above"""
    existing = bc.batch(fam, sources)
    half = len(existing) // 2
    return {"existing_a": existing[:half], "existing_b": existing[half:], "stride": stride_shapes(fam, sources)}


def natural_segments(lit, cuts, btype):
    """the list that cuts `lit` at `cuts` with the stream's own bytes as every history"""
    cuts = sorted({c for c in cuts if 0 < c < lit.size})
    lens = sc._cut(lit.size, cuts)
    return sc.segments(lens, np.full(len(lens), btype), [bc.natural_last8(lit, q) for q in [0] + cuts])
