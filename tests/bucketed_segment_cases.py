"""Configurations, segment lists and the batch layout for the bucketed encoder model passes under segment lists
(divans_gpu_codec_set_encode_path(c, 2) + divans_gpu_lit_encode_segments_batch), shared by the CPU tier
(tests/test_bucketed_segment_cases_cpu.py) and the GPU tier (tests/test_gpu_bucketed_segments.py).  numpy + ctypes only.

Three configurations the bucketed passes accept (tests/segment_cases.py has the first and the last):
  A      mm4_const_plain    one model, constant context, eight block types            -> lit_bucket.hip
  B      lsb6 / msb6        one model, the context a function of the previous byte    -> lit_bucket.hip
                            (what the literal-only compressor emits), one block type
  C      mm4_map_mix_bt1    two models, UTF8, one block type                          -> lit_bucket_mix.hip
A batch is everything segment_cases.shapes() gives (40 streams) plus the shapes of extra_shapes(): segment starts where the
sort kernels change phase (the 64-position wave step, the 2048 positions of a wave, the 8192-byte piece, the 65 536-byte slot)."""
import ctypes

import numpy as np

import segment_cases as sc

PIECE = 8192
# name -> offsets at which a segment starts (besides 0)
NAMED_CUTS = {
    "X_edges": [1, 2, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 8194, 16384, 19999],
    "X_slot": sorted({PIECE * k + d for k in range(1, 8) for d in (0, 1)} | {32767, 32768, 32769, 65535}),
}
SIZES = {"X_edges": 20000, "X_slot": 65536, "X_ones": 8200, "X_empty": 12000}


class LiteralOnly:
    """configuration B: config_context_mixing() turned into the literal-only compressor's kind -- no mixing, prediction mode LSB6 (0)
    or MSB6 (1), a 64-entry context map that is no identity, block type 0.  Has what segment_cases.shapes() asks of a family."""

    def __init__(self, mode, seed):
        self.name = {0: "lsb6_map_plain_bt1", 1: "msb6_map_plain_bt1"}[mode]
        self.mode, self.seed = mode, seed
        self.mm, self.ctxc, self.mix, self.n_btypes, self.cached, self.btype, self.base = 4, False, False, 1, True, 0, "context_mixing"

    def __repr__(self):
        return self.name

    def configure(self, cfg):
        cmap = np.zeros(256 * 64, np.uint8)
        cmap[:64] = (np.arange(64) * 5 + 3 + 7 * self.mode) % 64        # a bijection of the 64 contexts, not the identity
        ctypes.memmove(cfg.literal_context_map, cmap.ctypes.data, cmap.size)
        ctypes.memset(cfg.mixing_mask, 4, 8192)
        cfg.prediction_mode = self.mode
        cfg.context_mixing = 0
        cfg.btype = 0
        return cfg

    def pair(self, da, po):
        g = self.configure(da.config_context_mixing())
        o = self.configure(po.config_context_mixing())
        assert bytes(g) == bytes(o)
        return g, o


def _family(name):
    return next(f for f in sc.FAMILIES if f.name == name)


CONFIGS = {"A": _family("mm4_const_plain"), "B_lsb6": LiteralOnly(0, 40), "B_msb6": LiteralOnly(1, 41), "C": _family("mm4_map_mix_bt1")}
# the model pass divans_gpu_codec_last_encode_path reports for them: 2 = bucketed one-model, 3 = bucketed two-model
BUCKETED_PATH = {"A": 2, "B_lsb6": 2, "B_msb6": 2, "C": 3}


def natural_last8(lit, q):
    """last_8_literals at offset q of a stream coded without a list: the bytes before it, newest in bits 56..63, zero before the start"""
    tail = bytes(lit[max(0, q - 8):q]).rjust(8, b"\0")
    return int.from_bytes(tail, "little")


def _last8s(rng, lit, starts):
    """random histories whose newest byte is NOT the byte before the segment (0 at offset 0): every one of them changes the key of
    the segment's first position"""
    out = rng.integers(0, 1 << 64, size=len(starts), dtype=np.uint64)
    for i, q in enumerate(starts):
        nat = int(lit[q - 1]) if q else 0
        top = int(out[i] >> np.uint64(56))
        if top == nat:
            top = (top + 1 + int(rng.integers(0, 255))) % 256
            assert top != nat
        out[i] = np.uint64((int(out[i]) & ((1 << 56) - 1)) | (top << 56))
    return out


def extra_shapes(fam, sources):
    """[(name, literal bytes, segment list)]: X_edges, X_slot (NAMED_CUTS), X_ones (1-byte segments only: every position overridden, a
    list of 8200 segments), X_empty (three empty segments in a row on a piece base, then a non-empty one)"""
    rng = np.random.default_rng(95000 + fam.seed)
    corpus = sources[0]
    nb = fam.n_btypes
    bts = (lambda k: rng.integers(0, nb, size=k)) if nb > 1 else (lambda k: np.full(k, fam.btype))
    out = []

    def add(name, lit, lens):
        lens = np.asarray(lens, dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
        l8 = _last8s(rng, lit, starts)
        out.append((name, lit, sc.segments(lens, bts(len(lens)), l8)))

    o = 1000
    for name in ("X_edges", "X_slot"):
        n = SIZES[name]
        lit = corpus[o:o + n].copy(); o += n + 13
        add(name, lit, sc._cut(n, NAMED_CUTS[name]))
    n = SIZES["X_ones"]
    add("X_ones", corpus[o:o + n].copy(), [1] * n); o += n + 13
    n = SIZES["X_empty"]
    add("X_empty", corpus[o:o + n].copy(), [PIECE, 0, 0, 0, n - PIECE])
    return out


def batch(fam, sources):
    """the ~45 streams of a configuration: segment_cases.shapes() with the extra shapes among them (not all at the end: a launch
    sequence of 24 streams then holds some of each)"""
    base = sc.shapes(fam, sources)
    extra = extra_shapes(fam, sources)
    out = list(base)
    for k, x in enumerate(extra):
        out.insert(5 + 11 * k, x)
    return out


def layout(streams):
    """offsets of the streams' bytes in one buffer: every fourth stream on a 16-byte boundary, the others wherever the one before
    ended but never on one -- both load paths of the sort kernels run.  -> (buffer uint8, offsets int64, sizes int32)"""
    offs, cur = [], 0
    for i, (_, lit, _) in enumerate(streams):
        if i % 4 == 0:
            cur = (cur + 15) & ~15
        elif cur % 16 == 0:
            cur += 1 + i % 15
        offs.append(cur); cur += lit.size
    buf = np.zeros(cur + 64, np.uint8)
    for o, (_, lit, _) in zip(offs, streams):
        buf[o:o + lit.size] = lit
    return buf, np.array(offs, np.int64), np.array([s[1].size for s in streams], np.int32)


def bad_btype(streams, at, btype, k=None):
    """the batch with segment k (default: the one in the middle) of stream `at`'s list naming `btype`"""
    out = [(n, l, s.copy()) for n, l, s in streams]
    segs = out[at][2]
    assert segs.size > 0
    segs["btype"][segs.size // 2 if k is None else k] = btype
    return out


def empty_stream_with_bytes_in_its_list(streams, at):
    """the batch with stream `at` replaced by an empty stream whose list holds one segment of 5 bytes"""
    out = list(streams)
    out[at] = ("E", np.zeros(0, np.uint8), sc.segments([5], [streams[at][2]["btype"][0] if streams[at][2].size else 0], [0x0102030405060708]))
    return out
