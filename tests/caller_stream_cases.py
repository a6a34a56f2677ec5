"""What tests/test_gpu_caller_streams.py runs on a caller's non-blocking stream, and what it must get: the families (all of them
from the existing case modules), two rounds of different data per family at the three sizes, and the C oracle's bytes of every
stream of both rounds -- computed once, shared, never written to.  tests/test_caller_stream_cases_cpu.py checks the builder
without a GPU.

No family here has a table-driven mixing mask: every mask is one value (4 or 0), so every decode and model-encode instance is a
`<4, ...>` or `<0, ...>` one.  The `<-1, ...>` instances are unsafe on a codec whose tables the streaming encoder has used
("Known issue, open"); `assert_no_generic_instance` is called after every decode so that a later edit of the
family list cannot wander into them."""
import numpy as np

import bucketed_segment_cases as bc
import ctx_bucketed_cases as cx
import mix_bt_bucketed_cases as mb
import segment_cases as sc
import wide_block_type_cases as wc

SMALL_STREAMS, SMALL_LONGEST, EMPTY_AT = 37, 300, 5
CACHE_STREAMS, CACHE_LEN = 64, 4096           # a row cache has to fill
SEAM_LENS = (32769, 65536)                    # the chunk seam and the one-lane-per-chunk rANS path
ROUNDS = 2


class Base:
    """divans_lit_config_simple / _context_mixing as they come"""

    def __init__(self, base, seed):
        self.name, self.base, self.n_btypes, self.btype, self.seed, self.mm = base, base, 1, 0, seed, 4

    def __repr__(self):
        return self.name

    def configure(self, cfg):
        self.btype = int(cfg.btype)      # the configuration's own block type is whatever config_<base>() names (0 / 1) ...
        self.n_btypes = self.btype + 1   # ... and a codec that takes lists keeps tables for the types up to it
        return cfg

    def pair(self, da, po):
        g, o = self.configure(getattr(da, "config_" + self.base)()), self.configure(getattr(po, "config_" + self.base)())
        assert bytes(g) == bytes(o)
        return g, o


FAMILIES = {
    "simple": Base("simple", 80),
    "mixing": Base("context_mixing", 81),
    "A": bc.CONFIGS["A"],                      # mixing value 4, constant context, eight block types
    "C": bc.CONFIGS["C"],                      # mixing value 4, a context map, two models, one block type
    "cx_plain": cx.FAMILIES["plain"],          # context-keyed rows (mixing value 0), eight block types
    "cx_mix": cx.FAMILIES["mix"],
    "u2": mb.FAMILIES["u2"],                   # two models, two block types
    "wide9": wc.by_name("mm4_map_plain_bt9"),  # nine block types: the second table layout, list calls only
}
LIST_ONLY = ("wide9",)                         # the batch calls without lists return DIVANS_GPU_EINVAL there
# the four codecs that run side by side, and the second line-up with two of them on one configuration
SIDE_BY_SIDE = (("simple", "mixing", "cx_plain", "wide9"), ("simple", "mixing", "mixing", "wide9"))


def uniform_mask_value(cfg):
    """the one value of the configuration's mixing mask, or None for a table-driven mask"""
    mask = np.frombuffer(bytes(cfg.mixing_mask), np.uint8)
    return int(mask[0]) if (mask == mask[0]).all() else None


def assert_no_generic_instance(kernel_name):
    assert "<-1," not in kernel_name, f"{kernel_name}: a table-driven instance ran on a caller's stream (DESIGN.md section 4, known issue)"


def _rng(fam, round_, what):
    return np.random.default_rng(97000 + 100 * fam.seed + 10 * what + round_)


def small_streams(fam, sources, round_):
    """[(name, literal bytes, segment list)]: 37 ragged streams of at most 300 bytes, one of them empty, one of exactly 300, each
    with a list of 1..6 segments (an empty segment now and then) over the family's block types"""
    rng = _rng(fam, round_, 0)
    data = sc.Data(sources, rng)
    for _ in range(round_):          # the second round starts in another source
        data.take(1)
    out = []
    for i in range(SMALL_STREAMS):
        n = 0 if i == EMPTY_AT else SMALL_LONGEST if i == 0 else int(rng.integers(1, SMALL_LONGEST + 1))
        if n == 0:
            out.append((f"E{i}", np.zeros(0, np.uint8), sc.segments([], [], [])))
            continue
        k = int(rng.integers(1, min(6, n) + 1))
        cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False)).tolist() if k > 1 else []
        lens = sc.cut(n, cuts)
        if i % 7 == 3:
            lens = [0] + lens
        bts = rng.integers(0, fam.n_btypes, size=len(lens)) if fam.n_btypes > 1 else np.full(len(lens), fam.btype)
        out.append((f"R{i}", data.take(n), sc.segments(lens, bts, rng.integers(0, 1 << 64, size=len(lens), dtype=np.uint64))))
    return out


def natural_segments(fam, lit):
    """the one-segment list under which a stream is coded as the list-free calls code it: the configuration's own block type, zeros in front"""
    return sc.segments([lit.size], [fam.btype], [0]) if lit.size else sc.segments([], [], [])


def block_streams(fam, sources, round_, count, length):
    """`count` streams of `length` bytes without lists (for the entry points that take n x stream_len blocks)"""
    data = sc.Data(sources, _rng(fam, round_, 1 + length % 7))
    for _ in range(round_):
        data.take(1)
    return np.stack([data.take(length) for _ in range(count)])


def seam_streams(fam, sources, round_):
    data = sc.Data(sources, _rng(fam, round_, 9))
    for _ in range(round_):
        data.take(1)
    return [(f"L{n}", data.take(n), None) for n in SEAM_LENS]


_ORACLE = {}


def oracle(po, key, sources):
    """per family: (family, the oracle's configuration, rounds) with, for both rounds, the small batch with the oracle's bytes of every stream under its list
    (`listed`) and without one (`plain`; None for the list-only families)"""
    if key not in _ORACLE:
        fam = FAMILIES[key]
        o = fam.configure(getattr(po, "config_" + fam.base)())
        assert uniform_mask_value(o) in (0, 4), key
        rounds = []
        for r in range(ROUNDS):
            streams = small_streams(fam, sources, r)
            listed = [po.lit_segments_encode(o, lit, segs["len"], segs["btype"], segs["last8"]) for _, lit, segs in streams]
            plain = None if key in LIST_ONLY else [po.lit_encode(o, lit) if lit.size else np.zeros(0, np.uint8) for _, lit, _ in streams]
            rounds.append(dict(streams=streams, listed=listed, plain=plain))
        _ORACLE[key] = (fam, o, rounds)
    return _ORACLE[key]


def packed_layout(coded):
    """what divans_gpu_pack_streams must give for streams of these coded sizes: offsets = exclusive prefix sums of the sizes rounded
    up to 4 bytes, and their total"""
    sizes = np.array([c.size for c in coded], np.int64)
    rounded = (sizes + 3) & ~3
    return np.concatenate([[0], np.cumsum(rounded)[:-1]]).astype(np.int64), int(rounded.sum())
