"""Guards what tests/test_gpu_stride_bucketed.py compares against and codes: the C oracle under the stride families of
tests/stride_bucketed_cases.py against the second restatement, with and without segment lists; the premise of the stride sort -- in
the restatement's row trace both rows of every position are chosen by the byte d places back, taken from the segment's last8 for a
segment's first d bytes; and the teeth of the lists: of a segment's last8 exactly the byte lanes at distances 1 .. d are read."""
import numpy as np
import pytest

import bucketed_segment_cases as bc
import pyoracle as po
import ref_restatement as rr
import segment_cases as sc
import stride_bucketed_cases as stc
from ref_restatement import rr_segments_decode, rr_segments_encode, to_rr

KEYS = list(stc.FAMILIES)


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _cfg(key):
    fam = stc.FAMILIES[key]
    return fam, fam.configure(po.config_simple())


def _enc(cfg, lit, segs):
    return po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"]).tobytes()


def _reachable(cfg):
    cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)
    assert len(set(cmap.tolist())) == 1
    return np.frombuffer(bytes(cfg.mixing_mask), np.uint8)[int(cmap[0]) + 256 * np.arange(32)]


def test_the_families_are_what_they_are_named_for():
    assert set(stc.FAMILIES) == set(stc.EXPECTED_DISTANCE) == {"m5", "m6", "m7", "m8", "m12", "m8_12"}
    for key in KEYS:
        fam, cfg = _cfg(key)
        reach = _reachable(cfg)
        assert {stc.distance_of(int(v)) for v in reach} == {stc.EXPECTED_DISTANCE[key]} == {fam.dist}, key
        assert cfg.context_mixing == 0
        if key in ("m5", "m6", "m7", "m8", "m12"):
            assert set(bytes(cfg.mixing_mask)) == {int(key[1:])}
    fam, cfg = _cfg("m8_12")
    assert _reachable(cfg).tolist() == [8, 12] * 16
    rest = np.delete(np.frombuffer(bytes(cfg.mixing_mask), np.uint8), 7 + 256 * np.arange(32))
    assert set(rest.tolist()) == {5}                         # distance 2 where no position looks
    speeds = {k: [(s.inc, s.lim) for s in _cfg(k)[1].literal_adaptation] for k in KEYS}
    assert speeds["m7"] == list(sc.GENERIC_SPEEDS) and all(speeds[k] == speeds["m5"] != speeds["m7"] for k in KEYS if k != "m7")
    assert [stc.distance_of(v) for v in (4, 5, 6, 7, 8, 9, 11, 12, 15, 255)] == [1, 2, 3, 4, 8, 8, 8, 8, 8, 8]


def test_the_refused_families():
    cfg = stc.REFUSED["m5_two_models"].pair(po, po)[0]
    assert cfg.context_mixing == 2 and set(bytes(cfg.mixing_mask)) == {5}
    cfg = stc.REFUSED["m5_m6_mixed"].pair(po, po)[0]
    assert cfg.context_mixing == 0 and sorted(set(_reachable(cfg).tolist())) == [5, 6]
    cfg = stc.REFUSED["m5_lsb6_map"].pair(po, po)[0]
    cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)[:64]
    assert cfg.context_mixing == 0 and cfg.prediction_mode == 0 and set(bytes(cfg.mixing_mask)) == {5} and len(set(cmap.tolist())) == 64


@pytest.mark.parametrize("key", KEYS)
def test_oracle_equals_the_second_restatement(key, sources):
    """without a list on the small lengths of lengths(d), with lists on segment_cases' small shapes and the small stride shapes"""
    fam, cfg = _cfg(key)
    data = stc._Content(sources, np.random.default_rng(5 + fam.seed), first=fam.seed)
    for n in [n for n in stc.lengths(fam.dist) if n <= 65] + [300]:
        lit = data.take(n)
        coded = po.lit_encode(cfg, lit) if n else np.zeros(0, np.uint8)
        if n:
            assert rr.encode_stream(to_rr(cfg), lit)[0] == coded.tobytes(), n
            assert rr.decode_stream(to_rr(cfg), coded.tobytes(), n) == lit.tobytes(), n
    names = []
    for name, lit, segs in sc.shapes(fam, sources, small=True) + stc.stride_shapes(fam, sources, small=True):
        assert lit.size <= 1500 and int(segs["len"].sum()) == lit.size
        coded = po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])
        assert rr_segments_encode(cfg, lit, segs) == coded.tobytes(), name
        assert rr_segments_decode(cfg, coded.tobytes(), segs) == lit.tobytes(), name
        if name == "Y_natural":
            assert coded.tobytes() == po.lit_encode(cfg, lit).tobytes()
        names.append(name)
    assert names == ["S1", "S2", "S3", "S4", "S5", "S7", "Y_ones", "Y_cycle", "Y_empty", "Y_base", "Y_natural"]


class _RowTrace(rr.LiteralCoder):
    """the restatement, noting the table and the key (plane, index_b, index_c) of every row it touches"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.rows = []

    def _row(self, table, key):
        self.rows.append(("high" if table is self.high else "low" if table is self.low else "cm", key))
        return rr.LiteralCoder._row(table, key)


@pytest.mark.parametrize("key", KEYS)
def test_both_rows_follow_the_byte_at_the_stride_distance(key, sources):
    """The premise of the stride sort.  Row trace of the restatement over the small stride shapes: position p of a segment that starts
    at q touches the high row (plane 1, b_d, ctx) and the low row (plane 1, b_d, high nibble), where b_d is the stream's own byte
    p - d for p - q >= d and the byte lane at distance d - (p - q) of the segment's last8 before that."""
    fam, cfg = _cfg(key)
    d = fam.dist
    ctx = fam.ctx
    for name, lit, segs in stc.stride_shapes(fam, sources, small=True):
        lc = _RowTrace(**to_rr(cfg))
        enc = rr.AnsEncoder()
        pos, want = 0, []
        for n, bt, l8 in zip(segs["len"].tolist(), segs["btype"].tolist(), segs["last8"].tolist()):
            lc.btype, lc.last_8 = bt, l8
            lc.code_bytes(bytes(lit[pos:pos + n]), n, enc=enc)
            for j in range(n):
                b_d = int(lit[pos + j - d]) if j >= d else (l8 >> (64 - 8 * (d - j))) & 0xFF
                want += [("high", (1, b_d, ctx)), ("low", (1, b_d, int(lit[pos + j]) >> 4))]
            pos += n
        assert lc.rows == want, (key, name)
    # and without a list: zero history in front of the stream
    lit = sources[0][4000:4200]
    lc = _RowTrace(**to_rr(cfg))
    lc.code_bytes(bytes(lit), lit.size, enc=rr.AnsEncoder())
    assert [r[1][1] for r in lc.rows[::2]] == [0] * d + lit[:lit.size - d].tolist()


@pytest.mark.parametrize("key", KEYS)
def test_of_a_last8_exactly_the_lanes_up_to_the_distance_are_read(key, sources):
    """The teeth.  A one-byte segment in the middle of a text reads ONE byte of its last8, the lane at distance d: changing it changes
    the oracle's bytes, changing any other lane does not.  A long segment reads the lanes at distances 1 .. d (its first d
    positions) and none beyond: distance d + 1 changes nothing."""
    fam, cfg = _cfg(key)
    d = fam.dist
    lit = sources[0][20000:23000].copy()
    lane = lambda k: np.uint64((ord("e") ^ ord(" ")) << (64 - 8 * k))      # turns the `e` at distance k into a blank

    def coded(lens, at, flip=None):
        starts = [0] + np.cumsum(lens)[:-1].tolist()
        l8 = np.array([bc.natural_last8(lit, q) for q in starts], np.uint64)
        l8[at] = np.uint64(int.from_bytes(b"e" * 8, "little"))      # not the stream's own; the rows of `e` and of the blank are trained by then
        if flip:
            l8[at] ^= lane(flip)
        return _enc(cfg, lit, sc.segments(lens, np.full(len(lens), fam.btype), l8))

    one = [2000, 1, lit.size - 2001]
    base = coded(one, 1)
    for k in range(1, 9):
        assert (coded(one, 1, flip=k) != base) == (k == d), (key, "one byte", k)
    long = [2000, lit.size - 2000]
    base = coded(long, 1)
    for k in range(1, 9):
        assert (coded(long, 1, flip=k) != base) == (k <= d), (key, "long", k)


@pytest.mark.parametrize("key", KEYS)
def test_the_batches(key, sources):
    """what the GPU tier codes: the lengths without a list, their ragged layout, and the lists"""
    fam = stc.FAMILIES[key]
    d = fam.dist
    assert set(stc.lengths(d)) >= {0, 1, d - 1, d, d + 1, 63, 64, 65, 8191, 8192, 8193, 8192 + d - 1, 8192 + d, 16385, 65535, 65536}
    blocks = stc.plain_streams(fam, sources)
    assert len(blocks) <= 40 and [b.size for b in blocks][:len(stc.lengths(d))] == stc.lengths(d)
    assert sum(b.size == 65536 for b in blocks) == 1
    assert any(b.size > 8192 and len(set(b.tolist())) == 1 for b in blocks)          # a constant byte across a piece base
    buf, offs, sizes = stc.ragged_layout(blocks)
    assert offs[0] == 0 and (offs[1:] % 2 == 1).all() and all(offs[i] + sizes[i] <= offs[i + 1] for i in range(len(blocks) - 1))
    for b, o in zip(blocks, offs):
        assert (buf[int(o):int(o) + b.size] == b).all()
    batches = stc.list_batches(fam, sources)
    assert list(batches) == ["existing_a", "existing_b", "stride"]
    assert [s[0] for s in batches["existing_a"] + batches["existing_b"]] == [s[0] for s in bc.batch(fam, sources)]
    for streams in batches.values():
        assert 0 < len(streams) <= 40
        for name, lit, segs in streams:
            assert int(segs["len"].astype(np.int64).sum()) == lit.size <= 65536, name
            assert segs.size == 0 or int(segs["btype"].max()) < fam.n_btypes, name
    by = {s[0]: s for s in batches["stride"]}
    assert list(by) == ["Y_ones", "Y_cycle", "Y_empty", "Y_base", "Y_natural"]
    assert set(by["Y_ones"][2]["len"].tolist()) == {1}
    assert by["Y_cycle"][2]["len"].tolist()[:2 * d] == list(range(1, d + 1)) * 2
    e = by["Y_empty"][2]["len"].tolist()
    assert e[:5] == [1, 0, 2, 0, 0] and e.count(0) > 100
    starts = set(np.concatenate([[0], np.cumsum(by["Y_base"][2]["len"].astype(np.int64))[:-1]]).tolist())
    assert starts >= {b + k for b in stc.PIECE_BASES for k in range(-d, d + 1)} and by["Y_base"][1].size > stc.PIECE_BASES[1] + d
    _, lit, segs = by["Y_natural"]
    cfg = fam.configure(po.config_simple())
    assert _enc(cfg, lit, segs) == po.lit_encode(cfg, lit).tobytes() and segs.size > 8
    for name in ("Y_ones", "Y_cycle", "Y_empty", "Y_base"):      # random histories: the list changes what is written
        _, lit, segs = by[name]
        assert _enc(cfg, lit, segs) != po.lit_encode(cfg, lit).tobytes(), name
