"""Guards what tests/test_gpu_ctx_bucketed.py compares against and codes: the oracle's segment driver under the mixing-value-0
families against the second restatement, the shapes tests/ctx_bucketed_cases.py adds (their lists add up, their streams fit a
64 KiB slot, and each has teeth: the block type of a segment that spans a piece base matters, empty segments do not), and the
premise of the context-keyed pass: under uniform mixing value 0 the coded bytes depend on a position's context alone.

The restatement is pure Python (a few KB/s), so it codes the new shapes at a 32nd of their length (new_shapes(small=True)): it knows
no pieces, and the lists keep their order of lengths, block types and histories.  The teeth are shown on the full shapes."""
import ctypes

import numpy as np
import pytest

import bucketed_segment_cases as bc
import ctx_bucketed_cases as cc
import pyoracle as po
import segment_cases as sc
from ref_restatement import rr_segments_decode, rr_segments_encode

KEYS = list(cc.FAMILIES)


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _cfg(key):
    fam = cc.FAMILIES[key]
    return fam, fam.configure(getattr(po, "config_" + fam.base)())


def _enc(cfg, lit, segs):
    return po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"]).tobytes()


@pytest.mark.parametrize("key", ["plain", "mix"])
def test_oracle_segment_driver_equals_the_second_restatement(key, sources):
    fam, cfg = _cfg(key)
    assert set(bytes(cfg.mixing_mask)) == {0} and cfg.context_mixing == (2 if fam.mix else 0) and fam.n_btypes == 8
    cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)
    assert len({cmap[64 * t:64 * t + 64].tobytes() for t in range(8)}) == 8        # a wrong block type is another map
    names = []
    for name, lit, segs in sc.shapes(fam, sources, small=True) + cc.new_shapes(fam, sources, small=True):
        assert lit.size <= 2100 and int(segs["len"].sum()) == lit.size
        coded = po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])
        assert rr_segments_encode(cfg, lit, segs) == coded.tobytes(), name
        assert rr_segments_decode(cfg, coded.tobytes(), segs) == lit.tobytes(), name
        names.append(name)
    assert names == ["S1", "S2", "S3", "S4", "S5", "S7", "X_span", "X_bt_ones", "X_empty_bt"]


@pytest.mark.parametrize("key", KEYS)
def test_every_list_adds_up_and_every_stream_fits_a_slot(key, sources):
    fam = cc.FAMILIES[key]
    streams = cc.batch(fam, sources)
    assert len(streams) == sc.N_STREAMS + 7
    names = [s[0] for s in streams]
    assert [n for n in names if n.startswith("X_")] == ["X_span", "X_edges", "X_slot", "X_ones", "X_bt_ones", "X_empty", "X_empty_bt"]
    assert names.index("X_span") < 24 < names.index("X_bt_ones")           # both launch sequences of 24 hold new shapes
    for name, lit, segs in streams:
        assert int(segs["len"].astype(np.int64).sum()) == lit.size <= 65536, name
        assert segs.size == 0 or int(segs["btype"].max()) < fam.n_btypes, name
        if fam.n_btypes == 1:
            assert (segs["btype"] == fam.btype).all(), name
    by = {s[0]: s for s in streams}
    span = by["X_span"]
    assert span[1].size == 65536 and span[2]["len"].tolist() == cc.SPAN_LENS
    starts = np.concatenate([[0], np.cumsum(cc.SPAN_LENS)[:-1]])
    assert sorted(set(range(8)) - set((starts // cc.PIECE).tolist())) == [1, 3, 4, 5, 7]       # pieces without a segment start
    assert 24000 in starts.tolist() and 24000 % cc.PIECE != 0                                   # a block type changes mid-piece
    ones = by["X_bt_ones"][2]
    assert ones["len"].tolist()[1:-1] == [1] * 300 and ones["len"][0] < cc.PIECE < ones["len"][0] + 300
    e = by["X_empty_bt"][2]
    assert e["len"].tolist() == [0, cc.PIECE, 0, 0, 12000 - cc.PIECE]
    if fam.n_btypes > 1:
        assert len(set(span[2]["btype"].tolist())) == 5 and len(set(ones["btype"].tolist())) == 8
        bt = e["btype"].tolist()
        assert bt[0] != bt[1] and bt[2] not in (bt[1], bt[4]) and bt[3] not in (bt[1], bt[4])


def test_the_block_type_of_a_segment_that_spans_a_piece_base_matters(sources):
    """X_span: every segment but the first covers a piece base it does not start in; naming another block type for any of them
    changes the oracle's bytes, for both model counts"""
    for key in ("plain", "mix"):
        fam, cfg = _cfg(key)
        _, lit, segs = cc.new_shapes(fam, sources)[0]
        full = _enc(cfg, lit, segs)
        for k in (1, 2, 3, 4):
            other = segs.copy(); other["btype"][k] = (int(other["btype"][k]) + 1) % 8
            assert _enc(cfg, lit, other) != full, (key, k)


def test_one_byte_segments_take_their_own_block_type(sources):
    fam, cfg = _cfg("mix")
    _, lit, segs = cc.new_shapes(fam, sources)[1]
    full = _enc(cfg, lit, segs)
    for k in (1, 150, 151, 300):          # the first of the run, the ones on both sides of the piece base, the last
        other = segs.copy(); other["btype"][k] = (int(other["btype"][k]) + 3) % 8
        assert _enc(cfg, lit, other) != full, k


def test_empty_segments_install_nothing_that_lasts(sources):
    """X_empty_bt: dropping the empty segments, or giving them any block type or history, changes nothing; the block type of the
    non-empty segment behind them does"""
    for key in ("plain", "mix"):
        fam, cfg = _cfg(key)
        _, lit, segs = cc.new_shapes(fam, sources)[2]
        full = _enc(cfg, lit, segs)
        assert _enc(cfg, lit, segs[segs["len"] > 0]) == full
        for k in (0, 2, 3):
            other = segs.copy(); other["btype"][k] = (int(other["btype"][k]) + 1) % 8; other["last8"][k] = ~other["last8"][k]
            assert _enc(cfg, lit, other) == full, (key, k)
        other = segs.copy(); other["btype"][4] = int(segs["btype"][3])
        assert _enc(cfg, lit, other) != full, key


@pytest.mark.parametrize("mix", [False, True])
def test_the_row_is_a_function_of_the_context_alone(mix, sources):
    """The premise of the context-keyed sort.  Under uniform mixing value 0 two configurations whose (block type, prev, class of
    prev_prev) -> context tables agree on a stream's positions write the same bytes whatever else their maps hold: a stream without a
    list reads the 64 map entries of its own block type only, and the second configuration differs in every other entry.  More: the
    context NAMES the rows and nothing else, so a third configuration whose map is the first one's under a permutation of the 256
    context values -- the same partition of the positions into buckets -- writes the same bytes again.  Another partition does not."""
    fam = cc.FAMILIES["mix" if mix else "plain"]
    a = fam.configure(po.config_context_mixing())
    bt = int(a.btype)
    assert bt == 3 and set(bytes(a.mixing_mask)) == {0}
    cmap = np.frombuffer(bytes(a.literal_context_map), np.uint8).copy()
    own = slice(64 * bt, 64 * bt + 64)
    lit = sources[0][3000:9000]
    coded = po.lit_encode(a, lit).tobytes()

    def with_map(m):
        c = po.LitConfig.from_buffer_copy(bytes(a))
        ctypes.memmove(c.literal_context_map, m.ctypes.data, m.size)
        return c

    other = ((cmap.astype(np.int64) * 7 + 13) % 256).astype(np.uint8)
    other[own] = cmap[own]
    assert (other[:64] != cmap[:64]).any() and (other[64 * bt + 64:] != cmap[64 * bt + 64:]).any()
    assert po.lit_encode(with_map(other), lit).tobytes() == coded
    perm = np.random.default_rng(5).permutation(256).astype(np.uint8)
    renamed = cmap.copy(); renamed[own] = perm[cmap[own]]
    assert renamed[own].max() > 63 and (renamed[own] != cmap[own]).any()
    assert po.lit_encode(with_map(renamed), lit).tobytes() == coded
    merged = cmap.copy(); merged[own] = cmap[own] // 2
    assert po.lit_encode(with_map(merged), lit).tobytes() != coded


def test_the_helpers_for_the_other_gpu_cases(sources):
    for mode in range(4):
        cfg = cc.mode_config(po.config_context_mixing(), mode, True, mode)
        cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)
        assert set(bytes(cfg.mixing_mask)) == {0} and cmap[:128].max() == 255 and len(set(cmap[:128].tolist())) > 64
        assert cmap[:64].tobytes() != cmap[64:128].tobytes()
    for n in (1, 2, 65536):
        blocks = cc.plain_streams(n, sources)
        assert len(blocks) == 40 and all(b.size == n for b in blocks) and not blocks[1].any() and set(blocks[2].tolist()) <= {97, 98}
    buf, offs, sizes = cc.ragged_layout(cc.plain_streams(63, sources))
    assert (offs % 16 == 0).sum() >= 10 and (offs % 16 != 0).sum() >= 20
