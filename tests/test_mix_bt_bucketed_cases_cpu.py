"""Guards what tests/test_gpu_mix_bt_bucketed.py compares against and codes: the oracle's segment driver under the families of
tests/mix_bt_bucketed_cases.py (mixing value 4, two models, several block types) against the second restatement; the lists and the
slot counts; the teeth of the shapes (the block type of a segment matters, of an empty one does not); and the premise of the stride
model's sort under block types: a context only NAMES the high row of its (previous byte) bucket.

The restatement is pure Python (a few KB/s) and codes the small shapes; the teeth are shown on the full ones."""
import ctypes

import numpy as np
import pytest

import ctx_bucketed_cases as cc
import mix_bt_bucketed_cases as mc
import pyoracle as po
import segment_cases as sc
from ref_restatement import rr_segments_decode, rr_segments_encode

KEYS = list(mc.FAMILIES)


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _cfg(fam):
    return fam.configure(getattr(po, "config_" + fam.base)())


def _enc(cfg, lit, segs):
    return po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"]).tobytes()


@pytest.mark.parametrize("key", ["c8", "u2"])
def test_oracle_segment_driver_equals_the_second_restatement(key, sources):
    fam = mc.FAMILIES[key]
    cfg = _cfg(fam)
    assert set(bytes(cfg.mixing_mask)) == {4} and cfg.context_mixing == 2 and cfg.prediction_mode == 2 and fam.base == "context_mixing"
    names = []
    for name, lit, segs in mc.small_shapes(fam, sources):
        assert lit.size <= 2100 and int(segs["len"].sum()) == lit.size
        coded = po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])
        assert rr_segments_encode(cfg, lit, segs) == coded.tobytes(), name
        assert rr_segments_decode(cfg, coded.tobytes(), segs) == lit.tobytes(), name
        names.append(name)
    assert names == ["S1", "S2", "S3", "S4", "S5", "S7", "X_span", "X_bt_ones", "X_empty_bt", "X_all_slots"]


@pytest.mark.parametrize("key", KEYS)
def test_every_list_adds_up_and_every_stream_fits_a_slot(key, sources):
    fam = mc.FAMILIES[key]
    streams = mc.batch(fam, sources)
    assert len(streams) == sc.N_STREAMS + 8
    names = [s[0] for s in streams]
    assert names.index("X_all_slots") == mc.ALL_SLOTS_AT < 24 < names.index("X_bt_ones")
    for name, lit, segs in streams:
        assert int(segs["len"].astype(np.int64).sum()) == lit.size <= 65536, name
        assert segs.size == 0 or int(segs["btype"].max()) < fam.n_btypes, name
    assert max(s[1].size for s in streams) == 65536
    _, lit, segs = streams[mc.ALL_SLOTS_AT]
    assert lit.size == 4000 and set(lit.tolist()) == {ord("a")} and segs.size == 64
    assert 1 <= int(segs["len"].min()) and int(segs["len"].max()) <= 200
    assert segs["btype"].tolist() == [k % fam.n_btypes for k in range(64)]
    natural = [int(l8) >> 56 == (ord("a") if q else 0) for l8, q in zip(segs["last8"].tolist(), np.concatenate([[0], np.cumsum(segs["len"])[:-1]]).tolist())]
    assert sum(natural) >= 55 and not all(natural[::8])
    # the bucket of prev = 'a' uses every high row the chain keeps: (a, a) under the block types alone reaches all of them
    cfg = _cfg(fam)
    lut1 = np.zeros(256, np.uint8); lut0 = np.zeros(256, np.uint8)
    po.lib().orc_get_lut0(int(cfg.prediction_mode), lut0.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    po.lib().orc_get_lut1(int(cfg.prediction_mode), lut1.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)
    mine = mc.contexts_by_prev(cfg, fam.n_btypes)[ord("a")]
    used = {mine.index(int(cmap[((int(lut0[97]) | int(lut1[97])) & 63) + 64 * t])) for t in range(fam.n_btypes)}
    if fam.n_btypes == 8:
        assert used == set(range(8))
    else:
        assert len(used) == fam.n_btypes


def test_the_slot_counts():
    for key, fam in mc.FAMILIES.items():
        cfg = _cfg(fam)
        assert mc.high_row_slots(cfg, fam.n_btypes) == 8, key
    per_prev = [len(s) for s in mc.contexts_by_prev(_cfg(mc.FAMILIES["c8"]), 8)]
    assert set(per_prev) == {8}                                     # exactly 8 for every prev
    cmap = mc.clustered_map()
    assert len({cmap[64 * t:64 * t + 64].tobytes() for t in range(8)}) == 8        # the eight tables differ pairwise
    assert sorted(set(cmap[:512].tolist())) == sorted(mc.CLUSTER_VALUES)
    for name, (fam, count) in mc.REFUSED.items():
        assert mc.high_row_slots(_cfg(fam), fam.n_btypes) == count, name
    assert [c for _, c in mc.REFUSED.values()] == [9, 9, 12, 31]
    # one block type: what divans_gpu_codec_high_row_slots reports for a codec as it is created
    assert mc.high_row_slots(_cfg(mc.FAMILIES["c8"]), 1) <= 4


@pytest.mark.parametrize("key", KEYS)
def test_the_block_type_of_a_segment_matters_and_of_an_empty_one_does_not(key, sources):
    fam = mc.FAMILIES[key]
    cfg = _cfg(fam)
    nb = fam.n_btypes
    _, lit, segs = mc.all_slots(fam)
    full = _enc(cfg, lit, segs)
    for k in (0, 1, 31, 63):
        other = segs.copy(); other["btype"][k] = (int(other["btype"][k]) + 1) % nb
        assert _enc(cfg, lit, other) != full, (key, "X_all_slots", k)
    shapes = {s[0]: s for s in cc.new_shapes(fam, sources)}
    _, lit, segs = shapes["X_span"]                      # every segment but the first covers a piece base it does not start in
    full = _enc(cfg, lit, segs)
    for k in (1, 2, 3, 4):
        other = segs.copy(); other["btype"][k] = (int(other["btype"][k]) + 1) % nb
        assert _enc(cfg, lit, other) != full, (key, "X_span", k)
    _, lit, segs = shapes["X_empty_bt"]
    full = _enc(cfg, lit, segs)
    assert _enc(cfg, lit, segs[segs["len"] > 0]) == full
    for k in (0, 2, 3):
        other = segs.copy(); other["btype"][k] = (int(other["btype"][k]) + 1) % nb; other["last8"][k] = ~other["last8"][k]
        assert _enc(cfg, lit, other) == full, (key, "X_empty_bt", k)


def test_a_context_only_names_the_high_row(sources):
    """The premise of mix_bt_sort_kernel: under mixing value 4 the stride model's rows are high [ctx][prev] and low [prev][hi], the
    context model's First[ctx] and Second[hi][ctx] -- a context value is a NAME and nothing else.  c8 under a permutation of the 256
    context values (the same partition of every bucket's positions into high rows) writes the same bytes; merging two contexts
    (two block types of one previous byte then share a row) does not."""
    fam = mc.FAMILIES["c8"]
    a = _cfg(fam)
    cmap = np.frombuffer(bytes(a.literal_context_map), np.uint8).copy()
    streams = [mc.all_slots(fam)] + cc.new_shapes(fam, sources, small=True)
    coded = [_enc(a, lit, segs) for _, lit, segs in streams]

    def with_map(m):
        c = po.LitConfig.from_buffer_copy(bytes(a))
        ctypes.memmove(c.literal_context_map, m.ctypes.data, m.size)
        return c

    perm = np.random.default_rng(11).permutation(256).astype(np.uint8)
    renamed = perm[cmap]
    assert (renamed[:512] != cmap[:512]).any() and len(set(renamed[:512].tolist())) == 8
    assert [_enc(with_map(renamed), lit, segs) for _, lit, segs in streams] == coded
    merged = cmap.copy(); merged[merged == 255] = 128
    assert len(set(merged[:512].tolist())) == 7
    assert all(x != y for x, y in zip([_enc(with_map(merged), lit, segs) for _, lit, segs in streams], coded))
