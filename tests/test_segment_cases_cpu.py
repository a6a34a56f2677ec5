"""The reference of tests/test_gpu_segment_cases.py is the C oracle's segment driver (orc_lit_segments_encode / _decode).  This file
guards the oracle itself on the synthetic segment lists of tests/segment_cases.py: for every configuration family the shapes S1-S5
and S7 (trimmed to what the pure-Python restatement can afford) come out byte for byte as a segment driver over
ref_restatement.LiteralCoder writes them, in both directions, and the oracle refuses lists that do not add up to their stream."""
import numpy as np
import pytest

import pyoracle as po
from ref_restatement import rr_segments_decode, rr_segments_encode
import segment_cases as sc


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_oracle_segment_driver_equals_the_second_restatement(fam, sources):
    cfg = fam.configure(getattr(po, "config_" + fam.base)())
    names = []
    for name, lit, segs in sc.shapes(fam, sources, small=True):
        assert lit.size <= 1500 and int(segs["len"].sum()) == lit.size and int(segs["btype"].max()) < fam.n_btypes
        coded = po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])
        assert rr_segments_encode(cfg, lit, segs) == coded.tobytes(), name
        assert rr_segments_decode(cfg, coded.tobytes(), segs) == lit.tobytes(), name
        assert (po.lit_segments_decode(cfg, coded, lit.size, segs["len"], segs["btype"], segs["last8"]) == lit).all(), name
        if name == "S5":        # one segment, zero history, the configuration's own block type: the plain stream
            assert (coded == po.lit_encode(cfg, lit)).all() and coded.size == po.lit_encode(cfg, lit).size
        names.append(name)
    assert names == ["S1", "S2", "S3", "S4", "S5", "S7"]


def test_an_empty_segment_yields_to_the_one_that_follows(sources):
    """S4's empty segments carry their own block type and history: dropping them changes nothing, changing the segment that follows does"""
    fam = next(f for f in sc.FAMILIES if f.name == "mmx_map_mix")
    cfg = fam.configure(po.config_simple())
    _, lit, segs = next(s for s in sc.shapes(fam, sources, small=True) if s[0] == "S4")
    assert segs["len"].tolist()[0] == 0 and segs["len"].tolist()[2:4] == [0, 0] and segs["len"].tolist()[-1] == 0
    assert all(a != b for a, b in zip(segs["btype"][:-1], segs["btype"][1:]))
    enc = lambda s: po.lit_segments_encode(cfg, lit, s["len"], s["btype"], s["last8"]).tobytes()
    full = enc(segs)
    assert enc(segs[segs["len"] > 0]) == full
    other = segs.copy(); other["btype"][4] = (int(other["btype"][4]) + 1) % fam.n_btypes
    assert enc(other) != full
    other = segs.copy(); other["last8"][4] = ~other["last8"][4]
    assert enc(other) != full


def test_the_families_cover_every_instance_of_the_dispatch():
    triples = {(f.mm, f.ctxc, f.mix) for f in sc.FAMILIES}
    assert triples == {(mm, c, m) for mm in (4, 0, -1) for c in (True, False) for m in (True, False)}
    assert {(f.mm, f.ctxc, f.mix) for f in sc.FAMILIES if f.cached} == triples
    assert any(not f.cached for f in sc.FAMILIES) and any(f.n_btypes == 1 for f in sc.FAMILIES)
    for f in sc.FAMILIES:        # what the kernels' dispatch will see in the mixing mask
        cfg = f.configure(getattr(po, "config_" + f.base)())
        mask = np.frombuffer(bytes(cfg.mixing_mask), np.uint8)
        vals = set(mask[7 + 256 * np.arange(32)].tolist() if f.ctxc and f.mm < 0 else mask.tolist())      # (a constant context reaches 32 entries)
        assert vals == ({f.mm} if f.mm >= 0 else set(sc.MM_GENERIC_CACHED if f.cached else sc.MM_GENERIC)), f


def test_full_batch_layout(sources):
    fam = sc.FAMILIES[0]
    streams = sc.shapes(fam, sources)
    assert len(streams) == sc.N_STREAMS == 40
    names = [s[0] for s in streams]
    assert names[sc.EMPTY_AT] == "S0" and streams[sc.EMPTY_AT][1].size == 0 and streams[sc.EMPTY_AT][2].size == 0
    assert names.count("S6") == 1 and set(names) >= {"S0", "S1", "S2", "S3", "S4", "S5", "S6", "S7"}
    for name, lit, segs in streams:
        assert int(segs["len"].astype(np.int64).sum()) == lit.size, name
    by = {s[0]: s for s in streams}
    assert by["S2"][2]["len"].tolist() == [1] * 600
    assert np.cumsum(by["S3"][2]["len"]).tolist() == [15, 16, 17, 31, 32, 33, 47, 48, 49, 1000, 3000]
    assert np.cumsum(by["S6"][2]["len"]).tolist() == [32767, 32768, 32769, 40000]
    assert by["S7"][2]["len"].tolist()[:99] == list(range(1, 100)) and by["S7"][1].size == 5000
    assert by["S7"][2]["btype"].tolist()[:10] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    assert by["S5"][2].tolist() == [(3000, fam.btype, 0)]


def test_oracle_refuses_lists_that_do_not_add_up(sources):
    fam = sc.FAMILIES[0]
    cfg = fam.configure(getattr(po, "config_" + fam.base)())
    streams = sc.shapes(fam, sources)
    bad, which = sc.bad_lists(streams)
    assert which == (3, 5, 9)
    for i, (name, lit, segs) in enumerate(bad):
        good = streams[i]
        coded = po.lit_segments_encode(cfg, good[1], good[2]["len"], good[2]["btype"], good[2]["last8"])
        if i not in which:
            assert (segs == good[2]).all()
            continue
        assert int(segs["len"].astype(np.int64).sum()) - lit.size == {3: -7, 5: 7, 9: -lit.size}[i]
        with pytest.raises(RuntimeError):
            po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])
        with pytest.raises(RuntimeError):
            po.lit_segments_decode(cfg, coded, lit.size, segs["len"], segs["btype"], segs["last8"])
