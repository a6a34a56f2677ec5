"""The reference of the GPU tests with more than eight literal block types is the C oracle's segment driver, which takes any block
type below 256.  This file guards it on the families of tests/wide_block_type_cases.py: the small shapes come out byte for byte as a
segment driver over ref_restatement.LiteralCoder writes them, the 256 rows of every family's context map differ pairwise, and the
oracle's bytes change when the high block types of a list are folded onto the first eight -- so a kernel that did that could not
pass the GPU tier."""
import numpy as np
import pytest

import pyoracle as po
import segment_cases as sc
import wide_block_type_cases as wc
from ref_restatement import rr_segments_decode, rr_segments_encode


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _cfg(fam):
    return fam.configure(getattr(po, "config_" + fam.base)())


@pytest.mark.parametrize("fam", wc.FAMILIES, ids=repr)
def test_oracle_segment_driver_equals_the_second_restatement(fam, sources):
    cfg = _cfg(fam)
    seen = set()
    for name, lit, segs in sc.shapes(fam, sources, small=True):
        assert lit.size <= 1500 and int(segs["len"].sum()) == lit.size and int(segs["btype"].max()) < fam.n_btypes
        seen.update(segs["btype"].tolist())
        coded = po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])
        assert rr_segments_encode(cfg, lit, segs) == coded.tobytes(), name
        assert rr_segments_decode(cfg, coded.tobytes(), segs) == lit.tobytes(), name
        assert (po.lit_segments_decode(cfg, coded, lit.size, segs["len"], segs["btype"], segs["last8"]) == lit).all(), name
    assert max(seen) >= 8 and (fam.n_btypes == 9 or len(seen) > 100), (fam, sorted(seen))      # the lists do name the high types


def test_the_families_are_the_ones_the_dispatch_needs():
    wide = {(f.mm, f.mix, f.n_btypes) for f in wc.WIDE}
    assert wide >= {(mm, mix, 256) for mm in (4, 0, -1) for mix in (False, True)} | {(4, False, 9), (-1, True, 9)}
    assert {(f.mm, f.mix) for f in wc.WIDE if not f.cached and f.n_btypes == 256} == {(mm, mix) for mm in (4, 0, -1) for mix in (False, True)}
    assert {(f.mm, f.mix, f.n_btypes) for f in wc.CONST} == {(4, False, 256), (4, True, 256)}
    modes = {f.name: _cfg(f).prediction_mode for f in wc.FAMILIES}
    assert modes["mm4_map_plain_bt256_lsb6"] == wc.LSB6 and modes["mm0_map_mix_bt256_sign"] == wc.SIGN
    for f in wc.WIDE:
        cmap = np.frombuffer(bytes(_cfg(f).literal_context_map), np.uint8)
        assert cmap.max() == (255 if not f.cached else (31 if f.mm < 0 else 63)), f      # row caches exist below 32 767 rows per stream
        assert len(set(cmap.tolist())) > 1, f
    for f in wc.CONST:
        assert len(set(bytes(_cfg(f).literal_context_map))) == 1, f


@pytest.mark.parametrize("fam", wc.WIDE, ids=repr)
def test_all_256_rows_of_the_context_map_differ_pairwise(fam):
    cmap = np.frombuffer(bytes(_cfg(fam).literal_context_map), np.uint8).reshape(256, 64)
    assert len({r.tobytes() for r in cmap}) == 256
    if fam.mm >= 0 and fam.cached:     # the affine maps: a bijection of the 64 contexts per type
        assert all(sorted(r.tolist()) == list(range(64)) for r in cmap)


@pytest.mark.parametrize("fam", wc.WIDE, ids=repr)
def test_folding_the_high_block_types_changes_the_coded_bytes(fam, sources):
    """the stream of one-byte segments (S2: a block type and a history of its own per byte)"""
    cfg = _cfg(fam)
    _, lit, segs = next(s for s in sc.shapes(fam, sources) if s[0] == "S2")      # the 600 bytes the GPU tier codes
    assert segs["len"].tolist() == [1] * lit.size and int(segs["btype"].max()) >= 8
    enc = lambda s: po.lit_segments_encode(cfg, lit, s["len"], s["btype"], s["last8"]).tobytes()
    full = enc(segs)
    for how in ("minus8", "and7"):
        folded = wc.fold(segs, how)
        assert int(folded["btype"].max()) < max(8, fam.n_btypes - 8) and (folded["btype"] != segs["btype"]).any()
        assert enc(folded) != full, how
