"""Guards what tests/test_gpu_caller_streams.py runs and compares against (tests/caller_stream_cases.py): the families are the
existing case modules' own, none with a table-driven mixing mask; both rounds' batches have the shape the GPU test relies on
(37 ragged streams of at most 300 bytes, one empty, one of 300, lists that add up) and differ from each other; the oracle's bytes
decode back under their lists, equal the list-free coder under the natural one-segment list, and -- a few streams of every family,
the restatement being pure Python -- equal the second restatement's."""
import numpy as np
import pytest

import caller_stream_cases as cs
import pyoracle as po
import segment_cases as sc
import stride_bucketed_cases as st
from ref_restatement import rr_segments_decode, rr_segments_encode

KEYS = list(cs.FAMILIES)


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def test_no_family_has_a_table_driven_mask():
    for key, fam in cs.FAMILIES.items():
        cfg = fam.configure(getattr(po, "config_" + fam.base)())
        assert cs.uniform_mask_value(cfg) in (0, 4), key
    # ... and the check would see one: a table-driven family of tests/segment_cases.py, and every stride family
    generic = next(f for f in sc.FAMILIES if f.mm < 0)
    assert cs.uniform_mask_value(generic.configure(getattr(po, "config_" + generic.base)())) is None
    assert not set(map(id, cs.FAMILIES.values())) & {id(f) for f in vars(st).get("FAMILIES", {}).values()}
    cs.assert_no_generic_instance("divans_hip::lit_decode2_kernel_w7<4, true, false, false, 17>")
    with pytest.raises(AssertionError):
        cs.assert_no_generic_instance("divans_hip::lit_decode2_kernel_any<-1, true, false, true, 17>")


@pytest.mark.parametrize("key", KEYS)
def test_small_batches_have_the_shape_the_gpu_test_relies_on(key, sources):
    fam, o, rounds = cs.oracle(po, key, sources)
    assert len(rounds) == cs.ROUNDS == 2
    for r in rounds:
        streams = r["streams"]
        sizes = [lit.size for _, lit, _ in streams]
        assert len(streams) == 37 and max(sizes) == 300 == sizes[0] and sizes.count(0) == 1 and sizes[cs.EMPTY_AT] == 0
        for (name, lit, segs), coded in zip(streams, r["listed"]):
            assert int(segs["len"].sum()) == lit.size and (segs.size == 0 or int(segs["btype"].max()) < fam.n_btypes), name
            assert coded.size % 4 == 0
            if lit.size:
                assert (po.lit_segments_decode(o, coded, lit.size, segs["len"], segs["btype"], segs["last8"]) == lit).all(), name
        assert any((segs["len"] == 0).any() for _, lit, segs in streams if lit.size)
        if fam.n_btypes > 1:
            assert len({int(b) for _, _, segs in streams for b in segs["btype"]}) == fam.n_btypes
        if key in cs.LIST_ONLY:
            assert r["plain"] is None and max(int(b) for _, _, segs in streams for b in segs["btype"]) == 8
    a, b = rounds
    # a stale read of the other round is a wrong answer: no stream of one round is coded like the same stream of the other
    for i in range(37):
        if i != cs.EMPTY_AT:
            assert a["listed"][i].tobytes() != b["listed"][i].tobytes(), i


@pytest.mark.parametrize("key", KEYS)
def test_oracle_bytes_against_the_second_restatement(key, sources):
    fam, o, rounds = cs.oracle(po, key, sources)
    streams = rounds[0]["streams"]
    picked = sorted(range(37), key=lambda i: abs(streams[i][1].size - 120))[:2]      # two streams of about 120 bytes
    for i in picked:
        name, lit, segs = streams[i]
        coded = rounds[0]["listed"][i]
        assert rr_segments_encode(o, lit, segs) == coded.tobytes(), (key, name)
        assert rr_segments_decode(o, coded.tobytes(), segs) == lit.tobytes(), (key, name)
    if rounds[0]["plain"] is not None:
        for i in picked:
            name, lit, _ = streams[i]
            nat = cs.natural_segments(fam, lit)
            assert po.lit_segments_encode(o, lit, nat["len"], nat["btype"], nat["last8"]).tobytes() == rounds[0]["plain"][i].tobytes(), (key, name)


def test_packed_layout_is_a_prefix_sum_of_rounded_sizes():
    coded = [np.zeros(n, np.uint8) for n in (8, 0, 5, 12, 1)]
    offs, total = cs.packed_layout(coded)
    assert offs.tolist() == [0, 8, 8, 16, 28] and total == 32
