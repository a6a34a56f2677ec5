"""The reference of tests/test_gpu_plain_decoders.py is the C oracle's plain stream coder (orc_lit_stream_encode / _decode).  This file
guards the oracle on exactly the batches of tests/plain_decoder_cases.py: every stream of every family reads back, the nine streams whose
coded size sits at a refill point of the decoders' word ring are found, the streams of at most 400 bytes come out byte for byte as
ref_restatement.encode_stream writes them, and the block type a call without a list codes under changes the bytes."""
import numpy as np
import pytest

import plain_decoder_cases as pc
import pyoracle as po
import ref_restatement as rr
import segment_cases as sc
from ref_restatement import to_rr

_BATCHES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _batch(fam, sources):
    """(oracle configuration of a call without a list, streams, the oracle's bytes): computed once, shared, never written to"""
    if fam.name not in _BATCHES:
        ocfg = pc.oracle_config(fam, fam.configure(getattr(po, "config_" + fam.base)()))
        streams = pc.shapes(fam, sources)
        _BATCHES[fam.name] = (ocfg, streams, pc.oracle_bytes(ocfg, streams))
    return _BATCHES[fam.name]


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_oracle_reads_back_every_stream(fam, sources):
    ocfg, streams, coded = _batch(fam, sources)
    assert [s[0] for s in streams] == pc.ORDER and len(streams) == pc.N_STREAMS
    assert ocfg.btype == (0 if fam.n_btypes > 1 else fam.btype)
    for (name, lit), c in zip(streams, coded):
        assert c.size % 4 == 0 and (c.size == 0) == (lit.size == 0), name
        assert (po.lit_decode(ocfg, c, lit.size) == lit).all(), (fam.name, name)
    assert po.lit_encode(ocfg, np.zeros(0, np.uint8)).size == 0          # the empty stream: no chunk, no states


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_ring_targets_are_found(fam, sources):
    ocfg, streams, coded = _batch(fam, sources)
    words = {name: c.size // 4 for (name, _), c in zip(streams, coded)}
    chosen = {name: lit.size for name, lit in streams if name.startswith("W")}
    assert len(chosen) == len(pc.RING_WORDS) == 9, chosen
    for w in pc.RING_WORDS:
        assert words[f"W{w}"] == w and 1 <= chosen[f"W{w}"] <= pc.RING_SEARCH, f"{fam.name}: lengths chosen {chosen}, coded words {words}"


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_oracle_equals_the_second_restatement_on_the_short_streams(fam, sources):
    ocfg, streams, coded = _batch(fam, sources)
    cfg = to_rr(ocfg)
    short = [(name, lit, c) for (name, lit), c in zip(streams, coded) if 0 < lit.size <= 400]
    assert {f"O{n}" for n in pc.OUTPUT_GROUP} | {f"W{w}" for w in pc.RING_WORDS} <= {s[0] for s in short}
    for name, lit, c in short:
        assert rr.encode_stream(cfg, lit)[0] == c.tobytes(), (fam.name, name, lit.size)


@pytest.mark.parametrize("fam", [f for f in sc.FAMILIES if f.n_btypes == 8 and not f.ctxc], ids=repr)
def test_the_block_type_of_a_call_without_a_list_changes_the_bytes(fam, sources):
    """eight tables: the call codes under table 0, not under the configuration's own block type (3).  Under a table-driven mask the
    eight maps are unrelated (and the mask itself is read by context), so the bytes differ.  The families with mixing value 4 or 0
    everywhere give every block type another BIJECTION of the 64 contexts (segment_cases.Family.configure): over a whole stream that
    only renames rows which all start from the default row, so table 3 writes table 0's bytes -- there the bytes cannot tell which
    table a call without a list took, and this test says so instead of claiming it."""
    ocfg, streams, coded = _batch(fam, sources)
    own = fam.configure(getattr(po, "config_" + fam.base)())
    assert own.btype == 3 and ocfg.btype == 0
    by = {s[0]: i for i, s in enumerate(streams)}
    reads_context = fam.mm < 0
    for name in ("R0", "O49", "C32769"):
        lit = streams[by[name]][1]
        other = po.lit_encode(own, lit)
        differs = other.size != coded[by[name]].size or bool((other != coded[by[name]]).any())
        assert differs == reads_context, (fam.name, name)


def test_layouts(sources):
    fam = sc.FAMILIES[0]
    ocfg, streams, coded = _batch(fam, sources)
    buf, blank, offs, sizes = pc.literal_layout(streams)
    assert buf.size == blank.size == int(sizes.sum()) + sum(1 + i % 3 for i in range(len(streams))) + pc.TAIL
    assert (blank == pc.SENTINEL).all() and (buf[-pc.TAIL:] == pc.SENTINEL).all()
    for (name, lit), o in zip(streams, offs):
        assert (buf[int(o):int(o) + lit.size] == lit).all() and buf[int(o) - 1] == pc.SENTINEL, name
    cbuf, coffs, csizes = pc.coded_layout(coded)
    assert (coffs % 4 == 0).all() and (np.diff(coffs) == csizes[:-1]).all() and (cbuf[-pc.TAIL:] == pc.SENTINEL).all()
    data, cuts = pc.resumed_stream(sources)
    assert cuts[1:9] == [1, 2, 3, 7, 8, 9, 10, 17] and max(b - a for a, b in zip(cuts[:-1], cuts[1:])) <= 32768
