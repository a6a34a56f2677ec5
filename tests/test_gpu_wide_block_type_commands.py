"""The command entry points with more than eight literal block types: every family of tests/wide_block_type_cases.py decodes the
directed command batch of tests/command_cases.py from the C ORACLE's bytes -- without history, and with histories of the streams'
own (tests/history_cases.py, mode "own") -- and encodes it from raw bytes and lists under encode path 0, then round trips.  Both
builders cycle their Literal commands through fam.n_btypes: the 300 one-byte literals of command_cases walk all 256 rows of the context
map, the short lists of history_cases the first eleven.
Where the context map is not constant the kernels are the wide instances, spelt with one trailing template argument."""
import pytest

import command_cases as cc
import gpu_harness as gh
import history_cases as hc
import pyoracle as po
import wide_block_type_cases as wc

pytestmark = pytest.mark.gpu
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(fam, sources, history):
    """configurations, streams, the oracle's bytes, the layout (and the histories' layout): computed once, shared, never written to"""
    if (fam.name, history) not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        if history:
            _CASES[fam.name, history] = (g, o) + gh.history_batch(fam, o, hc.directed(fam, sources, "own"), "own")
        else:
            streams = cc.directed(fam, sources)
            coded = gh.oracle_bytes(o, streams)
            _CASES[fam.name, history] = (g, o, streams, coded, cc.layout(streams, coded), None)
    return _CASES[fam.name, history]


def _kernel(fam, hist):
    mm = fam.mm if fam.mm >= 0 else -1
    caches = (19 if fam.mix else 17) if fam.cached else 0
    return f"divans_hip::lit_decode2_cmd_{'hist_' if hist else ''}kernel<{mm}, {gh.tf(fam.ctxc)}, {gh.tf(fam.mix)}, {caches}{'' if fam.ctxc else ', 1'}>"


def test_the_directed_lists_walk_every_block_type(sources):
    fam = wc.by_name("mm4_map_plain_bt256")
    types = lambda streams: {t for s in streams for t in s["segs"]["btype"].tolist()}
    assert types(cc.directed(fam, sources)) == set(range(256))
    assert max(types(hc.directed(fam, sources, "own"))) >= 8      # (short lists: a few types, some of them behind the fused layout's eight)


@pytest.mark.parametrize("fam", wc.FAMILIES, ids=repr)
def test_directed_batch_without_history(fam, sources):
    import torch
    import divans_amd as da
    g, o, streams, coded, lay, _ = _case(fam, sources, False)
    t = gh.to_device(torch, lay)
    codec = gh.codec_for(da, fam, g, lay["lit_longest"])
    for what, setup in (("2 workgroups", lambda c: c.set_geometry(blocks=2)), ("1 workgroup", lambda c: c.set_geometry(blocks=1)),
                        ("direct-mapped decoder asked for", lambda c: c.set_decoder(2))):
        setup(codec)
        st, raw, flags, name = gh.decode_commands(torch, codec, lay, t)
        assert st == 0 and name == _kernel(fam, False), (what, st, name)
        gh.assert_raw(raw, lay, streams, what)
        assert not flags.any(), what
    # the encode call from the raw bytes and the lists, path 0: the oracle's bytes, then back through the decoder
    elay = gh.encode_layout(lay)
    res = gh.encode_commands(torch, codec, elay, gh.to_device(torch, elay))
    assert res["status"] == 0 and not res["flags"].any() and codec.last_encode_path() == 1, (res["status"], res["flags"].tolist(), codec.last_encode_path())
    gh.assert_coded(res, streams, coded, "encode, path 0")
    gh.round_trip_commands(torch, codec, streams, res, lay, "path 0")
    codec.close()


@pytest.mark.parametrize("fam", wc.FAMILIES, ids=repr)
def test_directed_batch_with_history(fam, sources):
    import torch
    import divans_amd as da
    g, o, streams, coded, lay, hlay = _case(fam, sources, True)
    t, ht = gh.to_device(torch, lay), gh.to_device(torch, hlay)
    codec = gh.codec_for(da, fam, g, lay["lit_longest"], even=True)
    for blocks in (2, 1):
        codec.set_geometry(blocks=blocks)
        st, raw, flags, name = gh.decode_commands(torch, codec, lay, t, hlay, ht)
        assert st == 0 and name == _kernel(fam, True), (blocks, st, name)
        gh.assert_raw(raw, lay, streams, f"{blocks} workgroups")
        assert not flags.any(), blocks
    elay = gh.encode_layout(lay)
    res = gh.encode_commands(torch, codec, elay, gh.to_device(torch, elay), hlay, ht)
    assert res["status"] == 0 and not res["flags"].any() and codec.last_encode_path() == 1, (res["status"], res["flags"].tolist(), codec.last_encode_path())
    gh.assert_coded(res, streams, coded, "encode, path 0")
    gh.round_trip_commands(torch, codec, streams, res, elay, "path 0", hlay, ht)
    codec.close()
