"""The segment entry points on every SEG = true kernel instance: each (MM, CTXC, MIX) family of tests/segment_cases.py codes one
batch of 40 streams whose segment boundaries sit where the kernels change phase (the streaming encoder's 16-byte lane window and
32-byte read-ahead, the decoders' 16-byte output group, the 32 768-byte rANS chunk seam), with empty segments, one-byte segments,
random last_8_literals and block types 0..7, an empty stream in the middle -- bit for bit against the C oracle
(tests/test_segment_cases_cpu.py guards the oracle on the same lists).  The decoders are given the ORACLE's bytes, so an encoder
fault cannot hide a decoder fault; the kernel instance that ran is asserted from its name.  Grids of one and two workgroups make
every resident group code several segmented streams in a row (the per-stream reset of the cursor, the context table, the history
and the Weights), tiny row caches force misses and write-backs."""
import pytest

import gpu_harness as gh
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(fam, sources):
    """the family's configurations, its batch and the oracle's bytes of every stream: computed once, shared, never written to"""
    if fam.name not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        streams = sc.shapes(fam, sources)
        coded = gh.oracle_bytes(o, streams)
        s5 = next(i for i, s in enumerate(streams) if s[0] == "S5")
        plain = po.lit_encode(o, streams[s5][1])
        assert coded[s5].size == plain.size and (coded[s5] == plain).all()      # one segment, zero history, own block type = the plain stream
        _CASES[fam.name] = (g, o, streams, coded)
    return _CASES[fam.name]


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_encode_bit_exact_vs_oracle(fam, sources):
    """default high-row cache, no cache, and grids of two and of one workgroup (16 resident groups: every group codes two or three
    streams in a row, the empty one between two others)"""
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    tin = gh.input_tensors(torch, streams)
    # two codecs, the settings of a chain applied one after the other (a codec's tables are then also reused from launch to launch)
    chains = ((("default", None), ("2 workgroups", dict(blocks=2)), ("1 workgroup", dict(blocks=1))),
              (("no cache", dict(cache_rows=0)), ("no cache, 1 workgroup", dict(blocks=1))))
    for chain in chains:
        codec = gh.codec_for(da, fam, g, tin["longest"])
        for what, geometry in chain:
            if geometry:
                codec.set_geometry(**geometry)
            st, got, _ = gh.encode_segments(codec, tin, fit=True)
            assert st == 0, (what, st)
            gh.assert_same(got, coded, streams, what)
        codec.close()


@pytest.mark.parametrize("fam", [f for f in sc.FAMILIES if f.cached], ids=repr)
def test_unified_and_split_caches_refuse_segment_lists(fam, sources):
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    few = streams[:4]
    tin = gh.input_tensors(torch, few)
    tcoded = gh.coded_tensors(torch, coded[:4])
    for what, setup in (("unified", lambda c: c.set_geometry(cache_rows=32)), ("split", lambda c: c.set_split_cache(32, 64))):
        codec = gh.codec_for(da, fam, g, tin["longest"])
        setup(codec)
        with pytest.raises(da.DivansGpuError, match="segment lists need"):
            gh.encode_segments(codec, tin, fit=True)
        if 1 in da.decoder_generations():        # these are the first generation's caches: a build that offers it decodes with it from here on
            with pytest.raises(da.DivansGpuError, match="segment lists need"):
                gh.decode_segments(torch, codec, tin, tcoded)
        else:                                    # the second generation has its own caches and serves the list
            st, back, name = gh.decode_segments(torch, codec, tin, tcoded)
            assert st == 0 and "lit_decode2_kernel" in name, (what, st, name)
            gh.assert_decoded(back, tin, few, what)
        codec.close()


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_decode_oracle_bytes_on_every_generation(fam, sources):
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    tin = gh.input_tensors(torch, streams)
    tcoded = gh.coded_tensors(torch, coded)
    for chain in gh.decoder_chains(da, fam):
        codec = gh.codec_for(da, fam, g, tin["longest"])
        for what, setup, gen in chain:
            setup(codec)
            st, back, name = gh.decode_segments(torch, codec, tin, tcoded)
            assert st == 0, (what, st, name)
            gh.assert_segment_kernel(fam, what, gen, name)
            gh.assert_decoded(back, tin, streams, what)
        codec.close()


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_lists_that_do_not_add_up_are_reported(fam, sources):
    """a list that covers 7 bytes too few, one that covers 7 too many, a stream with bytes and no list: BAD_SEGMENT in both directions
    and on every generation, each kind by itself and all three in one batch, whose other streams still come out as the oracle's"""
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    bad, which = sc.bad_lists(streams)
    good = streams[:len(bad)]
    batches = [("all three", bad, which)] + [(f"stream {i} alone", [bad[k] if k == i else good[k] for k in range(len(bad))], (i,)) for i in which]
    tcoded = gh.coded_tensors(torch, coded[:len(bad)])      # (the bad streams: what the oracle wrote under the list that does add up)
    tins = [gh.input_tensors(torch, batch) for _, batch, _ in batches]
    longest = max(t["longest"] for t in tins)
    codec = gh.codec_for(da, fam, g, longest)
    codec.set_geometry(blocks=2)      # 12 streams: two workgroups hold them all (and the codec then asks for tables of 32 streams, not of a full grid)
    for (what, batch, skip), tin in zip(batches, tins):
        st, got, _ = gh.encode_segments(codec, tin, fit=True)
        assert st & gh.BAD_SEGMENT, (what, "encode", st)
        gh.assert_same(got, coded, batch, what, skip=skip)
    st, got, _ = gh.encode_segments(codec, gh.input_tensors(torch, good), fit=True)      # ... and the same streams with their lists in order are clean
    assert st == 0
    codec.close()
    for chain in gh.decoder_chains(da, fam):
        codec = gh.codec_for(da, fam, g, longest)
        codec.set_geometry(blocks=2)
        for k, (label, setup, gen) in enumerate(chain):
            setup(codec)
            for (what, batch, skip), tin in zip(batches, tins):
                if k and len(skip) == 1:      # each kind by itself: once per generation, the batch of all three on every launch shape
                    continue
                st, back, name = gh.decode_segments(torch, codec, tin, tcoded)
                assert st & gh.BAD_SEGMENT, (what, label, st, name)
                gh.assert_segment_kernel(fam, label, gen, name)
                offs = tin["off"].cpu().numpy()
                for i, (nm, lit, segs) in enumerate(batch):
                    if i not in skip:
                        assert (back[int(offs[i]):int(offs[i]) + lit.size] == lit).all(), (what, label, i, nm)
            if k == 0:      # ... and the same streams with their lists in order are clean
                st, back, name = gh.decode_segments(torch, codec, gh.input_tensors(torch, good), tcoded)
                assert st == 0, (label, st, name)
        codec.close()


@pytest.mark.parametrize("name,speed", sc.WRAP_CASES, ids=[w[0] for w in sc.WRAP_CASES])
def test_segments_under_speeds_whose_row_totals_wrap(name, speed, sources):
    """the wrap-checked launch: generation 1 without a cache, whatever was asked for.  The streams are those the oracle codes and reads
    back (no wrapped row coded with again; without mixing that is exactly when the kernels report none, see
    test_speeds_under_which_the_references_row_totals_wrap)"""
    import torch
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == name)
    g, o = fam.pair(da, po)
    assert not da.speed_supported(*speed) and da.speed_accepted(*speed)
    for cfg in (g, o):
        for i in range(4):
            cfg.literal_adaptation[i].inc, cfg.literal_adaptation[i].lim = speed
    streams, coded = [], []
    for cand in sc.short_streams(fam, sources, 80):
        _, lit, segs = cand
        try:
            c = po.lit_segments_encode(o, lit, segs["len"], segs["btype"], segs["last8"])
            if (po.lit_segments_decode(o, c, lit.size, segs["len"], segs["btype"], segs["last8"]) == lit).all():
                streams.append(cand); coded.append(c)
        except RuntimeError:
            pass
    assert len(streams) >= 12 and sum(s[2].size >= 3 for s in streams) >= 6, len(streams)
    tin = gh.input_tensors(torch, streams)
    tcoded = gh.coded_tensors(torch, coded)
    mm = fam.mm if fam.mm >= 0 else -1
    for what, setup in (("default", lambda c: None), ("1 workgroup", lambda c: c.set_geometry(blocks=1))):
        codec = gh.codec_for(da, fam, g, tin["longest"])
        setup(codec)
        st, got, _ = gh.encode_segments(codec, tin, fit=True)
        assert st == 0, (what, st)
        gh.assert_same(got, coded, streams, what)
        st, back, kname = gh.decode_segments(torch, codec, tin, tcoded)
        codec.close()
        assert st == 0, (what, st, kname)
        assert f"lit_decode_kernel<{mm}, {gh.tf(fam.ctxc)}, {gh.tf(fam.mix)}, 0, true>" in kname, kname
        gh.assert_decoded(back, tin, streams, what)
