"""divans_gpu_codec_set_block_types above eight types on the segment entry points: every family of tests/wide_block_type_cases.py codes
the batch of tests/segment_cases.py (40 streams, the boundaries where the kernels change phase, block types drawn from all 9 or 256)
bit for bit against the C oracle, which takes any block type (tests/test_wide_block_type_cases_cpu.py guards it on these families and
shows that folding the high types onto the first eight changes its bytes).  The decoders are given the ORACLE's bytes; the kernel
that ran is asserted from its name: where the context map is not constant it is an instance of the wide context-table layout, spelt
with one trailing template argument, under a constant context one of the instances the codec has at eight types."""
import numpy as np
import pytest

import gpu_harness as gh
import pyoracle as po
import segment_cases as sc
import wide_block_type_cases as wc

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
        _CASES[fam.name] = (g, o, streams, gh.oracle_bytes(o, streams))
    return _CASES[fam.name]


def _assert_kernel(fam, what, gen, name):
    if fam.ctxc:        # no kernel reads a context table: the instances of eight types
        assert not name.endswith(", 1>") or name.count(",") == 4, (what, name)
        return gh.assert_segment_kernel(fam, what, gen, name)
    mm = fam.mm if fam.mm >= 0 else -1
    if gen == 2:        # lit_decode2_kernel_any<MM, false, MIX, true, caches, 1>: the high-row caches in the 2-way organisation, or none
        caches = (19 if fam.mix else 17) if fam.cached else 0
        assert name == f"divans_hip::lit_decode2_kernel_any<{mm}, false, {gh.tf(fam.mix)}, true, {caches}, 1>", (what, name)
    else:               # lit_decode_kernel<MM, false, MIX, 0, true, 1>: generation 1 reads the wide layout without a cache
        assert name == f"divans_hip::lit_decode_kernel<{mm}, false, {gh.tf(fam.mix)}, 0, true, 1>", (what, name)


@pytest.mark.parametrize("fam", wc.FAMILIES, ids=repr)
def test_encode_bit_exact_vs_oracle(fam, sources):
    """default high-row cache, no cache, one workgroup (16 resident groups: every group codes two or three streams in a row)"""
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    tin = gh.input_tensors(torch, streams)
    codec = gh.codec_for(da, fam, g, tin["longest"])
    for what, geometry in (("default", None), ("no cache", dict(cache_rows=0)), ("no cache, 1 workgroup", dict(blocks=1))):
        if geometry:
            codec.set_geometry(**geometry)
        st, got, _ = gh.encode_segments(codec, tin, fit=True)
        assert st == 0 and codec.last_encode_path() == 1, (what, st, codec.last_encode_path())      # path 0 codes a list with the streaming kernels
        gh.assert_same(got, coded, streams, what)
    codec.close()


@pytest.mark.parametrize("fam", wc.CONST, ids=repr)
def test_constant_context_under_the_bucketed_path(fam, sources):
    """a constant context keeps at 256 types what it has at eight: the plain family its bucketed pass (same bytes), the mixing family
    none -- at eight types as at 256 (set_encode_path(2) is refused with the reason it gives there)"""
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    tin = gh.input_tensors(torch, streams)
    codec = gh.codec_for(da, fam, g, tin["longest"])
    eight = da.LiteralCodec(g, max(tin["longest"], 16)); eight.set_block_types(8)
    if fam.mix:
        for c in (eight, codec):
            with pytest.raises(da.DivansGpuError, match="the bucketed encoder needs"):
                c.set_encode_path(2)
    else:
        eight.set_encode_path(2)
        codec.set_encode_path(2)
        st, got, _ = gh.encode_segments(codec, tin, fit=True)
        assert st == 0 and codec.last_encode_path() == 2, (st, codec.last_encode_path())
        gh.assert_same(got, coded, streams, "path 2")
    eight.close(); codec.close()


@pytest.mark.parametrize("fam", wc.FAMILIES, ids=repr)
def test_decode_oracle_bytes_on_every_generation(fam, sources):
    """generations 2 and 3 (a direct-mapped request on a wide list comes down to the 2-way instances): default, tiny caches with two
    workgroups and with one"""
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
            _assert_kernel(fam, what, gen, name)
            gh.assert_decoded(back, tin, streams, what)
        codec.close()


def _with_bad_type(streams, at, btype):
    """the batch with one segment of stream `at` naming `btype` (the longest segment: bytes are coded under it)"""
    out = [(name, lit, segs.copy()) for name, lit, segs in streams]
    segs = out[at][2]
    segs["btype"][int(np.argmax(segs["len"]))] = btype
    return out


@pytest.mark.parametrize("fam", wc.FAMILIES, ids=repr)
def test_a_block_type_without_a_table_is_reported(fam, sources):
    """a list that names n_btypes (at 256 types: 256, and 0xffffffff) among good neighbours: BAD_SEGMENT in both directions -- the kernels
    stay inside the tables -- and every other stream as the oracle has it"""
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    few, fcoded, at = streams[:12], coded[:12], 6
    assert few[at][1].size > 16
    tcoded = gh.coded_tensors(torch, fcoded)
    enc = gh.codec_for(da, fam, g, max(s[1].size for s in few)); enc.set_geometry(blocks=1)
    dec = gh.codec_for(da, fam, g, max(s[1].size for s in few)); dec.set_geometry(blocks=1)
    for btype in ((fam.n_btypes,) if fam.n_btypes < 256 else (256, 0xffffffff)):
        batch = _with_bad_type(few, at, btype)
        tin = gh.input_tensors(torch, batch)
        st, got, _ = gh.encode_segments(enc, tin, fit=True)
        assert st & gh.BAD_SEGMENT, (btype, "encode", st)
        gh.assert_same(got, fcoded, batch, f"type {btype}", skip=(at,))
        st, back, name = gh.decode_segments(torch, dec, tin, tcoded)
        assert st & gh.BAD_SEGMENT, (btype, "decode", st, name)
        _assert_kernel(fam, f"type {btype}", 2, name)
        gh.assert_decoded(back[:tin["total"]], tin, batch, f"type {btype}", skip=(at,))
    tin = gh.input_tensors(torch, few)        # ... and the same streams with their lists in order are clean
    st, got, _ = gh.encode_segments(enc, tin, fit=True)
    assert st == 0
    gh.assert_same(got, fcoded, few, "good lists")
    st, back, name = gh.decode_segments(torch, dec, tin, tcoded)
    assert st == 0, (st, name)
    gh.assert_decoded(back, tin, few, "good lists")
    enc.close(); dec.close()


@pytest.mark.parametrize("fam", wc.FAMILIES, ids=repr)
def test_lists_that_do_not_add_up_are_reported(fam, sources):
    """7 bytes too few, 7 too many, bytes and no list (segment_cases.bad_lists): BAD_SEGMENT in both directions, the other streams as the oracle's"""
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    bad, which = sc.bad_lists(streams)
    tin = gh.input_tensors(torch, bad)
    tcoded = gh.coded_tensors(torch, coded[:len(bad)])
    codec = gh.codec_for(da, fam, g, tin["longest"])
    codec.set_geometry(blocks=2)
    st, got, _ = gh.encode_segments(codec, tin, fit=True)
    assert st & gh.BAD_SEGMENT, ("encode", st)
    gh.assert_same(got, coded, bad, "bad lists", skip=which)
    st, back, name = gh.decode_segments(torch, codec, tin, tcoded)
    codec.close()
    assert st & gh.BAD_SEGMENT, ("decode", st, name)
    _assert_kernel(fam, "bad lists", 2, name)
    offs = tin["off"].cpu().numpy()
    for i, (nm, lit, segs) in enumerate(bad):
        if i not in which:
            assert (back[int(offs[i]):int(offs[i]) + lit.size] == lit).all(), (i, nm)


def test_lists_of_low_types_code_alike_under_both_layouts(sources):
    """the cross-check against the kernels that exist: the streams of the 9-type batch whose lists name types below 8 give the same coded
    bytes and the same decoded bytes under set_block_types(9) (the wide layout) as under set_block_types(8) (the fused one)"""
    import torch
    import divans_amd as da
    fam = wc.by_name("mm4_map_plain_bt9")
    g, o, streams, coded = _case(fam, sources)
    low = wc.low_types_only(streams)
    assert len(low) >= 8 and sum(s[1].size for s in low) > 2000, [s[0] for s in low]
    ref = [coded[i] for i, s in enumerate(streams) if any(s is t for t in low)]
    tin = gh.input_tensors(torch, low)
    tcoded = gh.coded_tensors(torch, ref)
    results = {}
    for n in (9, 8):
        codec = da.LiteralCodec(g, max(tin["longest"], 16))
        codec.set_block_types(n)
        st, got, _ = gh.encode_segments(codec, tin, fit=True)
        assert st == 0, (n, st)
        st, back, name = gh.decode_segments(torch, codec, tin, tcoded)
        codec.close()
        assert st == 0 and name.count(",") == (5 if n == 9 else 4), (n, st, name)      # a wide instance has a sixth template argument
        results[n] = (got, back)
    gh.assert_same(results[9][0], results[8][0], low, "9 types against 8")
    gh.assert_same(results[9][0], ref, low, "9 types against the oracle")
    assert (results[9][1] == results[8][1]).all()
    gh.assert_decoded(results[9][1], tin, low, "9 types")


def test_a_wrap_checked_speed_runs_the_wide_generation_1_instance(sources):
    """a speed whose row totals leave i16 (WRAP_CASES of the segment tests) with 256 types on short_streams: generation 1 without a
    cache, whatever was asked for -- the wide lit_decode_kernel instance"""
    import torch
    import divans_amd as da
    name, speed = sc.WRAP_CASES[0]
    assert name == "mm4_map_plain"
    fam = wc.by_name("mm4_map_plain_bt256")
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
    assert len(streams) >= 12 and max(int(s[2]["btype"].max()) for s in streams) >= 128, len(streams)
    tin = gh.input_tensors(torch, streams)
    tcoded = gh.coded_tensors(torch, coded)
    codec = gh.codec_for(da, fam, g, tin["longest"])
    st, got, _ = gh.encode_segments(codec, tin, fit=True)
    assert st == 0, st
    gh.assert_same(got, coded, streams, "wrap-checked")
    st, back, kname = gh.decode_segments(torch, codec, tin, tcoded)
    codec.close()
    assert st == 0, (st, kname)
    assert kname == "divans_hip::lit_decode_kernel<4, false, false, 0, true, 1>", kname
    gh.assert_decoded(back, tin, streams, "wrap-checked")


LATE_WRAP = [f for f in wc.WIDE if f.n_btypes == 256 and f.cached and f.prediction_mode is None]


@pytest.mark.parametrize("fam", LATE_WRAP, ids=repr)
def test_every_wide_generation_1_instance_under_a_wrap_checked_speed(fam, sources):
    """all six (mixing value, mixing) pairs under wide_block_type_cases.LATE_WRAP_SPEED: the launch is wrap-checked, and no stream of the
    batch is long enough for a row to wrap -- so with mixing too every stream must come out as the oracle's, with a clean status"""
    import torch
    import divans_amd as da
    g, o = fam.pair(da, po)
    assert not da.speed_supported(*wc.LATE_WRAP_SPEED) and da.speed_accepted(*wc.LATE_WRAP_SPEED)
    for cfg in (g, o):
        for i in range(4):
            cfg.literal_adaptation[i].inc, cfg.literal_adaptation[i].lim = wc.LATE_WRAP_SPEED
    streams = sc.short_streams(fam, sources, 40)
    coded = gh.oracle_bytes(o, streams)
    for (_, lit, segs), c in zip(streams, coded):
        assert (po.lit_segments_decode(o, c, lit.size, segs["len"], segs["btype"], segs["last8"]) == lit).all()
    tin = gh.input_tensors(torch, streams)
    tcoded = gh.coded_tensors(torch, coded)
    codec = gh.codec_for(da, fam, g, tin["longest"])
    st, got, _ = gh.encode_segments(codec, tin, fit=True)
    assert st == 0, st
    gh.assert_same(got, coded, streams, "late wrap")
    st, back, kname = gh.decode_segments(torch, codec, tin, tcoded)
    codec.close()
    assert st == 0, (st, kname)
    _assert_kernel(fam, "late wrap", 1, kname)
    gh.assert_decoded(back, tin, streams, "late wrap")


def test_what_a_wide_codec_refuses(sources):
    import torch
    import divans_amd as da
    fam = wc.by_name("mm4_map_mix_bt256")
    g, o, streams, coded = _case(fam, sources)
    codec = da.LiteralCodec(g, 4096)
    for n in (0, 257):
        with pytest.raises(da.DivansGpuError, match="1..256 consecutive literal block types"):
            codec.set_block_types(n)
    codec.set_block_types(9)
    assert codec.high_row_slots() == 0
    with pytest.raises(da.DivansGpuError, match="no bucketed encoder pass exists for more than 8 literal block types"):
        codec.set_encode_path(2)
    blocks = np.zeros((4, 4096), np.uint8)
    with pytest.raises(da.DivansGpuError, match="a batch call without segment lists is not available on a codec with more than 8 literal block types"):
        codec.encode_host(blocks, 4096)
    dev = torch.device("cuda")
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    with pytest.raises(da.DivansGpuError, match="a batch call without segment lists is not available"):
        codec.decode_batch(z(64, torch.uint8), z(4, torch.int64), z(4, torch.int32), 4, 4096, z(4 * 4096, torch.uint8))
    with pytest.raises(da.DivansGpuError, match="divans_gpu_lit_model_batch is not available"):
        codec.model_batch(z(4 * 4096, torch.uint8), 4, 4096)
    with pytest.raises(da.DivansGpuError, match="divans_gpu_codec_row_replay is not available"):
        codec.row_replay(z(4 * 4096, torch.uint8), 4, 4096)
    with pytest.raises(da.DivansGpuError, match="coding a stream call by call is not available"):
        codec.stream_encode_pieces([blocks[0]])
    with pytest.raises(da.DivansGpuError, match="coding a stream call by call is not available"):
        codec.stream_decode_chunks(np.zeros(64, np.uint8), 16)
    codec.set_block_types(8)        # the fused layout again: the calls without lists are back
    packed, offs, sizes = codec.encode_host(blocks, 4096)
    assert (codec.decode_host(packed, offs, sizes, 4096) == blocks).all()
    codec.close()
