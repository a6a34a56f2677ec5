"""The bucketed two-model encoder pass under several literal block types (launch_bucket_mix_bt_model, lit_bucket_ctx.hip) behind
divans_gpu_codec_set_encode_path(c, 2): a context map in use, every mixing value 4, dynamic mixing, and no previous byte that
reaches more than eight contexts (divans_gpu_codec_high_row_slots).  mix_bt_sort_kernel keys the stride model's positions by prev
and puts the block type of the covering segment into the payload's high-row slot; the context model's sort is ctx_sort_kernel.
Every comparison is against the C oracle's bytes (tests/test_mix_bt_bucketed_cases_cpu.py guards the oracle and the shapes); the
pass that ran is asserted through divans_gpu_codec_last_encode_path."""
import ctypes

import numpy as np
import pytest

import bucketed_segment_cases as bc
import gpu_harness as gh
import ctx_bucketed_cases as cc
import irtext
import mix_bt_bucketed_cases as mc
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
KEYS = list(mc.FAMILIES)
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(key, sources):
    """the configuration pair, its batch and the oracle's bytes of every stream: computed once, shared, never written to"""
    if key not in _CASES:
        import divans_amd as da
        fam = mc.FAMILIES[key]
        g, o = fam.pair(da, po)
        streams = mc.batch(fam, sources)
        _CASES[key] = (fam, g, o, streams, gh.oracle_bytes(o, streams))
    return _CASES[key]


@pytest.mark.parametrize("key", KEYS)
def test_path_2_codes_several_block_types_bit_exact(key, sources):
    import torch
    import divans_amd as da
    fam, g, o, streams, coded = _case(key, sources)
    tin = gh.ragged_tensors(torch, streams)
    assert tin["longest"] == 65536 and tin["n"] == 48
    codec = gh.codec_for(da, fam, g, tin["longest"])
    assert codec.high_row_slots() == 8
    codec.set_encode_path(2)
    outs = codec.alloc_encode_outputs(tin["n"])
    for what, sub in (("one launch sequence", None), ("launch sequences of 24 streams", 24)):
        if sub:
            codec.set_bucket_batch(sub)
        st, got, path = gh.encode_segments(codec, tin, outs)
        assert st == 0 and path == mc.BUCKETED_PATH == 3, (what, st, path)
        gh.assert_same(got, coded, streams, what)
    gh.assert_round_trip_segments(torch, codec, tin, outs, streams, key)
    codec.set_encode_path(1)
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, coded, streams, "streaming kernels")
    codec.set_encode_path(0)          # automatic: a list stays on the streaming kernels, as for every bucketed family
    few = streams[:12]
    st, got, path = gh.encode_segments(codec, gh.ragged_tensors(torch, few))
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, coded, few, "automatic, with a list")
    codec.close()


@pytest.mark.parametrize("name", list(mc.REFUSED))
def test_more_than_eight_high_rows_stay_on_the_streaming_kernels(name, sources):
    import torch
    import divans_amd as da
    fam, count = mc.REFUSED[name]
    g, o = fam.pair(da, po)
    streams = [s for s in sc.shapes(fam, sources) if s[1].size <= 5000][:16] + [mc.all_slots(fam)]
    coded = gh.oracle_bytes(o, streams)
    tin = gh.ragged_tensors(torch, streams)
    codec = gh.codec_for(da, fam, g, tin["longest"])
    assert codec.high_row_slots() == count
    with pytest.raises(da.DivansGpuError, match="bucketed encoder needs"):
        codec.set_encode_path(2)
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, coded, streams, "automatic")
    codec.close()


def test_high_row_slots_of_a_codec_with_one_block_type():
    """as it is created a codec keeps the table of its own block type: the count is that table's, and set_block_types brings the other"""
    import divans_amd as da
    fam = mc.FAMILIES["c8"]
    g, o = fam.pair(da, po)
    codec = da.LiteralCodec(g, 4096)
    cfg1 = po.LitConfig.from_buffer_copy(bytes(o))
    cmap = np.frombuffer(bytes(o.literal_context_map), np.uint8).copy()
    cmap[:64] = cmap[64 * fam.btype:64 * fam.btype + 64]                # high_row_slots(cfg, 1) reads block type 0
    ctypes.memmove(cfg1.literal_context_map, cmap.ctypes.data, cmap.size)
    assert codec.high_row_slots() == mc.high_row_slots(cfg1, 1) <= 4
    codec.set_block_types(8)
    assert codec.high_row_slots() == 8
    codec.set_block_types(1)
    assert codec.high_row_slots() == mc.high_row_slots(o, 1) <= 4
    codec.close()


@pytest.mark.parametrize("n", [1, 2, 63, 8192, 8193, 65536])
def test_path_2_without_a_list(n, sources):
    """encode_batch on a codec that keeps eight tables: ragged offsets on both load alignments.  A call without a list codes under
    table 0 -- block type 0 once set_block_types has rebuilt the tables, whatever divans_lit_config::btype (3 here) says -- on every
    path, so the oracle codes the streams with its block type set to 0."""
    import torch
    import divans_amd as da
    fam = mc.FAMILIES["c8"]
    g, o = fam.pair(da, po)
    assert g.btype == 3
    o0 = po.LitConfig.from_buffer_copy(bytes(o)); o0.btype = 0
    blocks = cc.plain_streams(n, sources)
    buf, offs, sizes = cc.ragged_layout(blocks)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    codec = da.LiteralCodec(g, max(n, 16))
    codec.set_block_types(8)
    codec.set_encode_path(2)
    outs = codec.alloc_encode_outputs(len(blocks))
    d_buf, d_offs, d_sizes = t(buf), t(offs), t(sizes)
    codec.encode_batch(d_buf, len(blocks), n, outs, in_offsets=d_offs, in_sizes=d_sizes)
    assert codec.status() == 0 and codec.last_encode_path() == mc.BUCKETED_PATH
    got = gh.split_outputs(outs, len(blocks))
    for i, (a, lit) in enumerate(zip(got, blocks)):
        b = po.lit_encode(o0, lit)
        assert a.size == b.size and (a == b).all(), (n, i)
    for path, ran in ((0, mc.AUTOMATIC_PATH_WITHOUT_A_LIST), (1, 1)):
        codec.set_encode_path(path)
        codec.encode_batch(d_buf, len(blocks), n, outs, in_offsets=d_offs, in_sizes=d_sizes)
        assert codec.status() == 0 and codec.last_encode_path() == ran
        for i, (a, b) in enumerate(zip(gh.split_outputs(outs, len(blocks)), got)):
            assert a.size == b.size and (a == b).all(), (path, n, i)
    codec.close()


@pytest.mark.parametrize("key", ["c8", "u2"])
def test_faulty_lists_are_reported_under_several_block_types(key, sources):
    """a list 7 bytes short, one 7 too long, bytes without a list, a block type outside the tables (in the first piece and in the
    third), an empty stream whose list holds bytes: BAD_SEGMENT each time, the call returns, the other streams are the oracle's, and
    the same codec is clean again afterwards"""
    import torch
    import divans_amd as da
    fam, g, o, streams, coded = _case(key, sources)
    good = streams[:12]
    bad, which = sc.bad_lists(streams)
    batches = [("all three", bad, which)] + [(f"stream {i} alone", [bad[k] if k == i else good[k] for k in range(12)], (i,)) for i in which]
    batches.append(("block type outside the tables", bc.bad_btype(good, 7, fam.n_btypes), (7,)))
    assert good[3][0] == "X_span"
    batches.append(("block type outside the tables, on the segment that covers pieces 3 to 5", bc.bad_btype(good, 3, 200, 3), (3,)))
    assert good[6][0] == "X_edges" and int(good[6][2]["len"][:13].sum()) == 16384
    batches.append(("block type outside the tables, in the stream's third piece", bc.bad_btype(good, 6, fam.n_btypes, 13), (6,)))
    batches.append(("empty stream, list of 5 bytes", bc.empty_stream_with_bytes_in_its_list(good, 4), (4,)))
    tins = [gh.ragged_tensors(torch, batch) for _, batch, _ in batches]
    codec = gh.codec_for(da, fam, g, max(t["longest"] for t in tins))
    codec.set_encode_path(2)
    for (what, batch, skip), tin in zip(batches, tins):
        st, got, path = gh.encode_segments(codec, tin)
        assert st & gh.BAD_SEGMENT and path == mc.BUCKETED_PATH, (what, st, path)
        gh.assert_same(got, coded, batch, what, skip=skip)
    st, got, path = gh.encode_segments(codec, gh.ragged_tensors(torch, good))
    assert st == 0 and path == mc.BUCKETED_PATH, (st, path)
    gh.assert_same(got, coded, good, "the same streams with their lists in order")
    codec.close()


def test_a_real_command_list_under_its_own_four_block_types():
    """random_then_unicode.ir: its own context map (4 block types, at most 6 contexts per previous byte), the mask forced to mixing
    value 4 and dynamic mixing on -- the reference's TestContextMixing arithmetic on a general stream"""
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text("random_then_unicode"))
    streams = gh.ir_streams(ir, 32)
    assert len(streams) >= 8 and all(0 < s[1].size <= 65536 for s in streams) and any(s[2].size > 1 for s in streams)
    assert ir.num_block_types == 4 and len({int(b) for s in streams for b in s[2]["btype"]}) > 1
    cfg = ir.lit_config(dynamic_context_mixing=2, use_context_map=1)
    ctypes.memset(cfg.mixing_mask, 4, 8192)
    assert cfg.context_mixing == 2
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    assert 1 < mc.high_row_slots(ocfg, 4) <= 8
    coded = gh.oracle_bytes(ocfg, streams)
    tin = gh.ragged_tensors(torch, streams)
    codec = da.LiteralCodec(cfg, max(tin["longest"], 16))
    codec.set_block_types(ir.num_block_types)
    assert codec.high_row_slots() == mc.high_row_slots(ocfg, 4)
    codec.set_encode_path(2)
    outs = codec.alloc_encode_outputs(tin["n"])
    st, got, path = gh.encode_segments(codec, tin, outs)
    assert st == 0 and path == mc.BUCKETED_PATH, (st, path)
    gh.assert_same(got, coded, streams, "random_then_unicode")
    gh.assert_round_trip_segments(torch, codec, tin, outs, streams, "random_then_unicode")
    codec.close()
    ir.close()
