"""The bucketed encoder model passes under segment lists (divans_gpu_codec_set_encode_path(c, 2) with
divans_gpu_lit_encode_segments_batch): bucket_sort_kernel<true> and mix_sort_kernel<MODEL, true> take the keys of a segment's first
bytes from its last8.  Every configuration of tests/bucketed_segment_cases.py codes one batch of 44 streams -- the shapes of
tests/segment_cases.py plus segment starts on the sort kernels' wave, piece and slot edges, a list of 8200 one-byte segments, empty
segments on a piece base -- bit for bit against the C oracle (tests/test_bucketed_segment_cases_cpu.py guards the oracle and the
shapes), in one launch sequence and in two; the pass that ran is asserted through divans_gpu_codec_last_encode_path."""
import ctypes

import numpy as np
import pytest

import bucketed_segment_cases as bc
import gpu_harness as gh
import irtext
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
KEYS = list(bc.CONFIGS)
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(key, sources):
    """the configuration pair, its batch and the oracle's bytes of every stream: computed once, shared, never written to"""
    if key not in _CASES:
        import divans_amd as da
        fam = bc.CONFIGS[key]
        g, o = fam.pair(da, po)
        streams = bc.batch(fam, sources)
        _CASES[key] = (fam, g, o, streams, gh.oracle_bytes(o, streams))
    return _CASES[key]


@pytest.mark.parametrize("key", KEYS)
def test_bucketed_pass_codes_segment_lists_bit_exact(key, sources):
    import torch
    import divans_amd as da
    fam, g, o, streams, coded = _case(key, sources)
    tin = gh.ragged_tensors(torch, streams)
    assert tin["longest"] == 65536
    codec = gh.codec_for(da, fam, g, tin["longest"])
    assert codec.last_encode_path() == 0
    codec.set_encode_path(2)
    for what, sub in (("one launch sequence", None), ("launch sequences of 24 streams", 24)):
        if sub:
            codec.set_bucket_batch(sub)
        st, got, path = gh.encode_segments(codec, tin)
        assert st == 0 and path == bc.BUCKETED_PATH[key], (what, st, path)
        gh.assert_same(got, coded, streams, what)
    codec.set_encode_path(1)
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, coded, streams, "streaming kernels")
    codec.close()


@pytest.mark.parametrize("key", KEYS)
def test_the_default_path_did_not_move(key, sources):
    """automatic: a segment list still goes through the streaming kernels, the plain entry point through the bucketed pass"""
    import torch
    import divans_amd as da
    fam, g, o, streams, coded = _case(key, sources)
    few = streams[:16]
    tin = gh.ragged_tensors(torch, few)
    codec = gh.codec_for(da, fam, g, tin["longest"])
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, coded, few, "automatic, with a list")
    outs = codec.alloc_encode_outputs(tin["n"])
    codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
    assert codec.status() == 0 and codec.last_encode_path() == bc.BUCKETED_PATH[key]
    plain = [po.lit_encode(o, lit) if lit.size else np.zeros(0, np.uint8) for _, lit, _ in few]
    gh.assert_same(gh.split_outputs(outs, tin["n"]), plain, few, "plain entry point")
    codec.set_encode_path(2)      # ... and it stays so once the bucketed pass also serves the lists
    codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
    assert codec.status() == 0 and codec.last_encode_path() == bc.BUCKETED_PATH[key]
    gh.assert_same(gh.split_outputs(outs, tin["n"]), plain, few, "plain entry point under path 2")
    codec.close()


@pytest.mark.parametrize("key", KEYS)
def test_faulty_lists_are_reported_by_the_bucketed_pass(key, sources):
    """lists that cover too few / too many bytes, bytes without a list, a block type outside the tables, an empty stream whose list
    holds bytes: BAD_SEGMENT each time, the other streams as the oracle's, and the same codec clean again afterwards"""
    import torch
    import divans_amd as da
    fam, g, o, streams, coded = _case(key, sources)
    good = streams[:12]
    bad, which = sc.bad_lists(streams)
    batches = [("all three", bad, which)] + [(f"stream {i} alone", [bad[k] if k == i else good[k] for k in range(12)], (i,)) for i in which]
    outside = fam.n_btypes if fam.n_btypes > 1 else fam.btype + 1
    batches.append(("block type outside the tables", bc.bad_btype(good, 7, outside), (7,)))
    assert good[5][0] == "X_edges" and int(good[5][2]["len"][:13].sum()) == 16384
    batches.append(("block type outside the tables, in the stream's third piece", bc.bad_btype(good, 5, outside, 13), (5,)))
    batches.append(("empty stream, list of 5 bytes", bc.empty_stream_with_bytes_in_its_list(good, 4), (4,)))
    tins = [gh.ragged_tensors(torch, batch) for _, batch, _ in batches]
    codec = gh.codec_for(da, fam, g, max(t["longest"] for t in tins))
    codec.set_encode_path(2)
    for (what, batch, skip), tin in zip(batches, tins):
        st, got, path = gh.encode_segments(codec, tin)
        assert st & gh.BAD_SEGMENT and path == bc.BUCKETED_PATH[key], (what, st, path)
        gh.assert_same(got, coded, batch, what, skip=skip)
    st, got, path = gh.encode_segments(codec, gh.ragged_tensors(torch, good))
    assert st == 0 and path == bc.BUCKETED_PATH[key], (st, path)
    gh.assert_same(got, coded, good, "the same streams with their lists in order")
    codec.close()


@pytest.mark.parametrize("name", ["alice29", "alice29-priors", "random_then_unicode"])
def test_real_command_lists(name):
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text(name))
    streams = gh.ir_streams(ir, 32)
    assert len(streams) >= 8 and all(0 < s[1].size <= 65536 for s in streams) and any(s[2].size > 1 for s in streams)
    cfg = ir.lit_config(dynamic_context_mixing=0)
    # made eligible for the bucketed pass here: constant context, mixing value 4 everywhere, one model
    ctypes.memset(cfg.literal_context_map, 0, ctypes.sizeof(cfg.literal_context_map))
    ctypes.memset(cfg.mixing_mask, 4, 8192)
    cfg.context_mixing = 0
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    coded = gh.oracle_bytes(ocfg, streams)
    tin = gh.ragged_tensors(torch, streams)
    codec = da.LiteralCodec(cfg, max(tin["longest"], 16))
    codec.set_block_types(ir.num_block_types)
    codec.set_encode_path(2)
    outs = codec.alloc_encode_outputs(tin["n"])
    st, got, path = gh.encode_segments(codec, tin, outs)
    assert st == 0 and path == 2, (st, path)
    gh.assert_same(got, coded, streams, name)
    gh.assert_round_trip_segments(torch, codec, tin, outs, streams, name)
    codec.close()
    ir.close()
