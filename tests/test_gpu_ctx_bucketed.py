"""The context-keyed bucketed encoder passes (lit_bucket_ctx.hip) behind divans_gpu_codec_set_encode_path(c, 2) -- and, for calls
without a segment list, behind "automatic": a context map in use and every mixing value 0, one model or two, up to eight block
types.  ctx_sort_kernel keys every position by
ctxf[block type of the covering segment][prev][class of prev_prev]; both models' chains walk the buckets of that one sort.  Every
comparison is against the C oracle's bytes (tests/test_ctx_bucketed_cases_cpu.py guards the oracle and the shapes); the pass that
ran is asserted through divans_gpu_codec_last_encode_path."""

import numpy as np
import pytest

import bucketed_segment_cases as bc
import gpu_harness as gh
import ctx_bucketed_cases as cc
import irtext
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
KEYS = list(cc.FAMILIES)
LENGTHS = [1, 2, 63, 64, 65, 8191, 8192, 8193, 16385, 40000, 65535, 65536]
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(key, sources):
    """the configuration pair, its batch and the oracle's bytes of every stream: computed once, shared, never written to"""
    if key not in _CASES:
        import divans_amd as da
        fam = cc.FAMILIES[key]
        g, o = fam.pair(da, po)
        streams = cc.batch(fam, sources)
        _CASES[key] = (fam, g, o, streams, gh.oracle_bytes(o, streams))
    return _CASES[key]


@pytest.mark.parametrize("key", KEYS)
def test_path_2_accepts_context_keyed_rows(key, sources):
    """mixing value 0 with a context map, 8 block types and 1: set_encode_path(2) is accepted -- as the codec is created (tables for the
    configuration's own block type) and after set_block_types -- and the call reports the bucketed pass, 2 for one model, 3 for two"""
    import torch
    import divans_amd as da
    fam, g, o, streams, coded = _case(key, sources)
    few = [s for s in streams if s[1].size <= 4000][:12]
    ref = [coded[k] for k, s in enumerate(streams) if s[1].size <= 4000][:12]
    tin = gh.ragged_tensors(torch, few)
    codec = da.LiteralCodec(g, max(tin["longest"], 16))
    codec.set_encode_path(2)
    codec.set_block_types(fam.n_btypes)
    codec.set_encode_path(0)
    codec.set_encode_path(2)
    assert codec.last_encode_path() == 0
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == cc.BUCKETED_PATH[key], (st, path)
    gh.assert_same(got, ref, few, "path 2")
    codec.set_encode_path(0)          # automatic: a list stays on the streaming kernels, a call without one takes the bucketed pass
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, ref, few, "automatic")
    outs = codec.alloc_encode_outputs(tin["n"])
    codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
    assert codec.status() == 0 and codec.last_encode_path() == cc.BUCKETED_PATH[key]
    auto = gh.split_outputs(outs, tin["n"])
    codec.set_encode_path(1)
    codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
    assert codec.status() == 0 and codec.last_encode_path() == 1
    for i, (a, b) in enumerate(zip(auto, gh.split_outputs(outs, tin["n"]))):
        assert a.size == b.size and (a == b).all(), f"automatic without a list: stream {i} ({few[i][0]})"
    codec.close()


@pytest.mark.parametrize("name", cc.REFUSED)
def test_a_constant_context_stays_refused(name):
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == name)
    g, _ = fam.pair(da, po)
    codec = gh.codec_for(da, fam, g, 4096)
    with pytest.raises(da.DivansGpuError, match="bucketed encoder needs"):
        codec.set_encode_path(2)
    codec.close()


@pytest.mark.parametrize("key", KEYS)
def test_context_keyed_pass_codes_segment_lists_bit_exact(key, sources):
    import torch
    import divans_amd as da
    fam, g, o, streams, coded = _case(key, sources)
    tin = gh.ragged_tensors(torch, streams)
    assert tin["longest"] == 65536 and tin["n"] == 47
    codec = gh.codec_for(da, fam, g, tin["longest"])
    codec.set_encode_path(2)
    for what, sub in (("one launch sequence", None), ("launch sequences of 24 streams", 24)):
        if sub:
            codec.set_bucket_batch(sub)
        st, got, path = gh.encode_segments(codec, tin)
        assert st == 0 and path == cc.BUCKETED_PATH[key], (what, st, path)
        gh.assert_same(got, coded, streams, what)
    codec.set_encode_path(1)
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, coded, streams, "streaming kernels")
    codec.close()


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_context_keyed_pass_over_prediction_modes(mode, mix, sources):
    """LSB6 / MSB6 / UTF8 / SIGN: 1, 1, 4 and 8 classes of prev_prev; random maps whose contexts use the whole byte; two block types"""
    import torch
    import divans_amd as da
    g = cc.mode_config(da.config_context_mixing(), mode, mix, 10 * mode + mix)
    o = cc.mode_config(po.config_context_mixing(), mode, mix, 10 * mode + mix)
    assert bytes(g) == bytes(o)
    corpus, rtu, _ = sources
    L = 20000
    rng = np.random.default_rng(710 + mode)
    blocks = [corpus[3000:3000 + L], rtu[100000:100000 + L], rtu[200000:200000 + L], rng.integers(0, 256, L, dtype=np.uint8)]
    cuts = [1, 2, 5000, 8191, 8193, 12000, 16384]
    streams = []
    for k, lit in enumerate(blocks):
        lens = sc._cut(L, cuts)
        starts = [0] + cuts
        streams.append((f"M{k}", lit.copy(), sc.segments(lens, (np.arange(len(lens)) + k) % 2, bc._last8s(rng, lit, starts))))
    coded = gh.oracle_bytes(o, streams)
    tin = gh.ragged_tensors(torch, streams)
    codec = da.LiteralCodec(g, L)
    codec.set_block_types(2)
    codec.set_encode_path(2)
    st, got, path = gh.encode_segments(codec, tin)
    assert st == 0 and path == (3 if mix else 2), (st, path)
    gh.assert_same(got, coded, streams, f"mode {mode}")
    outs = codec.alloc_encode_outputs(tin["n"])       # and without the lists: block type 0 throughout
    codec.encode_batch(tin["lit"], tin["n"], L, outs, in_offsets=tin["off"], in_sizes=tin["sz"])
    assert codec.status() == 0 and codec.last_encode_path() == (3 if mix else 2)
    for i, (a, lit) in enumerate(zip(gh.split_outputs(outs, tin["n"]), blocks)):
        b = po.lit_encode(o, lit)
        assert a.size == b.size and (a == b).all(), (mode, mix, i)
    codec.close()


@pytest.mark.parametrize("key", ["plain", "mix"])
@pytest.mark.parametrize("n", LENGTHS)
def test_context_keyed_pass_without_a_list(n, key, sources):
    """encode_batch under path 2: ragged offsets on both load alignments, the configuration's own block type (3, not 0)"""
    import torch
    import divans_amd as da
    fam = cc.FAMILIES[key]
    g, o = fam.pair(da, po)
    assert g.btype == 3
    blocks = cc.plain_streams(n, sources)
    buf, offs, sizes = cc.ragged_layout(blocks)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    codec = da.LiteralCodec(g, max(n, 16))
    codec.set_encode_path(2)
    outs = codec.alloc_encode_outputs(len(blocks))
    codec.encode_batch(t(buf), len(blocks), n, outs, in_offsets=t(offs), in_sizes=t(sizes))
    assert codec.status() == 0 and codec.last_encode_path() == cc.BUCKETED_PATH[key]
    got = gh.split_outputs(outs, len(blocks))
    for i, (a, lit) in enumerate(zip(got, blocks)):
        b = po.lit_encode(o, lit)
        assert a.size == b.size and (a == b).all(), (n, key, i)
    codec.close()


@pytest.mark.parametrize("key", ["plain", "mix"])
def test_faulty_lists_are_reported_by_the_context_keyed_pass(key, sources):
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
    batches.append(("empty stream, list of 5 bytes", bc.empty_stream_with_bytes_in_its_list(good, 4), (4,)))
    tins = [gh.ragged_tensors(torch, batch) for _, batch, _ in batches]
    codec = gh.codec_for(da, fam, g, max(t["longest"] for t in tins))
    codec.set_encode_path(2)
    for (what, batch, skip), tin in zip(batches, tins):
        st, got, path = gh.encode_segments(codec, tin)
        assert st & gh.BAD_SEGMENT and path == cc.BUCKETED_PATH[key], (what, st, path)
        gh.assert_same(got, coded, batch, what, skip=skip)
    st, got, path = gh.encode_segments(codec, gh.ragged_tensors(torch, good))
    assert st == 0 and path == cc.BUCKETED_PATH[key], (st, path)
    gh.assert_same(got, coded, good, "the same streams with their lists in order")
    codec.close()


@pytest.mark.parametrize("mixing", [0, 2])
@pytest.mark.parametrize("name", ["alice29-q11", "random_then_unicode"])
def test_real_command_lists_under_their_own_context_maps(name, mixing):
    """The literals of an IR file as the container codes them: its context map, no mixing values named -> every mixing value 0.
    random_then_unicode.ir brings 4 block types with 11 distinct contexts and takes the context-keyed pass.  alice29-q11.ir's map
    holds ONE context (all 64 entries of its one block type are equal): a constant context is one bucket per stream, which the pass
    refuses by rule -- that file is coded by the streaming kernels and the refusal is what is asserted for it."""
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text(name))
    streams = gh.ir_streams(ir, 32)
    assert len(streams) >= 8 and all(0 < s[1].size <= 65536 for s in streams) and any(s[2].size > 1 for s in streams)
    cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
    assert set(bytes(cfg.mixing_mask)) == {0}            # uniformly 0: no mixing-value-4 pass can be what runs below
    cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)[:64 * ir.num_block_types]
    constant = len(set(cmap.tolist())) == 1
    assert constant == (name == "alice29-q11")
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    coded = gh.oracle_bytes(ocfg, streams)
    tin = gh.ragged_tensors(torch, streams)
    codec = da.LiteralCodec(cfg, max(tin["longest"], 16))
    codec.set_block_types(ir.num_block_types)
    if constant:
        with pytest.raises(da.DivansGpuError, match="bucketed encoder needs"):
            codec.set_encode_path(2)
    else:
        codec.set_encode_path(2)
    outs = codec.alloc_encode_outputs(tin["n"])
    st, got, path = gh.encode_segments(codec, tin, outs)
    assert st == 0 and path == (1 if constant else 3 if mixing else 2), (st, path)
    gh.assert_same(got, coded, streams, name)
    gh.assert_round_trip_segments(torch, codec, tin, outs, streams, name)
    codec.close()
    ir.close()
