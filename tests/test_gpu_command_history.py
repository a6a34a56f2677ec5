"""divans_gpu_lit_decode_commands_history_batch / divans_gpu_lit_encode_commands_history_batch: command lists of streams that have
known bytes in front of them -- the earlier pieces of a file, or a dictionary the streams of a batch share.  A COPY may reach into
those bytes, a Literal command near a stream's start takes its context from them.

Every expectation is the C ORACLE's bytes (po.lit_segments_encode) for the segments the Python executor of tests/history_cases.py
derives, and that executor's raw bytes (tests/test_history_cases_cpu.py pins it to the executor the merged tests trust); nothing is
compared with the code under test but where a test says so (the cross-check against the merged call, the all-NULL triple).  Raw
outputs and histories lie between sentinel bytes and are compared whole afterwards."""
import numpy as np
import pytest

import command_cases as cc
import gpu_harness as gh
import history_cases as hc
import irtext
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(fam, sources, mode):
    """the family's configurations and its directed batch under one mode: computed once, shared, never written to"""
    if (fam.name, mode) not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        _CASES[fam.name, mode] = (g, o) + gh.history_batch(fam, o, hc.directed(fam, sources, mode), mode)
    return _CASES[fam.name, mode]


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_directed_decode(fam, sources):
    """histories of their own at every alignment (grids of two workgroups and of one: every group runs several streams in a row, so
    the cursor's history is reset), one range shared by every stream, and windows of one dictionary that partly overlap"""
    import torch
    import divans_amd as da
    codec = None
    for mode in hc.MODES:
        g, o, streams, coded, lay, hlay = _case(fam, sources, mode)
        codec = codec or gh.codec_for(da, fam, g, lay["lit_longest"], even=True)
        t, ht = gh.to_device(torch, lay), gh.to_device(torch, hlay)
        for blocks in ((2, 1) if mode == "own" else (2,)):
            what = f"{mode}, {blocks} workgroups"
            codec.set_geometry(blocks=blocks)
            st, raw, flags, name = gh.decode_commands(torch, codec, lay, t, hlay, ht)
            assert st == 0 and "lit_decode2_cmd_hist_kernel" in name, (what, st, name)
            gh.assert_raw(raw, lay, streams, what)
            assert not flags.any(), what
    codec.close()


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_directed_encode(fam, sources):
    """the same batches, and the lists on the prepare kernel's edges, through the encode call under every encode path the family has:
    the oracle's bytes and literal sizes, then back through the decode call"""
    import torch
    import divans_amd as da
    g, o = fam.pair(da, po)
    batches = [(mode,) + _case(fam, sources, mode)[2:] for mode in hc.MODES]
    batches.append(("prepare edges",) + gh.history_batch(fam, o, hc.encode_extras(fam, sources)))
    codec = gh.codec_for(da, fam, g, max(b[3]["lit_longest"] for b in batches), even=True)
    codec.set_geometry(blocks=2)
    paths = gh.encode_paths(codec, da)
    for which, streams, coded, lay, hlay in batches:
        lay = gh.encode_layout(lay)
        t, ht = gh.to_device(torch, lay), gh.to_device(torch, hlay)
        for path in paths:
            what = f"{which}, path {path}"
            codec.set_encode_path(path)
            res = gh.encode_commands(torch, codec, lay, t, hlay, ht)
            assert res["status"] == 0 and not res["flags"].any(), (what, res["status"], np.flatnonzero(res["flags"]).tolist())
            assert codec.last_encode_path() == 1 if path == 1 else codec.last_encode_path() in (2, 3), (what, codec.last_encode_path())
            gh.assert_coded(res, streams, coded, what)
        gh.round_trip_commands(torch, codec, streams, res, lay, which, hlay, ht)
    codec.close()


def _cut_layout(pieces, coded, base=37):
    """pieces of ONE buffer: the raw ranges lie back to back from `base` on, piece k's history is the buffer from `base` to its start"""
    lay = cc.layout(pieces, coded)
    total = sum(p["raw"].size for p in pieces)
    expect = np.full(base + total + 64, cc.RAW_SENTINEL, np.uint8)
    expect[base:base + total] = np.concatenate([p["raw"] for p in pieces])
    lay["expect"] = expect
    lay["raw"] = np.full(expect.size, cc.RAW_SENTINEL, np.uint8)
    lay["raw_off"] = np.array([base + p["raw_at"] for p in pieces], np.int64)
    hlay = dict(hist_off=np.full(len(pieces), base, np.int64), hist_sz=np.array([p["raw_at"] for p in pieces], np.int32))
    return lay, hlay


def _decode_pieces_in_turn(torch, codec, lay, t, ht, with_ins=True):
    """one decode call per piece, each reading what the earlier calls wrote -> (the whole raw buffer, [status of call k])"""
    raw = t["raw"].clone()
    ins = lambda k: (t["ins"], t["ins_off"][k:], t["ins_sz"][k:]) if with_ins else (None, None, None)
    sts = []
    for k in range(lay["n"]):
        codec.decode_commands_batch(t["coded"], t["coded_off"][k:], t["coded_sz"][k:], 1, t["cmd_begin"][k:], t["cmds"], t["lit_sz"][k:], lay["lit_longest"],
                                    raw, t["raw_off"][k:], t["raw_sz"][k:], *ins(k), hist=raw, hist_offsets=ht["hist_off"][k:], hist_sizes=ht["hist_sz"][k:])
        sts.append(codec.status())
    return raw.cpu().numpy(), sts


def test_three_pieces_of_one_buffer_with_history_inside_the_raw_buffer(sources):
    """one encode call whose history ranges lie inside d_raw: a 3-piece cut of one buffer, each piece's history the bytes in front of it"""
    import torch
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == "mm4_map_mix")
    g, o = fam.pair(da, po)
    rng = np.random.default_rng(96700)
    s = cc.Stream("file", fam, sc._Data(sources, rng), rng)
    for i in range(90):
        s.lit(5 + i % 9).copy(3 + i % 40, 1 + (i * 7) % s.produced).ins(i % 4)
    pieces = hc.cut(s.done(), 3)
    assert all(hc.reaching_copies(p) for p in pieces[1:])
    coded = gh.oracle_bytes(o, pieces)
    lay, hlay = _cut_layout(pieces, coded)
    enc = gh.encode_layout(lay)
    codec = gh.codec_for(da, fam, g, lay["lit_longest"], even=True)
    t, ht = gh.to_device(torch, enc), gh.to_device(torch, hlay)
    res = gh.encode_commands(torch, codec, enc, t, hlay, ht, hist_is_raw=True)
    assert res["status"] == 0 and not res["flags"].any(), res["status"]
    gh.assert_coded(res, pieces, coded, "3 pieces")
    raw, sts = _decode_pieces_in_turn(torch, codec, lay, gh.to_device(torch, lay), ht)
    codec.close()
    assert sts == [0, 0, 0]
    gh.assert_raw(raw, lay, pieces, "3 pieces decoded in turn")


@pytest.mark.parametrize("fam", [f for f in sc.FAMILIES if f.name in ("mm4_const_plain", "mm0_map_mix", "mmx_map_plain_nocache")], ids=repr)
def test_history_decodes_as_an_insert_through_the_merged_call(fam, sources):
    """cross-check against merged code: decoding with history H writes the same bytes at raw[0:] as the call WITHOUT history
    writes at raw[h:] for [INSERT h] + cmds, H in front of the insert bytes.  The merged symbol, unchanged."""
    import torch
    import divans_amd as da
    g, o, streams, coded, lay, hlay = _case(fam, sources, "own")
    plain = [hc.as_plain(s) for s in streams]
    play = cc.layout(plain, coded)
    codec = gh.codec_for(da, fam, g, lay["lit_longest"], even=True)
    st, with_hist, flags, name = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay), hlay, gh.to_device(torch, hlay))
    t = gh.to_device(torch, play)
    raw = t["raw"].clone()
    codec.decode_commands_batch(t["coded"], t["coded_off"], t["coded_sz"], play["n"], t["cmd_begin"], t["cmds"], t["lit_sz"], play["lit_longest"],
                                raw, t["raw_off"], t["raw_sz"], t["ins"], t["ins_off"], t["ins_sz"])
    st2 = codec.status()
    codec.close()
    assert st == 0 and st2 == 0 and not flags.any(), (st, st2)
    raw = raw.cpu().numpy()
    assert (raw == play["expect"]).all(), "the merged call on [INSERT h] + cmds"
    for i, s in enumerate(streams):
        a = int(lay["raw_off"][i]); b = int(play["raw_off"][i]) + s["hist"].size
        assert (with_hist[a:a + s["raw"].size] == raw[b:b + s["raw"].size]).all(), s["name"]


@pytest.mark.parametrize("mixing", [0, 2])
def test_golden_ir_cut_into_pieces(mixing):
    """real data: the device command list of alice29-q11 cut at command boundaries into 8 pieces, each with every raw byte in front of
    it as its history.  All pieces are encoded in ONE call (history inside d_raw) and decoded piece by piece in successive calls,
    each reading what the earlier calls wrote: coded bytes against the per-piece oracle, raw bytes against divans_ir_expand."""
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text("alice29-q11"))
    cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    whole = gh.ir_stream(ir, "alice29-q11")
    pieces = hc.cut(whole, 8)
    reaching = sum(len(hc.reaching_copies(p)) for p in pieces)
    assert reaching > 0 and all(p["cmds"].size for p in pieces), "no copy of the cut lists reaches into history: the test would prove nothing"
    coded = gh.oracle_bytes(ocfg, pieces)
    lay, hlay = _cut_layout(pieces, coded)
    enc = gh.encode_layout(lay)
    with_ins = whole["ins"].size > 0
    codec = da.LiteralCodec(cfg, gh.max_stream_len(lay["lit_longest"], even=True))
    codec.set_block_types(ir.num_block_types)
    ht = gh.to_device(torch, hlay)
    res = gh.encode_commands(torch, codec, enc, gh.to_device(torch, enc), hlay, ht, with_ins=with_ins, hist_is_raw=True)
    assert res["status"] == 0 and not res["flags"].any(), res["status"]
    gh.assert_coded(res, pieces, coded, "alice29-q11 in 8 pieces")
    back = cc.layout(pieces, [c.copy() for c in res["coded"]], lit_sizes=res["lit_sz"].tolist())
    for k in ("expect", "raw", "raw_off"):
        back[k] = lay[k]
    raw, sts = _decode_pieces_in_turn(torch, codec, back, gh.to_device(torch, back), ht, with_ins=with_ins)
    full = ir.expand()
    codec.close(); ir.close()
    assert sts == [0] * 8, sts
    gh.assert_raw(raw, lay, pieces, "alice29-q11 decoded piece by piece")
    assert (raw[37:37 + full.size] == full).all()


FAULT_FAMILIES = [f for f in sc.FAMILIES if f.name in ("mm4_const_plain", "mm0_map_plain", "mm4_map_mix", "mmx_map_mix_nocache")]


@pytest.mark.parametrize("fam", FAULT_FAMILIES, ids=repr)
def test_faulty_lists_are_reported_and_contained(fam, sources):
    """every faulty list among good neighbours, one call each way: BAD_COMMAND and no other bit (the decoder may add BAD_STREAM: the
    victim's literals are dropped), the stream flags name the victim alone, the neighbours come out exact, no sentinel byte is touched"""
    import torch
    import divans_amd as da
    g, o = fam.pair(da, po)
    victim, neighbour = hc.victim_base(fam, sources)
    at = 3
    good = [neighbour, neighbour, neighbour, victim, neighbour, neighbour, neighbour]
    _, coded, lay, hlay = gh.history_batch(fam, o, good)
    codec = gh.codec_for(da, fam, g, 64, even=True)
    codec.set_geometry(blocks=1)
    ht = gh.to_device(torch, hlay)
    st, raw, flags, name = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay), hlay, ht)
    assert st == 0 and not flags.any(), (st, name)
    gh.assert_raw(raw, lay, good, "the good list")
    none = sc.segments([], [], [])
    empty = po.lit_segments_encode(o, np.zeros(0, np.uint8), none["len"], none["btype"], none["last8"])
    for what, cmds in hc.faulty_lists(victim):
        batch = list(good)
        batch[at] = dict(victim, cmds=cmds)
        lay = cc.layout(batch, coded)
        st, raw, flags, name = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay), hlay, ht)
        assert st & cc.BAD_COMMAND and not st & ~(cc.BAD_COMMAND | cc.BAD_STREAM), (what, st, name)
        assert flags[at] == 1 and int(flags.sum()) == 1, (what, flags[:lay["n"]].tolist())
        gh.assert_raw(raw, lay, batch, what, skip=(at,))
        enc = gh.encode_layout(lay)
        res = gh.encode_commands(torch, codec, enc, gh.to_device(torch, enc), hlay, ht)
        assert res["status"] == cc.BAD_COMMAND and np.flatnonzero(res["flags"]).tolist() == [at] and int(res["lit_sz"][at]) == 0, (what, res["status"])
        assert res["coded"][at].size == empty.size and (res["coded"][at] == empty).all(), what
        gh.assert_coded(res, batch, coded, what, skip=(at,))
    for what, hist, raw_bytes in hc.faulty_bytes(victim):       # encode only: a history or raw byte that a history-reaching copy compares
        batch = list(good)
        batch[at] = dict(victim, hist=hist, raw=raw_bytes)
        enc = gh.encode_layout(cc.layout(batch, coded))
        hl = hc.history_layout(batch)
        res = gh.encode_commands(torch, codec, enc, gh.to_device(torch, enc), hl, gh.to_device(torch, hl))
        assert res["status"] == cc.BAD_COMMAND and np.flatnonzero(res["flags"]).tolist() == [at] and int(res["lit_sz"][at]) == 0, (what, res["status"])
        assert res["coded"][at].size == empty.size and (res["coded"][at] == empty).all(), what
        gh.assert_coded(res, batch, coded, what, skip=(at,))
    codec.close()


def test_partial_history_triple_is_refused_and_a_null_triple_is_the_merged_call(sources):
    """DIVANS_GPU_EINVAL for every incomplete triple, in both calls; all three NULL: the outputs of the merged symbols, byte for byte"""
    import torch
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == "mm4_map_mix")
    g, o = fam.pair(da, po)
    streams = cc.directed(fam, sources)[:30]                    # the merged tests' batch: lists without history
    coded = gh.oracle_bytes(o, streams)
    lay = cc.layout(streams, coded)
    enc = gh.encode_layout(lay)
    codec = gh.codec_for(da, fam, g, lay["lit_longest"], even=True)
    L, h = codec._lib, codec._h
    t, te = gh.to_device(torch, lay), gh.to_device(torch, enc)
    n = lay["n"]
    some = torch.zeros(64, dtype=torch.uint8, device=t["raw"].device)
    hoff = torch.zeros(n, dtype=torch.int64, device=some.device); hsz = torch.zeros(n, dtype=torch.int32, device=some.device)
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a

    def decode(sym, raw, *triple):
        return getattr(L, sym)(h, *[ptr(x) for x in (t["coded"], t["coded_off"], t["coded_sz"], n, t["cmd_begin"], t["cmds"], t["lit_sz"], lay["lit_longest"],
                                                    t["ins"], t["ins_off"], t["ins_sz"], raw, t["raw_off"], t["raw_sz"]) + triple])

    def encode(sym, outs, lit_sz, *triple):
        return getattr(L, sym)(h, *[ptr(x) for x in (te["raw"], te["raw_off"], te["raw_sz"], n, te["cmd_begin"], te["cmds"], lay["lit_longest"],
                                                    te["ins"], te["ins_off"], te["ins_sz"], outs["out"], outs["slot"], outs["offsets"], outs["sizes"], lit_sz) + triple])

    def outputs():
        return gh.encode_outputs(codec, n), torch.full((n,), gh.SIZE_SENTINEL, dtype=torch.int32, device=some.device)
    raw = t["raw"].clone()
    outs, lit_sz = outputs()
    for gone in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2)):
        triple = [some, hoff, hsz]
        for k in gone:
            triple[k] = None
        assert decode("divans_gpu_lit_decode_commands_history_batch", raw, *triple) == -1 and b"history bytes" in L.divans_gpu_last_error(), gone
        assert encode("divans_gpu_lit_encode_commands_history_batch", outs, lit_sz, *triple) == -1 and b"history bytes" in L.divans_gpu_last_error(), gone
    with pytest.raises(da.DivansGpuError):
        codec.decode_commands_batch(t["coded"], t["coded_off"], t["coded_sz"], n, t["cmd_begin"], t["cmds"], t["lit_sz"], lay["lit_longest"],
                                    raw, t["raw_off"], t["raw_sz"], t["ins"], t["ins_off"], t["ins_sz"], hist=some)
    assert (raw == t["raw"]).all() and (outs["out"] == gh.OUT_SENTINEL).all(), "a refused call wrote something"
    results = []
    for sym in ("divans_gpu_lit_decode_commands_batch", "divans_gpu_lit_decode_commands_history_batch"):
        raw = t["raw"].clone()
        assert decode(sym, raw, *((None, None, None) if "history" in sym else ())) == 0
        results.append((codec.status(), raw.cpu().numpy()))
    assert results[0][0] == results[1][0] == 0 and (results[0][1] == results[1][1]).all() and (results[0][1] == lay["expect"]).all()
    results = []
    for sym in ("divans_gpu_lit_encode_commands_batch", "divans_gpu_lit_encode_commands_history_batch"):
        outs, lit_sz = outputs()
        assert encode(sym, outs, lit_sz, *((None, None, None) if "history" in sym else ())) == 0
        results.append((codec.status(), outs["out"].cpu().numpy(), outs["offsets"].cpu().numpy(), outs["sizes"].cpu().numpy(), lit_sz.cpu().numpy()))
    codec.close()
    assert results[0][0] == results[1][0] == 0
    for a, b in zip(results[0][1:], results[1][1:]):
        assert (a == b).all()
    offs, sizes = results[1][2], results[1][3]
    for i, ref in enumerate(coded):
        assert int(sizes[i]) == ref.size and (results[1][1][int(offs[i]):int(offs[i]) + ref.size] == ref).all(), streams[i]["name"]
