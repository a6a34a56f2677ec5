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
import history_cases as hc
import irtext
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
OUT_SENTINEL, SIZE_SENTINEL = 0x3C, 0x5A5A5A5A
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _code(ocfg, streams):
    return [po.lit_segments_encode(ocfg, s["lit"], s["segs"]["len"], s["segs"]["btype"], s["segs"]["last8"]) for s in streams]


def _batch(fam, o, streams, mode="own"):
    """(streams, the oracle's bytes, the batch's layout with the coded bytes in place, the histories' layout)"""
    coded = _code(o, streams)
    return streams, coded, cc.layout(streams, coded), hc.history_layout(streams, mode, hc.dictionary_of(fam))


def _case(fam, sources, mode):
    """the family's configurations and its directed batch under one mode: computed once, shared, never written to"""
    if (fam.name, mode) not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        _CASES[fam.name, mode] = (g, o) + _batch(fam, o, hc.directed(fam, sources, mode), mode)
    return _CASES[fam.name, mode]


def _tensors(torch, lay):
    dev = torch.device("cuda")
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in lay.items() if isinstance(v, np.ndarray)}


def _even(n):
    """the codec keeps an even max_stream_len, and alloc_encode_outputs sizes the slots for the length it was given"""
    return max(n, 16) + n % 2


def _codec(da, fam, g, longest):
    codec = da.LiteralCodec(g, _even(longest))
    codec.set_block_types(fam.n_btypes)
    return codec


def _hist_args(ht):
    return dict(hist=ht["hist"], hist_offsets=ht["hist_off"], hist_sizes=ht["hist_sz"])


def _decode(torch, codec, lay, t, hlay, ht, with_ins=True):
    """-> (status, the whole raw buffer, stream flags, name of the kernel that ran); asserts that the history buffer is untouched"""
    raw = t["raw"].clone()
    flags = torch.zeros(lay["n"] + 16, dtype=torch.uint8, device=raw.device)
    codec.set_stream_flags(flags)
    ins = (t["ins"], t["ins_off"], t["ins_sz"]) if with_ins else (None, None, None)
    try:
        codec.decode_commands_batch(t["coded"], t["coded_off"], t["coded_sz"], lay["n"], t["cmd_begin"], t["cmds"], t["lit_sz"], lay["lit_longest"],
                                    raw, t["raw_off"], t["raw_sz"], *ins, **_hist_args(ht))
        st = codec.status()
    finally:
        codec.set_stream_flags(None)
    assert (ht["hist"].cpu().numpy() == hlay["hist"]).all(), "the decode call wrote to the history buffer"
    return st, raw.cpu().numpy(), flags.cpu().numpy(), codec.last_decode_kernel()


def _assert_raw(got, lay, streams, what, skip=()):
    """the whole raw buffer against the expectation, sentinels included (the raw ranges of the streams in `skip` left out)"""
    same = got == lay["expect"]
    for i in skip:
        ro = int(lay["raw_off"][i]); same[ro:ro + int(lay["raw_sz"][i])] = True
    if same.all():
        return
    at = int(np.argmin(same))
    inside = [i for i in range(lay["n"]) if int(lay["raw_off"][i]) <= at < int(lay["raw_off"][i]) + int(lay["raw_sz"][i])]
    if inside:
        i = inside[0]
        raise AssertionError(f"{what}: stream {i} ({streams[i]['name']}, {int(lay['raw_sz'][i])} raw bytes, {streams[i]['hist'].size} history bytes) "
                             f"wrong from its byte {at - int(lay['raw_off'][i])}")
    raise AssertionError(f"{what}: sentinel byte {at} of the raw buffer overwritten with {int(got[at])}")


def _enc_lay(lay):
    """the layout with the raw bytes in place (what a compressor hands over)"""
    lay = dict(lay)
    lay["raw"] = lay["expect"].copy()
    return lay


def _encode(torch, codec, lay, t, hlay, ht, with_ins=True, hist_is_raw=False):
    """-> dict(status, coded = [bytes of stream i], lit_sz, flags) and asserts that the call left its inputs and everything behind its
    outputs alone.  hist_is_raw: the history pointer is the raw buffer itself (ht holds the offsets and sizes only)."""
    n = lay["n"]
    outs = codec.alloc_encode_outputs(n)
    outs["out"].fill_(OUT_SENTINEL); outs["offsets"].fill_(-1); outs["sizes"].fill_(-1)
    lit_sz = torch.full((n + 16,), SIZE_SENTINEL, dtype=torch.int32, device=t["raw"].device)
    flags = torch.zeros(n + 16, dtype=torch.uint8, device=t["raw"].device)
    codec.set_stream_flags(flags)
    ins = (t["ins"], t["ins_off"], t["ins_sz"]) if with_ins else (None, None, None)
    hist = dict(hist=t["raw"], hist_offsets=ht["hist_off"], hist_sizes=ht["hist_sz"]) if hist_is_raw else _hist_args(ht)
    try:
        codec.encode_commands_batch(t["raw"], t["raw_off"], t["raw_sz"], n, t["cmd_begin"], t["cmds"], lay["lit_longest"], outs, lit_sz, *ins, **hist)
        st = codec.status()
    finally:
        codec.set_stream_flags(None)
    out = outs["out"].cpu().numpy(); offs = outs["offsets"].cpu().numpy(); sz = outs["sizes"].cpu().numpy()
    for k in ("raw", "cmds", "cmd_begin", "ins", "raw_off", "raw_sz", "ins_off", "ins_sz"):
        assert (t[k].cpu().numpy() == np.ascontiguousarray(lay[k])).all(), f"the call wrote to its input `{k}`"
    for k in ("hist_off", "hist_sz") + (() if hist_is_raw else ("hist",)):
        assert (ht[k].cpu().numpy() == hlay[k]).all(), f"the call wrote to its input `{k}`"
    lit_sz = lit_sz.cpu().numpy(); flags = flags.cpu().numpy()
    assert (lit_sz[n:] == SIZE_SENTINEL).all() and not flags[n:].any() and (out[n * outs["slot"]:] == OUT_SENTINEL).all(), "bytes written behind the outputs"
    spans = [(int(offs[i]), int(offs[i]) + int(sz[i])) for i in range(n)]
    for i, (b, e) in enumerate(spans):
        assert i * outs["slot"] <= b <= e <= (i + 1) * outs["slot"], f"stream {i} lies outside its slot: {b}..{e}"
    return dict(status=st, coded=[out[b:e] for b, e in spans], lit_sz=lit_sz[:n], flags=flags[:n])


def _assert_coded(res, streams, coded, what, skip=()):
    for i, (got, ref) in enumerate(zip(res["coded"], coded)):
        if i in skip:
            continue
        assert got.size == ref.size and (got == ref).all(), f"{what}: stream {i} ({streams[i]['name']}, {streams[i]['hist'].size} history bytes) differs from the oracle"
        assert int(res["lit_sz"][i]) == streams[i]["lit"].size, (what, i, streams[i]["name"])


def _paths(codec, da):
    """the encode paths to run: the streaming kernels, and the bucketed passes where the codec has them"""
    paths = [1]
    try:
        codec.set_encode_path(2)
        paths.append(2)
    except da.DivansGpuError:
        pass
    return paths


def _round_trip(torch, codec, streams, res, lay, hlay, ht, what):
    """the contract: the GPU's coded bytes (re-laid at 4-byte offsets) and its d_lit_sizes, with the same lists and history, decode to the raw bytes"""
    back = cc.layout(streams, [c.copy() for c in res["coded"]], lit_sizes=res["lit_sz"].tolist())
    assert (back["expect"] == lay["expect"]).all()
    st, raw, flags, name = _decode(torch, codec, back, _tensors(torch, back), hlay, ht)
    assert st == 0 and not flags.any(), (what, st, name)
    _assert_raw(raw, back, streams, what + ", round trip")


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_directed_decode(fam, sources):
    """histories of their own at every alignment (grids of two workgroups and of one: every group runs several streams in a row, so
    the cursor's history is reset), one range shared by every stream, and windows of one dictionary that partly overlap"""
    import torch
    import divans_amd as da
    codec = None
    for mode in hc.MODES:
        g, o, streams, coded, lay, hlay = _case(fam, sources, mode)
        codec = codec or _codec(da, fam, g, lay["lit_longest"])
        t, ht = _tensors(torch, lay), _tensors(torch, hlay)
        for blocks in ((2, 1) if mode == "own" else (2,)):
            what = f"{mode}, {blocks} workgroups"
            codec.set_geometry(blocks=blocks)
            st, raw, flags, name = _decode(torch, codec, lay, t, hlay, ht)
            assert st == 0 and "lit_decode2_cmd_hist_kernel" in name, (what, st, name)
            _assert_raw(raw, lay, streams, what)
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
    batches.append(("prepare edges",) + _batch(fam, o, hc.encode_extras(fam, sources)))
    codec = _codec(da, fam, g, max(b[3]["lit_longest"] for b in batches))
    codec.set_geometry(blocks=2)
    paths = _paths(codec, da)
    for which, streams, coded, lay, hlay in batches:
        lay = _enc_lay(lay)
        t, ht = _tensors(torch, lay), _tensors(torch, hlay)
        for path in paths:
            what = f"{which}, path {path}"
            codec.set_encode_path(path)
            res = _encode(torch, codec, lay, t, hlay, ht)
            assert res["status"] == 0 and not res["flags"].any(), (what, res["status"], np.flatnonzero(res["flags"]).tolist())
            assert codec.last_encode_path() == 1 if path == 1 else codec.last_encode_path() in (2, 3), (what, codec.last_encode_path())
            _assert_coded(res, streams, coded, what)
        _round_trip(torch, codec, streams, res, lay, hlay, ht, which)
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
    coded = _code(o, pieces)
    lay, hlay = _cut_layout(pieces, coded)
    enc = _enc_lay(lay)
    codec = _codec(da, fam, g, lay["lit_longest"])
    t, ht = _tensors(torch, enc), _tensors(torch, hlay)
    res = _encode(torch, codec, enc, t, hlay, ht, hist_is_raw=True)
    assert res["status"] == 0 and not res["flags"].any(), res["status"]
    _assert_coded(res, pieces, coded, "3 pieces")
    raw, sts = _decode_pieces_in_turn(torch, codec, lay, _tensors(torch, lay), ht)
    codec.close()
    assert sts == [0, 0, 0]
    _assert_raw(raw, lay, pieces, "3 pieces decoded in turn")


@pytest.mark.parametrize("fam", [f for f in sc.FAMILIES if f.name in ("mm4_const_plain", "mm0_map_mix", "mmx_map_plain_nocache")], ids=repr)
def test_history_decodes_as_an_insert_through_the_merged_call(fam, sources):
    """cross-check against merged code: decoding with history H writes the same bytes at raw[0:] as the call WITHOUT history
    writes at raw[h:] for [INSERT h] + cmds, H in front of the insert bytes.  The merged symbol, unchanged."""
    import torch
    import divans_amd as da
    g, o, streams, coded, lay, hlay = _case(fam, sources, "own")
    plain = [hc.as_plain(s) for s in streams]
    play = cc.layout(plain, coded)
    codec = _codec(da, fam, g, lay["lit_longest"])
    st, with_hist, flags, name = _decode(torch, codec, lay, _tensors(torch, lay), hlay, _tensors(torch, hlay))
    t = _tensors(torch, play)
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


def _ir_stream(ir, name):
    cmds, ins = ir.device_commands()
    lit, segs = ir.literal_segments()
    return dict(name=name, cmds=cmds, lit=lit, ins=ins, raw=ir.expand(), segs=segs)


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
    whole = _ir_stream(ir, "alice29-q11")
    pieces = hc.cut(whole, 8)
    reaching = sum(len(hc.reaching_copies(p)) for p in pieces)
    assert reaching > 0 and all(p["cmds"].size for p in pieces), "no copy of the cut lists reaches into history: the test would prove nothing"
    coded = _code(ocfg, pieces)
    lay, hlay = _cut_layout(pieces, coded)
    enc = _enc_lay(lay)
    with_ins = whole["ins"].size > 0
    codec = da.LiteralCodec(cfg, _even(lay["lit_longest"]))
    codec.set_block_types(ir.num_block_types)
    ht = _tensors(torch, hlay)
    res = _encode(torch, codec, enc, _tensors(torch, enc), hlay, ht, with_ins=with_ins, hist_is_raw=True)
    assert res["status"] == 0 and not res["flags"].any(), res["status"]
    _assert_coded(res, pieces, coded, "alice29-q11 in 8 pieces")
    back = cc.layout(pieces, [c.copy() for c in res["coded"]], lit_sizes=res["lit_sz"].tolist())
    for k in ("expect", "raw", "raw_off"):
        back[k] = lay[k]
    raw, sts = _decode_pieces_in_turn(torch, codec, back, _tensors(torch, back), ht, with_ins=with_ins)
    full = ir.expand()
    codec.close(); ir.close()
    assert sts == [0] * 8, sts
    _assert_raw(raw, lay, pieces, "alice29-q11 decoded piece by piece")
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
    _, coded, lay, hlay = _batch(fam, o, good)
    codec = _codec(da, fam, g, 64)
    codec.set_geometry(blocks=1)
    ht = _tensors(torch, hlay)
    st, raw, flags, name = _decode(torch, codec, lay, _tensors(torch, lay), hlay, ht)
    assert st == 0 and not flags.any(), (st, name)
    _assert_raw(raw, lay, good, "the good list")
    none = sc.segments([], [], [])
    empty = po.lit_segments_encode(o, np.zeros(0, np.uint8), none["len"], none["btype"], none["last8"])
    for what, cmds in hc.faulty_lists(victim):
        batch = list(good)
        batch[at] = dict(victim, cmds=cmds)
        lay = cc.layout(batch, coded)
        st, raw, flags, name = _decode(torch, codec, lay, _tensors(torch, lay), hlay, ht)
        assert st & cc.BAD_COMMAND and not st & ~(cc.BAD_COMMAND | cc.BAD_STREAM), (what, st, name)
        assert flags[at] == 1 and int(flags.sum()) == 1, (what, flags[:lay["n"]].tolist())
        _assert_raw(raw, lay, batch, what, skip=(at,))
        enc = _enc_lay(lay)
        res = _encode(torch, codec, enc, _tensors(torch, enc), hlay, ht)
        assert res["status"] == cc.BAD_COMMAND and np.flatnonzero(res["flags"]).tolist() == [at] and int(res["lit_sz"][at]) == 0, (what, res["status"])
        assert res["coded"][at].size == empty.size and (res["coded"][at] == empty).all(), what
        _assert_coded(res, batch, coded, what, skip=(at,))
    for what, hist, raw_bytes in hc.faulty_bytes(victim):       # encode only: a history or raw byte that a history-reaching copy compares
        batch = list(good)
        batch[at] = dict(victim, hist=hist, raw=raw_bytes)
        enc = _enc_lay(cc.layout(batch, coded))
        hl = hc.history_layout(batch)
        res = _encode(torch, codec, enc, _tensors(torch, enc), hl, _tensors(torch, hl))
        assert res["status"] == cc.BAD_COMMAND and np.flatnonzero(res["flags"]).tolist() == [at] and int(res["lit_sz"][at]) == 0, (what, res["status"])
        assert res["coded"][at].size == empty.size and (res["coded"][at] == empty).all(), what
        _assert_coded(res, batch, coded, what, skip=(at,))
    codec.close()


def test_partial_history_triple_is_refused_and_a_null_triple_is_the_merged_call(sources):
    """DIVANS_GPU_EINVAL for every incomplete triple, in both calls; all three NULL: the outputs of the merged symbols, byte for byte"""
    import torch
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == "mm4_map_mix")
    g, o = fam.pair(da, po)
    streams = cc.directed(fam, sources)[:30]                    # the merged tests' batch: lists without history
    coded = _code(o, streams)
    lay = cc.layout(streams, coded)
    enc = _enc_lay(lay)
    codec = _codec(da, fam, g, lay["lit_longest"])
    L, h = codec._lib, codec._h
    t, te = _tensors(torch, lay), _tensors(torch, enc)
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
        outs = codec.alloc_encode_outputs(n)
        outs["out"].fill_(OUT_SENTINEL); outs["offsets"].fill_(-1); outs["sizes"].fill_(-1)
        return outs, torch.full((n,), SIZE_SENTINEL, dtype=torch.int32, device=some.device)
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
    assert (raw == t["raw"]).all() and (outs["out"] == OUT_SENTINEL).all(), "a refused call wrote something"
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
