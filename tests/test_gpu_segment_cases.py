"""The segment entry points on every SEG = true kernel instance: each (MM, CTXC, MIX) family of tests/segment_cases.py codes one
batch of 40 streams whose segment boundaries sit where the kernels change phase (the streaming encoder's 16-byte lane window and
32-byte read-ahead, the decoders' 16-byte output group, the 32 768-byte rANS chunk seam), with empty segments, one-byte segments,
random last_8_literals and block types 0..7, an empty stream in the middle -- bit for bit against the C oracle
(tests/test_segment_cases_cpu.py guards the oracle on the same lists).  The decoders are given the ORACLE's bytes, so an encoder
fault cannot hide a decoder fault; the kernel instance that ran is asserted from its name.  Grids of one and two workgroups make
every resident group code several segmented streams in a row (the per-stream reset of the cursor, the context table, the history
and the Weights), tiny row caches force misses and write-backs."""
import numpy as np
import pytest

import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
BAD_SEGMENT = 4
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _oracle(ocfg, streams):
    return [po.lit_segments_encode(ocfg, lit, segs["len"], segs["btype"], segs["last8"]) for _, lit, segs in streams]


def _case(fam, sources):
    """the family's configurations, its batch and the oracle's bytes of every stream: computed once, shared, never written to"""
    if fam.name not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        streams = sc.shapes(fam, sources)
        coded = _oracle(o, streams)
        s5 = next(i for i, s in enumerate(streams) if s[0] == "S5")
        plain = po.lit_encode(o, streams[s5][1])
        assert coded[s5].size == plain.size and (coded[s5] == plain).all()      # one segment, zero history, own block type = the plain stream
        _CASES[fam.name] = (g, o, streams, coded)
    return _CASES[fam.name]


def _input_tensors(torch, streams):
    """streams: [(name, lit uint8[n], segs)] -> device tensors of the segment entry points"""
    dev = torch.device("cuda")
    sizes = np.array([s[1].size for s in streams], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes[:-1].astype(np.int64))]).astype(np.int64)
    segs = np.concatenate([s[2] for s in streams] + [np.zeros(1, sc.SEG_DTYPE)])      # (one spare record: the array is never empty)
    seg_begin = np.concatenate([[0], np.cumsum([s[2].size for s in streams])]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lit = np.concatenate([s[1] for s in streams] + [np.zeros(64, np.uint8)])
    return dict(lit=t(lit), off=t(offs), sz=t(sizes), sb=t(seg_begin), segs=t(segs.view(np.uint8)), longest=int(sizes.max()), n=len(streams),
                total=int(sizes.sum()))


def _coded_tensors(torch, coded):
    """the oracle's streams side by side, each at a 16-byte boundary"""
    dev = torch.device("cuda")
    sizes = np.array([c.size for c in coded], dtype=np.int32)
    assert (sizes % 4 == 0).all()
    offs = np.concatenate([[0], np.cumsum((sizes[:-1].astype(np.int64) + 15) & ~15)]).astype(np.int64)
    buf = np.zeros(int(offs[-1]) + int(sizes[-1]) + 64, np.uint8)
    for o, c in zip(offs, coded):
        buf[int(o):int(o) + c.size] = c
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(buf), t(offs), t(sizes)


def _codec(da, fam, g, longest):
    codec = da.LiteralCodec(g, max(longest, 16))
    codec.set_block_types(fam.n_btypes)
    return codec


def _encode(torch, codec, tin):
    """-> (status, [coded bytes of stream i])"""
    outs = codec.alloc_encode_outputs(tin["n"], max(tin["longest"], 16))
    codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], tin["n"], tin["longest"], tin["sb"], tin["segs"], outs)
    st = codec.status()
    out = outs["out"].cpu().numpy(); offs = outs["offsets"].cpu().numpy(); sz = outs["sizes"].cpu().numpy()
    return st, [out[int(offs[i]):int(offs[i]) + int(sz[i])] for i in range(tin["n"])]


def _decode(torch, codec, tin, tcoded):
    """-> (status, decoded bytes of the whole batch, name of the kernel that ran)"""
    back = torch.zeros_like(tin["lit"])
    codec.decode_segments_batch(tcoded[0], tcoded[1], tcoded[2], tin["n"], tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"])
    st = codec.status()
    return st, back.cpu().numpy(), codec.last_decode_kernel()


def _b(v):
    return "true" if v else "false"


def _assert_same(got, ref, streams, what, skip=()):
    for i, (g, r) in enumerate(zip(got, ref)):
        if i in skip:
            continue
        assert g.size == r.size and (g == r).all(), f"{what}: stream {i} ({streams[i][0]}, {streams[i][1].size} bytes, {streams[i][2].size} segments) differs from the oracle"


def _assert_decoded(back, tin, streams, what, skip=()):
    offs = tin["off"].cpu().numpy()
    for i, (name, lit, segs) in enumerate(streams):
        if i in skip:
            continue
        got = back[int(offs[i]):int(offs[i]) + lit.size]
        assert (got == lit).all(), f"{what}: stream {i} ({name}, {lit.size} bytes, {segs.size} segments) decoded wrong from byte {int(np.argmax(got != lit))}"
    assert not back[tin["total"]:].any(), f"{what}: bytes written behind the batch"


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_encode_bit_exact_vs_oracle(fam, sources):
    """default high-row cache, no cache, and grids of two and of one workgroup (16 resident groups: every group codes two or three
    streams in a row, the empty one between two others)"""
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    tin = _input_tensors(torch, streams)
    # two codecs, the settings of a chain applied one after the other (a codec's tables are then also reused from launch to launch)
    chains = ((("default", None), ("2 workgroups", dict(blocks=2)), ("1 workgroup", dict(blocks=1))),
              (("no cache", dict(cache_rows=0)), ("no cache, 1 workgroup", dict(blocks=1))))
    for chain in chains:
        codec = _codec(da, fam, g, tin["longest"])
        for what, geometry in chain:
            if geometry:
                codec.set_geometry(**geometry)
            st, got = _encode(torch, codec, tin)
            assert st == 0, (what, st)
            _assert_same(got, coded, streams, what)
        codec.close()


@pytest.mark.parametrize("fam", [f for f in sc.FAMILIES if f.cached], ids=repr)
def test_unified_and_split_caches_refuse_segment_lists(fam, sources):
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    few = streams[:4]
    tin = _input_tensors(torch, few)
    tcoded = _coded_tensors(torch, coded[:4])
    for what, setup in (("unified", lambda c: c.set_geometry(cache_rows=32)), ("split", lambda c: c.set_split_cache(32, 64))):
        codec = _codec(da, fam, g, tin["longest"])
        setup(codec)
        with pytest.raises(da.DivansGpuError, match="segment lists need"):
            _encode(torch, codec, tin)
        if 1 in da.decoder_generations():        # these are the first generation's caches: a build that offers it decodes with it from here on
            with pytest.raises(da.DivansGpuError, match="segment lists need"):
                _decode(torch, codec, tin, tcoded)
        else:                                    # the second generation has its own caches and serves the list
            st, back, name = _decode(torch, codec, tin, tcoded)
            assert st == 0 and "lit_decode2_kernel" in name, (what, st, name)
            _assert_decoded(back, tin, few, what)
        codec.close()


def _decoder_chains(da, fam):
    """one codec per chain, its settings applied one after the other: [(label, setup(codec), generation the kernel name must show)]"""
    tiny = ((8, 8, 0, 0), (5, 5, 5, 5)) if fam.cached else (None, None)      # (no row cache exists above 32 766 rows per stream)
    chains = []
    for gen in (2, 3):
        if gen in da.decoder_generations():
            chain = [("default", lambda c: None, 2)] if not chains else []
            chain.append((f"generation {gen}", lambda c, gen=gen: c.set_decoder(gen), 2))
            chain.append((f"generation {gen}, tiny caches, 2 workgroups", lambda c, gen=gen: c.set_decoder(gen, tiny[0], tiny[1], blocks=2), 2))
            chain.append((f"generation {gen}, tiny caches, 1 workgroup", lambda c, gen=gen: c.set_decoder(gen, tiny[0], tiny[1], blocks=1), 2))
            chains.append(chain)
    if 1 in da.decoder_generations():
        chains.append([("generation 1", lambda c: c.set_decoder(1), 1),
                       ("generation 1, no cache, 1 workgroup", lambda c: c.set_geometry(blocks=1, cache_rows=0), 1)])
    return chains


def _assert_kernel(fam, what, gen, name):
    mm = fam.mm if fam.mm >= 0 else -1
    if gen == 2:        # lit_decode2_kernel_*<MM, CTXC, MIX, SEG, caches>
        assert "lit_decode2_kernel" in name and f"<{mm}, {_b(fam.ctxc)}, {_b(fam.mix)}, true, " in name, (what, name)
        assert name.endswith(", 0>") == (not fam.cached), (what, name)
    else:               # lit_decode_kernel<MM, CTXC, MIX, cache, SEG>
        cache = 2 if fam.cached and "no cache" not in what else 0
        assert f"lit_decode_kernel<{mm}, {_b(fam.ctxc)}, {_b(fam.mix)}, {cache}, true>" in name, (what, name)


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_decode_oracle_bytes_on_every_generation(fam, sources):
    import torch
    import divans_amd as da
    g, o, streams, coded = _case(fam, sources)
    tin = _input_tensors(torch, streams)
    tcoded = _coded_tensors(torch, coded)
    for chain in _decoder_chains(da, fam):
        codec = _codec(da, fam, g, tin["longest"])
        for what, setup, gen in chain:
            setup(codec)
            st, back, name = _decode(torch, codec, tin, tcoded)
            assert st == 0, (what, st, name)
            _assert_kernel(fam, what, gen, name)
            _assert_decoded(back, tin, streams, what)
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
    tcoded = _coded_tensors(torch, coded[:len(bad)])      # (the bad streams: what the oracle wrote under the list that does add up)
    tins = [_input_tensors(torch, batch) for _, batch, _ in batches]
    longest = max(t["longest"] for t in tins)
    codec = _codec(da, fam, g, longest)
    codec.set_geometry(blocks=2)      # 12 streams: two workgroups hold them all (and the codec then asks for tables of 32 streams, not of a full grid)
    for (what, batch, skip), tin in zip(batches, tins):
        st, got = _encode(torch, codec, tin)
        assert st & BAD_SEGMENT, (what, "encode", st)
        _assert_same(got, coded, batch, what, skip=skip)
    st, got = _encode(torch, codec, _input_tensors(torch, good))      # ... and the same streams with their lists in order are clean
    assert st == 0
    codec.close()
    for chain in _decoder_chains(da, fam):
        codec = _codec(da, fam, g, longest)
        codec.set_geometry(blocks=2)
        for k, (label, setup, gen) in enumerate(chain):
            setup(codec)
            for (what, batch, skip), tin in zip(batches, tins):
                if k and len(skip) == 1:      # each kind by itself: once per generation, the batch of all three on every launch shape
                    continue
                st, back, name = _decode(torch, codec, tin, tcoded)
                assert st & BAD_SEGMENT, (what, label, st, name)
                _assert_kernel(fam, label, gen, name)
                offs = tin["off"].cpu().numpy()
                for i, (nm, lit, segs) in enumerate(batch):
                    if i not in skip:
                        assert (back[int(offs[i]):int(offs[i]) + lit.size] == lit).all(), (what, label, i, nm)
            if k == 0:      # ... and the same streams with their lists in order are clean
                st, back, name = _decode(torch, codec, _input_tensors(torch, good), tcoded)
                assert st == 0, (label, st, name)
        codec.close()


WRAP_CASES = [("mm4_map_plain", (0x3000, 0x1000)), ("mmx_map_plain", (8180, 64)), ("mm4_const_plain", (0x7800, 0x7800))]


@pytest.mark.parametrize("name,speed", WRAP_CASES, ids=[w[0] for w in WRAP_CASES])
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
    tin = _input_tensors(torch, streams)
    tcoded = _coded_tensors(torch, coded)
    mm = fam.mm if fam.mm >= 0 else -1
    for what, setup in (("default", lambda c: None), ("1 workgroup", lambda c: c.set_geometry(blocks=1))):
        codec = _codec(da, fam, g, tin["longest"])
        setup(codec)
        st, got = _encode(torch, codec, tin)
        assert st == 0, (what, st)
        _assert_same(got, coded, streams, what)
        st, back, kname = _decode(torch, codec, tin, tcoded)
        codec.close()
        assert st == 0, (what, st, kname)
        assert f"lit_decode_kernel<{mm}, {_b(fam.ctxc)}, {_b(fam.mix)}, 0, true>" in kname, kname
        _assert_decoded(back, tin, streams, what)
