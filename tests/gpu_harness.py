"""What the GPU test families share: uploading a batch, calling an entry point, comparing what came back with the C oracle.  One copy of
each helper; a test module imports this module and the `*_cases.py` modules, never another test module.  Nothing here is a test, so
pytest does not rewrite the asserts: every assert carries its own message (the call, the stream's index, its name where it has one).
torch, divans_amd and the oracle are imported inside the functions that need them, so the CPU tier can import the module."""
import numpy as np

import bucketed_segment_cases as bc
import command_cases as cc
import history_cases as hc
import segment_cases as sc

BAD_SEGMENT = 4
OUT_SENTINEL, SIZE_SENTINEL = 0x3C, 0x5A5A5A5A        # the fill of the encoders' output slots and of d_lit_sizes


# ---- device plumbing --------------------------------------------------------------------------------------------------------------
def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def to_device(torch, arrays):
    """the numpy arrays of a layout -> device tensors under the same keys (what is not an array is left out)"""
    dev = torch.device("cuda")
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items() if isinstance(v, np.ndarray)}


def max_stream_len(longest, even=False):
    """the length a test's codec is created for.  even: the codec keeps an even max_stream_len, and alloc_encode_outputs sizes the
    slots for the length it was given"""
    return max(longest, 16) + (longest % 2 if even else 0)


def codec_for(da, fam, g, longest, even=False):
    codec = da.LiteralCodec(g, max_stream_len(longest, even))
    codec.set_block_types(fam.n_btypes)
    return codec


def encode_paths(codec, da):
    """the encode paths to run: the streaming kernels, and the bucketed passes where the codec has them"""
    paths = [1]
    try:
        codec.set_encode_path(2)
        paths.append(2)
    except da.DivansGpuError:
        pass
    return paths


def tf(v):
    """a bool as a kernel name spells it"""
    return "true" if v else "false"


def implementations():
    """the device's restatements of the CDF arithmetic this build can run a script on (include/divans_gpu.h,
    divans_gpu_selftest_cdf_ops_on): generation 1, lit_decode2.hip, the bucketed encoder passes, and in experiment builds
    lit_decode_t.hip"""
    import divans_amd as da
    return [0, 1, 2] + ([3] if da.experimental_decoders() else [])


# ---- the oracle and the inputs ----------------------------------------------------------------------------------------------------
def oracle_bytes(ocfg, streams):
    """the C oracle's coded bytes of every stream under its segment list; a stream is (name, lit, segs) or a dict with `lit` and `segs`"""
    import pyoracle as po
    pairs = [(s["lit"], s["segs"]) if isinstance(s, dict) else (s[1], s[2]) for s in streams]
    return [po.lit_segments_encode(ocfg, lit, segs["len"], segs["btype"], segs["last8"]) for lit, segs in pairs]


def as_tuples(streams):
    """dict-shaped streams (command lists) as the (name, lit, segs) the segment entry points' helpers take"""
    return [(s["name"], s["lit"], s["segs"]) for s in streams]


def ir_stream(ir, name):
    cmds, ins = ir.device_commands()
    lit, segs = ir.literal_segments()
    return dict(name=name, cmds=cmds, lit=lit, ins=ins, raw=ir.expand(), segs=segs)


def ir_streams(ir, count):
    """`count` streams cut from the IR's command list as test_gpu_general_streams.test_many_general_streams_in_one_batch cuts them:
    stream k = the literals of commands [a, b), with the Copy / Dict boundaries and block types of the file"""
    lit, segs = ir.literal_segments()
    ends = np.cumsum(segs["len"].astype(np.int64))
    span = min(390, max(2, segs.size // 2))
    streams = []
    for k in range(count):
        a = (k * 149) % (segs.size - span); b = a + 1 + (k * 37) % span
        lo = int(ends[a - 1]) if a else 0
        hi = int(ends[b - 1])
        while hi - lo > 65536:      # (a file of few, long Literal commands)
            b -= 1; hi = int(ends[b - 1])
        if b > a:
            streams.append((f"{a}:{b}", lit[lo:hi].copy(), segs[a:b].copy()))
    return streams


def _segment_arrays(streams):
    segs = np.concatenate([s[2] for s in streams] + [np.zeros(1, sc.SEG_DTYPE)])      # (one spare record: the array is never empty)
    seg_begin = np.concatenate([[0], np.cumsum([s[2].size for s in streams])]).astype(np.int32)
    return seg_begin, segs.view(np.uint8)


def ragged_tensors(torch, streams):
    """streams: [(name, lit uint8[n], segs)] in the ragged layout of bucketed_segment_cases.layout -> device tensors of the segment
    entry points (`offs`, `sizes`: the layout on the host)"""
    buf, offs, sizes = bc.layout(streams)
    seg_begin, segs = _segment_arrays(streams)
    t = to_device(torch, dict(lit=buf, off=offs, sz=sizes, sb=seg_begin, segs=segs))
    return dict(t, longest=int(sizes.max()), n=len(streams), offs=offs, sizes=sizes)


def input_tensors(torch, streams):
    """streams: [(name, lit uint8[n], segs)] back to back, 64 zero bytes behind -> device tensors of the segment entry points"""
    sizes = np.array([s[1].size for s in streams], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes[:-1].astype(np.int64))]).astype(np.int64)
    seg_begin, segs = _segment_arrays(streams)
    lit = np.concatenate([s[1] for s in streams] + [np.zeros(64, np.uint8)])
    t = to_device(torch, dict(lit=lit, off=offs, sz=sizes, sb=seg_begin, segs=segs))
    return dict(t, longest=int(sizes.max()), n=len(streams), total=int(sizes.sum()))


def coded_tensors(torch, coded):
    """the oracle's streams side by side, each at a 16-byte boundary -> (bytes, offsets, sizes) on the device"""
    sizes = np.array([c.size for c in coded], dtype=np.int32)
    assert (sizes % 4 == 0).all(), f"coded_tensors: coded sizes that are no whole words: {sizes[sizes % 4 != 0].tolist()}"
    offs = np.concatenate([[0], np.cumsum((sizes[:-1].astype(np.int64) + 15) & ~15)]).astype(np.int64)
    buf = np.zeros(int(offs[-1]) + int(sizes[-1]) + 64, np.uint8)
    for o, c in zip(offs, coded):
        buf[int(o):int(o) + c.size] = c
    t = to_device(torch, dict(buf=buf, offs=offs, sizes=sizes))
    return t["buf"], t["offs"], t["sizes"]


def encode_layout(lay):
    """a command_cases.layout with the raw bytes in place (what a compressor hands over): `raw` = `expect`"""
    lay = dict(lay)
    lay["raw"] = lay["expect"].copy()
    return lay


def history_batch(fam, o, streams, mode="own"):
    """(streams, the oracle's bytes, the batch's layout with the coded bytes in place, the histories' layout)"""
    coded = oracle_bytes(o, streams)
    return streams, coded, cc.layout(streams, coded), hc.history_layout(streams, mode, hc.dictionary_of(fam))


def plain_device(torch, case):
    """a list-free decoder case (plain_decoder_cases: `lit` = literal_layout, `cod` = coded_layout) on the device"""
    buf, blank, offs, sizes = case["lit"]
    cbuf, coffs, csizes = case["cod"]
    t = to_device(torch, dict(lit=buf, blank=blank, off=offs, sz=sizes, coded=cbuf, coff=coffs, csz=csizes))
    return dict(t, n=len(sizes), longest=int(sizes.max()))


# ---- the calls --------------------------------------------------------------------------------------------------------------------
def split_outputs(outs, n):
    """[coded bytes of stream i] as the encoders' `offsets` and `sizes` describe them in `out`"""
    out, offs, sz = _host(outs["out"]), _host(outs["offsets"]), _host(outs["sizes"])
    return [out[int(offs[i]):int(offs[i]) + int(sz[i])] for i in range(n)]


def encode_segments(codec, tin, outs=None, fit=False):
    """encode_segments_batch -> (status, [coded bytes of stream i], the pass that ran).  outs: the caller's slots; without them fresh
    ones, sized for the codec's max_stream_len or (fit) for this batch's longest stream"""
    outs = outs or (codec.alloc_encode_outputs(tin["n"], max(tin["longest"], 16)) if fit else codec.alloc_encode_outputs(tin["n"]))
    codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], tin["n"], tin["longest"], tin["sb"], tin["segs"], outs)
    st = codec.status()
    return st, split_outputs(outs, tin["n"]), codec.last_encode_path()


def decode_segments(torch, codec, tin, tcoded):
    """decode_segments_batch of tcoded = (bytes, offsets, sizes) -> (status, decoded bytes of the whole batch, name of the kernel that ran)"""
    back = torch.zeros_like(tin["lit"])
    codec.decode_segments_batch(tcoded[0], tcoded[1], tcoded[2], tin["n"], tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"])
    st = codec.status()
    return st, back.cpu().numpy(), codec.last_decode_kernel()


def assert_round_trip_segments(torch, codec, tin, outs, streams, what):
    """the codec's own coded bytes (the `outs` of an encode call) through decode_segments_batch: status 0, every stream as it went in"""
    st, back, name = decode_segments(torch, codec, tin, (outs["out"], outs["offsets"], outs["sizes"]))
    assert st == 0, f"{what}: decode_segments_batch of the codec's own bytes: status {st} ({name})"
    assert_decoded(back, tin, streams, what)


def decode_plain(codec, dv):
    """decode_batch of a plain_device case -> (status, the whole output buffer, name of the kernel that ran)"""
    back = dv["blank"].clone()
    codec.decode_batch(dv["coded"], dv["coff"], dv["csz"], dv["n"], dv["longest"], back, out_offsets=dv["off"], out_sizes=dv["sz"])
    st = codec.status()
    return st, back.cpu().numpy(), codec.last_decode_kernel()


def hist_args(ht):
    return dict(hist=ht["hist"], hist_offsets=ht["hist_off"], hist_sizes=ht["hist_sz"])


def _insert_args(t, with_ins):
    return (t["ins"], t["ins_off"], t["ins_sz"]) if with_ins else (None, None, None)


def decode_commands(torch, codec, lay, t, hlay=None, ht=None, with_ins=True):
    """decode_commands_batch, with the history ht (layout hlay) where one is given -> (status, the whole raw buffer, stream flags, name
    of the kernel that ran); asserts that the history buffer is untouched"""
    raw = t["raw"].clone()
    flags = torch.zeros(lay["n"] + 16, dtype=torch.uint8, device=raw.device)
    codec.set_stream_flags(flags)
    try:
        codec.decode_commands_batch(t["coded"], t["coded_off"], t["coded_sz"], lay["n"], t["cmd_begin"], t["cmds"], t["lit_sz"], lay["lit_longest"],
                                    raw, t["raw_off"], t["raw_sz"], *_insert_args(t, with_ins), **(hist_args(ht) if ht else {}))
        st = codec.status()
    finally:
        codec.set_stream_flags(None)
    if ht:
        assert (ht["hist"].cpu().numpy() == hlay["hist"]).all(), "decode_commands_batch wrote to the history buffer"
    return st, raw.cpu().numpy(), flags.cpu().numpy(), codec.last_decode_kernel()


def encode_outputs(codec, n):
    """slots of divans_gpu_lit_encode_bound(the codec's max_stream_len), pre-filled with the sentinels"""
    outs = codec.alloc_encode_outputs(n)
    outs["out"].fill_(OUT_SENTINEL); outs["offsets"].fill_(-1); outs["sizes"].fill_(-1)
    return outs


def encode_commands(torch, codec, lay, t, hlay=None, ht=None, n=None, with_ins=True, lit_cap=None, outs=None, hist_is_raw=False):
    """encode_commands_batch, with the history ht (layout hlay) where one is given -> dict(status, coded = [bytes of stream i], lit_sz,
    flags, out = the whole slot buffer, spans = [(begin, end) of stream i in it], slot) and asserts that the call left its inputs and
    everything behind its outputs alone.  hist_is_raw: the history pointer is the raw buffer itself (ht holds the offsets and sizes only)."""
    n = lay["n"] if n is None else n
    cap = lay["lit_longest"] if lit_cap is None else lit_cap
    outs = outs or encode_outputs(codec, n)
    lit_sz = torch.full((n + 16,), SIZE_SENTINEL, dtype=torch.int32, device=t["raw"].device)
    flags = torch.zeros(n + 16, dtype=torch.uint8, device=t["raw"].device)
    hist = {} if not ht else dict(hist=t["raw"], hist_offsets=ht["hist_off"], hist_sizes=ht["hist_sz"]) if hist_is_raw else hist_args(ht)
    codec.set_stream_flags(flags)
    try:
        codec.encode_commands_batch(t["raw"], t["raw_off"], t["raw_sz"], n, t["cmd_begin"], t["cmds"], cap, outs, lit_sz, *_insert_args(t, with_ins), **hist)
        st = codec.status()
    finally:
        codec.set_stream_flags(None)
    out = outs["out"].cpu().numpy(); offs = outs["offsets"].cpu().numpy(); sz = outs["sizes"].cpu().numpy()
    for k in ("raw", "cmds", "cmd_begin", "ins", "raw_off", "raw_sz", "ins_off", "ins_sz"):
        assert (t[k].cpu().numpy() == np.ascontiguousarray(lay[k])).all(), f"encode_commands_batch wrote to its input `{k}`"
    for k in (("hist_off", "hist_sz") + (() if hist_is_raw else ("hist",))) if ht else ():
        assert (ht[k].cpu().numpy() == hlay[k]).all(), f"encode_commands_batch wrote to its input `{k}`"
    lit_sz = lit_sz.cpu().numpy(); flags = flags.cpu().numpy()
    assert (lit_sz[n:] == SIZE_SENTINEL).all() and not flags[n:].any() and (out[n * outs["slot"]:] == OUT_SENTINEL).all(), \
        "encode_commands_batch: bytes written behind the outputs"
    spans = [(int(offs[i]), int(offs[i]) + int(sz[i])) for i in range(n)]
    for i, (b, e) in enumerate(spans):
        assert i * outs["slot"] <= b <= e <= (i + 1) * outs["slot"], f"encode_commands_batch: stream {i} lies outside its slot: {b}..{e}"
    return dict(status=st, coded=[out[b:e] for b, e in spans], lit_sz=lit_sz[:n], flags=flags[:n], out=out, spans=spans, slot=outs["slot"])


def round_trip_commands(torch, codec, streams, res, lay, what, hlay=None, ht=None):
    """the contract: the GPU's coded bytes (re-laid at 4-byte offsets) and its d_lit_sizes, with the same lists and history, decode to the raw bytes"""
    back = cc.layout(streams, [c.copy() for c in res["coded"]], lit_sizes=res["lit_sz"].tolist())
    assert (back["expect"] == lay["expect"]).all(), f"{what}, round trip: the re-laid batch expects other raw bytes"
    st, raw, flags, name = decode_commands(torch, codec, back, to_device(torch, back), hlay, ht)
    assert st == 0 and not flags.any(), f"{what}, round trip: status {st}, flagged streams {np.flatnonzero(flags).tolist()} ({name})"
    assert_raw(raw, back, streams, what + ", round trip")


# ---- the assertions ---------------------------------------------------------------------------------------------------------------
def assert_same(got, ref, streams, what, skip=()):
    """coded streams against the expected ones (the oracle's, in most callers); streams: the batch's (name, lit, segs), or None where
    the streams have no names (then `ref` holds exactly the batch)"""
    assert len(got) == (len(ref) if streams is None else len(streams)) and len(ref) >= len(got), f"{what}: {len(got)} streams against {len(ref)} expected"
    for i, (g, r) in enumerate(zip(got, ref)):
        if i in skip:
            continue
        who = "" if streams is None else f"{streams[i][0]}, {streams[i][1].size} bytes, {streams[i][2].size} segments, "
        assert g.size == r.size and (g == r).all(), f"{what}: stream {i} ({who}{g.size} bytes against {r.size}) differs from the expected bytes"


def assert_coded(res, streams, coded, what, skip=()):
    """the result of encode_commands: coded bytes and literal sizes against the oracle and the streams"""
    for i, (got, ref) in enumerate(zip(res["coded"], coded)):
        if i in skip:
            continue
        s = streams[i]
        who = f"{s['name']}, {s['cmds'].size} commands" + (f", {s['hist'].size} history bytes" if "hist" in s else "")
        assert got.size == ref.size and (got == ref).all(), f"{what}: stream {i} ({who}) differs from the oracle"
        assert int(res["lit_sz"][i]) == s["lit"].size, f"{what}: stream {i} ({who}): literal size {int(res['lit_sz'][i])}, the stream has {s['lit'].size}"


def assert_raw(got, lay, streams, what, skip=()):
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
        hist = f", {streams[i]['hist'].size} history bytes" if "hist" in streams[i] else ""
        raise AssertionError(f"{what}: stream {i} ({streams[i]['name']}, {int(lay['raw_sz'][i])} raw bytes{hist}) wrong from its byte {at - int(lay['raw_off'][i])}")
    raise AssertionError(f"{what}: sentinel byte {at} of the raw buffer overwritten with {int(got[at])}")


def assert_decoded(back, tin, streams, what, skip=()):
    """the output of decode_segments against the streams; where the layout has a `total` (input_tensors) nothing lies behind it"""
    offs = _host(tin["off"])
    for i, (name, lit, segs) in enumerate(streams):
        if i in skip:
            continue
        got = back[int(offs[i]):int(offs[i]) + lit.size]
        assert (got == lit).all(), f"{what}: stream {i} ({name}, {lit.size} bytes, {segs.size} segments) decoded wrong from byte {int(np.argmax(got != lit))}"
    if "total" in tin:
        assert not back[tin["total"]:].any(), f"{what}: bytes written behind the batch"


def assert_plain_decoded(back, case, what):
    """the output of decode_plain against the case's streams, and every sentinel byte between and behind them"""
    buf, _, offs, _ = case["lit"]
    for i, ((name, lit), off) in enumerate(zip(case["streams"], offs)):
        got = back[int(off):int(off) + lit.size]
        assert (got == lit).all(), f"{what}: stream {i} ({name}, {lit.size} bytes, {case['coded'][i].size // 4} coded words) decoded wrong from byte {int(np.argmax(got != lit))}"
    wrong = np.flatnonzero(back != buf)
    assert wrong.size == 0, f"{what}: sentinel byte {int(wrong[0]) if wrong.size else -1} of {buf.size} written to"


def decoder_chains(da, fam):
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


def assert_segment_kernel(fam, what, gen, name):
    """the fused SEG = true instance of the family, by decoder generation"""
    mm = fam.mm if fam.mm >= 0 else -1
    if gen == 2:        # lit_decode2_kernel_*<MM, CTXC, MIX, SEG, caches>
        assert "lit_decode2_kernel" in name and f"<{mm}, {tf(fam.ctxc)}, {tf(fam.mix)}, true, " in name, f"{what}: {name} is not the family's lit_decode2_kernel instance"
        assert name.endswith(", 0>") == (not fam.cached), f"{what}: {name}: row caches {'expected' if fam.cached else 'not expected'}"
    else:               # lit_decode_kernel<MM, CTXC, MIX, cache, SEG>
        cache = 2 if fam.cached and "no cache" not in what else 0
        assert f"lit_decode_kernel<{mm}, {tf(fam.ctxc)}, {tf(fam.mix)}, {cache}, true>" in name, f"{what}: {name} is not the family's lit_decode_kernel instance"


def assert_command_kernel(fam, name, what):
    """lit_decode2_cmd_kernel<MM, CTXC, MIX, caches>: the high-row caches in the 2-way organisation (1 | 16, with mixing 1 | 2 | 16), or none"""
    mm = fam.mm if fam.mm >= 0 else -1
    caches = (19 if fam.mix else 17) if fam.cached else 0
    want = f"divans_hip::lit_decode2_cmd_kernel<{mm}, {tf(fam.ctxc)}, {tf(fam.mix)}, {caches}>"
    assert name == want, f"{what}: {name} ran, not {want}"
