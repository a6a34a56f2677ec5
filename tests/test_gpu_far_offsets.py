"""Every batch entry point with data placed beyond 4 GiB (tests/far_offset_cases.py has the design; tests/test_far_offset_cases_cpu.py
proves on a numpy model that a truncated or sign-extended offset would be seen here).

A  the encoders: far in_offsets, out_slot = 2^30 + 16 with eight streams (the slots end above 2^31 and 2^32)
B  the decoders: far coded input, far raw output (an odd offset among them), row_replay, the learned byte order
C  the codec's own work arrays past 2^32: 32 840 ragged streams on a codec created for 65 536-byte streams (simple, mixing and a
   context-keyed family; NOT a stride family -- an open fault at this shape, DESIGN.md section 4, "Offsets beyond 4 GiB")
D  the pack pass with a total above 2^32
E  the uniform layout (no offset arrays): 65 584 streams of 65 536 bytes, stream * stream_len passes 2^32

A wrong address must show as wrong bytes, never as a fault: every far buffer is an allocation with FRONT bytes in front of the view
the library is handed, at every alias of a far input lies a decoy, and every far output is searched for bytes that are not the sentinel
outside the expected windows.  Every call is compared with the C oracle and with the same call at offsets under 1 MiB.

The kernels and passes that ran are printed (pytest -rP shows them): last_decode_kernel() and last_encode_path()."""
import numpy as np
import pytest

import bucketed_segment_cases as bc
import command_cases as cc
import ctx_bucketed_cases as cx
import encode_dispatch_cases as ed
import far_offset_cases as fo
import gpu_harness as gh
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
G31, G32 = fo.G31, fo.G32
# Device memory a test needs free, or it skips with the reason.  Parts A and B hold the far buffers: two of 8 GiB, or one and the
# encoders' slots of 10 GiB; encode_commands_batch alone takes three far arguments (raw bytes, insert bytes, slots: 26 GiB).
NEED = 27 << 30
# Part C: the codec's own arrays at 32 840 streams of 65 536-byte slots -- bucketed work arrays (24 GiB one model, 60 GiB two), the
# streaming kernels' pairs and model_batch's (17 GiB each), three sets of output slots (8 GiB each), the tables and a candidate.
NEED_WORK = {"simple": 90 << 30, "mixing": 130 << 30, "context_keyed": 110 << 30}
# Part E: input, output and packed bytes (4.3 GiB each), the slots of a sub-batch of 32 768 streams (8 GiB), its work arrays, the tables.
NEED_UNIFORM = {"simple": 50 << 30, "mixing": 90 << 30}
INPUT_FILL = 0x5A
EMPTY = np.zeros(0, np.uint8)
_POOL = {}


class Far:
    """an allocation `a` and the view `r` = a[FRONT:] the library is handed"""

    def __init__(self, torch, total, fill):
        self.torch, self.fill = torch, fill
        self.a = torch.full((total,), fill, dtype=torch.uint8, device="cuda")
        self.r = self.a[fo.FRONT:]
        self.dirty = []

    def put(self, pieces):
        """the buffer holds `pieces` [(offset in the allocation, bytes)] and the fill everywhere else"""
        self.wipe()
        for at, data in pieces:
            self.a[at:at + data.size] = self.torch.from_numpy(np.ascontiguousarray(data)).cuda()
            self.dirty.append((at, data.size))

    def wipe(self, windows=None):
        for at, n in self.dirty if windows is None else windows:
            self.a[at:at + n] = self.fill
        if windows is None:
            self.dirty = []

    def get(self, o, n):
        """n bytes at offset o of R"""
        return self.a[fo.FRONT + o:fo.FRONT + o + n].cpu().numpy()

    def foreign(self, windows):
        """how many pieces outside `windows` [(offset in the allocation, size)] hold something else than the fill: looked at in chunks
        of at most SCAN_CHUNK bytes, eight bytes at a time where a piece allows it"""
        t = self.torch
        word = int.from_bytes(bytes([self.fill]) * 8, "little", signed=True)
        bad = t.zeros((), dtype=t.int64, device=self.a.device)
        for a, b in fo.outside(windows, self.a.numel()):
            lo, hi = -(-a // 8) * 8, b // 8 * 8
            if hi - lo < 64:
                bad += (self.a[a:b] != self.fill).sum()
                continue
            if a < lo:
                bad += (self.a[a:lo] != self.fill).sum()
            if hi < b:
                bad += (self.a[hi:b] != self.fill).sum()
            for c in range(lo, hi, fo.SCAN_CHUNK):
                bad += (self.a[c:min(c + fo.SCAN_CHUNK, hi)].view(t.int64) != word).sum()
        return int(bad.item())

    def untouched_outside(self, windows, what):
        """asserts the sentinel scan, and leaves the buffer filled again whatever it found"""
        n = self.foreign(windows)
        if n:
            self.a.fill_(self.fill)
        else:
            self.wipe(windows)
        assert n == 0, f"{what}: {n} pieces outside the expected windows were written to"


def _drop(*names):
    import torch
    for name in names or list(_POOL):
        _POOL.pop(name, None)
    torch.cuda.empty_cache()


def _far(name):
    """the module's far buffers, made when first asked for: "in" / "in2" inputs, "out" raw output, "slots" the encoders' output"""
    import torch
    if name not in _POOL:
        size = fo.SLOT_ALLOC if name == "slots" else fo.ALLOC
        _POOL[name] = Far(torch, size, INPUT_FILL if name.startswith("in") else fo.SENTINEL)
    return _POOL[name]


@pytest.fixture(scope="module", autouse=True)
def memory():
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip(f"the far buffers need {NEED >> 30} GiB of device memory, {free >> 30} GiB are free")
    yield
    _drop()


@pytest.fixture(scope="module")
def pair(corpus):
    return fo.streams(corpus)


def _d(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _image(lay, real, decoy):
    return fo.image(lay, real, decoy)


def _two_segments(streams, btype, seed):
    """a two-segment list per stream, the second under a context that is not the natural one"""
    rng = np.random.default_rng(seed)
    out = []
    for lit in streams:
        cut = lit.size // 2
        out.append(sc.segments([cut, lit.size - cut], [btype, btype], rng.integers(0, 1 << 64, size=2, dtype=np.uint64)))
    return out


def _seg_tensors(lists):
    segs = np.concatenate(list(lists) + [np.zeros(1, sc.SEG_DTYPE)])
    begin = np.concatenate([[0], np.cumsum([s.size for s in lists])]).astype(np.int32)
    return _d(begin), _d(segs.view(np.uint8))


def _oracle_segments(o, streams, lists):
    return [po.lit_segments_encode(o, lit, s["len"], s["btype"], s["last8"]) if lit.size else EMPTY for lit, s in zip(streams, lists)]


def _oracle(o, streams):
    return [po.lit_encode(o, s) if s.size else EMPTY for s in streams]


# ---- A: the encoders -------------------------------------------------------------------------------------------------------------

def _slot_outputs(torch, slots):
    return dict(slot=fo.OUT_SLOT, out=slots.r, offsets=torch.full((8,), -1, dtype=torch.int64, device="cuda"),
                sizes=torch.full((8,), -1, dtype=torch.int32, device="cuda"))


def _read_slots(slots, outs, want, what):
    """the far slots after an encode call: sizes, right-aligned offsets, the sentinel scan, the coded bytes"""
    sizes = [w.size for w in want]
    offs = fo.slot_offsets(sizes)
    windows = [(fo.FRONT + o, s) for o, s in zip(offs, sizes) if s]
    got_sz, got_off = outs["sizes"].cpu().tolist(), outs["offsets"].cpu().tolist()
    if got_sz != sizes or got_off != offs:
        slots.a.fill_(slots.fill)
    assert got_sz == sizes, (what, got_sz, sizes)
    assert got_off == offs, (what, "d_out_offsets: not right-aligned in the far slots", got_off, offs)
    got = [slots.get(o, s) for o, s in zip(offs, sizes)]
    slots.untouched_outside(windows, what)
    gh.assert_same(got, want, None, what)
    return got


ENCODE_ROWS = [k for k, r in ed.TABLE.items() if r.accepted and not r.wrap and not r.path_2_before_types]


@pytest.mark.parametrize("key", ENCODE_ROWS)
def test_encoders_read_far_input_and_write_far_slots(key, pair):
    """encode_batch, encode_batch_chunks and encode_segments_batch on a row of encode_dispatch_cases.TABLE, under the streaming
    kernels and the row's bucketed pass, on a codec for short streams (one rANS lane per stream) and on one above 32 768 bytes (one
    lane per chunk, two lanes per chunk, the stitch)"""
    import torch
    import divans_amd as da
    assert ENCODE_ROWS == ["stride_1", "stride_3", "two_model", "context_keyed", "context_keyed_two_model", "two_model_block_types", "two_model_as_created"]
    row = ed.TABLE[key]
    g, o = row.family.pair(da, po)
    real, decoy = pair
    lists = _two_segments(real, row.family.btype, 97100)
    want = {"batch": _oracle(o, real), "chunks": _oracle(o, real), "segments": _oracle_segments(o, real, lists)}
    sb, segs = _seg_tensors(lists)
    sizes = _d(fo.LENGTHS, np.int32)
    lays = fo.layouts(fo.LENGTHS, 1)
    near = fo.near_layout(fo.LENGTHS, 1)
    src, slots = _far("in"), _far("slots")
    longest = max(fo.LENGTHS)
    ran = set()
    for msl, splits in ((8192, (0,)), (40000, (1, 2))):
        assert fo.OUT_SLOT % 16 == 0 and fo.OUT_SLOT >= da.encode_bound(msl)
        codec = da.LiteralCodec(g, msl)
        if row.types is not None:
            codec.set_block_types(row.types)
        chunks = torch.zeros((8, 2), dtype=torch.int32, device="cuda")

        def call(entry, outs, offs):
            if entry == "segments":
                codec.encode_segments_batch(src.r, offs, sizes, 8, longest, sb, segs, outs)
            else:
                chunks.zero_()
                codec.encode_batch(src.r, 8, longest, outs, in_offsets=offs, in_sizes=sizes, chunk_bytes=chunks if entry == "chunks" else None)
            return codec.status(), codec.last_encode_path()

        for path in (1, 2):
            codec.set_encode_path(path)
            expect_path = {"batch": row.ran[path][0], "chunks": row.ran[path][0], "segments": row.ran[path][1]}
            for entry in ("batch", "chunks", "segments"):
                for split in splits if entry != "segments" else splits[:1]:
                    codec.set_rans_split(split)
                    what = f"{key}, max_stream_len {msl}, path {path}, {entry}, rans split {split}"
                    src.put(_image(near, real, decoy))
                    nouts = codec.alloc_encode_outputs(8)
                    st, p = call(entry, nouts, _d(near.offsets, np.int64))
                    assert st == 0 and p == expect_path[entry], (what, "near", st, p)
                    control = gh.split_outputs(nouts, 8)
                    control_chunks = chunks.cpu().numpy().copy()
                    gh.assert_same(control, want[entry], None, what + ", near offsets")
                    for lay in lays:
                        src.put(_image(lay, real, decoy))
                        outs = _slot_outputs(torch, slots)
                        st, p = call(entry, outs, _d(lay.offsets, np.int64))
                        where = f"{what}, input at {sorted(lay.anchored)}"
                        assert st == 0 and p == expect_path[entry], (where, st, p)
                        got = _read_slots(slots, outs, want[entry], where)
                        gh.assert_same(got, control, None, where + " against the near call")
                        if entry == "chunks":
                            assert (chunks.cpu().numpy() == control_chunks).all() and (control_chunks.sum(axis=1) == [w.size for w in want[entry]]).all(), where
                    ran.add((msl, path, entry, p, split))
        codec.close()
    print(key, "ran (max_stream_len, path asked, entry, pass, rans split):", sorted(ran))


@pytest.mark.parametrize("cfg_name", ["simple", "mixing"])
def test_model_batch_and_encode_packed_read_far_input(cfg_name, pair):
    import torch
    import divans_amd as da
    real, decoy = pair
    g = getattr(da, "config_" + ("simple" if cfg_name == "simple" else "context_mixing"))()
    o = getattr(po, "config_" + ("simple" if cfg_name == "simple" else "context_mixing"))()
    want = _oracle(o, real)
    traces = []
    for s in real:
        _, tr = po.lit_encode(o, s, trace=True) if s.size else (None, np.zeros((0, 3), np.int16))
        traces.append(tr[:, 1].astype(np.uint32) | (tr[:, 2].astype(np.uint32) << 16))
    sizes = _d(fo.LENGTHS, np.int32)
    src = _far("in")
    longest = max(fo.LENGTHS)
    codec = da.LiteralCodec(g, longest)
    ref_off, ref_total = np.cumsum([0] + [w.size for w in want])[:-1], sum(w.size for w in want)
    assert all(w.size % 4 == 0 for w in want)
    ran = set()
    for path in (1, 2):
        codec.set_encode_path(path)
        for lay in [fo.near_layout(fo.LENGTHS, 1)] + fo.layouts(fo.LENGTHS, 1):
            what = f"{cfg_name}, path {path}, input at {sorted(lay.anchored) or 'near offsets'}"
            src.put(_image(lay, real, decoy))
            offs = _d(lay.offsets, np.int64)
            pairs = codec.model_batch(src.r, 8, longest, in_offsets=offs, in_sizes=sizes)
            assert codec.status() == 0, what
            ran.add(("model_batch", path, codec.last_encode_path()))
            pairs = pairs.cpu().numpy().view(np.uint32)
            for i, tr in enumerate(traces):
                assert (pairs[i, :tr.size] == tr).all(), f"{what}: the pairs of stream {i} differ from the oracle's trace"
            packed = torch.full((ref_total + 512,), fo.SENTINEL, dtype=torch.uint8, device="cuda")
            poff = torch.full((8,), -1, dtype=torch.int64, device="cuda"); psz = torch.full((8,), -1, dtype=torch.int32, device="cuda")
            total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            codec.encode_packed(src.r, 8, longest, packed, poff, psz, total, in_offsets=offs, in_sizes=sizes)
            assert codec.status() == 0, what
            ran.add(("encode_packed", path, codec.last_encode_path()))
            assert psz.cpu().tolist() == [w.size for w in want] and poff.cpu().tolist() == ref_off.tolist() and int(total.item()) == ref_total, what
            got = packed.cpu().numpy()
            gh.assert_same([got[a:a + w.size] for a, w in zip(ref_off, want)], want, None, what + ", encode_packed")
            assert (got[ref_total:] == fo.SENTINEL).all(), what
    codec.close()
    print(cfg_name, "ran (entry, path asked, pass):", sorted(ran))


def _command_streams(fam, sources):
    """eight general streams with Literal, Copy and Insert commands in each; raw and insert sizes suit the anchors (stream 0 is long
    enough to straddle 2^32 from seven bytes in front of it)"""
    rng = np.random.default_rng(97200 + fam.seed)
    data = sc._Data(sources, rng)
    out = []
    for k, n in enumerate((300, 47, 20, 16, 12, 4097, 700, 65)):
        s = cc.Stream(f"F{k}", fam, data, rng)
        a = max(4, n // 3)
        s.lit(a).copy(max(2, n // 5), 1 + k % min(a, 4)).ins(12 + k, 1 + k % 3).lit(max(3, n // 4)).copy(5, 3).ins(9, 2).lit(2 + k)
        out.append(s.done())
    assert all({cc.COPY, cc.INSERT, cc.LITERAL} <= set(s["cmds"]["kind"].tolist()) for s in out)
    return out


def _straddles(lays, sizes):
    at = {a: (lay.offsets[k], sizes[k]) for lay in lays for a, k in lay.anchored.items()}
    assert sorted(at) == sorted(fo.ANCHORS)
    for a, edge in (("straddles_2g", G31), ("straddles_4g", G32)):
        assert at[a][0] < edge < at[a][0] + at[a][1], a
    assert at["ends_at_4g"][0] + at["ends_at_4g"][1] == G32


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _xor(streams):
    return [s ^ np.uint8(0x15) for s in streams]


def _cmd_tensors(streams):
    cmds = np.concatenate([s["cmds"] for s in streams] + [np.zeros(1, cc.CMD_DTYPE)])
    begin = np.concatenate([[0], np.cumsum([s["cmds"].size for s in streams])]).astype(np.int32)
    return _d(begin), _d(cmds.view(np.uint8))


def test_encode_commands_batch_reads_far_raw_and_insert_bytes(sources):
    """raw_offsets, ins_offsets and out_slot far: the row "stride_1" of the dispatch table (eight block types), both encode paths"""
    import torch
    import divans_amd as da
    fam = bc.CONFIGS["A"]
    g, o = fam.pair(da, po)
    streams = _command_streams(fam, sources)
    raw, ins = [s["raw"] for s in streams], [s["ins"] for s in streams]
    want = _oracle_segments(o, [s["lit"] for s in streams], [s["segs"] for s in streams])
    raw_sz, ins_sz = [r.size for r in raw], [i.size for i in ins]
    raw_lays, ins_lays = fo.layouts(raw_sz, 1), fo.layouts(ins_sz, 1)
    _straddles(raw_lays, raw_sz); _straddles(ins_lays, ins_sz)
    cmd_begin, cmds = _cmd_tensors(streams)
    lit_cap = max(s["lit"].size for s in streams)
    _drop("out")
    src, src2, slots = _far("in"), _far("in2"), _far("slots")
    codec = da.LiteralCodec(g, max(lit_cap, 16))
    codec.set_block_types(fam.n_btypes)
    ran = set()
    for path in (1, 2):
        codec.set_encode_path(path)
        for j in range(max(len(raw_lays), len(ins_lays)) + 1):
            far = j > 0
            rl = raw_lays[(j - 1) % len(raw_lays)] if far else fo.near_layout(raw_sz, 1)
            il = ins_lays[(j - 1) % len(ins_lays)] if far else fo.near_layout(ins_sz, 1)
            what = f"path {path}, raw at {sorted(rl.anchored) or 'near offsets'}, insert bytes at {sorted(il.anchored) or 'near offsets'}"
            src.put(_image(rl, raw, _xor(raw))); src2.put(_image(il, ins, _xor(ins)))
            outs = _slot_outputs(torch, slots) if far else codec.alloc_encode_outputs(8)
            lit_sz = torch.full((8,), -1, dtype=torch.int32, device="cuda")
            codec.encode_commands_batch(src.r, _d(rl.offsets, np.int64), _d(raw_sz, np.int32), 8, cmd_begin, cmds, lit_cap, outs, lit_sz,
                                        src2.r, _d(il.offsets, np.int64), _d(ins_sz, np.int32))
            st, p = codec.status(), codec.last_encode_path()
            assert st == 0 and p == (1 if path == 1 else 2), (what, st, p)
            ran.add((path, p))
            assert lit_sz.cpu().tolist() == [s["lit"].size for s in streams], what
            if far:
                got = _read_slots(slots, outs, want, what)
                gh.assert_same(got, control, None, what + " against the near call")
            else:
                control = gh.split_outputs(outs, 8)
                gh.assert_same(control, want, None, what)
    codec.close()
    _drop("in2")
    print("encode_commands_batch ran (path asked, pass):", sorted(ran))


# ---- B: the decoders -------------------------------------------------------------------------------------------------------------

def _read_out(out, offsets, want, what):
    windows = [(fo.FRONT + o, w.size) for o, w in zip(offsets, want) if w.size]
    got = [out.get(o, w.size) for o, w in zip(offsets, want)]
    out.untouched_outside(windows, what)
    gh.assert_same(got, want, None, what)


def _paired(a, b):
    """the layouts of two buffers side by side: every layout of either is used"""
    return [(a[j % len(a)], b[j % len(b)]) for j in range(max(len(a), len(b)))]


def _decode_far(codec, call, coded, dcoded, want, what, kernels):
    """one decode entry point at near offsets and at every pair of far layouts: status, bytes against the expectation (the oracle's
    input), the sentinel scan.  call(coded R, coded offsets, coded sizes, out R, out offsets, out sizes)"""
    csz, rsz = [c.size for c in coded], [w.size for w in want]
    clays, rlays = fo.layouts(csz, 4, [d.size for d in dcoded]), fo.layouts(rsz, 1)
    _straddles(clays, csz); _straddles(rlays, rsz)
    assert any(o % 2 for lay in rlays for o in lay.offsets) and all(o % 4 == 0 for lay in clays for o in lay.offsets)
    cin, out = _far("in"), _far("out")
    for cl, rl in [(fo.near_layout(csz, 4), fo.near_layout(rsz, 1))] + _paired(clays, rlays):
        where = f"{what}, coded at {sorted(cl.anchored) or 'near offsets'}, output at {sorted(rl.anchored) or 'near offsets'}"
        cin.put(_image(cl, coded, dcoded))
        call(cin.r, _d(cl.offsets, np.int64), _d(csz, np.int32), out.r, _d(rl.offsets, np.int64), _d(rsz, np.int32))
        st = codec.status()
        kernels.add(codec.last_decode_kernel())
        if st:
            out.a.fill_(out.fill)
        assert st == 0, (where, st)
        _read_out(out, rl.offsets, want, where)


@pytest.mark.parametrize("cfg_name", ["simple", "mixing"])
def test_decode_batch_reads_far_coded_bytes_and_writes_far_output(cfg_name, pair):
    """every generation of the build; lit_decode2 without caches, with the library's caches and -- the plain stride-1 decoder -- with
    the pinned high rows"""
    import divans_amd as da
    real, decoy = pair
    name = "simple" if cfg_name == "simple" else "context_mixing"
    g, o = getattr(da, "config_" + name)(), getattr(po, "config_" + name)()
    coded, dcoded = _oracle(o, real), _oracle(o, decoy)
    for c, s in zip(coded, real):
        assert not s.size or (po.lit_decode(o, c, s.size) == s).all()
    longest = max(fo.LENGTHS)
    settings = [("library's choice", None)]
    if cfg_name == "simple":
        settings.append(("pinned high rows", lambda c: c.set_high_row_pinning(2)))
    settings += [(f"generation {gen}", lambda c, gen=gen: c.set_decoder(gen)) for gen in da.decoder_generations()]
    settings.append(("lit_decode2 without caches", lambda c: c.set_decoder(2, (0, 0, 0, 0))))
    seen = {}
    for what, setup in settings:
        codec = da.LiteralCodec(g, longest)
        if setup:
            setup(codec)
        kernels = set()
        _decode_far(codec, lambda ci, co, cs, ro, roff, rs: codec.decode_batch(ci, co, cs, 8, longest, ro, out_offsets=roff, out_sizes=rs),
                    coded, dcoded, real, f"{cfg_name}, {what}", kernels)
        codec.close()
        seen[what] = sorted(kernels)
    if cfg_name == "simple":
        assert any(", 33>" in k for k in seen["pinned high rows"]), seen
    assert all(k.endswith(", 0>") for k in seen["lit_decode2 without caches"]), seen
    for what, kernels in seen.items():
        print(f"decode_batch {cfg_name}, {what}: {kernels}")


@pytest.mark.parametrize("key", ["A", "C"])
def test_decode_segments_batch_far(key, pair):
    import divans_amd as da
    fam = bc.CONFIGS[key]
    g, o = fam.pair(da, po)
    real, decoy = pair
    lists = _two_segments(real, fam.btype, 97300)
    coded, dcoded = _oracle_segments(o, real, lists), _oracle_segments(o, decoy, lists)
    sb, segs = _seg_tensors(lists)
    longest = max(fo.LENGTHS)
    codec = da.LiteralCodec(g, longest)
    codec.set_block_types(fam.n_btypes)
    kernels = set()
    _decode_far(codec, lambda ci, co, cs, ro, roff, rs: codec.decode_segments_batch(ci, co, cs, 8, longest, sb, segs, ro, roff, rs),
                coded, dcoded, real, f"decode_segments_batch {fam.name}", kernels)
    codec.close()
    print(f"decode_segments_batch {fam.name}: {sorted(kernels)}")


@pytest.mark.parametrize("name", ["mm4_const_plain", "mmx_map_plain_nocache"])
def test_decode_commands_batch_far(name, sources):
    """coded, raw and insert offsets all far: a family whose commands kernel has the high-row caches and one above 32 766 rows per
    stream, which has none"""
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == name)
    g, o = fam.pair(da, po)
    streams = _command_streams(fam, sources)
    lits, lists = [s["lit"] for s in streams], [s["segs"] for s in streams]
    coded, dcoded = _oracle_segments(o, lits, lists), _oracle_segments(o, _xor(lits), lists)
    raw, ins = [s["raw"] for s in streams], [s["ins"] for s in streams]
    ins_sz = [i.size for i in ins]
    ins_lays = fo.layouts(ins_sz, 1)
    _straddles(ins_lays, ins_sz)
    cmd_begin, cmds = _cmd_tensors(streams)
    lit_sz = _d([l.size for l in lits], np.int32)
    lit_cap = max(l.size for l in lits)
    _drop("slots")
    src2 = _far("in2")
    codec = da.LiteralCodec(g, max(lit_cap, 16))
    codec.set_block_types(fam.n_btypes)
    kernels, state = set(), {"k": 0}

    def call(ci, co, cs, ro, roff, rs):
        k = state["k"]; state["k"] += 1
        il = ins_lays[(k - 1) % len(ins_lays)] if k else fo.near_layout(ins_sz, 1)
        src2.put(_image(il, ins, _xor(ins)))
        codec.decode_commands_batch(ci, co, cs, 8, cmd_begin, cmds, lit_sz, lit_cap, ro, roff, rs, src2.r, _d(il.offsets, np.int64), _d(ins_sz, np.int32))

    _decode_far(codec, call, coded, dcoded, raw, f"decode_commands_batch {name}", kernels)
    assert state["k"] >= len(ins_lays) + 1
    codec.close()
    _drop("in2")
    assert all(k.endswith(f", {(19 if fam.mix else 17) if fam.cached else 0}>") for k in kernels), kernels
    print(f"decode_commands_batch {name}: {sorted(kernels)}")


def test_row_replay_reads_far_literals(pair):
    """a measurement aid: it returns a time and leaves the codec decoding correctly"""
    import torch
    import divans_amd as da
    real, decoy = pair
    g, o = da.config_simple(), po.config_simple()
    src = _far("in")
    longest = max(fo.LENGTHS)
    codec = da.LiteralCodec(g, longest)
    sizes = _d(fo.LENGTHS, np.int32)
    for lay in fo.layouts(fo.LENGTHS, 1):
        src.put(_image(lay, real, decoy))
        assert codec.row_replay(src.r, 8, longest, offsets=_d(lay.offsets, np.int64), sizes=sizes) > 0
        assert codec.status() == 0
    coded = _oracle(o, real)
    csz = [c.size for c in coded]
    lay = fo.near_layout(csz, 4)
    src.put(_image(lay, coded, coded))
    back = torch.full((1 << 20,), fo.SENTINEL, dtype=torch.uint8, device="cuda")
    rl = fo.near_layout(fo.LENGTHS, 1)
    codec.decode_batch(src.r, _d(lay.offsets, np.int64), _d(csz, np.int32), 8, longest, back, out_offsets=_d(rl.offsets, np.int64), out_sizes=sizes)
    assert codec.status() == 0
    back = back.cpu().numpy()
    gh.assert_same([back[a:a + s.size] for a, s in zip(rl.offsets, real)], real, None, "decode after row_replay")
    codec.close()


def test_byte_order_is_learned_from_a_batch_wholly_above_4g(pair):
    """the ranking of test_byte_order_is_learned_from_the_data_the_codec_sees (tests/test_gpu_parity.py), from the far bytes: at the
    truncated alias of every stream lie bytes whose most frequent values are others"""
    import divans_amd as da
    real, _ = pair
    real = [s for s in real if s.size]                  # seven streams, all above 2^32
    n = len(real)
    offs = [G32 + 4096 + 8192 * k + 1 for k in range(n)]
    assert all(G32 < a and a + s.size < G32 + G31 for a, s in zip(offs, real)) and all(fo.wrong_offsets(a) == {"truncated": a - G32} for a in offs)
    decoys = [np.resize(np.array([0x01, 0x02, 0x03, 0x03, 0x02, 0x01, 0x01], np.uint8), s.size) for s in real]
    src = _far("in")
    src.put([(fo.FRONT + a, s) for a, s in zip(offs, real)] + [(fo.FRONT + a - G32, d) for a, d in zip(offs, decoys)])
    m = min(64, n)          # the sample the kernel takes: 64 streams spread over the batch (all of a smaller one), the first 2 KiB of each
    sample = [real[(j * n) // m][:2048] for j in range(m)]
    counts = np.bincount(np.concatenate(sample), minlength=256)
    order = sorted(range(256), key=lambda b: (-int(counts[b]), b))
    expect = [0] * 256
    for r, b in enumerate(order):
        expect[b] = r
    wrong = np.bincount(np.concatenate([decoys[(j * n) // m][:2048] for j in range(m)]), minlength=256)
    assert sorted(range(256), key=lambda b: (-int(wrong[b]), b))[:3] != order[:3]
    g, o = da.config_simple(), po.config_simple()
    longest = max(s.size for s in real)
    codec = da.LiteralCodec(g, longest)
    assert codec.byte_order() == {"mode": 0, "ready": False}
    outs = codec.alloc_encode_outputs(n)
    codec.encode_batch(src.r, n, longest, outs, in_offsets=_d(offs, np.int64), in_sizes=_d([s.size for s in real], np.int32))
    assert codec.status() == 0
    bo = codec.byte_order(with_rank=True)
    assert bo["ready"] and bo["rank"] == expect, (sorted(range(256), key=lambda b: bo["rank"][b])[:8], order[:8])
    gh.assert_same(gh.split_outputs(outs, n), _oracle(o, real), None, "the batch above 2^32")
    codec.close()


# ---- C: the codec's work arrays past 2^32 ----------------------------------------------------------------------------------------

def _work_memory(need, what):
    import torch
    _drop()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{what} needs about {need >> 30} GiB of device memory, {free >> 30} GiB are free")


def _work_config(which, da):
    """(product configuration, oracle configuration, block types to set or None, the bucketed pass last_encode_path reports)"""
    if which == "simple":
        return da.config_simple(), po.config_simple(), None, 2
    if which == "mixing":
        return da.config_context_mixing(), po.config_context_mixing(), None, 3
    g, o = cx.FAMILIES["plain"].pair(da, po)
    return g, o, 8, 2


@pytest.mark.parametrize("which", ["simple", "mixing", "context_keyed"])
def test_work_arrays_past_4g(which, corpus):
    """stream * slot * element size passes 2^31 and 2^32 in every work array (far_offset_cases.THRESHOLDS) although the streams are
    short: the streaming kernels and the bucketed pass agree on all streams, the oracle agrees on the sample around the thresholds.
    No stride family is among the configurations: DESIGN.md section 4, "Offsets beyond 4 GiB", known issue."""
    import torch
    import divans_amd as da
    _work_memory(NEED_WORK[which], f"{fo.WORK_STREAMS} streams on a codec for {fo.WORK_MAX_STREAM_LEN}-byte streams ({which})")
    n, msl = fo.WORK_STREAMS, fo.WORK_MAX_STREAM_LEN
    g, o, types, bucketed = _work_config(which, da)
    buf, offs, sizes = fo.work_batch(corpus)
    longest = int(sizes.max())
    streams = [buf[int(a):int(a) + int(s)] for a, s in zip(offs, sizes)]
    sample = fo.work_sample()
    want = {i: (po.lit_encode(o, streams[i]) if streams[i].size else EMPTY) for i in sample}
    btype = int(g.btype)
    cuts = sizes // 2
    seg = np.zeros(2 * n, sc.SEG_DTYPE)
    seg["len"][0::2] = cuts; seg["len"][1::2] = sizes - cuts; seg["btype"] = btype
    # the natural context: the bytes of a call without a list
    seg["last8"][1::2] = np.array([bc.natural_last8(s, int(c)) for s, c in zip(streams, cuts)], dtype=np.uint64)
    sb, segs = _d(np.arange(0, 2 * n + 1, 2, dtype=np.int32)), _d(seg.view(np.uint8))
    d_in, d_off, d_sz = _d(buf), _d(offs, np.int64), _d(sizes, np.int32)
    pick = _d(sample, np.int64)
    codec = da.LiteralCodec(g, msl)
    if types:
        codec.set_block_types(types)
    codec.set_bucket_batch(n)
    results = {}
    for path in (1, 2):
        codec.set_encode_path(path)
        ran = 1 if path == 1 else bucketed
        outs = codec.alloc_encode_outputs(n)      # slots of divans_gpu_lit_encode_bound(65 536): ragged streams are bounded by the codec's length
        outs["out"].zero_()
        codec.encode_batch(d_in, n, longest, outs, in_offsets=d_off, in_sizes=d_sz)
        assert codec.status() == 0 and codec.last_encode_path() == ran, (which, path, codec.last_encode_path())
        souts = codec.alloc_encode_outputs(n)      # slots of divans_gpu_lit_encode_bound(65 536): ragged streams are bounded by the codec's length
        souts["out"].zero_()
        codec.encode_segments_batch(d_in, d_off, d_sz, n, longest, sb, segs, souts)
        assert codec.status() == 0 and codec.last_encode_path() == ran, (which, path, "segments", codec.last_encode_path())
        for k in ("out", "offsets", "sizes"):
            assert torch.equal(outs[k], souts[k]), (which, path, f"a natural two-segment list changed `{k}`")
        pairs = codec.model_batch(d_in, n, longest, in_offsets=d_off, in_sizes=d_sz)
        assert codec.status() == 0 and codec.last_encode_path() == ran
        used = pairs[:, :2 * longest].clone()
        picked = pairs[pick, :2 * longest].cpu().numpy().view(np.uint32)
        del pairs
        for row, i in zip(picked, sample):
            if streams[i].size:
                _, tr = po.lit_encode(o, streams[i], trace=True)
                assert (row[:2 * streams[i].size] == (tr[:, 1].astype(np.uint32) | (tr[:, 2].astype(np.uint32) << 16))).all(), (which, path, "pairs of stream", i)
        out = outs["out"]; o_off = outs["offsets"].cpu().numpy(); o_sz = outs["sizes"].cpu().numpy()
        for i in sample:
            got = out[int(o_off[i]):int(o_off[i]) + int(o_sz[i])].cpu().numpy()
            assert got.size == want[i].size and (got == want[i]).all(), (which, path, "stream", i, "differs from the oracle")
        for what, dec in (("decode_batch", lambda back: codec.decode_batch(out, outs["offsets"], outs["sizes"], n, longest, back, out_offsets=d_off, out_sizes=d_sz)),
                          ("decode_segments_batch", lambda back: codec.decode_segments_batch(out, outs["offsets"], outs["sizes"], n, longest, sb, segs, back, d_off, d_sz))):
            back = torch.zeros_like(d_in)
            dec(back)
            assert codec.status() == 0, (which, path, what)
            assert torch.equal(back, d_in), (which, path, what)
        print(f"work arrays, {which}, path {path}: pass {ran}, {codec.last_decode_kernel()}")
        results[path] = (outs, used)
        del souts
    (o1, p1), (o2, p2) = results[1], results[2]
    for k in ("out", "offsets", "sizes"):
        assert torch.equal(o1[k], o2[k]), (which, f"the streaming kernels and the bucketed pass differ in `{k}`")
    written = (torch.arange(2 * longest, device="cuda")[None, :] < 2 * d_sz[:, None])
    assert torch.equal(p1[written], p2[written]), (which, "the pairs of the streaming kernels and of the bucketed pass differ")
    codec.close()
    del results, o1, o2, p1, p2
    torch.cuda.empty_cache()


# ---- D: the pack pass with a total above 2^32 ------------------------------------------------------------------------------------

def test_pack_streams_with_a_total_above_4g():
    import torch
    import divans_amd as da
    _drop()
    free, _ = torch.cuda.mem_get_info()
    if free < (12 << 30):
        pytest.skip(f"two buffers of 4.5 GiB and the pattern's temporaries need 12 GiB of device memory, {free >> 30} GiB are free")
    half = 3 << 29                                      # 1.5 GiB
    sizes = np.array([half + 4, half, half - 4], dtype=np.int64)
    src_off = np.array([2 * half, half, 0], dtype=np.int64)          # the first stream's source lies above 2^31 and ends above 2^32
    total_src = int(src_off[0] + sizes[0]) + 64
    assert src_off[0] >= G31 and src_off[0] + sizes[0] > G32 and (src_off % 4 == 0).all() and (sizes < G32).all()
    rounded = (sizes + 3) & ~3
    ref_off = np.cumsum(rounded) - rounded
    ref_total = int(rounded.sum())
    assert ref_total > G32 and ref_off[2] > G31 and ref_off.tolist() == [0, half + 4, 2 * half + 4]
    src = torch.empty(total_src, dtype=torch.uint8, device="cuda")
    step = 1 << 27
    for a in range(0, total_src, step):     # a pattern that depends on the position and has no period of 2^31 or 2^32
        i = torch.arange(a, min(a + step, total_src), dtype=torch.int64, device="cuda")
        src[a:a + i.numel()] = ((((i * 2654435761) >> 20) ^ (i >> 29)) & 0xFF).to(torch.uint8)
        del i
    tail = 4096
    packed = torch.full((ref_total + tail,), fo.SENTINEL, dtype=torch.uint8, device="cuda")
    poff = torch.full((3,), -1, dtype=torch.int64, device="cuda"); total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    codec = da.LiteralCodec(da.config_simple(), 64)
    outputs = {"out": src, "offsets": _d(src_off, np.int64), "sizes": _d(sizes.astype(np.uint32).view(np.int32))}
    codec.pack_into(outputs, 3, packed, poff, total)
    assert codec.status() == 0
    assert poff.cpu().tolist() == ref_off.tolist() and int(total.item()) == ref_total, (poff.cpu().tolist(), int(total.item()))
    for i in range(3):
        a, b, s = int(ref_off[i]), int(src_off[i]), int(sizes[i])
        assert torch.equal(packed[a:a + s], src[b:b + s]), f"stream {i}"
    assert bool((packed[ref_total:] == fo.SENTINEL).all()), "bytes behind the total were written"
    codec.close()
    del src, packed
    torch.cuda.empty_cache()


# ---- E: the uniform layout -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg_name", ["simple", "mixing"])
def test_uniform_layout_past_4g(cfg_name, corpus):
    """no offset arrays: stream i is d_in + i * stream_len, and i * 65 536 passes 2^32 at stream 65 536 -- the benchmark's step plus
    48 streams, through encode_packed and decode_batch"""
    import torch
    import divans_amd as da
    _work_memory(NEED_UNIFORM[cfg_name], f"the uniform layout of 65 584 streams of 65 536 bytes ({cfg_name})")
    L, n = 65536, 65536 + 48
    name = "simple" if cfg_name == "simple" else "context_mixing"
    g, o = getattr(da, "config_" + name)(), getattr(po, "config_" + name)()
    block = corpus[3000:3000 + L]
    d_in = _d(block).repeat(n)
    index = torch.arange(n, dtype=torch.int32, device="cuda").view(torch.uint8).view(n, 4)
    d_in.view(n, L)[:, :4] = index
    assert d_in.numel() == n * L and n * L > G32
    codec = da.LiteralCodec(g, L)
    packed = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    poff = torch.full((n,), -1, dtype=torch.int64, device="cuda"); psz = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    codec.encode_packed(d_in, n, L, packed, poff, psz, total)
    assert codec.status() == 0
    path = codec.last_encode_path()
    offs, sz = poff.cpu().numpy(), psz.cpu().numpy()
    rounded = (sz.astype(np.int64) + 3) & ~3
    assert (offs == np.cumsum(rounded) - rounded).all() and int(total.item()) == int(rounded.sum())
    for i in (0, 65535, 65536, n - 1):
        mine = block.copy(); mine[:4] = np.frombuffer(np.uint32(i).tobytes(), np.uint8)
        assert (d_in[i * L:(i + 1) * L].cpu().numpy() == mine).all()
        ref = po.lit_encode(o, mine)
        got = packed[int(offs[i]):int(offs[i]) + int(sz[i])].cpu().numpy()
        assert got.size == ref.size and (got == ref).all(), (cfg_name, "stream", i, "differs from the oracle")
    back = torch.zeros_like(d_in)
    codec.decode_batch(packed, poff, psz, n, L, back)
    assert codec.status() == 0
    assert torch.equal(back, d_in), cfg_name
    print(f"uniform layout, {cfg_name}: pass {path}, {codec.last_decode_kernel()}")
    codec.close()
    del d_in, back, packed
    torch.cuda.empty_cache()
