"""The batch C ABI on a CALLER'S NON-BLOCKING stream, and several codecs side by side, on the GPU.

include/divans_gpu.h promises that the device-pointer batch calls are asynchronous and stream-ordered on the stream the codec was
created with.  Every other GPU test creates its codecs on torch's current stream -- the null stream, which serialises against
everything and hides any ordering the library forgets.  Here every codec lives on `torch.cuda.Stream()` (asserted non-blocking
through hipStreamGetFlags), every tensor a call touches is made under that stream, the host looks at a result only after
`stream.synchronize()` (never torch.cuda.synchronize()) or after the library call that is documented to wait, and:

  * THE DELAY.  A sleep kernel of DELAY_MS milliseconds (torch.cuda._sleep, calibrated once per session with events) is put on the
    stream directly in front of every library call under test.  Nothing the call enqueues has then started when the call returns,
    so a host-side step of the library that assumes completion -- a synchronous copy, a read of a total or a status word, a blob
    upload, a free -- deterministically sees the previous contents, not sometimes.
  * every output buffer is filled with a sentinel first, and every codec and buffer is used for two rounds with different data:
    a stale read returns the other round's well-formed bytes, or the sentinel, never the right ones;
  * every byte is compared with the C oracle's (tests/caller_stream_cases.py; tests/test_caller_stream_cases_cpu.py guards them).

DELAY_MS.  Host-side time of one call on the null stream, time.perf_counter around the call, nothing synchronised, warm codec,
37 streams of at most 300 bytes, measured on an MI355X host by `test_host_side_call_times_stay_below_the_delay` (it prints them):
see HOST_TIMES_MS below.  Four times the longest, and at least 20 ms, is the delay; the margin of four is for a loaded host.

The ordering defects that would FAULT (a free or a remap under a running kernel) are looked for on the CPU runtime only
(tests/test_caller_stream_contract_cpu.py).  Two value-level mutations of capi.cpp were run against test_host_wrappers_delayed on
a GPU, each a library built from a copy of the sources with one line gone ("Caller streams"):
  * no hipStreamWaitEvent(c->s_out, c->ev_done[i]) in divans_gpu_lit_decode_host_pipelined: the test FAILS (simple and mixing,
    round 0, slices of one stream: the copy-out delivers the other round's plaintext), and passes on the tree;
  * no hipStreamSynchronize in front of hipMemcpy(out_packed, ...) in divans_gpu_lit_encode_host_chunks (which
    divans_gpu_lit_encode_host forwards to: one line serves both): the test passes as on the tree -- the pageable device-to-host
    copies in front of that wait seem to return only when done on this runtime, so the wait is redundant there.  The serial
    wrappers' final waits are therefore checked by the CPU runtime, which takes the strictest reading of the API, not here.
No family has a table-driven mixing mask (tests/caller_stream_cases.py): no `<-1, ...>` instance runs here."""
import ctypes
import threading
import time

import numpy as np
import pytest

import caller_stream_cases as cs
import gpu_harness as gh
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu

# measured host-side times, milliseconds, the longest over the families and both encode paths (see the docstring)
HOST_TIMES_MS = {"encode_batch": 0.072, "encode_segments_batch": 0.064, "encode_packed (3 sub-batches)": 0.22, "decode_batch": 0.007, "decode_segments_batch": 0.009,
                 "pack_streams": 0.007, "decode_commands_batch with history (219 streams)": 0.030}
DELAY_MS = max(20.0, 4 * max(HOST_TIMES_MS.values()))      # 20 ms: four times the longest is 0.88 ms
SENTINEL = 0xA7
KEYS = list(cs.FAMILIES)
BAD_STREAM, BAD_SEGMENT = 2, 4
MUST_SUCCEED = ("set_block_types", "set_byte_order(2)", "set_byte_order(1)", "set_byte_order(0)", "set_encode_path(1)")
# the plain stride-1 decoder's instances by cache mode (lit_decode2.hip): 1 = high-row cache, direct mapped -- the codec's default
# organisation --, 1 | 16 = 2-way (set_decoder(generation=3)), 1 | 32 (CM_PIN) = the hottest rows pinned
TAGGED_DIRECT_MAPPED, PINNED = "divans_hip::lit_decode2_kernel_w7<4, true, false, false, 1>", "divans_hip::lit_decode2_kernel_w7<4, true, false, false, 33>"


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _loaded_hip():
    """the libamdhip64 torch has loaded (dlopen of a path already mapped gives that very library)"""
    import torch  # noqa: F401
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError("torch has not loaded libamdhip64")


class Side:
    """a caller's non-blocking stream with the delay kernel"""

    def __init__(self, torch):
        self.torch = torch
        self.stream = torch.cuda.Stream()
        flags = ctypes.c_uint(0xFFFF)
        rc = _loaded_hip().hipStreamGetFlags(ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(flags))
        assert rc == 0 and flags.value == 1, f"torch.cuda.Stream() is not a hipStreamNonBlocking stream (rc {rc}, flags {flags.value})"
        self.cycles_per_ms = None

    def calibrate(self):
        torch = self.torch
        cycles = 20_000_000
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(1000)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); torch.cuda._sleep(cycles); e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.5, ms
        self.cycles_per_ms = cycles / ms

    def delay(self, ms=None):
        """the sleep kernel in front of a library call; returns an event recorded right behind it: while that event has not
        completed, nothing enqueued behind it has started"""
        torch = self.torch
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(int(self.cycles_per_ms * (DELAY_MS if ms is None else ms)))
            ev = torch.cuda.Event()
            ev.record()
        return ev

    def up(self, a):
        with self.torch.cuda.stream(self.stream):
            return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

    def full(self, n, value, dtype):
        with self.torch.cuda.stream(self.stream):
            return self.torch.full((n,), value, dtype=dtype, device="cuda")

    def host(self, t):
        """the tensor on the host, after the stream -- and nothing else -- has been waited for"""
        self.stream.synchronize()
        with self.torch.cuda.stream(self.stream):
            h = t.cpu()
        return h.numpy()


@pytest.fixture(scope="module")
def side():
    import torch
    s = Side(torch)
    s.calibrate()
    return s


# ---- tensors of a batch ----------------------------------------------------------------------------------------------------------
def _layout(streams):
    sizes = np.array([lit.size for _, lit, _ in streams], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes + (np.arange(len(sizes)) % 3))[:-1]]).astype(np.int64)      # no stream on the one before's end
    buf = np.zeros(int(offs[-1] + sizes[-1]) + 64, np.uint8)
    for o, (_, lit, _) in zip(offs, streams):
        buf[int(o):int(o) + lit.size] = lit
    return buf, offs, sizes


def _coded_layout(coded):
    offs, total = cs.packed_layout(coded)
    buf = np.zeros(total + 64, np.uint8)
    for o, c in zip(offs, coded):
        buf[int(o):int(o) + c.size] = c
    return buf, offs, np.array([c.size for c in coded], np.int32)


def _batch(side, streams):
    buf, offs, sizes = _layout(streams)
    segs = np.concatenate([s[2] for s in streams] + [np.zeros(1, sc.SEG_DTYPE)])
    seg_begin = np.concatenate([[0], np.cumsum([s[2].size for s in streams])]).astype(np.int32)
    return dict(lit=side.up(buf), off=side.up(offs), sz=side.up(sizes), sb=side.up(seg_begin), segs=side.up(segs.view(np.uint8)), n=len(streams),
                longest=int(sizes.max()), offs=offs, sizes=sizes, buf=buf)


def _blank(side, outs):
    with side.torch.cuda.stream(side.stream):
        outs["out"].fill_(SENTINEL); outs["offsets"].fill_(-1); outs["sizes"].fill_(-1)


def _split(side, outs, n):
    out, offs, sz = side.host(outs["out"]), side.host(outs["offsets"]), side.host(outs["sizes"])
    for i in range(n):
        assert 0 <= int(sz[i]) <= out.size and 0 <= int(offs[i]) <= out.size - int(sz[i]), f"stream {i}: offset {int(offs[i])}, size {int(sz[i])} (a sentinel, or stale)"
    return [out[int(offs[i]):int(offs[i]) + int(sz[i])] for i in range(n)]


def _codec(da, side, fam, g, longest=cs.SMALL_LONGEST):
    with side.torch.cuda.stream(side.stream):
        codec = da.LiteralCodec(g, longest, stream=side.stream)
        if fam.n_btypes > 1:
            codec.set_block_types(fam.n_btypes)
    return codec


def _decoded(side, back, tin, what):
    got = side.host(back)
    for i, (o, n) in enumerate(zip(tin["offs"], tin["sizes"])):
        want = tin["buf"][int(o):int(o) + int(n)]
        assert (got[int(o):int(o) + int(n)] == want).all(), f"{what}: stream {i} decoded wrong"
    mask = np.ones(got.size, bool)
    for o, n in zip(tin["offs"], tin["sizes"]):
        mask[int(o):int(o) + int(n)] = False
    assert (got[mask] == SENTINEL).all(), f"{what}: a byte outside every stream's range was written"


# ---- 0. the delay is long enough ---------------------------------------------------------------------------------------------------
def test_host_side_call_times_stay_below_the_delay(sources, side):
    """the host-side time of every kind of call under test, on the NULL stream with nothing synchronised: each stays below the
    delay (which is four times the longest recorded in HOST_TIMES_MS, and at least 20 ms), so a delayed call returns before
    anything it enqueued has started"""
    import torch
    import divans_amd as da
    times = {}
    for key in ("simple", "mixing", "cx_mix", "wide9"):
        fam, o, rounds = cs.oracle(po, key, sources)
        g = fam.pair(da, po)[0]
        codec = da.LiteralCodec(g, cs.SMALL_LONGEST)
        if fam.n_btypes > 1:
            codec.set_block_types(fam.n_btypes)
        null = Side.__new__(Side); null.torch = torch; null.stream = torch.cuda.current_stream()
        tin = _batch(null, rounds[0]["streams"])
        outs = codec.alloc_encode_outputs(tin["n"])
        cbuf, coffs, csz = _coded_layout(rounds[0]["listed"])
        d_c, d_co, d_cs = null.up(cbuf), null.up(coffs), null.up(csz)
        back = torch.zeros(tin["buf"].size, dtype=torch.uint8, device="cuda")
        packed = torch.zeros(outs["out"].numel(), dtype=torch.uint8, device="cuda"); poff = torch.zeros(tin["n"], dtype=torch.int64, device="cuda"); total = torch.zeros(1, dtype=torch.int64, device="cuda")
        calls = {
            "encode_segments_batch": lambda: codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], tin["n"], tin["longest"], tin["sb"], tin["segs"], outs),
            "decode_segments_batch": lambda: codec.decode_segments_batch(d_c, d_co, d_cs, tin["n"], tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"]),
            "pack_streams": lambda: codec.pack_into(outs, tin["n"], packed, poff, total),
        }
        if key not in cs.LIST_ONLY:
            pbuf, poffs, psz = _coded_layout(rounds[0]["plain"])
            d_p, d_po, d_ps = null.up(pbuf), null.up(poffs), null.up(psz)
            calls["decode_batch"] = lambda: codec.decode_batch(d_p, d_po, d_ps, tin["n"], tin["longest"], back, out_offsets=tin["off"], out_sizes=tin["sz"])
            calls["encode_batch"] = lambda: codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
            calls["encode_packed"] = lambda: codec.encode_packed(tin["lit"], tin["n"], tin["longest"], packed, poff, outs["sizes"], total, in_offsets=tin["off"], in_sizes=tin["sz"], sub_batch=16)
        for path in (1, 2):
            try:
                codec.set_encode_path(path)
            except da.DivansGpuError:
                continue
            for name, fn in calls.items():
                fn(); torch.cuda.synchronize()          # warm: tables, work buffers
                t0 = time.perf_counter(); fn(); dt = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                times[f"{key}/path{path}/{name}"] = max(times.get(f"{key}/path{path}/{name}", 0.0), dt)
        assert codec.status() == 0
        codec.close()
    longest = max(times.values())
    print("host-side call times, ms:", {k: round(v, 3) for k, v in sorted(times.items())}, "longest", round(longest, 3))
    assert DELAY_MS >= 20.0 and 4 * longest <= DELAY_MS, f"four times the longest host-side call time, {longest:.2f} ms, is above the delay of {DELAY_MS} ms"


def test_a_read_that_does_not_wait_sees_the_previous_contents(sources, side):
    """the method's own proof, kept in the tree: behind a delayed encode call a synchronous copy on the NULL stream -- what a step
    of the library that forgot to wait for the codec's stream would issue -- reads the sentinel in every offset and size, every
    time; once the stream has been waited for, the same buffers hold the oracle's"""
    import torch
    import divans_amd as da
    fam, o, rounds = cs.oracle(po, "simple", sources)
    codec = _codec(da, side, fam, fam.pair(da, po)[0])
    n = cs.SMALL_STREAMS
    with torch.cuda.stream(side.stream):
        outs = codec.alloc_encode_outputs(n)
    shown = 0
    for r, rd in enumerate(rounds + rounds[:1]):      # the codec's first call allocates its tables: three rounds, two must show it
        tin = _batch(side, rd["streams"])
        _blank(side, outs)
        side.stream.synchronize()
        ev = side.delay()
        codec.encode_batch(tin["lit"], n, tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
        assert torch.cuda.current_stream().cuda_stream == 0      # the copies below go through the null stream, which waits for no non-blocking one
        early_sizes, early_offsets = outs["sizes"].cpu().numpy(), outs["offsets"].cpu().numpy()
        if not ev.query():      # else the host stalled past the delay and the early read shows nothing
            shown += 1
            assert (early_sizes == -1).all() and (early_offsets == -1).all(), (r, early_sizes[:8])
        gh.assert_same(_split(side, outs, n), rd["plain"], None, f"round {r}: encode_batch")
    assert shown >= 2, f"the delay had run out before the early read in {len(rounds) + 1 - shown} of {len(rounds) + 1} rounds"
    assert codec.status() == 0
    codec.close()


# ---- 1. every device-pointer entry point, delayed, against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_device_entry_points_delayed(key, sources, side):
    import torch
    import divans_amd as da
    fam, o, rounds = cs.oracle(po, key, sources)
    g = fam.pair(da, po)[0]
    codec = _codec(da, side, fam, g)
    n = cs.SMALL_STREAMS
    with torch.cuda.stream(side.stream):
        outs = codec.alloc_encode_outputs(n)
        packed = torch.empty(outs["out"].numel(), dtype=torch.uint8, device="cuda"); poff = torch.empty(n, dtype=torch.int64, device="cuda")
        psz = torch.empty(n, dtype=torch.int32, device="cuda"); total = torch.empty(1, dtype=torch.int64, device="cuda")
        chunks = torch.empty((n, 1), dtype=torch.int32, device="cuda")
    held = []
    for r, rd in enumerate(rounds + rounds[:1]):      # round 0, round 1, and round 0 again behind round 1's contents
        streams, listed, plain = rd["streams"], rd["listed"], rd["plain"]
        tin = _batch(side, streams)
        back = side.full(tin["buf"].size, SENTINEL, torch.uint8)
        paths = []
        for path in (1, 2):
            try:
                codec.set_encode_path(path); paths.append(path)
            except da.DivansGpuError:
                # no bucketed pass: above eight block types, and where two block types of config_context_mixing's map reach too many rows
                assert path == 2 and key in cs.LIST_ONLY + ("mixing",), (key, path)
        for path in paths:
            codec.set_encode_path(path)
            what = f"{key}, round {r}, path {path}"
            if plain is not None:
                _blank(side, outs)
                ev = side.delay()
                codec.encode_batch(tin["lit"], n, tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
                held.append(not ev.query())
                gh.assert_same(_split(side, outs, n), plain, None, what + ": encode_batch")
                assert codec.last_encode_path() in ((1,) if path == 1 else (2, 3)), what
                _blank(side, outs)
                with torch.cuda.stream(side.stream):
                    chunks.zero_()
                side.delay()
                codec.encode_batch(tin["lit"], n, tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"], chunk_bytes=chunks)
                gh.assert_same(_split(side, outs, n), plain, None, what + ": encode_batch_chunks")
                assert side.host(chunks)[:, 0].tolist() == [c.size for c in plain], what
                # encode_packed in three sub-batches through codec-owned slots; pack_streams against a numpy prefix sum
                want_off, want_total = cs.packed_layout(plain)
                with torch.cuda.stream(side.stream):
                    packed.fill_(SENTINEL); poff.fill_(-1); psz.fill_(-1); total.fill_(-1)
                side.delay()
                codec.encode_packed(tin["lit"], n, tin["longest"], packed, poff, psz, total, in_offsets=tin["off"], in_sizes=tin["sz"], sub_batch=16)
                hp, ho, hs, ht = side.host(packed), side.host(poff), side.host(psz), side.host(total)
                assert int(ht[0]) == want_total and (ho == want_off).all() and hs.tolist() == [c.size for c in plain], what + ": encode_packed"
                gh.assert_same([hp[int(a):int(a) + int(b)] for a, b in zip(ho, hs)], plain, None, what + ": encode_packed")
                with torch.cuda.stream(side.stream):
                    packed.fill_(SENTINEL); poff.fill_(-1); total.fill_(-1)
                _blank(side, outs)
                codec.encode_batch(tin["lit"], n, tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
                ev = side.delay()
                codec.pack_into(outs, n, packed, poff, total)
                held.append(not ev.query())
                hp, ho, ht = side.host(packed), side.host(poff), side.host(total)
                assert int(ht[0]) == want_total and (ho == want_off).all(), what + ": pack_streams"
                gh.assert_same([hp[int(a):int(a) + c.size] for a, c in zip(ho, plain)], plain, None, what + ": pack_streams")
                if True:      # (every family with list-free calls: the pairs under the configuration's own block type)
                    side.delay()
                    with torch.cuda.stream(side.stream):
                        pairs = codec.model_batch(tin["lit"], n, tin["longest"], in_offsets=tin["off"], in_sizes=tin["sz"])
                    hpairs = side.host(pairs).view(np.uint32)
                    for i, (_, lit, _) in enumerate(streams):
                        if lit.size:
                            _, tr = po.lit_encode(o, lit, trace=True)
                            assert (hpairs[i, :2 * lit.size] == (tr[:, 1].astype(np.uint32) | (tr[:, 2].astype(np.uint32) << 16))).all(), (what, "model_batch", i)
            _blank(side, outs)
            ev = side.delay()
            codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], n, tin["longest"], tin["sb"], tin["segs"], outs)
            held.append(not ev.query())
            gh.assert_same(_split(side, outs, n), listed, None, what + ": encode_segments_batch")
        # the decoders read the ORACLE's bytes: a wrong encoder above cannot hide a wrong decoder
        for coded, name in ((plain, "decode_batch"), (listed, "decode_segments_batch")):
            if coded is None:
                continue
            cbuf, coffs, csz = _coded_layout(coded)
            d_c, d_co, d_cs = side.up(cbuf), side.up(coffs), side.up(csz)
            with torch.cuda.stream(side.stream):
                back.fill_(SENTINEL)
            ev = side.delay()
            if name == "decode_batch":
                codec.decode_batch(d_c, d_co, d_cs, n, tin["longest"], back, out_offsets=tin["off"], out_sizes=tin["sz"])
            else:
                codec.decode_segments_batch(d_c, d_co, d_cs, n, tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"])
            held.append(not ev.query())
            cs.assert_no_generic_instance(codec.last_decode_kernel())
            _decoded(side, back, tin, f"{key}, round {r}: {name}")
        assert codec.status() == 0, (key, r)      # documented to wait: nothing else does here
    # the premise of the method, on the warm rounds: the call had returned before the delay in front of it ended (a host that
    # stalls past a delay now and then loses that one call's power, nothing else: three in four must have held)
    warm = held[len(held) // 3:]
    assert 4 * sum(warm) >= 3 * len(warm), f"{key}: delayed calls returned only after their delay had run out: {held}"
    codec.close()


def test_command_entry_points_delayed(sources, side):
    """decode_commands_batch and encode_commands_batch without history (the directed batch of tests/command_cases.py) and with it
    (tests/history_cases.py, histories of their own, then one range shared by all streams), one family, one codec for all three
    batches: the raw buffer whole -- sentinels between the streams included -- and the coded bytes against the oracle's.  The encode
    call reads the two ends of the command list back and is documented to wait for the stream once: that wait is behind the delay too."""
    import torch
    import command_cases as cc
    import history_cases as hc
    import divans_amd as da
    fam = cs.FAMILIES["cx_mix"]
    g, o = fam.pair(da, po)
    batches = [("no history", cc.directed(fam, sources), None), ("own histories", hc.directed(fam, sources, "own"), "own"),
               ("a shared history", hc.directed(fam, sources, "shared"), "shared")]
    code = lambda streams: [po.lit_segments_encode(o, s["lit"], s["segs"]["len"], s["segs"]["btype"], s["segs"]["last8"]) for s in streams]
    batches = [(what, streams, mode, code(streams)) for what, streams, mode in batches]
    longest = max(cc.layout(streams, coded)["lit_longest"] for _, streams, _, coded in batches)
    codec = _codec(da, side, fam, g, longest=longest + longest % 2)
    for what, streams, mode, coded in batches:
        lay = cc.layout(streams, coded)
        n = lay["n"]
        t = {k: side.up(v) for k, v in lay.items() if isinstance(v, np.ndarray)}
        hist = {}
        if mode:
            hlay = hc.history_layout(streams, mode, hc.dictionary_of(fam))
            ht = {k: side.up(v) for k, v in hlay.items() if isinstance(v, np.ndarray)}
            hist = dict(hist=ht["hist"], hist_offsets=ht["hist_off"], hist_sizes=ht["hist_sz"])
        assert lay["lit_longest"] <= codec.max_stream_len
        ins = (t["ins"], t["ins_off"], t["ins_sz"])
        ev = side.delay()
        t0 = time.perf_counter()
        codec.decode_commands_batch(t["coded"], t["coded_off"], t["coded_sz"], n, t["cmd_begin"], t["cmds"], t["lit_sz"], lay["lit_longest"],
                                    t["raw"], t["raw_off"], t["raw_sz"], *ins, **hist)
        dt = (time.perf_counter() - t0) * 1e3
        if mode == "shared":      # the warm call: its host-side time has the margin of four under the delay as well, and it returned within it
            print(f"host-side time of decode_commands_batch (history), ms: {dt:.3f}")
            assert 4 * dt <= DELAY_MS and not ev.query(), dt
        cs.assert_no_generic_instance(codec.last_decode_kernel())
        got = side.host(t["raw"])
        assert (got == lay["expect"]).all(), f"{what}: decode_commands_batch: raw byte {int(np.argmin(got == lay['expect']))} is wrong"
        assert codec.status() == 0, what
        d_raw = side.up(lay["expect"])
        for path in (1, 2):
            codec.set_encode_path(path)
            with torch.cuda.stream(side.stream):
                outs = codec.alloc_encode_outputs(n)
                lit_sz = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            _blank(side, outs)
            side.delay()
            codec.encode_commands_batch(d_raw, t["raw_off"], t["raw_sz"], n, t["cmd_begin"], t["cmds"], lay["lit_longest"], outs, lit_sz, *ins, **hist)
            gh.assert_same(_split(side, outs, n), coded, None, f"{what}, path {path}: encode_commands_batch")
            assert side.host(lit_sz).tolist() == [s["lit"].size for s in streams], (what, path)
            assert codec.status() == 0 and codec.last_encode_path() in ((1,) if path == 1 else (2, 3)), (what, path)
    codec.close()


@pytest.mark.parametrize("key", ["simple", "cx_mix", "wide9"])
def test_status_calls_delayed(key, sources, side):
    """status() is 0 on good input and names the right bit on one damaged stream / one bad list among good neighbours,
    set_stream_flags names exactly that stream, clear_status queued behind a failing call clears that call's bit and a later
    call's bit is kept"""
    import torch
    import divans_amd as da
    fam, o, rounds = cs.oracle(po, key, sources)
    g = fam.pair(da, po)[0]
    codec = _codec(da, side, fam, g)
    n = cs.SMALL_STREAMS
    flags = side.full(n, 0, torch.uint8)
    codec.set_stream_flags(flags)
    for r, rd in enumerate(rounds):
        streams, listed = rd["streams"], rd["listed"]
        tin = _batch(side, streams)
        back = side.full(tin["buf"].size, SENTINEL, torch.uint8)
        cbuf, coffs, csz = _coded_layout(listed)
        victim = max(range(6, n), key=lambda i: streams[i][1].size - 1000 * (i % 2 != r))      # the longest stream of one parity: another one each round
        assert listed[victim].size >= 40
        bad = cbuf.copy(); bad[int(coffs[victim]) + 20] ^= 0x40
        d_good, d_bad, d_co, d_cs = side.up(cbuf), side.up(bad), side.up(coffs), side.up(csz)
        dec = lambda d: codec.decode_segments_batch(d, d_co, d_cs, n, tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"])
        side.delay(); dec(d_good)
        assert codec.status() == 0 and not side.host(flags).any(), (key, r)
        side.delay(); dec(d_bad)
        assert codec.status() == BAD_STREAM, (key, r)
        assert np.flatnonzero(side.host(flags)).tolist() == [victim], (key, r)
        with torch.cuda.stream(side.stream):
            flags.zero_()
        # a list that covers 7 bytes too few, among good neighbours
        segs = [s[2].copy() for s in streams]
        k = int(np.argmax(segs[victim]["len"])); assert segs[victim]["len"][k] > 7
        segs[victim]["len"][k] -= 7
        d_badsegs = side.up(np.concatenate(segs + [np.zeros(1, sc.SEG_DTYPE)]).view(np.uint8))
        with torch.cuda.stream(side.stream):
            outs = codec.alloc_encode_outputs(n)
        side.delay()
        codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], n, tin["longest"], tin["sb"], d_badsegs, outs)
        assert codec.status() == BAD_SEGMENT, (key, r)
        # clear_status behind a failing call; then a call that fails in another way: only the later bit is left
        side.delay(); dec(d_bad)
        assert codec._lib.divans_gpu_codec_clear_status(codec._h) == 0
        side.delay()
        codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], n, tin["longest"], tin["sb"], d_badsegs, outs)
        assert codec.status() == BAD_SEGMENT, (key, r)
        assert codec.status() == 0
        with torch.cuda.stream(side.stream):
            flags.zero_()
    codec.set_stream_flags(None)
    codec.close()


# ---- 2. status_async ---------------------------------------------------------------------------------------------------------------
def test_status_async_is_stream_ordered(sources, side):
    """the word, in page-locked memory from divans_gpu_host_alloc, still holds its sentinel when the call returns -- the copy is
    stream-ordered, not synchronous --; read after an event recorded behind the call, it reports 2 behind a delayed failing
    decode, 0 after clear_status, 0 behind a delayed clean one"""
    import torch
    import divans_amd as da
    fam, o, rounds = cs.oracle(po, "mixing", sources)
    g = fam.pair(da, po)[0]
    codec = _codec(da, side, fam, g)
    n = cs.SMALL_STREAMS
    pin = da.PinnedBuffer(64)
    word = pin.array[:4].view(np.uint32)
    p_word = ctypes.c_void_p(pin.array.ctypes.data)
    seen_early = []      # the word as the host saw it right behind the call, whenever the delay in front was still running then
    for r, rd in enumerate(rounds):
        tin = _batch(side, rd["streams"])
        back = side.full(tin["buf"].size, SENTINEL, torch.uint8)
        cbuf, coffs, csz = _coded_layout(rd["plain"])
        bad = cbuf.copy(); bad[int(coffs[7]) + 5] ^= 0x04
        d_good, d_bad, d_co, d_cs = side.up(cbuf), side.up(bad), side.up(coffs), side.up(csz)

        def ask(d):
            word[0] = 0xEEEEEEEE
            ev0 = side.delay()
            codec.decode_batch(d, d_co, d_cs, n, tin["longest"], back, out_offsets=tin["off"], out_sizes=tin["sz"])
            assert codec._lib.divans_gpu_codec_status_async(codec._h, p_word) == 0
            with torch.cuda.stream(side.stream):
                ev = torch.cuda.Event(); ev.record()
            early = int(word[0])
            if not ev0.query():      # (a host that stalled past the delay -- the codec's first call allocates its tables -- has seen nothing either way)
                seen_early.append(early)
                assert early == 0xEEEEEEEE, "status_async wrote the word before the stream got there: the copy is not stream-ordered"
            ev.synchronize()
            return int(word[0])

        assert ask(d_bad) == BAD_STREAM, r
        assert codec._lib.divans_gpu_codec_clear_status(codec._h) == 0
        assert ask(d_good) == 0, r
        _decoded(side, back, tin, f"round {r}: decode_batch behind status_async")
    assert len(seen_early) >= 2, f"only {len(seen_early)} of 4 calls returned while their delay was still running: the test showed too little"
    codec.close()
    pin.close()


# ---- 3. setters with work in flight --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["simple", "A", "cx_plain", "wide9"])
def test_setters_behind_a_delayed_launch(key, sources, side):
    """each setter is called behind a delayed launch with no wait by the test in between, then the next call is made: the bytes
    of the launch in flight and of the call after the setter are both the oracle's"""
    import torch
    import divans_amd as da
    fam, o, rounds = cs.oracle(po, key, sources)
    g = fam.pair(da, po)[0]
    codec = _codec(da, side, fam, g)
    n = cs.SMALL_STREAMS
    types = fam.n_btypes
    fewer = 8 if types == 9 else 2 if types == 8 else types
    def fewer_types_and_back():      # two blob uploads behind the launches in flight; nothing is coded under the fewer types (the lists name all of them)
        codec.set_block_types(fewer); codec.set_block_types(types)
    setters = [("set_block_types", fewer_types_and_back),
               ("set_geometry", lambda: codec.set_geometry(blocks=64)), ("set_decoder", lambda: codec.set_decoder(generation=3)),
               ("set_split_cache", lambda: codec.set_split_cache(32, 0)),
               ("set_byte_order(2)", lambda: codec.set_byte_order(2)), ("set_byte_order(1)", lambda: codec.set_byte_order(1)), ("set_byte_order(0)", lambda: codec.set_byte_order(0)),
               ("set_high_row_pinning", lambda: codec.set_high_row_pinning(2)), ("set_encode_path(2)", lambda: codec.set_encode_path(2)), ("set_encode_path(1)", lambda: codec.set_encode_path(1)),
               ("set_bucket_batch", lambda: codec.set_bucket_batch(16)), ("set_rans_split", lambda: codec.set_rans_split(1))]
    with torch.cuda.stream(side.stream):
        outs = [codec.alloc_encode_outputs(n), codec.alloc_encode_outputs(n)]
    tins = [_batch(side, rd["streams"]) for rd in rounds]
    coded = [_coded_layout(rd["listed"]) for rd in rounds]
    d_coded = [tuple(side.up(a) for a in c) for c in coded]
    backs = [side.full(t["buf"].size, SENTINEL, torch.uint8) for t in tins]

    def work(r, what):
        """one encode and one decode of round r's data, delayed, into round r's buffers; returns a checker"""
        tin, out, back, (d_c, d_co, d_cs) = tins[r], outs[r], backs[r], d_coded[r]
        _blank(side, out)
        with torch.cuda.stream(side.stream):
            back.fill_(SENTINEL)
        side.delay()
        codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], n, tin["longest"], tin["sb"], tin["segs"], out)
        codec.decode_segments_batch(d_c, d_co, d_cs, n, tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"])
        cs.assert_no_generic_instance(codec.last_decode_kernel())

        def check():
            gh.assert_same(_split(side, out, n), rounds[r]["listed"], None, f"{key}: encode_segments_batch {what}")
            _decoded(side, back, tin, f"{key}: decode_segments_batch {what}")
        return check

    for i, (name, setter) in enumerate(setters):
        if fewer == types and name == "set_block_types":
            continue
        in_flight = work(i % 2, f"in flight under {name}")
        # no wait by the test: whatever the setter needs of the stream it has to get itself.  The block types, the byte order and
        # the streaming path exist on every codec and must be taken; the tuning calls may be refused where the configuration has no
        # such organisation (as tests/c/capi_contract.cpp's tried()), with DIVANS_GPU_EINVAL and nothing disturbed
        if name in MUST_SUCCEED:
            setter()
        else:
            try:
                setter()
            except da.DivansGpuError as e:
                assert "(-1)" in str(e), (name, str(e))
        after = work(1 - i % 2, f"behind {name}")
        in_flight()
        after()
        assert codec.status() == 0, name
    codec.close()


# ---- 4. the library's call-to-call state ----------------------------------------------------------------------------------------------
def test_learned_byte_order_behind_a_delayed_decode(sources, side):
    """a decode-only codec: the first decode runs in numeric order on the tagged caches, the learn kernel runs behind it, the second
    decode runs under the learned rank on the pinned instance (cache mode 33 for 1); both decode right"""
    import torch
    import divans_amd as da
    fam = cs.FAMILIES["simple"]
    g, o = fam.pair(da, po)
    n, L = cs.CACHE_STREAMS, cs.CACHE_LEN
    codec = _codec(da, side, fam, g, longest=L)
    names = []
    for r in range(cs.ROUNDS):
        blocks = cs.block_streams(fam, (sources[0], sources[0], sources[0]), r, n, L)      # text: a rank worth learning
        coded = [po.lit_encode(o, b) for b in blocks]
        cbuf, coffs, csz = _coded_layout(coded)
        d_c, d_co, d_cs = side.up(cbuf), side.up(coffs), side.up(csz)
        back = side.full(n * L, SENTINEL, torch.uint8)
        assert codec.byte_order()["ready"] == (r > 0)
        side.delay()
        codec.decode_batch(d_c, d_co, d_cs, n, L, back)
        names.append(codec.last_decode_kernel())
        cs.assert_no_generic_instance(names[-1])
        assert (side.host(back).reshape(n, L) == blocks).all(), r
        assert codec.status() == 0
    assert codec.byte_order()["ready"] and names == [TAGGED_DIRECT_MAPPED, PINNED], names
    codec.close()


def test_placement_search_call_by_call_delayed(sources, side):
    """the set-up of test_placement_search_one_candidate_per_call_changes_no_byte on the caller's stream, every call delayed: each
    qualifying decode runs on one placement of the tables (a fresh block or fresh mapped chunks, swapped in between launches of a
    stream nothing else serialises) and the next reads its time; the bytes are right on every candidate and table_placement() shows
    that the search ran to its end.  Then the eager form (tune_tables) and row_replay, which wait for the stream themselves."""
    import torch
    import divans_amd as da
    import workload
    fam = cs.FAMILIES["simple"]
    g, o = fam.pair(da, po)
    L = 2048
    codec = _codec(da, side, fam, g, longest=L)
    n = codec.info().resident_groups // 2 + 16
    both = [workload.make_blocks(sources[0], 5 + 6 * r, n, block_len=L) for r in range(cs.ROUNDS)]
    d_in = [side.up(b) for b in both]
    with torch.cuda.stream(side.stream):
        outs = [codec.alloc_encode_outputs(n, L) for _ in both]
        back = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    for r in range(cs.ROUNDS):
        _blank(side, outs[r])
        side.delay()
        codec.encode_batch(d_in[r], n, L, outs[r])
        got = _split(side, outs[r], n)
        gh.assert_same(got[:48], [po.lit_encode(o, b) for b in both[r][:48]], None, f"round {r}: encode_batch")
    codec.search_tables(4)
    pl = codec.table_placement()
    assert pl["policy_candidates"] == 4 and pl["tried"] == 0 and not pl["searching"]
    seen = []
    for call in range(7):
        r = call % 2      # the two rounds take turns: what the call before left in `back` is the other round's plaintext
        with torch.cuda.stream(side.stream):
            back.fill_(SENTINEL)
        side.delay()
        codec.decode_batch(outs[r]["out"], outs[r]["offsets"], outs[r]["sizes"], n, L, back)
        cs.assert_no_generic_instance(codec.last_decode_kernel())
        if call == 2:      # another shape in between: decoded on the placement in use, not part of the comparison
            with torch.cuda.stream(side.stream):
                few = torch.full((48, L), SENTINEL, dtype=torch.uint8, device="cuda")
            side.delay()
            codec.decode_batch(outs[r]["out"], outs[r]["offsets"], outs[r]["sizes"], 48, L, few)
            assert (side.host(few) == both[r][:48]).all()
        assert (side.host(back) == both[r]).all() and codec.status() == 0, call
        pl = codec.table_placement()
        seen.append((pl["tried"], pl["searching"]))
    assert seen == [(0, True), (1, True), (2, True), (3, True), (4, False), (4, False), (4, False)], seen
    assert 0 < pl["best_ms"] <= pl["first_ms"] <= pl["worst_ms"], pl
    codec.tune_tables(3)
    with torch.cuda.stream(side.stream):
        back.fill_(SENTINEL)
    side.delay()
    codec.decode_batch(outs[1]["out"], outs[1]["offsets"], outs[1]["sizes"], n, L, back)
    pl = codec.table_placement()
    assert pl["tried"] == 3 and not pl["searching"] and (side.host(back) == both[1]).all() and codec.status() == 0, pl
    side.delay()
    assert codec.row_replay(d_in[0], n, L) > 0
    with torch.cuda.stream(side.stream):
        back.fill_(SENTINEL)
    side.delay()
    codec.decode_batch(outs[0]["out"], outs[0]["offsets"], outs[0]["sizes"], n, L, back)
    assert (side.host(back) == both[0]).all() and codec.status() == 0
    codec.close()


# ---- 5. the host wrappers, delayed -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["simple", "mixing"])
def test_host_wrappers_delayed(key, sources, side):
    """encode_host, encode_host_chunks (its chunk sizes against the oracle's coded sizes, which is what encode_batch_chunks is held
    to in test_device_entry_points_delayed: they sum to the coded size), decode_host, the two pipelined calls with slices of 1, 7 and
    64 streams into page-locked and pageable buffers: every one behind the delay, two rounds on one codec, against the oracle.  In
    front of every pipelined call the serial wrappers code the other round's data, so that every staging buffer holds it.
    (The pipelined wrappers wait for the codec's stream before they start, so the delay ends there: what makes a missing edge of
    theirs visible is the slice's own kernel time against a copy that starts at once, and the other round's bytes in the buffer.)"""
    import divans_amd as da
    fam = cs.FAMILIES[key]
    g, o = fam.pair(da, po)
    n, L = cs.CACHE_STREAMS, cs.CACHE_LEN
    codec = _codec(da, side, fam, g, longest=L)
    pin_in, pin_out, pin_back = da.PinnedBuffer(n * L), da.PinnedBuffer(da.encode_bound(L) * n + 64), da.PinnedBuffer(n * L)
    both = []
    for r in range(cs.ROUNDS):
        b = cs.block_streams(fam, sources, r, n, L)
        both.append((b, [po.lit_encode(o, x) for x in b]))
    for r in range(cs.ROUNDS):
        blocks, coded = both[r]
        want_off, want_total = cs.packed_layout(coded)
        what = f"{key}, round {r}"

        def other_round():
            """the OTHER round's bytes through the serial wrappers: they are then what every device staging buffer holds, so a
            pipelined copy that does not wait for its slice's kernel delivers well-formed bytes of the wrong round"""
            ob, oc = both[1 - r]
            p2, o2, s2 = codec.encode_host(ob, L)
            gh.assert_same([p2[int(a):int(a) + int(z)] for a, z in zip(o2, s2)], oc, None, f"{what}: encode_host of the other round")
            assert (codec.decode_host(p2, o2, s2, L) == ob).all(), what

        def check(res, name):
            packed, offs, sizes = res
            assert packed.size == want_total and (offs == want_off).all() and sizes.tolist() == [c.size for c in coded], f"{what}: {name}: total, offsets or sizes are not this call's"
            gh.assert_same([packed[int(a):int(a) + int(b)] for a, b in zip(offs, sizes)], coded, None, f"{what}: {name}")
            return res

        side.delay()
        packed, offs, sizes = check(codec.encode_host(blocks, L), "encode_host")
        # encode_host_chunks through the ABI (the wrapper has no method for it)
        cap = da.encode_bound(L) * n + 64
        out = np.full(cap, SENTINEL, np.uint8); h_off = np.full(n, 0xEEEEEEEEEEEEEEEE, np.uint64); h_sz = np.full(n, 0xEEEEEEEE, np.uint32); h_ch = np.full((n, 1), 0xEEEEEEEE, np.uint32)
        total = ctypes.c_size_t(0x5a5a)
        side.delay()
        rc = codec._lib.divans_gpu_lit_encode_host_chunks(codec._h, ctypes.c_void_p(blocks.ctypes.data), L, n, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(cap),
                                                         ctypes.c_void_p(h_off.ctypes.data), ctypes.c_void_p(h_sz.ctypes.data), ctypes.byref(total),
                                                         ctypes.c_void_p(h_ch.ctypes.data), 1)
        assert rc == 0
        check((out[:total.value], h_off.astype(np.int64), h_sz), "encode_host_chunks")
        assert h_ch[:, 0].tolist() == [c.size for c in coded] and int(h_ch.sum()) == sum(c.size for c in coded), what
        side.delay()
        assert (codec.decode_host(packed, offs, sizes, L) == blocks).all(), what
        for slices in (1, 7, 64):
            pin_in.array[:] = blocks.reshape(-1); pin_out.array[:] = SENTINEL; pin_back.array[:] = SENTINEL
            for data, dst in ((blocks, None), (pin_in.array, pin_out.array)):
                other_round()
                side.delay()
                check(codec.encode_host_pipelined(data, L, slice_streams=slices, out=dst), f"encode_host_pipelined({slices})")
            other_round()
            side.delay()
            assert (codec.decode_host_pipelined(packed, offs, sizes, L, slice_streams=slices) == blocks).all(), (what, slices)
            other_round()
            side.delay()
            assert (codec.decode_host_pipelined(pin_out.array[:packed.size], offs, sizes, L, slice_streams=slices, out=pin_back.array) == blocks).all(), (what, slices)
        cs.assert_no_generic_instance(codec.last_decode_kernel())
    for b in (pin_in, pin_out, pin_back):
        b.close()
    codec.close()


@pytest.mark.parametrize("key", ["simple", "mixing"])
def test_long_streams_and_piecewise_coding_delayed(key, sources, side):
    """streams of 32 769 and 65 536 bytes (the chunk seam, the one-lane-per-chunk rANS path) through encode_batch / decode_batch,
    and one stream through stream_encode_pieces / stream_decode_chunks with the cuts of test_stream_coded_piece_by_piece"""
    import torch
    import divans_amd as da
    fam = cs.FAMILIES[key]
    g, o = fam.pair(da, po)
    codec = _codec(da, side, fam, g, longest=65536)
    with torch.cuda.stream(side.stream):
        outs = codec.alloc_encode_outputs(2)
    for r in range(cs.ROUNDS):
        streams = cs.seam_streams(fam, sources, r)
        coded = [po.lit_encode(o, lit) for _, lit, _ in streams]
        tin = _batch(side, [(nm, lit, sc.segments([], [], [])) for nm, lit, _ in streams])
        _blank(side, outs)
        side.delay()
        codec.encode_batch(tin["lit"], 2, tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
        gh.assert_same(_split(side, outs, 2), coded, None, f"{key}, round {r}: encode_batch at the chunk seam")
        cbuf, coffs, csz = _coded_layout(coded)
        back = side.full(tin["buf"].size, SENTINEL, torch.uint8)
        d_c, d_co, d_cs = side.up(cbuf), side.up(coffs), side.up(csz)
        side.delay()
        codec.decode_batch(d_c, d_co, d_cs, 2, tin["longest"], back, out_offsets=tin["off"], out_sizes=tin["sz"])
        cs.assert_no_generic_instance(codec.last_decode_kernel())
        _decoded(side, back, tin, f"{key}, round {r}: decode_batch at the chunk seam")
        assert codec.status() == 0
    data = np.concatenate([sources[0][:70000], sources[1][200000:260000]])
    cuts = [0, 1, 2, 17, 4096, 32767, 32768, 32769, 65536, 65537, 100000, data.size]
    ref = po.lit_encode(o, data)
    for r in range(cs.ROUNDS):
        side.delay()
        got, sizes = codec.stream_encode_pieces([data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
        assert got.size == ref.size and (got == ref).all() and sum(sizes) == got.size, (key, r)
        side.delay()
        back, used = codec.stream_decode_chunks(ref, data.size, chunks_per_call=1 + r)
        assert used == ref.size and (back == data).all(), (key, r)
    codec.close()


# ---- 6. codecs side by side ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lineup", [0, 1])
def test_four_codecs_on_four_threads(lineup, sources):
    """four host threads, each with a non-blocking stream and a codec of its own (the second line-up has two codecs on one
    configuration: the same kernel functions with other grids and LDS sizes), start at a barrier and run three rounds of encode,
    pack, decode, segment encode and segment decode without delays; every byte is the oracle's.  Codecs are created before the
    barrier and closed after every thread has joined."""
    import torch
    import divans_amd as da
    keys = cs.SIDE_BY_SIDE[lineup]
    cases = [cs.oracle(po, k, sources) for k in keys]
    sides, codecs = [], []
    for k, (fam, o, rounds) in zip(keys, cases):
        s = Side(torch)
        sides.append(s)
        codecs.append(_codec(da, s, fam, fam.pair(da, po)[0]))
    barrier = threading.Barrier(len(keys))
    errors = [None] * len(keys)

    def run(i):
        key, (fam, o, rounds), s, codec = keys[i], cases[i], sides[i], codecs[i]
        n = cs.SMALL_STREAMS
        try:
            with torch.cuda.stream(s.stream):
                outs = codec.alloc_encode_outputs(n)
                packed = torch.empty(outs["out"].numel(), dtype=torch.uint8, device="cuda"); poff = torch.empty(n, dtype=torch.int64, device="cuda"); total = torch.empty(1, dtype=torch.int64, device="cuda")
            try:
                codec.set_encode_path(2)
            except da.DivansGpuError:
                pass
            barrier.wait()
            for r in range(3):
                rd = rounds[(r + i) % cs.ROUNDS]
                streams, listed, plain = rd["streams"], rd["listed"], rd["plain"]
                tin = _batch(s, streams)
                back = s.full(tin["buf"].size, SENTINEL, torch.uint8)
                what = f"thread {i} ({key}), round {r}"
                if plain is not None:
                    _blank(s, outs)
                    with torch.cuda.stream(s.stream):
                        packed.fill_(SENTINEL); total.fill_(-1)
                    codec.encode_batch(tin["lit"], n, tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
                    codec.pack_into(outs, n, packed, poff, total)
                    want_off, want_total = cs.packed_layout(plain)
                    hp, ho, ht = s.host(packed), s.host(poff), s.host(total)
                    assert int(ht[0]) == want_total and (ho == want_off).all(), what
                    gh.assert_same([hp[int(a):int(a) + c.size] for a, c in zip(ho, plain)], plain, None, what + ": encode_batch + pack_streams")
                    codec.decode_batch(packed, poff, outs["sizes"], n, tin["longest"], back, out_offsets=tin["off"], out_sizes=tin["sz"])
                    cs.assert_no_generic_instance(codec.last_decode_kernel())
                    _decoded(s, back, tin, what + ": decode_batch")
                    with torch.cuda.stream(s.stream):
                        back.fill_(SENTINEL)
                _blank(s, outs)
                codec.encode_segments_batch(tin["lit"], tin["off"], tin["sz"], n, tin["longest"], tin["sb"], tin["segs"], outs)
                gh.assert_same(_split(s, outs, n), listed, None, what + ": encode_segments_batch")
                codec.decode_segments_batch(outs["out"], outs["offsets"], outs["sizes"], n, tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"])
                cs.assert_no_generic_instance(codec.last_decode_kernel())
                _decoded(s, back, tin, what + ": decode_segments_batch")
                assert codec.status() == 0, what
            # the thread's own error text: a refused call here must not show another thread's message
            refused, word = ((lambda: codec.set_block_types(1000), "context tables"), (lambda: codec.set_high_row_pinning(99), "pinning"),
                             (lambda: codec.set_byte_order(99), "byte order"), (lambda: codec.set_block_types(0), "context tables"))[i]
            for _ in range(20):
                with pytest.raises(da.DivansGpuError) as e:
                    refused()
                assert word in str(e.value), f"thread {i} was refused with another thread's message: {e.value}"
            errors[i] = ("ok", str(e.value), "")
        except BaseException as exc:      # noqa: BLE001 -- reported by the main thread
            barrier.abort()
            errors[i] = ("failed", exc, "")

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(keys))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in codecs:
        c.close()
    for i, e in enumerate(errors):
        assert e is not None and e[0] == "ok", f"thread {i} ({keys[i]}): {e[1]!r}"
