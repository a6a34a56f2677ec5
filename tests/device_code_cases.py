"""The case file of tests/c/device_code.cpp (the decode kernels' source on the CPU: tests/c/README.md, "Device code on the CPU"), built
from the case builders the GPU tier uses -- plain_decoder_cases, segment_cases.shapes(small=True), stride_bucketed_cases -- with the
C oracle's bytes as the coded streams.  numpy + ctypes only.

Streams stay at a few hundred bytes (every lane of the emulated workgroup is a fiber: a decoded byte costs tens of microseconds);
the 32 768-byte chunk seam is crossed once, on the families of SEAM_FAMILIES.  Buffers are exact: no spare bytes behind the coded
streams, the offset and size arrays or the segment list, so that an overrun leaves the allocation."""
import struct

import numpy as np

import bucketed_segment_cases as bc
import far_offset_cases as fo
import plain_decoder_cases as pc
import pyoracle as po
import segment_cases as sc
import stride_bucketed_cases as sb

SHORT = 420                                   # the longest stream of segment_cases.shapes(small=True)
SEAM = ("C32768", "C32769")
SEAM_FAMILIES = ("mm0_const_plain", "mm4_map_mix")      # one non-mixing, one mixing
STRIDE_FAMILIES = ("m5", "m6", "m7", "m12")
KEEP, NO_PIN = 0xFFFFFFFF, 0xFFFFFFFF
BAD_SEGMENT = 4
SENTINEL = pc.SENTINEL


def setting(label, generation=0, rows=None, shifts=(5, 5, 5, 5), blocks=0, pinning=NO_PIN):
    """generation 0: divans_gpu_codec_set_geometry(blocks) only; rows None: set_decoder without cache arguments"""
    return dict(label=label, generation=generation, rows=tuple(rows) if rows is not None else (KEEP,) * 4, shifts=tuple(shifts), blocks=blocks, pinning=pinning)


def cm_value(mix, seg, which):
    """the CM template argument of (`none`, `high` direct mapped, `high2` 2-way, `full2` 2-way) -- lit_decode2.hip: 1 hs, 2 hc, 4 ls, 8 lc, 16 2-way"""
    high = 3 if mix else 1
    full = high | (8 if mix else 4)
    return {"none": 0, "high": high, "high2": high | 16, "full2": (high if seg else full) | 16}[which]


def decoder_settings(cached, seg):
    """[(setting, key of cm_value)]: CM = 0, the high rows direct mapped (1 / 3), 2-way (17 / 19) and -- calls without a list -- the
    full 2-way set (21 / 27), on one workgroup (every resident group decodes a second stream) and once on two"""
    out = [(setting("library's choice, 2 workgroups", blocks=2), None),
           (setting("no caches, 1 workgroup", 2, (0, 0, 0, 0), blocks=1), "none")]
    if cached:
        out += [(setting("high rows direct mapped, tiny, 1 workgroup", 2, (4, 4, 0, 0), blocks=1), "high"),
                (setting("high rows 2-way, tiny, 2 workgroups", 3, (4, 4, 0, 0), blocks=2), "high2")]
        if not seg:
            out.append((setting("all four 2-way, tiny, 1 workgroup", 3, (4, 4, 4, 4), (0, 1, 2, 3), blocks=1), "full2"))
    return out


def _exact_coded(coded):
    sizes = np.array([c.size for c in coded], np.uint32)
    offs = np.concatenate([[0], np.cumsum(sizes[:-1].astype(np.int64))]).astype(np.uint64)
    return (np.concatenate(list(coded) + [np.zeros(0, np.uint8)]).astype(np.uint8), offs, sizes)


def _literal_layout(streams):
    """as plain_decoder_cases.literal_layout (gaps of 1, 2, 3, 1, ... sentinel bytes, TAIL behind) for any number of streams"""
    offs, cur = [], 0
    for i, (_, lit) in enumerate(streams):
        cur += 1 + i % 3
        offs.append(cur); cur += lit.size
    blank = np.full(cur + pc.TAIL, SENTINEL, np.uint8)
    buf = blank.copy()
    for o, (_, lit) in zip(offs, streams):
        buf[o:o + lit.size] = lit
    return buf, blank, np.array(offs, np.int64), np.array([s[1].size for s in streams], np.int32)


def _packed_layout(streams):
    """the streams back to back from offset 0 and 64 bytes behind, as tests/c/capi_contract.cpp lays a batch out"""
    sizes = np.array([s[1].size for s in streams], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes[:-1].astype(np.int64))]).astype(np.int64)
    blank = np.full(int(sizes.sum()) + 64, SENTINEL, np.uint8)
    buf = blank.copy()
    for o, (_, lit) in zip(offs, streams):
        buf[int(o):int(o) + lit.size] = lit
    return buf, blank, offs, sizes


def _slotted_coded(coded):
    """what the encoders leave (include/divans_gpu.h, divans_gpu_lit_encode_batch): one slot a stream, a multiple of 16 bytes, the coded
    bytes RIGHT-aligned in it, 0x3C elsewhere; an empty stream has size 0 and the offset of its slot's end"""
    sizes = np.array([c.size for c in coded], np.uint32)
    slot = (int(sizes.max()) + 15) // 16 * 16 + 64
    offs = ((np.arange(len(coded), dtype=np.int64) + 1) * slot - sizes.astype(np.int64)).astype(np.uint64)
    buf = np.full(len(coded) * slot, 0x3C, np.uint8)
    for o, c in zip(offs, coded):
        buf[int(o):int(o) + c.size] = c
    return buf, offs, sizes


def _case(name, cfg, set_types, streams, coded, settings, segs=None, expect_status=0, slotted=False):
    """streams: [(name, literal bytes)]; segs: the streams' segment lists as the DEVICE is given them; slotted: the batch as the
    library's own encoders and tests/c/capi_contract.cpp lay it out"""
    buf, blank, offs, sizes = _packed_layout(streams) if slotted else _literal_layout(streams)
    cbuf, coffs, csizes = _slotted_coded(coded) if slotted else _exact_coded(coded)
    case = dict(name=name, cfg=bytes(cfg), set_types=set_types, max_stream_len=max(int(sizes.max()), 16), n=len(streams), longest=int(sizes.max()),
                coded=cbuf, coff=coffs, csz=csizes, expect=buf, blank=blank, ooff=offs.astype(np.uint64), osz=sizes.astype(np.uint32),
                settings=[s for s, _ in settings], cm_keys=[k for _, k in settings], expect_status=expect_status)
    if segs is not None:
        case["seg_begin"] = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.uint32)
        case["segs"] = np.concatenate(list(segs) + [np.zeros(0, sc.SEG_DTYPE)])
    return case


def plain_case(fam, sources, seam=False):
    """plain_decoder_cases.shapes() without the streams above SHORT bytes (seam: with the two around the chunk seam)"""
    o = fam.configure(getattr(po, "config_" + fam.base)())
    o0 = pc.oracle_config(fam, o)
    streams = [(n, lit) for n, lit in pc.shapes(fam, sources) if lit.size <= SHORT or (seam and n in SEAM)]
    assert {"EMPTY", "O1", "O16", "O17", "W15", "W33", "W49"} <= {n for n, _ in streams} and len(streams) > pc.GROUPS
    settings = decoder_settings(fam.cached, False)
    if fam.name == "mm4_const_plain":        # the pinned organisation of the high stride rows: one instance
        settings.append((setting("high rows pinned, 1 workgroup", 2, (8, 0, 0, 0), blocks=1, pinning=2), "pinned"))
    if seam:      # a 32 769-byte stream takes many seconds per launch: the library's choice only
        settings = settings[:1]
    return _case(f"plain/{fam.name}" + ("/seam" if seam else ""), o, fam.n_btypes if fam.n_btypes > 1 else 0, streams, pc.oracle_bytes(o0, streams), settings)


def segment_case(fam, sources, bad_type=False):
    """segment_cases.shapes(small=True) plus the empty stream; bad_type: one segment of stream 2 names block type 9 on the device's list
    (the oracle codes it under the codec's last type, which is what the kernel falls back to): BAD_SEGMENT, every byte still right"""
    o = fam.configure(getattr(po, "config_" + fam.base)())
    shapes = sc.shapes(fam, sources, small=True)
    shapes.insert(3, ("S0", np.zeros(0, np.uint8), sc.segments([], [], [])))
    return _segment_case(f"segments/{fam.name}", fam, o, shapes, bad_type)


def stride_segment_case(fam, sources):
    o = fam.configure(po.config_simple())
    return _segment_case(f"stride_segments/{fam.name}", fam, o, sb.stride_shapes(fam, sources, small=True), False)


def _segment_case(name, fam, o, shapes, bad_type):
    oracle_lists = [segs.copy() for _, _, segs in shapes]
    device_lists = [segs.copy() for _, _, segs in shapes]
    if bad_type:
        assert fam.n_btypes == 8 and device_lists[2].size > 1
        oracle_lists[2]["btype"][1] = 7; device_lists[2]["btype"][1] = 9
        name += "/type9"
    coded = [po.lit_segments_encode(o, lit, segs["len"], segs["btype"], segs["last8"]) if lit.size else np.zeros(0, np.uint8) for (_, lit, _), segs in zip(shapes, oracle_lists)]
    settings = decoder_settings(fam.cached, True)
    if bad_type:
        settings = settings[:2]
    return _case(name, o, fam.n_btypes, [(n, lit) for n, lit, _ in shapes], coded, settings, segs=device_lists, expect_status=BAD_SEGMENT if bad_type else 0)


def stride_plain_case(fam, sources):
    """stride_bucketed_cases.plain_streams up to SHORT bytes: the lengths around the stride distance and the 64-position step"""
    o = fam.configure(po.config_simple())
    o0 = pc.oracle_config(fam, o)
    streams = [(f"L{lit.size}", lit) for lit in sb.plain_streams(fam, sources) if lit.size <= SHORT]
    return _case(f"stride_plain/{fam.name}", o, fam.n_btypes if fam.n_btypes > 1 else 0, streams, pc.oracle_bytes(o0, streams), decoder_settings(True, False))


def ragged(n, longest):
    """tests/c/capi_contract.cpp's sizes: stream 5 empty, stream 0 full"""
    v = [0 if i == 5 else 1 + (i * 37) % longest for i in range(n)]
    v[0] = longest
    return v


def ragged37_cases(sources):
    """The DECODE half of the row `stride_3/ragged37` of tests/c/capi_contract.cpp (the second occurrence of the
    open m6 fault): a codec for 300-byte streams with eight block types, ragged(37, 300) cut from the corpus back to back, two segments
    a stream, no decoder setting (the library's own: three workgroups, direct mapped), the coded bytes where the encoders leave them.
    The coded bytes are the ORACLE's: the encoder kernels do not run in this tier."""
    fam = sb.FAMILIES["m6"]
    o = fam.configure(po.config_simple())
    corpus, at, streams, lists = sources[0], 0, [], []
    for i, n in enumerate(ragged(37, 300)):
        streams.append((f"r{i}", corpus[at:at + n].copy())); at += n
        lists.append(sc.segments([n // 2, n - n // 2], [fam.btype] * 2, [0, 0]))
    own = [(setting("the library's own launch"), None)]
    plain = _case("ragged37/m6/decode_batch", o, 8, streams, pc.oracle_bytes(pc.oracle_config(fam, o), streams), own, slotted=True)
    coded = [po.lit_segments_encode(o, lit, sg["len"], sg["btype"], sg["last8"]) if lit.size else np.zeros(0, np.uint8) for (_, lit), sg in zip(streams, lists)]
    listed = _case("ragged37/m6/decode_segments_batch", o, 8, streams, coded, own, segs=lists, slotted=True)
    plain["max_stream_len"] = listed["max_stream_len"] = 300
    return [plain, listed]


# ---- the work-array shape of tests/test_gpu_far_offsets.py::test_work_arrays_past_4g for m6 (the first occurrence) ----
# stream indices around every threshold of far_offset_cases.THRESHOLDS (DESIGN's table), the first and the last stream
WORK_THRESHOLD_STREAMS = (0, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, fo.WORK_STREAMS - 1)
WORK_KERNELS = ("divans_hip::lit_decode2_kernel_any<-1, true, false, false, 17>", "divans_hip::lit_decode2_kernel_any<-1, true, false, true, 17>")
WORK_GRID = 1280


def write_work(path, corpus, full=False):
    """the file `device_code work` reads: far_offset_cases.work_batch() for the family m6 on a codec for 65 536-byte streams with eight
    block types, 32 840 streams.  full=False, the threshold form: the streams of WORK_THRESHOLD_STREAMS keep their real lengths, every
    other stream has length 0; full=True: every stream as the GPU test has it.  Per listed stream: index, the natural last8 of its second
    segment, the literal bytes, the ORACLE's coded bytes (a natural two-segment list codes the same bytes as no list)."""
    fam = sb.FAMILIES["m6"]
    o = fam.configure(po.config_simple())
    o0 = pc.oracle_config(fam, o)
    buf, offs, sizes = fo.work_batch(corpus)
    keep = range(fo.WORK_STREAMS) if full else WORK_THRESHOLD_STREAMS
    out = [b"DVWORK01"]
    name = ("work/m6/full" if full else "work/m6/thresholds").encode()
    listed = [i for i in keep if int(sizes[i]) > 0]
    out += [struct.pack("<I", len(name)), name, bytes(o), struct.pack("<4I", 8, fo.WORK_MAX_STREAM_LEN, fo.WORK_STREAMS, len(listed))]
    for i in listed:
        lit = buf[int(offs[i]):int(offs[i]) + int(sizes[i])]
        coded = po.lit_encode(o0, lit)
        out += [struct.pack("<IQ", i, int(bc.natural_last8(lit, lit.size // 2))), struct.pack("<I", lit.size), lit.tobytes(), struct.pack("<I", coded.size), coded.tobytes()]
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return len(listed)


def all_cases(sources):
    cases = []
    for fam in sc.FAMILIES:
        cases.append(plain_case(fam, sources))
        cases.append(segment_case(fam, sources))
    # (a family whose context map is not constant: only there does the byte loop read the block type's context table)
    cases.append(segment_case(next(f for f in sc.FAMILIES if f.name == "mm0_map_plain"), sources, bad_type=True))
    for name in STRIDE_FAMILIES:
        cases.append(stride_plain_case(sb.FAMILIES[name], sources))
        cases.append(stride_segment_case(sb.FAMILIES[name], sources))
    cases += ragged37_cases(sources)
    for name in SEAM_FAMILIES:
        cases.append(plain_case(next(f for f in sc.FAMILIES if f.name == name), sources, seam=True))
    return cases


def expected_kernel(case, fam, k):
    """the instance setting k of the case must run, or None where the library chooses the caches (then only the family is known)"""
    key = case["cm_keys"][k]
    seg = "seg_begin" in case
    mm = fam.mm if fam.mm >= 0 else -1
    front = f"<{mm}, {'true' if fam.ctxc else 'false'}, {'true' if fam.mix else 'false'}, {'true' if seg else 'false'}, "
    if case["name"].startswith("ragged37/"):      # the library's own launch of the second occurrence: direct mapped, three workgroups
        return front, f"divans_hip::lit_decode2_kernel_any{front}1>"
    if key is None:
        return front, None
    cm = 33 if key == "pinned" else cm_value(fam.mix, seg, key)
    return front, f"divans_hip::lit_decode2_kernel_{'w7' if mm >= 0 else 'any'}{front}{cm}>"


def write_cases(path, cases):
    def s(text):
        b = text.encode()
        return struct.pack("<I", len(b)) + b

    out = [b"DVSIMT01", struct.pack("<I", len(cases))]
    for c in cases:
        has_segs = "seg_begin" in c
        out += [s(c["name"]), c["cfg"], struct.pack("<6I", c["set_types"], c["max_stream_len"], c["n"], c["longest"], int(has_segs), c["expect_status"])]
        out += [struct.pack("<Q", c["coded"].size), c["coded"].tobytes(), c["coff"].astype("<u8").tobytes(), c["csz"].astype("<u4").tobytes()]
        assert c["expect"].size == c["blank"].size
        out += [struct.pack("<Q", c["expect"].size), c["expect"].tobytes(), c["blank"].tobytes(), c["ooff"].astype("<u8").tobytes(), c["osz"].astype("<u4").tobytes()]
        if has_segs:
            out += [c["seg_begin"].astype("<u4").tobytes(), struct.pack("<I", c["segs"].size), c["segs"].tobytes()]
        out.append(struct.pack("<I", len(c["settings"])))
        for st in c["settings"]:
            out += [struct.pack("<11I", st["generation"], *st["rows"], *st["shifts"], st["blocks"], st["pinning"]), s(st["label"])]
    with open(path, "wb") as f:
        f.write(b"".join(out))
