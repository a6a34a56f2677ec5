"""Streams, placements and expected windows for the batch entry points with data placed beyond 4 GiB, shared by the CPU tier
(tests/test_far_offset_cases_cpu.py) and the GPU tier (tests/test_gpu_far_offsets.py).  numpy only.

Every device address of the library is base + a 64-bit offset.  The two realistic ways to get one wrong are
  * the 32-bit truncation      o -> o mod 2^32, and
  * the 32-bit sign extension  o -> (o mod 2^32) - 2^32 where bit 31 of o is set,
and a wrong offset has to show as wrong BYTES, never as a fault.  So a far buffer is an allocation A of FRONT + REGION bytes of
which the library is handed the view R = A[FRONT:]: offsets are relative to R, a truncated offset lands in R itself and a
sign-extended one in the FRONT bytes in front of it.  At every such alias of a far input lies a decoy, a different valid stream of
the same length; a far output is checked by a scan for a sentinel byte over everything outside the expected windows, the aliases
included.

The eight ANCHORS cannot all be used in one buffer at once: a stream that starts at 2^32 has its truncated alias where the near
control lies, a stream that straddles 2^32 covers the place of the one that starts there.  layouts() therefore spreads them over as
few layouts as keep all windows, real and decoy, disjoint; in each layout the streams whose anchor belongs to another layout lie at
unremarkable near offsets (SPARE), so every call still runs all eight streams."""
import numpy as np

G31, G32 = 1 << 31, 1 << 32
FRONT = G31                                 # bytes of the allocation in front of R: where sign-extended offsets land
REGION = G32 + G31 + (1 << 20)              # bytes of R
ALLOC = FRONT + REGION                      # 8 GiB + 1 MiB
SCAN_CHUNK = 256 << 20                      # the sentinel scan looks at this much at a time
SENTINEL = 0xEE
LENGTHS = (300, 47, 2, 0, 1, 4097, 700, 65)
# anchor -> (the stream that lies there, its offset in R for a stream of `size` bytes whose start is a multiple of `align`).
# One anchor has to carry the empty stream: it is offset 0, since every call is also made with all eight streams at near offsets
# (near_layout) and every layout keeps the streams of other layouts near, so the near control loses nothing by it.
ANCHORS = {
    "near": (3, lambda size, align: 0),
    "straddles_2g": (1, lambda size, align: (G31 - 3) // align * align),
    "above_2g": (2, lambda size, align: G31 + 16),
    "straddles_4g": (0, lambda size, align: (G32 - 7) // align * align),
    "ends_at_4g": (5, lambda size, align: G32 - size),
    "at_4g": (4, lambda size, align: G32),
    "after_4g": (7, lambda size, align: -(-(G32 + 1) // align) * align),
    "far": (6, lambda size, align: -(-(G32 + G31 + 3) // align) * align),
}
SPARE, SPARE_STEP = 1 << 18, 1 << 15        # stream k away from its anchor: R + SPARE + k * SPARE_STEP (+ 1 where the start may be odd)
OUT_SLOT = (1 << 30) + 16                   # the encoders' output slot: slots 1 .. 7 end above 2^31, 3 .. 7 above 2^32
SLOT_REGION = 8 * OUT_SLOT
SLOT_ALLOC = FRONT + SLOT_REGION + (1 << 20)


def wrong_offsets(o):
    """{model: the offset a kernel would use instead of o} for the models that change o"""
    low = o % G32
    out = {}
    if low != o:
        out["truncated"] = low
    if low >= G31 and low - G32 != o:
        out["sign_extended"] = low - G32
    return out


def streams(corpus):
    """-> (the eight streams, their eight decoys): all sixteen non-empty ones different, a decoy differs from its stream in every byte"""
    real = [corpus[10000 + 7919 * i:10000 + 7919 * i + n].copy() for i, n in enumerate(LENGTHS)]
    decoy = [(s ^ np.uint8(0x15)) if s.size <= 4 else corpus[150000 + 6007 * i:150000 + 6007 * i + s.size].copy() for i, s in enumerate(real)]
    for s, d in zip(real, decoy):       # a wrong read must differ wherever it is looked at: make every byte differ
        same = s == d
        d[same] ^= np.uint8(0x15)
    return real, decoy


class Layout:
    """offsets[k]: stream k's offset in R.  anchored: {anchor: stream} for the anchors this layout uses.
    decoys: [(stream, model, offset in R, size)]"""

    def __init__(self, sizes, align):
        self.sizes, self.align = [int(s) for s in sizes], align
        self.offsets = [SPARE + k * SPARE_STEP + (1 if align == 1 else 0) for k in range(len(sizes))]
        self.anchored, self.decoys = {}, []

    def windows(self):
        """[(offset in R, size, what)] of every non-empty stream and decoy"""
        out = [(o, s, f"stream {k}") for k, (o, s) in enumerate(zip(self.offsets, self.sizes)) if s]
        return out + [(o, s, f"decoy of stream {k} ({m})") for k, m, o, s in self.decoys if s]

    def real_windows(self):
        return [(o, s) for o, s in zip(self.offsets, self.sizes) if s]


def overlap(windows):
    """the first two windows (offset, size, ...) that share a byte, or None"""
    w = sorted(windows)
    for a, b in zip(w, w[1:]):
        if a[0] + a[1] > b[0]:
            return a, b
    return None


def layouts(sizes, align=1, decoy_sizes=None):
    """The anchors spread over as few layouts as keep every window disjoint (greedy, in the order of ANCHORS).  sizes[k]: bytes of
    stream k as this kind of buffer holds it (raw or coded); decoy_sizes[k]: bytes of its decoy (default: the same)."""
    decoy_sizes = sizes if decoy_sizes is None else decoy_sizes
    out = []
    for anchor, (k, at) in ANCHORS.items():
        o = at(int(sizes[k]), align)
        assert o % align == 0, (anchor, o, align)
        decoys = [(k, m, w, int(decoy_sizes[k])) for m, w in wrong_offsets(o).items()]
        for lay in out + [Layout(sizes, align)]:
            keep = lay.offsets[k], list(lay.decoys)
            if k in lay.anchored.values():
                continue
            lay.offsets[k] = o
            lay.decoys = lay.decoys + decoys
            if overlap(lay.windows()) is None:
                lay.anchored[anchor] = k
                if lay not in out:
                    out.append(lay)
                break
            lay.offsets[k], lay.decoys = keep
    return out


def near_layout(sizes, align=1):
    """the same streams with every offset under 1 MiB: the control a far call must agree with byte for byte"""
    lay = Layout(sizes, align)
    assert max(o + s for o, s in zip(lay.offsets, lay.sizes)) < 1 << 20
    return lay


def image(lay, real, decoy):
    """[(offset in the allocation, bytes)] to write for a layout: the streams and the decoys"""
    out = [(FRONT + o, real[k]) for k, o in enumerate(lay.offsets) if real[k].size]
    return out + [(FRONT + o, decoy[k]) for k, _, o, _ in lay.decoys if decoy[k].size]


def slot_offsets(sizes, slot=OUT_SLOT):
    """where the encoders leave stream i: right-aligned in slot i"""
    return [(i + 1) * slot - int(s) for i, s in enumerate(sizes)]


def outside(windows, total):
    """the complement of the windows [(offset in the allocation, size)] in [0, total): what the sentinel scan covers, as sorted
    [(begin, end)] -- the numpy model of the device scan"""
    out, cur = [], 0
    for o, s in sorted((o, s) for o, s in windows if s):
        assert cur <= o and o + s <= total, "windows overlap or leave the allocation"
        if o > cur:
            out.append((cur, o))
        cur = o + s
    if cur < total:
        out.append((cur, total))
    return out


def scan_hits(segments, begin, size):
    """would the sentinel scan over `segments` (outside()) see a write of `size` bytes at `begin`?"""
    return any(a < begin + size and begin < b for a, b in segments)


# ---- part C: codec work arrays past 2^32 -------------------------------------------------------------------------------------
WORK_MAX_STREAM_LEN = 65536
WORK_STREAMS = 32768 + 72
WORK_LENGTHS = (0, 1, 2, 17, 64, 300)
# stream index at which stream * slot * element size passes 2^31 or 2^32 bytes for a codec created for 65 536-byte streams (slots
# of 65 536 positions, 131 072 nibbles): the arrays of divans_amd/csrc/capi.cpp (ensure_sf, ensure_bucket, ensure_bucket_mix) and
# the d_pairs of divans_gpu_lit_model_batch
THRESHOLDS = {
    4096: "512 KiB a stream (sfs, xs: 8 bytes a position; the streaming kernels' d_sf and model_batch's d_pairs: 4 bytes a nibble) pass 2^31",
    8192: "512 KiB a stream pass 2^32; 256 KiB a stream (maxes: 4 bytes a position) pass 2^31",
    16384: "256 KiB a stream pass 2^32; 128 KiB a stream (inv, the two-model sorted: 2 bytes a position) pass 2^31",
    32768: "128 KiB a stream pass 2^32; 64 KiB a stream (the one-model sorted) pass 2^31; the word index stream * 131 072 of the pairs passes 2^32",
}


def work_batch(corpus, n=WORK_STREAMS):
    """(buffer, offsets int64, sizes int32): n ragged streams, lengths cycling through WORK_LENGTHS, each a corpus cut whose first
    four bytes (as far as it has them) carry the stream index"""
    sizes = np.array([WORK_LENGTHS[i % len(WORK_LENGTHS)] for i in range(n)], np.int32)
    ends = np.cumsum(sizes.astype(np.int64))
    offs = ends - sizes
    buf = np.zeros(int(ends[-1]) + 64, np.uint8)
    for i in range(n):
        s = int(sizes[i])
        if s:
            a = (i * 211) % (corpus.size - 512)
            cut = corpus[a:a + s].copy()
            tag = np.frombuffer(np.uint32(i).tobytes(), np.uint8)
            cut[:min(4, s)] = tag[:min(4, s)]
            buf[int(offs[i]):int(offs[i]) + s] = cut
    return buf, offs, sizes


def work_sample(n=WORK_STREAMS):
    """the streams compared with the oracle: within 64 of every threshold, the last one, every 97th"""
    pick = set(range(0, n, 97)) | {n - 1}
    for t in THRESHOLDS:
        pick |= set(range(t - 64, t + 65))
    return sorted(i for i in pick if 0 <= i < n)
