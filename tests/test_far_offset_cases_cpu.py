"""Guards tests/far_offset_cases.py: the placements are what they claim, no two windows share a byte, every alias stays inside the
allocation, and -- the reason the GPU tier means anything -- THE DETECTION PROPERTY on a numpy model of the buffers: a kernel that
truncated or sign-extended an offset to 32 bits would read bytes that differ from the true stream, or write where the sentinel scan
looks."""
import numpy as np
import pytest

import far_offset_cases as fo
import pyoracle as po

G31, G32 = fo.G31, fo.G32


class Sparse:
    """an allocation of `total` bytes that holds `fill` wherever nothing was written"""

    def __init__(self, total, fill, pieces=()):
        self.total, self.fill, self.pieces = total, fill, []
        for at, data in pieces:
            self.write(at, data)

    def write(self, at, data):
        assert 0 <= at and at + len(data) <= self.total
        self.pieces.append((at, np.array(data, np.uint8)))

    def read(self, at, size):
        assert 0 <= at and at + size <= self.total, "the read leaves the allocation"
        out = np.full(size, self.fill, np.uint8)
        for p, data in self.pieces:
            a, b = max(at, p), min(at + size, p + data.size)
            if a < b:
                out[a - at:b - at] = data[a - p:b - p]
        return out


@pytest.fixture(scope="module")
def pair(corpus):
    return fo.streams(corpus)


def _coded(cfg, streams):
    return [po.lit_encode(cfg, s) if s.size else np.zeros(0, np.uint8) for s in streams]


@pytest.fixture(scope="module", params=["raw", "coded_simple", "coded_mixing"])
def kind(request, pair):
    """(name, align, the streams as this kind of buffer holds them, their decoys)"""
    real, decoy = pair
    if request.param == "raw":
        return request.param, 1, real, decoy
    cfg = po.config_simple() if request.param == "coded_simple" else po.config_context_mixing()
    return request.param, 4, _coded(cfg, real), _coded(cfg, decoy)


def test_the_streams(pair):
    real, decoy = pair
    assert tuple(s.size for s in real) == fo.LENGTHS and tuple(d.size for d in decoy) == fo.LENGTHS
    every = [bytes(x) for x in real + decoy if x.size]
    assert len(set(every)) == len(every) == 14
    for s, d in zip(real, decoy):
        assert (s != d).all()
    assert fo.ALLOC == 2 ** 31 + 2 ** 32 + 2 ** 31 + 2 ** 20 and fo.ALLOC % 8 == 0 and fo.SLOT_ALLOC % 8 == 0
    assert sorted(k for k, _ in fo.ANCHORS.values()) == list(range(8))


def test_the_two_wrong_address_models():
    assert fo.wrong_offsets(0) == {} and fo.wrong_offsets(G31 - 3) == {}
    assert fo.wrong_offsets(G31 + 16) == {"sign_extended": 16 - G31}
    assert fo.wrong_offsets(G32 - 7) == {"sign_extended": -7}
    assert fo.wrong_offsets(G32) == {"truncated": 0}
    assert fo.wrong_offsets(G32 + 1) == {"truncated": 1}
    assert fo.wrong_offsets(G32 + G31 + 3) == {"truncated": G31 + 3, "sign_extended": 3 - G31}


def test_placements_are_what_they_claim(kind):
    name, align, real, decoy = kind
    sizes = [s.size for s in real]
    lays = fo.layouts(sizes, align, [d.size for d in decoy])
    used = [a for lay in lays for a in lay.anchored]
    assert sorted(used) == sorted(fo.ANCHORS) and all(lay.anchored for lay in lays), (name, [lay.anchored for lay in lays])
    at = {a: (lay.offsets[k], sizes[k]) for lay in lays for a, k in lay.anchored.items()}
    assert at["near"] == (0, 0)        # the empty stream: the near controls are near_layout and the spares of every layout
    o, s = at["straddles_2g"]; assert o < G31 < o + s and G31 - o <= 4
    o, s = at["above_2g"]; assert o == G31 + 16 and s > 0
    o, s = at["straddles_4g"]; assert o < G32 < o + s and G32 - o <= 8 and fo.LENGTHS[fo.ANCHORS["straddles_4g"][0]] >= 300
    o, s = at["ends_at_4g"]; assert o + s == G32 and s > 0
    o, s = at["at_4g"]; assert o == G32 and s > 0
    o, s = at["after_4g"]; assert G32 < o <= G32 + 4 and s > 0
    o, s = at["far"]; assert G32 + G31 < o <= G32 + G31 + 4 and s > 0
    for lay in lays:
        assert len(lay.offsets) == 8
        assert all(o % align == 0 for o in lay.offsets) and all(o % align == 0 for _, _, o, _ in lay.decoys)
        if align == 1:      # raw bytes may start anywhere: an odd offset is among them
            assert any(o % 2 for o in lay.offsets)
        assert fo.overlap(lay.windows()) is None
        for o, s, what in lay.windows():
            assert -fo.FRONT <= o and o + s <= fo.REGION, (name, what)
        for k, o in enumerate(lay.offsets):
            if k not in lay.anchored.values():
                assert o + sizes[k] < 1 << 20
    near = fo.near_layout(sizes, align)
    assert fo.overlap(near.windows()) is None and not near.decoys and all(o % align == 0 for o in near.offsets)


def test_a_wrong_read_gives_other_bytes(kind):
    """both models, every far placement: what lies at the wrong address is not the stream -- it is its decoy"""
    name, align, real, decoy = kind
    checked = 0
    for lay in fo.layouts([s.size for s in real], align, [d.size for d in decoy]):
        mem = Sparse(fo.ALLOC, 0x5A, fo.image(lay, real, decoy))
        for k, o in enumerate(lay.offsets):
            assert (mem.read(fo.FRONT + o, real[k].size) == real[k]).all()      # the right address holds the stream
        for anchor, k in lay.anchored.items():
            for model, w in fo.wrong_offsets(lay.offsets[k]).items():
                if not real[k].size:
                    continue        # an empty stream reads nothing
                got = mem.read(fo.FRONT + w, real[k].size)
                assert not (got == real[k]).all(), (name, anchor, model)
                m = min(real[k].size, decoy[k].size)
                assert (got[:m] == decoy[k][:m]).all(), (name, anchor, model)
                checked += 1
    # sign extension: above_2g, straddles_4g, ends_at_4g, far; truncation: at_4g, after_4g, far
    assert checked == 7


def test_a_wrong_write_is_seen_by_the_sentinel_scan(kind):
    name, align, real, _ = kind
    sizes = [s.size for s in real]
    checked = 0
    for lay in fo.layouts(sizes, align):
        segments = fo.outside([(fo.FRONT + o, s) for o, s in lay.real_windows()], fo.ALLOC)
        assert sum(b - a for a, b in segments) == fo.ALLOC - sum(sizes)
        for anchor, k in lay.anchored.items():
            assert not sizes[k] or not fo.scan_hits(segments, fo.FRONT + lay.offsets[k], sizes[k])     # the right write is not an alarm
            for model, w in fo.wrong_offsets(lay.offsets[k]).items():
                if sizes[k]:
                    assert 0 <= fo.FRONT + w and fo.FRONT + w + sizes[k] <= fo.ALLOC
                    assert fo.scan_hits(segments, fo.FRONT + w, sizes[k]), (name, anchor, model)
                    checked += 1
    assert checked == 7


@pytest.mark.parametrize("cfg_name", ["simple", "mixing"])
def test_the_encoders_far_slots(cfg_name, pair):
    """out_slot = 2^30 + 16, eight streams: slots end above 2^31 and 2^32, and a coded stream written at a truncated or sign-extended
    offset changes a byte outside the eight expected windows"""
    coded = _coded(po.config_simple() if cfg_name == "simple" else po.config_context_mixing(), pair[0])
    sizes = [c.size for c in coded]
    slot = fo.OUT_SLOT
    assert slot % 16 == 0 and slot >= 15392      # divans_gpu_lit_encode_bound(4097) is 15392 (asserted on the GPU tier against the library)
    offs = fo.slot_offsets(sizes)
    ends = [(i + 1) * slot for i in range(8)]
    assert [e > G31 for e in ends] == [False] + [True] * 7 and [e > G32 for e in ends] == [False] * 3 + [True] * 5
    assert all(o % 4 == 0 for o in offs) and ends[-1] == fo.SLOT_REGION and fo.FRONT + ends[-1] <= fo.SLOT_ALLOC
    segments = fo.outside([(fo.FRONT + o, s) for o, s in zip(offs, sizes)], fo.SLOT_ALLOC)
    wrong = 0
    for i, (o, s) in enumerate(zip(offs, sizes)):
        for model, w in fo.wrong_offsets(o).items():
            if s:
                assert 0 <= fo.FRONT + w and fo.FRONT + w + s <= fo.SLOT_ALLOC, (i, model)
                assert fo.scan_hits(segments, fo.FRONT + w, s), (i, model)
        wrong += bool(s and fo.wrong_offsets(o))
    assert wrong == 5       # every non-empty stream of the slots 2 .. 7 (stream 3 is the empty one)


def test_the_sentinel_scan_model():
    seg = fo.outside([(10, 5), (20, 0), (30, 2)], 40)
    assert seg == [(0, 10), (15, 30), (32, 40)]
    assert fo.scan_hits(seg, 14, 2) and not fo.scan_hits(seg, 10, 5) and fo.scan_hits(seg, 9, 1) and not fo.scan_hits(seg, 30, 2)
    with pytest.raises(AssertionError):
        fo.outside([(10, 5), (12, 5)], 40)


def test_the_work_array_batch(corpus):
    n = fo.WORK_STREAMS
    buf, offs, sizes = fo.work_batch(corpus)
    assert n == 32768 + 72 and sizes.size == n and set(sizes.tolist()) == set(fo.WORK_LENGTHS) and buf.size < 3 << 20
    assert tuple(sizes[:6]) == fo.WORK_LENGTHS
    for i in (3, 4, 5, 4097, 32771, n - 1):
        if sizes[i] >= 4:
            assert int.from_bytes(bytes(buf[int(offs[i]):int(offs[i]) + 4]), "little") == i
    long = [bytes(buf[int(o):int(o) + int(s)]) for o, s in zip(offs, sizes) if s >= 4]
    assert len(set(long)) == len(long)
    # stream * bytes-per-stream passes 2^31 / 2^32 at the thresholds: 512, 256, 128 and 64 KiB a stream for 65 536-byte slots
    for per, (t31, t32) in {512 << 10: (4096, 8192), 256 << 10: (8192, 16384), 128 << 10: (16384, 32768), 64 << 10: (32768, 65536)}.items():
        assert (t31 - 1) * per < G31 <= t31 * per and (t32 - 1) * per < G32 <= t32 * per
        assert t31 in fo.THRESHOLDS and (t32 in fo.THRESHOLDS or t32 > n)
    assert max(fo.THRESHOLDS) + 64 < n
    pick = fo.work_sample()
    for t in fo.THRESHOLDS:
        assert all(i in pick for i in range(t - 64, t + 65))
    assert n - 1 in pick and 97 in pick and len(pick) < 1000
    assert {int(sizes[i]) for i in pick} == set(fo.WORK_LENGTHS)
