"""Configurations, shapes and batches for the bucketed two-model encoder pass under SEVERAL literal block types
(launch_bucket_mix_bt_model, lit_bucket_ctx.hip: a context map in use, every mixing value 4, dynamic mixing), shared by the CPU tier
(tests/test_mix_bt_bucketed_cases_cpu.py) and the GPU tier (tests/test_gpu_mix_bt_bucketed.py).  numpy + ctypes only.

The stride model's buckets are keyed by the previous byte and keep eight high-nibble rows: the pass exists where no previous byte
reaches more than eight contexts over all block types and classes of the byte before it (high_row_slots below restates the count
divans_gpu_codec_high_row_slots gives).  Families, all with mixing value 4, two models, config_context_mixing() as their base:
  u2   UTF8, two block types, the maps of tests/segment_cases.py ((i * (2t + 1)) % 64)                     exactly 8 slots
  c8   UTF8, eight block types, a clustered map of eight contexts whose values use the whole byte           exactly 8 slots for every prev
  s8   the same map under SIGN (8 classes of prev_prev)                                                     8 slots
REFUSED: c8 with one entry of block type 5 naming a ninth context (9 slots under UTF8 and SIGN), u2's maps with three block types
(12), and segment_cases' mm4_map_mix (eight bijections of the 64 contexts: 31).
A batch is ctx_bucketed_cases.batch() plus X_all_slots: one `prev` bucket that uses every high row of the chain."""
import ctypes

import numpy as np

import bucketed_segment_cases as bc
import ctx_bucketed_cases as cc
import pyoracle as po
import segment_cases as sc

CLUSTER_VALUES = (0, 3, 17, 40, 63, 64, 128, 255)
ALL_SLOTS_AT = 17            # where X_all_slots sits in a batch: among the first 24 streams
BUCKETED_PATH = 3            # what divans_gpu_codec_last_encode_path reports for the pass
# "automatic" for a call without a list on these codecs: the bucketed pass, measured ahead of the streaming kernels at 16 384 and at
# 64 streams.  A call with a list keeps the streaming kernels unless path 2 is asked for.
AUTOMATIC_PATH_WITHOUT_A_LIST = 3


def clustered_map():
    """cmap[64 t + i] = V[(5 i + 3 t + (i >> 3)) % 8] for the eight block types"""
    i = np.arange(64)
    cmap = np.zeros(256 * 64, np.uint8)
    for t in range(8):
        cmap[64 * t:64 * t + 64] = np.asarray(CLUSTER_VALUES, np.uint8)[(5 * i + 3 * t + (i >> 3)) % 8]
    return cmap


class MixBt(sc.Family):
    """a family of tests/segment_cases.py (mixing value 4, a context map, two models) with its own map, prediction mode and block types"""

    def __init__(self, name, n_btypes, seed, mode=2, clustered=False, patch=None):
        super().__init__(name, 4, False, True, n_btypes=n_btypes, seed=seed)
        self.mode, self.clustered, self.patch = mode, clustered, patch
        self.btype = min(3, n_btypes - 1)           # the configuration's own block type (shape S5): one the codec keeps a table for

    def configure(self, cfg):
        super().configure(cfg)                      # the maps (i * (2t + 1)) % 64, mixing value 4, context_mixing 2
        if self.clustered:
            cmap = clustered_map()
            if self.patch:
                cmap[self.patch[0]] = self.patch[1]
            ctypes.memmove(cfg.literal_context_map, cmap.ctypes.data, cmap.size)
        cfg.prediction_mode = self.mode
        cfg.btype = self.btype
        return cfg


FAMILIES = {
    "u2": MixBt("mm4_map_mix_u2", 2, 70),
    "c8": MixBt("mm4_map_mix_c8", 8, 71, clustered=True),
    "s8": MixBt("mm4_map_mix_s8", 8, 72, mode=3, clustered=True),
}
# name -> (family, the count divans_gpu_codec_high_row_slots gives)
REFUSED = {
    "c8_ninth_context": (MixBt("mm4_map_mix_c8_nine", 8, 73, clustered=True, patch=(64 * 5 + 37, 200)), 9),
    "s8_ninth_context": (MixBt("mm4_map_mix_s8_nine", 8, 74, mode=3, clustered=True, patch=(64 * 5 + 37, 200)), 9),
    "u3": (MixBt("mm4_map_mix_u3", 3, 75), 12),
    "mm4_map_mix": (next(f for f in sc.FAMILIES if f.name == "mm4_map_mix"), 31),
}


def contexts_by_prev(cfg, n_btypes):
    """[prev] -> the distinct contexts literal_context_map[((lut0[prev] | lut1[prev_prev]) & 63) + 64 t] takes over t < n_btypes and
    every prev_prev, in order of first appearance, t-major (literal.rs:97-115)"""
    lut0 = np.zeros(256, np.uint8); lut1 = np.zeros(256, np.uint8)
    po.lib().orc_get_lut0(int(cfg.prediction_mode), lut0.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    po.lib().orc_get_lut1(int(cfg.prediction_mode), lut1.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)
    classes = list(dict.fromkeys(lut1.tolist()))
    out = []
    for prev in range(256):
        seen = []
        for t in range(n_btypes):
            for v in classes:
                c = int(cmap[((int(lut0[prev]) | v) & 63) + 64 * t])
                if c not in seen:
                    seen.append(c)
        out.append(seen)
    return out


def high_row_slots(cfg, n_btypes):
    return max(len(s) for s in contexts_by_prev(cfg, n_btypes))


def all_slots(fam, n=4000):
    """X_all_slots: n bytes of b"a" in 64 segments of lengths 1..200 with block types cycling 0..n_btypes-1; natural histories except
    that every eighth is random.  One `prev` bucket (but for the first byte of the segments with a random history) that uses every
    high row `a` reaches."""
    rng = np.random.default_rng(96000 + fam.seed)
    lit = np.full(n, ord("a"), np.uint8)
    assert 64 + 2 <= n <= 62 * 200
    lens = rng.integers(1, min(200, 2 * n // 64) + 1, size=64).astype(np.int64)
    lens[:2] = [1, 2]               # a one-byte segment first: the second position of the stream belongs to the next segment
    while lens.sum() != n:          # settle the sum inside 1..200
        k = int(rng.integers(2, 64))
        lens[k] += int(np.clip(n - lens.sum(), 1 - lens[k], 200 - lens[k]))
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    l8 = np.array([bc.natural_last8(lit, q) for q in starts], dtype=np.uint64)
    l8[::8] = rng.integers(0, 1 << 64, size=len(l8[::8]), dtype=np.uint64)
    return ("X_all_slots", lit, sc.segments(lens, np.arange(64) % fam.n_btypes, l8))


def batch(fam, sources):
    out = cc.batch(fam, sources)
    out.insert(ALL_SLOTS_AT, all_slots(fam))
    return out


def small_shapes(fam, sources):
    """what the pure-Python restatement can afford: the small shapes of the two case files below this one and a 400-byte X_all_slots"""
    return sc.shapes(fam, sources, small=True) + cc.new_shapes(fam, sources, small=True) + [all_slots(fam, 400)]
