"""Configurations, shapes and batches for the context-keyed bucketed encoder passes (lit_bucket_ctx.hip: a context map in use, every
mixing value 0), shared by the CPU tier (tests/test_ctx_bucketed_cases_cpu.py) and the GPU tier (tests/test_gpu_ctx_bucketed.py).
numpy + ctypes only.

The configurations are families of tests/segment_cases.py -- mm0_map_plain (one model) and mm0_map_mix (two), eight block types,
each with another bijection of the 64 contexts -- and the same two with one block type.  A batch is bucketed_segment_cases.batch()
plus the shapes at which the block type of a position is not the one of a segment that starts in its 8 KiB piece:
  X_span      five long segments of different block types on 65 536 bytes: pieces 1, 3, 4, 5 and 7 hold no segment start
  X_bt_ones   300 one-byte segments with cycling block types across the piece base at 8192
  X_empty_bt  empty segments whose block type differs from both neighbours', at offset 0 and on a piece base"""
import ctypes

import numpy as np

import bucketed_segment_cases as bc
import segment_cases as sc

PIECE = bc.PIECE
SPAN_LENS = [8000, 12000, 4000, 30000, 65536 - 54000]
SPAN_BTYPES = [1, 4, 2, 6, 3]
ONES_FIRST, ONES_COUNT, ONES_SIZE = PIECE - 150, 300, 9000
EMPTY_LENS, EMPTY_BTYPES, EMPTY_SIZE = [0, PIECE, 0, 0, 12000 - PIECE], [5, 1, 6, 7, 2], 12000


def _family(name):
    return next(f for f in sc.FAMILIES if f.name == name)


FAMILIES = {
    "plain": _family("mm0_map_plain"),
    "mix": _family("mm0_map_mix"),
    "plain_bt1": sc.Family("mm0_map_plain_bt1", 0, False, False, n_btypes=1, seed=60),
    "mix_bt1": sc.Family("mm0_map_mix_bt1", 0, False, True, n_btypes=1, seed=61),
}
# what divans_gpu_codec_last_encode_path reports: 2 = bucketed one-model, 3 = bucketed two-model
BUCKETED_PATH = {"plain": 2, "mix": 3, "plain_bt1": 2, "mix_bt1": 3}
# constant context: one bucket per stream, the bucketed passes refuse them
REFUSED = ("mm0_const_plain", "mm0_const_mix")


def new_shapes(fam, sources, small=False):
    """[(name, literal bytes, segment list)].  small: the same lists at a 32nd of the lengths (X_span) / with fewer bytes around them,
    for the pure-Python restatement, which knows no pieces: to it only the order of lengths, block types and histories matters."""
    rng = np.random.default_rng(97000 + fam.seed)
    corpus = sources[0]
    nb = fam.n_btypes
    bt = (lambda v: np.asarray(v) % nb) if nb > 1 else (lambda v: np.full(len(v), fam.btype))
    out = []

    def add(name, lit, lens, btypes):
        lens = np.asarray(lens, dtype=np.int64)
        assert int(lens.sum()) == lit.size
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
        out.append((name, lit, sc.segments(lens, bt(btypes), bc._last8s(rng, lit, starts))))

    lens = [l // 32 for l in SPAN_LENS] if small else SPAN_LENS
    add("X_span", corpus[2000:2000 + sum(lens)].copy(), lens, SPAN_BTYPES)
    first, size = (40, 400) if small else (ONES_FIRST, ONES_SIZE)
    count = 60 if small else ONES_COUNT
    add("X_bt_ones", corpus[70000:70000 + size].copy(), [first] + [1] * count + [size - first - count], np.arange(count + 2))
    lens = [0, 200, 0, 0, 150] if small else EMPTY_LENS
    add("X_empty_bt", corpus[90000:90000 + sum(lens)].copy(), lens, EMPTY_BTYPES)
    return out


def batch(fam, sources):
    """bucketed_segment_cases.batch() with the new shapes among its streams: a launch sequence of 24 streams holds some of each"""
    out = bc.batch(fam, sources)
    for at, x in zip((3, 30, 41), new_shapes(fam, sources)):
        out.insert(at, x)
    return out


def mode_config(cfg, mode, mix, seed):
    """a configuration of config_context_mixing()'s layout under prediction mode `mode` (LSB6, MSB6, UTF8, SIGN: 1, 1, 4, 8 classes of
    prev_prev) with random context maps of two block types whose values use the whole byte, every mixing value 0"""
    rng = np.random.default_rng(98000 + seed)
    cmap = np.zeros(256 * 64, np.uint8)
    cmap[:128] = rng.integers(0, 256, size=128, dtype=np.uint8)
    cmap[5] = 255; cmap[64 + 9] = 0
    ctypes.memmove(cfg.literal_context_map, cmap.ctypes.data, cmap.size)
    ctypes.memset(cfg.mixing_mask, 0, 8192)
    cfg.prediction_mode = mode
    cfg.context_mixing = 2 if mix else 0
    cfg.btype = 0
    return cfg


def plain_streams(n, sources, count=40):
    """`count` streams of n bytes for the entry point without lists: text, random bytes, an all-zero stream (one bucket), an `ab` stream"""
    rng = np.random.default_rng(99000 + n)
    data = sc._Data(sources, rng)
    out = [data.take(n) for _ in range(count)]
    out[1] = np.zeros(n, np.uint8)
    out[2] = np.resize(np.frombuffer(b"ab", dtype=np.uint8), n).copy()
    return out


def ragged_layout(blocks):
    """bucketed_segment_cases.layout() for streams without lists"""
    return bc.layout([("", b, None) for b in blocks])
