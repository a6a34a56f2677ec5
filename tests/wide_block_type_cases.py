"""Configuration families with more than eight literal block types (divans_gpu_codec_set_block_types(9 .. 256)): above eight types a
codec whose context map is not constant keeps its context tables in a second layout -- lut0 | lut1 fused once, one 64-byte row of
the context map per type -- that kernel instances of their own read.  Shared by the CPU tier (tests/test_wide_block_type_cases_cpu.py:
the C oracle against the Python restatement) and the GPU tier (tests/test_gpu_wide_block_types.py, tests/test_gpu_wide_block_type_commands.py).

The families are segment_cases.Family with n_btypes 9 (the first count over the fused layout: type 8 is the first row the fused tables
never had) or 256, and a configure() of their own that gives every one of the 256 rows of literal_context_map a map of its own, so that
a kernel that reads the row of another type -- t - 8, t & 7, the last one -- codes other bytes.  The batches are segment_cases.shapes,
command_cases.directed and history_cases.directed as they stand: all three draw or cycle block types from fam.n_btypes."""
import ctypes

import numpy as np

import segment_cases as sc

LSB6, SIGN = 0, 3       # prediction modes with one lut1 class and with eight: both ends of the class axis of SEL[prev][class]


def affine_map():
    """cmap[64 t + i] = ((2 (t % 32) + 1) i + 9 (t // 32)) % 64: a bijection of the 64 contexts per type (an odd factor), all 256
    different (32 factors x 8 offsets), 64 contexts in all -- the row caches still exist"""
    t = np.arange(256)[:, None]
    i = np.arange(64)[None, :]
    return (((2 * (t % 32) + 1) * i + 9 * (t // 32)) % 64).astype(np.uint8).reshape(-1)


class WideFamily(sc.Family):
    def __init__(self, name, mm, ctxc, mix, n_btypes, cached=True, seed=0, prediction_mode=None):
        super().__init__(name, mm, ctxc, mix, n_btypes=n_btypes, cached=cached, seed=seed)
        self.prediction_mode = prediction_mode

    def configure(self, cfg):
        cfg = super().configure(cfg)        # the mixing mask, the speeds, the prediction mode of the table-driven families, the constant maps
        if not self.ctxc:
            if self.mm >= 0 and self.cached:
                cmap = affine_map()
            else:       # the random maps of segment_cases, drawn for all 256 types; without a cache over the whole byte (256 contexts:
                        # 65 536 high rows per plane, more than the 32 766 a row cache's tags can name, whatever the mixing value)
                rng = np.random.default_rng(7500 + self.seed)
                cmap = rng.integers(0, 32 if self.cached else 256, size=256 * 64, dtype=np.uint8)
            ctypes.memmove(cfg.literal_context_map, cmap.ctypes.data, cmap.size)
        if self.prediction_mode is not None:
            cfg.prediction_mode = self.prediction_mode
        return cfg


def families():
    out = []
    seed = 100
    for mm in (4, 0, -1):
        for mix in (False, True):
            tag = f"mm{mm if mm >= 0 else 'x'}_map_{'mix' if mix else 'plain'}"
            out.append(WideFamily(tag + "_bt256", mm, False, mix, 256, seed=seed)); seed += 1
    out.append(WideFamily("mm4_map_plain_bt9", 4, False, False, 9, seed=seed)); seed += 1
    out.append(WideFamily("mmx_map_mix_bt9", -1, False, True, 9, seed=seed)); seed += 1
    out.append(WideFamily("mmx_map_plain_bt256_nocache", -1, False, False, 256, cached=False, seed=seed)); seed += 1
    # ... and the other five (mixing value, mixing) pairs without a cache: every cache-less wide decoder instance runs
    for mm, mix in ((-1, True), (0, False), (0, True), (4, False), (4, True)):
        tag = f"mm{mm if mm >= 0 else 'x'}_map_{'mix' if mix else 'plain'}_bt256_nocache"
        out.append(WideFamily(tag, mm, False, mix, 256, cached=False, seed=seed + 20)); seed += 1
    out.append(WideFamily("mm4_map_plain_bt256_lsb6", 4, False, False, 256, seed=seed, prediction_mode=LSB6)); seed += 1
    out.append(WideFamily("mm0_map_mix_bt256_sign", 0, False, True, 256, seed=seed, prediction_mode=SIGN)); seed += 1
    out.append(WideFamily("mm4_const_plain_bt256", 4, True, False, 256, seed=seed)); seed += 1
    out.append(WideFamily("mm4_const_mix_bt256", 4, True, True, 256, seed=seed)); seed += 1
    return out


FAMILIES = families()
WIDE = [f for f in FAMILIES if not f.ctxc]      # the families whose kernels read the second layout
CONST = [f for f in FAMILIES if f.ctxc]         # a constant context: no kernel reads a table, the instances of eight types


# a speed under which a row total leaves i16 (divans_gpu_speed_supported is false: the wrap-checked launch, generation 1 without a cache)
# but only at the 328th update of one row: 64 + 100 k passes 0x7fff before it reaches the limit.  No stream of segment_cases.short_streams
# (at most 199 bytes) gets there, so whatever the mixing every such stream is coded and read back clean by the oracle and by the kernels.
LATE_WRAP_SPEED = (100, 0x7fff)


def by_name(name):
    return next(f for f in FAMILIES if f.name == name)


def fold(segs, how):
    """the list with every block type t >= 8 replaced by t - 8 ("minus8") or every type by t & 7 ("and7"): what a kernel that maps the
    high types onto the fused layout's eight would code"""
    out = segs.copy()
    bt = out["btype"].astype(np.int64)
    out["btype"] = np.where(bt >= 8, bt - 8, bt) if how == "minus8" else bt & 7
    return out


def low_types_only(streams):
    """the streams of a batch whose lists name block types below 8 only (for the cross-check of the two layouts)"""
    return [s for s in streams if s[2].size == 0 or int(s[2]["btype"].max()) < 8]
