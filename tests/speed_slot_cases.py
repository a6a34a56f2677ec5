"""Four DIFFERENT adaptation speeds under every encoder pass and decoder, shared by the CPU tier (tests/test_speed_slot_cases_cpu.py)
and the GPU tier (tests/test_gpu_speed_slots.py).  numpy + ctypes only.

literal_adaptation holds four (inc, lim) pairs.  The stride model blends with slot 0 for both nibbles; the context-map model, which
exists only under dynamic mixing, with slot 2 for its low-nibble rows and slot 3 for its high-nibble rows; slot 1 is never read
(literal.rs:241,320,354).  The families of the other case modules leave all four slots at one speed, so a kernel that took slot 3
where slot 2 belongs would write their bytes all the same.  Here every family of those modules -- and five that only the streaming
kernels and the decoders serve -- is coded under the four rotations of EDGE_SPEEDS: every speed sits in every slot once.
  (8100, 16384), (8160, 1)   totals settle near 32 700, every update renormalises
  (1, 16384)                 one renormalisation per 16 320 updates of a row
  (2, 1024)                  one per 480
A batch is small: its longest streams are 17 000 bytes of one value, just past the 16 320 updates (1, 16384) needs: a bucketed
pass renormalises that row at the end of its second 8 KiB piece and carries it over the piece base at 16 384.  Every stream has a segment list cut at CUTS with the
stream's own history at each cut (a row keeps its key across a segment start) and block types that cycle over the family's tables;
the two long constant streams keep ONE block type, so that one row collects all the updates."""
import numpy as np

import bucketed_segment_cases as bc
import ctx_bucketed_cases as cc
import mix_bt_bucketed_cases as mc
import segment_cases as sc
import stride_bucketed_cases as stc

EDGE_SPEEDS = [(8100, 16384), (8160, 1), (1, 16384), (2, 1024)]
ROTATIONS = [EDGE_SPEEDS[r:] + EDGE_SPEEDS[:r] for r in range(4)]
# not divans_gpu_speed_supported, but accepted: in a slot nothing reads it must change nothing
UNREAD_SPEED = (0x3000, 0x1000)
# (1, 16384) against this: the same row until the 16 320th update
LATER_RENORM = (1, 20000)
RENORM_AFTER = 16320
LONG = 17000
CUTS = [1, 2, 5000, 8191, 8193, 12000, 16384]
# the same order of lengths for the pure-Python restatement, which knows no pieces
SMALL_LONG = 13
SMALL_CUTS = [1, 2, 4, 6, 7, 9, 12]


class Case:
    """a family of another case module, the pass divans_gpu_codec_last_encode_path reports for it under path 2 (None: no bucketed pass
    serves it) and the slots its configuration reads"""

    def __init__(self, fam, path):
        self.fam, self.path = fam, path
        self.read = (0, 2, 3) if fam.mix else (0,)
        self.unread = tuple(i for i in range(4) if i not in self.read)

    def __repr__(self):
        return self.fam.name


def _sc(name):
    return next(f for f in sc.FAMILIES if f.name == name)


CASES = {}
for _k, _f in bc.CONFIGS.items():
    CASES["seg_" + _k] = Case(_f, bc.BUCKETED_PATH[_k])
for _k, _f in cc.FAMILIES.items():
    CASES["ctx_" + _k] = Case(_f, cc.BUCKETED_PATH[_k])
for _k, _f in mc.FAMILIES.items():
    CASES["mixbt_" + _k] = Case(_f, mc.BUCKETED_PATH)
for _k, _f in stc.FAMILIES.items():
    CASES["stride_" + _k] = Case(_f, stc.BUCKETED_PATH)
# no bucketed pass: a constant context under mixing value 0, 31 high-row slots, table-driven masks
STREAMING_ONLY = ("mm0_const_plain", "mm0_const_mix", "mm4_map_mix", "mmx_map_plain", "mmx_map_mix")
for _k in STREAMING_ONLY:
    CASES[_k] = Case(_sc(_k), None)
KEYS = list(CASES)


def total_stays_in_i16(inc, lim):
    """divans_gpu_speed_supported restated.  blend adds inc to a row's total at every update and takes a quarter off (with 16 for the
    bias of the last entry) once the total reaches lim: one trajectory from the default row's 64, followed until it repeats."""
    seen, v = set(), 64
    while v not in seen:
        seen.add(v)
        v += inc
        if v > 0x7fff:
            return False
        if v >= lim:
            if v + 16 > 0x7fff:
                return False
            v += 16; v -= v >> 2
    return True


def set_speeds(cfg, speeds):
    for i, (inc, lim) in enumerate(speeds):
        cfg.literal_adaptation[i].inc = inc; cfg.literal_adaptation[i].lim = lim
    return cfg


def speeds_of(cfg):
    return [(int(s.inc), int(s.lim)) for s in cfg.literal_adaptation]


def pair(case, da, po, speeds):
    """(product configuration, oracle configuration): the family's own pair() with `speeds` written over whatever it left there"""
    g, o = case.fam.pair(da, po)
    set_speeds(g, speeds); set_speeds(o, speeds)
    assert bytes(g) == bytes(o) and speeds_of(g) == [tuple(s) for s in speeds]
    return g, o


def with_slots(po, cfg, **slots):
    """a copy of the oracle configuration with slot s<i> set: with_slots(po, cfg, s1=(2, 1024))"""
    c = po.LitConfig.from_buffer_copy(bytes(cfg))
    for k, (inc, lim) in slots.items():
        c.literal_adaptation[int(k[1:])].inc = inc; c.literal_adaptation[int(k[1:])].lim = lim
    return c


def swapped(po, cfg, a, b):
    sp = speeds_of(cfg)
    sp[a], sp[b] = sp[b], sp[a]
    return set_speeds(po.LitConfig.from_buffer_copy(bytes(cfg)), sp)


def block_type_0(po, cfg):
    """what a call WITHOUT a list codes under once divans_gpu_codec_set_block_types has rebuilt the tables: table 0, whatever
    divans_lit_config::btype says"""
    c = po.LitConfig.from_buffer_copy(bytes(cfg)); c.btype = 0
    return c


def one_block_type(fam):
    """the block type the long constant streams keep: not the configuration's own where the family has another"""
    return (fam.btype + 1) % fam.n_btypes


def natural_list(fam, lit, cuts, btypes=None):
    cuts = [c for c in cuts if 0 < c < lit.size]
    lens = sc._cut(lit.size, cuts) if lit.size else []
    starts = ([0] + cuts)[:len(lens)]
    if btypes is None:
        btypes = np.arange(len(lens)) % fam.n_btypes
    return sc.segments(lens, np.resize(np.asarray(btypes), len(lens)), [bc.natural_last8(lit, q) for q in starts])


def batch(fam, data, small=False):
    """[(name, literal bytes, segment list)]: twelve streams from data = (corpus, shuffle384).  small: the same streams and lists at
    a 1000th of the lengths, for the restatement (they cannot reach the (1, 16384) renormalisation)."""
    corpus, shuffle384 = data
    long_, cuts = (SMALL_LONG, SMALL_CUTS) if small else (LONG, CUTS)
    run, text, mid = (7, 3, 5) if small else (9000, 3000, 4096)
    t = corpus[5000:5000 + text]
    rng = np.random.default_rng(65536)
    named = [
        ("K_61", np.full(long_, 0x61, np.uint8)),
        ("K_ff", np.full(long_, 0xff, np.uint8)),
        ("K_0ff0", np.resize(np.array([0x0f, 0xf0], np.uint8), long_)),
        ("K_run_text", np.concatenate([np.full(run, 0x41, np.uint8), t])),
        ("K_text_run", np.concatenate([t, np.full(run, 0x7a, np.uint8)])),
        ("K_arange", np.resize(np.arange(256, dtype=np.uint8), mid)),
        ("K_random", rng.integers(0, 256, mid, dtype=np.uint8)),
        ("K_text", corpus[30000:30000 + mid].copy()),
        ("K_shuffle", np.resize(shuffle384, mid)),
        ("K_empty", np.zeros(0, np.uint8)),
        ("K_one", corpus[777:778].copy()),
        ("K_two", corpus[778:780].copy()),
    ]
    one = one_block_type(fam)
    return [(name, lit, natural_list(fam, lit, cuts, [one] if name in ("K_61", "K_ff") else None)) for name, lit in named]


def sensitivity_streams(fam, data):
    """the constant stream and the text stream the slot-sensitivity checks code, with their lists"""
    b = batch(fam, data)
    text = data[0][5000:8000].copy()
    return [b[0], ("K_text3000", text, natural_list(fam, text, CUTS))]
