"""Which encoder model pass a call runs: one table for every kind of codec, the three encode paths and calls with and without a
segment list.  The rule (select_pass, divans_amd/csrc/capi.cpp): the codec's bucketed pass on request (path 2) and, for a call without
a list, under "automatic" (path 0); the streaming kernels otherwise -- and always under a speed whose row totals leave i16.  Path 2 is
accepted wherever a pass exists for the configuration, a wrap-checked stride-1 codec included.

Every row is a codec of the case modules; every call codes three streams of at most 300 bytes (the choice of the pass does not depend
on the data, and every sort, chain and unsort kernel runs at that size) and is compared with the C oracle's bytes.  The pass that ran
is read through divans_gpu_codec_last_encode_path: 1 streaming, 2 bucketed one-model, 3 bucketed two-model."""
import numpy as np
import pytest

import bucketed_segment_cases as bc
import ctx_bucketed_cases as cx
import mix_bt_bucketed_cases as mb
import pyoracle as po
import segment_cases as sc
import stride_bucketed_cases as stc
from test_gpu_bucketed_segments import _assert_same, _encode, _oracle, _split, _tensors

pytestmark = pytest.mark.gpu
WRAP_SPEED = (0x7800, 0x7800)       # a row's total leaves i16 at its second update


def _sc(name):
    return next(f for f in sc.FAMILIES if f.name == name)


class Row:
    """family: the configuration.  types: what set_block_types is given (None: the codec stays as created, tables for the
    configuration's own block type).  accepted: set_encode_path(2) succeeds.  ran: last_encode_path() after a call without a list and
    after one with a list, for the paths 0, 1 and 2 -- where path 2 is refused the codec keeps path 1, which it was given before.
    wrap: WRAP_SPEED in every slot.  path_2_before_types: path 2 is asked for (and accepted) on the codec as created, then the block
    types are set and the table is walked."""

    def __init__(self, family, types, accepted, ran, wrap=False, path_2_before_types=False):
        self.family, self.types, self.accepted, self.ran, self.wrap, self.path_2_before_types = family, types, accepted, ran, wrap, path_2_before_types


def _bucketed(p):
    return {0: (p, 1), 1: (1, 1), 2: (p, p)}


STREAMING = {0: (1, 1), 1: (1, 1), 2: (1, 1)}
TABLE = {
    "stride_1": Row(bc.CONFIGS["A"], 8, True, _bucketed(2)),
    "stride_3": Row(stc.FAMILIES["m6"], 8, True, _bucketed(2)),
    "two_model": Row(bc.CONFIGS["C"], 1, True, _bucketed(3)),
    "context_keyed": Row(cx.FAMILIES["plain"], 8, True, _bucketed(2)),
    "context_keyed_two_model": Row(cx.FAMILIES["mix"], 8, True, _bucketed(3)),
    "two_model_block_types": Row(mb.FAMILIES["u2"], 2, True, _bucketed(3)),
    # mixing value 0 under a constant context: one bucket per stream, no pass
    "no_pass": Row(_sc(cx.REFUSED[0]), 8, False, STREAMING),
    # the stride-1 pass exists, so path 2 is accepted; every call runs the streaming kernels, which watch for wrapped rows
    "stride_1_wrap_checked": Row(bc.CONFIGS["A"], 8, True, STREAMING, wrap=True),
    # mixing value 4 with a map and two models: the two-model pass while the codec keeps one block type's tables; with all eight a
    # previous byte reaches 31 contexts (mix_bt_bucketed_cases.REFUSED) and no pass is left, whatever path was accepted before
    "two_model_as_created": Row(_sc("mm4_map_mix"), None, True, _bucketed(3)),
    "two_model_then_8_types": Row(_sc("mm4_map_mix"), 8, False, STREAMING, path_2_before_types=True),
}
_CASES = {}


def _streams(row, corpus):
    """(streams of a call with a two-segment list each, the same bytes with no list) -- at most 300 bytes a stream"""
    fam = row.family
    rng = np.random.default_rng(97000)
    if row.wrap:        # no previous byte twice: no row is coded with after its second update
        lits = [(np.arange(n, dtype=np.uint8) * 37 % 251).astype(np.uint8) for n in (30, 9, 5)]
    else:
        lits = [corpus[5000 + 1000 * i:5000 + 1000 * i + n].copy() for i, n in enumerate((300, 47, 2))]
    out = []
    for i, lit in enumerate(lits):
        cut = lit.size // 2
        last8 = rng.integers(0, 1 << 64, size=2, dtype=np.uint64) if not row.wrap else [0, bc.natural_last8(lit, cut)]
        out.append((f"D{i}", lit, sc.segments([cut, lit.size - cut], [fam.btype, fam.btype], last8)))
    return out


def _case(key, corpus):
    """configurations, streams and the oracle's bytes with and without the lists: computed once, never written to"""
    if key not in _CASES:
        import divans_amd as da
        row = TABLE[key]
        g, o = row.family.pair(da, po)
        if row.wrap:
            assert not da.speed_supported(*WRAP_SPEED) and da.speed_accepted(*WRAP_SPEED)
            for cfg in (g, o):
                for i in range(4):
                    cfg.literal_adaptation[i].inc, cfg.literal_adaptation[i].lim = WRAP_SPEED
        streams = _streams(row, corpus)
        with_list = _oracle(o, streams)
        without = [po.lit_encode(o, lit) for _, lit, _ in streams]
        if row.wrap:    # the premise: the oracle reads its own bytes back, so no wrapped row was coded with
            for (_, lit, s), a, b in zip(streams, with_list, without):
                assert (po.lit_segments_decode(o, a, lit.size, s["len"], s["btype"], s["last8"]) == lit).all() and (po.lit_decode(o, b, lit.size) == lit).all()
        _CASES[key] = (g, streams, with_list, without)
    return _CASES[key]


@pytest.mark.parametrize("key", list(TABLE))
def test_the_pass_a_call_runs(key, corpus):
    import torch
    import divans_amd as da
    row = TABLE[key]
    g, streams, with_list, without = _case(key, corpus)
    assert len(streams) == 3 and max(s[1].size for s in streams) <= 300
    tin = _tensors(torch, streams)
    codec = da.LiteralCodec(g, max(tin["longest"], 16))
    if row.path_2_before_types:
        codec.set_encode_path(2)
    if row.types is not None:
        codec.set_block_types(row.types)
    assert codec.last_encode_path() == 0
    outs = codec.alloc_encode_outputs(tin["n"])
    if row.path_2_before_types:     # the path accepted earlier is still set: with no pass left the call runs the streaming kernels
        codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
        assert codec.status() == 0 and codec.last_encode_path() == 1
        _assert_same(_split(tin, outs), without, streams, f"{key}, the path 2 of before the block types")
    for path in (0, 1, 2):
        if path < 2 or row.accepted:
            codec.set_encode_path(path)
        else:
            with pytest.raises(da.DivansGpuError, match="bucketed encoder needs"):
                codec.set_encode_path(path)
        no_list, listed = row.ran[path]
        codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
        st, ran = codec.status(), codec.last_encode_path()
        assert st == 0 and ran == no_list, (key, path, "no list", st, ran)
        _assert_same(_split(tin, outs), without, streams, f"{key}, path {path}, no list")
        st, got, ran = _encode(codec, tin, outs)
        assert st == 0 and ran == listed, (key, path, "two-segment lists", st, ran)
        _assert_same(got, with_list, streams, f"{key}, path {path}, two-segment lists")
    codec.close()
