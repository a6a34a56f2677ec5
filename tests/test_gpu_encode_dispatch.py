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
import gpu_harness as gh
import pyoracle as po
import segment_cases as sc
from encode_dispatch_cases import TABLE, WRAP_SPEED

pytestmark = pytest.mark.gpu
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
        with_list = gh.oracle_bytes(o, streams)
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
    tin = gh.ragged_tensors(torch, streams)
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
        gh.assert_same(gh.split_outputs(outs, tin["n"]), without, streams, f"{key}, the path 2 of before the block types")
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
        gh.assert_same(gh.split_outputs(outs, tin["n"]), without, streams, f"{key}, path {path}, no list")
        st, got, ran = gh.encode_segments(codec, tin, outs)
        assert st == 0 and ran == listed, (key, path, "two-segment lists", st, ran)
        gh.assert_same(got, with_list, streams, f"{key}, path {path}, two-segment lists")
    codec.close()
