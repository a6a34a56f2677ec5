"""Every encoder pass and every decoder under four DIFFERENT adaptation speeds (tests/speed_slot_cases.py: the families of the other
case modules and five that only the streaming kernels serve, each under the four rotations of the edge speeds, so that every speed
sits in every slot once).  One small batch per case -- its longest streams just past the 16 320 updates after which (1, 16384)
renormalises a row -- is coded with its segment lists and without them, by the bucketed pass where the family has one (asserted
through divans_gpu_codec_last_encode_path: the speeds must route the call nowhere else) and by the streaming kernels, bit for bit
against the C oracle, and decoded by every generation the build offers.  A kernel that took slot 3 where slot 2 belongs, or slot 0
for a context-map row, writes other bytes here (tests/test_speed_slot_cases_cpu.py shows that on the oracle and guards it).

A second test per family puts a speed whose row totals wrap into the slots the configuration does not read: no byte may change,
the bucketed pass stays in use, the second-generation decoder stays in use and the status stays 0."""
import numpy as np
import pytest

import gpu_harness as gh
import pyoracle as po
import speed_slot_cases as ss

pytestmark = pytest.mark.gpu
# workgroups of the streaming kernels and decoders: 32 resident groups hold the twelve streams of a batch, one each as under the default
# grid, and the codec then asks for CDF tables of 32 streams instead of a full grid's (seconds of allocation under eight block types)
GRID = 2
_REFS = {}


@pytest.fixture(scope="module")
def data(corpus, shuffle384):
    return (corpus, shuffle384)


def _refs(key, r, data):
    """the configuration pair of (family, rotation), the batch and the oracle's bytes with the lists and without: computed once,
    shared, never written to"""
    if (key, r) not in _REFS:
        import divans_amd as da
        case = ss.CASES[key]
        g, o = ss.pair(case, da, po, ss.ROTATIONS[r])
        o0 = ss.block_type_0(po, o)
        streams = ss.batch(case.fam, data)
        plain = [po.lit_encode(o0, lit) if lit.size else np.zeros(0, np.uint8) for _, lit, _ in streams]
        _REFS[(key, r)] = (case, g, o0, streams, gh.oracle_bytes(o, streams), plain)
    return _REFS[(key, r)]


def _first_differing_nibble(torch, codec, tin, o0, streams, i):
    """the model pass alone (the codec's current encode path) against the oracle's put_start_freq trace of stream i"""
    n = streams[i][1].size
    pairs = codec.model_batch(tin["lit"], tin["n"], tin["longest"], in_offsets=tin["off"], in_sizes=tin["sz"])
    torch.cuda.synchronize()
    have = pairs.cpu().numpy().view(np.uint32)[i, :2 * n]
    _, tr = po.lit_encode(o0, streams[i][1], trace=True)
    want = tr[:, 1].astype(np.uint32) | (tr[:, 2].astype(np.uint32) << 16)
    d = np.flatnonzero(have != want)
    if d.size == 0:
        return "the model pass agrees with the oracle's trace: the bytes differ behind it"
    k = int(d[0])
    return (f"first differing nibble {k} (the {'low' if k & 1 else 'high'} nibble of byte {k // 2}): (start, freq) = "
            f"({int(have[k]) & 0xffff}, {int(have[k]) >> 16}), the oracle has ({int(want[k]) & 0xffff}, {int(want[k]) >> 16})")


def _encode_plain(torch, codec, tin, o0, streams, ref, what, path):
    """encode_batch on the ragged layout -> the pass that ran; every stream's bytes are the oracle's"""
    outs = codec.alloc_encode_outputs(tin["n"])
    codec.encode_batch(tin["lit"], tin["n"], tin["longest"], outs, in_offsets=tin["off"], in_sizes=tin["sz"])
    st, ran = codec.status(), codec.last_encode_path()
    assert st == 0 and ran == path, (what, st, ran)
    for i, (a, b) in enumerate(zip(gh.split_outputs(outs, tin["n"]), ref)):
        if a.size != b.size or (a != b).any():
            pytest.fail(f"{what}: stream {i} ({streams[i][0]}, {streams[i][1].size} bytes) differs from the oracle; "
                        + _first_differing_nibble(torch, codec, tin, o0, streams, i))
    return outs


def _generations(da, codec):
    """set_decoder for every generation the build offers and the configuration is accepted by (2 and 3 always are)"""
    for gen in da.decoder_generations():
        try:
            codec.set_decoder(gen, blocks=GRID)
        except da.DivansGpuError:
            assert gen not in (2, 3)
            continue
        yield gen


def _assert_back(back, buf, tin, streams, what):
    back = back.cpu().numpy()
    for (name, lit, _), off in zip(streams, tin["offs"]):
        got = back[int(off):int(off) + lit.size]
        assert (got == lit).all(), f"{what}: {name} ({lit.size} bytes) decoded wrong from byte {int(np.argmax(got != lit))}"
    assert (back == buf).all(), f"{what}: bytes written between the streams"


def _code_and_decode(torch, da, case, g, o0, streams, coded, plain, decode=True):
    """the whole of one codec's work: lists under path 2 and 1, no lists under path 2 and 1, every decoder on both"""
    tin = gh.ragged_tensors(torch, streams)
    buf = tin["lit"].cpu().numpy()
    assert tin["longest"] == ss.LONG
    codec = da.LiteralCodec(g, tin["longest"])
    codec.set_block_types(case.fam.n_btypes)
    codec.set_geometry(blocks=GRID)
    codec.set_decoder(2, blocks=GRID)
    paths = ([(2, case.path)] if case.path else []) + [(1, 1)]
    for ask, ran in paths:
        codec.set_encode_path(ask)
        outs = codec.alloc_encode_outputs(tin["n"])
        st, got, path = gh.encode_segments(codec, tin, outs)
        assert st == 0 and path == ran, (f"lists, path {ask}", st, path)
        gh.assert_same(got, coded, streams, f"lists, path {ask}")
    for gen in _generations(da, codec) if decode else ():
        back = torch.zeros_like(tin["lit"])
        codec.decode_segments_batch(outs["out"], outs["offsets"], outs["sizes"], tin["n"], tin["longest"], tin["sb"], tin["segs"], back, tin["off"], tin["sz"])
        assert codec.status() == 0, ("lists", gen)
        _assert_back(back, buf, tin, streams, f"lists, generation {gen}")
    for ask, ran in paths:
        codec.set_encode_path(ask)
        outs = _encode_plain(torch, codec, tin, o0, streams, plain, f"no lists, path {ask}", ran)
    for gen in _generations(da, codec) if decode else ():
        back = torch.zeros_like(tin["lit"])
        codec.decode_batch(outs["out"], outs["offsets"], outs["sizes"], tin["n"], tin["longest"], back, out_offsets=tin["off"], out_sizes=tin["sz"])
        assert codec.status() == 0, ("no lists", gen)
        _assert_back(back, buf, tin, streams, f"no lists, generation {gen}")
    return codec, tin, buf, outs


@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("key", ss.KEYS)
def test_four_distinct_speeds(key, r, data):
    import torch
    import divans_amd as da
    case, g, o0, streams, coded, plain = _refs(key, r, data)
    for sp in ss.ROTATIONS[r]:
        assert da.speed_supported(*sp) and ss.total_stays_in_i16(*sp), sp         # the bucketed passes must still apply
    assert len(set(ss.speeds_of(g))) == 4
    codec, _, _, _ = _code_and_decode(torch, da, case, g, o0, streams, coded, plain)
    codec.close()


@pytest.mark.parametrize("key", ss.KEYS)
def test_a_wrapping_speed_in_a_slot_nothing_reads(key, data):
    """slot 1 always, slots 2 and 3 of a one-model configuration: (0x3000, 0x1000) there is accepted and changes nothing -- the bytes
    are those of the configuration without it, the bucketed pass and the second-generation decoder stay in use, the status stays 0"""
    import torch
    import divans_amd as da
    r = ss.KEYS.index(key) % 4
    case, g, o0, streams, coded, plain = _refs(key, r, data)
    assert not da.speed_supported(*ss.UNREAD_SPEED) and da.speed_accepted(*ss.UNREAD_SPEED) and not ss.total_stays_in_i16(*ss.UNREAD_SPEED)
    g2 = da.LitConfig.from_buffer_copy(bytes(g))
    for slot in case.unread:
        g2.literal_adaptation[slot].inc, g2.literal_adaptation[slot].lim = ss.UNREAD_SPEED
    assert case.unread in ((1,), (1, 2, 3)) and bytes(g2) != bytes(g)
    codec, tin, buf, outs = _code_and_decode(torch, da, case, g2, o0, streams, coded, plain, decode=False)
    back = torch.zeros_like(tin["lit"])
    codec.decode_batch(outs["out"], outs["offsets"], outs["sizes"], tin["n"], tin["longest"], back, out_offsets=tin["off"], out_sizes=tin["sz"])
    assert codec.status() == 0
    assert "lit_decode2_kernel" in codec.last_decode_kernel(), codec.last_decode_kernel()      # not the wrap-checked launch
    _assert_back(back, buf, tin, streams, "no lists, a wrapping speed in the unread slots")
    codec.close()
