"""The pinned organisation of the plain stride-1 decoder's high stride rows (lit_decode2.hip, CM_PIN = 32: kernel instance <4, true,
false, false, 33>) against the tagged caches on the oracle's coded bytes.  The byte order is the English hint
(divans_gpu_codec_set_byte_order(2)), whose ranks the test reads back, so the streams can be built around the slot count P: the rows of
the previous bytes of rank < P live in LDS, every other high row goes to the table in memory.

One workgroup (16 resident groups, group s mod 16 decodes stream s) with 48 streams keeps the library's 32-row caches (P = 34) and makes
every group decode three streams one after the other -- the LDS slots start from the default CDF each time; the same kind of batch on the
library's own grid is resident all at once and gets the 64-row caches (P = 68)."""
import re

import numpy as np
import pytest

import gpu_harness as gh
import pyoracle as po
import plain_decoder_cases as pc

pytestmark = pytest.mark.gpu

GROUPS = 16
_NAME = re.compile(r"lit_decode2_kernel_w7<4, true, false, false, (\d+)>$")
_CASES = {}


def _rank():
    import divans_amd as da
    codec = da.LiteralCodec(da.config_simple(), 4096)
    codec.set_byte_order(2)
    bo = codec.byte_order(with_rank=True)
    codec.close()
    assert bo["ready"] and sorted(bo["rank"]) == list(range(256))
    return bo["rank"]


def _streams(P, corpus, rank):
    """[(name, bytes)] x 48.  Streams s, s + 16, s + 32 share a group.  (The byte before a stream's first is 0, whatever the stream holds.)"""
    rng = np.random.default_rng(1300 + P)
    by_rank = np.array(sorted(range(256), key=lambda b: rank[b]), np.uint8)
    a, b = by_rank[P - 1], by_rank[P]
    pinned_only = by_rank[:P][rng.integers(0, P, 30000)]
    unpinned_only = by_rank[P:][rng.integers(0, 256 - P, 20000)]
    alternating = np.resize(np.array([a, b], np.uint8), 5001)
    around = np.concatenate([by_rank[:P - 1], by_rank[P:P + 20]])
    once = around[rng.integers(0, around.size, 6000)]
    once[3000] = a                                        # the last pinned row: touched exactly once, by the byte after this one
    assert (pinned_only[:, None] != by_rank[None, P:]).all() and (unpinned_only[:, None] != by_rank[None, :P]).all()
    assert int((once == a).sum()) == 1
    text = lambda n, o: corpus[o:o + n].copy()
    first = [("pinned only", pinned_only), ("unpinned only", unpinned_only), ("ranks P-1 and P", alternating), ("rank P-1 once", once),
             ("C32767", text(32767, 1000)), ("C32768", text(32768, 40000)), ("C32769", text(32769, 80000)), ("C40000", text(40000, 120000))]
    first += [(f"text {k}", text(int(rng.integers(1, 3000)), 5000 * k)) for k in range(8)]
    # behind the long streams of the first round: the empty stream, one byte, and the directed streams again (slots written by a whole
    # text stream must read as the default CDF); behind the directed ones: chunk seams
    second = [("C32769 again", text(32769, 3)), ("C40000 again", text(40000, 7)), ("text", text(2000, 11)), ("text", text(2001, 13)),
              ("EMPTY", np.zeros(0, np.uint8)), ("O1", text(1, 17)), ("pinned only again", pinned_only[:7000].copy()), ("unpinned only again", unpinned_only[:7000].copy())]
    second += [(f"text b{k}", text(int(rng.integers(1, 3000)), 7000 * k + 1)) for k in range(8)]
    third = [("O1", text(1, 19)), ("EMPTY", np.zeros(0, np.uint8)), ("C32768 again", text(32768, 23)), ("C32767 again", text(32767, 29)),
             ("ranks P-1 and P again", alternating[1:].copy()), ("rank P-1 once again", once.copy()), ("text", text(2999, 31)), ("text", text(64, 37))]
    third += [(f"text c{k}", text(int(rng.integers(1, 3000)), 9000 * k + 2)) for k in range(8)]
    out = first + second + third
    assert len(out) == 3 * GROUPS
    assert sorted(s.size for _, s in out)[:4] == [0, 0, 1, 1] and {32767, 32768, 32769, 40000} <= {s.size for _, s in out}
    return out


def _case(P, corpus):
    """streams, the oracle's bytes and both layouts for slot count P: computed once, shared, never written to"""
    if P not in _CASES:
        rank = _rank()
        streams = _streams(P, corpus, rank)
        coded = pc.oracle_bytes(po.config_simple(), streams)
        _CASES[P] = dict(streams=streams, coded=coded, lit=pc.literal_layout(streams), cod=pc.coded_layout(coded), rank=rank)
    return _CASES[P]


def _cm(name):
    m = _NAME.search(name)
    assert m, name
    return int(m.group(1))


def _codec(da, case, one_workgroup):
    codec = da.LiteralCodec(da.config_simple(), int(case["lit"][3].max()))
    if one_workgroup:
        codec.set_geometry(blocks=1)
    return codec


@pytest.mark.parametrize("P", [34, 68])
def test_both_organisations_decode_the_oracles_bytes(P, corpus):
    """P = 34: one workgroup, 48 streams in three rounds.  P = 68: the library's grid and the caches it picks for a resident batch."""
    import torch
    import divans_amd as da
    case = _case(P, corpus)
    dv = gh.plain_device(torch, case)
    codec = _codec(da, case, one_workgroup=P == 34)
    codec.set_byte_order(2)
    assert codec.byte_order(with_rank=True)["rank"] == case["rank"]
    tagged = 17 if P == 34 else 1           # 2-way sets for a batch of several rounds, direct mapped for a resident one
    for what, mode, cm in (("by the byte order", 0, 33), ("tagged", 1, tagged), ("pinned", 2, 33), ("tagged again", 1, tagged), ("by the byte order again", 0, 33)):
        codec.set_high_row_pinning(mode)
        st, back, name = gh.decode_plain(codec, dv)
        assert st == 0, (what, st, name)
        assert _cm(name) == cm, (what, name)
        gh.assert_plain_decoded(back, case, f"P = {P}, {what}")
    # round trip: the encoder writes the oracle's bytes, whatever the decoder's organisation
    outs = codec.alloc_encode_outputs(dv["n"])
    codec.encode_batch(dv["lit"], dv["n"], dv["longest"], outs, in_offsets=dv["off"], in_sizes=dv["sz"])
    assert codec.status() == 0
    out = outs["out"].cpu().numpy(); offs = outs["offsets"].cpu().numpy(); sz = outs["sizes"].cpu().numpy()
    for i, ((name, lit), ref) in enumerate(zip(case["streams"], case["coded"])):
        assert int(sz[i]) == ref.size and (out[int(offs[i]):int(offs[i]) + int(sz[i])] == ref).all(), (i, name)
    with pytest.raises(da.DivansGpuError):
        codec.set_high_row_pinning(3)
    codec.close()


def test_numeric_order_keeps_the_two_way_sets(corpus):
    import torch
    import divans_amd as da
    case = _case(34, corpus)
    dv = gh.plain_device(torch, case)
    codec = _codec(da, case, one_workgroup=True)
    codec.set_byte_order(1)
    for call in range(2):
        st, back, name = gh.decode_plain(codec, dv)
        assert st == 0 and _cm(name) == 17, (call, st, name)
        gh.assert_plain_decoded(back, case, f"numeric order, call {call}")
    codec.set_high_row_pinning(2)            # forced: the byte values 0 .. 33 are pinned
    st, back, name = gh.decode_plain(codec, dv)
    assert st == 0 and _cm(name) == 33, (st, name)
    gh.assert_plain_decoded(back, case, "numeric order, pinned on request")
    codec.close()


def test_learned_order_pins_from_the_second_decode_on(corpus):
    """a codec that only decodes learns its order from the first call's output: that call runs the 2-way instance, the next the pinned one"""
    import torch
    import divans_amd as da
    case = _case(34, corpus)
    dv = gh.plain_device(torch, case)
    codec = _codec(da, case, one_workgroup=True)
    assert codec.byte_order() == {"mode": 0, "ready": False}
    for call, cm in enumerate((17, 33, 33)):
        st, back, name = gh.decode_plain(codec, dv)
        assert st == 0 and _cm(name) == cm, (call, st, name)
        gh.assert_plain_decoded(back, case, f"learned order, call {call}")
        assert codec.byte_order()["ready"]
    codec.set_decoder(3)                     # a caller who chooses an organisation keeps it
    st, back, name = gh.decode_plain(codec, dv)
    assert st == 0 and _cm(name) == 17, (st, name)
    gh.assert_plain_decoded(back, case, "2-way on request")
    codec.close()
