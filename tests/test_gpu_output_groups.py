"""The decoders' output stores (lit_decode2.hip, both byte loops of decode2_body) at every alignment of the output pointer.  Written for
64-byte output groups -- a dword per lane where the group is whole and its address 4-byte aligned, bytes otherwise; measured and dropped,
DESIGN.md section 5, round 13 -- and kept for the 16-byte groups that stay: lengths around 16, 64 and 128 bytes and the chunk seam, each
at output offsets of every residue mod 4, through decode_batch(..., out_offsets, out_sizes).  The output equals the oracle's input and no
byte outside [out, out + len) is written, under the tagged and the pinned plain decoder and under mixing."""
import numpy as np
import pytest

import pyoracle as po
import plain_decoder_cases as pc

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 32767, 32769, 65536)
_CASES = {}


def _layout(streams):
    """stream k at an offset = k mod 4 (mod 4), at least 5 sentinel bytes between streams and pc.TAIL behind"""
    offs, cur = [], 3
    for k, lit in enumerate(streams):
        cur += 5
        cur += (k - cur) % 4
        offs.append(cur); cur += lit.size
    blank = np.full(cur + pc.TAIL, pc.SENTINEL, np.uint8)
    buf = blank.copy()
    for o, lit in zip(offs, streams):
        buf[o:o + lit.size] = lit
    return buf, blank, np.array(offs, np.int64), np.array([s.size for s in streams], np.int32)


def _case(cfg_name, corpus):
    if cfg_name not in _CASES:
        ocfg = po.config_simple() if cfg_name == "simple" else po.config_context_mixing()
        streams = [corpus[977 * k:977 * k + n].copy() for k, n in enumerate(n for n in LENGTHS for _ in range(4))]
        buf, blank, offs, sizes = _layout(streams)
        assert [int(o) % 4 for o in offs] == [k % 4 for k in range(len(streams))]
        assert all({int(o) % 4 for o, s in zip(offs, sizes) if s == n} == {0, 1, 2, 3} for n in LENGTHS)
        coded = [po.lit_encode(ocfg, s) for s in streams]
        _CASES[cfg_name] = dict(streams=streams, lit=(buf, blank, offs, sizes), cod=pc.coded_layout(coded))
    return _CASES[cfg_name]


def _decode_and_check(torch, codec, case, what):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf, blank, offs, sizes = case["lit"]
    cbuf, coffs, csizes = case["cod"]
    back = t(blank)
    assert back.data_ptr() % 4 == 0
    codec.decode_batch(t(cbuf), t(coffs), t(csizes), len(sizes), int(sizes.max()), back, out_offsets=t(offs), out_sizes=t(sizes))
    st, name = codec.status(), codec.last_decode_kernel()
    assert st == 0, (what, st, name)
    back = back.cpu().numpy()
    for i, (lit, off) in enumerate(zip(case["streams"], offs)):
        got = back[int(off):int(off) + lit.size]
        assert (got == lit).all(), f"{what}: stream {i} ({lit.size} bytes at offset {int(off)} = {int(off) % 4} mod 4) decoded wrong from byte {int(np.argmax(got != lit))} ({name})"
    wrong = np.flatnonzero(back != buf)
    assert wrong.size == 0, f"{what}: sentinel byte {int(wrong[0]) if wrong.size else -1} of {buf.size} written to ({name})"
    return name


def test_plain_decoder_every_length_at_every_alignment(corpus):
    import torch
    import divans_amd as da
    case = _case("simple", corpus)
    codec = da.LiteralCodec(da.config_simple(), 65536)
    codec.set_byte_order(2)
    for what, mode, cm in (("tagged caches", 1, ", 1>"), ("pinned rows", 2, ", 33>")):
        codec.set_high_row_pinning(mode)
        name = _decode_and_check(torch, codec, case, what)
        assert "lit_decode2_kernel_w7<4, true, false, false" in name and name.endswith(cm), (what, name)
    codec.set_geometry(blocks=1)        # 60 streams on 16 groups: a group's next stream starts at another alignment
    for what, mode, cm in (("tagged caches, one workgroup", 1, ", 17>"), ("pinned rows, one workgroup", 2, ", 33>")):
        codec.set_high_row_pinning(mode)
        name = _decode_and_check(torch, codec, case, what)
        assert name.endswith(cm), (what, name)
    codec.close()


def test_mixing_decoder_every_length_at_every_alignment(corpus):
    import torch
    import divans_amd as da
    case = _case("mixing", corpus)
    codec = da.LiteralCodec(da.config_context_mixing(), 65536)
    name = _decode_and_check(torch, codec, case, "library's choice")
    assert "lit_decode2_kernel" in name and ", true, false, " in name, name
    codec.set_geometry(blocks=1)
    _decode_and_check(torch, codec, case, "one workgroup")
    codec.close()
