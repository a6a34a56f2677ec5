"""The calls WITHOUT a segment list on every SEG = false instance of lit_decode2_kernel: each (MM, CTXC, MIX) family of
tests/segment_cases.py decodes one batch of 34 streams (tests/plain_decoder_cases.py) from the C ORACLE's bytes under every cache set
the dispatch holds -- none, the high rows, the high and the low rows; direct mapped and 2-way -- on grids of two and of one workgroup,
and the kernel instance that ran is asserted from its name.  The batch has streams around the 16-byte output group, streams whose CODED
size is exactly 15 .. 49 words (the refill points of the LDS word ring), the 32 768-byte chunk seam, the empty stream, two streams that
keep a handful of rows busy; coded streams start at every 4-byte offset of a 16-byte line, literal offsets at every alignment, with
sentinel bytes between and behind.  On one workgroup every resident group decodes two or three streams in a row (the per-stream reset
of the four caches and of the ring).  The families with a context map and eight block types have low-nibble rows above 16 383: the
upper tag bits of the caches.

The same batch goes through the list-free encoders (both model passes where the family has a bucketed one), and one 70 000-byte stream
per family through the call-by-call interface, cut so that last_8_literals is assembled over several pieces -- bit for bit against the
oracle (tests/test_plain_decoder_cases_cpu.py guards the oracle on the same streams).

The one omission: a table of more than 32 766 rows per stream has no row caches (the `_nocache` families decode without)."""
import re

import numpy as np
import pytest

import gpu_harness as gh
import plain_decoder_cases as pc
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
_CASES = {}
_SEEN = {}          # template arguments of every asserted lit_decode2_kernel instance -> the family that ran it first
_RAN = set()
_NAME = re.compile(r"lit_decode2_kernel_\w+<(-?\d+), (true|false), (true|false), (true|false), (\d+)>")
# (label, rows, shifts, index into the CM value pairs below)
CACHE_SETS = (("no caches", (0, 0, 0, 0), (5, 5, 5, 5), 0),
              ("high rows, tiny", (4, 4, 0, 0), (5, 5, 5, 5), 1),
              ("all four, tiny", (4, 4, 4, 4), (0, 1, 2, 3), 2),
              ("all four, medium", (64, 8, 32, 64), (8, 31, 4, 5), 2))
# the CM template value of (none, high rows, high + low rows): [mixing][generation]
CM_VALUES = {False: {2: (0, 1, 5), 3: (0, 17, 21)}, True: {2: (0, 3, 11), 3: (0, 19, 27)}}
# the model pass set_encode_path(2) selects for a call without a list; every other family is refused (streaming kernels only):
# a constant context under mixing value 4 without mixing, one block type under dynamic mixing, the context-keyed rows of mixing value 0
BUCKETED_PATH = {"mm4_const_plain": 2, "mm4_map_mix_bt1": 3, "mm0_map_plain": 2, "mm0_map_mix": 3}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(fam, sources):
    """the family's configurations, its batch, the oracle's bytes and both layouts: computed once, shared, never written to"""
    if fam.name not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        o0 = pc.oracle_config(fam, o)
        streams = pc.shapes(fam, sources)
        coded = pc.oracle_bytes(o0, streams)
        _CASES[fam.name] = dict(g=g, o=o, o0=o0, streams=streams, coded=coded, lit=pc.literal_layout(streams), cod=pc.coded_layout(coded))
    return _CASES[fam.name]


def _codec(da, fam, case):
    codec = da.LiteralCodec(case["g"], int(case["lit"][3].max()))
    if fam.n_btypes > 1:        # one block type: the codec keeps the table of the configuration's own
        codec.set_block_types(fam.n_btypes)
    return codec


def _assert_kernel(fam, what, name, cmv=None):
    """lit_decode2_kernel_*<MM, CTXC, MIX, false, CMV>; cmv None: non-zero exactly when the family's table admits row caches"""
    m = _NAME.search(name)
    assert m, (what, name)
    mm, ctxc, mix, seg, got = int(m.group(1)), m.group(2) == "true", m.group(3) == "true", m.group(4) == "true", int(m.group(5))
    assert (mm, ctxc, mix, seg) == (fam.mm if fam.mm >= 0 else -1, fam.ctxc, fam.mix, False), (what, name)
    if cmv is None:
        assert (got != 0) == fam.cached, (what, name)
    else:
        assert got == cmv, (what, name, cmv)
        _SEEN.setdefault(m.group(0)[m.group(0).index("<"):], fam.name)


def _generation_chain(da, fam, gen):
    """[(label, setup(codec), CM value the name must show or None)]: the launch the library shapes by itself, then every cache set on
    two workgroups and on one"""
    chain = [("library's choice, 2 workgroups", lambda c: c.set_geometry(blocks=2), None)]
    for blocks in (2, 1):
        for label, rows, shifts, k in CACHE_SETS:
            if any(rows) and not fam.cached:
                continue
            chain.append((f"generation {gen}, {label}, {blocks} workgroup{'s' if blocks > 1 else ''}",
                          lambda c, rows=rows, shifts=shifts, blocks=blocks: c.set_decoder(gen, rows, shifts, blocks=blocks), CM_VALUES[fam.mix][gen][k]))
    return chain


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_decode_oracle_bytes_on_every_cache_set(fam, sources):
    """one codec per generation (2: direct mapped, 3: 2-way), its settings applied one after the other, so that the tables and the LDS
    layout are also reused from launch to launch.  Generation 1 exists in experiment builds only: a default build does not run its
    chain.  No row cache exists above 32 766 rows per stream: there set_decoder refuses rows and only the launches without run."""
    import torch
    import divans_amd as da
    case = _case(fam, sources)
    dv = gh.plain_device(torch, case)
    for gen in (2, 3):
        assert gen in da.decoder_generations()
        codec = _codec(da, fam, case)
        if not fam.cached:
            with pytest.raises(da.DivansGpuError, match="row caches need fewer than 32767 rows"):
                codec.set_decoder(gen, (4, 4, 4, 4), (0, 1, 2, 3), blocks=2)
            codec.close()
            codec = _codec(da, fam, case)      # (the refused call has already left the library's choice of organisation)
        for what, setup, cmv in _generation_chain(da, fam, gen):
            setup(codec)
            st, back, name = gh.decode_plain(codec, dv)
            assert st == 0, (what, st, name)
            _assert_kernel(fam, what, name, cmv)
            gh.assert_plain_decoded(back, case, what)
        codec.close()
    for chain in gh.decoder_chains(da, fam):
        if chain[0][2] != 1:
            continue
        codec = _codec(da, fam, case)
        for what, setup, _ in chain:
            setup(codec)
            st, back, name = gh.decode_plain(codec, dv)
            assert st == 0, (what, st, name)
            cache = 2 if fam.cached and "no cache" not in what else 0
            assert f"lit_decode_kernel<{fam.mm if fam.mm >= 0 else -1}, {gh.tf(fam.ctxc)}, {gh.tf(fam.mix)}, {cache}, false>" in name, (what, name)
            gh.assert_plain_decoded(back, case, what)
        codec.close()
    _RAN.add(fam.name)


def test_every_list_free_instance_was_asserted():
    """12 triples x 5 cache sets: the 60 SEG = false instances of lit_decode2_kernel_*.  Follows from the families and the chain; where
    the cases above all ran in this session the names they asserted are compared with it (and printed: pytest -s)."""
    want = set()
    for fam in sc.FAMILIES:
        if fam.cached:
            for gen in (2, 3):
                for cmv in CM_VALUES[fam.mix][gen]:
                    want.add(f"<{fam.mm if fam.mm >= 0 else -1}, {'true' if fam.ctxc else 'false'}, {'true' if fam.mix else 'false'}, false, {cmv}>")
    assert len(want) == 60
    assert set(_SEEN) <= want
    if _RAN == {f.name for f in sc.FAMILIES}:
        assert set(_SEEN) == want, sorted(want - set(_SEEN))
        for args in sorted(_SEEN, key=lambda a: [int(x) if x.lstrip("-").isdigit() else x for x in a[1:-1].split(", ")]):
            print(f"lit_decode2_kernel_*{args}  ({_SEEN[args]})")


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_encoders_write_the_oracles_bytes(fam, sources):
    """encode_batch on the streaming kernels and, where the family has one, on its bucketed pass; 32 resident groups for 34 streams, so
    two groups of the streaming kernels code a second stream"""
    import torch
    import divans_amd as da
    case = _case(fam, sources)
    dv = gh.plain_device(torch, case)
    codec = _codec(da, fam, case)
    codec.set_geometry(blocks=2)
    for ask in (1, 2):
        want = 1 if ask == 1 else BUCKETED_PATH.get(fam.name)
        if want is None:
            with pytest.raises(da.DivansGpuError, match="bucketed encoder needs"):
                codec.set_encode_path(ask)
            continue
        codec.set_encode_path(ask)
        outs = codec.alloc_encode_outputs(dv["n"])
        codec.encode_batch(dv["lit"], dv["n"], dv["longest"], outs, in_offsets=dv["off"], in_sizes=dv["sz"])
        st, ran = codec.status(), codec.last_encode_path()
        assert st == 0 and ran == want, (f"path {ask}", st, ran)
        out = outs["out"].cpu().numpy(); offs = outs["offsets"].cpu().numpy(); sz = outs["sizes"].cpu().numpy()
        for i, ((name, lit), ref) in enumerate(zip(case["streams"], case["coded"])):
            got = out[int(offs[i]):int(offs[i]) + int(sz[i])]
            assert int(sz[i]) == ref.size, f"path {ask}: stream {i} ({name}, {lit.size} bytes) has {int(sz[i])} coded bytes, the oracle {ref.size}"
            assert (got == ref).all(), f"path {ask}: stream {i} ({name}, {lit.size} bytes) differs from the oracle from coded byte {int(np.argmax(got != ref))}"
        assert int(sz[pc.ORDER.index("EMPTY")]) == 0
    codec.close()


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_streams_resumed_piece_by_piece(fam, sources):
    """divans_gpu_lit_stream_*: tables, Weights and last_8_literals resumed from call to call under every family (strides up to 8 look
    back over the piece boundaries at 1, 2, 3, 7, 8, 9, 10 and 17 bytes).  No set_block_types: the configuration's own block type."""
    import divans_amd as da
    case = _case(fam, sources)
    data, cuts = pc.resumed_stream(sources)
    ref = po.lit_encode(case["o"], data)
    codec = da.LiteralCodec(case["g"], 65536)
    coded, sizes = codec.stream_encode_pieces([data[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    assert coded.size == ref.size, (coded.size, ref.size)
    assert (coded == ref).all(), f"coded byte {int(np.argmax(coded != ref))} differs from the oracle"
    assert sum(sizes) == coded.size and len(sizes) == (2 * data.size + 65535) // 65536
    for per_call in (1, 2):
        back, used = codec.stream_decode_chunks(ref, data.size, chunks_per_call=per_call)
        assert (back == data).all(), f"{per_call} chunks per call: decoded wrong from byte {int(np.argmax(back != data))}"
        assert used == ref.size, (per_call, used, ref.size)
    # and again on the same codec: a new stream starts from fresh tables
    ref2 = po.lit_encode(case["o"], data[:40000])
    coded2, _ = codec.stream_encode_pieces([data[:5000], data[5000:5001], data[5001:40000]])
    assert coded2.size == ref2.size and (coded2 == ref2).all()
    back2, used2 = codec.stream_decode_chunks(ref2, 40000)
    assert used2 == ref2.size and (back2 == data[:40000]).all()
    codec.close()
