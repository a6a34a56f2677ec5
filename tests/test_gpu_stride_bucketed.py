"""The bucketed one-model encoder pass at the strides 2, 3, 4 and 8 (lit_bucket.hip, bucket_sort_stride_kernel) behind
divans_gpu_codec_set_encode_path(c, 2) -- and, for calls without a segment list, behind "automatic": every reachable mixing value of
one stride distance (5, 6, 7 -> 2, 3, 4; 8 and above -> 8), a constant context, no mixing.  The bucket key of a position is the byte
that many places back; a segment's first positions take it from the segment's last8.  Every comparison is against the C oracle's
bytes (tests/test_stride_bucketed_cases_cpu.py guards the oracle, the premise and the shapes); the pass that ran is asserted through
divans_gpu_codec_last_encode_path, the distance through divans_gpu_codec_bucket_stride."""
import numpy as np
import pytest

import bucketed_segment_cases as bc
import gpu_harness as gh
import pyoracle as po
import segment_cases as sc
import stride_bucketed_cases as stc

pytestmark = pytest.mark.gpu
KEYS = list(stc.FAMILIES)
_PLAIN, _LISTS = {}, {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _plain(key, sources):
    """(family, product configuration, oracle configuration, streams, the oracle's bytes of every stream): computed once, never written to"""
    if key not in _PLAIN:
        import divans_amd as da
        fam = stc.FAMILIES[key]
        g, o = fam.pair(da, po)
        blocks = stc.plain_streams(fam, sources)
        _PLAIN[key] = (fam, g, o, blocks, [po.lit_encode(o, b) if b.size else np.zeros(0, np.uint8) for b in blocks])
    return _PLAIN[key]


def _lists(key, sources):
    if key not in _LISTS:
        import divans_amd as da
        fam = stc.FAMILIES[key]
        g, o = fam.pair(da, po)
        batches = stc.list_batches(fam, sources)
        _LISTS[key] = (fam, g, o, batches, {name: gh.oracle_bytes(o, streams) for name, streams in batches.items()})
    return _LISTS[key]


@pytest.mark.parametrize("key", KEYS)
def test_stride_pass_without_a_list(key, sources):
    """every length of lengths(d) in one ragged batch (odd offsets, stream 0 at offset 0): path 2 is accepted -- as the codec is
    created and after set_block_types --, reports 2 and the distance, writes the oracle's bytes; "automatic" takes the pass the case
    module records; path 1 writes the same bytes and the decoder gives the input back"""
    import torch
    import divans_amd as da
    fam, g, o, blocks, coded = _plain(key, sources)
    buf, offs, sizes = stc.ragged_layout(blocks)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_buf, d_off, d_sz = t(buf), t(offs), t(sizes)
    n, longest = len(blocks), int(sizes.max())
    assert longest == 65536
    codec = da.LiteralCodec(g, longest)
    assert codec.bucket_stride() == stc.EXPECTED_DISTANCE[key]
    codec.set_encode_path(2)
    codec.set_block_types(fam.n_btypes)
    assert codec.bucket_stride() == stc.EXPECTED_DISTANCE[key]
    codec.set_encode_path(0)
    codec.set_encode_path(2)
    assert codec.last_encode_path() == 0
    outs = codec.alloc_encode_outputs(n)
    for what, sub in (("one launch sequence", None), ("launch sequences of 7 streams", 7)):
        if sub:
            codec.set_bucket_batch(sub)
        codec.encode_batch(d_buf, n, longest, outs, in_offsets=d_off, in_sizes=d_sz)
        assert codec.status() == 0 and codec.last_encode_path() == stc.BUCKETED_PATH, what
        gh.assert_same(gh.split_outputs(outs, n), coded, None, f"path 2, {what}")
    back = torch.zeros_like(d_buf)
    codec.decode_batch(outs["out"], outs["offsets"], outs["sizes"], n, longest, back, out_offsets=d_off, out_sizes=d_sz)
    assert codec.status() == 0
    back = back.cpu().numpy()
    for i, (b, off) in enumerate(zip(blocks, offs)):
        assert (back[int(off):int(off) + b.size] == b).all(), (key, i)
    codec.set_encode_path(0)
    codec.encode_batch(d_buf, n, longest, outs, in_offsets=d_off, in_sizes=d_sz)
    assert codec.status() == 0 and codec.last_encode_path() == stc.AUTOMATIC_PATH_WITHOUT_A_LIST
    gh.assert_same(gh.split_outputs(outs, n), coded, None, "automatic")
    codec.set_encode_path(1)
    codec.encode_batch(d_buf, n, longest, outs, in_offsets=d_off, in_sizes=d_sz)
    assert codec.status() == 0 and codec.last_encode_path() == 1
    gh.assert_same(gh.split_outputs(outs, n), coded, None, "path 1")
    codec.close()


@pytest.mark.parametrize("key", KEYS)
def test_stride_pass_through_the_host_entry_point(key, sources):
    """encode_host: equal lengths, one past the first piece base by the distance"""
    import divans_amd as da
    fam, g, o, blocks, coded = _plain(key, sources)
    L = 8192 + fam.dist
    rows = [(b, c) for b, c in zip(blocks, coded) if b.size >= L][:6]
    data = np.stack([b[:L] for b, _ in rows])
    ref = [c if b.size == L else po.lit_encode(o, b[:L]) for b, c in rows]
    codec = gh.codec_for(da, fam, g, L)
    codec.set_encode_path(2)
    packed, offs, sizes = codec.encode_host(data, L)
    assert codec.status() == 0 and codec.last_encode_path() == stc.BUCKETED_PATH
    gh.assert_same([packed[int(a):int(a) + int(s)] for a, s in zip(offs, sizes)], ref, None, "encode_host")
    back = codec.decode_host(packed, offs, sizes, L)
    assert (np.asarray(back).reshape(len(rows), L) == data).all()
    codec.close()


@pytest.mark.parametrize("batch", ["existing_a", "existing_b", "stride"])
@pytest.mark.parametrize("key", KEYS)
def test_stride_pass_codes_segment_lists_bit_exact(key, batch, sources):
    import torch
    import divans_amd as da
    fam, g, o, batches, coded = _lists(key, sources)
    streams, ref = batches[batch], coded[batch]
    tin = gh.ragged_tensors(torch, streams)
    codec = gh.codec_for(da, fam, g, tin["longest"])
    assert codec.bucket_stride() == stc.EXPECTED_DISTANCE[key]
    codec.set_encode_path(2)
    outs = codec.alloc_encode_outputs(tin["n"])
    for what, sub in (("one launch sequence", None), ("launch sequences of 9 streams", 9)):
        if sub:
            codec.set_bucket_batch(sub)
        st, got, path = gh.encode_segments(codec, tin, outs)
        assert st == 0 and path == stc.BUCKETED_PATH, (what, st, path)
        gh.assert_same(got, ref, streams, what)
    gh.assert_round_trip_segments(torch, codec, tin, outs, streams, f"{key}, {batch}")
    codec.set_encode_path(0)          # automatic: a list stays on the streaming kernels
    st, got, path = gh.encode_segments(codec, tin, outs)
    assert st == 0 and path == 1, (st, path)
    gh.assert_same(got, ref, streams, "automatic, with a list")
    codec.close()


def test_stride_model_pass_matches_the_oracle_trace(sources):
    """the (start, freq) pair of every nibble straight out of the model pass on a fresh codec, against the oracle's put_start_freq
    trace: distance 3, streams that cross a piece base, one of them a constant byte"""
    import torch
    import divans_amd as da
    fam = stc.FAMILIES["m6"]
    g, o = fam.pair(da, po)
    L = 9001
    data = stc._Content(sources, np.random.default_rng(31), first=0)
    blocks = np.stack([data.take(L) for _ in range(10)])
    codec = da.LiteralCodec(g, L)
    codec.set_encode_path(2)
    pairs = codec.model_batch(torch.from_numpy(blocks).to("cuda:0"), blocks.shape[0], L)
    torch.cuda.synchronize()
    assert codec.status() == 0 and codec.last_encode_path() == stc.BUCKETED_PATH
    pairs = pairs.cpu().numpy().view(np.uint32)[:, :2 * L]
    for i in range(blocks.shape[0]):
        _, tr = po.lit_encode(o, blocks[i], trace=True)
        want = tr[:, 1].astype(np.uint32) | (tr[:, 2].astype(np.uint32) << 16)
        assert (pairs[i] == want).all(), (i, int(np.argmax(pairs[i] != want)))
    codec.close()


@pytest.mark.parametrize("name", list(stc.REFUSED))
def test_the_other_strides_stay_refused(name):
    """two models, a mask that mixes distances, a context that follows from the previous byte: no bucketed pass, distance 0"""
    import divans_amd as da
    g, _ = stc.REFUSED[name].pair(da, po)
    codec = da.LiteralCodec(g, 4096)
    assert codec.bucket_stride() == 0
    with pytest.raises(da.DivansGpuError, match="bucketed encoder needs"):
        codec.set_encode_path(2)
    codec.close()


def test_the_stride_1_codecs_report_distance_1():
    import divans_amd as da
    codec = da.LiteralCodec(da.config_simple(), 4096)
    assert codec.bucket_stride() == 1
    codec.close()
    codec = da.LiteralCodec(da.config_context_mixing(), 4096)      # two models: the pass of lit_bucket_mix.hip, not this one
    assert codec.bucket_stride() == 0
    codec.close()


@pytest.mark.parametrize("key", ["m5", "m12"])
def test_faulty_lists_are_reported_by_the_stride_pass(key, sources):
    """lists that cover too few / too many bytes, bytes without a list, an empty stream whose list holds bytes: BAD_SEGMENT as under
    stride 1, the other streams as the oracle's, and the same codec clean again afterwards"""
    import torch
    import divans_amd as da
    fam, g, o, batches, coded = _lists(key, sources)
    streams, ref = batches["existing_a"], coded["existing_a"]
    good = streams[:12]
    bad, which = sc.bad_lists(streams)
    cases = [("all three", bad, which), ("empty stream, list of 5 bytes", bc.empty_stream_with_bytes_in_its_list(good, 4), (4,)),
             ("block type outside the tables", bc.bad_btype(good, 7, fam.n_btypes), (7,))]
    tins = [gh.ragged_tensors(torch, b) for _, b, _ in cases]
    codec = gh.codec_for(da, fam, g, max(t["longest"] for t in tins))
    codec.set_encode_path(2)
    for (what, b, skip), tin in zip(cases, tins):
        st, got, path = gh.encode_segments(codec, tin)
        assert st & gh.BAD_SEGMENT and path == stc.BUCKETED_PATH, (what, st, path)
        gh.assert_same(got, ref, b, what, skip=skip)
    st, got, path = gh.encode_segments(codec, gh.ragged_tensors(torch, good))
    assert st == 0 and path == stc.BUCKETED_PATH, (st, path)
    gh.assert_same(got, ref, good, "the same streams with their lists in order")
    codec.close()
