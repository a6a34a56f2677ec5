"""The rANS pass by itself (rans_encode_kernel, rans_encode2_kernel, rans_encode2_split_kernel, rans_stitch_kernel) on the directed
batches of tests/rans_pass_cases.py, through divans_gpu_selftest_rans_batch -- the launcher and the RansBatch the encode entry points
use -- against the C oracle's ANSEncoder (orc_ans_encode_pairs; tests/test_rans_pass_cases_cpu.py guards it), bit for bit.

For every batch and every kernel variant it lists: sizes, offsets, per-chunk sizes and bytes are the oracle's stream by stream; every
stream ends at its slot's end; every byte of the output area that belongs to no stream -- the room in front of a stream in its slot
and both guard zones -- still holds the value the area was filled with; the status word is 0; and the variants agree byte for byte.
An empty stream reports size 0 at its slot's end under all three."""
import numpy as np
import pytest

import pyoracle as po
import rans_pass_cases as rc

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def codec():
    import divans_amd as da
    c = da.LiteralCodec(da.config_simple(), 4096)
    yield c
    c.close()


def check_against_oracle(b, impl, got, ref):
    """`got` = what selftest_rans_batch returned for batch b under impl; ref = [(bytes, chunk sizes)] per stream.  Returns the streams' bytes."""
    n = len(b.sizes); slot, guard, area = got["slot"], got["guard"], got["area"]
    tag = (b.name, impl)
    assert got["status"] == 0, tag
    assert area.size == 2 * guard + n * slot
    ref_sizes = np.array([c.size for c, _ in ref], dtype=np.int64)
    assert (got["sizes"].astype(np.int64) == ref_sizes).all(), (tag, np.flatnonzero(got["sizes"] != ref_sizes)[:8])
    # right-aligned: a stream ends where its slot ends, and the offsets carry out_base
    rel = got["offsets"].astype(np.int64) - b.out_base
    slot_end = (np.arange(n, dtype=np.int64) + 1) * slot
    assert (rel + ref_sizes == slot_end).all(), (tag, np.flatnonzero(rel + ref_sizes != slot_end)[:8])
    untouched = np.ones(area.size, dtype=bool)
    streams = []
    for i, (coded, chunks) in enumerate(ref):
        lo = guard + int(rel[i]); hi = lo + coded.size
        untouched[lo:hi] = False
        mine = area[lo:hi]
        if not np.array_equal(mine, coded):
            at = int(np.flatnonzero(mine != coded)[0])
            raise AssertionError(f"{tag}: stream {i} ({b.patterns[i]}, {int(b.sizes[i])} bytes) differs from the oracle at coded byte {at} of {coded.size}")
        want = chunks + [0] * (got["chunk_bytes"].shape[1] - len(chunks))
        assert got["chunk_bytes"][i].tolist() == want, (tag, i, got["chunk_bytes"][i].tolist(), want)
        streams.append(mine)
    stray = np.flatnonzero(untouched & (area != FILL))
    assert stray.size == 0, f"{tag}: {stray.size} bytes outside the streams were written, first at area byte {int(stray[0])} (guard {guard}, slot {slot})"
    return streams


@pytest.mark.parametrize("name", rc.NAMES)
def test_rans_kernels_equal_the_oracle_and_write_nothing_else(codec, name):
    b = rc.batch(name)
    ref = [po.ans_encode_pairs(rc.stream_pairs(b, i)) for i in range(len(b.sizes))]
    first = None
    for impl in b.impls:
        got = codec.selftest_rans_batch(impl, b.pairs, b.sizes, out_base=b.out_base, fill=FILL)
        streams = check_against_oracle(b, impl, got, ref)
        assert codec.status() == 0
        if first is None:
            first = (got, streams)
        else:       # the kernel variants agree with each other in everything they report
            assert np.array_equal(got["offsets"], first[0]["offsets"]) and np.array_equal(got["sizes"], first[0]["sizes"])
            assert np.array_equal(got["chunk_bytes"], first[0]["chunk_bytes"]) and np.array_equal(got["area"], first[0]["area"]), (name, impl)
    empty = np.flatnonzero(b.sizes == 0)
    got0 = first[0]
    assert (got0["sizes"][empty] == 0).all()
    assert (got0["offsets"][empty].astype(np.int64) == b.out_base + (empty + 1) * got0["slot"]).all()


@pytest.mark.parametrize("impl", rc.ALL_IMPLS)
@pytest.mark.parametrize("kind", sorted(rc.BAD_PAIRS))
def test_a_pair_outside_the_domain_is_reported_and_leaves_the_codec_usable(codec, kind, impl):
    import divans_amd as da
    good, bad = rc.bad_batch(kind)
    with pytest.raises(da.DivansGpuError, match=r"\(-1\).*invalid \(start,freq\) pair"):        # DIVANS_GPU_EINVAL
        codec.selftest_rans_batch(impl, bad.pairs, bad.sizes, fill=FILL)
    assert codec.status() == 0                                  # the entry cleared the word
    ref = [po.ans_encode_pairs(rc.stream_pairs(good, i)) for i in range(len(good.sizes))]
    got = codec.selftest_rans_batch(impl, good.pairs, good.sizes, fill=FILL)
    check_against_oracle(good, impl, got, ref)
    assert codec.status() == 0


def test_entry_refuses_what_the_chunk_parallel_kernels_cannot_take(codec):
    import divans_amd as da
    pairs = np.full((1, 2 * 65537 + 2), rc.word(0, 32767), dtype=np.uint32)
    for impl in (1, 2):
        with pytest.raises(da.DivansGpuError, match=r"\(-1\)"):
            codec.selftest_rans_batch(impl, pairs, [65537])
    with pytest.raises(da.DivansGpuError, match=r"\(-1\)"):         # sf_stride not a multiple of 4
        codec.selftest_rans_batch(0, pairs[:, :6], [3])
    with pytest.raises(da.DivansGpuError, match=r"\(-1\)"):         # rows shorter than the longest stream
        codec.selftest_rans_batch(0, pairs[:, :8], [5])
    with pytest.raises(da.DivansGpuError, match=r"\(-1\)"):
        codec.selftest_rans_batch(3, pairs[:, :8], [4])
    assert codec.status() == 0
