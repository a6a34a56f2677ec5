"""The pack pass by itself: scan_sizes_kernel (one block; above 1024 streams every thread scans several sizes) and pack_copy_kernel.

* divans_gpu_pack_streams on synthetic slots against a few lines of numpy -- an exclusive prefix sum of the sizes rounded up to 4,
  then a copy -- at stream counts on both sides of 1024 and of its multiples, with sizes of every residue modulo 4 and empty streams.
* divans_gpu_lit_encode_packed on 2500 ragged streams with sub-batches that cross `accumulate` with several sizes per thread and a
  partial last sub-batch, every stream against the C oracle, offsets and total against the same numpy scan, and one call whose buffer
  ends inside the second sub-batch."""
import numpy as np
import pytest

import pyoracle as po

pytestmark = pytest.mark.gpu
SENTINEL = 0xEE
# What the outputs hold before a call.  An offset or size the kernels fail to write then still names a place inside the buffer: the
# offsets start out at the end of the packed streams (where no non-empty stream belongs), with TAIL sentinel bytes behind it -- more
# than the longest stream of these tests -- and the sizes at a value no coded stream has.
TAIL, STALE_SIZE = 512, 4


def numpy_scan(sizes):
    """(exclusive prefix sum of the sizes rounded up to 4, its total)"""
    rounded = (np.asarray(sizes, dtype=np.int64) + 3) & ~3
    ends = np.cumsum(rounded)
    return ends - rounded, int(ends[-1]) if len(ends) else 0


@pytest.fixture(scope="module")
def codec():
    import divans_amd as da
    c = da.LiteralCodec(da.config_simple(), 64)
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2047, 2049, 3000, 5000])
def test_pack_streams_equals_a_numpy_scan_and_copy(codec, n):
    import torch
    dev = torch.device("cuda")
    rng = np.random.default_rng(1000 + n)
    sizes = rng.integers(0, 201, n).astype(np.int32)
    if n >= 8:
        sizes[:8] = [0, 1, 2, 3, 4, 5, 6, 7]
        sizes[-4:] = [199, 198, 0, 197]                 # the last stream's rounding is part of the total
        assert (sizes == 0).sum() >= 2 and set(int(s) % 4 for s in sizes) == {0, 1, 2, 3} and sizes.max() <= 200
    # the slots: the streams in a shuffled order at 4-byte aligned places, room for the rounded-up read of each, gaps in between
    order = rng.permutation(n)
    room = ((sizes[order].astype(np.int64) + 3) & ~3) + 4 * rng.integers(0, 4, n)
    begin = np.cumsum(room) - room
    src_off = np.empty(n, dtype=np.int64); src_off[order] = begin
    slots = rng.integers(0, 256, int(room.sum()) + 16, dtype=np.uint8)
    assert (src_off % 4 == 0).all() and (src_off + ((sizes + 3) & ~3) <= slots.size).all()
    ref_off, ref_total = numpy_scan(sizes)
    outputs = {"out": torch.from_numpy(slots).to(dev), "offsets": torch.from_numpy(src_off).to(dev), "sizes": torch.from_numpy(sizes).to(dev)}
    packed = torch.full((ref_total + TAIL,), SENTINEL, dtype=torch.uint8, device=dev)
    poff = torch.full((n,), ref_total, dtype=torch.int64, device=dev); total = torch.full((1,), -1, dtype=torch.int64, device=dev)
    codec.pack_into(outputs, n, packed, poff, total)
    assert codec.status() == 0
    got_off = poff.cpu().numpy(); got = packed.cpu().numpy()
    assert int(total.item()) == ref_total, (n, int(total.item()), ref_total)
    assert np.array_equal(got_off, ref_off), (n, np.flatnonzero(got_off != ref_off)[:8])
    for i in range(n):
        s = int(sizes[i])
        assert np.array_equal(got[ref_off[i]:ref_off[i] + s], slots[src_off[i]:src_off[i] + s]), (n, i, s)
    assert (got[ref_total:] == SENTINEL).all()          # nothing behind the last stream's rounded-up end


N_PACKED, L_PACKED = 2500, 64
_PACKED_REF = {}


def packed_reference(cfg_name, corpus):
    """(blocks, lengths, the oracle's coded streams, their numpy scan, the packed image): computed once per configuration, never written to"""
    if cfg_name not in _PACKED_REF:
        rng = np.random.default_rng(77)
        lens = rng.integers(0, L_PACKED + 1, N_PACKED).astype(np.int32)
        lens[[0, 1023, 1024, 1099, 1100, N_PACKED - 1]] = [L_PACKED, 0, 1, L_PACKED, 0, 63]
        blocks = np.stack([np.resize(corpus[97 * i:97 * i + L_PACKED], L_PACKED) for i in range(N_PACKED)])
        noisy = rng.integers(0, N_PACKED, 300)
        blocks[noisy] = rng.integers(0, 256, (noisy.size, L_PACKED), dtype=np.uint8)
        ocfg = po.config_simple() if cfg_name == "simple" else po.config_context_mixing()
        coded = [po.lit_encode(ocfg, blocks[i, :lens[i]]) for i in range(N_PACKED)]
        sizes = np.array([c.size for c in coded], dtype=np.int32)
        off, total = numpy_scan(sizes)
        image = np.zeros(total, dtype=np.uint8)
        for c, o in zip(coded, off):
            image[o:o + c.size] = c
        assert (sizes % 4 == 0).all()           # coded streams are whole words: the image has no gaps
        _PACKED_REF[cfg_name] = (blocks, lens, sizes, off, total, image)
    return _PACKED_REF[cfg_name]


@pytest.fixture(scope="module", params=["simple", "mixing"])
def packed_setup(request, corpus):
    import torch
    import divans_amd as da
    dev = torch.device("cuda")
    blocks, lens, sizes, off, total, image = packed_reference(request.param, corpus)
    cfg = da.config_simple() if request.param == "simple" else da.config_context_mixing()
    c = da.LiteralCodec(cfg, L_PACKED)
    d_in = torch.from_numpy(np.concatenate([blocks.reshape(-1), np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.arange(N_PACKED, dtype=torch.int64, device=dev) * L_PACKED
    d_sz = torch.from_numpy(lens).to(dev)
    yield c, d_in, d_off, d_sz, sizes, off, total, image
    c.close()


@pytest.mark.parametrize("sub", [0, 1100, 1024, 1025, 2500])
def test_encode_packed_equals_the_oracle_and_the_numpy_scan(packed_setup, sub):
    import torch
    c, d_in, d_off, d_sz, ref_sizes, ref_off, ref_total, image = packed_setup
    dev = d_in.device
    packed = torch.full((ref_total + TAIL,), SENTINEL, dtype=torch.uint8, device=dev)
    poff = torch.full((N_PACKED,), ref_total, dtype=torch.int64, device=dev); sizes = torch.full((N_PACKED,), STALE_SIZE, dtype=torch.int32, device=dev)
    total = torch.full((1,), -1, dtype=torch.int64, device=dev)
    c.encode_packed(d_in, N_PACKED, L_PACKED, packed, poff, sizes, total, in_offsets=d_off, in_sizes=d_sz, sub_batch=sub)
    assert c.status() == 0
    got_sizes = sizes.cpu().numpy(); got_off = poff.cpu().numpy(); got = packed.cpu().numpy()
    assert np.array_equal(got_sizes, ref_sizes), (sub, np.flatnonzero(got_sizes != ref_sizes)[:8])
    assert int(total.item()) == ref_total, (sub, int(total.item()), ref_total)
    assert np.array_equal(got_off, ref_off), (sub, np.flatnonzero(got_off != ref_off)[:8])
    for i in range(N_PACKED):
        o, s = int(ref_off[i]), int(ref_sizes[i])
        assert np.array_equal(got[o:o + s], image[o:o + s]), (sub, i)
    assert (got[ref_total:] == SENTINEL).all()


def test_encode_packed_into_a_buffer_that_ends_inside_the_second_sub_batch(packed_setup):
    import torch
    c, d_in, d_off, d_sz, ref_sizes, ref_off, ref_total, image = packed_setup
    dev = d_in.device
    sub = 1100
    cap = int(ref_off[1700]) + 2                      # inside sub-batch 1 (streams 1100 .. 2199), inside a stream's first word
    ends = ref_off + ((ref_sizes.astype(np.int64) + 3) & ~3)
    fit = int(np.flatnonzero(ends > cap)[0])        # the first stream that does not fit
    assert sub < fit < 2 * sub and ref_sizes[fit] > 0
    packed = torch.full((ref_total + TAIL,), SENTINEL, dtype=torch.uint8, device=dev)
    poff = torch.full((N_PACKED,), ref_total, dtype=torch.int64, device=dev); sizes = torch.full((N_PACKED,), STALE_SIZE, dtype=torch.int32, device=dev)
    total = torch.full((1,), -1, dtype=torch.int64, device=dev)
    rc = c._lib.divans_gpu_lit_encode_packed(c._h, d_in.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), L_PACKED, N_PACKED, packed.data_ptr(), cap,
                                             poff.data_ptr(), sizes.data_ptr(), total.data_ptr(), sub)
    assert rc == 0
    assert c.status() & 8                           # DIVANS_GPU_STATUS_OUTPUT_FULL
    # sizes, offsets and total still say what was needed
    assert np.array_equal(sizes.cpu().numpy(), ref_sizes) and np.array_equal(poff.cpu().numpy(), ref_off) and int(total.item()) == ref_total
    got = packed.cpu().numpy()
    first_out = int(ref_off[fit])
    assert np.array_equal(got[:first_out], image[:first_out])         # everything before the first stream that did not fit is intact
    assert (got[first_out:] == SENTINEL).all()                        # and no later stream was written, inside the buffer or behind it
    assert c.status() == 0
