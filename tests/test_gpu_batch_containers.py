"""many complete streams per call with the CMD coders / framing on host threads overlapped with the
LIT coders on the GPU (include/divans_batch.h).  Every container must be byte-identical to the per-stream ABI's and the oracle's."""
import numpy as np
import pytest

import pyoracle as po

pytestmark = pytest.mark.gpu


def test_batch_containers_equal_per_stream_abi_and_oracle(corpus):
    import divans_amd as da
    import workload
    import ffi_harness as fh
    lib = fh.product_library()
    rng = np.random.default_rng(5)
    sizes = [0, 1, 15, 16, 4097, 65536, 70001, 200000] + [int(x) for x in rng.integers(1, 90000, size=24)]
    blocks = workload.make_blocks(corpus, 100, len(sizes), block_len=65536)
    inputs = [np.resize(blocks[i], s) if s <= 65536 else np.concatenate([blocks[i], corpus[:s - 65536]]) for i, s in enumerate(sizes)]
    for opts, ffi_opts, orc in ((dict(), [(5, 0)], dict()),
                                (dict(dynamic_context_mixing=2, force_stride=0, window_size=16), [(5, 0), (4, 2), (9, 0), (2, 16)],
                                 dict(dynamic_context_mixing=2, force_stride=0, window_size=16))):
        containers, timing = da.batch_compress(inputs, da.batch_options(host_threads=4, **opts))
        assert timing["total_ms"] > 0 and timing["host_overlapped_ms"] >= 0
        for i in (0, 1, 3, 4, 5, 6, 7, 11, 20, 31):
            ref = po.stream_compress_raw(inputs[i], po.stream_options(call_buffer_size=65536, **orc), call_inputs=[inputs[i].size])
            assert containers[i].size == ref.size and (containers[i] == ref).all(), (i, sizes[i])
        for i in (2, 5, 6, 9):
            assert (containers[i] == fh.ffi_compress(lib, inputs[i], ffi_opts)).all()
        back, t2 = da.batch_decompress(containers, sum(sizes), da.batch_options(host_threads=4))
        for i, x in enumerate(inputs):
            assert back[i].size == x.size and (back[i] == x).all(), i
        assert (fh.ffi_decompress(lib, containers[7], sizes[7]) == inputs[7]).all()


def test_batch_decompress_groups_configurations_and_rejects_damage(corpus):
    import divans_amd as da
    a, _ = da.batch_compress([corpus[:30000], corpus[40000:45000]], da.batch_options())
    b, _ = da.batch_compress([corpus[100:20100]], da.batch_options(dynamic_context_mixing=2, force_stride=0))
    mixed = [a[0], b[0], a[1]]
    back, _ = da.batch_decompress(mixed, 30000 + 20000 + 5000, da.batch_options())
    assert (back[0] == corpus[:30000]).all() and (back[1] == corpus[100:20100]).all() and (back[2] == corpus[40000:45000]).all()
    bad = a[0].copy(); bad[bad.size // 2] ^= 0x10
    with pytest.raises(da.DivansGpuError):
        da.batch_decompress([a[1], bad], 40000, da.batch_options())
    with pytest.raises(da.DivansGpuError):
        da.batch_decompress([a[1], bad], 40000, da.batch_options(skip_crc=1))


def test_batch_one_long_stream_among_many_short_ones(corpus):
    # length classes + slices: a 3 MB stream next to 1500 short ones neither sizes the whole batch by its length nor switches
    # the bucketed encoder off for the others; several slices per class exercise the lane pipeline
    import divans_amd as da
    import workload
    rng = np.random.default_rng(17)
    blocks = workload.make_blocks(corpus, 7, 1500, block_len=8192)
    lens = rng.integers(1, 8193, size=1500)
    inputs = [blocks[i, :lens[i]] for i in range(1500)]
    big = np.resize(corpus, 3 * 1024 * 1024 + 17)
    inputs.insert(700, big)
    inputs.insert(3, np.resize(corpus[50000:], 150000))
    containers, timing = da.batch_compress(inputs, da.batch_options(host_threads=4))
    assert timing["host_overlapped_ms"] > 0
    for i in (0, 3, 4, 699, 700, 701, 1501):
        ref = po.stream_compress_raw(inputs[i], po.stream_options(call_buffer_size=65536), call_inputs=[inputs[i].size])
        assert containers[i].size == ref.size and (containers[i] == ref).all(), i
    back, _ = da.batch_decompress(containers, sum(x.size for x in inputs), da.batch_options(host_threads=4))
    for i, x in enumerate(inputs):
        assert back[i].size == x.size and (back[i] == x).all(), i


def test_batch_decompress_names_the_damaged_stream(corpus):
    # a LIT stream whose damage passes framing (skip_crc) is caught by the decoder's integrity check, and the call says which one
    import divans_amd as da
    inputs = [corpus[k * 5000:k * 5000 + 4000 + k] for k in range(40)]
    containers, _ = da.batch_compress(inputs, da.batch_options())
    bad = [c.copy() for c in containers]
    bad[23][bad[23].size // 2] ^= 0x04
    with pytest.raises(da.DivansGpuError) as ei:
        da.batch_decompress(bad, sum(x.size for x in inputs), da.batch_options(skip_crc=1))
    assert "23" in str(ei.value)


def test_batch_decompress_with_damaged_containers_in_bulk(corpus):
    """containers are untrusted input: 240 batches of 6 containers with one or two of them damaged (bit flips, overwritten / deleted /
    inserted spans, truncation, a splice with another container), with and without the CRC check.  Every call either refuses the
    batch -- naming a container that really was damaged -- or, when the damage was harmless, returns exactly the original bytes."""
    import re
    import divans_amd as da
    rng = np.random.default_rng(23)
    inputs = [corpus[k * 7000:k * 7000 + 3000 + 211 * k] for k in range(6)]
    total = sum(x.size for x in inputs)
    sets = [da.batch_compress(inputs, da.batch_options())[0],
            da.batch_compress(inputs, da.batch_options(dynamic_context_mixing=2, force_stride=0))[0]]
    refused = accepted = 0
    for it in range(240):
        cs = [c.copy() for c in sets[it & 1]]
        victims = sorted(set(int(v) for v in rng.integers(0, 6, size=1 + (it % 3 == 0))))
        for v in victims:
            c = cs[v]
            at = int(rng.integers(0, min(c.size, 64))) if rng.integers(0, 4) == 0 else int(rng.integers(0, c.size))
            kind = int(rng.integers(0, 6))
            if kind == 0:
                c[at] ^= np.uint8(1 << int(rng.integers(0, 8)))
            elif kind == 1:
                m = min(c.size - at, int(rng.integers(1, 32))); c[at:at + m] = rng.integers(0, 256, m, dtype=np.uint8)
            elif kind == 2:
                c = c[:at].copy()
            elif kind == 3:
                m = min(c.size - at, int(rng.integers(1, 300))); c = np.concatenate([c[:at], c[at + m:]])
            elif kind == 4:
                c = np.concatenate([c[:at], rng.integers(0, 256, int(rng.integers(1, 64)), dtype=np.uint8), c[at:]])
            else:
                other = sets[it & 1][(v + 1) % 6]
                c = np.concatenate([c[:at], other[int(rng.integers(0, other.size)):]])
            cs[v] = np.ascontiguousarray(c) if c.size else np.zeros(1, np.uint8)[:0]
        try:
            back, _ = da.batch_decompress(cs, total + (1 << 16), da.batch_options(skip_crc=int(rng.integers(0, 2))))
        except da.DivansGpuError as e:
            refused += 1
            m = re.search(r"container (\d+)", str(e))
            if m:
                assert int(m.group(1)) in victims, (it, str(e), victims)
            continue
        accepted += 1
        for i, x in enumerate(inputs):
            if i not in victims:
                assert back[i].size == x.size and (back[i] == x).all(), (it, i)
    assert refused > 200 and refused + accepted == 240
    # and the library is still in working order
    back, _ = da.batch_decompress(sets[0], total, da.batch_options())
    assert all((back[i] == inputs[i]).all() for i in range(6))


def test_one_call_over_all_devices_equals_one_call_per_device(corpus):
    """divans_batch_options::device = DIVANS_BATCH_ALL_DEVICES (-1) -- the split over the node's GPUs sits behind the C ABI:
    contiguous stream ranges [n r / D, n (r + 1) / D), one driving thread per device inside the call, outputs in stream order.  The
    containers and the payloads must be bit-identical to one-device calls (on a one-GPU box D = 1: the same path, one share)."""
    import torch
    import divans_amd as da
    import workload
    rng = np.random.default_rng(23)
    n = 257
    blocks = workload.make_blocks(corpus, 40, n, block_len=20000)
    lens = rng.integers(0, 20001, size=n)
    inputs = [blocks[i, :lens[i]] for i in range(n)]
    D = torch.cuda.device_count()
    for all_devices, opts in ((-1, dict()), (-2, dict()), (-2, dict(dynamic_context_mixing=2, force_stride=0, window_size=18))):     # -2: the sharded code path even at D = 1
        all_c, t_all = da.batch_compress(inputs, da.batch_options(device=all_devices, host_threads=6, **opts))
        assert t_all["total_ms"] > 0
        ref = []
        for r in range(D):          # one call per device on its contiguous range
            b, e = n * r // D, n * (r + 1) // D
            part, _ = da.batch_compress(inputs[b:e], da.batch_options(device=r, host_threads=6, **opts))
            ref.extend(part)
        assert len(all_c) == len(ref) == n
        for i in range(n):
            assert all_c[i].size == ref[i].size and (all_c[i] == ref[i]).all(), i
        back, _ = da.batch_decompress(all_c, int(lens.sum()), da.batch_options(device=all_devices, host_threads=6))
        for i in range(n):
            assert back[i].size == inputs[i].size and (back[i] == inputs[i]).all(), i
        bad = [c.copy() for c in all_c]
        victim = n - 2
        bad[victim][bad[victim].size // 2] ^= 0x20
        with pytest.raises(da.DivansGpuError, match="container %d|device" % victim):
            da.batch_decompress(bad, int(lens.sum()), da.batch_options(device=all_devices))
    with pytest.raises(da.DivansGpuError):
        da.batch_compress(inputs[:4], da.batch_options(device=-3))
