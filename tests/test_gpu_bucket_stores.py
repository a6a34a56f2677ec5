"""The bucketed encoder's pair stores at group and quad edges and its one-pass sort ("simple" configuration, set_encode_path(2)):
every nibble's (start, freq) pair against the oracle's trace, the coded bytes against the oracle and the streaming encoder."""
import numpy as np
import pytest

import pyoracle as po
import workload

pytestmark = pytest.mark.gpu

PIECE = 8192


def _host_runs(data):
    """Piece-wise stable sort by previous byte, as the sort kernel defines it: (first slot, length) of every non-empty
    (piece, previous byte) run, slots counted from the start of the stream's slot."""
    runs = []
    for base in range(0, len(data), PIECE):
        piece = data[base:base + PIECE]
        keys = np.empty(len(piece), np.int64)
        keys[0] = data[base - 1] if base else 0
        keys[1:] = piece[:-1]
        counts = np.bincount(keys, minlength=256)
        starts = np.cumsum(counts) - counts
        runs += [(base + int(starts[k]), int(counts[k])) for k in range(256) if counts[k]]
    return runs


def _check(streams):
    """One ragged call per encoder path; pairs and coded bytes of every stream against the oracle."""
    import torch
    import divans_amd as da
    dev = torch.device("cuda", 0)
    n = len(streams)
    lens = np.array([len(s) for s in streams], np.int32)
    L = int(lens.max())
    starts = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)   # back to back: every source alignment
    d_in = torch.from_numpy(np.concatenate(list(streams) + [np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.from_numpy(starts).to(dev); d_sz = torch.from_numpy(lens).to(dev)
    codec = da.LiteralCodec(da.config_simple(), L)
    got = []
    for path in (2, 1):
        codec.set_encode_path(path)
        outs = codec.alloc_encode_outputs(n)
        codec.encode_batch(d_in, n, L, outs, in_offsets=d_off, in_sizes=d_sz)
        pairs = codec.model_batch(d_in, n, L, in_offsets=d_off, in_sizes=d_sz) if path == 2 else None
        torch.cuda.synchronize()
        assert codec.status() == 0
        got.append((outs["offsets"].cpu().numpy(), outs["sizes"].cpu().numpy(), outs["out"].cpu().numpy(),
                    pairs.cpu().numpy().view(np.uint32) if pairs is not None else None))
    codec.close()
    (o2, s2, b2, p2), (o1, s1, b1, _) = got
    ocfg = po.config_simple()
    for i, data in enumerate(streams):
        ref, tr = po.lit_encode(ocfg, data, trace=True)
        want = tr[:, 1].astype(np.uint32) | (tr[:, 2].astype(np.uint32) << 16)
        have = p2[i, :2 * len(data)]
        assert (have == want).all(), ("pair", i, len(data), int(np.argmax(have != want)))
        coded2 = b2[o2[i]:o2[i] + s2[i]]
        assert s2[i] == ref.size and (coded2 == ref).all(), ("oracle", i, len(data))
        assert s1[i] == s2[i] and (b1[o1[i]:o1[i] + s1[i]] == coded2).all(), ("streaming", i, len(data))


def test_group_and_quad_edges():
    # few buckets per stream: quads with one to four busy lanes and idle quads beside them; 256 values: more buckets than lanes
    rng = np.random.default_rng(20260)
    streams = []
    for k in (1, 2, 3, 4, 5, 8, 9, 256):
        values = rng.permutation(256)[:k].astype(np.uint8)
        for length in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 600):
            streams.append(values[rng.integers(0, k, length)])
    runs = [r for s in streams for r in _host_runs(s)]
    assert {first & 7 for first, _ in runs} == set(range(8)), "run starts miss a slot alignment"
    assert {cnt & 7 for _, cnt in runs} == set(range(8)), "run lengths miss a residue"
    _check(streams)


def test_lane_recycling(corpus):
    # text and random bytes side by side: full and partial groups meet in the same quads while lanes take new tasks
    rng = np.random.default_rng(7)
    text = workload.make_blocks(corpus, 21, 150, block_len=600)
    noise = rng.integers(0, 256, (150, 600), dtype=np.uint8)
    streams = [text[i // 2] if i % 2 == 0 else noise[i // 2] for i in range(300)]
    _check(streams)


def test_sort_edges():
    rng = np.random.default_rng(99)
    streams = []
    for length in (63, 64, 65, 2047, 2048, 2049, 4097, 8191, 8192, 8193, 16385):
        streams.append(np.full(length, 0x61, np.uint8))                           # one key: in-wave rank up to 2047, 8192 per piece
        streams.append((np.arange(length) % 256).astype(np.uint8))               # every key, one position per 64 at a time
        streams.append(np.where(np.arange(length) % 2 == 0, 7, 200).astype(np.uint8))
        noise = rng.integers(0, 256, length, dtype=np.uint8)
        noise[length // 3] = 0; noise[length // 2] = 255
        streams.append(noise)
    _check(streams)
