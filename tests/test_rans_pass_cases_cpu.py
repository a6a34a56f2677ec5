"""The reference of tests/test_gpu_rans_pass.py is the C oracle's ANSEncoder on caller-supplied pairs (orc_ans_encode_pairs).  This file
guards that oracle and the batches of tests/rans_pass_cases.py without a GPU: the oracle writes what the second restatement
(ref_restatement.AnsEncoder, Python) writes, every output fits divans_gpu_lit_encode_bound, `f1` stays the input that comes within 16
bytes of it, the patterns hold the push combination they are named after for a whole chunk (counted from the reference's arithmetic
alone), and every (impl, pattern, length) the GPU tier is meant to see is in some batch."""
import numpy as np
import pytest

import pyoracle as po
import rans_pass_cases as rc
import ref_restatement as rr


def second_opinion(pairs):
    """(bytes, per-chunk sizes) of ref_restatement.AnsEncoder on the pair words"""
    enc = rr.AnsEncoder()
    sizes = []; done = 0
    for p in pairs:
        p = int(p)
        enc.put_start_freq(p & 0xffff, p >> 16)
        if len(enc.out) != done:
            sizes.append(len(enc.out) - done); done = len(enc.out)
    enc.flush_chunk()
    if len(enc.out) != done:
        sizes.append(len(enc.out) - done)
    return bytes(enc.out), sizes


def bound(size):
    import divans_amd as da
    return da.encode_bound(size)


@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_equals_the_second_restatement_and_fits_the_bound(name):
    b = rc.batch(name)
    assert len(b.sizes) > 0 and b.pairs.shape == (len(b.sizes), b.sf_stride) and b.sf_stride % 4 == 0
    assert b.sf_stride >= 2 * int(b.sizes.max()) and b.impls
    seen = set()
    for i, size in enumerate(int(s) for s in b.sizes):
        pairs = rc.stream_pairs(b, i)
        assert (b.pairs[i, 2 * size:] == rc.JUNK).all()
        freq = pairs >> 16; start = pairs & 0xffff
        assert ((freq >= 1) & (freq <= 32767) & (start + freq <= 32768)).all(), (name, i)       # the documented domain, and a distribution
        coded, chunks = po.ans_encode_pairs(pairs)
        assert coded.size == sum(chunks) <= bound(size) and len(chunks) == (2 * size + rc.CHUNK - 1) // rc.CHUNK, (name, i)
        assert coded.size % 4 == 0 and (coded.size == 0) == (size == 0)
        # the second restatement: every short stream, and the first stream of each (pattern, length) among the long ones of the
        # pattern batches' full-length entry (65 536 bytes) -- one full-length stream per pattern
        full = size == 65536 and name.startswith("long-")
        if size <= 4096 and (b.patterns[i], size) not in seen or full:
            seen.add((b.patterns[i], size))
            ref, ref_chunks = second_opinion(pairs)
            assert coded.tobytes() == ref and chunks == ref_chunks, (name, i, size)


def test_f1_is_the_tight_case():
    """freq = 1 throughout: 15 bits per symbol.  One chunk leaves 122 896 of the 122 912 bytes divans_gpu_lit_encode_bound(32768) allows
    -- which is also the stride of the chunk-0 scratch area -- and two chunks 245 792 of 245 808; no other pattern comes closer."""
    for pattern in ("f1_hi", "f1_lo"):
        for size, coded, limit in ((32768, 122896, 122912), (65536, 245792, 245808)):
            got, chunks = po.ans_encode_pairs(rc.pattern_pairs(pattern, size))
            assert bound(size) == limit and got.size == coded and chunks == [122896] * (size // 32768)
            assert 0 <= bound(size) - got.size <= 16
    for pattern in rc.PATTERNS:
        for size in (32768, 65536):
            got, _ = po.ans_encode_pairs(rc.pattern_pairs(pattern, size, seed=1))
            assert got.size <= (122896 if size == 32768 else 245792), (pattern, size)


COVERAGE = {      # (both lanes push, first lane only, second lane only) over the 32 768 steps of a full chunk; None = at least 1000 of each kind
    "f1_hi": (15000, 0, 0), "f1_lo": (15000, 0, 0), "first_lane": (0, 15000, 0), "second_lane": (0, 0, 15000), "no_push": (0, 0, 0),
    "random": None,
}


@pytest.mark.parametrize("pattern", sorted(COVERAGE))
def test_patterns_hold_their_push_combination_for_a_whole_chunk(pattern):
    """on the first 65 536-symbol chunk of the full-length stream of the pattern's batch"""
    b = rc.batch(f"long-{pattern}")
    i = list(b.sizes).index(65536)
    counts = rc.push_counts(rc.stream_pairs(b, i)[:rc.CHUNK])
    assert sum(counts) == rc.CHUNK // 2
    want = COVERAGE[pattern]
    if want is None:
        assert min(counts) >= 1000, counts
    else:
        for got, w in zip(counts[:3], want):
            assert (got == 0) if w == 0 else (got >= w), (pattern, counts)
    # the simulation is the oracle's arithmetic: its pushed words are the chunk's words
    coded, chunks = po.ans_encode_pairs(rc.stream_pairs(b, i)[:rc.CHUNK])
    assert chunks == [16 + 4 * (2 * counts[0] + counts[1] + counts[2])]


def test_every_named_shape_is_in_some_batch():
    have = set()
    for name in rc.NAMES:
        b = rc.batch(name)
        for impl in b.impls:
            have |= {(impl, p, int(s)) for p, s in zip(b.patterns, b.sizes)}
        if name.startswith("count-"):
            n = int(name.split("-")[1])
            assert len(b.sizes) == n and b.sizes[n - 1] == 65536 and b.sizes[n // 2] == 65536
            assert b.patterns[n - 1] == b.patterns[n // 2] == "f1_hi"
            for g in range(0, n, 64):                        # empty streams inside every 64-stream group that has room for them
                group = b.sizes[g:g + 64]
                assert group.size <= min(rc.ZERO_SLOTS) or (group == 0).sum() >= 1
                if group.size == 64:
                    assert (group == 0).sum() >= 3
            if n >= 127:                                     # (below that the empty and the full streams displace some of the cycle)
                assert set(range(35)) <= set(int(s) for s in b.sizes)
    for impl in rc.ALL_IMPLS:
        for p in rc.PATTERNS:
            for s in rc.LENGTHS:
                assert (impl, p, s) in have, (impl, p, s)
    for p in rc.PATTERNS:
        for s in rc.LENGTHS_IMPL0:
            assert (0, p, s) in have and (1, p, s) not in have and (2, p, s) not in have
    assert {int(n.split("-")[1]) for n in rc.NAMES if n.startswith("count-")} == set(rc.STREAM_COUNTS)
    ring1 = rc.batch("ring1")
    assert {(2 * int(s) - rc.CHUNK) % 64 for s in ring1.sizes} == set(range(0, 64, 2)) and ring1.impls == rc.ALL_IMPLS
    hand = rc.batch("handover")
    assert hand.impls == rc.ALL_IMPLS and hand.out_base == 4096 and hand.sf_stride == 2 * int(hand.sizes.max()) + 12
    hand3 = rc.batch("handover3")
    assert hand3.impls == (0,) and hand3.out_base == 4096 and hand3.sf_stride == 2 * int(hand3.sizes.max()) + 12 and hand3.sizes.max() > 65536


@pytest.mark.parametrize("kind", sorted(rc.BAD_PAIRS))
def test_bad_pair_batches(kind):
    good, bad = rc.bad_batch(kind)
    diff = np.argwhere(good.pairs != bad.pairs)
    assert diff.tolist() == [[rc.BAD_STREAM, rc.BAD_SYMBOL]]
    assert rc.CHUNK <= rc.BAD_SYMBOL < 2 * int(bad.sizes[rc.BAD_STREAM]) and rc.BAD_STREAM == len(bad.sizes) // 2
    w = int(bad.pairs[rc.BAD_STREAM, rc.BAD_SYMBOL]); start, freq = w & 0xffff, w >> 16
    assert (freq == 0) + (freq >= 32768) + (start >= 32768) == 1
    with pytest.raises(RuntimeError):                       # the reference's debug_asserts trip too
        po.ans_encode_pairs(rc.stream_pairs(bad, rc.BAD_STREAM))
