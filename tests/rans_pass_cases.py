"""Directed batches for the rANS pass alone (include/divans_gpu.h: divans_gpu_selftest_rans_batch), shared by the CPU tier
(tests/test_rans_pass_cases_cpu.py: the oracle against the second restatement, the bound, the coverage conditions) and the GPU tier
(tests/test_gpu_rans_pass.py: rans_encode_kernel, rans_encode2_kernel, rans_encode2_split_kernel and rans_stitch_kernel against the
oracle, bit for bit, with every byte around the streams watched).

A batch is rows of (start | freq << 16) words, oldest symbol first, one row of `sf_stride` words per stream; a stream of `size` BYTES
owns the first 2 * size words of its row, everything behind them holds JUNK -- a word that is no valid pair, so coding it both changes
the bytes and raises the status word.  Nothing here is random at run time: every generator is seeded by the batch and the stream.

Value patterns, per symbol, by its distance d from the END of its 65 536-symbol chunk (the encoder walks a chunk backwards, state a
takes the even distances, state b the odd ones; rans_encode2_split_kernel gives each state a lane):
  f1_hi / f1_lo   freq 1 everywhere with start 32767 / 0: every symbol adds 15 bits, the most a pair can -- the input that fills
                  divans_gpu_lit_encode_bound and the chunk-0 scratch stride to within 16 bytes
  first_lane      (start 0, freq 1) at even d, (start 1, freq 32767) at odd d: only state a ever pushes a word
  second_lane     the mirror: only state b pushes
  no_push         (0, 32767): 2^-15 short of free, no word is ever pushed (a chunk is its 16 bytes of states)
  one_bit         (16384, 16384): one bit per symbol
  random          freq log-uniform in [1, 32767], start uniform in [0, 32768 - freq]
  seam_f1_np / seam_np_f1   f1_hi in chunk 0 and no_push in chunk 1 / the reverse: the largest and the smallest chunk side by side
"""
import collections

import numpy as np

CHUNK = 65536                    # symbols per chunk (ans.rs NUM_SYMBOLS_BEFORE_FLUSH)
JUNK = 0xDEADBEEF                # start 0xBEEF >= 32768 and freq 0xDEAD >= 32768: never a valid pair
PATTERNS = ("f1_hi", "f1_lo", "first_lane", "second_lane", "no_push", "one_bit", "random", "seam_f1_np", "seam_np_f1")
ALL_IMPLS = (0, 1, 2)            # 0 rans_encode_kernel, 1 rans_encode2_kernel + stitch, 2 rans_encode2_split_kernel + stitch

SHORT_LENGTHS = tuple(range(35)) + (63, 64, 65, 96, 127, 128, 129)
LONG_LENGTHS = (32767, 32768, 32769, 32770, 32771) + tuple(32768 + k for k in range(30, 35)) + (65535, 65536)
LENGTHS = SHORT_LENGTHS + LONG_LENGTHS          # bytes, on every impl
LENGTHS_IMPL0 = (65537, 98305)                   # three and four chunks: rans_encode_kernel only
RING1_EXTRA = tuple(range(1, 35))                # bytes past the first chunk in the `ring1` batch
STREAM_COUNTS =(1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
ZERO_SLOTS = (7, 8, 40)                          # positions inside every 64-stream group that hold an empty stream
BAD_PAIRS = {"freq0": (5, 0), "freq32768": (0, 32768), "start32768": (32768, 1)}      # (start, freq)

Batch = collections.namedtuple("Batch", "name pairs sizes sf_stride out_base impls patterns")


def word(start, freq):
    return np.uint32(start | (freq << 16))


def _distance(nsym):
    """distance of every symbol from the end of its chunk"""
    i = np.arange(nsym, dtype=np.int64)
    end = np.minimum((i // CHUNK + 1) * CHUNK, nsym)
    return end - 1 - i


def pattern_pairs(pattern, size, seed=0):
    """the 2 * size pair words of one stream of `size` bytes under `pattern`"""
    nsym = 2 * size
    d = _distance(nsym)
    if pattern == "f1_hi":
        return np.full(nsym, word(32767, 1), dtype=np.uint32)
    if pattern == "f1_lo":
        return np.full(nsym, word(0, 1), dtype=np.uint32)
    if pattern == "no_push":
        return np.full(nsym, word(0, 32767), dtype=np.uint32)
    if pattern == "one_bit":
        return np.full(nsym, word(16384, 16384), dtype=np.uint32)
    if pattern in ("first_lane", "second_lane"):
        pushing = (d & 1) == (0 if pattern == "first_lane" else 1)
        return np.where(pushing, word(0, 1), word(1, 32767)).astype(np.uint32)
    if pattern in ("seam_f1_np", "seam_np_f1"):
        chunk0 = np.arange(nsym) < CHUNK
        f1 = chunk0 if pattern == "seam_f1_np" else ~chunk0
        return np.where(f1, word(32767, 1), word(0, 32767)).astype(np.uint32)
    if pattern == "random":
        rng = np.random.default_rng([20260117, seed, size])
        freq = np.clip(np.floor(np.exp(rng.random(nsym) * np.log(32768.0))).astype(np.int64), 1, 32767)
        start = np.floor(rng.random(nsym) * (32768 - freq + 1)).astype(np.int64)
        start = np.minimum(start, 32768 - freq)
        return (start | (freq << 16)).astype(np.uint32)
    raise ValueError(pattern)


def _stride(sizes, extra=0):
    longest = 2 * int(max(sizes)) + extra
    return max(4, (longest + 3) & ~3)


def make_batch(name, streams, impls=ALL_IMPLS, out_base=0, sf_stride=None):
    """streams: list of (pattern, size); the row behind a stream's pairs is JUNK"""
    sizes = np.array([s for _, s in streams], dtype=np.uint32)
    stride = sf_stride if sf_stride is not None else _stride(sizes)
    assert stride % 4 == 0 and stride >= 2 * int(sizes.max())
    pairs = np.full((len(streams), stride), JUNK, dtype=np.uint32)
    for i, (pattern, size) in enumerate(streams):
        pairs[i, :2 * size] = pattern_pairs(pattern, size, seed=i)
    return Batch(name, pairs, sizes, stride, out_base, tuple(impls), tuple(p for p, _ in streams))


def count_streams(n):
    """n short `random` streams whose lengths cycle through 0 .. 34, empty streams inside every group of 64, and a full two-chunk f1_hi
    stream at n - 1 and at n // 2: the tight case on both sides of a block edge"""
    streams = [("random", 0 if i % 64 in ZERO_SLOTS else i % 35) for i in range(n)]
    streams[n // 2] = ("f1_hi", 65536)
    streams[n - 1] = ("f1_hi", 65536)
    return streams


def _builders():
    b = collections.OrderedDict()
    for p in PATTERNS:
        b[f"short-{p}"] = lambda p=p: make_batch(f"short-{p}", [(p, s) for s in SHORT_LENGTHS])
        b[f"long-{p}"] = lambda p=p: make_batch(f"long-{p}", [(p, s) for s in LONG_LENGTHS])
    # chunk 1 of 2 .. 68 symbols: every residue of the prefetch ring where the chunk does not begin at the row's first word
    b["ring1"] = lambda: make_batch("ring1", [("random", 32768 + k) for k in RING1_EXTRA])
    # three and four chunks, one lane per stream
    b["chunks3"] = lambda: make_batch("chunks3", [(p, s) for p in PATTERNS for s in LENGTHS_IMPL0], impls=(0,))
    for n in STREAM_COUNTS:
        b[f"count-{n}"] = lambda n=n: make_batch(f"count-{n}", count_streams(n))
    # the form in which the sub-batched model passes hand the pairs over: rows longer than the longest stream, the offsets of a later sub-batch
    hand = [("random", 33), ("f1_hi", 65536), ("random", 0), ("seam_np_f1", 32769), ("random", 32800), ("first_lane", 65536), ("one_bit", 1),
            ("second_lane", 32770), ("f1_lo", 32768)]
    b["handover"] = lambda: make_batch("handover", hand, out_base=4096, sf_stride=2 * 65536 + 12)
    hand3 = [("random", 98306), ("f1_hi", 65537), ("random", 0), ("seam_f1_np", 98305), ("random", 17), ("second_lane", 98305)]
    b["handover3"] = lambda: make_batch("handover3", hand3, impls=(0,), out_base=4096, sf_stride=2 * 98306 + 12)
    return b


_BUILDERS = _builders()
NAMES = tuple(_BUILDERS)


def batch(name):
    """the batch of that name, built afresh (the large ones are not worth keeping between tests)"""
    return _BUILDERS[name]()


BAD_STREAMS = [("random", 10), ("random", 0), ("random", 32800), ("random", 33), ("random", 7)]
BAD_STREAM, BAD_SYMBOL = 2, CHUNK + 5           # the middle stream, inside its chunk 1 (symbols 65 536 .. 65 599)


def bad_batch(kind):
    """(good batch, the same batch with one pair outside the kernels' domain): BAD_PAIRS[kind] in chunk 1 of the middle stream"""
    good = make_batch(f"bad-{kind}", BAD_STREAMS)
    start, freq = BAD_PAIRS[kind]
    pairs = good.pairs.copy()
    pairs[BAD_STREAM, BAD_SYMBOL] = np.uint32(start | (freq << 16))
    return good, good._replace(pairs=pairs)


def stream_pairs(b, i):
    return b.pairs[i, :2 * int(b.sizes[i])]


def push_counts(chunk_pairs):
    """(both, first lane only, second lane only, none) over the steps of one chunk, a step being the symbols at distances 2j (state a,
    the first lane of rans_encode2_split_kernel) and 2j + 1 (state b) from the chunk's end.  Plain integers, ans.rs:302-329."""
    n = len(chunk_pairs)
    assert n % 2 == 0
    st = [1 << 31, 1 << 31]
    counts = [0, 0, 0, 0]
    for j in range(n // 2):
        pushed = [0, 0]
        for lane in (0, 1):
            p = int(chunk_pairs[n - 1 - (2 * j + lane)])
            start, freq = p & 0xffff, p >> 16
            s = st[lane]
            if s >= (freq << 48):
                pushed[lane] = 1
                s >>= 32
            st[lane] = ((s // freq) << 15) + s % freq + start
        counts[{(1, 1): 0, (1, 0): 1, (0, 1): 2, (0, 0): 3}[tuple(pushed)]] += 1
    return tuple(counts)
