"""Offline simulation of the two organisations the plain stride-1 decoder has for its HIGH stride rows under a constant context
(lit_decode2.hip; design aid, not product).  There the row of a byte is the rank of the byte before it in the launch's byte order;
the functions restate the kernel's lookups: 2-way sets that evict the way not used most recently, and rows pinned by rank
(tests/test_pinned_rows_cpu.py).  A companion of sim_row_cache.py, which sweeps cache sizes and hashes over all rows of a configuration
and runs on import; this one only defines functions and prints when run as a script."""
import os
import sys

import numpy as np


def learned_rank(streams, sample_streams=64, sample_len=2048):
    """learn_byte_rank_kernel: a histogram of the first `sample_len` bytes of `sample_streams` streams spread over the batch; rank of a
    byte value = how many values are more frequent, ties by value.  -> rank[256]"""
    n = len(streams)
    k = min(sample_streams, n)
    cnt = np.zeros(256, np.int64)
    for j in range(k):
        cnt += np.bincount(streams[(j * n) // k][:sample_len], minlength=256)
    order = sorted(range(256), key=lambda x: (-int(cnt[x]), x))
    rank = np.empty(256, np.int64)
    rank[order] = np.arange(256)
    return rank


def high_row_ranks(stream, rank):
    """rank of the previous byte at every position (the byte before the first is 0): the low byte of the high stride row"""
    prev = np.concatenate([[0], stream[:-1]]).astype(np.int64)
    return rank[prev]


def high_rows_2way_misses(stream, rank, rows=32):
    """Table2::load, CM_2WAY with dm_shift 31: set = rank & (rows / 2 - 1), two tags and the most recently used way per set; a miss
    replaces the OTHER way (empty sets start with way 0 marked as used) and every access marks its way.  -> misses"""
    sets = rows // 2
    t0 = [-1] * sets; t1 = [-1] * sets; mru = [0] * sets
    miss = 0
    for r in high_row_ranks(stream, rank).tolist():
        s = r & (sets - 1)
        if t1[s] == r: way = 1
        elif t0[s] == r: way = 0
        else:
            way = mru[s] ^ 1
            miss += 1
            if way: t1[s] = r
            else: t0[s] = r
        mru[s] = way
    return miss


def high_rows_pinned_misses(stream, rank, slots):
    """Table2::load, CM_PIN: the rows of rank < slots live in LDS, every other access goes to memory.  -> misses"""
    return int((high_row_ranks(stream, rank) >= slots).sum())


def pinned_slots(rows):
    """lit_decode2_stream_lds: the LDS of `rows` tagged rows (34 bytes each) as 32-byte slots"""
    return min(rows * 34 // 32, 256)


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import workload
    batch = workload.make_blocks(workload.load_corpus(), 0, 64)
    rank = learned_rank(batch)
    for bi in (0, 21, 42, 63):
        n = batch[bi].size
        print(f"high rows, text stream {bi}: 2-way 32 rows {high_rows_2way_misses(batch[bi], rank) * 100 / n:5.2f} % misses, pinned 32 "
              f"{high_rows_pinned_misses(batch[bi], rank, 32) * 100 / n:5.2f} %, pinned {pinned_slots(32)} {high_rows_pinned_misses(batch[bi], rank, pinned_slots(32)) * 100 / n:5.2f} %")


if __name__ == "__main__":
    main()
