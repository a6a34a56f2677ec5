"""The premise of the pinned organisation of the plain stride-1 decoder's high stride rows (lit_decode2.hip, CM_PIN),
on a Python restatement of the kernel's two lookups (tests/tools/sim_pinned_rows.py): with the byte order learned as
learn_byte_rank_kernel learns it (64 streams x 2 KiB), keeping the rows of ranks 0 .. P-1 in the LDS that 32 tagged rows take
(P = 34) sends fewer high rows to memory than the 2-way sets do, on every single stream -- benchmark text and the non-text control."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

import sim_pinned_rows as sim
import workload

N_EVAL = 8
ROWS = 32


def _batch(src):
    """64 streams as bench.py cuts them (the rank is learned from all of them), 8 of them spread over the batch evaluated"""
    batch = workload.make_blocks(src, 0, 64)
    return batch, [batch[(j * 64) // N_EVAL] for j in range(N_EVAL)]


def test_pinned_slots_of_the_library_sizes():
    assert [sim.pinned_slots(r) for r in (4, 8, 16, 32, 64, 128, 256)] == [4, 8, 17, 34, 68, 136, 256]


def test_learned_rank_is_a_permutation_by_frequency(corpus):
    batch, _ = _batch(corpus)
    rank = sim.learned_rank(batch)
    assert sorted(rank.tolist()) == list(range(256))
    assert rank[ord(" ")] == 0 and rank[ord("e")] == 1        # English text
    cnt = np.zeros(256, np.int64)
    for s in batch:
        cnt += np.bincount(s[:2048], minlength=256)
    by_rank = cnt[np.argsort(rank)]
    assert (np.diff(by_rank) <= 0).all()


@pytest.mark.parametrize("source", ["text", "random_then_unicode"])
def test_pinned_rows_miss_less_than_two_way_sets_on_every_stream(source, corpus, random_then_unicode):
    batch, streams = _batch(corpus if source == "text" else random_then_unicode)
    rank = sim.learned_rank(batch)
    slots = sim.pinned_slots(ROWS)
    assert slots == 34
    for i, s in enumerate(streams):
        two_way = sim.high_rows_2way_misses(s, rank, ROWS)
        pinned = sim.high_rows_pinned_misses(s, rank, slots)
        print(f"{source} stream {i}: 2-way {100 * two_way / s.size:.2f} % misses, pinned {slots}: {100 * pinned / s.size:.2f} %")
        assert pinned < two_way, (source, i, pinned, two_way)
        # the slot rule itself: a row is in LDS exactly when the rank of the previous byte is below the slot count
        assert pinned == int((sim.high_row_ranks(s, rank) >= slots).sum())


def test_two_way_model_on_a_directed_sequence():
    """sets of two with the way NOT used most recently evicted: a, b, c in one set -> c evicts a; then a misses and evicts b"""
    rank = np.arange(256)
    # previous bytes 0, 16, 32 share set 0 of 16 sets; the stream's own first previous byte is 0
    seq = np.array([16, 32, 0, 16, 16, 0], np.uint8)      # previous bytes seen: 0, 16, 32, 0, 16, 16
    # 0 miss (way 1), 16 miss (way 0), 32 miss (evicts 0), 0 miss (evicts 16), 16 miss (evicts 32), 16 hit
    assert sim.high_rows_2way_misses(seq, rank, 32) == 5
    assert sim.high_rows_pinned_misses(seq, rank, 34) == 0
    assert sim.high_rows_pinned_misses(seq, rank, 17) == 1
