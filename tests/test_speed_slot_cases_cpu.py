"""Guards what tests/test_gpu_speed_slots.py compares against and codes (tests/speed_slot_cases.py): for every family and every
rotation of the edge speeds the C oracle round-trips the batch, with its lists and without, and agrees with the second restatement;
and the inputs have teeth -- swapping two slots a configuration reads changes the oracle's bytes, changing one it does not read
changes none, and the long constant stream really reaches the one renormalisation (1, 16384) brings in 16 320 updates.

The restatement is pure Python (a few KB/s), so it codes batch(small=True): the same twelve streams and lists at a 1000th of the
lengths.  Those short copies cannot reach the (1, 16384) renormalisation; the full batch shows that one on the oracle alone.  The
oracle's calls of a family run on a few threads (ctypes releases the interpreter lock)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pyoracle as po
import speed_slot_cases as ss
from ref_restatement import rr_segments_decode, rr_segments_encode

ROT = range(len(ss.ROTATIONS))


@pytest.fixture(scope="module")
def sources(corpus, shuffle384):
    return (corpus, shuffle384)


@pytest.fixture(scope="module")
def pool():
    po.lib()
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        yield ex


def _cfg(case, r):
    return ss.pair(case, po, po, ss.ROTATIONS[r])[1]


def _enc(cfg, stream):
    _, lit, segs = stream
    return po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])


def _round_trip(cfg, cfg0, stream):
    """-> None, or what went wrong"""
    name, lit, segs = stream
    coded = _enc(cfg, stream)
    if not (po.lit_segments_decode(cfg, coded, lit.size, segs["len"], segs["btype"], segs["last8"])[:lit.size] == lit).all():
        return f"{name}: with its list"
    if lit.size:
        if not (po.lit_decode(cfg0, po.lit_encode(cfg0, lit), lit.size)[:lit.size] == lit).all():
            return f"{name}: without a list"
    return None


def test_the_cases_and_their_batches(sources):
    assert len(ss.CASES) == 22 and sum(c.path is None for c in ss.CASES.values()) == 5
    for sp in ss.EDGE_SPEEDS + [ss.LATER_RENORM]:
        assert ss.total_stays_in_i16(*sp), sp         # divans_gpu_speed_supported (the GPU tier asks the library): the bucketed passes must still apply
    assert not ss.total_stays_in_i16(*ss.UNREAD_SPEED) and not ss.total_stays_in_i16(8180, 64) and ss.total_stays_in_i16(16, 8192)
    for slot in range(4):                             # every speed sits in every slot once
        assert sorted(rot[slot] for rot in ss.ROTATIONS) == sorted(ss.EDGE_SPEEDS)
    for key, case in ss.CASES.items():
        fam = case.fam
        assert case.read == ((0, 2, 3) if fam.mix else (0,)) and sorted(case.read + case.unread) == [0, 1, 2, 3]
        before = bytes(fam.pair(po, po)[1])
        g, o = ss.pair(case, po, po, ss.ROTATIONS[1])
        assert ss.speeds_of(o) == ss.ROTATIONS[1] and bytes(fam.pair(po, po)[1]) == before      # the family itself is left alone
        off = po.LitConfig.literal_adaptation.offset
        assert bytes(o)[:off] == before[:off] and off + 16 == len(before)                        # nothing but the speeds differs
        assert (o.context_mixing > 1) == fam.mix
        full, small = ss.batch(fam, sources), ss.batch(fam, sources, small=True)
        assert [s[0] for s in full] == [s[0] for s in small] and len(full) == 12
        assert [s[1].size for s in full] == [17000, 17000, 17000, 12000, 12000, 4096, 4096, 4096, 4096, 0, 1, 2]
        assert sum(s[1].size for s in small) <= 85
        for streams, cuts in ((full, ss.CUTS), (small, ss.SMALL_CUTS)):
            for name, lit, segs in streams:
                assert int(segs["len"].astype(np.int64).sum()) == lit.size and (segs["len"] > 0).all(), (key, name)
                starts = np.concatenate([[0], np.cumsum(segs["len"])[:-1]]).astype(np.int64).tolist() if segs.size else []
                assert starts == ([0] + [c for c in cuts if c < lit.size])[:len(starts)] and (lit.size == 0) == (segs.size == 0), (key, name)
                assert all(int(l8) == ss.bc.natural_last8(lit, q) for l8, q in zip(segs["last8"], starts)), (key, name)
                if name in ("K_61", "K_ff"):
                    assert set(segs["btype"].tolist()) == {ss.one_block_type(fam)} and (fam.n_btypes == 1 or ss.one_block_type(fam) != fam.btype)
                else:
                    assert segs["btype"].tolist() == [k % fam.n_btypes for k in range(segs.size)], (key, name)
        assert full[0][1].size - 8 > ss.RENORM_AFTER and full[0][2].size == 8      # (the first 8 positions of a stride-8 row have another key)
        assert len(set(full[0][1].tolist())) == 1


@pytest.mark.parametrize("key", ss.KEYS)
def test_oracle_round_trips_every_stream_under_every_rotation(key, sources, pool):
    case = ss.CASES[key]
    streams = ss.batch(case.fam, sources)
    jobs = []
    for r in ROT:
        cfg = _cfg(case, r)
        cfg0 = ss.block_type_0(po, cfg)
        jobs += [(r, pool.submit(_round_trip, cfg, cfg0, s)) for s in streams]
    for r, job in jobs:
        assert job.result() is None, (key, r, job.result())


@pytest.mark.parametrize("key", ss.KEYS)
def test_oracle_equals_the_second_restatement_under_every_rotation(key, sources):
    """on the short copies, which keep the order of lengths, block types and histories but cannot reach the (1, 16384) renormalisation"""
    case = ss.CASES[key]
    streams = [s for s in ss.batch(case.fam, sources, small=True) if s[1].size]
    for r in ROT:
        cfg = _cfg(case, r)
        for s in streams:
            coded = _enc(cfg, s).tobytes()
            assert rr_segments_encode(cfg, s[1], s[2]) == coded, (key, r, s[0])
            assert rr_segments_decode(cfg, coded, s[2]) == s[1].tobytes(), (key, r, s[0])


@pytest.mark.parametrize("key", ss.KEYS)
def test_read_slots_matter_and_unread_slots_do_not(key, sources, pool):
    case = ss.CASES[key]
    swaps = [(0, 2), (0, 3), (2, 3)] if case.fam.mix else [(0, 1)]        # without mixing: slot 0 against another speed
    streams = ss.sensitivity_streams(case.fam, sources)
    assert [s[1].size for s in streams] == [17000, 3000]
    jobs = []
    for r in ROT:
        cfg = _cfg(case, r)
        elsewhere = {f"s{u}": ss.ROTATIONS[r][(u + 2) % 4] for u in case.unread}
        unsupported = {f"s{u}": ss.UNREAD_SPEED for u in case.unread}
        for s in streams:
            base = pool.submit(_enc, cfg, s)
            jobs += [(r, s[0], f"slots {a} and {b} swapped", True, base, pool.submit(_enc, ss.swapped(po, cfg, a, b), s)) for a, b in swaps]
            jobs += [(r, s[0], f"unread slots {case.unread}: {kw}", False, base, pool.submit(_enc, ss.with_slots(po, cfg, **kw), s))
                     for kw in (elsewhere, unsupported)]
    for r, name, what, changes, base, other in jobs:
        assert (base.result().tobytes() != other.result().tobytes()) == changes, (key, r, name, what)


@pytest.mark.parametrize("key", ss.KEYS)
def test_the_constant_stream_reaches_the_renormalisation(key, sources, pool):
    """(1, 16384) and (1, 20000) keep a row equal until its 16 320th update: the long constant stream, with its list, codes differently
    under them in every slot the configuration reads -- and a copy that ends 320 updates earlier does not"""
    case = ss.CASES[key]
    full = ss.batch(case.fam, sources)[0]
    lit = full[1][:ss.RENORM_AFTER - 320]
    short = (full[0], lit, ss.natural_list(case.fam, lit, ss.CUTS, [ss.one_block_type(case.fam)]))
    jobs = []
    for r in ROT:
        cfg = _cfg(case, r)
        for slot in case.read:
            if ss.ROTATIONS[r][slot] == (1, 16384):
                later = ss.with_slots(po, cfg, **{f"s{slot}": ss.LATER_RENORM})
                jobs.append((r, slot, [pool.submit(_enc, c, s) for s in (full, short) for c in (cfg, later)]))
    assert sorted(slot for _, slot, _ in jobs) == list(case.read)
    for r, slot, coded in jobs:
        a, b, c, d = (j.result().tobytes() for j in coded)
        assert a != b and c == d, (key, r, slot)
