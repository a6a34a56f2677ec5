"""Guards what tests/test_gpu_bucketed_segments.py compares against and codes: the oracle's segment driver under the literal-only
configurations (B of tests/bucketed_segment_cases.py; A and C are families of tests/test_segment_cases_cpu.py) against the second
restatement, and the added shapes themselves -- every list adds up, every stream fits a 64 KiB slot, and every segment start the
shapes are named for carries a history that matters: taking it away changes the coded bytes."""
import numpy as np
import pytest

import bucketed_segment_cases as bc
import pyoracle as po
import segment_cases as sc
from ref_restatement import rr_segments_decode, rr_segments_encode

_BATCHES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _cfg(key):
    fam = bc.CONFIGS[key]
    return fam, fam.configure(getattr(po, "config_" + fam.base)())


def _extra(key, sources):
    if key not in _BATCHES:
        _BATCHES[key] = bc.extra_shapes(bc.CONFIGS[key], sources)
    return _BATCHES[key]


def _enc(cfg, lit, segs):
    return po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"]).tobytes()


@pytest.mark.parametrize("key", ["B_lsb6", "B_msb6"])
def test_oracle_segment_driver_equals_the_second_restatement(key, sources):
    fam, cfg = _cfg(key)
    assert cfg.context_mixing == 0 and cfg.prediction_mode == fam.mode and cfg.btype == 0
    cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8)[:64]
    assert sorted(cmap.tolist()) == list(range(64)) and (cmap != np.arange(64)).any()
    assert set(bytes(cfg.mixing_mask)) == {4}
    names = []
    for name, lit, segs in sc.shapes(fam, sources, small=True):
        assert lit.size <= 1500 and int(segs["len"].sum()) == lit.size and int(segs["btype"].max()) == 0
        coded = po.lit_segments_encode(cfg, lit, segs["len"], segs["btype"], segs["last8"])
        assert rr_segments_encode(cfg, lit, segs) == coded.tobytes(), name
        assert rr_segments_decode(cfg, coded.tobytes(), segs) == lit.tobytes(), name
        assert (po.lit_segments_decode(cfg, coded, lit.size, segs["len"], segs["btype"], segs["last8"]) == lit).all(), name
        if name == "S5":
            assert coded.tobytes() == po.lit_encode(cfg, lit).tobytes()
        names.append(name)
    assert names == ["S1", "S2", "S3", "S4", "S5", "S7"]


def test_the_context_map_moves_rows_without_changing_them(sources):
    """without mixing and with the context a function of the previous byte, the high row [ctx][prev] is chosen by prev alone: LSB6 and
    MSB6 under different maps write the same bytes -- which is why the one-model bucketed pass may key its buckets by prev"""
    (fa, ca), (fb, cb) = _cfg("B_lsb6"), _cfg("B_msb6")
    assert bytes(ca.literal_context_map) != bytes(cb.literal_context_map) and ca.prediction_mode != cb.prediction_mode
    lit = sources[0][5000:8000]
    assert po.lit_encode(ca, lit).tobytes() == po.lit_encode(cb, lit).tobytes()


@pytest.mark.parametrize("key", list(bc.CONFIGS))
def test_every_list_adds_up_and_every_stream_fits_a_slot(key, sources):
    fam = bc.CONFIGS[key]
    streams = bc.batch(fam, sources)
    assert len(streams) == sc.N_STREAMS + 4
    names = [s[0] for s in streams]
    assert [n for n in names if n.startswith("X_")] == ["X_edges", "X_slot", "X_ones", "X_empty"]
    assert max(names.index(n) for n in names if n.startswith("X_")) > 24 > names.index("X_edges")      # both launch sequences of 24 hold some
    for name, lit, segs in streams:
        assert int(segs["len"].astype(np.int64).sum()) == lit.size <= 65536, name
        assert segs.size == 0 or int(segs["btype"].max()) < fam.n_btypes, name
        if fam.n_btypes == 1:
            assert (segs["btype"] == fam.btype).all(), name
    by = {s[0]: s for s in streams}
    for name, cuts in bc.NAMED_CUTS.items():
        assert by[name][1].size == bc.SIZES[name] and np.cumsum(by[name][2]["len"]).tolist() == cuts + [bc.SIZES[name]]
    assert by["X_slot"][1].size == 65536
    assert by["X_ones"][2]["len"].tolist() == [1] * 8200 and by["X_ones"][2].size > 256
    assert by["X_empty"][2]["len"].tolist() == [8192, 0, 0, 0, 12000 - 8192]
    buf, offs, sizes = bc.layout(streams)
    assert (offs % 16 == 0).sum() >= 10 and (offs % 16 != 0).sum() >= 20
    assert all(offs[i] + sizes[i] <= offs[i + 1] for i in range(len(streams) - 1))
    big = [i for i, s in enumerate(streams) if s[1].size > 16384]
    assert {int(offs[i]) % 16 == 0 for i in big} == {True, False}      # long streams on both load paths
    for (name, lit, _), o in zip(streams, offs):
        assert (buf[int(o):int(o) + lit.size] == lit).all()


@pytest.mark.parametrize("key", list(bc.CONFIGS))
def test_every_added_history_differs_from_the_bytes_before_it(key, sources):
    """the newest byte of every segment's last8 is not the byte before the segment: under A and B (keys from the previous byte alone)
    each start moves a position to another bucket; and the lists change what the oracle writes"""
    fam, cfg = _cfg(key)
    for name, lit, segs in _extra(key, sources):
        starts = np.concatenate([[0], np.cumsum(segs["len"].astype(np.int64))[:-1]])
        for q, l8 in zip(starts.tolist(), segs["last8"].tolist()):
            assert (l8 >> 56) != (int(lit[q - 1]) if q else 0), (name, q)
        assert _enc(cfg, lit, segs) != po.lit_encode(cfg, lit).tobytes(), name


@pytest.mark.parametrize("name", list(bc.NAMED_CUTS))
def test_every_named_cut_has_teeth(name, sources):
    """configuration C: giving the segment that starts at a named cut the stream's own bytes as history changes the oracle's bytes"""
    fam, cfg = _cfg("C")
    _, lit, segs = next(s for s in _extra("C", sources) if s[0] == name)
    full = _enc(cfg, lit, segs)
    starts = np.concatenate([[0], np.cumsum(segs["len"].astype(np.int64))[:-1]]).tolist()
    for cut in bc.NAMED_CUTS[name]:
        k = starts.index(cut)
        other = segs.copy()
        other["last8"][k] = bc.natural_last8(lit, cut)
        assert int(other["last8"][k]) != int(segs["last8"][k])
        assert _enc(cfg, lit, other) != full, (name, cut)


def test_empty_segments_on_a_piece_base_yield_to_the_one_that_follows(sources):
    fam, cfg = _cfg("C")
    _, lit, segs = next(s for s in _extra("C", sources) if s[0] == "X_empty")
    full = _enc(cfg, lit, segs)
    assert _enc(cfg, lit, segs[segs["len"] > 0]) == full
    for k in (1, 2, 3):
        other = segs.copy(); other["last8"][k] = ~other["last8"][k]
        assert _enc(cfg, lit, other) == full
    other = segs.copy(); other["last8"][4] = bc.natural_last8(lit, 8192)
    assert _enc(cfg, lit, other) != full


def test_the_faulty_batches(sources):
    fam = bc.CONFIGS["A"]
    streams = bc.batch(fam, sources)[:12]
    bad = bc.bad_btype(streams, 7, 8)
    assert sum(int((b[2]["btype"] != g[2]["btype"]).sum()) for b, g in zip(bad, streams)) == 1 and int(bad[7][2]["btype"].max()) == 8
    e = bc.empty_stream_with_bytes_in_its_list(streams, 4)
    assert e[4][1].size == 0 and e[4][2]["len"].tolist() == [5] and all(a is b for a, b in zip(e[:4] + e[5:], streams[:4] + streams[5:]))
