"""The command lists with history of tests/history_cases.py without a GPU.  The defining identity: a stream with history H is the
stream WITHOUT history whose list begins with an INSERT of H -- so the new executor is pinned to command_cases.execute, which the
merged tests already trust (against the product's IR walk and the reference's vectors): same segments, raw = H ++ raw."""
import numpy as np
import pytest

import command_cases as cc
import history_cases as hc
import segment_cases as sc


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _same_segments(a, b):
    return a.size == b.size and (a["len"] == b["len"]).all() and (a["btype"] == b["btype"]).all() and (a["last8"] == b["last8"]).all()


def _assert_identity(s):
    p = hc.as_plain(s)
    raw, segs = cc.execute(p["cmds"], p["lit"], p["ins"])
    h = s["hist"].size
    assert raw.size == h + s["raw"].size and (raw[:h] == s["hist"]).all() and (raw[h:] == s["raw"]).all(), s["name"]
    assert _same_segments(segs, s["segs"]), s["name"]


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_history_is_an_insert_in_front_of_the_list(fam, sources):
    for mode in hc.MODES:
        streams = hc.directed(fam, sources, mode)
        for s in streams:
            _assert_identity(s)
            assert (s["segs"]["btype"] < fam.n_btypes).all() and int(s["segs"]["len"].sum()) == s["lit"].size
        if mode != "own":
            D = hc.dictionary_of(fam)
            assert all(s["hist"].size == 0 or (D[s["hist_at"]:s["hist_at"] + s["hist"].size] == s["hist"]).all() for s in streams)
    for s in hc.encode_extras(fam, sources):
        _assert_identity(s)


def test_directed_batch_holds_what_it_is_meant_to_hold(sources):
    fam = sc.FAMILIES[0]
    streams = hc.directed(fam, sources)
    by = {s["name"]: s for s in streams}
    assert len(streams) <= 300 and sum(s["lit"].size > cc.CHUNK for s in streams) == 1
    assert set(s["hist"].size for s in streams) >= set(hc.SIZES)
    for h in hc.SIZES:                                          # last8 of a first Literal: the history's last bytes behind zeros
        s = by[f"first_lit_h{h}"]
        assert int(s["segs"]["last8"][0]) == int.from_bytes(bytes(s["hist"][-8:]).rjust(8, b"\0"), "little")
    for h in (1, 8, 17):
        for p in range(1, 8):
            s = by[f"lit_at_pos{p}_h{h}"]
            assert s["cmds"]["kind"].tolist() == [cc.COPY, cc.LITERAL] and s["cmds"]["len"][0] == p
    for h in hc.SIZES[1:]:                                      # a COPY as the first command: distance pos + h, and distance 1
        assert by[f"copy_first_oldest_h{h}"]["cmds"]["arg"][0] == h and by[f"copy_first_oldest_h{h}"]["raw"][0] == by[f"copy_first_oldest_h{h}"]["hist"][0]
        assert by[f"copy_first_newest_h{h}"]["cmds"]["arg"][0] == 1 and by[f"copy_first_newest_h{h}"]["raw"][0] == by[f"copy_first_newest_h{h}"]["hist"][-1]
    for j in range(17):                                         # the crossing at byte j of a copy that does not overlap
        kind, n, d, _ = by[f"cross_at{j}"]["cmds"].tolist()[1]
        assert kind == cc.COPY and d - 24 == j and j < n <= d and len(hc.reaching_copies(by[f"cross_at{j}"])) == (1 if j else 0)
    for n in hc.LENGTHS:
        (i, pos, nn, d), = hc.reaching_copies(by[f"cross_len{n}"])
        assert nn == n <= d and 0 < d - pos <= 16
    seen = set()
    for pos in (1, 5, 16, 17):                                  # overlapping copies whose period straddles the history's end
        for d in range(max(pos + 1, 2), 41):
            (i, p, n, dd), = hc.reaching_copies(by[f"overlap_pos{pos}_d{d}"])
            assert (p, dd) == (pos, d) and pos < d < n
            seen.add(n)
    assert seen >= {15, 16, 17, 63, 64, 65, 129, 300}
    assert by["no_history"]["hist"].size == 0 and not hc.reaching_copies(by["no_history"])
    lay = hc.history_layout(streams)
    assert sorted(set(int(o) % 16 for o in lay["hist_off"])) == list(range(16))
    for s, o in zip(streams, lay["hist_off"].tolist()):         # sentinels in front of and behind every range
        assert lay["hist"][o - 1] == hc.HIST_SENTINEL and lay["hist"][o + s["hist"].size] == hc.HIST_SENTINEL
        assert (lay["hist"][o:o + s["hist"].size] == s["hist"]).all()
    shared = hc.directed(fam, sources, "shared")
    lay = hc.history_layout(shared, "shared", hc.dictionary_of(fam))
    assert len(set(lay["hist_off"].tolist())) == 1 and set(lay["hist_sz"].tolist()) == {0, hc.DICT}
    over = hc.directed(fam, sources, "overlap")
    lay = hc.history_layout(over, "overlap", hc.dictionary_of(fam))
    spans = sorted((int(o), int(o) + int(z)) for o, z in zip(lay["hist_off"], lay["hist_sz"]) if z)
    assert len(set(spans)) > 100 and any(a[0] < b[0] < a[1] < b[1] for a, b in zip(spans[:-1], spans[1:])), "no two ranges partly overlap"


def test_encode_extras_sit_on_the_prepare_kernels_edges(sources):
    fam = sc.FAMILIES[0]
    extras = hc.encode_extras(fam, sources)
    assert sorted(hc.reaching_copies(s)[0][0] for s in extras[:4]) == [62, 63, 64, 65]
    for c in range(16):
        (i, pos, n, d), = hc.reaching_copies(extras[4 + c])
        assert pos == 32 and n == 48 and d == 48 + c and n <= d      # raw bytes 32 .. 48 + c - 1 come from history: the piece at 48 crosses at c


def test_lists_that_must_fail_do_fail(sources):
    fam = sc.FAMILIES[0]
    v, g = hc.victim_base(fam, sources)
    hc.execute_with_history(v["cmds"], v["lit"], v["ins"], v["hist"], raw_size=v["raw"].size)
    for what, cmds in hc.faulty_lists(v):
        with pytest.raises(ValueError):
            hc.execute_with_history(cmds, v["lit"], v["ins"], v["hist"], raw_size=v["raw"].size)
    # one byte further back than the history holds, and the same list with one more history byte: the bound is exactly pos + h
    far = v["cmds"].copy(); far["arg"][1] = 10 + v["hist"].size + 1
    with pytest.raises(ValueError):
        hc.execute_with_history(far, v["lit"], v["ins"], v["hist"])
    hc.execute_with_history(far, v["lit"], v["ins"], np.concatenate([[7], v["hist"]]).astype(np.uint8))
    for what, hist, raw in hc.faulty_bytes(v):                  # the changed byte is one the list's copies compare
        r, _ = hc.execute_with_history(v["cmds"], v["lit"], v["ins"], hist)
        assert not (r == raw).all(), what


def test_cut_pieces_give_the_whole_back(sources):
    fam = sc.FAMILIES[0]
    rng = np.random.default_rng(3)
    s = cc.Stream("file", fam, sc._Data(sources, rng), rng)
    for i in range(60):
        s.lit(5 + i % 9).copy(3 + i % 40, 1 + (i * 7) % s.produced).ins(i % 4)
    whole = s.done()
    pieces = hc.cut(whole, 3)
    assert (np.concatenate([p["raw"] for p in pieces]) == whole["raw"]).all() and (np.concatenate([p["lit"] for p in pieces]) == whole["lit"]).all()
    assert np.concatenate([p["segs"] for p in pieces]).tobytes() == whole["segs"].tobytes()
    assert any(hc.reaching_copies(p) for p in pieces[1:]) and pieces[0]["hist"].size == 0
