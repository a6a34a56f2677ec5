"""Command lists with HISTORY for divans_gpu_lit_decode_commands_history_batch / divans_gpu_lit_encode_commands_history_batch, shared
by the CPU tier (tests/test_history_cases_cpu.py) and the GPU tier (tests/test_gpu_command_history.py).  numpy only.

A stream's history is h known bytes H that lie logically in front of its output: a COPY may reach 1 .. pos + h bytes back, a Literal
command's last8 is the eight bytes in front of it in H ++ out.  execute_with_history() is the plain Python executor of such a list
(command_cases.execute with a world that does not begin empty); as_plain() restates a stream as the list the merged calls understand
-- [INSERT h] + cmds with H in front of the insert bytes -- which pins the one to the other.  directed() is the batch of streams whose
copies and literals sit where the history ends; history_layout() places the histories in memory the way the GPU tests hand them over.

MODES of a batch: "own" -- every stream has a range of its own, at every alignment 0 .. 15 between sentinel bytes; "shared" -- one
dictionary, the same range for every stream that has a history; "overlap" -- windows of one dictionary that partly overlap."""
import numpy as np

import command_cases as cc
import segment_cases as sc

COPY, INSERT, LITERAL = cc.COPY, cc.INSERT, cc.LITERAL
HIST_SENTINEL = 0x96
SIZES = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 4096)      # history sizes around last8, a copy step's 16 lanes and its 64 bytes
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 129, 300)             # copy lengths: the copy loop moves 16 lanes x 4 bytes per step
DICT = 4096
MODES = ("own", "shared", "overlap")


def execute_with_history(cmds, lit, ins, hist, raw_size=None):
    """-> (raw uint8[], segments of the Literal commands with bytes).  Raises ValueError on a command that cannot run."""
    world = bytearray(bytes(hist))
    h = len(world)
    lit = bytes(lit); ins = bytes(ins)
    lp = 0
    lens, bts, l8s = [], [], []
    for kind, n, arg, _ in cmds.tolist():
        if raw_size is not None and kind in (LITERAL, COPY, INSERT) and len(world) - h + n > raw_size:
            raise ValueError("command past the raw size")
        if kind == LITERAL:
            if n == 0:
                continue
            tail = bytes(world[-8:]).rjust(8, b"\0")        # zeros only in front of the history's start, newest byte last
            lens.append(n); bts.append(arg); l8s.append(int.from_bytes(tail, "little"))
            if lp + n > len(lit):
                raise ValueError("literal bytes run out")
            world += lit[lp:lp + n]; lp += n
        elif kind == COPY:
            if n == 0:
                continue
            if arg == 0 or arg > len(world):                # len(world) = pos + h
                raise ValueError("copy from in front of the history")
            for _ in range(n):                              # byte by byte: an overlapping copy repeats
                world.append(world[-arg])
        elif kind == INSERT:
            if n == 0:
                continue
            if arg + n > len(ins):
                raise ValueError("insert outside its bytes")
            world += ins[arg:arg + n]
        else:
            raise ValueError("unknown kind")
    if lp != len(lit):
        raise ValueError("literal bytes left over")
    return np.frombuffer(bytes(world[h:]), dtype=np.uint8).copy(), sc.segments(lens, bts, l8s)


def as_plain(stream):
    """the stream as a list WITHOUT history: [INSERT h at 0] + cmds, the history in front of the insert bytes (offsets shifted by h);
    its raw bytes are H ++ raw, its literals and segments the stream's own"""
    h = stream["hist"].size
    cmds = np.concatenate([cc.commands([(INSERT, h, 0)]), stream["cmds"]])
    shifted = cmds["kind"] == INSERT
    shifted[0] = False
    cmds["arg"][shifted] += h
    return dict(name=stream["name"] + "_plain", cmds=cmds, lit=stream["lit"], ins=np.concatenate([stream["hist"], stream["ins"]]),
                raw=np.concatenate([stream["hist"], stream["raw"]]), segs=stream["segs"])


class HStream(cc.Stream):
    """one stream under construction in front of `hist` (uint8[]); `hist_at` = where its history begins inside the batch's dictionary
    (modes "shared" and "overlap"), or None"""

    def __init__(self, name, fam, data, rng, hist, hist_at=None):
        super().__init__(name, fam, data, rng)
        self.hist, self.hist_at = np.asarray(hist, np.uint8), hist_at
        self.h = self.hist.size

    def copy(self, n, d):
        assert n == 0 or 1 <= d <= self.produced + self.h, (self.name, n, d, self.produced, self.h)
        self.recs.append((COPY, n, d)); self.produced += n
        return self

    def reach(self, n, back):
        """a copy whose source begins `back` bytes in front of out[0]"""
        return self.copy(n, self.produced + back)

    def done(self):
        lit = np.concatenate(self.lits) if self.lits else np.zeros(0, np.uint8)
        ins = np.frombuffer(bytes(self.inss), dtype=np.uint8).copy()
        cmds = cc.commands(self.recs)
        raw, segs = execute_with_history(cmds, lit, ins, self.hist)
        assert raw.size == self.produced
        return dict(name=self.name, cmds=cmds, lit=lit, ins=ins, raw=raw, segs=segs, hist=self.hist, hist_at=self.hist_at)


def reaching_copies(stream):
    """[(index of the command, pos, len, distance)] of the stream's copies whose source begins in front of out[0]"""
    out, pos = [], 0
    for i, (kind, n, arg, _) in enumerate(stream["cmds"].tolist()):
        if kind == COPY and n and arg > pos:
            out.append((i, pos, n, arg))
        pos += n
    return out


def dictionary_of(fam):
    return np.random.default_rng(96500 + fam.seed).integers(0, 256, size=DICT, dtype=np.uint8)


def directed(fam, sources, mode="own"):
    """the directed batch of a family, in a fixed order: [dict(name, cmds, lit, ins, raw, segs, hist, hist_at)].  Under "own" a
    stream asked for h history bytes gets h bytes of its own; under "shared" every stream with a history gets the whole dictionary
    (h = 4096: the cases keep their shape, their distances follow h); under "overlap" it gets a window of h bytes of the dictionary."""
    assert mode in MODES
    rng = np.random.default_rng(96000 + fam.seed)
    data = sc._Data(sources, rng)
    D = dictionary_of(fam)
    count = [0]

    def S(name, h):
        count[0] += 1
        if h == 0:
            return HStream(name, fam, data, rng, np.zeros(0, np.uint8))
        if mode == "own":
            return HStream(name, fam, data, rng, data.take(h))
        if mode == "shared":
            return HStream(name, fam, data, rng, D, 0)
        at = (count[0] * 37) % (DICT - h + 1)
        return HStream(name, fam, data, rng, D[at:at + h], at)
    out = []
    for h in SIZES:                                             # a Literal as the first command: last8 = history's tail behind zeros
        out.append(S(f"first_lit_h{h}", h).lit(20).done())
    for h in (1, 8, 17):                                        # Literal commands that start at pos 1 .. 7 behind a short copy from history
        for p in range(1, 8):
            s = S(f"lit_at_pos{p}_h{h}", h)
            out.append(s.copy(p, 1 + p % s.h).lit(12).done())
    for k, h in enumerate(SIZES[1:]):                           # a COPY as the very first command: the oldest and the newest history byte
        s = S(f"copy_first_oldest_h{h}", h)
        out.append(s.copy(LENGTHS[k % len(LENGTHS)], s.h).lit(9).done())
        s = S(f"copy_first_newest_h{h}", h)
        out.append(s.copy(LENGTHS[(k + 4) % len(LENGTHS)], 1).lit(9).done())
    for j in range(17):                                         # source starts in history, ends in the output: the crossing at byte j of the copy
        out.append(S(f"cross_at{j}", 64).lit(24).reach(j + 5, j).lit(5).done())     # (j = 0: it starts exactly at out[0])
    for k, n in enumerate(LENGTHS):                             # ... at every length, still not overlapping
        out.append(S(f"cross_len{n}", 64).lit(310).reach(n, (5 * k + 1) % 17).lit(3).done())
    for pos in (1, 5, 16, 17):                                  # overlapping, pos < distance < len: the period straddles the history's end
        for d in range(max(pos + 1, 2), 41):
            lens = [n for n in (d + 1,) + LENGTHS if n > d]
            out.append(S(f"overlap_pos{pos}_d{d}", 64).lit(pos).copy(lens[(pos + d) % len(lens)], d).lit(4).done())
    out.append(S("reach_then_copy_of_it_then_lit", 64).lit(3).reach(20, 10).copy(12, 20).lit(8).done())
    out.append(S("reach_then_lit_near_start", 9).reach(5, 9).lit(10).done())         # last8 = 3 history bytes + 5 copied from history
    out.append(S("reach_then_lit", 64).lit(10).reach(9, 30).lit(6).done())
    out.append(S("no_history", 0).lit(20).copy(9, 4).ins(5).lit(7).done())
    out.append(S("far_reach", 4096).lit(50).reach(300, 4096).lit(2).done())          # the oldest byte of a 4096-byte history, 300 bytes on
    out.append(S("insert_then_reach", 64).ins(7).reach(30, 20).lit(5).done())
    for k in range(10):                                         # random fill
        s = S(f"random{k}", int(rng.integers(0, 100)))
        for _ in range(int(rng.integers(2, 30))):
            kind = int(rng.integers(0, 4))
            if kind == 0 or s.produced + s.h == 0:
                s.lit(int(rng.integers(1, 40)))
            elif kind == 1:
                s.ins(int(rng.integers(1, 30)), int(rng.integers(0, 4)))
            else:
                s.copy(int(rng.integers(1, 60)), int(rng.integers(1, s.produced + s.h + 1)))
        out.append(s.done())
    # the rANS chunk seam (literal 32 768) inside a Literal command of a stream whose copies reach into history before and behind it
    s = S("chunk_seam_spanned", 64).reach(6, 60).lit(cc.CHUNK - 9).reach(20, 30).lit(30).reach(7, 64).lit(211).done()
    assert s["lit"].size == 33000
    out.append(s)
    assert len(set(s["name"] for s in out)) == len(out) <= 300
    return out


def encode_extras(fam, sources):
    """further lists for the encoder's prepare kernel (64 commands per block, 16-byte pieces): a history-reaching copy as command
    62 .. 65 of a list, and a copy source that crosses the history's end at each byte 0 .. 15 of a piece the copy covers whole"""
    rng = np.random.default_rng(96800 + fam.seed)
    data = sc._Data(sources, rng)
    out = []
    for at in (62, 63, 64, 65):
        s = HStream(f"reach_as_command{at}", fam, data, rng, data.take(4096))
        for i in range(at):
            s.lit(1) if i % 2 == 0 else s.copy(1, 1)
        out.append(s.reach(40, 100).lit(3).reach(5, 4096).done())
        assert out[-1]["cmds"]["kind"][at] == COPY and reaching_copies(out[-1])[0][0] == at
    for c in range(16):         # the copy covers raw 32 .. 79; its source is history up to raw 48 + c: pieces 32 (history), 48 (crossing at c), 64 (raw)
        out.append(HStream(f"piece_crossing_at{c}", fam, data, rng, data.take(64)).lit(32).copy(48, 48 + c).lit(3).done())
    return out


def cut(stream, pieces):
    """a stream WITHOUT history cut at command boundaries into `pieces` streams of about the same number of commands; piece k's
    history is every raw byte in front of it.  The insert bytes stay whole (an INSERT command keeps its offset)."""
    cmds, raw = stream["cmds"], stream["raw"]
    edges = [round(k * cmds.size / pieces) for k in range(pieces + 1)]
    starts = np.concatenate([[0], np.cumsum(cmds["len"].astype(np.int64))])
    lstarts = np.concatenate([[0], np.cumsum(np.where(cmds["kind"] == LITERAL, cmds["len"], 0).astype(np.int64))])
    out = []
    for k in range(pieces):
        a, b = edges[k], edges[k + 1]
        c = cmds[a:b].copy()
        lit = stream["lit"][int(lstarts[a]):int(lstarts[b])].copy()
        hist = raw[:int(starts[a])]
        r, segs = execute_with_history(c, lit, stream["ins"], hist)
        assert (r == raw[int(starts[a]):int(starts[b])]).all()
        out.append(dict(name=f"{stream['name']}_piece{k}", cmds=c, lit=lit, ins=stream["ins"], raw=r, segs=segs, hist=hist, hist_at=None,
                        raw_at=int(starts[a])))
    return out


def history_layout(streams, mode="own", dictionary=None):
    """The histories in memory -> dict(hist uint8[], hist_off int64[n], hist_sz int32[n]).  "own": every stream's range at alignment
    i % 16, sentinel bytes between and behind them; "shared" / "overlap": the dictionary once, at an odd offset between sentinels,
    every stream's range inside it at its hist_at."""
    off = []
    if mode == "own":
        p = 16
        for i, s in enumerate(streams):
            p += (i % 16 - p) % 16
            if off and p < off[-1] + streams[i - 1]["hist"].size + 1:
                p += 16
            off.append(p); p += s["hist"].size + 1
        buf = np.full(p + 64, HIST_SENTINEL, np.uint8)
        for s, o in zip(streams, off):
            buf[o:o + s["hist"].size] = s["hist"]
        assert sorted(set(o % 16 for o in off[:16])) == list(range(min(len(streams), 16)))
    else:
        assert dictionary is not None
        base = 5
        buf = np.full(base + dictionary.size + 64, HIST_SENTINEL, np.uint8)
        buf[base:base + dictionary.size] = dictionary
        for s in streams:
            at = s["hist_at"] if s["hist"].size else 0
            assert (buf[base + at:base + at + s["hist"].size] == s["hist"]).all()
            off.append(base + at)
    return dict(hist=buf, hist_off=np.array(off, np.int64), hist_sz=np.array([s["hist"].size for s in streams], np.int32))


def victim_base(fam, sources):
    """the stream the faulty lists are made from -- lit 10, a history-reaching copy (12 bytes from 15 bytes in front of out[0]),
    insert 4, lit 9, a copy that straddles the history's end (30 bytes, distance 39 at pos 35: 4 history bytes, then raw), lit 6 --
    and a good neighbour, both with 20 history bytes of their own"""
    rng = np.random.default_rng(96900 + fam.seed)
    data = sc._Data(sources, rng)
    v = HStream("victim", fam, data, rng, data.take(20)).lit(10).reach(12, 15).ins(4).lit(9).reach(30, 4).lit(6).done()
    g = HStream("neighbour", fam, data, rng, data.take(20)).lit(21).reach(33, 20).ins(5).lit(40).copy(5, 1).done()
    assert v["cmds"]["kind"].tolist() == [LITERAL, COPY, INSERT, LITERAL, COPY, LITERAL] and v["cmds"]["arg"][1] == 25 and v["cmds"]["arg"][4] == 39
    return v, g


def faulty_lists(victim):
    """[(what, the victim's command list)]: each must raise BAD_COMMAND in both calls; the coded bytes stay those of the good list"""
    good = victim["cmds"]; h = victim["hist"].size

    def edit(k, value):
        c = good.copy(); c["arg"][k] = value
        return c
    return [("distance pos + h + 1", edit(1, 10 + h + 1)), ("distance 0 with a history", edit(1, 0)),
            ("distance pos + h + 1 behind the first block of bytes", edit(4, 35 + h + 1)), ("distance 0xffffffff", edit(1, 0xffffffff))]


def faulty_bytes(victim):
    """[(what, history, raw)] for the encode call: each must raise BAD_COMMAND there"""
    def changed(a, at):
        b = a.copy(); b[at] ^= 0x55
        return b
    hist, raw = victim["hist"], victim["raw"]
    h = hist.size
    return [("first history byte under the history-reaching copy changed", changed(hist, h - 15), raw),
            ("last history byte under it changed", changed(hist, h - 15 + 11), raw),
            ("history byte under the straddling copy changed", changed(hist, h - 2), raw),
            ("raw byte under the straddling copy's history part changed", hist, changed(raw, 35 + 1)),
            ("raw byte under its raw part changed", hist, changed(raw, 35 + 20))]
