"""Command lists for divans_gpu_lit_decode_commands_batch, shared by the CPU tier (tests/test_command_cases_cpu.py) and the GPU tier
(tests/test_gpu_command_decode.py).  numpy only.

execute() is a plain Python executor of a command list whose literal bytes are known -- walk() of ir.cpp, cmd_to_raw of the
reference: it returns the raw bytes and the segments (len, btype, last8) the literal coder sees, from which the C oracle
(po.lit_segments_encode) makes the coded bytes.  directed() is the batch of streams whose commands end where the decoder changes
phase; layout() places a batch in memory the way the GPU tests hand it over, at every alignment and between sentinel bytes."""
import numpy as np

import segment_cases as sc

COPY, INSERT, LITERAL = 0, 1, 3
CMD_DTYPE = np.dtype([("kind", "<u4"), ("len", "<u4"), ("arg", "<u4"), ("reserved", "<u4")])
BAD_STREAM, BAD_SEGMENT, BAD_COMMAND = 2, 4, 16
RAW_SENTINEL, CODED_SENTINEL, INS_SENTINEL = 0xA5, 0x5A, 0xC3
CHUNK = 32768       # literal bytes of one 65 536-symbol rANS chunk


def commands(records):
    c = np.zeros(len(records), dtype=CMD_DTYPE)
    for i, (kind, n, arg) in enumerate(records):
        c[i] = (kind, n, arg, 0)
    return c


def execute(cmds, lit, ins, raw_size=None):
    """-> (raw uint8[], segments of the Literal commands with bytes).  Raises ValueError on a command that cannot run (with
    `raw_size` given: also on one that would write past it)."""
    out = bytearray()
    lit = bytes(lit); ins = bytes(ins)
    lp = 0
    lens, bts, l8s = [], [], []
    for kind, n, arg, _ in cmds.tolist():
        if raw_size is not None and kind in (LITERAL, COPY, INSERT) and len(out) + n > raw_size:
            raise ValueError("command past the raw size")
        if kind == LITERAL:
            if n == 0:
                continue
            tail = bytes(out[-8:]).rjust(8, b"\0")      # zeros in front of the stream's start, newest byte last
            lens.append(n); bts.append(arg); l8s.append(int.from_bytes(tail, "little"))
            if lp + n > len(lit):
                raise ValueError("literal bytes run out")
            out += lit[lp:lp + n]; lp += n
        elif kind == COPY:
            if n == 0:
                continue
            if arg == 0 or arg > len(out):
                raise ValueError("copy from in front of the stream")
            if arg >= n:
                out += out[len(out) - arg:len(out) - arg + n]
            else:
                for _ in range(n):      # byte by byte: an overlapping copy repeats
                    out.append(out[-arg])
        elif kind == INSERT:
            if n == 0:
                continue
            if arg + n > len(ins):
                raise ValueError("insert outside its bytes")
            out += ins[arg:arg + n]
        else:
            raise ValueError("unknown kind")
    if lp != len(lit):
        raise ValueError("literal bytes left over")
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), sc.segments(lens, bts, l8s)


class Stream:
    """one stream under construction: commands, literal bytes, insert bytes"""

    def __init__(self, name, fam, data, rng):
        self.name, self.fam, self.data, self.rng = name, fam, data, rng
        self.recs, self.lits, self.inss = [], [], bytearray()
        self.produced, self.nlit, self.bt = 0, 0, 0

    def lit(self, n, bt=None):
        if bt is None:          # block types cycle where the family has several
            bt = self.bt % self.fam.n_btypes; self.bt += 1
        self.recs.append((LITERAL, n, bt))
        if n:
            self.lits.append(self.data.take(n))
        self.produced += n; self.nlit += n
        return self

    def copy(self, n, d):
        assert n == 0 or 1 <= d <= self.produced, (self.name, n, d, self.produced)
        self.recs.append((COPY, n, d)); self.produced += n
        return self

    def ins(self, n, pad=1):
        """`pad` unused bytes in front of the word inside the insert bytes: words sit at odd offsets"""
        self.inss += bytes(self.rng.integers(0, 256, size=pad, dtype=np.uint8).tolist())
        self.recs.append((INSERT, n, len(self.inss)))
        self.inss += bytes(self.rng.integers(0, 256, size=n, dtype=np.uint8).tolist())
        self.produced += n
        return self

    def done(self):
        lit = np.concatenate(self.lits) if self.lits else np.zeros(0, np.uint8)
        ins = np.frombuffer(bytes(self.inss), dtype=np.uint8).copy()
        cmds = commands(self.recs)
        raw, segs = execute(cmds, lit, ins)
        assert raw.size == self.produced
        return dict(name=self.name, cmds=cmds, lit=lit, ins=ins, raw=raw, segs=segs)


def literal_end_positions(stream):
    """positions (0..15) inside the decoder's 16-literal output group at which a Literal command of the stream ends"""
    ends = np.cumsum([n for k, n, _, _ in stream["cmds"].tolist() if k == LITERAL and n])
    return set(int((e - 1) % 16) for e in ends)


def directed(fam, sources):
    """the directed batch of a family, in a fixed order: [dict(name, cmds, lit, ins, raw, segs)]"""
    rng = np.random.default_rng(97000 + fam.seed)
    data = sc._Data(sources, rng)
    S = lambda name: Stream(name, fam, data, rng)
    out = []
    for n in (1, 15, 16, 17):                                   # a Literal command as the only command
        out.append(S(f"only_lit{n}").lit(n).done())
    s = S("lit1to17_each_then_copy")                            # a command ends at every position of the 16-byte output group
    for n in range(1, 18):
        s.lit(n)
        s.copy(1 + n % 5, min(1 + n % 3, s.produced))
    s.lit((16 - s.nlit % 16) % 16 + 16).copy(4, 2)              # ... the group's last position included
    out.append(s.done())
    assert literal_end_positions(out[-1]) == set(range(16))
    for d in (1, 2, 3, 7, 8, 15):                               # overlapping copies whose sources all lie in front of the command
        out.append(S(f"copy_d{d}_len50").lit(40).copy(50, d).lit(9).done())
    for d in (16, 17, 31, 32, 33):                              # ... and ones whose 16-byte steps read what earlier steps wrote
        out.append(S(f"copy_d{d}_len100").lit(40).copy(100, d).lit(9).done())
    out.append(S("copy_all_so_far").lit(5).copy(5, 5).lit(4).done())                # distance = every byte produced so far
    out.append(S("copy_all_so_far_overlapping").lit(5).copy(23, 5).lit(4).done())
    s = S("short_copies_after_literals")                        # last8 = a literal's tail and a copy
    for n in range(1, 10):
        s.lit(11).copy(n, 1 + (n * 3) % 11)
    out.append(s.lit(3).done())
    out.append(S("second_literal_near_start").lit(3).copy(2, 1).lit(10).done())     # fewer than eight bytes in front of it
    out.append(S("adjacent_literals_near_start").lit(3).lit(4).lit(20).done())
    out.append(S("inserts").ins(1).lit(20).ins(8, 3).lit(5).ins(16, 1).lit(7).ins(17, 5).lit(3).ins(100, 7).done())
    out.append(S("inserts_then_copies_of_them").ins(17).copy(40, 17).lit(6).ins(8, 1).copy(9, 3).lit(2).done())
    s = S("many_small")                                         # 300 one-byte literals alternating with copies of 1 .. 3 bytes
    for i in range(300):
        s.lit(1).copy(1 + i % 3, 1 + i % 2)
    out.append(s.done())
    out.append(S("ends_in_copy").lit(12).copy(30, 5).done())
    out.append(S("ends_in_insert").lit(12).ins(9).done())
    out.append(S("ends_in_empty_commands").lit(12).copy(3, 2).lit(0).copy(0, 0).ins(0, 0).done())
    out.append(S("empty_commands").lit(0).copy(0, 0).ins(0, 0).lit(10).lit(0).copy(0, 7).ins(0, 2).lit(0).lit(5).copy(6, 4).done())
    out.append(S("no_literals").ins(20).copy(30, 7).ins(3, 1).copy(10, 50).done())
    out.append(S("empty_stream").done())
    out.append(S("long_copy").lit(100).copy(4900, 100).copy(5000, 5000).lit(20).done())      # 5000 bytes, not overlapping
    out.append(S("adjacent_literals").lit(7).lit(9).done())
    while len(out) < 38:                                        # random fill
        s = S(f"random{len(out)}")
        for _ in range(int(rng.integers(2, 30))):
            kind = int(rng.integers(0, 4))
            if kind == 0 or s.produced == 0:
                s.lit(int(rng.integers(1, 40)))
            elif kind == 1:
                s.ins(int(rng.integers(1, 30)), int(rng.integers(0, 4)))
            else:
                s.copy(int(rng.integers(1, 60)), int(rng.integers(1, s.produced + 1)))
        out.append(s.done())
    # The rANS chunk seam (literal 32 768): Literal commands that end on literals 32 767, 32 768 and 32 769 with commands between
    # them -- a boundary exactly on the seam -- and, in a second stream (one stream cannot hold both), a Literal command that spans it
    s = S("chunk_seam_boundaries").lit(10000).copy(300, 77).lit(CHUNK - 1 - 10000).copy(5, 9).lit(1).ins(3).lit(1).copy(2, 1).lit(231).done()
    ends = np.cumsum([n for k, n, _, _ in s["cmds"].tolist() if k == LITERAL])
    assert {CHUNK - 1, CHUNK, CHUNK + 1} <= set(ends.tolist()) and s["lit"].size == 33000
    out.append(s)
    s = S("chunk_seam_spanned").lit(CHUNK - 9).copy(20, 3).lit(30).copy(7, 40).lit(211).done()
    assert s["lit"].size == 33000
    out.append(s)
    assert len(out) == 40
    return out


def prefix_streams(cmds, lit, ins, count):
    """`count` ragged prefixes of one command list (an IR's): stream k = its first n_k commands and the literals they cover"""
    out = []
    is_lit = cmds["kind"] == LITERAL
    lit_ends = np.cumsum(np.where(is_lit, cmds["len"], 0).astype(np.int64))
    for k in range(count):
        n = 1 + (k * 197) % 900 + (3 * k if k % 5 == 0 else 0)
        c = cmds[:n].copy()
        l = lit[:int(lit_ends[n - 1])].copy()
        raw, segs = execute(c, l, ins)
        out.append(dict(name=f"prefix{n}", cmds=c, lit=l, ins=ins, raw=raw, segs=segs))
    return out


def layout(streams, coded, lit_sizes=None):
    """The batch in memory: raw outputs start at every alignment 0 .. 15, coded streams at every 4-byte offset of a 16-byte line,
    insert bytes at odd offsets, sentinel bytes between and behind all of them.  -> dict of numpy arrays (`expect` = the raw buffer
    as a correct decode leaves it, `raw` = as it is handed over: sentinels everywhere)."""
    n = len(streams)
    raw_off, coded_off, ins_off = [], [], []
    p = 16
    for i, s in enumerate(streams):
        p += (i % 16 - p) % 16
        if raw_off and p < raw_off[-1] + streams[i - 1]["raw"].size + 1:
            p += 16
        raw_off.append(p); p += s["raw"].size + 1
    raw_total = p + 64
    p = 16
    for i, c in enumerate(coded):
        assert c.size % 4 == 0
        p += (4 * (i % 4) - p) % 16
        coded_off.append(p); p += c.size + 4
    coded_total = p + 64
    p = 1
    for s in streams:
        p |= 1
        ins_off.append(p); p += s["ins"].size + 2
    ins_total = p + 16
    expect = np.full(raw_total, RAW_SENTINEL, np.uint8)
    cbuf = np.full(coded_total, CODED_SENTINEL, np.uint8)
    ibuf = np.full(ins_total, INS_SENTINEL, np.uint8)
    for s, c, ro, co, io in zip(streams, coded, raw_off, coded_off, ins_off):
        expect[ro:ro + s["raw"].size] = s["raw"]
        cbuf[co:co + c.size] = c
        ibuf[io:io + s["ins"].size] = s["ins"]
    assert sorted(set(o % 16 for o in raw_off[:16])) == list(range(min(n, 16))) and all(o % 4 == 0 for o in coded_off)
    cmds = np.concatenate([s["cmds"] for s in streams] + [np.zeros(1, CMD_DTYPE)])       # (one spare record: the array is never empty)
    ls = np.array([s["lit"].size for s in streams] if lit_sizes is None else lit_sizes, dtype=np.int32)
    return dict(n=n, expect=expect, raw=np.full(raw_total, RAW_SENTINEL, np.uint8),
                raw_off=np.array(raw_off, np.int64), raw_sz=np.array([s["raw"].size for s in streams], np.int32),
                coded=cbuf, coded_off=np.array(coded_off, np.int64), coded_sz=np.array([c.size for c in coded], np.int32),
                ins=ibuf, ins_off=np.array(ins_off, np.int64), ins_sz=np.array([s["ins"].size for s in streams], np.int32),
                cmds=cmds.view(np.uint8), cmd_begin=np.concatenate([[0], np.cumsum([s["cmds"].size for s in streams])]).astype(np.int32),
                lit_sz=ls, lit_longest=max(int(ls.max()), 16))


def victim_base(fam, sources):
    """the stream the faulty lists are made from, and a good neighbour"""
    rng = np.random.default_rng(99000 + fam.seed)
    data = sc._Data(sources, rng)
    v = Stream("victim", fam, data, rng).lit(30).copy(20, 10).ins(12).lit(15).copy(8, 3).lit(6).done()
    g = Stream("neighbour", fam, data, rng).lit(21).copy(33, 4).ins(5).lit(40).done()
    return v, g


def faulty_lists(fam, victim):
    """[(what, the victim's command list, its literal size as told to the decoder, the status bit it must raise)]; the coded bytes
    stay those of the good list"""
    good = victim["cmds"]; nlit = victim["lit"].size

    def edit(k, field, value):
        c = good.copy(); c[field][k] = value
        return c
    assert good["kind"].tolist() == [LITERAL, COPY, INSERT, LITERAL, COPY, LITERAL]
    return [
        ("distance 0", edit(1, "arg", 0), nlit, BAD_COMMAND),
        ("distance one more than the bytes produced", edit(1, "arg", 31), nlit, BAD_COMMAND),
        ("distance 0xffffffff", edit(1, "arg", 0xffffffff), nlit, BAD_COMMAND),
        ("insert range past its bytes", edit(2, "arg", int(good["arg"][2]) + 1), nlit, BAD_COMMAND),
        ("insert offset 0xfffffffc", edit(2, "arg", 0xfffffffc), nlit, BAD_COMMAND),
        ("kind 2", edit(4, "kind", 2), nlit, BAD_COMMAND),
        ("kind 7", edit(0, "kind", 7), nlit, BAD_COMMAND),
        ("command lengths above the raw size", edit(4, "len", 8 + 5), nlit, BAD_COMMAND),
        ("a copy of 0xfffffff0 bytes", edit(4, "len", 0xfffffff0), nlit, BAD_COMMAND),
        ("command lengths below the raw size", edit(4, "len", 3), nlit, BAD_COMMAND),
        ("literal lengths above d_lit_sizes", good.copy(), nlit - 3, BAD_SEGMENT),
        ("literal lengths below d_lit_sizes", good.copy(), nlit + 3, BAD_SEGMENT),
        ("block type outside the tables", edit(3, "arg", 200), nlit, BAD_SEGMENT),
    ]
