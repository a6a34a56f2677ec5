"""Inputs and expectations for divans_gpu_lit_encode_commands_batch, shared by the CPU tier (tests/test_command_encode_cases_cpu.py)
and the GPU tier (tests/test_gpu_command_encode.py).  numpy only.

prepare() is a plain restatement of the device step in front of the segment encoders (lit_commands.hip): from a stream's raw bytes
and its command list to the literal bytes in command order and one segment per Literal command with bytes -- or to the status bit
the list raises.  count_edges() is a batch whose command counts sit around the kernel's block of 64 commands, faulty_inputs() the
lists and raw buffers that must be refused (and the two that must not)."""
import numpy as np

import command_cases as cc
import segment_cases as sc

BLOCK = 64          # commands per scan block of lit_commands_prepare_kernel: its only block size (one command per lane of a wave)
PIECE = 16          # raw bytes per lane and step of its data walk; a wave moves 64 * PIECE = 1024 bytes per step


def prepare(cmds, raw, ins, n_btypes, lit_cap):
    """-> (literal bytes, segments) or the status bit.  Every command is checked first, in list order, and the first one that
    cannot run decides the bit (a command of length 0 is checked for its kind alone); then the bytes are compared."""
    raw = np.asarray(raw, np.uint8); ins = np.asarray(ins, np.uint8)
    pos = lpos = 0
    todo = []
    for kind, n, arg, _ in cmds.tolist():
        if kind not in (cc.COPY, cc.INSERT, cc.LITERAL):
            return cc.BAD_COMMAND
        if n == 0:
            continue
        if pos + n > raw.size:
            return cc.BAD_COMMAND
        if kind == cc.LITERAL:
            if arg >= n_btypes or lpos + n > lit_cap:
                return cc.BAD_SEGMENT
            lpos += n
        elif kind == cc.COPY:
            if arg == 0 or arg > pos:
                return cc.BAD_COMMAND
        elif arg > ins.size or n > ins.size - arg:
            return cc.BAD_COMMAND
        todo.append((kind, pos, n, arg))
        pos += n
    if pos != raw.size:
        return cc.BAD_COMMAND
    lits, lens, bts, l8s = [], [], [], []
    for kind, p, n, arg in todo:
        here = raw[p:p + n]
        if kind == cc.LITERAL:
            tail = bytes(raw[max(p - 8, 0):p]).rjust(8, b"\0")      # zeros in front of the stream's start, newest byte last
            lits.append(here); lens.append(n); bts.append(arg); l8s.append(int.from_bytes(tail, "little"))
        elif kind == cc.COPY:
            if not (here == raw[p - arg:p - arg + n]).all():        # every source byte already exists: raw[q] == raw[q - distance]
                return cc.BAD_COMMAND
        elif not (here == ins[arg:arg + n]).all():
            return cc.BAD_COMMAND
    lit = np.concatenate(lits) if lits else np.zeros(0, np.uint8)
    return lit, sc.segments(lens, bts, l8s)


def same_lists(got, lit, segs):
    """prepare()'s result against the expected literals and segments"""
    if isinstance(got, int):
        return False
    glit, gsegs = got
    return (glit.size == lit.size and (glit == lit).all() and gsegs.size == segs.size and (gsegs["len"] == segs["len"]).all()
            and (gsegs["btype"] == segs["btype"]).all() and (gsegs["last8"] == segs["last8"]).all())


def _counted(name, fam, data, rng, count):
    """a stream of exactly `count` commands: the last command of every block of BLOCK is a Literal command and the first command of
    the next block a Copy that reads it; in between literals, copies, inserts and empty commands take turns"""
    s = cc.Stream(name, fam, data, rng)
    for i in range(count):
        at = i % BLOCK
        if at == BLOCK - 1 or i == 0:
            s.lit(5 + i % 7)
        elif at == 0:
            s.copy(9, 1 + (i // BLOCK) % 4)  # distance 1 .. 4 <= the 5 .. 11 literals in front of it; 9 bytes: it overlaps, too
        elif i % 11 == 5:
            s.ins(1 + i % 6, i % 3)
        elif i % 13 == 7:
            s.copy(0, 0) if i % 2 else s.lit(0)
        elif i % 3 == 1:
            s.copy(1 + i % 9, 1 + i % min(s.produced, 23))
        else:
            s.lit(1 + i % 4)
    out = s.done()
    assert out["cmds"].size == count
    for i in range(BLOCK, count, BLOCK):
        assert out["cmds"]["kind"][i - 1] == cc.LITERAL and out["cmds"]["kind"][i] == cc.COPY and out["cmds"]["arg"][i] <= out["cmds"]["len"][i - 1]
    return out


def count_edges(fam, sources):
    """streams whose command counts sit around the block edges of the prepare kernel's scans, and the contexts near a stream's start"""
    rng = np.random.default_rng(98000 + fam.seed)
    data = sc._Data(sources, rng)
    out = [_counted(f"count{n}", fam, data, rng, n) for n in (0, 1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 1000)]
    S = lambda name: cc.Stream(name, fam, data, rng)
    out.append(S("last8_spans_three_commands").lit(20).copy(3, 5).ins(2).lit(9).done())        # 3 literals, 3 copied, 2 inserted bytes
    out.append(S("second_literal_near_start").lit(3).copy(2, 1).lit(10).done())                # five bytes in front of it
    # the data walk's edges: commands that end just in front of, on and just behind a lane's piece and a wave's step
    s = S("piece_edges")
    for n in (PIECE - 1, PIECE, PIECE + 1, 64 * PIECE - 1, 64 * PIECE, 64 * PIECE + 1):
        s.lit(n).copy(n, 1 + n // 2).ins(n, 1)
    out.append(s.done())
    assert [s["cmds"].size for s in out[:10]] == [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000]
    return out


def _changed(stream, at):
    raw = stream["raw"].copy()
    raw[at] ^= 0x55
    return raw


def faulty_inputs(fam, victim, sources):
    """[dict(what, cmds, raw, ins, lit_cap, bit, lit, segs)]: bit = the status bit the input must raise, 0 = it must pass and give
    (lit, segs).  `victim` = cc.victim_base()'s: lit 30, copy (20, 10), insert 12, lit 15, copy (8, 3), lit 6 -- 91 raw bytes."""
    good = victim["cmds"]
    assert good["kind"].tolist() == [cc.LITERAL, cc.COPY, cc.INSERT, cc.LITERAL, cc.COPY, cc.LITERAL] and good["len"].tolist() == [30, 20, 12, 15, 8, 6]
    nlit = victim["lit"].size
    cap = 64
    out = []

    def add(what, bit, cmds=None, raw=None, lit_cap=cap, base=victim, lit=None, segs=None):
        out.append(dict(what=what, bit=bit, cmds=base["cmds"] if cmds is None else cmds, raw=base["raw"] if raw is None else raw, ins=base["ins"],
                        lit_cap=lit_cap, lit=lit, segs=segs))
    for what, cmds, _, bit in cc.faulty_lists(fam, victim):
        if bit == cc.BAD_COMMAND or what == "block type outside the tables":
            add(what, bit, cmds=cmds)
    assert sum(e["bit"] == cc.BAD_COMMAND for e in out) == 10 and sum(e["bit"] == cc.BAD_SEGMENT for e in out) == 1
    # lengths that add up to the raw size modulo 2^32: a sum kept in 32 bits would take this list for the good one
    wrap = np.concatenate([good[:4], cc.commands([(cc.COPY, 0xfffffff0, 3), (cc.COPY, 0x10, 3)]), good[4:]])
    add("lengths that add up to the raw size modulo 2^32", cc.BAD_COMMAND, cmds=wrap)
    add("literal lengths one above lit_stream_len", cc.BAD_SEGMENT, lit_cap=nlit - 1)
    add("lit_stream_len exactly the literal total", 0, lit_cap=nlit, lit=victim["lit"], segs=victim["segs"])
    add("first byte of a copy's target changed", cc.BAD_COMMAND, raw=_changed(victim, 30))
    add("last byte of a copy's target changed", cc.BAD_COMMAND, raw=_changed(victim, 49))
    add("byte of an overlapping copy beyond its first period changed", cc.BAD_COMMAND, raw=_changed(victim, 30 + 10 + 3))
    rng = np.random.default_rng(99500 + fam.seed)
    long_copy = cc.Stream("long_copy", fam, sc._Data(sources, rng), rng).lit(100).copy(4900, 100).copy(5000, 5000).lit(20).done()
    add("byte at a multiple of 16 inside a 5000-byte copy changed", cc.BAD_COMMAND, raw=_changed(long_copy, 5000 + 16 * 131), lit_cap=128, base=long_copy)
    add("last byte of an insert changed", cc.BAD_COMMAND, raw=_changed(victim, 50 + 11))
    # a literal byte no later copy reads: nothing to object to, the changed byte is simply what gets coded
    raw = _changed(victim, 85 + 2)
    lit = victim["lit"].copy(); lit[45 + 2] ^= 0x55
    add("byte inside the last literal command changed", 0, raw=raw, lit=lit, segs=victim["segs"])
    return out
