"""Audit of the vector-memory traffic the kernels hide from the compiler, on hipcc's gfx950 assembly.

Six places in the device code issue loads or stores through `asm volatile` (Table2::gload_async, the rANS encode kernels'
16-deep prefetch, rans_store_word, bk_store_quad / _pair / _word).  hipcc does not count such operations in its s_waitcnt
bookkeeping and treats a hidden load's destination as written at ;;#ASMEND, so it may read, copy, spill or reuse the register
before the data lands.  Whether it does depends on register allocation, i.e. on every edit, flag and compiler release; a
parity test only sees it when the data happens to be late.  This module reads the assembly and checks three contracts.

Structure.  Inline asm is what stands between ;;#ASMSTART and ;;#ASMEND.  A function starts at `_Z...: ; @` and ends at
.Lfunc_end.  Each function gets a control-flow graph from its .LBB labels, s_branch and s_cbranch_*; the contracts are
forward data-flow problems over it, solved to a fixed point (states merge by union at a join), so a block laid out behind a
loop body is followed where control goes and not where the text goes.  Instructions are classified by prefix only (buffer_,
global_, flat_, ds_, scratch_, v_, s_waitcnt, s_nop, branches, writes of exec); the first operand of a v_ instruction, of a
load and of a returning ds_ instruction is its destination, every other register operand is a source.

Contract A -- hidden loads with a VGPR destination.  From the asm load on, along every path, until a wait that covers it, no
instruction may read the destination, write it under an exec that can include the loading lanes, copy it (v_mov, v_accvgpr)
or store it to scratch, and none may be pending at a call or an indirect jump.  Pending at s_endpgm is allowed.
  Covering waits.  A hidden buffer_ load (the decoders) is covered by vmcnt(0) only.  A hidden global_ load (the rANS ring)
  is also covered by a counted wait: vector-memory LOADS return in order while stores -- hidden or visible, they share the
  counter -- may be acknowledged early.  If load k were still outstanding, so would be every load issued after it; with at
  least N loads issued after load k on every path, vmcnt(N) (at most N operations outstanding) therefore proves k complete,
  whatever the stores in between did.  This is the source's own argument ("at most 12 outstanding proves the quad requested
  three steps ago"): a step issues four loads, three steps make twelve.  Only buffer_ / global_ / scratch_ loads count as
  younger loads (a flat_ load may return out of order); the count merges by minimum at a join.
  Modelling decision 1, the guarded wait.  The byte loop waits only `if (__ballot(missed))`; hipcc emits a block that holds
  nothing but the asm `s_waitcnt vmcnt(0)`, entered by fall-through and skipped by a wave-uniform branch (s_cbranch_vcc* /
  scc*) to the block behind it.  The skipping edge carries "nothing pending": the ballot is over the `missed` flags of exactly
  these loads, so where it is zero no lane of the wave issued one.  The checker recognises the shape, not the ballot's
  operand; Audit.guarded_waits counts the sites.
  Modelling decision 2, the complementary exec arm.  hipcc lowers if/else to `s_and_saveexec X, c; s_xor X, exec, X` (X := the
  else mask), the then arm, `s_or_saveexec X, X; s_xor exec, exec, X` or `s_andn2_saveexec X, X` (exec := the else mask), the
  else arm, `s_or exec, exec, X`.  A load issued in the then arm ran under a subset of the then mask (hipcc's control flow is
  structured: inside the arm exec only narrows, or is restored by the s_or that closes a nested region), and the else arm's
  exec is disjoint from it.  VALU and memory instructions act per lane, so an access of the destination in the else arm
  touches no lane whose data is in flight (the pinned decoder's ds_read_u16 into the load's register for the lanes that hit).
  Such accesses are exempt until exec is written by anything but a narrowing (s_and_saveexec, s_and / s_andn2 exec, exec, Y);
  Audit.complement_writes and .complement_reads count them.
  Modelling decision 3, the wave-uniform flag.  Where the miss test is uniform (the pinned decoder's first row of a stream:
  every lane's rank comes from one LDS byte) hipcc branches on the scalar unit instead: `s_mov_b64 X, -1`, the load's block
  ends with `s_mov_b64 X, 0`, and the LDS read of the same register sits behind `s_andn2_b64 vcc, exec, X; s_cbranch_vccnz`.
  The two blocks exclude each other through X, which a merge of paths forgets.  Each pending load therefore carries the
  constants (0 / -1, from s_mov_b64 only) of the register pairs that feed such a branch, as its own path set them, and does
  not flow along the edge that its value of X rules out (vcc = exec & ~X or exec & X; exec is not zero where a vector load
  was issued).  Any other write of X forgets the constant.  Audit.flag_branches counts the branches that pruned a load.

Contract B -- hidden stores.  (1) An asm store wider than 8 bytes needs two wait states (what an `s_nop 1` ending the string would give)
before its data registers are overwritten: either the string itself pads, or no instruction within two states behind
;;#ASMEND (an instruction is one state, s_nop N is N + 1; every path is followed) writes them.  (2) A hidden store that
feeds a later load of the same kernel must be separated from it by vmcnt(0) (only that proves a store complete).  What the
assembly can show of "feeds": two buffer_ accesses through the same descriptor registers, or two global_ accesses off the
same scalar base, may alias and are findings.  The hidden stores of today's build all address through a VGPR pair (`off`),
whose provenance the assembly does not give; loads that can run while such a store may be outstanding are counted
(Audit.store_unknown), not judged -- the source's claim for them is that a kernel never reads the plane it writes that way.

Contract C -- facts DESIGN.md asserts of one decoder instance, for all: per kernel the scratch size (metadata) and every
flat_ instruction.  A generic-pointer access other than the one flat_load_dword that selects between out_sizes[s] and the
stream_len kernel argument is a finding in a kernel that also addresses LDS (a wild ds_ offset reads zero, a wild flat
address can fault); a lit_decode2_kernel_any instance with scratch is a finding.
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _isa_compare():
    spec = importlib.util.spec_from_file_location("divans_isa_compare", os.path.join(ROOT, "scripts", "isa_compare.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Ins = namedtuple("Ins", "mnem ops text line asm")     # asm: ordinal of the inline-asm block the instruction stands in, or -1
Finding = namedtuple("Finding", "rule kernel line text detail")


class Function:
    def __init__(self, name):
        self.name, self.ins, self.labels, self.meta = name, [], {}, {}


_VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
_SREG = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")
_START = re.compile(r"^(_Z\w+):\s*; @")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
VMEM = ("buffer_", "global_", "flat_", "scratch_")


def _regs(rx, s):
    out = set()
    for m in rx.finditer(s):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def vregs(s):
    return _regs(_VREG, s)


def _operands(ops):
    return [o.strip() for o in re.split(r",(?![^\[]*\])", ops)] if ops else []


def parse(text):
    """The functions of one assembly file, in file order."""
    funcs, cur, asm, n_asm = [], None, -1, 0
    for no, raw in enumerate(text.split("\n"), 1):
        m = _START.match(raw)
        if m:
            cur, asm = Function(m.group(1)), -1
            funcs.append(cur)
            continue
        if cur is None:
            continue
        line = raw.strip()
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if line.startswith(";;#ASMSTART"):
            asm, n_asm = n_asm, n_asm + 1
            continue
        if line.startswith(";;#ASMEND"):
            asm = -1
            continue
        m = _LABEL.match(line)
        if m:
            cur.labels[m.group(1)] = len(cur.ins)
            continue
        line = re.split(r";|//", line, 1)[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        parts = line.split(None, 1)
        cur.ins.append(Ins(parts[0], parts[1] if len(parts) > 1 else "", line, no, asm))
    return funcs


def vmem_load(i):
    return i.mnem.startswith(VMEM) and "_load_" in i.mnem


def vmem_store(i):
    return i.mnem.startswith(VMEM) and "_store_" in i.mnem


def dest_and_sources(i):
    """(VGPRs written, VGPRs read)."""
    ops = _operands(i.ops)
    m = i.mnem
    has_dest = (m.startswith("v_") or vmem_load(i) or (m.startswith("ds_") and ("read" in m or "permute" in m or "rtn" in m or "swizzle" in m))
                or ("_atomic_" in m and re.search(r"\b(glc|sc0)\b", i.ops) is not None))
    if not ops:
        return set(), set()
    if not has_dest:
        return set(), vregs(i.ops)
    d = vregs(ops[0])
    s = vregs(",".join(ops[1:]))
    if m.startswith(("v_mac", "v_fmac", "v_writelane", "v_swap", "v_dot", "v_mfma")) or "dst_unused:UNUSED_PRESERVE" in i.ops:
        s |= d
    return d, s


def vmcnt_of(i):
    """The vmcnt bound of an s_waitcnt, or None if it leaves vmcnt alone."""
    if i.mnem != "s_waitcnt":
        return None
    m = re.search(r"vmcnt\((\d+)\)", i.ops)
    if m:
        return int(m.group(1))
    if "cnt(" in i.ops:
        return None
    v = int(i.ops, 0)           # the raw gfx9 immediate: vmcnt is bits 3:0 and 15:14
    return (v & 15) | ((v >> 14) & 3) << 4


def _pair(op):
    r = sorted(_regs(_SREG, op))
    return (r[0], r[-1]) if r else None


def exec_write(i):
    ops = _operands(i.ops)
    return "saveexec" in i.mnem or i.mnem.startswith("v_cmpx") or (i.mnem.startswith("s_") and bool(ops) and ops[0] in ("exec", "exec_lo", "exec_hi"))


def exec_narrows(i):
    ops = _operands(i.ops)
    if i.mnem.startswith("s_and_saveexec"):
        return True
    return i.mnem in ("s_and_b64", "s_andn2_b64") and len(ops) == 3 and ops[0] == "exec" and ops[1] == "exec"


class Cfg:
    def __init__(self, f):
        ins, n = f.ins, len(f.ins)
        leaders = {0} | {v for v in f.labels.values() if v < n}
        for k, i in enumerate(ins):
            if i.mnem.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")) and k + 1 < n:
                leaders.add(k + 1)
        self.starts = sorted(leaders) if n else []
        self.block_of = {s: b for b, s in enumerate(self.starts)}
        self.ends = self.starts[1:] + [n]
        self.succ = []
        for b, s in enumerate(self.starts):
            last = ins[self.ends[b] - 1]
            out = []
            if last.mnem.startswith("s_branch"):
                out = [self.block_of[f.labels[last.ops.strip()]]]
            elif last.mnem.startswith("s_cbranch"):
                out = [self.block_of[f.labels[last.ops.strip()]]]
                if b + 1 < len(self.starts):
                    out.append(b + 1)
            elif last.mnem.startswith(("s_endpgm", "s_setpc")):
                out = []
            elif b + 1 < len(self.starts):
                out = [b + 1]
            self.succ.append(out)
        self.pred = [[] for _ in self.starts]
        for b, out in enumerate(self.succ):
            for t in out:
                self.pred[t].append(b)


def guarded_wait_edges(f, cfg):
    """{(block in front, block behind)} of the edges that skip a block holding only the asm vmcnt(0) (decision 1)."""
    edges = set()
    for b in range(1, len(cfg.starts) - 1):
        body = f.ins[cfg.starts[b]:cfg.ends[b]]
        if not body or any(i.asm < 0 or vmcnt_of(i) != 0 for i in body):
            continue
        last = f.ins[cfg.ends[b - 1] - 1]
        if cfg.pred[b] == [b - 1] and re.match(r"s_cbranch_(vccz|vccnz|scc0|scc1)$", last.mnem) and cfg.succ[b - 1][0] == b + 1 and cfg.succ[b] == [b + 1]:
            edges.add((b - 1, b + 1))
    return edges


class Audit:
    """The result over any number of functions: findings plus the counts the contracts' docstring promises."""
    def __init__(self):
        self.findings = []
        self.hidden_loads = {}      # kernel -> number of asm loads
        self.hidden_stores = {}     # kernel -> number of asm stores
        self.asm_load_blocks = 0    # asm blocks that hold a load
        self.guarded_waits = 0
        self.complement_writes = 0
        self.complement_reads = 0
        self.flag_branches = 0
        self.store_unknown = 0
        self.flat = {}              # kernel -> [flat_ instruction texts]
        self.scratch = {}           # kernel -> bytes

    def rules(self):
        return sorted({f.rule for f in self.findings})


def _merge(dst, src):
    """Union of two contract-A states (pending: key -> younger loads, minimum wins; open / flip: intersection)."""
    if dst is None:
        return (dict(src[0]), src[1], src[2], src[3]), True
    changed = False
    pend = dst[0]
    for k, v in src[0].items():
        if k not in pend or v < pend[k]:
            pend[k] = v
            changed = True
    op, fl = dst[1] & src[1], dst[2] & src[2]
    st = dst[3] | src[3]
    if op != dst[1] or fl != dst[2] or st != dst[3]:
        changed = True
    return (pend, op, fl, st), changed


def _rekey(pend, fn):
    out = {}
    for key, v in pend.items():
        nk = fn(key)
        out[nk] = min(v, out.get(nk, 64))
    return out


def uniform_flag_branches(f, cfg):
    """{block: (flag pair, value of the flag with which the branch is TAKEN)} for blocks that end in `s_and[n2]_b64 vcc, exec, X` ...
    `s_cbranch_vcc[n]z` (decision 3)."""
    out = {}
    for b in range(len(cfg.starts)):
        last = f.ins[cfg.ends[b] - 1]
        if last.mnem not in ("s_cbranch_vccnz", "s_cbranch_vccz"):
            continue
        for k in range(cfg.ends[b] - 2, cfg.starts[b] - 1, -1):
            i = f.ins[k]
            ops = _operands(i.ops)
            if ops and ops[0] == "vcc" or (i.mnem.startswith("v_") and "vcc" in ops[:1]):
                if i.mnem in ("s_and_b64", "s_andn2_b64") and len(ops) == 3 and ops[1] == "exec" and _pair(ops[2]):
                    nonzero_when = -1 if i.mnem == "s_and_b64" else 0      # the flag's value that leaves vcc = exec, i.e. not zero
                    taken_when = nonzero_when if last.mnem == "s_cbranch_vccnz" else -1 - nonzero_when
                    out[b] = (_pair(ops[2]), taken_when)
                break
            if i.mnem.startswith("v_cmp") and not i.mnem.endswith("_e64"):
                break       # an e32 compare writes vcc implicitly
    return out


def _store_base(i):
    ops = _operands(i.ops)
    if i.mnem.startswith("buffer_"):
        return ("buffer", next((o for o in ops if o.startswith("s[")), "?"))
    if i.mnem.startswith("global_"):
        return ("global", next((o for o in ops if o.startswith("s[")), "off"))
    return (i.mnem.split("_")[0], "?")


def audit_function(f, audit, src=""):
    cfg = Cfg(f)
    ins = f.ins
    name = f.name
    if not ins:
        return
    skip_edges = guarded_wait_edges(f, cfg)
    audit.guarded_waits += len(skip_edges)
    flag_branch = uniform_flag_branches(f, cfg)
    flags = {x for x, _ in flag_branch.values()}
    pruned = set()
    loads = [k for k, i in enumerate(ins) if i.asm >= 0 and vmem_load(i)]
    stores = [k for k, i in enumerate(ins) if i.asm >= 0 and vmem_store(i)]
    if loads:
        audit.hidden_loads[name] = len(loads)
        audit.asm_load_blocks += len({ins[k].asm for k in loads})
    if stores:
        audit.hidden_stores[name] = len(stores)
    for k, i in enumerate(ins):
        if i.asm >= 0 and i.mnem.startswith("ds_") and dest_and_sources(i)[0]:
            audit.findings.append(Finding("A.unmodelled", name, i.line, i.text, "asm LDS read with a VGPR destination (lgkmcnt is not modelled)"))
    seen = set()

    def report(rule, k, detail, key=None):
        key = (rule, k, key)
        if key not in seen:
            seen.add(key)
            audit.findings.append(Finding(rule, name, ins[k].line, ins[k].text, detail))

    counted = set()     # (kind, instruction) exemptions already counted

    def step(k, state):
        """state after instruction k; state = (pending, open else masks, masks ready to flip, pending hidden-store bases)"""
        pend, opn, flip, st = state
        i = ins[k]
        d, s = dest_and_sources(i)
        # --- contract A: accesses of pending destinations
        if pend:
            drop = []
            for key in pend:
                ld, mode = key[0], key[1]
                regs = dest_and_sources(ins[ld])[0]
                wr, rd = d & regs, s & regs
                if not (wr or rd):
                    continue
                if mode == "C":
                    if wr and ("w", k) not in counted:
                        counted.add(("w", k)); audit.complement_writes += 1
                    if rd and ("r", k) not in counted:
                        counted.add(("r", k)); audit.complement_reads += 1
                    continue
                what = "v%d" % min(wr or rd)
                origin = "%s pending since line %d (%s)" % (what, ins[ld].line, ins[ld].text)
                if rd and i.mnem.startswith("scratch_store"):
                    report("A.spill", k, origin, ld)
                elif rd and i.mnem.startswith(("v_mov", "v_accvgpr")):
                    report("A.copy", k, origin, ld)
                elif rd:
                    report("A.read", k, origin, ld)
                else:
                    report("A.write", k, origin, ld)
                drop.append(key)
            if drop:
                pend = {key: v for key, v in pend.items() if key not in drop}
        if pend and i.mnem.startswith(("s_swappc", "s_setpc", "s_call")):
            for key in pend:
                report("A.call", k, "line %d (%s) pending at a call" % (ins[key[0]].line, ins[key[0]].text), key[0])
            pend = {}
        # --- contract B.2: loads under a pending hidden store
        if st and vmem_load(i):
            base = _store_base(i)
            for sb in st:
                if sb == base and base[1] not in ("off", "?"):
                    report("B.store_read", k, "a hidden store through %s %s may be outstanding" % sb)
                elif ("u", k) not in counted and sb[0] == base[0]:
                    counted.add(("u", k)); audit.store_unknown += 1
        # --- waits
        n = vmcnt_of(i)
        if n is not None:
            if n == 0:
                pend, st = {}, frozenset()
            elif pend:
                pend = {key: v for key, v in pend.items() if not (ins[key[0]].mnem.startswith("global_") and v >= n)}
        # --- memory operations issued
        if vmem_load(i) and not i.mnem.startswith("flat_") and pend:
            pend = {key: min(v + 1, 64) for key, v in pend.items()}
        if i.asm >= 0 and vmem_load(i):
            pend = dict(pend)
            pend[(k, "I", opn, frozenset())] = 0
        if i.asm >= 0 and vmem_store(i):
            st = st | {_store_base(i)}
        ops = _operands(i.ops)
        # --- the wave-uniform flags of decision 3, as each pending load's path knows them
        if pend and flags and ops and i.mnem.startswith(("s_", "v_cmp", "v_readlane", "v_readfirstlane")) and _pair(ops[0]):
            x = _pair(ops[0])
            val = {"0": 0, "-1": -1}.get(ops[1]) if i.mnem == "s_mov_b64" and len(ops) == 2 and x in flags else None
            pend = _rekey(pend, lambda key: (key[0], key[1], key[2], frozenset({f for f in key[3] if f[0][1] < x[0] or x[1] < f[0][0]} | ({(x, val)} if val is not None else set()))))
        # --- exec and the masks of decision 2
        if exec_write(i) or (i.mnem.startswith(("s_", "v_cmp", "v_readlane", "v_readfirstlane")) and ops and _pair(ops[0])):
            x = _pair(ops[0]) if ops else None
            flipped = None
            if i.mnem.startswith("s_or_saveexec") and len(ops) == 2 and ops[0] == ops[1] and x in opn:
                opn, flip = opn - {x}, flip | {x}
                x = None
            elif i.mnem.startswith("s_andn2_saveexec") and len(ops) == 2 and ops[0] == ops[1] and x in opn:
                opn, flipped = opn - {x}, x
                x = None
            elif i.mnem == "s_xor_b64" and len(ops) == 3 and ops[0] == "exec" and ops[1] == "exec" and _pair(ops[2]) in flip:
                flipped = _pair(ops[2])
                flip = flip - {flipped}
            elif i.mnem == "s_xor_b64" and len(ops) == 3 and ops[1] == "exec" and k > 0 and ins[k - 1].mnem.startswith("s_and_saveexec") \
                    and _pair(_operands(ins[k - 1].ops)[0]) == _pair(ops[2]):
                # X := the else mask: a region opens; loads issued before it are not inside it
                pend = _rekey(pend, lambda key: (key[0], key[1], key[2] - {x}, key[3]))
                opn, flip = opn | {x}, flip - {x}
                x = None
            if x is not None:       # any other write of a register pair forgets what it held
                hit = {p for p in opn | flip if not (p[1] < x[0] or x[1] < p[0])}
                if hit:
                    opn, flip = opn - hit, flip - hit
                    pend = _rekey(pend, lambda key: (key[0], key[1], key[2] - hit, key[3]))
            if exec_write(i):
                new = {}
                for key, v in pend.items():
                    ld, mode, o, facts = key
                    if flipped is not None and flipped in o:
                        mode, o = "C", o - {flipped}
                    elif mode == "C" and not exec_narrows(i):
                        mode = "I"
                    nk = (ld, mode, o, facts)
                    new[nk] = min(v, new.get(nk, 64))
                pend = new
        return pend, opn, flip, st

    entry = [None] * len(cfg.starts)
    entry[0] = ({}, frozenset(), frozenset(), frozenset())
    work = [0]
    while work:
        b = work.pop()
        state = entry[b]
        state = (dict(state[0]), state[1], state[2], state[3])
        for k in range(cfg.starts[b], cfg.ends[b]):
            state = step(k, state)
        for t in cfg.succ[b]:
            out = state
            if (b, t) in skip_edges:
                out = ({}, state[1], state[2], state[3])
            elif b in flag_branch and state[0] and len(cfg.succ[b]) == 2 and cfg.succ[b][0] != cfg.succ[b][1]:
                x, taken_when = flag_branch[b]
                want = taken_when if t == cfg.succ[b][0] else -1 - taken_when
                keep = {key: v for key, v in state[0].items() if (x, -1 - want) not in key[3]}
                if len(keep) != len(state[0]):
                    pruned.add(b)
                    out = (keep, state[1], state[2], state[3])
            entry[t], changed = _merge(entry[t], out)
            if changed and t not in work:
                work.append(t)
    audit.flag_branches += len(pruned)
    # --- contract B.1: the pad behind a wide asm store
    for k in stores:
        i = ins[k]
        if not re.search(r"dwordx[34]$", i.mnem):
            continue
        ops = _operands(i.ops)
        data = vregs(ops[0] if i.mnem.startswith("buffer_") else ops[1])
        states, j = 0, k + 1
        while j < len(ins) and ins[j].asm == i.asm:
            states += int(ins[j].ops, 0) + 1 if ins[j].mnem == "s_nop" else 1
            j += 1

        def walk(j, left, depth=0):
            while left > 0 and j < len(ins) and depth < 8:
                x = ins[j]
                if dest_and_sources(x)[0] & data:
                    report("B.store_pad", j, "writes data of the %s at line %d within %d wait state(s)" % (i.mnem, i.line, 2 - left + 1), k)
                    return
                if x.mnem.startswith(("s_endpgm", "s_setpc")):
                    return
                if x.mnem.startswith(("s_branch", "s_cbranch")):
                    for t in cfg.succ[cfg.block_of[max(s for s in cfg.starts if s <= j)]]:
                        walk(cfg.starts[t], left - 1, depth + 1)
                    return
                left -= int(x.ops, 0) + 1 if x.mnem == "s_nop" else 1
                j += 1
        walk(j, 2 - states)
    # --- contract C
    flat = [i.text for i in ins if i.mnem.startswith("flat_")]
    if flat:
        audit.flat[name] = flat
    audit.scratch[name] = f.meta.get("private_segment_fixed_size", 0)
    uses_lds = any(i.mnem.startswith("ds_") for i in ins)
    if uses_lds and (len(flat) > 1 or any(not t.startswith("flat_load_dword ") for t in flat)):
        audit.findings.append(Finding("C.flat", name, ins[0].line, "; ".join(flat), "generic-pointer access beyond the one stream-length select, in a kernel that addresses LDS"))
    if "lit_decode2_kernel_any" in name and audit.scratch[name]:
        audit.findings.append(Finding("C.scratch", name, ins[0].line, "", "%d bytes of scratch in a lit_decode2_kernel_any instance" % audit.scratch[name]))


def redefinitions(f):
    """The record DESIGN.md section 4 keeps.  For every hidden load of `f`: (line, text, destination registers, [(line, text, wait)]) --
    the instructions that are first to write a destination register again on some path from the load, each with the line of the
    last vmcnt(0) passed on the way ("guard" for the skipping edge of a guarded wait), or None where the path has none."""
    cfg = Cfg(f)
    skip = guarded_wait_edges(f, cfg)
    out = []
    for k, i in enumerate(f.ins):
        if i.asm < 0 or not vmem_load(i):
            continue
        regs = dest_and_sources(i)[0]
        found, seen, work = {}, set(), [(k + 1, None)]
        while work:
            j, wait = work.pop()
            if j >= len(f.ins) or (j, wait is None) in seen:
                continue
            seen.add((j, wait is None))
            x = f.ins[j]
            if dest_and_sources(x)[0] & regs:
                found.setdefault((x.line, x.text), wait)
                if wait is None:
                    found[(x.line, x.text)] = None
                continue
            if vmcnt_of(x) == 0:
                wait = x.line
            if j + 1 in cfg.block_of or j + 1 == len(f.ins):
                b = cfg.block_of[max(s for s in cfg.starts if s <= j)]
                work += [(cfg.starts[t], "guard" if (b, t) in skip else wait) for t in cfg.succ[b]]
            else:
                work.append((j + 1, wait))
        out.append((i.line, i.text, sorted(regs), sorted((l, t, w) for (l, t), w in found.items())))
    return out


def audit_text(text, audit=None, meta=None):
    """Run the three contracts over every function of one assembly text."""
    audit = audit or Audit()
    for f in parse(text):
        f.meta = (meta or {}).get(f.name, {})
        audit_function(f, audit)
    return audit


def metadata(text):
    """{kernel: its metadata record's figures}, through scripts/isa_compare.py's reader."""
    ic = _isa_compare()
    lines = []
    for l in text.split("\n"):
        l = re.split(r";|//", l, 1)[0].rstrip()
        if l.strip() and not re.match(r"\s*\.(file|ident|loc)\b", l):
            lines.append(l)
    if "amdhsa.kernels:" not in lines:
        return {}
    return {name: meta for name, _, meta in ic.kernels(lines)}


def demangle(names):
    return _isa_compare().demangle(list(names))


def compile_assembly(sources=None, tree=ROOT, jobs=16):
    """{source: assembly text} of the default build's HIP sources, compiled in parallel into a temporary directory."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from divans_amd import build as dbuild
    sources = sources or [s for s in dbuild.SOURCES if s.endswith(".hip")]
    cc = dbuild.hipcc()
    with tempfile.TemporaryDirectory() as tmp:
        def one(src):
            out = os.path.join(tmp, src + ".s")
            res = subprocess.run([cc] + dbuild.FLAGS + ["-S", "--cuda-device-only", "-x", "hip", os.path.join(tree, "divans_amd", "csrc", src), "-o", out],
                                 capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError("hipcc failed on %s:\n%s" % (src, res.stdout + res.stderr))
            with open(out) as fh:
                return fh.read()
        with ThreadPoolExecutor(max_workers=max(1, min(jobs, 16, len(sources)))) as ex:
            return dict(zip(sources, ex.map(one, sources)))


def audit_build(texts):
    """One Audit over {source: assembly text}."""
    audit = Audit()
    for src in sorted(texts):
        audit_text(texts[src], audit, metadata(texts[src]))
    return audit


if __name__ == "__main__":
    # python tests/tools/isa_audit.py [--trace PART_OF_A_DEMANGLED_NAME] [assembly files; none: compile the default build]
    args = sys.argv[1:]
    want = args.pop(args.index("--trace") + 1) if "--trace" in args else None
    args = [x for x in args if x != "--trace"]
    texts = {os.path.basename(p): open(p).read() for p in args} if args else compile_assembly()
    if want:
        for src in sorted(texts):
            funcs = parse(texts[src])
            nice = demangle([f.name for f in funcs])
            for f in funcs:
                if want in nice[f.name]:
                    for line, text, regs, redefs in redefinitions(f):
                        print("%s | line %d | %s" % (nice[f.name], line, text))
                        for l, t, w in redefs:
                            print("    next written at line %d (%s); vmcnt(0) in front of it: %s" % (l, t, w))
        sys.exit(0)
    a = audit_build(texts)
    nice = demangle({f.kernel for f in a.findings})
    for f in a.findings:
        print("%s | %s | line %d | %s | %s" % (f.rule, nice.get(f.kernel, f.kernel), f.line, f.text, f.detail))
    print("findings %d; hidden loads %d in %d kernels (%d asm blocks); hidden stores %d in %d kernels" % (
        len(a.findings), sum(a.hidden_loads.values()), len(a.hidden_loads), a.asm_load_blocks, sum(a.hidden_stores.values()), len(a.hidden_stores)))
    print("exemptions: guarded waits %d, complement-arm writes %d, complement-arm reads %d, uniform-flag branches %d; loads under a hidden store of unknown base %d" % (
        a.guarded_waits, a.complement_writes, a.complement_reads, a.flag_branches, a.store_unknown))
