#!/usr/bin/env python3
"""Cost of a COPY that reaches into a stream's history (divans_gpu_lit_decode_commands_history_batch) against a copy of the same
length inside the stream's own output.  An IR's device command list is cut at command boundaries into P pieces, piece k's history
being every raw byte in front of it (tests/history_cases.py: cut()).  For every piece behind the first, two lists:
  A  the piece as cut: copies whose distance exceeds the bytes produced so far read the history;
  B  the same list with every such copy that can be redirected (len <= pos) given the distance pos: same length, same place, source
     inside the output.  Copies that cannot (the first few of a piece) stay as they are in both lists.
Both are coded by the encode call (the raw bytes of B are what its list produces), then N replicas of the piece -- a raw range of
their own each, coded bytes, lists and history shared -- are decoded through the history call.  N streams are resident all at once,
so a batch time is one stream's time, and (A - B) / redirected copies is the extra time of ONE history-reaching copy.
One JSON line per (piece, mixing).

usage: command_history_rate.py [--streams N] [--reps K] [--pieces P] [ir name]"""
import argparse, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--pieces", type=int, default=8)
ap.add_argument("name", nargs="?", default="alice29-q11")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import divans_amd as da, irtext
import command_cases as cc, history_cases as hc

dev = torch.device("cuda", 0)
n = args.streams
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def timed(fn):
    """milliseconds of `reps` calls, each between two synchronisations, after one call that is not counted"""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def redirected(piece):
    """(list B, number of copies redirected, their mean length)"""
    cmds = piece["cmds"].copy()
    lens = []
    for i, pos, ln, d in hc.reaching_copies(piece):
        if ln <= pos:
            cmds["arg"][i] = pos; lens.append(ln)
    return cmds, len(lens), (sum(lens) / len(lens) if lens else 0.0)


for mixing in (0, 2):
    ir = da.CommandIR(irtext.load_ir_text(args.name))
    cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
    cmds, ins = ir.device_commands()
    lit, _ = ir.literal_segments()
    whole = dict(name=args.name, cmds=cmds, lit=lit, ins=ins, raw=ir.expand())
    pieces = hc.cut(whole, args.pieces)
    longest = max(p["lit"].size for p in pieces)
    L = max(longest, 16) + longest % 2
    codec = da.LiteralCodec(cfg, L)
    codec.set_block_types(ir.num_block_types)
    d_hist = t(np.concatenate([whole["raw"], np.zeros(16, np.uint8)]))
    d_ins = t(np.concatenate([ins, np.zeros(16, np.uint8)]))
    for k, piece in enumerate(pieces):
        cmds_b, moved, mean_len = redirected(piece)
        if not moved:
            continue
        h = piece["hist"].size
        R, C = int(piece["raw"].size), int(piece["cmds"].size)
        raw_b, _ = hc.execute_with_history(cmds_b, piece["lit"], ins, piece["hist"])
        times = {}
        for which, c, raw in (("A", piece["cmds"], piece["raw"]), ("B", cmds_b, raw_b)):
            d_cmds = t(np.concatenate([c, np.zeros(1, cc.CMD_DTYPE)]).view(np.uint8))
            one = dict(hist=d_hist, hist_offsets=t(np.zeros(1, np.int64)), hist_sizes=t(np.array([h], np.int32)))
            outs = codec.alloc_encode_outputs(1)
            lsz = torch.zeros(1, dtype=torch.int32, device=dev)
            codec.encode_commands_batch(t(np.concatenate([raw, np.zeros(16, np.uint8)])), t(np.zeros(1, np.int64)), t(np.array([R], np.int32)), 1,
                                        t(np.array([0, C], np.int32)), d_cmds, L, outs, lsz, d_ins, t(np.zeros(1, np.int64)), t(np.array([ins.size], np.int32)), **one)
            assert codec.status() == 0 and int(lsz[0].item()) == piece["lit"].size, which
            csz = int(outs["sizes"][0].item()); coff = int(outs["offsets"][0].item())
            d_coded = torch.cat([outs["out"][coff:coff + csz].clone(), torch.zeros(64, dtype=torch.uint8, device=dev)])
            z64 = torch.zeros(n, dtype=torch.int64, device=dev)
            full = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)
            d_raw = torch.zeros(n * R + 64, dtype=torch.uint8, device=dev)
            d_roff = torch.arange(n, dtype=torch.int64, device=dev) * R
            d_cmds_n = d_cmds[:16 * C].repeat(n)        # (a list of its own per stream: the begins ascend)
            cmd_begin = torch.arange(n + 1, dtype=torch.int32, device=dev) * C
            times[which] = timed(lambda: codec.decode_commands_batch(d_coded, z64, full(csz), n, cmd_begin, d_cmds_n, full(piece["lit"].size), L, d_raw, d_roff, full(R),
                                                                     d_ins, z64, full(int(ins.size)), hist=d_hist, hist_offsets=z64, hist_sizes=full(h)))
            assert codec.status() == 0, which
            d_ref = t(raw)
            assert all(torch.equal(d_raw[j * R:(j + 1) * R], d_ref) for j in (0, n // 3, n - 1)), which
            kernel = codec.last_decode_kernel()
            del d_raw, d_cmds_n
        a, b = min(times["A"]), min(times["B"])
        print(json.dumps({"ir": args.name, "dynamic_context_mixing": mixing, "piece": k, "pieces": args.pieces, "streams": n, "history_bytes": h,
                          "raw_bytes_per_stream": R, "literal_bytes_per_stream": int(piece["lit"].size), "commands_per_stream": C,
                          "history_reaching_copies": len(hc.reaching_copies(piece)), "redirected_in_B": moved, "mean_length_of_those": round(mean_len, 2),
                          "kernel": kernel, "A_history_ms": round(a, 3), "A_ms_all": [round(x, 3) for x in times["A"]],
                          "B_inside_ms": round(b, 3), "B_ms_all": [round(x, 3) for x in times["B"]],
                          "extra_us_per_history_reaching_copy": round((a - b) * 1e3 / moved, 4)}), flush=True)
        torch.cuda.empty_cache()
    codec.close(); ir.close()
