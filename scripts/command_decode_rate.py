#!/usr/bin/env python3
"""Cost of decoding general streams from their command lists (divans_gpu_lit_decode_commands_batch): an IR's stream replicated N
times in HBM -- coded bytes, command list and raw output of its own per stream, the insert bytes shared -- decoded through
decode_commands_batch, and the same coded bytes through decode_segments_batch, which does strictly less work (no Copy / Insert
commands, no raw output, every context handed over): the floor to compare with.  One JSON line per (IR, mixing).

usage: command_decode_rate.py [--tree DIR] [--streams N] [--reps K] [ir name ...]
  --tree DIR   import divans_amd (and tests/irtext.py) from another checkout, e.g. the parent commit's: a tree without the command
               entry point measures the segment call alone"""
import argparse, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("names", nargs="*", default=["alice29-priors", "random_then_unicode"])
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import divans_amd as da, irtext

dev = torch.device("cuda", 0)
n = args.streams


def timed(fn):
    """milliseconds of `reps` calls, each between two synchronisations, after one call that is not counted"""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t = time.perf_counter(); fn(); torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


for name in args.names:
    for mixing in (0, 2):
        ir = da.CommandIR(irtext.load_ir_text(name))
        lit, segs = ir.literal_segments()
        raw = ir.expand()
        cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
        L, R, S = int(lit.size), int(raw.size), int(segs.size)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        codec = da.LiteralCodec(cfg, max(L, 16))
        codec.set_block_types(ir.num_block_types)
        # the coded bytes: one stream through the codec's own encoder, replicated at 16-byte boundaries
        one = codec.alloc_encode_outputs(1, max(L, 16))
        seg1 = t(segs.view(np.uint8))
        codec.encode_segments_batch(t(np.concatenate([lit, np.zeros(64, np.uint8)])), t(np.zeros(1, np.int64)), t(np.array([L], np.int32)), 1, L,
                                    t(np.array([0, S], np.int32)), seg1, one)
        assert codec.status() == 0
        csz = int(one["sizes"][0].item()); coff = int(one["offsets"][0].item())
        slot = (csz + 15) & ~15
        coded1 = torch.zeros(slot, dtype=torch.uint8, device=dev); coded1[:csz] = one["out"][coff:coff + csz]
        d_coded = torch.cat([coded1.repeat(n), torch.zeros(64, dtype=torch.uint8, device=dev)])
        d_coff = torch.arange(n, dtype=torch.int64, device=dev) * slot
        d_csz = torch.full((n,), csz, dtype=torch.int32, device=dev)
        d_lsz = torch.full((n,), L, dtype=torch.int32, device=dev)
        # floor: the segment call (literals out, contexts in)
        d_segs = seg1.repeat(n)
        seg_begin = torch.arange(n + 1, dtype=torch.int32, device=dev) * S
        d_loff = torch.arange(n, dtype=torch.int64, device=dev) * L
        back = torch.zeros(n * L + 64, dtype=torch.uint8, device=dev)
        seg_ms = timed(lambda: codec.decode_segments_batch(d_coded, d_coff, d_csz, n, L, seg_begin, d_segs, back, d_loff, d_lsz))
        assert codec.status() == 0
        d_lit = t(lit)
        assert all(torch.equal(back[k * L:(k + 1) * L], d_lit) for k in (0, n // 2, n - 1))
        rec = {"ir": name, "dynamic_context_mixing": mixing, "streams": n, "literal_bytes_per_stream": L, "raw_bytes_per_stream": R,
               "literal_commands_per_stream": S, "segments_kernel": codec.last_decode_kernel(),
               "segments_ms": round(min(seg_ms), 3), "segments_ms_all": [round(x, 3) for x in seg_ms],
               "segments_ns_per_literal_byte": round(min(seg_ms) * 1e6 / (n * L), 3)}
        del back, d_segs
        if hasattr(codec, "decode_commands_batch"):
            cmds, ins = ir.device_commands()
            C = int(cmds.size)
            d_cmds = t(cmds.view(np.uint8)).repeat(n)
            cmd_begin = torch.arange(n + 1, dtype=torch.int32, device=dev) * C
            d_ins = t(np.concatenate([ins, np.zeros(16, np.uint8)]))
            d_ioff = torch.zeros(n, dtype=torch.int64, device=dev)
            d_isz = torch.full((n,), int(ins.size), dtype=torch.int32, device=dev)
            d_raw = torch.zeros(n * R + 64, dtype=torch.uint8, device=dev)
            d_roff = torch.arange(n, dtype=torch.int64, device=dev) * R
            d_rsz = torch.full((n,), R, dtype=torch.int32, device=dev)
            cmd_ms = timed(lambda: codec.decode_commands_batch(d_coded, d_coff, d_csz, n, cmd_begin, d_cmds, d_lsz, L, d_raw, d_roff, d_rsz, d_ins, d_ioff, d_isz))
            assert codec.status() == 0
            d_ref = t(raw)
            assert all(torch.equal(d_raw[k * R:(k + 1) * R], d_ref) for k in (0, n // 3, n - 1))
            best = min(cmd_ms)
            rec.update({"commands_per_stream": C, "copy_and_insert_commands_per_stream": C - S, "commands_kernel": codec.last_decode_kernel(),
                        "commands_ms": round(best, 3), "commands_ms_all": [round(x, 3) for x in cmd_ms],
                        "ns_per_command": round(best * 1e6 / (n * C), 3), "ns_per_literal_byte": round(best * 1e6 / (n * L), 3),
                        "raw_GBps": round(n * R / best / 1e6, 3), "commands_over_segments": round(best / min(seg_ms), 3),
                        "extra_ns_per_copy_or_insert_command": round((best - min(seg_ms)) * 1e6 / (n * max(C - S, 1)), 3), "raw_output_ok": True})
            del d_raw, d_cmds
        print(json.dumps(rec), flush=True)
        codec.close(); ir.close()
        torch.cuda.empty_cache()
