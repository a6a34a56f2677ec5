#!/usr/bin/env python3
"""Cost of encoding general streams from their command lists (divans_gpu_lit_encode_commands_batch): the counterpart of
scripts/command_decode_rate.py, on the same streams and batches.  An IR's stream replicated N times in HBM -- raw bytes and command
list of its own per stream, the insert bytes shared -- coded through encode_commands_batch; the prepare kernel's own time inside that
call (lit_commands.hip: literals and segments derived and the Copy / Insert commands verified on the device); the same streams through
encode_segments_batch on lists the host prepared, which is what a caller had to do before and the yardstick; and the host's time for
preparing one stream's lists (divans_ir_literal_segments).  One JSON line per (IR, mixing).

usage: command_encode_rate.py [--streams N] [--reps K] [ir name ...]"""
import argparse, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("names", nargs="*", default=["alice29-priors", "random_then_unicode"])
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import divans_amd as da, irtext

dev = torch.device("cuda", 0)
n = args.streams


def timed(fn, after=lambda: None):
    """milliseconds of `reps` calls, each between two synchronisations, after one call that is not counted; `after` runs behind each"""
    fn(); torch.cuda.synchronize()
    ms, extra = [], []
    for _ in range(args.reps):
        t = time.perf_counter(); fn(); torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
        extra.append(after())
    return ms, extra


for name in args.names:
    for mixing in (0, 2):
        ir = da.CommandIR(irtext.load_ir_text(name))
        t0 = time.perf_counter()
        for _ in range(5):
            lit, segs = ir.literal_segments()
        host_ms = (time.perf_counter() - t0) * 1e3 / 5
        raw = ir.expand()
        cmds, ins = ir.device_commands()
        cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
        L, R, S, C = int(lit.size), int(raw.size), int(segs.size), int(cmds.size)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        codec = da.LiteralCodec(cfg, max(L, 16))
        codec.set_block_types(ir.num_block_types)
        outs = codec.alloc_encode_outputs(n)
        # the yardstick: the segment call on host-prepared lists
        d_lit = t(lit).repeat(n)
        d_lit = torch.cat([d_lit, torch.zeros(64, dtype=torch.uint8, device=dev)])
        d_loff = torch.arange(n, dtype=torch.int64, device=dev) * L
        d_lsz = torch.full((n,), L, dtype=torch.int32, device=dev)
        d_segs = t(segs.view(np.uint8)).repeat(n)
        seg_begin = torch.arange(n + 1, dtype=torch.int32, device=dev) * S
        seg_ms, _ = timed(lambda: codec.encode_segments_batch(d_lit, d_loff, d_lsz, n, L, seg_begin, d_segs, outs))
        assert codec.status() == 0
        o0, z0 = int(outs["offsets"][0].item()), int(outs["sizes"][0].item())
        ref = outs["out"][o0:o0 + z0].clone()
        del d_lit, d_segs
        # the new call: raw bytes and command lists
        d_raw = torch.cat([t(raw).repeat(n), torch.zeros(64, dtype=torch.uint8, device=dev)])
        d_roff = torch.arange(n, dtype=torch.int64, device=dev) * R
        d_rsz = torch.full((n,), R, dtype=torch.int32, device=dev)
        d_cmds = t(cmds.view(np.uint8)).repeat(n)
        cmd_begin = torch.arange(n + 1, dtype=torch.int32, device=dev) * C
        d_ins = t(np.concatenate([ins, np.zeros(16, np.uint8)]))
        d_ioff = torch.zeros(n, dtype=torch.int64, device=dev)
        d_isz = torch.full((n,), int(ins.size), dtype=torch.int32, device=dev)
        got_lsz = torch.zeros(n, dtype=torch.int32, device=dev)
        cmd_ms, prep_ms = timed(lambda: codec.encode_commands_batch(d_raw, d_roff, d_rsz, n, cmd_begin, d_cmds, L, outs, got_lsz, d_ins, d_ioff, d_isz),
                                codec.last_prepare_ms)
        assert codec.status() == 0 and bool((got_lsz == L).all())
        slot = outs["slot"]
        for k in (0, n // 3, n - 1):
            o, z = int(outs["offsets"][k].item()), int(outs["sizes"][k].item())
            assert z == z0 and o - k * slot == o0 and torch.equal(outs["out"][o:o + z], ref)
        best, prep, seg = min(cmd_ms), min(prep_ms), min(seg_ms)
        print(json.dumps({
            "ir": name, "dynamic_context_mixing": mixing, "streams": n, "literal_bytes_per_stream": L, "raw_bytes_per_stream": R,
            "commands_per_stream": C, "literal_commands_per_stream": S, "encode_path": codec.last_encode_path(),
            "commands_ms": round(best, 3), "commands_ms_all": [round(x, 3) for x in cmd_ms],
            "prepare_kernel_ms": round(prep, 3), "prepare_kernel_ms_all": [round(x, 3) for x in prep_ms],
            "segments_ms": round(seg, 3), "segments_ms_all": [round(x, 3) for x in seg_ms],
            "host_prepare_ms_per_stream": round(host_ms, 3), "host_prepare_ms_for_the_batch_on_one_core": round(host_ms * n, 1),
            "commands_over_segments": round(best / seg, 3), "prepare_share_of_the_call": round(prep / best, 3),
            "prepare_raw_GBps": round(n * R / prep / 1e6, 1), "prepare_ns_per_command": round(prep * 1e6 / (n * C), 3),
            "coded_bytes_equal_the_segment_call": True}), flush=True)
        codec.close(); ir.close()
        del d_raw, d_cmds
        torch.cuda.empty_cache()
