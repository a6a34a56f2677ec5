#!/usr/bin/env python3
"""Encoder model pass at the strides 2 and 8 under a constant context, one model: streaming kernels (encode path 1, the table-driven
lit_model_encode_kernel<-1, true, false, ., .>) against the bucketed pass keyed by the byte at the stride distance (encode path 2,
launch_bucket_stride_model), same box, alternating on one codec, divans_gpu_info::last_model_ms / last_rans_ms of every call -- the
events bench.py reads.
Workloads: (a) for the masks 5 (distance 2) and 8 (distance 8) `big` and `small` streams of 64 KiB of tests/workload.make_blocks
text, without a list; (b) `copies` copies of the whole literal stream of random_then_unicode.ir (59 KB, 15 000 segments, 4 block
types) with its list, under a constant context and a mask of 5.
One JSON line per workload: the rule for automatic selection of calls without a list is path 2 ahead at BOTH batch sizes of (a) by
more than the spread of path 1's own repeats.
usage: stride_bucketed_rate.py [big] [small] [copies] [rounds]"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, torch
import divans_amd as da, irtext, workload

big = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
small = int(sys.argv[2]) if len(sys.argv) > 2 else 64
copies = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 4
dev = torch.device("cuda", 0)
L = 65536


def coded_equal(a, b):
    if not torch.equal(a["sizes"], b["sizes"]):
        return False
    sz = a["sizes"].to(torch.int64)
    within = torch.arange(int(sz.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(sz, 0) - sz, sz)
    return bool(torch.equal(a["out"][torch.repeat_interleave(a["offsets"], sz) + within], b["out"][torch.repeat_interleave(b["offsets"], sz) + within]))


def measure(what, codec, n, encode):
    outs = {p: codec.alloc_encode_outputs(n) for p in (1, 2)}
    ms = {1: [], 2: []}
    for r in range(rounds + 1):                 # round 0 warms both paths up (allocations, table placement)
        for p in (1, 2):
            codec.set_encode_path(p)
            encode(outs[p])
            torch.cuda.synchronize()
            inf = codec.info()
            assert codec.status() == 0 and codec.last_encode_path() == p
            if r:
                ms[p].append((round(float(inf.last_model_ms), 3), round(float(inf.last_rans_ms), 3)))
    m1 = [m[0] for m in ms[1]]; m2 = [m[0] for m in ms[2]]
    print(json.dumps({"workload": what, "streams": n, "bucket_stride": codec.bucket_stride(), "paths_bit_equal": coded_equal(outs[1], outs[2]),
                      "streaming_model_ms": m1, "bucketed_model_ms": m2,
                      "streaming_rans_ms": [m[1] for m in ms[1]], "bucketed_rans_ms": [m[1] for m in ms[2]],
                      "streaming_spread_ms": round(max(m1) - min(m1), 3), "bucketed_ahead_by_ms": round(min(m1) - max(m2), 3),
                      "speedup_of_medians": round(float(np.median(m1) / np.median(m2)), 2)}), flush=True)


corpus = workload.load_corpus()
for n in (big, small):
    d_in = torch.cat([torch.from_numpy(workload.make_blocks(corpus, k, min(1024, n - k))).to(dev) for k in range(0, n, 1024)])
    for value in (5, 8):
        cfg = da.config_simple()
        ctypes.memset(cfg.mixing_mask, value, 8192)
        codec = da.LiteralCodec(cfg, L)
        measure(f"make_blocks text, mask {value}, no list", codec, n, lambda o: codec.encode_batch(d_in, n, L, o))
        codec.close()
    del d_in
    torch.cuda.empty_cache()

ir = da.CommandIR(irtext.load_ir_text("random_then_unicode"))
lit, segs = ir.literal_segments()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_lit = t(np.concatenate([np.tile(lit, copies), np.zeros(64, np.uint8)]))
d_off = t(np.arange(copies, dtype=np.int64) * lit.size)
d_sz = t(np.full(copies, lit.size, np.int32))
d_sb = t((np.arange(copies + 1, dtype=np.int64) * segs.size).astype(np.int32))
d_segs = t(np.tile(segs, copies).view(np.uint8))
cfg = ir.lit_config(dynamic_context_mixing=0)
ctypes.memset(cfg.literal_context_map, 0, ctypes.sizeof(cfg.literal_context_map))
ctypes.memset(cfg.mixing_mask, 5, 8192)
cfg.context_mixing = 0
codec = da.LiteralCodec(cfg, lit.size)
codec.set_block_types(ir.num_block_types)
measure(f"random_then_unicode.ir whole ({lit.size} bytes, {segs.size} segments each), mask 5, {ir.num_block_types} block types", codec, copies,
        lambda o: codec.encode_segments_batch(d_lit, d_off, d_sz, copies, lit.size, d_sb, d_segs, o))
codec.close()
ir.close()
