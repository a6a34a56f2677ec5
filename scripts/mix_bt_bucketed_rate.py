#!/usr/bin/env python3
"""Encoder model pass under uniform mixing value 4 with dynamic mixing and SEVERAL literal block types: streaming kernels (encode
path 1, lit_model_encode_kernel<4, false, true, ., .>) against the bucketed two-model pass with the block type in the stride model's
high-row slot (encode path 2, launch_bucket_mix_bt_model), same box, alternating on one codec, divans_gpu_info::last_model_ms /
last_rans_ms of every call -- the events bench.py reads.
Workloads: (a) the clustered eight-block-type map of tests/mix_bt_bucketed_cases.py (family c8) on `big` and on `small` streams of
64 KiB of tests/workload.make_blocks text, without a list, on a codec that keeps all eight tables; (b) `copies` copies of the whole
literal stream of random_then_unicode.ir (59 KB, 15 000 segments, 4 block types) under the IR's own context map with the mask forced
to mixing value 4, with its list.
One JSON line per workload: the rule for automatic selection of calls without a list is path 2 ahead at BOTH batch sizes of (a) by
more than the spread of path 1's own repeats.
usage: mix_bt_bucketed_rate.py [big] [small] [copies] [rounds]"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, torch
import divans_amd as da, irtext, workload
import mix_bt_bucketed_cases as mc

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
            assert codec.status() == 0 and codec.last_encode_path() == (1 if p == 1 else 3)
            if r:
                ms[p].append((round(float(inf.last_model_ms), 3), round(float(inf.last_rans_ms), 3)))
    m1 = [m[0] for m in ms[1]]; m2 = [m[0] for m in ms[2]]
    print(json.dumps({"workload": what, "streams": n, "high_row_slots": codec.high_row_slots(), "paths_bit_equal": coded_equal(outs[1], outs[2]),
                      "streaming_model_ms": m1, "bucketed_model_ms": m2,
                      "streaming_rans_ms": [m[1] for m in ms[1]], "bucketed_rans_ms": [m[1] for m in ms[2]],
                      "streaming_spread_ms": round(max(m1) - min(m1), 3), "bucketed_ahead_by_ms": round(min(m1) - max(m2), 3),
                      "speedup_of_medians": round(float(np.median(m1) / np.median(m2)), 2)}), flush=True)


corpus = workload.load_corpus()
for n in (big, small):
    d_in = torch.cat([torch.from_numpy(workload.make_blocks(corpus, k, min(1024, n - k))).to(dev) for k in range(0, n, 1024)])
    cfg = mc.FAMILIES["c8"].configure(da.config_context_mixing())
    assert set(bytes(cfg.mixing_mask)) == {4} and cfg.context_mixing == 2
    codec = da.LiteralCodec(cfg, L)
    codec.set_block_types(8)
    measure("make_blocks text, clustered map c8, no list, 8 block types kept", codec, n, lambda o: codec.encode_batch(d_in, n, L, o))
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
cfg = ir.lit_config(dynamic_context_mixing=2, use_context_map=1)
ctypes.memset(cfg.mixing_mask, 4, 8192)
codec = da.LiteralCodec(cfg, lit.size)
codec.set_block_types(ir.num_block_types)
measure(f"random_then_unicode.ir whole ({lit.size} bytes, {segs.size} segments each), {ir.num_block_types} block types", codec, copies,
        lambda o: codec.encode_segments_batch(d_lit, d_off, d_sz, copies, lit.size, d_sb, d_segs, o))
codec.close()
ir.close()
