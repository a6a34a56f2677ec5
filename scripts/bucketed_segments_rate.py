#!/usr/bin/env python3
"""Encoder model pass of general streams (segment lists): streaming kernels (encode path 1) against the bucketed passes
(encode path 2), same box, alternating, divans_gpu_info::last_model_ms / last_rans_ms of every call.
Batches: (a) `streams` streams cut from alice29-priors' command list as tests/test_gpu_general_streams.py cuts them (a few
hundred bytes to 1.5 KB each, up to 390 segments); (b) the whole literal stream of random_then_unicode (59 KB, 15 000 segments),
`streams` / 4 copies.  Configurations: A (one model, constant context, eight block types) and C (two models, UTF8, one block type;
every segment then names block type 0) of tests/bucketed_segment_cases.py.  One JSON line per (batch, configuration).
usage: bucketed_segments_rate.py [streams] [rounds]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, torch
import divans_amd as da, irtext
import pyoracle as po
import bucketed_segment_cases as bc

n_streams = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)


def cut_streams(name, count):
    ir = da.CommandIR(irtext.load_ir_text(name))
    lit, segs = ir.literal_segments()
    ir.close()
    ends = np.cumsum(segs["len"].astype(np.int64))
    out = []
    for k in range(count):
        a = (k * 149) % (segs.size - 400); b = a + 1 + (k * 37) % 390
        lo = int(ends[a - 1]) if a else 0
        out.append((lit[lo:int(ends[b - 1])].copy(), segs[a:b].copy()))
    return out


def whole_stream(name, count):
    ir = da.CommandIR(irtext.load_ir_text(name))
    lit, segs = ir.literal_segments()
    ir.close()
    return [(lit, segs)] * count


def tensors(streams, one_btype):
    sizes = np.array([s[0].size for s in streams], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes[:-1].astype(np.int64))]).astype(np.int64)
    segs = np.concatenate([s[1] for s in streams])
    if one_btype:
        segs = segs.copy(); segs["btype"] = 0
    seg_begin = np.concatenate([[0], np.cumsum([s[1].size for s in streams])]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lit = np.concatenate([s[0] for s in streams] + [np.zeros(64, np.uint8)])
    return t(lit), t(offs), t(sizes), t(seg_begin), t(segs.view(np.uint8)), int(sizes.max()), int(sizes.sum()), int(segs.size)


for batch_name, streams in (("alice29-priors command ranges", cut_streams("alice29-priors", n_streams)),
                            ("random_then_unicode whole", whole_stream("random_then_unicode", max(1, n_streams // 4)))):
    for key in ("A", "C"):
        fam = bc.CONFIGS[key]
        cfg, ocfg = fam.pair(da, po)
        d_lit, d_off, d_sz, d_sb, d_segs, longest, total, nsegs = tensors(streams, fam.n_btypes == 1)
        n = len(streams)
        codec = da.LiteralCodec(cfg, max(longest, 16))
        codec.set_block_types(fam.n_btypes)
        outs = {p: codec.alloc_encode_outputs(n) for p in (1, 2)}
        ms = {1: [], 2: []}
        for r in range(rounds + 1):                 # round 0 warms both paths up (allocations, table placement)
            for p in (1, 2):
                codec.set_encode_path(p)
                codec.encode_segments_batch(d_lit, d_off, d_sz, n, longest, d_sb, d_segs, outs[p])
                torch.cuda.synchronize()
                inf = codec.info()
                assert codec.status() == 0 and codec.last_encode_path() == (1 if p == 1 else bc.BUCKETED_PATH[key])
                if r:
                    ms[p].append((round(float(inf.last_model_ms), 3), round(float(inf.last_rans_ms), 3)))
        same = bool(torch.equal(outs[1]["sizes"], outs[2]["sizes"]))
        if same:
            sz = outs[1]["sizes"].to(torch.int64)
            idx = torch.repeat_interleave(outs[1]["offsets"], sz) + (torch.arange(int(sz.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(sz, 0) - sz, sz))
            same = bool(torch.equal(outs[1]["out"][idx], outs[2]["out"][idx]))
        print(json.dumps({"batch": batch_name, "configuration": key + " (" + fam.name + ")", "streams": n, "literal_bytes": total, "longest_stream": longest,
                          "segments": nsegs, "paths_bit_equal": same,
                          "streaming_model_ms": [m[0] for m in ms[1]], "bucketed_model_ms": [m[0] for m in ms[2]],
                          "streaming_rans_ms": [m[1] for m in ms[1]], "bucketed_rans_ms": [m[1] for m in ms[2]]}), flush=True)
        codec.close()
