#!/usr/bin/env python3
"""What the wide context-table layout costs (divans_gpu_codec_set_block_types above eight types: two dependent LDS reads per byte for
the context where the fused tables need one).  One batch of segment lists -- the literals of alice29-priors.ir, whose lists name
block types 0..7, replicated N times -- is encoded and decoded under three codecs that produce the SAME bytes:

    fused    set_block_types(8)                 the fused tables, the kernels of eight types
    wide9    set_block_types(9), the same lists the wide layout (type 8 is never named)
    wide256  set_block_types(256), block type t of a list replaced by t + 8 k, k cycling through 0..31 from segment to segment; the
             context map's rows 8..255 repeat rows 0..7, so the contexts -- and the coded bytes -- stay what they are

The three run in turn inside every repetition, so that each is measured against the fused call of the same run; per direction the
best time, every repetition and the fused call's own spread are printed.  Both mixing settings, and two configurations:

    ir       the IR's own configuration: more than 32 766 rows per stream, so the instances WITHOUT row caches run
    cached   the same literals and lists under config_context_mixing's kind of configuration (mixing value 4, UTF8, 64 contexts, a
             bijection of them per block type): 20 480 rows and more, the instances WITH the high-row caches, all three codecs in the
             2-way organisation (the only one the wide instances have)
usage: wide_block_types_rate.py [copies] [repetitions]"""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import divans_amd as da, irtext

copies = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda", 0)
for source, mixing in ((s, m) for s in ("ir", "cached") for m in (0, 2)):
    ir = da.CommandIR(irtext.load_ir_text("alice29-priors"))
    lit, segs = ir.literal_segments()
    assert ir.num_block_types <= 8 and int(segs["btype"].max()) < 8
    if source == "ir":
        cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
        cmap = np.frombuffer(bytes(cfg.literal_context_map), np.uint8).reshape(256, 64).copy()
    else:
        cfg = da.config_context_mixing()
        cfg.context_mixing = mixing
        cmap = np.zeros((256, 64), np.uint8)
        cmap[:8] = (np.arange(64)[None, :] * (2 * np.arange(8)[:, None] + 1)) % 64
    cmap[8:] = np.tile(cmap[:8], (31, 1))
    ctypes.memmove(cfg.literal_context_map, cmap.ctypes.data, cmap.size)
    spread = segs.copy()
    spread["btype"] = segs["btype"] + 8 * (np.arange(segs.size) % 32)
    n, L = copies, int(lit.size)
    d_all = torch.cat([torch.from_numpy(lit).to(dev).repeat(n), torch.zeros(64, dtype=torch.uint8, device=dev)])
    d_off = torch.arange(n, dtype=torch.int64, device=dev) * L
    d_sz = torch.full((n,), L, dtype=torch.int32, device=dev)
    seg_begin = torch.arange(n + 1, dtype=torch.int32, device=dev) * int(segs.size)
    lists = {k: torch.from_numpy(np.ascontiguousarray(np.tile(v, n)).view(np.uint8)).to(dev) for k, v in (("low", segs), ("spread", spread))}
    runs = []
    for name, types, which in (("fused", 8, "low"), ("wide9", 9, "low"), ("wide256", 256, "spread")):
        codec = da.LiteralCodec(cfg, max(L, 16))
        codec.set_block_types(types)
        if source == "cached":
            codec.set_decoder(3)
        codec.search_tables(1)      # no table-placement search: a wide codec takes no part in it, and the fused one is measured on like terms
        runs.append(dict(name=name, types=types, codec=codec, segs=lists[which], outs=codec.alloc_encode_outputs(n, max(L, 16)), enc=[], dec=[]))
    back = torch.zeros_like(d_all)
    for rep in range(reps + 1):        # (the first repetition allocates tables and work arrays: not recorded)
        for r in runs:
            c = r["codec"]
            torch.cuda.synchronize(); t = time.perf_counter()
            c.encode_segments_batch(d_all, d_off, d_sz, n, L, seg_begin, r["segs"], r["outs"])
            torch.cuda.synchronize(); e = time.perf_counter() - t
            back.zero_()
            torch.cuda.synchronize(); t = time.perf_counter()
            c.decode_segments_batch(r["outs"]["out"], r["outs"]["offsets"], r["outs"]["sizes"], n, L, seg_begin, r["segs"], back, d_off, d_sz)
            torch.cuda.synchronize(); d = time.perf_counter() - t
            assert c.status() == 0 and torch.equal(back[:n * L], d_all[:n * L]), r["name"]
            r["kernel"] = c.last_decode_kernel()
            if rep:
                r["enc"].append(e * 1e3); r["dec"].append(d * 1e3)
    sizes = [r["outs"]["sizes"].cpu().numpy() for r in runs]
    offs = [r["outs"]["offsets"].cpu().numpy() for r in runs]
    first = [r["outs"]["out"][int(o[0]):int(o[0]) + int(s[0])].cpu().numpy() for r, o, s in zip(runs, offs, sizes)]
    assert all((s == sizes[0]).all() for s in sizes) and all((f == first[0]).all() for f in first), "the three codecs wrote different bytes"
    base = runs[0]
    for r in runs:
        print(json.dumps({"configuration": source, "rows_per_stream": int(r["codec"].info().rows_per_stream), "dynamic_context_mixing": mixing, "codec": r["name"], "block_types": r["types"], "streams": n, "literal_bytes_per_stream": L,
                          "segments_per_stream": int(segs.size), "decode_kernel": r["kernel"],
                          "encode_ms_best": round(min(r["enc"]), 2), "encode_ms": [round(x, 2) for x in r["enc"]],
                          "decode_ms_best": round(min(r["dec"]), 2), "decode_ms": [round(x, 2) for x in r["dec"]],
                          "encode_vs_fused": round(min(r["enc"]) / min(base["enc"]), 4), "decode_vs_fused": round(min(r["dec"]) / min(base["dec"]), 4),
                          "fused_encode_spread": round(max(base["enc"]) / min(base["enc"]), 4), "fused_decode_spread": round(max(base["dec"]) / min(base["dec"]), 4)}), flush=True)
        r["codec"].close()
    ir.close()
