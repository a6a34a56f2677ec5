"""One list-free batch per configuration family for the calls WITHOUT a segment list (divans_gpu_lit_decode_batch / _encode_batch, the
product's default), shared by the CPU tier (tests/test_plain_decoder_cases_cpu.py: the C oracle on exactly these streams) and the GPU
tier (tests/test_gpu_plain_decoders.py: every SEG = false instance of lit_decode2_kernel under every cache set).  numpy + ctypes only.

The families are those of tests/segment_cases.py.  The oracle codes a family's streams under oracle_config(): a codec that was given
eight context tables (divans_gpu_codec_set_block_types) codes a call without a list under table 0, whatever divans_lit_config::btype
says; a codec with one table under the configuration's own block type.

shapes() returns N_STREAMS streams in the order ORDER.  One workgroup holds 16 resident groups and group s mod 16 decodes stream s:
the order makes one group decode a stream that crosses the 32 768-byte chunk seam and then a one-byte stream, one the empty stream
between two others, one a stream of exactly 15 coded words after the 40 000-byte one (order_properties)."""
import numpy as np

import pyoracle as po
import segment_cases as sc
from speed_slot_cases import block_type_0

# the decoders' 16-byte output group: cnt < 16 on the last group, one group exactly, one byte more
OUTPUT_GROUP = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)
# coded sizes in 32-bit words around the refill points of the decoders' 32-word ring (16 words per refill, 32 preloaded, 16 held)
RING_WORDS = (15, 16, 17, 31, 32, 33, 47, 48, 49)
RING_SEARCH = 399                    # prefixes of 1 .. RING_SEARCH bytes of each source are tried
CHUNK_SEAM = (32767, 32768, 32769, 40000)        # 32 768 bytes = one chunk of 65 536 symbols
NARROW = 6000
N_FILL = 7
ORDER = (["R0", "C32769", "C40000", "C32767", "C32768", "K_zero", "K_period12"] + [f"O{n}" for n in OUTPUT_GROUP[1:10]]
         + ["EMPTY", "O1"] + [f"W{w}" for w in RING_WORDS] + ["O49"] + [f"R{k}" for k in range(1, N_FILL)])
N_STREAMS = len(ORDER)
GROUPS = 16                          # resident groups of one workgroup
SENTINEL = 0xa5
TAIL = 64                            # sentinel bytes behind both buffers
_RING_SOURCES = ("text", "random_then_unicode", "shuffle384", "uniform random")


def oracle_config(fam, cfg):
    """the oracle configuration a call without a list answers to (module docstring)"""
    return block_type_0(po, cfg) if fam.n_btypes > 1 else cfg


def ring_streams(fam, ocfg, sources, rng):
    """{words: (source name, literal bytes)}: for every target of RING_WORDS the shortest prefix of a source whose coded size under
    `ocfg` is exactly that many words.  Target k asks source k mod 4 first, then the others in turn."""
    corpus, rtu, shuffle384 = sources
    windows = []
    for name, src in zip(_RING_SOURCES[:3], (corpus, rtu, shuffle384)):
        if src.size > RING_SEARCH:
            o = int(rng.integers(0, src.size - RING_SEARCH))
            windows.append((name, src[o:o + RING_SEARCH].copy()))
        else:
            windows.append((name, np.resize(src, RING_SEARCH).copy()))
    windows.append((_RING_SOURCES[3], rng.integers(0, 256, size=RING_SEARCH, dtype=np.uint8)))
    found = []
    for name, w in windows:
        by_words = {}
        for n in range(1, RING_SEARCH + 1):
            size = po.lit_encode(ocfg, w[:n]).size
            assert size % 4 == 0
            by_words.setdefault(size // 4, n)
        found.append(by_words)
    out = {}
    for k, words in enumerate(RING_WORDS):
        for j in range(4):
            name, w = windows[(k + j) % 4]
            n = found[(k + j) % 4].get(words)
            if n is not None:
                out[words] = (name, w[:n].copy())
                break
    missing = [w for w in RING_WORDS if w not in out]
    assert not missing, f"{fam.name}: no prefix of 1..{RING_SEARCH} bytes codes to {missing} words; found " \
                        f"{ {w: (out[w][0], out[w][1].size) for w in out} }"
    return out


def shapes(fam, sources):
    """[(name, literal bytes)] of a family in the order ORDER; sources = (corpus, random_then_unicode, shuffle384)"""
    rng = np.random.default_rng(97000 + fam.seed)
    data = sc._Data(sources, rng)
    ocfg = oracle_config(fam, fam.configure(getattr(po, "config_" + fam.base)()))
    by = {}
    for n in OUTPUT_GROUP:
        by[f"O{n}"] = data.take(n)
    for words, (_, lit) in ring_streams(fam, ocfg, sources, rng).items():
        by[f"W{words}"] = lit
    for n in CHUNK_SEAM:
        by[f"C{n}"] = data.take(n)
    by["EMPTY"] = np.zeros(0, np.uint8)
    # a handful of rows take every update: the caches always hit, and a row renormalises under the families' slow speeds
    by["K_zero"] = np.zeros(NARROW, np.uint8)
    by["K_period12"] = np.resize(np.frombuffer(b"abracadabra ", dtype=np.uint8), NARROW).copy()
    for k in range(N_FILL):
        by[f"R{k}"] = data.take(int(rng.integers(1, 4001)))
    assert sorted(by) == sorted(ORDER)
    out = [(name, by[name]) for name in ORDER]
    order_properties(out)
    return out


def order_properties(streams):
    """what the order promises about the streams one resident group of a one-workgroup grid decodes one after the other"""
    assert len(streams) == N_STREAMS > 2 * GROUPS
    name = [s[0] for s in streams]
    size = [s[1].size for s in streams]
    chains = [list(range(g, N_STREAMS, GROUPS)) for g in range(GROUPS)]
    pairs = [(a, b) for c in chains for a, b in zip(c[:-1], c[1:])]
    assert any(size[a] > 32768 and size[b] == 1 for a, b in pairs), "no group decodes a one-byte stream after a chunk seam"
    assert any(size[a] == 40000 and name[b] == f"W{RING_WORDS[0]}" for a, b in pairs), "no group decodes a ring-edge stream after the longest one"
    assert any(len(c) == 3 and size[c[0]] > 0 and size[c[1]] == 0 and size[c[2]] > 0 for c in chains), "no group decodes the empty stream between two others"
    assert all(len(c) >= 2 for c in chains)              # every group decodes a second stream: its caches and its ring start again
    assert sorted(size)[:2] == [0, 1] and max(size) == 40000


def literal_layout(streams):
    """the streams' bytes back to back with gaps of 1, 2, 3, 1, ... sentinel bytes and TAIL behind: every alignment mod 4 occurs.
    -> (buffer with the literals in place, the same buffer with sentinels only, offsets int64, sizes int32)"""
    offs, cur = [], 0
    for i, (_, lit) in enumerate(streams):
        cur += 1 + i % 3
        offs.append(cur); cur += lit.size
    blank = np.full(cur + TAIL, SENTINEL, np.uint8)
    buf = blank.copy()
    for o, (_, lit) in zip(offs, streams):
        buf[o:o + lit.size] = lit
    offs = np.array(offs, np.int64)
    assert set((offs % 4).tolist()) == {0, 1, 2, 3}
    return buf, blank, offs, np.array([s[1].size for s in streams], np.int32)


def coded_layout(coded):
    """the coded streams back to back at 4-byte granularity, as divans_gpu_pack_streams leaves them, TAIL sentinel bytes behind
    -> (buffer, offsets int64, sizes int32)"""
    sizes = np.array([c.size for c in coded], np.int32)
    assert (sizes % 4 == 0).all()
    offs = np.concatenate([[0], np.cumsum(sizes[:-1].astype(np.int64))]).astype(np.int64)
    assert {4, 8, 12} <= set((offs % 16).tolist()), "the coded streams do not start at every 4-byte offset of a 16-byte line"
    buf = np.full(int(sizes.astype(np.int64).sum()) + TAIL, SENTINEL, np.uint8)
    for o, c in zip(offs, coded):
        buf[int(o):int(o) + c.size] = c
    return buf, offs, sizes


def oracle_bytes(ocfg, streams):
    """the oracle's coded bytes of every stream; the empty stream codes to 0 bytes"""
    return [po.lit_encode(ocfg, lit) if lit.size else np.zeros(0, np.uint8) for _, lit in streams]


def resumed_stream(sources):
    """the 70 000 bytes tests hand over piece by piece (text followed by random_then_unicode) and where they are cut: the first eight
    bytes arrive in pieces shorter than the longest stride, so last_8_literals is assembled over several calls"""
    corpus, rtu, _ = sources
    data = np.concatenate([corpus[1000:36000], rtu[200000:235000]])
    cuts = [0, 1, 2, 3, 7, 8, 9, 10, 17, 4096, 32767, 32768, 32769, 65536, 65537, data.size]
    assert data.size == 70000 and cuts == sorted(set(cuts))
    return data, cuts
