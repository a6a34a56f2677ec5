"""The task feed of the bucketed encoder's chain kernels (bucket_chain_kernel; bk_chain_loop, lit_bucket_dev.h) at its edges: windows of 64 long tasks, the
switch to 256-task windows, a window that holds both kinds, one task on a whole grid and no task at all.  Every batch runs in the
"simple" and the "mixing" configuration; every stream's coded bytes under set_encode_path(2) are compared with the streaming
encoder's and with the oracle's."""
import numpy as np
import pytest

import pyoracle as po

pytestmark = pytest.mark.gpu

LONG = np.full(2049, 0x61, np.uint8)          # one bucket of 2048 positions (the first "long" class) and one of one position
SHORT = np.frombuffer(b"ab", np.uint8)        # two buckets of one position
CASES = {
    "long63": [LONG] * 63, "long64": [LONG] * 64, "long65": [LONG] * 65,                 # a window of 64 long tasks, then the 256-task windows
    "short127": [SHORT] * 127, "short128": [SHORT] * 128, "short129": [SHORT] * 129,     # 254, 256 and 258 tasks around one window
    "long65_short128": [LONG] * 65 + [SHORT] * 128,                                      # the window across the end of the long tasks holds both kinds
    "one_byte": [np.frombuffer(b"a", np.uint8)],                                         # a single task
    "all_empty": [np.zeros(0, np.uint8)] * 64,                                           # no task: every lane leaves on the first claim
}
MAX_LEN = 2049


@pytest.fixture(scope="module")
def codecs():
    import divans_amd as da
    made = {"simple": da.LiteralCodec(da.config_simple(), MAX_LEN), "mixing": da.LiteralCodec(da.config_context_mixing(), MAX_LEN)}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def oracle_bytes():
    """coded bytes of the few distinct streams, once per configuration"""
    cfgs = {"simple": po.config_simple(), "mixing": po.config_context_mixing()}
    memo = {}

    def ref(cfg_name, data):
        key = (cfg_name, data.tobytes())
        if key not in memo:
            memo[key] = po.lit_encode(cfgs[cfg_name], data)
        return memo[key]
    return ref


@pytest.mark.parametrize("cfg_name", ["simple", "mixing"])
@pytest.mark.parametrize("case", list(CASES))
def test_task_feed_edges(case, cfg_name, codecs, oracle_bytes):
    import torch
    dev = torch.device("cuda", 0)
    streams = CASES[case]
    n = len(streams)
    lens = np.array([len(s) for s in streams], np.int32)
    L = max(int(lens.max()), 1)
    starts = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    d_in = torch.from_numpy(np.concatenate(list(streams) + [np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.from_numpy(starts).to(dev); d_sz = torch.from_numpy(lens).to(dev)
    codec = codecs[cfg_name]
    got = []
    for path in (2, 1):
        codec.set_encode_path(path)
        outs = codec.alloc_encode_outputs(n)
        codec.encode_batch(d_in, n, L, outs, in_offsets=d_off, in_sizes=d_sz)
        torch.cuda.synchronize()
        assert codec.status() == 0
        assert codec.last_encode_path() == (1 if path == 1 else 2 if cfg_name == "simple" else 3)
        got.append((outs["offsets"].cpu().numpy(), outs["sizes"].cpu().numpy(), outs["out"].cpu().numpy()))
    (o2, s2, b2), (o1, s1, b1) = got
    for i, data in enumerate(streams):
        ref = oracle_bytes(cfg_name, data)
        coded2 = b2[o2[i]:o2[i] + s2[i]]
        assert s2[i] == ref.size and (coded2 == ref).all(), ("oracle", i)
        assert s1[i] == s2[i] and (b1[o1[i]:o1[i] + s1[i]] == coded2).all(), ("streaming", i)
