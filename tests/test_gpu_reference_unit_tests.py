"""the reference's own unit tests, run against the GPU device primitives (not only the oracle).

* probability/common_tests.rs:152-185 `operation_test_helper` -- two CDF implementations must agree exactly after every blend
  and at the mixing rates 0, 1/4, 1/2, 3/4, 1: implementation A = the device functions the kernels are made of (blend_row,
  blend_row_known_max, average_rows, scaled_div start/freq, the ballot search) through divans_gpu_selftest_cdf_ops,
  implementation B = the CPU restatements (C oracle and the independent Python one).
* common_tests.rs:3-126 `declare_common_tests!` -- start/freq chain identity, every 15-bit offset decodes to a monotone symbol
  inside its range, the LCG sample run (seed 1, common_tests.rs:44-48), repeated symbol 15 keeps all pdf > 0.
* codec/weights.rs through Weights::update sequences (row a19 had no isolated GPU test).
* Since the device holds several restatements of that arithmetic, every script runs on each of them (`impl`: the generation-1
  streaming kernels, lit_decode2.hip, the bucketed encoder passes, in experiment builds lit_decode_t.hip) through divans_gpu_selftest_cdf_ops_on, against ONE table of
  expected values: the oracle's C script interpreter (oracle/cdf_ops.c), which the Python restatement must match in full.
  tests/test_gpu_cdf_ops_sweeps.py adds the edge-directed sweeps.
* test_ans.rs:177-260 `encode_test_nibble_helper` for its five TestSelection variants: the model runs on the host (independent
  restatement), its (start, freq) pairs go through the GPU rANS pass alone, bytes compared with ANSEncoder's.
"""
import ctypes
import os

import numpy as np
import pytest

import cdf_ops_sweeps as sw
import gpu_harness as gh
import pyoracle as po
import ref_restatement as rr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MED, SLOW = sw.MED, sw.SLOW


@pytest.fixture(scope="module")
def codec():
    import divans_amd as da
    c = da.LiteralCodec(da.config_simple(), 4096)
    yield c
    c.close()


IMPLS = gh.implementations()


def run_both(codec, impl, ops):
    """the script on the device implementation `impl`; expected records from the C interpreter, which the Python restatement
    (Mirror, itself checked call by call against the oracle's functions) must match in full"""
    exp = sw.second_opinion(ops)
    got = codec.selftest_cdf_ops(np.array(ops, dtype=np.uint32), impl).astype(np.int64)
    sw.compare(impl, ops, got, exp, "reference unit test")
    if impl == 0:       # divans_gpu_selftest_cdf_ops is implementation 0
        assert (codec.selftest_cdf_ops(np.array(ops, dtype=np.uint32)).astype(np.int64) == got).all()
    return got


@pytest.mark.parametrize("impl", IMPLS)
def test_operation_test_helper_on_the_device_primitives(codec, impl):
    ops = sw.script_operation_test_helper()
    got = run_both(codec, impl, ops)
    # assert_cdf_similar(average(.., all), cdf0) / (average(.., 0), cdf1): within max0*max1/160 after cross-scaling (common_tests.rs:128-150)
    r0, r1 = got[len(ops) - 6], got[29]
    for rec, ref in ((got[-1], r0), (got[-2], r1)):
        m0, m1 = int(rec[15]), int(ref[15])
        assert all(abs(int(rec[i]) * m1 - int(ref[i]) * m0) < m0 * m1 // 160 for i in range(16))


@pytest.mark.parametrize("impl", IMPLS)
def test_declare_common_tests_invariants(codec, impl):
    ops = sw.script_declare_common_tests()
    got = run_both(codec, impl, ops)
    sf = got[100:116]
    for s in range(1, 16):                                 # common_tests.rs:14-17
        assert sf[s, 0] == 1 + sf[s - 1, 0] + sf[s - 1, 1]
    dec = got[116:]
    assert (np.diff(dec[:, 2]) >= 0).all() and dec[0, 2] == 0 and dec[-1, 2] == 15     # monotone symbols, :29-39
    offs = np.arange(1 << 15)
    assert ((offs >= dec[:, 0] - 1) & (offs <= dec[:, 0] + dec[:, 1])).all()


@pytest.mark.parametrize("impl", IMPLS)
def test_lcg_sample_run_and_symbol_15_stress(codec, impl):
    got = run_both(codec, impl, sw.script_lcg_sample_run())
    final = got[-1]
    assert (np.diff(np.concatenate([[0], final])) > 0).all()      # every pdf entry still positive


@pytest.mark.parametrize("impl", IMPLS)
def test_weights_update_sequences(codec, impl):
    run_both(codec, impl, sw.script_weights_update_sequences())


def test_what_an_implementation_lacks_is_refused(codec):
    import divans_amd as da
    if not da.experimental_decoders():
        with pytest.raises(da.DivansGpuError, match="experiment builds"):
            codec.selftest_cdf_ops(np.array([(6, 0, 0, 0)], dtype=np.uint32), 3)
    else:
        assert 3 in IMPLS
    with pytest.raises(da.DivansGpuError, match="no decoder"):
        codec.selftest_cdf_ops(np.array([(9, 1 << 31, 0, 0)], dtype=np.uint32), 2)
    with pytest.raises(da.DivansGpuError, match="unknown implementation"):
        codec.selftest_cdf_ops(np.array([(6, 0, 0, 0)], dtype=np.uint32), 4)


# ---------------------------------------------------------------- test_ans.rs nibble helpers
def init_src(n):
    seed = np.fromfile(os.path.join(GOLDEN, "init_src_seed.bin"), dtype=np.uint8)
    return np.resize(seed, n)


VARIANTS = {  # adapt_probability, adaptive_context_mixing, independent_hilo, two_models   (test_ans.rs:86-176)
    "TestContextMixing": (True, True, False, True),
    "TestContextMixingPureAverage": (True, False, False, True),
    "TestAdapt": (True, False, False, False),
    "TestNoAdapt": (False, False, False, False),
    "TestSimple": (False, False, True, False),
}


def nibble_helper_pairs(src, adapt, acm, indep, two):
    """encode_test_nibble_helper, test_ans.rs:177-260, on the independent restatement; returns the (start, freq) pairs and ANSEncoder's bytes"""
    enc = rr.AnsEncoder()
    pairs = []
    weights = [rr.Weights(), rr.Weights()]
    cdf_high = rr.Cdf(); cdf_low = [rr.Cdf() for _ in range(16)]
    cdf_low_adv = [rr.Cdf() for _ in range(16)]; cdf_high_adv = [rr.Cdf() for _ in range(16)]
    last = 0
    Q2 = 1 << 13
    def put(sym, cdf):
        s, f = cdf.sym_to_start_and_freq(sym)
        pairs.append((s & 0xFFFF) | ((f & 0xFFFF) << 16)); enc.put_start_freq(s, f)
        return f
    for v in src:
        v = int(v)
        b0 = weights[0].norm_weight_as_u16_as_i32() if acm else Q2
        b1 = weights[1].norm_weight_as_u16_as_i32() if acm else Q2
        hi = v >> 4
        fr = put(hi, cdf_high.average(cdf_high_adv[last], b0) if two else cdf_high_adv[last])
        if acm:
            weights[0].update([cdf_high.sym_to_start_and_freq(hi)[1], cdf_high_adv[last].sym_to_start_and_freq(hi)[1]], fr)
        if adapt:
            if two:
                cdf_high.blend(hi, SLOW)
            cdf_high_adv[last].blend(hi, MED)
        cdfl = cdf_low[0 if indep else hi]
        lo = v & 0xF
        fr = put(lo, cdfl.average(cdf_low_adv[last], b1) if two else cdf_low_adv[last])
        if acm:
            weights[1].update([cdfl.sym_to_start_and_freq(lo)[1], cdf_low_adv[last].sym_to_start_and_freq(lo)[1]], fr)
        if adapt:
            if two:
                cdfl.blend(lo, SLOW)
            cdf_low_adv[last].blend(lo, SLOW)
        last = v & 0xF
    enc.flush_chunk()
    return np.array(pairs, dtype=np.uint32), bytes(enc.out)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("source", ["init_src", "shuffle384"])
def test_ans_nibble_helper_streams_through_the_gpu_rans_pass(codec, variant, source, shuffle384):
    n = 4097 if source == "init_src" else 40000           # entropy16_* sizes are 16 / 4092 / 4097; 40 000 bytes crosses the 65 536-symbol chunk
    src = init_src(n) if source == "init_src" else np.resize(shuffle384, n)
    pairs, ref = nibble_helper_pairs(src, *VARIANTS[variant])
    got = codec.selftest_rans_pairs(pairs)
    assert got.tobytes() == ref
    # and the decoder side of the restatement reads those bytes back with the mirrored model (decode_test_nibble_helper, :262-368)
    dec = rr.AnsDecoder(ref)
    adapt, acm, indep, two = VARIANTS[variant]
    if not two and not acm:
        cdf_low_adv = [rr.Cdf() for _ in range(16)]; cdf_high_adv = [rr.Cdf() for _ in range(16)]
        last = 0
        for v in src[:2000]:
            hi, _, _ = dec.get_nibble(cdf_high_adv[last])
            if adapt:
                cdf_high_adv[last].blend(hi, MED)
            lo, _, _ = dec.get_nibble(cdf_low_adv[last])
            if adapt:
                cdf_low_adv[last].blend(lo, SLOW)
            assert ((hi << 4) | lo) == int(v)
            last = lo
