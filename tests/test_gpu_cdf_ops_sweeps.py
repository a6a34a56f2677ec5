"""Edge-directed sweeps of the CDF arithmetic on EVERY restatement of it the device holds (include/divans_gpu.h,
divans_gpu_selftest_cdf_ops_on): the generation-1 streaming kernels, lit_decode2.hip, the bucketed encoder passes, and in
experiment builds lit_decode_t.hip.  The
stream-level parity tests take a row only through the states their data reaches; these put rows, Weights and rANS states AT
the edges (op 8 loads them) and compare every record with the oracle's C script interpreter (oracle/cdf_ops.c), which the
independent Python restatement double-checks on a thinning of every sweep (tests/cdf_ops_sweeps.py; CPU tier:
tests/test_cdf_ops_oracle_cpu.py).  Expected values never come from a device implementation.

  blend         every speed the tests and the benchmark use: rows of every shape at each total of the speed's trajectory whose
                next update renormalises, one update before and after, the smallest and the largest; every symbol, twice
  search        >= 32 rows (totals 16 .. 32767, every shape): all 16 symbols, all 32768 slots, and the decode step at each slot
  average       >= 64 ordered row pairs x every mixing rate the Weights can hand over (q << 7, q = 0 .. 256)
  mixed_encode  the mixing encoder's nibble on those pairs: every rate, every symbol, Weights loaded with the values that move
                the normalisation (mix_nibble's shortcut total, mixed_sf2's masked neighbour, each feeding weights_update)
  state         the decode step at states 2^31 .. 2^63 - 1 (the cuts at bits 15 and 47 of advance_state), slots at both ends of a symbol
  mixed_decode  the mixing decoder's nibble over slots across the range
  weights       Weights::update on the cross product of edge probabilities from every loaded Weights; 2 x 20 000 one-sided updates
"""
import numpy as np
import pytest

import cdf_ops_sweeps as sw
import gpu_harness as gh

pytestmark = pytest.mark.gpu
IMPLS = gh.implementations()


@pytest.fixture(scope="module")
def codec():
    import divans_amd as da
    c = da.LiteralCodec(da.config_simple(), 4096)
    yield c
    c.close()


def run_sweep(codec, impl, name):
    ops, exp, bounds = sw.sweep(name)
    for lo, hi in sw.chunks(bounds):         # whole cases per call: a case loads what it needs, every call starts from the default state
        got = codec.selftest_cdf_ops(ops[lo:hi], impl)
        sw.compare(impl, ops[lo:hi], got, exp[lo:hi], f"{name} sweep, ops {lo}..{hi}")
    return ops, exp, bounds


def test_speeds_of_the_sweeps_are_supported():
    import divans_amd as da
    speeds = sw.all_speeds()
    for sp in sw.default_speeds() + [(1, 16384), (8160, 1), (8100, 16384), (4096, 16384)]:
        assert sp in speeds
    for sp in speeds:
        assert da.speed_supported(*sp), sp


@pytest.mark.parametrize("impl", IMPLS)
def test_blend_at_the_renormalisation_edges(codec, impl):
    run_sweep(codec, impl, "blend")


@pytest.mark.parametrize("impl", IMPLS)
def test_start_freq_and_search_at_every_slot(codec, impl):
    ops, exp, bounds = run_sweep(codec, impl, "search" if impl != 2 else "search_encoder")
    for i in range(len(bounds) - 1):          # the records equal the oracle's: the reference's invariants hold for both or neither
        sw.check_search_records(ops[bounds[i]:bounds[i + 1]], exp[bounds[i]:bounds[i + 1]])


@pytest.mark.parametrize("impl", IMPLS)
def test_average_at_every_reachable_rate(codec, impl):
    run_sweep(codec, impl, "average")


@pytest.mark.parametrize("impl", IMPLS)
def test_mixed_encode_step_feeds_the_weights(codec, impl):
    run_sweep(codec, impl, "mixed_encode")


@pytest.mark.parametrize("impl", [i for i in IMPLS if i != 2])
def test_state_step_across_the_state_range(codec, impl):
    run_sweep(codec, impl, "state")


@pytest.mark.parametrize("impl", [i for i in IMPLS if i != 2])
def test_mixed_decode_step(codec, impl):
    run_sweep(codec, impl, "mixed_decode")


@pytest.mark.parametrize("impl", IMPLS)
def test_weights_update_at_the_values_that_move_the_shifts(codec, impl):
    run_sweep(codec, impl, "weights")
