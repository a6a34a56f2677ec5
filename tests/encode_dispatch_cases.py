"""Which encoder model pass a call runs: one table for every kind of codec, the three encode paths and calls with and without a
segment list (select_pass, divans_amd/csrc/capi.cpp).  tests/test_gpu_encode_dispatch.py walks the table on the GPU,
tests/test_capi_launch_contract_cpu.py on the CPU-side HIP runtime, tests/test_gpu_far_offsets.py takes its encoder rows from it."""
import struct

import bucketed_segment_cases as bc
import ctx_bucketed_cases as cx
import mix_bt_bucketed_cases as mb
import segment_cases as sc
import stride_bucketed_cases as stc

WRAP_SPEED = (0x7800, 0x7800)       # a row's total leaves i16 at its second update
NONE = 0xFFFFFFFF


def _sc(name):
    return next(f for f in sc.FAMILIES if f.name == name)


class Row:
    """family: the configuration.  types: what set_block_types is given (None: the codec stays as created, tables for the
    configuration's own block type).  accepted: set_encode_path(2) succeeds.  ran: last_encode_path() after a call without a list and
    after one with a list, for the paths 0, 1 and 2 -- where path 2 is refused the codec keeps path 1, which it was given before.
    wrap: WRAP_SPEED in every slot.  path_2_before_types: path 2 is asked for (and accepted) on the codec as created, then the block
    types are set and the table is walked."""

    def __init__(self, family, types, accepted, ran, wrap=False, path_2_before_types=False):
        self.family, self.types, self.accepted, self.ran, self.wrap, self.path_2_before_types = family, types, accepted, ran, wrap, path_2_before_types


def _bucketed(p):
    return {0: (p, 1), 1: (1, 1), 2: (p, p)}


STREAMING = {0: (1, 1), 1: (1, 1), 2: (1, 1)}
TABLE = {
    "stride_1": Row(bc.CONFIGS["A"], 8, True, _bucketed(2)),
    "stride_3": Row(stc.FAMILIES["m6"], 8, True, _bucketed(2)),
    "two_model": Row(bc.CONFIGS["C"], 1, True, _bucketed(3)),
    "context_keyed": Row(cx.FAMILIES["plain"], 8, True, _bucketed(2)),
    "context_keyed_two_model": Row(cx.FAMILIES["mix"], 8, True, _bucketed(3)),
    "two_model_block_types": Row(mb.FAMILIES["u2"], 2, True, _bucketed(3)),
    # mixing value 0 under a constant context: one bucket per stream, no pass
    "no_pass": Row(_sc(cx.REFUSED[0]), 8, False, STREAMING),
    # the stride-1 pass exists, so path 2 is accepted; every call runs the streaming kernels, which watch for wrapped rows
    "stride_1_wrap_checked": Row(bc.CONFIGS["A"], 8, True, STREAMING, wrap=True),
    # mixing value 4 with a map and two models: the two-model pass while the codec keeps one block type's tables; with all eight a
    # previous byte reaches 31 contexts (mix_bt_bucketed_cases.REFUSED) and no pass is left, whatever path was accepted before
    "two_model_as_created": Row(_sc("mm4_map_mix"), None, True, _bucketed(3)),
    "two_model_then_8_types": Row(_sc("mm4_map_mix"), 8, False, STREAMING, path_2_before_types=True),
}


def config_records(po):
    """the ten codecs of the table as the driver tests/c/capi_contract.cpp reads them (the oracle's configuration structs have the
    product's bytes: Family.pair asserts it wherever both exist)"""
    out = b""
    for key, row in TABLE.items():
        o = row.family.configure(getattr(po, "config_" + row.family.base)())
        if row.wrap:
            for i in range(4):
                o.literal_adaptation[i].inc, o.literal_adaptation[i].lim = WRAP_SPEED
        out += struct.pack("<32sIIII", key.encode(), NONE if row.types is None else row.types, int(row.path_2_before_types), int(row.family.btype), 0) + bytes(o)
    return out
