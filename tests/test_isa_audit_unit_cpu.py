"""tests/tools/isa_audit.py on hand-written gfx950 assembly: every rule of the three contracts in a form that passes and in a
form that fails, the failing one for the reason it names.  No compiler, no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import isa_audit as ia  # noqa: E402

LOAD = "\t;;#ASMSTART\n\tbuffer_load_ushort v33, v33, s[28:31], 0 offen\n\t;;#ASMEND\n"
WAIT = "\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n"


def kernel(body, name="_Z6kernelv"):
    return "%s: ; @%s\n; %%bb.0:\n%s\ts_endpgm\n.Lfunc_end0:\n" % (name, name, body)


def rules(body, **kw):
    a = ia.audit_text(kernel(body, **kw))
    return [f.rule for f in a.findings], a


def test_wait_then_use_passes_and_use_without_wait_fails():
    assert rules(LOAD + "\tv_add_u32_e32 v1, v2, v3\n" + WAIT + "\tv_and_b32_e32 v1, 0xffff, v33\n")[0] == []
    got, a = rules(LOAD + "\tv_add_u32_e32 v1, v2, v3\n\tv_and_b32_e32 v1, 0xffff, v33\n" + WAIT)
    assert got == ["A.read"] and "v33" in a.findings[0].detail and a.findings[0].text.startswith("v_and_b32")
    # the compiler's own wait covers too, a wait for the other counters does not
    assert rules(LOAD + "\ts_waitcnt vmcnt(0) lgkmcnt(0)\n\tv_mov_b32_e32 v1, v33\n")[0] == []
    assert rules(LOAD + "\ts_waitcnt lgkmcnt(0)\n\tv_and_b32_e32 v1, 1, v33\n")[0] == ["A.read"]
    assert rules(LOAD + "\ts_waitcnt vmcnt(1)\n\tv_and_b32_e32 v1, 1, v33\n")[0] == ["A.read"]       # a buffer load: vmcnt(0) only
    # a register range that holds the destination is the destination
    assert rules(LOAD + "\tv_lshl_add_u64 v[32:33], v[8:9], 2, s[46:47]\n")[0] == ["A.write"]
    assert rules(LOAD + "\tv_lshl_add_u64 v[34:35], v[8:9], 2, s[46:47]\n")[0] == []


# one stream per trip of the outer loop, the byte loop inside it requests the next row and waits under a guard
STREAMS = """\ts_branch .LBB0_2
.LBB0_1:
\ts_or_b64 exec, exec, s[8:9]
\tv_add_u32_e32 v8, s95, v8
\tv_cmp_le_u32_e32 vcc, s59, v8
\ts_cbranch_vccnz .LBB0_9
.LBB0_2:
%s\tglobal_load_dword v5, v[6:7], off
%s.LBB0_3:
\tv_cmp_ne_u16_e32 vcc, 0, v38
\ts_cbranch_vccz .LBB0_5
; %%bb.4:
""" + WAIT + """.LBB0_5:
\tv_and_b32_e32 v1, 0xffff, v33
\tv_lshl_add_u32 v33, v22, 5, v40
""" + LOAD + """\ts_add_u32 s4, s4, 1
\ts_cmp_lt_u32 s4, s5
\ts_cbranch_scc1 .LBB0_3
; %%bb.6:
%s\ts_branch .LBB0_1
.LBB0_9:
"""


def test_stream_end_shape():
    redefine = "\tv_lshl_add_u64 v[32:33], v[8:9], 2, s[46:47]\n"
    # the register is next defined behind the loop header's own vmcnt(0): passes (the shape of <-1, true, false, true, 1>)
    got, a = rules(STREAMS % ("", "\ts_waitcnt vmcnt(0)\n" + redefine, ""))
    assert got == [] and a.guarded_waits == 1 and a.hidden_loads == {"_Z6kernelv": 1}
    # ... in front of it: the request past the stream's last byte may land in the next stream's address
    got, a = rules(STREAMS % (redefine, "\ts_waitcnt vmcnt(0)\n", ""))
    assert got == ["A.write"] and a.findings[0].text.startswith("v_lshl_add_u64 v[32:33]")
    # ... and the fix: one wait behind the byte loop
    assert rules(STREAMS % (redefine, "\ts_waitcnt vmcnt(0)\n", WAIT))[0] == []
    # pending at the end of the program is allowed
    assert rules(LOAD)[0] == []


def test_guarded_wait():
    ok = "\tv_cmp_ne_u16_e32 vcc, 0, v38\n\ts_cbranch_vccz .LBB0_2\n; %bb.1:\n" + WAIT + ".LBB0_2:\n\tv_and_b32_e32 v1, 1, v33\n"
    got, a = rules(LOAD + ok)
    assert got == [] and a.guarded_waits == 1
    # a divergent skip (exec) is no ballot, and a block that holds more than the wait is not the shape
    assert rules(LOAD + ok.replace("s_cbranch_vccz", "s_cbranch_execz"))[0] == ["A.read"]
    assert rules(LOAD + ok.replace(WAIT, WAIT + "\tv_mov_b32_e32 v9, 0\n"))[0] == ["A.read"]
    # a guard over a counted wait is not one either
    assert rules(LOAD + ok.replace("vmcnt(0)", "vmcnt(1)"))[0] == ["A.read"]


ARMS = """\tv_cmp_ne_u32_e64 s[2:3], s70, v44
\ts_and_saveexec_b64 s[64:65], s[2:3]
\ts_xor_b64 s[2:3], exec, s[64:65]
\ts_cbranch_execz .LBB0_2
; %bb.1:
""" + LOAD + """.LBB0_2:
\ts_or_saveexec_b64 s[2:3], s[2:3]
\tv_mov_b32_e32 v47, 1
\ts_xor_b64 exec, exec, s[2:3]
; %bb.3:
\tds_read_u16 v33, v46
; %bb.4:
\ts_or_b64 exec, exec, s[2:3]
"""


def test_complementary_exec_arm():
    tail = WAIT + "\tv_and_b32_e32 v1, 1, v33\n"
    got, a = rules(ARMS + tail)
    assert got == [] and a.complement_writes == 1
    # the same write behind the s_or that joins the arms can hit the loading lanes
    moved = ARMS.replace("\tds_read_u16 v33, v46\n", "") + "\tds_read_u16 v33, v46\n"
    assert rules(moved + tail)[0] == ["A.write"]
    # ... and so can one between s_or_saveexec and the s_xor, where exec is the whole region's
    assert rules(ARMS.replace("v_mov_b32_e32 v47, 1", "v_mov_b32_e32 v33, 1") + tail)[0] == ["A.write"]
    # the else mask in the saved register itself, and the s_andn2_saveexec form
    same = ARMS.replace("s_xor_b64 s[2:3], exec, s[64:65]", "s_xor_b64 s[64:65], exec, s[64:65]").replace("s[2:3], s[2:3]", "s[64:65], s[64:65]") \
               .replace("exec, exec, s[2:3]", "exec, exec, s[64:65]")
    assert rules(same + tail)[0] == []
    andn2 = ARMS.replace("\ts_or_saveexec_b64 s[2:3], s[2:3]\n\tv_mov_b32_e32 v47, 1\n\ts_xor_b64 exec, exec, s[2:3]\n", "\ts_andn2_saveexec_b64 s[2:3], s[2:3]\n")
    assert rules(andn2 + tail)[0] == []
    # a load from in front of the region is not in its then arm: the else arm's lanes may be loading ones
    assert rules(LOAD + ARMS.replace(LOAD, "\tv_mov_b32_e32 v9, 0\n") + tail)[0] == ["A.write"]
    # a mask register written in between is no else mask any more
    assert rules(ARMS.replace(LOAD, LOAD + "\ts_mov_b64 s[2:3], s[10:11]\n") + tail)[0] == ["A.write"]


FLAG = """\ts_mov_b64 s[2:3], -1
\tv_cmp_le_u32_e32 vcc, s70, v44
\ts_cbranch_vccz .LBB0_2
; %bb.1:
""" + LOAD + """\ts_mov_b64 s[2:3], 0
.LBB0_2:
\tv_mov_b32_e32 v30, 0
\ts_andn2_b64 vcc, exec, s[2:3]
\ts_cbranch_vccnz .LBB0_4
; %bb.3:
\tds_read_u16 v33, v46
.LBB0_4:
""" + WAIT


def test_uniform_flag():
    got, a = rules(FLAG)
    assert got == [] and a.flag_branches == 1
    assert rules(FLAG.replace("\ts_mov_b64 s[2:3], 0\n", ""))[0] == ["A.write"]            # the load's path does not clear the flag
    assert rules(FLAG.replace("s_cbranch_vccnz", "s_cbranch_vccz"))[0] == ["A.write"]      # the branch goes the other way
    assert rules(FLAG.replace("\tv_mov_b32_e32 v30, 0\n", "\ts_or_b64 s[2:3], s[2:3], s[8:9]\n"))[0] == ["A.write"]   # the flag is no constant any more


def test_copy_spill_call():
    assert rules(LOAD + "\tv_mov_b32_e32 v70, v33\n" + WAIT)[0] == ["A.copy"]
    assert rules(LOAD + "\tv_accvgpr_write_b32 a3, v33\n" + WAIT)[0] == ["A.copy"]
    assert rules(LOAD + "\tscratch_store_dword off, v33, off offset:16\n" + WAIT)[0] == ["A.spill"]
    assert rules(LOAD + "\ts_swappc_b64 s[30:31], s[16:17]\n" + WAIT)[0] == ["A.call"]
    assert rules(LOAD + WAIT + "\tscratch_store_dword off, v33, off offset:16\n\tv_mov_b32_e32 v70, v33\n\ts_swappc_b64 s[30:31], s[16:17]\n")[0] == []


def test_out_of_line_block_is_followed_where_control_goes():
    # the use stands in the text between the load and the wait, but only the path through the wait reaches it
    body = LOAD + "\ts_branch .LBB0_2\n.LBB0_1:\n\tv_and_b32_e32 v1, 1, v33\n\ts_branch .LBB0_3\n.LBB0_2:\n" + WAIT + "\ts_branch .LBB0_1\n.LBB0_3:\n"
    assert rules(body)[0] == []
    # and the reverse: the wait stands in front of the use in the text, but control reaches the use without it
    body = LOAD + "\ts_branch .LBB0_2\n.LBB0_1:\n" + WAIT + "\ts_branch .LBB0_3\n.LBB0_2:\n\tv_and_b32_e32 v1, 1, v33\n\ts_branch .LBB0_1\n.LBB0_3:\n"
    assert rules(body)[0] == ["A.read"]


def ring(n_wait, k_use, stores=0):
    """sixteen hidden 16-byte loads into v[10:13] .. v[70:73], `stores` hidden stores, vmcnt(n_wait), then a use of load k_use's first register"""
    body = "".join("\t;;#ASMSTART\n\tglobal_load_dwordx4 v[%d:%d], v[2:3], off\n\t;;#ASMEND\n" % (10 + 4 * k, 13 + 4 * k) for k in range(16))
    body += "\t;;#ASMSTART\n\tglobal_store_dword v[4:5], v6, off\n\t;;#ASMEND\n" * stores
    return body + "\t;;#ASMSTART\n\ts_waitcnt vmcnt(%d)\n\t;;#ASMEND\n\tv_add_u32_e32 v1, 1, v%d\n" % (n_wait, 10 + 4 * k_use) + WAIT


def test_counted_wait_over_sixteen_loads():
    # vmcnt(12) proves the loads with at least twelve younger ones: 0 .. 3, the first quad
    for k in range(16):
        assert rules(ring(12, k))[0] == ([] if k <= 3 else ["A.read"]), k
    assert rules(ring(15, 0))[0] == [] and rules(ring(15, 1))[0] == ["A.read"]
    assert rules(ring(0, 15))[0] == []
    # stores share the counter but may be acknowledged early: they do not make a load older
    assert rules(ring(12, 3, stores=5))[0] == [] and rules(ring(12, 4, stores=5))[0] == ["A.read"]
    # a hidden load into a register whose earlier load is not proven complete
    again = "\t;;#ASMSTART\n\tglobal_load_dwordx4 v[10:13], v[2:3], off\n\t;;#ASMEND\n"
    assert rules(again + again + WAIT)[0] == ["A.write"]
    assert rules(again + again.replace("10:13", "14:17") + "\ts_waitcnt vmcnt(1)\n" + again + WAIT)[0] == []


QUAD = "\t;;#ASMSTART\n\tglobal_store_dwordx4 v[2:3], v[4:7], off%s\n\t;;#ASMEND\n"


def test_wide_store_pad():
    got, a = rules(QUAD % "" + "\tv_mov_b32_e32 v5, 0\n")
    assert got == ["B.store_pad"] and "global_store_dwordx4" in a.findings[0].detail
    assert rules(QUAD % "" + "\ts_mov_b32 s4, 0\n\tv_mov_b32_e32 v5, 0\n")[0] == ["B.store_pad"]       # the second wait state
    assert rules(QUAD % "" + "\ts_mov_b32 s4, 0\n\ts_mov_b32 s5, 0\n\tv_mov_b32_e32 v5, 0\n")[0] == []
    assert rules(QUAD % "" + "\ts_nop 1\n\tv_mov_b32_e32 v5, 0\n")[0] == []
    assert rules(QUAD % "" + "\ts_nop 0\n\tv_mov_b32_e32 v5, 0\n")[0] == ["B.store_pad"]
    assert rules(QUAD % "\n\ts_nop 1" + "\tv_mov_b32_e32 v5, 0\n")[0] == []                              # the pad inside the string
    assert rules(QUAD % "" + "\tv_mov_b32_e32 v3, 0\n\tv_mov_b32_e32 v8, 0\n")[0] == []                  # the address is not the data
    assert rules(QUAD % "" + "\ts_branch .LBB0_1\n.LBB0_1:\n\tv_mov_b32_e32 v7, 0\n")[0] == ["B.store_pad"]   # across a branch
    assert rules((QUAD % "").replace("dwordx4", "dwordx2") + "\tv_mov_b32_e32 v5, 0\n")[0] == []         # 8 bytes: no hazard
    assert rules("\t;;#ASMSTART\n\tbuffer_store_dwordx4 v[4:7], v2, s[28:31], 0 offen\n\t;;#ASMEND\n\tv_mov_b32_e32 v4, 0\n")[0] == ["B.store_pad"]


def test_hidden_store_feeding_a_load():
    store = "\t;;#ASMSTART\n\tbuffer_store_short v4, v2, s[28:31], 0 offen\n\t;;#ASMEND\n"
    assert rules(store + "\tbuffer_load_ushort v9, v3, s[28:31], 0 offen\n")[0] == ["B.store_read"]
    assert rules(store + "\ts_waitcnt vmcnt(0)\n\tbuffer_load_ushort v9, v3, s[28:31], 0 offen\n")[0] == []
    assert rules(store + "\ts_waitcnt vmcnt(1)\n\tbuffer_load_ushort v9, v3, s[28:31], 0 offen\n")[0] == ["B.store_read"]
    assert rules(store + "\tbuffer_load_ushort v9, v3, s[32:35], 0 offen\n")[0] == []
    got, a = rules("\t;;#ASMSTART\n\tglobal_store_dword v[2:3], v4, off\n\t;;#ASMEND\n\tglobal_load_dword v9, v[6:7], off\n")
    assert got == [] and a.store_unknown == 1 and a.hidden_stores == {"_Z6kernelv": 1}


def test_contract_c():
    lds = "\tds_read_b32 v1, v2\n"
    assert rules(lds + "\tflat_load_dword v60, v[14:15]\n")[0] == []
    assert rules(lds + "\tflat_load_dword v60, v[14:15]\n\tflat_load_dword v61, v[16:17]\n")[0] == ["C.flat"]
    assert rules(lds + "\tflat_store_dword v[14:15], v60\n")[0] == ["C.flat"]
    assert rules(lds + "\tflat_load_ushort v60, v[14:15]\n")[0] == ["C.flat"]
    got, a = rules("\tflat_load_dword v60, v[14:15]\n\tflat_load_dword v61, v[16:17]\n")
    assert got == [] and len(a.flat["_Z6kernelv"]) == 2
    name = "_ZN10divans_hip22lit_decode2_kernel_anyILin1ELb1ELb0ELb1ELi17EEEvNS_8LitBatchE"
    a = ia.audit_text(kernel(lds, name=name), meta={name: {"private_segment_fixed_size": 16}})
    assert [f.rule for f in a.findings] == ["C.scratch"]
    a = ia.audit_text(kernel(lds, name=name), meta={name: {"private_segment_fixed_size": 0}})
    assert a.findings == [] and a.scratch == {name: 0}


def test_redefinition_record():
    redefine = "\tv_lshl_add_u64 v[32:33], v[8:9], 2, s[46:47]\n"
    f = ia.parse(kernel(STREAMS % (redefine, "\ts_waitcnt vmcnt(0)\n", "")))[0]
    (line, text, regs, redefs), = ia.redefinitions(f)
    assert regs == [33] and text.startswith("buffer_load_ushort v33")
    by_text = {t.split()[0]: w for _, t, w in redefs}
    assert by_text["v_lshl_add_u64"] is None                 # reached from the loop's exit with no wait on the way
    assert by_text["v_lshl_add_u32"] is not None             # the next request's address: behind the guarded wait
