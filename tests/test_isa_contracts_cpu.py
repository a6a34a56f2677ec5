"""The contracts of tests/tools/isa_audit.py on the default build: the six HIP sources are compiled to gfx950 assembly once (no GPU,
nothing written into the tree) and every kernel is checked for what the compiler does not check itself -- a hidden load's register
touched before a covering wait, a wide hidden store's data overwritten too early, a hidden store feeding a load, and the facts
DESIGN.md section 4 asserts of the decoders (scratch, generic-pointer accesses).  A missing hipcc is an error, not a skip."""
import os
import re
import sys
import time

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import isa_audit as ia  # noqa: E402

CM_HS, CM_HC = 1, 2     # lit_decode2.hip: the high-nibble stride / context-map row caches


@pytest.fixture(scope="module")
def build():
    t0 = time.time()
    texts = ia.compile_assembly()
    t1 = time.time()
    audit = ia.audit_build(texts)
    names = ia.demangle(set(audit.scratch))
    print("\nisa audit: %d sources compiled in %.0f s, %d kernels analysed in %.0f s" % (len(texts), t1 - t0, len(audit.scratch), time.time() - t1))
    return texts, audit, names


def _template_args(nice):
    m = re.match(r"(\w+)<(.*)>$", nice)
    return (m.group(1), [a.strip() for a in m.group(2).split(",")]) if m else (nice, [])


def _async_instance(nice):
    """Does the source give this decoder instance a gload_async?  decode2_body requests the high-nibble rows through
    load<..., HIGH && DIVANS_D2_ASYNC>: the stride row where CM has CM_HS, with mixing also the context-map row where it has CM_HC."""
    fam, args = _template_args(nice)
    if fam in ("lit_decode2_kernel_w7", "lit_decode2_kernel_any"):
        mix, cm = args[2] == "true", int(args[4])
    elif fam in ("lit_decode2_cmd_kernel", "lit_decode2_cmd_hist_kernel"):
        mix, cm = args[2] == "true", int(args[3])
    else:
        return False
    return bool(cm & ((CM_HS | CM_HC) if mix else CM_HS))


def test_no_findings(build):
    _, audit, names = build
    print("\nexemptions: guarded waits %d, complement-arm writes %d, complement-arm reads %d, uniform-flag branches %d; "
          "loads that can run under a hidden store whose base the assembly does not give: %d" % (
              audit.guarded_waits, audit.complement_writes, audit.complement_reads, audit.flag_branches, audit.store_unknown))
    lines = ["%s | %s | line %d | %s | %s" % (f.rule, names.get(f.kernel, f.kernel), f.line, f.text, f.detail) for f in audit.findings]
    assert not lines, "\n" + "\n".join(lines)


def test_kernels_with_hidden_traffic_are_the_ones_the_source_implies(build):
    _, audit, names = build
    nice = lambda ks: sorted(names[k] for k in ks)
    rans = ["rans_encode2_kernel", "rans_encode2_split_kernel", "rans_encode_kernel"]       # rans_encode_chunk / _split: prefetch ring and word stores
    chains = [n for n in nice(audit.scratch) if _template_args(n)[0] in ("bucket_chain_kernel", "mix_chain_kernel", "mix_chain_ctx_kernel")]   # bk_store_group
    decoders = [n for n in nice(audit.scratch) if _async_instance(n)]
    assert len(chains) >= 3 and len(decoders) >= 90
    assert nice(audit.hidden_loads) == sorted(decoders + rans)
    assert nice(audit.hidden_stores) == sorted(chains + rans)
    # every asynchronous decoder waits for its requests in one place, the byte loop, under the ballot
    assert audit.guarded_waits == len(decoders)
    # the rANS ring: sixteen requests in front of the loop and sixteen inside it, per kernel
    assert all(audit.hidden_loads[k] == 32 for k in audit.hidden_loads if names[k] in rans)


def test_no_hidden_load_escapes_the_parser(build):
    texts, audit, _ = build
    blocks = loads = 0
    for text in texts.values():         # counted on the raw text, without the parser
        for body in re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", text, re.S):
            n = len(re.findall(r"^\s*(?:buffer|global|flat|scratch)_load_", body, re.M))
            loads += n
            blocks += n > 0
    assert loads > 0 and sum(audit.hidden_loads.values()) == loads and audit.asm_load_blocks == blocks


def test_decoder_facts_hold_for_every_instance(build):
    _, audit, names = build
    any_instances = [k for k in audit.scratch if names[k].startswith("lit_decode2_kernel_any<")]
    assert len(any_instances) >= 32 and all(audit.scratch[k] == 0 for k in any_instances)
    # generic-pointer accesses: one flat_load_dword (out_sizes[s] or the stream_len kernel argument) in the kernels that make that choice
    assert audit.flat and all(len(v) == 1 and v[0].startswith("flat_load_dword ") for v in audit.flat.values())
    families = {_template_args(names[k])[0] for k in audit.flat}
    assert families <= {"lit_decode2_kernel_any", "lit_model_encode_kernel", "lit_decode_kernel"}, families
    # the streaming encoder instances that ran before the open fault of DESIGN.md section 4: no scratch, that one flat load
    enc = [k for k in audit.scratch if names[k].startswith("lit_model_encode_kernel<-1, true, false")]
    assert enc and all(audit.scratch[k] == 0 and len(audit.flat.get(k, [])) <= 1 for k in enc)
