"""Wait states of the library's gfx950 assembly (tools/asm_hazards.py; no device): hipcc pads nothing inside an `asm volatile` string, and the
strings of ba_solve.hip, orb_fast.hip, orb_pyramid.hip and orb_describe.hip pad by hand. The requirement of every producer -> consumer class is
read off probe kernels hipcc pads itself; the scanner is checked on hand-written fragments (one that violates and one that just satisfies
every rule); then every csrc/*.hip must scan clean. The .s of a source is compiled once per process and shared with
test_kernel_resources.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.fixture(scope="module")
def ah():
    import asm_hazards
    return asm_hazards


@pytest.fixture(scope="module")
def req(ah):
    return ah.calibrate()


def _fn(body, name="frag"):
    return "\t.type\t%s,@function\n%s:\n%s\n.Lfunc_end0:\n" % (name, name, "\n".join("\t" + l if not l.endswith(":") else l for l in body))


def _pad_nop(n):
    return ["s_nop %d" % (n - 1)] if n > 0 else []


# (rule key, producer, consumer): the consumer reads what the producer wrote
PAIRS = [
    ("valu_dpp", "v_mul_f64 v[248:249], v[244:245], v[246:247]", "v_mov_b64_dpp v[246:247], v[248:249] row_newbcast:15 row_mask:0xf bank_mask:0xf"),
    ("valu_dpp", "v_add_f32_e32 v7, v1, v2", "v_add_f32_dpp v3, v7, v7 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"),
    ("trans_valu", "v_rsq_f64_e32 v[10:11], v[12:13]", "v_mul_f64 v[14:15], v[10:11], v[16:17]"),
    ("trans_valu", "v_rcp_f32_e32 v10, v12", "v_fma_f32 v14, -v10, |v16|, v18"),
    ("valu_mfma", "v_xor_b32_e32 v5, 0x80000000, v5", "v_mfma_f64_16x16x4_f64 v[20:27], v[4:5], v[8:9], v[20:27]"),                     # A
    ("valu_mfma", "v_mul_f64 v[8:9], v[0:1], v[2:3]", "v_mfma_f64_16x16x4_f64 v[20:27], v[4:5], v[8:9], v[20:27]"),                      # B
    ("valu_mfma", "v_accvgpr_write_b32 a7, v3", "v_mfma_f64_16x16x4_f64 a[0:7], v[4:5], v[8:9], a[0:7]"),                                 # C
    ("mfma64_valu", "v_mfma_f64_16x16x4_f64 v[20:27], v[4:5], v[8:9], v[20:27]", "v_add_f64 v[0:1], v[26:27], v[2:3]"),
    ("mfma64_valu", "v_mfma_f64_16x16x4_f64 a[0:7], v[4:5], v[8:9], 0", "v_accvgpr_read_b32 v1, a3"),
    ("mfma64_mem", "v_mfma_f64_16x16x4_f64 v[20:27], v[4:5], v[8:9], v[20:27]", "ds_write_b128 v0, v[24:27] offset:16"),
    ("mfma64_mem", "v_mfma_f64_16x16x4_f64 a[0:7], v[4:5], v[8:9], 0", "global_store_dwordx4 v9, a[0:3], s[2:3]"),
    ("mfma8_valu", "v_mfma_i32_32x32x32_i8 v[0:15], v[16:19], v[20:23], 0", "v_max_i32_e32 v30, v15, v31"),
    ("valu_readlane", "v_xor_b32_e32 v1, v2, v1", "v_readfirstlane_b32 s0, v1"),
    ("valu_readlane", "v_xor_b32_e32 v1, v2, v1", "v_readlane_b32 s0, v1, 5"),
    ("m0_ldsdma", "s_mov_b32 m0, s7", "global_load_lds_dwordx4 v4, s[2:3]"),
    ("valu_sdwa", "v_mul_lo_u32 v1, v2, v1", "v_add_u32_sdwa v1, v1, v3 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1"),
]
FILLER = ["s_add_u32 s40, s40, 1", "v_mov_b32_e32 v100, 0", "s_waitcnt lgkmcnt(0)", "v_add_u32_e32 v101, v102, v103"]   # touch no register of PAIRS


def test_calibration_reads_the_requirements_off_hipcc(ah, req):
    """Every class has a probe that hipcc padded (or left adjacent); the classes the hand-written strings lean on are not zero. For the reader:
    ROCm 7's hipcc leaves DPP 2, transcendental 1, MFMA operand 2, f64 16x16x4 result 19 (VALU) / 18 (memory), i8 32x32x32 result 12."""
    print({r.what: req[r.key] for r in ah.RULES})
    assert set(req) == {r.key for r in ah.RULES}
    for k in ("valu_dpp", "valu_mfma", "mfma64_valu", "mfma64_mem", "mfma8_valu"):
        assert req[k] > 0, k
    assert req["mfma64_valu"] >= req["valu_mfma"] and req["mfma64_mem"] >= req["valu_dpp"]   # (a 16-pass result waits longer than an operand)


def test_a_probe_that_yields_no_pair_is_an_error(ah):
    """A probe the optimiser folded away (no producer -> consumer pair in its function) raises; so does one whose gap holds no s_nop."""
    rule = {r.key: r for r in ah.RULES}["valu_dpp"]
    body = dict(ah.functions(_fn(["v_mov_b32_e32 v1, 0", "global_store_dword v0, v1, s[2:3]", "s_endpgm"])))["frag"]
    with pytest.raises(RuntimeError, match="folded away"):
        ah.measure(body, rule)
    body = dict(ah.functions(_fn(["v_mul_f64 v[0:1], v[0:1], v[2:3]", "s_waitcnt vmcnt(0)", "v_mov_b64_dpp v[2:3], v[0:1] row_newbcast:15 row_mask:0xf bank_mask:0xf"])))["frag"]
    assert ah.measure(body, rule) == (1, False)     # one state, none of it an s_nop: calibrate() refuses such a probe
    body = dict(ah.functions(_fn(["v_mul_f64 v[0:1], v[0:1], v[2:3]", "s_nop 1", "v_mov_b64_dpp v[2:3], v[0:1] row_newbcast:15 row_mask:0xf bank_mask:0xf"])))["frag"]
    assert ah.measure(body, rule) == (2, True)


@pytest.mark.parametrize("key,producer,consumer", PAIRS)
def test_scanner_on_fragments_one_state_short_and_just_enough(ah, req, key, producer, consumer):
    need = req[key]
    if need == 0:   # (hipcc asks for nothing here: adjacent is clean and there is nothing to violate)
        assert ah.scan(_fn([producer, consumer]), req) == []
        return
    # just enough: padded by one s_nop; by independent instructions; by a mix of the two
    assert ah.scan(_fn([producer] + _pad_nop(need) + [consumer]), req) == []
    assert ah.scan(_fn([producer] + [FILLER[i % 4] for i in range(need)] + [consumer]), req) == []
    assert ah.scan(_fn([producer, FILLER[0]] + _pad_nop(need - 1) + [consumer]), req) == []
    # one state short, each way
    for body in ([producer] + _pad_nop(need - 1) + [consumer], [producer] + [FILLER[i % 4] for i in range(need - 1)] + [consumer]):
        found = [f for f in ah.scan(_fn(body), req, "frag.s") if f.rule.key == key]
        assert len(found) == 1, (body, [str(f) for f in ah.scan(_fn(body), req)])
        f = found[0]
        assert f.found == need - 1 and f.required == need and f.producer.text == producer and f.consumer.text == consumer
        assert f.consumer.line == 2 + len(body) and "frag" in str(f) and "%d required" % need in str(f)


def test_scanner_register_overlap_modifiers_and_history(ah, req):
    need = req["valu_dpp"]
    dpp = "v_mov_b32_dpp v9, v3 row_shr:1 row_mask:0xf bank_mask:0xf"
    # a 64-bit pair overlapping the read by its upper half only / not at all
    assert len(ah.scan(_fn(["v_mul_f64 v[2:3], v[0:1], v[4:5]"] + _pad_nop(need - 1) + [dpp]), req)) == 1
    assert ah.scan(_fn(["v_mul_f64 v[4:5], v[0:1], v[6:7]"] + _pad_nop(need - 1) + [dpp]), req) == []
    assert ah.scan(_fn(["v_mul_f64 v[0:1], v[2:3], v[4:5]"] + _pad_nop(need - 1) + [dpp]), req) == []     # (v3 is read by the producer, not written)
    # a source behind a modifier and in front of the trailing DPP controls is still a source; the destination is not
    i = ah.Ins(1, "v_fma_f64 v[0:1], -v[2:3], |v[4:5]|, -|v[6:7]|")
    assert i.dst == {("v", 0), ("v", 1)} and i.src == {("v", k) for k in range(2, 8)}
    i = ah.Ins(1, "v_mov_b64_dpp v[246:247], v[248:249] row_newbcast:15 row_mask:0xf bank_mask:0xf")
    assert i.dst == {("v", 246), ("v", 247)} and i.src == {("v", 248), ("v", 249)}
    i = ah.Ins(1, "v_cvt_f32_i32_sdwa v1, sext(v2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1")
    assert i.dst == {("v", 1)} and i.src == {("v", 2)}
    assert ah.Ins(1, "v_cmp_lt_f64_e32 vcc, v[0:1], v[2:3]").dst == set() and ah.Ins(1, "v_readfirstlane_b32 s0, v1").dst == set()
    assert ah.Ins(1, "s_nop 7").states == 8 and ah.Ins(1, "s_nop 0").states == 1 and ah.Ins(1, "s_waitcnt vmcnt(0)").states == 1
    assert ah.Ins(1, "global_load_lds_dwordx4 v4, s[2:3]").src == {("v", 4), ("m0", 0)} and ah.Ins(1, "s_mov_b32 m0, s3").dst == {("m0", 0)}
    assert ah.Ins(1, "s_mov_b32 s3, m0").dst == set()
    # the history ends at a label a branch names and behind s_branch, not at a label nothing jumps to
    prod = "v_add_f32_e32 v3, v1, v2"
    assert len(ah.scan(_fn([prod, ".LBB0_9:", dpp]), req)) == 1
    assert ah.scan(_fn(["s_cbranch_scc1 .LBB0_2", prod, ".LBB0_2:", dpp]), req) == []
    assert ah.scan(_fn([prod, "s_branch .LBB0_3", dpp, ".LBB0_3:", "s_endpgm"]), req) == []
    # comments, directives and the inline-asm markers are not instructions
    assert len(ah.scan(_fn([prod, ";;#ASMSTART", "; a comment", ".loc 1 2 3", ";;#ASMEND", dpp]), req)) == 1
    # two functions: each is reported under its own (demangled) name
    two = _fn([prod, dpp], "_ZN3ovs6k_testEv") + _fn([prod] + _pad_nop(need) + [dpp], "clean")
    assert [f.kernel for f in ah.scan(two, req)] == ["ovs::k_test"]


def test_scanner_sees_the_last_pivots_broadcast_of_the_hand_scheduled_block(ah, req):
    """The sequence k_chol_resident had until this check existed (factor_steps<15>: y_15 broadcast one state behind its product), as hipcc
    printed it, and the padded form."""
    was = ["v_mul_f64 v[248:249], v[244:245], v[246:247]", ";;#ASMEND", "ds_write_b64 v250, v[246:247] offset:120", ";;#ASMSTART",
           "v_mov_b64_dpp v[246:247], v[248:249] row_newbcast:15 row_mask:0xf bank_mask:0xf"]
    found = ah.scan(_fn(was, "_ZN3ovs15k_chol_residentILb1EEEvPdS1_iPi"), req)
    assert len(found) == 1 and found[0].found == 1 and found[0].required == req["valu_dpp"] and "k_chol_resident<true>" in str(found[0])
    assert "row_newbcast:15" in str(found[0])
    assert ah.scan(_fn(was[:4] + ["s_nop 1"] + was[4:]), req) == []


def test_every_kernel_source_is_free_of_wait_state_findings(ah, req):
    """collect() over all of csrc/*.hip: no producer -> consumer pair closer than hipcc itself would leave it. The zero is a zero over
    something: the classes of the hand-written strings all occur."""
    found = ah.collect()
    for f in found:
        print(f)
    assert not found, "\n".join(str(f) for f in found)
    cov = ah.coverage()
    print(cov)
    assert cov["valu_dpp"][1] >= 400          # (ba_solve.hip alone has that many v_mov_b64_dpp)
    for k in ("trans_valu", "mfma64_valu", "mfma64_mem", "mfma8_valu", "m0_ldsdma"):
        assert cov[k][0] > 0, k
    for k in ("valu_mfma", "valu_readlane", "valu_sdwa"):
        assert cov[k][1] > 0, k
