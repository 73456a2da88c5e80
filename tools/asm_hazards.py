#!/usr/bin/env python3
"""Wait states of the gfx950 assembly hipcc emits for csrc/*.hip, checked without a device.

hipcc pads the hazards of the instructions it selects itself; inside an `asm volatile` string it pads nothing, and the strings of this
library (the pivot chain of k_chol_resident, the tied matrix-instruction tile update, the SDWA and LDS-DMA statements) pad by hand. This
tool reads the .s of every source (tools/kernel_resources.py's compile step: the Makefile's flags, one cached compilation per source and
process) and reports every producer -> consumer pair that has fewer wait states between its two instructions than its class requires.

The requirement of a class is not typed in: for every class a few-line probe kernel written with builtins only (PROBES, compiled for
gfx950 into a temporary directory) is padded by hipcc's own hazard recogniser, and the number of states hipcc leaves between the probe's
producer and its consumer is the requirement. A probe counts only where hipcc inserted an s_nop between the two (then the states left are
exactly what it requires) or left them adjacent (it requires none); anything else -- the optimiser folded the probe away, or scheduled
unrelated instructions between the two -- raises instead of silently weakening or disabling a rule.

Model: every function of the .s is read straight-line along fall-through. An issued instruction is one wait state, `s_nop N` is N + 1.
"States between" a producer and a consumer is the sum over the instructions strictly between them. The history is dropped at a label some
branch names and behind an unconditional branch / s_endpgm / s_setpc_b64, so
  - a hazard across a TAKEN branch (producer before the branch, consumer at its target, a loop's back edge included) is not seen, nor is
    one across the fall-through into a label that is also a branch target;
  - only the register operands written in the instruction's text are followed (v / a registers and m0): a DPP instruction's `old` value
    (its destination, read where row_mask / bank_mask disable lanes) and other implicit reads are not;
  - classes without a rule (a matrix instruction's result read by another matrix instruction as A / B or as a partly overlapping C,
    v_cmpx -> exec readers, SGPR hazards apart from m0 -> LDS-DMA, VMEM / LDS data hazards: those are s_waitcnt's) are not checked.

usage: tools/asm_hazards.py            (prints the calibrated requirements and every finding; exit status 1 if there is one)"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr   # noqa: E402

# ---- parsing ------------------------------------------------------------------------------------------------------------------------------
_REG = re.compile(r"(?<![\w.])([va])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")
_MEM = ("ds_", "global_", "buffer_", "flat_", "scratch_", "tbuffer_")
_TRANS = re.compile(r"v_(rsq|rcp|sqrt|exp|log|sin|cos)_")
_READS_DST = re.compile(r"v_(pk_)?(fmac|mac)_|v_writelane_|v_dot\w*c_")


def _regs(tok):
    """Registers named in one operand token: {('v', 248), ('v', 249)} for `-|v[248:249]|`."""
    out = set()
    for f, one, lo, hi in _REG.findall(tok):
        if one:
            out.add((f, int(one)))
        else:
            out.update((f, i) for i in range(int(lo), int(hi) + 1))
    return out


def _split(rest):
    """Operands of an instruction: split at top-level commas (op_sel:[0,1] keeps its own)."""
    ops, depth, cur = [], 0, ""
    for ch in rest:
        if ch == "[" or ch == "(":
            depth += 1
        elif ch == "]" or ch == ")":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        ops.append(cur.strip())
    return ops


class Ins:
    """One issued instruction: mnemonic, wait states it occupies, registers written (dst) and read (src) by its written operands."""
    __slots__ = ("line", "text", "mnem", "states", "dst", "src")

    def __init__(self, line, text):
        self.line, self.text = line, text
        parts = text.split(None, 1)
        self.mnem = parts[0]
        # the register is the first blank-separated token of an operand: what follows the last one are DPP / SDWA / offset controls
        ops = [o.split()[0] if o.split() else "" for o in _split(parts[1] if len(parts) > 1 else "")]
        self.states = 1
        if self.mnem == "s_nop":
            self.states = int(ops[0], 0) + 1
        self.dst, self.src = set(), set()
        if self.mnem.startswith("v_"):
            if self.mnem.startswith("v_swap_"):
                self.dst = self.src = _regs(ops[0]) | _regs(ops[1])
            else:
                d = _regs(ops[0]) if ops and re.fullmatch(r"[va](\d+|\[\d+:\d+\])", ops[0]) else set()
                self.dst = d
                for o in ops[1 if d else 0:]:
                    self.src |= _regs(o)
                if d and _READS_DST.match(self.mnem):
                    self.src |= d
        elif self.mnem.startswith(_MEM):
            # every register a memory instruction names counts as read: address, data, and a load's destination too (overwriting a
            # matrix instruction's result inside its window is the same hazard)
            for o in ops:
                self.src |= _regs(o)
            if ops and ops[0] == "m0":
                self.src.add(("m0", 0))
            if "_load_lds_" in self.mnem or (self.mnem.startswith("buffer_load") and re.search(r"\blds\b", text)):
                self.src.add(("m0", 0))   # the LDS address of an LDS-DMA load
        elif self.mnem.startswith("s_"):
            if ops and ops[0] == "m0" and not self.mnem.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_setpc")):
                self.dst = {("m0", 0)}

    # classes
    def is_mfma(self):
        return self.mnem.startswith(("v_mfma_", "v_smfmac_"))

    def is_valu(self):   # (v_nop writes nothing; readlane / readfirstlane / compares write scalar registers: no vector dst, never a producer)
        return self.mnem.startswith("v_") and not self.is_mfma()

    def is_mem(self):
        return self.mnem.startswith(_MEM)


def functions(text):
    """[(symbol, [Ins or None])] of a .s: per `.type X,@function` symbol its instructions in program order; None marks a place where the
    straight-line history ends (a label that a branch names; behind an unconditional branch, s_endpgm, s_setpc_b64)."""
    targets = set(re.findall(r"^\s+s_c?branch\w*\s+(\S+)", text, re.M))
    funcs = set(re.findall(r"^\s+\.type\s+([^\s,]+),@function", text, re.M))
    out, cur = [], None
    for no, raw in enumerate(text.splitlines(), 1):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^([^\s:]+):", line)
        if m:
            lab = m.group(1)
            if lab in funcs:
                cur = []
                out.append((lab, cur))
            elif cur is not None and lab.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and lab in targets:
                cur.append(None)
            continue
        s = line.strip()
        if cur is None or s.startswith("."):
            continue
        ins = Ins(no, s)
        cur.append(ins)
        if ins.mnem in ("s_branch", "s_endpgm", "s_setpc_b64"):
            cur.append(None)
    return out


# ---- rules --------------------------------------------------------------------------------------------------------------------------------
class Rule:
    def __init__(self, key, what, producer, consumer, probes):
        self.key, self.what, self.producer, self.consumer, self.probes = key, what, producer, consumer, probes


def _f64_mfma(i):
    return i.mnem.startswith("v_mfma_f64_16x16x4")


def _i8_mfma(i):   # the 8-pass 32x32 forms: i8 (K = 32) and the block-scaled f8f6f4 instruction (K = 64; k_hamming_near feeds it FP4)
    return i.mnem.startswith(("v_mfma_i32_32x32x32_i8", "v_mfma_scale_f32_32x32x64_f8f6f4"))


RULES = [
    Rule("valu_dpp", "VALU write -> DPP read", Ins.is_valu, lambda i: i.is_valu() and i.mnem.endswith("_dpp"), ("valu_dpp32", "valu_dpp64")),
    Rule("trans_valu", "transcendental result -> VALU read", lambda i: bool(_TRANS.match(i.mnem)),
         lambda i: (i.is_valu() or i.is_mfma()) and not _TRANS.match(i.mnem),
         ("rsq64_valu", "rsq32_valu")),
    Rule("valu_mfma", "VALU write -> MFMA A/B/C operand", Ins.is_valu, Ins.is_mfma, ("valu_mfma_ab", "valu_mfma_c")),
    Rule("mfma64_valu", "v_mfma_f64_16x16x4_f64 result -> VALU read", _f64_mfma, Ins.is_valu, ("mfma64_valu",)),
    Rule("mfma64_mem", "v_mfma_f64_16x16x4_f64 result -> LDS / memory instruction", _f64_mfma, Ins.is_mem, ("mfma64_global", "mfma64_lds")),
    Rule("mfma8_valu", "v_mfma_i32_32x32x32_i8 / v_mfma_scale_f32_32x32x64_f8f6f4 (FP4) result -> VALU read", _i8_mfma, Ins.is_valu,
         ("mfma8_valu", "mfma4_valu")),
    Rule("valu_readlane", "VALU write -> v_readlane / v_readfirstlane", Ins.is_valu, lambda i: i.mnem.startswith(("v_readlane_", "v_readfirstlane_")),
         ("valu_readfirstlane", "valu_readlane")),
    Rule("m0_ldsdma", "SALU write of m0 -> LDS-DMA load", lambda i: i.mnem.startswith("s_") and ("m0", 0) in i.dst,
         lambda i: i.is_mem() and ("m0", 0) in i.src, ("m0_ldsdma",)),
    Rule("valu_sdwa", "VALU write -> SDWA source", Ins.is_valu, lambda i: i.is_valu() and i.mnem.endswith("_sdwa"), ("valu_sdwa",)),
]
MUST_BE_NONZERO = ("valu_dpp", "valu_mfma", "mfma64_valu", "mfma64_mem", "mfma8_valu")

PROBES = r"""
#include <hip/hip_runtime.h>
typedef double v4d __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
#define PROBE extern "C" __global__ void __launch_bounds__(64)
// (`old` comes from memory: a v_mov writing it would be the nearer VALU write, and hipcc pads for that one too)
PROBE valu_dpp32(const int* in, int* out) {
    const int x = in[threadIdx.x] ^ in[threadIdx.x + 64];
    out[threadIdx.x] = __builtin_amdgcn_update_dpp(in[threadIdx.x + 128], x, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
}
PROBE valu_dpp64(const double* in, double* out) {
    const double x = in[threadIdx.x] * in[threadIdx.x + 64];
    out[threadIdx.x] = __builtin_amdgcn_update_dpp(in[threadIdx.x + 128], x, 0x15f /* row_newbcast:15 */, 0xf, 0xf, false);
}
// (the transcendental's argument depends on every load: no s_waitcnt is left to fall between it and its reader)
PROBE rsq64_valu(const double* in, double* out) {
    const double y = in[threadIdx.x + 64];
    out[threadIdx.x] = __builtin_amdgcn_rsq(in[threadIdx.x] + y) * y;
}
PROBE rsq32_valu(const float* in, float* out) {
    const float y = in[threadIdx.x + 64];
    out[threadIdx.x] = __builtin_amdgcn_rsqf(in[threadIdx.x] + y) * y;
}
PROBE valu_mfma_ab(const double* in, v4d* out) {
    const double a = in[threadIdx.x] * in[threadIdx.x + 64], b = in[threadIdx.x + 128];
    out[threadIdx.x] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, out[threadIdx.x], 0, 0, 0);
}
PROBE valu_mfma_c(const double* in, v4d* out) {
    const double a = in[threadIdx.x], b = in[threadIdx.x + 64];
    v4d c = out[threadIdx.x];
    c.w = c.w * a;
    out[threadIdx.x] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
PROBE mfma64_valu(const double* in, double* out) {
    const v4d c = {0.0, 0.0, 0.0, 0.0};
    const v4d d = __builtin_amdgcn_mfma_f64_16x16x4f64(in[threadIdx.x], in[threadIdx.x + 64], c, 0, 0, 0);
    out[threadIdx.x] = d.x * in[threadIdx.x + 128];
}
PROBE mfma64_global(const double* in, v4d* out) {
    const v4d c = {0.0, 0.0, 0.0, 0.0};
    out[threadIdx.x] = __builtin_amdgcn_mfma_f64_16x16x4f64(in[threadIdx.x], in[threadIdx.x + 64], c, 0, 0, 0);
}
PROBE mfma64_lds(const double* in, double* out) {
    __shared__ v4d buf[64];
    const v4d c = {0.0, 0.0, 0.0, 0.0};
    buf[threadIdx.x] = __builtin_amdgcn_mfma_f64_16x16x4f64(in[threadIdx.x], in[threadIdx.x + 64], c, 0, 0, 0);
    __syncthreads();
    out[threadIdx.x] = buf[63 - threadIdx.x].y;
}
PROBE mfma8_valu(const v4i* in, int* out) {
    v16i c;
    for (int i = 0; i < 16; ++i) c[i] = 0;
    const v16i d = __builtin_amdgcn_mfma_i32_32x32x32_i8(in[threadIdx.x], in[threadIdx.x + 64], c, 0, 0, 0);
    out[threadIdx.x] = d[0] ^ in[threadIdx.x + 128].x;
}
PROBE mfma4_valu(const v8i* in, float* out) {
    v16f c;
    for (int i = 0; i < 16; ++i) c[i] = 0.f;
    const v16f d = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(in[threadIdx.x], in[threadIdx.x + 64], c, 4, 4, 0, 127, 0, 127);
    out[threadIdx.x] = d[0] * out[threadIdx.x + 64];
}
PROBE valu_readfirstlane(const int* in, int* out) {
    const int x = in[threadIdx.x] ^ in[threadIdx.x + 64];
    out[__builtin_amdgcn_readfirstlane(x)] = 1;
}
PROBE valu_readlane(const int* in, int* out) {
    const int x = in[threadIdx.x] ^ in[threadIdx.x + 64];
    out[__builtin_amdgcn_readlane(x, 5)] = 1;
}
PROBE m0_ldsdma(const int* in, int* out, int at) {
    __shared__ int buf[1024];
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in + threadIdx.x),
                                     (__attribute__((address_space(3))) void*)(buf + at), 4, 0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    out[threadIdx.x] = buf[threadIdx.x];
}
PROBE valu_sdwa(const unsigned* in, unsigned* out) {
    const unsigned q = in[threadIdx.x + 64], p = in[threadIdx.x] * q;
    out[threadIdx.x] = (p >> 16) + (q >> 16);
}
"""


def between(seq, ip, ic):
    """(wait states, whether an s_nop is among them) of the instructions strictly between positions ip < ic of one straight-line run."""
    mid = seq[ip + 1:ic]
    return sum(i.states for i in mid), any(i.mnem == "s_nop" for i in mid)


def _runs(body):
    run = []
    for i in body:
        if i is None:
            if run:
                yield run
            run = []
        else:
            run.append(i)
    if run:
        yield run


def measure(body, rule):
    """What hipcc left for `rule` in one probe function: over the consumers whose operand was LAST written by a producer of the class, the
    fewest states between the two. Returns (states, exact); raises if the pair is not there."""
    best = None
    for run in _runs(body):
        for ic, c in enumerate(run):
            if not rule.consumer(c):
                continue
            for r in c.src:
                for ip in range(ic - 1, -1, -1):
                    if r in run[ip].dst:
                        if rule.producer(run[ip]):
                            n, nop = between(run, ip, ic)
                            if best is None or n < best[0]:
                                best = (n, nop or n == 0)
                        break
    if best is None:
        raise RuntimeError("probe for '%s': hipcc emitted no producer -> consumer pair of the class (folded away?)" % rule.what)
    return best


_REQ = None


def calibrate():
    """{rule key: wait states required}, from hipcc's own padding of PROBES; cached per process."""
    global _REQ
    if _REQ is not None:
        return _REQ
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "hazard_probes.hip")
        open(src, "w").write(PROBES)
        subprocess.run(["/opt/rocm/bin/hipcc", *kr.FLAGS, "--cuda-device-only", "-S", src, "-o", os.path.join(td, "hazard_probes.s")], cwd=td, check=True,
                       stderr=subprocess.DEVNULL)
        bodies = dict(functions(open(os.path.join(td, "hazard_probes.s")).read()))
    req = {}
    for rule in RULES:
        worst = 0
        for p in rule.probes:
            n, exact = measure(bodies[p], rule)
            if not exact:
                raise RuntimeError("probe %s for '%s': %d states between producer and consumer and none of them an s_nop -- hipcc's "
                                   "requirement cannot be read off this probe" % (p, rule.what, n))
            worst = max(worst, n)
        req[rule.key] = worst
    for k in MUST_BE_NONZERO:
        if req[k] <= 0:
            raise RuntimeError("calibration gave no requirement for rule %s: the check would be switched off" % k)
    _REQ = req
    return req


class Finding:
    def __init__(self, file, symbol, rule, producer, consumer, found, required):
        self.file, self.symbol, self.rule, self.producer, self.consumer, self.found, self.required = file, symbol, rule, producer, consumer, found, required
        self.kernel = symbol

    def __str__(self):
        return "%s: %s: line %d: %s: `%s` (line %d) -> `%s`: %d wait state(s) between, %d required" % (
            self.file, self.kernel, self.consumer.line, self.rule.what, self.producer.text, self.producer.line, self.consumer.text, self.found,
            self.required)


def scan(text, req, file="<asm>", rules=RULES):
    """Findings of one .s text under the requirements `req` ({rule key: states})."""
    out = []
    for sym, body in functions(text):
        for run in _runs(body):
            start, acc = [], 0
            for i in run:
                start.append(acc)
                acc += i.states
            for ic, c in enumerate(run):
                if not c.src:
                    continue
                for rule in rules:
                    need = req.get(rule.key, 0)
                    if need <= 0 or not rule.consumer(c):
                        continue
                    for ip in range(ic - 1, -1, -1):
                        p = run[ip]
                        gap = start[ic] - start[ip] - p.states
                        if gap >= need:
                            break
                        if p.dst and rule.producer(p) and (p.dst & c.src):
                            out.append(Finding(file, sym, rule, p, c, gap, need))
                            break   # (the nearest producer names the finding)
    if out:
        names = kr.demangle([f.symbol for f in out])
        for f, n in zip(out, names):
            f.kernel = n
    return out


def collect(files=None):
    """Findings over csrc/*.hip (or the named files)."""
    req = calibrate()
    out = []
    for src in kr.sources():
        if files is not None and os.path.basename(src) not in files:
            continue
        txt = kr.device_asm(src)
        if txt is not None:
            out += scan(txt, req, os.path.basename(src))
    return out


def coverage(files=None):
    """{rule key: (producers, consumers) of its classes in the library's .s}: what the zero of collect() is a zero over."""
    n = {r.key: [0, 0] for r in RULES}
    for src in kr.sources():
        if files is not None and os.path.basename(src) not in files:
            continue
        for _, body in functions(kr.device_asm(src) or ""):
            for i in body:
                if i is not None:
                    for r in RULES:
                        n[r.key][0] += bool(i.dst and r.producer(i))
                        n[r.key][1] += bool(i.src and r.consumer(i))
    return {k: tuple(v) for k, v in n.items()}


def main():
    req = calibrate()
    cov = coverage()
    print("# wait states hipcc leaves in the probes (= required); producers / consumers of each class in csrc/*.hip")
    for r in RULES:
        print("%-62s %3d  (%d / %d)" % (r.what, req[r.key], *cov[r.key]))
    found = collect()
    for f in found:
        print(f)
    print("%d finding(s)" % len(found))
    return 1 if found else 0


if __name__ == "__main__":
    sys.exit(main())
