"""CPU check of the shipped device code: wait-state hazards at the edges of inline assembly, and scratch use.

hipcc pads the hazards of the instructions it generates itself, but an `asm` statement is one opaque instruction to it: nothing is inserted
inside the string, and a hazard whose producer or consumer lies inside it goes unseen (profiles/r05_experiments.txt, section 2: a v_mbcnt_lo
that read vcc right behind the compare that wrote it).  Such a hazard gives right answers until it does not, so it cannot be looked for on the
GPU.  This test compiles kernels.hip and table_dev.hip to device listings with the product's flags and walks every instruction pair that
involves an asm block, following both sides of each branch (the asm loops' local labels `1b` / `2f` included).
"""
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from arpeggia_amd.build import CSRC, FLAGS, hipcc

VCC, EXEC = {("s", 106), ("s", 107)}, {("s", 126), ("s", 127)}
_NAMED = {"vcc": VCC, "vcc_lo": {("s", 106)}, "vcc_hi": {("s", 107)}, "exec": EXEC, "exec_lo": {("s", 126)}, "exec_hi": {("s", 127)}}
_REG = re.compile(r"\b([sv])(?:(\d+)|\[(\d+):(\d+)\])|\b(vcc(?:_lo|_hi)?|exec(?:_lo|_hi)?)\b")
_CARRY_OUT = re.compile(r"v_(add|sub|subrev|addc|subb|subbrev)_co_|v_div_scale_|v_mad_[iu]64_")
_CARRY_IN = re.compile(r"v_(cndmask|addc_co|subb_co|subbrev_co)_")  # (their last operand is a mask / carry-in, not a constant)
_VMEM = ("global_", "buffer_", "flat_", "scratch_")
_WIDE_STORE = re.compile(r"(global|buffer|flat|scratch)_store_dwordx[34]$")
_LOADS = re.compile(r"_load|^ds_read|_rtn_|^ds_(bpermute|permute|swizzle)")
_ENDS = ("s_endpgm", "s_setpc_b64", "s_swappc_b64", "s_trap")
MAX_WAIT = 5  # the largest minimum below


def regs(text):
    out = set()
    for kind, n, lo, hi, named in _REG.findall(text):
        if named:
            out |= _NAMED[named]
        else:
            out |= {(kind, k) for k in (range(int(n), int(n) + 1) if n else range(int(lo), int(hi) + 1))}
    return out


class Inst:
    def __init__(self, text, asm, line):
        self.text, self.asm, self.line = text, asm, line
        self.op, _, rest = text.partition(" ")
        self.ops = [o.split()[0] for o in rest.split(",") if o.strip()]
        op, ops = self.op, self.ops
        self.valu = op.startswith("v_")
        n_dst = 0 if not self.valu or not ops else (2 if _CARRY_OUT.match(op) else 1)
        dst = regs(" ".join(ops[:n_dst]))
        self.s_written = {r for r in dst if r[0] == "s"} | (EXEC if op.startswith("v_cmpx") else set())
        self.v_written = {r for r in dst if r[0] == "v"}
        if (_LOADS.search(op) or (op.startswith(_VMEM) and "_atomic" in op and re.search(r"\b(sc0|glc)\b", text))) and not re.search(r"\blds\b|_lds_", text):
            self.v_written |= {r for r in regs(ops[0]) if r[0] == "v"}
        srcs = ops[n_dst:-1] if _CARRY_IN.match(op) else ops[n_dst:]
        self.vcc_const = self.valu and any(re.search(r"\bvcc(_lo|_hi)?\b", o) for o in srcs)
        self.vmem_s = {r for r in regs(" ".join(ops)) if r[0] == "s"} if op.startswith(_VMEM) else set()
        self.lane_sel = regs(ops[-1]) if op.startswith(("v_readlane", "v_writelane")) else set()
        self.lane_read = {r for r in regs(ops[1]) if r[0] == "v"} if op.startswith(("v_readlane", "v_readfirstlane")) else set()
        self.dpp = self.valu and ("_dpp" in op or "row_mask:" in text or "dpp8:" in text)
        self.store_data = regs(ops[0 if op.startswith("buffer_") else 1]) if _WIDE_STORE.match(op) else set()
        self.waits = int(ops[0], 0) + 1 if op == "s_nop" else 1


# (name, minimum wait states, producer -> registers it hands on, consumer -> registers it takes)
RULES = [
    ("VALU writes vcc -> VALU reads it as a constant", 1, lambda p: p.s_written & VCC if p.valu else set(), lambda c: VCC if c.vcc_const else set()),
    ("VALU writes SGPR -> VMEM reads it", 5, lambda p: p.s_written if p.valu else set(), lambda c: c.vmem_s),
    ("VALU writes SGPR/vcc -> v_readlane/v_writelane lane select", 4, lambda p: p.s_written if p.valu else set(), lambda c: c.lane_sel),
    ("VALU writes exec -> DPP", 5, lambda p: p.s_written & EXEC if p.valu else set(), lambda c: EXEC if c.dpp else set()),
    ("VALU writes VGPR -> v_readfirstlane/v_readlane reads it", 1, lambda p: p.v_written if p.valu else set(), lambda c: c.lane_read),
    ("asm store_dwordx3/x4 -> write of its data VGPRs", 2, lambda p: p.store_data if p.asm else set(), lambda c: c.v_written),
]


def functions(listing):
    """{symbol: [Inst | ('label', name)]} for every function of a device listing, with the asm blocks marked."""
    names = set(re.findall(r"^\s*\.type\s+([^,\s]+),@function", listing, re.M))
    funcs, body, asm = {}, None, False
    for no, raw in enumerate(listing.splitlines(), 1):
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            asm = True
        elif s.startswith(";;#ASMEND"):
            asm = False
        s = s.split(";")[0].strip()
        m = re.match(r"^([\w.$]+):(.*)$", s)
        if m and m.group(1) in names:
            body = funcs[m.group(1)] = []
            continue
        if body is None or not s:
            continue
        if m and m.group(1).startswith(".Lfunc_end"):
            body = None
            continue
        if m:
            body.append(("label", m.group(1)))
            s = m.group(2).strip()
        if s and not s.startswith("."):
            body.append(Inst(s, asm, no))
    return funcs


def successors(body):
    """[[index of each instruction's possible next instruction]]; `1b` / `2f` are the nearest label 1 before / label 2 after."""
    labels = {item[1]: k for k, item in enumerate(body) if not isinstance(item, Inst)}
    out = []
    for i, inst in enumerate(body):
        if not isinstance(inst, Inst) or not inst.op.startswith(("s_branch", "s_cbranch_") + _ENDS):
            out.append([i + 1])
            continue
        if inst.op.startswith(_ENDS):
            out.append([])
            continue
        target = inst.ops[0]
        m = re.fullmatch(r"(\d+)([bf])", target)
        if m:
            span = range(i, -1, -1) if m.group(2) == "b" else range(i, len(body))
            k = next(k for k in span if body[k] == ("label", m.group(1)))
        else:
            k = labels[target]
        out.append([k] if inst.op == "s_branch" else [i + 1, k])
    return out


def scan_function(body):
    """[(rule, minimum, wait states, producer, consumer)]: one per consumer and rule, its nearest producer."""
    found, succ = {}, successors(body)
    for p, prod in enumerate(body):
        if not isinstance(prod, Inst):
            continue
        handed = [(rule, need, rs, take) for rule, need, produce, take in RULES if (rs := produce(prod))]
        if not handed:
            continue
        todo, seen = [(k, 0) for k in succ[p]], set()
        while todo:
            k, waited = todo.pop()
            if k >= len(body) or (k, waited) in seen:
                continue
            seen.add((k, waited))
            cons = body[k]
            if not isinstance(cons, Inst):
                todo.append((k + 1, waited))
                continue
            for rule, need, rs, take in handed:
                if waited < need and (prod.asm or cons.asm) and rs & take(cons):
                    key = (rule, cons.line)
                    if key not in found or found[key][2] > waited:
                        found[key] = (rule, need, waited, prod, cons)
            if waited + cons.waits < MAX_WAIT:
                todo += [(n, waited + cons.waits) for n in succ[k]]
    return sorted(found.values(), key=lambda f: f[4].line)


def scan(listing):
    return {name: hits for name, body in functions(listing).items() if (hits := scan_function(body))}


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"^void |\(.*$", "", d) for n, d in zip(names, out)}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    try:
        cc = hipcc()
    except RuntimeError:
        pytest.skip("no hipcc: the device code cannot be compiled")
    out = tmp_path_factory.mktemp("isa")

    def compile_one(src):
        dst = out / (src + ".s")
        subprocess.run([cc, *FLAGS, "-S", "--cuda-device-only", str(CSRC / src), "-o", str(dst)], check=True, capture_output=True)
        return src, dst.read_text()

    with ThreadPoolExecutor(2) as pool:
        return dict(pool.map(compile_one, ["kernels.hip", "table_dev.hip"]))


def test_no_wait_state_hazard_at_inline_asm(listings):
    report = []
    for src, text in listings.items():
        hits = scan(text)
        names = demangle(sorted(hits))
        for name, found in hits.items():
            for rule, need, waited, prod, cons in found:
                report.append(f"{src}: {names[name]}: {rule} needs {need} wait state(s), has {waited}:\n"
                              f"    {prod.line}: {prod.text}\n    {cons.line}: {cons.text}")
    assert not report, f"{len(report)} hazard(s):\n" + "\n".join(report)


# No kernel of the project uses scratch (private segment).  The RES + STAGE variants k_emit<12, 4, {true,false}, false, true, true> kept 12 bytes
# of spilled registers there (VERDICT.md, weak point 7) until their record stores took the wave's region base in scalar registers.  (The rocprim
# sort kernels table_dev.hip instantiates are the library's own and not checked.)
def test_no_kernel_uses_scratch(listings):
    sizes = {}
    for text in listings.values():
        for name, size in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", text, re.M):
            sizes[name] = int(size)
    ours = {n: size for n, size in sizes.items() if n.startswith("_ZN3arp")}
    assert len(ours) > 40
    spilling = sorted(n for n, size in ours.items() if size)
    assert not spilling, demangle(spilling)


# ---- the scanner on hand-written listings: it flags both of round 5's patterns and passes their padded / reordered forms ----

def listing(*lines):
    return "\n".join(["\t.type\tf,@function", "f:"] + [f"\t{s}" for s in lines] + [".Lfunc_end0:"]) + "\n"


def rules_hit(*lines):
    return [f[0] for f in scan(listing(*lines)).get("f", [])]


COMPACT = ["v_cmp_ne_u32 vcc, 0, v168", "v_mbcnt_lo_u32_b32 v0, vcc_lo, 0", "v_mbcnt_hi_u32_b32 v0, vcc_hi, v0", "v_ffbh_u32 v1, v168"]
STORE = ["v_readfirstlane_b32 s1, v25", "v_readfirstlane_b32 s0, v24", ";;#ASMSTART", "s_and_saveexec_b64 s[60:61], s[80:81]",
         "global_store_dwordx4 v6, v[2:5], s[0:1]", "s_mov_b64 exec, s[60:61]", ";;#ASMEND", "v_add_u32_e32 v35, s41, v35"]


def test_scanner_flags_vcc_read_right_behind_its_compare():
    assert rules_hit(";;#ASMSTART", *COMPACT, ";;#ASMEND") == [RULES[0][0]]
    # the fix: v_ffbh_u32 moved up between the compare and v_mbcnt_lo
    assert rules_hit(";;#ASMSTART", COMPACT[0], COMPACT[3], *COMPACT[1:3], ";;#ASMEND") == []
    # the carry-in / select operand is not a constant read; compiler code on both sides is hipcc's own business
    assert rules_hit(";;#ASMSTART", "v_cmp_le_f32 vcc, v1, v2", "v_addc_co_u32 v0, vcc, v0, v0, vcc", ";;#ASMEND") == []
    assert rules_hit(*COMPACT) == []


def test_scanner_flags_readfirstlane_base_of_asm_store():
    assert rules_hit(*STORE) == [RULES[1][0]]
    hits = scan(listing(*STORE))["f"]
    assert [(f[2], f[3].text, f[4].text) for f in hits] == [(1, STORE[1], STORE[4])]
    # a base made scalar long before: five other instructions, or s_nop 4 opening the string
    assert rules_hit(*STORE[:2], *["v_add_u32_e32 v7, v7, v7"] * 4, *STORE[2:]) == []
    assert rules_hit(*STORE[:3], "s_nop 4", *STORE[3:]) == []
    assert rules_hit(*STORE[:3], "s_nop 2", *STORE[3:]) == [RULES[1][0]]


def test_scanner_follows_both_sides_of_branches_and_asm_labels():
    # the hazard sits on the loop's back edge only: 1b leads from the readfirstlane to the load with one wait state (the branch's) between them
    loop = [";;#ASMSTART", "1:", "global_load_dword v3, v4, s[2:3]", "s_nop 4", "v_readfirstlane_b32 s2, v1", "s_cbranch_scc1 1b", ";;#ASMEND"]
    assert rules_hit(*loop) == [RULES[1][0]]
    assert rules_hit(*loop[:5], "s_nop 3", *loop[5:]) == []
    # the taken side of a forward branch: 2f skips the padding that the fall-through has
    fwd = [";;#ASMSTART", "v_readfirstlane_b32 s2, v1", "s_cbranch_scc1 2f", "s_nop 4", "2:", "global_load_dword v3, v4, s[2:3]", ";;#ASMEND"]
    assert rules_hit(*fwd) == [RULES[1][0]]
    assert rules_hit(*fwd[:2], "s_nop 4", *fwd[2:]) == []
    # a compiler branch out of the producer's block
    assert rules_hit("v_readfirstlane_b32 s0, v1", "s_branch .LBB0_2", "s_nop 7", ".LBB0_2:", ";;#ASMSTART", "buffer_load_dword v2, v3, s[0:3], 0 offen",
                     ";;#ASMEND") == [RULES[1][0]]


def test_scanner_knows_the_other_rules():
    asm = lambda *l: [";;#ASMSTART", *l, ";;#ASMEND"]
    assert rules_hit(*asm("v_cmp_lt_u32_e64 s[4:5], v1, v2", "s_nop 2", "v_readlane_b32 s6, v3, s4")) == [RULES[2][0]]
    assert rules_hit(*asm("v_cmp_lt_u32_e64 s[4:5], v1, v2", "s_nop 3", "v_readlane_b32 s6, v3, s4")) == []
    assert rules_hit(*asm("v_cmpx_ne_u32_e32 vcc, 0, v1", "s_nop 3", "v_mov_b32_dpp v2, v3 row_shr:1 row_mask:0xf bank_mask:0xf")) == [RULES[3][0]]
    assert rules_hit(*asm("v_add_u32_e32 v1, v2, v3", "v_readfirstlane_b32 s0, v1")) == [RULES[4][0]]
    assert rules_hit(*asm("v_add_u32_e32 v1, v2, v3", "s_nop 0", "v_readfirstlane_b32 s0, v1")) == []
    assert rules_hit(*asm("global_store_dwordx4 v6, v[2:5], s[0:1] nt"), "v_mov_b32_e32 v3, 0") == [RULES[5][0]]
    assert rules_hit(*asm("global_store_dwordx4 v6, v[2:5], s[0:1] nt", "s_nop 1"), "v_mov_b32_e32 v3, 0") == []
    assert rules_hit(*asm("global_store_dwordx4 v6, v[2:5], s[0:1] nt"), "v_mov_b32_e32 v9, 0") == []
