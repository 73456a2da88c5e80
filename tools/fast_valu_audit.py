"""Static instruction census of one kernel in a gfx950 assembly listing, per basic block: VALU / SALU / LDS / VMEM counts, barriers and the
loop nest hipcc prints with each block ("in Loop: Header=..."). Used to itemise k_fast_cells' glue:
    hipcc <the Makefile's flags> --cuda-device-only -S orb_fast.hip -o orb_fast.s
    python tools/fast_valu_audit.py orb_fast.s k_fast_cellsILb0
v_readfirstlane / v_readlane / v_writelane count as VALU (SQ_INSTS_VALU counts them); s_waitcnt, s_nop and s_barrier are listed apart."""
import re
import sys


def census(path, kernel):
    blocks, cur, on = [], None, False
    for line in open(path):
        s = line.strip()
        if not on:
            if s.startswith("_ZN") and ":" in s and kernel in s.split(":")[0]:
                on = True
                cur = {"name": "entry", "nest": "", "valu": 0, "salu": 0, "lds": 0, "vmem": 0, "bar": 0, "ops": []}
                blocks.append(cur)
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.(\d+):", s)
        if m:
            nest = ""
            d = re.search(r"Depth[ =](\d+)", s)
            if d:
                nest = "d" + d.group(1)
            cur = {"name": m.group(1) or "bb." + m.group(2), "nest": nest, "valu": 0, "salu": 0, "lds": 0, "vmem": 0, "bar": 0, "ops": []}
            blocks.append(cur)
            continue
        if s.startswith(";") and not s.startswith(";;"):
            d = re.search(r"=>\s*This .*Depth[ =](\d+)", s)
            if d and cur is not None and not cur["ops"]:
                cur["nest"] = "d" + d.group(1) + "*"
            continue
        op = s.split()[0] if s else ""
        if not op or op.startswith(";") or op.startswith("."):
            continue
        cur["ops"].append(op)
        if op == "s_barrier":
            cur["bar"] += 1
        elif op in ("s_waitcnt", "s_nop"):
            pass
        elif op.startswith("v_"):
            cur["valu"] += 1
        elif op.startswith("ds_"):
            cur["lds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            cur["vmem"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
    return blocks


if __name__ == "__main__":
    bl = census(sys.argv[1], sys.argv[2])
    tot = 0
    print("%-12s %-5s %5s %5s %4s %5s %3s  first ops" % ("block", "nest", "VALU", "SALU", "LDS", "VMEM", "bar"))
    for b in bl:
        tot += b["valu"]
        print("%-12s %-5s %5d %5d %4d %5d %3d  %s" % (b["name"], b["nest"], b["valu"], b["salu"], b["lds"], b["vmem"], b["bar"], " ".join(b["ops"][:4])))
    print("static VALU in the kernel: %d" % tot)
