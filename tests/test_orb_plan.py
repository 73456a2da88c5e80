"""The ORB extractor's geometry planner (openvslam_amd/csrc/orb_plan.inc) without a device: tests/orb_plan_host.cc, built by the plain host compiler
from the planner and orb_geometry.h alone, dumps the plan of a geometry; here every section is held to recorded digests (tests/golden/
orb_plan_digests.json: the planner's output when it was moved out of orb_api.hip, byte-equal to the functions it replaced), to the outcomes the
table below names, and to an independent restatement of what the three pyramid kernels assume: taps, the chain's regions, the pair kernel's
regions, the column-pair records. The same program runs clean under AddressSanitizer and UndefinedBehaviorSanitizer.
`python tests/test_orb_plan.py --write-golden` records the digests anew (after a deliberate change of the plan only)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nversion_numpy as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "orb_plan_digests.json")
MAXL = 16

# (rows, cols, levels, scale, keypoints) -> what the planner decides: geometry ok, cells, level-0 root grid, resize_hwin_ok of levels 1..,
# chain (ok, TX, TY, LDS bytes), pair plans of l2 = 2.. ; None = not pinned
CASES = {
    (333, 403, 8, "1.2", 300): dict(cells=87, hwin="1111111", chain=(True, 4, 4, 25008), pairs="111111"),
    (55, 700, 4, "1.2", 300): dict(cells=20, roots=(39, 1), hwin="111", chain=(True, 6, 1, None), pairs="11"),
    (480, 640, 4, "2.0", 300): dict(hwin="000", chain=(True, 5, 5, None), pairs="00"),
    (480, 640, 8, "1.5", 1000): dict(hwin="0000001", chain=(True, None, None, None), pairs="000000"),
    (480, 640, 8, "1.25", 1000): dict(hwin="1111111", chain=(True, None, None, None), pairs="000110"),
    (480, 640, 16, "1.2", 1000): dict(hwin="1" * 15, chain=(False, None, None, 65856), pairs="1" * 14),
    (480, 640, 1, "1.2", 500): dict(hwin="", chain=(False, None, None, None), pairs=""),
    (40, 40, 2, "1.2", 50): dict(cells=0, hwin="1", chain=(True, 1, 1, None), pairs=""),
    (60, 1920, 8, "1.2", 1000): dict(roots=(86, 1), hwin="1111111", chain=(True, 15, 1, None), pairs="111111"),
    (9000, 100, 2, "1.2", 100): None,   # refused: a side above 8191
}

TAP = np.dtype([("o0", "<u2"), ("o1", "<u2"), ("a0", "<i2"), ("a1", "<i2")])
CELL = np.dtype([("min_x", "<u2"), ("min_y", "<u2"), ("cw", "u1"), ("ch", "u1"), ("level", "u1"), ("pad", "u1")])
CHAIN_SPAN = np.dtype([(k, "<i2") for k in ("c0", "c1", "o0", "o1")])
PAIR_SPAN = np.dtype([(k, "<i2") for k in ("s_lo", "b0", "n", "own", "a0", "an", "pad0", "pad1")])
HTAP = np.dtype([(k, "<u4") for k in ("sel_a", "sel_b", "ca", "cb", "wa", "pad0", "pad1", "pad2")])
LEVEL = np.dtype([(k, "<i4") for k in ("rows", "cols", "pitch", "ncx", "ncy", "cell_base", "max_bx", "max_by", "n_keypts", "kp_cap", "kp_base", "cand_cap", "gx",
                                        "gy", "max_nodes")] + [("inv_ncx", "<f4"), ("resize_hwin_ok", "<i4"), ("ncx_magic", "<u4")] +
                 [(k, "<i8") for k in ("plane_off", "cand_off", "node_off", "xtab_off", "ytab_off")] + [("dx", "<f8"), ("dy", "<f8"), ("scale", "<f4"), ("kp_size", "<f4")],
                 align=True)
FRAME = np.dtype([(k, "<i4") for k in ("num_levels", "total_cells", "total_kp_cap", "ini_thr", "min_thr", "variant")] + [("cell_base_tab", "<i4", (MAXL,)), ("lv", LEVEL, (MAXL,))],
                 align=True)
LIMITS = ("kTileW", "kTileH", "kSrcWords", "kSrcRows", "kPairSrcWords", "kPairSrcRows", "kPairGroups", "kChainTileW0", "kChainTileH0", "kChainMaxW", "kChainMaxW0",
          "kChainMaxH0", "kChainMaxLds", "sizeof_FrameGeo", "sizeof_LevelGeo", "OVS_MAX_LEVELS")


def key(case):
    return "%dx%d L%d s%s n%d" % case


def sections(blob):
    out, at = {}, 0
    while at < len(blob):
        name = blob[at:at + 8].rstrip(b"\0").decode()
        n = int.from_bytes(blob[at + 8:at + 16], "little")
        out[name] = blob[at + 16:at + 16 + n]
        at += 16 + n
    assert at == len(blob)
    return out


def digests(secs):
    return {k: hashlib.sha256(v).hexdigest() for k, v in secs.items()}


def run_all(exe, tmp):
    """Every case's sections, and nothing on stderr."""
    got = {}
    for case in CASES:
        path = os.path.join(str(tmp), "plan.bin")
        r = subprocess.run([exe, path] + [str(v) for v in case], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "" and r.stdout == "", (case, r.returncode, r.stderr)
        with open(path, "rb") as f:
            got[case] = sections(f.read())
    return got


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CPP, "orb_plan_host"])
    return run_all(os.path.join(CPP, "orb_plan_host"), tmp_path_factory.mktemp("orb_plan"))


class Plan:
    def __init__(self, secs):
        self.lim = dict(zip(LIMITS, np.frombuffer(secs["limits"], "<i4").tolist()))
        self.geo = np.frombuffer(secs["geo"], FRAME)[0]
        self.L = int(self.geo["num_levels"])
        self.lv = self.geo["lv"][:self.L]
        self.taps = np.frombuffer(secs["taps"], TAP)
        self.cells = np.frombuffer(secs["cells"], CELL)
        head = np.frombuffer(secs["chain"][:32], "<i4").tolist()
        self.chain_ok, self.TX, self.TY, self.bufA, self.bufB, self.tap_cap, self.lds, nspans = head
        self.spans = np.frombuffer(secs["chain"][32:], CHAIN_SPAN)
        assert len(self.spans) == nspans
        self.pair_off = np.frombuffer(secs["pairs"][:4 * MAXL], "<i4").tolist()
        self.pair_spans = np.frombuffer(secs["pairs"][4 * MAXL:], PAIR_SPAN)
        self.htab_off = np.frombuffer(secs["htaps"][:4 * MAXL], "<i4").tolist()
        self.htaps = np.frombuffer(secs["htaps"][4 * MAXL:], HTAP)
        self.totals = np.frombuffer(secs["totals"], "<u8").tolist()
        t = secs["tables"]
        assert int.from_bytes(t[:4], "little") == self.L
        f = np.frombuffer(t[4:4 + 16 * self.L], "<f4").reshape(4, self.L)
        self.sf, self.isf, self.ls, self.ils = f
        self.npl = np.frombuffer(t[4 + 16 * self.L:], "<i4")

    def axis_taps(self, level, axis):
        g = self.lv[level]
        off, n = (int(g["ytab_off"]), int(g["rows"])) if axis else (int(g["xtab_off"]), int(g["cols"]))
        return self.taps[off:off + n]

    def size(self, level, axis):
        return int(self.lv[level]["rows" if axis else "cols"])


def plans(dumps):
    return {case: Plan(secs) for case, secs in dumps.items() if CASES[case] is not None}


# ---- 1. digests
def test_every_section_hashes_to_the_recorded_digest(dumps):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(key(c) for c in CASES)
    for case, secs in dumps.items():
        assert digests(secs) == want[key(case)], key(case)


# ---- 2. outcomes
def test_outcomes_are_the_ones_the_table_names(dumps):
    for case, want in CASES.items():
        secs = dumps[case]
        ok = int.from_bytes(secs["result"], "little", signed=True)
        if want is None:
            assert ok == 0 and sorted(secs) == ["limits", "result"], case
            continue
        assert ok == 1, case
        p = Plan(secs)
        assert len(secs["geo"]) == FRAME.itemsize == p.lim["sizeof_FrameGeo"] and LEVEL.itemsize == p.lim["sizeof_LevelGeo"] and p.lim["OVS_MAX_LEVELS"] == MAXL
        assert p.L == case[2]
        if "cells" in want:
            assert int(p.geo["total_cells"]) == len(p.cells) == want["cells"], case
        if "roots" in want:
            assert (int(p.lv[0]["gx"]), int(p.lv[0]["gy"])) == want["roots"], case
        assert "".join(str(int(g["resize_hwin_ok"])) for g in p.lv[1:]) == want["hwin"], case
        c_ok, tx, ty, lds = want["chain"]
        assert bool(p.chain_ok) == c_ok, case
        if tx is not None:
            assert (p.TX, p.TY) == (tx, ty), case
        if lds is not None:
            assert p.lds == lds, case
        assert "".join("1" if p.pair_off[l2] >= 0 else "0" for l2 in range(2, p.L)) == want["pairs"], case
        assert all(o == -1 for o in p.pair_off[:2] + p.pair_off[max(p.L, 2):])


# ---- 3. the restatement
def reference_taps(src, dst):
    """tests/nversion_numpy's tap positions and its 11-bit rounding; on both axes a tap outside the image collapses onto one pixel (the
    planner's tables do so for rows too: both source rows are then the same, whatever the weights)."""
    s, f = nv._linear_taps(src, dst)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, src - 1), nv._q11(np.float32(1.0) - f), nv._q11(f)


def test_tables_sizes_and_taps(dumps):
    for case, p in plans(dumps).items():
        rows, cols, L, scale, nfeat = case
        sf = np.cumprod(np.array([1.0] + [np.float32(scale)] * (L - 1), np.float32), dtype=np.float32)
        assert p.sf.tolist() == sf.tolist() and p.isf.tolist() == (np.float32(1) / sf).tolist() and p.ls.tolist() == (sf * sf).tolist()
        assert p.ils.tolist() == (np.float32(1) / (sf * sf)).tolist()
        assert int(p.npl.sum()) == nfeat or int(p.npl[-1]) == 0
        assert [int(g["n_keypts"]) for g in p.lv] == p.npl.tolist()
        at = 0
        for l in range(L):
            g = p.lv[l]
            if l == 0:
                assert (int(g["rows"]), int(g["cols"])) == (rows, cols)
                continue
            assert (int(g["rows"]), int(g["cols"])) == (int(np.round(rows / np.float64(sf[l]))), int(np.round(cols / np.float64(sf[l])))), (case, l)
            for axis in (0, 1):
                assert int(g["ytab_off" if axis else "xtab_off"]) == at
                t = p.axis_taps(l, axis)
                at += len(t)
                o0, o1, a0, a1 = reference_taps(p.size(l - 1, axis), p.size(l, axis))
                assert t["o0"].tolist() == o0.tolist() and t["o1"].tolist() == o1.tolist(), (case, l, axis)
                assert t["a0"].tolist() == a0.tolist() and t["a1"].tolist() == a1.tolist(), (case, l, axis)
        assert at == len(p.taps)
        assert sum(int(g["ncx"]) * int(g["ncy"]) for g in p.lv) == len(p.cells) == int(p.geo["total_cells"])
        last = p.lv[L - 1]
        assert p.totals[0] == (int(last["plane_off"]) + int(last["pitch"]) * int(last["rows"]) if L > 1 else 0)
        assert p.totals[1] == sum(int(g["cand_cap"]) for g in p.lv) and p.totals[2] == sum(2 * int(g["max_nodes"]) for g in p.lv)


def footprint(taps, lo, hi):
    """source range [f0, f1) the outputs [lo, hi) read"""
    t = taps[lo:hi]
    return int(t["o0"].min()), int(t["o1"].max()) + 1


def test_chain_regions(dumps):
    for case, p in plans(dumps).items():
        lim = p.lim
        if p.L < 2:
            assert not p.chain_ok and len(p.spans) == 0
            continue
        TX, TY = p.TX, p.TY
        assert TX == max(1, -(-case[1] // lim["kChainTileW0"])) and TY == max(1, -(-case[0] // lim["kChainTileH0"]))
        sp = p.spans.reshape(p.L, TX + TY)
        exceeded = False
        for axis in (0, 1):
            T = TY if axis else TX
            col = sp[:, TX:] if axis else sp[:, :TX]
            for l in range(1, p.L):
                size = p.size(l, axis)
                assert int(col[l, 0]["o0"]) == 0 and int(col[l, T - 1]["o1"]) == size, (case, axis, l)
                assert all(int(col[l, t]["o1"]) == int(col[l, t + 1]["o0"]) for t in range(T - 1)), (case, axis, l)   # a partition of [0, size)
            for t in range(T):
                for l in range(p.L):
                    c0, c1, o0, o1 = (int(col[l, t][k]) for k in ("c0", "c1", "o0", "o1"))
                    assert 0 <= c0 <= c1 <= p.size(l, axis) and o0 <= o1
                    if l >= 1 and o1 > o0:
                        assert c0 <= o0 and o1 <= c1, (case, axis, t, l)
                    if l == 0:
                        assert o0 == o1 == 0 and (axis or c0 % 4 == 0)
                    if l + 1 < p.L and int(col[l + 1, t]["c1"]) > int(col[l + 1, t]["c0"]):   # what the region one level up reads
                        f0, f1 = footprint(p.axis_taps(l + 1, axis), int(col[l + 1, t]["c0"]), int(col[l + 1, t]["c1"]))
                        assert c0 <= f0 and f1 <= c1, (case, axis, t, l)
                    ext = c1 - c0
                    if l == 0:
                        exceeded |= ext > (lim["kChainMaxH0"] if axis else lim["kChainMaxW0"])
                    elif not axis:
                        exceeded |= ext > lim["kChainMaxW"]
        # the LDS of the tile that needs most: even levels in one buffer, odd ones in the other, 16-byte granules; every tap of a tile
        bufs, tap_cap = [16, 16], 0
        for tj in range(TY):
            for ti in range(TX):
                ntap = 0
                for l in range(p.L):
                    W = int(sp[l, ti]["c1"]) - int(sp[l, ti]["c0"])
                    H = int(sp[l, TX + tj]["c1"]) - int(sp[l, TX + tj]["c0"])
                    bufs[l & 1] = max(bufs[l & 1], (-(-W // 4) * 4 * H + 15) // 16 * 16)
                    ntap += W + H if l else 0
                tap_cap = max(tap_cap, ntap)
        assert (p.bufA, p.bufB, p.tap_cap) == (bufs[0], bufs[1], tap_cap), case
        lds = bufs[0] + bufs[1] + CHAIN_SPAN.itemsize * 2 * MAXL + 16 * MAXL + TAP.itemsize * tap_cap
        assert p.lds == lds
        assert bool(p.chain_ok) == (not exceeded and lds <= lim["kChainMaxLds"]), (case, exceeded, lds)


def test_pair_regions(dumps):
    seen = 0
    for case, p in plans(dumps).items():
        lim = p.lim
        at = 0
        for l2 in range(2, p.L):
            if p.pair_off[l2] < 0:
                continue
            assert p.pair_off[l2] == at and int(p.lv[l2 - 1]["resize_hwin_ok"]) and int(p.lv[l2]["resize_hwin_ok"]), (case, l2)
            for axis in (0, 1):
                size1, size2 = p.size(l2 - 1, axis), p.size(l2, axis)
                step, unit = (lim["kTileH"], 1) if axis else (lim["kTileW"], 4)
                t1, t2 = p.axis_taps(l2 - 1, axis), p.axis_taps(l2, axis)
                nt = -(-size2 // step)
                spans = p.pair_spans[at:at + nt]
                at += nt
                nxt = 0
                for i, s in enumerate(spans):
                    s_lo, b0, n, own, a0, an = (int(s[k]) for k in ("s_lo", "b0", "n", "own", "a0", "an"))
                    assert b0 == nxt and 1 <= own <= n and int(s["pad0"]) == int(s["pad1"]) == 0, (case, l2, axis, i)   # owned ranges follow each other from 0
                    nxt = b0 + unit * own
                    if axis:
                        assert s_lo == b0 and n <= lim["kSrcRows"] and an <= lim["kPairSrcRows"]
                    else:
                        assert s_lo % 16 == 0 and b0 % 4 == 0 and a0 % 16 == 0 and s_lo <= b0
                        assert n <= lim["kPairGroups"] and (b0 - s_lo) // 4 + n <= lim["kSrcWords"] and an <= lim["kPairSrcWords"]
                    mid_end = min(b0 + unit * n, size1)
                    f0, f1 = footprint(t2, i * step, min((i + 1) * step, size2))   # the upper tile reads the middle region
                    assert b0 <= f0 and f1 <= mid_end, (case, l2, axis, i)
                    f0, f1 = footprint(t1, b0, mid_end)                              # the whole middle region reads the lower range
                    assert a0 <= f0 and f1 <= a0 + unit * an, (case, l2, axis, i)
                    seen += 1
                assert size1 <= nxt < size1 + unit, (case, l2, axis)   # ... and end where the middle level ends (x: in whole 4-pixel groups)
        assert at == len(p.pair_spans)
    assert seen > 100


def test_column_pair_records(dumps):
    seen = 0
    for case, p in plans(dumps).items():
        at = 0
        for l in range(MAXL):
            read = l >= 1 and l < p.L and (p.pair_off[l] >= 0 or (l + 1 < p.L and p.pair_off[l + 1] >= 0))
            assert (p.htab_off[l] >= 0) == read, (case, l)
            if not read:
                continue
            assert p.htab_off[l] == at
            t = p.axis_taps(l, 0)
            cols = len(t)
            n = (cols + 1) // 2
            r = p.htaps[at:at + n]
            at += n
            xa = np.arange(0, cols, 2)
            xb = np.minimum(xa + 1, cols - 1)
            base = 4 * r["wa"].astype(np.int64)
            assert (r["wa"] == t["o0"][xa] >> 2).all() and not r["pad0"].any() and not r["pad1"].any() and not r["pad2"].any()
            for sel, x in (("sel_a", xa), ("sel_b", xb)):
                s = r[sel].astype(np.int64)
                # each half selects byte k = 0 .. 7 of the two aligned words at wa by its low three bits; the byte above it is the constant zero
                assert (s & 0xFFF8FFF8 == 0x0C000C00).all(), (case, l, sel)
                assert (base + (s & 7) == t["o0"][x]).all() and (base + ((s >> 16) & 7) == t["o1"][x]).all(), (case, l, sel)
            for c, x in (("ca", xa), ("cb", xb)):
                v = r[c].astype(np.int64)
                assert (((v >> 4) & 0xFFFF) == t["a0"][x]).all() and ((v >> 20) == t["a1"][x]).all() and not (v & 0xF).any(), (case, l, c)
            seen += n
        assert at == len(p.htaps)
    assert seen > 1000


# ---- 5. the sanitizers (4, the single definition of the limits, is a static_assert of the program: it compiled)
def test_host_program_runs_clean_under_the_sanitizers(dumps, tmp_path):
    exe = str(tmp_path / "orb_plan_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I",   # (the runtimes inside the program: it stands alone)
                           os.path.join(ROOT, "openvslam_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "orb_plan_host.cc")])
    got = run_all(exe, tmp_path)
    assert {c: digests(s) for c, s in got.items()} == {c: digests(s) for c, s in dumps.items()}


if __name__ == "__main__" and sys.argv[1:] == ["--write-golden"]:
    import tempfile
    subprocess.check_call(["make", "-s", "-C", CPP, "orb_plan_host"])
    with tempfile.TemporaryDirectory() as tmp:
        got = run_all(os.path.join(CPP, "orb_plan_host"), tmp)
    with open(GOLDEN, "w") as f:
        json.dump({key(c): digests(s) for c, s in got.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
