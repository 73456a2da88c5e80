#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on config 2: 1920x1080 mono, 8 pyramid levels, 2000 ORB features, extract + all-pairs
Hamming match (match::robust::brute_force_match, thr 50 / ratio 0.9), device-resident, on N MI355X of one node.

A "step" = one pass of the hot path over one batch of synthetic input per GPU: ORB-extract B frames already resident in HBM,
then match every frame against its predecessor (B problems of ~2000 x ~2000 descriptors), all on one stream.
value = ORB keypoints+descriptors produced per second, whole job (all ranks), with matches/s and Hamming distances/s next to
it. Frames shard across ranks with no data-path collective (replicas) => "scaling": "weak".

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
       N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times K steps and prints the headline line (value, ms_per_step, the rates and the per-stage event
times of the timed steps). --full adds the side measurements and checks: each-kernel-alone and popcount-form passes, the
rooflines (with rocprofv3 child runs), local BA, the other BASELINE configs, the class-boundary latency, the CPU oracle's
baseline and the parity check of the last timed step. --dump-outputs DIR writes what the last timed step computed (rank 0's
frames) as float .npy files, see dump_outputs().
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ROWS, COLS, NFEAT, LEVELS = 1080, 1920, 2000, 8
LOWE_RATIO = 0.9
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (/opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec, 6.29 TB/s measured copy)



PMC_STAGE_SOURCES = {"fast": ("orb_fast.hip",), "pyramid": ("orb_pyramid.hip",), "tree": ("orb_tree.hip",),
                     "describe": ("orb_describe.hip", "orb_pattern.inc"), "match_near": ("match_hamming.hip",),
                     "match_resolve": ("match_hamming.hip",)}


def pmc_stage_fingerprint(src_dir, stage, read=None):
    """sha256[:16] of the sources a stage's kernels are compiled from: its .hip file(s) and the shared headers of csrc/."""
    import hashlib
    read = read or (lambda fn: open(os.path.join(src_dir, fn), "rb").read())
    hsh = hashlib.sha256()
    for fn in sorted(set(PMC_STAGE_SOURCES[stage]) | {f for f in os.listdir(src_dir) if f.endswith(".h")}):
        hsh.update(fn.encode() + b"\0" + read(fn))
    return hsh.hexdigest()[:16]

class collector_paused:
    """The interpreter's cyclic collector is run once and then held off over a wall-clock timed region: a full collection in a process that
    has torch imported takes 35-40 ms on this box, and where it lands depends only on the allocation count -- from round 5's first bench
    line on it landed in the first of the 20 timed linearisations and local_ba.ms_per_linearisation read 1.8 ms instead of 0.06
    (profiles/r05ae_lba_probe.txt). What timeit does for the same reason. The GPU work inside the regions is untouched."""

    def __enter__(self):
        import gc
        gc.collect()
        self._was = gc.isenabled()
        gc.disable()

    def __exit__(self, *exc):
        import gc
        if self._was:
            gc.enable()
        return False


def synth_video_threaded(rows, cols, n_frames, seed=0, frames_per_scene=8, step=(3, 2), threads=16):
    """synth.synth_video's frames, byte for byte, generated one scene per task on a thread pool (numpy releases the interpreter lock in
    the noise and the arithmetic): the two 256-frame 1080p input batches take ~40 s on one core, which a plain run cannot afford."""
    from concurrent.futures import ThreadPoolExecutor
    from openvslam_amd.synth import frame_from_scene, synth_scene
    out = np.empty((n_frames, rows, cols), np.uint8)

    def scene(first):
        sc = synth_scene(rows, cols, seed * 1000 + first // frames_per_scene)
        for i in range(first, min(first + frames_per_scene, n_frames)):
            k = i - first
            out[i] = frame_from_scene(sc, rows, cols, (step[0] * k, step[1] * k), noise_seed=seed * 100003 + i)

    with ThreadPoolExecutor(max(1, min(threads, os.cpu_count() or 1))) as pool:
        list(pool.map(scene, range(0, n_frames, frames_per_scene)))
    return out


def dump_outputs(path, last_out, Bc, budget_bytes=64 << 20):
    """--dump-outputs: what the last timed step handed its caller (extract_batch_dev + brute_force_match_batch_dev), rank 0's frames
    in frame order, the valid rows of each frame only (rows behind a frame's count are stale bytes of earlier steps):
      frame_index.npy      (F,) float64     which frames of the step are in the files
      keypoint_counts.npy  (F,) float64     keypoints per frame
      keypoints.npy        (n, 7) float32   x, y, size, angle, response, octave, class_id (the 28-byte records; the two ints exact)
      descriptors.npy      (n, 8) float64   the 256-bit descriptor as eight little-endian 32-bit words (exact)
      match_counts.npy     (F,) float64     matches of frame b against its predecessor in the scene
      match_pairs.npy      (m, 2) float32   (idx_1 in the predecessor, idx_2 in frame b) index pairs, exact below 2^24
    When all frames could exceed budget_bytes at the keypoint capacity, a fixed seeded sample of frames is written (the choice does not
    depend on the outputs, so two builds dump the same frames)."""
    cap = last_out[0]["cap"]
    n_frames = Bc * len(last_out)
    per_frame = cap * (7 * 4 + 8 * 8 + 2 * 4) + 3 * 8
    keep = min(n_frames, max(1, budget_bytes // per_frame))
    frames = np.arange(n_frames) if keep == n_frames else np.sort(np.random.default_rng(20240).choice(n_frames, keep, replace=False))
    kps, desc, kcnt, pairs, mcnt = [], [], [], [], []
    for g in frames:
        lo = last_out[g // Bc]
        b = g % Bc
        n, m = int(lo["cnt"][b]), int(lo["mcnt"][b])
        rec = np.ascontiguousarray(lo["kps"][b, :n]).reshape(n, 28)
        kps.append(np.concatenate([rec.view("<f4")[:, :5], rec.view("<i4")[:, 5:7].astype(np.float32)], 1))
        desc.append(np.ascontiguousarray(lo["desc"][b, :n]).view("<u4").astype(np.float64))
        pairs.append(lo["pairs"][b, :m].astype(np.float32))
        kcnt.append(n)
        mcnt.append(m)
    os.makedirs(path, exist_ok=True)
    arrays = {"frame_index": frames.astype(np.float64), "keypoint_counts": np.array(kcnt, np.float64),
              "keypoints": np.concatenate(kps).reshape(-1, 7), "descriptors": np.concatenate(desc).reshape(-1, 8),
              "match_counts": np.array(mcnt, np.float64), "match_pairs": np.concatenate(pairs).reshape(-1, 2)}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return arrays


def level_sizes(rows, cols, scale=1.2, levels=8):
    sf = np.float32(1.0)
    out = [(rows, cols)]
    for _ in range(1, levels):
        sf = np.float32(scale) * sf
        out.append((int(np.floor(rows / float(sf) + 0.5)), int(np.floor(cols / float(sf) + 0.5))))
    return out


def algorithmic_bytes(rows, cols, n_kp_frame, n_cand_frame):
    """ALGORITHMIC bytes per frame for each extract kernel (SURVEY.md 8(d) minimum-pass model, split per kernel)."""
    lv = level_sizes(rows, cols)
    px = [r * c for r, c in lv]
    return {
        "pyramid": sum(px[:-1]) + sum(px[1:]),          # each level read once as a source, levels 1..7 written once
        "fast": sum(px),                                # every level read once for FAST/NMS (6 419 321 B at 1080p)
        "tree": 8 * n_cand_frame + 8 * n_kp_frame,      # candidate list read once, selected keypoints written
        "describe": n_kp_frame * (43 * 43 + 32 + 28),   # 43x43 patch per keypoint in, descriptor + cv::KeyPoint out
    }


def live_pmc_traffic(stage_kernel_prefix, batch=128, timeout_s=150):
    """HBM-side bytes and VALU wave-instructions per launch of the kernels whose name starts with `stage_kernel_prefix`, measured NOW: three
    rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE, SQ_INSTS_VALU; each counter in its own run, with --kernel-trace only) over a short child run of this script (2 steps + 1 warm-up, `batch` frames per
    launch, one stream, one FAST launch per step). Units and the gfx950 correction as tools/pmc_summary.py: both counters in KiB, FETCH_SIZE reports half
    the bytes of a coalesced read stream (profiles/r01_hbm_calib.txt). Returns ({"bytes", "insts_valu", "batch"} per launch at `batch` frames, note) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not exe:
        return None, "rocprofv3 not found"
    child = [sys.executable, os.path.abspath(__file__), "--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-ba", "--overlap", "0",
             "--batch", str(batch), "--fast-split", "0", "--live-pmc", "0"]
    means = {}
    with tempfile.TemporaryDirectory(prefix="ovs_pmc_", dir="/tmp") as td:
        env = dict(os.environ, TMPDIR="/tmp")
        for counter in ("FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU"):
            out = os.path.join(td, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "-o", "p", "--"] + child
            try:
                pr = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            except Exception as ex:   # timeout, OSError
                return None, "rocprofv3 --pmc %s: %r" % (counter, ex)
            vals = []
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        name = row.get("Kernel_Name", "").replace("void ", "")
                        if name.startswith(stage_kernel_prefix) and row.get("Counter_Name") == counter:
                            vals.append(float(row["Counter_Value"]))
            if not vals:
                return None, "rocprofv3 --pmc %s: no %s dispatches in the output (rc %d)" % (counter, stage_kernel_prefix, pr.returncode)
            means[counter] = sum(vals) / len(vals)
    return {"bytes": int((2.0 * means["FETCH_SIZE"] + means["WRITE_SIZE"]) * 1024.0), "insts_valu": int(means["SQ_INSTS_VALU"]), "batch": batch}, \
        "%d frames per launch" % batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="frames per step per GPU (a multiple of 8: frames come in 8-frame scenes)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget-s", type=float, default=12.0, help="wall-time budget of the CPU-oracle sample (cpu_baseline + parity); at least 8 frames run")
    ap.add_argument("--no-ba", action="store_true", help="skip the local-BA side section (profiling runs)")
    ap.add_argument("--pipeline", type=int, default=1, help="sub-batches of the extract issued on overlapping internal streams (1 = off)")
    ap.add_argument("--chains", type=int, default=1, help="independent extract->match pipelines the batch is split over (own handles and "
                                                          "streams, no cross-chain synchronisation)")
    ap.add_argument("--fast-split", type=int, default=1, help="1: FAST on level 0 (+ its quad-tree) runs on an internal stream beside the pyramid; "
                                                                "0: one FAST launch over all levels after the pyramid (profiling runs)")
    ap.add_argument("--match-first", type=int, default=0, help="1: the matcher's stream gets the high-priority queue instead of the extraction's (A/B)")
    ap.add_argument("--overlap", type=int, default=1, help="1: matching of step k runs on a second stream under the extraction of step "
                                                            "k+1 (double-buffered outputs); 0: one stream, strictly serial")
    ap.add_argument("--live-pmc", type=int, default=1, help="1: roofline.traffic from rocprofv3 --pmc passes THIS run spawns (two short child runs of this "
                                                             "script under the profiler, FETCH_SIZE and WRITE_SIZE separately); falls back to the committed "
                                                             "profiles/pmc_traffic.json when rocprofv3 is missing, fails or times out; 0: the committed file only")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run every side measurement and check (rooflines, "
                                                        "popcount form, local BA, other configs, class latency, CPU baseline + parity); "
                                                        "--no-cpu-baseline, --cpu-budget-s, --no-ba and --live-pmc act on these only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs (rank 0) to DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU fallback for the product path)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched as plain `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run, rendezvous on
        # 127.0.0.1 (the container hostname may not resolve); rank 0's JSON line passes through on stdout, the exit code is the job's
        have = torch.cuda.device_count()
        if have < args.gpus and os.environ.get("OVS_BENCH_ONE_DEVICE") != "1":
            raise SystemExit("bench.py --gpus %d needs %d HIP devices on this node, found %d" % (args.gpus, args.gpus, have))
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE=%d (torch.distributed.run --nproc-per-node must equal --gpus)" % (args.gpus, world))
    # Test hook (tests/test_bench_cli.py): OVS_BENCH_ONE_DEVICE=1 puts every rank on device 0 and uses gloo for the process group (RCCL refuses
    # two ranks on one device), so that the multi-rank code path -- sharding, barriers, max-over-ranks clock, the sums over ranks, the
    # sharded local-BA exchange, rank 0's single JSON line -- runs on a one-GPU box. Its numbers mean nothing; the line says so.
    one_device = os.environ.get("OVS_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit("rank %d: LOCAL_RANK %d but only %d HIP devices on this node" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_device:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from openvslam_amd import _lib, feature, match

    B = args.batch
    L = _lib.lib()
    # ---- synthetic input, resident in HBM before the timed region (each rank gets its own frames)
    # TWO distinct batches, alternated step by step: 2 x 265 MB of input cannot sit in the 256 MiB Infinity Cache, so level-0 reads
    # of the timed region come from HBM (bench hygiene)
    # (the ranks of a node share its 16 host threads)
    frames = synth_video_threaded(ROWS, COLS, B, seed=100 + rank, threads=max(1, 16 // world))
    d_frames = torch.from_numpy(frames).cuda()
    frames_alt = synth_video_threaded(ROWS, COLS, B, seed=900 + rank, threads=max(1, 16 // world))
    d_frames_alt = torch.from_numpy(frames_alt).cuda()
    n_chain = max(1, args.chains)
    if B % (8 * n_chain):
        raise SystemExit("--batch must be a multiple of 8 * --chains")
    Bc = B // n_chain

    class Chain:
        """One extract -> match pipeline over Bc frames: its own extractor / matcher handles, output buffers and streams. Chains share
        nothing, so the GPU always has kernels of several chains to pick from and the latency-bound ones (quad-tree, resolver) run under
        another chain's FAST or pyramid; inside a chain the matching of step k runs under the extraction of step k+1."""

        def __init__(self, lo):
            self.frames = [d_frames[lo:lo + Bc], d_frames_alt[lo:lo + Bc]]
            self.ex = feature.orb_extractor(feature.orb_params(NFEAT, 1.2, LEVELS, 20, 7), max_rows=ROWS, max_cols=COLS, max_batch=Bc,
                                            device=local_rank)
            if args.pipeline > 1:
                self.ex.set_pipeline(args.pipeline)
            self.ex.set_fast_split(bool(args.fast_split))
            cap = self.ex.max_keypoints
            self.mt = match.robust(LOWE_RATIO, False, max_n1=cap, max_n2=cap, max_batch=Bc, device=local_rank)
            # outputs are double-buffered so that step k's matching can run under step k+1's extraction
            self.n_buf = 2 if args.overlap else 1
            self.bufs = []
            for _ in range(self.n_buf):
                self.bufs.append(dict(kps=torch.zeros((Bc, cap, 7), dtype=torch.float32, device="cuda"),
                                      desc=torch.zeros((Bc, cap, 32), dtype=torch.uint8, device="cuda"),
                                      cnt=torch.zeros((Bc,), dtype=torch.int32, device="cuda"),
                                      pairs=torch.zeros((Bc, cap, 2), dtype=torch.int32, device="cuda"),
                                      mcnt=torch.zeros((Bc,), dtype=torch.int32, device="cuda"),
                                      desc_prev=torch.zeros((Bc, cap, 32), dtype=torch.uint8, device="cuda"),
                                      cnt_prev=torch.zeros((Bc,), dtype=torch.int32, device="cuda")))
            # frame b (keyframe side, idx_2) is matched against frame b-1 inside its 8-frame scene (frame side, idx_1)
            self.prev = torch.tensor([(b - 1) if b % 8 else min(b + 7, Bc - 1) for b in range(Bc)], dtype=torch.long, device="cuda")
            # the extraction is the critical path: it gets the high-priority queue, matching fills the slots it leaves free
            multi = args.overlap or n_chain > 1
            self.s_ext = torch.cuda.Stream(priority=0 if args.match_first else -1) if multi else torch.cuda.current_stream()
            self.s_match = torch.cuda.Stream(priority=-1 if args.match_first else 0) if args.overlap else self.s_ext
            self.ev_ext = [torch.cuda.Event() for _ in range(self.n_buf)]
            self.ev_match = [torch.cuda.Event() for _ in range(self.n_buf)]
            self.k = 0

        def step(self):
            k = self.k % self.n_buf
            self.k += 1
            b = self.bufs[k]
            self.last = (k, self.k & 1)                      # (output buffer set, input batch) of the most recent step: the parity check reads it
            if args.overlap:
                self.s_ext.wait_event(self.ev_match[k])      # the matcher of two steps ago has released this buffer set
            self.ex.extract_batch_dev(self.frames[self.k & 1], b["kps"], b["desc"], b["cnt"], stream=self.s_ext.cuda_stream)
            if args.overlap:
                self.ev_ext[k].record(self.s_ext)
                self.s_match.wait_event(self.ev_ext[k])
            with torch.cuda.stream(self.s_match):
                torch.index_select(b["desc"], 0, self.prev, out=b["desc_prev"])   # gather "previous frame" descriptor blocks (device)
                torch.index_select(b["cnt"], 0, self.prev, out=b["cnt_prev"])
                self.mt.brute_force_match_batch_dev(b["desc_prev"], b["cnt_prev"], b["desc"], b["cnt"], b["pairs"], b["mcnt"],
                                                    stream=self.s_match.cuda_stream)
                if args.overlap:
                    self.ev_match[k].record(self.s_match)

    chains = [Chain(c * Bc) for c in range(n_chain)]
    ex = chains[0].ex
    torch.cuda.synchronize()   # inputs and buffers were created on the default stream

    def step():
        for ch in chains:
            ch.step()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    for ch in chains:
        _lib.check(L.ovs_orb_profile_enable(ch.ex._h, 1), "profile_enable")
        _lib.check(L.ovs_matcher_profile_enable(ch.mt._h, 1), "profile_enable")
    with collector_paused():
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        t1 = time.perf_counter()
    elapsed = t1 - t0
    # ---- the LAST timed step's outputs, copied to the host before anything else touches the buffers: what the parity check below compares
    # with the CPU oracle (so the checked bytes are the ones the timed schedule itself produced: level-0 split, overlap, second stream)
    # (a plain run takes it only for --dump-outputs)
    last_out = None
    if rank == 0 and (args.full or args.dump_outputs):
        last_out = []
        for ch in chains:
            k, which = ch.last
            b = ch.bufs[k]
            last_out.append(dict(which=which, cap=ch.ex.max_keypoints,
                                 kps=b["kps"].cpu().numpy().view(np.uint8).reshape(Bc, -1, 28), desc=b["desc"].cpu().numpy(),
                                 cnt=b["cnt"].cpu().numpy(), pairs=b["pairs"].cpu().numpy(), mcnt=b["mcnt"].cpu().numpy()))
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, last_out, Bc)
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    # ---- per-stage HIP-event times over the timed region (recorded on the launch stream by the library)
    # (summed over the chains: with several chains in flight the figures are per-chain launch durations under sharing)
    # (with the level-0 split on, "pyramid" is the window in which the seven resize launches AND the level-0 FAST launch run side by side,
    #  "fast" is the launch over levels 1..7 that follows; fast_level0 is the level-0 launch's own duration inside that window)
    stage_ms = {"pyramid": 0.0, "fast": 0.0, "tree": 0.0, "describe": 0.0, "match_near": 0.0, "match_resolve": 0.0}
    fast_l0_ms = 0.0
    for ch in chains:
        aux = C.c_float()
        nca = C.c_int32()
        _lib.check(L.ovs_orb_profile_read_aux(ch.ex._h, C.byref(aux), C.byref(nca)), "profile_read_aux")
        fast_l0_ms += aux.value / max(nca.value, 1)
        st4 = (C.c_float * 4)()
        st2 = (C.c_float * 2)()
        nc = C.c_int32()
        _lib.check(L.ovs_orb_profile_read(ch.ex._h, st4, C.byref(nc)), "profile_read")
        calls = max(nc.value, 1)
        _lib.check(L.ovs_matcher_profile_read(ch.mt._h, st2, C.byref(nc)), "profile_read")
        for key, v in zip(("pyramid", "fast", "tree", "describe"), st4):
            stage_ms[key] += v / calls
        stage_ms["match_near"] += st2[0] / calls
        stage_ms["match_resolve"] += st2[1] / calls

    # units per step: with two output buffer sets each one is permanently paired with one of the two alternating input batches (step parity
    # picks both), so the mean over the buffer sets is the exact per-step average of the timed region (K even; +-1 step's difference else)
    kp_step = matches_step = pairs_step = 0
    for ch in chains:
        for b in ch.bufs:
            cnt = b["cnt"].cpu().numpy().astype(np.int64)
            kp_step += cnt.sum() / float(ch.n_buf)
            matches_step += b["mcnt"].cpu().numpy().astype(np.int64).sum() / float(ch.n_buf)
            pairs_step += (cnt * cnt[ch.prev.cpu().numpy()]).sum() / float(ch.n_buf)
    totals = torch.tensor([kp_step, matches_step, pairs_step], dtype=torch.float64, device="cuda")
    if world > 1:
        dist.all_reduce(totals, op=dist.ReduceOp.SUM)
    kp_all, matches_all, pairs_all = (float(x) for x in totals.cpu().numpy())

    head = {
        "metric": "ORB kpts+descriptors/sec and Hamming matches/sec @1920x1080, 8-level pyramid",
        "value": round(kp_all * args.steps / elapsed, 1),
        "unit": "keypoints+descriptors/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: 1920x1080 mono, 8 pyramid levels (x1.2), 2000 ORB features, extract + "
                               "robust::brute_force_match (thr 50, ratio 0.9) against the previous frame",
                   "frames_per_step_per_gpu": B, "distinct_input_batches": 2, "sharding": "frames across ranks, no collective",
                   "schedule": ("%d independent chain(s) of %d frames; " % (n_chain, Bc))
                               + ("matching of step k on a second stream under the extraction of step k+1 (double-buffered)"
                                  if args.overlap else "extraction and matching serial on one stream")},
        "frames_per_sec": round(B * world * args.steps / elapsed, 2),
        "matches_per_sec": round(matches_all * args.steps / elapsed, 1),
        "hamming_distances_per_sec": round(pairs_all * args.steps / elapsed, 1),
        "keypoints_per_frame": round(kp_step / B, 2),
        "matches_per_frame": round(matches_step / B, 2),
        "stage_ms_per_step": {k: round(v, 5) for k, v in stage_ms.items()},
        "fast_level0_ms_inside_pyramid_window": round(fast_l0_ms, 5),
        **({"test_hook": "OVS_BENCH_ONE_DEVICE=1: all ranks on ONE device over gloo -- a code-path test, not a measurement"} if one_device else {}),
    }
    if not args.full:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps(head))
        return

    # ---- the same stages with each kernel ALONE on the GPU (extract, sync, match, sync): what the per-kernel rooflines below are quoted
    # on, because under the two-stream schedule the matcher and the pyramid stretch each other
    iso_ms = {k: 0.0 for k in stage_ms}
    n_iso = 4
    for ch in chains:
        ch.ex.set_fast_split(False)   # one FAST launch over all levels, strictly after the pyramid
        for _ in range(n_iso):
            b = ch.bufs[0]
            ch.ex.extract_batch_dev(ch.frames[0], b["kps"], b["desc"], b["cnt"], stream=ch.s_ext.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(ch.s_match):
                torch.index_select(b["desc"], 0, ch.prev, out=b["desc_prev"])
                torch.index_select(b["cnt"], 0, ch.prev, out=b["cnt_prev"])
                ch.mt.brute_force_match_batch_dev(b["desc_prev"], b["cnt_prev"], b["desc"], b["cnt"], b["pairs"], b["mcnt"],
                                                    stream=ch.s_match.cuda_stream)
            torch.cuda.synchronize()
        st4 = (C.c_float * 4)()
        st2 = (C.c_float * 2)()
        nc = C.c_int32()
        _lib.check(L.ovs_orb_profile_read(ch.ex._h, st4, C.byref(nc)), "profile_read")
        calls = max(nc.value, 1)
        _lib.check(L.ovs_matcher_profile_read(ch.mt._h, st2, C.byref(nc)), "profile_read")
        for key, v in zip(("pyramid", "fast", "tree", "describe"), st4):
            iso_ms[key] += v / calls
        iso_ms["match_near"] += st2[0] / calls
        iso_ms["match_resolve"] += st2[1] / calls

    # ---- the popcount (vector-ALU) form of the all-pairs stage, alone, on the same inputs: bit-identical output (checked), its time
    # is what roofline_valu is quoted on; the timed region above runs the default (matrix-core) form
    popc_ms = 0.0
    popc_same = True
    for ch in chains:
        b = ch.bufs[0]
        ref_cnt = b["mcnt"].clone()
        ref_pairs = b["pairs"].clone()
        ch.mt.set_near_path("popcount")
        for _ in range(n_iso):
            with torch.cuda.stream(ch.s_match):
                ch.mt.brute_force_match_batch_dev(b["desc_prev"], b["cnt_prev"], b["desc"], b["cnt"], b["pairs"], b["mcnt"],
                                                    stream=ch.s_match.cuda_stream)
            torch.cuda.synchronize()
        st2 = (C.c_float * 2)()
        nc = C.c_int32()
        _lib.check(L.ovs_matcher_profile_read(ch.mt._h, st2, C.byref(nc)), "profile_read")
        popc_ms += st2[0] / max(nc.value, 1)
        popc_same = popc_same and bool(torch.equal(ref_cnt, b["mcnt"]))
        for i in range(min(4, Bc)):
            k = int(ref_cnt[i])
            popc_same = popc_same and bool(torch.equal(ref_pairs[i, :k], b["pairs"][i, :k]))
        ch.mt.set_near_path("matrix")

    # ---- north_star's own form of the all-pairs stage (popcount on the vector ALU, "no MFMA") under the SAME schedule and the same clock as
    # `value`: K steps bracketed by barriers, max over ranks. The last step runs on the same input batch as the last step of the main region,
    # so its outputs must equal the snapshot taken there (counts, keypoint records, descriptors, match pairs).
    for ch in chains:
        ch.mt.set_near_path("popcount")
        ch.ex.set_fast_split(bool(args.fast_split))
    for _ in range(2 + (args.steps & 1)):
        step()
    with collector_paused():
        barrier()
        tp0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        elapsed_popc = time.perf_counter() - tp0
    if world > 1:
        tt = torch.tensor([elapsed_popc], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed_popc = float(tt.item())
    popc_sched_same = None
    if rank == 0:
        popc_sched_same = True
        for ch, lo_ in zip(chains, last_out):
            k, which = ch.last
            b = ch.bufs[k]
            cnt_, mcnt_ = b["cnt"].cpu().numpy(), b["mcnt"].cpu().numpy()
            popc_sched_same = popc_sched_same and which == lo_["which"] and np.array_equal(cnt_, lo_["cnt"]) and np.array_equal(mcnt_, lo_["mcnt"])
            if popc_sched_same:   # rows behind a frame's count are stale bytes of earlier steps: compare the valid prefixes only
                ds, pr = b["desc"].cpu().numpy(), b["pairs"].cpu().numpy()
                kp_ = b["kps"].cpu().numpy().view(np.uint8).reshape(Bc, -1, 28)
                for i in range(Bc):
                    popc_sched_same = popc_sched_same and np.array_equal(ds[i, :cnt_[i]], lo_["desc"][i, :cnt_[i]]) \
                        and np.array_equal(kp_[i, :cnt_[i]], lo_["kps"][i, :cnt_[i]]) and np.array_equal(pr[i, :mcnt_[i]], lo_["pairs"][i, :mcnt_[i]])
    for ch in chains:
        ch.mt.set_near_path("matrix")

    ba_res = None if args.no_ba else bench_local_ba(world, rank, dist, torch)
    # a local map ten times larger (a loop-closure sized window): the size at which sharding the linearisation over GPUs can pay, see
    # DESIGN.md section 5 for the expected curve. Measured at N = 1 too (about a second with its scene): the single-device time is the
    # scaling curve's reference.
    ba_large = None if args.no_ba else bench_local_ba(world, rank, dist, torch, iters=10, n_pose=200, n_pt=100000, obs_per_pose=5000)
    side = None
    if world == 1 and not args.no_ba and not args.no_cpu_baseline:
        try:
            side = bench_other_configs()
        except Exception as ex:   # a side section must never cost the headline line
            side = {"error": repr(ex)}

    out = None
    if rank == 0:
        n_cand = 0
        for l in range(LEVELS):
            n_cand += len(ex.debug_candidates(l, frame=0)[0])
        ab = algorithmic_bytes(ROWS, COLS, kp_step / B, n_cand)
        ab["match_near"] = (2 * (kp_step / B) * 32 + (kp_step / B) * 8)   # (Nq+Nt)*32 + Nq*8 per problem (144 000 B at 2000x2000)
        ab["match_resolve"] = (kp_step / B) * (4 + 8)
        # the dominant kernel and its launch duration: from the each-kernel-alone pass when the level-0 split is on (the timed region then
        # runs FAST as two launches, one of them concurrent with the pyramid, so no single event pair brackets "the FAST launch" there);
        # both sets of HIP-event times are printed
        dom = max(iso_ms, key=lambda k: iso_ms[k])
        achieved = ab[dom] * B / (iso_ms[dom] * 1e-3) / 1e9
        # roofline.traffic: HBM-side bytes per launch from rocprofv3 PMC passes. Counters cannot be collected from inside this process: at
        # N = 1 the run spawns short child runs of itself under rocprofv3 (live_pmc_traffic, --live-pmc 1) after the timed region; the committed
        # summary of the same command (tools/gpu_pmc.sh -> profiles/pmc_traffic.json) is the labelled fallback, and the source of the other stages.
        traffic = None
        pmc = {}
        pmc_stale = None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath):
            try:
                pmc = json.load(open(tpath))
                # the counters describe the kernels they were collected from: a stage's figure is refused when the sources of that stage's
                # kernels (its .hip file + the shared headers) have changed since (per stage: a matcher edit does not age the FAST counters)
                src_dir = os.path.join(ROOT, "openvslam_amd", "csrc")
                by_stage = pmc.get("csrc_sha16_by_stage", {})
                now = pmc_stage_fingerprint(src_dir, dom)
                if by_stage.get(dom) != now:
                    pmc_stale = "profiles/pmc_traffic.json: the %s counters were collected from other kernel sources (fingerprint %s, now %s): re-run tools/gpu_pmc.sh" % (
                        dom, by_stage.get(dom), now)
                    pmc = {}
                # the PMC passes may have run at another frames-per-launch: every per-launch count here is linear in it
                pmc_scale = Bc / float(pmc.get("batch", Bc))
                traffic = int(pmc[dom] * pmc_scale) if dom in pmc else None
            except Exception:
                traffic = None
        traffic_live_note = None
        live_valu = None
        if args.live_pmc and world == 1 and not one_device and dom == "fast":
            try:
                live, note = live_pmc_traffic("ovs::k_fast_cells")
            except Exception as ex_:   # a side measurement must never cost the headline line
                live, note = None, repr(ex_)
            if live is not None:
                traffic = int(live["bytes"] * (Bc / float(live["batch"])))
                traffic_live_note = ("measured in THIS run: rocprofv3 --pmc child passes of `bench.py --steps 2 --overlap 0 --fast-split 0` (FETCH_SIZE, "
                                     "WRITE_SIZE, SQ_INSTS_VALU each in its own pass, --kernel-trace only), (2*FETCH + WRITE) KiB per k_fast_cells launch "
                                     "at %s, scaled to %d" % (note, Bc))
                live_valu = int(live["insts_valu"] * (Bc / float(live["batch"])))
            else:
                traffic_live_note = "live PMC passes unavailable (%s)" % note
        roof = {"bound": "hbm", "kernel": {"pyramid": "k_resize_pair_u8 (x3) + k_resize_linear_u8", "fast": "k_fast_cells", "tree": "k_tree",
                                           "describe": "k_describe", "match_near": "k_hamming_near",
                                           "match_resolve": "k_bf_resolve"}[dom],
                "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                "traffic": traffic,
                "traffic_source": traffic_live_note if live_valu is not None else
                ((traffic_live_note + "; " if traffic_live_note else "") +
                 ("profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `bench.py --overlap 0`, (2*FETCH + WRITE) KiB, collected at "
                  "%s frames per launch and scaled to %d; not measured in this run)" % (pmc.get("batch", "the same"), Bc) if traffic else str(pmc_stale))),
                "algorithmic_bytes_per_launch": int(ab[dom] * Bc), "launch_ms": round(iso_ms[dom] / n_chain, 5),
                "launch_ms_source": "HIP events on the launch stream, kernel alone on the GPU (4 launches after the timed region, same inputs)",
                "launches_per_step": n_chain}
        # whole extract against the SURVEY 8(d) per-frame figure (19 377 963 B at 1080p/2000)
        extract_ms = sum(stage_ms[k] for k in ("pyramid", "fast", "tree", "describe"))   # windows are consecutive: their sum is the chain
        lv = level_sizes(ROWS, COLS)
        px = [r * c for r, c in lv]
        frame_bytes = px[0] + sum(px[1:]) + 2 * sum(px) + (kp_step / B) * 60
        extract_gbs = frame_bytes * B / (extract_ms * 1e-3) / 1e9

        # ---- integer-VALU rooflines ("pair-distances/s vs the integer-ALU peak"): FAST and the matcher are issue-bound,
        # not HBM-bound, so their honest ceiling is the VALU issue rate measured on this chip (profiles/r01_valu_issue_rate.txt:
        # 2-operand 32-bit ops 2.4 cycles per wave-instruction, v_bcnt / packed / 3-operand ops 4.2), 1024 SIMDs x 2.4 GHz.
        simd_hz = 1024 * 2.4e9
        pairs_launch = pairs_step / n_chain
        near_s = iso_ms["match_near"] / n_chain * 1e-3
        # k_hamming_near runs on the matrix cores since round 2: a 256-bit Hamming distance is an exact i8 dot product of 256 terms
        # (2 * 256 integer ops per pair, v_mfma_i32_32x32x32_i8). Peak: 2x the dense bf16 rate of MI355X_MICROARCH.md (2.5 PF) = 5.0e15;
        # the issue-rate ceiling measured on this chip with tools/ubench/mfma_i8_ubench is 4.6e15 (34.8 cycles per MFMA per SIMD).
        near_ops = pairs_launch * 512.0
        valu_counts = {k: int(v * Bc / float(pmc.get("batch", Bc))) for k, v in pmc["insts_valu"].items()} if isinstance(pmc.get("insts_valu"), dict) else {}
        roofline_mfma = {
            "k_hamming_near": {"bound": "mfma", "unit": "TOP/s (i8)", "achieved": round(near_ops / near_s / 1e12, 1), "peak": 5000.0,
                               "frac": round(near_ops / near_s / 5.0e15, 4),
                               # the micro-architecture guide's measured i8 ceiling (>= 3944 TOP/s, 16x16x64) beside the 5000 TOP/s dense figure
                               "peak_guide_measured": 3944.0, "frac_of_guide_measured": round(near_ops / near_s / 3.944e15, 4),
                               "ubench_ceiling": 4600.0,
                               "frac_of_ubench_ceiling": round(near_ops / near_s / 4.6e15, 4),
                               "launch_ms_alone": round(near_s * 1e3, 5), "pair_distances_per_s": round(pairs_launch / near_s, 1),
                               "ops_model": "512 integer ops per pair (256 multiply-adds), 8 x v_mfma_i32_32x32x32_i8 per 32 x 32 pairs",
                               "vector_path_floor_pairs_per_s": round(simd_hz * 64.0 / (8 * 2.4 + 8 * 4.2), 1),
                               "achieved_GBps_algorithmic": round(ab["match_near"] * Bc / near_s / 1e9, 2)},
        }
        popc_s = popc_ms / n_chain * 1e-3
        popc_peak = simd_hz * 64.0 / (8 * 2.4 + 8 * 4.2)          # 8 v_xor_b32 + 8 v_bcnt_u32_b32 per 64 pairs per SIMD
        roofline_valu = {
            "k_hamming_near_popc": {"unit": "pair-distances/s", "achieved": round(pairs_launch / popc_s, 1), "peak": round(popc_peak, 1),
                                    "frac": round(pairs_launch / popc_s / popc_peak, 4), "launch_ms_alone": round(popc_s * 1e3, 5),
                                    "floor_model": "8 v_xor_b32 (2.4 cyc) + 8 v_bcnt_u32_b32 (4.2 cyc) per 64 pairs per SIMD",
                                    "note": "the selectable popcount form of the all-pairs stage (ovs_matcher_set_near_path); not the form the "
                                            "timed region runs", "same_pairs_as_matrix_path": popc_same},
        }
        if live_valu is not None:
            valu_counts["fast"] = live_valu
        if valu_counts.get("fast"):
            fast_s = iso_ms["fast"] / n_chain * 1e-3
            # What one VALU wave-instruction of THIS kernel costs a SIMD: measured with mixed instruction streams at the kernel's 7 waves per SIMD
            # (tools/ubench/valu_rate mix, profiles/r05d_valu_mix.txt): the pre-test's opcode mix (5 v_alignbyte + 18 v_sub/v_add + 2 v_or + 6 v_bitop3 + 1 v_and
            # per 4-pixel group, with its real dependences) issues at 3.71 cycles per instruction, the exact scorer's mix (16-bit min / max with a
            # v_perm / v_bfe every fourth) at 2.69, a pure fast-class VOP2 stream of the same shape at 2.77 -- neither the 2.3-cycle back-to-back rate of
            # a single opcode nor the 4 cycles per instruction rounds 3-4 priced everything at (SQ_ACTIVE_INST_VALU == SQ_INSTS_VALU on this kernel is
            # the counter's quad-cycle quantisation, not a busy measure). Weighted by the kernel's own mix per wave and cell (~160
            # pre-test, ~250 scoring, ~136 prologue / compaction / NMS instructions, the last group priced at 4.0): 3.32 cycles.
            cyc = (160 * 3.71 + 250 * 2.69 + 136 * 4.0) / 546.0
            roofline_valu["k_fast_cells"] = {"unit": "VALU wave-instructions/s", "achieved": round(valu_counts["fast"] / fast_s, 1),
                                             "peak": round(simd_hz / cyc, 1), "frac": round(valu_counts["fast"] / fast_s / (simd_hz / cyc), 4),
                                             "cycles_per_instruction_model": round(cyc, 3),
                                             "frac_if_every_instruction_cost_4_cycles": round(valu_counts["fast"] / fast_s / (simd_hz / 4.0), 4),
                                             "launch_ms_alone": round(fast_s * 1e3, 5), "insts_valu_per_launch": valu_counts["fast"],
                                             "insts_source": "rocprofv3 --pmc SQ_INSTS_VALU child pass of this run" if live_valu is not None
                                             else "profiles/pmc_traffic.json (SQ_INSTS_VALU pass)",
                                             "floor_model": "256 CUs x 4 SIMDs x 2.4 GHz / 3.32 cycles per VALU wave-instruction (mixed-stream microbenchmark "
                                                            "at 7 waves per SIMD, weighted by the kernel's instruction mix). Rounds 3-5 ran at 0.61-0.63 of it: "
                                                            "what kept the slots free was the wait for a cell's tile, and round 6's group-major work order "
                                                            "(neighbouring workgroups read neighbouring pieces of the same image rows: HBM-side traffic 1.28x -> "
                                                            "1.0x the algorithmic bytes) brought it to ~0.8; what is left is the instruction count itself "
                                                            "(~2100 wave-instructions per 64x64 cell, the same in the barrier-free one-wave-per-cell form)"}
        # ---- per-call latency of orb_extractor::extract through the C++ class boundary at THIS config's size, H2D / D2H
        # included (openvslam_amd/cpp/bench_shim; one call = one upload, one kernel chain, one D2H, one wait)
        class_lat = None
        if world == 1 and not args.no_cpu_baseline:
            try:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import class_latency
                class_lat = class_latency.measure(ROWS, COLS, NFEAT, 100)
            except Exception as ex_:   # a side section must never cost the headline line
                class_lat = {"error": repr(ex_)}

        # ---- CPU oracle on a bounded sample of the frames of the LAST timed step: its wall time is cpu_baseline (rank 0, N = 1 only), its
        # outputs are the parity check of that step's keypoint records, descriptors and match pairs (N > 1: eight frames, check only)
        cpu = None
        parity = {"checked_frames": 0, "bit_exact": None, "note": "--no-cpu-baseline: the oracle did not run"}
        if not args.no_cpu_baseline:
            cpu, parity = cpu_baseline((frames, frames_alt), last_out, Bc, budget_s=args.cpu_budget_s if world == 1 else 0.0)
            if world > 1:
                cpu = None

        out = {
            **head,
            "stage_ms_per_step_each_kernel_alone": {k: round(v, 5) for k, v in iso_ms.items()},
            "extract_algorithmic_GBps": round(extract_gbs, 2),
            "extract_frac_of_hbm_peak": round(extract_gbs / HBM_PEAK_GBS, 5),
            "roofline": roof,
            "roofline_valu": roofline_valu,
            "roofline_mfma": roofline_mfma,
            "class_boundary_latency": class_lat,
            "cpu_baseline": cpu,
            "local_ba": ba_res,
            "local_ba_large": ba_large,
            "other_configs": side,
            "parity": parity,
            "value_popcount_near_path": round(kp_all * args.steps / elapsed_popc, 1),
            "ms_per_step_popcount_near_path": round(elapsed_popc / args.steps * 1e3, 4),
            "popcount_near_path_same_outputs_as_value_run": popc_sched_same,
        }
        if cpu:
            out["speedup_vs_cpu_baseline"] = round(out["value"] / cpu["value"], 1)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    native_multi = None
    if rank == 0 and world > 1 and not args.no_ba:
        # SURVEY 8(e) "measure both": the native one-process entry (ovs_ba_multi_*) over all of this node's devices with the packed RCCL
        # all-reduce and with the direct xGMI peer exchange, in a SUBPROCESS with a time limit (a side measurement must never cost the
        # headline line; the process group is gone: the other ranks are exiting and their devices are idle)
        import subprocess
        try:
            pr = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ba_multi_bench.py"), str(world)], capture_output=True, text=True, timeout=180)
            native_multi = json.loads(pr.stdout.strip().splitlines()[-1]) if pr.stdout.strip() else {"error": "no output", "stderr": pr.stderr[-300:]}
        except Exception as ex:
            native_multi = {"error": repr(ex)}
    if rank == 0:
        if native_multi is not None:
            out["local_ba_native_multi"] = native_multi
        print(json.dumps(out))
        if out["parity"]["bit_exact"] is False or popc_sched_same is False:
            sys.stdout.flush()
            raise SystemExit("bench.py: PARITY FAILURE (%s; popcount-form outputs equal: %s)" % (json.dumps(out["parity"]), popc_sched_same))


def bench_local_ba(world, rank, dist, torch, iters=20, n_pose=50, n_pt=20000, obs_per_pose=2000):
    """BASELINE configs[4]: local BA, 50 keyframes x 2000 observations, 20 000 landmarks, fp64: one linearisation = residuals +
    Jacobians + Hpp/Hll/Hpl/bp/bl blocks. Edges are sharded by keyframe over the ranks; Hll|bl (1.92 MB) are all-reduced over
    RCCL. Reported beside the headline metric (not part of `value`)."""
    from openvslam_amd import ba
    from openvslam_amd.synth import synth_local_ba
    d = synth_local_ba(n_pose=n_pose, n_pt=n_pt, obs_per_pose=obs_per_pose, seed=0)
    shard = ba.shard_edges_by_keyframe(d["edges"], len(d["poses"]), rank, world)
    poses = torch.from_numpy(d["poses"]).cuda()
    fixed = torch.from_numpy(d["pose_fixed"]).cuda()
    pts = torch.from_numpy(d["points"]).cuda()
    edges = torch.from_numpy(shard.view(np.uint8)).cuda()
    lin = ba.local_ba_linearizer(d["cam"], d["huber_delta"])
    for _ in range(3):
        out = lin.linearize(poses, fixed, pts, edges)
    with collector_paused():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = lin.linearize(poses, fixed, pts, edges)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    n_edges = len(d["edges"])
    alg_bytes = n_edges * 32 + n_pose * 56 + n_pt * 24 + n_edges * 144 + n_pt * 96 + n_pose * 336   # ~20.0 MB / iteration at config 5
    # HBM-side traffic of one linearisation from the committed rocprofv3 --pmc passes (tools/gpu_lba_pmc.sh: FETCH_SIZE and WRITE_SIZE in their own
    # passes, (2 * FETCH + WRITE) KiB summed over k_linearize2 and k_reduce_scalars); null when the file is missing
    size_key = "config5" if (n_pose, n_pt, obs_per_pose) == (50, 20000, 2000) else ("large" if (n_pose, n_pt, obs_per_pose) == (200, 100000, 5000) else None)
    traffic = None
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_lba.json")) as fh:
            traffic = json.load(fh)[size_key]["traffic_bytes_per_linearisation"] if size_key and world == 1 else None
    except (OSError, KeyError, ValueError):
        traffic = None
    gbps = alg_bytes * iters / dt / 1e9
    roofline = {"bound": "hbm", "kernel": "k_linearize2 + k_reduce_scalars (one linearisation)", "achieved": round(gbps, 2), "peak": 8000.0,
                "unit": "GB/s", "frac": round(gbps / 8000.0, 4), "algorithmic_bytes_per_linearisation": alg_bytes, "traffic": traffic,
                "traffic_source": "profiles/pmc_lba.json (tools/gpu_lba_pmc.sh: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, 2 x FETCH + WRITE)" if traffic else None,
                "what_bounds_it": "its traffic at the rate partial-line requests allow: 1.5x the algorithmic bytes (the edge records are read by both "
                                  "halves), gathered 24-byte landmarks and 40-byte records; the 144-byte Hpl records leave as whole lines since round 6 "
                                  "(through LDS: 0.124 -> 0.100 ms per million edges); six waves per SIMD instead of two changed nothing "
                                  "(profiles/r06ay_lba_pmc_summary.txt, DESIGN.md 3.6)"}
    return {"workload": "%s%d keyframes x %d observations, %d landmarks, fp64, Huber sqrt(5.991)"
                        % ("BASELINE configs[4]: " if (n_pose, n_pt, obs_per_pose) == (50, 20000, 2000) else "", n_pose, obs_per_pose, n_pt),
            "ms_per_linearisation": round(dt / iters * 1e3, 4), "edges_per_sec": round(n_edges * iters / dt, 1),
            "algorithmic_GBps": round(alg_bytes * iters / dt / 1e9, 2), "allreduce_bytes": (n_pt * 12 + 2) * 8 if world > 1 else 0,
            "roofline": roofline,
            "chi2": float(out["chi2"][0].item()), "kernels": "ovs_ba_graph: k_linearize2 (ONE launch: keyframe-side workgroups -- one lane per edge in keyframe order, the 27 pose-block terms as a fixed-shape sum per 256 edges, the 144-byte Hpl records written as whole lines through LDS -- interleaved with landmark-side workgroups -- one lane per edge in landmark order, a landmark's terms added in its edges' order) + k_reduce_scalars (finishes the keyframes' blocks and the scalars; no atomics, bit-reproducible)",
            "exchange": "ONE packed all-reduce of Hll|bl|chi2 per linearisation" if world > 1 else "none (1 rank)",
            # DESIGN.md section 5, written down before any multi-GPU node ran this: what ms_per_linearisation is expected to be at this N
            "expected_ms_per_linearisation": _expected_lba_ms(world, n_pt, dt / iters * 1e3 if world == 1 else None),
            "tolerance_vs_oracle": "Hpl, Hll, bl bit-exact; Hpp, bp, chi2 1e-13 rel (1 GPU); landmark sums 1e-10 rel (multi-rank)"}


def _expected_lba_ms(world, n_pt, one_device_ms):
    """DESIGN.md section 5's model of the sharded linearisation: compute = the one-device time / N (0.032 ms at config 5, 0.122 ms at
    local_ba_large when not measured in this run), exchange = a ring all-reduce of the packed (12 n_pt + 2) f64 buffer over xGMI: 2 (N - 1) hops
    of 5-10 us plus 2 (N - 1) / N x bytes at <= 153 GB/s per link. Returned as [low, high]; at N = 1 the measured time itself."""
    if world == 1:
        return [round(one_device_ms, 4), round(one_device_ms, 4)]
    base = 0.032 if n_pt <= 20000 else 0.122
    nbytes = (n_pt * 12 + 2) * 8
    wire = 2.0 * (world - 1) / world * nbytes / 153e9 * 1e3
    return [round(base / world + 2 * (world - 1) * 0.005 + wire, 4), round(base / world + 2 * (world - 1) * 0.010 + 2.0 * wire, 4)]


def bench_other_configs(iters=10):
    """BASELINE configs[0], [2], [3] (parity-test cases) timed once each through the HOST entry points (H2D + kernels +
    D2H per call: these matchers are latency-bound, tiny problems) next to the CPU oracle on the same inputs. Not part of `value`.
    Part of the cpu_baseline leg: the oracle is only timed and compared here, it never feeds the product path."""
    import numpy as np
    from oracle import binding as ob
    from openvslam_amd import feature, match, synth
    out = {}

    def timeit(fn, n, warm=1):
        """median of n individually timed calls after `warm` untimed ones (a mean over 10 calls right after an oracle
        timing loop read 21x too high on a fresh box)"""
        for _ in range(warm):
            r = fn()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return ts[len(ts) // 2] * 1e3, r

    iters = max(iters, 50)
    warm = 10

    sf = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)]).astype(np.float32)).astype(np.float32)
    # configs[0]: 752x480, 1000 features, area::match_in_consistent_area (margin 100) between two frames 5 px apart
    a = synth.synth_frame(480, 752, seed=0)
    b = synth.synth_frame(480, 752, seed=0, shift=(5, 0), noise_seed=4242)
    ex = feature.orb_extractor(feature.orb_params(1000), max_rows=480, max_cols=752)
    ka, da = ex.extract(a)
    kb, db = ex.extract(b)
    gp, ogp = match.grid_params(752, 480), ob.grid_params(752, 480)
    am = match.area(0.9, True, max_targets=2048, max_queries=2048)
    prev0 = np.ascontiguousarray(np.stack([ka["x"], ka["y"]], 1), np.float32)
    g_ms, (gn, gm) = timeit(lambda: am.match_in_consistent_area(gp, ka, da, kb, db, prev0.copy(), 100), iters, warm)
    fa, fb = match.frame_dev(gp, ka, da), match.frame_dev(gp, kb, db)   # what the class shims do: a frame goes up once, matchers take the handle
    r_ms, (rn, rm) = timeit(lambda: am.match_in_consistent_area(gp, fa, None, fb, None, prev0.copy(), 100), iters, warm)
    c_ms, (cn, cm) = timeit(lambda: ob.area_match_in_consistent_area(ogp, ka, da, kb, db, prev0.copy(), 100, 0.9, True), 3)
    e_ms, _ = timeit(lambda: ex.extract(a), iters, warm)
    out["config0_euroc_mono_init"] = {"extract_ms_per_frame_host_api": round(e_ms, 3), "area_match_ms": round(r_ms, 3),
                                      "area_match_host_arrays_per_call_ms": round(g_ms, 3), "area_match_cpu_oracle_ms": round(c_ms, 3),
                                      "matches": int(gn), "parity": bool(gn == cn and rn == cn and np.array_equal(gm, cm) and np.array_equal(rm, cm))}
    # configs[2]: KITTI geometry 1241x376 x2, 2000 features each, stereo::compute
    left, right, _ = synth.synth_stereo_pair(376, 1241, seed=1)
    el = feature.orb_extractor(feature.orb_params(2000), max_rows=376, max_cols=1241)
    er = feature.orb_extractor(feature.orb_params(2000), max_rows=376, max_cols=1241)
    kl, dl = el.extract(left)
    kr, dr = er.extract(right)
    st = match.stereo(el, er, kl, dl, kr, dr, 386.1448, 0.5372)
    g_ms, (xr, _) = timeit(st.compute, iters, warm)
    oxl, oxr = ob.OrbExtractor(ob.make_params(2000)), ob.OrbExtractor(ob.make_params(2000))
    oxl.extract(left)
    oxr.extract(right)
    c_ms, (wxr, _, _) = timeit(lambda: ob.stereo_compute(oxl, oxr, kl, dl, kr, dr, 386.1448, 0.5372), 3)
    out["config2_kitti_stereo"] = {"stereo_compute_ms": round(g_ms, 3), "stereo_compute_cpu_oracle_ms": round(c_ms, 3),
                                   "valid_depths": int((xr >= 0).sum()), "parity": bool(np.array_equal(xr.view(np.uint32), wxr.view(np.uint32)))}
    # configs[3]: 3840x1920, 4000 frame keypoints, 10 000 landmarks, projection::match_frame_and_landmarks, margin 5
    k, d = synth.synth_keypoints(4000, 1920, 3840, seed=1)
    lm = synth.synth_landmarks(k, d, 10000, 1920, 3840, seed=2, n_from_frame=5200)
    gp, ogp = match.grid_params(3840, 1920), ob.grid_params(3840, 1920)
    pm = match.projection(0.8, True, max_targets=4096, max_queries=10240)
    g_ms, (ga, gn) = timeit(lambda: pm.match_frame_and_landmarks(gp, k, d, sf, lm["xy"], lm["level"], lm["desc"], 5.0, lm_valid=lm["valid"]), iters, warm)
    fk = match.frame_dev(gp, k, d)
    r_ms, (ra, rn) = timeit(lambda: pm.match_frame_and_landmarks(gp, fk, None, sf, lm["xy"], lm["level"], lm["desc"], 5.0, lm_valid=lm["valid"]), iters, warm)
    c_ms, (ca, cn) = timeit(lambda: ob.projection_match_frame_and_landmarks(ogp, k, d, sf, lm["xy"], lm["level"], lm["desc"], 5.0, 0.8,
                                                                           lm_valid=lm["valid"]), 3)
    out["config3_equirect_projection"] = {"match_frame_and_landmarks_ms": round(r_ms, 3), "host_arrays_per_call_ms": round(g_ms, 3),
                                          "cpu_oracle_ms": round(c_ms, 3), "matches": int(gn),
                                          "parity": bool(np.array_equal(ga, ca) and np.array_equal(ra, ca))}
    # per-frame pose-only optimisation (tracking thread): 2000 observations, 40 % stereo, 10 % outliers
    from openvslam_amd import ba
    T0, pobs, pcam, pbf, _ = synth.synth_pose_frame(ob.POSE_OBS_DTYPE, 2000, 7)
    g_ms, (gT, gout, gnv) = timeit(lambda: ba.pose_optimize(T0, pobs, pcam, pbf), iters, warm)
    c_ms, (cT, cout, cnv) = timeit(lambda: ob.pose_optimize(T0, pobs, pcam, pbf), 3)
    out["pose_optimizer_2000_obs"] = {"pose_optimize_ms": round(g_ms, 3), "cpu_oracle_ms": round(c_ms, 3), "num_valid": int(gnv),
                                      "parity": bool(np.allclose(gT, cT, rtol=0, atol=1e-9) and gnv == cnv)}
    # BASELINE configs[4] end to end: both optimisation rounds of local_bundle_adjuster::optimize (5 + 10 LM iterations, outlier gate)
    from oracle import lba
    d = synth.synth_local_ba(seed=0, pose_noise=0.03, point_noise=0.03)
    g_ms, gr = timeit(lambda: ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"]), 5, 2)
    ba.local_ba_set_solver("host")   # the reduced camera system on the host (rounds 1-3, BASELINE's north star): timed beside the default
    try:
        h_ms, hr = timeit(lambda: ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"]), 3, 1)
    finally:
        ba.local_ba_set_solver("device")
    c_ms, cr = timeit(lambda: lba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"]), 1)
    out["config4_local_ba_optimize"] = {"local_ba_optimize_ms": round(g_ms, 1), "cpu_oracle_ms": round(c_ms, 1),
                                        "lm_iterations": [int(gr["info"][4]), int(gr["info"][5])],
                                        "chi2_before_after": [float(gr["info"][0]), float(gr["info"][3])],
                                        "outliers": int(gr["mono_outlier"].sum()),
                                        "parity": bool(np.allclose(gr["poses"], cr["poses"], rtol=1e-7, atol=1e-8)
                                                       and np.allclose(gr["points"], cr["points"], rtol=1e-7, atol=1e-8)),
                                        "local_ba_optimize_host_solver_ms": round(h_ms, 1),
                                        "host_solver_same_result": bool(np.allclose(gr["poses"], hr["poses"], rtol=1e-9, atol=1e-10)),
                                        "note": "linearisation, landmark elimination (Schur complement), the Cholesky solve of the reduced camera system "
                                                "(288 x 288 here; csrc/ba_solve.hip, f64 matrix cores) and back-substitution on the GPU: an LM trial reads back "
                                                "three scalars and a flag. host_solver: ovs_local_ba_set_solver(1), the system crosses PCIe and is solved on "
                                                "the host once per trial (rounds 1-3)"}
    out["note"] = ("median of >= 50 calls after 10 warm-up calls; matcher figures with the frame side resident (ovs_frame_dev, as the class shims "
                   "use it) and, beside them, with host arrays re-uploaded per call; CPU oracle single-threaded on the same inputs")
    return out


def cpu_baseline(frame_sets, last_out, Bc, budget_s=12.0):
    """The CPU oracle ("port": from-spec restatement, there is no reference source to build) on a bounded sample of the frames the LAST timed
    step processed: extract + brute_force_match in the bench's own pairing (frame b against b-1 inside its 8-frame scene, the scene's first
    frame against its last). Two results: the wall time of the oracle work (cpu_baseline) and, computed afterwards outside that clock, the
    comparison of the oracle's outputs with the bytes the timed GPU schedule left in its output buffers (parity)."""
    from oracle import binding as ob
    ob.build()
    threads = min(8, os.cpu_count() or 1)   # upstream's optional OpenMP shape: parallel over the 8 pyramid levels
    ox = ob.OrbExtractor(ob.make_params(NFEAT), threads=threads)
    n_total = Bc * len(last_out)
    res = {}       # global frame index -> (keypoint records, descriptors)
    pairs = {}     # global frame index (keyframe side) -> oracle match pairs against its `prev` frame
    n_kp = n_match = 0
    t0 = time.perf_counter()
    g = 0
    while g < n_total:
        c, b = divmod(g, Bc)
        k, d = ox.extract(frame_sets[last_out[c]["which"]][g])
        res[g] = (k, d)
        n_kp += len(k)
        if b % 8:
            pairs[g] = ob.robust_brute_force_match(res[g - 1][1], d, None, LOWE_RATIO)
            n_match += len(pairs[g])
        first = c * Bc + (b // 8) * 8
        if b == min((b // 8) * 8 + 7, Bc - 1) and first != g:      # the scene is complete: its first frame is matched against its last
            pairs[first] = ob.robust_brute_force_match(d, res[first][1], None, LOWE_RATIO)
            n_match += len(pairs[first])
        g += 1
        if g % 8 == 0 and time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    n_frames = g
    # ---- parity of the timed step (outside the clock above)
    bad = []
    for g in range(n_frames):
        c, b = divmod(g, Bc)
        lo = last_out[c]
        k, d = res[g]
        n = int(lo["cnt"][b])
        if n != len(k) or not np.array_equal(lo["kps"][b, :n].reshape(-1), k.view(np.uint8).reshape(-1)):
            bad.append("frame %d: keypoint records (gpu %d, oracle %d)" % (g, n, len(k)))
        elif not np.array_equal(lo["desc"][b, :n], d):
            bad.append("frame %d: descriptors" % g)
        if g in pairs:
            m = int(lo["mcnt"][b])
            if m != len(pairs[g]) or not np.array_equal(lo["pairs"][b, :m], pairs[g]):
                bad.append("frame %d: match pairs (gpu %d, oracle %d)" % (g, m, len(pairs[g])))
    parity = {"checked_frames": n_frames, "checked_match_problems": len(pairs), "bit_exact": not bad,
              "what": "the LAST timed step's output buffers (28-byte keypoint records, 32-byte descriptors, brute_force_match index pairs) against the "
                      "in-repo CPU oracle run on the same frames; the oracle is a from-spec restatement (upstream source unavailable: parity unpinned)",
              **({"mismatches": bad[:8]} if bad else {})}
    cpu = {"value": round(n_kp / dt, 1), "unit": "keypoints+descriptors/s", "cores": threads, "kind": "port",
           "kind_note": "scalar from-spec restatement (oracle/): no SIMD resize / FAST / GaussianBlur as upstream gets from OpenCV, so the ratio to it "
                        "overstates what the GPU path gains over a real OpenVSLAM build",
           "sample": "%d frames 1920x1080 (extract, OpenMP over levels) + %d brute_force_match calls, %.1f s wall" % (n_frames, len(pairs), dt),
           "frames_per_sec": round(n_frames / dt, 3), "matches_per_sec": round(n_match / dt, 1)}
    return cpu, parity


if __name__ == "__main__":
    main()
