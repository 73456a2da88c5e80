"""The local-BA graph at the sizes where its host plan (openvslam_amd/csrc/ba_graph_plan.inc; its decisions alone: tests/test_ba_graph_plan.py) can
still go wrong on the device: a landmark run closed by the landmark count next to a landmark of more edges than a workgroup has slots, a keyframe
of exactly one chunk next to one of a chunk and one entry, the work order of k_schur_l where the serpentine turns round (9 and 17 free
keyframes), and the two edge lists ovs_ba_graph_create refuses. Small scenes: a few hundred landmarks, a few seconds in all."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openvslam_amd.synth import synth_local_ba

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def observe(d, pairs, seed, stereo_frac=0.0):
    """Edges for the (keyframe, landmark) pairs of a synth_local_ba scene, shuffled: exact projection + N(0, 1) px; a share of them stereo
    (u_r = u - bf / z + N(0, 1)). Every landmark of the scene lies in front of every keyframe. Returns (mono, stereo, bf)."""
    from openvslam_amd.ba import EDGE_DTYPE, EDGE_STEREO_DTYPE, quat_to_rot
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs)[rng.permutation(len(pairs))]
    k, j = pairs[:, 0], pairs[:, 1]
    R = np.stack([quat_to_rot(q) for q in d["poses_true"][:, 3:]])
    pc = np.einsum("eab,eb->ea", R[k], d["points_true"][j]) + d["poses_true"][k, :3]
    assert (pc[:, 2] > 1.0).all()
    fx, fy, cx, cy = d["cam"]
    bf = 0.12 * fx
    e = np.zeros(len(pairs), EDGE_STEREO_DTYPE)
    e["pose_idx"], e["point_idx"] = k, j
    e["obs_x"] = fx * pc[:, 0] / pc[:, 2] + cx + rng.normal(size=len(e))
    e["obs_y"] = fy * pc[:, 1] / pc[:, 2] + cy + rng.normal(size=len(e))
    e["obs_x_right"] = e["obs_x"] - bf / pc[:, 2] + rng.normal(size=len(e))
    e["inv_sigma_sq"] = rng.choice([1.0, 1.0 / 1.44, 1.0 / 2.0736], len(e))
    is_st = rng.random(len(e)) < stereo_frac
    mono = np.zeros(int((~is_st).sum()), EDGE_DTYPE)
    for name in EDGE_DTYPE.names:
        mono[name] = e[name][~is_st]
    return mono, np.ascontiguousarray(e[is_st]), bf


def scene(kind):
    if kind == "runs":
        # 257 landmarks of one edge each: the 257th opens a run of its own (256 landmarks close the first); beside them a landmark of 257 edges,
        # a workgroup of its own whose edges pass in pieces of 256 (it needs 257 keyframes: a keyframe observes a landmark once)
        d = synth_local_ba(n_pose=257, n_pt=258, obs_per_pose=1, seed=11, pose_noise=0.01, point_noise=0.01, n_fixed=2)
        pairs = [(j, j) for j in range(257)] + [(k, 257) for k in range(257)]
        mono, st, bf = observe(d, pairs, 12)
        assert np.bincount(mono["point_idx"]).tolist() == [1] * 257 + [257]
    else:
        # keyframe 2 has exactly 512 edges (one chunk, two full half chunks), keyframe 3 exactly 513 (a second chunk of one entry), keyframe 4
        # one; landmarks 513 .. 518 are observed by nobody; mono and stereo edges mixed
        assert kind == "chunks"
        d = synth_local_ba(n_pose=5, n_pt=520, obs_per_pose=1, seed=13, pose_noise=0.01, point_noise=0.01, n_fixed=2)
        pairs = [(0, j) for j in range(40)] + [(2, j) for j in range(512)] + [(3, j) for j in range(513)] + [(4, 519)]
        mono, st, bf = observe(d, pairs, 14, stereo_frac=0.35)
        assert np.bincount(np.r_[mono["pose_idx"], st["pose_idx"]]).tolist() == [40, 0, 512, 513, 1] and len(mono) and len(st)
    return d, mono, st, bf


@pytest.mark.parametrize("kind", ["runs", "chunks"])
def test_linearisation_at_the_partition_edges_matches_the_oracle(oracle, kind):
    """The standard of test_graph_linearize_is_deterministic_and_matches_oracle (test_gpu_ba.py): Hll | bl | Hpl array-equal to the oracle, Hpp | bp |
    chi2 within 1e-13 (fixed-shape tree against a sequential sum), two runs the same bits."""
    import torch
    from oracle import lba
    from openvslam_amd import ba
    d, mono, st, bf = scene(kind)
    hm, hs = lba.SQRT_CHI2_MONO, lba.SQRT_CHI2_STEREO
    g = ba.graph(len(d["poses"]), d["pose_fixed"], len(d["points"]), mono, d["cam"], st, bf)
    P, X = torch.from_numpy(d["poses"]).cuda(), torch.from_numpy(d["points"]).cuda()
    runs = []
    for _ in range(2):
        out = g.linearize_dev(P, X, hm, hs)
        torch.cuda.synchronize()
        runs.append({k: t.cpu().numpy().copy() for k, t in ba.graph.views(out, g.n_pose, g.n_pt, g.n_edge).items()})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    want = oracle.ba_linearize(d["poses"], d["pose_fixed"], d["points"], mono, d["cam"], hm)
    if len(st):
        s = oracle.ba_linearize_stereo(d["poses"], d["pose_fixed"], d["points"], st, d["cam"], bf, hs)
        for k in ("Hpp", "bp", "Hll", "bl", "chi2"):
            want[k] = want[k] + s[k]
        want["Hpl"] = np.concatenate([want["Hpl"], s["Hpl"]])
    got = runs[0]
    for k in ("Hpl", "Hll", "bl"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("Hpp", "bp", "chi2"):
        scale = np.abs(want[k]).max()
        assert np.allclose(got[k], want[k], rtol=1e-13, atol=1e-13 * scale), k
    free = d["pose_fixed"] == 0
    md = max(np.abs(np.einsum("kii->ki", want["Hpp"][free])).max(), np.abs(np.einsum("kii->ki", want["Hll"])).max())
    assert np.isclose(got["max_diag"][0], md, rtol=1e-13)


# n_free -> the scene: 9 free keyframes put row 8 of the pair table on XCD 7, 17 put row 16 on XCD 0 again
OPT_SCENES = {9: dict(n_pose=11, n_pt=300, obs_per_pose=100, seed=21, pose_noise=0.01, point_noise=0.01, n_fixed=2),
              17: dict(n_pose=19, n_pt=400, obs_per_pose=90, seed=22, pose_noise=0.01, point_noise=0.01, n_fixed=2)}

CHILD = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from openvslam_amd import ba
from openvslam_amd.synth import synth_local_ba
from test_gpu_ba_graph_edges import OPT_SCENES
res = {}
for nf, kw in OPT_SCENES.items():
    d = synth_local_ba(**kw)
    r = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"])
    res.update({"%%d_%%s" %% (nf, k): np.asarray(v) for k, v in r.items()})
np.savez(sys.argv[1], **res)
"""


@pytest.fixture(scope="module")
def scanned(tmp_path_factory):
    """Both scenes optimised with OVS_BA_SCHUR_LISTS=0 (read once per process: a fresh child): every trial's k_schur scans for the pairs' common
    landmarks itself and never reads wg_pair."""
    out = tmp_path_factory.mktemp("schur_scan") / "scan.npz"
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), str(out)], env=dict(os.environ, OVS_BA_SCHUR_LISTS="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("n_free", sorted(OPT_SCENES))
def test_optimisation_on_the_work_order_equals_the_per_trial_scan(scanned, n_free):
    from openvslam_amd import ba
    d = synth_local_ba(**OPT_SCENES[n_free])
    assert int((d["pose_fixed"] == 0).sum()) == n_free
    r = ba.local_ba_optimize(d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"])
    assert r["info"][4] >= 1 and r["info"][1] < r["info"][0]      # trials ran and were accepted
    for k, v in r.items():
        assert np.array_equal(np.asarray(v), scanned["%d_%s" % (n_free, k)]), k


def test_graph_create_refuses_a_bad_index_and_a_duplicated_edge():
    from openvslam_amd import _lib, ba
    live = _lib.lib().ovs_debug_live_resources
    d, mono, st, bf = scene("chunks")
    args = (len(d["poses"]), d["pose_fixed"], len(d["points"]))
    ba.graph(*args, mono, d["cam"], st, bf).__del__()      # a warm cycle: the arena pool and this thread's page-locked image persist by design
    c0 = live()
    bad_m, bad_s, neg = mono.copy(), st.copy(), mono.copy()
    bad_m["point_idx"][7] = len(d["points"])
    bad_s["pose_idx"][len(st) - 1] = len(d["poses"])
    neg["pose_idx"][0] = -1
    for m, s in ((bad_m, st), (mono, bad_s), (neg, st)):
        with pytest.raises(_lib.OvsError) as err:
            ba.graph(*args, m, d["cam"], s, bf)
        assert err.value.status == -1      # OVS_ERR_INVALID
        assert "(ovs_ba_graph_create: an edge's keyframe or landmark index is out of range)" in str(err.value)
        assert live() == c0
    # the same (keyframe, landmark) once more: among the mono edges, and as a stereo edge beside its mono edge
    twice = np.concatenate([mono, mono[3:4]])
    also = np.concatenate([st, st[:1]])
    for name in mono.dtype.names:
        also[name][-1] = mono[name][5]
    for m, s, e in ((twice, st, mono[3]), (mono, also, mono[5])):
        with pytest.raises(_lib.OvsError) as err:
            ba.graph(*args, m, d["cam"], s, bf)
        assert err.value.status == -1
        assert "(ovs_ba_graph_create: keyframe %d has two edges to landmark %d)" % (e["pose_idx"], e["point_idx"]) in str(err.value)
        assert live() == c0
    ba.graph(*args, mono, d["cam"], st, bf).__del__()      # and the good list still builds
    assert live() == c0
