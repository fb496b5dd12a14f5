"""Batched tracking pipeline (main.py:76-132) vs the per-frame CPU oracle chain."""
import numpy as np
import pytest

from oracle import pipeline as op


@pytest.fixture(scope="module")
def seq():
    from slam355.synthetic import stereo_sequence

    return stereo_sequence(4, 1280, 720, seed=3)


def test_oracle_chain_recovers_forward_motion(seq):
    L, R, poses, rig = seq
    cache = {}
    for i in range(2):
        out = op.track_pair(L[i], R[i], L[i + 1], rig.P_l, rig.P_r, seed=5, frame=i, orb_cache=cache)
        assert out["n_temporal"] >= 10 and out["n_pnp"] >= 10
        # true relative motion: frame i+1 is 1 m ahead -> points move by -1 m in z
        rel = np.linalg.inv(poses[i + 1]) @ poses[i]
        assert np.allclose(out["tvec"], rel[:3, 3], atol=0.05)


def test_chain_poses_reference_semantics():
    from slam355.pipeline import chain_poses, relative_transform

    r = np.array([[0.0, 0.01, 0.0], [0, 0, 0], [0.0, -0.02, 0.001]])
    t = np.array([[0.0, 0.0, -1.0], [1, 1, 1], [0.1, 0.0, -1.0]])
    n = np.array([50, -1, 40])  # frame 1: PnP skipped -> previous T reused (main.py:94-98)
    P, T = chain_poses(np.eye(4), r, t, n)
    T0, T2 = relative_transform(r[0], t[0]), relative_transform(r[2], t[2])
    assert np.allclose(P[0], T0) and np.allclose(P[1], T0 @ T0) and np.allclose(P[2], T0 @ T0 @ T2)
    assert np.allclose(T0[:3, 3], [0, 0, 1.0])  # the sign flip of transformation.py:15-16


@pytest.mark.gpu
def test_gpu_tracker_matches_oracle_chain(seq):
    import torch
    from slam355.pipeline import Tracker

    L, R, poses, rig = seq
    B = 3
    trk = Tracker(B, 720, 1280, rig.P_l, rig.P_r, seed=5)
    trk.imgs.copy_(torch.from_numpy(np.concatenate([L[:B + 1], R[:B]])))
    rv, tv, n = trk.track(0)
    torch.cuda.synchronize()
    c = trk.counters()
    rv, tv, n = rv.cpu().numpy(), tv.cpu().numpy(), n.cpu().numpy()
    cache = {}
    for i in range(B):
        e = op.track_pair(L[i], R[i], L[i + 1], rig.P_l, rig.P_r, seed=5, frame=i, orb_cache=cache)
        assert c["stereo"][i] == e["n_stereo"], i
        assert c["f_inliers"][i] == e["n_f"], i
        assert np.array_equal(trk.f_mask[i, :e["n_stereo"]].cpu().numpy().astype(bool), e["f_mask"])
        X = trk.X[i, :e["n_f"]].cpu().numpy()
        assert np.all(np.abs(X - e["X"]) <= 1e-9 * np.maximum(1, np.abs(e["X"])))
        assert c["temporal"][i] == e["n_temporal"], i
        assert n[i] == e["n_pnp"], i
        assert np.allclose(rv[i], e["rvec"], atol=1e-8) and np.allclose(tv[i], e["tvec"], atol=1e-8)


@pytest.fixture(scope="module")
def corridor():
    from slam355.synthetic import corridor_sequence

    return corridor_sequence(4, 1280, 720, seed=21)


def test_corridor_scene_reaches_c2_keypoint_count(corridor):
    """BASELINE C2 = 2000 ORB kp/frame: with 64 kp per tile the textured corridor
    fills every tile's level budgets (levels 6-7 of a 216x192 patch cannot
    hold keypoints, so 56 per tile caps at ~1780)."""
    import oracle

    L, R, poses, rig = corridor
    _, _, _, cnt = oracle.orb_tiles_batch(np.concatenate([L[:2], R[:1]]), 64, 1 << 13)
    assert cnt.min() >= 2000, cnt
    out = op.track_pair(L[0], R[0], L[1], rig.P_l, rig.P_r, max_kp=64, seed=1, frame=0)
    assert out["n_stereo"] >= 400 and out["n_pnp"] >= 50, (out["n_stereo"], out["n_pnp"])
    rel = np.linalg.inv(poses[1]) @ poses[0]
    assert np.allclose(out["tvec"], rel[:3, 3], atol=0.05)


@pytest.mark.gpu
def test_gpu_tracker_corridor_c2_matches_oracle_and_chains_on_device(corridor):
    """C2 shape (2000+ kp/frame): per pair counts, masks and PnP equal the oracle
    chain; the device pose chain (k_pose_chain) equals the host chain_poses and
    continues across two track() calls."""
    import torch
    from slam355.pipeline import Tracker, chain_poses

    L, R, poses, rig = corridor
    B = 3
    trk = Tracker(B, 720, 1280, rig.P_l, rig.P_r, max_kp_per_tile=64, seed=2)
    trk.imgs.copy_(torch.from_numpy(np.concatenate([L[:B + 1], R[:B]])))
    rv, tv, n = trk.track(0)
    P1 = trk.poses.cpu().numpy()
    c = trk.counters()
    assert c["orb"].min() >= 2000
    rv, tv, n = rv.cpu().numpy(), tv.cpu().numpy(), n.cpu().numpy()
    cache = {}
    for i in range(B):
        e = op.track_pair(L[i], R[i], L[i + 1], rig.P_l, rig.P_r, max_kp=64, seed=2, frame=i,
                          orb_cache=cache)
        assert c["orb"][i] == len(cache[("L", i)][0])
        assert c["stereo"][i] == e["n_stereo"] and c["f_inliers"][i] == e["n_f"], i
        assert c["temporal"][i] == e["n_temporal"] and n[i] == e["n_pnp"], i
        assert np.allclose(rv[i], e["rvec"], atol=1e-8) and np.allclose(tv[i], e["tvec"], atol=1e-8)
    Ph, T = chain_poses(np.eye(4), rv, tv, n)
    assert np.allclose(P1, Ph, rtol=0, atol=1e-12)
    # second call continues the chain from the last pose (same frames again)
    trk.track(0)
    P2 = trk.poses.cpu().numpy()
    Ph2, _ = chain_poses(Ph[-1], rv, tv, n, T_prev=T)
    assert np.allclose(P2, Ph2, rtol=0, atol=1e-10)
    gt = np.stack([np.linalg.inv(poses[0]) @ poses[i + 1] for i in range(B)])
    assert np.abs(P1[:, :3, 3] - gt[:, :3, 3]).max() < 0.1


@pytest.mark.gpu
def test_gpu_device_chain_stale_transform():
    """ninl < 0 (PnP skipped, main.py:94) reuses the previous T on the device too."""
    import torch
    from slam355 import _lib
    from slam355.device import ptr, stream_ptr
    from slam355.pipeline import chain_poses

    r = np.array([[0.0, 0.01, 0.0], [0, 0, 0], [0.0, -0.02, 0.001], [0.3, -0.2, 0.1]])
    t = np.array([[0.0, 0.0, -1.0], [1, 1, 1], [0.1, 0.0, -1.0], [2.0, -1.0, 0.5]])
    n = np.array([50, -1, 40, -1], np.int32)
    dev = torch.device("cuda")
    st = torch.from_numpy(np.concatenate([np.eye(4), np.eye(4)]).ravel()).to(dev)
    out = torch.zeros((4, 16), dtype=torch.float64, device=dev)
    tr, tt, tn = (torch.from_numpy(a).to(dev) for a in (r, t, n))  # alive until the kernel ran
    _lib.call("slam_pose_chain", ptr(tr), ptr(tt), ptr(tn), 4, ptr(st), ptr(out), stream_ptr())
    P, T = chain_poses(np.eye(4), r, t, n)
    assert np.allclose(out.cpu().numpy().reshape(4, 4, 4), P, rtol=0, atol=1e-12)
    assert np.allclose(st.cpu().numpy()[16:].reshape(4, 4), T, rtol=0, atol=1e-14)


def _tie_frame(H=720, W=1280):
    """A grid of identical isolated bright pixels: every dot has the same FAST
    score and Harris response, so retainBest keeps all ~340 tied level-0
    keypoints of a tile (the oracle, like OpenCV, keeps every tie), more than
    the per-tile keypoint workspace (max_kp + 64) holds."""
    img = np.full((H, W), 40, np.uint8)
    img[::8, ::8] = 220
    return img


@pytest.mark.gpu
def test_gpu_tracker_raises_on_orb_overflow(corridor):
    """an overflowing ORB tile must not silently become a frame
    with no matches and a stale pose -- Tracker.check() raises."""
    import torch
    from slam355 import _lib
    from slam355.pipeline import Tracker

    L, R, poses, rig = corridor
    B = 1
    trk = Tracker(B, 720, 1280, rig.P_l, rig.P_r, max_kp_per_tile=64, seed=2)
    tie = _tie_frame()
    trk.imgs.copy_(torch.from_numpy(np.stack([L[0], tie, R[0]])))
    trk.track(0)
    assert int(trk.ows.count[1].item()) < 0  # the tie frame overflowed
    with pytest.raises(_lib.SlamError, match="overflow"):
        trk.check()
    trk.imgs.copy_(torch.from_numpy(np.stack([L[0], L[1], R[0]])))
    trk.track(0)
    trk.check()  # flag was reset; a normal batch passes


@pytest.fixture(scope="module")
def corridor9():
    from slam355.synthetic import corridor_sequence

    return corridor_sequence(9, 1280, 720, seed=21)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 1])
def test_gpu_window_mapper_equals_per_frame_maps(corridor9, n):
    """WindowMapper (the bench's tracked leg): one slam_map_windows call maps
    every window of the batch exactly as MapStore.append frame by frame does
    (rows and map points bit for bit, frame index = pair index in the window);
    problems() gives each window the export_data / read_bal_data problem of its
    frames (make_cam_params of the window's first n poses).  n = 1: one pair per
    window, no nearest-landmark partials at all (an empty workspace slice)."""
    import torch
    from slam355.mapping import MapStore
    from slam355.pipeline import Tracker, WindowMapper
    from slam355.XXXport_files import U_OFF, V_OFF, make_cam_params

    L, R, poses, rig = corridor9
    B = 8
    trk = Tracker(B, 720, 1280, rig.P_l, rig.P_r, max_kp_per_tile=64, seed=6)
    wm = WindowMapper(trk, n)
    trk.imgs.copy_(torch.from_numpy(np.concatenate([L[:B + 1], R[:B]])))
    wm.save_pose0(None)
    trk.track(0)
    wm.map_batch(torch.cuda.current_stream())
    wm.event.synchronize()
    probs = wm.problems(rig.P_l)
    assert len(probs) == B // n
    t_cnt = trk.t_cnt.cpu().numpy()
    dev_poses = trk.poses.cpu().numpy()
    for w in range(B // n):
        st = MapStore(capacity=n * trk.cap, max_queries=trk.cap)
        rows = []
        for j in range(n):
            b = w * n + j
            r = st.append(wm.abs[b], trk.Q1[b], trk.q1[b], j, 0.01, count=trk.t_cnt[b:b + 1])
            rows.append(r[: int(t_cnt[b])].cpu().numpy())
        om = np.vstack(rows)
        cams, pts, ci, pi, qs = probs[w]
        assert np.array_equal(pts, st.points().cpu().numpy())
        assert np.array_equal(ci, om[:, 0].astype(np.int64)) and np.array_equal(pi, om[:, 1].astype(np.int64))
        assert np.array_equal(qs, np.stack([om[:, 2] - U_OFF, om[:, 3] - V_OFF], 1))
        frames = [np.eye(4) if w == 0 else dev_poses[w * n - 1]] + [dev_poses[w * n + j] for j in range(n - 1)]
        assert np.array_equal(cams, make_cam_params(frames, rig.P_l).reshape(-1, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 8])
def test_gpu_tracked_frames_feed_local_ba(request, B):
    """tracking and local BA as one pipeline.  B tracked pairs
    -> device pose chain -> relative_to_abs3DPoints -> appendKeyPoints on the
    device map -> the export_data / read_bal_data problem -> BAProblem LM;
    equals the oracle chain (track_pair, the reference pose rule,
    oracle.mapping.append_keypoints, oracle Schur LM) step by step."""
    import torch
    from oracle import ba as oba
    from oracle import geometry as og
    from oracle import mapping as omap
    from slam355 import XXXport_files as xp
    from slam355.ba import BAProblem
    from slam355.pipeline import LocalMap, Tracker

    import shapes_ref as sr

    L, R, poses, rig = request.getfixturevalue("corridor" if B == 3 else "corridor9")
    trk = Tracker(B, 720, 1280, rig.P_l, rig.P_r, max_kp_per_tile=64, seed=6)
    lm = LocalMap(trk)
    trk.imgs.copy_(torch.from_numpy(np.concatenate([L[:B + 1], R[:B]])))
    trk.track(0)
    lm.add(0)
    # oracle chain (main.py:79-127)
    cache = {}
    Qs = np.empty((0, 3))
    om_rows, bf_rows = [], []
    pose, T = np.eye(4), np.eye(4)
    frames = [np.eye(4)]
    t_cnt = trk.t_cnt.cpu().numpy()
    d_abs, d_Q1, d_q1 = lm.abs.cpu().numpy(), trk.Q1.cpu().numpy(), trk.q1.cpu().numpy()
    for i in range(B):
        e = op.track_pair(L[i], R[i], L[i + 1], rig.P_l, rig.P_r, max_kp=64, seed=6, frame=i,
                          orb_cache=cache)
        if e["n_pnp"] >= 0:
            T, _, _ = og.pose_matrix_from_pnp(e["rvec"], e["tvec"])
        pose = pose @ T
        frames.append(pose)
        absP = og.relative_to_abs3DPoints(e["Q1"], pose)
        # the device's inputs to the association: the same temporal matches
        # (bit-exact image points), 3-D points within the triangulation /
        # pose-chain tolerance of the oracle's
        n = int(t_cnt[i])
        assert n == len(e["q1"]) and np.array_equal(d_q1[i, :n], e["q1"]), i
        assert np.allclose(d_Q1[i, :n], e["Q1"], rtol=1e-8, atol=1e-8), i
        assert np.allclose(d_abs[i, :n], absP, rtol=1e-7, atol=1e-7), i
        # appendKeyPoints on exactly the device's inputs: the association (nearest
        # landmark of a map that holds near-duplicate points, and the gate) is
        # exact given its inputs, but a near-tie can flip under the 1e-9-level
        # differences of the upstream triangulation, so it is checked on them
        Qs_in = Qs
        Qs, rows = omap.append_keypoints(Qs, d_abs[i, :n], 0.01, d_q1[i, :n], i, d_Q1[i, :n])
        om_rows.append(rows)
        # and the same frame by brute force with the first index on ties (the
        # device's rule, pinned by test_map_ties.py): the same map, every index
        bQs, brows = sr.map_assoc(Qs_in, d_abs[i, :n], 0.01, d_q1[i, :n], i, d_Q1[i, :n])
        assert np.array_equal(bQs, Qs), i
        bf_rows.append(brows)
    om = np.vstack(om_rows)
    got = lm.optimization_matrix()
    assert np.array_equal(got, np.vstack(bf_rows))  # every index, ties included
    assert got.shape == om.shape
    assert np.array_equal(got[:, [0, 2, 3]], om[:, [0, 2, 3]])
    gQ = lm.store.points().cpu().numpy()
    assert gQ.shape == Qs.shape and np.array_equal(gQ, Qs)
    # landmark indices: equal, except that when the map holds EXACT duplicates
    # (two matches of one frame appended at identical coordinates) the nearest
    # landmark is a tie; the device takes the first index, scipy's KDTree the
    # first in its tree's leaf order (unpinned).  Such rows must point at
    # bit-identical landmarks.
    gi, oi = got[:, 1].astype(np.int64), om[:, 1].astype(np.int64)
    diff = gi != oi
    assert np.array_equal(gQ[gi[diff]], gQ[oi[diff]]), np.where(diff)[0]
    assert diff.sum() <= 0.01 * len(gi)
    assert np.allclose(np.stack(lm.poses), np.stack(frames), rtol=0, atol=1e-10)
    cams, pts, ci, pi, qs = lm.problem(rig.P_l)
    # the oracle's problem from the device's association (ties resolved alike)
    ec, ep_, eci, epi, eqs = xp.problem_from_map(got, frames, Qs, rig.P_l)
    assert np.allclose(cams, ec, atol=1e-10) and np.array_equal(ci, eci) and np.array_equal(pi, epi)
    prob = BAProblem(cams, pts, ci, pi, qs)
    st = oba.LMState(1e-4)
    oc, opt = ec.copy(), ep_.copy()
    pairs = oba._obs_pairs(eci, epi)
    for it in range(3):
        # every iteration starts the oracle from the device's parameters, so a
        # rounding difference of one (ill-conditioned, real-track) solve does not
        # compound into the next; lambda follows the same accept/reject chain
        c0 = None
        if it:
            oc, opt = prob.params()
            c0 = prob.state()["COST"]
        prob.iterate(1)
        oc, opt, info = oba.lm_iteration_schur(oc, opt, eci, epi, eqs, st, pairs)
        s = prob.state()
        assert bool(s["ACCEPTED"]) == bool(info["accepted"]), it
        if c0 is not None:  # the same parameters: the cost itself agrees to rounding
            assert abs(c0 - info["cost"]) <= 1e-12 * info["cost"], it
        # the step: the map holds mismatched far points (cost ~1e8), so the
        # reduced system is ill-conditioned and the new cost agrees to ~1e-8
        # of itself; the achieved decrease agrees to 1e-5 of the decrease
        assert abs(s["COST_NEW"] - info["cost_new"]) <= 1e-7 * abs(info["cost_new"]), it
        dec = info["cost"] - info["cost_new"]
        assert abs((info["cost"] - s["COST_NEW"]) - dec) <= 1e-5 * abs(dec), it
        gc, gp = prob.params()
        assert np.allclose(gc, oc, rtol=1e-6, atol=1e-8), it


@pytest.mark.gpu
def test_gpu_orb_pipelined_tracker_equals_serial():
    """Tracker(orb_stream=...): ORB of batch k+1 on its own stream into the other
    of two workspaces while batch k's matching / PnP runs -- the same poses,
    counts and chained trajectory as the one-stream tracker, batch by batch."""
    import torch
    from slam355.pipeline import Tracker
    from slam355.synthetic import corridor_sequence

    B, nb = 4, 3
    L, R, poses, rig = corridor_sequence(B * nb + 1, 1280, 720, seed=33)
    packs = [torch.from_numpy(np.concatenate([L[k * B:k * B + B + 1], R[k * B:k * B + B]])).cuda()
             for k in range(nb)]
    ref = Tracker(B, 720, 1280, rig.P_l, rig.P_r, max_kp_per_tile=64, seed=2)
    pip = Tracker(B, 720, 1280, rig.P_l, rig.P_r, max_kp_per_tile=64, seed=2,
                  stream=torch.cuda.Stream(), orb_stream=torch.cuda.Stream())
    got, exp = [], []
    for k in range(nb):
        ref.track(k * B, imgs=packs[k])
        exp.append((ref.rvec.clone(), ref.tvec.clone(), ref.p_ninl.clone(), ref.poses.clone(),
                    ref.t_cnt.clone()))
    torch.cuda.synchronize()
    for k in range(nb):  # enqueued back to back: batch k+1's ORB overlaps batch k
        with torch.cuda.stream(pip.stream):
            pip.track(k * B, imgs=packs[k])
            got.append((pip.rvec.clone(), pip.tvec.clone(), pip.p_ninl.clone(),
                        pip.poses.clone(), pip.t_cnt.clone()))
    torch.cuda.synchronize()
    for k in range(nb):
        for a, b in zip(got[k], exp[k]):
            assert torch.equal(a, b), k
    ref.check()
    pip.check()


# ----------------------------------------------------------------------------- BASELINE C1
C1_CAP = 25  # ORB max_number_of_kp per tile giving C1's 500 kp/frame at 640x480
@pytest.fixture(scope="module")
def c1_seq():
    """BASELINE config 1: synthetic 640x480 grayscale, 500 ORB kp/frame, a
    2-keyframe window.  At 640x480 a tile's patch is 144x96, so only pyramid
    levels 0-2 can hold keypoints (border 31): cap 14 per tile gives 3 + 3 + 2
    per tile = 288 kp/frame; cap 25 gives 5 + 5 + 4 = 14 per tile = 504, i.e.
    the config's 500 kp/frame."""
    from slam355.synthetic import corridor_sequence

    # 0.45 m texture cells (0.3 at 1280x720): at half the resolution the finer
    # cells alias and leave too few temporal matches for PnP
    return corridor_sequence(3, 640, 480, seed=41, cell=0.45)


def test_oracle_c1_chain_is_c1_shaped(c1_seq):
    """The C1 sequence gives ~500 kp per frame at C1_CAP (25 per tile: at
    640x480 only pyramid levels 0-2 of a patch hold keypoints, so cap 14 would
    give 288) and a tracked pose."""
    import oracle

    L, R, poses, rig = c1_seq
    _, _, _, cnt = oracle.orb_tiles_batch(np.concatenate([L[:2], R[:1]]), C1_CAP, 1 << 13)
    assert 450 <= cnt.min() and cnt.max() <= 520, cnt
    for i in range(2):  # both pairs reach PnP (>= 5 temporal matches)
        out = op.track_pair(L[i], R[i], L[i + 1], rig.P_l, rig.P_r, max_kp=C1_CAP, seed=4, frame=i)
        assert out["n_stereo"] >= 50 and out["n_pnp"] >= 5, (out["n_stereo"], out["n_pnp"])
        rel = np.linalg.inv(poses[i + 1]) @ poses[i]
        assert np.allclose(out["tvec"], rel[:3, 3], atol=0.25)


@pytest.mark.gpu
def test_gpu_tracker_c1_640x480_matches_oracle_chain(c1_seq):
    """VERDICT r3 #1 (C1 = main.py:76-132 at 640x480, 500 kp/frame, a
    2-keyframe window; C1_CAP = 25 per tile gives the 500 kp/frame, DESIGN.md
    §2): the batched Tracker against oracle.pipeline.track_pair per pair --
    ORB counts, stereo / F-LMedS counts and mask, X at 1e-9, temporal count,
    PnP inliers and pose at 1e-8, and the device-chained poses against the host
    chain of the oracle's PnP results (the stale-T rule included)."""
    import torch
    from slam355.pipeline import Tracker, chain_poses

    L, R, poses, rig = c1_seq
    B = 2
    trk = Tracker(B, 480, 640, rig.P_l, rig.P_r, max_kp_per_tile=C1_CAP, seed=4)
    trk.imgs.copy_(torch.from_numpy(np.concatenate([L[:B + 1], R[:B]])))
    rv, tv, n = trk.track(0)
    P = trk.poses.cpu().numpy()
    c = trk.counters()
    assert 450 <= c["orb"].min() and c["orb"].max() <= 520, c["orb"]
    cache = {}
    erv, etv, en = [], [], []
    for i in range(B):
        e = op.track_pair(L[i], R[i], L[i + 1], rig.P_l, rig.P_r, max_kp=C1_CAP, seed=4, frame=i,
                          orb_cache=cache)
        assert c["orb"][i] == len(cache[("L", i)][0]), i
        assert c["orb"][B + 1 + i] == len(cache[("R", i)][0]), i
        assert c["stereo"][i] == e["n_stereo"] and c["f_inliers"][i] == e["n_f"], i
        assert np.array_equal(trk.f_mask[i, :e["n_stereo"]].cpu().numpy().astype(bool), e["f_mask"])
        X = trk.X[i, :e["n_f"]].cpu().numpy()
        assert np.all(np.abs(X - e["X"]) <= 1e-9 * np.maximum(1, np.abs(e["X"])))
        assert c["temporal"][i] == e["n_temporal"], i
        assert int(n[i]) == e["n_pnp"], i
        assert np.allclose(rv[i].cpu().numpy(), e["rvec"], rtol=0, atol=1e-8)
        assert np.allclose(tv[i].cpu().numpy(), e["tvec"], rtol=0, atol=1e-8)
        erv.append(e["rvec"]), etv.append(e["tvec"]), en.append(e["n_pnp"])
    Ph, _ = chain_poses(np.eye(4), np.array(erv), np.array(etv), np.array(en))
    assert np.allclose(P, Ph, rtol=0, atol=1e-8)
    gt = np.stack([np.linalg.inv(poses[0]) @ poses[i + 1] for i in range(B)])
    assert np.abs(P[:, :3, 3] - gt[:, :3, 3]).max() < 0.5
