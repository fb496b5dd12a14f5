"""Relocalization without a GPU: the reference chain on the revisit scene (a
prior-free pose where guided matching from the drifted prior fails),
posegraph.edge_from_localization against finite differences, and the argument
errors of the new entry points.

Bars: the scene bars are those of tests/test_map_life.py (status 0, translation
error < 0.03 m); the edge's linear map agrees with central differences to 1e-6
relative (step 1e-6: truncation ~1e-12, rounding ~1e-10)."""
import ctypes

import numpy as np
import pytest

import guided_ref as gr
import pose_refine_ref as pr
import reloc_ref as rr


def _frame(s, f, **kw):
    return rr.relocalize(s["map"], s["kp"][f], s["desc"][f], s["n_kp"][f], s["P"], 100 + f,
                         prior=s["prior"][f], seed=7, item=f, **kw)


def test_guided_matching_from_the_drifted_prior_fails():
    s = rr.revisit_scene()
    m = s["map"]
    n = m["n"]
    for f in range(s["nviews"]):
        uv, _ = gr.project(m["X"][:n], s["prior"][f], s["P"], s["W"], s["H"], 0.0, 0.1)
        i2, d2, g = gr.window_knn2(m["desc"][:n], uv, np.full(n, 15.0, np.float32), s["desc"][f],
                                   s["kp"][f], s["n_kp"][f], s["W"], s["H"], 64, (7, 10))
        _, good = gr.unique(i2, d2, g, s["cap"])
        rows = gr.track_rows(i2, good, s["kp"][f], f)
        out = pr.refine(rows, len(rows), m["X"], s["prior"][f], s["P"], min_inliers=10, **rr.REFINE)
        print(f"frame {f}: guided rows {len(rows)}, status {out['status']}")
        assert out["status"] != 0


def test_reference_chain_relocalizes():
    s = rr.revisit_scene()
    m = s["map"]
    alive = int((~np.isnan(m["X"][:m["n"], 0])).sum())
    print(f"map: {m['n']} slots, {alive} alive")
    for f in range(s["nviews"]):
        o = _frame(s, f)
        ref = o["refined"]
        terr = np.linalg.norm(ref["pose"][:3, 3] - s["true"][f, :3, 3])
        imp = s["kind"][f][o["owner"][o["rows"][:, 1].astype(int)]] == 2
        print(f"frame {f}: {int((s['kind'][f] == 0).sum())} in view, rows {len(o['rows'])}, "
              f"PnP inliers {o['pnp'][2]}, refined inliers {ref['ninl']}, impostor rows {int(imp.sum())}, "
              f"translation error {terr:.4f}, margin {ref['margin']:.2e}")
        assert ref["status"] == 0 and terr < 0.03
        assert not ref["mask"][imp].any()                 # every impostor row is rejected
        assert ref["margin"] > 1e-6
    # clutter only: the prior comes back bit for bit at status 1
    o = _frame(s, s["nf"] - 1)
    assert o["count"] == 0 and o["refined"]["status"] == 1
    assert np.array_equal(o["refined"]["pose"].view(np.uint64), s["prior"][-1].view(np.uint64))


def test_last_range_limits_the_landmarks():
    s = rr.revisit_scene()
    m = s["map"]
    for f in range(s["nviews"]):
        o = _frame(s, f, lo=0, hi=8)
        l = o["rows"][:, 1].astype(int)
        terr = np.linalg.norm(o["refined"]["pose"][:3, 3] - s["true"][f, :3, 3])
        print(f"frame {f}: rows {len(l)} with last in [0, 8), status {o['refined']['status']}, "
              f"translation error {terr:.4f}")
        assert len(l) > 0 and (m["last"][l] < 8).all() and (m["last"][l] >= 0).all()
        assert len(l) < len(_frame(s, f)["rows"])


# ----------------------------------------------------------------------------- the edge
def _rand_pose(rng):
    from slam355 import posegraph as pg

    T = np.eye(4)
    T[:3, :3] = pg._so3_exp(rng.normal(0, 0.8, 3))
    T[:3, 3] = rng.normal(0, 5.0, 3)
    return T


def _spd(rng):
    A = rng.normal(0, 1, (6, 6))
    return A @ A.T * 1e3 + np.eye(6)


def _perturbed(T, d):
    """The camera-to-world pose after X_cam <- Exp(dw) X_cam + dv."""
    from slam355 import posegraph as pg

    Rc, tc = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
    E = pg._so3_exp(d[:3])
    Rn, tn = E @ Rc, E @ tc + d[3:]
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = Rn.T, -Rn.T @ tn
    return out


@pytest.mark.parametrize("seed", range(6))
def test_edge_map_against_central_differences(seed):
    from slam355 import posegraph as pg

    rng = np.random.default_rng(seed)
    T, info = _rand_pose(rng), _spd(rng)
    Tr = _rand_pose(rng)
    x_ref = np.concatenate([pg._so3_log(Tr[:3, :3].T), -Tr[:3, :3].T @ Tr[:3, 3]])
    meas, W, L = pg.edge_from_localization(x_ref, T, info, return_map=True)
    Rt = T[:3, :3].T
    x_cur = np.concatenate([pg._so3_log(Rt), -Rt @ T[:3, 3]])
    assert np.allclose(meas, pg.relative_pose(x_ref, x_cur), rtol=0, atol=1e-14)
    h, fd = 1e-6, np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        zp = pg.edge_from_localization(x_ref, _perturbed(T, d), info)[0]
        zm = pg.edge_from_localization(x_ref, _perturbed(T, -d), info)[0]
        fd[:, k] = (zp - zm) / (2 * h)
    err = np.abs(L - fd).max() / np.abs(fd).max()
    print(f"seed {seed}: linear map vs central differences {err:.2e}")
    assert err <= 1e-6
    assert np.array_equal(W, W.T) and np.linalg.eigvalsh(W).min() > 0
    assert np.allclose(np.linalg.inv(W), L @ np.linalg.inv(info) @ L.T, rtol=1e-8, atol=0)


def test_edge_batched_and_errors():
    from slam355 import posegraph as pg

    rng = np.random.default_rng(9)
    T = np.stack([_rand_pose(rng) for _ in range(3)])
    info = np.stack([_spd(rng) for _ in range(3)])
    x_ref = rng.normal(0, 0.5, (3, 6))
    meas, W = pg.edge_from_localization(x_ref, T, info)
    assert meas.shape == (3, 6) and W.shape == (3, 6, 6)
    for b in range(3):
        one = pg.edge_from_localization(x_ref[b], T[b], info[b])
        assert np.array_equal(one[0], meas[b]) and np.array_equal(one[1], W[b])
    bad = info[0].copy()
    bad[2, 2] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        pg.edge_from_localization(x_ref[0], T[0], bad)
    with pytest.raises(np.linalg.LinAlgError):
        pg.edge_from_localization(x_ref[0], T[0], np.zeros((6, 6)))
    with pytest.raises(ValueError):
        pg.edge_from_localization(x_ref[:2], T, info)


# ----------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu():
    from slam355 import _lib, matcher

    L = _lib.lib
    err = lambda: L.slam_last_error()  # noqa: E731
    buf = (ctypes.c_double * 64)()       # never read: every call below is refused before any GPU call
    q = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q2 = ctypes.c_void_p(q.value + 64)

    def each_null(call, names):
        for k, name in enumerate(names):
            ptrs = [q] * len(names)
            ptrs[k] = None
            assert call(ptrs=ptrs) == -1 and name.encode() in err(), name

    S = matcher.MAP_KNN_SEGMENT
    assert S == L.slam_hamming_map_segment() and 8 <= S <= 16384
    nb = ctypes.c_size_t(0)
    assert L.slam_hamming_map_workspace_bytes(3, 100, 3 * S + 5, ctypes.byref(nb)) == 0
    assert nb.value == 3 * 4 * 100 * 8
    assert L.slam_hamming_map_workspace_bytes(3, 100, 10, None) == -1 and b"bytes" in err()
    for bad in (0, 65536):
        assert L.slam_hamming_map_workspace_bytes(bad, 100, 10, ctypes.byref(nb)) == -1 and b"batch" in err()
        assert L.slam_hamming_map_workspace_bytes(3, bad, 10, ctypes.byref(nb)) == -1 and b"q_cap" in err()
    for bad in (0, (1 << 20) + 1):
        assert L.slam_hamming_map_workspace_bytes(3, 100, bad, ctypes.byref(nb)) == -1 and b"x_cap" in err()

    knn_names = ["d_q", "d_nq", "d_desc", "d_X", "d_last", "d_n", "d_range", "d_idx2", "d_dist2",
                 "d_good", "d_ws"]

    def knn(q_cap=100, x_cap=500, batch=2, max_dist=64, ratio=(7, 10), ws=1 << 30, ptrs=(q,) * 11):
        p = list(ptrs)
        return L.slam_hamming_map_knn2(p[0], p[1], q_cap, p[2], p[3], p[4], p[5], x_cap, p[6], batch,
                                       max_dist, ratio[0], ratio[1], p[7], p[8], p[9], p[10], ws, None)
    each_null(knn, knn_names)
    for bad in (0, 65536):
        assert knn(batch=bad) == -1 and b"batch" in err()
        assert knn(q_cap=bad) == -1 and b"q_cap" in err()
    for bad in (0, (1 << 20) + 1):
        assert knn(x_cap=bad) == -1 and b"x_cap" in err()
    for bad in (-1, 257):
        assert knn(max_dist=bad) == -1 and b"max_dist" in err()
    for bad in ((0, 10), (11, 10), (-1, 10), (7, 0)):
        assert knn(ratio=bad) == -1 and b"ratio" in err()
    assert knn(ws=2 * 100 * 8 - 1) == -1 and b"ws_bytes" in err() and b"1600" in err()
    odd = ctypes.c_void_p(q.value + 8)
    assert knn(ptrs=[odd] + [q] * 10) == -1 and b"d_q" in err() and b"aligned" in err()
    assert knn(ptrs=[q, q, odd] + [q] * 8) == -1 and b"d_desc" in err() and b"aligned" in err()

    rows_names = ["d_owner", "d_n", "d_kp", "d_X", "d_rows", "d_count", "d_Q", "d_q"]

    def rows(x_cap=50, kp_cap=20, batch=2, rows_cap=20, ptrs=(q,) * 8):
        p = list(ptrs)
        return L.slam_reloc_rows(p[0], p[1], x_cap, p[2], kp_cap, p[3], batch, 0, rows_cap, p[4], p[5],
                                 p[6], p[7], None)
    each_null(rows, rows_names)
    for bad in (0, 65536):
        assert rows(batch=bad) == -1 and b"batch" in err()
    for bad in (0, (1 << 20) + 1):
        assert rows(x_cap=bad, rows_cap=1 << 20) == -1 and b"x_cap" in err()
        assert rows(kp_cap=bad, rows_cap=1 << 20) == -1 and b"kp_cap" in err()
    assert rows(rows_cap=19) == -1 and b"rows_cap" in err()
    assert rows(x_cap=10, rows_cap=9) == -1 and b"rows_cap" in err()

    pose_names = ["d_rvec", "d_tvec", "d_ninl", "d_count", "d_P", "d_poses", "d_count_out"]

    def pose(batch=2, min_inliers=10, prior=None, ptrs=(q,) * 5 + (q2, q2)):
        p = list(ptrs)
        return L.slam_reloc_pose(p[0], p[1], p[2], p[3], p[4], prior, batch, min_inliers, p[5], p[6], None)
    each_null(pose, pose_names)
    for bad in (0, 65536):
        assert pose(batch=bad) == -1 and b"batch" in err()
    assert pose(min_inliers=-1) == -1 and b"min_inliers" in err()
    assert pose(prior=q2) == -1 and b"alias" in err()
