"""Landmark life cycle: slam_map_score / spawn / cull / compact / slam_rows_remap and
LandmarkMap.score / spawn / cull / compact / step against tests/map_life_ref.py (a
NumPy restatement of the header's definitions), and what the cycle is for: a map
that follows the camera.

Bars: everything is integer or copied data and must be bit-exact, except the
world point a spawn computes (three products and three sums in f64, stated
left to right and built without contraction): within 1 ulp, observed distance
printed.  The scene bars (status 0, >= 200 rows, translation error < 0.03 m,
clutter culled, no landmark twice) are met by the CPU reference chain first."""
import ctypes
import functools

import numpy as np
import pytest

import guided_ref as gr
import map_life_ref as ml
import pose_refine_ref as pr

W, H = 640, 480
P3 = np.array([[500.0, 0, 320.0, 0], [0, 500.0, 240.0, 0], [0, 0, 1.0, 0]])
GATE = 2.4477
RADIUS = (15.0, 5.0)
MAX_DIST, RATIO = 64, (7, 10)
Z_RANGE = (0.1, 70.0)
CULL = dict(min_visible=4, ratio=(1, 4), age=4, min_found=2)


# ----------------------------------------------------------------------------- scene
def _flip(rng, d, nbits):
    bits = np.unpackbits(d, axis=-1)
    for row in bits.reshape(-1, 256):
        row[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(bits, axis=-1)


def _yaw_pose(x, yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[0, 3] = x
    return T


@functools.lru_cache(maxsize=None)
def _scene():
    """800 landmarks along a 22 m run of 16 frames (1.5 m and 0.01 rad of yaw per
    frame), predictions 0.1 m / 0.004 rad off.  A frame's keypoints are its visible
    landmarks (+-1 px, 20 flipped descriptor bits) and 40 clutter keypoints with
    random descriptors at the projections of random frustum points; every keypoint
    comes with its camera-frame point, as stereo triangulation would give it."""
    rng = np.random.default_rng(31)
    nl, nf, cap, B, nclutter = 800, 16, 448, 4, 40
    X = np.stack([rng.uniform(-7, 31, nl), rng.uniform(-4, 4, nl), rng.uniform(6, 20, nl)], 1)
    D = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
    true = np.stack([_yaw_pose(1.5 * f, 0.01 * f) for f in range(nf)])
    pred = np.stack([_yaw_pose(1.5 * f + 0.1, 0.01 * f + 0.004) for f in range(nf)])
    kp = np.zeros((nf, cap, 5), np.float32)
    desc = np.zeros((nf, cap, 32), np.uint8)
    n_kp = np.zeros(nf, np.int32)
    truth = np.full((nf, cap), -1, np.int64)            # keypoint -> true landmark, -1 clutter
    Xc = np.zeros((nf, cap, 3))
    pairs = np.full((nf, cap, 2), -1, np.int32)
    for f in range(nf):
        uv, _ = gr.project(X, true[f], P3, W, H, 2.0, 0.1)    # the pixel noise stays inside
        vis = np.nonzero(~np.isnan(uv[:, 0]))[0]
        pts = uv[vis].astype(np.float64) + rng.uniform(-1.0, 1.0, (len(vis), 2))
        cam = (X[vis] - true[f, :3, 3]) @ true[f, :3, :3]
        z = rng.uniform(6.0, 20.0, nclutter)
        clutter = np.stack([rng.uniform(-0.6, 0.6, nclutter) * z, rng.uniform(-0.45, 0.45, nclutter) * z, z], 1)
        pts = np.r_[pts, clutter[:, :2] / clutter[:, 2:] * 500.0 + (320.0, 240.0)]
        cam = np.r_[cam, clutter]
        des = np.r_[_flip(rng, D[vis], 20), rng.integers(0, 256, (nclutter, 32), dtype=np.uint8)]
        lm = np.r_[vis, np.full(nclutter, -1)]
        order = rng.permutation(len(pts))
        m = len(pts)
        assert m <= cap
        kp[f, :m, :2], desc[f, :m], truth[f, :m], n_kp[f] = pts[order], des[order], lm[order], m
        stereo = rng.permutation(m)                     # the stereo pairs come in no particular order
        Xc[f, :m], pairs[f, :m, 0], pairs[f, :m, 1] = cam[order][stereo], stereo, stereo
    vis0 = np.sort(truth[0, :n_kp[0]][truth[0, :n_kp[0]] >= 0])
    keyframe = np.zeros(nf, np.uint8)
    keyframe[B - 1::B] = 1                              # the last frame of every batch
    return dict(X=X, D=D, true=true, pred=pred, kp=kp, desc=desc, n_kp=n_kp, truth=truth, Xc=Xc,
                pairs=pairs, count=n_kp.copy(), keyframe=keyframe, vis0=vis0, cap=cap, nl=nl, nf=nf,
                B=B, x_cap=1024, rows_cap=cap)


def _start_map(s):
    return ml.add(ml.new_map(s["x_cap"]), s["X"][s["vis0"]], s["D"][s["vis0"]], 0)


def _match(s, m, f, uv, radius):
    """Steps 3-5 of guided matching for frame f -> (rows, owner, good [n])."""
    n = m["n"]
    i2, d2, g = gr.window_knn2(m["desc"][:n], uv[:n], np.full(n, radius, np.float32), s["desc"][f],
                               s["kp"][f], s["n_kp"][f], W, H, MAX_DIST, RATIO)
    owner, good = gr.unique(i2, d2, g, s["cap"])
    return gr.track_rows(i2, good, s["kp"][f], f), owner, good


def _refine(m, rows, pose):
    return pr.refine(rows, len(rows), m["X"], pose, P3, loss=1, loss_scale=GATE, gate=GATE,
                     min_depth=0.1, n_rounds=4, iters=10, min_inliers=10)


def _localize_ref(s, m, f):
    """LandmarkMap.localize for one frame on the CPU -> (second refinement, rows, owner, good, uv)."""
    n = m["n"]
    uv, _ = gr.project(m["X"][:n], s["pred"][f], P3, W, H, 0.0, 0.1)
    one = _refine(m, _match(s, m, f, uv, RADIUS[0])[0], s["pred"][f])
    uv, _ = gr.project(m["X"][:n], one["pose"], P3, W, H, 0.0, 0.1)
    rows, owner, good = _match(s, m, f, uv, RADIUS[1])
    return _refine(m, rows, one["pose"]), rows, owner, good, uv


def _pad(s, m, uvs, goods, rows_l, owners):
    """Per-frame results -> the batch arrays the device keeps."""
    B, n = len(uvs), m["n"]
    uv = np.full((B, s["x_cap"], 2), np.nan, np.float32)
    good = np.zeros((B, s["x_cap"]), np.uint8)
    rows = np.zeros((B, s["rows_cap"], 4))
    count = np.zeros(B, np.int32)
    for b in range(B):
        uv[b, :n], good[b, :n] = uvs[b], goods[b]
        rows[b, :len(rows_l[b])], count[b] = rows_l[b], len(rows_l[b])
    return uv, good, rows, count, np.stack(owners)


def _life_ref(s, m, f0, uv, good, rows, count, owner, poses, status):
    """score, spawn and cull of the batch that starts at frame f0, as LandmarkMap.step
    orders them -> (map, owner, rows, count, spawned, dropped, nculled)."""
    B = s["B"]
    fr = slice(f0, f0 + B)
    m = ml.score(m, uv, good, np.full(B, m["n"]), f0)
    flags = (s["keyframe"][fr] != 0) & (np.asarray(status) == 0)
    m, owner, rows, count, spawned, dropped = ml.spawn(
        m, s["Xc"][fr], s["pairs"][fr], s["count"][fr], s["kp"][fr], s["desc"][fr], s["n_kp"][fr],
        owner, poses, flags, *Z_RANGE, f0, rows, count)
    m, nculled = ml.cull(m, f0 + B - 1, **CULL)
    return m, owner, rows, count, spawned, dropped, nculled


def _origins(s, origin, f0, owner0, owner1):
    """The true landmark (-1: clutter) behind every map slot, after a spawn."""
    origin = origin.copy()
    for b in range(s["B"]):
        for j in np.nonzero(owner0[b] != owner1[b])[0]:
            origin[owner1[b, j]] = s["truth"][f0 + b, j]
    return origin


def _check_cycle(s, m, origin, now):
    """What the cycle promises about the map after the cull at `now`."""
    n = m["n"]
    alive = ~np.isnan(m["X"][:n, 0])
    old_clutter = (origin[:n] < 0) & (now - m["born"][:n] >= CULL["age"])
    assert not (alive & old_clutter).any()
    true_alive = origin[:n][alive & (origin[:n] >= 0)]
    assert len(np.unique(true_alive)) == len(true_alive)
    return int(alive.sum()), int(len(true_alive))


@functools.lru_cache(maxsize=None)
def _reference_run(grow):
    s = _scene()
    m = _start_map(s)
    origin = np.full(s["x_cap"], -2, np.int64)
    origin[:m["n"]] = s["vis0"]
    status, nrows, terr, sizes = [], [], [], []
    for f0 in range(0, s["nf"], s["B"]):
        res = [_localize_ref(s, m, f) for f in range(f0, f0 + s["B"])]
        for b, (two, rows, _, _, _) in enumerate(res):
            status.append(two["status"])
            nrows.append(len(rows))
            terr.append(np.linalg.norm(two["pose"][:3, 3] - s["true"][f0 + b, :3, 3]))
        if not grow:
            continue
        uv, good, rows, count, owner = _pad(s, m, [r[4] for r in res], [r[3] for r in res],
                                            [r[1] for r in res], [r[2] for r in res])
        poses = np.stack([r[0]["pose"] for r in res])
        m, owner1, *_ = _life_ref(s, m, f0, uv, good, rows, count, owner, poses, status[-s["B"]:])
        origin = _origins(s, origin, f0, owner, owner1)
        sizes.append((m["n"],) + _check_cycle(s, m, origin, f0 + s["B"] - 1))
    return dict(status=status, rows=nrows, terr=terr, sizes=sizes, map=m)


# ----------------------------------------------------------------------------- CPU
def test_reference_fixed_map_loses_the_camera():
    r = _reference_run(False)
    print("fixed map: rows per frame", r["rows"], "status", r["status"])
    assert r["rows"][0] == len(_scene()["vis0"]) and r["status"][:8] == [0] * 8
    assert r["status"][-3:] == [1, 1, 1]


def test_reference_cycle_follows_the_camera():
    r = _reference_run(True)
    print("cycle: rows per frame", r["rows"], "\n translation error", np.round(r["terr"], 4),
          "\n (slots, alive, true alive) after each batch", r["sizes"])
    assert r["status"] == [0] * 16
    assert min(r["rows"]) >= 200
    assert max(r["terr"]) < 0.03
    assert r["sizes"][-1][0] > len(_scene()["vis0"])         # the clutter and twice checks ran in _check_cycle


def test_argument_errors_without_gpu():
    from slam355 import _lib

    L = _lib.lib
    err = lambda: L.slam_last_error()  # noqa: E731
    buf = (ctypes.c_double * 64)()       # never read: every call below is refused before any GPU call
    q = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def each_null(call, names):
        for k, name in enumerate(names):
            ptrs = [q] * len(names)
            ptrs[k] = None
            assert call(ptrs=ptrs) == -1 and name.encode() in err(), name

    def score(x_cap=10, batch=2, ptrs=(q,) * 6):
        uv, good, nq, vis, found, last = ptrs
        return L.slam_map_score(uv, good, nq, x_cap, batch, 0, vis, found, last, None)
    each_null(score, ["d_uv", "d_good", "d_nq", "d_visible", "d_found", "d_last"])
    for bad in (0, -1, (1 << 20) + 1):
        assert score(x_cap=bad) == -1 and b"x_cap" in err()
    for bad in (0, 65536):
        assert score(batch=bad) == -1 and b"batch" in err()

    nb = ctypes.c_size_t(0)
    assert L.slam_map_spawn_workspace_bytes(4, 100, ctypes.byref(nb)) == 0 and nb.value >= 4 * 100 * 4
    assert L.slam_map_spawn_workspace_bytes(1025, 100, ctypes.byref(nb)) == -1 and b"batch" in err()
    assert L.slam_map_spawn_workspace_bytes(4, 70000, ctypes.byref(nb)) == -1 and b"kp_cap" in err()
    assert L.slam_map_spawn_workspace_bytes(4, 100, None) == -1 and b"bytes" in err()

    spawn_names = ["d_Xc", "d_pairs", "d_count", "d_kp", "d_kp_desc", "d_nkp", "d_owner", "d_poses",
                   "d_spawn", "d_X", "d_desc", "d_visible", "d_found", "d_born", "d_last", "d_n",
                   "d_rows", "d_rows_count", "d_spawned", "d_dropped", "d_ws"]

    def spawn(p_cap=30, kp_cap=20, batch=2, x_cap=50, rows_cap=20, z=(0.1, 70.0), ws=1 << 20,
              ptrs=(q,) * 21):
        p = list(ptrs)
        return L.slam_map_spawn(p[0], p[1], p[2], p_cap, p[3], p[4], p[5], kp_cap, p[6], p[7], p[8],
                                batch, z[0], z[1], 0, p[9], p[10], p[11], p[12], p[13], p[14], p[15],
                                x_cap, p[16], p[17], rows_cap, p[18], p[19], p[20], ws, None)
    each_null(spawn, spawn_names)
    for bad in (0, 1025):
        assert spawn(batch=bad) == -1 and b"batch" in err()
    for bad in (0, (1 << 20) + 1):
        assert spawn(p_cap=bad) == -1 and b"p_cap" in err()
        assert spawn(x_cap=bad, rows_cap=1 << 20) == -1 and b"x_cap" in err()
    for bad in (0, 65536):
        assert spawn(kp_cap=bad, rows_cap=65536) == -1 and b"kp_cap" in err()
    assert spawn(rows_cap=19) == -1 and b"rows_cap" in err()
    assert spawn(x_cap=10, rows_cap=9) == -1 and b"rows_cap" in err()
    for bad in ((70.0, 0.1), (1.0, 1.0), (float("nan"), 1.0), (0.1, float("nan"))):
        assert spawn(z=bad) == -1 and b"z_min" in err()
    assert spawn(ws=8) == -3 and b"ws_size" in err()
    odd = ctypes.c_void_p(q.value + 8)
    assert spawn(ptrs=[q] * 4 + [odd] + [q] * 16) == -1 and b"d_kp_desc" in err() and b"aligned" in err()

    def cull(x_cap=10, num=1, den=4, ptrs=(q,) * 6):
        X, vis, found, born, n, nc = ptrs
        return L.slam_map_cull(X, vis, found, born, n, x_cap, 7, 4, num, den, 4, 2, nc, None)
    each_null(cull, ["d_X", "d_visible", "d_found", "d_born", "d_n", "d_nculled"])
    assert cull(x_cap=0) == -1 and b"x_cap" in err()
    assert cull(num=-1) == -1 and b"ratio" in err()
    assert cull(den=0) == -1 and b"ratio" in err()

    q2 = ctypes.c_void_p(q.value + 64)
    compact_names = ["d_X", "d_desc", "d_visible", "d_found", "d_born", "d_last", "d_n", "d_X_out",
                     "d_desc_out", "d_visible_out", "d_found_out", "d_born_out", "d_last_out",
                     "d_remap", "d_n_out"]

    def compact(x_cap=10, ptrs=(q,) * 7 + (q2,) * 8):
        return L.slam_map_compact(*ptrs[:7], x_cap, *ptrs[7:], None)
    each_null(compact, compact_names)
    assert compact(x_cap=0) == -1 and b"x_cap" in err()
    assert compact(ptrs=(q,) * 15) == -1 and b"alias" in err()
    assert compact(ptrs=(q,) * 7 + (q2,) * 7 + (q,)) == -1 and b"d_n_out" in err()

    def remap(rows_cap=10, batch=2, x_cap=10, ptrs=(q, q, q, q2, q2)):
        rows, count, rm, out, cout = ptrs
        return L.slam_rows_remap(rows, count, rows_cap, batch, rm, x_cap, out, cout, None)
    each_null(remap, ["d_rows", "d_count", "d_remap", "d_rows_out", "d_count_out"])
    for bad in (0, 65536):
        assert remap(batch=bad) == -1 and b"batch" in err()
        assert remap(rows_cap=bad) == -1 and b"rows_cap" in err()
    assert remap(x_cap=0) == -1 and b"x_cap" in err()
    assert remap(ptrs=(q,) * 5) == -1 and b"alias" in err()


# ----------------------------------------------------------------------------- GPU
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}.get(a.dtype.itemsize, a.dtype))


def _same(a, b):
    """Bit for bit (NaN payloads aside: every NaN here is the one quiet NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _random_map(rng, cap, n, dead=0.0):
    m = ml.new_map(cap)
    m["X"][:] = rng.normal(0, 5, (cap, 3))
    m["desc"][:] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    for k in ml.FIELDS[2:]:
        m[k][:] = rng.integers(0, 50, cap)
    m["X"][rng.random(cap) < dead] = np.nan
    m["n"] = n
    return m


def _map_to_dev(m):
    return {k: _dev(m[k]) for k in ml.FIELDS} | {"n": _dev(np.array([m["n"]], np.int32))}


def _map_from_dev(d):
    return {k: d[k].cpu().numpy() for k in ml.FIELDS} | {"n": int(d["n"].item())}


def _assert_maps_equal(got, want, upto=None):
    """Bit-exact on the slots in use (upto, default the whole arrays)."""
    assert got["n"] == want["n"]
    for k in ml.FIELDS:
        assert _same(got[k][:upto], want[k][:upto]), k


@pytest.mark.gpu
@pytest.mark.parametrize("x_cap", [1, 255, 256, 257, 1025])
def test_score_against_reference(x_cap):
    from slam355 import _lib
    from slam355.device import ptr

    rng = np.random.default_rng(x_cap)
    B = 3
    nq = np.array([x_cap, x_cap // 2, -3], np.int32)
    uv = rng.uniform(0, 600, (B, x_cap, 2)).astype(np.float32)
    uv[rng.random((B, x_cap)) < 0.4] = np.nan
    good = (rng.random((B, x_cap)) < 0.5).astype(np.uint8)
    good[np.isnan(uv[..., 0])] = 0
    for b in range(B):                      # stale entries that would count if they were read
        k = max(int(nq[b]), 0)
        uv[b, k:], good[b, k:] = 7.0, 1
    m = _random_map(rng, x_cap, x_cap)
    m["last"][:] = rng.integers(0, 14, x_cap)            # frames 10..12: some later, some earlier
    want = ml.score(m, uv, good, nq, 10)
    d = _map_to_dev(m)
    ins = [_dev(uv), _dev(good), _dev(nq)]               # kept alive over the call
    _lib.call("slam_map_score", ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), x_cap, B, 10,
              ptr(d["visible"]), ptr(d["found"]), ptr(d["last"]), None)
    _assert_maps_equal(_map_from_dev(d), want)
    assert (want["visible"] != m["visible"]).any() or x_cap == 1


SPAWN_COUNTS = [0, 1, 63, 64, 65, 256, 257, 300, 400, -2]


@functools.lru_cache(maxsize=None)
def _spawn_case(wide=False):
    """wide: three frames of 2049, 2100 and 1025 entries (three and two chunks of
    the 1024-lane workgroup), most of them candidates."""
    rng = np.random.default_rng(67)
    B, p_cap, kp_cap, x_cap = (3, 2100, 2100, 2200) if wide else (67, 300, 350, 1500)
    counts = [2049, 2100, 1025] if wide else SPAWN_COUNTS
    count = np.array([counts[b % len(counts)] for b in range(B)], np.int32)
    flags = (rng.random(B) < 0.7).astype(np.uint8)
    flags[:len(counts)] = 1
    nkp = rng.integers(200, kp_cap + 1, B).astype(np.int32)
    if wide:
        nkp[:] = kp_cap
    else:
        flags[[12, 13, 40]] = 0
        flags[41] = 2                                    # any non-zero value is a keyframe
        nkp[5], nkp[6], nkp[7] = -1, kp_cap + 9, 0
    z = rng.uniform(1.0, 60.0, (B, p_cap))
    Xc = np.stack([rng.uniform(-0.6, 0.6, (B, p_cap)) * z, rng.uniform(-0.4, 0.4, (B, p_cap)) * z, z], 2)
    kind = rng.integers(0, 20, (B, p_cap))
    Xc[kind == 0, rng.integers(0, 3, (kind == 0).sum())] = np.nan
    Xc[kind == 1, rng.integers(0, 3, (kind == 1).sum())] = np.inf
    Xc[kind == 2, 2] = Z_RANGE[0]                        # exactly z_min and exactly z_max: excluded
    Xc[kind == 3, 2] = Z_RANGE[1]
    Xc[kind == 4, 2] = -5.0
    Xc[kind == 5, 2] = np.nextafter(Z_RANGE[1], 0.0)     # one step inside: included
    pairs = rng.integers(-1, kp_cap + 5, (B, p_cap, 2)).astype(np.int32)
    pairs[:, :, 0] = np.where(rng.random((B, p_cap)) < 0.5, pairs[:, :, 0] % 120, pairs[:, :, 0])
    if wide:                                             # nine entries in ten name a keypoint of their own
        own = np.stack([rng.permutation(kp_cap)[:p_cap] for _ in range(B)])
        pairs[:, :, 0] = np.where(rng.random((B, p_cap)) < 0.9, own, pairs[:, :, 0])
    owner = np.where(rng.random((B, kp_cap)) < 0.3, rng.integers(0, 1000, (B, kp_cap)), -1).astype(np.int32)
    kp = rng.uniform(0, 600, (B, kp_cap, 5)).astype(np.float32)
    desc = rng.integers(0, 256, (B, kp_cap, 32), dtype=np.uint8)
    poses = np.stack([_yaw_pose(0.3 * b, 0.02 * b) @ _yaw_pose(0.0, 0.1) for b in range(B)])
    poses[:, 1, 3] = rng.uniform(-1, 1, B)
    poses[:, 2, 3] = rng.uniform(-1, 1, B)
    rows = rng.uniform(0, 100, (B, kp_cap, 4))
    rows_count = rng.integers(0, 40, B).astype(np.int32)
    return dict(B=B, p_cap=p_cap, kp_cap=kp_cap, x_cap=x_cap, count=count, flags=flags, nkp=nkp, Xc=Xc,
                pairs=pairs, owner=owner, kp=kp, desc=desc, poses=poses, rows=rows,
                rows_count=rows_count, map=_random_map(rng, x_cap, 0))


def _ulp_distance(a, b):
    """Largest distance in units of the last place over finite a, b of equal sign pattern."""
    ia, ib = a.view(np.int64), b.view(np.int64)
    return int(np.abs(ia - ib).max()) if a.size else 0


@pytest.mark.gpu
@pytest.mark.parametrize("n0,wide", [pytest.param(0, False, id="0"), pytest.param(5, False, id="5"),
                                     pytest.param(1490, False, id="1490"),
                                     pytest.param(1500, False, id="1500"),
                                     pytest.param(0, True, id="wide")])
def test_spawn_against_reference(n0, wide):
    import torch
    from slam355 import _lib
    from slam355.device import ptr

    c = _spawn_case(wide)
    B, x_cap = c["B"], c["x_cap"]
    m = ml.copy_map(c["map"])
    m["n"] = n0
    want, owner, rows, rows_count, spawned, dropped = ml.spawn(
        m, c["Xc"], c["pairs"], c["count"], c["kp"], c["desc"], c["nkp"], c["owner"], c["poses"],
        c["flags"], *Z_RANGE, 100, c["rows"], c["rows_count"])
    total = int(spawned.sum()) + dropped
    assert total > x_cap                                   # from n0 = 0 on, acceptance ends inside a frame
    cut = np.nonzero(np.cumsum(spawned) == spawned.sum())[0][0]
    print(f"n0 {n0}: {total} candidates, {int(spawned.sum())} accepted, {dropped} dropped, last accepting frame {cut}")
    d = _map_to_dev(m)
    nb = ctypes.c_size_t(0)
    _lib.call("slam_map_spawn_workspace_bytes", B, c["kp_cap"], ctypes.byref(nb))
    ws = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device="cuda")
    d_owner, d_rows, d_rc = _dev(c["owner"]), _dev(c["rows"]), _dev(c["rows_count"])
    d_spawned = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    d_dropped = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ins = [_dev(c[k]) for k in ("Xc", "pairs", "count", "kp", "desc", "nkp", "poses", "flags")]
    _lib.call("slam_map_spawn", ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), c["p_cap"], ptr(ins[3]),
              ptr(ins[4]), ptr(ins[5]), c["kp_cap"], ptr(d_owner), ptr(ins[6]), ptr(ins[7]), B,
              Z_RANGE[0], Z_RANGE[1], 100, ptr(d["X"]), ptr(d["desc"]), ptr(d["visible"]),
              ptr(d["found"]), ptr(d["born"]), ptr(d["last"]), ptr(d["n"]), x_cap, ptr(d_rows),
              ptr(d_rc), c["kp_cap"], ptr(d_spawned), ptr(d_dropped), ptr(ws), ws.numel(), None)
    got = _map_from_dev(d)
    assert got["n"] == want["n"] == min(n0 + total, x_cap)
    assert _same(d_spawned.cpu().numpy(), spawned) and int(d_dropped.item()) == dropped
    assert _same(d_owner.cpu().numpy(), owner)
    assert _same(d_rc.cpu().numpy(), rows_count) and _same(d_rows.cpu().numpy(), rows)
    for k in ml.FIELDS[1:]:
        assert _same(got[k], want[k]), k
    assert _same(got["X"][:n0], want["X"][:n0]) and _same(got["X"][want["n"]:], want["X"][want["n"]:])
    ulp = _ulp_distance(got["X"][n0:want["n"]], want["X"][n0:want["n"]])
    print(f"n0 {n0}: new X within {ulp} ulp of the reference")
    assert ulp <= 1


@pytest.mark.gpu
def test_cull_against_reference():
    from slam355 import _lib
    from slam355.device import ptr

    now, age, minv, minf, num, den = 20, 4, 4, 2, 1, 4
    # (visible, found, born): each inequality at equality and one step to either side
    cases = [(minv, 0, now), (minv - 1, 0, now), (minv + 1, 0, now),               # visible >= min_visible
             (8, 2, now), (8, 1, now), (9, 2, now), (7, 2, now), (12, 3, now), (13, 3, now),  # den f < num v
             (2, minf - 1, now - age), (2, minf - 1, now - age + 1), (2, minf - 1, now - age - 1),
             (2, minf, now - age), (2, minf + 1, now - age - 3), (2, 0, now + 5),
             (1 << 30, 1 << 28, now), (1 << 30, (1 << 28) - 1, now), (1 << 30, (1 << 28) + 1, now),
             (1 << 30, 1 << 29, now),                       # 4 found = 2^31: a 32-bit product wraps
             (2, 1, -(1 << 31)), (2, 1, (1 << 31) - 1)]     # now - born needs 64 bits as well
    rng = np.random.default_rng(5)
    extra = 700                                           # several workgroups, random fields
    n = 2 * len(cases) + extra
    cap = n + 40
    m = _random_map(rng, cap, n, dead=0.1)
    m["X"][:2 * len(cases)] = 1.0
    for k, (v, f, born) in enumerate(cases):
        for i in (2 * k, 2 * k + 1):
            m["visible"][i], m["found"][i], m["born"][i] = v, f, born
        m["X"][2 * k + 1] = [np.nan, 3.0, 4.0]             # dead already: stays untouched, not counted
    m["visible"][n:], m["found"][n:] = 100, 0              # slots past n: not landmarks
    m["X"][n:] = 2.0
    want, nculled = ml.cull(m, now, minv, (num, den), age, minf)
    expect = [1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    assert [int(np.isnan(want["X"][2 * k, 0])) for k in range(len(cases))] == expect
    d = _map_to_dev(m)
    out = _dev(np.array([-9], np.int32))
    _lib.call("slam_map_cull", ptr(d["X"]), ptr(d["visible"]), ptr(d["found"]), ptr(d["born"]),
              ptr(d["n"]), cap, now, minv, num, den, age, minf, ptr(out), None)
    got = _map_from_dev(d)
    assert int(out.item()) == nculled > len(cases) // 3
    assert np.array_equal(_bits(got["X"]), _bits(want["X"]))   # the dead ones keep their bits
    _assert_maps_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 256, 257, 1025, 3073])
def test_compact_and_remap_against_reference(n):
    import torch
    from slam355 import _lib
    from slam355.device import ptr

    rng = np.random.default_rng(n)
    cap, B, rows_cap = n + 3, 3, 300
    patterns = {"alive": np.zeros(n, bool), "dead": np.ones(n, bool),
                "alternating": np.arange(n) % 2 == 0, "random": rng.random(n) < 0.4}
    for name, dead in patterns.items():
        m = _random_map(rng, cap, n)
        m["X"][:n][dead] = np.nan
        m["X"][n:] = 1.0                                   # alive-looking slots past n
        want, remap = ml.compact(m)
        d = _map_to_dev(m)
        o = _map_to_dev(_random_map(rng, cap, 0))
        d_remap = torch.full((cap,), 77, dtype=torch.int32, device="cuda")
        _lib.call("slam_map_compact", *(ptr(d[k]) for k in ml.FIELDS), ptr(d["n"]), cap,
                  *(ptr(o[k]) for k in ml.FIELDS), ptr(d_remap), ptr(o["n"]), None)
        _assert_maps_equal(_map_from_dev(o), want, upto=want["n"])
        assert _same(d_remap.cpu().numpy(), remap), name
        _assert_maps_equal(_map_from_dev(d), m)            # the source is left alone
        # rows: counts 0, 1 and rows_cap; dead, out-of-range and non-finite landmarks among them
        rows = rng.uniform(0, 600, (B, rows_cap, 4))
        rows[..., 1] = np.sort(rng.integers(0, cap, (B, rows_cap)), axis=1)
        odd = rng.integers(0, 12, (B, rows_cap))
        for k, v in enumerate((-1.0, float(cap), 1e12, np.nan, -0.5, cap - 0.5, -np.inf)):
            rows[..., 1][odd == k] = v
        count = np.array([0, 1, rows_cap], np.int32)
        wrows, wcount = ml.rows_remap(rows, count, remap)
        d_out = torch.full((B, rows_cap, 4), -3.0, dtype=torch.float64, device="cuda")
        d_cnt = torch.full((B,), -3, dtype=torch.int32, device="cuda")
        ins = [_dev(rows), _dev(count)]                    # kept alive over the call
        _lib.call("slam_rows_remap", ptr(ins[0]), ptr(ins[1]), rows_cap, B, ptr(d_remap), cap,
                  ptr(d_out), ptr(d_cnt), None)
        grows, gcount = d_out.cpu().numpy(), d_cnt.cpu().numpy()
        assert _same(gcount, wcount), name
        for b in range(B):
            assert _same(grows[b, :gcount[b]], wrows[b, :gcount[b]]), (name, b)
            assert (grows[b, gcount[b]:] == -3.0).all()


# ----------------------------------------------------------------------------- the map over the sequence
def _new_landmark_map(s):
    from slam355.mapping import LandmarkMap

    return LandmarkMap(s["x_cap"], s["cap"], W, H, P3).add(s["X"][s["vis0"]], s["D"][s["vis0"]])


def _batch_args(s, f0):
    fr = slice(f0, f0 + s["B"])
    return [_dev(s[k][fr]) for k in ("pred", "kp", "desc", "n_kp", "Xc", "pairs", "count", "keyframe")]


def _state(lm):
    return {k: getattr(lm, k).cpu().numpy() for k in ml.FIELDS} | {"n": int(lm.n_dev.item())}


def _step(lm, s, f0):
    res = lm.step(f0, *_batch_args(s, f0), z_range=Z_RANGE, cull=CULL, radius=RADIUS,
                  max_dist=MAX_DIST, ratio=RATIO)
    return [t.cpu().numpy().copy() for t in res]


@pytest.mark.gpu
def test_step_end_to_end():
    """Every batch: rows, owner, counts and the whole landmark state equal the
    reference fed the GPU's own second-pass uv and refined poses; the cycle's
    promises hold on the GPU's results; a map that never grows loses the camera."""
    s = _scene()
    lm = _new_landmark_map(s)
    m = _start_map(s)
    origin = np.full(s["x_cap"], -2, np.int64)
    origin[:m["n"]] = s["vis0"]
    for f0 in range(0, s["nf"], s["B"]):
        _assert_maps_equal(_state(lm), m, upto=m["n"])
        pose, rows, count, mask, ninl, status, info = _step(lm, s, f0)
        uv = lm.uv.cpu().numpy()
        n = m["n"]
        assert (lm._nq.cpu().numpy() == n).all()
        res = [_match(s, m, f0 + b, uv[b], RADIUS[1]) for b in range(s["B"])]
        uvp, good, rows0, count0, owner0 = _pad(s, m, [uv[b, :n] for b in range(s["B"])],
                                                [r[2] for r in res], [r[0] for r in res],
                                                [r[1] for r in res])
        assert _same(lm.good.cpu().numpy()[:, :n], good[:, :n])
        m, owner1, wrows, wcount, spawned, dropped, nculled = _life_ref(
            s, m, f0, uvp, good, rows0, count0, owner0, pose, status)
        origin = _origins(s, origin, f0, owner0, owner1)
        _assert_maps_equal(_state(lm), m, upto=m["n"])
        assert _same(lm.owner.cpu().numpy(), owner1)
        assert _same(count, wcount)
        for b in range(s["B"]):
            assert _same(rows[b, :count[b]], wrows[b, :count[b]]), (f0, b)
        assert _same(lm.spawned.cpu().numpy(), spawned) and int(lm.dropped.item()) == dropped == 0
        assert int(lm.nculled.item()) == nculled
        slots, (alive, true_alive) = m["n"], _check_cycle(s, m, origin, f0 + s["B"] - 1)
        terr = [np.linalg.norm(pose[b, :3, 3] - s["true"][f0 + b, :3, 3]) for b in range(s["B"])]
        print(f"frames {f0}..{f0 + s['B'] - 1}: rows {count0.tolist()}, spawned {int(spawned.sum())}, "
              f"culled {nculled}, slots {slots}, alive {alive} ({true_alive} true), "
              f"translation error {max(terr):.4f}")
        assert (status == 0).all() and count0.min() >= 200 and max(terr) < 0.03
    assert lm.size() == m["n"] and lm.n == m["n"]
    # the same frames against a map that is never grown
    fixed = _new_landmark_map(s)
    status = np.concatenate([fixed.localize(f0, *_batch_args(s, f0)[:4], radius=RADIUS, max_dist=MAX_DIST,
                                            ratio=RATIO)[5].cpu().numpy()
                             for f0 in range(0, s["nf"], s["B"])])
    assert status[-3:].tolist() == [1, 1, 1] and (status[:8] == 0).all()
    assert fixed.n == len(s["vis0"]) and int(fixed.n_dev.item()) == fixed.n


@pytest.mark.gpu
def test_compaction_in_the_middle_changes_nothing_but_the_indices():
    s = _scene()
    a, b = _new_landmark_map(s), _new_landmark_map(s)
    total = None
    for k, f0 in enumerate(range(0, s["nf"], s["B"])):
        ra, rb = _step(a, s, f0), _step(b, s, f0)
        if k >= 2:     # after the compaction: poses, counts, inliers, status, info and masks
            for i in (0, 2, 4, 5, 6):
                assert np.array_equal(_bits(ra[i]), _bits(rb[i])), (f0, i)
            matched = ra[2] - a.spawned.cpu().numpy()      # the rows the refinement saw
            for f in range(s["B"]):
                assert np.array_equal(ra[3][f, :matched[f]], rb[3][f, :matched[f]]), (f0, f)
        if k == 1:
            before = b.size()
            remap = b.compact().cpu().numpy()
            total = remap.copy()
            dead = np.isnan(a.X[:before, 0].cpu().numpy())
            assert b.n == int((~dead).sum()) < before and (remap[:before][dead] == -1).all()
            assert (remap[before:] == -1).all() and int(b.n_dev.item()) == b.n
    # landmarks born after the compaction sit (slots dropped) lower in b
    n_a = a.size()
    shift = before - int((total[:before] >= 0).sum())
    total[before:n_a] = np.arange(before, n_a) - shift
    ta, tb = a.tracks(drop_dead=True), b.tracks(drop_dead=True)
    # b's compaction already dropped the rows of what was dead then, whatever a culled later is dropped in both
    keep = total[ta[:, 1].astype(np.int64)] >= 0
    ta = ta[keep]
    ta[:, 1] = total[ta[:, 1].astype(np.int64)]
    assert len(tb) > 3000 and np.array_equal(ta, tb)
    assert len(a.tracks(drop_dead=False)) > len(a.tracks())


@pytest.mark.gpu
def test_step_in_graph_capture():
    import torch

    s = _scene()
    eager, graphed = _new_landmark_map(s), _new_landmark_map(s)
    _step(eager, s, 0)
    want = _step(eager, s, s["B"])
    _step(graphed, s, 0)                                   # also allocates every buffer
    args = _batch_args(s, s["B"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):    # a host sync or a hipMalloc here fails the capture
        got = graphed.step(s["B"], *args, z_range=Z_RANGE, cull=CULL, radius=RADIUS, max_dist=MAX_DIST,
                           ratio=RATIO)
    for t in got:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in got]
    count = got[2]
    assert np.array_equal(count, want[2]) and count.min() >= 200
    for i in (0, 4, 5, 6):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), i
    spawned = graphed.spawned.cpu().numpy()
    assert _same(spawned, eager.spawned.cpu().numpy()) and spawned.sum() > 0
    for f in range(s["B"]):
        assert np.array_equal(got[1][f, :count[f]], want[1][f, :count[f]])
        matched = count[f] - spawned[f]                    # the rows the refinement saw
        assert np.array_equal(got[3][f, :matched], want[3][f, :matched])
    n = eager.size()
    assert graphed.size() == n > len(s["vis0"])
    _assert_maps_equal(_state(graphed), _state(eager), upto=n)
    assert _same(graphed.owner.cpu().numpy(), eager.owner.cpu().numpy())
