"""Fusing duplicate landmarks: slam_map_fuse / slam_rows_fuse and LandmarkMap.fuse /
step(fuse=...) against tests/map_fuse_ref.py (a NumPy restatement of the header's
definitions), and what fusing is for: a map whose spawn made twins ends up with
one landmark and one track per physical point.

Bars: every output is integer or copied data, so everything is bit-exact.  The
scene bars (no fusion across different truth, no landmark twice in a frame of the
rewritten rows, at most 1 in 10 planted pairs with both twins alive at the end)
are met by the CPU reference chain first, then asserted on the device's result."""
import ctypes
import functools

import numpy as np
import pytest

import guided_ref as gr
import map_fuse_ref as mf
import map_life_ref as ml
import points_refine_ref as pts
import test_map_life as tl

THR = dict(px=3.0, rel_depth=0.125, max_dist=64)


# ----------------------------------------------------------------------------- hand-made states
def _blank(cap, B, kp_cap, n=None, found=None):
    """cap live landmarks at one pixel and one depth with equal descriptors and
    nobody losing anything: every pair planted with _lose passes all thresholds."""
    m = ml.new_map(cap)
    m["X"][:] = 1.0
    m["n"] = cap if n is None else n
    m["visible"][:] = 10 + np.arange(cap)
    m["found"][:] = np.arange(cap, 0, -1) if found is None else found
    m["born"][:] = 20 + 3 * np.arange(cap)
    m["last"][:] = 90 - 2 * np.arange(cap)
    return dict(map=m, uv=np.full((B, cap, 2), 100.0, np.float32), z=np.full((B, cap), 8.0),
                idx2=np.full((B, cap, 2), -1, np.int32), good0=np.zeros((B, cap), np.uint8),
                good=np.zeros((B, cap), np.uint8), owner=np.full((B, kp_cap), -1, np.int32),
                nq=np.full(B, m["n"], np.int32))


def _lose(st, b, l, w, j):
    """In frame b, l and w both match keypoint j and w keeps it."""
    cap = st["good"].shape[1]
    for i, g in ((l, 0), (w, 1)):
        if 0 <= i < cap:
            st["good0"][b, i], st["good"][b, i], st["idx2"][b, i, 0] = 1, g, j
    if 0 <= j < st["owner"].shape[1]:
        st["owner"][b, j] = w
    return st


def _inputs(st):
    return [st[k] for k in ("uv", "z", "idx2", "good0", "good", "owner", "nq")]


def _flip_bits(d, nbits):
    bits = np.unpackbits(d)
    bits[:nbits] ^= 1
    return np.packbits(bits)


def _case_chain():
    """c loses to b in frame 0, b loses to a in frame 1, found a > b > c: all end at a."""
    a, b, c = 2, 5, 1
    st = _blank(7, 2, 4, found=[1, 3, 9, 1, 1, 6, 1])
    _lose(st, 0, c, b, 1)
    _lose(st, 1, b, a, 3)
    return st, {b: a, c: a}


def _case_best_partner():
    """Pairs a-b and b-c, a outranks c outranks b: b goes to a, c stays."""
    a, b, c = 4, 0, 3
    st = _blank(6, 2, 4, found=[2, 1, 1, 5, 8, 1])
    _lose(st, 0, b, a, 0)
    _lose(st, 1, b, c, 2)
    return st, {b: a}


def _case_cycle():
    """l loses to w in frame 0, w loses to l in frame 1: one survivor, by rank."""
    st = _blank(4, 2, 3, found=[1, 4, 7, 1])
    _lose(st, 0, 1, 2, 0)
    _lose(st, 1, 2, 1, 1)
    return st, {1: 2}


def _case_equal_found():
    st = _blank(6, 1, 3, found=[5, 5, 5, 5, -2, -9])
    _lose(st, 0, 1, 3, 0)     # 3 keeps the keypoint, the lower index 1 survives
    _lose(st, 0, 5, 4, 2)     # negative counts are both 0: the lower index again
    return st, {3: 1, 5: 4}


def _case_dead():
    st = _blank(6, 1, 4)
    _lose(st, 0, 1, 0, 0)     # the partner is dead
    _lose(st, 0, 2, 3, 1)     # the loser is dead
    _lose(st, 0, 5, 4, 2)     # both alive
    st["map"]["X"][0] = [np.nan, 1.0, 1.0]
    st["map"]["X"][2] = np.nan
    return st, {5: 4}


def _case_stale():
    """Entries at or beyond nq_b, and slots at or beyond *d_n, tempting but stale."""
    st = _blank(10, 2, 6, n=8)
    st["nq"][:] = [6, 9]
    _lose(st, 0, 1, 6, 0)     # the partner is beyond nq_0
    _lose(st, 0, 7, 0, 1)     # the loser is beyond nq_0
    _lose(st, 0, 3, 2, 2)     # both below: fused
    _lose(st, 1, 4, 8, 3)     # below nq_1, the partner beyond *d_n
    _lose(st, 1, 8, 5, 4)     # below nq_1, the loser beyond *d_n
    _lose(st, 1, 7, 6, 5)     # both below nq_1 and *d_n: fused
    return st, {3: 2, 7: 6}


def _case_owner():
    st = _blank(9, 1, 8)
    for l, w in ((1, -1), (2, 9), (3, 1 << 20), (4, -(1 << 31)), (6, 6)):
        _lose(st, 0, l, w, l)                # owner -1, out of range, the loser itself
    st["good"][0, 6] = 0
    _lose(st, 0, 7, 0, 7)
    st["idx2"][0, 5, 0], st["good0"][0, 5] = 8, 1     # the keypoint index out of range
    st["idx2"][0, 8, 0], st["good0"][0, 8] = -1, 1
    return st, {7: 0}


def _case_good0():
    st = _blank(6, 1, 3)
    _lose(st, 0, 1, 0, 0)
    st["good0"][0, 1] = 0                    # failed the descriptor tests
    _lose(st, 0, 3, 2, 1)
    st["good"][0, 3] = 1                     # did not lose
    _lose(st, 0, 5, 4, 2)
    return st, {5: 4}


def _case_thresholds():
    """Each of the three thresholds exactly met (even l) and just exceeded."""
    st = _blank(16, 1, 8)
    for k in range(8):
        _lose(st, 0, 2 * k + 1, 2 * k, k)
    uv, z, desc = st["uv"][0], st["z"][0], st["map"]["desc"]
    uv[1] = [103.0, 100.0]                                   # du du = 9 = px px
    uv[3] = [np.nextafter(np.float32(103.0), np.float32(200.0)), 100.0]
    uv[4], uv[5] = [10.0, 20.0], [10.0 - 1.5, 20.0 + 2.5]    # 2.25 + 6.25 = 8.5 <= 9
    uv[6], uv[7] = [10.0, 20.0], [10.0 - 1.5, 20.0 + 2.625]  # 2.25 + 6.890625 > 9
    z[9] = 9.0                                               # |8 - 9| = 0.125 * 8
    z[10], z[11] = np.nextafter(9.0, 10.0), 8.0              # just beyond, the loser the nearer one
    desc[13] = _flip_bits(desc[12], 64)
    desc[15] = _flip_bits(desc[14], 65)
    return st, {1: 0, 5: 4, 9: 8, 13: 12}


HAND = dict(chain=_case_chain, best_partner=_case_best_partner, cycle=_case_cycle,
            equal_found=_case_equal_found, dead=_case_dead, stale=_case_stale, owner=_case_owner,
            good0=_case_good0, thresholds=_case_thresholds)


def _check_hand(st, fused, m, to, nfused):
    """A fuse result against the case's hand-written survivors and the Apply rules."""
    m0 = st["map"]
    cap = len(m0["X"])
    want_to = np.arange(cap, dtype=np.int32)
    for i, r in fused.items():
        want_to[i] = r
    assert np.array_equal(to, want_to) and to.dtype == np.int32
    assert nfused == len(fused)
    for r in range(cap):
        kids = [i for i, rr in fused.items() if rr == r]
        if r in fused:                                       # dead; its own counters stay
            assert np.isnan(m["X"][r]).all()
            kids = []
        else:
            assert tl._same(m["X"][r], m0["X"][r])
        assert m["visible"][r] == m0["visible"][r] + sum(m0["visible"][i] for i in kids)
        assert m["found"][r] == m0["found"][r] + sum(m0["found"][i] for i in kids)
        assert m["born"][r] == min([m0["born"][r]] + [m0["born"][i] for i in kids])
        assert m["last"][r] == max([m0["last"][r]] + [m0["last"][i] for i in kids])
    assert np.array_equal(m["desc"], m0["desc"]) and m["n"] == m0["n"]


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_hand_made(name):
    st, fused = HAND[name]()
    before = ml.copy_map(st["map"])
    m, to, nfused = mf.fuse(st["map"], *_inputs(st), **THR)
    _check_hand(st, fused, m, to, nfused)
    tl._assert_maps_equal(st["map"], before)                 # the input is left alone


def _rows_cases():
    """-> (rows [B,6,4], count [B], to [8], expected rows per frame as lists)."""
    to = np.arange(8, dtype=np.int32)
    to[[1, 2, 5]] = [4, 4, 6]                               # 1 and 2 were fused into 4, 5 into 6
    nan = np.nan
    frames = [
        # both twins observed: the survivor's row is kept even at the higher k
        ([[0, 1, 10, 11], [0, 3, 12, 13], [0, 4, 14, 15], [0, 2, 16, 17]],
         [[0, 3, 12, 13], [0, 4, 14, 15]]),
        # two rows of fused landmarks, none of the survivor: the lowest k, renamed
        ([[1, 0, 1, 1], [1, 2, 20, 21], [1, 1, 22, 23], [1, 5, 24, 25]],
         [[1, 0, 1, 1], [1, 4, 20, 21], [1, 6, 24, 25]]),
        # two rows of the survivor itself: the lowest k
        ([[2, 6, 1, 2], [2, 5, 3, 4], [2, 6, 5, 6]], [[2, 6, 1, 2]]),
        # rows that belong to nobody pass through, even beside one another
        ([[3, nan, 1, 2], [3, -1, 3, 4], [3, 8, 5, 6], [3, 3.5, 7, 8], [3, nan, 9, 10], [3, 3.5, 7, 8]],
         [[3, nan, 1, 2], [3, -1, 3, 4], [3, 8, 5, 6], [3, 3.5, 7, 8], [3, nan, 9, 10], [3, 3.5, 7, 8]]),
        # a count above rows_cap is clamped
        ([[4, 1, 1, 2], [4, 7, 3, 4], [4, 7, 5, 6], [4, 2, 7, 8], [4, 0, 9, 10], [4, 4, 11, 12]],
         [[4, 7, 3, 4], [4, 0, 9, 10], [4, 4, 11, 12]]),
        # a negative count is no rows
        ([[5, 1, 1, 2], [5, 2, 3, 4]], []),
    ]
    count = np.array([4, 4, 3, 6, 99, -3], np.int32)
    rows = np.full((len(frames), 6, 4), 77.0)
    for b, (r, _) in enumerate(frames):
        rows[b, :len(r)] = r
    return rows, count, to, [np.array(w, np.float64).reshape(-1, 4) for _, w in frames]


def test_reference_rows_hand_made():
    rows, count, to, want = _rows_cases()
    before = rows.copy()
    out, cnt = mf.rows_fuse(rows, count, to)
    assert cnt.tolist() == [len(w) for w in want]
    for b, w in enumerate(want):
        assert tl._same(out[b, :cnt[b]], w), b
    assert tl._same(rows, before)


def test_argument_errors_without_gpu():
    from slam355 import _lib

    L = _lib.lib
    err = lambda: L.slam_last_error()  # noqa: E731
    buf = (ctypes.c_double * 64)()       # never read: every call below is refused before any GPU call
    q = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q2 = ctypes.c_void_p(q.value + 64)
    nan = float("nan")

    def each_null(call, names):
        for k, name in enumerate(names):
            ptrs = [q] * len(names)
            ptrs[k] = None
            assert call(ptrs=ptrs) == -1 and (name + " is null").encode() in err(), name

    nb = ctypes.c_size_t(0)
    assert L.slam_map_fuse_workspace_bytes(1100, ctypes.byref(nb)) == 0 and nb.value >= 8 * 1100
    for bad in (0, -1, (1 << 20) + 1):
        assert L.slam_map_fuse_workspace_bytes(bad, ctypes.byref(nb)) == -1 and b"x_cap" in err()
    assert L.slam_map_fuse_workspace_bytes(10, None) == -1 and b"bytes" in err()
    assert L.slam_rows_fuse_workspace_bytes(3, 1100, ctypes.byref(nb)) == 0 and nb.value >= 3 * 1100 * 4
    for bad in (0, 65536):
        assert L.slam_rows_fuse_workspace_bytes(bad, 10, ctypes.byref(nb)) == -1 and b"batch" in err()
    for bad in (0, (1 << 20) + 1):
        assert L.slam_rows_fuse_workspace_bytes(3, bad, ctypes.byref(nb)) == -1 and b"x_cap" in err()
    assert L.slam_rows_fuse_workspace_bytes(3, 10, None) == -1 and b"bytes" in err()

    names = ["d_uv", "d_z", "d_idx2", "d_good0", "d_good", "d_owner", "d_nq", "d_X", "d_desc",
             "d_visible", "d_found", "d_born", "d_last", "d_n", "d_to", "d_nfused", "d_ws"]

    def fuse(batch=2, kp_cap=20, x_cap=50, px=3.0, rel=0.1, max_dist=64, ws=1 << 20, ptrs=(q,) * 17):
        p = list(ptrs)
        return L.slam_map_fuse(*p[:7], batch, kp_cap, *p[7:14], x_cap, px, rel, max_dist, p[14], p[15],
                               p[16], ws, None)
    each_null(fuse, names)
    for bad in (0, 65536):
        assert fuse(batch=bad) == -1 and b"batch" in err()
        assert fuse(kp_cap=bad) == -1 and b"kp_cap" in err()
    for bad in (0, (1 << 20) + 1):
        assert fuse(x_cap=bad) == -1 and b"x_cap" in err()
    for bad in (0.0, -1.0, nan):
        assert fuse(px=bad) == -1 and b"px" in err()
    for bad in (-0.5, nan):
        assert fuse(rel=bad) == -1 and b"rel_depth" in err()
    for bad in (-1, 257):
        assert fuse(max_dist=bad) == -1 and b"max_dist" in err()
    assert fuse(ws=8 * 50 - 1) == -3 and b"ws_size" in err()
    odd = ctypes.c_void_p(q.value + 8)
    assert fuse(ptrs=[q] * 8 + [odd] + [q] * 8) == -1 and b"d_desc" in err() and b"aligned" in err()
    odd = ctypes.c_void_p(q.value + 4)
    assert fuse(ptrs=[q] * 16 + [odd]) == -1 and b"d_ws" in err() and b"aligned" in err()

    def rows(rows_cap=10, batch=2, x_cap=10, ws=1 << 20, ptrs=(q, q, q, q2, q2, q)):
        r, c, to, out, cout, w = ptrs
        return L.slam_rows_fuse(r, c, rows_cap, batch, to, x_cap, out, cout, w, ws, None)
    each_null(rows, ["d_rows", "d_count", "d_to", "d_rows_out", "d_count_out", "d_ws"])
    for bad in (0, 65536):
        assert rows(batch=bad) == -1 and b"batch" in err()
        assert rows(rows_cap=bad) == -1 and b"rows_cap" in err()
    for bad in (0, (1 << 20) + 1):
        assert rows(x_cap=bad) == -1 and b"x_cap" in err()
    assert rows(ptrs=(q, q, q, q, q2, q)) == -1 and b"alias" in err()
    assert rows(ptrs=(q, q2, q, q2, q2, q)) == -1 and b"alias" in err()
    assert rows(ws=2 * 10 * 4 - 1) == -3 and b"ws_size" in err()


def test_fuse_needs_an_observe_and_a_gpu():
    import torch
    from slam355.mapping import LandmarkMap

    if torch.cuda.is_available():
        lm = LandmarkMap(16, 8, tl.W, tl.H, tl.P3)
    else:
        with pytest.raises(RuntimeError, match="GPU"):
            LandmarkMap(16, 8, tl.W, tl.H, tl.P3)
        lm = object.__new__(LandmarkMap)                     # what the constructor would have left
        lm.uv = lm.good0 = None
    with pytest.raises(ValueError, match="fuse"):
        lm.fuse()


# ----------------------------------------------------------------------------- the scene with planted twins
N_TWINS, TWIN_OFFSET, TWIN_BITS = 60, 0.02, 20
FUSE = dict(px=3.0, rel_depth=0.1, max_dist=64)


@functools.lru_cache(maxsize=None)
def _twin_scene():
    """The scene of test_map_life.py; every fourth landmark of the first frame gets
    a twin TWIN_OFFSET metres off (a random direction) with TWIN_BITS other bits of
    its descriptor flipped.  -> (scene, X, desc, origin of the initial slots,
    planted pairs [(slot, twin slot)])."""
    s = tl._scene()
    rng = np.random.default_rng(77)
    vis0 = s["vis0"]
    pick = np.arange(0, len(vis0), 4)[:N_TWINS]
    assert len(pick) == N_TWINS
    d = rng.normal(size=(N_TWINS, 3))
    X = np.r_[s["X"][vis0], s["X"][vis0[pick]] + TWIN_OFFSET * d / np.linalg.norm(d, axis=1, keepdims=True)]
    D = np.r_[s["D"][vis0], tl._flip(rng, s["D"][vis0[pick]], TWIN_BITS)]
    origin = np.r_[vis0, vis0[pick]]
    return s, X, D, origin, [(int(i), len(vis0) + k) for k, i in enumerate(pick)]


def _observe_ref(s, m, f, pose, radius):
    """Steps 1-5 of guided matching for frame f at `pose`."""
    n = m["n"]
    uv, z = gr.project(m["X"][:n], pose, tl.P3, tl.W, tl.H, 0.0, 0.1)
    i2, d2, g0 = gr.window_knn2(m["desc"][:n], uv, np.full(n, radius, np.float32), s["desc"][f],
                                s["kp"][f], s["n_kp"][f], tl.W, tl.H, tl.MAX_DIST, tl.RATIO)
    owner, good = gr.unique(i2, d2, g0, s["cap"])
    return dict(uv=uv, z=z, idx2=i2, good0=g0, good=good, owner=owner,
                rows=gr.track_rows(i2, good, s["kp"][f], f))


def _localize_ref(s, m, f):
    one = tl._refine(m, _observe_ref(s, m, f, s["pred"][f], tl.RADIUS[0])["rows"], s["pred"][f])
    obs = _observe_ref(s, m, f, one["pose"], tl.RADIUS[1])
    return tl._refine(m, obs["rows"], one["pose"]), obs


def _pad(s, m, obs):
    """Per-frame by-products -> the batch arrays the device keeps (stale past n)."""
    B, n, cap = len(obs), m["n"], s["x_cap"]
    out = dict(uv=np.full((B, cap, 2), np.nan, np.float32), z=np.zeros((B, cap)),
               idx2=np.full((B, cap, 2), -1, np.int32), good0=np.zeros((B, cap), np.uint8),
               good=np.zeros((B, cap), np.uint8), owner=np.stack([o["owner"] for o in obs]),
               nq=np.full(B, n, np.int32), rows=np.zeros((B, s["rows_cap"], 4)),
               count=np.zeros(B, np.int32))
    for b, o in enumerate(obs):
        for k in ("uv", "z", "idx2", "good0", "good"):
            out[k][b, :n] = o[k]
        out["rows"][b, :len(o["rows"])], out["count"][b] = o["rows"], len(o["rows"])
    return out


def _no_landmark_twice(tracks, x_cap):
    """What refine_points' reference makes of the rows: every row that names a
    landmark is that landmark's observation in its frame, none is shadowed."""
    for rows, count in tracks:
        tab = pts.index_rows(rows, count, x_cap)
        for f in range(len(count)):
            v = rows[f, :count[f], 1]
            named = int(((v >= 0) & (v < x_cap) & (np.floor(v) == v)).sum())
            if int((tab[f] >= 0).sum()) != named:
                return False
    return True


def _twins_alive(X, planted):
    return sum(1 for i, t in planted if not np.isnan(X[i, 0]) and not np.isnan(X[t, 0]))


@functools.lru_cache(maxsize=None)
def _twin_reference_run():
    """localize / score / spawn / fuse / cull per batch on the CPU, as
    LandmarkMap.step(fuse=...) orders them; keeps what each fuse read and wrote."""
    s, X, D, origin0, planted = _twin_scene()
    m = ml.add(ml.new_map(s["x_cap"]), X, D, 0)
    origin = np.full(s["x_cap"], -2, np.int64)
    origin[:m["n"]] = origin0
    tracks, batches, status, wrong = [], [], [], 0
    B = s["B"]
    for f0 in range(0, s["nf"], B):
        fr = slice(f0, f0 + B)
        res = [_localize_ref(s, m, f) for f in range(f0, f0 + B)]
        st = [r[0]["status"] for r in res]
        status += st
        p = _pad(s, m, [r[1] for r in res])
        poses = np.stack([r[0]["pose"] for r in res])
        m = ml.score(m, p["uv"], p["good"], p["nq"], f0)
        flags = (s["keyframe"][fr] != 0) & (np.asarray(st) == 0)
        m, owner1, rows, count, _, dropped = ml.spawn(
            m, s["Xc"][fr], s["pairs"][fr], s["count"][fr], s["kp"][fr], s["desc"][fr], s["n_kp"][fr],
            p["owner"], poses, flags, *tl.Z_RANGE, f0, p["rows"], p["count"])
        assert dropped == 0
        origin = tl._origins(s, origin, f0, p["owner"], owner1)
        p["owner"] = owner1
        tracks = tracks + [(rows, count)]
        before = dict(map=m, tracks=tracks, obs=p)
        m, to, nfused = mf.fuse(m, p["uv"], p["z"], p["idx2"], p["good0"], p["good"], owner1, p["nq"],
                                **FUSE)
        tracks = [mf.rows_fuse(r, c, to) for r, c in tracks]
        fused = np.nonzero(to != np.arange(len(to)))[0]
        wrong += int(((origin[fused] != origin[to[fused]]) | (origin[fused] < 0)).sum())
        batches.append(dict(before=before, map=m, to=to, nfused=nfused, tracks=tracks))
        m, _ = ml.cull(m, f0 + B - 1, **tl.CULL)
    return dict(batches=batches, map=m, tracks=tracks, status=status, wrong=wrong, origin=origin)


def test_reference_scene_fuses_the_planted_twins():
    s, _, _, _, planted = _twin_scene()
    r = _twin_reference_run()
    both = _twins_alive(r["map"]["X"], planted)
    print("fused per batch", [b["nfused"] for b in r["batches"]], "across different truth", r["wrong"],
          f"\n planted pairs with both twins alive at the end: {both} of {len(planted)} "
          f"({both / len(planted):.3f})", "slots", r["map"]["n"])
    assert r["status"] == [0] * s["nf"]
    assert r["batches"][0]["nfused"] >= len(planted) // 2     # the fuse is what removes them
    assert r["wrong"] == 0
    assert _no_landmark_twice(r["tracks"], s["x_cap"])
    for b in r["batches"]:                                   # no row names a fused landmark any more
        for rows, count in b["tracks"]:
            for f in range(len(count)):
                v = rows[f, :count[f], 1].astype(int)
                assert (b["to"][v] == v).all()
    assert 10 * both <= len(planted)


# ----------------------------------------------------------------------------- GPU
def _dev(a):
    return tl._dev(a)


def _device_fuse(m, uv, z, idx2, good0, good, owner, nq, px, rel_depth, max_dist):
    """slam_map_fuse through the C ABI -> (map, to, nfused)."""
    import torch
    from slam355 import _lib
    from slam355.device import ptr

    cap = len(m["X"])
    d = tl._map_to_dev(m)
    ins = [_dev(a) for a in (uv, z, idx2, good0, good, owner, nq)]
    nb = ctypes.c_size_t(0)
    _lib.call("slam_map_fuse_workspace_bytes", cap, ctypes.byref(nb))
    ws = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device="cuda")
    to = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    nfused = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _lib.call("slam_map_fuse", *(ptr(t) for t in ins), int(owner.shape[0]), int(owner.shape[1]),
              *(ptr(d[k]) for k in ml.FIELDS), ptr(d["n"]), cap, float(px), float(rel_depth),
              int(max_dist), ptr(to), ptr(nfused), ptr(ws), ws.numel(), None)
    return tl._map_from_dev(d), to.cpu().numpy(), int(nfused.item())


def _device_rows_fuse(rows, count, to):
    """slam_rows_fuse through the C ABI -> (rows_out with -3 where nothing was written, count_out)."""
    import torch
    from slam355 import _lib
    from slam355.device import ptr

    B, rows_cap = rows.shape[:2]
    ins = [_dev(rows), _dev(count), _dev(to)]
    nb = ctypes.c_size_t(0)
    _lib.call("slam_rows_fuse_workspace_bytes", B, len(to), ctypes.byref(nb))
    ws = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((B, rows_cap, 4), -3.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    _lib.call("slam_rows_fuse", ptr(ins[0]), ptr(ins[1]), rows_cap, B, ptr(ins[2]), len(to), ptr(out),
              ptr(cnt), ptr(ws), ws.numel(), None)
    return out.cpu().numpy(), cnt.cpu().numpy()


def _assert_rows_equal(grows, gcount, wrows, wcount):
    assert tl._same(gcount, wcount)
    for b in range(len(wcount)):
        assert np.array_equal(tl._bits(grows[b, :wcount[b]]), tl._bits(wrows[b, :wcount[b]])), b
        assert (grows[b, wcount[b]:] == -3.0).all()          # nothing written past the count


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_on_device(name):
    st, fused = HAND[name]()
    want = mf.fuse(st["map"], *_inputs(st), **THR)
    m, to, nfused = _device_fuse(st["map"], *_inputs(st), **THR)
    _check_hand(st, fused, m, to, nfused)
    tl._assert_maps_equal(m, want[0])
    assert np.array_equal(tl._bits(m["X"]), tl._bits(want[0]["X"]))


@pytest.mark.gpu
def test_rows_hand_made_on_device():
    rows, count, to, want = _rows_cases()
    out, cnt = _device_rows_fuse(rows, count, to)
    wrows, wcount = mf.rows_fuse(rows, count, to)
    _assert_rows_equal(out, cnt, wrows, wcount)
    for b, w in enumerate(want):
        assert tl._same(out[b, :cnt[b]], w), b


@functools.lru_cache(maxsize=None)
def _random_case():
    """x_cap 1100 with 1061 slots in use, three frames with three nq, 200 keypoints.
    Per frame the keypoints' owners and, for 80 of them, one or two losers each are
    drawn from the whole array, stale entries included; a pair passes every test unless one
    of the spoilers below hits it.  Chains of depth 3 are planted across the
    frames on landmarks nothing else touches."""
    rng = np.random.default_rng(1100)
    cap, n, B, kp_cap = 1100, 1061, 3, 200
    m = tl._random_map(rng, cap, n, dead=0.04)
    m["found"][:] = rng.integers(-3, 12, cap)                # many ties, some negative
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    m["desc"][:] = tl._flip(rng, np.tile(base, (cap, 1)), 24)    # any two within 48 bits
    far = rng.random(cap) < 0.05
    m["desc"][far] = rng.integers(0, 256, (int(far.sum()), 32), dtype=np.uint8)
    nq = np.array([1061, 900, 1100], np.int32)
    uv = rng.uniform(0, 600, (B, cap, 2)).astype(np.float32)
    z = rng.uniform(5, 30, (B, cap))
    idx2 = rng.integers(-1, kp_cap + 2, (B, cap, 2)).astype(np.int32)
    good0 = (rng.random((B, cap)) < 0.3).astype(np.uint8)    # losers of keypoints that others own
    good = np.zeros((B, cap), np.uint8)
    owner = np.full((B, kp_cap), -1, np.int32)
    chains = [rng.permutation(np.arange(40 * c, 40 * c + 40))[:4] for c in range(5)]
    reserved = np.concatenate(chains)
    m["X"][reserved] = 1.0
    m["desc"][reserved] = base
    free = np.setdiff1d(np.arange(cap), reserved)
    for b in range(B):
        who = rng.permutation(free)
        owners, losers = who[:kp_cap - 10], who[kp_cap:]
        k = 0
        for j, w in enumerate(owners):
            owner[b, j] = w
            good0[b, w], good[b, w], idx2[b, w, 0] = 1, 1, j
            for l in losers[k:k + (rng.integers(1, 3) if j < 80 else 0)]:
                k += 1
                good0[b, l], good[b, l], idx2[b, l, 0] = 1, 0, j
                uv[b, l] = uv[b, w] + rng.uniform(-1.5, 1.5, 2).astype(np.float32)
                z[b, l] = z[b, w] * rng.uniform(0.93, 1.07)
                spoil = rng.integers(0, 30)
                if spoil == 0:
                    uv[b, l, rng.integers(0, 2)] = np.nan
                elif spoil == 1:
                    uv[b, w, rng.integers(0, 2)] = np.inf
                elif spoil == 2:
                    uv[b, l, 0] += 3.0
                elif spoil == 3:
                    z[b, l] = z[b, w] * 1.2
                elif spoil == 4:
                    z[b, l] = np.nan
                elif spoil == 5:
                    good0[b, l] = 0
                elif spoil == 6:
                    good[b, l] = 1
                elif spoil == 7:
                    idx2[b, l, 0] = [-1, kp_cap, kp_cap - 1, 1 << 30][rng.integers(0, 4)]
        for j, w in zip(range(kp_cap - 10, kp_cap - 5), (-1, -5, cap, 1 << 24, 1061)):
            owner[b, j] = w
            l = losers[k]
            k += 1
            good0[b, l], good[b, l], idx2[b, l, 0] = 1, 0, j
        # chain c: its member 3 - b loses to member 2 - b in frame b; found falls along the chain
        for c, ch in enumerate(chains):
            w, l, j = ch[2 - b], ch[3 - b], kp_cap - 5 + c
            owner[b, j] = w
            good0[b, w], good[b, w], idx2[b, w, 0] = 1, 1, j
            good0[b, l], good[b, l], idx2[b, l, 0] = 1, 0, j
            uv[b, l], z[b, l] = uv[b, w], z[b, w]
    for ch in chains:
        m["found"][ch] = [40, 30, 20, 10]
    return dict(map=m, uv=uv, z=z, idx2=idx2, good0=good0, good=good, owner=owner, nq=nq, chains=chains)


@pytest.mark.gpu
def test_fuse_against_reference():
    c = _random_case()
    cap = len(c["map"]["X"])
    want, wto, wn = mf.fuse(c["map"], *_inputs(c), **FUSE)
    pairs = mf.pairs(c["map"], *_inputs(c), **FUSE)
    in_pairs = len({i for _, l, w in pairs for i in (l, w)})
    partners = {}
    for _, l, w in pairs:
        partners.setdefault(l, set()).add(w)
        partners.setdefault(w, set()).add(l)
    deep = sum(1 for i, p in partners.items() if wto[i] != i and wto[i] not in p)
    print(f"{len(pairs)} candidate pairs over {in_pairs} landmarks, {wn} fused, "
          f"{deep} of them into a root that is no partner of theirs")
    assert cap / 5 < in_pairs < cap / 2 and wn > cap / 10 and deep >= 10
    for ch in c["chains"]:                                   # depth 3 across the frames
        assert (wto[ch] == ch[0]).all()
    assert len({b for b, _, _ in pairs}) == 3
    got, to, nfused = _device_fuse(c["map"], *_inputs(c), **FUSE)
    assert np.array_equal(to, wto) and nfused == wn
    tl._assert_maps_equal(got, want)
    assert np.array_equal(tl._bits(got["X"]), tl._bits(want["X"]))    # the NaN pattern, old and new


@pytest.mark.gpu
def test_rows_fuse_against_reference():
    c = _random_case()
    cap = len(c["map"]["X"])
    _, to, _ = mf.fuse(c["map"], *_inputs(c), **FUSE)
    rng = np.random.default_rng(1300)
    rows_cap = 1300
    count = np.array([0, 1, 1024, 1025, 1300, -4, 4000], np.int32)
    B = len(count)
    rows = rng.uniform(0, 600, (B, rows_cap, 4))
    fused = np.nonzero(to != np.arange(cap))[0]
    family = np.concatenate([fused, to[fused]])              # twins and their survivors: collisions
    lm = np.where(rng.random((B, rows_cap)) < 0.6, family[rng.integers(0, len(family), (B, rows_cap))],
                  rng.integers(0, cap, (B, rows_cap))).astype(np.float64)
    odd = rng.integers(0, 40, (B, rows_cap))
    for k, v in enumerate((-1.0, float(cap), 1e12, np.nan, -0.5, 3.5, cap - 0.5, -np.inf, -0.0)):
        lm[odd == k] = v
    rows[..., 1] = lm
    wrows, wcount = mf.rows_fuse(rows, count, to)
    print("rows kept per frame", wcount.tolist(), "of", np.clip(count, 0, rows_cap).tolist())
    assert (wcount[2:5] < count[2:5]).all() and wcount[5] == 0
    grows, gcount = _device_rows_fuse(rows, count, to)
    _assert_rows_equal(grows, gcount, wrows, wcount)


def _upload(lm, m, obs, tracks):
    """Put a reference state where LandmarkMap keeps its own."""
    for k in ml.FIELDS:
        getattr(lm, k).copy_(_dev(m[k]))
    lm.n_dev.fill_(m["n"])
    lm.n, lm._exact = m["n"], True
    lm.uv, lm.z, lm.idx2, lm.good0, lm.good, lm.owner = (
        _dev(obs[k]) for k in ("uv", "z", "idx2", "good0", "good", "owner"))
    lm._nq = _dev(obs["nq"])
    lm._tracks = [(_dev(r), _dev(c)) for r, c in tracks]


def _tracks_np(lm):
    return [(r.cpu().numpy(), c.cpu().numpy()) for r, c in lm._tracks]


@pytest.mark.gpu
def test_fuse_per_batch_parity_on_the_scene():
    """LandmarkMap.fuse on the reference chain's own state before each of its fuses."""
    from slam355.mapping import LandmarkMap

    s = _twin_scene()[0]
    r = _twin_reference_run()
    lm = LandmarkMap(s["x_cap"], s["cap"], tl.W, tl.H, tl.P3)
    for k, b in enumerate(r["batches"]):
        _upload(lm, b["before"]["map"], b["before"]["obs"], b["before"]["tracks"])
        nfused, to = lm.fuse(**FUSE)
        assert int(nfused.item()) == b["nfused"] and np.array_equal(to.cpu().numpy(), b["to"]), k
        tl._assert_maps_equal(tl._state(lm), b["map"])
        got = _tracks_np(lm)
        assert len(got) == len(b["tracks"]) == k + 1
        for (grows, gcount), (wrows, wcount) in zip(got, b["tracks"]):
            assert tl._same(gcount, wcount)
            for f in range(len(wcount)):
                assert tl._same(grows[f, :wcount[f]], wrows[f, :wcount[f]]), (k, f)
    assert sum(b["nfused"] for b in r["batches"]) >= N_TWINS // 2


def _twin_map():
    from slam355.mapping import LandmarkMap

    s, X, D, _, _ = _twin_scene()
    return LandmarkMap(s["x_cap"], s["cap"], tl.W, tl.H, tl.P3).add(X, D)


NO_CULL = dict(min_visible=1 << 30, age=1 << 30)


def _step(lm, s, f0, cull=tl.CULL, **kw):
    res = lm.step(f0, *tl._batch_args(s, f0), z_range=tl.Z_RANGE, cull=cull, radius=tl.RADIUS,
                  max_dist=tl.MAX_DIST, ratio=tl.RATIO, **kw)
    return [t.cpu().numpy().copy() for t in res]


@pytest.mark.gpu
def test_step_with_fuse_end_to_end():
    """The three scene conditions on the device's own run; fuse=None is the step of before."""
    s, _, _, origin0, planted = _twin_scene()
    lm, plain, none = _twin_map(), _twin_map(), _twin_map()
    origin = np.full(s["x_cap"], -2, np.int64)
    origin[:len(origin0)] = origin0
    wrong, fused_total = 0, 0
    for f0 in range(0, s["nf"], s["B"]):
        n0 = lm.size()
        res = _step(lm, s, f0, fuse=FUSE)
        assert (res[5] == 0).all()
        owner = lm.owner.cpu().numpy()
        for b, j in zip(*np.nonzero(owner >= n0)):           # the slots this step's spawn filled
            origin[owner[b, j]] = s["truth"][f0 + b, j]
        assert int(lm.dropped.item()) == 0
        to = lm.to.cpu().numpy()
        fused = np.nonzero(to != np.arange(len(to)))[0]
        assert len(fused) == int(lm.nfused.item())
        fused_total += len(fused)
        wrong += int(((origin[fused] != origin[to[fused]]) | (origin[fused] < 0)).sum())
        a, b = _step(plain, s, f0), _step(none, s, f0, fuse=None)
        for i in (0, 1, 2):                                  # poses, rows, counts
            assert np.array_equal(tl._bits(a[i]), tl._bits(b[i])), (f0, i)
    tl._assert_maps_equal(tl._state(plain), tl._state(none))
    both = _twins_alive(lm.X.cpu().numpy(), planted)
    print(f"fused {fused_total}, across different truth {wrong}, planted pairs with both twins alive "
          f"at the end: {both} of {len(planted)} ({both / len(planted):.3f})")
    assert wrong == 0
    assert _no_landmark_twice(_tracks_np(lm), s["x_cap"])
    assert 10 * both <= len(planted)
    assert fused_total >= len(planted) // 2                  # the fuse removed them, not the cull


@pytest.mark.gpu
def test_fuse_and_compact_in_either_order():
    s = _twin_scene()[0]
    x_cap = s["x_cap"]
    # compact after fuse: the fused landmarks are gone, the survivors' rows renumbered
    a = _twin_map()
    _step(a, s, 0, fuse=FUSE)
    to = a.to.cpu().numpy()
    fused = np.nonzero(to != np.arange(x_cap))[0]
    assert len(fused) >= N_TWINS // 2
    before = _tracks_np(a)
    dead = np.isnan(a.X[:, 0].cpu().numpy())
    remap = a.compact().cpu().numpy()
    assert (remap[fused] == -1).all() and (remap[to[fused]] >= 0).all()
    assert not np.isnan(a.X[:a.n, 0].cpu().numpy()).any()
    for (rows, count), (rows0, count0) in zip(_tracks_np(a), before):
        for f in range(len(count)):
            v0 = rows0[f, :count0[f], 1].astype(int)
            assert np.array_equal(rows[f, :count[f], 1], remap[v0[~dead[v0]]])
    t = a.tracks()
    assert len(np.unique(t[:, :2], axis=0)) == len(t) > 0   # no landmark twice in a frame
    assert _no_landmark_twice(_tracks_np(a), x_cap)
    # fuse after compact: the renumbered rows and state fuse as the reference says
    b = _twin_map()
    _step(b, s, 0, cull=NO_CULL)                             # the twins stay alive, both in the tracks
    b.X[5:200:7] = float("nan")                              # some die, so the compaction renumbers
    remap = b.compact().cpu().numpy()
    assert (remap[5:200:7] == -1).all() and remap[204] == 204 - 28
    _step(b, s, s["B"], cull=NO_CULL)
    m = tl._state(b)
    obs = {k: getattr(b, k).cpu().numpy() for k in ("uv", "z", "idx2", "good0", "good", "owner")}
    obs["nq"] = b._nq.cpu().numpy()
    tracks = _tracks_np(b)
    want, wto, wn = mf.fuse(m, *_inputs(obs), **FUSE)
    nfused, to = b.fuse(**FUSE)
    assert int(nfused.item()) == wn > 0 and np.array_equal(to.cpu().numpy(), wto)
    tl._assert_maps_equal(tl._state(b), want)
    for (grows, gcount), (rows, count) in zip(_tracks_np(b), tracks):
        wrows, wcount = mf.rows_fuse(rows, count, wto)
        assert tl._same(gcount, wcount)
        for f in range(len(wcount)):
            assert tl._same(grows[f, :wcount[f]], wrows[f, :wcount[f]])
    assert _no_landmark_twice(_tracks_np(b), x_cap)


@pytest.mark.gpu
def test_fuse_in_graph_capture():
    import torch

    s = _twin_scene()[0]
    r = _twin_reference_run()
    b = r["batches"][0]
    from slam355.mapping import LandmarkMap

    lm = LandmarkMap(s["x_cap"], s["cap"], tl.W, tl.H, tl.P3)
    _upload(lm, b["before"]["map"], b["before"]["obs"], b["before"]["tracks"])
    lm.fuse(rewrite_tracks=False, **FUSE)                    # warm-up: allocates the buffers
    assert np.array_equal(lm.to.cpu().numpy(), b["to"])
    _upload(lm, b["before"]["map"], b["before"]["obs"], b["before"]["tracks"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):    # a host sync or a hipMalloc here fails the capture
        lm.fuse(rewrite_tracks=False, **FUSE)
        nfused, to = lm.fuse(rewrite_tracks=False, **FUSE)   # the second call finds nothing left
    to.fill_(-1)
    nfused.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    # the second call runs on what the first left: every pair has lost a member by then
    want, wto, wn = mf.fuse(b["map"], *_inputs(b["before"]["obs"]), **FUSE)
    assert wn == 0 and np.array_equal(wto, np.arange(s["x_cap"]))
    assert int(nfused.item()) == wn and np.array_equal(to.cpu().numpy(), wto)
    tl._assert_maps_equal(tl._state(lm), want)
    tl._assert_maps_equal(want, b["map"])
    for (rows, count), (rows0, count0) in zip(_tracks_np(lm), b["before"]["tracks"]):
        assert tl._same(rows, rows0) and tl._same(count, count0)     # rewrite_tracks=False
