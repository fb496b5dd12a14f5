"""Plain NumPy restatement of guided matching (include/slam355.h, "Guided
matching"): projection in the stated operation order, the cell index, the
windowed kNN-2 as brute force over all targets with the window predicate in
float32 (keypoints outside the image are in no cell, so they are no
candidates), the one-landmark-per-keypoint pass and the track rows.  Test
infrastructure only; every function works on ONE batch item."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def project(X, pose, P, W, H, margin=0.0, min_depth=0.1):
    """X [n,3] f64, pose 4x4 camera-to-world, P 3x4 -> (uv [n,2] f32 with NaN
    where invalid, z [n] f64)."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    T = np.asarray(pose, np.float64).reshape(4, 4)
    P = np.asarray(P, np.float64).reshape(3, 4)
    d = [X[:, k] - T[k, 3] for k in range(3)]
    xc = [(T[0, k] * d[0] + T[1, k] * d[1]) + T[2, k] * d[2] for k in range(3)]
    h = [((P[i, 0] * xc[0] + P[i, 1] * xc[1]) + P[i, 2] * xc[2]) + P[i, 3] for i in range(3)]
    with np.errstate(all="ignore"):
        u, v = h[0] / h[2], h[1] / h[2]
        ok = ((xc[2] > min_depth) & (h[2] > 0) & (margin <= u) & (u < W - margin)
              & (margin <= v) & (v < H - margin))
        uv = np.stack([u, v], 1).astype(np.float32)
    uv[~ok] = np.nan
    return uv, xc[2]


def kp_grid(kp, nkp, W, H, cell):
    """kp [cap,5] f32 -> (cell_ptr [gw*gh+1] i32, list of sorted index arrays per cell)."""
    kp = np.asarray(kp, np.float32)
    n = min(max(int(nkp), 0), len(kp))
    gw, gh = -(-W // cell), -(-H // cell)
    x, y = kp[:n, 0], kp[:n, 1]
    inv = np.float32(1.0) / np.float32(cell)
    with np.errstate(invalid="ignore"):
        ok = (x >= 0) & (x < np.float32(W)) & (y >= 0) & (y < np.float32(H))
    j = np.nonzero(ok)[0]
    c = (y[j] * inv).astype(np.int32) * gw + (x[j] * inv).astype(np.int32)
    members = [np.sort(j[c == k]).astype(np.int32) for k in range(gw * gh)]
    ptr = np.zeros(gw * gh + 1, np.int32)
    ptr[1:] = np.cumsum([len(m) for m in members])
    return ptr, members


def hamming(q, t):
    """[nq,32] u8 x [nt,32] u8 -> [nq,nt] i32."""
    return _POP[q[:, None, :] ^ t[None, :, :]].sum(2, dtype=np.int32)


def candidates(u, v, r, kp, nt, W, H):
    """Indices j < nt of the keypoints inside the image and inside the window
    |kx - u| <= r, |ky - v| <= r, the differences rounded to float32."""
    kp = np.asarray(kp, np.float32)
    nt = min(max(int(nt), 0), len(kp))
    u, v, r = np.float32(u), np.float32(v), np.float32(r)
    if not (np.isfinite(u) and np.isfinite(v) and r > 0):
        return np.zeros(0, np.int64)
    kx, ky = kp[:nt, 0], kp[:nt, 1]
    with np.errstate(invalid="ignore"):
        inside = (kx >= 0) & (kx < np.float32(W)) & (ky >= 0) & (ky < np.float32(H))
        win = (np.abs(kx - u) <= r) & (np.abs(ky - v) <= r)   # float32 throughout
    return np.nonzero(inside & win)[0]


def window_knn2(q, quv, qr, t, kp, nt, W, H, max_dist, ratio):
    """q [nq,32] u8, quv [nq,2] f32, qr [nq] f32, t [cap,32] u8, kp [cap,5] f32
    -> (idx2 [nq,2], dist2 [nq,2] i32, good [nq] u8); brute force over all targets."""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    nq = len(q)
    nt = min(max(int(nt), 0), len(t))
    quv = np.asarray(quv, np.float32).reshape(nq, 2)
    qr = np.asarray(qr, np.float32).reshape(nq)
    idx2 = np.full((nq, 2), -1, np.int32)
    dist2 = np.full((nq, 2), -1, np.int32)
    good = np.zeros(nq, np.uint8)
    D = hamming(q, np.asarray(t, np.uint8)[:nt]) if nq and nt else np.zeros((nq, nt), np.int32)
    num, den = ratio
    for i in range(nq):
        j = candidates(quv[i, 0], quv[i, 1], qr[i], kp, nt, W, H)
        key = np.sort((D[i, j].astype(np.int64) << 16) | j)[:2]
        for s, k in enumerate(key):
            idx2[i, s], dist2[i, s] = k & 0xFFFF, k >> 16
        if len(key) >= 1:
            d1 = int(dist2[i, 0])
            good[i] = d1 <= max_dist and (len(key) < 2 or den * d1 < num * int(dist2[i, 1]))
    return idx2, dist2, good


def unique(idx2, dist2, good, t_cap):
    """-> (owner [t_cap] i32, good_out [nq] u8): smallest (d1, query) keeps the keypoint."""
    owner = np.full(t_cap, -1, np.int32)
    best = {}
    for qi in np.nonzero(good)[0]:
        j = int(idx2[qi, 0])
        k = (int(dist2[qi, 0]), int(qi))
        if j not in best or k < best[j]:
            best[j] = k
    good_out = np.zeros(len(good), np.uint8)
    for j, (_, qi) in best.items():
        owner[j] = qi
        good_out[qi] = 1
    return owner, good_out


def track_rows(idx2, good, kp, frame):
    """-> rows [n,4] f64 = [frame, landmark, x, y] in ascending landmark order."""
    qi = np.nonzero(good)[0]
    j = idx2[qi, 0]
    kp = np.asarray(kp, np.float32)
    return np.stack([np.full(len(qi), float(frame)), qi.astype(np.float64),
                     kp[j, 0].astype(np.float64), kp[j, 1].astype(np.float64)], 1).reshape(-1, 4)
