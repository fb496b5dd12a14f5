"""Plain NumPy restatement of the landmark life cycle (include/slam355.h,
"Landmark life cycle"): score, spawn, cull, compact and the row remap, written
from the header's definitions as sequential loops.  Test infrastructure only.

A map is a dict: X [cap,3] f64, desc [cap,32] u8, visible / found / born /
last [cap] i32 and n (int).  Every function returns new arrays and leaves its
inputs alone."""
import numpy as np

FIELDS = ("X", "desc", "visible", "found", "born", "last")


def new_map(cap):
    m = dict(X=np.zeros((cap, 3)), desc=np.zeros((cap, 32), np.uint8), n=0)
    for k in FIELDS[2:]:
        m[k] = np.zeros(cap, np.int32)
    return m


def copy_map(m):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()}


def add(m, X, desc, frame=0):
    """What LandmarkMap.add does: a landmark enters as `spawn` would make it."""
    m = copy_map(m)
    n, k = m["n"], len(X)
    m["X"][n:n + k], m["desc"][n:n + k] = X, desc
    m["visible"][n:n + k] = m["found"][n:n + k] = 1
    m["born"][n:n + k] = m["last"][n:n + k] = frame
    m["n"] = n + k
    return m


def _clamp(v, hi):
    return min(max(int(v), 0), hi)


def score(m, uv, good, nq, frame0):
    """uv [B,cap,2] f32, good [B,cap] u8, nq [B]: entries >= nq_b are not used."""
    m = copy_map(m)
    cap = len(m["X"])
    for b in range(len(nq)):
        k = _clamp(nq[b], cap)
        seen = np.isfinite(uv[b, :k, 0])
        hit = good[b, :k] != 0
        m["visible"][:k] += seen.astype(np.int32)
        m["found"][:k] += hit.astype(np.int32)
        m["last"][:k] = np.where(hit, np.maximum(m["last"][:k], frame0 + b), m["last"][:k])
    return m


def spawn(m, Xc, pairs, count, kp, desc, nkp, owner, poses, flags, z_min, z_max, frame0, rows,
          rows_count):
    """-> (map, owner, rows, rows_count, spawned [B] i32, dropped)."""
    m, owner, rows = copy_map(m), owner.copy(), rows.copy()
    rows_count = np.asarray(rows_count, np.int32).copy()
    B, p_cap = Xc.shape[:2]
    kp_cap, rows_cap, cap = kp.shape[1], rows.shape[1], len(m["X"])
    n0 = _clamp(m["n"], cap)
    spawned = np.zeros(B, np.int32)
    r = 0                                       # candidates so far
    for b in range(B):
        rc = _clamp(rows_count[b], rows_cap)
        if flags[b]:
            taken = set()
            T = np.asarray(poses[b], np.float64).reshape(4, 4)
            for k in range(_clamp(count[b], p_cap)):
                j = int(pairs[b, k, 0])
                if not 0 <= j < _clamp(nkp[b], kp_cap) or owner[b, j] != -1 or j in taken:
                    continue
                x, y, z = (np.float64(v) for v in Xc[b, k])
                if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z) and z_min < z < z_max):
                    continue
                taken.add(j)                    # a candidate, accepted or not
                i = n0 + r
                r += 1
                if i >= cap:
                    continue
                m["X"][i] = [((T[c, 0] * x + T[c, 1] * y) + T[c, 2] * z) + T[c, 3] for c in range(3)]
                m["desc"][i] = desc[b, j]
                m["visible"][i] = m["found"][i] = 1
                m["born"][i] = m["last"][i] = frame0 + b
                owner[b, j] = i
                if rc < rows_cap:
                    rows[b, rc] = [frame0 + b, i, np.float64(kp[b, j, 0]), np.float64(kp[b, j, 1])]
                rc += 1
                spawned[b] += 1
        rows_count[b] = min(rc, rows_cap)
    m["n"] = min(n0 + r, cap)
    return m, owner, rows, rows_count, spawned, max(n0 + r - cap, 0)


def cull(m, now, min_visible=4, ratio=(1, 4), age=4, min_found=2):
    """-> (map, nculled); Python integers, so no product overflows."""
    m = copy_map(m)
    died = 0
    for i in range(_clamp(m["n"], len(m["X"]))):
        if np.isnan(m["X"][i, 0]):
            continue
        v, f, born = int(m["visible"][i]), int(m["found"][i]), int(m["born"][i])
        if (v >= min_visible and ratio[1] * f < ratio[0] * v) or (now - born >= age and f < min_found):
            m["X"][i] = np.nan
            died += 1
    return m, died


def compact(m):
    """-> (map with the live landmarks of [0, n) moved to the front in their
    order -- entries past the new n are zeros here and unspecified on the
    device --, remap [cap] i32)."""
    cap = len(m["X"])
    n = _clamp(m["n"], cap)
    live = np.nonzero(~np.isnan(m["X"][:n, 0]))[0]
    out = new_map(cap)
    for k in FIELDS:
        out[k][:len(live)] = m[k][live]
    out["n"] = len(live)
    remap = np.full(cap, -1, np.int32)
    remap[live] = np.arange(len(live), dtype=np.int32)
    return out, remap


def rows_remap(rows, count, remap):
    """rows [B,rows_cap,4], count [B] -> (rows_out zero past the new counts, count_out)."""
    B, rows_cap = rows.shape[:2]
    x_cap = len(remap)
    out, cnt = np.zeros_like(rows), np.zeros(B, np.int32)
    for b in range(B):
        for k in range(_clamp(count[b], rows_cap)):
            v = rows[b, k, 1]
            if not (v > -1.0 and v < x_cap) or remap[int(v)] < 0:
                continue
            out[b, cnt[b]] = [rows[b, k, 0], remap[int(v)], rows[b, k, 2], rows[b, k, 3]]
            cnt[b] += 1
    return out, cnt
