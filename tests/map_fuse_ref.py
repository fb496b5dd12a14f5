"""Plain NumPy restatement of fusing duplicate landmarks (include/slam355.h,
"Landmark life cycle", item 5): the candidate pairs, the forest of best
partners, the merge and the track rows after it, written from the header's
definitions as sequential loops.  Test infrastructure only.

A map is the dict of map_life_ref.py.  Every function returns new arrays and
leaves its inputs alone."""
import numpy as np

from map_life_ref import _clamp, copy_map

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def pairs(m, uv, z, idx2, good0, good, owner, nq, px, rel_depth, max_dist):
    """-> the candidate pairs [(b, l, w)] in order of b, then l."""
    cap = len(m["X"])
    n = _clamp(m["n"], cap)
    B, kp_cap = owner.shape
    out = []
    px2 = np.float64(px) * np.float64(px)
    for b in range(B):
        nqb = _clamp(nq[b], cap)
        for l in range(min(nqb, n)):
            if good0[b, l] == 0 or good[b, l] != 0:
                continue
            j = int(idx2[b, l, 0])
            if not 0 <= j < kp_cap:
                continue
            w = int(owner[b, j])
            if not 0 <= w < nqb or w == l or w >= n:
                continue
            if np.isnan(m["X"][l, 0]) or np.isnan(m["X"][w, 0]):
                continue
            if not (np.isfinite(uv[b, l]).all() and np.isfinite(uv[b, w]).all()):
                continue
            du = np.float64(uv[b, l, 0]) - np.float64(uv[b, w, 0])
            dv = np.float64(uv[b, l, 1]) - np.float64(uv[b, w, 1])
            if not du * du + dv * dv <= px2:
                continue
            zl, zw = np.float64(z[b, l]), np.float64(z[b, w])
            with np.errstate(invalid="ignore"):
                if not abs(zl - zw) <= np.float64(rel_depth) * (zl if zl < zw else zw):
                    continue
            if int(_POP[m["desc"][l] ^ m["desc"][w]].sum()) > max_dist:
                continue
            out.append((b, l, w))
    return out


def _rank(found, i):
    """Smaller is better: more often found (negative counts as 0), then the lower index."""
    return (-max(int(found[i]), 0), i)


def fuse(m, uv, z, idx2, good0, good, owner, nq, px=3.0, rel_depth=0.1, max_dist=64):
    """-> (map, to [cap] i32, nfused)."""
    cap = len(m["X"])
    n = _clamp(m["n"], cap)
    found = m["found"]                       # as on entry
    parent = list(range(cap))
    for _, l, w in pairs(m, uv, z, idx2, good0, good, owner, nq, px, rel_depth, max_dist):
        for i, partner in ((l, w), (w, l)):
            if _rank(found, partner) < _rank(found, parent[i]):
                parent[i] = partner
    to = np.arange(cap, dtype=np.int32)
    for i in range(n):
        r = i
        while parent[r] != r:
            r = parent[r]
        to[i] = r
    m = copy_map(m)
    nfused = 0
    for i in range(n):
        r = int(to[i])
        if r == i:
            continue
        m["visible"][r] += m["visible"][i]
        m["found"][r] += m["found"][i]
        m["born"][r] = min(m["born"][r], m["born"][i])
        m["last"][r] = max(m["last"][r], m["last"][i])
        m["X"][i] = np.nan
        nfused += 1
    return m, to, nfused


def _target(v, to):
    """The landmark a row stands for after the fuse, or None for a row copied as it is."""
    x_cap = len(to)
    if not (v >= 0.0 and v < x_cap) or float(int(v)) != v:
        return None
    r = int(to[int(v)])
    return r if 0 <= r < x_cap else None


def rows_fuse(rows, count, to):
    """rows [B,rows_cap,4], count [B] -> (rows_out zero past the new counts, count_out)."""
    B, rows_cap = rows.shape[:2]
    out, cnt = np.zeros_like(rows), np.zeros(B, np.int32)
    for b in range(B):
        c = _clamp(count[b], rows_cap)
        best = {}                            # v' -> (not the survivor's own row, k) of the row kept
        for k in range(c):
            r = _target(rows[b, k, 1], to)
            if r is not None:
                key = (rows[b, k, 1] != r, k)
                if r not in best or key < best[r]:
                    best[r] = key
        for k in range(c):
            r = _target(rows[b, k, 1], to)
            if r is None:
                out[b, cnt[b]] = rows[b, k]
            elif best[r][1] == k:
                out[b, cnt[b]] = [rows[b, k, 0], float(r), rows[b, k, 2], rows[b, k, 3]]
            else:
                continue
            cnt[b] += 1
    return out, cnt
