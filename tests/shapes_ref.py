"""Plain NumPy references for the shape / tie tests of BoW (test_bow_shapes.py),
the stereo-VO pose (test_vo_shapes.py) and map association (test_map_ties.py),
with the input builders that make those comparisons exact.  Test
infrastructure only; nothing here touches a GPU."""
import numpy as np


# ----------------------------------------------------------------------------- BoW
def bow_labels_int(X, C):
    """argmin_j |c_j|^2 - 2 x.c_j in int64, first index on ties.  For bytes and
    integer centres in [0, 255] every product and sum stays below 2^23, so the
    f64 expression of k_bow_hist / oracle.bow.labels has this value exactly in
    any summation order and a tie here is a tie there."""
    X = np.asarray(X).astype(np.int64).reshape(-1, 32)
    C = np.asarray(C)
    Ci = C.astype(np.int64)
    assert np.array_equal(Ci, C) and Ci.min() >= 0 and Ci.max() <= 255
    return np.argmin((Ci * Ci).sum(1)[None, :] - 2 * (X @ Ci.T), axis=1)


def bow_centres(rng, K):
    """K integer centres: every other row full-range bytes, the rest in [0, 2]
    (many natural ties among those), and rows 3, 5 and K-1 equal when K >= 7."""
    C = rng.integers(0, 256, (K, 32))
    C[1::2] = rng.integers(0, 3, (len(C[1::2]), 32))
    if K >= 7:
        C[5] = C[3]
        C[K - 1] = C[3]
    return C.astype(np.float64)


def bow_descriptors(rng, C, B, cap):
    """[B, cap, 32] bytes: full-range rows, rows in [0, 2], and copies of
    centre 3 (a three-way tie that must resolve to 3) when it is planted."""
    d = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    small = rng.random((B, cap)) < 0.4
    d[small] = rng.integers(0, 3, (int(small.sum()), 32), dtype=np.uint8)
    if len(C) >= 7:
        d[rng.random((B, cap)) < 0.1] = C[3].astype(np.uint8)
    return d


def bow_expected(desc, count, C):
    """-> (labels [B, cap] with -1 at and beyond the clamped count, hist [B, K])."""
    B, cap, _ = desc.shape
    K = len(C)
    lab = np.full((B, cap), -1, np.int32)
    hist = np.zeros((B, K), np.int32)
    for b in range(B):
        n = min(max(int(count[b]), 0), cap)
        lab[b, :n] = bow_labels_int(desc[b, :n], C)
        hist[b] = np.bincount(lab[b, :n], minlength=K)
    return lab, hist


# rows of the database that hold a planted tie: r, r + 1 (the neighbouring lane),
# r + 256 (the same lane's second trip), r + 300.  In the third group the lowest
# index sits in a HIGHER lane (250) than a later copy (550 -> lane 38).
BOW_TIE_GROUPS = (0, 37, 250)
BOW_TIE_OFFSETS = (0, 1, 256, 300)


def bow_query_case(rng, K, n_rows=600):
    """-> (db [n_rows, K] i32 in [0, 30], queries [3, K] i32).  Query g differs
    from the rows of group g in bin 0 by one count, so its distance to them is
    2 / (2 p + 1) > 0, and every row outside the groups is strictly farther from
    every query than that."""
    import oracle.bow as ob

    db = rng.integers(0, 31, (n_rows, K))
    planted = np.zeros(n_rows, bool)
    qs = []
    for g, r in enumerate(BOW_TIE_GROUPS):
        p = rng.integers(0, 31, K)
        p[0] = 5 + 10 * g  # K = 1: 5, 15, 25, far from one another
        rows = [r + o for o in BOW_TIE_OFFSETS]
        db[rows] = p
        planted[rows] = True
        q = p.copy()
        q[0] += 1
        qs.append(q)
    qs = np.array(qs)

    def too_close(row):
        return any(ob.chi2(q, row) <= ob.chi2(q, db[r]) for q, r in zip(qs, BOW_TIE_GROUPS))

    for i in np.flatnonzero(~planted):
        while too_close(db[i]):  # K = 1 mostly; redraw until the planted tie is the minimum
            db[i] = rng.integers(0, 31, K)
    return db.astype(np.int32), qs.astype(np.int32)


def bow_query_expected(q, db, n):
    """oracle.bow.chi2 + np.argmin (first index) over db[:n]; n <= 0 -> (-1, -1.0)."""
    import oracle.bow as ob

    if n <= 0:
        return -1, -1.0
    d = [ob.chi2(q.astype(np.int64), db[i].astype(np.int64)) for i in range(n)]
    return int(np.argmin(d)), float(np.min(d))


# ----------------------------------------------------------------------------- stereo-VO pose
def distinct_rel_gap(errs):
    """Smallest relative gap between two distinct values of errs (inf if < 2)."""
    u = np.unique(np.asarray(errs, np.float64))
    if len(u) < 2:
        return np.inf
    return float(np.min(np.diff(u) / u[1:]))


# ----------------------------------------------------------------------------- map association
def map_assoc(Qs, absP, threshold, p2, frame, rel):
    """appendKeyPoints by brute force in k_map_nn / k_map_assoc's own expression:
    d2 = (dx dx + dy dy) + dz dz, first index on ties, new = not (sqrt(best) <
    threshold |rel|), appended indices from the prefix count.  -> (map, rows)."""
    Qs = np.asarray(Qs, np.float64).reshape(-1, 3)
    absP = np.asarray(absP, np.float64).reshape(-1, 3)
    rel = np.asarray(rel, np.float64).reshape(-1, 3)
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    n, M = len(absP), len(Qs)
    if M == 0:
        new = np.ones(n, bool)
        ind = np.zeros(n, np.int64)
    else:
        ind, best = np.zeros(n, np.int64), np.zeros(n)
        for s in range(0, n, 512):  # blocks of queries: the [512, M] table stays small
            dx, dy, dz = (absP[s:s + 512, None, k] - Qs[None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            ind[s:s + 512] = np.argmin(d2, axis=1)
            best[s:s + 512] = d2[np.arange(len(d2)), ind[s:s + 512]]
        gate = threshold * np.sqrt((rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2])
        new = ~(np.sqrt(best) < gate)
    idx = np.where(new, M + np.cumsum(new) - 1, ind)
    rows = np.column_stack([np.full(n, float(frame)), idx.astype(float), p2[:, 0], p2[:, 1]])
    return np.vstack([Qs, absP[new]]), rows.reshape(-1, 4)


def lattice_map(rng, M):
    """M distinct points on the lattice of halves in [-32, 32)^3, in random
    order: half of them fill a quarter of the cube [-4, 4)^3 (equidistant
    neighbours are common there, and they sit in different NN chunks), the
    others are spread thinly (their queries mostly become new points)."""
    cells = np.arange(128 ** 3).reshape(128, 128, 128)
    dense = cells[56:72, 56:72, 56:72].ravel()
    sparse = np.setdiff1d(cells.ravel(), dense)
    flat = np.concatenate([rng.choice(dense, M // 2, replace=False),
                           rng.choice(sparse, M - M // 2, replace=False)])
    flat = rng.permutation(flat)
    return np.stack([flat // 128 ** 2, flat // 128 % 128, flat % 128], 1) / 2.0 - 32.0


def lattice_frame(rng, Qs, N):
    """N queries = a map point plus an offset in {-1, -1/2, 0, 1/2, 1}^3 (every
    distance exact, many equidistant neighbours), rel with |rel| in [2, 6] on
    the lattice, pixel coordinates."""
    absP = Qs[rng.integers(0, len(Qs), N)] + rng.integers(-2, 3, (N, 3)) / 2.0
    rel = rng.integers(-4, 5, (N, 3)) / 2.0
    rel[:, 2] = rng.integers(4, 9, N) / 2.0
    return absP, rel, rng.uniform(0, 1000, (N, 2))
