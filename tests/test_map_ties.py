"""Map association (k_map_nn, k_map_assoc) where test_mapping.py's goldens do
not reach: exact nearest-neighbour ties (inside an NN chunk and between chunk
partials), the gate at equality, M on the 1024-point chunk boundary, N on the
256-query and 1024-row tile boundaries, appended indices that continue across
association tiles, all-matched and all-new frames.

Coordinates lie on a lattice of halves, so every squared distance is exact and
equal distances are exact ties.  The reference is brute force with the
kernel's own expression and the first index on ties (shapes_ref.map_assoc);
scipy's KDTree leaves ties unspecified, so the oracle is used only to check
that reference on tie-free input.  Rows and map are compared bit for bit.
"""
import numpy as np
import pytest

import shapes_ref as sr
from oracle import mapping as om

THR = 0.25
M_CASES = [1023, 1024, 1025, 2049]
N_CASES = [1, 256, 257, 1024, 1025]


def _lattice_case(M, N):
    rng = np.random.default_rng(100 * M + N)
    Qs = sr.lattice_map(rng, M)
    absP, rel, p2 = sr.lattice_frame(rng, Qs, N)
    return Qs, absP, rel, p2


def _cross_chunk_case():
    """M = 2049.  Queries 0 / 1: equidistant to map indices j and j + 1024 (one in
    each of two chunks; the lower index stored in the first chunk, and for query
    1 the pair reversed in space); query 2: equidistant to j2 and j2 + 1 in one
    chunk; query 3: equidistant to indices 1000, 1030 and 2048 (three chunks).
    The planted landmarks lie outside the lattice cube, far from the rest."""
    Qs, absP, rel, p2 = _lattice_case(2049, 8)
    j, j2 = 517, 1500
    Qs[j], Qs[j + 1024] = [40.5, 40, 40], [39.5, 40, 40]
    Qs[j + 1], Qs[j + 1025] = [39.5, 50, 40], [40.5, 50, 40]
    Qs[j2], Qs[j2 + 1] = [60, 40, 40.5], [60, 40, 39.5]
    Qs[1000], Qs[1030], Qs[2048] = [80.5, 0, 0], [80, 0.5, 0], [80, 0, 0.5]
    absP[:4] = [[40, 40, 40], [40, 50, 40], [60, 40, 40], [80, 0, 0]]
    rel[:4] = [0, 0, 4]  # gate 1 > 1/2: matched
    return Qs, absP, rel, p2, [j, j + 1, j2, 1000]


def _gate_case():
    """rel = (0, 0, 6), threshold 0.5: the gate is exactly 3."""
    Qs = np.array([[0.0, 0, 0], [100, 0, 0]])
    absP = np.array([[3.0, 0, 0], [2.5, 0, 0], [100, 0, -3], [100, 2.5, 0], [0, 0, 0]])
    rel = np.tile([0.0, 0, 6], (5, 1))
    p2 = np.arange(10.0).reshape(5, 2)
    return Qs, absP, rel, p2, [2, 0, 3, 1, 0]  # 3 < 3 is false: new; 2.5 < 3: matched


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("M,N", [(0, 5), (1, 3), (1025, 300), (3000, 700)])
def test_brute_force_equals_kdtree_oracle_without_ties(M, N):
    rng = np.random.default_rng(M + N)
    Qs = rng.uniform(-50, 50, (M, 3))
    rel = rng.uniform(-20, 20, (N, 3)) + [0, 0, 30]
    src = Qs[rng.integers(0, M, N)] if M else np.zeros((N, 3))
    absP = src + rng.normal(0, 1, (N, 1)) * rng.choice([0.01, 1.0], (N, 1))
    p2 = rng.uniform(0, 1000, (N, 2))
    Qo, rows = om.append_keypoints(Qs, absP, 0.01, p2, 3, rel)
    Qb, rb = sr.map_assoc(Qs, absP, 0.01, p2, 3, rel)
    assert np.array_equal(Qb, Qo) and np.array_equal(rb, rows)
    if M > 1:
        assert M < len(Qo) < M + N  # both branches


@pytest.mark.parametrize("M", M_CASES)
def test_lattice_cases_hold_ties_and_both_branches(M):
    Qs, absP, rel, p2 = _lattice_case(M, 1300)
    assert len(np.unique(Qs, axis=0)) == M
    Qo, rows = sr.map_assoc(Qs, absP, THR, p2, 7, rel)
    new = rows[:, 1] >= M
    for tile in (slice(0, 1024), slice(1024, 1300)):  # run > 0 matters in the second tile
        assert new[tile].any() and (~new[tile]).any()
    assert np.array_equal(rows[new, 1], M + np.arange(new.sum()))
    d = absP[:, None, :] - Qs[None, :, :]
    d2 = (d ** 2).sum(2)  # exact on the lattice
    tie = d2 == d2.min(1, keepdims=True)
    assert (tie.sum(1) > 1).sum() >= 100  # exact ties are common
    cross = (tie[:, :1024].any(1) & tie[:, 1024:].any(1)).sum()
    print(f"M = {M}: {new.sum()} new, {(tie.sum(1) > 1).sum()} tied queries, {cross} across chunks")
    if M == 2049:  # ties between a landmark of the first chunk and one of a later chunk too
        assert cross >= 50
    # the gate at equality occurs too: sqrt(best) == threshold |rel| -> new
    gate = THR * np.sqrt((rel ** 2).sum(1))
    assert np.all(new[np.sqrt(d2.min(1)) == gate])


def test_planted_cases_expect_the_lowest_index():
    Qs, absP, rel, p2, want = _cross_chunk_case()
    _, rows = sr.map_assoc(Qs, absP, THR, p2, 0, rel)
    assert list(rows[:4, 1]) == want
    Qs, absP, rel, p2, want = _gate_case()
    Qo, rows = sr.map_assoc(Qs, absP, 0.5, p2, 0, rel)
    assert list(rows[:, 1]) == want and np.array_equal(Qo[2:], absP[[0, 2]])


# ----------------------------------------------------------------------------- GPU
def _gpu_append(Qs, absP, rel, p2, thr, frame, count=None):
    """-> (rows [N,4] as written into a NaN-filled buffer, map after the call)."""
    import torch
    from slam355.mapping import MapStore

    dev = torch.device("cuda")
    N = len(absP)
    store = MapStore(capacity=len(Qs) + N, max_queries=max(N, 1), Qs=Qs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)  # noqa: E731
    out = torch.full((max(N, 1), 4), float("nan"), dtype=torch.float64, device=dev)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    rows = store.append(t(absP), t(rel), t(p2), frame, threshold=thr, count=cnt, rows=out)
    return rows.cpu().numpy(), store.points().cpu().numpy()


def _check(case, thr=THR, frame=7, count=None):
    Qs, absP, rel, p2 = case[:4]
    n = len(absP) if count is None else count
    rows, pts = _gpu_append(Qs, absP, rel, p2, thr, frame, count)
    Qo, erows = sr.map_assoc(Qs, absP[:n], thr, p2[:n], frame, rel[:n])
    assert np.array_equal(rows[:n], erows)
    assert np.all(np.isnan(rows[n:]))  # rows past count are not written
    assert np.array_equal(pts, Qo)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("M", M_CASES)
def test_gpu_lattice_ties_across_chunk_boundaries(M):
    _check(_lattice_case(M, 1300))


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_CASES)
def test_gpu_lattice_query_tile_boundaries(N):
    _check(_lattice_case(1025, N))


@pytest.mark.gpu
def test_gpu_tie_between_chunk_partials_takes_the_lower_index():
    case = _cross_chunk_case()
    rows = _check(case)
    assert list(rows[:4, 1]) == case[4]


@pytest.mark.gpu
def test_gpu_device_count_below_n():
    _check(_lattice_case(1025, 1300), count=1100)  # the second tile ends early
    _check(_lattice_case(1025, 1300), count=0)
    _check(_lattice_case(1025, 1300), count=1500)  # clamped to N


@pytest.mark.gpu
def test_gpu_gate_at_equality_is_new():
    case = _gate_case()
    rows = _check(case, thr=0.5)
    assert list(rows[:, 1]) == case[4]


@pytest.mark.gpu
def test_gpu_all_matched_all_new_and_empty_map():
    Qs, absP, rel, p2 = _lattice_case(1025, 1300)
    # every point is a landmark itself: distance 0 < gate, the map keeps its size
    hit = (Qs[np.random.default_rng(0).integers(0, 1025, 1300)], rel, p2)
    rows = _check((Qs, *hit))
    assert np.all(rows[:, 1] < 1025)
    # threshold 0: nothing is below the gate, all 1300 points are appended in order
    rows = _check((Qs, absP, rel, p2), thr=0.0)
    assert np.array_equal(rows[:, 1], 1025 + np.arange(1300.0))
    # far from every landmark, positive threshold
    rows = _check((Qs, absP + 500.0, rel, p2))
    assert np.array_equal(rows[:, 1], 1025 + np.arange(1300.0))
    # an empty map makes every point new
    rows = _check((np.zeros((0, 3)), absP, rel, p2))
    assert np.array_equal(rows[:, 1], np.arange(1300.0))
