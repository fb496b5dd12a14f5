"""BoW kernels beyond the golden's one shape (40 x 100 descriptors, K = 50, 40
database rows): every K branch of chi2 and the kMaxK limit, the second trip of
the 256-lane strides, ties, empty clusters, n_iter = 0.

Descriptors are bytes and centres integers in [0, 255], so |c|^2 - 2 x.c is
exact in f64 in any order: labels and histograms are compared bit for bit with
an int64 reference (shapes_ref.bow_labels_int) and a tie is a real tie.  Query
values are compared with == against oracle.bow.chi2, as test_bow.py does.
"""
import numpy as np
import pytest

import shapes_ref as sr
from oracle import bow as ob

# every K in {1, 7, 8, 9, 64, 127, 128} and cap in {1, 255, 256, 257, 700} once
HIST_CASES = [(1, 1), (7, 255), (8, 256), (9, 257), (64, 700), (127, 257), (128, 700)]
QUERY_K = [1, 7, 8, 9, 50, 128]
QUERY_N_DB = [0, -3, 1, 256, 257, 600]
# (N, K): N on both sides of one 256-lane workgroup, K = 1 and the limit
LLOYD_CASES = [(1, 1), (1, 128), (255, 128), (257, 1), (257, 128), (1000, 128)]


def _hist_case(K, cap):
    rng = np.random.default_rng(1000 * K + cap)
    C = sr.bow_centres(rng, K)
    count = np.array([cap, 0, cap + 3, cap // 2, 1, max(cap - 1, 0)], np.int32)
    desc = sr.bow_descriptors(rng, C, len(count), cap)
    return C, desc, count


def _lloyd_case(N, K):
    """X bytes in [0, 200); centres = rows of X where there are enough, else
    random integers; for K = 128, centre 5 duplicates centre 2 (the first index
    takes its points) and centre 77 is all 255 (every point is nearer to another
    centre): both stay empty."""
    rng = np.random.default_rng(10 * N + K)
    X = rng.integers(0, 200, (N, 32), dtype=np.uint8)
    if N >= K:
        C0 = X[rng.choice(N, K, replace=False)].astype(np.float64)
    else:
        C0 = rng.integers(0, 200, (K, 32)).astype(np.float64)
    empty = []
    if K == 128:
        C0[5] = C0[2]
        C0[77] = 255.0
        empty = [5, 77]
    return X, C0, empty


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,cap", HIST_CASES)
def test_int64_labels_agree_with_oracle(K, cap):
    """The int64 reference and oracle.bow.labels (f64, BLAS order) agree on
    integer inputs, ties included; the planted three-way tie resolves to 3."""
    C, desc, _ = _hist_case(K, cap)
    X = desc.reshape(-1, 32)
    ref = sr.bow_labels_int(X, C)
    assert np.array_equal(ob.labels(X, C), ref)
    if K >= 7:
        same = np.all(X == C[3].astype(np.uint8), axis=1)
        assert (same.any() or cap == 1) and np.all(ref[same] == 3)
        assert not np.any(ref == 5) and not np.any(ref == K - 1)


@pytest.mark.parametrize("N,K", LLOYD_CASES)
def test_lloyd_cases_have_empty_clusters_and_exact_first_step(N, K):
    X, C0, empty = _lloyd_case(N, K)
    lab0 = sr.bow_labels_int(X, C0)
    assert np.array_equal(ob.labels(X, C0), lab0)
    for j in empty:
        assert not np.any(lab0 == j)
    C1, _ = ob.lloyd(X, C0, 1)
    for j in range(K):  # one exact integer sum divided once; empty: unchanged
        m = lab0 == j
        want = X[m].astype(np.int64).sum(0) / m.sum() if m.any() else C0[j]
        assert np.array_equal(C1[j], want), j


@pytest.mark.parametrize("K", QUERY_K)
def test_query_case_minimum_is_the_planted_tie(K):
    db, qs = sr.bow_query_case(np.random.default_rng(K), K)
    for q, r in zip(qs, sr.BOW_TIE_GROUPS):
        d = np.array([ob.chi2(q.astype(np.int64), row.astype(np.int64)) for row in db])
        tied = np.flatnonzero(d == d.min())
        assert d.min() > 0 and list(tied) == [r + o for o in sr.BOW_TIE_OFFSETS]
        assert sr.bow_query_expected(q, db, 600) == (r, d.min())


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("K,cap", HIST_CASES)
def test_gpu_labels_and_histograms_exact(K, cap):
    import torch
    from slam355 import bag_of_words as bw

    C, desc, count = _hist_case(K, cap)
    elab, ehist = sr.bow_expected(desc, count, C)
    dev = torch.device("cuda")
    h, lab = bw.histograms(torch.from_numpy(desc).to(dev), torch.from_numpy(count).to(dev),
                           torch.from_numpy(C).to(dev), labels=True)
    assert np.array_equal(lab.cpu().numpy(), elab)  # -1 at and beyond the clamped count
    assert np.array_equal(h.cpu().numpy(), ehist)
    # count = None: every row
    full = np.full(len(count), cap, np.int32)
    elab, ehist = sr.bow_expected(desc, full, C)
    h, lab = bw.histograms(torch.from_numpy(desc).to(dev), None, torch.from_numpy(C).to(dev),
                           labels=True)
    assert np.array_equal(lab.cpu().numpy(), elab) and np.array_equal(h.cpu().numpy(), ehist)


@pytest.mark.gpu
def test_gpu_more_than_128_clusters_is_refused():
    import torch
    from slam355 import _lib, bag_of_words as bw
    from slam355.device import ptr, stream_ptr

    dev = torch.device("cuda")
    K = 129
    C = torch.zeros((K, 32), dtype=torch.float64, device=dev)
    desc = torch.zeros((2, 4, 32), dtype=torch.uint8, device=dev)
    hist = torch.full((2, K), -7, dtype=torch.int32, device=dev)
    lab = torch.full((2, 4), -7, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.SlamError):
        _lib.call("slam_bow_histograms", ptr(desc), None, 4, 2, 4, ptr(C), K, ptr(lab), ptr(hist),
                  stream_ptr())
    torch.cuda.synchronize()
    assert bool((hist == -7).all()) and bool((lab == -7).all())  # nothing was launched
    with pytest.raises(_lib.SlamError):
        bw.histograms(desc, None, C)
    q = torch.zeros((1, K), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.SlamError):
        bw.query(q, q, torch.ones(1, dtype=torch.int32, device=dev))
    with pytest.raises(_lib.SlamError):
        bw.lloyd(desc.reshape(-1, 32), np.zeros((K, 32)), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("K", QUERY_K)
def test_gpu_query_ties_and_strides(K):
    """600 database rows (three trips of the 256-lane stride), n_db on both
    sides of 256, ties at a non-zero distance inside a lane, between
    neighbouring lanes and with the lowest index in the higher lane."""
    import torch
    from slam355 import bag_of_words as bw

    rng = np.random.default_rng(K)
    db, qs = sr.bow_query_case(rng, K)
    # the three tie queries, three database rows (distance 0 to themselves) and
    # three random histograms, each against every n_db
    q = np.concatenate([qs, db[[1, 299, 599]], rng.integers(0, 31, (3, K)).astype(np.int32)])
    q = np.repeat(q, len(QUERY_N_DB), axis=0)
    n = np.tile(np.array(QUERY_N_DB, np.int32), len(q) // len(QUERY_N_DB))
    dev = torch.device("cuda")
    idx, val = bw.query(torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev),
                        torch.from_numpy(n).to(dev))
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    for k in range(len(q)):
        ei, ev = sr.bow_query_expected(q[k], db, int(n[k]))
        assert int(idx[k]) == ei and float(val[k]) == ev, (k, int(n[k]))


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", LLOYD_CASES)
def test_gpu_lloyd_shapes(N, K):
    import torch
    from slam355 import bag_of_words as bw

    X, C0, empty = _lloyd_case(N, K)
    Xd = torch.from_numpy(X).cuda()
    # n_iter = 0: centres untouched, labels of the given centres
    C, lab = bw.lloyd(Xd, C0, 0)
    assert np.array_equal(C.cpu().numpy(), C0)
    assert np.array_equal(lab.cpu().numpy(), sr.bow_labels_int(X, C0))
    # n_iter = 1 from integer centres: exact sums divided once
    eC, elab = ob.lloyd(X, C0, 1)
    C, lab = bw.lloyd(Xd, C0, 1)
    C = C.cpu().numpy()
    assert np.array_equal(C, eC)
    for j in empty:
        assert np.array_equal(C[j], C0[j])  # an empty cluster keeps its centre, bit for bit
    assert np.array_equal(lab.cpu().numpy(), elab)
    for it in (2, 5):
        eC, elab = ob.lloyd(X, C0, it)
        C, lab = bw.lloyd(Xd, C0, it)
        assert np.allclose(C.cpu().numpy(), eC, rtol=1e-12, atol=1e-12)
        assert np.array_equal(lab.cpu().numpy(), elab)
