"""The workgroup rank and scan of csrc/wg_scan.hpp through the C entry points whose
keep flag is a direct input: slam_compact_matches, slam_filter_pairs,
slam_track_rows, slam_reloc_rows, slam_rows_remap and slam_lk_filter, at the counts
where a wave, the 1024-lane workgroup and the chunk loop begin and end, and
slam_map_compact with a block scan that crosses a wave.

Every output is copied or integer data in the order of the input, so the
reference is NumPy boolean indexing and the bar is equality on [:count] and on
count.  An item is one keep pattern; entries past an item's count are set to
"keep" so that reading them shows; the last item of a launch has another count
than the rest, so a running offset that leaked from one item into the next, or
from one chunk of 1024 into the wrong one, moves rows.
"""
import numpy as np
import pytest

import map_life_ref as ml

pytestmark = pytest.mark.gpu

CAP = 2100
COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 2100]
_I = np.arange(CAP)
PATTERNS = {
    "none": np.zeros(CAP, bool),
    "all": np.ones(CAP, bool),
    "even": _I % 2 == 0,
    "lane 63 of every wave": _I % 64 == 63,
    "first of every chunk": _I % 1024 == 0,
    "random half": np.random.default_rng(1).random(CAP) < 0.5,
}
FRAME0 = 40


def _launch(k, shared_count=False):
    """-> (keep [B, CAP] with the entries past each count set, counts [B], rng): the six
    patterns at COUNTS[k] and a seventh item (the random half) at another count."""
    n, other = COUNTS[k], COUNTS[(k + 3) % len(COUNTS)]
    counts = np.array([n] * len(PATTERNS) + [n if shared_count else other], np.int32)
    keep = np.stack(list(PATTERNS.values()) + [PATTERNS["random half"]])
    for b, c in enumerate(counts):
        keep[b, c:] = True
    return keep, counts, np.random.default_rng(100 + k)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(shape, dtype):
    import torch

    return torch.full(shape, -3, dtype=dtype, device="cuda")


def _call(name, *args):
    from slam355 import _lib
    from slam355.device import ptr

    _lib.call(name, *(ptr(a) if hasattr(a, "data_ptr") else a for a in args), None)


def _check(got_count, want_count, pairs):
    """pairs: (device array [B, ...], list of the expected leading rows per item)."""
    got_count = got_count.cpu().numpy()
    assert np.array_equal(got_count, want_count), (got_count, want_count)
    for got, want in pairs:
        got = got.cpu().numpy()
        for b, w in enumerate(want):
            assert len(w) == want_count[b]
            assert np.array_equal(got[b, :len(w)], w), b


def _kept(keep, counts):
    return [np.nonzero(keep[b, :c])[0] for b, c in enumerate(counts)]


@pytest.mark.parametrize("k", range(len(COUNTS)), ids=[str(c) for c in COUNTS])
def test_compact_matches(k):
    import torch

    keep, counts, rng = _launch(k)
    B = len(counts)
    idx2 = rng.integers(0, 60000, (B, CAP, 2)).astype(np.int32)
    ins = [_dev(idx2), _dev(keep.astype(np.uint8)), _dev(counts)]
    pairs, count = _out((B, CAP, 2), torch.int32), _out((B,), torch.int32)
    _call("slam_compact_matches", *ins, CAP, B, None, 0.0, pairs, count)
    sel = _kept(keep, counts)
    want = [np.stack([q, idx2[b, q, 0]], 1) for b, q in enumerate(sel)]
    _check(count, [len(q) for q in sel], [(pairs, want)])


@pytest.mark.parametrize("k", range(len(COUNTS)), ids=[str(c) for c in COUNTS])
def test_filter_pairs(k):
    import torch

    keep, counts, rng = _launch(k)
    B = len(counts)
    pairs = rng.integers(0, 60000, (B, CAP, 2)).astype(np.int32)
    ins = [_dev(pairs), _dev(counts), _dev(keep.astype(np.uint8))]
    out, count = _out((B, CAP, 2), torch.int32), _out((B,), torch.int32)
    _call("slam_filter_pairs", *ins, CAP, B, out, count)
    sel = _kept(keep, counts)
    _check(count, [len(q) for q in sel], [(out, [pairs[b, q] for b, q in enumerate(sel)])])


@pytest.mark.parametrize("k", range(len(COUNTS)), ids=[str(c) for c in COUNTS])
def test_track_rows(k):
    """keep = good and idx2[..., 0] < kp_cap: one good entry in eight names no keypoint."""
    import torch

    good, counts, rng = _launch(k)
    B = len(counts)
    idx2 = rng.integers(0, CAP, (B, CAP, 2)).astype(np.int32)
    idx2[..., 0][rng.random((B, CAP)) < 0.125] = CAP
    keep = good & (idx2[..., 0] < CAP)
    kp = rng.uniform(0, 600, (B, CAP, 5)).astype(np.float32)
    ins = [_dev(idx2), _dev(good.astype(np.uint8)), _dev(counts), _dev(kp)]
    rows, count = _out((B, CAP, 4), torch.float64), _out((B,), torch.int32)
    _call("slam_track_rows", ins[0], ins[1], ins[2], CAP, ins[3], CAP, B, FRAME0, CAP, rows, count)
    sel = _kept(keep, counts)
    want = [np.stack([np.full(len(q), FRAME0 + b), q, kp[b, idx2[b, q, 0], 0], kp[b, idx2[b, q, 0], 1]], 1)
            .astype(np.float64) for b, q in enumerate(sel)]
    _check(count, [len(q) for q in sel], [(rows, want)])


@pytest.mark.parametrize("k", range(len(COUNTS)), ids=[str(c) for c in COUNTS])
def test_reloc_rows(k):
    """keep = 0 <= owner[i] < kp_cap; the map's count is one word for the whole launch."""
    import torch

    keep, counts, rng = _launch(k, shared_count=True)
    B, n = len(counts), int(counts[0])
    owner = np.where(keep, rng.integers(0, CAP, (B, CAP)), rng.choice([-1, CAP, -7], (B, CAP))).astype(np.int32)
    kp = rng.uniform(0, 600, (B, CAP, 5)).astype(np.float32)
    X = rng.normal(0, 5, (CAP, 3))
    ins = [_dev(owner), _dev(np.array([n], np.int32)), _dev(kp), _dev(X)]
    rows, Q, q = (_out((B, CAP, w), torch.float64) for w in (4, 3, 2))
    count = _out((B,), torch.int32)
    _call("slam_reloc_rows", ins[0], ins[1], CAP, ins[2], CAP, ins[3], B, FRAME0, CAP, rows, count, Q, q)
    sel = _kept(keep, counts)
    xy = [kp[b, owner[b, i], :2].astype(np.float64) for b, i in enumerate(sel)]
    want_rows = [np.column_stack([np.full(len(i), FRAME0 + b), i, xy[b]]).astype(np.float64)
                 for b, i in enumerate(sel)]
    _check(count, [len(i) for i in sel], [(rows, want_rows), (Q, [X[i] for i in sel]), (q, xy)])


@pytest.mark.parametrize("k", range(len(COUNTS)), ids=[str(c) for c in COUNTS])
def test_rows_remap(k):
    """keep = remap[landmark] >= 0: a row names landmark k when kept, CAP + k (dead) when not."""
    import torch

    keep, counts, rng = _launch(k)
    B = len(counts)
    remap = np.r_[rng.permutation(CAP), np.full(CAP, -1)].astype(np.int32)
    rows = rng.uniform(0, 600, (B, CAP, 4))
    rows[..., 1] = np.where(keep, _I, CAP + _I)
    ins = [_dev(rows), _dev(counts), _dev(remap)]
    out, count = _out((B, CAP, 4), torch.float64), _out((B,), torch.int32)
    _call("slam_rows_remap", ins[0], ins[1], CAP, B, ins[2], 2 * CAP, out, count)
    sel = _kept(keep, counts)
    want = []
    for b, r in enumerate(sel):
        w = rows[b, r].copy()
        w[:, 1] = remap[r]
        want.append(w)
    _check(count, [len(r) for r in sel], [(out, want)])


@pytest.mark.parametrize("k", range(len(COUNTS)), ids=[str(c) for c in COUNTS])
def test_lk_filter(k):
    """keep = status: err = 0 < max_error and every rounded p2 lies inside the image."""
    import torch

    keep, counts, rng = _launch(k)
    B, H, W = len(counts), 480, 640
    p1 = rng.uniform(0, 600, (B, CAP, 2)).astype(np.float32)
    p2 = np.stack([rng.uniform(1, W - 2, (B, CAP)), rng.uniform(1, H - 2, (B, CAP))], 2).astype(np.float32)
    ins = [_dev(p1), _dev(p2), _dev(keep.astype(np.uint8)), _dev(np.zeros((B, CAP), np.float32)), _dev(counts)]
    tp1, tp2 = _out((B, CAP, 2), torch.float32), _out((B, CAP, 2), torch.float32)
    idx, count = _out((B, CAP), torch.int32), _out((B,), torch.int32)
    _call("slam_lk_filter", ins[0], 2, ins[1], ins[2], ins[3], ins[4], CAP, B, H, W, 1.0, 1, tp1, tp2, idx, count)
    sel = _kept(keep, counts)
    _check(count, [len(i) for i in sel],
           [(tp1, [p1[b, i] for b, i in enumerate(sel)]), (tp2, [np.rint(p2[b, i]) for b, i in enumerate(sel)]),
            (idx, sel)])


def test_map_compact_block_scan_crosses_a_wave():
    """x_cap = 70,000 is 69 blocks of 1024 landmarks: the scan of the block counts
    runs over more than one wave.  A seeded random third of the landmarks is dead."""
    import torch

    cap = 70_000
    rng = np.random.default_rng(70)
    m = ml.new_map(cap)
    m["X"][:] = rng.normal(0, 5, (cap, 3))
    m["desc"][:] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    for f in ml.FIELDS[2:]:
        m[f][:] = rng.integers(0, 50, cap)
    m["X"][rng.random(cap) < 1 / 3] = np.nan
    m["n"] = cap
    want, remap = ml.compact(m)
    src = [_dev(m[f]) for f in ml.FIELDS] + [_dev(np.array([cap], np.int32))]
    dst = [torch.zeros_like(t) for t in src[:-1]]
    d_remap, d_n = _out((cap,), torch.int32), _out((1,), torch.int32)
    _call("slam_map_compact", *src, cap, *dst, d_remap, d_n)
    n = int(d_n.item())
    assert n == want["n"] and 0.6 * cap < n < 0.7 * cap
    assert np.array_equal(d_remap.cpu().numpy(), remap)
    for f, t in zip(ml.FIELDS, dst):
        assert np.array_equal(t.cpu().numpy()[:n], want[f][:n]), f
