"""prediff_amd.probability_matching without a GPU: the NumPy restatement (tests/_probmatch_ref.py) pinned on hand-computed cases and on the
properties of the definitions, and the argument checks of the three public functions."""
import numpy as np
import pytest
import torch

import _probmatch_ref as R
from prediff_amd import match_cdf, probability_matched_mean, rank_frames

SIZES = ((5, 7), (37, 53), (128, 128))
THR = 16 / 255


def f32(a):
    return np.asarray(a, np.float32)


def radar(rng, shape, zeros=0.7):
    """mostly exact zeros, the rest from 8 distinct values around the threshold: ties everywhere"""
    levels = f32([0.02, 0.05, 0.08, 0.11, 0.2, 0.35, 0.6, 0.9])
    v = levels[rng.integers(0, 8, shape)]
    return np.where(rng.random(shape) < zeros, np.float32(0), v).astype(np.float32)


# ------------------------------------------------------------------------------------------------ hand-computed
def test_restatement_match_cdf_by_hand_with_ties():
    x = f32([3, 1, 1, 2, 3, 0]).reshape(1, 1, 2, 3, 1)
    ref = f32([20, 10, 50, 20, 40, 30]).reshape(1, 1, 2, 3, 1)
    # order_x = [5, 1, 2, 3, 0, 4] (ties by pixel index), s = [10, 20, 20, 30, 40, 50]
    assert np.array_equal(R.rank_frames(x)[1].ravel(), [5, 1, 2, 3, 0, 4])
    assert np.array_equal(R.rank_frames(x)[0].ravel(), f32([0, 1, 1, 2, 3, 3]))
    assert np.array_equal(R.match_cdf(x, ref).ravel(), f32([40, 20, 20, 30, 50, 10]))


def test_restatement_threshold_cap_by_hand():
    ref = f32([3, 4, 0, 2]).reshape(1, 1, 2, 2, 1)          # n_r = 3 wet pixels above thr = 1
    x = f32([0, 5, 0, 2]).reshape(1, 1, 2, 2, 1)            # n_x = 2 < n_r: s = [0, 2, 3, 4] -> [0, 1, 3, 4]
    assert np.array_equal(R.match_cdf(x, ref, threshold=1.0).ravel(), f32([0, 4, 1, 3]))
    assert np.array_equal(R.match_cdf(x, ref).ravel(), f32([0, 4, 2, 3]))
    ref = f32([0, 4, 0, 2]).reshape(1, 1, 2, 2, 1)          # n_r = 2
    x = f32([0, 5, 3, 2]).reshape(1, 1, 2, 2, 1)            # n_x = 3 > n_r: the rule is a no-op, s = [0, 0, 2, 4]
    assert np.array_equal(R.match_cdf(x, ref, threshold=1.0).ravel(), f32([0, 4, 2, 0]))
    assert np.array_equal(R.match_cdf(x, ref).ravel(), f32([0, 4, 2, 0]))


def test_restatement_pmm_by_hand():
    ens = f32([[1, 5, 2, 8], [3, 1, 4, 6], [2, 9, 0, 7]]).reshape(3, 1, 1, 2, 2, 1)
    mean, q = R.pmm_parts(ens.reshape(3, 4))
    assert np.array_equal(mean, f32([2, 5, 2, 7]))
    assert np.array_equal(q, f32([1, 2, 5, 8]))             # P = [0 1 1 2 2 3 4 5 6 7 8 9], q[r] = P[3 r + 1]
    assert np.array_equal(R.probability_matched_mean(ens).ravel(), f32([1, 5, 2, 8]))   # order_mean = [0, 2, 1, 3]


def test_restatement_non_finite_and_signed_zero_rules():
    x = f32([0.0, -0.0, 1.0, -1.0]).reshape(1, 1, 2, 2, 1)
    srt, order = R.rank_frames(x)
    assert np.array_equal(order.ravel(), [3, 0, 1, 2])
    assert np.array_equal(srt.ravel().view(np.uint32), f32([-1.0, 0.0, -0.0, 1.0]).view(np.uint32))    # the original bits
    out = R.match_cdf(x, x)
    assert np.array_equal(out.ravel().view(np.uint32), f32([0.0, 0.0, 1.0, -1.0]).view(np.uint32))     # -0.0 read as +0.0 in ref
    for bad in (np.nan, np.inf, -np.inf):
        y = np.concatenate([x, x], axis=1)
        y[0, 1, 1, 0, 0] = bad
        srt, order = R.rank_frames(y)
        assert (order[0, 1] == -1).all() and np.isnan(srt[0, 1]).all() and np.array_equal(order[0, 0], [3, 0, 1, 2])
        xx = np.concatenate([x, x], axis=1)
        out = R.match_cdf(xx, y)
        assert np.isnan(out[0, 1]).all() and np.isfinite(out[0, 0]).all()
        out = R.match_cdf(y, xx)
        assert np.isnan(out[0, 1]).all() and np.isfinite(out[0, 0]).all()
        ens = np.stack([xx, y, xx])
        out = R.probability_matched_mean(ens)
        assert np.isnan(out[0, 1]).all() and np.isfinite(out[0, 0]).all()


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_properties(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    thr = np.float32(THR)
    for make in (lambda: rng.random((1, 1, H, W, 1), dtype=np.float32), lambda: radar(rng, (1, 1, H, W, 1)),
                 lambda: radar(rng, (1, 1, H, W, 1), zeros=0.9)):
        x, ref = make(), make()
        assert np.array_equal(R.match_cdf(x, x), x)                                     # idempotence
        order = R.rank_frames(x)[1].ravel()
        out = R.match_cdf(x, ref)
        assert np.array_equal(np.sort(out.ravel()), np.sort(ref.ravel()))               # the multiset of ref
        assert (np.diff(out.ravel()[order]) >= 0).all()                                 # monotone along order_x
        out = R.match_cdf(x, ref, threshold=THR)
        assert (np.diff(out.ravel()[order]) >= 0).all()
        n_x = int((x > thr).sum())
        assert int((out > thr).sum()) <= n_x                                            # matching never grows the rain area
        if int((ref > thr).sum()) <= n_x:
            assert np.array_equal(out, R.match_cdf(x, ref))                             # ... and is a no-op otherwise
        assert np.array_equal(R.probability_matched_mean(x[None]), x)                   # M = 1
        assert np.array_equal(R.probability_matched_mean(np.stack([x] * 5)), x)         # identical members


@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_pmm_is_invariant_under_member_permutation(H, W):
    rng = np.random.default_rng(H + W)
    ens = (rng.integers(0, 256, (7, 1, 2, H, W, 1)) / 256).astype(np.float32)          # k / 256: every fp64 sum is exact
    out = R.probability_matched_mean(ens)
    for _ in range(2):
        assert np.array_equal(R.probability_matched_mean(ens[rng.permutation(7)]), out)
    assert np.isin(out, ens).all()                                                      # a selection of member values


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_raise_value_errors():
    x = torch.zeros((2, 3, 4, 5, 1))
    with pytest.raises(ValueError, match="last axis 1"):
        rank_frames(torch.zeros((2, 3, 4, 5)))
    with pytest.raises(ValueError, match="last axis 1"):
        match_cdf(torch.zeros((2, 3, 4, 5, 2)), x)
    with pytest.raises(ValueError, match="last axis 1"):
        probability_matched_mean(torch.zeros((2, 2, 3, 4, 5, 3)))
    with pytest.raises(ValueError, match=r"\(M, B, T, H, W, 1\)"):
        probability_matched_mean(x)
    with pytest.raises(ValueError, match="float32"):
        rank_frames(x.double())
    big = torch.zeros((1, 1, 129, 128, 1))
    for call in (lambda: rank_frames(big), lambda: match_cdf(big, big), lambda: probability_matched_mean(big[None])):
        with pytest.raises(ValueError, match=r"129 x 128 are not supported: H W <= 16384"):
            call()
    for ref in (torch.zeros((2, 2, 4, 5, 1)), torch.zeros((1, 3, 4, 5, 1)), torch.zeros((2, 3, 5, 4, 1)), torch.zeros((1, 2, 3, 4, 5, 1))):
        with pytest.raises(ValueError, match="ref must be"):
            match_cdf(x, ref)
    with pytest.raises(ValueError, match="threshold must be None or a finite number"):
        match_cdf(x, x, threshold=float("nan"))
    with pytest.raises(ValueError, match="threshold must be None or a finite number"):
        match_cdf(x, x, threshold="wet")
    for M in (0, 513):
        with pytest.raises(ValueError, match=rf"holds {M} members: 1 \.\. 512"):
            probability_matched_mean(torch.zeros((M, 1, 1, 1, 1, 1)))
    nc = torch.zeros((2, 3, 5, 4, 1)).transpose(2, 3)
    assert nc.shape == x.shape and not nc.is_contiguous()
    with pytest.raises(ValueError, match="x must be contiguous"):
        rank_frames(nc)
    with pytest.raises(ValueError, match="x must be contiguous"):
        match_cdf(nc, x)
    with pytest.raises(ValueError, match="ref must be contiguous"):
        match_cdf(x, nc)
    with pytest.raises(ValueError, match="ens must be contiguous"):
        probability_matched_mean(nc[None].expand(2, 2, 3, 4, 5, 1))
    with pytest.raises(ValueError, match="x is on cpu, ref on meta"):
        match_cdf(x, torch.zeros((2, 3, 4, 5, 1), device="meta"))
    for call in (lambda: rank_frames(x), lambda: match_cdf(x, x), lambda: match_cdf(x, x[:, :1].contiguous(), threshold=THR),
                 lambda: probability_matched_mean(x[None])):
        with pytest.raises(ValueError, match="no CPU path"):
            call()
