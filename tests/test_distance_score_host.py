"""prediff_amd.distance_score without a GPU: the constructor and argument refusals, compute() on hand-written states, and the properties
of tests/_distance_ref.py, the fp64 restatement that tests/test_distance_score.py holds the device to."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import _distance_ref as R
from prediff_amd import SEVIRDistanceScore, distance_map
from prediff_amd._lib import PrediffHipError
from prediff_amd.distance_score import METRICS, NO_EVENT


def disc(H, W, cy, cx, radius):
    r, c = np.mgrid[0:H, 0:W]
    return ((r - cy) ** 2 + (c - cx) ** 2 <= radius ** 2).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the class
def test_constructor_refusals():
    for layout in ("NTHWX", "NTHHW", "THWC", "NTWC", "NTHC", "NT"):
        with pytest.raises(ValueError):
            SEVIRDistanceScore(layout=layout)
    with pytest.raises(NotImplementedError):
        SEVIRDistanceScore(mode="3")
    for mode in ("1", "2"):
        with pytest.raises(ValueError):
            SEVIRDistanceScore(mode=mode)
    with pytest.raises(ValueError):
        SEVIRDistanceScore(metrics_list=("hausdorff", "csi"))
    with pytest.raises(ValueError):
        SEVIRDistanceScore(threshold_list=())
    with pytest.raises(ValueError):
        SEVIRDistanceScore(threshold_list=tuple(range(10, 100, 10)))          # nine
    for cutoff in (0, -1.0, math.inf, math.nan, "10", True):
        with pytest.raises(ValueError):
            SEVIRDistanceScore(cutoff=cutoff)
    m = SEVIRDistanceScore(layout="NHWT", mode="1", seq_len=6, threshold_list=(16, 74), metrics_list=("hausdorff",), cutoff=10)
    assert m.keep_seq_len_dim and m.Tk == 6 and m.threshold_list == (16.0, 74.0) and m.cutoff == 10.0 and m.metrics_list == ("hausdorff",)
    d = SEVIRDistanceScore()
    assert d.threshold_list == (16.0, 74.0, 133.0, 160.0, 181.0, 219.0) and d.cutoff is None and d.mode == "0"
    assert SEVIRDistanceScore.METRICS == METRICS == ("med_miss", "med_false", "hausdorff", "baddeley", "frac_both")
    assert len(SEVIRDistanceScore(threshold_list=range(8)).threshold_list) == 8 and NO_EVENT == 2 ** 31 - 1
    assert [(n, dt) for n, dt, _ in SEVIRDistanceScore.STATE] == [("sums", torch.float64), ("counts", torch.int64)]
    assert [shape(m, 6) for _, _, shape in SEVIRDistanceScore.STATE] == [(4, 2, 6), (6, 2, 6)]


def test_cpu_tensors_and_shapes_are_refused():
    x = torch.rand((1, 2, 8, 8, 1))
    with pytest.raises(PrediffHipError):
        distance_map(x, 16)
    with pytest.raises(PrediffHipError):
        SEVIRDistanceScore().update(x, x)
    with pytest.raises(PrediffHipError):
        SEVIRDistanceScore().update_members(x[None], x)
    with pytest.raises(ValueError):
        SEVIRDistanceScore().update(x, x[:, :1])
    with pytest.raises(ValueError):
        SEVIRDistanceScore().update_members(x, x)                             # not (M,) + target.shape
    with pytest.raises(ValueError):
        distance_map(x, 16, layout="NTC")
    with pytest.raises(ValueError):
        distance_map(x, 16, layout="NTHW")                                    # one letter per axis
    SEVIRDistanceScore().sync()                                               # no process group: a no-op


def test_compute_on_a_hand_written_state():
    K, T = 2, 3
    sums = np.zeros((4, K, T))
    counts = np.zeros((6, K, T), np.int64)
    # threshold 0: steps 0, 1, 2 have 2, 1, 0 pairs with both sets; threshold 1: 4 pairs each step, all with both sets
    counts[0] = [[2, 2, 2], [4, 4, 4]]
    counts[2] = [[2, 1, 0], [4, 4, 4]]
    counts[3] = [[2, 2, 2], [4, 4, 0]]
    sums[0] = [[3.0, 1.5, 0.0], [4.0, 8.0, 12.0]]
    sums[1] = [[1.0, 2.5, 0.0], [2.0, 2.0, 2.0]]
    sums[2] = [[10.0, 5.0, 0.0], [20.0, 24.0, 28.0]]
    sums[3] = [[1.0, 3.0, 5.0], [6.0, 10.0, 0.0]]
    m1 = SEVIRDistanceScore(mode="1", seq_len=T, threshold_list=(16, 74))
    m1.sums, m1.counts = torch.from_numpy(sums), torch.from_numpy(counts)
    r = m1.compute()
    assert set(r) == set(METRICS) and all(v.shape == (T, K) for v in r.values())
    assert np.array_equal(r["med_miss"], [[1.5, 1.0], [1.5, 2.0], [np.nan, 3.0]], equal_nan=True)
    assert np.array_equal(r["med_false"], [[0.5, 0.5], [2.5, 0.5], [np.nan, 0.5]], equal_nan=True)
    assert np.array_equal(r["hausdorff"], [[5.0, 5.0], [5.0, 6.0], [np.nan, 7.0]], equal_nan=True)
    assert np.array_equal(r["baddeley"], [[0.5, 1.5], [1.5, 2.5], [2.5, np.nan]], equal_nan=True)
    assert np.array_equal(r["frac_both"], [[1.0, 1.0], [0.5, 1.0], [0.0, 1.0]])
    m2 = SEVIRDistanceScore(mode="2", seq_len=T, threshold_list=(16, 74), metrics_list=("med_miss", "frac_both"))
    m2.sums, m2.counts = torch.from_numpy(sums), torch.from_numpy(counts)
    r2 = m2.compute()
    assert list(r2) == ["med_miss", "frac_both"] and r2["med_miss"].shape == (K,)
    assert math.isnan(r2["med_miss"][0]) and r2["med_miss"][1] == 2.0 and np.array_equal(r2["frac_both"], [0.5, 1.0])
    m0 = SEVIRDistanceScore(mode="0", threshold_list=(16, 74))
    m0.sums, m0.counts = torch.from_numpy(sums[:, :, :1].copy()), torch.from_numpy(counts[:, :, :1].copy())
    r0 = m0.compute()
    assert r0["hausdorff"].shape == (K,) and np.array_equal(r0["hausdorff"], [5.0, 5.0]) and np.array_equal(r0["baddeley"], [0.5, 1.5])
    for k, v in R.compute(sums, counts, "1").items():
        assert np.array_equal(v, r[k], equal_nan=True), k


def test_compute_before_any_update_is_nan_of_the_right_shape():
    e0 = SEVIRDistanceScore().compute()
    e1 = SEVIRDistanceScore(mode="1", seq_len=4, threshold_list=(16, 74, 133)).compute()
    e2 = SEVIRDistanceScore(mode="2", seq_len=4, threshold_list=(16,)).compute()
    assert set(e0) == set(e1) == set(e2) == set(METRICS)
    for met in METRICS:
        assert e0[met].shape == (6,) and e1[met].shape == (4, 3) and e2[met].shape == (1,)
        assert np.isnan(e0[met]).all() and np.isnan(e1[met]).all() and np.isnan(e2[met]).all()
    m = SEVIRDistanceScore()
    m.reset()
    assert m.sums is None and m.counts is None


# ------------------------------------------------------------------------------------------------ the restatement
def test_reference_d2_equals_scipy_edt_on_non_empty_masks():
    rng = np.random.default_rng(5)
    masks = []
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 5), (128, 3), (33, 128), (128, 128)):
        for density in (0.001, 0.05, 0.5):
            m = rng.random((H, W)) < density
            m[rng.integers(H), rng.integers(W)] = True
            masks.append(m)
        for corner in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            m = np.zeros((H, W), bool)
            m[corner] = True
            masks.append(m)
    for m in masks:
        edt = np.rint(ndimage.distance_transform_edt(~m) ** 2).astype(np.int64)
        assert np.array_equal(R.d2_of_mask(m), edt), m.shape
    one = np.zeros((128, 128), bool)
    one[0, 0] = True
    assert R.d2_of_mask(one).max() == 32258 == 2 * 127 ** 2
    assert (R.d2_of_mask(np.zeros((4, 6), bool)) == R.NO_EVENT).all() and (R.d2_of_mask(np.ones((4, 6), bool)) == 0).all()


def test_reference_event_sets():
    d = np.float32(1.0 / 255.0)
    v = np.float32(16.0) * d
    while v / d >= np.float32(16.0):                          # the smallest fp32 whose quotient reaches 16
        v = np.nextafter(v, np.float32(0.0))
    below, on = v, np.nextafter(v, np.float32(1.0))
    assert below / d < np.float32(16.0) <= on / d
    f = np.array([[below, on, np.nan, np.inf, -np.inf, 0.0]], np.float32)
    assert R.event_mask(f, 16).tolist() == [[False, True, False, True, False, False]]
    assert R.event_mask(np.array([[0.25, np.nextafter(np.float32(0.25), np.float32(0.0)), np.nan]], np.float32), 0.25, scaled=False).tolist() == \
        [[True, False, False]]
    assert R.pair_metrics(f, f, 16) == {"skipped": True}


def test_reference_identity_swap_and_shifted_disc():
    rng = np.random.default_rng(9)
    a = (rng.random((24, 31)) ** 4).astype(np.float32)
    b = (rng.random((24, 31)) ** 4).astype(np.float32)
    for cutoff in (None, 10.0):
        same = R.pair_metrics(a, a, 74, cutoff)
        assert same["both"] and (same["med_miss"], same["med_false"], same["hausdorff"], same["baddeley"]) == (0.0, 0.0, 0.0, 0.0)
        ab, ba = R.pair_metrics(a, b, 74, cutoff), R.pair_metrics(b, a, 74, cutoff)
        assert ab["both"] and ab["med_miss"] > 0
        assert ab["med_miss"] == ba["med_false"] and ab["med_false"] == ba["med_miss"]
        assert ab["hausdorff"] == ba["hausdorff"] and ab["baddeley"] == ba["baddeley"] and ab["n_pred"] == ba["n_target"]
    d0, d1 = disc(32, 32, 12, 12, 6), disc(32, 32, 15, 16, 6)
    p = R.pair_metrics(d1, d0, 74)
    assert p["hausdorff"] == 5.0 and p["hausdorff_d2"] == 25 and 0 < p["med_miss"] <= 5 and 0 < p["med_false"] <= 5
    # empty sets: nothing but Baddeley's Delta with a cutoff is defined; two empty sets give 0
    z = np.zeros((32, 32), np.float32)
    e = R.pair_metrics(z, d0, 74)
    assert not e["both"] and e["n_pred"] == 0 and e["med_miss"] is None and e["hausdorff"] is None and e["baddeley"] is None
    ec = R.pair_metrics(z, d0, 74, cutoff=4.0)
    assert ec["med_false"] is None and 0 < ec["baddeley"] <= 4.0
    zz = R.pair_metrics(z, z, 74, cutoff=4.0)
    assert zz["baddeley"] == 0.0 and R.pair_metrics(z, z, 74)["baddeley"] is None
    # a hand-computed pair on a 1 x 5 line: F = {0}, O = {3}: d_F = 0 1 2 3 4, d_O = 3 2 1 0 1
    f, o = np.zeros((1, 5), np.float32), np.zeros((1, 5), np.float32)
    f[0, 0], o[0, 3] = 1.0, 1.0
    h = R.pair_metrics(f, o, 74)
    assert (h["med_miss"], h["med_false"], h["hausdorff"]) == (3.0, 3.0, 3.0) and abs(h["baddeley"] - math.sqrt(29.0 / 5.0)) <= 1e-15
    hc = R.pair_metrics(f, o, 74, cutoff=2.0)                    # w_F = 0 1 2 2 2, w_O = 2 2 1 0 1
    assert abs(hc["baddeley"] - math.sqrt(11.0 / 5.0)) <= 1e-15


def test_reference_state_counts():
    d0, z = disc(16, 16, 6, 6, 3), np.zeros((16, 16), np.float32)
    bad = d0.copy()
    bad[0, 0] = np.nan
    ens = np.stack([d0, z, bad])[None, None]                      # (M = 1, N = 1, T = 3, H, W)
    tgt = np.stack([d0, d0, d0])[None]
    for cutoff, defined in ((None, [1, 0, 0]), (5.0, [1, 1, 0])):
        sums, counts = R.distance_state(R.frame_maps(ens, (74, 300)), R.frame_maps(tgt, (74, 300)), cutoff, True)
        n = int(d0.sum())
        assert counts[:, 0].tolist() == [[1, 1, 0], [0, 0, 1], [1, 0, 0], defined, [n, 0, 0], [n, n, 0]]
        assert counts[:, 1].tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 0], [1, 1, 0] if cutoff else [0, 0, 0], [0, 0, 0], [0, 0, 0]]
        assert (sums[:3] == 0).all()
    s0, c0 = R.distance_state(R.frame_maps(ens, (74,)), R.frame_maps(tgt, (74,)), None, False)
    assert s0.shape == (4, 1, 1) and c0[:, 0, 0].tolist() == [2, 1, 1, 1, int(d0.sum()), 2 * int(d0.sum())]
