"""prediff_amd.scale_score on the device (scale_energy, SEVIRScaleScore) against tests/_scale_ref.py, the numpy restatement (itself checked
in tests/test_scale_score_host.py).

Tolerances.  Q_l, the energy state and the counts are integers: equal.  compute(): |got - ref| <= 1e-12 max(1, |ref|) -- the integers
are equal, and each value is at most a few fp64 operations from them."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import _scale_ref as R
from prediff_amd import SEVIRScaleScore, scale_energy
from prediff_amd import _lib as L
from prediff_amd._lib import PrediffHipError
from prediff_amd.scale_score import DIVISOR, METRICS

pytestmark = pytest.mark.gpu

DYADIC = [(2, 2), (4, 4), (8, 8), (64, 64), (128, 128)]
PADDED = [(1, 1), (3, 5), (9, 1), (33, 40), (65, 128), (128, 3), (63, 65)]
THRESHOLDS = {1: (74,), 3: (16, 74, 133), 8: (8, 16, 40, 74, 100, 133, 181, 219)}
ON = 1.0                                       # 255 on the 0-255 scale: an event of every threshold used here


def cuda5(x):
    """(N, T, H, W) numpy -> NTHWC tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(x))[..., None].cuda()


def energy_masks(H, W):
    """(names, masks (P, H, W) bool)"""
    rng = np.random.default_rng(100 * H + W)
    r, c = np.mgrid[0:H, 0:W]
    masks = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool), "checkerboard": (r + c) % 2 == 0,
             "one column": c == W // 3, "random 0.001": rng.random((H, W)) < 0.001, "random 0.5": rng.random((H, W)) < 0.5}
    for name, (y, x) in {"corner 00": (0, 0), "corner 0W": (0, W - 1), "corner H0": (H - 1, 0), "corner HW": (H - 1, W - 1)}.items():
        masks[name] = (r == y) & (c == x)
    return tuple(masks), np.stack(list(masks.values()))


def blob(H, W, cy, cx, sigma, amp):
    r, c = np.mgrid[0:H, 0:W]
    d2 = (r - cy) ** 2 + (c - cx) ** 2
    return np.where(d2 <= (3 * sigma) ** 2, amp * np.exp(-d2 / (2.0 * sigma ** 2)), 0.0)


def storm_frames(shape, seed):
    """(..., H, W) fp32 in [0, 1]: 1 .. 4 cells per frame and a sparse speckle, so that the low thresholds have events in every frame
    and the high ones in some"""
    H, W = shape[-2:]
    rng = np.random.default_rng(seed)
    out = np.zeros((int(np.prod(shape[:-2])), H, W))
    for f in out:
        for _ in range(rng.integers(1, 5)):
            f += blob(H, W, rng.uniform(0, H - 1), rng.uniform(0, W - 1), rng.uniform(0.8, max(min(H, W) / 8.0, 1.0)), rng.uniform(0.3, 1.0))
        f += (rng.random((H, W)) < 0.01) * rng.uniform(0.0, 0.6, (H, W))
    return np.minimum(out, 1.0).astype(np.float32).reshape(shape)


def close(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(ref)) and bool((np.nan_to_num(np.abs(got - ref)) <= 1e-12 * np.maximum(1.0, np.nan_to_num(np.abs(ref)))).all())


# ------------------------------------------------------------------------------------------------ scale_energy
@pytest.mark.parametrize("shape", DYADIC + PADDED)
def test_hip_scale_energy_equals_q_levels(shape):
    H, W = shape
    n = R.top_level(H, W)
    names, masks = energy_masks(H, W)
    frames = (masks * ON).astype(np.float32)
    got = scale_energy(cuda5(frames[:, None]), 74)
    assert got.dtype == torch.int64 and got.shape == (len(names), 1, n + 1)
    got = got.cpu().numpy()[:, 0]
    for name, m, g in zip(names, masks, got):
        assert np.array_equal(g, R.q_levels(m)), (shape, name, g, R.q_levels(m))
        assert R.parseval_holds(g, n)
    assert (got[names.index("empty")] == 0).all() and got[names.index("full")][0] == H * W and got[names.index("full")][n] == (H * W) ** 2
    if shape == (128, 128):
        assert got[names.index("full")].tolist() == [4 ** (7 + l) for l in range(8)]
    # the raw comparison gives the same integers for the same event sets
    raw = scale_energy(cuda5(frames[:, None]), 0.5, scaled=False).cpu().numpy()[:, 0]
    assert np.array_equal(raw, got)


def test_hip_scale_energy_event_test_nan_and_views():
    d = np.float32(DIVISOR)
    v = np.float32(16.0) * d
    while v / d >= np.float32(16.0):
        v = np.nextafter(v, np.float32(0.0))
    below, on = v, np.nextafter(v, np.float32(1.0))          # `on` is the smallest fp32 whose quotient reaches 16: an event
    f = np.zeros((1, 1, 5, 9), np.float32)
    f[0, 0, 1, 2], f[0, 0, 3, 7], f[0, 0, 4, 0] = below, on, np.nan
    got = scale_energy(cuda5(f), 16).cpu().numpy()
    assert np.array_equal(got, R.scale_energy(f, 16)) and got[0, 0].tolist() == [1, 1, 1, 1, 1]          # `on` alone is an event
    g = np.zeros((1, 1, 5, 9), np.float32)
    g[0, 0, 0, 0], g[0, 0, 2, 4], g[0, 0, 4, 8] = np.nextafter(np.float32(0.25), np.float32(0.0)), 0.25, np.nan
    got = scale_energy(cuda5(g), 0.25, scaled=False).cpu().numpy()
    assert np.array_equal(got, R.scale_energy(g, 0.25, scaled=False)) and got[0, 0].tolist() == [1, 1, 1, 1, 1]
    nan_only = np.full((1, 1, 3, 4), np.nan, np.float32)
    assert (scale_energy(cuda5(nan_only), 16).cpu().numpy() == 0).all()
    # a threshold that zero reaches: the padding still holds no event
    z = np.zeros((1, 1, 3, 5), np.float32)
    assert scale_energy(cuda5(z), 0).cpu().numpy()[0, 0].tolist() == R.q_levels(np.ones((3, 5), np.int64)).tolist()
    # in place through the strides: an NHWT tensor, a sliced batch, a layout without C, a cropped view, another dtype
    x = storm_frames((4, 3, 65, 72), 3)
    ref = R.scale_energy(x, 74)
    xc = torch.from_numpy(x).cuda()
    assert np.array_equal(scale_energy(xc, 74, layout="NTHW").cpu().numpy(), ref)
    nhwt = xc.permute(0, 2, 3, 1).contiguous()
    assert np.array_equal(scale_energy(nhwt, 74, layout="NHWT").cpu().numpy(), ref)
    assert np.array_equal(scale_energy(xc[..., None][::2], 74).cpu().numpy(), ref[::2])
    assert np.array_equal(scale_energy(xc[:, 1:, 2:30, 5:][..., None], 74).cpu().numpy(), R.scale_energy(x[:, 1:, 2:30, 5:], 74))
    assert np.array_equal(scale_energy(xc.double(), 74, layout="NTHW").cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ SEVIRScaleScore.update
MAX_M = 16


@lru_cache(maxsize=None)
def update_case(H, W):
    """(ens (16, 2, 3, H, W), target (2, 3, H, W), records at the eight thresholds): member 0 has an empty forecast at (0, 1) and a NaN
    pixel at (1, 2), member 2 an inf pixel at (0, 0), the target is empty at (0, 2) and has an inf pixel at (1, 0): every pair of (1, 0) is
    skipped.  The restatement's records are made once per shape; a state of M members and K thresholds is a sum over a part of them."""
    ens, target = storm_frames((MAX_M, 2, 3, H, W), 7 * H + W), storm_frames((2, 3, H, W), 11 * H + W)
    ens[0, 0, 1] = 0.0
    ens[0, 1, 2, H // 2, W // 3] = np.nan
    ens[2, 0, 0, H - 1, W - 1] = np.inf
    target[0, 2] = 0.0
    target[1, 0, 0, 0] = -np.inf
    return ens, target, R.pair_records(ens, target, THRESHOLDS[8])


def reference_state(H, W, K, M, keep_seq):
    _, _, (scored, q) = update_case(H, W)
    ks = [THRESHOLDS[8].index(t) for t in THRESHOLDS[K]]
    return R.state_of_records(scored[:M], q[:M][:, :, :, ks], keep_seq)


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("shape", [(8, 8), (33, 40), (128, 128)])
def test_hip_scale_update_equals_the_restatement(shape, K, M):
    H, W = shape
    n = R.top_level(H, W)
    ens, target, _ = update_case(H, W)
    ec, tc = torch.from_numpy(ens[:M])[..., None].cuda(), cuda5(target)
    for mode in ("0", "1", "2"):
        energy, counts = reference_state(H, W, K, M, mode != "0")
        a = SEVIRScaleScore(mode=mode, seq_len=3, threshold_list=THRESHOLDS[K])
        a.update_members(ec, tc)
        assert a.levels == n + 1
        assert torch.equal(a.energy.cpu(), torch.from_numpy(energy)) and torch.equal(a.counts.cpu(), torch.from_numpy(counts)), (shape, K, M, mode)
        assert int(a.counts.sum()) == 6 * M and int(a.counts[1].sum()) == M + (1 if M < 3 else 2)
        # update_members scores as M update calls do
        b = SEVIRScaleScore(mode=mode, seq_len=3, threshold_list=THRESHOLDS[K])
        for i in range(M):
            b.update(ec[i], tc)
        assert torch.equal(a.energy, b.energy) and torch.equal(a.counts, b.counts)
        # the integer Parseval identity, and Q_0(Z) = misses + false alarms, at every threshold and lead time
        got = a.energy.cpu().numpy()
        for k, thr in enumerate(THRESHOLDS[K]):
            for tk in range(got.shape[3]):
                assert all(R.parseval_holds(got[f, k, :, tk], n) for f in range(3)), (k, tk)
                ts = range(3) if mode == "0" else [tk]
                scored = np.isfinite(ens[:M]).all(axis=(-2, -1)) & np.isfinite(target).all(axis=(-2, -1))[None]
                wrong = sum(int((R.event_mask(ens[m, i, t], thr) != R.event_mask(target[i, t], thr)).sum())
                            for m in range(M) for i in range(2) for t in ts if scored[m, i, t])
                assert got[2, k, 0, tk] == wrong
        res, ref = a.compute(), R.compute(energy, counts, n, mode)
        assert set(res) == set(METRICS)
        for met in METRICS:
            lead = (3,) if mode == "1" else ()
            assert res[met].shape == lead + ((K,) if met in ("mse_random", "base_rate", "freq_bias") else (K, n + 1)), met
            assert close(res[met], ref[met]), (met, mode, res[met], ref[met])


def test_hip_identity_and_swap():
    a, b = storm_frames((2, 3, 33, 128), 31), storm_frames((2, 3, 33, 128), 32)
    ac, bc = cuda5(a), cuda5(b)
    kw = dict(mode="1", seq_len=3, threshold_list=THRESHOLDS[3])
    same = SEVIRScaleScore(**kw)
    same.update(ac, ac)
    assert int(same.energy[2].abs().sum()) == 0 and torch.equal(same.energy[0], same.energy[1]) and same.counts.tolist() == [[2, 2, 2], [0, 0, 0]]
    r = same.compute()
    assert (r["mse"] == 0).all() and (r["iss"][r["mse_random"] > 0] == 1).all() and (r["mse_random"][:, 0] > 0).all()
    ab, ba = SEVIRScaleScore(**kw), SEVIRScaleScore(**kw)
    ab.update(ac, bc)
    ba.update(bc, ac)
    assert int(ab.energy[2, 0, 0].min()) > 0
    assert torch.equal(ab.energy[0], ba.energy[1]) and torch.equal(ab.energy[1], ba.energy[0]) and torch.equal(ab.energy[2], ba.energy[2])


def test_hip_state_accumulates_resets_and_keeps_its_padded_side():
    p1, t1 = storm_frames((2, 3, 33, 40), 60), storm_frames((2, 3, 33, 40), 61)
    p2, t2 = storm_frames((1, 3, 50, 64), 62), storm_frames((1, 3, 50, 64), 63)          # another shape, the same S = 64
    m = SEVIRScaleScore(mode="1", seq_len=3, threshold_list=(16, 74))
    m.update(cuda5(p1), cuda5(t1))
    first = m.energy.clone()
    m.update(cuda5(p2), cuda5(t2))
    e1, c1 = R.scale_state(p1[None], t1, (16, 74), True)
    e2, c2 = R.scale_state(p2[None], t2, (16, 74), True)
    assert np.array_equal(m.counts.cpu().numpy(), c1 + c2) and np.array_equal(m.energy.cpu().numpy(), e1 + e2)
    before = m.energy.clone()
    for shape in ((1, 3, 65, 8), (1, 3, 8, 8)):                                          # S = 128, S = 8
        x = cuda5(storm_frames(shape, 64))
        with pytest.raises(ValueError, match="reset"):
            m.update(x, x)
    assert torch.equal(m.energy, before) and m.levels == 7
    m.reset()
    assert m.energy is None and m.levels is None and np.isnan(m.compute()["base_rate"]).all()
    m.update(cuda5(p1), cuda5(t1))
    assert torch.equal(m.energy, first)


# ------------------------------------------------------------------------------------------------ refusals (before any launch)
def test_hip_refusals():
    for shape in ((1, 1, 129, 16, 1), (1, 1, 16, 129, 1)):
        x = torch.rand(shape).cuda()
        s = SEVIRScaleScore()
        with pytest.raises(PrediffHipError, match="128"):
            s.update(x, x)
        assert int(s.energy.abs().sum()) == 0 and int(s.counts.sum()) == 0
        with pytest.raises(PrediffHipError, match="128"):
            scale_energy(x, 16)
    x = torch.rand((1, 1, 16, 16, 2)).cuda()
    with pytest.raises(ValueError):
        SEVIRScaleScore().update(x, x)
    with pytest.raises(ValueError):
        scale_energy(x, 16)
    with pytest.raises(ValueError):
        SEVIRScaleScore().update_members(torch.zeros((513, 1, 1, 8, 8, 1), device="cuda"), torch.zeros((1, 1, 8, 8, 1), device="cuda"))
    # the C ABI itself: nine thresholds, a workspace that is too small, a workspace that aliases an input
    x = torch.rand((1, 2, 16, 16, 1)).cuda()
    sizes, st = [1, 2, 16, 16, 1], list(x.stride())
    energy, counts = torch.zeros((3, 9, 8, 1), dtype=torch.int64).cuda(), torch.zeros((2, 1), dtype=torch.int64).cuda()
    need = L.scale_ws_bytes(1, 1, sizes)
    assert need > 0 and need % 16 == 0 and L.scale_ws_bytes(1, 9, sizes) == -1 and L.scale_ws_bytes(1, 0, sizes) == -1
    assert L.scale_ws_bytes(1, 1, [1, 2, 129, 16, 1]) == -1 and L.scale_ws_bytes(1, 1, [1, 2, 16, 129, 1]) == -1
    assert L.scale_ws_bytes(513, 1, sizes) == -1 and L.scale_ws_bytes(0, 1, sizes) == -1 and L.scale_ws_bytes(1, 1, [1, 2, 16, 16, 2]) == -1
    assert L.scale_ws_bytes(512, 8, [1, 2, 128, 128, 1]) > 0
    big = torch.empty(need // 8, dtype=torch.float64).cuda()
    with pytest.raises(PrediffHipError, match="thresholds"):
        L.scale_update(x, x, 1, sizes, [0] + st, st, tuple(range(9)), DIVISOR, False, energy, counts, big)
    with pytest.raises(PrediffHipError, match="workspace"):
        L.scale_update(x, x, 1, sizes, [0] + st, st, (16,), DIVISOR, False, energy, counts, big[:need // 8 - 2])
    with pytest.raises(PrediffHipError, match="alias"):
        L.scale_update(x, x, 1, sizes, [0] + st, st, (16,), DIVISOR, False, energy, counts, x.view(-1))
    with pytest.raises(PrediffHipError, match="stride"):
        L.scale_update(x, x, 1, sizes, [0] + st, [st[0], st[1], -st[2], st[3], st[4]], (16,), DIVISOR, False, energy, counts, big)
    assert int(energy.abs().sum()) == 0 and int(counts.sum()) == 0
    L.scale_update(x, x, 1, sizes, [0] + st, st, (16,), DIVISOR, False, energy, counts, big)     # and the accepted call runs
    assert counts[:, 0].tolist() == [2, 0]
