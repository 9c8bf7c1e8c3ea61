"""prediff_amd.distance_score on the device (distance_map, SEVIRDistanceScore) against tests/_distance_ref.py, the brute-force fp64
restatement (itself checked in tests/test_distance_score_host.py).

Tolerances.  Distance maps and counts: equal.  Sums: |got - ref| <= 1e-11 max(1, |ref|) -- a pair's value is an fp64 sum of at most
16384 non-negative terms at one rounding each, 16384 * 2^-53 ~ 1.8e-12 relative for either summation order, about 3.6e-12 between the
two, with headroom for the fold over the pairs (the measured deviations are in DESIGN.md, "Distance maps").  The Hausdorff distance of a single pair: 2 ulp of sqrt(int).  Identities that hold bit for bit (identity, swap, repeat)
are compared with torch.equal."""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import _distance_ref as R
from prediff_amd import SEVIRDistanceScore, distance_map
from prediff_amd import _lib as L
from prediff_amd._lib import PrediffHipError
from prediff_amd.distance_score import DIVISOR, NO_EVENT

pytestmark = pytest.mark.gpu

MAP_SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (128, 3), (33, 128), (128, 128)]
THRESHOLDS = {1: (74,), 3: (16, 74, 133), 8: (8, 16, 40, 74, 100, 133, 181, 219)}
ON = 1.0                                       # 255 on the 0-255 scale: an event of every threshold used here


def cuda5(x):
    """(N, T, H, W) numpy -> NTHWC tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(x))[..., None].cuda()


@lru_cache(maxsize=None)
def map_masks(H, W):
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


def disc(H, W, cy, cx, radius):
    r, c = np.mgrid[0:H, 0:W]
    return ((r - cy) ** 2 + (c - cx) ** 2 <= radius ** 2).astype(np.float32)


def close(got, ref):
    return (np.abs(got - ref) <= 1e-11 * np.maximum(1.0, np.abs(ref))).all()


# ------------------------------------------------------------------------------------------------ distance_map
@pytest.mark.parametrize("shape", MAP_SHAPES)
def test_hip_distance_map_equals_the_restatement(shape):
    H, W = shape
    names, masks = map_masks(H, W)
    frames = (masks * ON).astype(np.float32)
    got = distance_map(cuda5(frames[:, None]), 74)
    assert got.dtype == torch.int32 and got.shape == (len(names), 1, H, W)
    got = got.cpu().numpy()[:, 0]
    for name, m, g in zip(names, masks, got):
        assert np.array_equal(g, R.d2_of_mask(m)), (shape, name)
    assert (got[names.index("empty")] == NO_EVENT).all() and (got[names.index("full")] == 0).all()
    if shape == (128, 128):
        assert got[names.index("corner 00")].max() == 32258
    # the raw comparison gives the same maps for the same event sets
    raw = distance_map(cuda5(frames[:, None]), 0.5, scaled=False).cpu().numpy()[:, 0]
    assert np.array_equal(raw, got)


def test_hip_distance_map_event_test_nan_and_views():
    d = np.float32(DIVISOR)
    v = np.float32(16.0) * d
    while v / d >= np.float32(16.0):
        v = np.nextafter(v, np.float32(0.0))
    below, on = v, np.nextafter(v, np.float32(1.0))          # `on` is the smallest fp32 whose quotient reaches 16: an event
    f = np.zeros((1, 1, 5, 9), np.float32)
    f[0, 0, 1, 2], f[0, 0, 3, 7], f[0, 0, 4, 0] = below, on, np.nan
    got = distance_map(cuda5(f), 16).cpu().numpy()
    assert np.array_equal(got, R.distance_map(f, 16)) and got[0, 0, 3, 7] == 0 and got[0, 0, 1, 2] == 4 + 25 and got[0, 0, 4, 0] == 1 + 49
    g = np.zeros((1, 1, 5, 9), np.float32)
    g[0, 0, 0, 0], g[0, 0, 2, 4], g[0, 0, 4, 8] = np.nextafter(np.float32(0.25), np.float32(0.0)), 0.25, np.nan
    got = distance_map(cuda5(g), 0.25, scaled=False).cpu().numpy()
    assert np.array_equal(got, R.distance_map(g, 0.25, scaled=False)) and got[0, 0, 2, 4] == 0 and got[0, 0, 0, 0] == 4 + 16
    nan_only = np.full((1, 1, 3, 4), np.nan, np.float32)
    assert (distance_map(cuda5(nan_only), 16).cpu().numpy() == NO_EVENT).all()
    # in place through the strides: an NHWT tensor, a sliced batch, a layout without C, another dtype
    x = storm_frames((4, 3, 33, 40), 3)
    ref = R.distance_map(x, 74)
    xc = torch.from_numpy(x).cuda()
    assert np.array_equal(distance_map(xc, 74, layout="NTHW").cpu().numpy(), ref)
    nhwt = xc.permute(0, 2, 3, 1).contiguous()
    assert np.array_equal(distance_map(nhwt, 74, layout="NHWT").cpu().numpy(), ref)
    assert np.array_equal(distance_map(xc[..., None][::2], 74).cpu().numpy(), ref[::2])
    assert np.array_equal(distance_map(xc[:, 1:, 2:30, 5:][..., None], 74).cpu().numpy(), R.distance_map(x[:, 1:, 2:30, 5:], 74))
    assert np.array_equal(distance_map(xc.double(), 74, layout="NTHW").cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ SEVIRDistanceScore.update
@lru_cache(maxsize=None)
def update_case(H, W, K):
    """(pred, target (2, 3, H, W), maps of both): pair (0, 1) has an empty forecast, (0, 2) an empty target, (1, 0) both empty, (1, 1) a
    NaN pixel; the restatement's maps are made once per case"""
    pred, target = storm_frames((2, 3, H, W), 7 * H + W), storm_frames((2, 3, H, W), 11 * H + W)
    pred[0, 1] = 0.0
    target[0, 2] = 0.0
    pred[1, 0] = target[1, 0] = 0.0
    pred[1, 1, H // 2, W // 3] = np.nan
    return pred, target, R.frame_maps(pred[None], THRESHOLDS[K]), R.frame_maps(target, THRESHOLDS[K])


@pytest.mark.parametrize("shape,K", [((7, 5), 1), ((7, 5), 3), ((7, 5), 8), ((33, 128), 3), ((33, 128), 8), ((128, 128), 1), ((128, 128), 3)])
def test_hip_distance_update_equals_the_restatement(shape, K):
    pred, target, pm, tm = update_case(*shape, K)
    pc, tc = cuda5(pred), cuda5(target)
    worst = 0.0
    for cutoff in (None, 10.0):
        for mode in ("0", "1", "2"):
            m = SEVIRDistanceScore(mode=mode, seq_len=3, threshold_list=THRESHOLDS[K], cutoff=cutoff)
            m.update(pc, tc)
            sums, counts = R.distance_state(pm, tm, cutoff, mode != "0")
            got_s, got_c = m.sums.cpu().numpy(), m.counts.cpu().numpy()
            assert got_s.shape == sums.shape and np.array_equal(got_c, counts), (shape, K, cutoff, mode)
            dev = float((np.abs(got_s - sums) / np.maximum(1.0, np.abs(sums))).max())
            worst = max(worst, dev)
            print(f"[distance_score parity] {shape} K={K} cutoff={cutoff} mode={mode}: max relative deviation {dev:.2e}")
            assert close(got_s, sums), (shape, K, cutoff, mode, dev)
            assert int(got_c[1].sum()) == K and int(got_c[0].sum()) == 5 * K          # one skipped pair of six, at every threshold
            res, ref = m.compute(), R.compute(sums, counts, mode)
            for met in m.metrics_list:
                assert res[met].shape == ((3, K) if mode == "1" else (K,))
                assert np.allclose(res[met], ref[met], rtol=1e-11, atol=1e-11, equal_nan=True), (met, mode)
    print(f"[distance_score parity] {shape} K={K}: worst {worst:.2e}")


def test_hip_hausdorff_of_a_single_pair_and_the_shifted_disc():
    pred, target = storm_frames((1, 1, 37, 53), 21), storm_frames((1, 1, 37, 53), 22)
    for thr in (16, 74):
        p = R.pair_metrics(pred[0, 0], target[0, 0], thr)
        assert p["both"]
        m = SEVIRDistanceScore(threshold_list=(thr,))
        m.update(cuda5(pred), cuda5(target))
        want = math.sqrt(p["hausdorff_d2"])
        assert abs(float(m.sums[2, 0, 0]) - want) <= 2 * np.spacing(want)
        assert m.counts[:, 0, 0].tolist() == [1, 0, 1, 1, p["n_pred"], p["n_target"]]
    d0, d1 = disc(32, 32, 12, 12, 6), disc(32, 32, 15, 16, 6)
    m = SEVIRDistanceScore(threshold_list=(74,))
    m.update(cuda5(d1[None, None]), cuda5(d0[None, None]))
    r = m.compute()
    assert r["hausdorff"][0] == 5.0 and 0 < r["med_miss"][0] <= 5 and 0 < r["med_false"][0] <= 5 and r["frac_both"][0] == 1.0


# ------------------------------------------------------------------------------------------------ properties
def test_hip_identity_swap_and_repeat_are_bit_exact():
    a, b = storm_frames((2, 3, 33, 128), 31), storm_frames((2, 3, 33, 128), 32)
    ac, bc = cuda5(a), cuda5(b)
    for cutoff in (None, 10.0):
        kw = dict(mode="1", seq_len=3, threshold_list=THRESHOLDS[3], cutoff=cutoff)
        same = SEVIRDistanceScore(**kw)
        same.update(ac, ac)
        assert torch.equal(same.sums, torch.zeros_like(same.sums)) and int(same.counts[0].sum()) == 18
        ab, ba = SEVIRDistanceScore(**kw), SEVIRDistanceScore(**kw)
        ab.update(ac, bc)
        ba.update(bc, ac)
        assert float(ab.sums[0].abs().sum()) > 0
        assert torch.equal(ab.sums[0], ba.sums[1]) and torch.equal(ab.sums[1], ba.sums[0])
        assert torch.equal(ab.sums[2:], ba.sums[2:])
        assert torch.equal(ab.counts[:4], ba.counts[:4]) and torch.equal(ab.counts[4], ba.counts[5])


@pytest.mark.parametrize("M", [1, 3, 32])
def test_hip_members_equal_sequential_updates(M):
    shape = (2, 3, 33, 40)
    target = storm_frames(shape, 50)
    ens = storm_frames((M,) + shape, 51)
    ens[0, 0, 0] = 0.0                                       # an empty forecast
    ens[M - 1, 1, 2, 5, 5] = np.inf                          # a skipped pair
    ec, tc = torch.from_numpy(ens)[..., None].cuda(), cuda5(target)
    for mode, cutoff in (("1", None), ("0", 10.0)):
        kw = dict(mode=mode, seq_len=3, threshold_list=THRESHOLDS[3], cutoff=cutoff)
        a, b, again = (SEVIRDistanceScore(**kw) for _ in range(3))
        a.update_members(ec, tc)
        for i in range(M):
            b.update(ec[i], tc)
        assert torch.equal(a.counts, b.counts) and int(a.counts[:2, 0].sum()) == M * 6 and int(a.counts[1, 0].sum()) == 1
        assert close(a.sums.cpu().numpy(), b.sums.cpu().numpy())
        again.update_members(ec, tc)
        assert torch.equal(again.sums, a.sums) and torch.equal(again.counts, a.counts)     # the same call gives the same bits
    if M == 3:
        sums, counts = R.distance_state(R.frame_maps(ens, THRESHOLDS[3]), R.frame_maps(target, THRESHOLDS[3]), 10.0, False)
        assert np.array_equal(a.counts.cpu().numpy(), counts) and close(a.sums.cpu().numpy(), sums)


def test_hip_state_accumulates_and_resets():
    p1, t1 = storm_frames((2, 3, 33, 40), 60), storm_frames((2, 3, 33, 40), 61)
    p2, t2 = storm_frames((1, 3, 33, 40), 62), storm_frames((1, 3, 33, 40), 63)
    m = SEVIRDistanceScore(mode="1", seq_len=3, threshold_list=(16, 74), cutoff=6.0)
    m.update(cuda5(p1), cuda5(t1))
    first = m.sums.clone()
    m.update(cuda5(p2), cuda5(t2))
    s1, c1 = R.distance_state(R.frame_maps(p1[None], (16, 74)), R.frame_maps(t1, (16, 74)), 6.0, True)
    s2, c2 = R.distance_state(R.frame_maps(p2[None], (16, 74)), R.frame_maps(t2, (16, 74)), 6.0, True)
    assert np.array_equal(m.counts.cpu().numpy(), c1 + c2) and close(m.sums.cpu().numpy(), s1 + s2)
    m.reset()
    assert m.sums is None and np.isnan(m.compute()["baddeley"]).all()
    m.update(cuda5(p1), cuda5(t1))
    assert torch.equal(m.sums, first)


# ------------------------------------------------------------------------------------------------ refusals (before any launch)
def test_hip_refusals():
    for shape in ((1, 1, 129, 16, 1), (1, 1, 16, 129, 1)):
        x = torch.rand(shape).cuda()
        s = SEVIRDistanceScore()
        with pytest.raises(PrediffHipError, match="128"):
            s.update(x, x)
        assert float(s.sums.abs().sum()) == 0.0 and int(s.counts.sum()) == 0
        with pytest.raises(PrediffHipError, match="128"):
            distance_map(x, 16)
    x = torch.rand((1, 1, 16, 16, 2)).cuda()
    with pytest.raises(ValueError):
        SEVIRDistanceScore().update(x, x)
    with pytest.raises(ValueError):
        distance_map(x, 16)
    with pytest.raises(ValueError):
        SEVIRDistanceScore(threshold_list=tuple(range(9)))
    with pytest.raises(ValueError):
        SEVIRDistanceScore().update_members(torch.zeros((513, 1, 1, 8, 8, 1), device="cuda"), torch.zeros((1, 1, 8, 8, 1), device="cuda"))
    # the C ABI itself: nine thresholds, a workspace that is too small, a workspace that aliases an input
    x = torch.rand((1, 2, 16, 16, 1)).cuda()
    sizes, st = [1, 2, 16, 16, 1], list(x.stride())
    sums, counts = torch.zeros((4, 9, 1), dtype=torch.float64).cuda(), torch.zeros((6, 9, 1), dtype=torch.int64).cuda()
    need = L.distance_ws_bytes(1, 1, sizes)
    assert need > 0 and L.distance_ws_bytes(1, 9, sizes) == -1 and L.distance_ws_bytes(1, 1, [1, 2, 129, 16, 1]) == -1
    assert L.distance_ws_bytes(513, 1, sizes) == -1 and L.distance_ws_bytes(1, 1, [1, 2, 16, 16, 2]) == -1
    big = torch.empty(need // 8, dtype=torch.float64).cuda()
    with pytest.raises(PrediffHipError, match="thresholds"):
        L.distance_update(x, x, 1, sizes, [0] + st, st, tuple(range(9)), DIVISOR, None, False, sums, counts, big)
    with pytest.raises(PrediffHipError, match="workspace"):
        L.distance_update(x, x, 1, sizes, [0] + st, st, (16,), DIVISOR, None, False, sums, counts, big[:need // 8 - 2])
    with pytest.raises(PrediffHipError, match="alias"):
        L.distance_update(x, x, 1, sizes, [0] + st, st, (16,), DIVISOR, None, False, sums, counts, x.view(-1))
    with pytest.raises(PrediffHipError, match="cutoff"):
        L.distance_update(x, x, 1, sizes, [0] + st, st, (16,), DIVISOR, -1.0, False, sums, counts, big)
    assert float(sums.abs().sum()) == 0.0 and int(counts.sum()) == 0
    L.distance_update(x, x, 1, sizes, [0] + st, st, (16,), DIVISOR, None, False, sums, counts, big)     # and the accepted call runs
    assert counts[0, 0, 0].item() == 2


# ------------------------------------------------------------------------------------------------ evaluate_context
def test_evaluate_context_updates_distance_scores():
    """evaluate_context on the tiny latent-diffusion model of the config tests: the distance scores see every sample where the object
    scores do, and a call without the keywords returns what it returned before."""
    import _templates as TP
    from _cases import TINY_UNET_CFGS, TINY_VAE_CFG
    from _weights import seeded_input, seeded_state_dict
    from test_alignment import _tiny_alignment
    from prediff_amd import config as CFG
    from prediff_amd.autoencoder_kl import AutoencoderKL
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.latent_diffusion import LatentDiffusion
    vae = AutoencoderKL(**TINY_VAE_CFG, precision="fp32")
    vae.load_state_dict(seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 601))
    cfg = TINY_UNET_CFGS["axial"]
    net = CuboidTransformerUNet(**cfg, precision="fp32")
    net.load_state_dict(seeded_state_dict(TP.unet_template(cfg, "tiny_unet_schema.json", "axial"), 600))
    T_in, (T_out, H, W, _) = cfg["input_shape"][0], cfg["target_shape"]
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(T_out, H * 4, W * 4, 1), timesteps=1000, use_ema=False,
                          latent_shape=tuple(cfg["target_shape"]), first_stage_model=vae.cuda(),
                          cond_stage_model="__is_first_stage__").cuda().eval()
    al = _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    B, S = 2, 2
    seq = seeded_input("dsseq", (B, T_in + T_out, H * 4, W * 4, 1), 29, kind="uniform").cuda()
    run_cfg = {"layout": {"in_len": T_in, "out_len": T_out}, "eval": {"num_samples_per_context": S}}
    thr = (100, 160)                                        # uniform [0, 1) targets: events at 0.39 and 0.63
    ds, ads = (SEVIRDistanceScore(layout="NTHWC", mode="1", seq_len=T_out, threshold_list=thr, cutoff=5.0) for _ in range(2))
    torch.manual_seed(7)
    out = CFG.evaluate_context(ldm, seq, run_cfg, distance_score=ds, aligned_distance_score=ads, timesteps=3)
    torch.manual_seed(7)
    plain = CFG.evaluate_context(ldm, seq, run_cfg, timesteps=3)
    assert set(out) == set(plain) == {"pred", "aligned_pred"}
    for k in out:
        assert len(out[k]) == len(plain[k]) == S and all(torch.equal(a, b) for a, b in zip(out[k], plain[k])), k
    tgt = seq[:, T_in:]
    for metric, preds in ((ds, out["pred"]), (ads, out["aligned_pred"])):
        manual = SEVIRDistanceScore(layout="NTHWC", mode="1", seq_len=T_out, threshold_list=thr, cutoff=5.0)
        for pr in preds:
            manual.update(pr.float(), tgt)
        assert torch.equal(metric.sums, manual.sums) and torch.equal(metric.counts, manual.counts)
        assert int(metric.counts[:2, 0, 0].sum()) == B * S
        ens = np.stack([pr.float().cpu().numpy()[..., 0] for pr in preds])
        sums, counts = R.distance_state(R.frame_maps(ens, thr), R.frame_maps(tgt.cpu().numpy()[..., 0], thr), 5.0, True)
        assert np.array_equal(metric.counts.cpu().numpy(), counts) and close(metric.sums.cpu().numpy(), sums)
