"""prediff_amd.frame_score.SEVIRFrameScore (MSE / MAE / SSIM of the reference's test_step, on the device) against an fp64 restatement
of its definitions written here (torch.float64 on the CPU, separable valid-mode conv2d), which is itself pinned against a direct
double-loop evaluation with explicit 11 x 11 weights.

Tolerances.  MSE / MAE sums: relative 1e-12 (only the fp64 fold order differs, <= n 2^-53).  SSIM per lead time: the same formula is
evaluated once more with torch ops in fp32 on the CPU (the torchmetrics arithmetic); with e32 its absolute deviation from the fp64
restatement on that input, the kernel must stay within max(4 e32, 1e-6).  Every GPU case prints its e32 and the kernel's deviation, and
appends the line to the file FRAME_SCORE_PARITY_LOG names (scripts/frame_score_parity.py -> profiles/frame_score_parity.log)."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from prediff_amd._lib import PrediffHipError
from prediff_amd.frame_score import SEVIRFrameScore


# ------------------------------------------------------------------------------------------------ the yardstick
def _gauss(dtype):
    d = torch.arange(-5, 6, dtype=dtype)
    g = torch.exp(-((d / 1.5) ** 2) / 2)
    return g / g.sum()


def ssim_frames(p, t, R, dtype=torch.float64):
    """p, t: (F, C, H, W) -> (F,) SSIM of every frame, all arithmetic in `dtype`."""
    p, t = p.to(dtype), t.to(dtype)
    Fn, C, H, W = p.shape
    g = _gauss(dtype)

    def blur(x):
        x = x.reshape(Fn * C, 1, H, W)
        return F.conv2d(F.conv2d(x, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))

    mp, mt, epp, ett, ept = blur(p), blur(t), blur(p * p), blur(t * t), blur(p * t)
    vp, vt, cov = (epp - mp * mp).clamp_min(0), (ett - mt * mt).clamp_min(0), ept - mp * mt
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    s = ((2 * mp * mt + c1) * (2 * cov + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    return s.reshape(Fn, -1).mean(dim=1)


def _canon(x, layout):
    """x in `layout` -> (N, T, C, H, W)."""
    for a in "NTHWC":
        if a not in layout:
            x, layout = x.unsqueeze(-1), layout + a
    return x.permute(*[layout.index(a) for a in "NTCHW"])


def restate(updates, layout, keep_seq, data_range, dtype=torch.float64):
    """The state after `updates` ((pred, target) CPU tensors in `layout`): sums (3, T') fp64 and counts (2, T') int64.  The error sums are
    always fp64; `dtype` is the arithmetic of the SSIM."""
    sums = cnt = None
    for p, t in updates:
        p, t = _canon(p.float(), layout), _canon(t.float(), layout)
        N, T, C, H, W = p.shape
        # data_range=None: max - min of each tensor of this call, in the tensors' own fp32 (torchmetrics)
        R = data_range if data_range is not None else max(float(p.max() - p.min()), float(t.max() - t.min()))
        d = p.double() - t.double()
        fs = ssim_frames(p.reshape(N * T, C, H, W), t.reshape(N * T, C, H, W), float(np.float32(R)), dtype).double().reshape(N, T)
        s = torch.stack([(d * d).sum(dim=(0, 2, 3, 4)), d.abs().sum(dim=(0, 2, 3, 4)), fs.sum(dim=0)])
        n = torch.tensor([[N * C * H * W] * T, [N] * T], dtype=torch.int64)
        if not keep_seq:
            s, n = s.sum(dim=1, keepdim=True), n.sum(dim=1, keepdim=True)
        sums, cnt = (s, n) if sums is None else (sums + s, cnt + n)
    return sums.numpy(), cnt.numpy()


def _same(a, b):
    """bit-equal, NaNs in the same places"""
    return np.array_equal(a, b, equal_nan=True)


def check(label, metric, updates, layout, data_range):
    """The metric's state against the restatement of `updates`; returns (e32, deviation) per lead time."""
    keep = metric.keep_seq_len_dim
    s64, n64 = restate(updates, layout, keep, data_range)
    s32, _ = restate(updates, layout, keep, data_range, torch.float32)
    got, gn = metric.sums.cpu().numpy(), metric.counts.cpu().numpy()
    assert np.array_equal(gn, n64), label
    for k, name in ((0, "sq"), (1, "abs")):
        assert np.array_equal(np.isnan(got[k]), np.isnan(s64[k])), (label, name)
        ok = ~np.isnan(s64[k])
        rel = np.abs(got[k][ok] - s64[k][ok]) / np.maximum(np.abs(s64[k][ok]), 1e-300)
        print(f"[frame_score parity] {label}: {name} sum max rel err {rel.max() if rel.size else 0.0:.2e}")
        assert (rel <= 1e-12).all(), (label, name, rel)
    frames = n64[1].astype(np.float64)
    ref, r32, mine = s64[2] / frames, s32[2] / frames, got[2] / frames
    assert np.array_equal(np.isnan(mine), np.isnan(ref)), (label, mine, ref)
    ok = ~np.isnan(ref)
    e32 = np.where(np.isnan(r32[ok]), 0.0, np.abs(r32[ok] - ref[ok]))
    dev = np.abs(mine[ok] - ref[ok])
    line = (f"[frame_score parity] {label}: ssim e32 (fp32 torch ops vs fp64) per lead time {np.array2string(e32, precision=2)}  "
            f"kernel deviation {np.array2string(dev, precision=2)}")
    print(line)
    if os.environ.get("FRAME_SCORE_PARITY_LOG"):
        with open(os.environ["FRAME_SCORE_PARITY_LOG"], "a") as f:
            f.write(line + "\n")
    assert (dev <= np.maximum(4.0 * e32, 1e-6)).all(), (label, dev, e32)
    return e32, dev


def make_pair(shape, seed, noise=0.1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(shape, generator=g)
    p = (t + noise * torch.randn(shape, generator=g)).clamp(0.0, 1.0)
    return p * scale, t * scale


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_against_direct_double_loop():
    """The separable fp64 restatement equals the non-separable definition evaluated pixel by pixel with explicit 11 x 11 weights."""
    p, t = make_pair((1, 2, 13, 14), 1)
    R = 1.0
    g = [math.exp(-((i - 5) / 1.5) ** 2 / 2) for i in range(11)]
    g = [x / sum(g) for x in g]
    w2 = [[g[i] * g[j] for j in range(11)] for i in range(11)]
    pp, tt = p.double().tolist(), t.double().tolist()
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    vals = []
    for c in range(2):
        for y in range(13 - 10):
            for x in range(14 - 10):
                mp = mt = epp = ett = ept = 0.0
                for i in range(11):
                    for j in range(11):
                        a, b, w = pp[0][c][y + i][x + j], tt[0][c][y + i][x + j], w2[i][j]
                        mp, mt, epp, ett, ept = mp + w * a, mt + w * b, epp + w * a * a, ett + w * b * b, ept + w * a * b
                vp, vt, cov = max(epp - mp * mp, 0.0), max(ett - mt * mt, 0.0), ept - mp * mt
                vals.append(((2 * mp * mt + c1) * (2 * cov + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2)))
    direct = sum(vals) / len(vals)
    got = float(ssim_frames(p, t, R)[0])
    assert len(vals) == 2 * 3 * 4 and abs(got - direct) <= 1e-12, (got, direct)
    assert 0.0 < direct < 1.0


def test_constructor_validation():
    for layout in ("NTHWX", "NTHHW", "THWC"):
        with pytest.raises(ValueError):
            SEVIRFrameScore(layout=layout)
    for layout in ("NTWC", "NTHC", "NT"):                  # H or W missing
        with pytest.raises(ValueError):
            SEVIRFrameScore(layout=layout)
    with pytest.raises(NotImplementedError):
        SEVIRFrameScore(mode="3")
    for mode in ("1", "2"):
        with pytest.raises(ValueError):
            SEVIRFrameScore(mode=mode)
    with pytest.raises(ValueError):
        SEVIRFrameScore(metrics_list=("mse", "psnr"))
    m = SEVIRFrameScore(layout="NHWT", mode="1", seq_len=6, metrics_list=("ssim",), data_range=255)
    assert m.keep_seq_len_dim and m.data_range == 255.0


def test_compute_from_hand_set_state():
    sums = torch.tensor([[8.0, 2.0, 6.0], [4.0, 1.0, 9.0], [1.5, 1.0, 0.5]], dtype=torch.float64)
    counts = torch.tensor([[16, 16, 16], [2, 2, 2]], dtype=torch.int64)
    m = SEVIRFrameScore(mode="1", seq_len=3)
    m.sums, m.counts = sums, counts
    r = m.compute()
    assert set(r) == {"mse", "mae", "ssim"}
    assert np.array_equal(r["mse"], [0.5, 0.125, 0.375]) and np.array_equal(r["mae"], [0.25, 0.0625, 0.5625])
    assert np.array_equal(r["ssim"], [0.75, 0.5, 0.25])
    m2 = SEVIRFrameScore(mode="2", seq_len=3, metrics_list=("ssim", "mse"))
    m2.sums, m2.counts = sums, counts
    r2 = m2.compute()
    assert list(r2) == ["ssim", "mse"] and r2["ssim"] == 0.5 and r2["mse"] == pytest.approx(1.0 / 3.0, abs=1e-15)
    m0 = SEVIRFrameScore(mode="0")
    m0.sums, m0.counts = sums.sum(dim=1, keepdim=True), counts.sum(dim=1, keepdim=True)
    r0 = m0.compute()
    assert r0 == {"mse": 16.0 / 48.0, "mae": 14.0 / 48.0, "ssim": 0.5}
    # no update: NaNs of the mode's shape
    e0, e1, e2 = SEVIRFrameScore().compute(), SEVIRFrameScore(mode="1", seq_len=4).compute(), SEVIRFrameScore(mode="2", seq_len=4).compute()
    assert all(isinstance(e0[k], float) and math.isnan(e0[k]) for k in ("mse", "mae", "ssim"))
    assert all(e1[k].shape == (4,) and np.isnan(e1[k]).all() for k in ("mse", "mae", "ssim"))
    assert all(isinstance(e2[k], float) and math.isnan(e2[k]) for k in ("mse", "mae", "ssim"))


def test_update_members_needs_data_range_and_update_needs_the_device():
    x = torch.zeros((2, 1, 2, 16, 16, 1))
    with pytest.raises(ValueError, match="data_range"):
        SEVIRFrameScore().update_members(x, x[0])
    with pytest.raises(ValueError):
        SEVIRFrameScore(data_range=1.0).update_members(x[:, :, :1], x[0])       # not (M,) + target.shape
    with pytest.raises(ValueError):
        SEVIRFrameScore().update(x[0], x[0, :, :1])
    with pytest.raises(PrediffHipError):
        SEVIRFrameScore().update(x[0], x[0])                                    # CPU tensors
    with pytest.raises(PrediffHipError):
        SEVIRFrameScore(data_range=1.0).update_members(x, x[0])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_SYNC_SUMS = [[8.0, 2.0], [4.0, 1.0], [1.5, 1.0]]
_SYNC_COUNTS = [[16, 16], [2, 2]]


def _sync_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = SEVIRFrameScore(mode="1", seq_len=2)
        if rank == 0:                                   # rank 1 made no update: it takes part with a zero state
            m.sums, m.counts = torch.tensor(_SYNC_SUMS, dtype=torch.float64), torch.tensor(_SYNC_COUNTS, dtype=torch.int64)
        m.sync()
        q.put((rank, m.sums.tolist(), m.counts.tolist(), m.compute()["mse"].tolist()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sync_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r[0]: r[1:] for r in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        assert got[r][0] == _SYNC_SUMS and got[r][1] == _SYNC_COUNTS and got[r][2] == [0.5, 0.125], (r, got[r])
    SEVIRFrameScore().sync()                            # no process group: a no-op


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["0", "1"])
def test_hip_frame_score_v1_shape(mode):
    p, t = make_pair((4, 6, 128, 128, 1), 10)
    m = SEVIRFrameScore(layout="NTHWC", mode=mode, seq_len=6, data_range=1.0)
    m.update(p.cuda(), t.cuda())
    check(f"v1 (4,6,128,128,1) mode {mode}", m, [(p, t)], "NTHWC", 1.0)
    r = m.compute()
    s64, n64 = restate([(p, t)], "NTHWC", mode == "1", 1.0)
    assert np.allclose(r["mse"], (s64[0] / n64[0]) if mode == "1" else float(s64[0, 0] / n64[0, 0]), rtol=1e-12, atol=0)
    assert np.all(np.asarray(r["ssim"]) > 0.0) and np.all(np.asarray(r["ssim"]) < 1.0)


@pytest.mark.gpu
def test_hip_frame_score_strided_view_in_place():
    p, t = make_pair((4, 6, 128, 128, 1), 11)
    pc, tc = p.cuda(), t.cuda()
    a = SEVIRFrameScore(layout="NTHWC", mode="1", seq_len=6, data_range=1.0)
    a.update(pc, tc)
    pv, tv = pc[..., 0].permute(0, 2, 3, 1), tc[..., 0].permute(0, 2, 3, 1)        # NHWT views of the same memory
    assert not pv.is_contiguous()
    b = SEVIRFrameScore(layout="NHWT", mode="1", seq_len=6, data_range=1.0)
    b.update(pv, tv)
    assert torch.equal(a.sums, b.sums) and torch.equal(a.counts, b.counts)
    check("NHWT strided view", b, [(pv.cpu(), tv.cpu())], "NHWT", 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 37, 53, 1), (3, 2, 11, 11, 1), (2, 2, 40, 45, 3), (1, 2, 11, 70, 2)])
def test_hip_frame_score_geometries(shape):
    p, t = make_pair(shape, 12)
    for mode in ("0", "1"):
        m = SEVIRFrameScore(layout="NTHWC", mode=mode, seq_len=shape[1], data_range=1.0)
        m.update(p.cuda(), t.cuda())
        check(f"geometry {shape} mode {mode}", m, [(p, t)], "NTHWC", 1.0)


@pytest.mark.gpu
def test_hip_frame_score_refuses_frames_below_the_window():
    for shape in ((1, 2, 10, 32, 1), (1, 2, 32, 10, 1)):
        x = torch.rand(shape).cuda()
        m = SEVIRFrameScore(data_range=1.0)
        with pytest.raises(PrediffHipError, match="11"):
            m.update(x, x)
        assert float(m.sums.abs().sum()) == 0.0 and int(m.counts.sum()) == 0


@pytest.mark.gpu
def test_hip_frame_score_identical_and_constant_frames():
    _, t = make_pair((2, 3, 64, 64, 1), 13)
    tc = t.cuda()
    m = SEVIRFrameScore(mode="1", seq_len=3, data_range=1.0)
    m.update(tc, tc)
    r = m.compute()
    assert np.all(r["mse"] == 0.0) and np.all(r["mae"] == 0.0) and np.all(np.abs(r["ssim"] - 1.0) <= 1e-6)
    check("pred is target", m, [(t, t)], "NTHWC", 1.0)
    # constant frames: E[xx] - mu^2 is rounding noise of either sign -> the variance clamp; the result is finite
    cp, ct = torch.full((2, 3, 32, 32, 1), 0.7), torch.full((2, 3, 32, 32, 1), 0.4)
    ct[1] = 0.7
    m = SEVIRFrameScore(mode="1", seq_len=3, data_range=1.0)
    m.update(cp.cuda(), ct.cuda())
    assert np.isfinite(m.compute()["ssim"]).all()
    check("constant frames", m, [(cp, ct)], "NTHWC", 1.0)


@pytest.mark.gpu
def test_hip_frame_score_data_range():
    p, t = make_pair((2, 3, 48, 48, 1), 14)
    p = p * 0.8                                         # the two value ranges differ
    auto = SEVIRFrameScore(mode="1", seq_len=3)
    auto.update(p.cuda(), t.cuda())
    R = max(float(p.max() - p.min()), float(t.max() - t.min()))
    fixed = SEVIRFrameScore(mode="1", seq_len=3, data_range=R)
    fixed.update(p.cuda(), t.cuda())
    assert torch.equal(auto.sums, fixed.sums) and torch.equal(auto.counts, fixed.counts)
    check("data_range=None", auto, [(p, t)], "NTHWC", None)
    # a second call has a range of its own
    p2, t2 = make_pair((2, 3, 48, 48, 1), 15, scale=3.0)
    auto.update(p2.cuda(), t2.cuda())
    check("data_range=None, two calls", auto, [(p, t), (p2, t2)], "NTHWC", None)
    # frames in [0, 255]
    p3, t3 = make_pair((2, 3, 48, 48, 1), 16, scale=255.0)
    m = SEVIRFrameScore(mode="1", seq_len=3, data_range=255.0)
    m.update(p3.cuda(), t3.cuda())
    check("[0, 255] frames, data_range=255", m, [(p3, t3)], "NTHWC", 255.0)


@pytest.mark.gpu
def test_hip_frame_score_nan_stays_in_its_lead_time():
    p, t = make_pair((2, 6, 48, 48, 1), 17)
    clean = SEVIRFrameScore(mode="1", seq_len=6, data_range=1.0)
    clean.update(p.cuda(), t.cuda())
    pn = p.clone()
    pn[1, 2, 20, 30, 0] = float("nan")
    m = SEVIRFrameScore(mode="1", seq_len=6, data_range=1.0)
    m.update(pn.cuda(), t.cuda())
    r, rc = m.compute(), clean.compute()
    others = [0, 1, 3, 4, 5]
    for k in ("mse", "mae", "ssim"):
        assert math.isnan(r[k][2]), k
        assert np.isfinite(r[k][others]).all() and np.array_equal(r[k][others], rc[k][others]), k
    assert torch.equal(m.sums[:, others], clean.sums[:, others])
    check("one NaN pixel at lead time 2", m, [(pn, t)], "NTHWC", 1.0)


@pytest.mark.gpu
def test_hip_frame_score_bf16_input():
    p, t = make_pair((2, 3, 32, 40, 1), 18)
    pb, tb = p.bfloat16().cuda(), t.bfloat16().cuda()
    a, b = (SEVIRFrameScore(mode="1", seq_len=3, data_range=1.0) for _ in range(2))
    a.update(pb, tb)
    b.update(pb.float(), tb.float())
    assert torch.equal(a.sums, b.sums) and torch.equal(a.counts, b.counts)
    check("bf16 input", a, [(pb.float().cpu(), tb.float().cpu())], "NTHWC", 1.0)


@pytest.mark.gpu
def test_hip_frame_score_state_handling():
    p, t = make_pair((2, 3, 32, 40, 1), 19)
    p2, t2 = make_pair((3, 3, 32, 40, 1), 20)
    m = SEVIRFrameScore(mode="1", seq_len=3, data_range=1.0)
    m.update(p.cuda(), t.cuda())
    first = m.sums.clone()
    m.update(p2.cuda(), t2.cuda())
    check("two updates", m, [(p, t), (p2, t2)], "NTHWC", 1.0)
    m.reset()
    assert m.sums is None and math.isnan(SEVIRFrameScore.compute(m)["mse"][0])
    m.update(p.cuda(), t.cuda())
    assert torch.equal(m.sums, first)                   # reset() cleared the state; the same call gives the same bits
    again = SEVIRFrameScore(mode="1", seq_len=3, data_range=1.0)
    again.update(p.cuda(), t.cuda())
    assert torch.equal(again.sums, first) and torch.equal(again.counts, m.counts)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [5, 32])
def test_hip_frame_score_members_equal_sequential_updates(M):
    shape = (1, 6, 48, 64, 1)
    g = torch.Generator().manual_seed(21 + M)
    t = torch.rand(shape, generator=g)
    ens = (t.unsqueeze(0) + 0.15 * torch.randn((M,) + shape, generator=g)).clamp(0.0, 1.0)
    ec, tc = ens.cuda(), t.cuda()
    for mode in ("1", "0"):
        a, b = (SEVIRFrameScore(mode=mode, seq_len=6, data_range=1.0) for _ in range(2))
        a.update_members(ec, tc)
        for i in range(M):
            b.update(ec[i], tc)
        assert torch.equal(a.counts, b.counts)
        sa, sb = a.sums.cpu().numpy(), b.sums.cpu().numpy()
        assert (np.abs(sa - sb) <= 1e-12 * np.abs(sb)).all(), (sa, sb)
        check(f"update_members M={M} mode {mode}", a, [(ens[i], t) for i in range(M)], "NTHWC", 1.0)
    with pytest.raises(ValueError):
        SEVIRFrameScore(data_range=1.0).update_members(torch.zeros((513, 1, 1, 11, 11, 1), device="cuda"),
                                                       torch.zeros((1, 1, 11, 11, 1), device="cuda"))


@pytest.mark.gpu
def test_evaluate_context_updates_frame_scores():
    """evaluate_context on the tiny latent-diffusion model of the config tests (tiny VAE + axial denoiser + guidance network): the frame
    scores see every sample where the skill scores do."""
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
    B, K = 2, 2
    seq = seeded_input("fsseq", (B, T_in + T_out, H * 4, W * 4, 1), 23, kind="uniform").cuda()
    run_cfg = {"layout": {"in_len": T_in, "out_len": T_out}, "eval": {"num_samples_per_context": K}}
    fs, afs = (SEVIRFrameScore(layout="NTHWC", mode="1", seq_len=T_out, data_range=1.0) for _ in range(2))
    out = CFG.evaluate_context(ldm, seq, run_cfg, frame_score=fs, aligned_frame_score=afs, timesteps=3)
    assert len(out["pred"]) == K and len(out["aligned_pred"]) == K
    tgt = seq[:, T_in:]
    for metric, preds, label in ((fs, out["pred"], "evaluate_context"), (afs, out["aligned_pred"], "evaluate_context aligned")):
        manual = SEVIRFrameScore(layout="NTHWC", mode="1", seq_len=T_out, data_range=1.0)
        for pr in preds:
            manual.update(pr.float(), tgt)
        assert torch.equal(metric.sums, manual.sums) and torch.equal(metric.counts, manual.counts)
        assert int(metric.counts[1, 0]) == B * K
        check(label, metric, [(pr.float().cpu(), tgt.cpu()) for pr in preds], "NTHWC", 1.0)
    assert not torch.equal(fs.sums, afs.sums)
