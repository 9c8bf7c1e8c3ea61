"""prediff_amd.extrapolation on the device: pd_advect and pd_lk_motion against the fp64 restatement of tests/_extrapolation_ref.py,
the exactness properties of the definition, and the forecast through the package's scores.

Whatever the binding writes (the advected frames, the motion field, the workspace) is a slice between two NaN-filled guards of GUARD
floats that must stay NaN, and every input must compare equal afterwards.

Bounds.  Integer motion and zero motion: bit for bit.  Fractional motion: |dev - ref| <= 2^-14 (max - min of frame and fill) -- a
coordinate below 2^9 rounds by <= 2^-15 px against a slope of at most one range per pixel, three lerps add <= 6 * 2^-24 of the range, and
the sum is doubled.  Motion: 8 e32, e32 = max |fp32 restatement - fp64 restatement| of the same case (asserted < 1e-4 px in
test_extrapolation_host.py); the margin covers another summation order and fused multiply-adds."""
import functools

import numpy as np
import pytest
import torch

import _extrapolation_ref as R
from prediff_amd import LagrangianPersistence, SEVIRFrontEnd
from prediff_amd import _lib as L
from prediff_amd.frame_score import SEVIRFrameScore
from prediff_amd.sevir_skill import SEVIRSkillScore

pytestmark = pytest.mark.gpu

GUARD = 1024
SHAPES = [(5, 7), (33, 70)]
B, K = 2, 3


class Guarded:
    """a float32 device tensor of `shape` between two NaN guards"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())


@functools.lru_cache(maxsize=None)
def frames(H, W):
    """seeded random frames (B, H, W), CPU fp32; shared, never written to"""
    return torch.randn((B, H, W), generator=torch.Generator().manual_seed(H * 1000 + W))


@functools.lru_cache(maxsize=None)
def field(H, W, kind):
    """a motion field (B, 2, H, W), CPU fp32: "const" (2, -3), "zero", "int" per-pixel integers in [-4, 4], "frac" per-pixel uniform in
    [-3.5, 3.5]"""
    g = torch.Generator().manual_seed(H * 1000 + W + 7)
    if kind == "const":
        return torch.tensor([2.0, -3.0]).view(1, 2, 1, 1).expand(B, 2, H, W).contiguous()
    if kind == "zero":
        return torch.zeros((B, 2, H, W))
    if kind == "int":
        return torch.randint(-4, 5, (B, 2, H, W), generator=g).float()
    return torch.rand((B, 2, H, W), generator=g) * 7.0 - 3.5


def run_advect(frame, mot, fill, out_len=K):
    """pd_advect through the binding into a guarded output; returns it on the CPU after checking the guards and the inputs"""
    Bn, H, W = frame.shape
    f, m = frame.cuda(), mot.cuda()
    out = Guarded((Bn, out_len, H, W, 1))
    L.advect(f, m, out.t, Bn, out_len, H, W, H * W, fill)
    torch.cuda.synchronize()
    assert out.intact()
    assert torch.equal(f.cpu(), frame) and torch.equal(m.cpu().view(torch.int32), mot.view(torch.int32))
    return out.t.cpu()


@pytest.mark.parametrize("fill", [0.0, -1.5])
@pytest.mark.parametrize("kind", ["const", "zero", "int"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_hip_advect_integer_motion_bit_for_bit(H, W, kind, fill):
    frame, mot = frames(H, W), field(H, W, kind)
    got = run_advect(frame, mot, fill)
    v = mot.long()
    yy, xx = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    bb = torch.arange(B).view(B, 1, 1)
    shifted_out = 0
    for k in range(1, K + 1):
        sy, sx = yy - k * v[:, 0], xx - k * v[:, 1]
        inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        want = torch.where(inside, frame[bb, sy.clamp(0, H - 1), sx.clamp(0, W - 1)], torch.tensor(fill))
        assert torch.equal(got[:, k - 1, :, :, 0], want), (kind, k)
        assert (got[:, k - 1, :, :, 0][~inside] == fill).all()
        shifted_out += int((~inside).sum())
    if kind == "zero":
        assert shifted_out == 0 and all(torch.equal(got[:, k, :, :, 0], frame) for k in range(K))
    else:
        assert shifted_out > 0


@pytest.mark.parametrize("fill", [0.0, -1.5])
@pytest.mark.parametrize("H,W", SHAPES)
def test_hip_advect_fractional_motion(H, W, fill):
    frame, mot = frames(H, W), field(H, W, "frac")
    got = run_advect(frame, mot, fill).double().numpy()
    ref = R.advect(frame.numpy(), mot.numpy(), K, fill=fill)
    span = max(float(frame.max()), fill) - min(float(frame.min()), fill)
    # some taps are half inside: a coordinate strictly between -1 and 0, or between the last cell and the one after it
    cy = np.arange(H)[None, :, None] - mot[:, 0].double().numpy()
    assert (((cy > -1) & (cy < 0)) | ((cy > H - 1) & (cy < H))).any()
    dev = np.abs(got - ref).max()
    print(f"[extrapolation] advect {H}x{W} fill={fill}: max |dev - ref| = {dev:.2e}, bound {2.0 ** -14 * span:.2e}")
    assert dev <= 2.0 ** -14 * span


def test_hip_advect_hostile_motion():
    H, W = 33, 70
    fill = -1.5
    frame, mot = frames(H, W), field(H, W, "frac").clone()
    hostile = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]
    g = torch.Generator().manual_seed(5)
    where = torch.zeros((B, H, W), dtype=torch.bool)
    for i, bad in enumerate(hostile * 4):
        b, c, y, x = int(torch.randint(B, (1,), generator=g)), i % 2, int(torch.randint(H, (1,), generator=g)), int(torch.randint(W, (1,), generator=g))
        mot[b, c, y, x] = bad
        where[b, y, x] = True
    mot[1, :, 0, 0] = torch.tensor([float("nan"), float("inf")])                    # both components at once, in a corner
    where[1, 0, 0] = True
    got = run_advect(frame, mot, fill)
    assert torch.isfinite(got).all()
    for k in range(K):
        assert (got[:, k, :, :, 0][where] == fill).all()
    ref = R.advect(frame.numpy(), mot.numpy(), K, fill=fill)
    span = max(float(frame.max()), fill) - min(float(frame.min()), fill)
    assert (ref[:, :, :, :, 0][np.broadcast_to(where.numpy()[:, None], (B, K, H, W))] == fill).all()
    assert np.abs(got.double().numpy() - ref).max() <= 2.0 ** -14 * span


# ------------------------------------------------------------------------------------------------ motion
@pytest.mark.parametrize("name", list(R.MOTION_CASES))
def test_hip_motion_against_restatement(name):
    ctx_np, opts, m64, e32 = R.motion_case(name)
    Bn, T, H, W, _ = ctx_np.shape
    ctx = torch.from_numpy(ctx_np.copy()).cuda()
    need = L.lk_ws_bytes(Bn, T, H, W, opts["levels"], opts["iters"], opts["radius"], opts["pairs"])
    assert need > 0 and need % 4 == 0
    out, ws = Guarded((Bn, 2, H, W)), Guarded((need // 4,))
    L.lk_motion(ctx, out.t, Bn, T, H, W, opts["levels"], opts["iters"], opts["radius"], opts["damping"], opts["pairs"], ws.t)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    assert np.array_equal(ctx.cpu().numpy(), ctx_np)
    got = out.t.cpu().double().numpy()
    dev = np.abs(got - m64).max()
    print(f"[extrapolation] motion {name}: max |dev - ref| = {dev:.2e} px, e32 = {e32:.2e}, bound {8 * e32:.2e}")
    assert np.isfinite(got).all()
    assert dev <= 8 * e32
    # the class gives the same bits as the binding
    lp = LagrangianPersistence(out_len=1, **opts)
    assert torch.equal(lp.motion(ctx), out.t)


def test_hip_workspace_too_small_is_refused():
    ctx = torch.zeros((1, 3, 16, 16, 1), device="cuda")
    need = L.lk_ws_bytes(1, 3, 16, 16, 2, 3, 2, 3)
    with pytest.raises(L.PrediffHipError, match="workspace"):
        L.lk_motion(ctx, torch.empty((1, 2, 16, 16), device="cuda"), 1, 3, 16, 16, 2, 3, 2, 1e-2, 3, torch.empty(need // 4 - 1, device="cuda"))
    with pytest.raises(L.PrediffHipError, match="radius"):
        L.lk_motion(ctx, torch.empty((1, 2, 16, 16), device="cuda"), 1, 3, 16, 16, 2, 3, 12, 1e-2, 3, torch.empty(need // 4, device="cuda"))


# ------------------------------------------------------------------------------------------------ exactness
def test_hip_zero_context_gives_zero_motion_and_forecast():
    ctx = torch.zeros((2, 4, 40, 72, 1), device="cuda")
    lp = LagrangianPersistence(levels=3, radius=4)
    m, f = lp.motion(ctx), lp.forecast(ctx)
    assert m.shape == (2, 2, 40, 72) and f.shape == (2, 6, 40, 72, 1)
    assert bool((m == 0).all()) and bool((f == 0).all())
    assert lp.forecast(ctx, out_len=2).shape == (2, 2, 40, 72, 1)


def test_hip_batch_equals_sequences_alone_and_runs_repeat():
    ctx_np = R.motion_case("16x24")[0]
    ctx = torch.from_numpy(ctx_np.copy()).cuda()
    lp = LagrangianPersistence(out_len=4, levels=2, radius=2)
    m, f = lp.motion(ctx), lp.forecast(ctx)
    assert ctx.shape[0] == 3
    for b in range(3):
        one = ctx[b:b + 1].contiguous()
        assert torch.equal(lp.motion(one), m[b:b + 1]) and torch.equal(lp.forecast(one), f[b:b + 1])
    assert torch.equal(lp.motion(ctx), m) and torch.equal(lp.forecast(ctx), f)
    assert torch.equal(LagrangianPersistence(out_len=4, levels=2, radius=2).forecast(ctx), f)
    assert np.array_equal(ctx.cpu().numpy(), ctx_np)
    # forecast is advect of the last frame along motion; a (B, H, W, 1) frame and a (B, H, W) frame are the same call
    assert torch.equal(lp.advect(ctx[:, -1], m), f) and torch.equal(lp.advect(ctx[:, -1, :, :, 0].contiguous(), m), f)


def test_hip_forecast_replays_from_a_graph():
    a = torch.from_numpy(R.motion_case("40x72")[0].copy()).cuda()
    b = a.flip(0).contiguous()
    lp = LagrangianPersistence(levels=3, radius=4, pairs=2)
    eager = [lp.forecast(x) for x in (a, b)]                                       # the first call allocates the workspace
    assert not torch.equal(eager[0], eager[1])
    static = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lp.forecast(static)
    for x, ref in ((b, eager[1]), (a, eager[0])):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------ through the package
@pytest.mark.parametrize("name", ["64-slow", "64-fast"])
def test_hip_forecast_through_the_scores(name):
    """The forecast goes into the scores as it is.  Per lead: its MSE is < 0.25 x Eulerian persistence's (the zero-motion advect) on the
    inputs the host test proved that for, and the frame score's MSE of it equals the fp64 MSE of the same frames to the score's own 1e-12.

    Against the restatement's forecast f64 that 1e-12 cannot hold: the two forecasts differ by fp32 rounding of the motion and of the
    interpolation.  What holds the device instead is the restatement's own fp32 error, as for the motion: with f32 the forecast
    restated in fp32 throughout, r32 = rms(f32 - f64) and x32 = max |f32 - f64| per lead, the device forecast must sit within
    rms <= 8 r32 and max <= 8 x32 of f64, and its MSE -- by Cauchy-Schwarz on (f - t) = (f64 - t) + (f - f64) -- within
    2 sqrt(mse64) 8 r32 + (8 r32)^2 of mse64: 4e-5 .. 3e-4 of mse64 on these sequences (|mse32 - mse64| itself is printed beside it; it
    is a signed sum that cancels to 3e-7 .. 3e-6 of mse64 and is no stable yardstick)."""
    ctx_np, tgt_np, levels, m64, f64, f32 = R.skill_case(name)
    ctx, tgt = torch.from_numpy(ctx_np.copy()).cuda(), torch.from_numpy(tgt_np.copy()).cuda()
    Kt = tgt.shape[1]
    lp = LagrangianPersistence(out_len=Kt, levels=levels)
    fc = lp.forecast(ctx)
    pers = lp.advect(ctx[:, -1], torch.zeros((ctx.shape[0], 2) + tuple(ctx.shape[2:4]), device="cuda"))
    assert fc.shape == tgt.shape and all(torch.equal(pers[:, k], ctx[:, -1]) for k in range(Kt))

    def mse(pred):
        s = SEVIRFrameScore(mode="1", seq_len=Kt, metrics_list=("mse", "mae"))
        s.update(pred, tgt)
        return s.compute()["mse"]

    mse_f, mse_p = mse(fc), mse(pers)
    print(f"[extrapolation] {name}: device MSE / persistence's per lead {np.round(mse_f / mse_p, 4).tolist()}")
    assert mse_f.shape == (Kt,) and (mse_f < 0.25 * mse_p).all()
    own = ((fc.cpu().double().numpy() - tgt_np) ** 2).mean(axis=(0, 2, 3, 4))
    assert np.allclose(mse_f, own, rtol=1e-12, atol=0)
    ax = (0, 2, 3, 4)
    mse64 = ((f64 - tgt_np) ** 2).mean(axis=ax)
    mse32 = ((f32.astype(np.float64) - tgt_np) ** 2).mean(axis=ax)
    d32, dev = f32.astype(np.float64) - f64, fc.cpu().double().numpy() - f64
    r32, x32 = np.sqrt((d32 ** 2).mean(axis=ax)), np.abs(d32).max(axis=ax)
    rdev, xdev = np.sqrt((dev ** 2).mean(axis=ax)), np.abs(dev).max(axis=ax)
    bound = 2 * np.sqrt(mse64) * 8 * r32 + (8 * r32) ** 2
    with np.printoptions(precision=2):
        print(f"[extrapolation] {name}: rms(dev - f64) {rdev} against r32 {r32}; max {xdev} against x32 {x32}")
        print(f"[extrapolation] {name}: |mse_dev - mse64| {np.abs(mse_f - mse64)} bound {bound}; |mse32 - mse64| {np.abs(mse32 - mse64)}")
    assert (r32 > 0).all() and (rdev <= 8 * r32).all() and (xdev <= 8 * x32).all()
    assert (np.abs(mse_f - mse64) <= bound).all()

    # CSI / POD / bias of the same tensors, on the 0 .. 255 scale the thresholds are in, with no reshaping
    skill = SEVIRSkillScore(layout="NTHWC", mode="1", seq_len=Kt, threshold_list=(16, 74), metrics_list=("csi", "pod", "bias"))
    skill_p = SEVIRSkillScore(layout="NTHWC", mode="1", seq_len=Kt, threshold_list=(16, 74), metrics_list=("csi", "pod", "bias"))
    skill.update(fc, tgt)
    skill_p.update(pers, tgt)
    csi, csi_p = skill.compute()[16]["csi"], skill_p.compute()[16]["csi"]
    assert csi.shape == (Kt,) and (csi > csi_p).all()
    vil = SEVIRFrontEnd().export(fc)
    assert vil.shape == fc.shape[:4] and vil.dtype == torch.uint8
