"""prediff_amd.anvil on the device: pd_anvil_analyse / pd_anvil_evolve (and pd_steps_finish as step 10) against the fp64 restatement of
tests/_anvil_ref.py, the exactness properties of the definition, and the forecast through the package's scores.

Whatever the bindings write (phi, gamma, R, the forecast, the workspace) is a slice between two NaN-filled guards of GUARD floats that
must stay NaN, and every input must compare equal afterwards.

Bounds.  Against the restatement: 8 e32, e32 = max |fp32 restatement - fp64 restatement| of the same quantity of the same case
(measured and bounded in test_anvil_host.py); the margin covers another summation order, the packed transforms and fused multiply-adds.
Step 10: on the device's own R against step 10 of the restatement on that R; the pixels within 8 e32(R) of the threshold may be cut on
either side and are left out with the output pixels whose taps they are (at most 1 %), the rest agrees within the fractional-motion
bound of test_extrapolation.py, 2^-14 of the range."""
import numpy as np
import pytest
import torch

import _anvil_ref as A
import _steps_ref as S
from prediff_amd import AutoregressiveExtrapolation, LagrangianPersistence
from prediff_amd import _lib as L
from prediff_amd.frame_score import SEVIRFrameScore

pytestmark = pytest.mark.gpu

GUARD = 1024
AX = (0, 2, 3, 4)


class Guarded:
    """a float32 device tensor of `shape` between two NaN guards, NaN itself until written"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())


def cuda(c):
    return torch.from_numpy(c.ctx.copy()).cuda(), torch.from_numpy(c.motion.copy()).cuda()


def run_device(c, finish=False):
    """pd_anvil_analyse and pd_anvil_evolve (and step 10) through the bindings into guarded buffers; returns the outputs on the CPU as
    fp64 after checking the guards and the inputs"""
    ctx, motion = cuda(c)
    w, g = torch.from_numpy(c.w.copy()).cuda(), torch.from_numpy(c.g.copy()).cuda()
    B, T, H, W, Lv, K = c.B, c.T, c.H, c.W, c.L, c.K
    need = L.anvil_ws_bytes(B, H, W, Lv, c.ar)
    assert need > 0 and need % 16 == 0
    ws = Guarded((need // 4,))
    out = dict(phi=Guarded((B, Lv, 2, H, W)), gamma=Guarded((B, Lv, 2, H, W)), R=Guarded((B, K, H, W)))
    L.anvil_analyse(ctx, motion, w, g, c.W0, B, T, H, W, Lv, c.ar, out["phi"].t, out["gamma"].t, ws.t)
    L.anvil_evolve(out["phi"].t, B, K, H, W, Lv, c.ar, out["R"].t, ws.t)
    if finish:
        out["out"] = Guarded((B, K, H, W, 1))
        L.steps_finish(ctx, motion, out["R"].t, out["out"].t, 1, B, T, K, H, W, c.thr, 0, 0)
    torch.cuda.synchronize()
    assert ws.intact() and all(x.intact() for x in out.values())
    assert np.array_equal(ctx.cpu().numpy(), c.ctx) and np.array_equal(motion.cpu().numpy(), c.motion)
    assert np.array_equal(w.cpu().numpy(), c.w) and np.array_equal(g.cpu().numpy(), c.g)
    got = {k: x.t.cpu().double().numpy() for k, x in out.items()}
    assert all(np.isfinite(v).all() for v in got.values())
    return got


def engine(c, **kw):
    """the class at the case's options; its motion estimator fits the smallest frames (two pyramid levels)"""
    return AutoregressiveExtrapolation(out_len=c.K, levels=c.L, ar_order=c.ar, window=c.window,
                                       motion=LagrangianPersistence(levels=2, radius=3), **kw)


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name", list(A.CASES))
def test_hip_analyse_and_evolve_against_restatement(name):
    c = A.case(name)
    got = run_device(c)
    for k in ("gamma", "phi", "R"):
        dev = np.abs(got[k] - getattr(c, k)).max()
        print(f"[anvil] {name} {k}: max |dev - ref| = {dev:.2e}, e32 = {c.e32[k]:.2e}, bound {8 * c.e32[k]:.2e}")
    for k in ("gamma", "phi", "R"):
        assert np.abs(got[k] - getattr(c, k)).max() <= 8 * c.e32[k], k
    # the class gives the same bits as the bindings
    ctx, motion = cuda(c)
    ae = engine(c)
    an = ae.analyse(ctx, motion)
    assert all(np.array_equal(an[k].cpu().double().numpy(), got[k]) for k in ("gamma", "phi"))
    assert an["motion"] is motion and an["phi"].shape == an["gamma"].shape == (c.B, c.L, 2, c.H, c.W)
    R = ae.evolve(ctx, motion)
    assert R.shape == (c.B, c.K, c.H, c.W) and np.array_equal(R.cpu().double().numpy(), got["R"])


@pytest.mark.parametrize("name", list(A.CASES))
def test_hip_forecast_against_restatement(name):
    c = A.case(name)
    got = run_device(c, finish=True)
    R = got["R"]
    ref = A.finish(R, c.motion, c.thr)
    thr = float(np.float32(c.thr))
    near = np.abs(R - thr) <= 8 * c.e32["R"]
    left_out = S.advect_leads(near[None].astype(np.float64), c.motion)[0][..., None] > 0   # the output pixels with a near pixel among their taps
    share = left_out.mean()
    span = max(float(np.where(R > thr, R, 0.0).max()), 0.0)
    dev = np.abs(got["out"] - ref)[~left_out].max()
    print(f"[anvil] forecast {name}: {int(near.sum())} pixels near thr, {share:.2%} of the output left out; "
          f"max |dev - ref| = {dev:.2e}, bound {2.0 ** -14 * span:.2e}")
    assert share <= 0.01
    assert dev <= 2.0 ** -14 * span
    wet = (got["out"] > 0).mean()
    assert 0.02 < wet < 0.98 and (got["out"] >= 0).all()
    # the class: the same bits
    ctx, motion = cuda(c)
    fc = engine(c).forecast(ctx, motion)
    assert fc.shape == (c.B, c.K, c.H, c.W, 1) and np.array_equal(fc.cpu().double().numpy(), got["out"])


# ------------------------------------------------------------------------------------------------ exact properties
def test_hip_zero_context_gives_zeros():
    c = A.case("24x16-ar2")
    ctx, motion = cuda(c)
    ae = engine(c)
    dark = torch.zeros_like(ctx)
    for kw in (dict(motion=motion), dict()):
        f, R = ae.forecast(dark, **kw), ae.evolve(dark, **kw)
        assert f.shape == (c.B, c.K, c.H, c.W, 1) and bool((f == 0).all()) and bool((R == 0).all())
    an = ae.analyse(dark)
    assert bool((an["phi"] == 0).all()) and bool((an["gamma"] == 0).all()) and bool((an["motion"] == 0).all())


def test_hip_persistence_limit():
    """identical frames and zero motion: every difference is exactly zero on the device too, and R^(k) is the sum of the levels"""
    p = S.persistence_case()
    ctx = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(p.ctx[:, :1], (1, 4, 16, 16, 1)))).cuda()
    ae = AutoregressiveExtrapolation(out_len=p.K, levels=p.L, window=2.0)
    R = ae.evolve(ctx, torch.zeros((1, 2, 16, 16), device="cuda"))
    d = float(np.abs(R.cpu().double().numpy() - p.A0[:, None]).max())
    print(f"[anvil] persistence: max |R^(k) - A_0| = {d:.2e}")
    assert d <= 1e-6 and all(torch.equal(R[:, k], R[:, 0]) for k in range(p.K))


def test_hip_sequences_are_independent_and_runs_repeat():
    c = A.case("24x16-ar2")
    ctx, motion = cuda(c)
    ae = engine(c)
    an, R, f = ae.analyse(ctx, motion), ae.evolve(ctx, motion), ae.forecast(ctx, motion)
    assert c.B == 2 and not torch.equal(f[0], f[1])
    held = ae._ws[str(ctx.device)][1]
    for b in range(c.B):                                                           # a sequence alone
        xb, vb = ctx[b:b + 1].contiguous(), motion[b:b + 1].contiguous()
        one = ae.analyse(xb, vb)
        assert torch.equal(one["phi"], an["phi"][b:b + 1]) and torch.equal(one["gamma"], an["gamma"][b:b + 1])
        assert torch.equal(ae.evolve(xb, vb), R[b:b + 1]) and torch.equal(ae.forecast(xb, vb), f[b:b + 1])
    again = ae.analyse(ctx, motion)
    assert torch.equal(again["phi"], an["phi"]) and torch.equal(again["gamma"], an["gamma"])
    assert torch.equal(ae.evolve(ctx, motion), R) and torch.equal(ae.forecast(ctx, motion), f)
    assert torch.equal(engine(c).forecast(ctx, motion), f)
    # a shorter horizon is a prefix; the estimated motion is LagrangianPersistence's, and the field analyse returns is the one used
    assert torch.equal(ae.forecast(ctx, motion, out_len=2), f[:, :2])
    est = ae.analyse(ctx)["motion"]
    assert torch.equal(est, ae.motion.motion(ctx)) and torch.equal(ae.forecast(ctx), ae.forecast(ctx, est))
    assert torch.equal(ae.forecast(ctx, motion), ae.forecast(ctx, ae.analyse(ctx, motion)["motion"]))
    # one workspace serves every call at the frame size with no more sequences (the single sequences above too): nothing is
    # reallocated under a captured graph
    ae.analyse(ctx, motion), ae.forecast(ctx, motion), ae.evolve(ctx, motion, out_len=5)
    assert ae._ws[str(ctx.device)][1] is held


def test_hip_forecast_replays_from_a_graph():
    c = A.case("32x64-ar2")
    ctx, motion = cuda(c)
    other = (ctx.flip(0).contiguous(), motion.flip(0).contiguous())
    ae = engine(c)
    eager = [ae.forecast(x, v) for x, v in ((ctx, motion), other)]                 # the first call allocates the workspace
    assert not torch.equal(eager[0], eager[1])
    static = [t.clone() for t in (ctx, motion)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ae.forecast(static[0], static[1])
    for src, ref in ((other, eager[1]), ((ctx, motion), eager[0])):
        for dst, t in zip(static, src):
            dst.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def test_hip_workspace_too_small_is_refused_and_nothing_is_written():
    c = A.case("16x16-ar1")
    ctx, motion = cuda(c)
    w, g = torch.from_numpy(c.w.copy()).cuda(), torch.from_numpy(c.g.copy()).cuda()
    need = L.anvil_ws_bytes(c.B, c.H, c.W, c.L, c.ar)
    par = [Guarded((c.B, c.L, 2, c.H, c.W)) for _ in range(2)]
    small = Guarded((need // 4,))
    short = small.t.view(torch.uint8)[:need - 1]                                   # one byte too small
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*workspace"):
        L.anvil_analyse(ctx, motion, w, g, c.W0, c.B, c.T, c.H, c.W, c.L, c.ar, par[0].t, par[1].t, short)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(x.buf).all()) for x in par) and bool(torch.isnan(small.buf).all())
    ws, R = Guarded((need // 4,)), Guarded((c.B, c.K, c.H, c.W))
    L.anvil_analyse(ctx, motion, w, g, c.W0, c.B, c.T, c.H, c.W, c.L, c.ar, par[0].t, par[1].t, ws.t)
    torch.cuda.synchronize()
    before = ws.buf.clone()
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*workspace"):
        L.anvil_evolve(par[0].t, c.B, c.K, c.H, c.W, c.L, c.ar, R.t, ws.t.view(torch.uint8)[:need - 1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(R.buf).all()) and torch.equal(ws.buf.view(torch.int32), before.view(torch.int32))


def test_hip_calls_refuse_bad_fields():
    c = A.case("16x16-ar1")
    ctx, motion = cuda(c)
    ae = engine(c)
    for v, msg in ((motion[:, :1].contiguous(), r"motion must be \(2, 2, 16, 16\)"), (motion.double(), "motion must be a float32"),
                   (motion.cpu(), "no CPU path"), (motion.transpose(2, 3), "motion must be contiguous")):
        for call in (ae.analyse, ae.evolve, ae.forecast):
            with pytest.raises(ValueError, match=msg):
                call(ctx, v)
    # the library: a window that is no table of 2 r + 1 weights, a context too short, an output that is an input, a misaligned output
    w, g = torch.from_numpy(c.w.copy()).cuda(), torch.from_numpy(c.g.copy()).cuda()
    ws = torch.empty(L.anvil_ws_bytes(c.B, c.H, c.W, c.L, c.ar) // 4, device="cuda")
    phi, gamma = (torch.empty((c.B, c.L, 2, c.H, c.W), device="cuda") for _ in range(2))
    args = (c.B, c.T, c.H, c.W, c.L, c.ar)
    with pytest.raises(L.PrediffHipError, match=r"window must hold the 2 r \+ 1 weights"):
        L.anvil_analyse(ctx, motion, w, g[:-1].contiguous(), c.W0, *args, phi, gamma, ws)
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*2 context frames, AR\(1\) on first differences needs >= 3"):
        L.anvil_analyse(ctx[:, :2].contiguous(), motion, w, g, c.W0, c.B, 2, c.H, c.W, c.L, c.ar, phi, gamma, ws)
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*window_sum_sq must be positive"):
        L.anvil_analyse(ctx, motion, w, g, 0.0, *args, phi, gamma, ws)
    with pytest.raises(L.PrediffHipError, match="phi must be a contiguous fp32 tensor of 3072 elements"):
        L.anvil_analyse(ctx, motion, w, g, c.W0, *args, phi[:1], gamma, ws)
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*R aliases an input"):
        L.anvil_evolve(phi, c.B, 2 * c.L, c.H, c.W, c.L, c.ar, phi, ws)
    R = torch.empty(c.B * c.K * c.H * c.W + 1, device="cuda")[1:]
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*16-byte aligned"):
        L.anvil_evolve(phi, c.B, c.K, c.H, c.W, c.L, c.ar, R, ws)


# ------------------------------------------------------------------------------------------------ through the package
def test_hip_forecast_through_the_scores():
    """The 128 x 128 case through SEVIRFrameScore, per lead.  Its MSE is below 0.75 of that of LagrangianPersistence.advect with the same
    motion (test_anvil_host.py proved that of the restatement on these inputs), and within the Cauchy-Schwarz bound of
    test_extrapolation.py of the restatement's MSE, built from this case's own fp32 error: with f32 the forecast restated in fp32
    throughout, r32 = rms(f32 - f64) and x32 = max |f32 - f64| per lead, the device forecast must sit within rms <= 8 r32 and
    max <= 8 x32 of f64, and its MSE -- by Cauchy-Schwarz on (f - t) = (f64 - t) + (f - f64) -- within 2 sqrt(mse64) 8 r32 + (8 r32)^2
    of mse64.  (A pixel cut on the other side of the threshold than in f64 would break this by orders of magnitude: none is.)"""
    c = A.case("128x128-ar2")
    ctx, motion = cuda(c)
    tgt = torch.from_numpy(c.tgt.copy()).cuda()
    ae = engine(c)
    fc = ae.forecast(ctx, motion)
    pers = ae.motion.advect(ctx[:, -1], motion, c.K)
    assert fc.shape == pers.shape == tgt.shape
    assert np.abs(pers.cpu().double().numpy() - c.persistence).max() <= 2.0 ** -14 * float(c.ctx.max())

    def mse(pred):
        s = SEVIRFrameScore(mode="1", seq_len=c.K, metrics_list=("mse", "mae"))
        s.update(pred, tgt)
        return s.compute()["mse"]

    mse_f, mse_p = mse(fc), mse(pers)
    print(f"[anvil] 128x128-ar2: device MSE / Lagrangian persistence's per lead {np.round(mse_f / mse_p, 4).tolist()}")
    assert mse_f.shape == (c.K,) and (mse_f < 0.75 * mse_p).all()
    own = ((fc.cpu().double().numpy() - c.tgt) ** 2).mean(axis=AX)
    assert np.allclose(mse_f, own, rtol=1e-12, atol=0)
    mse64 = ((c.forecast - c.tgt) ** 2).mean(axis=AX)
    d32, dev = c.forecast32.astype(np.float64) - c.forecast, fc.cpu().double().numpy() - c.forecast
    r32, x32 = np.sqrt((d32 ** 2).mean(axis=AX)), np.abs(d32).max(axis=AX)
    rdev, xdev = np.sqrt((dev ** 2).mean(axis=AX)), np.abs(dev).max(axis=AX)
    bound = 2 * np.sqrt(mse64) * 8 * r32 + (8 * r32) ** 2
    sci = lambda a: "[" + " ".join(f"{v:.2e}" for v in a) + "]"
    print(f"[anvil] 128x128-ar2: rms(dev - f64) {sci(rdev)} against r32 {sci(r32)}; max {sci(xdev)} against x32 {sci(x32)}")
    print(f"[anvil] 128x128-ar2: |mse_dev - mse64| {sci(np.abs(mse_f - mse64))} bound {sci(bound)}, mse64 {sci(mse64)}")
    assert (r32 > 0).all() and (rdev <= 8 * r32).all() and (xdev <= 8 * x32).all()
    assert (np.abs(mse_f - mse64) <= bound).all()
