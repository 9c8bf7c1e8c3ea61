"""prediff_amd.steps on the device: pd_steps_analyse / pd_steps_evolve / pd_steps_finish against the fp64 restatement of
tests/_steps_ref.py, the exactness properties of the definition, and the ensemble through the package's scores.

Whatever the bindings write (the parameters, R, the forecast, the workspace) is a slice between two NaN-filled guards of GUARD floats that
must stay NaN, and every input must compare equal afterwards.

Bounds.  Against the restatement: 8 e32, e32 = max |fp32 restatement - fp64 restatement| of the same quantity of the same case
(measured and bounded in test_steps_host.py); the margin covers another summation order and fused multiply-adds.  Step 9: on the device's
own R against step 9 of the restatement on that R; the pixels within delta = 8 e32(R) of the threshold may be cut on either side and
are left out with the output pixels whose taps they are (at most 1 %), the rest agrees within the fractional-motion bound of
test_extrapolation.py, 2^-14 of the range."""
import numpy as np
import pytest
import torch

import _extrapolation_ref as X
import _steps_ref as S
from prediff_amd import LagrangianPersistence, StochasticExtrapolation, steps_bands
from prediff_amd import _lib as L
from prediff_amd.ensemble_score import SEVIREnsembleScore
from prediff_amd.frame_score import SEVIRFrameScore

pytestmark = pytest.mark.gpu

GUARD = 1024


class Guarded:
    """a float32 device tensor of `shape` between two NaN guards, NaN itself until written"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())


def run_device(c, noise, M, finish=None):
    """pd_steps_analyse and pd_steps_evolve (and pd_steps_finish with finish = (mask, match)) through the bindings into guarded buffers;
    returns the outputs on the CPU as fp64 after checking the guards and the inputs"""
    ctx, motion, w = torch.from_numpy(c.ctx.copy()).cuda(), torch.from_numpy(c.motion.copy()).cuda(), torch.from_numpy(c.w.copy()).cuda()
    nz = None if noise is None else torch.from_numpy(noise.copy()).cuda()
    B, T, H, W, Lv, K = c.B, ctx.shape[1], c.H, c.W, c.L, c.K
    need = L.steps_ws_bytes(B, M, H, W, Lv, c.ar)
    assert need > 0 and need % 8 == 0
    ws = Guarded((need // 4,))
    out = dict(mu=Guarded((B, Lv)), sigma=Guarded((B, Lv)), phi=Guarded((B, Lv, 3)), gamma=Guarded((B, Lv, 2)), R=Guarded((M, B, K, H, W)))
    L.steps_analyse(ctx, motion, w, B, T, H, W, Lv, c.ar, c.thr, out["mu"].t, out["sigma"].t, out["phi"].t, out["gamma"].t, ws.t)
    L.steps_evolve(nz, w, out["mu"].t, out["sigma"].t, out["phi"].t, M, B, K, H, W, Lv, c.ar, out["R"].t, ws.t)
    if finish is not None:
        out["out"] = Guarded((M, B, K, H, W, 1))
        L.steps_finish(ctx, motion, out["R"].t, out["out"].t, M, B, T, K, H, W, c.thr, int(finish[0] == "obs"), int(finish[1] == "mean"))
    torch.cuda.synchronize()
    assert ws.intact() and all(g.intact() for g in out.values())
    assert np.array_equal(ctx.cpu().numpy(), c.ctx) and np.array_equal(motion.cpu().numpy(), c.motion) and np.array_equal(w.cpu().numpy(), c.w)
    assert noise is None or np.array_equal(nz.cpu().numpy(), noise)
    got = {k: g.t.cpu().double().numpy() for k, g in out.items()}
    assert all(np.isfinite(v).all() for v in got.values())
    return got


def cuda(c):
    return torch.from_numpy(c.ctx.copy()).cuda(), torch.from_numpy(c.motion.copy()).cuda(), torch.from_numpy(c.noise.copy()).cuda()


def engine(c, **kw):
    """the class at the case's options; its motion estimator fits the smallest frames (two pyramid levels)"""
    return StochasticExtrapolation(out_len=c.K, levels=c.L, ar_order=c.ar, motion=LagrangianPersistence(levels=2, radius=3), **kw)


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name", list(S.CASES))
def test_hip_analyse_and_evolve_against_restatement(name):
    c = S.case(name)
    got = run_device(c, c.noise, c.M)
    got0 = run_device(c, None, 1)
    for k in ("mu", "sigma", "gamma", "phi", "R"):
        dev = np.abs(got[k] - getattr(c, k)).max()
        print(f"[steps] {name} {k}: max |dev - ref| = {dev:.2e}, e32 = {c.e32[k]:.2e}, bound {8 * c.e32[k]:.2e}")
    dev0 = np.abs(got0["R"] - c.R0).max()
    print(f"[steps] {name} R (no noise): max |dev - ref| = {dev0:.2e}, e32 = {c.e32['R0']:.2e}, bound {8 * c.e32['R0']:.2e}")
    for k in ("mu", "sigma", "gamma", "phi", "R"):
        assert np.abs(got[k] - getattr(c, k)).max() <= 8 * c.e32[k], k
    assert dev0 <= 8 * c.e32["R0"]
    assert all(np.array_equal(got[k], got0[k]) for k in ("mu", "sigma", "gamma", "phi"))
    # the class gives the same bits as the bindings
    ctx, motion, nz = cuda(c)
    se = engine(c)
    an = se.analyse(ctx, motion)
    assert all(np.array_equal(an[k].cpu().double().numpy(), got[k]) for k in ("mu", "sigma", "gamma", "phi"))
    assert an["motion"] is motion and an["phi"].shape == (c.B, c.L, 3) and an["gamma"].shape == (c.B, c.L, 2)
    assert np.array_equal(se.evolve(ctx, nz, motion).cpu().double().numpy(), got["R"])
    assert np.array_equal(se.evolve(ctx, motion=motion).cpu().double().numpy(), got0["R"])


@pytest.mark.parametrize("name,mask,match", S.FINISH_RUNS)
def test_hip_finish_against_restatement(name, mask, match):
    c = S.case(name)
    got = run_device(c, c.noise, c.M, finish=(mask, match))
    R = got["R"]
    ref = S.finish(R, c.ctx, c.motion, c.thr, mask, match)
    Rm, forced = S.mask_match(R, c.ctx, c.thr, mask, match)
    thr = float(np.float32(c.thr))
    near = (np.abs(Rm - thr) <= 8 * c.e32["R"]) & ~forced
    left_out = S.advect_leads(near.astype(np.float64), c.motion)[..., None] > 0    # the output pixels with a near pixel among their taps
    share = left_out.mean()
    span = max(float(np.where(Rm > thr, Rm, 0.0).max()), 0.0)
    dev = np.abs(got["out"] - ref)[~left_out].max()
    print(f"[steps] finish {name} mask={mask} match={match}: {int(near.sum())} pixels near thr, {share:.2%} of the output left out; "
          f"max |dev - ref| = {dev:.2e}, bound {2.0 ** -14 * span:.2e}")
    assert share <= 0.01
    assert dev <= 2.0 ** -14 * span
    wet = (got["out"] > 0).mean()
    assert 0.02 < wet < 0.98 and (got["out"] >= 0).all()
    # the class: the same bits
    ctx, motion, nz = cuda(c)
    fc = engine(c, mask=mask, match=match).forecast(ctx, noise=nz, motion=motion)
    assert fc.shape == (c.M, c.B, c.K, c.H, c.W, 1) and np.array_equal(fc.cpu().double().numpy(), got["out"])


def test_hip_persistence_limit():
    p = S.persistence_case()
    ctx, motion = torch.from_numpy(p.ctx.copy()).cuda(), torch.from_numpy(p.motion.copy()).cuda()
    R = StochasticExtrapolation(out_len=p.K, levels=p.L, ar_order=2).evolve(ctx, motion=motion).cpu().double().numpy()
    d = np.abs(R - p.A0[None, :, None]).max(axis=(0, 1, 3, 4))
    bound = p.K * S.EPS * p.sum_sigma + 8 * p.e32
    print(f"[steps] persistence: |R^(k) - A_0| = {d}, bound {bound:.3e} (e32 {p.e32:.2e})")
    assert R.shape == (1, 1, p.K, 16, 16) and (d <= bound).all()
    assert np.abs(R - p.R).max() <= 8 * p.e32


# ------------------------------------------------------------------------------------------------ exact properties
def test_hip_no_noise_equals_zero_noise_and_zero_context_gives_zeros():
    c = S.case("24x16-ar2")
    ctx, motion, nz = cuda(c)
    se = engine(c)
    zero = torch.zeros((1, c.B, c.K, c.H, c.W), device="cuda")
    assert torch.equal(se.evolve(ctx, motion=motion), se.evolve(ctx, zero, motion))
    assert torch.equal(se.forecast(ctx, motion=motion), se.forecast(ctx, noise=zero, motion=motion))
    assert se.forecast(ctx, motion=motion).shape == (1, c.B, c.K, c.H, c.W, 1)
    dark = torch.zeros_like(ctx)
    for kw in (dict(noise=nz, motion=motion), dict(noise=nz), dict(members=2), dict()):
        f = se.forecast(dark, **kw)
        assert f.shape[1:] == (c.B, c.K, c.H, c.W, 1) and bool((f == 0).all())
    an = se.analyse(dark)
    assert bool((an["sigma"] == 0).all()) and bool((an["gamma"] == 0).all()) and bool((an["motion"] == 0).all())
    assert bool((an["phi"] == torch.tensor([0.0, 0.0, 1.0], device="cuda")).all())


def test_hip_sequences_and_members_are_independent_and_runs_repeat():
    c = S.case("24x16-ar2")
    ctx, motion, nz = cuda(c)
    se = engine(c)
    R, f = se.evolve(ctx, nz, motion), se.forecast(ctx, noise=nz, motion=motion)
    assert c.M == 3 and c.B == 2 and not torch.equal(f[0], f[1]) and not torch.equal(f[0], f[2])
    for b in range(c.B):                                                           # a sequence alone
        one = dict(noise=nz[:, b:b + 1].contiguous(), motion=motion[b:b + 1].contiguous())
        assert torch.equal(se.forecast(ctx[b:b + 1].contiguous(), **one), f[:, b:b + 1])
    for m in (0, c.M - 1):                                                         # a member alone; the last is the odd one out
        alone = nz[m:m + 1].contiguous()
        assert torch.equal(se.evolve(ctx, alone, motion), R[m:m + 1]) and torch.equal(se.forecast(ctx, noise=alone, motion=motion), f[m:m + 1])
    assert torch.equal(se.evolve(ctx, nz, motion), R) and torch.equal(se.forecast(ctx, noise=nz, motion=motion), f)
    assert torch.equal(engine(c).forecast(ctx, noise=nz, motion=motion), f)
    # a shorter horizon is a prefix; the estimated motion is LagrangianPersistence's
    assert torch.equal(se.forecast(ctx, noise=nz[:, :, :2].contiguous(), motion=motion), f[:, :, :2])
    assert torch.equal(se.forecast(ctx, noise=nz), se.forecast(ctx, noise=nz, motion=se.motion.motion(ctx)))
    # one workspace serves every member count up to the largest seen at the shape: nothing is reallocated under a captured graph
    held = se._ws[str(ctx.device)][2]
    se.analyse(ctx, motion), se.forecast(ctx, motion=motion), se.forecast(ctx, noise=nz[:2].contiguous(), motion=motion)
    assert se._ws[str(ctx.device)][2] is held and torch.equal(se.forecast(ctx, noise=nz, motion=motion), f)
    g = torch.Generator(device="cuda").manual_seed(3)
    drawn = se.forecast(ctx, members=3, generator=g, motion=motion)
    g.manual_seed(3)
    assert torch.equal(drawn, se.forecast(ctx, noise=torch.randn((3, c.B, c.K, c.H, c.W), device="cuda", generator=g), motion=motion))


def test_hip_forecast_replays_from_a_graph():
    c = S.case("32x64-ar2")
    ctx, motion, nz = cuda(c)
    other = (ctx.flip(0).contiguous(), motion.flip(0).contiguous(), nz.flip(0).contiguous())
    se = engine(c)
    eager = [se.forecast(x, noise=n, motion=v) for x, v, n in ((ctx, motion, nz), other)]      # the first call allocates the workspace
    assert not torch.equal(eager[0], eager[1])
    static = [t.clone() for t in (ctx, motion, nz)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = se.forecast(static[0], noise=static[2], motion=static[1])
    for src, ref in ((other, eager[1]), ((ctx, motion, nz), eager[0])):
        for dst, t in zip(static, src):
            dst.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def test_hip_workspace_too_small_is_refused_and_nothing_is_written():
    c = S.case("16x16-ar1")
    ctx, motion, nz = cuda(c)
    w = steps_bands(c.H, c.W, c.L).cuda()
    need0, need = L.steps_ws_bytes(c.B, 0, c.H, c.W, c.L, c.ar), L.steps_ws_bytes(c.B, c.M, c.H, c.W, c.L, c.ar)
    assert 0 < need0 < need
    par = [Guarded(s) for s in ((c.B, c.L), (c.B, c.L), (c.B, c.L, 3), (c.B, c.L, 2))]
    small = Guarded((need0,))
    short = small.t.view(torch.uint8)[:need0 - 1]                                  # one byte too small
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*workspace"):
        L.steps_analyse(ctx, motion, w, c.B, ctx.shape[1], c.H, c.W, c.L, c.ar, c.thr, *(g.t for g in par), short)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g.buf).all()) for g in par) and bool(torch.isnan(small.buf).all())
    ws, R = Guarded((need // 4,)), Guarded((c.M, c.B, c.K, c.H, c.W))
    L.steps_analyse(ctx, motion, w, c.B, ctx.shape[1], c.H, c.W, c.L, c.ar, c.thr, *(g.t for g in par), ws.t)
    torch.cuda.synchronize()
    before = ws.buf.clone()
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*workspace"):
        L.steps_evolve(nz, w, par[0].t, par[1].t, par[2].t, c.M, c.B, c.K, c.H, c.W, c.L, c.ar, R.t, ws.t.view(torch.uint8)[:need - 1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(R.buf).all()) and torch.equal(ws.buf.view(torch.int32), before.view(torch.int32))


def test_hip_calls_refuse_bad_fields():
    c = S.case("16x16-ar1")
    ctx, motion, nz = cuda(c)
    se = engine(c)
    for kw, msg in ((dict(motion=motion[:, :1].contiguous()), r"motion must be \(2, 2, 16, 16\)"), (dict(motion=motion.double()), "motion must be a float32"),
                    (dict(motion=motion.cpu()), "no CPU path"), (dict(motion=motion.transpose(2, 3)), "motion must be contiguous"),
                    (dict(noise=nz[:, :1].contiguous()), r"noise must be \(3, 2, 3, 16, 16\)"), (dict(noise=nz[0]), r"noise must be \(M, B, K, H, W\)"),
                    (dict(noise=nz, out_len=2), r"noise must be \(3, 2, 2, 16, 16\)"), (dict(noise=nz.cpu()), "no CPU path")):
        with pytest.raises(ValueError, match=msg):
            se.forecast(ctx, **kw)
    # the library refuses an output that is one of its inputs
    w = steps_bands(c.H, c.W, c.L).cuda()
    par = [torch.empty(s, device="cuda") for s in ((c.B, c.L), (c.B, c.L), (c.B, c.L, 3))]
    ws = torch.empty(L.steps_ws_bytes(c.B, c.M, c.H, c.W, c.L, c.ar) // 4, device="cuda")
    with pytest.raises(L.PrediffHipError, match=r"status -1\).*R aliases an input"):
        L.steps_evolve(nz, w, *par, c.M, c.B, c.K, c.H, c.W, c.L, c.ar, nz, ws)


# ------------------------------------------------------------------------------------------------ through the package
def test_hip_forecast_through_the_scores():
    H = W = 32
    ctx_np, tgt_np = X.blobs(2, 4, 3, H, W, ((0.75, -0.5), (-0.5, 0.625)), seed=21, nblob=3, sigma=(4.0, 6.0))
    ctx, tgt = torch.from_numpy(ctx_np.copy()).cuda(), torch.from_numpy(tgt_np.copy()).cuda()
    se = StochasticExtrapolation(out_len=3, levels=3)
    ens = se.forecast(ctx, members=3, generator=torch.Generator(device="cuda").manual_seed(1))
    assert ens.shape == (3,) + tuple(tgt.shape)
    score = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=3, threshold_list=(16, 74))
    score.update(ens, tgt)
    res = score.compute()
    for k in ("crps", "crps_fair", "rmse", "spread"):
        assert res[k].shape == (3,) and np.isfinite(res[k]).all(), k
    assert np.isfinite(res[16]["brier"]).all() and np.isfinite(res["avg"]["brier"]).all()
    assert (res["crps_fair"] <= res["crps"]).all() and (res["spread"] > 0).all()
    frame = SEVIRFrameScore(mode="1", seq_len=3, metrics_list=("mse", "mae"), data_range=1.0)
    frame.update_members(ens, tgt)
    assert all(np.isfinite(v).all() for v in frame.compute().values())
    # S-PROG: one member, CRPS is the MAE (the ensemble score works on the 0 .. 255 scale: values divided by fp32(1 / 255))
    one = se.forecast(ctx)
    assert one.shape == (1,) + tuple(tgt.shape)
    s1 = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=3, threshold_list=(16,), metrics_list=("crps", "rmse"))
    s1.update(one, tgt)
    f1 = SEVIRFrameScore(mode="1", seq_len=3, metrics_list=("mae",), data_range=1.0)
    f1.update_members(one, tgt)
    mae = f1.compute()["mae"]
    assert (mae > 0).all() and np.allclose(s1.compute()["crps"], mae / float(np.float32(1 / 255)), rtol=1e-6, atol=0)
