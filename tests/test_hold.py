"""Held-region (inpainting) sampling on the device ("Held regions"): the held step kernels and pd_hold_blend against fp64
and, bit for bit, against the un-held kernels; the held loops in every driver mode against the fp64 restatement of tests/_hold_ref.py
driven by the CPU oracle denoiser; the mixture property on the kernels; and the front ends (rollout overlap="hold", hold_from_frames,
sample_ensemble, the tiled canvas).

The loops run on the tiny architecture of test_dpmpp_2m.py::_tiny_ldm with FOUR target frames (that model has two, which cannot hold
"two frames and a patch of a third"); the guided case needs the tiny alignment network, which is built for two target frames, and runs on
_tiny_ldm itself with the first frame and a patch of the second held."""
import functools
import math

import numpy as np
import pytest
import torch

import _dpmpp_ref as R
import _hold_ref as H
import _templates as TP
from _cases import TINY_UNET_CFGS, TINY_VAE_CFG
from _weights import seeded_input, seeded_state_dict
from oracle import diffusion as OD
from oracle import unet as OU
from oracle import vae as OV
from test_dpmpp_2m import DDIM10_BOUND, GUIDED_DDIM10_BOUND, STEP_KERNEL_BOUND, _ac_linear, _factor, _tiny_ldm, rel_l2

pytestmark = pytest.mark.gpu

T = 1000
CFG4 = dict(TINY_UNET_CFGS["axial"], target_shape=[4, 8, 8, 4])            # T_in = 3, T_out = 4, window 8 x 8, C = 4
VAE_TOL = {"fp32": 1e-4}                                                    # tests/test_hip_vae.py


# ------------------------------------------------------------------------------------------------ 5. the kernels
def _rows(sampler, B):
    """One coefficient row per sample, as the kernels get them: sample 0 first-order and stochastic with a hold at an inner level,
    sample 1 second-order with the LAST step's hold (1, 0), sample 2 second-order, no step noise."""
    base = {"ddim": [[0.05, 0.20, 0.30], [0.60, 0.80, 0.0], [0.97, 0.99, 0.05]],
            "dpmpp_2m": [[0.05, 0.90, 0.40, 0.0], [0.60, 0.80, 0.30, 1.9], [0.97, 0.50, 0.60, 0.5]],
            "dpmpp_2m_sde": [[0.05, 0.90, 0.40, 0.0, 0.7], [0.60, 0.80, 0.30, 1.9, 0.2], [0.97, 0.50, 0.60, 0.5, 0.0]]}[sampler]
    tail = [[2.5, 0.8, 0.6], [0.01, 1.0, 0.0], [0.3, 0.3, math.sqrt(1 - 0.09)]]      # gamma, k_x, k_n
    return torch.tensor([b + t for b, t in zip(base, tail)][:B], dtype=torch.float32)


def _f64_held(sampler, rows, zt, eps, noise, hist, shift, x0, m, hn):
    """(out, hist') in fp64 from the rows as the kernel gets them; NaNs behind a closed select do not enter."""
    c = rows.double()[:, :, None]
    z, e = zt.double(), eps.double()
    a = c[:, 0]
    z0 = (z - (1 - a).sqrt() * e) / a.sqrt()
    if sampler == "ddim":
        v = c[:, 1].sqrt() * z0 + (1 - c[:, 1] - c[:, 2] ** 2).clamp_min(0).sqrt() * e + c[:, 2] * noise.double()
        g = 3
    else:
        w = c[:, 3]
        D = torch.where(w != 0, z0 + w * (z0 - hist.double()), z0)
        v = c[:, 1] * z + c[:, 2] * D
        g = 4
        if sampler == "dpmpp_2m_sde":
            v = v + torch.where(c[:, 4] != 0, c[:, 4] * noise.double(), torch.zeros_like(v))
            g = 5
    if shift is not None:
        v = v - c[:, g] * shift.double()
    k_x, k_n = c[:, g + 1], c[:, g + 2]
    held = k_x * x0.double() + torch.where(k_n != 0, k_n * hn.double(), torch.zeros_like(v))
    md = m.double()
    mix = md * torch.where(md != 0, held, torch.zeros_like(held)) + (1 - md) * torch.where(md != 1, v, torch.zeros_like(v))
    return mix, z0


def _call(L, sampler, held, guided, rows, zt, eps, noise, hist, shift, x0, m, hn):
    """One launch of the (held or un-held, guided or not) kernel of `sampler`; returns (out, hist afterwards)."""
    B, per = zt.shape
    out, h = torch.empty_like(zt), hist.clone()
    g = {"ddim": 3, "dpmpp_2m": 4, "dpmpp_2m_sde": 5}[sampler]
    sh = shift if guided else None
    if held:
        r = rows.cuda().contiguous()
        if sampler == "ddim":
            L.ddim_step_held(zt, eps, noise, sh, x0, m, hn, r, out, B, per)
        elif sampler == "dpmpp_2m":
            L.dpmpp_2m_step_held(zt, eps, h, sh, x0, m, hn, r, out, B, per)
        else:
            L.dpmpp_2m_sde_step_held(zt, eps, noise, h, sh, x0, m, hn, r, out, B, per)
        return out, h
    r = rows[:, :g + 1 if guided else g].cuda().contiguous()
    if sampler == "ddim":
        L.ddim_step_guided(zt, eps, noise, sh, r, out, B, per) if guided else L.ddim_step(zt, eps, noise, r, out, B, per)
    elif sampler == "dpmpp_2m":
        L.dpmpp_2m_step_guided(zt, eps, h, sh, r, out, B, per) if guided else L.dpmpp_2m_step(zt, eps, h, r, out, B, per)
    elif guided:
        L.dpmpp_2m_sde_step_guided(zt, eps, noise, h, sh, r, out, B, per)
    else:
        L.dpmpp_2m_sde_step(zt, eps, noise, h, r, out, B, per)
    return out, h


@pytest.mark.parametrize("B,per", [(3, 96), (3, 1000), (2, 98304)])
def test_held_step_kernels(B, per):
    from prediff_amd import _lib as L
    g = torch.Generator().manual_seed(41 + per)
    zt, eps, noise, hist, shift, x0, hn = (torch.randn(B, per, generator=g).cuda() for _ in range(7))
    m = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (B, per), generator=g)].cuda()     # 0, 1 and 0.25 mixed within a sample
    hn[1] = float("nan")                              # sample 1 has k_n = 0: its hold noise is never read
    nan = torch.full_like(zt, float("nan"))
    for sampler in ("ddim", "dpmpp_2m", "dpmpp_2m_sde"):
        rows = _rows(sampler, B)
        hist_in = hist.clone()
        if sampler != "ddim":
            hist_in[0] = float("nan")                 # sample 0 has w = 0: the history is not read there
        for guided in (False, True):
            tag = f"{sampler}{' guided' if guided else ''} ({B}, {per})"
            ops = (zt, eps, noise, hist_in, shift, x0, m, hn)
            out, h = _call(L, sampler, True, guided, rows, *ops)
            ref, ref_h = _f64_held(sampler, rows.cpu(), *(None if (o is shift and not guided) else o.cpu() for o in ops))
            e = rel_l2(out, ref)
            print(f"[held step {tag}] rel-L2 vs fp64 {e:.2e}")
            assert bool(torch.isfinite(out).all()) and e <= STEP_KERNEL_BOUND, tag
            plain, plain_h = _call(L, sampler, False, guided, rows, *ops)
            assert torch.equal(out[m == 0], plain[m == 0]), tag                      # m = 0: the un-held kernel's bits
            assert torch.equal(out[1][m[1] == 1], x0[1][m[1] == 1]), tag             # m = 1 at (k_x, k_n) = (1, 0): x0's bits
            if sampler != "ddim":
                assert torch.equal(h, plain_h) and bool(torch.isfinite(h).all()) and rel_l2(h, ref_h) <= STEP_KERNEL_BOUND, tag
            # NaN behind m = 0 (x0, hold noise) and behind m = 1 (the step's own result, through eps): not in the output
            out2, _ = _call(L, sampler, True, guided, rows, zt, eps, noise, hist_in, shift, torch.where(m == 0, nan, x0), m,
                            torch.where(m == 0, nan, hn))
            assert torch.equal(out2, out), tag
            out3, _ = _call(L, sampler, True, guided, rows, zt, torch.where(m == 1, nan, eps), noise, hist_in, shift, x0, m, hn)
            assert torch.equal(out3, out), tag
    with pytest.raises(L.PrediffHipError):
        L.ddim_step_held(zt, eps, noise, None, x0, m[:1], hn, _rows("ddim", B).cuda(), torch.empty_like(zt), B, per)
    with pytest.raises(L.PrediffHipError):
        L.dpmpp_2m_step_held(zt, eps, hist, None, x0, m, hn, _rows("dpmpp_2m", B).cuda()[:, :6].contiguous(), torch.empty_like(zt), B, per)
    # the start rule, out of place and in place (noise = z: the starting latent is the noise of the held part)
    coef2 = _rows("ddim", B)[:, 4:6].contiguous()
    held = coef2[:, :1].double() * x0.cpu().double() + torch.where(coef2[:, 1:2] != 0, coef2[:, 1:2].double() * zt.cpu().double(), torch.zeros(1).double())
    md = m.cpu().double()
    ref = md * held + (1 - md) * zt.cpu().double()
    out = torch.empty_like(zt)
    L.hold_blend(zt, x0, m, zt, coef2.cuda(), out, B, per)
    e = rel_l2(out, ref)
    print(f"[pd_hold_blend ({B}, {per})] rel-L2 vs fp64 {e:.2e}")
    assert e <= STEP_KERNEL_BOUND and torch.equal(out[m == 0], zt[m == 0]) and torch.equal(out[1][m[1] == 1], x0[1][m[1] == 1])
    z2 = zt.clone()
    L.hold_blend(z2, x0, m, z2, coef2.cuda(), z2, B, per)
    assert torch.equal(z2, out)


# ------------------------------------------------------------------------------------------------ 6. the loops
@functools.lru_cache(maxsize=None)
def _sd4():
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    return seeded_state_dict(CuboidTransformerUNet(**CFG4, precision="fp32").state_dict(), 600)


def _ldm4(precision="fp32", **kw):
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.latent_diffusion import LatentDiffusion
    net = CuboidTransformerUNet(**CFG4, precision=precision)
    net.load_state_dict(_sd4())
    ldm_kw = dict(layout="NTHWC", data_shape=(4, 32, 32, 1), timesteps=T, use_ema=False, latent_shape=tuple(CFG4["target_shape"]),
                  first_stage_model=None, cond_stage_model=None)
    return LatentDiffusion(torch_nn_module=net, **dict(ldm_kw, **kw)).cuda().eval()


def _hold4(B, seed=7):
    """The first two target frames and a spatial patch of the third held (frame four is free); the known latent at unit scale."""
    M = torch.zeros(1, 4, 8, 8, 1)
    M[:, :2] = 1.0
    M[:, 2, 2:6, 3:7] = 1.0
    X = torch.randn((B, 4, 8, 8, 4), generator=torch.Generator().manual_seed(seed))
    return M, X


LOOPS = {"ddim eta 0": dict(sampler="ddim", ddim_steps=10, eta=0.0), "ddim eta 1": dict(sampler="ddim", ddim_steps=10, eta=1.0),
         "2m": dict(sampler="dpmpp_2m", steps=10), "2m-sde": dict(sampler="dpmpp_2m_sde", steps=10, eta=1.0)}


def _restated(kw, denoiser, zc, tape, M, X, hold_noise, **more):
    return H.held_loop(_ac_linear(), denoiser, zc, tape, 10, kw["sampler"], M, X, hold_noise=hold_noise, eta=kw.get("eta", 0.0), **more)


@pytest.mark.parametrize("name", list(LOOPS))
def test_held_loops_vs_restatement(name):
    """sample(hold_mask, hold_x0) for 10 steps, fp32, on a shared tape, against the restatement loop driven by the CPU oracle denoiser.
    Bound: the un-held test's of the same sampler (DDIM10_BOUND, times the grid's factor for the 2M loops)."""
    B, kw = 2, LOOPS[name]
    ldm, sd = _ldm4(), _sd4()
    zc = seeded_input("hold.zc", (B,) + tuple(CFG4["input_shape"]), 5)
    shape = ldm.get_batch_latent_shape(B)
    g = torch.Generator().manual_seed(3)
    tape = [torch.randn(shape, generator=g) for _ in range(1 + 2 * 10)]
    M, X = _hold4(B)
    bound = DDIM10_BOUND["fp32"] * (1.0 if kw["sampler"] == "ddim" else _factor(10, "quad"))
    Mb = M.expand(shape).bool()
    for hold_noise in ("fresh", "fixed"):
        ref = _restated(kw, lambda z, t, c: OU.unet_forward(sd, CFG4, z, t, c), zc, tape, M, X, hold_noise)
        out = ldm.sample(cond=zc.cuda(), batch_size=B, return_decoded=False, noise_tape=[t.cuda() for t in tape], hold_mask=M.cuda(),
                         hold_x0=X.cuda(), hold_noise=hold_noise, **kw)
        e, ef = rel_l2(out, ref), rel_l2(out.cpu()[~Mb], ref[~Mb])
        print(f"[held {name} {hold_noise}] rel-L2 vs the restatement loop {e:.3e} (free part alone {ef:.3e}; bound {bound:.2e})")
        assert torch.equal(out.cpu()[Mb], X[Mb])                                # the held part is hold_x0 bit for bit
        assert e < bound and ef < bound, hold_noise


def test_guided_held_ddim_vs_restatement():
    from test_alignment import _tiny_alignment
    ldm, cfg, sd = _tiny_ldm("fp32")
    B, n = 2, 10
    zc = seeded_input("hold.gzc", (B,) + tuple(cfg["input_shape"]), 21)
    shape = ldm.get_batch_latent_shape(B)
    g = torch.Generator().manual_seed(22)
    tape = [torch.randn(shape, generator=g) for _ in range(1 + 2 * n)]
    M = torch.zeros(1, 2, 8, 8, 1)
    M[:, 0] = 1.0
    M[:, 1, 2:6, 3:7] = 1.0
    X = torch.randn(shape, generator=g)
    al_cpu, al = _tiny_alignment(), _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    avg = torch.tensor([[0.4], [0.1]])
    lv = OD.schedule_buffers(OD.beta_schedule("linear", T))["posterior_log_variance_clipped"]
    kw = dict(sampler="ddim", ddim_steps=n, eta=0.0)
    ref = _restated(kw, lambda z, t, c: OU.unet_forward(sd, cfg, z, t, c), zc, tape, M, X, "fresh",
                    align_fn=lambda z, t: al_cpu.get_mean_shift(z, t, avg_x_gt=avg), logvar_clipped=lv)
    skw = dict(cond=zc.cuda(), batch_size=B, return_decoded=False, noise_tape=[t.cuda() for t in tape], hold_mask=M.cuda(), hold_x0=X.cuda(), **kw)
    out = ldm.sample(use_alignment=True, alignment_kwargs={"avg_x_gt": avg.cuda()}, **skw)
    e, d = rel_l2(out, ref), rel_l2(out, ldm.sample(**skw))
    print(f"[guided held DDIM-{n}] rel-L2 vs the guided restatement loop {e:.3e} (bound {GUIDED_DDIM10_BOUND:.0e}); guided vs un-guided {d:.3e}")
    Mb = M.expand(shape).bool()
    assert torch.equal(out.cpu()[Mb], X[Mb])                                    # guidance never moves the held part
    assert e < GUIDED_DDIM10_BOUND and d > 1e-3


# ------------------------------------------------------------------------------------------------ 7. the driver's modes
@pytest.mark.parametrize("name", ["ddim eta 1", "2m"])
def test_modes_agree_with_a_hold(name):
    """Lanes, the single graph and the eager loop give the same bits with a hold, from the device generator ("fresh": the draws are
    made in the same order in every mode); replays refresh the hold buffers; the un-held graphs are untouched by held calls."""
    B, kw = 4, dict(LOOPS[name])
    kw.update({"ddim_steps" if kw["sampler"] == "ddim" else "steps": 5})
    ldm = _ldm4()
    zc = seeded_input("hold.zc4", (B,) + tuple(CFG4["input_shape"]), 5).cuda()
    shape = ldm.get_batch_latent_shape(B)
    M, X = (t.cuda() for t in _hold4(B))
    M2, X2 = M.flip(1).contiguous(), X.flip(0).contiguous()
    skw = dict(cond=zc, batch_size=B, return_decoded=False, **kw)

    def run(seed=9, **hold):
        torch.manual_seed(seed)
        return ldm.sample(**skw, **hold)
    outs, others = {}, {}
    for lanes in (1, 2):
        ldm.num_streams = lanes
        outs[lanes] = run(hold_mask=M, hold_x0=X)
        assert lanes == 1 or 1 in ldm._graphs
        others[lanes] = run(hold_mask=M2, hold_x0=X2)                           # another mask and x0 on the same graphs: its own result
        assert not torch.equal(others[lanes], outs[lanes])
        assert torch.equal(run(hold_mask=M, hold_x0=X), outs[lanes]), lanes
    unheld_after = run()                                                        # an un-held call after held ones
    ldm.use_hip_graph = False
    eager, eager_other = run(hold_mask=M, hold_x0=X), run(hold_mask=M2, hold_x0=X2)
    assert bool(torch.isfinite(eager).all())
    assert torch.equal(outs[1], eager) and torch.equal(outs[2], eager)
    assert torch.equal(others[1], eager_other) and torch.equal(others[2], eager_other)
    assert torch.equal(eager[M.expand(shape) == 1], X[M.expand(shape) == 1])
    ldm.use_hip_graph = True
    fresh_module = _ldm4()
    fresh_module.num_streams = 2
    torch.manual_seed(9)
    unheld = fresh_module.sample(**skw)
    assert torch.equal(unheld_after, unheld)
    # an all-zero mask with "fixed" is the un-held run; an all-ones mask returns hold_x0
    assert torch.equal(run(hold_mask=torch.zeros_like(M), hold_x0=X, hold_noise="fixed"), unheld)
    assert torch.equal(run(hold_mask=torch.ones(1, device="cuda"), hold_x0=X), X)


# ------------------------------------------------------------------------------------------------ 8. the mixture on the kernels
@pytest.mark.parametrize("schedule", ["linear", "sqrt_linear"])
def test_mixture_property_on_the_kernels(schedule):
    """test_hold_host.py::test_hold_pulls_the_free_part_onto_the_held_component in fp32 on the device, the held kernels called directly
    with the product's tables: every held proj > 0.5 (the fp64 runs sit above 0.7; the margin covers fp32)."""
    from prediff_amd import _lib as L
    from prediff_amd import schedule as S
    ac = np.cumprod(1.0 - OD.beta_schedule(schedule, T)).astype(np.float32)
    B, per = H.B_MIX, H.D_MIX
    for seed in (1, 2):
        means, M, X, x_T = H.mixture_problem(seed)
        mix = R.Mixture(torch, torch.tensor(means, dtype=torch.float32).cuda(), R.MIXTURE_STDS)
        m = torch.tensor(M, dtype=torch.float32).expand(B, per).contiguous().cuda()
        x0, xT = torch.tensor(X, dtype=torch.float32).cuda(), torch.tensor(x_T, dtype=torch.float32).cuda()
        g = torch.Generator(device="cuda").manual_seed(100 + seed)
        for sampler, eta, method in H.MIXTURE_SETTINGS:
            steps = np.minimum(S.make_ddim_timesteps(method, 10, T), T - 1)
            if sampler == "ddim":
                sig, a, a_prev = S.make_ddim_sampling_parameters(ac.astype(np.float64), steps, eta)
                table = np.stack([a, a_prev, sig], 1)[::-1]
                cols, start = S.make_hold_coefficients(ac.astype(np.float64), steps)
            else:
                table, visited = S.make_dpmpp_2m_coefficients(ac, steps)
                cols, start = S.make_hold_coefficients(ac.astype(np.float64), steps, visited)
            rows = torch.tensor(np.concatenate([table, np.zeros((len(table), 1)), cols], 1), dtype=torch.float32).cuda()
            z = torch.empty_like(xT)
            L.hold_blend(xT, x0, m, xT, torch.tensor(start).cuda().expand(B, 2).contiguous(), z, B, per)
            hist = torch.full_like(z, float("nan"))
            for k in range(len(rows)):
                e = mix.eps(z, float(rows[k, 0])).contiguous()
                noise, hn = (torch.randn(B, per, generator=g, device="cuda") for _ in range(2))
                out, r = torch.empty_like(z), rows[k].expand(B, rows.shape[1]).contiguous()
                if sampler == "ddim":
                    L.ddim_step_held(z, e, noise, None, x0, m, hn, r, out, B, per)
                else:
                    L.dpmpp_2m_step_held(z, e, hist, None, x0, m, hn, r, out, B, per)
                z = out
            p = H.proj(z.double().cpu().numpy(), means, M)
            print(f"[mixture on the kernels {schedule} seed {seed} {sampler} eta {eta} {method}] held proj min {p.min():.3f}")
            assert torch.equal(z[m == 1], x0[m == 1]) and (p > 0.5).all(), (seed, sampler, eta, method)


# ------------------------------------------------------------------------------------------------ 9. rolling forecasts
def test_rollout_overlap_hold():
    """overlap="hold" at stride = out_len // 2 over three segments: the hand chain of _sample_latent(hold_mask, hold_x0) calls and
    context_advance, bit for bit; every segment's held frames are the previous segment's; "discard" is the rollout as it was."""
    from prediff_amd import _lib as L
    from prediff_amd.rollout import rollout_ensemble, rollout_sample
    ldm = _ldm4(scale_factor=0.5)
    ldm.num_streams = 1
    B, out_len, s = 2, 4, 2
    horizon = 2 * s + out_len
    zc = seeded_input("hold.roll.zc", (B,) + tuple(CFG4["input_shape"]), 11).cuda()
    shape = ldm.get_batch_latent_shape(B)
    g = torch.Generator().manual_seed(12)
    tapes = [[torch.randn(shape, generator=g).cuda() for _ in range(1 + 2 * 4)] for _ in range(3)]
    skw = dict(sampler="ddim", ddim_steps=4, eta=1.0)
    mask = torch.zeros(1, out_len, 1, 1, 1, device="cuda")
    mask[:, :out_len - s] = 1.0

    def chain(hold):
        ctx, origins, segs = zc.contiguous().unsqueeze(1), torch.zeros((1, 2), dtype=torch.int32), []
        for j in range(3):
            kw = {}
            if hold and j:
                x0 = torch.zeros(shape, device="cuda")
                x0[:, :out_len - s] = segs[-1][:, s:]
                kw = dict(hold_mask=mask, hold_x0=x0)
            segs.append(ldm._sample_latent(ctx[:, 0].contiguous(), shape, None, noise_tape=tapes[j], **kw, **skw))
            nxt = torch.empty_like(ctx)
            L.context_advance(ctx, segs[-1].contiguous(), origins, nxt, s, 1.0 / 0.5)
            ctx = nxt
        return segs
    segs = chain(True)
    kw = dict(cond=zc, horizon=horizon, stride=s, batch_size=B, noise_tape=tapes, return_decoded=False, **skw)
    out = rollout_sample(ldm, overlap="hold", **kw)
    assert out.shape == (B, horizon) + shape[2:] and bool(torch.isfinite(out).all())
    assert torch.equal(out, torch.cat([segs[0][:, :s], segs[1][:, :s], segs[2]], dim=1))
    for j in (1, 2):                                                            # consecutive segments agree where they meet
        assert torch.equal(segs[j][:, :out_len - s], segs[j - 1][:, s:]), j
    free = chain(False)
    assert not torch.equal(free[1][:, :out_len - s], free[0][:, s:])
    discard = rollout_sample(ldm, overlap="discard", **kw)
    assert torch.equal(discard, rollout_sample(ldm, **kw)) and torch.equal(discard, torch.cat([free[0][:, :s], free[1][:, :s], free[2]], dim=1))
    # the ensemble front end passes `overlap` through and stays invariant to the batch split
    ekw = dict(stride=s, base_seed=1000, sampler="dpmpp_2m", steps=4, return_decoded=False, overlap="hold")
    a = rollout_ensemble(ldm, zc[:1], 4, horizon, **ekw)
    b = rollout_ensemble(ldm, zc[:1], 4, horizon, micro_batch=1, **ekw)
    c = rollout_ensemble(ldm, zc[:1], 4, horizon, micro_batch=2, **ekw)
    assert a.shape == (4, horizon) + shape[2:]
    assert rel_l2(b, a) < 1e-6 and rel_l2(c, a) < 1e-6 and rel_l2(a[0], a[1]) > 1e-2


# ------------------------------------------------------------------------------------------------ 10. pixel frames, ensembles
def test_hold_from_frames_and_ensemble():
    from prediff_amd.autoencoder_kl import AutoencoderKL
    from prediff_amd.ensemble import sample_ensemble
    vsd = seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 510)
    vae = AutoencoderKL(**TINY_VAE_CFG, precision="fp32")
    vae.load_state_dict(vsd, strict=True)
    ldm = _ldm4(first_stage_model=vae, scale_factor=0.5)
    frames = seeded_input("hold.frames", (1, 2, 32, 32, 1), 1, kind="uniform")
    mask, x0 = ldm.hold_from_frames(frames.cuda(), first=1)
    assert mask.shape == (1, 4, 1, 1, 1) and mask.flatten().tolist() == [0.0, 1.0, 1.0, 0.0] and x0.shape == (1, 4, 8, 8, 4)
    ref = 0.5 * OV.vae_encode_mode(vsd, TINY_VAE_CFG, frames[0].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    e = rel_l2(x0[0, 1:3], ref)
    print(f"[hold_from_frames] rel-L2 vs scale_factor x the oracle encoder's mode {e:.3e}")
    assert e < VAE_TOL["fp32"] and not x0[:, 0].any() and not x0[:, 3].any()
    zc = seeded_input("hold.ens.zc", (1,) + tuple(CFG4["input_shape"]), 5).cuda()
    kw = dict(base_seed=1000, sampler="ddim", ddim_steps=4, eta=1.0, return_decoded=False, hold_mask=mask, hold_x0=x0)
    a = sample_ensemble(ldm, zc, 4, **kw)
    for k in range(4):                                                          # a batch-1 hold: every member holds the same frames
        assert torch.equal(a[k, 1:3], x0[0, 1:3]), k
    assert rel_l2(a[0, 0], a[1, 0]) > 1e-2                                      # ... and is free elsewhere
    b = sample_ensemble(ldm, zc, 4, micro_batch=2, **kw)
    assert rel_l2(b, a) < 1e-6


# ------------------------------------------------------------------------------------------------ 11. the tiled canvas
def test_tiled_canvas_hold():
    """The step runs on the canvas, so a canvas-shaped hold passes straight through: the held part is exact, and an all-zero mask with
    "fixed" is the un-held canvas run bit for bit."""
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.tiled import TiledLatentDiffusion
    cfg = TINY_UNET_CFGS["axial"]
    net = CuboidTransformerUNet(**cfg, precision="bf16")
    net.load_state_dict(seeded_state_dict(TP.unet_template(cfg, "tiny_unet_schema.json", "axial"), 600))
    canvas = (12, 13)
    ldm = TiledLatentDiffusion(net, canvas=canvas, stride=(4, 4), layout="NTHWC", data_shape=(2, 32, 32, 1), timesteps=T, use_ema=False,
                               latent_shape=tuple(cfg["target_shape"]), first_stage_model=None, cond_stage_model=None).cuda().eval()
    B = 2
    zc = seeded_input("hold.tiled.zc", (B, 3) + canvas + (4,), 3).cuda()
    x_T = seeded_input("hold.tiled.xT", (B, 2) + canvas + (4,), 4).cuda()
    M = torch.zeros((1, 2) + canvas + (1,), device="cuda")
    M[:, 0] = 1.0
    M[:, 1, 3:9, 2:11] = 1.0                                                    # a patch across window borders
    X = seeded_input("hold.tiled.x0", (B, 2) + canvas + (4,), 6).cuda()
    kw = dict(cond=zc, batch_size=B, return_decoded=False, sampler="dpmpp_2m", steps=4, x_T=x_T)
    torch.manual_seed(2)
    out = ldm.sample(hold_mask=M, hold_x0=X, **kw)
    Mb = M.expand(out.shape) == 1
    assert bool(torch.isfinite(out).all()) and torch.equal(out[Mb], X[Mb])
    unheld = ldm.sample(**kw)
    assert not torch.equal(out[~Mb], unheld[~Mb])
    assert torch.equal(ldm.sample(hold_mask=torch.zeros_like(M), hold_x0=X, hold_noise="fixed", **kw), unheld)
