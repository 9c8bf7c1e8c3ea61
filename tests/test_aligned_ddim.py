"""Knowledge-aligned DDIM: the guidance coefficients, the guided step kernel, the guided DDIM loop against an oracle
loop built from oracle.diffusion + oracle.unet + the guidance network's PyTorch CPU path, and the wiring of the front end."""
import numpy as np
import pytest
import torch

import _templates as TP
from _cases import TINY_UNET_CFGS, TINY_VAE_CFG, V1_ALIGN_ARGS, V1_LDM_KW, V1_UNET_CFG
from _weights import seeded_input, seeded_state_dict
from oracle import diffusion as OD
from oracle import unet as OU
from prediff_amd.schedule import make_ddim_guidance_coefficients

T = 1000


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _buffers():
    return OD.schedule_buffers(OD.beta_schedule("linear", T))


def _grid(n, method="uniform"):
    return np.minimum(OD.ddim_timesteps(n, T, method), T - 1)


def _gamma_f64(logvar_clipped, steps):
    """The rule restated: gamma_idx = sum over J_idx of exp(0.5 logvar_clipped[j]), J_idx = {steps[idx-1]+1 .. steps[idx]}
    ({0 .. steps[0]} for idx = 0)."""
    lv = np.asarray(logvar_clipped, dtype=np.float32).astype(np.float64)
    out, J = [], []
    for idx, t in enumerate(steps):
        lo = 0 if idx == 0 else int(steps[idx - 1]) + 1
        js = list(range(lo, int(t) + 1))
        J.append(js)
        out.append(sum(np.exp(0.5 * lv[j]) for j in js))
    return np.asarray(out), J


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("method,n", [("uniform", 10), ("uniform", 50), ("quad", 10), ("quad", 50)])
def test_guidance_coefficients(method, n):
    lv = _buffers()["posterior_log_variance_clipped"]
    steps = _grid(n, method)
    got = make_ddim_guidance_coefficients(lv, steps)
    ref, J = _gamma_f64(lv, steps)
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.array_equal(got, ref.astype(np.float32))
    # the J sets partition {0, ..., steps[-1]}: every DDPM timestep the chain covers is counted exactly once
    flat = [j for js in J for j in js]
    assert flat == list(range(int(steps[-1]) + 1))
    if method == "quad" and n == 50:
        assert steps[0] == steps[1] == 1 and J[1] == [] and got[1] == 0.0     # a repeated grid point: empty J, gamma 0
    for idx, js in enumerate(J):
        if len(js) == 1:                       # one timestep: exactly the reference's aligned ancestral shift coefficient
            assert got[idx] == np.float32(np.exp(0.5 * np.float64(lv[js[0]])))
    # the T-1 clamp repeats the last grid point at ddim_steps = T
    full = _grid(T)
    assert full[-1] == full[-2] == T - 1 and make_ddim_guidance_coefficients(lv, full)[-1] == 0.0


def test_sample_ensemble_ddim_forwards_alignment():
    """sampler="ddim" used to drop use_alignment and return un-guided members without an error."""
    from prediff_amd.ensemble import sample_ensemble

    class Stub:
        latent_shape = (2, 4, 4, 1)

        def __init__(self):
            self.calls = []

        def sample(self, cond, **kw):
            self.calls.append(kw)
            return torch.zeros((kw["batch_size"],) + self.latent_shape)

    ldm = Stub()
    y = torch.rand(1, 3, 4, 4, 1)
    avg = torch.tensor([[0.25]])
    out = sample_ensemble(ldm, {"y": y}, 3, sampler="ddim", ddim_steps=7, eta=0.5, use_alignment=True,
                          alignment_kwargs={"avg_x_gt": avg, "other": 1.5}, return_decoded=False)
    assert out.shape == (3, 2, 4, 4, 1) and len(ldm.calls) == 1
    kw = ldm.calls[0]
    assert kw["sampler"] == "ddim" and kw["ddim_steps"] == 7 and kw["eta"] == 0.5 and kw["batch_size"] == 3
    assert kw["use_alignment"] is True
    assert kw["alignment_kwargs"]["avg_x_gt"].shape == (3, 1) and torch.equal(kw["alignment_kwargs"]["avg_x_gt"], avg.expand(3, 1))
    assert kw["alignment_kwargs"]["other"] == 1.5
    # micro-batches: each call gets its own members' expansion
    ldm.calls.clear()
    sample_ensemble(ldm, {"y": y}, 3, sampler="ddim", micro_batch=2, use_alignment=True, alignment_kwargs={"avg_x_gt": avg},
                    return_decoded=False)
    assert [c["alignment_kwargs"]["avg_x_gt"].shape[0] for c in ldm.calls] == [2, 1]
    assert all(c["use_alignment"] for c in ldm.calls)


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def _f64_guided_step(zt, eps, noise, shift, coef4):
    c = coef4.double().reshape(-1, 4, *([1] * (zt.dim() - 1)))
    a, ap, sig, gam = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    z, e, s = zt.double(), eps.double(), shift.double()
    x0 = (z - (1 - a).sqrt() * e) / a.sqrt()
    out = ap.sqrt() * x0 + (1 - ap - sig ** 2).clamp_min(0).sqrt() * e - gam * s
    return out + sig * noise.double() if noise is not None else out


@pytest.mark.gpu
def test_guided_step_kernel():
    from prediff_amd import _lib as L
    B, per = 3, 1000                          # per_sample not a multiple of 256: the tail of the grid-stride loop
    g = torch.Generator().manual_seed(11)
    zt, eps, noise, shift = (torch.randn(B, per, generator=g).cuda() for _ in range(4))
    coef4 = torch.tensor([[0.05, 0.30, 0.40, 2.50], [0.60, 0.70, 0.00, 0.01], [0.97, 0.99, 0.05, 0.30]], dtype=torch.float32).cuda()
    for nz in (noise, None):
        out = torch.empty_like(zt)
        L.ddim_step_guided(zt, eps, nz, shift, coef4, out, B, per)
        ref = _f64_guided_step(zt.cpu(), eps.cpu(), None if nz is None else nz.cpu(), shift.cpu(), coef4.cpu())
        assert rel_l2(out, ref) <= 1e-6, nz is None
        # a zero shift is the un-guided step bit for bit
        out0, ung = torch.empty_like(zt), torch.empty_like(zt)
        L.ddim_step_guided(zt, eps, nz, torch.zeros_like(zt), coef4, out0, B, per)
        L.ddim_step(zt, eps, nz, coef4[:, :3].contiguous(), ung, B, per)
        assert torch.equal(out0, ung), nz is None


@pytest.mark.gpu
def test_guided_step_is_the_aligned_ddpm_step():
    """One DDIM step over one timestep with sigma = sqrt(posterior variance) and gamma = the same is the reference's aligned ancestral
    step: pd_ddim_step_guided with (a_t, a_{t-1}, sqrt(var~_t), sqrt(var~_t)) against pd_ddpm_step(mean_shift=g)."""
    from prediff_amd import _lib as L
    buf = _buffers()
    coef5 = torch.tensor(np.stack([buf[k] for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                                     "posterior_mean_coef2", "posterior_log_variance_clipped")])).cuda()
    ts = [999, 500, 1]
    B, per = len(ts), 1000
    g = torch.Generator().manual_seed(12)
    zt, eps, noise, shift = (torch.randn(B, per, generator=g).cuda() for _ in range(4))
    sd = [float(np.exp(0.5 * np.float64(buf["posterior_log_variance_clipped"][t]))) for t in ts]
    coef4 = torch.tensor([[buf["alphas_cumprod"][t], buf["alphas_cumprod_prev"][t], s, s] for t, s in zip(ts, sd)],
                         dtype=torch.float32).cuda()
    ddim, ddpm = torch.empty_like(zt), torch.empty_like(zt)
    L.ddim_step_guided(zt, eps, noise, shift, coef4, ddim, B, per)
    L.ddpm_step(zt, eps, noise, shift, torch.tensor(ts, dtype=torch.int64).cuda(), coef5, T, ddpm, B, per)
    for b, t in enumerate(ts):
        e = rel_l2(ddim[b], ddpm[b])
        print(f"[guided DDIM step vs aligned DDPM step] t={t}: rel-L2 {e:.2e}")
        assert e <= 1e-5, t


# ------------------------------------------------------------------------------------------------ GPU: the loop
def _oracle_guided_ddim(sd, cfg, zc, tape, n, eta, align_fn):
    """oracle.diffusion's DDIM loop with the guidance rule: z_prev = ddim_step(...) - gamma_idx * g(z_t, steps[idx])."""
    buf = _buffers()
    ac = buf["alphas_cumprod"]
    steps = _grid(n)
    sig, a, a_prev = OD.ddim_sampling_parameters(ac.astype(np.float64), steps, eta)
    gamma, _ = _gamma_f64(buf["posterior_log_variance_clipped"], steps)
    z = tape[0]
    B = z.shape[0]
    f = lambda v: torch.full((B,), float(v), dtype=torch.float32)
    for k, idx in enumerate(reversed(range(len(steps)))):
        t = torch.full((B,), int(steps[idx]), dtype=torch.long)
        with torch.no_grad():
            eps = OU.unet_forward(sd, cfg, z, t, zc)
        shift = align_fn(z, t).detach()
        z = OD.ddim_step(z, eps, f(a[idx]), f(a_prev[idx]), f(sig[idx]), tape[1 + k]) - float(np.float32(gamma[idx])) * shift
    return z


def _tiny_alignment():
    from test_alignment import _tiny_alignment as make          # the tiny guidance network pinned against the reference golden
    return make()


def _tiny_ldm(vae=None):
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.latent_diffusion import LatentDiffusion
    cfg = TINY_UNET_CFGS["axial"]
    sd = seeded_state_dict(TP.unet_template(cfg, "tiny_unet_schema.json", "axial"), 600)
    net = CuboidTransformerUNet(**cfg, precision="fp32")
    net.load_state_dict(sd)
    T_out, H, W, C = cfg["target_shape"]
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(T_out, H * 4, W * 4, 1), timesteps=T, use_ema=False,
                          latent_shape=tuple(cfg["target_shape"]), first_stage_model=vae,
                          cond_stage_model=("__is_first_stage__" if vae is not None else None))
    return ldm.cuda().eval(), cfg, sd


@pytest.mark.gpu
def test_tiny_guided_ddim_vs_oracle_and_paths():
    ldm, cfg, sd = _tiny_ldm()
    al_cpu, al = _tiny_alignment(), _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    B, n = 2, 10
    zc = seeded_input("gdzc", (B,) + tuple(cfg["input_shape"]), 21)
    shape = ldm.get_batch_latent_shape(B)
    gen = torch.Generator().manual_seed(22)
    tape = [torch.randn(shape, generator=gen) for _ in range(n + 1)]
    avg = torch.tensor([[0.4], [0.1]])
    ak = {"avg_x_gt": avg.cuda()}
    kw = dict(cond=zc.cuda(), batch_size=B, return_decoded=False, sampler="ddim", ddim_steps=n, noise_tape=tape)
    for eta in (0.0, 1.0):
        ref = _oracle_guided_ddim(sd, cfg, zc, tape, n, eta, lambda z, t: al_cpu.get_mean_shift(z, t, avg_x_gt=avg))
        out = ldm.sample(use_alignment=True, alignment_kwargs=ak, eta=eta, **kw)
        plain = ldm.sample(eta=eta, **kw)
        e, d = rel_l2(out, ref), rel_l2(out, plain)
        print(f"[tiny guided DDIM-{n} eta={eta}] rel-L2 vs oracle loop {e:.3e}; guided vs un-guided {d:.3e}")
        assert e < 1e-3
        assert d > 3e-2                      # the guidance moves the sample far beyond the parity bar
    # guide_scale 0: the un-guided DDIM sample, bit for bit (zero shift -> the guided epilogue is the un-guided step)
    al.guide_scale = 0.0
    assert torch.equal(ldm.sample(use_alignment=True, alignment_kwargs=ak, eta=1.0, **kw), ldm.sample(eta=1.0, **kw))
    al.guide_scale = 50.0
    # denoiser graphs on 1 / 2 lane streams next to the guidance, and the eager loop: the same latents bit for bit
    outs = []
    for lanes, graph in ((1, True), (2, True), (1, False)):
        ldm.aligned_lanes, ldm.use_hip_graph = lanes, graph
        outs.append(ldm.sample(use_alignment=True, alignment_kwargs=ak, eta=1.0, **kw))
    ldm.aligned_lanes, ldm.use_hip_graph = 1, True
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # x_T and return_intermediates
    lat, inter = ldm.ddim_sample_loop(zc.cuda(), shape, ddim_steps=n, eta=0.0, x_T=tape[0].cuda(), return_intermediates=True,
                                      use_alignment=True, alignment_kwargs=ak)
    assert len(inter) == n + 1 and torch.equal(inter[-1], lat)
    assert torch.equal(lat, ldm.sample(use_alignment=True, alignment_kwargs=ak, eta=0.0, **kw))
    with pytest.raises(NotImplementedError, match="inpainting"):
        ldm.sample(use_alignment=True, alignment_kwargs=ak, mask=torch.ones(shape), x0=torch.zeros(shape), **kw)


@pytest.mark.gpu
def test_aligned_generator_draws_same_in_every_mode():
    """No tape: the aligned ancestral loop draws each step's noise after the denoiser and the guidance, guided DDIM (eta = 1) at the
    start of the step.  One or two denoiser lanes next to the guidance and the eager loop consume the device generator alike: the
    same latents bit for bit under one seed."""
    ldm, cfg, _ = _tiny_ldm()
    al = _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    B = 2
    zc = seeded_input("gdzc", (B,) + tuple(cfg["input_shape"]), 21).cuda()
    ak = {"avg_x_gt": torch.tensor([[0.4], [0.1]]).cuda()}
    for kw in (dict(timesteps=3), dict(sampler="ddim", ddim_steps=4, eta=1.0)):
        outs = []
        for lanes, graph in ((1, True), (2, True), (1, False)):
            ldm.aligned_lanes, ldm.use_hip_graph = lanes, graph
            torch.manual_seed(31)
            outs.append(ldm.sample(cond=zc, batch_size=B, use_alignment=True, alignment_kwargs=ak, return_decoded=False, **kw))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), kw


@pytest.mark.gpu
def test_evaluate_context_ddim_aligned():
    from prediff_amd import config as CFG
    from prediff_amd.alignment import get_alignment_kwargs_avg_x
    from prediff_amd.autoencoder_kl import AutoencoderKL
    vae = AutoencoderKL(**TINY_VAE_CFG, precision="fp32")
    vae.load_state_dict(seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 601))
    ldm, cfg, _ = _tiny_ldm(vae=vae.cuda())
    al = _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    B, T_in, T_out = 2, cfg["input_shape"][0], cfg["target_shape"][0]
    seq = seeded_input("gdseq", (B, T_in + T_out, 32, 32, 1), 23, kind="uniform").cuda()
    gen = torch.Generator().manual_seed(24)
    tape = torch.stack([torch.randn(ldm.get_batch_latent_shape(B), generator=gen) for _ in range(6)])
    run_cfg = {"layout": {"in_len": T_in, "out_len": T_out}, "eval": {}}
    out = CFG.evaluate_context(ldm, seq, run_cfg, sampler="ddim", ddim_steps=5, eta=1.0, noise_tape=tape)
    assert len(out["aligned_pred"]) == 1 and out["aligned_pred"][0].shape == (B, T_out, 32, 32, 1)
    ctx, tgt = CFG.split_sequence(seq, T_in, T_out)
    direct = ldm.sample(cond={"y": ctx}, batch_size=B, use_alignment=True, sampler="ddim", ddim_steps=5, eta=1.0, noise_tape=tape,
                        alignment_kwargs=get_alignment_kwargs_avg_x(context_seq=ctx, target_seq=tgt))
    assert torch.equal(out["aligned_pred"][0], direct)
    assert not torch.equal(out["aligned_pred"][0], out["pred"][0])


@pytest.mark.gpu
def test_v1_guided_ddim10_vs_oracle():
    """The v1 size, B = 2, guided DDIM-10 at guide_scale 50: the fp32 and fp16x2 engines against one oracle loop."""
    from prediff_amd.alignment import SEVIRAvgIntensityAlignment
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.latent_diffusion import LatentDiffusion
    B, n = 2, 10
    sd = seeded_state_dict(TP.unet_template(V1_UNET_CFG, "v1_unet_schema.json"), 1234)
    zc = seeded_input("gv1c", (B, 7, 16, 16, 64), 31)
    tape = [seeded_input("gv1x", (B, 6, 16, 16, 64), 32)] + [seeded_input(f"gv1n{k}", (B, 6, 16, 16, 64), 33) for k in range(n)]
    avg = torch.tensor([[0.31], [0.12]])

    def make_alignment():
        al = SEVIRAvgIntensityAlignment(alignment_type="avg_x", guide_scale=50.0, model_type="cuboid", model_args=dict(V1_ALIGN_ARGS))
        al.model.load_state_dict(seeded_state_dict(al.model.state_dict(), 701))
        al.model.eval()
        return al

    al_cpu = make_alignment()
    nthr = torch.get_num_threads()
    torch.set_num_threads(min(nthr, 16))
    try:
        ref = _oracle_guided_ddim(sd, V1_UNET_CFG, zc, tape, n, 1.0, lambda z, t: al_cpu.get_mean_shift(z, t, avg_x_gt=avg))
    finally:
        torch.set_num_threads(nthr)
    for precision in ("fp32", "fp16x2"):
        net = CuboidTransformerUNet(**V1_UNET_CFG, precision=precision)
        net.load_state_dict(sd, strict=True)
        ldm = LatentDiffusion(torch_nn_module=net, **V1_LDM_KW).cuda().eval()
        al = make_alignment()
        al.model.cuda()
        ldm.set_alignment(al.get_mean_shift)
        out = ldm.sample(cond=zc.cuda(), batch_size=B, return_decoded=False, sampler="ddim", ddim_steps=n, eta=1.0,
                         noise_tape=[x.cuda() for x in tape], use_alignment=True, alignment_kwargs={"avg_x_gt": avg.cuda()})
        e = rel_l2(out, ref)
        print(f"[v1 guided DDIM-{n}, guide_scale 50] {precision}: rel-L2 vs the oracle loop {e:.3e}")
        assert e < 1e-3, precision
        del ldm, al, net
