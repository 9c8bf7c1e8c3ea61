"""GPU: the sampling driver (prediff_amd.LatentDiffusion) against the golden trajectories captured from the reference
and against the oracle loop, with identical noise tapes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _templates as TP  # noqa: E402
from _cases import TINY_UNET_CFGS, TINY_VAE_CFG  # noqa: E402
from _weights import seeded_input, seeded_state_dict  # noqa: E402
from oracle import diffusion as OD  # noqa: E402
from oracle import unet as OU  # noqa: E402
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet  # noqa: E402
from prediff_amd.latent_diffusion import LatentDiffusion  # noqa: E402


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _tiny_ldm(precision, vae=None):
    cfg = TINY_UNET_CFGS["axial"]
    sd = seeded_state_dict(TP.unet_template(cfg, "tiny_unet_schema.json", "axial"), 600)
    net = CuboidTransformerUNet(**cfg, precision=precision)
    net.load_state_dict(sd)
    T_out, H, W, C = cfg["target_shape"]
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(T_out, H * 4, W * 4, 1), timesteps=1000,
                          beta_schedule="linear", use_ema=False, latent_shape=tuple(cfg["target_shape"]),
                          first_stage_model=vae, cond_stage_model=("__is_first_stage__" if vae is not None else None),
                          scale_factor=1.0)
    return ldm.cuda().eval(), cfg, sd


def test_schedule_buffers_bit_exact(golden):
    ldm, _, _ = _tiny_ldm("bf16")
    g = golden("schedule")
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
              "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
              "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
        assert np.array_equal(getattr(ldm, k).cpu().numpy(), g[k]), k


@pytest.mark.parametrize("use_graph", [False, True])
def test_p_sample_and_loop_vs_reference(golden, use_graph):
    """fp32-split engine: one step at t in {999,500,1,0} and the 3-step loop of sample(timesteps=3) on the recorded tape."""
    ldm, cfg, sd = _tiny_ldm("fp32")
    ldm.use_hip_graph = use_graph
    g = golden("p_sample")
    B = 2
    zc = seeded_input("dzc", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    zt = seeded_input("dzt", (B,) + tuple(cfg["target_shape"]), 6).cuda()
    for tt in (999, 500, 1, 0):
        t = torch.full((B,), tt, dtype=torch.long, device="cuda")
        out = ldm.p_sample(zt=zt, zc=zc, t=t, noise=torch.as_tensor(g[f"psample_noise_{tt}"]).cuda())
        assert rel_l2(out, g[f"psample_{tt}"]) < 1e-4, tt
    s3 = golden("sample3")
    tape = torch.as_tensor(s3["tape"])
    lat = ldm.sample(cond=torch.as_tensor(s3["zc"]).cuda(), batch_size=B, timesteps=3, return_decoded=False, noise_tape=tape)
    e = rel_l2(lat, s3["latent"])
    print(f"[sample3 graph={use_graph}] latent rel-L2 vs reference {e:.3e}")
    assert e < 1e-4


def test_rng_draw_order_matches_reference_convention():
    """Without a tape the loop draws [x_T, n_{T-1}, ..., n_0] from the device generator, one full-latent draw per step
    (also at t = 0): reproduce it by hand with the same seed."""
    ldm, cfg, _ = _tiny_ldm("bf16")
    B = 2
    zc = seeded_input("dzc", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    shape = ldm.get_batch_latent_shape(B)
    for graph in (False, True):
        ldm.use_hip_graph = graph
        torch.manual_seed(99)
        a = ldm.sample(cond=zc, batch_size=B, timesteps=3, return_decoded=False)
        torch.manual_seed(99)
        tape = [torch.randn(shape, device="cuda") for _ in range(4)]
        b = ldm.sample(cond=zc, batch_size=B, timesteps=3, return_decoded=False, noise_tape=tape)
        assert torch.equal(a, b), graph


def test_ddim_vs_oracle_and_determinism():
    ldm, cfg, sd = _tiny_ldm("fp32")
    B = 2
    zc = seeded_input("dzc", (B,) + tuple(cfg["input_shape"]), 5)
    shape = ldm.get_batch_latent_shape(B)
    g = torch.Generator().manual_seed(3)
    tape = [torch.randn(shape, generator=g) for _ in range(11)]
    ac = ldm._alphas_cumprod_f64.astype(np.float32)
    for eta in (0.0, 1.0):
        ref = OD.ddim_sample_loop(ac, lambda z, t, c: OU.unet_forward(sd, cfg, z, t, c), zc, tape, 10, eta=eta)[-1]
        out = ldm.sample(cond=zc.cuda(), batch_size=B, return_decoded=False, sampler="ddim", ddim_steps=10, eta=eta, noise_tape=tape)
        e = rel_l2(out, ref)
        print(f"[ddim eta={eta}] rel-L2 vs oracle loop {e:.3e}")
        assert e < 1e-3
    a = ldm.sample(cond=zc.cuda(), batch_size=B, return_decoded=False, sampler="ddim", ddim_steps=10, eta=0.0, x_T=tape[0].cuda())
    b = ldm.sample(cond=zc.cuda(), batch_size=B, return_decoded=False, sampler="ddim", ddim_steps=10, eta=0.0, x_T=tape[0].cuda())
    assert torch.equal(a, b)          # eta = 0 is deterministic


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_lanes_do_not_change_results(sampler):
    """num_streams > 1 advances the batch as independent sub-batches on concurrent HIP streams (own graph + workspace each):
    same trajectories, bit for bit, as the single-graph and the eager paths, for taped and for generator-drawn noise."""
    ldm, cfg, _ = _tiny_ldm("bf16")
    B = 4
    zc = seeded_input("dzc4", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    shape = ldm.get_batch_latent_shape(B)
    g = torch.Generator().manual_seed(17)
    tape = [torch.randn(shape, generator=g) for _ in range(6)]
    kw = dict(cond=zc, batch_size=B, return_decoded=False)
    kw.update(dict(timesteps=4) if sampler == "ddpm" else dict(sampler="ddim", ddim_steps=5, eta=1.0))
    outs = {}
    for S in (1, 2, 4):
        ldm.num_streams = S
        outs[S] = ldm.sample(noise_tape=tape, **kw)
        torch.manual_seed(5)
        outs[S, "rng"] = ldm.sample(**kw)
    ldm.use_hip_graph = False
    eager = ldm.sample(noise_tape=tape, **kw)
    assert torch.equal(outs[1], eager) and torch.equal(outs[2], outs[1]) and torch.equal(outs[4], outs[1])
    assert torch.equal(outs[2, "rng"], outs[1, "rng"]) and torch.equal(outs[4, "rng"], outs[1, "rng"])
    assert bool(torch.isfinite(outs[2]).all())


def test_ancestral_hooks_same_in_every_mode():
    """Per-step hooks of the ancestral loop (intermediates every log_every_t, callback, img_callback, inpainting mask / x0) force the
    non-lane path: the single graph, the eager loop and num_streams = 2 give the same intermediates and hook arguments bit for bit."""
    ldm, cfg, _ = _tiny_ldm("bf16")
    B = 4
    zc = seeded_input("dzc4", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    shape = ldm.get_batch_latent_shape(B)
    g = torch.Generator().manual_seed(19)
    tape = [torch.randn(shape, generator=g) for _ in range(5)]
    x0 = torch.randn(shape, generator=g).cuda()
    mask = torch.zeros(shape, device="cuda")
    mask[:, :1] = 1.0
    runs = {}
    for name, S, graph in (("graph", 1, True), ("eager", 1, False), ("two streams", 2, True)):
        ldm.num_streams, ldm.use_hip_graph = S, graph
        seen = []
        torch.manual_seed(7)                  # the mask's q_sample draws from the device generator
        out, inter = ldm.p_sample_loop(cond=zc, shape=shape, timesteps=4, noise_tape=tape, return_intermediates=True, log_every_t=2,
                                       mask=mask, x0=x0, callback=seen.append, img_callback=lambda img, i: seen.append((i, img.clone())))
        runs[name] = (out, inter, seen)
    out, inter, seen = runs["graph"]
    assert len(inter) == 4 and torch.equal(inter[-1], out)      # x_T, then t = 3 (the first step), 2, 0
    assert [s for s in seen if isinstance(s, int)] == [3, 2, 1, 0]
    for name in ("eager", "two streams"):
        o, i, s = runs[name]
        assert torch.equal(o, out) and len(i) == len(inter) and all(torch.equal(a, b) for a, b in zip(i, inter)), name
        assert len(s) == len(seen), name
        for a, b in zip(s, seen):
            assert a == b if isinstance(b, int) else (a[0] == b[0] and torch.equal(a[1], b[1])), name


def test_ddim_intermediates_same_in_every_mode():
    """DDIM with return_intermediates: the single graph and the eager loop give the same list bit for bit; its last entry is the
    two-lane result without intermediates."""
    ldm, cfg, _ = _tiny_ldm("bf16")
    B = 4
    zc = seeded_input("dzc4", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    shape = ldm.get_batch_latent_shape(B)
    g = torch.Generator().manual_seed(23)
    tape = [torch.randn(shape, generator=g) for _ in range(6)]
    ldm.num_streams = 2
    lanes = ldm.ddim_sample_loop(zc, shape, ddim_steps=5, eta=1.0, noise_tape=tape)
    assert 1 in ldm._graphs                   # the second lane's graph: the batch did run as two lanes
    inters = []
    for graph in (True, False):
        ldm.use_hip_graph = graph
        out, inter = ldm.ddim_sample_loop(zc, shape, ddim_steps=5, eta=1.0, noise_tape=tape, return_intermediates=True)
        assert len(inter) == 6 and torch.equal(inter[-1], out)
        inters.append(inter)
    assert all(torch.equal(a, b) for a, b in zip(*inters))
    assert torch.equal(inters[0][-1], lanes)


def test_graph_tracks_weight_updates():
    ldm, cfg, sd = _tiny_ldm("bf16")
    B = 1
    zc = seeded_input("dzc", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    tape = [torch.randn(ldm.get_batch_latent_shape(B)) for _ in range(3)]
    a = ldm.sample(cond=zc, batch_size=B, timesteps=2, return_decoded=False, noise_tape=tape)
    ldm.torch_nn_module.load_state_dict(seeded_state_dict(sd, 601))
    b = ldm.sample(cond=zc, batch_size=B, timesteps=2, return_decoded=False, noise_tape=tape)
    ldm.use_hip_graph = False
    c = ldm.sample(cond=zc, batch_size=B, timesteps=2, return_decoded=False, noise_tape=tape)
    assert not torch.equal(a, b) and torch.equal(b, c)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_end_to_end_with_vae(golden, precision):
    """LatentDiffusion.sample(cond={'y': pixels}): VAE-encode the context frames -> 3 ancestral steps -> VAE-decode,
    against the decoded frames the reference produced for the same seeded weights and noise tape."""
    from prediff_amd.autoencoder_kl import AutoencoderKL
    vae = AutoencoderKL(**TINY_VAE_CFG, precision=precision)
    vae.load_state_dict(seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 601))
    ldm, cfg, _ = _tiny_ldm(precision, vae=vae)
    s3 = golden("sample3")
    B, T_in = 2, cfg["input_shape"][0]
    y = seeded_input("dy", (B, T_in, 32, 32, 1), 8, kind="uniform").cuda()
    zc = ldm.cond_stage_forward({"y": y})
    dec = ldm.sample(cond={"y": y}, batch_size=B, timesteps=3, noise_tape=torch.as_tensor(s3["tape"]))
    e_zc, e_dec = rel_l2(zc, s3["zc"]), rel_l2(dec, s3["decoded"])
    print(f"[e2e {precision}] context latent {e_zc:.3e}, decoded frames {e_dec:.3e} (vs reference)")
    assert dec.shape == (B, cfg["target_shape"][0], 32, 32, 1)
    tol = 1e-3 if precision == "fp32" else 5e-2       # north_star bar: 1e-3 rel-L2 for the fp32-class engine
    assert e_zc < tol and e_dec < tol


def test_shorten_cond_schedule_vs_reference(golden):
    """num_timesteps_cond = 4 (reference latent_diffusion.py:155-157, 295-299, 665-667): cond_ids bit-equal, and three ancestral steps
    with the conditioning latents re-noised in front of each one against the reference's output on the same tapes (draw order
    x_T, c_2, n_2, c_1, n_1, c_0, n_0); fp32-class engine, the bar of the plain loop."""
    cfg = TINY_UNET_CFGS["axial"]
    sd = seeded_state_dict(TP.unet_template(cfg, "tiny_unet_schema.json", "axial"), 600)
    net = CuboidTransformerUNet(**cfg, precision="fp32")
    net.load_state_dict(sd)
    T_out, H, W, C = cfg["target_shape"]
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(T_out, H * 4, W * 4, 1), timesteps=1000,
                          beta_schedule="linear", use_ema=False, latent_shape=tuple(cfg["target_shape"]), first_stage_model=None,
                          cond_stage_model=None, scale_factor=1.0, num_timesteps_cond=4).cuda().eval()
    g = golden("cond_schedule")
    assert ldm.shorten_cond_schedule and np.array_equal(ldm.cond_ids.cpu().numpy(), g["cond_ids"])
    B = 2
    lat = (B,) + tuple(cfg["target_shape"])
    zc = seeded_input("dzc", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    tx, tc = torch.as_tensor(g["tape_x"]), torch.as_tensor(g["tape_c"])
    tape = [tx[0]]
    for k in range(3):
        tape += [tc[k], tx[1 + k]]
    out = ldm.p_sample_loop(cond=zc, shape=lat, timesteps=3, noise_tape=tape)
    e = rel_l2(out, g["latent"])
    print(f"[shorten_cond_schedule] 3-step loop vs reference {e:.3e}")
    assert e < 1e-4
    with pytest.raises(NotImplementedError):
        ldm.ddim_sample_loop(zc, lat, ddim_steps=5)


def test_ensemble_members_are_batch_split_invariant():
    """prediff_amd.ensemble on one GPU: a member's trajectory depends only on (base_seed, member id), not on how the
    members are batched (=> not on the world size either; the 2-rank gather logic is covered on CPU/gloo)."""
    from prediff_amd.ensemble import sample_ensemble
    ldm, cfg, _ = _tiny_ldm("fp32")
    zc = seeded_input("dzc", (1,) + tuple(cfg["input_shape"]), 5).cuda()
    a = sample_ensemble(ldm, zc, 4, base_seed=1000, sampler="ddim", ddim_steps=5, return_decoded=False)
    b = sample_ensemble(ldm, zc, 4, base_seed=1000, sampler="ddim", ddim_steps=5, return_decoded=False, micro_batch=1)
    c = sample_ensemble(ldm, zc, 4, base_seed=1000, sampler="ddpm", timesteps=3, return_decoded=False, micro_batch=2)
    d = sample_ensemble(ldm, zc, 4, base_seed=1000, sampler="ddpm", timesteps=3, return_decoded=False)
    assert a.shape == (4,) + tuple(cfg["target_shape"])
    assert rel_l2(b, a) < 1e-6 and rel_l2(c, d) < 1e-6
    assert rel_l2(a[0], a[1]) > 1e-2            # members differ


def test_config_front_end_end_to_end():
    """YAML -> build_prediff -> evaluate_context (the sampling part of the reference test_step) on a reduced-size config."""
    import os
    from prediff_amd import config as CFG
    from prediff_amd.sevir_skill import SEVIRSkillScore
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = CFG.load_config(os.path.join(root, "configs", "prediff_sevirlr_v1.yaml"))
    # shrink: 32x32 frames, 2-level VAE, small denoiser / alignment net (same code paths, seconds instead of minutes)
    cfg["layout"].update(img_height=32, img_width=32)
    cfg["model"]["vae"].update(block_out_channels=[32, 64, 64], down_block_types=["DownEncoderBlock2D"] * 3,
                               up_block_types=["UpDecoderBlock2D"] * 3, layers_per_block=1, latent_channels=4, norm_num_groups=8)
    cfg["model"]["latent_model"].update(input_shape=[7, 8, 8, 4], target_shape=[6, 8, 8, 4], base_units=64, depth=[1, 1], num_heads=2)
    cfg["model"]["diffusion"].update(data_shape=[6, 32, 32, 1], latent_shape=[6, 8, 8, 4])
    cfg["model"]["align"]["model_args"].update(input_shape=[6, 8, 8, 4], base_units=32, num_heads=2)
    ldm, align = CFG.build_prediff(cfg, precision="bf16")
    for mod, seed in ((ldm.torch_nn_module, 1), (ldm.first_stage_model, 2), (align.model, 3)):
        mod.load_state_dict(seeded_state_dict(mod.state_dict(), seed))
    seq = seeded_input("seq", (2, 13, 32, 32, 1), 4, kind="uniform").cuda()
    score, ascore = (SEVIRSkillScore(layout="NTHWC", mode="0") for _ in range(2))
    out = CFG.evaluate_context(ldm, seq, cfg, score=score, aligned_score=ascore, timesteps=3)
    assert out["pred"][0].shape == (2, 6, 32, 32, 1) and out["aligned_pred"][0].shape == (2, 6, 32, 32, 1)
    assert bool(torch.isfinite(out["pred"][0]).all()) and bool(torch.isfinite(out["aligned_pred"][0]).all())
    assert not torch.equal(out["pred"][0], out["aligned_pred"][0])
    res = score.compute()
    assert set(res.keys()) == {16, 74, 133, 160, 181, 219, "avg"} and 0.0 <= res["avg"]["csi"] <= 1.0


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_config_front_end_vs_oracle_loop(precision, tol):
    """SURVEY §8 f1 with a parity statement: YAML -> build_prediff -> evaluate_context (the sampling part of the reference test_step,
    scripts/prediff/sevirlr/train_sevirlr_prediff.py:905-979, unaligned branch) against the ORACLE run of the same loop on one noise
    tape: VAE-encode the context, 4 ancestral steps, VAE-decode -> decoded frames, then the SEVIRSkillScore counts of those frames."""
    import os
    from oracle import diffusion as OD, skill as OS, unet as OU, vae as OV
    from prediff_amd import config as CFG
    from prediff_amd.sevir_skill import SEVIRSkillScore
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = CFG.load_config(os.path.join(root, "configs", "prediff_sevirlr_v1.yaml"))
    cfg["layout"].update(img_height=32, img_width=32)
    cfg["model"]["vae"].update(block_out_channels=[32, 64, 64], down_block_types=["DownEncoderBlock2D"] * 3,
                               up_block_types=["UpDecoderBlock2D"] * 3, layers_per_block=1, latent_channels=4, norm_num_groups=8)
    cfg["model"]["latent_model"].update(input_shape=[7, 8, 8, 4], target_shape=[6, 8, 8, 4], base_units=64, depth=[1, 1], num_heads=2)
    cfg["model"]["diffusion"].update(data_shape=[6, 32, 32, 1], latent_shape=[6, 8, 8, 4])
    cfg["model"]["align"]["alignment_type"] = None
    cfg["eval"] = dict(cfg.get("eval", {}), eval_aligned=False, eval_unaligned=True, num_samples_per_context=1)
    ldm, _ = CFG.build_prediff(cfg, precision=precision)
    usd = seeded_state_dict(ldm.torch_nn_module.state_dict(), 1)
    vsd = seeded_state_dict(ldm.first_stage_model.state_dict(), 2)
    ldm.torch_nn_module.load_state_dict(usd)
    ldm.first_stage_model.load_state_dict(vsd)
    B, steps = 2, 4
    seq = seeded_input("seqf1", (B, 13, 32, 32, 1), 4, kind="uniform")
    g = torch.Generator().manual_seed(99)
    tape = [torch.randn(B, 6, 8, 8, 4, generator=g) for _ in range(steps + 1)]
    score = SEVIRSkillScore(layout="NTHWC", mode="0")
    out = CFG.evaluate_context(ldm, seq.cuda(), cfg, score=score, timesteps=steps, noise_tape=torch.stack(tape))
    pred = out["pred"][0].float().cpu()
    # ---- the oracle's run of the same loop ----
    ucfg, vcfg = CFG.unet_kwargs(cfg["model"]["latent_model"]), CFG.vae_kwargs(cfg["model"]["vae"])
    ctx, tgt = seq[:, :7], seq[:, 7:13]
    zc = OV.vae_encode_mode(vsd, vcfg, ctx.permute(0, 1, 4, 2, 3).reshape(B * 7, 1, 32, 32))
    zc = zc.reshape(B, 7, *zc.shape[1:]).permute(0, 1, 3, 4, 2)
    buf = {k: torch.as_tensor(v) for k, v in OD.schedule_buffers(OD.beta_schedule("linear", 1000)).items()}
    traj = OD.ddpm_sample_loop(buf, lambda z, t, c: OU.unet_forward(usd, ucfg, z, t, c), zc, tape, steps)
    z0 = traj[-1]
    ref = OV.vae_decode(vsd, vcfg, z0.permute(0, 1, 4, 2, 3).reshape(B * 6, -1, 8, 8)).reshape(B, 6, 1, 32, 32).permute(0, 1, 3, 4, 2)
    e = rel_l2(pred, ref)
    print(f"[front end {precision}] decoded frames of evaluate_context vs the oracle loop: rel-L2 {e:.3e}")
    assert pred.shape == ref.shape and e < tol
    # skill counts: the HIP scorer on the HIP frames == the oracle scorer on the same frames (bit-exact integer work) ...
    hits, misses, fas = OS.counts(pred.numpy(), tgt.numpy(), t_axis=1, keep_seq=False)           # (mode "0": summed over the sequence)
    as_i64 = lambda t: t.cpu().numpy().astype(np.int64)
    assert np.array_equal(as_i64(score.hits), hits) and np.array_equal(as_i64(score.misses), misses) and np.array_equal(as_i64(score.fas), fas)
    # ... and the counts of the oracle's frames differ from them only where a pixel sits within the engine's error of a threshold
    h2, m2, f2 = OS.counts(ref.numpy(), tgt.numpy(), t_axis=1, keep_seq=False)
    npx = pred.numel()
    drift = (np.abs(hits - h2).sum() + np.abs(misses - m2).sum() + np.abs(fas - f2).sum()) / (npx * hits.shape[0])
    print(f"[front end {precision}] skill-count drift between the two pipelines: {drift:.2e} of the (pixel, threshold) decisions")
    assert drift < (1e-3 if precision == "fp32" else 3e-2)
