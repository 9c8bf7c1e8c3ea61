"""The stochastic DPM-Solver++(2M) step against the deterministic one at the v1 configuration, bf16 engine, one process (run on the GPU box):
  A. the step: 64 trajectories in two lanes, 50 steps of either sampler on the uniform grid (latent loop only), ms per step; the
     stochastic loop (eta = 1) draws one whole-batch normal per step on the device, as DDIM at eta > 0 does;
  B. one ensemble of 32 end to end (VAE encode + loop + decode) at 20 and 15 quad steps, samples / s; the members' noise comes from
     their own generators (ensemble.member_noise_fn), one draw for the deterministic solver and one per step more for the stochastic.
A and B interleave the samplers REPS times; every timed run follows an untimed run of the same sampler (graph capture, workspaces)."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.presets import V1_UNET_CFG, V1_VAE_CFG
from prediff_amd.seeding import seeded_state_dict
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
from prediff_amd.autoencoder_kl import AutoencoderKL
from prediff_amd.ensemble import sample_ensemble
from prediff_amd.latent_diffusion import LatentDiffusion

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
dev = torch.device("cuda")
net = CuboidTransformerUNet(**V1_UNET_CFG, precision="bf16")
net.load_state_dict(seeded_state_dict(net.state_dict(), 1234))
vae = AutoencoderKL(**V1_VAE_CFG, precision="bf16")
vae.load_state_dict(seeded_state_dict(vae.state_dict(), 77))
ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(6, 128, 128, 1), timesteps=1000, beta_schedule="linear",
                      use_ema=False, latent_shape=(6, 16, 16, 64), first_stage_model=vae, cond_stage_model="__is_first_stage__",
                      scale_factor=1.0).to(dev).eval()
ldm.num_streams = 2


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); return r, time.perf_counter() - t0


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return f"min {min(v):.3f} median {median(v):.3f} max {max(v):.3f}"


with torch.no_grad():
    B, N = 64, 50
    zc = torch.randn(B, 7, 16, 16, 64, device=dev)
    shape = ldm.get_batch_latent_shape(B)
    x_T = torch.randn(shape, device=dev)
    loops = {"dpmpp_2m": lambda n: ldm.dpmpp_2m_sample_loop(zc, shape, steps=n, discretize="uniform", x_T=x_T),
             "dpmpp_2m_sde": lambda n: ldm.dpmpp_2m_sde_sample_loop(zc, shape, steps=n, eta=1.0, discretize="uniform", x_T=x_T)}
    ms = {k: [] for k in loops}
    for rep in range(REPS):
        for name, fn in loops.items():
            fn(2)
            out, t = timed(lambda: fn(N))
            assert bool(torch.isfinite(out).all())
            ms[name].append(t * 1e3 / N)
            print(f"A rep {rep} {name}: {N} steps, {B} trajectories in 2 lanes: {t * 1e3 / N:.3f} ms / step ({B * N / t:.0f} trajectory-steps / s)")
    for name, v in ms.items():
        print(f"A {name}: ms / step {spread(v)}")
    print(f"A ratio of medians dpmpp_2m_sde / dpmpp_2m: {median(ms['dpmpp_2m_sde']) / median(ms['dpmpp_2m']):.4f}; "
          f"spread of the dpmpp_2m figure itself (max / min): {max(ms['dpmpp_2m']) / min(ms['dpmpp_2m']):.4f}")

    M = 32
    ctx = torch.rand(1, 7, 128, 128, 1, device=dev)
    runs = {f"{tag}-{n} quad": dict(sampler=name, steps=n, **kw) for n in (20, 15)
            for tag, name, kw in (("2m", "dpmpp_2m", {}), ("2m-sde", "dpmpp_2m_sde", {"eta": 1.0}))}
    sps = {k: [] for k in runs}
    for rep in range(REPS):
        for name, kw in runs.items():
            sample_ensemble(ldm, {"y": ctx}, M, base_seed=1000, **kw)
            out, t = timed(lambda: sample_ensemble(ldm, {"y": ctx}, M, base_seed=1000, **kw))
            assert out.shape[0] == M and bool(torch.isfinite(out).all())
            sps[name].append(M / t)
            print(f"B rep {rep} {name}: ensemble of {M} end to end {t:.3f} s, {M / t:.1f} samples / s")
    for name, v in sps.items():
        print(f"B {name}: samples / s {spread(v)}")
    for n in (20, 15):
        print(f"B ratio of medians 2m-sde-{n} / 2m-{n}: {median(sps[f'2m-sde-{n} quad']) / median(sps[f'2m-{n} quad']):.4f}")
