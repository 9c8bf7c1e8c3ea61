"""Tiled sampling against the plain sampler at the v1 configuration, bf16 engine, one process (run on the GPU box):
  A. the step: a 32 x 32 latent canvas (256 x 256 px), stride 8 -> 3 x 3 windows, B = 7 canvases = 63 windows per denoiser call, against the
     plain module at batch 63; DDIM, 50 uniform steps, one graph each (latent loop only), ms per step;
  B. one ensemble of 7 on the canvas end to end (tiled VAE encode + loop + tiled decode), s.
A interleaves the two arms REPS times; every timed run follows an untimed run of the same arm (graph capture, workspaces).
Usage: time_tiled.py [REPS] [LOG]; the lines are printed and written to LOG (default profiles/time_tiled.log)."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.presets import V1_UNET_CFG, V1_VAE_CFG
from prediff_amd.seeding import seeded_state_dict
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
from prediff_amd.autoencoder_kl import AutoencoderKL
from prediff_amd.ensemble import sample_ensemble
from prediff_amd.latent_diffusion import LatentDiffusion
from prediff_amd.tiled import TiledLatentDiffusion

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
LOG = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_tiled.log")
dev = torch.device("cuda")
net = CuboidTransformerUNet(**V1_UNET_CFG, precision="bf16")
net.load_state_dict(seeded_state_dict(net.state_dict(), 1234))
vae = AutoencoderKL(**V1_VAE_CFG, precision="bf16")
vae.load_state_dict(seeded_state_dict(vae.state_dict(), 77))
kw = dict(layout="NTHWC", data_shape=(6, 128, 128, 1), timesteps=1000, beta_schedule="linear", use_ema=False, latent_shape=(6, 16, 16, 64),
          first_stage_model=vae, cond_stage_model="__is_first_stage__", scale_factor=1.0)
plain = LatentDiffusion(torch_nn_module=net, **kw).to(dev).eval()
tiled = TiledLatentDiffusion(net, canvas=(32, 32), stride=(8, 8), **kw).to(dev).eval()
plain.num_streams = tiled.num_streams = 1
log = open(LOG, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); return r, time.perf_counter() - t0


def spread(v):
    return f"min {min(v):.3f} median {sorted(v)[len(v) // 2]:.3f} max {max(v):.3f}"


with torch.no_grad():
    B, N, nwin = 7, 50, tiled.geometry.nwin
    assert nwin == 9
    say(f"{torch.cuda.get_device_name(0)}; v1 bf16, canvas 32 x 32, stride 8: {nwin} windows, B = {B} -> {B * nwin} windows per denoiser call")
    zc_canvas = torch.randn(B, 7, 32, 32, 64, device=dev)
    zc_win = tiled.gather_windows(zc_canvas)
    x_canvas = torch.randn(tiled.get_batch_latent_shape(B), device=dev)
    zc_plain = zc_win.reshape((B * nwin,) + tuple(zc_win.shape[2:])).contiguous()
    x_plain = tiled.gather_windows(x_canvas).reshape((B * nwin,) + tuple(plain.latent_shape)).contiguous()
    loops = {"plain": lambda n: plain.ddim_sample_loop(zc_plain, tuple(x_plain.shape), ddim_steps=n, eta=0.0, x_T=x_plain),
             "tiled": lambda n: tiled.ddim_sample_loop(zc_win, tuple(x_canvas.shape), ddim_steps=n, eta=0.0, x_T=x_canvas)}
    ms = {k: [] for k in loops}
    for rep in range(REPS):
        for name, fn in loops.items():
            fn(2)
            out, t = timed(lambda: fn(N))
            assert bool(torch.isfinite(out).all())
            ms[name].append(t * 1e3 / N)
            say(f"A rep {rep} {name}: {N} DDIM steps, {B * nwin} windows in one graph: {t * 1e3 / N:.3f} ms / step")
    for name, v in ms.items():
        say(f"A {name}: ms / step {spread(v)}")
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    say(f"A tiled - plain, medians: {med['tiled'] - med['plain']:+.3f} ms / step (ratio {med['tiled'] / med['plain']:.4f}); "
        f"min-max spread of the plain arm: {max(ms['plain']) - min(ms['plain']):.3f} ms")

    M = 7
    ctx = torch.rand(1, 7, 256, 256, 1, device=dev)
    secs = []
    for rep in range(REPS):
        sample_ensemble(tiled, {"y": ctx}, M, base_seed=1000, sampler="ddim", ddim_steps=50)
        out, t = timed(lambda: sample_ensemble(tiled, {"y": ctx}, M, base_seed=1000, sampler="ddim", ddim_steps=50))
        assert tuple(out.shape) == (M, 6, 256, 256, 1) and bool(torch.isfinite(out).all())
        secs.append(t)
        say(f"B rep {rep}: ensemble of {M} on the 256 x 256 px canvas, DDIM-50, end to end {t:.3f} s ({M / t:.2f} canvases / s)")
    say(f"B: s {spread(secs)}")
log.close()
