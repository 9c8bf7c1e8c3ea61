"""Rolling forecasts at the v1 configuration, bf16 engine, one process (run on the GPU box):
  A. one pd_context_advance launch (stride 6, the 6 kept frames appended to a 12-frame latent) for 64 trajectories against the torch
     sequence it replaces (scale, [pd_window_gather,] cat, slice, and the append as a slice copy), device events around LAUNCHES
     back-to-back launches, the two arms interleaved REPS times after an untimed round; the outputs of the two arms are compared bit for bit:
       A1. the plain module: context (64, 1, 7, 16, 16, 64), forecast (64, 6, 16, 16, 64);
       A2. a 64 x 80 latent canvas at stride 8: 7 x 9 = 63 windows, context (64, 63, 7, 16, 16, 64), forecast (64, 6, 64, 80, 64);
  B. a 12-frame rollout end to end (rollout_ensemble: 32 members, stride 6, DDIM-50, VAE encode + two segments + one decode of 12 frames)
     against two plain sample_ensemble calls of the same size (each: VAE encode + one segment + a decode of 6 frames), interleaved; every
     timed call follows an untimed call of the same arm (graph capture, workspaces).
Usage: time_rollout.py [REPS] [LOG]; the lines are printed and written to LOG (default profiles/time_rollout.log)."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd import _lib as L
from prediff_amd.presets import V1_UNET_CFG, V1_VAE_CFG
from prediff_amd.seeding import seeded_state_dict
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
from prediff_amd.autoencoder_kl import AutoencoderKL
from prediff_amd.ensemble import sample_ensemble
from prediff_amd.latent_diffusion import LatentDiffusion
from prediff_amd.rollout import rollout_ensemble
from prediff_amd.tiled import TileGeometry

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LOG = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_rollout.log")
LAUNCHES = 10
dev = torch.device("cuda")
log = open(LOG, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def spread(v):
    return f"min {min(v):.3f} median {sorted(v)[len(v) // 2]:.3f} max {max(v):.3f}"


def event_ms(fn):
    """ms per call over LAUNCHES back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / LAUNCHES


def advance_arms(label, B, canvas, stride_hw):
    T_in, T_out, C, s, z_scale = 7, 6, 64, 6, 1.0 / 0.18215
    geo = TileGeometry((16, 16), canvas, stride_hw)
    nwin, origins = geo.nwin, geo.origins
    ctx = torch.randn(B, nwin, T_in, 16, 16, C, device=dev)
    z = torch.randn((B, T_out) + canvas + (C,), device=dev)
    out = {arm: (torch.empty_like(ctx), torch.empty((B, 2 * T_out) + canvas + (C,), device=dev)) for arm in ("kernel", "torch")}

    def kernel():
        nxt, fc = out["kernel"]
        L.context_advance(ctx, z, origins, nxt, s, z_scale, forecast=fc, f_off=0, f_cnt=s)

    def torch_sequence():
        nxt, fc = out["torch"]
        zs = z * z_scale
        if nwin > 1:
            zw = torch.empty((B, nwin, T_out, 16, 16, C), device=dev)
            L.window_gather(zs, zw, origins)
        else:
            zw = zs.unsqueeze(1)
        nxt.copy_(torch.cat([ctx, zw], dim=2)[:, :, s:s + T_in])
        fc[:, :s].copy_(z[:, :s])
    arms = {"kernel": kernel, "torch": torch_sequence}
    for fn in arms.values():                 # untimed: code objects, the origin table's upload, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    assert torch.equal(out["kernel"][0], out["torch"][0]) and torch.equal(out["kernel"][1][:, :s], out["torch"][1][:, :s])
    moved = (2 * ctx.numel() + 2 * s * z[:, 0].numel()) * 4 / 1e9          # the kernel's own traffic: every output element read once, written once
    say(f"{label}: B = {B}, {nwin} window(s), context {tuple(ctx.shape)}, forecast {tuple(z.shape)}; the kernel moves {moved:.3f} GB; "
        f"outputs of the two arms agree bit for bit")
    ms = {k: [] for k in arms}
    for rep in range(REPS):
        for name, fn in arms.items():
            ms[name].append(event_ms(fn))
    for name, v in ms.items():
        say(f"{label} {name}: ms / launch {spread(v)}")
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    say(f"{label} medians: kernel {med['kernel']:.3f} ms ({moved / med['kernel'] * 1e3:.0f} GB/s), torch sequence {med['torch']:.3f} ms "
        f"(ratio torch / kernel {med['torch'] / med['kernel']:.2f})")
    del out, ctx, z
    torch.cuda.empty_cache()


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); return r, time.perf_counter() - t0


with torch.no_grad():
    say(f"{torch.cuda.get_device_name(0)}; command: python scripts/time_rollout.py {REPS}")
    advance_arms("A1 plain", 64, (16, 16), (16, 16))
    advance_arms("A2 63 windows", 64, (64, 80), (8, 8))

    net = CuboidTransformerUNet(**V1_UNET_CFG, precision="bf16")
    net.load_state_dict(seeded_state_dict(net.state_dict(), 1234))
    vae = AutoencoderKL(**V1_VAE_CFG, precision="bf16")
    vae.load_state_dict(seeded_state_dict(vae.state_dict(), 77))
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(6, 128, 128, 1), timesteps=1000, beta_schedule="linear", use_ema=False,
                          latent_shape=(6, 16, 16, 64), first_stage_model=vae, cond_stage_model="__is_first_stage__",
                          scale_factor=0.18215).to(dev).eval()
    M = 32
    ctx = torch.rand(1, 7, 128, 128, 1, device=dev)
    kw = dict(base_seed=1000, sampler="ddim", ddim_steps=50)
    arms = {"rollout 12 frames": lambda: rollout_ensemble(ldm, {"y": ctx}, M, 12, stride=6, **kw),
            "two sample() calls": lambda: torch.cat([sample_ensemble(ldm, {"y": ctx}, M, **kw), sample_ensemble(ldm, {"y": ctx}, M, **kw)], dim=1)}
    secs = {k: [] for k in arms}
    for rep in range(REPS):
        for name, fn in arms.items():
            fn()
            out, t = timed(fn)
            assert tuple(out.shape) == (M, 12, 128, 128, 1) and bool(torch.isfinite(out).all())
            secs[name].append(t)
            say(f"B rep {rep} {name}: {M} members, DDIM-50, end to end {t:.3f} s")
    for name, v in secs.items():
        say(f"B {name}: s {spread(v)}")
    med = {k: sorted(v)[len(v) // 2] for k, v in secs.items()}
    say(f"B medians: rollout {med['rollout 12 frames']:.3f} s, two sample() calls {med['two sample() calls']:.3f} s "
        f"(ratio {med['rollout 12 frames'] / med['two sample() calls']:.4f})")
log.close()
