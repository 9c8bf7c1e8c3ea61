"""Time LagrangianPersistence (pd_lk_motion: the pyramid and the Lucas-Kanade iterations; pd_advect: one launch) on the GPU box, each
call beside its compulsory HBM traffic and beside one DDIM step of the v1 denoiser at the same batch, measured in the same process.

    python scripts/time_extrapolation.py [log] [reps]        (default: profiles/time_extrapolation.log, 30 repeats)

Two workloads, default options (4 levels, 3 iterations, radius 7, 3 pairs): B = 32 contexts of 7 x 128 x 128 -> 6 frames (the v1 shape,
one ensemble's worth) and B = 4 contexts of 13 x 384 x 384 -> 12 frames (full resolution).  Compulsory traffic is what the shapes
demand, every input read once and every output written once: motion reads the P + 1 newest frames and writes two fields; advect reads a
frame and two fields and writes K frames; forecast reads P + 1 frames and writes K.  After three warm-up calls (the first allocates the
workspace) each repeat times one call between two events with a device synchronise; the lines give the median, the minimum and the
maximum.  The DDIM step is the bf16 engine's 50-step latent loop (seeded weights, eta = 0, HIP graph) divided by 50, after an untimed
loop of the same length.  Report only: nothing here is a pass criterion, and there is no earlier version to compare a time with."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd import LagrangianPersistence  # noqa: E402
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet  # noqa: E402
from prediff_amd.latent_diffusion import LatentDiffusion  # noqa: E402
from prediff_amd.presets import V1_UNET_CFG  # noqa: E402
from prediff_amd.seeding import seeded_state_dict  # noqa: E402

LOG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "time_extrapolation.log")
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
out = open(LOG, "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return [once(fn) for _ in range(REPS)]


def line(name, ts, nbytes, step_us):
    med = statistics.median(ts)
    return (f"  {name:9}: median {med:9.1f} us  (min {min(ts):9.1f}, max {max(ts):9.1f}, {len(ts)} repeats)  compulsory {nbytes / 1e6:8.2f} MB"
            f" -> {nbytes / med / 1e3:7.1f} GB/s  |  {med / step_us * 100:6.2f} % of one DDIM step")


def ddim_step_us(ldm, B):
    """one step of the 50-step DDIM latent loop at batch B, in us: the median of three timed loops after an untimed one"""
    zc = torch.randn((B, 7, 16, 16, 64), generator=g, device=dev)
    shape = ldm.get_batch_latent_shape(B)
    x_T = torch.randn(shape, generator=g, device=dev)
    ldm.ddim_sample_loop(zc, shape, ddim_steps=50, eta=0.0, x_T=x_T)
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z = ldm.ddim_sample_loop(zc, shape, ddim_steps=50, eta=0.0, x_T=x_T)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6 / 50)
        assert bool(torch.isfinite(z).all())
    return statistics.median(ts)


net = CuboidTransformerUNet(**V1_UNET_CFG, precision="bf16")
net.load_state_dict(seeded_state_dict(net.state_dict(), 1234))
ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(6, 128, 128, 1), timesteps=1000, beta_schedule="linear",
                      use_ema=False, latent_shape=(6, 16, 16, 64), first_stage_model=None, cond_stage_model=None).to(dev).eval()

say("# python scripts/time_extrapolation.py (one MI355X, gfx950); fp32 NTHWC frames; default options; report only")
say(f"device {torch.cuda.get_device_name(0)}, {REPS} repeats per line, 3 warm-up calls")
with torch.no_grad():
    for B, T, H, W, K in ((32, 7, 128, 128, 6), (4, 13, 384, 384, 12)):
        lp = LagrangianPersistence(out_len=K)
        ctx = torch.rand((B, T, H, W, 1), generator=g, device=dev)
        P = min(lp.pairs, T - 1)
        frame = 4 * B * H * W
        launches = lp.levels - 1 + lp.levels * lp.iters
        step = ddim_step_us(ldm, B)
        say(f"B = {B} contexts of {T} x {H} x {W} -> {K} frames; motion {launches} launches, advect 1; one DDIM step of the v1 denoiser at "
            f"batch {B} (bf16, graph): {step:.0f} us")
        mot = lp.motion(ctx)
        say(line("motion", timed(lambda: lp.motion(ctx)), (P + 1 + 2) * frame, step))
        say(line("advect", timed(lambda: lp.advect(ctx[:, -1], mot)), (1 + 2 + K) * frame, step))
        say(line("forecast", timed(lambda: lp.forecast(ctx)), (P + 1 + K) * frame, step))
out.close()
