"""The held step against the un-held one at the v1 configuration, bf16 engine, 64 trajectories in two lanes, 50 steps of DDIM (eta 0) and
of DPM-Solver++(2M) on the uniform grid, latent loop only, ms per step (run on the GPU box).  One process times ONE source tree:
    python scripts/time_hold.py [REPS] [LABEL] [TRAJECTORIES]
(TRAJECTORIES: default 64; two lanes from 16 on, one lane below, where a step is shortest and the host's share of it largest)
and works on a tree without held regions too (the parent commit: only the un-held arms run there), so the un-held step of this tree is
compared with the parent's by running the two trees' processes alternately (profiles/time_hold.log).  The arms of a process interleave
REPS times; every timed run follows an untimed run of the same arm (graph capture, workspaces).  The held arms hold the first three
of the six target frames, hold_noise="fresh": one more whole-batch normal draw per step on the device."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.presets import V1_UNET_CFG
from prediff_amd.seeding import seeded_state_dict
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
from prediff_amd.latent_diffusion import LatentDiffusion

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
LABEL = sys.argv[2] if len(sys.argv) > 2 else "this tree"
B = int(sys.argv[3]) if len(sys.argv) > 3 else 64
LANES = 2 if B >= 16 else 1
dev = torch.device("cuda")
net = CuboidTransformerUNet(**V1_UNET_CFG, precision="bf16")
net.load_state_dict(seeded_state_dict(net.state_dict(), 1234))
ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(6, 128, 128, 1), timesteps=1000, beta_schedule="linear",
                      use_ema=False, latent_shape=(6, 16, 16, 64), first_stage_model=None, cond_stage_model=None, scale_factor=1.0).to(dev).eval()
ldm.num_streams = LANES
HELD = hasattr(ldm, "hold_from_frames")


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize(); return r, time.perf_counter() - t0


def median(v):
    return sorted(v)[len(v) // 2]


with torch.no_grad():
    N = 50
    zc = torch.randn(B, 7, 16, 16, 64, device=dev)
    shape = ldm.get_batch_latent_shape(B)
    x_T = torch.randn(shape, device=dev)
    loops = {"ddim": lambda n, **kw: ldm.ddim_sample_loop(zc, shape, ddim_steps=n, eta=0.0, x_T=x_T, **kw),
             "dpmpp_2m": lambda n, **kw: ldm.dpmpp_2m_sample_loop(zc, shape, steps=n, discretize="uniform", x_T=x_T, **kw)}
    arms = {f"{name} un-held": (fn, {}) for name, fn in loops.items()}
    if HELD:
        mask = torch.zeros(1, 6, 1, 1, 1, device=dev)
        mask[:, :3] = 1.0
        hold = dict(hold_mask=mask, hold_x0=torch.randn(shape, device=dev))
        arms.update({f"{name} held": (fn, hold) for name, fn in loops.items()})
    ms = {k: [] for k in arms}
    for rep in range(REPS):
        for arm, (fn, kw) in arms.items():
            fn(2, **kw)
            out, t = timed(lambda: fn(N, **kw))
            assert bool(torch.isfinite(out).all())
            ms[arm].append(t * 1e3 / N)
            print(f"[{LABEL}] rep {rep} {arm}: {N} steps, {B} trajectories in {LANES} lane(s): {t * 1e3 / N:.3f} ms / step", flush=True)
    for arm, v in ms.items():
        print(f"[{LABEL}] {arm}: ms / step min {min(v):.3f} median {median(v):.3f} max {max(v):.3f} ({len(v) * N} timed steps)")
    if HELD:
        for name in loops:
            print(f"[{LABEL}] {name}: held / un-held ratio of medians {median(ms[f'{name} held']) / median(ms[f'{name} un-held']):.4f}")
