"""The final latent of every fast-sampler arm as a SHA-256, to compare two source trees bit for bit (run on the GPU box):
    python scripts/sampler_bits.py [LABEL] > profiles/sampler_bits.txt
Only the public API is used (sample, num_streams, aligned_lanes, use_hip_graph, set_alignment), so the same file runs on an older tree.
Models: the tests' tiny fp32 U-Net (tests/_cases.py, "axial"; fp32 never splits K and is bit-reproducible) with four target frames, and
with its own two next to the tiny alignment network for the guided arms.  B = 4, 5 steps, one fixed noise tape.  Arms: the three
samplers, eta in {0, 1} where the sampler takes it, x {plain, guided, held "fresh", held "fixed", guided + held} x {two lanes, one graph,
eager}.  The first line carries LABEL; every other line must be the same on both trees."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _cases import TINY_ALIGN_ARGS, TINY_UNET_CFGS  # noqa: E402
from prediff_amd.alignment import SEVIRAvgIntensityAlignment  # noqa: E402
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet  # noqa: E402
from prediff_amd.latent_diffusion import LatentDiffusion  # noqa: E402
from prediff_amd.seeding import seeded_state_dict  # noqa: E402

B, STEPS, SEED = 4, 5, 2024
dev = torch.device("cuda")


def tiny_ldm(frames):
    cfg = dict(TINY_UNET_CFGS["axial"], target_shape=[frames, 8, 8, 4])
    net = CuboidTransformerUNet(**cfg, precision="fp32")
    net.load_state_dict(seeded_state_dict(net.state_dict(), 600))
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(frames, 32, 32, 1), timesteps=1000, use_ema=False,
                          latent_shape=tuple(cfg["target_shape"]), first_stage_model=None, cond_stage_model=None)
    return ldm.to(dev).eval(), cfg


def arms_of(ldm, cfg, guided):
    gen = torch.Generator().manual_seed(SEED + int(guided))
    shape = ldm.get_batch_latent_shape(B)
    zc = torch.randn((B,) + tuple(cfg["input_shape"]), generator=gen).to(dev)
    tape = [torch.randn(shape, generator=gen) for _ in range(1 + 2 * STEPS)]
    mask = torch.zeros((1, shape[1], 1, 1, 1), device=dev)
    mask[:, :shape[1] // 2] = 1.0
    hold = dict(hold_mask=mask, hold_x0=torch.randn(shape, generator=gen).to(dev))
    align = dict(use_alignment=True, alignment_kwargs={"avg_x_gt": torch.tensor([[0.4], [0.1], [0.3], [0.2]], device=dev)})
    if guided:
        variants = {"guided": align, "guided+held": dict(align, **hold)}
    else:
        variants = {"plain": {}, "held fresh": dict(hold, hold_noise="fresh"), "held fixed": dict(hold, hold_noise="fixed")}
    for sampler, etas in (("ddim", (0.0, 1.0)), ("dpmpp_2m", (None,)), ("dpmpp_2m_sde", (0.0, 1.0))):
        for eta in etas:
            for name, kw in variants.items():
                for mode, (lanes, graph) in {"two lanes": (2, True), "one graph": (1, True), "eager": (1, False)}.items():
                    ldm.num_streams = ldm.aligned_lanes = lanes
                    ldm.use_hip_graph = graph
                    torch.manual_seed(SEED)
                    out = ldm.sample(cond=zc, batch_size=B, return_decoded=False, sampler=sampler, ddim_steps=STEPS, noise_tape=tape,
                                     **({} if eta is None else {"eta": eta}), **kw)
                    torch.cuda.synchronize()
                    assert bool(torch.isfinite(out).all())
                    digest = hashlib.sha256(out.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
                    print(f"{sampler} eta={eta} | {name} | {mode} | {digest}", flush=True)


print(f"# sampler_bits: {sys.argv[1] if len(sys.argv) > 1 else 'this tree'}", flush=True)
with torch.no_grad():
    arms_of(*tiny_ldm(4), guided=False)
    ldm2, cfg2 = tiny_ldm(2)
    al = SEVIRAvgIntensityAlignment(alignment_type="avg_x", guide_scale=50.0, model_type="cuboid", model_args=dict(TINY_ALIGN_ARGS))
    al.model.load_state_dict(seeded_state_dict(al.model.state_dict(), 700))
    al.model.to(dev)
    ldm2.set_alignment(al.get_mean_shift)
    arms_of(ldm2, cfg2, guided=True)
