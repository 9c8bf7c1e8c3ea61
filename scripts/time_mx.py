"""MX (block-scaled e4m3) against the bf16 and the unit-scale e4m3 engines at the v1 configuration, one process (run on the GPU box;
log to profiles/time_mx.log):
  A. the step: 64 trajectories in two lanes, DDIM-50 latent loop, precision "bf16" / "fp8" / "mxfp8" interleaved REPS times, steps / s;
  B. one Conv3d launch at the level-0 (16 x 16 x 256) and level-1 (8 x 8 x 512) shapes of 32 trajectories, unit-scale e4m3 (pd_igemm,
     fp8) against MX (pd_igemm_mx), interleaved, event-timed, us per launch;
  C. (--ddim50) DDIM-50 rel-L2 of "mxfp8" / "mxfp8_conv" (and "bf16", "fp8_conv", "fp8" beside them) against the oracle loop on the CPU,
     one trajectory, on the inputs of tests/test_hip_configs.py::test_v1_ddim50_vs_oracle, which measures the README column."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from prediff_amd import _lib as L
from prediff_amd.presets import V1_UNET_CFG
from prediff_amd.seeding import seeded_state_dict
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
from prediff_amd.latent_diffusion import LatentDiffusion
from prediff_amd.packing import pack_conv_fp8, pack_conv_mx, quantize_mx, to_fp8

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = max(3, int(args[0])) if args else 3
dev = torch.device("cuda")
PRECISIONS = ("bf16", "fp8", "mxfp8")


def make_ldm(precision):
    net = CuboidTransformerUNet(**V1_UNET_CFG, precision=precision)
    net.load_state_dict(seeded_state_dict(net.state_dict(), 1234))
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(6, 128, 128, 1), timesteps=1000, beta_schedule="linear",
                          use_ema=False, latent_shape=(6, 16, 16, 64), first_stage_model=None, cond_stage_model=None,
                          scale_factor=1.0).to(dev).eval()
    ldm.num_streams = 2
    return ldm


def spread(v):
    return f"min {min(v):.1f} median {sorted(v)[len(v) // 2]:.1f} max {max(v):.1f}"


with torch.no_grad():
    B, N = 64, 50
    ldms = {p: make_ldm(p) for p in PRECISIONS}
    zc = torch.randn(B, 7, 16, 16, 64, device=dev)
    shape = ldms["bf16"].get_batch_latent_shape(B)
    x_T = torch.randn(shape, device=dev)
    sps = {p: [] for p in PRECISIONS}
    for rep in range(REPS):
        for p, ldm in ldms.items():
            ldm.ddim_sample_loop(zc, shape, ddim_steps=2, eta=0.0, x_T=x_T)          # untimed: graph capture, workspaces
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = ldm.ddim_sample_loop(zc, shape, ddim_steps=N, eta=0.0, x_T=x_T)
            torch.cuda.synchronize(); t = time.perf_counter() - t0
            assert bool(torch.isfinite(out).all())
            sps[p].append(B * N / t)
            print(f"A rep {rep} {p}: {N} steps, {B} trajectories in 2 lanes: {B * N / t:.0f} steps / s")
    for p, v in sps.items():
        print(f"A {p}: steps / s {spread(v)}")
    del ldms

    for level, (T, H, W, C) in enumerate(((13, 16, 16, 256), (13, 8, 8, 512))):
        Bt = 32
        M = Bt * T * H * W
        g = torch.Generator().manual_seed(level)
        x = torch.randn(M, C, generator=g).to(dev)
        wt = (torch.randn(C, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5).to(dev)
        geom = L.conv_geom(Bt, (T, H, W), (3, 3, 3))
        out = torch.empty(M, C, device=dev)
        a8, (w8, sw) = to_fp8(x, 16.0), pack_conv_fp8(wt)
        (am, sa), (wm, swm) = quantize_mx(x), pack_conv_mx(wt)
        forms = {"unit-scale e4m3": lambda: L.igemm(a8, w8, M=M, N=C, Cin=C, taps=27, w_tap_stride=C * C, geom=geom, alpha=1.0 / (16.0 * sw), out_f32=out, fp8=True),
                 "MX": lambda: L.igemm_mx(am, sa, wm, swm, M=M, N=C, taps=27, geom=geom, out_f32=out)}
        us = {k: [] for k in forms}
        for rep in range(REPS):
            for k, fn in forms.items():
                for _ in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record(); torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / 20)
        for k, v in us.items():
            print(f"B level {level} Conv3d {C} -> {C}, {Bt} trajectories, {k}: us / launch {spread(v)}")
        print(f"B level {level}: ratio of medians MX / unit-scale {sorted(us['MX'])[REPS // 2] / sorted(us['unit-scale e4m3'])[REPS // 2]:.4f}")

    if "--ddim50" in sys.argv:
        from oracle import diffusion as OD
        from oracle import unet as OU
        from prediff_amd.seeding import seeded_input
        # the inputs, the noise tape and the thread count of tests/test_hip_configs.py::test_v1_ddim50_vs_oracle (the README column)
        zc1 = seeded_input("d50c", (1, 7, 16, 16, 64), 21)
        xT = seeded_input("d50x", (1, 6, 16, 16, 64), 22)
        sd = {k: v.cpu() for k, v in make_ldm("bf16").torch_nn_module.state_dict().items()}
        ac = np.cumprod(1.0 - OD.beta_schedule("linear", 1000)).astype(np.float32)
        nthr = torch.get_num_threads()
        torch.set_num_threads(min(nthr, 32))
        t0 = time.time()
        traj = OD.ddim_sample_loop(ac, lambda z, t, c: OU.unet_forward(sd, V1_UNET_CFG, z, t, c), zc1, [xT] + [torch.zeros_like(xT)] * 50, 50, eta=0.0)
        torch.set_num_threads(nthr)
        t_cpu = time.time() - t0
        ref, outs = traj[-1].double(), {}
        for p in ("bf16", "fp8_conv", "fp8", "mxfp8_conv", "mxfp8"):
            ldm = make_ldm(p)
            outs[p] = ldm.sample(cond=zc1.to(dev), batch_size=1, sampler="ddim", ddim_steps=50, eta=0.0, x_T=xT.to(dev), return_decoded=False).cpu()
            assert bool(torch.isfinite(outs[p]).all())
            del ldm
        errs = ", ".join(f"{p} {float((o.double() - ref).norm() / ref.norm()):.3e}" for p, o in outs.items())
        print(f"C DDIM-50 rel-L2 against the oracle loop, one trajectory: {errs} (oracle {t_cpu:.0f} s on the CPU)")
        print(f"C mxfp8 and mxfp8_conv give the same bits: {torch.equal(outs['mxfp8'], outs['mxfp8_conv'])}"
              " (v1: the pair kernel takes every level-1 block, no LayerNorm-fed linear is left to MX)")
