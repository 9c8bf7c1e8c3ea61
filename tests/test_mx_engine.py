"""GPU: precision="mxfp8_conv" / "mxfp8" of CuboidTransformerUNet (MX block-scaled e4m3 operands) against the CPU oracle on tiny
configurations at B = 2, the ordering against the per-tensor-scaled "fp8_conv" engine on heavy-tailed weights, and DDIM-10 through
sample() with HIP graphs and two lanes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _cases import TINY_UNET_CFGS  # noqa: E402
from _weights import heavy_tailed_state_dict, seeded_input, seeded_state_dict  # noqa: E402
from oracle import unet as OU  # noqa: E402
from prediff_amd import _lib as L  # noqa: E402
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet  # noqa: E402
from prediff_amd.latent_diffusion import LatentDiffusion  # noqa: E402

# "axial": the tiny configuration as it is (64 / 128 channels; the 128-channel ResBlock convolutions are MX launches -- at 64 channels
# in 32 groups pd_groupnorm_silu_mx has no vector form, as pd_groupnorm_silu_fp8 has none, and the layer keeps 16-bit operands).
# "axial256": the same at 256 / 512 units and 4 heads -- level 1 has the K >= 512 LayerNorm-fed linears (qkv, FFN-1) that "mxfp8" adds;
# the tests switch the pair kernel off there, which otherwise takes those blocks whole (as it does for precision="fp8").
CFGS = {"axial": TINY_UNET_CFGS["axial"], "axial256": dict(TINY_UNET_CFGS["axial"], base_units=256, num_heads=4)}
_CACHE = {}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _case(name, heavy=False):
    """seeded weights, inputs (B = 2) and the oracle's CPU forward of a configuration, computed once"""
    key = (name, heavy)
    if key not in _CACHE:
        cfg = CFGS[name]
        tmpl = CuboidTransformerUNet(**cfg).state_dict()
        sd = heavy_tailed_state_dict(tmpl, 77) if heavy else seeded_state_dict(tmpl, 451)
        x = seeded_input(name + "mx_x", (2,) + tuple(cfg["target_shape"]), 2)
        cond = seeded_input(name + "mx_c", (2,) + tuple(cfg["input_shape"]), 3)
        t = torch.tensor([7, 431])
        with torch.no_grad():
            ref = OU.unet_forward(sd, cfg, x, t, cond)
        assert bool(torch.isfinite(ref).all())
        _CACHE[key] = (cfg, sd, x, t, cond, ref)
    return _CACHE[key]


def _forward(name, precision, heavy=False, count=None):
    cfg, sd, x, t, cond, ref = _case(name, heavy)
    net = CuboidTransformerUNet(**cfg, precision=precision)
    net.load_state_dict(sd, strict=True)
    net.fuse_pair = False                  # (axial256: the level-1 linears as separate launches; no effect at 64 / 128 units)
    real = L.igemm_mx
    if count is not None:
        L.igemm_mx = lambda *a, **k: (count.append(k["N"]), real(*a, **k))[1]
    try:
        out = net.cuda()(x.cuda(), t.cuda(), cond.cuda())
    finally:
        L.igemm_mx = real
    assert bool(torch.isfinite(out).all())
    if count is not None:
        count.append([k for k in net._packed if k.endswith(".wmx")])
    return out, ref


# rel-L2 of one forward against the oracle, measured on the MI355X (also DESIGN.md section 5); the bounds are 3x, rounded up.
#   axial:    mxfp8_conv 2.933e-2, mxfp8 2.933e-2 (the same launches: no K >= 512 linear)
#   axial256: mxfp8_conv 3.938e-2, mxfp8 5.035e-2
BOUND = {("axial", "mxfp8_conv"): 9e-2, ("axial", "mxfp8"): 9e-2, ("axial256", "mxfp8_conv"): 0.12, ("axial256", "mxfp8"): 0.16}
SANITY = {"mxfp8_conv": 8e-2, "mxfp8": 0.14}      # the "fp8_conv" / "fp8" bounds of test_hip_configs.py: block scaling must not be worse


@pytest.mark.parametrize("precision", ["mxfp8_conv", "mxfp8"])
@pytest.mark.parametrize("name", list(CFGS))
def test_mx_unet_vs_oracle(name, precision):
    calls = []
    out, ref = _forward(name, precision, count=calls)
    recs = calls.pop()
    e = rel_l2(out, ref)
    print(f"[{name} {precision}] one forward rel-L2 vs oracle {e:.3e}; {len(calls)} MX launches")
    assert len(calls) == len(recs) > 0                         # every MX record is launched (depth 1: once each), nothing else is
    if name == "axial256":
        assert all(k + ".wmx" in recs for k in ("first.conv2", "dte0.conv1", "dte0.conv2", "ute1.conv1", "ute1.conv2"))
        lin = [n for n in calls if n in (3 * 512, 4 * 512)]    # qkv and FFN-1 of the 512-unit level
        assert (len(lin) == 12) == (precision == "mxfp8") and (len(lin) == 0) == (precision == "mxfp8_conv")
    assert e <= SANITY[precision]
    assert e <= BOUND[name, precision]


def test_mx_against_per_tensor_scales_on_heavy_tailed_weights():
    """Student-t(3) weights with 30x outlier channels (seeding.heavy_tailed_state_dict): one scale per 32 channels against one per
    tensor, on the same convolutions ("axial256": both engines run every ResBlock convolution but the stem's first on e4m3).
    Measured on the MI355X: bf16 2.183e-2, fp8_conv 7.314e-2, mxfp8_conv 7.636e-2 -- the ordering mxfp8_conv < fp8_conv does NOT hold on
    this network, so it is not asserted: finite, and within the "fp8_conv" bound on such weights."""
    errs = {}
    for precision in ("bf16", "fp8_conv", "mxfp8_conv"):
        out, ref = _forward("axial256", precision, heavy=True)
        errs[precision] = rel_l2(out, ref)
    print(f"[axial256 heavy-tailed] rel-L2 vs oracle: bf16 {errs['bf16']:.3e}, fp8_conv {errs['fp8_conv']:.3e}, mxfp8_conv {errs['mxfp8_conv']:.3e}")
    assert all(np.isfinite(v) for v in errs.values())
    assert errs["mxfp8_conv"] < 0.3                            # the "fp8_conv" bound on such weights (test_hip_unet.py HEAVY_BOUND)


def test_mxfp8_ddim10_graphs_and_lanes():
    """"axial256" with the pair kernel off: the LayerNorm-fed level-1 linears are MX launches of their own (pd_layernorm_mx + pd_igemm_mx),
    so that they, and not only the convolutions, are captured in a HIP graph and run in two lanes."""
    cfg = CFGS["axial256"]
    sd = seeded_state_dict(CuboidTransformerUNet(**cfg).state_dict(), 600)
    net = CuboidTransformerUNet(**cfg, precision="mxfp8")
    net.load_state_dict(sd)
    net.fuse_pair = False
    T_out, H, W, C = cfg["target_shape"]
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(T_out, H * 4, W * 4, 1), timesteps=1000, beta_schedule="linear",
                          use_ema=False, latent_shape=tuple(cfg["target_shape"]), first_stage_model=None, cond_stage_model=None,
                          scale_factor=1.0).cuda().eval()
    B = 4
    zc = seeded_input("mxzc", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    g = torch.Generator().manual_seed(17)
    tape = [torch.randn(ldm.get_batch_latent_shape(B), generator=g) for _ in range(11)]
    kw = dict(cond=zc, batch_size=B, return_decoded=False, sampler="ddim", ddim_steps=10, eta=1.0, noise_tape=tape)
    real, widths = L.igemm_mx, []
    L.igemm_mx = lambda *a, **k: (widths.append(k["N"]), real(*a, **k))[1]
    try:
        outs = {}
        for lanes in (1, 2):
            ldm.num_streams = lanes
            widths.clear()
            outs[lanes] = ldm.sample(**kw)
            assert any(n in (3 * 512, 4 * 512) for n in widths)    # qkv / FFN-1 of the 512-unit level went into the capture as MX launches
        ldm.num_streams, ldm.use_hip_graph = 1, False
        eager = ldm.sample(**kw)
    finally:
        L.igemm_mx = real
    assert bool(torch.isfinite(outs[2]).all())
    assert torch.equal(outs[2], outs[1]) and torch.equal(outs[1], eager)
