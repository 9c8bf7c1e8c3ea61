"""Tiled sampling (prediff_amd/tiled.py, csrc/tile_blend.hip): the window geometry and its weights, the gather / blend
kernels, and TiledLatentDiffusion against the fp64 restatement in tests/_tiled_ref.py (written from the formulas, not from
prediff_amd.tiled) and against the plain LatentDiffusion where the tiling must not change a bit."""
import functools

import numpy as np
import pytest
import torch

import _dpmpp_ref as R2M
import _templates as TP
import _tiled_ref as R
from _cases import TINY_UNET_CFGS, TINY_VAE_CFG, V1_LDM_KW, V1_UNET_CFG
from _weights import seeded_input, seeded_state_dict
from oracle import diffusion as OD
from oracle import unet as OU
from prediff_amd.tiled import TiledLatentDiffusion, TileGeometry

T = 1000
CFG = TINY_UNET_CFGS["axial"]                 # window 8 x 8, C = 4, T_in = 3, T_out = 2
WINDOW, CANVAS, STRIDE = (8, 8), (12, 13), (4, 4)          # origins y {0, 4}, x {0, 4, 5}: a snapped window, three-fold cover along x
F = 4                                                        # TINY_VAE_CFG's down-sampling factor
# rel-L2 bounds of a 10-step run against the oracle loop, per engine precision, as tests/test_dpmpp_2m.py states them (DDIM10_BOUND);
# the 2M loop's is this times (1 + 2 max_k w_k) of its grid.  The blend is a convex combination: it cannot amplify a window's error.
DDIM10_BOUND = {"fp32": 1e-3, "bf16": 5e-2}
TINY_LDM_KW = dict(layout="NTHWC", data_shape=(2, 32, 32, 1), timesteps=T, use_ema=False, latent_shape=tuple(CFG["target_shape"]),
                   first_stage_model=None, cond_stage_model=None)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _ac_linear():
    return np.cumprod(1.0 - OD.beta_schedule("linear", T)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ CPU: geometry
AXIS_CASES = [(8, 12, 4), (8, 13, 4), (8, 8, 8), (8, 16, 8), (16, 40, 12)]      # (window, canvas, stride) of one axis


@pytest.mark.parametrize("blend", ["feather", "uniform"])
@pytest.mark.parametrize("iy,ix", [(i, (i + 1) % len(AXIS_CASES)) for i in range(len(AXIS_CASES))] + [(2, 2), (1, 1)])
def test_geometry(iy, ix, blend):
    window, canvas, stride = zip(AXIS_CASES[iy], AXIS_CASES[ix])
    geo = TileGeometry(window, canvas, stride, blend)
    org = R.origins(window, canvas, stride)
    assert geo.origins.dtype == torch.int32 and geo.origins.tolist() == [list(o) for o in org] and geo.nwin == len(org)
    ncover = R.cover(window, canvas, org)
    assert ncover.min() >= 1                                                 # the snapped last window: every cell is covered
    ref = R.weights(window, canvas, stride, blend)
    w = geo.weights()
    assert w.dtype == torch.float32 and tuple(w.shape) == (len(org),) + tuple(window)
    assert np.array_equal(w.numpy(), ref.astype(np.float32))                 # fp64 on the host, one rounding to fp32
    total = np.zeros(canvas, dtype=np.float64)
    for k, (y, x) in enumerate(org):
        total[y:y + window[0], x:x + window[1]] += w[k].double().numpy()
    assert (np.abs(total - 1.0) <= ncover * 2.0 ** -23).all()
    for k, (y, x) in enumerate(org):
        single = ncover[y:y + window[0], x:x + window[1]] == 1
        assert (w[k].numpy()[single] == 1.0).all()
    if (iy, ix) == (2, 2):                                                   # canvas = window: one window of weight exactly 1
        assert geo.nwin == 1 and bool((w == 1.0).all())
    # the pixel-scale geometry: the same rule at n = f h, s = f sh, origins f * origin
    pg = geo.scaled(F)
    pw, pc, ps = R.scaled(window, canvas, stride, F)
    assert pg.window == pw and pg.canvas == pc and pg.origins.tolist() == [[F * y, F * x] for y, x in org]
    assert np.array_equal(pg.weights().numpy(), R.weights(pw, pc, ps, blend).astype(np.float32))


def test_the_gpu_tests_geometry():
    assert R.origins_1d(8, 12, 4) == [0, 4] and R.origins_1d(8, 13, 4) == [0, 4, 5]
    assert len(R.origins(WINDOW, CANVAS, STRIDE)) == 6 and R.cover(WINDOW, CANVAS, R.origins(WINDOW, CANVAS, STRIDE)).max() == 6


# ------------------------------------------------------------------------------------------------ CPU: front end
class _NoForward(torch.nn.Module):
    def forward(self, *a):
        raise AssertionError("the denoiser must not run")

    def encode(self, *a):
        raise AssertionError("the VAE must not run")


def _cpu_tiled(canvas=(6, 7), stride=(2, 2), **kw):
    kw = dict(dict(layout="NTHWC", data_shape=(2, 8, 8, 1), timesteps=T, use_ema=False, latent_shape=(2, 4, 4, 1)), **kw)
    return TiledLatentDiffusion(_NoForward(), canvas=canvas, stride=stride, **kw)


def test_refusals():
    rng = torch.get_rng_state()
    for bad in (dict(canvas=(7, 8)), dict(canvas=(8, 7)), dict(stride=(0, 4)), dict(stride=(4, 9)), dict(blend="cosine")):
        with pytest.raises(ValueError):
            TileGeometry(**dict(dict(window=(8, 8), canvas=(12, 13), stride=(4, 4)), **bad))
    with pytest.raises(ValueError, match="smaller"):
        _cpu_tiled(canvas=(3, 7))
    with pytest.raises(NotImplementedError, match="num_timesteps_cond"):
        _cpu_tiled(num_timesteps_cond=4)
    ldm = _cpu_tiled()
    assert ldm.latent_shape == (2, 6, 7, 1) and ldm.data_shape == (2, 12, 14, 1) and ldm.get_batch_latent_shape(3) == (3, 2, 6, 7, 1)
    zc = torch.zeros(2, 3, 6, 7, 1)
    shape = ldm.get_batch_latent_shape(2)
    kw = dict(cond=zc, batch_size=2, return_decoded=False)
    ldm.set_alignment(lambda *a, **k: pytest.fail("the guidance must not run"))
    for sampler in ("ddpm", "ddim", "dpmpp_2m", "dpmpp_2m_sde"):
        with pytest.raises(NotImplementedError, match="use_alignment"):
            ldm.sample(use_alignment=True, sampler=sampler, **kw)
    for loop in (ldm.p_sample_loop, ldm.ddim_sample_loop, ldm.dpmpp_2m_sample_loop, ldm.dpmpp_2m_sde_sample_loop):
        with pytest.raises(NotImplementedError, match="use_alignment"):
            loop(zc, shape, use_alignment=True)
    with pytest.raises(ValueError, match="latent context"):                  # a latent context of the window's size, not the canvas's
        ldm.sample(**dict(kw, cond=torch.zeros(2, 3, 4, 4, 1)))
    vae_ldm = _cpu_tiled(first_stage_model=_NoForward(), cond_stage_model="__is_first_stage__")
    with pytest.raises(ValueError, match="pixel context"):                   # 2 x (6, 7) = (12, 14) is expected
        vae_ldm.sample(cond={"y": torch.zeros(2, 3, 12, 13, 1)}, batch_size=2)
    with pytest.raises(ValueError, match="pixel context"):
        vae_ldm.sample(cond={"y": torch.zeros(2, 3, 6, 7, 1)}, batch_size=2, sampler="ddim")
    # every refusal of the plain samplers stays
    with pytest.raises(NotImplementedError, match="x0"):
        _cpu_tiled(parameterization="x0").sample(sampler="dpmpp_2m", steps=5, **kw)
    with pytest.raises(NotImplementedError, match="clip_denoised"):
        _cpu_tiled(clip_denoised=True).sample(sampler="ddim", ddim_steps=5, **kw)
    with pytest.raises(NotImplementedError, match="inpainting"):
        ldm.sample(mask=torch.ones(shape), x0=torch.zeros(shape), sampler="dpmpp_2m_sde", steps=5, **kw)
    with pytest.raises(NotImplementedError, match="eta"):
        ldm.sample(eta=0.5, sampler="dpmpp_2m", steps=5, **kw)
    with pytest.raises(ValueError, match="steps"):
        ldm.sample(sampler="dpmpp_2m", steps=0, **kw)
    with pytest.raises(ValueError, match="ddim_steps"):
        ldm.sample(sampler="ddim", ddim_steps=0, **kw)
    assert torch.equal(torch.get_rng_state(), rng)                           # refused before any draw


def test_state_dict_schema():
    """The wrapper adds no parameter and no buffer: a plain LatentDiffusion checkpoint loads with strict=True."""
    from prediff_amd import TiledLatentDiffusion as Exported, TileGeometry as ExportedGeometry
    from prediff_amd.autoencoder_kl import AutoencoderKL
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.latent_diffusion import LatentDiffusion
    assert Exported is TiledLatentDiffusion and ExportedGeometry is TileGeometry
    kw = dict(TINY_LDM_KW, use_ema=True, cond_stage_model="__is_first_stage__", scale_by_std=True)
    plain = LatentDiffusion(CuboidTransformerUNet(**CFG, precision="bf16"), first_stage_model=AutoencoderKL(**TINY_VAE_CFG, precision="bf16"),
                            **{k: v for k, v in kw.items() if k != "first_stage_model"})
    tiled = TiledLatentDiffusion(CuboidTransformerUNet(**CFG, precision="bf16"), canvas=CANVAS, stride=STRIDE,
                                 first_stage_model=AutoencoderKL(**TINY_VAE_CFG, precision="bf16"),
                                 **{k: v for k, v in kw.items() if k != "first_stage_model"})
    assert list(tiled.state_dict().keys()) == list(plain.state_dict().keys())
    tiled.load_state_dict(plain.state_dict(), strict=True)
    assert type(tiled.torch_nn_module) is CuboidTransformerUNet
    assert tiled.latent_shape == (2, 12, 13, 4) and tiled.data_shape == (2, 48, 52, 1)
    assert tiled.window_latent_shape == (2, 8, 8, 4) and tiled.geometry.nwin == 6 and tiled.pixel_geometry.window == (32, 32)


# ------------------------------------------------------------------------------------------------ GPU: the kernels
@pytest.mark.gpu
@pytest.mark.parametrize("window,canvas,stride,C", [(WINDOW, CANVAS, STRIDE, 4), (WINDOW, CANVAS, STRIDE, 6), (WINDOW, CANVAS, STRIDE, 1),
                                                    ((32, 32), (48, 52), (16, 16), 1)])
def test_kernels(window, canvas, stride, C):
    """pd_window_gather is the index-slice copy; pd_window_blend against the fp64 restatement (fp64 weights) within
    ncover_max * 2^-23 * max|e|: per canvas element at most ncover_max products by a weight rounded once to fp32 and ncover_max fused
    accumulations rounded once each, of terms whose partial sums stay below max|e| (the weights are non-negative and sum to 1)."""
    from prediff_amd import _lib as L
    B, Tn = 2, 2
    org = R.origins(window, canvas, stride)
    o32 = torch.tensor(org, dtype=torch.int32)
    g = torch.Generator().manual_seed(41)
    z = torch.randn((B, Tn) + canvas + (C,), generator=g)
    e = torch.randn((B, len(org), Tn) + window + (C,), generator=g)
    win = torch.full(tuple(e.shape), float("nan")).cuda()
    L.window_gather(z.cuda(), win, o32)
    assert torch.equal(win.cpu(), R.gather(z, window, org))
    w64 = R.weights(window, canvas, stride)
    w32 = torch.tensor(w64.astype(np.float32)).cuda()
    out = torch.full(tuple(z.shape), float("nan")).cuda()
    L.window_blend(e.cuda(), w32, o32, out)
    ncover_max = int(R.cover(window, canvas, org).max())
    bound = ncover_max * 2.0 ** -23 * float(e.abs().max())
    err = float((out.cpu().double() - R.blend(e, w64, org, canvas)).abs().max())
    print(f"[pd_window_blend {window} on {canvas}, C = {C}] max abs error {err:.3e} (bound {bound:.3e}, {ncover_max}-fold cover)")
    assert err <= bound
    again = torch.full(tuple(z.shape), float("nan")).cuda()
    L.window_blend(e.cuda(), w32, o32, again)
    assert torch.equal(again, out)                                           # no atomics, a fixed order: the same bits
    # the wrappers refuse a table that leaves the canvas, and the blend one that leaves a cell uncovered
    bad = o32.clone()
    bad[-1, 1] += 1
    with pytest.raises(L.PrediffHipError, match="leave the canvas"):
        L.window_gather(z.cuda(), win, bad)
    with pytest.raises(L.PrediffHipError, match="uncovered"):
        L.window_blend(e[:, :-1].contiguous().cuda(), w32[:-1].contiguous(), o32[:-1].contiguous(), out)
    with pytest.raises(L.PrediffHipError):
        L.window_blend(e.cuda(), w32[:-1].contiguous(), o32, out)


# ------------------------------------------------------------------------------------------------ GPU: the module
@functools.lru_cache(maxsize=None)
def _tiny_sd():
    return seeded_state_dict(TP.unet_template(CFG, "tiny_unet_schema.json", "axial"), 600)


def _tiny_net(precision):
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    net = CuboidTransformerUNet(**CFG, precision=precision)
    net.load_state_dict(_tiny_sd())
    return net


def _plain(net, **kw):
    from prediff_amd.latent_diffusion import LatentDiffusion
    ldm = LatentDiffusion(torch_nn_module=net, **dict(TINY_LDM_KW, **kw)).cuda().eval()
    ldm.num_streams = 1
    return ldm


def _tiled(net, canvas=CANVAS, stride=STRIDE, lanes=1, **kw):
    ldm = TiledLatentDiffusion(net, canvas=canvas, stride=stride, **dict(TINY_LDM_KW, **kw)).cuda().eval()
    ldm.num_streams = lanes
    return ldm


def _canvas_inputs(B, canvas, seed, cfg=CFG):
    C = cfg["target_shape"][-1]
    zc = seeded_input("tiled.zc", (B, cfg["input_shape"][0]) + tuple(canvas) + (C,), seed)
    x_T = seeded_input("tiled.xT", (B, cfg["target_shape"][0]) + tuple(canvas) + (C,), seed + 1)
    return zc, x_T


@pytest.mark.gpu
def test_one_window_is_the_plain_sampler():
    """canvas = window: the gather is a copy and the blend multiplies by exactly 1.0, so every sampler gives the plain module's bits."""
    B = 2
    plain, tiled = _plain(_tiny_net("bf16")), _tiled(_tiny_net("bf16"), canvas=WINDOW, stride=WINDOW)
    assert tiled.geometry.nwin == 1 and tiled.latent_shape == plain.latent_shape
    zc, x_T = _canvas_inputs(B, WINDOW, 50)
    g = torch.Generator().manual_seed(51)
    tape = [x_T] + [torch.randn(tuple(x_T.shape), generator=g) for _ in range(5)]
    runs = {"ddim eta 0": dict(sampler="ddim", ddim_steps=5, eta=0.0, x_T=x_T.cuda()),
            "ddim eta 1": dict(sampler="ddim", ddim_steps=5, eta=1.0, noise_tape=tape),
            "dpmpp_2m": dict(sampler="dpmpp_2m", steps=5, x_T=x_T.cuda()),
            "dpmpp_2m_sde": dict(sampler="dpmpp_2m_sde", steps=5, noise_tape=tape),
            "ancestral": dict(timesteps=5, noise_tape=tape)}
    for name, kw in runs.items():
        a = plain.sample(cond=zc.cuda(), batch_size=B, return_decoded=False, **kw)
        b = tiled.sample(cond=zc.cuda(), batch_size=B, return_decoded=False, **kw)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), name


def _disjoint(net, cfg, ldm_kw, canvas, steps, plain_batch):
    from prediff_amd.latent_diffusion import LatentDiffusion
    window = tuple(cfg["target_shape"][1:3])
    tiled = TiledLatentDiffusion(net, canvas=canvas, stride=window, **ldm_kw).cuda().eval()
    plain = LatentDiffusion(torch_nn_module=net, **ldm_kw).cuda().eval()          # the same denoiser: the same launches at the same batch
    tiled.num_streams = plain.num_streams = 1
    org = R.origins(window, canvas, window)
    assert tiled.geometry.nwin == plain_batch == len(org) and int(R.cover(window, canvas, org).max()) == 1
    zc, x_T = _canvas_inputs(1, canvas, 60, cfg)
    kw = dict(return_decoded=False, sampler="ddim", ddim_steps=steps, eta=0.0)
    out = tiled.sample(cond=zc.cuda(), batch_size=1, x_T=x_T.cuda(), **kw)
    ref = plain.sample(cond=R.gather(zc, window, org)[0].cuda(), batch_size=plain_batch, x_T=R.gather(x_T, window, org)[0].cuda(), **kw)
    assert out.shape == (1, cfg["target_shape"][0]) + tuple(canvas) + (cfg["target_shape"][-1],) and bool(torch.isfinite(out).all())
    assert torch.equal(R.gather(out.cpu(), window, org)[0], ref.cpu())


@pytest.mark.gpu
def test_disjoint_windows_are_independent_samples():
    """stride = window: every cell has one window of weight 1.0, so each canvas quadrant is the matching sample of a plain run on the
    batch of gathered windows -- the same denoiser batch, hence bit for bit."""
    _disjoint(_tiny_net("bf16"), CFG, TINY_LDM_KW, (16, 16), 5, 4)


@pytest.mark.gpu
def test_disjoint_windows_at_the_v1_size():
    """The same at the v1 size (two 16 x 16 windows side by side, 3 steps): the pair and Conv3d kernels at batch = nwin under the new path."""
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    net = CuboidTransformerUNet(**V1_UNET_CFG, precision="bf16")
    net.load_state_dict(seeded_state_dict(TP.unet_template(V1_UNET_CFG, "v1_unet_schema.json"), 1234), strict=True)
    _disjoint(net, V1_UNET_CFG, V1_LDM_KW, (16, 32), 3, 2)


@pytest.fixture(scope="module")
def overlap_refs():
    """The restatement loops of test_overlap_vs_restatement_loop, run once: fp64 gather -> the CPU oracle denoiser on every window ->
    fp64 blend in place of the denoiser of the oracle DDIM loop and of the 2M restatement loop."""
    zc, x_T = _canvas_inputs(1, CANVAS, 70)
    den = R.tiled_denoiser(lambda z, t, c: OU.unet_forward(_tiny_sd(), CFG, z, t, c), WINDOW, CANVAS, STRIDE)
    ac = _ac_linear()
    ddim = OD.ddim_sample_loop(ac, den, zc, [x_T] + [torch.zeros_like(x_T)] * 10, 10, eta=0.0)[-1]
    two_m = R2M.sample_loop(ac, den, zc, x_T, 10, "quad")
    return dict(zc=zc, x_T=x_T, ddim=ddim, dpmpp_2m=two_m, factor=R2M.bound_factor(R2M.visits(ac, R2M.grid(10, ac, "quad"))))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_overlap_vs_restatement_loop(overlap_refs, precision):
    """The (12, 13) canvas, six overlapping windows, a latent context canvas: DDIM-10 and 2M-10 (quad grid) against the restatement loops.
    Bounds: the precision's DDIM-10 bound, times (1 + 2 max_k w_k) for 2M, as tests/test_dpmpp_2m.py states them."""
    r = overlap_refs
    ldm = _tiled(_tiny_net(precision))
    kw = dict(cond=r["zc"].cuda(), batch_size=1, return_decoded=False, x_T=r["x_T"].cuda())
    e_ddim = rel_l2(ldm.sample(sampler="ddim", ddim_steps=10, eta=0.0, **kw), r["ddim"])
    e_2m = rel_l2(ldm.sample(sampler="dpmpp_2m", steps=10, **kw), r["dpmpp_2m"])
    print(f"[tiled {precision}] DDIM-10 rel-L2 vs the restatement loop {e_ddim:.3e} (bound {DDIM10_BOUND[precision]:.0e}); "
          f"2M-10 {e_2m:.3e} (bound {DDIM10_BOUND[precision]:.0e} x {r['factor']:.3f})")
    assert e_ddim < DDIM10_BOUND[precision]
    assert e_2m < DDIM10_BOUND[precision] * r["factor"]


def _modes_agree(ldm, label):
    """Lanes (2 and 4 streams), the single graph and the eager loop give the same canvas bit for bit, also on a second call and after a
    run from another x_T (tests/test_dpmpp_2m.py::test_modes_agree_and_replays_are_clean on the canvas)."""
    B = 4
    zc, x_T = (v.cuda() for v in _canvas_inputs(B, CANVAS, 80))
    shape = ldm.get_batch_latent_shape(B)
    assert shape == (B, 2) + CANVAS + (4,)
    kw = dict(cond=zc, batch_size=B, return_decoded=False, sampler="dpmpp_2m", steps=6, lower_order_final=False, x_T=x_T)
    outs = {}
    for lanes in (1, 2, 4):
        ldm.num_streams = lanes
        outs[lanes] = ldm.sample(**kw)
        assert lanes == 1 or 1 in ldm._graphs                             # the second lane's graph: the batch did run as lanes
        assert torch.equal(ldm.sample(**kw), outs[lanes]), lanes
        other = ldm.sample(**dict(kw, x_T=x_T.flip(0)))
        assert not torch.equal(other, outs[lanes]) and torch.equal(ldm.sample(**kw), outs[lanes]), lanes
    ldm.num_streams = 2
    cw = ldm.gather_windows(zc)
    graph, inter = ldm.dpmpp_2m_sample_loop(cw, shape, steps=6, lower_order_final=False, x_T=x_T, return_intermediates=True)
    assert len(inter) == 7 and torch.equal(inter[-1], graph)               # intermediates force the single graph
    ldm.use_hip_graph = False
    eager = ldm.sample(**kw)
    eager_i = ldm.dpmpp_2m_sample_loop(zc, shape, steps=6, lower_order_final=False, x_T=x_T, return_intermediates=True)[1]
    assert bool(torch.isfinite(eager).all())
    print(f"[tiled modes, {label}] rel-L2 to the eager loop: one lane {rel_l2(outs[1], eager):.3e}, two lanes {rel_l2(outs[2], eager):.3e}, "
          f"four lanes {rel_l2(outs[4], eager):.3e}, the single graph {rel_l2(graph, eager):.3e}; two lanes to four {rel_l2(outs[2], outs[4]):.3e}")
    assert torch.equal(outs[1], eager) and torch.equal(graph, eager)
    assert len(eager_i) == len(inter) and all(torch.equal(a, b) for a, b in zip(inter, eager_i))
    assert torch.equal(outs[2], eager) and torch.equal(outs[4], eager)


@pytest.mark.gpu
def test_modes_agree_and_replays_are_clean():
    """B = 4 canvases of six windows, bf16, 2M with 6 steps, the engine's default settings: 24 windows per denoiser launch in one lane, 12 in
    two, 6 in four.  The denoiser's small-batch mode (CuboidTransformerUNet._splitk_mode: at most SPLITK_MAX_BATCH = 16 trajectories per
    launch, another fp32 summation order) would put these on both sides of its threshold -- 3.5e-3 rel-L2 between one lane and two was
    measured with the mode chosen per launch -- so TiledLatentDiffusion chooses it from the windows of the whole call
    (_pins_batch_mode): every mode agrees bit for bit, the module's own split_k setting is left as it was, and a later call small
    enough for the small-batch mode does not replay a step captured in the other one."""
    net = _tiny_net("bf16")
    ldm = _tiled(net)
    _modes_agree(ldm, "bf16")
    assert net.split_k is True
    # 2 canvases = 12 windows in the call: the small-batch mode, on a module whose lane-0 graph was captured for 2 canvases of a call of 24
    ldm.use_hip_graph, ldm.num_streams = True, 2
    zc, x_T = (v.cuda() for v in _canvas_inputs(4, CANVAS, 80))
    kw = dict(batch_size=2, return_decoded=False, sampler="dpmpp_2m", steps=6, lower_order_final=False)
    ldm.sample(cond=zc, **dict(kw, batch_size=4, x_T=x_T))
    ldm.num_streams = 1
    small = ldm.sample(cond=zc[:2], x_T=x_T[:2], **kw)
    fresh = _tiled(_tiny_net("bf16")).sample(cond=zc[:2], x_T=x_T[:2], **kw)
    assert torch.equal(small, fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_modes_agree_in_the_reproducible_modes(precision):
    """The same with the engine's batch-split-reproducible settings: bf16 with torch_nn_module.split_k = False, and fp32 (which never
    splits K): no kernel choice depends on the number of windows per launch there."""
    net = _tiny_net(precision)
    net.split_k = False
    _modes_agree(_tiled(net), f"{precision}, split_k = False")


@pytest.mark.gpu
@pytest.mark.parametrize("split_k", [False, True])
def test_window_chunks_give_the_same_bits(split_k):
    """max_windows_per_call = 3 (24 windows in 8 denoiser calls) against one call: the same bits, captured and eager, in the engine's
    batch-split-reproducible mode (torch_nn_module.split_k = False) and, the call being one of 24 windows, with its default too."""
    B = 4
    net = _tiny_net("bf16")
    net.split_k = split_k
    ldm = _tiled(net)
    zc, x_T = (v.cuda() for v in _canvas_inputs(B, CANVAS, 80))
    kw = dict(cond=zc, batch_size=B, return_decoded=False, sampler="dpmpp_2m", steps=6, lower_order_final=False, x_T=x_T)
    whole = ldm.sample(**kw)
    ldm.max_windows_per_call = 3
    assert not ldm._graphs                                                    # the captured step is dropped with its chunking
    assert torch.equal(ldm.sample(**kw), whole)
    ldm.use_hip_graph = False
    assert torch.equal(ldm.sample(**kw), whole)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_tiled_vae(precision):
    """The new code around the VAE (its own accuracy: test_hip_vae.py).  Encode: the tiled conditioning forward is the plain module's on
    the gathered 32 x 32 context tiles (one VAE call, the same frame batch), bit for bit.  Decode: the blend of the plain module's decoded
    windows, within the blend bound of test_kernels at pixel scale."""
    from prediff_amd.autoencoder_kl import AutoencoderKL
    vae = AutoencoderKL(**TINY_VAE_CFG, precision=precision)
    vae.load_state_dict(seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 601))
    kw = dict(first_stage_model=vae, cond_stage_model="__is_first_stage__", scale_factor=0.7)
    net = _tiny_net(precision)
    plain, tiled = _plain(net, **kw), _tiled(net, **kw)
    pw, pc, ps = R.scaled(WINDOW, CANVAS, STRIDE, F)
    assert (pw, pc) == ((32, 32), (48, 52)) and tiled.downsample_factor == F
    porg, org = R.origins(pw, pc, ps), R.origins(WINDOW, CANVAS, STRIDE)
    ctx = seeded_input("tiled.ctx", (1, 3) + pc + (1,), 90, kind="uniform")
    zc = tiled.cond_stage_forward({"y": ctx.cuda()})
    assert zc.shape == (1, 6, 3, 8, 8, 4)
    assert torch.equal(zc[0], plain.cond_stage_forward({"y": R.gather(ctx, pw, porg)[0].cuda()}))
    z = seeded_input("tiled.z", (1, 2) + CANVAS + (4,), 91)
    dec = tiled.decode_first_stage(z.cuda())
    tiles = plain.decode_first_stage(R.gather(z, WINDOW, org)[0].cuda()).cpu()
    assert dec.shape == (1, 2) + pc + (1,) and tiles.shape == (6, 2, 32, 32, 1)
    bound = int(R.cover(pw, pc, porg).max()) * 2.0 ** -23 * float(tiles.abs().max())
    err = float((dec.cpu().double() - R.blend(tiles[None], R.weights(pw, pc, ps), porg, pc)).abs().max())
    print(f"[tiled decode {precision}] max abs error vs the fp64 blend {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # end to end: pixel context canvas in, pixel canvas out
    out = tiled.sample(cond={"y": ctx.cuda()}, batch_size=1, sampler="ddim", ddim_steps=2)
    assert out.shape == (1, 2) + pc + (1,) and bool(torch.isfinite(out).all())


@pytest.mark.gpu
def test_ensemble_is_batch_split_invariant():
    """sample_ensemble on the canvas, the stochastic 2M solver: a member depends on (base_seed, member id) only -- its canvas-shaped
    draws come from its own generator -- so micro-batches of 2 and 4 agree bit for bit (fp32 engine: the reproducible setting of
    tests/test_dpmpp_2m_sde.py::test_ensemble_is_batch_split_invariant)."""
    from prediff_amd.ensemble import sample_ensemble
    ldm = _tiled(_tiny_net("fp32"), lanes=2)
    zc, _ = _canvas_inputs(1, CANVAS, 95)
    kw = dict(base_seed=1000, sampler="dpmpp_2m_sde", eta=1.0, steps=5, return_decoded=False)
    a = sample_ensemble(ldm, zc.cuda(), 4, micro_batch=4, **kw)
    b = sample_ensemble(ldm, zc.cuda(), 4, micro_batch=2, **kw)
    assert a.shape == (4, 2) + CANVAS + (4,) and bool(torch.isfinite(a).all())
    print(f"[tiled ensemble 2M-SDE-5] micro_batch 4 vs 2 rel-L2 {rel_l2(b, a):.3e}")
    assert torch.equal(a, b)
    assert rel_l2(a[0], a[1]) > 1e-2            # members differ
