"""Rolling forecasts on the device (prediff_amd/rollout.py, csrc/rollout.hip): pd_context_advance against the numpy
restatement in tests/_rollout_ref.py, and rollout_sample / rollout_ensemble against hand-written chains over the public loops, bit for bit.

Mode agreement: in every comparison both sides run on the same module with the same settings (one lane, graphs as configured), so both take
the same driver mode at every segment and torch.equal is a fair demand.  Tiny configurations (T_in = 3, T_out = 2), at most 3 sampler
steps; with out_len = 2 the issue's "stride = out_len" and "stride = 2" coincide, so the shorter stride tested is 1."""
import functools

import numpy as np
import pytest
import torch

import _rollout_ref as R
import _templates as TP
from _cases import TINY_UNET_CFGS, TINY_VAE_CFG
from _weights import seeded_input, seeded_state_dict
from prediff_amd.rollout import RolloutPlan, rollout_ensemble, rollout_sample
from prediff_amd.tiled import TiledLatentDiffusion, TileGeometry

pytestmark = pytest.mark.gpu

T = 1000
CFG = TINY_UNET_CFGS["axial"]                          # window 8 x 8, C = 4, T_in = 3, T_out = 2
CFG4 = dict(CFG, input_shape=[3, 4, 4, 4], target_shape=[2, 4, 4, 4])      # the same tiny architecture on a 4 x 4 window (canvas (6, 7))
T_IN, T_OUT = CFG["input_shape"][0], CFG["target_shape"][0]
SF = 0.18215
GUARD = 64                                              # floats on each side of an output buffer (a multiple of 4: alignment is kept)
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the kernel
def _guarded(shape, misalign=0):
    """A NaN-filled flat buffer and its view of `shape` with GUARD floats before and after (and `misalign` floats of offset)."""
    n = int(np.prod(shape))
    flat = torch.full((GUARD + misalign + n + GUARD,), NAN, device="cuda")
    return flat, flat[GUARD + misalign:GUARD + misalign + n].view(shape)


def _guards_untouched(flat, view, misalign=0):
    n = view.numel()
    return bool(torch.isnan(flat[:GUARD + misalign]).all()) and bool(torch.isnan(flat[GUARD + misalign + n:]).all())


def _advance_case(B, T_in, T_out, s, canvas, window, origins, C, z_scale, misalign, variant, seed):
    from prediff_amd import _lib as L
    nwin = len(origins)
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn((B, nwin, T_in) + window + (C,), generator=g)
    z = torch.randn((B, T_out) + canvas + (C,), generator=g)
    zflat, zdev = _guarded(tuple(z.shape), misalign)
    zdev.copy_(z)
    assert zdev.data_ptr() % 16 == 4 * misalign
    nflat, nxt = _guarded(tuple(ctx.shape))
    f_T = T_out + 3
    f_off, f_cnt = {"none": (0, 0), "kept": (0, s), "short": (2, s - 1)}[variant]
    fflat, fc = (None, None) if variant == "none" else _guarded((B, f_T) + canvas + (C,))
    L.context_advance(ctx.cuda(), zdev, torch.tensor(origins, dtype=torch.int32), nxt, s, z_scale, forecast=fc, f_off=f_off, f_cnt=f_cnt)
    torch.cuda.synchronize()
    label = (B, T_in, T_out, s, canvas, window, C, float(z_scale), misalign, variant)
    ref = torch.from_numpy(R.advance(ctx.numpy(), z.numpy(), z_scale, s, origins))
    assert not bool(torch.isnan(nxt).any()) and torch.equal(nxt.cpu(), ref), label
    assert _guards_untouched(nflat, nxt), label
    assert torch.equal(zdev.cpu(), z), label                                  # the inputs are only read
    if fc is not None:
        assert _guards_untouched(fflat, fc), label
        assert torch.equal(fc[:, f_off:f_off + f_cnt].cpu(), z[:, :f_cnt]), label                 # unscaled, bit for bit
        assert bool(torch.isnan(fc[:, :f_off]).all()) and bool(torch.isnan(fc[:, f_off + f_cnt:]).all()), label      # nothing else


TS_CASES = [(3, 2, 1), (3, 2, 2), (2, 3, 1), (2, 3, 2), (2, 3, 3)]          # (T_in, T_out, stride): every stride; (2, 3, 3) is z alone
Z_SCALES = (1.0, 0.5, float(np.float32(1.0 / 0.18215)))


@pytest.mark.parametrize("C,misalign", [(8, 0), (6, 0), (1, 0), (8, 1)])
def test_context_advance_plain(C, misalign):
    """B = 2, 4 x 4, one window at the origin: the float4 path (C = 8), the scalar path (C = 6, C = 1) and the scalar path on a base that
    is one float off a 16-byte boundary.  NaN-filled outputs between guard rows; torch.equal against the restatement."""
    seed = 100
    for T_in, T_out, s in TS_CASES:
        for z_scale in Z_SCALES:
            for variant in ("none", "kept", "short"):
                seed += 1
                _advance_case(2, T_in, T_out, s, (4, 4), (4, 4), [(0, 0)], C, z_scale, misalign, variant, seed)


@pytest.mark.parametrize("C,misalign", [(8, 0), (6, 0), (1, 0), (8, 1)])
def test_context_advance_windowed(C, misalign):
    """Canvas 6 x 7, window 4 x 4, stride (2, 2): six overlapping windows, the last column snapped to the border; B = 2 (several blocks)."""
    geo = TileGeometry((4, 4), (6, 7), (2, 2))
    origins = [tuple(o) for o in geo.origins.tolist()]
    assert origins == [(0, 0), (0, 2), (0, 3), (2, 0), (2, 2), (2, 3)]
    seed = 200
    for T_in, T_out, s in TS_CASES:
        for z_scale in Z_SCALES:
            for variant in ("none", "kept", "short"):
                seed += 1
                _advance_case(2, T_in, T_out, s, (6, 7), (4, 4), origins, C, z_scale, misalign, variant, seed)


def test_context_advance_past_2_31_bytes():
    """Element offsets are 64-bit: a window stack of 2.31e9 bytes and a forecast buffer of 2.6e9 (two 64 x 64 windows on a 64 x 96 canvas,
    C = 64, B = 550), compared on the device against index slices and one fp32 multiply.  (2^31 ELEMENTS would take 8.6 GB per buffer:
    the index arithmetic is the same int64 expressions, so that size is not run.)"""
    from prediff_amd import _lib as L
    B, C, s, scale = 550, 64, 1, float(np.float32(1.0 / 0.18215))
    origins = [(0, 0), (0, 32)]
    g = torch.Generator(device="cuda").manual_seed(7)
    ctx = torch.randn((B, 2, 2, 64, 64, C), generator=g, device="cuda")
    z = torch.randn((B, 2, 64, 96, C), generator=g, device="cuda")
    assert ctx.numel() * 4 > 2 ** 31
    nxt = torch.full(tuple(ctx.shape), NAN, device="cuda")
    fc = torch.full((B, 3, 64, 96, C), NAN, device="cuda")
    L.context_advance(ctx, z, torch.tensor(origins, dtype=torch.int32), nxt, s, scale, forecast=fc, f_off=2, f_cnt=1)
    assert torch.equal(nxt[:, :, 0], ctx[:, :, 1])
    for k, (y, x) in enumerate(origins):
        assert torch.equal(nxt[:, k, 1], z[:, 0, y:y + 64, x:x + 64] * scale), k
    assert torch.equal(fc[:, 2], z[:, 0]) and bool(torch.isnan(fc[:, :2]).all())


def test_context_advance_refusals():
    from prediff_amd import _lib as L
    o = torch.zeros((1, 2), dtype=torch.int32)
    ctx, z = torch.zeros(2, 1, 3, 4, 4, 8).cuda(), torch.zeros(2, 2, 4, 4, 8).cuda()
    nxt, fc = torch.empty_like(ctx), torch.empty(2, 5, 4, 4, 8).cuda()
    L.context_advance(ctx, z, o, nxt, 2, 1.0, forecast=fc, f_off=3, f_cnt=2)                      # the well-formed call
    both, zn = torch.zeros(2 * ctx.numel() - 8).cuda(), torch.zeros(z.numel() + ctx.numel() - 8).cuda()
    cases = {"an aliased ctx_next": dict(ctx_next=ctx), "ctx_next overlapping ctx": dict(ctx=both[:ctx.numel()].view(ctx.shape),
                                                                                         ctx_next=both[ctx.numel() - 8:].view(ctx.shape)),
             "ctx_next overlapping z": dict(z=zn[:z.numel()].view(z.shape), ctx_next=zn[z.numel() - 8:].view(ctx.shape)),
             "forecast on z": dict(forecast=z.view(2, 2, 4, 4, 8), f_cnt=1),
             "stride 0": dict(stride=0), "stride T_out + 1": dict(stride=3), "f_off + f_cnt > f_T": dict(f_off=4, f_cnt=2),
             "f_cnt > T_out": dict(f_off=0, f_cnt=3), "f_cnt without a buffer": dict(forecast=None, f_cnt=1),
             "a CPU ctx": dict(ctx=ctx.cpu()), "a CPU z": dict(z=z.cpu()), "a CPU ctx_next": dict(ctx_next=nxt.cpu()),
             "a CPU forecast": dict(forecast=fc.cpu()), "a wrong ctx_next shape": dict(ctx_next=torch.empty(2, 1, 2, 4, 4, 8).cuda()),
             "a wrong z": dict(z=torch.zeros(2, 2, 4, 4, 4).cuda()), "a wrong forecast": dict(forecast=torch.empty(2, 5, 4, 5, 8).cuda()),
             "two origins": dict(origins=torch.zeros((2, 2), dtype=torch.int32)),
             "an origin outside": dict(origins=torch.ones((1, 2), dtype=torch.int32))}
    for name, bad in cases.items():
        a = dict(dict(ctx=ctx, z=z, origins=o, ctx_next=nxt, stride=2, z_scale=1.0, forecast=fc, f_off=0, f_cnt=2), **bad)
        with pytest.raises(L.PrediffHipError):
            L.context_advance(a["ctx"], a["z"], a["origins"], a["ctx_next"], a["stride"], a["z_scale"], forecast=a["forecast"],
                              f_off=a["f_off"], f_cnt=a["f_cnt"])
            pytest.fail(name)


# ------------------------------------------------------------------------------------------------ modules
@functools.lru_cache(maxsize=None)
def _tiny_sd():
    return seeded_state_dict(TP.unet_template(CFG, "tiny_unet_schema.json", "axial"), 600)


def _net(precision="bf16", cfg=CFG):
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    net = CuboidTransformerUNet(**cfg, precision=precision)
    net.load_state_dict(_tiny_sd() if cfg is CFG else seeded_state_dict(net.state_dict(), 600))
    return net


def _vae(precision="bf16"):
    from prediff_amd.autoencoder_kl import AutoencoderKL
    vae = AutoencoderKL(**TINY_VAE_CFG, precision=precision)
    vae.load_state_dict(seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 601))
    return vae


def _ldm_kw(cfg=CFG, **kw):
    To, H, W, _ = cfg["target_shape"]
    return dict(dict(layout="NTHWC", data_shape=(To, 4 * H, 4 * W, 1), timesteps=T, use_ema=False, latent_shape=tuple(cfg["target_shape"]),
                     first_stage_model=None, cond_stage_model=None, scale_factor=SF), **kw)


def _plain(net=None, **kw):
    from prediff_amd.latent_diffusion import LatentDiffusion
    ldm = LatentDiffusion(torch_nn_module=net or _net(), **_ldm_kw(**kw)).cuda().eval()
    ldm.num_streams = 1
    return ldm


def _tapes(shape, n, seed, draws=5):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(tuple(shape), generator=g) for _ in range(draws)] for _ in range(n)]


SAMPLERS = {"ddim": dict(sampler="ddim", ddim_steps=2, eta=0.0), "dpmpp_2m_sde": dict(sampler="dpmpp_2m_sde", steps=3, eta=1.0)}


def _loop(ldm, name, zc, shape, **kw):
    """The public loop of SAMPLERS[name] on a latent context."""
    if name in ("ddim", "guided"):
        return ldm.ddim_sample_loop(zc, shape, ddim_steps=2, eta=0.0 if name == "ddim" else 1.0, **kw)
    return ldm.dpmpp_2m_sde_sample_loop(zc, shape, steps=3, eta=1.0, **kw)


def _latent_chain(ldm, name, zc, horizon, s, tapes, to_context=lambda c: c, loop_kw=None):
    """The hand chain: the public loop per segment, torch cat / slice / one fp32 scale between segments, the restatement's assembly.
    zc: the latent context (a canvas for the tiled module, `to_context` makes the loop's condition of it)."""
    B = zc.shape[0]
    shape = ldm.get_batch_latent_shape(B)
    n = R.n_segments(T_OUT, horizon, s)
    scale = float(np.float32(1.0 / float(ldm.scale_factor)))
    segs = []
    for j in range(n):
        z = _loop(ldm, name, to_context(zc), shape, noise_tape=tapes[j], **((loop_kw or (lambda j: {}))(j)))
        segs.append(z.cpu().numpy())
        zc = torch.cat([zc, z * scale], dim=1)[:, s:s + zc.shape[1]].contiguous()
    return torch.from_numpy(R.assemble(segs, T_OUT, horizon, s)).cuda()


@pytest.fixture(scope="module")
def plain_vae():
    """One plain module (latent context, a VAE to decode with) shared by the chain tests; they leave it unchanged."""
    return _plain(first_stage_model=_vae())


@pytest.mark.parametrize("s", [T_OUT, 1])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_rollout_vs_hand_chain(plain_vae, name, s):
    """horizon = 2 out_len + 1 = 5: three segments at stride 2 (the last keeps one frame), four at stride 1 (the last keeps two)."""
    ldm, B, horizon = plain_vae, 2, 2 * T_OUT + 1
    n = RolloutPlan(T_IN, T_OUT, horizon, s).segments
    assert n == {2: 3, 1: 4}[s]
    zc = seeded_input("roll.zc", (B,) + tuple(CFG["input_shape"]), 11).cuda()
    tapes = _tapes(ldm.get_batch_latent_shape(B), n, 12)
    ref = _latent_chain(ldm, name, zc, horizon, s, tapes)
    kw = dict(cond=zc, horizon=horizon, stride=s, batch_size=B, noise_tape=tapes, **SAMPLERS[name])
    keep = zc.clone()
    lat = rollout_sample(ldm, return_decoded=False, **kw)
    assert lat.shape == (B, horizon) + tuple(CFG["target_shape"][1:]) and bool(torch.isfinite(lat).all())
    assert torch.equal(lat, ref)
    assert torch.equal(zc, keep)                                              # the caller's context is never written
    dec = rollout_sample(ldm, **kw)
    assert dec.shape == (B, horizon, 32, 32, 1) and torch.equal(dec, ldm.decode_first_stage(ref))
    assert torch.equal(rollout_sample(ldm, return_decoded=False, **kw), lat)   # the ping-pong buffers leave nothing behind


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_one_segment_is_sample(plain_vae, name):
    ldm, B = plain_vae, 2
    zc = seeded_input("roll.zc", (B,) + tuple(CFG["input_shape"]), 13).cuda()
    tape = _tapes(ldm.get_batch_latent_shape(B), 1, 14)
    for decoded in (False, True):
        ref = ldm.sample(cond=zc, batch_size=B, return_decoded=decoded, noise_tape=tape[0], **SAMPLERS[name])
        for horizon in (T_OUT, T_OUT - 1):
            out = rollout_sample(ldm, zc, horizon, batch_size=B, return_decoded=decoded, noise_tape=tape, **SAMPLERS[name])
            assert out.shape[1] == horizon and torch.equal(out, ref[:, :horizon]), (decoded, horizon)
    x_T = tape[0][0].cuda()
    ref = ldm.sample(cond=zc, batch_size=B, return_decoded=False, x_T=x_T, **SAMPLERS["ddim"])
    assert torch.equal(rollout_sample(ldm, zc, T_OUT, batch_size=B, return_decoded=False, x_T=[x_T], **SAMPLERS["ddim"]), ref)


def test_scale_factor_one_half():
    ldm, B, horizon, s = _plain(scale_factor=0.5), 2, T_OUT + 1, 1
    zc = seeded_input("roll.zc", (B,) + tuple(CFG["input_shape"]), 15).cuda()
    tapes = _tapes(ldm.get_batch_latent_shape(B), 2, 16)
    ref = _latent_chain(ldm, "ddim", zc, horizon, s, tapes)
    other = _latent_chain(_plain(ldm.torch_nn_module), "ddim", zc, horizon, s, tapes)          # scale_factor = SF
    out = rollout_sample(ldm, zc, horizon, stride=s, batch_size=B, return_decoded=False, noise_tape=tapes, **SAMPLERS["ddim"])
    assert torch.equal(out, ref)
    assert torch.equal(out[:, :1], other[:, :1]) and not torch.equal(out[:, 1:], other[:, 1:])   # the scale enters with the first fed-back frame


def test_recondition_pixel():
    """The VAE round trip between segments against a loop over the public sample(): pixel cat / slice."""
    ldm = _plain(first_stage_model=_vae(), cond_stage_model="__is_first_stage__")
    B, horizon, s = 2, T_OUT + 2, 1                                           # three segments
    y = seeded_input("roll.y", (B, T_IN, 32, 32, 1), 17, kind="uniform").cuda()
    tapes = _tapes(ldm.get_batch_latent_shape(B), 3, 18)
    lat, pix, yj = [], [], y
    for j in range(3):
        z = ldm.sample(cond={"y": yj}, batch_size=B, return_decoded=False, noise_tape=tapes[j], **SAMPLERS["dpmpp_2m_sde"])
        x = ldm.sample(cond={"y": yj}, batch_size=B, return_decoded=True, noise_tape=tapes[j], **SAMPLERS["dpmpp_2m_sde"])
        lat.append(z.cpu().numpy()), pix.append(x.cpu().numpy())
        yj = torch.cat([yj, x], dim=1)[:, s:s + T_IN]
    kw = dict(cond={"y": y}, horizon=horizon, stride=s, recondition="pixel", batch_size=B, noise_tape=tapes, **SAMPLERS["dpmpp_2m_sde"])
    out = rollout_sample(ldm, **kw)
    assert out.shape == (B, horizon, 32, 32, 1) and torch.equal(out.cpu(), torch.from_numpy(R.assemble(pix, T_OUT, horizon, s)))
    assert torch.equal(rollout_sample(ldm, return_decoded=False, **kw).cpu(), torch.from_numpy(R.assemble(lat, T_OUT, horizon, s)))
    # the default mode on the same module feeds latents back: segment 0 agrees, the fed-back segments do not
    a, b = (rollout_sample(ldm, return_decoded=False, **dict(kw, recondition=mode)) for mode in ("latent", "pixel"))
    assert torch.equal(a[:, :s], b[:, :s]) and not torch.equal(a[:, s:], b[:, s:])


# ------------------------------------------------------------------------------------------------ the tiled module
def _tiled(net, canvas, stride, cfg, **kw):
    ldm = TiledLatentDiffusion(net, canvas=canvas, stride=stride, **_ldm_kw(cfg, **kw)).cuda().eval()
    ldm.num_streams = 1
    return ldm


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_tiled_rollout_vs_hand_chain(name):
    """Canvas (6, 7) of 4 x 4 windows at stride (2, 2): six overlapping windows, two segments.  The chain keeps the context as a canvas
    (torch cat / slice / scale) and gathers its windows with gather_windows in front of every loop; the driver keeps the window stack and
    lets the kernel cut the new frames out of the forecast canvas."""
    ldm = _tiled(_net(cfg=CFG4), (6, 7), (2, 2), CFG4)
    assert ldm.geometry.nwin == 6
    B, horizon, s = 2, T_OUT + 1, 1
    zc = seeded_input("roll.tiled.zc", (B, T_IN, 6, 7, 4), 19).cuda()
    tapes = _tapes(ldm.get_batch_latent_shape(B), 2, 20)
    ref = _latent_chain(ldm, name, zc, horizon, s, tapes, to_context=ldm.gather_windows)
    kw = dict(cond=zc, horizon=horizon, stride=s, batch_size=B, noise_tape=tapes, **SAMPLERS[name])
    out = rollout_sample(ldm, return_decoded=False, **kw)
    assert out.shape == (B, horizon, 6, 7, 4) and bool(torch.isfinite(out).all()) and torch.equal(out, ref)


def test_tiled_one_window_is_the_plain_rollout():
    net = _net()
    vae = _vae()
    plain, tiled = _plain(net, first_stage_model=vae), _tiled(net, (8, 8), (8, 8), CFG, first_stage_model=vae)
    assert tiled.geometry.nwin == 1
    B, horizon = 2, 2 * T_OUT
    zc = seeded_input("roll.zc", (B,) + tuple(CFG["input_shape"]), 21).cuda()
    tapes = _tapes(plain.get_batch_latent_shape(B), 2, 22)
    for name, kw in SAMPLERS.items():
        a = rollout_sample(plain, zc, horizon, batch_size=B, return_decoded=False, noise_tape=tapes, **kw)
        b = rollout_sample(tiled, zc, horizon, batch_size=B, return_decoded=False, noise_tape=tapes, **kw)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), name
    # decoded: one VAE call on all four frames, the blend multiplies by exactly 1.0
    a, b = (rollout_sample(m, zc, horizon, batch_size=B, noise_tape=tapes, **SAMPLERS["ddim"]) for m in (plain, tiled))
    assert a.shape == (B, horizon, 32, 32, 1) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ ensembles
def test_rollout_ensemble():
    from prediff_amd.ensemble import _LazyTape, member_noise_fn, sample_ensemble
    ldm = _plain(_net("fp32"))                                               # fp32: the engine's batch-split-reproducible setting
    M, seed, s = 4, 1000, 1
    zc = seeded_input("roll.ens.zc", (1,) + tuple(CFG["input_shape"]), 23).cuda()
    kw = dict(base_seed=seed, return_decoded=False, **SAMPLERS["dpmpp_2m_sde"])
    # one segment: sample_ensemble's own stream
    assert torch.equal(rollout_ensemble(ldm, zc, M, T_OUT, **kw), sample_ensemble(ldm, zc, M, **kw))
    assert torch.equal(rollout_ensemble(ldm, zc, M, T_OUT, micro_batch=2, **kw), sample_ensemble(ldm, zc, M, micro_batch=2, **kw))
    # two segments: segment j of member k draws from member_noise_fn(..., base_seed + (j << 32), ...)
    horizon = T_OUT + 1
    ks = list(range(M))
    tapes = [_LazyTape(member_noise_fn(tuple(ldm.latent_shape), ks, seed + (j << 32), zc.device)) for j in range(2)]
    ref = _latent_chain(ldm, "dpmpp_2m_sde", zc.expand(M, *zc.shape[1:]).contiguous(), horizon, s, tapes)
    out = rollout_ensemble(ldm, zc, M, horizon, stride=s, **kw)
    assert out.shape == (M, horizon) + tuple(CFG["target_shape"][1:]) and torch.equal(out, ref)
    assert not torch.equal(out[0], out[1])                                    # members differ
    assert torch.equal(rollout_ensemble(ldm, zc, M, horizon, stride=s, micro_batch=2, **kw), out)      # whatever the batch split


# ------------------------------------------------------------------------------------------------ guided
def test_guided_rollout():
    """Knowledge alignment with its own avg_x_gt per segment; the alignment function sees y = None in the chain's loops, as in the
    driver's later segments, and segment 0's y (the caller's latent context here) is not read by the avg_x objective."""
    from test_alignment import _tiny_alignment
    ldm = _plain(_net("fp32"))
    al = _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    B, horizon, s = 2, T_OUT + 2, 1                                           # three segments
    zc = seeded_input("roll.gd.zc", (B,) + tuple(CFG["input_shape"]), 25).cuda()
    tapes = _tapes(ldm.get_batch_latent_shape(B), 3, 26)
    aks = [{"avg_x_gt": torch.tensor([[0.4 - 0.1 * j], [0.1 + 0.2 * j]]).cuda()} for j in range(3)]
    kw = dict(cond=zc, horizon=horizon, stride=s, batch_size=B, return_decoded=False, noise_tape=tapes, use_alignment=True,
              sampler="ddim", ddim_steps=2, eta=1.0)
    ref = _latent_chain(ldm, "guided", zc, horizon, s, tapes, loop_kw=lambda j: dict(use_alignment=True, alignment_kwargs=aks[j]))
    out = rollout_sample(ldm, alignment_kwargs=aks, **kw)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, ref)
    same = rollout_sample(ldm, alignment_kwargs=aks[0], **kw)
    assert torch.equal(same, rollout_sample(ldm, alignment_kwargs=[aks[0]] * 3, **kw))
    assert torch.equal(same[:, :s], out[:, :s]) and not torch.equal(same[:, s:], out[:, s:])      # the later segments' targets differ
    plain = rollout_sample(ldm, **dict(kw, use_alignment=False))
    assert not torch.equal(plain[:, :s], out[:, :s])                          # and the guidance does move the sample
