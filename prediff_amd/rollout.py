"""Rolling forecasts: more frames than the checkpoint's horizon from the unchanged checkpoint ("Rolling forecasts").

Not in the reference, which forecasts exactly `latent_shape[0]` frames per call.  A forecast of `horizon` frames is a chain of sampler
runs ("segments") of `out_len` frames each, `stride` frames apart; every segment but the last contributes its first `stride` frames
(a receding horizon: the frames nearest their context are kept), and the context of the next segment is cut from the previous context
followed by the previous forecast:
    cat_j = [ctx_j ; z_j / scale_factor]  (in_len + out_len frames),   ctx_{j+1} = cat_j[stride : stride + in_len].
The VAE is frame-wise, so a forecast latent can serve as a context latent directly: z approximates scale_factor * E(x), and the context
the denoiser was trained on is E(x).mode(), unscaled -- hence z / scale_factor, and no VAE call between two segments
(recondition="latent").  The advance and the append of the kept frames are ONE launch (pd_context_advance, csrc/rollout.hip), which for
``TiledLatentDiffusion`` also cuts the new context frames out of the forecast canvas window by window.  recondition="pixel" instead sends
the fed-back frames through the VAE round trip the model saw in training (decode, then the module's own cond_stage_forward).

Forecast quality on a trained checkpoint is unmeasured (no checkpoint at hand); what the tests pin is the rule itself.
"""
import contextlib
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from .ensemble import _LazyTape, member_noise_fn, sample_ensemble
from .step_rules import FAST_SAMPLERS
from .tiled import TiledLatentDiffusion

RECONDITION = ("latent", "pixel")
OVERLAP = ("discard", "hold")


def _int(name, v):
    try:
        ok = not isinstance(v, bool) and int(v) == v
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


class RolloutPlan:
    """Which segment forecasts which frame.  Host code only.

    RolloutPlan(in_len, out_len, horizon, stride=None): `stride` in [1, out_len] (default out_len), `horizon` >= 1.
    segments: n = 1 if horizon <= out_len else ceil((horizon - out_len) / stride) + 1; starts[j] = j * stride: segment j forecasts the
    result frames [starts[j], starts[j] + out_len); keep[j]: the leading frames of segment j that enter the result (stride for every
    segment but the last, horizon - (n - 1) * stride for the last); source(f) = (j, f - j * stride) with j = min(f // stride, n - 1).
    The context of segment j + 1 is frames [stride, stride + in_len) of [ctx_j ; forecast_j]."""

    def __init__(self, in_len: int, out_len: int, horizon: int, stride: Optional[int] = None):
        self.in_len, self.out_len = _int("in_len", in_len), _int("out_len", out_len)
        if self.in_len < 1 or self.out_len < 1:
            raise ValueError(f"in_len and out_len must be >= 1, got {in_len} and {out_len}")
        self.stride = self.out_len if stride is None else _int("stride", stride)
        if not 1 <= self.stride <= self.out_len:
            raise ValueError(f"stride must lie in [1, out_len] = [1, {self.out_len}], got {stride}")
        self.horizon = _int("horizon", horizon)
        if self.horizon < 1:
            raise ValueError(f"horizon must lie in [1, inf), got {horizon}")
        s = self.stride
        self.segments = 1 if self.horizon <= self.out_len else math.ceil((self.horizon - self.out_len) / s) + 1
        n = self.segments
        self.starts: List[int] = [j * s for j in range(n)]
        self.keep: List[int] = [s] * (n - 1) + [self.horizon - (n - 1) * s]

    def source(self, f: int) -> Tuple[int, int]:
        """(segment, frame of that segment) of result frame f"""
        if not 0 <= f < self.horizon:
            raise ValueError(f"frame must lie in [0, horizon) = [0, {self.horizon}), got {f}")
        j = min(f // self.stride, self.segments - 1)
        return j, f - j * self.stride


def _per_segment(name, value, n, single=()):
    """None -> n x None; a value of a type in `single` -> repeated; else a sequence of exactly n entries"""
    if value is None or isinstance(value, single):
        return [value] * n
    if isinstance(value, torch.Tensor) or not isinstance(value, Sequence) or len(value) != n:
        got = f"{len(value)} entries" if isinstance(value, Sequence) and not isinstance(value, torch.Tensor) else type(value).__name__
        raise ValueError(f"{name} must be None or a sequence of one entry per segment ({n} segments); got {got}")
    return list(value)


def _plan_for(ldm, cond, horizon, stride):
    y = cond.get("y") if isinstance(cond, dict) else cond
    if not isinstance(y, torch.Tensor) or y.dim() != 5:
        raise ValueError('rollout needs a tensor context (B, T_in, H, W, C), or {"y": that}')
    return RolloutPlan(int(y.shape[1]), int(ldm.latent_shape[0]), horizon, stride), y


@torch.no_grad()
def rollout_sample(ldm, cond, horizon, stride=None, recondition="latent", batch_size=16, return_decoded=True, noise_tape=None, x_T=None,
                   use_alignment=False, alignment_kwargs=None, overlap="discard", **sampler_kwargs):
    """`horizon` forecast frames from a ``LatentDiffusion`` or ``TiledLatentDiffusion`` whose checkpoint forecasts latent_shape[0] of them.

    cond, batch_size, return_decoded, use_alignment and the sampler keywords (sampler, ddim_steps, eta, steps, discretize,
    lower_order_final, timesteps) are ``sample``'s, and segment 0 IS ``sample``'s run: horizon <= out_len returns the first `horizon`
    frames of what ``sample`` returns, bit for bit.  Taken per segment (RolloutPlan(...).segments of them): `noise_tape` and `x_T`, each
    None or a sequence with one entry per segment (an entry has ``sample``'s semantics); `alignment_kwargs`, one dict for every segment or
    a sequence of dicts.  recondition="latent": the next context is [ctx ; z / scale_factor][stride : stride + in_len], one
    pd_context_advance launch per segment, the VAE decodes once at the end (never with return_decoded=False), and the alignment function
    sees the caller's pixel context y in segment 0 and y=None afterwards.  recondition="pixel": the next PIXEL context is
    [y ; decode(z)][stride : stride + in_len], encoded by the module's cond_stage_forward (needs cond_stage_model="__is_first_stage__").
    overlap="discard": the out_len - stride frames that segment j + 1 forecasts again are forecast freely and segment j's are dropped.
    overlap="hold" (stride < out_len; the three fast samplers): segment j >= 1 runs with its first out_len - stride frames HELD to the
    latent frames z_{j-1}[:, stride:] (``sample``'s hold_mask / hold_x0, DESIGN.md §7 "Held regions"; `hold_noise` is taken here), so
    it out-paints segment j - 1 in time and consecutive segments agree where they meet.  The held frames are latents and pass
    through no VAE, also with recondition="pixel".
    Returns (B, horizon, ...): decoded frames, or latents with return_decoded=False."""
    kw = dict(sampler_kwargs)
    if kw.pop("mask", None) is not None or kw.pop("x0", None) is not None:
        raise NotImplementedError("inpainting (mask / x0) is not defined for a rolling forecast")
    if kw.pop("hold_mask", None) is not None or kw.pop("hold_x0", None) is not None:
        raise NotImplementedError('hold_mask / hold_x0 are not defined for a rolling forecast (which segment would they hold?); '
                                  'overlap="hold" holds the frames two segments share')
    hold_noise = kw.pop("hold_noise", "fresh")
    if overlap not in OVERLAP:
        raise ValueError(f"overlap must be one of {OVERLAP}; got {overlap!r}")
    if kw.pop("return_intermediates", False):
        raise NotImplementedError("return_intermediates=True is not defined for a rolling forecast")
    if recondition not in RECONDITION:
        raise ValueError(f"recondition must be one of {RECONDITION}; got {recondition!r}")
    tiled = isinstance(ldm, TiledLatentDiffusion)
    if tiled:
        ldm._refuse_alignment(use_alignment)
        ldm._check_latent_context(cond)
    if use_alignment:
        assert ldm.alignment_fn is not None, "Alignment function not set."
    if recondition == "pixel" and (ldm.cond_stage_model is None or ldm.cond_stage_model is not ldm.first_stage_model):
        raise ValueError('recondition="pixel" encodes the decoded forecast as the next context: it needs cond_stage_model="__is_first_stage__"')
    plan, y0 = _plan_for(ldm, cond, horizon, stride)
    n, s = plan.segments, plan.stride
    if overlap == "hold":
        if s == plan.out_len:
            raise ValueError(f'overlap="hold" needs stride < out_len = {plan.out_len}: with stride == out_len no frame is forecast twice')
        ldm._check_hold(None, None, hold_noise)
    tapes, x_Ts = _per_segment("noise_tape", noise_tape, n), _per_segment("x_T", x_T, n)
    aks = _per_segment("alignment_kwargs", alignment_kwargs, n, single=(dict,))
    loop_kw = dict(ldm._pop_sampler_kwargs(kw), timesteps=kw.pop("timesteps", None), verbose=kw.pop("verbose", False))
    if kw:
        raise TypeError(f"rollout_sample got unexpected keyword arguments {sorted(kw)}")
    if overlap == "hold" and loop_kw["sampler"] not in FAST_SAMPLERS:
        raise NotImplementedError('overlap="hold" is defined for sampler="ddim" | "dpmpp_2m" | "dpmpp_2m_sde" (held regions)')
    B = int(batch_size)
    shape = ldm.get_batch_latent_shape(batch_size=B)
    dev = ldm.betas.device
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        held = None
        if overlap == "hold":                     # the frames a segment shares with the one before it
            held = torch.zeros((1, plan.out_len) + (1,) * (len(shape) - 2), dtype=torch.float32, device=dev)
            held[:, :plan.out_len - s] = 1.0

        def run(zc, y, j, prev=None):
            hold = {}
            if held is not None and prev is not None:
                x0 = torch.zeros(shape, dtype=torch.float32, device=prev.device)
                x0[:, :plan.out_len - s].copy_(prev[:, s:])
                hold = dict(hold_mask=held, hold_x0=x0, hold_noise=hold_noise)
            return ldm._sample_latent(zc, shape, y, x_T=x_Ts[j], noise_tape=tapes[j], use_alignment=use_alignment, alignment_kwargs=aks[j],
                                      **hold, **loop_kw)
        if recondition == "pixel" and n > 1:
            return _pixel_chain(ldm, cond, plan, B, run, return_decoded)
        zc, y = ldm._latent_context(cond, B)
        z = run(zc, y, 0)
        if n == 1:
            return (ldm.decode_first_stage(z) if return_decoded else z)[:, :plan.horizon]
        if not isinstance(zc, torch.Tensor):
            raise ValueError("a rolling forecast needs a tensor latent context")
        # the context as a window stack (B, nwin, T_in, h, w, C): the plain module's is one window at the origin
        if tiled:
            ctx, origins = (zc if zc.dim() == 6 else ldm.gather_windows(zc)), ldm.geometry.origins
        else:
            ctx, origins = zc.contiguous().float().unsqueeze(1), torch.zeros((1, 2), dtype=torch.int32)
        z_scale = 1.0 / float(ldm.scale_factor)
        out = torch.empty((B, plan.horizon) + tuple(shape[2:]), dtype=torch.float32, device=z.device)
        spare = [torch.empty_like(ctx), torch.empty_like(ctx) if n > 2 else None]      # ping-pong; the caller's context is never written
        for j in range(n - 1):
            nxt = spare[j % 2]
            with L.on_device(z):
                L.context_advance(ctx, z.contiguous().float(), origins, nxt, s, z_scale, forecast=out, f_off=plan.starts[j], f_cnt=plan.keep[j])
            ctx = nxt
            z = run(ctx if tiled else ctx[:, 0], None, j + 1, z)
        out[:, plan.starts[-1]:].copy_(z[:, :plan.keep[-1]])
        return ldm.decode_first_stage(out) if return_decoded else out


def _pixel_chain(ldm, cond, plan, B, run, return_decoded):
    """recondition="pixel": every segment is `sample`'s run on the pixel context [y ; decode(z)][stride : stride + in_len]; the kept pixel
    frames are those decoded for the feedback (the last segment is decoded only when pixels are returned)."""
    y =(cond.get("y") if isinstance(cond, dict) else cond)[:B]
    kept, z = [], None
    for j in range(plan.segments):
        cj = dict(cond, y=y) if isinstance(cond, dict) else y
        zc, yj = ldm._latent_context(cj, B)
        z = run(zc, yj, j, z)
        last = j == plan.segments - 1
        x = ldm.decode_first_stage(z) if return_decoded or not last else None
        kept.append((x if return_decoded else z)[:, :plan.keep[j]])
        if not last:
            y = torch.cat([y, x], dim=1)[:, plan.stride:plan.stride + plan.in_len].contiguous()
    return torch.cat(kept, dim=1)


def rollout_ensemble(ldm, cond, num_members, horizon, stride=None, base_seed=0, **kw):
    """`num_members` rolling forecasts for ONE context, sharded like ``ensemble.sample_ensemble`` (whose `micro_batch`, `group` and
    `force_collective` keywords, and whose defaults sampler="ddim", eta=0.0, are taken here too; every other keyword is
    ``rollout_sample``'s).  Member k draws segment j from member_noise_fn(latent_shape, ks, base_seed + (j << 32), device): segment 0 is
    exactly sample_ensemble's stream, and a member's rollout depends on (base_seed, k) alone, not on the batch split, the rank or the
    world size (beyond what the engine's own batch-size modes imply).  Returns (num_members, horizon, ...) on every rank."""
    ens_kw = {k: kw.pop(k) for k in ("micro_batch", "group", "force_collective") if k in kw}
    for k in ("noise_tape", "x_T", "batch_size"):
        if k in kw:
            raise TypeError(f"rollout_ensemble draws every member's noise itself: {k} is not accepted")
    kw.setdefault("sampler", "ddim")
    kw.setdefault("eta", 0.0)
    plan, y = _plan_for(ldm, cond, horizon, stride)
    latent_shape, device = tuple(ldm.latent_shape), y.device
    ak = kw.pop("alignment_kwargs", None)

    def expand(d, m):
        if d is None:
            return None
        return {k: (v.expand(m, *v.shape[1:]) if torch.is_tensor(v) and v.shape[0] == 1 else v) for k, v in d.items()}

    def sample_fn(cb, ks):
        tapes = [_LazyTape(member_noise_fn(latent_shape, ks, int(base_seed) + (j << 32), device)) for j in range(plan.segments)]
        akb = expand(ak, len(ks)) if ak is None or isinstance(ak, dict) else [expand(d, len(ks)) for d in ak]
        return rollout_sample(ldm, cb, horizon, stride, batch_size=len(ks), noise_tape=tapes, alignment_kwargs=akb, **kw)
    return sample_ensemble(ldm, cond, num_members, base_seed=base_seed, sample_fn=sample_fn, **ens_kw)
