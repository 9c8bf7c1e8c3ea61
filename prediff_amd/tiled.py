"""Tiled sampling: forecast a domain larger than the window the checkpoint was trained on ("Tiled sampling").

MultiDiffusion-style fusion (Bar-Tal et al. 2023, arXiv:2302.08113); not in the reference.  The denoiser's position tables and axial
cuboids tie it to one latent window (h, w), so a canvas (Hc, Wc) is covered by overlapping windows and ONE denoiser call on the canvas is
    gather the windows (pd_window_gather) -> the unchanged denoiser on the batch of B * nwin windows -> blend (pd_window_blend)
with eps_canvas(cell) = sum over the windows covering the cell of g^_win(cell) * eps_win(cell), g^ normalised per cell on the host.
Every step epilogue is linear in (z, eps, noise, history), so stepping the blended eps on the canvas equals blending the stepped windows:
the sampler loops, their RNG order, the graph capture and the lanes of ``LatentDiffusion`` run unchanged on canvas-shaped tensors.
The VAE is tiled the same way: each window is conditioned on the encoding of exactly its own context tile (no blending), and the
decoded pixel tiles are blended with the same weight rule at pixel scale.

Forecast quality on a trained checkpoint is unmeasured (no checkpoint at hand); what the tests pin is the rule itself.
"""
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .latent_diffusion import LatentDiffusion

BLENDS = ("feather", "uniform")


def _pair(v) -> Tuple[int, int]:
    a, b = (v, v) if isinstance(v, (int, np.integer)) else v
    return int(a), int(b)


def _origins_1d(n: int, size: int, s: int):
    """sorted(set(min(k s, size - n))): the last window is snapped to the border, so every cell is covered"""
    return sorted({min(k * s, size - n) for k in range(math.ceil((size - n) / s) + 1)})


def _ramp(n: int, s: int, blend: str) -> np.ndarray:
    if blend == "uniform":
        return np.ones(n, dtype=np.float64)
    o = n - s
    return np.asarray([min(1.0, (k + 1) / (o + 1), (n - k) / (o + 1)) for k in range(n)], dtype=np.float64)


class TileGeometry:
    """Windows of (h, w) cells at stride (sh, sw) over a canvas (Hc, Wc), row-major (y outer), and their blend weights.  Host code only.

    origins: int32 (nwin, 2) of (y, x); weights(): fp32 (nwin, h, w), g = ramp_y (x) ramp_x normalised per canvas cell over the windows
    that cover it (fp64, rounded to fp32 once; a cell covered by one window holds exactly 1.0); scaled(f): the same geometry at f x the
    resolution (the pixel-scale tiles of a VAE with down-sampling factor f)."""

    def __init__(self, window, canvas, stride, blend: str = "feather"):
        self.window, self.canvas, self.stride = _pair(window), _pair(canvas), _pair(stride)
        if blend not in BLENDS:
            raise ValueError(f"blend must be one of {BLENDS}; got {blend!r}")
        self.blend = blend
        for n, size, s in zip(self.window, self.canvas, self.stride):
            if n < 1 or size < n:
                raise ValueError(f"the canvas {self.canvas} is smaller than the window {self.window}")
            if not 1 <= s <= n:
                raise ValueError(f"the stride {self.stride} must lie in [1, window] = [1, {self.window}]")
        self.origins_y = _origins_1d(self.window[0], self.canvas[0], self.stride[0])
        self.origins_x = _origins_1d(self.window[1], self.canvas[1], self.stride[1])
        self.origins = torch.tensor([[y, x] for y in self.origins_y for x in self.origins_x], dtype=torch.int32)
        self._weights = None

    @property
    def nwin(self) -> int:
        return int(self.origins.shape[0])

    def weights(self) -> torch.Tensor:
        if self._weights is None:
            (h, w), (Hc, Wc) = self.window, self.canvas
            g = np.outer(_ramp(h, self.stride[0], self.blend), _ramp(w, self.stride[1], self.blend))
            total = np.zeros((Hc, Wc), dtype=np.float64)
            for y, x in self.origins.tolist():           # ascending window index
                total[y:y + h, x:x + w] += g
            out = np.stack([g / total[y:y + h, x:x + w] for y, x in self.origins.tolist()])
            self._weights = torch.from_numpy(out.astype(np.float32))
        return self._weights

    def scaled(self, f: int) -> "TileGeometry":
        f = int(f)
        return TileGeometry(tuple(f * v for v in self.window), tuple(f * v for v in self.canvas), tuple(f * v for v in self.stride), self.blend)


def _refusing_alignment(name):
    def loop(self, *args, **kwargs):
        self._refuse_alignment(kwargs.get("use_alignment", False))
        return getattr(super(TiledLatentDiffusion, self), name)(*args, **kwargs)
    loop.__name__ = name
    loop.__doc__ = f"LatentDiffusion.{name} on the canvas (knowledge alignment is refused before any draw)."
    return loop


class TiledLatentDiffusion(LatentDiffusion):
    """``LatentDiffusion`` on a canvas of (Hc, Wc) latent cells covered by windows of the model's own size.

    TiledLatentDiffusion(torch_nn_module, canvas=(Hc, Wc), stride=(sh, sw), blend="feather", max_windows_per_call=None, **ldm_kwargs):
    `ldm_kwargs` are the plain module's own, `latent_shape` / `data_shape` those of ONE window; the module then exposes `latent_shape` /
    `data_shape` of the canvas (the window's stay in `window_latent_shape` / `window_data_shape`), so sample(), every sampler loop and
    ensemble.sample_ensemble work on the canvas unchanged.  `torch_nn_module` stays the plain U-Net and the state_dict has exactly the
    plain module's keys: construct the plain modules, load the checkpoints, then wrap.

    Conditioning: cond = {"y": (B, T_in, f Hc, f Wc, C_px)} with cond_stage_model="__is_first_stage__" (f = the VAE's down-sampling
    factor), or a latent canvas (B, T_in, Hc, Wc, C) with cond_stage_model=None.  Inside the loops the condition is the batch-major
    window stack (B, nwin, T_in, h, w, C).  `max_windows_per_call` runs the denoiser on that many windows at a time."""

    def __init__(self, torch_nn_module, canvas, stride, blend: str = "feather", max_windows_per_call: Optional[int] = None, **ldm_kwargs):
        ntc = ldm_kwargs.get("num_timesteps_cond")
        if ntc is not None and ntc > 1:
            raise NotImplementedError("num_timesteps_cond > 1 (shorten_cond_schedule) is not defined for tiled sampling")
        if ldm_kwargs.get("cond_stage_model") not in (None, "__is_first_stage__"):
            raise NotImplementedError('tiled sampling conditions on the first stage ("__is_first_stage__") or on a latent canvas (None)')
        super().__init__(torch_nn_module, **ldm_kwargs)
        T, h, w, C = self.latent_shape
        Td, hd, wd, Cd = self.data_shape
        f = hd // h
        if f < 1 or (hd, wd) != (f * h, f * w):
            raise ValueError(f"data_shape {self.data_shape} is not an integer multiple of latent_shape {self.latent_shape} in H and W")
        self.geometry = TileGeometry((h, w), canvas, stride, blend)
        self.pixel_geometry = self.geometry.scaled(f)
        self.downsample_factor = f
        self.window_latent_shape, self.window_data_shape = self.latent_shape, self.data_shape
        Hc, Wc = self.geometry.canvas
        self.latent_shape, self.data_shape = (T, Hc, Wc, C), (Td, f * Hc, f * Wc, Cd)
        self.max_windows_per_call = max_windows_per_call
        self._call_windows, self._graphs_pinned = None, None      # see _pins_batch_mode
        self._tile_ws: Dict = {}
        self._tile_weights: Dict = {}

    @property
    def max_windows_per_call(self):
        return self._max_windows_per_call

    @max_windows_per_call.setter
    def max_windows_per_call(self, value):
        if value is not None and int(value) < 1:
            raise ValueError(f"max_windows_per_call must be positive, got {value}")
        self._max_windows_per_call = None if value is None else int(value)
        self._graphs = {}             # a captured step holds the chunking it was captured with

    # ------------------------------------------------------------------------------------------------ workspace
    def _tile_buf(self, name, shape, device):
        """Per-lane buffers, keyed like the engine's workspace (`torch_nn_module._ws_slot`): allocated by the warm-up calls that precede
        a graph capture, reused by the capture and by every later call."""
        key = (name, tuple(shape), str(device), getattr(self.torch_nn_module, "_ws_slot", 0))
        t = self._tile_ws.get(key)
        if t is None:
            t = self._tile_ws[key] = torch.zeros(shape, dtype=torch.float32, device=device)
        return t

    def _weights_on(self, geometry, device):
        key = (geometry is self.pixel_geometry, str(device))
        t = self._tile_weights.get(key)
        if t is None:
            t = self._tile_weights[key] = geometry.weights().to(device)
        return t

    def _gather(self, canvas, geometry, out=None):
        """(B, T, H, W, C) on `geometry`'s canvas -> its windows (B, nwin, T, h, w, C)"""
        if canvas.dim() != 5 or tuple(canvas.shape[2:4]) != geometry.canvas:
            raise ValueError(f"expected a (B, T, {geometry.canvas[0]}, {geometry.canvas[1]}, C) canvas, got {tuple(canvas.shape)}")
        canvas = canvas.contiguous().float()
        B, T, _, _, C = canvas.shape
        shape = (B, geometry.nwin, T) + geometry.window + (C,)
        out = torch.empty(shape, dtype=torch.float32, device=canvas.device) if out is None else out
        with L.on_device(canvas):
            L.window_gather(canvas, out, geometry.origins)
        return out

    def gather_windows(self, z):
        """The latent windows (B, nwin, T, h, w, C) of a latent canvas (B, T, Hc, Wc, C)."""
        return self._gather(z, self.geometry)

    # ------------------------------------------------------------------------------------------------ the three overrides
    def apply_model(self, x_noisy, t, cond):
        """One denoiser call on the canvas: gather -> torch_nn_module on the window batch -> blend.  Capture-safe: no synchronisation, and
        its buffers live in the per-lane workspace."""
        geo, net = self.geometry, self.torch_nn_module
        x = x_noisy.contiguous().float()
        B, nwin = x.shape[0], geo.nwin
        n = B * nwin
        with L.on_device(x):
            zw = self._gather(x, geo, out=self._tile_buf("z.win", (B, nwin) + tuple(x.shape[1:2]) + geo.window + tuple(x.shape[4:]), x.device))
            if not isinstance(cond, torch.Tensor):
                raise TypeError("tiled sampling needs a tensor condition: the window stack (B, nwin, T_in, h, w, C) or a latent canvas")
            if cond.dim() == 6:
                if cond.shape[:2] != (B, nwin):
                    raise ValueError(f"condition {tuple(cond.shape)} is not a stack of {nwin} windows for each of {B} samples")
                cw = cond.contiguous().float()
            else:
                cw = self._gather(cond, geo, out=self._tile_buf("c.win", (B, nwin) + tuple(cond.shape[1:2]) + geo.window + tuple(cond.shape[4:]), x.device))
            zf, cf = zw.reshape((n,) + tuple(zw.shape[2:])), cw.reshape((n,) + tuple(cw.shape[2:]))
            tw = t.reshape(B, 1).expand(B, nwin).reshape(n)
            chunk = self.max_windows_per_call or n
            # the windows of the whole sampler call (every lane's), or of this call when it is made outside a sampler loop
            pin = self._pins_batch_mode(n if self._call_windows is None else self._call_windows)
            if chunk >= n:
                ew = self._denoise(zf, tw, cf, pin)
            else:
                ew = self._tile_buf("eps.win", tuple(zf.shape), x.device)
                for a in range(0, n, chunk):
                    ew[a:a + chunk].copy_(self._denoise(zf[a:a + chunk], tw[a:a + chunk], cf[a:a + chunk], pin))
            out = torch.empty_like(x)
            L.window_blend(ew.reshape(zw.shape), self._weights_on(geo, x.device), geo.origins, out)
        return out

    def _pins_batch_mode(self, windows):
        """Whether a call of `windows` windows in all runs its denoiser launches with `torch_nn_module.split_k = False`.

        The denoiser picks a small-batch mode (split-K Conv3d, finer GroupNorm chunks: another fp32 summation order) from the
        trajectories of ONE launch, at most SPLITK_MAX_BATCH of them.  Tiling multiplies that number by nwin, so the lanes and window
        chunks of one call -- 24 windows in one launch, 12 in two lanes, 6 in four -- would sit on both sides of the threshold and no
        longer agree bit for bit.  The mode is therefore chosen from the windows of the whole call: above the threshold every launch of
        the call, whatever its own size, runs in the engine's batch-split-reproducible mode (whose kernels are those of a large launch);
        at or below it nothing is changed, and the launches are the plain module's at the same batch."""
        net = self.torch_nn_module
        limit = getattr(net, "SPLITK_MAX_BATCH", None)
        return limit is not None and getattr(net, "split_k", False) is True and windows > limit

    def _denoise(self, z, t, c, pin=False):
        net = self.torch_nn_module
        if pin:
            net.split_k = False
        try:
            out = net(z, t, c)
        finally:
            if pin:
                net.split_k = True
        out = out[0] if isinstance(out, tuple) else out
        return out.contiguous().float()

    def instantiate_cond_stage(self, cond_stage_model, cond_stage_forward):
        super().instantiate_cond_stage(cond_stage_model, cond_stage_forward)
        if self.cond_stage_model is None:
            return
        plain = self.cond_stage_forward

        def func(c):
            """{"y": (B, T_in, f Hc, f Wc, C_px)} -> (B, nwin, T_in, h, w, C): every window gets the encoding (.mode()) of exactly its
            own context tile, in one VAE call on B * nwin * T_in frames."""
            y = c.get("y") if isinstance(c, dict) else c
            pg = self.pixel_geometry
            if not isinstance(y, torch.Tensor) or y.dim() != 5 or tuple(y.shape[2:4]) != pg.canvas:
                got = tuple(y.shape) if isinstance(y, torch.Tensor) else type(y).__name__
                raise ValueError(f"the pixel context must be (B, T_in, {pg.canvas[0]}, {pg.canvas[1]}, C): {self.downsample_factor} x the "
                                 f"latent canvas {self.geometry.canvas}; got {got}")
            B = y.shape[0]
            tiles = self._gather(y, pg)
            zc = plain({"y": tiles.reshape((B * pg.nwin,) + tuple(tiles.shape[2:]))})
            return zc.reshape((B, pg.nwin) + tuple(zc.shape[1:]))
        self.cond_stage_forward = func

    @torch.no_grad()
    def decode_first_stage(self, z):
        """z / scale_factor -> windows -> the VAE decoder on B * nwin * T frames -> pixel tiles blended onto (B, T, f Hc, f Wc, C_px)"""
        z = (1.0 / self.scale_factor * z).contiguous().float()
        B, pg = z.shape[0], self.pixel_geometry
        zw = self.gather_windows(z)
        out = self.first_stage_model.decode(self._to_frames(zw.reshape((B * pg.nwin,) + tuple(zw.shape[2:]))))
        if hasattr(out, "sample") and not isinstance(out, torch.Tensor):
            out = out.sample
        tiles = self._from_frames(out.float(), B * pg.nwin)
        canvas = torch.empty((B, tiles.shape[1]) + pg.canvas + (tiles.shape[-1],), dtype=torch.float32, device=z.device)
        with L.on_device(z):
            L.window_blend(tiles.reshape((B, pg.nwin) + tuple(tiles.shape[1:])), self._weights_on(pg, z.device), pg.origins, canvas)
        return canvas

    # ------------------------------------------------------------------------------------------------ refusals and the driver
    @staticmethod
    def _refuse_alignment(use_alignment):
        if use_alignment:
            raise NotImplementedError("use_alignment=True: the avg_x knowledge-alignment objective is defined on one window, not on a canvas")

    def sample(self, cond, *args, **kwargs):
        """LatentDiffusion.sample on the canvas.  Refused before any draw: use_alignment, and a context that is not canvas-sized."""
        self._refuse_alignment(kwargs.get("use_alignment", args[1] if len(args) > 1 else False))
        self._check_latent_context(cond)
        return super().sample(cond, *args, **kwargs)

    def hold_from_frames(self, frames, first=0):
        """Held regions (hold_mask / hold_x0, canvas-shaped) pass straight through to the step on the canvas; encoding pixel frames
        into a canvas latent is not defined here (the tiled VAE encodes context tiles window by window, without blending)."""
        raise NotImplementedError("hold_from_frames is not defined on a canvas: pass a canvas-shaped latent as hold_x0")

    def _check_latent_context(self, cond):
        """Without a condition stage the context is a latent canvas (also checked by rollout.rollout_sample)."""
        if self.cond_stage_model is None:
            zc = cond if isinstance(cond, torch.Tensor) else (cond.get("y") if isinstance(cond, dict) else None)
            if not isinstance(zc, torch.Tensor) or zc.dim() != 5 or tuple(zc.shape[2:4]) != self.geometry.canvas:
                got = tuple(zc.shape) if isinstance(zc, torch.Tensor) else type(zc).__name__
                raise ValueError(f"the latent context must be a canvas (B, T_in, {self.geometry.canvas[0]}, {self.geometry.canvas[1]}, C); got {got}")

    p_sample = _refusing_alignment("p_sample")
    p_sample_loop = _refusing_alignment("p_sample_loop")
    ddim_sample_loop = _refusing_alignment("ddim_sample_loop")
    dpmpp_2m_sample_loop = _refusing_alignment("dpmpp_2m_sample_loop")
    dpmpp_2m_sde_sample_loop = _refusing_alignment("dpmpp_2m_sde_sample_loop")

    def _run_sampler(self, rule, cond, shape, *args, **kwargs):
        """A latent canvas as condition (cond_stage_model=None) becomes the window stack once per run, not once per step, and the
        denoiser's batch mode is chosen from the windows of the whole call (_pins_batch_mode), whatever the lanes make of them."""
        self._refuse_alignment(kwargs.get("use_alignment", False))
        if isinstance(cond, torch.Tensor) and cond.dim() == 5 and cond.is_cuda:
            cond = self.gather_windows(cond)
        windows = int(shape[self.batch_axis]) * self.geometry.nwin
        pin = self._pins_batch_mode(windows)
        if pin != self._graphs_pinned:          # a captured step holds the kernels of the mode it was captured in (_pins_batch_mode)
            self._graphs, self._graphs_pinned = {}, pin
        self._call_windows = windows
        try:
            return super()._run_sampler(rule, cond, shape, *args, **kwargs)
        finally:
            self._call_windows = None
