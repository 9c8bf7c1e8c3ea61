"""Optical-flow extrapolation on the device: the forecast every nowcasting score is read against ("Extrapolation baseline").

Lagrangian persistence advects the last observed frame along the motion observed in the context (pysteps' ``extrapolation`` nowcast,
the baseline of DGMR, LDCast and the PreDiff paper's tables); with a zero motion field the same ``advect`` is Eulerian persistence, a
copy of the last frame bit for bit.  Frames are the (B, T, H, W, 1) fp32 tensors ``SEVIRFrontEnd.ingest`` writes and the scores read.

Definition (tests/_extrapolation_ref.py restates it in NumPy; csrc/extrapolation.hip implements it).  Motion v = (v_y, v_x) is in
pixels per frame, one steady field per sequence.

  Pairs.      P = min(pairs, T - 1); pair p is I0_p = ctx[:, T - 2 - p], I1_p = ctx[:, T - 1 - p].  All pairs share the one field.
  Pyramid.    Level 0 is the frames; level l + 1 is the mean of each 2 x 2 block of level l.  H and W are divisible by 2^(levels - 1),
              the coarsest sides are >= 4, the sides <= 512.
  Gradients.  gy(y, x) = (I(y + 1, x) - I(y - 1, x)) / 2 with indices clamped to the frame (replicate border), gx alike; of I0_p, once
              per level.
  Window.     S[f](y, x) = the sum of f over |y' - y| <= radius, |x' - x| <= radius; cells outside the frame add nothing.
  Tensor.     Per level G = sum_p (S[gy gy], S[gy gx], S[gx gx]).
  Iteration   (``iters`` per level), at flow v:  It_p(y, x) = bil_clamp(I1_p, y + v_y, x + v_x) - I0_p(y, x);
              b = sum_p (S[gy It_p], S[gx It_p]);  d solves (G + damping I) d = b (closed 2 x 2 form);  v <- v - d.
  bil_clamp.  The coordinate is clamped to [0, H - 1] x [0, W - 1], then bilinear from floor, the upper taps clamped too.
  Coarse to fine.  v = 0 at the coarsest level; going down a level v_fine(y, x) = 2 v_coarse(y // 2, x // 2).
  Damping.    A pixel whose window holds no texture keeps the coarser level's estimate (b = 0 gives d = 0): that is how motion reaches
              the empty cells ahead of an echo.  An all-zero context gives v = 0 exactly.
  Advection.  F_k(y, x) = bil_fill(last, y - k v_y(y, x), x - k v_x(y, x)), k = 1 .. K: always one interpolation of the last observed
              frame, so lead time adds no blur.  A tap outside the frame reads ``fill``; a coordinate that is not finite, or further
              than 2^20 from the frame, gives ``fill`` (no index is formed from it: ``motion`` may be the caller's).

The defaults were chosen on a NumPy prototype with translating Gaussian blobs at 64 x 64 and 128 x 128 moving 1.5 .. 3.6 pixels per
frame (DESIGN.md §7 has the figures).  Their quality on real SEVIR motion is not measured: the class is the instrument, not a result.

``motion``, ``advect`` and ``forecast`` run pd_lk_motion / pd_advect; there is no torch or CPU path.  The first call at a shape
allocates the workspace (one per device, of the latest shape); later calls at that shape only launch, and can be captured in a HIP
graph.  A call at another shape replaces the workspace: a graph captured before it must be captured again.
"""
import math
from typing import Optional

import torch

from . import _lib as L
from ._args import as_int as _int

MAX_SIDE, MIN_COARSE, MAX_LEVELS, MAX_ITERS, MAX_RADIUS, MAX_PAIRS = 512, 4, 8, 64, 9, 16       # the limits of pd_lk_motion


def _frames(name, x, rank_shape):
    """the checks every tensor argument shares, ahead of its shape: a float32, non-empty tensor"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.numel() == 0:
        raise ValueError(f"{name} must be {rank_shape}, got the empty shape {tuple(x.shape)}")


def _on_device(name, x):
    if not x.is_cuda:
        raise ValueError(f"{name} must be on a CUDA(HIP) device: there is no CPU path")


class LagrangianPersistence:
    """LagrangianPersistence(out_len=6, levels=4, iters=3, radius=7, damping=1e-2, pairs=3, fill=0.0)

    out_len: the frames ``advect`` and ``forecast`` write unless told otherwise.  levels / iters / radius / damping / pairs: the motion
    estimate of the module docstring.  fill: what a tap outside the frame reads."""

    def __init__(self, out_len: int = 6, levels: int = 4, iters: int = 3, radius: int = 7, damping: float = 1e-2, pairs: int = 3,
                 fill: float = 0.0):
        self.out_len = _int("out_len", out_len)
        self.levels, self.iters = _int("levels", levels), _int("iters", iters)
        self.radius, self.pairs = _int("radius", radius), _int("pairs", pairs)
        if self.out_len < 1:
            raise ValueError(f"out_len must be >= 1, got {out_len}")
        if not 1 <= self.levels <= MAX_LEVELS:
            raise ValueError(f"levels must be 1 .. {MAX_LEVELS}, got {levels}")
        if not 1 <= self.iters <= MAX_ITERS:
            raise ValueError(f"iters must be 1 .. {MAX_ITERS}, got {iters}")
        if not 1 <= self.radius <= MAX_RADIUS:
            raise ValueError(f"radius must be 1 .. {MAX_RADIUS} (the window's products of a tile stay in LDS), got {radius}")
        if self.pairs < 1:
            raise ValueError(f"pairs must be >= 1, got {pairs}")
        self.damping, self.fill = float(damping), float(fill)
        if not (self.damping > 0 and math.isfinite(self.damping)):
            raise ValueError(f"damping must be positive and finite (it keeps the 2 x 2 system solvable), got {damping!r}")
        if not math.isfinite(self.fill):
            raise ValueError(f"fill must be finite, got {fill!r}")
        self._ws = {}                # device -> ((B, T, H, W), the workspace of pd_lk_motion): the latest shape only

    # ---------------------------------------------------------------------------------------- host arithmetic
    def _check_context(self, shape):
        """(B, T, H, W) of a context shape this estimator takes, or ValueError."""
        if len(shape) != 5 or shape[-1] != 1:
            raise ValueError(f"ctx must be (B, T, H, W, 1), got {tuple(shape)}")
        B, T, H, W = (int(s) for s in shape[:4])
        if T < 2:
            raise ValueError(f"motion needs T >= 2 context frames, got {T}")
        if min(self.pairs, T - 1) > MAX_PAIRS:
            raise ValueError(f"min(pairs, T - 1) = {min(self.pairs, T - 1)} frame pairs: at most {MAX_PAIRS} are supported")
        f = 1 << (self.levels - 1)
        if H % f or W % f:
            raise ValueError(f"frames of {H} x {W} are not divisible by 2^(levels - 1) = {f}")
        if min(H, W) // f < MIN_COARSE or max(H, W) > MAX_SIDE:
            raise ValueError(f"frames of {H} x {W} with {self.levels} levels: the coarsest sides must be >= {MIN_COARSE} and the sides "
                             f"<= {MAX_SIDE}")
        return B, T, H, W

    def _out_len(self, out_len):
        K = self.out_len if out_len is None else _int("out_len", out_len)
        if K < 1:
            raise ValueError(f"out_len must be >= 1, got {out_len}")
        return K

    # ---------------------------------------------------------------------------------------- device
    @torch.no_grad()
    def motion(self, ctx: torch.Tensor) -> torch.Tensor:
        """ctx (B, T, H, W, 1) fp32 on the device, T >= 2 -> (B, 2, H, W) fp32: (v_y, v_x) in pixels per frame."""
        _frames("ctx", ctx, "(B, T, H, W, 1)")
        B, T, H, W = self._check_context(ctx.shape)
        if not ctx.is_contiguous():
            raise ValueError("ctx must be contiguous")
        _on_device("ctx", ctx)
        dev, key = str(ctx.device), (B, T, H, W)
        with L.on_device(ctx):
            held = self._ws.get(dev)
            if held is None or held[0] != key:
                need = L.lk_ws_bytes(B, T, H, W, self.levels, self.iters, self.radius, self.pairs)
                if need < 0:
                    raise L.PrediffHipError(f"pd_lk_motion: unsupported shape {tuple(ctx.shape)}")
                held = self._ws[dev] = (key, torch.empty((need + 3) // 4, dtype=torch.float32, device=ctx.device))
            ws = held[1]
            out = torch.empty((B, 2, H, W), dtype=torch.float32, device=ctx.device)
            L.lk_motion(ctx, out, B, T, H, W, self.levels, self.iters, self.radius, self.damping, self.pairs, ws)
        return out

    @torch.no_grad()
    def advect(self, frame: torch.Tensor, motion: torch.Tensor, out_len: Optional[int] = None) -> torch.Tensor:
        """frame (B, H, W, 1) or (B, H, W) fp32, motion (B, 2, H, W) fp32 -> (B, K, H, W, 1) fp32, lead k at [:, k - 1].  Each image of
        `frame` must be contiguous; the step between images is free, so ``ctx[:, -1]`` is read in place."""
        K = self._out_len(out_len)
        _frames("frame", frame, "(B, H, W, 1) or (B, H, W)")
        _frames("motion", motion, "(B, 2, H, W)")
        if frame.dim() == 4 and frame.shape[-1] == 1:
            frame = frame[..., 0]
        if frame.dim() != 3:
            raise ValueError(f"frame must be (B, H, W, 1) or (B, H, W), got {tuple(frame.shape)}")
        B, H, W = frame.shape
        if max(H, W) > MAX_SIDE:
            raise ValueError(f"frames of {H} x {W}: the sides must be <= {MAX_SIDE}")
        if tuple(motion.shape) != (B, 2, H, W):
            raise ValueError(f"motion must be (B, 2, H, W) = {(B, 2, H, W)}, got {tuple(motion.shape)}")
        if not motion.is_contiguous():
            raise ValueError("motion must be contiguous")
        if not frame[0].is_contiguous() or (B > 1 and frame.stride(0) < H * W):
            raise ValueError("every image of frame must be contiguous")
        _on_device("frame", frame), _on_device("motion", motion)
        if motion.device != frame.device:
            raise ValueError(f"frame is on {frame.device}, motion on {motion.device}")
        with L.on_device(frame):
            out = torch.empty((B, K, H, W, 1), dtype=torch.float32, device=frame.device)
            L.advect(frame, motion, out, B, K, H, W, frame.stride(0) if B > 1 else H * W, self.fill)
        return out

    @torch.no_grad()
    def forecast(self, ctx: torch.Tensor, out_len: Optional[int] = None) -> torch.Tensor:
        """ctx (B, T, H, W, 1) -> (B, K, H, W, 1): the last frame advected along the context's motion."""
        K = self._out_len(out_len)
        motion = self.motion(ctx)
        return self.advect(ctx[:, -1], motion, K)
