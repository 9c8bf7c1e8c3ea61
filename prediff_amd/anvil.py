"""Growth and decay extrapolation on the device: the deterministic ANVIL forecast, the baseline that continues each region's own
observed trend ("Growth and decay extrapolation").

``LagrangianPersistence`` freezes the intensities of the last frame and S-PROG relaxes every scale towards its mean; neither can let a
cell intensify or die.  ANVIL (Pulkkinen et al. 2020, "Nowcasting of convective rainfall using volumetric radar observations", written
for VIL; pysteps' ``nowcasts.anvil``) is an autoregressive *integrated* model, ARI(p, 1), of the cascade levels in Lagrangian
coordinates whose AR parameters are estimated *locally*, in a moving Gaussian window.  pysteps is not a dependency; the definition below
is the engine's own.  tests/_anvil_ref.py restates it in NumPy; csrc/anvil.hip implements it.  Frames are the (B, T, H, W, 1) fp32
tensors ``SEVIRFrontEnd.ingest`` writes and the scores read; thr is the threshold as fp32; p = ar_order.

  1. Motion.       v = ``motion`` if given, else ``self.motion.motion(ctx)`` (a ``LagrangianPersistence``).
  2. Lagrangian frames, by pd_advect's rule with fill 0 and no floor:  A_0 = ctx[:, T-1];  A_j = advect(ctx[:, T-1-j], v) at lead j,
                   j = 1 .. p + 1.
  3. Bands.        w_l = ``steps_bands(H, W, levels)``.
  4. Cascade,      not normalised:  Y_lj = Re IFFT(w_l FFT(A_j)).
  5. Differences.  D_lj = Y_lj - Y_l,j+1,  j = 0 .. p.
  6. Local moments.  r = ceil(3 window);  g[d] = exp(-d^2 / (2 window^2)), d = -r .. r, computed in fp64 and rounded to fp32 once (the
                   device reads them as a table).  G[f](y, x) is the row pass sum_d g[d] f(y, x + d) over the taps inside the frame
                   followed by the same pass down the columns; taps outside the frame are omitted and nothing is renormalised (it
                   cancels below); d ascending, fp32.  c_jk = G[D_lj D_lk] for (j, k) in {(0,0), (1,1), (0,1)}, and (2,2), (0,2) for
                   AR(2).
  7. Local correlations, fp32 per pixel.  ms_b = max(mean(A_0^2), 1e-20) (an fp64 mean);  W0 = (sum_d g[d])^2 in fp64;
                   delta_b = fp32(1e-6 W0 ms_b);  gamma_1 = c_01 / (sqrt(c_00 + delta) sqrt(c_11 + delta)),
                   gamma_2 = c_02 / (sqrt(c_00 + delta) sqrt(c_22 + delta)).  The product of two roots, not the root of a product (which
                   underflows to 0 / 0 on an empty frame); the regulariser is smooth on purpose: a dead / alive switch per pixel would
                   flip between fp32 and fp64.
  8. Yule-Walker   per pixel, fp32, eps = 1e-3.  gamma_1 <- clamp(gamma_1, -(1-eps), 1-eps).  AR(1): phi1 = gamma_1, phi2 = 0.  AR(2):
                   gamma_2 <- clamp(gamma_2, 2 gamma_1^2 - 1 + eps, 1-eps), phi1 = gamma_1 (1-gamma_2) / (1-gamma_1^2),
                   phi2 = (gamma_2 - gamma_1^2) / (1-gamma_1^2).  ``analyse`` returns phi and the clamped gamma.
  9. ARI iteration, pointwise in Lagrangian coordinates.  D_l^(0) = D_l0, D_l^(-1) = D_l1, Y_l^(0) = Y_l0;
                   D_l^(k) = phi1 D_l^(k-1) + phi2 D_l^(k-2),  Y_l^(k) = Y_l^(k-1) + D_l^(k);  R^(k) = sum_l Y_l^(k), l ascending: what
                   ``evolve`` returns.  No transform runs here.
 10. Finish.       Q = R where R > thr else 0;  out[b, k](y, x) = bil_fill(Q, y - k v_y, x - k v_x) with fill 0: pd_steps_finish with one
                   member, mask = 0, match = 0.

An all-zero context gives an all-zero forecast exactly.  Identical context frames with zero motion give R^(k) = A_0 up to the rounding
of the bands (every D is exactly zero).  Sequences are independent, and the same inputs give the same bits (no atomics).

Frames and levels are those ``steps_bands`` accepts: sides 2^a or 3 * 2^a, 8 .. 512, H W <= 16384 (128 x 128, the SEVIR-LR frame, is the
largest square); 2 <= levels <= floor(log2(max(H, W))) - 1.  T >= ar_order + 2: one frame more than STEPS, because the model is on first
differences.  The defaults (levels=6, ar_order=2, window=16 pixels: pysteps' 50 km at SEVIR-LR's 3 km pixels, threshold=16/255) are the
literature's; their quality on real SEVIR is not measured: the class is the instrument, not a result.

There is no torch or CPU path.  The first call at a frame size allocates the workspace (one per device, of the latest (H, W) and the
largest B seen at it); later calls at that size with no more sequences only launch, and ``forecast`` with a caller-supplied ``motion``
(or the default motion estimator already warmed up) can be captured in a HIP graph.  A call at another (H, W) or with a larger B
replaces the workspace: a graph captured before it must be captured again.
"""
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._args import as_int as _int
from .extrapolation import LagrangianPersistence, _frames, _on_device
from .steps import _check_frame, steps_bands

MIN_WINDOW, MAX_WINDOW = 0.5, 32.0                             # r = ceil(3 window) <= 96, the limit of csrc/anvil.hip


def anvil_window(window: float):
    """step 6's weights: (g (2 r + 1,) float32 on the CPU, computed in fp64 and rounded once; W0 = (sum g)^2 in fp64 of the rounded g)"""
    r = int(math.ceil(3 * window))
    d = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-d * d / (2.0 * window * window)).astype(np.float32)
    return torch.from_numpy(g), float(g.astype(np.float64).sum()) ** 2


class AutoregressiveExtrapolation:
    """AutoregressiveExtrapolation(out_len=6, levels=6, ar_order=2, window=16.0, threshold=16/255, motion=None)

    out_len: the leads ``evolve`` and ``forecast`` write unless told otherwise.  levels / ar_order / window (the Gaussian window's sigma
    in pixels, 0.5 .. 32) / threshold: the module docstring's.  motion: the LagrangianPersistence that estimates the motion field when a
    call is given none (default-constructed if None)."""

    def __init__(self, out_len: int = 6, levels: int = 6, ar_order: int = 2, window: float = 16.0, threshold: float = 16 / 255,
                 motion: Optional[LagrangianPersistence] = None):
        self.out_len, self.levels, self.ar_order = _int("out_len", out_len), _int("levels", levels), _int("ar_order", ar_order)
        if self.out_len < 1:
            raise ValueError(f"out_len must be >= 1, got {out_len}")
        if self.levels < 2:
            raise ValueError(f"levels must be >= 2, got {levels}")
        if self.ar_order not in (1, 2):
            raise ValueError(f"ar_order must be 1 or 2, got {ar_order}")
        try:
            self.window, self.threshold = float(window), float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"window and threshold must be finite numbers, got {window!r} and {threshold!r}") from None
        if not MIN_WINDOW <= self.window <= MAX_WINDOW:                             # false for a NaN
            raise ValueError(f"window must be {MIN_WINDOW} .. {MAX_WINDOW} pixels, got {window!r}")
        if not math.isfinite(self.threshold):
            raise ValueError(f"threshold must be finite, got {threshold!r}")
        if motion is not None and not isinstance(motion, LagrangianPersistence):
            raise ValueError(f"motion must be a LagrangianPersistence or None, got {type(motion).__name__}")
        self.motion = LagrangianPersistence() if motion is None else motion
        self._g, self._w0 = anvil_window(self.window)
        self._ws = {}                # device -> ((H, W), the workspace of the largest B seen at it, the bands, the window): the latest frame size only

    # ---------------------------------------------------------------------------------------- host checks
    def _check_context(self, ctx):
        _frames("ctx", ctx, "(B, T, H, W, 1)")
        if ctx.dim() != 5 or ctx.shape[-1] != 1:
            raise ValueError(f"ctx must be (B, T, H, W, 1), got {tuple(ctx.shape)}")
        B, T, H, W = (int(s) for s in ctx.shape[:4])
        if T < self.ar_order + 2:
            raise ValueError(f"AR({self.ar_order}) on first differences needs T >= {self.ar_order + 2} context frames, got {T}")
        _check_frame(H, W, self.levels)
        if not ctx.is_contiguous():
            raise ValueError("ctx must be contiguous")
        _on_device("ctx", ctx)
        return B, T, H, W

    @staticmethod
    def _check_motion(motion, shape, like):
        _frames("motion", motion, str(shape))
        if tuple(motion.shape) != tuple(shape):
            raise ValueError(f"motion must be {tuple(shape)}, got {tuple(motion.shape)}")
        if not motion.is_contiguous():
            raise ValueError("motion must be contiguous")
        _on_device("motion", motion)
        if motion.device != like.device:
            raise ValueError(f"ctx is on {like.device}, motion on {motion.device}")

    def _out_len(self, out_len):
        K = self.out_len if out_len is None else _int("out_len", out_len)
        if K < 1:
            raise ValueError(f"out_len must be >= 1, got {out_len}")
        return K

    # ---------------------------------------------------------------------------------------- device
    def _analyse(self, ctx, motion):
        """steps 1 .. 8: (phi, gamma, motion, workspace)"""
        B, T, H, W = self._check_context(ctx)
        if motion is None:
            motion = self.motion.motion(ctx)
        else:
            self._check_motion(motion, (B, 2, H, W), ctx)
        dev = str(ctx.device)
        with L.on_device(ctx):
            need = L.anvil_ws_bytes(B, H, W, self.levels, self.ar_order)
            if need < 0:
                raise L.PrediffHipError(f"pd_anvil_analyse: unsupported shape {tuple(ctx.shape)}")
            # the layout is a function of (B, H, W) that both launches work out for themselves, so a workspace of more sequences serves
            # fewer: it is replaced only by another frame size or a larger batch
            held = self._ws.get(dev)
            if held is None or held[0] != (H, W) or held[1].numel() * 8 < need:
                if held is not None and held[0] == (H, W):
                    bands, g = held[2], held[3]
                else:
                    bands, g = steps_bands(H, W, self.levels).to(ctx.device), self._g.to(ctx.device)
                held = self._ws[dev] = ((H, W), torch.empty(need // 8, dtype=torch.float64, device=ctx.device), bands, g)
            _, ws, bands, g = held
            phi, gamma = (torch.empty((B, self.levels, 2, H, W), dtype=torch.float32, device=ctx.device) for _ in range(2))
            L.anvil_analyse(ctx, motion, bands, g, self._w0, B, T, H, W, self.levels, self.ar_order, phi, gamma, ws)
        return phi, gamma, motion, ws

    def _evolve(self, ctx, motion, out_len):
        K = self._out_len(out_len)
        phi, _, motion, ws = self._analyse(ctx, motion)
        B, _, H, W = (int(s) for s in ctx.shape[:4])
        with L.on_device(ctx):
            R = torch.empty((B, K, H, W), dtype=torch.float32, device=ctx.device)
            L.anvil_evolve(phi, B, K, H, W, self.levels, self.ar_order, R, ws)
        return R, motion

    @torch.no_grad()
    def analyse(self, ctx: torch.Tensor, motion: Optional[torch.Tensor] = None) -> dict:
        """ctx (B, T, H, W, 1) fp32 on the device [, motion (B, 2, H, W)] -> {"phi": (B, L, 2, H, W) = (phi1, phi2), "gamma":
        (B, L, 2, H, W) = the clamped (gamma_1, gamma_2), "motion": (B, 2, H, W)}: the local AR model of every level."""
        phi, gamma, motion, _ = self._analyse(ctx, motion)
        return {"phi": phi, "gamma": gamma, "motion": motion}

    @torch.no_grad()
    def evolve(self, ctx: torch.Tensor, motion: Optional[torch.Tensor] = None, out_len: Optional[int] = None) -> torch.Tensor:
        """-> (B, K, H, W) fp32: the recomposed Lagrangian fields R of step 9, lead k at [:, k - 1]."""
        return self._evolve(ctx, motion, out_len)[0]

    @torch.no_grad()
    def forecast(self, ctx: torch.Tensor, motion: Optional[torch.Tensor] = None, out_len: Optional[int] = None) -> torch.Tensor:
        """-> (B, K, H, W, 1) fp32: what ``LagrangianPersistence.forecast`` returns and every score reads."""
        R, motion = self._evolve(ctx, motion, out_len)
        B, K, H, W = R.shape
        with L.on_device(ctx):
            out = torch.empty((B, K, H, W, 1), dtype=torch.float32, device=ctx.device)
            L.steps_finish(ctx, motion, R, out, 1, B, int(ctx.shape[1]), K, H, W, self.threshold, 0, 0)
        return out
