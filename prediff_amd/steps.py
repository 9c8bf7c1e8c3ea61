"""Stochastic extrapolation on the device: the STEPS ensemble every ensemble score is read against, and with the noise switched off
S-PROG, the scale-filtered deterministic forecast ("Stochastic extrapolation").

STEPS is Lagrangian extrapolation in which every spatial scale loses predictability at its own observed rate and is refilled with noise
of the observed spectrum.  pysteps is not a dependency; the definition below is the engine's own, written after pysteps'
``nowcasts.steps`` with a Gaussian log-wavenumber cascade, AR(1) or AR(2) in Lagrangian coordinates, non-parametric FFT noise,
``mask_method="obs"`` and ``probmatching_method="mean"``.  tests/_steps_ref.py restates it in NumPy; csrc/steps.hip implements it.
Frames are the (B, T, H, W, 1) fp32 tensors ``SEVIRFrontEnd.ingest`` writes and the scores read; thr is the threshold as fp32.

  0. Floor.        X(x) = max(x, thr).
  1. Motion.       v = ``motion`` if given, else ``LagrangianPersistence.motion(ctx)``.
  2. Lagrangian frames, by pd_advect's rule with fill 0:  A_0 = X(ctx[:, T-1]),  A_1 = X(advect(ctx[:, T-2], v) at lead 1),
                   A_2 = X(advect(ctx[:, T-3], v) at lead 2) (AR(2) only).
  3. Bands         (``steps_bands``).  For cell (ky, kx): fy = min(ky, H-ky)/H, fx = min(kx, W-kx)/W, r = max(H,W) sqrt(fy^2 + fx^2),
                   r_max = max(H,W)/2, u = min(L-1, (L-1) log(max(r,1)) / log(r_max)), g_l = exp(-(u-l)^2 / (2 0.5^2)),
                   w_l = g_l / sum_j g_j: real, even in k, summing to one over l at every k.
  4. Cascade.      Y_lj = Re IFFT(w_l FFT(A_j)); mu_lj, sigma_lj its mean and population standard deviation over the pixels (fp64
                   sums); N_lj = (Y_lj - mu_lj) / sigma_lj.  A level with sigma_lj^2 <= 1e-10 max(mean(A_j^2), 1e-30) is dead: its N = 0
                   and its gamma = 0; for j = 0 it carries only its mean (``sigma`` reports 0).
  5. AR model      per level, in fp64, each result rounded to fp32 once.  gamma_i = mean(N_l0 N_li); eps = 1e-6;
                   gamma_1 <- clamp(gamma_1, -(1-eps), 1-eps).  AR(1): phi1 = gamma_1, phi2 = 0.  AR(2):
                   gamma_2 <- clamp(gamma_2, 2 gamma_1^2 - 1 + eps, 1-eps), phi1 = gamma_1 (1-gamma_2) / (1-gamma_1^2),
                   phi2 = (gamma_2 - gamma_1^2) / (1-gamma_1^2).  phi0 = sqrt(max(0, 1 - phi1 gamma_1 - phi2 gamma_2)).
  6. Noise.        P = |FFT(A_0 - mean(A_0))| (the modulus of FFT(A_0) with the cell k = 0 set to 0).  Per (m, b, k) with white field z:
                   e_l = Re IFFT(w_l P FFT(z)), e^_l = (e_l - mean) / std; a std that is exactly zero or not finite gives e^_l = 0.
  7. Evolution     pointwise in Lagrangian coordinates: N_l^(0) = N_l0, N_l^(-1) = N_l1,
                   N_l^(k) = phi1 N_l^(k-1) + phi2 N_l^(k-2) + phi0 e^_l^(k).
  8. Recomposition.  R^(k) = sum_l (mu_l0 + sigma_l0 N_l^(k)), l ascending: what ``evolve`` returns.  R^(0) is A_0.
  9. Finish        per (m, b, k).  wet0 = A_0 > thr.  mask="obs": R <- thr where wet0 is false.  match="mean": with S = {R > thr}, if S
                   and wet0 are both non-empty, R[S] += mean(A_0[wet0]) - mean(R[S]) (fp64 means, the shift rounded to fp32).
                   Q = R where R > thr else 0.  out[m, b, k](y, x) = bil_fill(Q, y - k v_y, x - k v_x) with fill 0: pd_advect's rule at
                   the single lead k, its handling of non-finite and far-away coordinates included.

An all-zero context gives an all-zero forecast exactly.  Members are independent: a member alone, with its own noise, gives the bits it
gives inside any ensemble; the same inputs give the same bits (no atomics).

Only the frames the LDS-resident FFT takes are supported: sides 2^a or 3 * 2^a, 8 .. 512, and H W <= 16384 (128 x 128, the SEVIR-LR
frame, is the largest square); 2 <= levels <= floor(log2(max(H, W))) - 1.  The defaults (levels=6, ar_order=2, threshold=16/255) are the
literature's (pysteps' examples, the STEPS baselines of DGMR and LDCast); their quality on real SEVIR is not measured: the class is the
instrument, not a result.

There is no torch or CPU path.  The first call at a shape allocates the workspace (one per device, of the latest (B, H, W) and the
largest member count seen at it); later calls at that shape with no more members only launch, and ``forecast`` with a caller-supplied
``noise`` (and ``motion``, or the default motion estimator already warmed up) can be captured in a HIP graph.  A call at another
(B, H, W) or with more members replaces the workspace: a graph captured before it must be captured again.
"""
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._args import as_int as _int
from .extrapolation import LagrangianPersistence, _frames, _on_device

MIN_SIDE, MAX_SIDE, MAX_ELEMS, MAX_MEMBERS = 8, 512, 16384, 512          # the limits of csrc/steps.hip


def _side_ok(n):
    if n < MIN_SIDE or n > MAX_SIDE:
        return False
    if n % 3 == 0:
        n //= 3
    return n & (n - 1) == 0


def _check_frame(H, W, levels):
    if not (_side_ok(H) and _side_ok(W) and H * W <= MAX_ELEMS):
        raise ValueError(f"frames of {H} x {W} are not supported: sides 2^a or 3 * 2^a, {MIN_SIDE} .. {MAX_SIDE}, and H W <= {MAX_ELEMS} "
                         f"(the transform of a frame stays in LDS)")
    top = int(math.floor(math.log2(max(H, W)))) - 1
    if not 2 <= levels <= top:
        raise ValueError(f"levels must be 2 .. floor(log2(max(H, W))) - 1 = {top} for frames of {H} x {W}, got {levels}")


def steps_bands(H: int, W: int, levels: int) -> torch.Tensor:
    """The cascade's band weights w_l(k) of step 3: (levels, H, W) float32 on the CPU, computed in fp64 and rounded once."""
    H, W, levels = _int("H", H), _int("W", W), _int("levels", levels)
    _check_frame(H, W, levels)
    ky, kx = np.arange(H), np.arange(W)
    fy = np.minimum(ky, H - ky)[:, None] / H
    fx = np.minimum(kx, W - kx)[None, :] / W
    m = max(H, W)
    r = m * np.sqrt(fy * fy + fx * fx)
    u = np.minimum(levels - 1, (levels - 1) * np.log(np.maximum(r, 1.0)) / np.log(m / 2))
    g = np.exp(-(u[None] - np.arange(levels)[:, None, None]) ** 2 / (2 * 0.5 ** 2))
    return torch.from_numpy((g / g.sum(axis=0)).astype(np.float32))


class StochasticExtrapolation:
    """StochasticExtrapolation(out_len=6, levels=6, ar_order=2, threshold=16/255, mask="obs", match="mean", motion=None)

    out_len: the leads ``evolve`` and ``forecast`` write unless told otherwise.  levels / ar_order / threshold / mask ("obs" or None) /
    match ("mean" or None): the module docstring's.  motion: the LagrangianPersistence that estimates the motion field when a call is
    given none (default-constructed if None)."""

    def __init__(self, out_len: int = 6, levels: int = 6, ar_order: int = 2, threshold: float = 16 / 255, mask: Optional[str] = "obs",
                 match: Optional[str] = "mean", motion: Optional[LagrangianPersistence] = None):
        self.out_len, self.levels, self.ar_order = _int("out_len", out_len), _int("levels", levels), _int("ar_order", ar_order)
        if self.out_len < 1:
            raise ValueError(f"out_len must be >= 1, got {out_len}")
        if self.levels < 2:
            raise ValueError(f"levels must be >= 2, got {levels}")
        if self.ar_order not in (1, 2):
            raise ValueError(f"ar_order must be 1 or 2, got {ar_order}")
        try:
            self.threshold = float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"threshold must be a finite number, got {threshold!r}") from None
        if not math.isfinite(self.threshold):
            raise ValueError(f"threshold must be finite, got {threshold!r}")
        if mask not in ("obs", None):
            raise ValueError(f'mask must be "obs" or None, got {mask!r}')
        if match not in ("mean", None):
            raise ValueError(f'match must be "mean" or None, got {match!r}')
        self.mask, self.match = mask, match
        if motion is not None and not isinstance(motion, LagrangianPersistence):
            raise ValueError(f"motion must be a LagrangianPersistence or None, got {type(motion).__name__}")
        self.motion = LagrangianPersistence() if motion is None else motion
        self._ws = {}                # device -> ((B, H, W), members it holds, the workspace, the bands on the device): the latest shape only

    # ---------------------------------------------------------------------------------------- host checks
    def _check_context(self, ctx):
        _frames("ctx", ctx, "(B, T, H, W, 1)")
        if ctx.dim() != 5 or ctx.shape[-1] != 1:
            raise ValueError(f"ctx must be (B, T, H, W, 1), got {tuple(ctx.shape)}")
        B, T, H, W = (int(s) for s in ctx.shape[:4])
        if T < self.ar_order + 1:
            raise ValueError(f"AR({self.ar_order}) needs T >= {self.ar_order + 1} context frames, got {T}")
        _check_frame(H, W, self.levels)
        if not ctx.is_contiguous():
            raise ValueError("ctx must be contiguous")
        _on_device("ctx", ctx)
        return B, T, H, W

    @staticmethod
    def _check_field(name, x, shape, like):
        _frames(name, x, str(shape))
        if tuple(x.shape) != tuple(shape):
            raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(x.shape)}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        _on_device(name, x)
        if x.device != like.device:
            raise ValueError(f"ctx is on {like.device}, {name} on {x.device}")

    def _out_len(self, out_len, noise=None):
        if out_len is None:
            return self.out_len if noise is None or not isinstance(noise, torch.Tensor) or noise.dim() != 5 else int(noise.shape[2])
        K = _int("out_len", out_len)
        if K < 1:
            raise ValueError(f"out_len must be >= 1, got {out_len}")
        return K

    # ---------------------------------------------------------------------------------------- device
    def _analyse(self, ctx, motion, M):
        """steps 0 .. 5 into the workspace of M members: (mu, sigma, phi, gamma, motion, bands, workspace)"""
        B, T, H, W = self._check_context(ctx)
        if motion is None:
            motion = self.motion.motion(ctx)
        else:
            self._check_field("motion", motion, (B, 2, H, W), ctx)
        dev, key = str(ctx.device), (B, H, W)
        with L.on_device(ctx):
            # the analysis' part of the workspace depends on (B, H, W) only and the members' part follows it, so a workspace of more
            # members serves fewer: it is replaced only by another shape or a larger member count
            held = self._ws.get(dev)
            if held is None or held[0] != key or held[1] < M:
                need = L.steps_ws_bytes(B, M, H, W, self.levels, self.ar_order)
                if need < 0:
                    raise L.PrediffHipError(f"pd_steps_analyse: unsupported shape {tuple(ctx.shape)} with {M} members")
                bands = held[3] if held is not None and held[0][1:] == (H, W) else steps_bands(H, W, self.levels).to(ctx.device)
                held = self._ws[dev] = (key, M, torch.empty(need // 8, dtype=torch.float64, device=ctx.device), bands)
            ws, bands = held[2], held[3]
            mu, sigma = (torch.empty((B, self.levels), dtype=torch.float32, device=ctx.device) for _ in range(2))
            phi = torch.empty((B, self.levels, 3), dtype=torch.float32, device=ctx.device)
            gamma = torch.empty((B, self.levels, 2), dtype=torch.float32, device=ctx.device)
            L.steps_analyse(ctx, motion, bands, B, T, H, W, self.levels, self.ar_order, self.threshold, mu, sigma, phi, gamma, ws)
        return mu, sigma, phi, gamma, motion, bands, ws

    def _evolve(self, ctx, noise, motion, out_len):
        K = self._out_len(out_len, noise)
        B, T, H, W = self._check_context(ctx)
        M = 1
        if noise is not None:
            _frames("noise", noise, "(M, B, K, H, W)")
            if noise.dim() != 5:
                raise ValueError(f"noise must be (M, B, K, H, W), got {tuple(noise.shape)}")
            M = int(noise.shape[0])
            if not 1 <= M <= MAX_MEMBERS:
                raise ValueError(f"noise holds {M} members: 1 .. {MAX_MEMBERS} are supported")
            self._check_field("noise", noise, (M, B, K, H, W), ctx)
        mu, sigma, phi, _, motion, bands, ws = self._analyse(ctx, motion, M)
        with L.on_device(ctx):
            R = torch.empty((M, B, K, H, W), dtype=torch.float32, device=ctx.device)
            L.steps_evolve(noise, bands, mu, sigma, phi, M, B, K, H, W, self.levels, self.ar_order, R, ws)
        return R, motion

    @torch.no_grad()
    def analyse(self, ctx: torch.Tensor, motion: Optional[torch.Tensor] = None) -> dict:
        """ctx (B, T, H, W, 1) fp32 on the device [, motion (B, 2, H, W)] -> {"mu", "sigma": (B, L), "phi": (B, L, 3) = (phi1, phi2,
        phi0), "gamma": (B, L, 2), "motion": (B, 2, H, W)}: the cascade of the last frame and the AR model of every level."""
        mu, sigma, phi, gamma, motion, _, _ = self._analyse(ctx, motion, 0)
        return {"mu": mu, "sigma": sigma, "phi": phi, "gamma": gamma, "motion": motion}

    @torch.no_grad()
    def evolve(self, ctx: torch.Tensor, noise: Optional[torch.Tensor] = None, motion: Optional[torch.Tensor] = None,
               out_len: Optional[int] = None) -> torch.Tensor:
        """-> (M, B, K, H, W) fp32: the recomposed Lagrangian fields R of step 8, lead k at [:, :, k - 1].  noise: (M, B, K, H, W) fp32
        standard normal on the device, or None for one member with zero innovations (S-PROG)."""
        return self._evolve(ctx, noise, motion, out_len)[0]

    @torch.no_grad()
    def forecast(self, ctx: torch.Tensor, members: Optional[int] = None, noise: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None, motion: Optional[torch.Tensor] = None,
                 out_len: Optional[int] = None) -> torch.Tensor:
        """-> (M, B, K, H, W, 1) fp32, what ``SEVIREnsembleScore.update`` and the ``update_members`` of the other scores take.
        members=M draws the noise with torch.randn(..., generator=generator) on the device of ctx; noise: the caller's; neither: S-PROG,
        M = 1."""
        if members is not None:
            if noise is not None:
                raise ValueError("give members or noise, not both")
            M = _int("members", members)
            if not 1 <= M <= MAX_MEMBERS:
                raise ValueError(f"members must be 1 .. {MAX_MEMBERS}, got {members}")
            B, T, H, W = self._check_context(ctx)
            noise = torch.randn((M, B, self._out_len(out_len), H, W), dtype=torch.float32, device=ctx.device, generator=generator)
        R, motion = self._evolve(ctx, noise, motion, out_len)
        M, B, K, H, W = R.shape
        with L.on_device(ctx):
            out = torch.empty((M, B, K, H, W, 1), dtype=torch.float32, device=ctx.device)
            L.steps_finish(ctx, motion, R, out, M, B, int(ctx.shape[1]), K, H, W, self.threshold, int(self.mask == "obs"),
                           int(self.match == "mean"))
        return out
