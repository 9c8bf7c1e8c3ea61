"""Probability matching on the device: the rank order of frames (``rank_frames``), CDF matching of forecast frames onto a reference
(``match_cdf``) and the probability-matched mean of an ensemble (``probability_matched_mean``).  DESIGN.md §7, "Probability matching".
Not in the reference.  ``match_cdf`` is pysteps' ``nonparam_match_empirical_cdf`` with its wet-area adjustment, a free function there
too; PMM is Ebert 2001, Mon. Wea. Rev. 129, 2461.  tests/_probmatch_ref.py restates all three in NumPy; csrc/probmatch.hip implements them.

Frames are the fp32 tensors the rest of the package writes: contiguous, on the HIP device, the last three axes (H, W, 1) with 1 <= H, W and
n = H W <= 16384 (a frame is sorted in the LDS of one workgroup; the sides are under no other constraint).

ORDER means one thing: ascending by the exact fp32 value, ties by ascending flat pixel index: ``np.argsort(frame.ravel(), kind="stable")``.
-0.0 ties with +0.0; denormals order by their exact value (values are compared as integer keys, never flushed); a frame with a non-finite
pixel (NaN or +-inf) is never ordered, each function says what it gets instead.

  rank_frames(x) -> (sorted, order).  x (..., H, W, 1).  order int32 (..., n): the order above.  sorted fp32 (..., n):
      sorted[r] = x.ravel()[order[r]], the original bits (a -0.0 stays -0.0).  A frame with a non-finite pixel: order -1, sorted NaN.

  match_cdf(x, ref, threshold=None) -> out shaped like x.  x (B, T, H, W, 1) or (M, B, T, H, W, 1); ref (B, T, H, W, 1) or (B, 1, H, W, 1),
      the second broadcast over T, both over M.  Per frame: s = the ref frame sorted ascending, -0.0 read as +0.0.  With threshold thr
      (rounded to fp32 once): n_x = #{x > thr} and s[r] <- thr where s[r] > thr, for every r < n - n_x: when the reference has more wet
      pixels than the forecast, its lowest surplus wet values are capped, so matching never grows the rain area; otherwise a no-op.
      Then out.ravel()[order_x[r]] = s[r].  A non-finite pixel in x's frame or in its ref frame: the output frame is NaN throughout.
      Each ref frame is sorted once, however many frames of x share it.

  probability_matched_mean(ens) -> out (B, T, H, W, 1).  ens (M, B, T, H, W, 1), 1 <= M <= 512.  Per (b, t):
      mean = float32((sum_m float64(ens[m])) / M): the sum in fp64 in member order 0 .. M-1, the division in fp64, one rounding.
      P = the M n member values of the frame in ascending order (-0.0 read as +0.0); q[r] = P[r M + M // 2], r = 0 .. n-1: Ebert's "keep
      every M-th value", from the middle of each block; M = 1 gives q = P.  out.ravel()[order_mean[r]] = q[r].
      A non-finite pixel in any member's frame: the output frame is NaN throughout.

Every result is a selection of input values (and thr): exact, with no atomics, so the same inputs give the same bits and a frame alone gives
the bits it gives inside a batch.  ``StochasticExtrapolation`` is not changed: CDF-matched STEPS is the composition
``match_cdf(se.forecast(ctx, members=32), ctx[:, -1:], threshold=16/255)``.  The quality of PMM and of CDF-matched STEPS on real SEVIR is
not measured: these functions are the instrument, not a result.

There is no torch or CPU path.  The module keeps one workspace per device, sized by the largest call seen; a later call that fits only
launches, so the three functions can be captured in a HIP graph once warmed up at the shape (a call that needs more replaces the
workspace: a graph captured before it must be captured again).
"""
import math
from typing import Optional

import torch

from . import _lib as L

MAX_ELEMS, MAX_MEMBERS = 16384, 512          # the limits of csrc/probmatch.hip

_WS = {}                                      # device -> the workspace (uint8), the largest seen


def _workspace(device, need):
    held = _WS.get(str(device))
    if held is None or held.numel() < need:
        held = _WS[str(device)] = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    return held


def _frames(name, x, ranks, form):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() not in ranks or x.shape[-1] != 1:
        raise ValueError(f"{name} must be {form} with the last axis 1, got {tuple(x.shape)}")
    H, W = int(x.shape[-3]), int(x.shape[-2])
    if H * W > MAX_ELEMS:
        raise ValueError(f"{name}: frames of {H} x {W} are not supported: H W <= {MAX_ELEMS} (a frame is sorted in LDS)")
    return H, W


def _placed(name, x):
    if x.numel() == 0:
        raise ValueError(f"{name} must not be empty, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _on_device(name, x):
    if not x.is_cuda:
        raise ValueError(f"{name} must be on a CUDA(HIP) device: there is no CPU path")


@torch.no_grad()
def rank_frames(x: torch.Tensor):
    """x (..., H, W, 1) fp32 -> (sorted fp32 (..., H W), order int32 (..., H W)): the module docstring's."""
    H, W = _frames("x", x, range(3, 65), "(..., H, W, 1)")
    _placed("x", x)
    _on_device("x", x)
    lead = tuple(x.shape[:-3])
    frames = math.prod(lead)
    if L.pm_ws_bytes(L.PM_RANK, 1, frames, H, W) < 0:
        raise ValueError(f"x {tuple(x.shape)}: too many frames in one call")
    with L.on_device(x):
        sorted_out = torch.empty(lead + (H * W,), dtype=torch.float32, device=x.device)
        order = torch.empty(lead + (H * W,), dtype=torch.int32, device=x.device)
        L.rank_frames(x, frames, H, W, sorted_out, order)
    return sorted_out, order


@torch.no_grad()
def match_cdf(x: torch.Tensor, ref: torch.Tensor, threshold: Optional[float] = None) -> torch.Tensor:
    """x (B, T, H, W, 1) or (M, B, T, H, W, 1), ref (B, T, H, W, 1) or (B, 1, H, W, 1) -> x's frames with the values of their ref frame in
    x's rank order: the module docstring's."""
    H, W = _frames("x", x, (5, 6), "(B, T, H, W, 1) or (M, B, T, H, W, 1)")
    _frames("ref", ref, (5,), "(B, T, H, W, 1) or (B, 1, H, W, 1)")
    B, T = int(x.shape[-5]), int(x.shape[-4])
    if tuple(ref.shape) not in ((B, T, H, W, 1), (B, 1, H, W, 1)):
        raise ValueError(f"ref must be {(B, T, H, W, 1)} or {(B, 1, H, W, 1)} for x {tuple(x.shape)}, got {tuple(ref.shape)}")
    if threshold is not None:
        try:
            threshold = float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"threshold must be None or a finite number, got {threshold!r}") from None
        if not math.isfinite(threshold):
            raise ValueError(f"threshold must be None or a finite number, got {threshold!r}")
    _placed("x", x)
    _placed("ref", ref)
    if x.device != ref.device:
        raise ValueError(f"x is on {x.device}, ref on {ref.device}")
    _on_device("x", x)
    lead, ref_T = (int(x.shape[0]) if x.dim() == 6 else 1), int(ref.shape[1])
    need = L.pm_ws_bytes(L.PM_CDF, 1, B * ref_T, H, W)
    if need < 0 or L.pm_ws_bytes(L.PM_RANK, 1, lead * B * T, H, W) < 0:
        raise ValueError(f"x {tuple(x.shape)}: too many frames in one call")
    with L.on_device(x):
        out = torch.empty_like(x)
        L.cdf_match(x, ref, lead, B, T, ref_T, H, W, threshold, out, _workspace(x.device, need))
    return out


@torch.no_grad()
def probability_matched_mean(ens: torch.Tensor) -> torch.Tensor:
    """ens (M, B, T, H, W, 1) -> (B, T, H, W, 1): the ensemble mean's placement with the members' pooled intensities (module docstring)."""
    H, W = _frames("ens", ens, (6,), "(M, B, T, H, W, 1)")
    M, B, T = (int(s) for s in ens.shape[:3])
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"ens holds {M} members: 1 .. {MAX_MEMBERS} are supported")
    _placed("ens", ens)
    _on_device("ens", ens)
    need = L.pm_ws_bytes(L.PM_PMM, M, B * T, H, W)
    if need < 0:
        raise ValueError(f"ens {tuple(ens.shape)}: too many frames in one call")
    with L.on_device(ens):
        out = torch.empty((B, T, H, W, 1), dtype=torch.float32, device=ens.device)
        L.pmm(ens, M, B * T, H, W, out, _workspace(ens.device, need))
    return out
