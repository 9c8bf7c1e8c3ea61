"""Distance-map verification on the device: the squared distance map of a frame's event set (``distance_map``) and the mean error
distances, the Hausdorff distance and Baddeley's Delta per lead time and threshold (``SEVIRDistanceScore``).
Not in the reference; the measures are Gilleland 2011 (Wea. Forecasting 26, 281) and 2017 (Wea. Forecasting 32, 187), as MET's distance-map tool.

A frame is one (n, t) image of H x W pixels (C is 1 or absent from the layout; sides 1 to 128, the frame's maps live in LDS).

    event set      for threshold thr_k of ``threshold_list`` (on the 0-255 scale): E_k(x) = { s : float32(x[s]) / float32(1/255) >=
                   float32(thr_k) }, the IEEE division and comparison of pd_sevir_skill_counts: exactly the sets CSI counts.  A NaN is
                   never an event.
    d2_A[s]        min over a in A of (row_s - row_a)^2 + (col_s - col_a)^2: an exact integer, at most 2 127^2 = 32258; for an empty A it
                   is NO_EVENT = 2**31 - 1 at every pixel.  d_A = sqrt(float64(d2_A)).
    per pair (F = forecast events, O = observed events) and threshold
      med_miss     mean over s in O of d_F[s]: how far the observed storm lies from anything forecast      F and O both non-empty
      med_false    mean over s in F of d_O[s]: how far the forecast storm lies from anything observed      F and O both non-empty
      hausdorff    sqrt(max(max over O of d2_F, max over F of d2_O)), the maximum taken on the integers     F and O both non-empty
      baddeley     sqrt((1 / (H W)) sum over all pixels of (w(d_F[s]) - w(d_O[s]))^2), w(d) = min(d, c), c = float64(cutoff) in pixels.
                   With a finite cutoff an empty set has w = c everywhere and baddeley is defined for every pair that is not skipped
                   (two empty sets give 0); with cutoff=None, w(d) = d and it is defined only when F and O are both non-empty.
A pair in which either frame holds a non-finite pixel adds 1 to ``skipped`` at every threshold and nothing else.
Distances are in pixels: a user who wants kilometres multiplies the result.

``update(pred, target)``: equal shapes in ``layout``, any dtype (read as ``.float()``), in place through their strides.
``update_members(ens, target)``: ens is (M,) + target.shape and scores as M ``update(ens[i], target)`` calls would; the target's maps
are made once.  State, K thresholds: fp64 sums [4, K, T'] (med_miss, med_false, hausdorff, baddeley) and int64 counts [6, K, T'] (pairs,
skipped, pairs with F and O non-empty, pairs where baddeley is defined, event pixels in pred, in target), accumulated until ``reset()``;
``sync`` is the base's.  ``compute()``: the three distances over the pairs with both sets non-empty, baddeley over the pairs where it is
defined, frac_both = both / pairs; a zero count gives NaN.  Every number of a pair is added in a fixed order (csrc/distances.hip) and the
pairs are folded in a fixed order: the same inputs give the same bits.
"""
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .score_base import AXES, SEVIRScoreBase, axes_of

METRICS = ("med_miss", "med_false", "hausdorff", "baddeley", "frac_both")
NO_EVENT = 2 ** 31 - 1
MAX_THRESHOLDS = 8
DIVISOR = float(np.float32(1.0 / 255.0))       # as SEVIRSkillScore


def distance_map(frames: torch.Tensor, threshold: float, layout: str = "NTHWC", scaled: bool = True) -> torch.Tensor:
    """d2 of the event set of every frame: int32, shaped as the N, T, H, W axes; NO_EVENT everywhere in a frame without events.
    scaled=False compares the raw value with float32(threshold), with no division by float32(1/255)."""
    if len(set(layout)) != len(layout) or set(layout) - set(AXES) or set("NTHW") - set(layout) or frames.dim() != len(layout):
        raise ValueError(f"layout {layout!r}: distinct letters of N, T, H, W, C naming N, T, H and W, one per axis of frames "
                         f"{tuple(frames.shape)}")
    if not frames.is_cuda:
        raise L.PrediffHipError("distance_map runs on the HIP device the frames were decoded on")
    x = frames.detach().float()
    sizes, strides = axes_of(layout, x)
    if sizes[4] != 1:
        raise ValueError(f"C = {sizes[4]}: distance maps are made of one channel")
    N, T, H, W = sizes[:4]
    d2 = torch.empty((N, T, H, W), dtype=torch.int32, device=x.device)
    with L.on_device(x):
        L.distance_map(x, sizes, strides, threshold, DIVISOR if scaled else 1.0, d2)
    return d2


class SEVIRDistanceScore(SEVIRScoreBase):
    METRICS = METRICS
    LAYOUT_NEEDS_HW = "distances are measured over H and W"
    STATE = (("sums", torch.float64, lambda self, Tk: (4, len(self.threshold_list), Tk)),     # med_miss, med_false, hausdorff, baddeley
             ("counts", torch.int64, lambda self, Tk: (6, len(self.threshold_list), Tk)))     # pairs, skipped, both, baddeley defined,
    #                                                                                           event pixels in pred, in target

    def __init__(self, layout: str = "NTHWC", mode: str = "0", seq_len: Optional[int] = None,
                 threshold_list: Sequence[float] = (16, 74, 133, 160, 181, 219), metrics_list: Sequence[str] = METRICS,
                 cutoff: Optional[float] = None):
        threshold_list = tuple(float(t) for t in threshold_list)
        if not 1 <= len(threshold_list) <= MAX_THRESHOLDS:
            raise ValueError(f"{len(threshold_list)} thresholds: 1 .. {MAX_THRESHOLDS} are supported")
        if cutoff is not None and not (isinstance(cutoff, (int, float)) and not isinstance(cutoff, bool) and 0 < cutoff < math.inf):
            raise ValueError(f"cutoff {cutoff!r}: None or a positive finite number of pixels")
        self.threshold_list = threshold_list
        self.cutoff = None if cutoff is None else float(cutoff)
        super().__init__(layout, mode, seq_len, metrics_list)

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        if pred.dim() != len(self.layout) or pred.shape != target.shape:
            raise ValueError(f"pred and target must have one shape in layout {self.layout!r}; got {tuple(pred.shape)} and "
                             f"{tuple(target.shape)}")
        self._launch(pred.unsqueeze(0), target)

    def update_members(self, ens: torch.Tensor, target: torch.Tensor):
        self._launch(ens, target)

    def _launch(self, ens, target):
        x, y, M, sizes, xs, ys = self._members(ens, target)
        if sizes[4] != 1:
            raise ValueError(f"C = {sizes[4]}: distance maps are made of one channel")
        dev = ens.device
        self._state_on(dev)
        # an unsupported shape (no size, -1) gets one element: the launch below says which
        ws = self._workspace(max(L.distance_ws_bytes(M, len(self.threshold_list), sizes) // 8, 1), torch.float64, dev)
        with L.on_device(ens):
            L.distance_update(x, y, M, sizes, xs, ys, self.threshold_list, DIVISOR, self.cutoff, self.keep_seq_len_dim, self.sums,
                              self.counts, ws)

    def compute(self):
        K, Tk = len(self.threshold_list), self.Tk
        if self.sums is None:
            s, n = np.zeros((4, K, Tk)), np.zeros((6, K, Tk), np.int64)
        else:
            s, n = self.sums.cpu().numpy(), self.counts.cpu().numpy()
        s, nf = s.transpose(0, 2, 1), n.astype(np.float64).transpose(0, 2, 1)                  # per lead time: (T', K)
        with np.errstate(divide="ignore", invalid="ignore"):
            per = {"med_miss": s[0] / nf[2], "med_false": s[1] / nf[2], "hausdorff": s[2] / nf[2], "baddeley": s[3] / nf[3],
                   "frac_both": nf[2] / nf[0]}
        return {met: self._finish(per[met]) for met in self.metrics_list}
