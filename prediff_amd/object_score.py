"""Object-based verification on the device: the storm objects of a frame (``label_objects``) and SAL per lead time (``SEVIRObjectScore``).
Not in the reference; SAL is Wernli et al. 2008, Mon. Wea. Rev. 136, 4470.

A frame is one (n, t) image of H x W pixels (C is 1 or absent from the layout; sides up to 128, the label image lives in LDS).

    thr            float32(threshold), or float32(thr_factor) * max(frame): one fp32 product, every frame its own (Wernli's R* = R_max / 15)
    object pixel   v >= thr and v > 0 (a NaN never is one; a NaN in the frame makes the threshold of ``threshold=None`` NaN)
    objects        the components of that mask under ``connectivity`` 4 or 8 that have at least ``min_pixels`` pixels, numbered
                   1, 2, ... in raster order of their first pixel; 0 is background.  Smaller components are left out of the table, the count,
                   S and L2, and stay in A and L1, which use the whole field.
    per object n   mass R_n = sum v, peak P_n = max v, area, centroid x_n = sum v (row, col) / R_n
    per frame      D = sum v / (H W) and x = sum v (row, col) / sum v over all pixels; V = sum R_n (R_n / P_n) / sum R_n;
                   r = sum R_n |x - x_n| / sum R_n; d = sqrt((H - 1)^2 + (W - 1)^2)
    per pair       A = (D_F - D_O) / ((D_F + D_O) / 2)        defined when D_F + D_O != 0
                   S = (V_F - V_O) / ((V_F + V_O) / 2)        defined when both frames have an object
                   L1 = |x_F - x_O| / d                       defined when both frames have mass (sum v != 0) and d > 0
                   L2 = 2 |r_F - r_O| / d, L = L1 + L2        defined where S and L1 are
A pair in which either frame holds a non-finite pixel adds 1 to ``skipped`` and nothing else.

``update(pred, target)``: equal shapes in ``layout``, any dtype (read as ``.float()``), in place through their strides.
``update_members(ens, target)``: ens is (M,) + target.shape and scores as M ``update(ens[i], target)`` calls would; the target's frames
are labelled once.  State: fp64 sums [7, T'] (S, A, L1, L2, L, |S|, |A|) and int64 counts [8, T'] (pairs, skipped, pairs where S / A /
L1 / L is defined, objects in pred, objects in target), accumulated until ``reset()``; ``sync`` is the base's.  ``compute()``: the mean of
each component over the pairs where it is defined (L2 over L's pairs) and the mean objects per frame; a zero count gives NaN.  Every
number of a frame is order-independent (integer sums, see csrc/objects.hip) and the pair sums are folded in a fixed order: the same
inputs give the same bits.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .score_base import AXES, SEVIRScoreBase, axes_of

METRICS = ("S", "A", "L", "L1", "L2", "abs_S", "abs_A", "n_obj_pred", "n_obj_target")
TABLE_COLUMNS = ("mass", "peak", "area", "row", "col", "first_pixel")
RECORD = 9                    # doubles per frame record of pd_objects_label


def _check_params(threshold, thr_factor, connectivity, min_pixels):
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity {connectivity!r}: 4 or 8")
    if not thr_factor > 0:
        raise ValueError(f"thr_factor {thr_factor!r} must be positive")
    if not (isinstance(min_pixels, int) and min_pixels >= 1):
        raise ValueError(f"min_pixels {min_pixels!r}: an integer >= 1")
    return None if threshold is None else float(threshold)


def label_objects(frames: torch.Tensor, layout: str = "NTHWC", threshold: Optional[float] = None, thr_factor: float = 1.0 / 15.0,
                  connectivity: int = 8, min_pixels: int = 1, max_objects: int = 256):
    """The objects of every frame: (labels int32 shaped as the N, T, H, W axes, n_objects int32 (N, T), table fp64
    (N, T, max_objects, 6) with the columns TABLE_COLUMNS, rows beyond n_objects zero).  Objects beyond max_objects are left out of the
    table only.  A frame with a non-finite pixel gets its labels and count, and zero masses / centroids."""
    threshold = _check_params(threshold, thr_factor, connectivity, min_pixels)
    if max_objects < 1:
        raise ValueError(f"max_objects {max_objects!r}: at least one table row")
    if len(set(layout)) != len(layout) or set(layout) - set(AXES) or set("NTHW") - set(layout) or frames.dim() != len(layout):
        raise ValueError(f"layout {layout!r}: distinct letters of N, T, H, W, C naming N, T, H and W, one per axis of frames "
                         f"{tuple(frames.shape)}")
    if not frames.is_cuda:
        raise L.PrediffHipError("label_objects runs on the HIP device the frames were decoded on")
    x = frames.detach().float()
    sizes, strides = axes_of(layout, x)
    if sizes[4] != 1:
        raise ValueError(f"C = {sizes[4]}: objects are labelled on one channel")
    N, T, H, W = sizes[:4]
    dev = x.device
    # an unsupported shape (no size, -1) gets one record: the launch below says what is wrong
    rec = torch.empty(max(L.objects_ws_bytes(0, sizes) // 8, RECORD), dtype=torch.float64, device=dev)
    labels = torch.empty((N, T, H, W), dtype=torch.int32, device=dev)
    table = torch.zeros((N, T, max_objects, len(TABLE_COLUMNS)), dtype=torch.float64, device=dev)
    with L.on_device(x):
        L.objects_label(x, sizes, strides, threshold, thr_factor, connectivity, min_pixels, rec, labels, table, max_objects)
    n_objects = rec[:N * T * RECORD].view(N, T, RECORD)[..., 7].to(torch.int32)
    return labels, n_objects, table


class SEVIRObjectScore(SEVIRScoreBase):
    METRICS = METRICS
    LAYOUT_NEEDS_HW = "objects are connected over H and W"
    STATE = (("sums", torch.float64, lambda self, Tk: (7, Tk)),      # S, A, L1, L2, L, |S|, |A|
             ("counts", torch.int64, lambda self, Tk: (8, Tk)))      # pairs, skipped, S / A / L1 / L defined, objects in pred, in target

    def __init__(self, layout: str = "NTHWC", mode: str = "0", seq_len: Optional[int] = None, metrics_list: Sequence[str] = METRICS,
                 threshold: Optional[float] = None, thr_factor: float = 1.0 / 15.0, connectivity: int = 8, min_pixels: int = 1):
        super().__init__(layout, mode, seq_len, metrics_list)
        self.threshold = _check_params(threshold, thr_factor, connectivity, min_pixels)
        self.thr_factor, self.connectivity, self.min_pixels = float(thr_factor), connectivity, min_pixels

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
            raise ValueError(f"C = {sizes[4]}: objects are labelled on one channel")
        dev = ens.device
        self._state_on(dev)
        # an unsupported shape (no size, -1) gets one element: the launch below says which
        ws = self._workspace(max(L.objects_ws_bytes(M, sizes) // 8, 1), torch.float64, dev)
        with L.on_device(ens):
            L.sal_update(x, y, M, sizes, xs, ys, self.threshold, self.thr_factor, self.connectivity, self.min_pixels,
                         self.keep_seq_len_dim, self.sums, self.counts, ws)

    def compute(self):
        Tk = self.Tk
        if self.sums is None:
            s, n = np.zeros((7, Tk)), np.zeros((8, Tk), np.int64)
        else:
            s, n = self.sums.cpu().numpy(), self.counts.cpu().numpy()
        nf = n.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            per = {"S": s[0] / nf[2], "A": s[1] / nf[3], "L1": s[2] / nf[4], "L2": s[3] / nf[5], "L": s[4] / nf[5],
                   "abs_S": s[5] / nf[2], "abs_A": s[6] / nf[3], "n_obj_pred": nf[6] / nf[0], "n_obj_target": nf[7] / nf[0]}
        return {met: self._finish(per[met]) for met in self.metrics_list}
