"""Frame scores of decoded SEVIR samples on the device: MSE, MAE and SSIM, over everything or per lead time.

The reference's ``test_step`` (scripts/prediff/sevirlr/train_sevirlr_prediff.py:937-965) scores every decoded sample with torchmetrics'
``MeanSquaredError``, ``MeanAbsoluteError`` and ``StructuralSimilarityIndexMeasure`` next to ``SEVIRSkillScore``; this class gives the
same three numbers without that package.  Constructor keywords follow ``SEVIRSkillScore`` / ``SEVIREnsembleScore`` (``layout``, ``mode``,
``seq_len``, ``metrics_list``); the frames are scored as they are (no division by a preprocess scale: the reference feeds these three
metrics the raw [0, 1] frames).

    mse  = sum (p - t)^2 / elements            mae = sum |p - t| / elements            (torchmetrics over all updates)
    ssim = sum of the frames' SSIM / frames    (torchmetrics' default SSIM with the frames flattened to ``(b t) c h w``)

A frame is one (n, t) image of C channels.  Its SSIM: 11 x 11 Gaussian window (sigma 1.5, weights summing to 1), window means mu_p, mu_t,
E[pp], E[tt], E[pt]; var_p = max(E[pp] - mu_p^2, 0), var_t alike, cov = E[pt] - mu_p mu_t; c1 = (0.01 R)^2, c2 = (0.03 R)^2;
ssim = (2 mu_p mu_t + c1)(2 cov + c2) / ((mu_p^2 + mu_t^2 + c1)(var_p + var_t + c2)), averaged over the C (H - 10)(W - 10) windows that
lie inside the frame (what torchmetrics keeps after it crops its reflect padding away).  R is ``data_range``; ``data_range=None`` is
torchmetrics' default: R = max(pred.max() - pred.min(), target.max() - target.min()) of THAT CALL's tensors, found on the device.  There is
no NaN masking: a NaN pixel makes its frame's SSIM and its lead time's MSE / MAE NaN.

``update(pred, target)``: equal shapes in ``layout``, any dtype (read as ``.float()``), in place through their strides -- one launch of
pd_frame_score_update, whose sums are fp64 in a fixed order (the same inputs give the same bits).  ``update_members(ens, target)``: ens is
(M,) + target.shape and scores as M ``update(ens[i], target)`` calls would, but the target's tiles and window moments are staged and
computed once for all members; it needs an explicit ``data_range``.  State: fp64 sums [3, T'] (squared error, absolute error, frame SSIM)
and int64 counts [2, T'] (elements, frames), accumulated until ``reset()``; ``sync(group)`` all-reduces both with SUM and is called on every
rank of the group, also on ranks that made no update.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .score_base import SEVIRScoreBase

METRICS = ("mse", "mae", "ssim")


class SEVIRFrameScore(SEVIRScoreBase):
    METRICS = METRICS
    LAYOUT_NEEDS_HW = "SSIM windows slide over H and W"
    STATE = (("sums", torch.float64, lambda self, Tk: (3, Tk)),      # sum (p - t)^2, sum |p - t|, sum of the frames' SSIM
             ("counts", torch.int64, lambda self, Tk: (2, Tk)))      # elements, frames

    def __init__(self, layout: str = "NTHWC", mode: str = "0", seq_len: Optional[int] = None,
                 metrics_list: Sequence[str] = METRICS, data_range: Optional[float] = None):
        super().__init__(layout, mode, seq_len, metrics_list)
        self.data_range = None if data_range is None else float(data_range)

    def reset(self):
        super().reset()
        self._range = None           # 2 floats on the device: the value ranges of the last data_range=None update

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        if pred.dim() != len(self.layout) or pred.shape != target.shape:
            raise ValueError(f"pred and target must have one shape in layout {self.layout!r}; got {tuple(pred.shape)} and "
                             f"{tuple(target.shape)}")
        self._launch(pred.unsqueeze(0), target)

    def update_members(self, ens: torch.Tensor, target: torch.Tensor):
        if self.data_range is None:
            raise ValueError("update_members needs an explicit data_range: the per-call range of data_range=None is undefined for a "
                             "stacked ensemble")
        self._launch(ens, target)

    def _launch(self, ens, target):
        x, y, M, sizes, xs, ys = self._members(ens, target)
        dev, data_range = ens.device, self.data_range
        self._state_on(dev)
        # an unsupported shape (no size, -1) gets one element: the launch below says which
        ws = self._workspace(max(L.frame_score_ws_doubles(M, sizes), 1), torch.float64, dev)
        if data_range is None and (self._range is None or self._range.device != dev):
            self._range = torch.empty(2, dtype=torch.float32, device=dev)
        with L.on_device(ens):
            L.frame_score_update(x, y, M, sizes, xs, ys, 0.0 if data_range is None else data_range,
                                 self._range if data_range is None else None, self.keep_seq_len_dim, self.sums, self.counts, ws)

    def compute(self):
        Tk = self.seq_len if self.keep_seq_len_dim else 1
        if self.sums is None:
            s, n = np.zeros((3, Tk)), np.zeros((2, Tk), np.int64)
        else:
            s, n = self.sums.cpu().numpy(), self.counts.cpu().numpy()
        nf = n.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            per = {"mse": s[0] / nf[0], "mae": s[1] / nf[0], "ssim": s[2] / nf[1]}
        return {met: self._finish(per[met]) for met in self.metrics_list}
