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
from .sevir_skill import axes_of

MAX_MEMBERS = 512
METRICS = ("mse", "mae", "ssim")


class SEVIRFrameScore:
    def __init__(self, layout: str = "NTHWC", mode: str = "0", seq_len: Optional[int] = None,
                 metrics_list: Sequence[str] = METRICS, data_range: Optional[float] = None):
        if mode not in ("0", "1", "2"):
            raise NotImplementedError(f"mode {mode} not supported!")
        if "N" not in layout or "T" not in layout or len(set(layout)) != len(layout) or set(layout) - set("NTHWC"):
            raise ValueError(f"layout {layout!r}: distinct letters of N, T, H, W, C with N and T present")
        if "H" not in layout or "W" not in layout:
            raise ValueError(f"layout {layout!r}: SSIM windows slide over H and W, both must be named")
        bad = [m for m in metrics_list if m not in METRICS]
        if bad:
            raise ValueError(f"unknown metrics {bad}; supported: {METRICS}")
        self.layout, self.mode, self.seq_len = layout, mode, seq_len
        self.metrics_list = tuple(metrics_list)
        self.data_range = None if data_range is None else float(data_range)
        self.keep_seq_len_dim = mode in ("1", "2")
        if self.keep_seq_len_dim and not isinstance(seq_len, int):
            raise ValueError("seq_len must be provided when we need to keep seq_len dim.")
        self.reset()

    def reset(self):
        self.sums = None             # fp64 [3, T']: sum (p - t)^2, sum |p - t|, sum of the frames' SSIM
        self.counts = None           # int64 [2, T']: elements, frames
        self._ws = None
        self._range = None           # 2 floats on the device: the value ranges of the last data_range=None update

    def _alloc_state(self, dev):
        Tk = self.seq_len if self.keep_seq_len_dim else 1
        self.sums = torch.zeros((3, Tk), dtype=torch.float64, device=dev)
        self.counts = torch.zeros((2, Tk), dtype=torch.int64, device=dev)

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        if pred.dim() != len(self.layout) or tuple(pred.shape) != tuple(target.shape):
            raise ValueError(f"pred and target must have one shape in layout {self.layout!r}; got {tuple(pred.shape)} and "
                             f"{tuple(target.shape)}")
        self._launch(pred.unsqueeze(0), target, self.data_range)

    def update_members(self, ens: torch.Tensor, target: torch.Tensor):
        if self.data_range is None:
            raise ValueError("update_members needs an explicit data_range: the per-call range of data_range=None is undefined for a "
                             "stacked ensemble")
        if ens.dim() != len(self.layout) + 1 or tuple(ens.shape[1:]) != tuple(target.shape):
            raise ValueError(f"ens must be (M,) + target.shape with target in layout {self.layout!r}; got {tuple(ens.shape)} "
                             f"and {tuple(target.shape)}")
        if not 1 <= ens.shape[0] <= MAX_MEMBERS:
            raise ValueError(f"{ens.shape[0]} members: 1 .. {MAX_MEMBERS} are supported")
        self._launch(ens, target, self.data_range)

    def _launch(self, ens, target, data_range):
        if not (ens.is_cuda and target.is_cuda):
            raise L.PrediffHipError("SEVIRFrameScore.update runs on the HIP device the frames were decoded on")
        if self.keep_seq_len_dim:
            assert target.shape[self.layout.find("T")] == self.seq_len
        dev = ens.device
        if self.sums is None:
            self._alloc_state(dev)
        elif self.sums.device != dev:            # a zero state that sync() made before this rank's first update
            self.sums, self.counts = self.sums.to(dev), self.counts.to(dev)
        x, y = ens.detach().float(), target.detach().float()          # read in place through their strides
        M = x.shape[0]
        sizes, xs = axes_of(self.layout, x, lead=1)
        _, ys = axes_of(self.layout, y)
        need = L.frame_score_ws_doubles(M, sizes)
        if need > 0 and (self._ws is None or self._ws.numel() < need or self._ws.device != dev):
            self._ws = torch.empty(need, dtype=torch.float64, device=dev)
        if self._ws is None:                     # an unsupported shape: the launch below says which
            self._ws = torch.empty(1, dtype=torch.float64, device=dev)
        if data_range is None and (self._range is None or self._range.device != dev):
            self._range = torch.empty(2, dtype=torch.float32, device=dev)
        with L.on_device(ens):
            L.frame_score_update(x, y, M, sizes, [x.stride(0)] + xs, ys, 0.0 if data_range is None else data_range,
                                 self._range if data_range is None else None, self.keep_seq_len_dim, self.sums, self.counts, self._ws)

    def sync(self, group=None):
        """All-reduce the state with SUM over the ranks of `group`; every rank must call it, including ranks that made no update
        (they take part with a zero state)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self.sums is None:
            nccl = dist.get_backend(group) == "nccl"
            self._alloc_state(torch.device("cuda", torch.cuda.current_device()) if nccl else torch.device("cpu"))
        for t in (self.sums, self.counts):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def _finish(self, per_t):
        """per_t: (T',) scores -> the mode's form (scalar for "0" and "2", (T,) array for "1")."""
        if self.mode == "0":
            return float(per_t[0])
        if self.mode == "1":
            return per_t
        return float(np.mean(per_t))

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
