"""Ensemble verification of SEVIR frames: CRPS, fair CRPS, Brier score, ensemble-mean RMSE and spread, on the device.

Not in the reference: its evaluation stops at the per-sample ``SEVIRSkillScore`` (datasets/sevir/evaluation.py:88-285); this class
scores the M members of one forecast *as an ensemble* (what ``ensemble.sample_ensemble`` returns).  Constructor keywords follow
``SEVIRSkillScore`` (``layout``, ``mode``, ``seq_len``, ``preprocess_type`` "sevir" / "sevir_pool{s}", ``threshold_list``, ``eps``);
both the members and the target are preprocessed exactly as there (divided by fp32(1/255), then max-pooled over (H, W) for
"sevir_pool{s}").  A pooled pixel is valid when the target and all M members are non-NaN there.  Per valid pixel, with members x_1..x_M,
observation y and ensemble mean m:

    crps      = (1/M) sum_i |x_i - y| - 1/(2 M^2) sum_ij |x_i - x_j|
    crps_fair = (1/M) sum_i |x_i - y| - 1/(2 M (M - 1)) sum_ij |x_i - x_j|            (NaN for M = 1)
    brier     = sum (c - M o)^2 / (M^2 n_valid),  c = #{x_i >= thr}, o = [y >= thr]  (the sum is exact int64)
    rmse      = sqrt(sum (m - y)^2 / n_valid)
    spread    = sqrt(sum s^2 / n_valid),  s^2 = sum_i (x_i - m)^2 / (M - 1)         (NaN for M = 1)

``update(ens, target)``: ens is (M,) + target.shape on the device, target is in ``layout``; one ``sample_ensemble`` result of one context
scores as ``update(ens.unsqueeze(1), target)`` with ``layout="NTHWC"``.  One launch of pd_ensemble_score_update reads every member value
once, in place through its strides; the floating sums are reduced in a fixed order (the same inputs give the same bits).  State: int64
n_valid[T], int64 Brier sums [thr, T], fp64 sums [T] of the absolute-error, pairwise, squared-error and variance terms; it accumulates
over updates (all with the same M) until ``reset()``.  ``sync(group)`` all-reduces it with SUM and must be called on every rank of the
group, also on ranks that made no update: ``sample_ensemble`` hands the whole ensemble to every rank, so each context must be updated
on exactly ONE rank before the sync (or the context counts world-size times).
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .score_base import SEVIRScoreBase, parse_preprocess, thresholds_on

METRICS = ("crps", "crps_fair", "brier", "rmse", "spread")


class SEVIREnsembleScore(SEVIRScoreBase):
    METRICS = METRICS
    SEQ_LEN_ERROR = AssertionError   # as SEVIRSkillScore
    STATE = (("n_valid", torch.int64, lambda self, Tk: (Tk,)),
             ("brier_sums", torch.int64, lambda self, Tk: (len(self.threshold_list), Tk)),
             ("sums", torch.float64, lambda self, Tk: (4, Tk)))      # sum |x - y|, sum_ij |x_i - x_j|, (m - y)^2, s^2

    def __init__(self, layout: str = "NHWT", mode: str = "0", seq_len: Optional[int] = None, preprocess_type: str = "sevir",
                 threshold_list: Sequence[int] = (16, 74, 133, 160, 181, 219),
                 metrics_list: Sequence[str] = METRICS, eps: float = 1e-4):
        # eps: accepted for keyword parity with SEVIRSkillScore; no score here divides by a count that eps would guard
        self.threshold_list, self.eps = tuple(threshold_list), eps
        super().__init__(layout, mode, seq_len, metrics_list)
        if not 1 <= len(threshold_list) <= 8:
            raise ValueError("1 to 8 thresholds are supported")
        self.preprocess_type = preprocess_type
        self.pool_scale = parse_preprocess(preprocess_type, layout)

    def reset(self):
        super().reset()
        self.num_members = None      # M of the updates so far
        self._thr = None

    def update(self, ens: torch.Tensor, target: torch.Tensor):
        x, y, M, sizes, xs, ys = self._members(ens, target)
        if self.num_members is not None and M != self.num_members:
            raise ValueError(f"{M} members after updates with {self.num_members}: reset() first")
        dev = ens.device
        self._state_on(dev)
        self._thr = thresholds_on(self._thr, self.threshold_list, dev)
        ws = self._workspace(L.ensemble_score_ws_doubles(M, sizes, self.pool_scale), torch.float64, dev)
        divisor = float(np.float32(1.0 / 255.0))       # as SEVIRSkillScore
        with L.on_device(ens):
            L.ensemble_score_update(x, y, self._thr, divisor, M, sizes, xs, ys, self.pool_scale, self.keep_seq_len_dim,
                                    self.n_valid, self.brier_sums, self.sums, ws)
        self.num_members = M

    def _sync_more(self, dist, group):
        """The member count is agreed as well: ranks that made updates must have used the same M (ValueError on every rank otherwise)."""
        # [max M, -min M] over the ranks with updates (a rank without any contributes 0 and -2^40)
        m = self.num_members
        mm = torch.tensor([m, -m] if m is not None else [0, -(1 << 40)], dtype=torch.int64, device=self.n_valid.device)
        dist.all_reduce(mm, op=dist.ReduceOp.MAX, group=group)
        hi, lo = int(mm[0]), -int(mm[1])
        if hi > 0 and hi != lo:
            raise ValueError(f"sync: ranks updated with different member counts ({lo} .. {hi})")
        if hi > 0:
            self.num_members = hi

    def compute(self):
        Tk = self.seq_len if self.keep_seq_len_dim else 1
        if self.n_valid is None:
            n, br, s, M = np.zeros(Tk, np.int64), np.zeros((len(self.threshold_list), Tk), np.int64), np.zeros((4, Tk)), 1
        else:
            n, br, s, M = self.n_valid.cpu().numpy(), self.brier_sums.cpu().numpy(), self.sums.cpu().numpy(), self.num_members or 1
        nf = n.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            per = {
                "crps": (s[0] / M - s[1] / (2.0 * M * M)) / nf,
                "crps_fair": (s[0] / M - s[1] / (2.0 * M * (M - 1))) / nf if M > 1 else np.full(Tk, np.nan),
                "rmse": np.sqrt(s[2] / nf),
                "spread": np.sqrt(s[3] / nf) if M > 1 else np.full(Tk, np.nan),
            }
            brier = br.astype(np.float64) / (float(M) * M * nf)          # [thr, T']
        ret = {thr: {} for thr in self.threshold_list}
        ret["avg"] = {}
        for met in self.metrics_list:
            if met == "brier":
                for i, thr in enumerate(self.threshold_list):
                    ret[thr]["brier"] = self._finish(brier[i])
                ret["avg"]["brier"] = self._finish(brier.mean(axis=0))
            else:
                ret[met] = self._finish(per[met])
        return ret
