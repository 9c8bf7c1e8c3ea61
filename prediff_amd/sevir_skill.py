"""SEVIR skill scores (CSI / POD / SUCR / BIAS) on the decoded frames -- reference ``SEVIRSkillScore``
(datasets/sevir/evaluation.py:88-285) without the torchmetrics dependency.

Same constructor keywords, ``update(pred, target)`` / ``compute()`` / ``reset()`` and result dictionary; the counting
(the only per-pixel work) is ONE launch of pd_sevir_skill_counts instead of the reference's per-threshold loop.
``preprocess_type="sevir_pool{s}"`` (evaluation.py:220-231: max-pool over (H, W) with kernel = stride = s, the CSI-pool4 /
CSI-pool16 scores) is one launch of pd_sevir_skill_counts_pooled, which reads the frames in place through their strides in any
5-letter layout (the reference's rearrange needs all of N, T, H, W, C, so a 4-letter layout is refused at construction).  Counts
are exact int64, so scores match the reference bit for bit given the same frames.  `sync()` sums the counters over the
ranks of a process group (what torchmetrics' dist_reduce_fx="sum" does at compute time); every rank of the group calls it, a rank
that made no update takes part with zero counters (score_base.py).
"""
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .score_base import AXES, axes_of, parse_preprocess  # noqa: F401  (their home until score_base.py: still imported from here)
from .score_base import SEVIRScoreBase, thresholds_on


class SEVIRSkillScore(SEVIRScoreBase):
    LAYOUT_CHECKED = False           # as the reference: any layout with a T that parse_preprocess accepts
    SEQ_LEN_ERROR = AssertionError   # the reference asserts
    STATE = (("_counts", torch.int64, lambda self, Tk: (len(self.threshold_list), Tk, 3)),)      # hits, misses, false alarms

    def __init__(self, layout: str = "NHWT", mode: str = "0", seq_len: Optional[int] = None, preprocess_type: str = "sevir",
                 threshold_list: Sequence[int] = (16, 74, 133, 160, 181, 219),
                 metrics_list: Sequence[str] = ("csi", "bias", "sucr", "pod"), eps: float = 1e-4):
        self.preprocess_type = preprocess_type
        self.pool_scale = parse_preprocess(preprocess_type, layout)
        self.pooled = preprocess_type != "sevir"
        self.threshold_list, self.eps = tuple(threshold_list), eps
        self._thr = None
        super().__init__(layout, mode, seq_len, metrics_list)

    # reference state attributes (float tensors there; exact integers here)
    @property
    def hits(self):
        return self._state(0)

    @property
    def misses(self):
        return self._state(1)

    @property
    def fas(self):
        return self._state(2)

    def _state(self, k):
        if self._counts is None:
            shape = (len(self.threshold_list), self.seq_len) if self.keep_seq_len_dim else (len(self.threshold_list),)
            return torch.zeros(shape)
        c = self._counts[..., k].float()
        return c if self.keep_seq_len_dim else c[:, 0]

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        assert pred.shape == target.shape and pred.dim() == len(self.layout)
        if not pred.is_cuda:
            raise L.PrediffHipError("SEVIRSkillScore.update runs on the HIP device the frames were decoded on")
        ta = self.layout.find("T")
        T = pred.shape[ta]
        if self.keep_seq_len_dim:
            assert T == self.seq_len
        self._state_on(pred.device)
        self._thr = thresholds_on(self._thr, self.threshold_list, pred.device)
        divisor = float(np.float32(1.0 / 255.0))       # data.float() / PREPROCESS_SCALE_01['vil'] (sevir_dataloader.py:679)
        if self.pooled:
            p, q = pred.detach().float(), target.detach().float()       # read in place through their strides
            sizes, ps = axes_of(self.layout, p)
            _, qs = axes_of(self.layout, q)
            with L.on_device(pred):
                L.sevir_skill_counts_pooled(p, q, self._thr, divisor, self._counts, sizes, ps, qs, self.pool_scale, self.keep_seq_len_dim)
            return
        outer, inner = math.prod(pred.shape[:ta]), math.prod(pred.shape[ta + 1:])
        with L.on_device(pred):
            L.sevir_skill_counts(pred.detach().float().contiguous(), target.detach().float().contiguous(), self._thr, divisor,
                                 self._counts, outer, T, inner, self.keep_seq_len_dim)

    @staticmethod
    def pod(hits, misses, fas, eps):
        return hits / (hits + misses + eps)

    @staticmethod
    def sucr(hits, misses, fas, eps):
        return hits / (hits + fas + eps)

    @staticmethod
    def csi(hits, misses, fas, eps):
        return hits / (hits + misses + fas + eps)

    @staticmethod
    def bias(hits, misses, fas, eps):
        b = (hits + fas) / (hits + misses + eps)
        return torch.pow(b / torch.log(torch.tensor(2.0)), 2.0)

    def compute(self):
        fn = {"pod": self.pod, "csi": self.csi, "sucr": self.sucr, "bias": self.bias}
        hits, misses, fas = self.hits.cpu(), self.misses.cpu(), self.fas.cpu()
        ret = {thr: {} for thr in self.threshold_list}
        ret["avg"] = {}
        for met in self.metrics_list:
            scores = fn[met](hits, misses, fas, self.eps).numpy()
            avg = np.zeros((self.seq_len,)) if self.keep_seq_len_dim else 0
            for i, thr in enumerate(self.threshold_list):
                score = scores[i] if self.keep_seq_len_dim else scores[i].item()
                ret[thr][met] = np.mean(score).item() if self.mode == "2" else score
                avg = avg + score
            avg = avg / len(self.threshold_list)
            ret["avg"][met] = np.mean(avg).item() if self.mode == "2" else avg
        return ret
