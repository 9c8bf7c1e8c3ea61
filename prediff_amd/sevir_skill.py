"""SEVIR skill scores (CSI / POD / SUCR / BIAS) on the decoded frames -- reference ``SEVIRSkillScore``
(datasets/sevir/evaluation.py:88-285) without the torchmetrics dependency.

Same constructor keywords, ``update(pred, target)`` / ``compute()`` / ``reset()`` and result dictionary; the counting
(the only per-pixel work) is ONE launch of pd_sevir_skill_counts instead of the reference's per-threshold loop.
``preprocess_type="sevir_pool{s}"`` (evaluation.py:220-231: max-pool over (H, W) with kernel = stride = s, the CSI-pool4 /
CSI-pool16 scores) is one launch of pd_sevir_skill_counts_pooled, which reads the frames in place through their strides in any
5-letter layout (the reference's rearrange needs all of N, T, H, W, C, so a 4-letter layout is refused at construction).  Counts
are exact int64, so scores match the reference bit for bit given the same frames.  `sync()` sums the counters over the
ranks of a process group (what torchmetrics' dist_reduce_fx="sum" does at compute time).
"""
import re
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L

AXES = "NTHWC"


def parse_preprocess(preprocess_type: str, layout: str) -> int:
    """Pool scale of a preprocess_type ("sevir": 1, "sevir_pool{s}": s, the first integer in the string as in the reference);
    a pooled preprocess needs a layout that names N, T, H, W and C."""
    if preprocess_type == "sevir":
        return 1
    if not preprocess_type.startswith("sevir_pool"):
        raise NotImplementedError(f"preprocess_type {preprocess_type!r}: only 'sevir' and 'sevir_pool{{s}}' are implemented")
    m = re.search(r"\d+", preprocess_type)
    if m is None or int(m.group()) < 1:
        raise ValueError(f"preprocess_type {preprocess_type!r}: no positive pool scale")
    if sorted(layout) != sorted(AXES):
        raise ValueError(f"preprocess_type {preprocess_type!r} pools over H and W and needs a layout of the letters N, T, H, W, C; "
                         f"got {layout!r}")
    return int(m.group())


def axes_of(layout: str, x: torch.Tensor, lead: int = 0):
    """(sizes, strides) of x's N, T, H, W, C axes (after `lead` leading axes); an axis the layout does not name has size 1, stride 0."""
    sizes, strides = [], []
    for a in AXES:
        i = layout.find(a)
        sizes.append(x.shape[lead + i] if i >= 0 else 1)
        strides.append(x.stride(lead + i) if i >= 0 else 0)
    return sizes, strides


class SEVIRSkillScore:
    def __init__(self, layout: str = "NHWT", mode: str = "0", seq_len: Optional[int] = None, preprocess_type: str = "sevir",
                 threshold_list: Sequence[int] = (16, 74, 133, 160, 181, 219),
                 metrics_list: Sequence[str] = ("csi", "bias", "sucr", "pod"), eps: float = 1e-4):
        self.preprocess_type = preprocess_type
        self.pool_scale = parse_preprocess(preprocess_type, layout)
        self.pooled = preprocess_type != "sevir"
        if mode not in ("0", "1", "2"):
            raise NotImplementedError(f"mode {mode} not supported!")
        self.layout, self.mode, self.seq_len = layout, mode, seq_len
        self.threshold_list, self.metrics_list, self.eps = tuple(threshold_list), tuple(metrics_list), eps
        self.keep_seq_len_dim = mode in ("1", "2")
        if self.keep_seq_len_dim:
            assert isinstance(seq_len, int), "seq_len must be provided when we need to keep seq_len dim."
        self._counts = None          # int64 (n_thr, T or 1, 3) on the device of the first update
        self._thr = None

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

    def reset(self):
        self._counts = None

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        assert pred.shape == target.shape and pred.dim() == len(self.layout)
        if not pred.is_cuda:
            raise L.PrediffHipError("SEVIRSkillScore.update runs on the HIP device the frames were decoded on")
        ta = self.layout.find("T")
        T = pred.shape[ta]
        if self.keep_seq_len_dim:
            assert T == self.seq_len
        outer = int(np.prod(pred.shape[:ta])) if ta > 0 else 1
        inner = int(np.prod(pred.shape[ta + 1:])) if ta + 1 < pred.dim() else 1
        dev = pred.device
        if self._counts is None:
            self._counts = torch.zeros((len(self.threshold_list), T if self.keep_seq_len_dim else 1, 3), dtype=torch.int64, device=dev)
            self._thr = torch.tensor(self.threshold_list, dtype=torch.float32, device=dev)
        divisor = float(np.float32(1.0 / 255.0))       # data.float() / PREPROCESS_SCALE_01['vil'] (sevir_dataloader.py:679)
        if self.pooled:
            p, q = pred.detach().float(), target.detach().float()       # read in place through their strides
            sizes, ps = axes_of(self.layout, p)
            _, qs = axes_of(self.layout, q)
            with L.on_device(pred):
                L.sevir_skill_counts_pooled(p, q, self._thr, divisor, self._counts, sizes, ps, qs, self.pool_scale, self.keep_seq_len_dim)
            return
        with L.on_device(pred):
            L.sevir_skill_counts(pred.detach().float().contiguous(), target.detach().float().contiguous(), self._thr, divisor,
                                 self._counts, outer, T, inner, self.keep_seq_len_dim)

    def sync(self, group=None):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and self._counts is not None:
            dist.all_reduce(self._counts, op=dist.ReduceOp.SUM, group=group)

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
