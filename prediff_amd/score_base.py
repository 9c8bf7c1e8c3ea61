"""What the seven SEVIR score classes share (``SEVIRSkillScore``, ``SEVIREnsembleScore``, ``SEVIRFrameScore``, ``SEVIRSpectralScore``,
``SEVIRObjectScore``, ``SEVIRDistanceScore``, ``SEVIRScaleScore``):
the N, T, H, W, C view of a tensor in a layout, the constructor checks, the life cycle of the accumulated state and its ``sync``, the
member-stack checks of ``update`` and the workspace.  A subclass declares its metrics, its state tensors and what its layout must
name; ``update`` and ``compute`` are its own.
"""
import re
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L

AXES = "NTHWC"
MAX_MEMBERS = 512            # members of one update (the limit of the kernels)


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
    shape, stride = x.shape, x.stride()
    at = [layout.find(a) for a in AXES]
    return [shape[lead + i] if i >= 0 else 1 for i in at], [stride[lead + i] if i >= 0 else 0 for i in at]


def thresholds_on(held: Optional[torch.Tensor], threshold_list, dev) -> torch.Tensor:
    """The thresholds as fp32 on `dev`: `held` when it is that already."""
    if held is None or held.device != dev:
        held = torch.tensor(threshold_list, dtype=torch.float32, device=dev)
    return held


class SEVIRScoreBase:
    METRICS: Optional[Sequence[str]] = None      # the metrics a metrics_list may name; None: not checked at construction
    LAYOUT_CHECKED = True                        # distinct letters of N, T, H, W, C with N and T present ...
    LAYOUT_NEEDS_HW = None                       # ... and, where this is a reason text, H and W as well
    SEQ_LEN_ERROR = ValueError                   # what mode "1" / "2" without seq_len raises
    # the accumulated state: (attribute, dtype, shape(self, Tk)) per tensor; None until the first update or sync
    STATE = ()

    def __init__(self, layout: str, mode: str, seq_len: Optional[int], metrics_list: Sequence[str]):
        if mode not in ("0", "1", "2"):
            raise NotImplementedError(f"mode {mode} not supported!")
        if self.LAYOUT_CHECKED:
            if "N" not in layout or "T" not in layout or len(set(layout)) != len(layout) or set(layout) - set(AXES):
                raise ValueError(f"layout {layout!r}: distinct letters of N, T, H, W, C with N and T present")
            if self.LAYOUT_NEEDS_HW and ("H" not in layout or "W" not in layout):
                raise ValueError(f"layout {layout!r}: {self.LAYOUT_NEEDS_HW}, both must be named")
        if self.METRICS is not None:
            bad = [m for m in metrics_list if m not in self.METRICS]
            if bad:
                raise ValueError(f"unknown metrics {bad}; supported: {self.METRICS}")
        self.layout, self.mode, self.seq_len = layout, mode, seq_len
        self.metrics_list = tuple(metrics_list)
        self.keep_seq_len_dim = mode in ("1", "2")
        if self.keep_seq_len_dim and not isinstance(seq_len, int):
            raise self.SEQ_LEN_ERROR("seq_len must be provided when we need to keep seq_len dim.")
        self.reset()

    # ---- state ------------------------------------------------------------------------------------------------------------------
    @property
    def Tk(self):
        """Lead times the state keeps apart (T' of the subclasses' docstrings)."""
        return self.seq_len if self.keep_seq_len_dim else 1

    def reset(self):
        for name, _, _ in self.STATE:
            setattr(self, name, None)
        self._ws = None

    def _alloc_state(self, dev):
        for name, dtype, shape in self.STATE:
            setattr(self, name, torch.zeros(shape(self, self.Tk), dtype=dtype, device=dev))

    def _state_tensors(self):
        return [getattr(self, name) for name, _, _ in self.STATE]

    def _state_on(self, dev):
        """The state for an update on `dev`: zeros at the first one; a zero state that sync() made before this rank's first update moves."""
        first = getattr(self, self.STATE[0][0])
        if first is None:
            self._alloc_state(dev)
        elif first.device != dev:
            for name, _, _ in self.STATE:
                setattr(self, name, getattr(self, name).to(dev))

    def sync(self, group=None):
        """All-reduce the state with SUM over the ranks of `group`; every rank must call it, including ranks that made no update
        (they take part with a zero state: on the current CUDA device for nccl, on the CPU otherwise)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if getattr(self, self.STATE[0][0]) is None:
            nccl = dist.get_backend(group) == "nccl"
            self._alloc_state(torch.device("cuda", torch.cuda.current_device()) if nccl else torch.device("cpu"))
        for t in self._state_tensors():
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self._sync_more(dist, group)

    def _sync_more(self, dist, group):
        """What a subclass agrees on besides the sums (called on every rank, after them)."""

    def _finish(self, per_t):
        """per_t: (T', ...) -> the mode's form: [0] for "0", the array for "1", the mean over lead times for "2" (floats for 1-D input)."""
        if self.mode == "0":
            return per_t[0] if per_t.ndim > 1 else float(per_t[0])
        if self.mode == "1":
            return per_t
        return np.mean(per_t, axis=0) if per_t.ndim > 1 else float(np.mean(per_t))

    # ---- update -----------------------------------------------------------------------------------------------------------------
    def _members(self, ens: torch.Tensor, target: torch.Tensor):
        """Check a member stack ens = (M,) + target.shape against its target (in `layout`, on the HIP device) and return
        (x, y, M, sizes, member_strides, target_strides): the fp32 views the kernels read in place through their strides,
        member_strides with the M axis first."""
        if ens.dim() != len(self.layout) + 1 or ens.shape[1:] != target.shape:
            raise ValueError(f"ens must be (M,) + target.shape with target in layout {self.layout!r}; got {tuple(ens.shape)} "
                             f"and {tuple(target.shape)}")
        M = ens.shape[0]
        if not 1 <= M <= MAX_MEMBERS:
            raise ValueError(f"{M} members: 1 .. {MAX_MEMBERS} are supported")
        if not (ens.is_cuda and target.is_cuda):
            raise L.PrediffHipError(f"{type(self).__name__}.update runs on the HIP device the frames were decoded on")
        if self.keep_seq_len_dim:
            assert target.shape[self.layout.find("T")] == self.seq_len
        x, y = ens.detach().float(), target.detach().float()
        sizes, xs = axes_of(self.layout, x, lead=1)
        _, ys = axes_of(self.layout, y)
        return x, y, M, sizes, [x.stride(0)] + xs, ys

    def _workspace(self, n: int, dtype, dev: torch.device):
        """A buffer of at least n elements on `dev`, kept between updates; it grows, and follows the updates to another device."""
        ws = self._ws
        if ws is None or ws.numel() < n or ws.device != dev:
            ws = self._ws = torch.empty(n, dtype=dtype, device=dev)
        return ws
