"""Intensity-scale verification on the device: the Haar energies of a frame's event field (``scale_energy``) and the intensity-scale skill
score with the energies of forecast and observation per lead time, threshold and spatial scale (``SEVIRScaleScore``).
Not in the reference; the score is Casati, Ross and Stephenson 2004 (Meteorol. Appl. 11, 141) and Casati 2010 (Wea. Forecasting 25, 113)
for frames that are not dyadic, as MET's Wavelet-Stat tool and pysteps' intensity_scale.

A frame is one (n, t) image of H x W pixels (C is 1 or absent from the layout; sides 1 to 128, the frame's bit planes live in LDS).

    event set      for threshold thr_k of ``threshold_list`` (on the 0-255 scale): pixel s is an event when float32(x[s]) / float32(1/255)
                   >= float32(thr_k), the IEEE division and comparison of pd_sevir_skill_counts: exactly the sets CSI and
                   SEVIRDistanceScore use.  A NaN is never an event.  I_F, I_O: the 0 / 1 event fields of forecast and observation;
                   Z = I_F - I_O.
    padding        the frame sits at the top-left corner of an S x S field whose other pixels hold no event in either field, S = 2^n the
                   smallest power of two >= max(H, W, 2) (n = 1 .. 7), and N = S^2 is the area of every normalisation (MET's "pad").
    components     F_l(A): the field of 2^l x 2^l block means of A (F_0 = A); W_l = F_{l-1} - F_l for l = 1 .. n, and F_n, the domain
                   mean: L = n + 1 orthogonal components that sum to A.  Component l carries features of 2^(l-1) pixels, the last one
                   the domain bias.
    integer form   Q_l(A), l = 0 .. n: the sum over the 2^l-blocks of (block sum of A)^2, an integer <= 4^(n + l) <= 2^28.  Then
                       mean(W_l(A)^2) = (4 Q_{l-1} - Q_l) / (4^l N)   for l = 1 .. n,        mean(F_n(A)^2) = Q_n / (4^n N),
                   and sum over l = 1 .. n of (4 Q_{l-1} - Q_l) 4^(n-l), plus Q_n, equals 4^n Q_0 on the integers (Parseval).
                   Q_0(I_F), Q_0(I_O) are the event counts, Q_0(Z) is misses + false alarms.  The device computes only Q(I_F), Q(I_O)
                   and Q(Z): after the event test nothing is floating point, so the state is exact and independent of any order.

``scale_energy(frames, threshold)`` is the primitive: Q_l of every frame's event field.
``update(pred, target)``: equal shapes in ``layout``, any dtype (read as ``.float()``), in place through their strides.
``update_members(ens, target)``: ens is (M,) + target.shape and scores as M ``update(ens[i], target)`` calls would; the target's bit
planes are made once.  State, K thresholds: int64 ``energy`` [3, K, 8, T'] (Q of I_F, I_O, Z; levels above n stay zero) and int64
``counts`` [2, T'] (pairs scored, pairs skipped), accumulated until ``reset()``; ``sync`` is the base's, and the ranks agree on n.  A pair
in which either frame holds a non-finite pixel adds 1 to ``skipped`` and nothing else.  The first update fixes n (``levels`` = n + 1); a
later update whose frames pad to another S raises ValueError.

``compute()``, per lead time, pooled over the P = counts[0] pairs that were scored; every difference 4 Q_{l-1} - Q_l is formed in int64
and divided once in fp64:

    mse (T', K, L)             the component mean squares of Z by the two formulas above on the pooled Q(Z), divided by P
    mse_random (T', K)         B_f (1 - B_o) + B_o (1 - B_f), B_f = Q_0(I_F) / (N P), B_o = Q_0(I_O) / (N P): the MSE of a random placement
                               of the same numbers of events (MET's form, which does not assume an unbiased forecast)
    iss (T', K, L)             1 - L mse_l / mse_random: 1 is perfect, 0 the random placement, negative is worse than that at this scale
    energy_pred, energy_target (T', K, L)   the same component formulas on the pooled Q(I_F) and Q(I_O)
    energy_bias (T', K, L)     (energy_pred - energy_target) / (energy_pred + energy_target): Casati's relative energy difference
    base_rate, freq_bias (T', K)            B_o;  Q_0(I_F) / Q_0(I_O)

Each metric follows ``mode`` ("0": pooled over all lead times, "1": per lead time, "2": the mean of the per-lead-time values).  A zero
denominator gives NaN.  Before any update ``levels`` is None and the level axis of the results is empty.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .score_base import AXES, SEVIRScoreBase, axes_of

METRICS = ("mse", "mse_random", "iss", "energy_pred", "energy_target", "energy_bias", "base_rate", "freq_bias")
MAX_THRESHOLDS = 8
MAX_LEVELS = 8                                 # Q_0 .. Q_7: sides up to 128
DIVISOR = float(np.float32(1.0 / 255.0))       # as SEVIRSkillScore


def top_level(H: int, W: int) -> int:
    """n with S = 2^n the smallest power of two >= max(H, W, 2)"""
    return max(int(max(H, W) - 1).bit_length(), 1)


def scale_energy(frames: torch.Tensor, threshold: float, layout: str = "NTHWC", scaled: bool = True) -> torch.Tensor:
    """Q_l, l = 0 .. n, of the event field of every frame, padded as the module docstring says: int64 (N, T, n + 1).
    scaled=False compares the raw value with float32(threshold), with no division by float32(1/255)."""
    if len(set(layout)) != len(layout) or set(layout) - set(AXES) or set("NTHW") - set(layout) or frames.dim() != len(layout):
        raise ValueError(f"layout {layout!r}: distinct letters of N, T, H, W, C naming N, T, H and W, one per axis of frames "
                         f"{tuple(frames.shape)}")
    if not frames.is_cuda:
        raise L.PrediffHipError("scale_energy runs on the HIP device the frames were decoded on")
    x = frames.detach().float()
    sizes, strides = axes_of(layout, x)
    if sizes[4] != 1:
        raise ValueError(f"C = {sizes[4]}: event fields are made of one channel")
    N, T, H, W = sizes[:4]
    q = torch.empty((N, T, MAX_LEVELS), dtype=torch.int64, device=x.device)
    with L.on_device(x):
        L.scale_energy(x, sizes, strides, threshold, DIVISOR if scaled else 1.0, q)
    return q[..., :top_level(H, W) + 1]


def component_means(q: np.ndarray, n: int, area_pairs: np.ndarray) -> np.ndarray:
    """q: int64 (..., n + 1) pooled Q_0 .. Q_n; area_pairs: int64 (...) = N P.  -> fp64 (..., n + 1): mean(W_l^2) for l = 1 .. n, then
    mean(F_n^2), over the N pixels of the P pairs; the differences in int64, one fp64 division each."""
    num = np.concatenate([4 * q[..., :-1] - q[..., 1:], q[..., -1:]], axis=-1)
    den = area_pairs[..., None] * np.array([4 ** l for l in range(1, n + 1)] + [4 ** n], dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return num.astype(np.float64) / den.astype(np.float64)


class SEVIRScaleScore(SEVIRScoreBase):
    METRICS = METRICS
    LAYOUT_NEEDS_HW = "scales are separated over H and W"
    STATE = (("energy", torch.int64, lambda self, Tk: (3, len(self.threshold_list), MAX_LEVELS, Tk)),     # Q_l of I_F, I_O, Z
             ("counts", torch.int64, lambda self, Tk: (2, Tk)))                                           # pairs, skipped

    def __init__(self, layout: str = "NTHWC", mode: str = "0", seq_len: Optional[int] = None,
                 threshold_list: Sequence[float] = (16, 74, 133, 160, 181, 219), metrics_list: Sequence[str] = METRICS):
        threshold_list = tuple(float(t) for t in threshold_list)
        if not 1 <= len(threshold_list) <= MAX_THRESHOLDS:
            raise ValueError(f"{len(threshold_list)} thresholds: 1 .. {MAX_THRESHOLDS} are supported")
        self.threshold_list = threshold_list
        super().__init__(layout, mode, seq_len, metrics_list)

    def reset(self):
        super().reset()
        self._n = None               # S = 2^n of the updates so far

    @property
    def levels(self):
        """L = n + 1, the components per threshold; None before the first update."""
        return None if self._n is None else self._n + 1

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
            raise ValueError(f"C = {sizes[4]}: event fields are made of one channel")
        n = top_level(sizes[2], sizes[3])
        if self._n is not None and n != self._n:
            raise ValueError(f"{sizes[2]} x {sizes[3]} frames pad to a side of {2 ** n} after updates with {2 ** self._n}: reset() first")
        dev = ens.device
        self._state_on(dev)
        # an unsupported shape (no size, -1) gets one element: the launch below says which
        ws = self._workspace(max(L.scale_ws_bytes(M, len(self.threshold_list), sizes) // 8, 1), torch.float64, dev)
        with L.on_device(ens):
            L.scale_update(x, y, M, sizes, xs, ys, self.threshold_list, DIVISOR, self.keep_seq_len_dim, self.energy, self.counts, ws)
        self._n = n

    def _sync_more(self, dist, group):
        """The padded side is agreed as well: a rank without updates takes the others' n; two different ones raise ValueError on every
        rank."""
        # [max n, -min n] over the ranks with updates (a rank without any contributes 0 and -2^40)
        n = self._n
        nn = torch.tensor([n, -n] if n is not None else [0, -(1 << 40)], dtype=torch.int64, device=self.counts.device)
        dist.all_reduce(nn, op=dist.ReduceOp.MAX, group=group)
        hi, lo = int(nn[0]), -int(nn[1])
        if hi > 0 and hi != lo:
            raise ValueError(f"sync: ranks updated with frames that pad to different sides ({2 ** lo} .. {2 ** hi})")
        if hi > 0:
            self._n = hi

    def compute(self):
        K, Tk, n = len(self.threshold_list), self.Tk, self._n
        if self.energy is None:
            e, c = np.zeros((3, K, MAX_LEVELS, Tk), np.int64), np.zeros((2, Tk), np.int64)
        else:
            e, c = self.energy.cpu().numpy(), self.counts.cpu().numpy()
        nl = 0 if n is None else n + 1
        q = e.transpose(0, 3, 1, 2)[..., :nl]                                                  # per lead time: (3, T', K, L)
        area_pairs = np.broadcast_to((c[0] * 4 ** (n or 0))[:, None], (Tk, K))                 # N P
        q0 = (e[:, :, 0, :].transpose(0, 2, 1)).astype(np.float64)                             # (3, T', K): events of F, of O; misses + false alarms
        if nl:
            comp = [component_means(q[a], n, area_pairs) for a in range(3)]
        else:
            comp = [np.zeros((Tk, K, 0))] * 3
        with np.errstate(divide="ignore", invalid="ignore"):
            bf, bo = q0[0] / area_pairs.astype(np.float64), q0[1] / area_pairs.astype(np.float64)
            rnd = bf * (1.0 - bo) + bo * (1.0 - bf)
            per = {"mse": comp[2], "mse_random": rnd, "iss": 1.0 - nl * comp[2] / rnd[..., None], "energy_pred": comp[0],
                   "energy_target": comp[1], "energy_bias": (comp[0] - comp[1]) / (comp[0] + comp[1]), "base_rate": bo,
                   "freq_bias": np.where(q0[1] > 0, q0[0] / q0[1], np.nan)}
        return {met: self._finish(per[met]) for met in self.metrics_list}
