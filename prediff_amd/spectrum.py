"""Radially averaged power spectra of forecasts and observations on the device: what a score that counts exceedances or pixel errors
cannot see -- the loss of small scales (blur).

The diagnostic of the nowcasting literature (DGMR, LDCast, pysteps' ``rapsd``): the radially averaged power spectral density (RAPSD) of
forecast and observation per lead time, and with it their spectral coherence, the scale below which the forecast carries no information
about the truth.  Constructor keywords follow ``SEVIRFrameScore`` (``layout``, ``mode``, ``seq_len``, ``metrics_list``).

Definition.  A frame is one (n, t, c) image x[h, w], fp32, H x W (sides 2^a or 3 * 2^a, 8 .. 512), optionally times the periodic Hann
window (1/2 - 1/2 cos(2 pi h / H)) (1/2 - 1/2 cos(2 pi w / W)).  F[ky, kx] = sum x[h, w] exp(-2 pi i (ky h / H + kx w / W)); signed
frequencies ky' = ky if ky < H / 2 else ky - H, kx' alike.  With L = max(H, W) the radius of a cell is
rho = L sqrt((ky' / H)^2 + (kx' / W)^2) and its bin b = floor(rho + 1/2); bins 0 .. L / 2 are kept (nb = L / 2 + 1), the corners
beyond are dropped.  Ties exist (rho = 1.5 exactly), so the bin comes from integers, never from a floating-point square root: b is the
largest integer with (2 b - 1)^2 H^2 W^2 <= 4 L^2 (ky'^2 W^2 + kx'^2 H^2) (``spectrum_bins``).  For square frames and b < L / 2 this
is the binning of pysteps' ``rapsd``.

Per pair (pred p, target t of one (n, t, c)), with P, T their transforms and s = 1 / (H W), every cell of bin b adds
s |P|^2 to S_p[b], s |T|^2 to S_t[b] and s Re(P conj T) to S_x[b].  State: fp64 ``sums`` [3, T', nb], int64 ``frames`` [T'] (pairs
added), accumulated until ``reset()``; static int64 ``cells`` [nb].  No NaN masking: a NaN pixel makes its lead time's bins NaN.

    psd_pred = S_p / (frames cells)      psd_target = S_t / (frames cells)      coherence = S_x / sqrt(S_p S_t)
    lsd = sqrt(mean over b = 1 .. nb - 1 of (10 log10(psd_pred / psd_target))^2)          (log-spectral distance, dB)

``wavenumber`` = b / L (cycles per pixel) and ``wavelength_px`` = L / b (inf at 0) are known after the first update.  Mode "0" pools
all lead times, "1" returns (T, nb) arrays and lsd (T,), "2" the mean of the per-lead-time results.

``update(pred, target)``: equal shapes in ``layout``, any dtype (read as ``.float()``), in place through their strides: one call of
pd_spectrum_update (prediff_amd/csrc/spectrum.hip: a batched 2-D FFT with a fused radial reduction; fp64 sums in a fixed order, the
same inputs give the same bits).  ``update_members(ens, target)``: ens is (M,) + target.shape, every member is paired with the target.
``sync(group)`` all-reduces ``sums`` and ``frames`` with SUM and is called on every rank of the group, also on ranks that made no
update.  The class is the instrument: spectra of a trained checkpoint's forecasts are not measured here.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .score_base import SEVIRScoreBase

METRICS = ("psd_pred", "psd_target", "coherence", "lsd")
WINDOWS = ("none", "hann")
# the workspace one update may hold (complex frames of the strip form + per-pair partials); more pairs than fit run in several chunks
WS_CAP_BYTES = 256 << 20


def spectrum_bins(H: int, W: int):
    """The radial bins of an H x W frame (even sides) by the integer rule: (bin_of_cell int64 [H, W] -- dropped corners hold their bin
    > L / 2 --, cell_order int32 (the kept cells ky W + kx, grouped by bin, ascending within a bin), bin_start int32 [nb + 1],
    cells int64 [nb])."""
    H, W = int(H), int(W)
    if H < 2 or W < 2 or H % 2 or W % 2 or max(H, W) > 512:
        raise ValueError(f"spectrum_bins: sides {H} x {W} must be even, 2 .. 512 (int64 suffices up to there)")
    Lm = max(H, W)
    ky = np.arange(H, dtype=np.int64)
    kx = np.arange(W, dtype=np.int64)
    ky = np.where(ky < H // 2, ky, ky - H)[:, None]
    kx = np.where(kx < W // 2, kx, kx - W)[None, :]
    # (2 b - 1)^2 <= q / (H W)^2 <=> 2 b - 1 <= m = isqrt(floor(q / (H W)^2)): the left side is an integer
    q = 4 * Lm * Lm * (ky * ky * W * W + kx * kx * H * H)
    f = q // (H * H * W * W)
    m = np.floor(np.sqrt(f.astype(np.float64))).astype(np.int64)
    m = np.where(m * m > f, m - 1, m)
    m = np.where((m + 1) * (m + 1) <= f, m + 1, m)
    bins = (m + 1) // 2
    nb = Lm // 2 + 1
    flat = bins.reshape(-1)
    order = np.argsort(flat, kind="stable")
    order = order[flat[order] < nb]
    cells = np.bincount(flat[order], minlength=nb).astype(np.int64)
    bin_start = np.concatenate([[0], np.cumsum(cells)]).astype(np.int32)
    return bins, order.astype(np.int32), bin_start, cells


class SEVIRSpectralScore(SEVIRScoreBase):
    METRICS = METRICS
    LAYOUT_NEEDS_HW = "the transform runs over H and W"
    STATE = (("sums", torch.float64, lambda self, Tk: (3, Tk, max(self.hw) // 2 + 1)),       # S_p, S_t, S_x
             ("frames", torch.int64, lambda self, Tk: (Tk,)))                               # pairs added

    def __init__(self, layout: str = "NTHWC", mode: str = "0", seq_len: Optional[int] = None,
                 metrics_list: Sequence[str] = METRICS, window: str = "none"):
        if window not in WINDOWS:
            raise ValueError(f"unknown window {window!r}; supported: {WINDOWS}")
        self.window = window
        self._bins = {}              # (H, W, device) -> (cell_order, bin_start) int32 on the device
        super().__init__(layout, mode, seq_len, metrics_list)

    def reset(self):
        super().reset()
        self.cells = None            # int64 [nb] (host): cells per bin
        self.hw = None               # (H, W) of the frames of this state

    @property
    def wavenumber(self):
        Lm = max(self.hw)
        return np.arange(Lm // 2 + 1, dtype=np.float64) / Lm

    @property
    def wavelength_px(self):
        with np.errstate(divide="ignore"):
            return 1.0 / self.wavenumber

    def _alloc_state(self, dev):
        """The number of bins comes from the frame sides: a rank that syncs before its first update sets `hw = (H, W)` first."""
        if self.hw is None:
            raise ValueError("sync() before any update: set .hw = (H, W) so that the zero state has the group's number of bins")
        super()._alloc_state(dev)
        if self.cells is None:
            self.cells = spectrum_bins(*self.hw)[3]

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        if pred.dim() != len(self.layout) or pred.shape != target.shape:
            raise ValueError(f"pred and target must have one shape in layout {self.layout!r}; got {tuple(pred.shape)} and "
                             f"{tuple(target.shape)}")
        self._launch(pred.unsqueeze(0), target)

    def update_members(self, ens: torch.Tensor, target: torch.Tensor):
        self._launch(ens, target)

    def _launch(self, ens, target):
        x, y, M, sizes, xs, ys = self._members(ens, target)
        dev = ens.device
        H, W = int(sizes[2]), int(sizes[3])
        need = L.spectrum_ws_bytes(M, sizes)
        if need < 0:                             # an unsupported shape: the library refuses it before any launch and says which side
            i32, f64 = (torch.empty(1, dtype=d, device=dev) for d in (torch.int32, torch.float64))
            with L.on_device(ens):
                L.spectrum_update(x, y, M, sizes, xs, ys, i32, i32, 0, 0, False, f64, i32, f64)
            raise L.PrediffHipError(f"pd_spectrum_update: unsupported shape {tuple(sizes)}")
        if self.hw is not None and self.hw != (H, W):
            raise ValueError(f"frames of {H} x {W} after frames of {self.hw[0]} x {self.hw[1]}: reset() first, the bins differ")
        key = (H, W, dev)
        if key not in self._bins:
            _, order, start, cells = spectrum_bins(H, W)
            self._bins[key] = (torch.from_numpy(order).to(dev), torch.from_numpy(start).to(dev), cells)
        order, start, cells = self._bins[key]
        self.hw, self.cells = (H, W), cells
        self._state_on(dev)
        one = L.spectrum_ws_bytes(1, [1, 1, H, W, 1])
        want = max(one, min(need, int(WS_CAP_BYTES)))
        ws = self._workspace((want + 7) // 8, torch.float64, dev)[:want // 8]       # an earlier, larger buffer does not lift the cap
        with L.on_device(ens):
            L.spectrum_update(x, y, M, sizes, xs, ys, order, start, cells.shape[0], WINDOWS.index(self.window),
                              self.keep_seq_len_dim, self.sums, self.frames, ws)

    def compute(self):
        Tk = self.seq_len if self.keep_seq_len_dim else 1
        if self.sums is None:
            nb = 1 if self.hw is None else max(self.hw) // 2 + 1
            s, n, cells = np.zeros((3, Tk, nb)), np.zeros((Tk,), np.int64), np.ones((nb,), np.int64)
        else:
            s, n, cells = self.sums.cpu().numpy(), self.frames.cpu().numpy(), self.cells
        den = n.astype(np.float64)[:, None] * cells.astype(np.float64)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            psd_p, psd_t = s[0] / den, s[1] / den
            coh = s[2] / np.sqrt(s[0] * s[1])
            db = 10.0 * np.log10(psd_p[:, 1:] / psd_t[:, 1:])
            lsd = np.sqrt(np.mean(db * db, axis=1)) if db.shape[1] else np.full((Tk,), np.nan)
        per = {"psd_pred": psd_p, "psd_target": psd_t, "coherence": coh, "lsd": lsd}
        return {met: self._finish(per[met]) for met in self.metrics_list}
