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
from .sevir_skill import axes_of

MAX_MEMBERS = 512
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


class SEVIRSpectralScore:
    def __init__(self, layout: str = "NTHWC", mode: str = "0", seq_len: Optional[int] = None,
                 metrics_list: Sequence[str] = METRICS, window: str = "none"):
        if mode not in ("0", "1", "2"):
            raise NotImplementedError(f"mode {mode} not supported!")
        if "N" not in layout or "T" not in layout or len(set(layout)) != len(layout) or set(layout) - set("NTHWC"):
            raise ValueError(f"layout {layout!r}: distinct letters of N, T, H, W, C with N and T present")
        if "H" not in layout or "W" not in layout:
            raise ValueError(f"layout {layout!r}: the transform runs over H and W, both must be named")
        bad = [m for m in metrics_list if m not in METRICS]
        if bad:
            raise ValueError(f"unknown metrics {bad}; supported: {METRICS}")
        if window not in WINDOWS:
            raise ValueError(f"unknown window {window!r}; supported: {WINDOWS}")
        self.layout, self.mode, self.seq_len = layout, mode, seq_len
        self.metrics_list = tuple(metrics_list)
        self.window = window
        self.keep_seq_len_dim = mode in ("1", "2")
        if self.keep_seq_len_dim and not isinstance(seq_len, int):
            raise ValueError("seq_len must be provided when we need to keep seq_len dim.")
        self._bins = {}              # (H, W, device) -> (cell_order, bin_start) int32 on the device
        self.reset()

    def reset(self):
        self.sums = None             # fp64 [3, T', nb]: S_p, S_t, S_x
        self.frames = None           # int64 [T']: pairs added
        self.cells = None            # int64 [nb] (host): cells per bin
        self.hw = None               # (H, W) of the frames of this state
        self._ws = None

    @property
    def wavenumber(self):
        Lm = max(self.hw)
        return np.arange(Lm // 2 + 1, dtype=np.float64) / Lm

    @property
    def wavelength_px(self):
        with np.errstate(divide="ignore"):
            return 1.0 / self.wavenumber

    def _alloc_state(self, dev, nb):
        Tk = self.seq_len if self.keep_seq_len_dim else 1
        self.sums = torch.zeros((3, Tk, nb), dtype=torch.float64, device=dev)
        self.frames = torch.zeros((Tk,), dtype=torch.int64, device=dev)

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        if pred.dim() != len(self.layout) or tuple(pred.shape) != tuple(target.shape):
            raise ValueError(f"pred and target must have one shape in layout {self.layout!r}; got {tuple(pred.shape)} and "
                             f"{tuple(target.shape)}")
        self._launch(pred.unsqueeze(0), target)

    def update_members(self, ens: torch.Tensor, target: torch.Tensor):
        if ens.dim() != len(self.layout) + 1 or tuple(ens.shape[1:]) != tuple(target.shape):
            raise ValueError(f"ens must be (M,) + target.shape with target in layout {self.layout!r}; got {tuple(ens.shape)} "
                             f"and {tuple(target.shape)}")
        if not 1 <= ens.shape[0] <= MAX_MEMBERS:
            raise ValueError(f"{ens.shape[0]} members: 1 .. {MAX_MEMBERS} are supported")
        self._launch(ens, target)

    def _launch(self, ens, target):
        if not (ens.is_cuda and target.is_cuda):
            raise L.PrediffHipError("SEVIRSpectralScore.update runs on the HIP device the frames were decoded on")
        if self.keep_seq_len_dim:
            assert target.shape[self.layout.find("T")] == self.seq_len
        dev = ens.device
        x, y = ens.detach().float(), target.detach().float()          # read in place through their strides
        M = x.shape[0]
        sizes, xs = axes_of(self.layout, x, lead=1)
        _, ys = axes_of(self.layout, y)
        H, W = int(sizes[2]), int(sizes[3])
        need = L.spectrum_ws_bytes(M, sizes)
        if need < 0:                             # an unsupported shape: the library refuses it before any launch and says which side
            i32, f64 = (torch.empty(1, dtype=d, device=dev) for d in (torch.int32, torch.float64))
            with L.on_device(ens):
                L.spectrum_update(x, y, M, sizes, [x.stride(0)] + xs, ys, i32, i32, 0, 0, False, f64, i32, f64)
            raise L.PrediffHipError(f"pd_spectrum_update: unsupported shape {tuple(sizes)}")
        if self.hw is not None and self.hw != (H, W):
            raise ValueError(f"frames of {H} x {W} after frames of {self.hw[0]} x {self.hw[1]}: reset() first, the bins differ")
        key = (H, W, dev)
        if key not in self._bins:
            _, order, start, cells = spectrum_bins(H, W)
            self._bins[key] = (torch.from_numpy(order).to(dev), torch.from_numpy(start).to(dev), cells)
        order, start, cells = self._bins[key]
        nb = cells.shape[0]
        self.hw, self.cells = (H, W), cells
        if self.sums is None:
            self._alloc_state(dev, nb)
        elif self.sums.device != dev:            # a zero state that sync() made before this rank's first update
            self.sums, self.frames = self.sums.to(dev), self.frames.to(dev)
        one = L.spectrum_ws_bytes(1, [1, 1, H, W, 1])
        want = max(one, min(need, int(WS_CAP_BYTES)))
        if self._ws is None or self._ws.numel() * 8 < want or self._ws.device != dev:
            self._ws = torch.empty((want + 7) // 8, dtype=torch.float64, device=dev)
        ws = self._ws[:want // 8]                # an earlier, larger buffer does not lift the cap
        with L.on_device(ens):
            L.spectrum_update(x, y, M, sizes, [x.stride(0)] + xs, ys, order, start, nb, WINDOWS.index(self.window),
                              self.keep_seq_len_dim, self.sums, self.frames, ws)

    def sync(self, group=None):
        """All-reduce the state with SUM over the ranks of `group`; every rank must call it, including ranks that made no update
        (they take part with a zero state; its number of bins comes from the frame sides, so such a rank sets `hw = (H, W)` first)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self.sums is None:
            if self.hw is None:
                raise ValueError("sync() before any update: set .hw = (H, W) so that the zero state has the group's number of bins")
            nccl = dist.get_backend(group) == "nccl"
            self._alloc_state(torch.device("cuda", torch.cuda.current_device()) if nccl else torch.device("cpu"), max(self.hw) // 2 + 1)
            self.cells = spectrum_bins(*self.hw)[3]
        for t in (self.sums, self.frames):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def _finish(self, per_t):
        """per_t: (T', ...) -> the mode's form: [0] for "0", the array for "1", the mean over lead times for "2"."""
        if self.mode == "0":
            return per_t[0] if per_t.ndim > 1 else float(per_t[0])
        if self.mode == "1":
            return per_t
        return np.mean(per_t, axis=0) if per_t.ndim > 1 else float(np.mean(per_t))

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
