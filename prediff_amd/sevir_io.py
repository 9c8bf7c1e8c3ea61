"""The SEVIR pixel front end: raw VIL events in, model frames out, and back ("SEVIR pixel front end").

Public SEVIR VIL is uint8, layout NHWT, (N, 384, 384, 49), one frame per 5 minutes.  The reference turns it into model input in two
places: offline, ``save_downsampled_dataset`` (datasets/sevir/sevir_dataloader.py:460-467: every ft-th frame, then the maximum of each
fh x fw block of bytes) writes SEVIR-LR; at load time ``preprocess_data_dict`` (:645) computes scale * (x.float() + offset) and
changes the layout to NTHWC.  Its metrics want the 0..255 VIL scale back: ``process_data_dict_back`` (:679), x / scale - offset.
``SEVIRFrontEnd`` is that chain on the device, bit for bit: ``ingest`` is ONE launch (pd_sevir_ingest, csrc/sevir_io.hip) from the raw
bytes to the (context, target) sequences of any number of windows per event, ``export`` ONE launch (pd_sevir_export) from frames to the
VIL scale as fp32 or as rounded bytes.  Reading HDF5 stays outside the package; there is no CPU or torch path here.
"""
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L
from ._args import as_int as _int

# (scale, offset) of preprocess_data_dict per rescale mode and data type (the reference's PREPROCESS_SCALE_* / PREPROCESS_OFFSET_*
# tables, sevir_dataloader.py:25-44): Python floats, rounded to fp32 once where they meet the fp32 tensor
RESCALE = {
    "01": {"vil": (1 / 255, 0)},
    "sevir": {"vil": (1 / 47.54, -33.44)},
}
DATA_TYPES = ("vis", "ir069", "ir107", "vil", "lght")
EXPORT_MODE = {(torch.float32, "NTHWC"): 0, (torch.uint8, "NTHW"): 1, (torch.uint8, "NHWT"): 2}      # enum pd_sevir_export_mode

_start_tables = {}       # (starts, device) -> the device copy


def _start_table(starts: Tuple[int, ...], device):
    """The device copy of a table of window starts, uploaded once per (table, device) and kept: later calls, a graph capture's among
    them, only look it up."""
    key = (starts, str(device))
    dev = _start_tables.get(key)
    if dev is None:
        dev = _start_tables[key] = torch.tensor(starts, dtype=torch.int32).to(device)
    return dev


class SEVIRFrontEnd:
    """SEVIRFrontEnd(in_len=7, out_len=6, factors=(2, 3, 3), rescale="01", data_type="vil", pool="max")

    factors = (ft, fh, fw): the temporal stride and the spatial block of ``save_downsampled_dataset`` ((2, 3, 3) is the SEVIR-LR recipe,
    (1, 1, 1) the full-resolution configuration's).  rescale: "01" (x / 255 scale) or "sevir", as ``preprocess_data_dict``.  Only "vil"
    and the block maximum are implemented (the reference's run-time ``downsample_dict`` average pool is not part of the recipe)."""

    def __init__(self, in_len: int = 7, out_len: int = 6, factors: Sequence[int] = (2, 3, 3), rescale: str = "01", data_type: str = "vil",
                 pool: str = "max"):
        self.in_len, self.out_len = _int("in_len", in_len), _int("out_len", out_len)
        if self.in_len < 1 or self.out_len < 0:
            raise ValueError(f"in_len must be >= 1 and out_len >= 0, got {in_len} and {out_len}")
        if len(factors) != 3:
            raise ValueError(f"factors must be (ft, fh, fw), got {factors!r}")
        self.factors = tuple(_int("factors", f) for f in factors)
        if min(self.factors) < 1:
            raise ValueError(f"factors must be >= 1, got {factors!r}")
        if rescale not in RESCALE:
            raise ValueError(f"Invalid rescale option: {rescale!r} (one of {sorted(RESCALE)})")
        if data_type not in DATA_TYPES:
            raise ValueError(f"data_type must be one of {DATA_TYPES}, got {data_type!r}")
        if data_type not in RESCALE[rescale]:
            raise NotImplementedError(f"data type {data_type!r} is not implemented (only 'vil')")
        if pool in ("mean", "avg"):
            raise NotImplementedError("a mean pool is not implemented: the SEVIR-LR recipe takes the block maximum")
        if pool != "max":
            raise ValueError(f"pool must be 'max', got {pool!r}")
        self.rescale, self.data_type, self.pool = rescale, data_type, pool
        self.scale, self.offset = (float(v) for v in RESCALE[rescale][data_type])

    # ---------------------------------------------------------------------------------------- host arithmetic
    def lr_shape(self, raw_shape) -> Tuple[int, int, int, int]:
        """(N, T_lr, H / fh, W / fw) of raw events (N, H, W, T): T_lr = ceil(T / ft) frames 0, ft, 2 ft, ..."""
        if len(raw_shape) != 4:
            raise ValueError(f"raw events are (N, H, W, T), got shape {tuple(raw_shape)}")
        N, H, W, T = (int(s) for s in raw_shape)
        ft, fh, fw = self.factors
        if min(N, H, W, T) < 1:
            raise ValueError(f"raw events {tuple(raw_shape)} are empty")
        if H % fh or W % fw:
            raise ValueError(f"raw frames of {H} x {W} are not divisible by the factors {fh} x {fw}")
        return N, math.ceil(T / ft), H // fh, W // fw

    def check_windows(self, raw_shape, starts) -> Tuple[int, ...]:
        """The window starts (LR frame indices) as a tuple of ints, each window [start, start + in_len + out_len) inside the event."""
        T_lr = self.lr_shape(raw_shape)[1]
        if isinstance(starts, torch.Tensor) or not isinstance(starts, Sequence) or len(starts) < 1:
            raise ValueError(f"starts must be a non-empty sequence of LR frame indices, got {starts!r}")
        starts = tuple(_int("starts", s) for s in starts)
        span = self.in_len + self.out_len
        for s in starts:
            if s < 0 or s + span > T_lr:
                raise ValueError(f"window [{s}, {s} + {self.in_len} + {self.out_len}) runs past the {T_lr} LR frames of the event "
                                 f"(T = {raw_shape[3]}, ft = {self.factors[0]}): the last valid start is {T_lr - span}")
        return starts

    # ---------------------------------------------------------------------------------------- device
    @torch.no_grad()
    def ingest(self, raw: torch.Tensor, starts: Sequence[int] = (0,)) -> Tuple[torch.Tensor, torch.Tensor]:
        """raw (N, H, W, T) uint8 on the device -> (ctx, tgt): fp32 (N * len(starts), in_len, H / fh, W / fw, 1) and (..., out_len, ...),
        sequence n * len(starts) + k = window k of event n, frames [starts[k], starts[k] + in_len) and the out_len after them.  With
        out_len = 0 the target has no elements.  The first call with a new `starts` uploads the table (not capturable); later calls,
        and ``export``, are a launch each."""
        if not isinstance(raw, torch.Tensor) or raw.dtype != torch.uint8:
            raise ValueError(f"raw events must be a uint8 tensor, got {getattr(raw, 'dtype', type(raw).__name__)}")
        N, T_lr, Hl, Wl = self.lr_shape(raw.shape)
        starts = self.check_windows(raw.shape, starts)
        if not raw.is_contiguous():
            raise ValueError("raw events must be contiguous in the NHWT layout")
        if not raw.is_cuda:
            raise ValueError("raw events must be on a CUDA(HIP) device: there is no CPU path")
        _, H, W, T = raw.shape
        nwin = len(starts)
        with L.on_device(raw):
            table = _start_table(starts, raw.device)
            ctx = torch.empty((N * nwin, self.in_len, Hl, Wl, 1), dtype=torch.float32, device=raw.device)
            tgt = torch.empty((N * nwin, self.out_len, Hl, Wl, 1), dtype=torch.float32, device=raw.device)
            L.sevir_ingest(raw, table, ctx, tgt if self.out_len else None, N, H, W, T, self.factors, nwin, self.in_len, self.out_len,
                           self.scale, self.offset)
        return ctx, tgt

    @torch.no_grad()
    def export(self, frames: torch.Tensor, dtype=torch.uint8, layout: Optional[str] = None) -> torch.Tensor:
        """frames (B, T, H, W, 1) fp32 on the device -> the VIL scale, frames / scale - offset.  dtype=torch.float32: fp32 NTHWC.
        dtype=torch.uint8: clamped to [0, 255], rounded half to even, (B, T, H, W) with layout="NTHW" (the default) or (B, H, W, T)
        with layout="NHWT" (the raw layout)."""
        if layout is None:
            layout = "NTHWC" if dtype == torch.float32 else "NTHW"
        if (dtype, layout) not in EXPORT_MODE:
            raise ValueError(f"export writes float32 NTHWC, or uint8 NTHW / NHWT; got {dtype} {layout!r}")
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32:
            raise ValueError(f"frames must be a float32 tensor, got {getattr(frames, 'dtype', type(frames).__name__)}")
        if frames.dim() != 5 or frames.shape[-1] != 1 or frames.numel() == 0:
            raise ValueError(f"frames must be (B, T, H, W, 1), got {tuple(frames.shape)}")
        if not frames.is_contiguous():
            raise ValueError("frames must be contiguous")
        if not frames.is_cuda:
            raise ValueError("frames must be on a CUDA(HIP) device: there is no CPU path")
        B, T, H, W, _ = frames.shape
        shape = {"NTHWC": (B, T, H, W, 1), "NTHW": (B, T, H, W), "NHWT": (B, H, W, T)}[layout]
        with L.on_device(frames):
            out = torch.empty(shape, dtype=dtype, device=frames.device)
            L.sevir_export(frames, out, B, T, H, W, self.scale, self.offset, EXPORT_MODE[(dtype, layout)])
        return out
