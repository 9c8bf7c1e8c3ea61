"""CPU restatement (numpy / torch, fp64) of the tiled-sampling rule of DESIGN.md §7, written from the formulas and independent of
prediff_amd.tiled:

    origins per axis: sorted(set(min(k s, size - n) for k in range(ceil((size - n) / s) + 1))); windows row-major, y outer
    ramp[k] = min(1, (k + 1) / (o + 1), (n - k) / (o + 1)) with o = n - s ("feather"), 1 ("uniform");  g = ramp_y (x) ramp_x
    g^_win(cell) = g(cell) / sum of g over the windows covering the cell
    gather: z_win = z[:, :, oy : oy + h, ox : ox + w, :] as (B, nwin, T, h, w, C)
    blend: canvas(cell) = sum over the covering windows, in ascending window index, of g^_win * e_win
"""
import math

import numpy as np
import torch


def origins_1d(n, size, s):
    return sorted(set(min(k * s, size - n) for k in range(math.ceil((size - n) / s) + 1)))


def origins(window, canvas, stride):
    return [(y, x) for y in origins_1d(window[0], canvas[0], stride[0]) for x in origins_1d(window[1], canvas[1], stride[1])]


def ramp(n, s, blend):
    o = n - s
    return np.asarray([1.0 if blend == "uniform" else min(1.0, (k + 1) / (o + 1), (n - k) / (o + 1)) for k in range(n)], dtype=np.float64)


def cover(window, canvas, org):
    """number of windows covering each canvas cell"""
    n = np.zeros(canvas, dtype=np.int64)
    for y, x in org:
        n[y:y + window[0], x:x + window[1]] += 1
    return n


def weights(window, canvas, stride, blend="feather"):
    """fp64 (nwin, h, w): the normalised weights before their one rounding to fp32"""
    (h, w), org = window, origins(window, canvas, stride)
    g = ramp(h, stride[0], blend)[:, None] * ramp(w, stride[1], blend)[None, :]
    total = np.zeros(canvas, dtype=np.float64)
    for y, x in org:
        total[y:y + h, x:x + w] += g
    return np.stack([g / total[y:y + h, x:x + w] for y, x in org])


def scaled(window, canvas, stride, f):
    return tuple(f * v for v in window), tuple(f * v for v in canvas), tuple(f * v for v in stride)


def gather(z, window, org):
    """(B, T, Hc, Wc, C) -> (B, nwin, T, h, w, C), by index slices (dtype kept)"""
    return torch.stack([z[:, :, y:y + window[0], x:x + window[1], :] for y, x in org], dim=1).contiguous()


def blend(e, wts, org, canvas):
    """e (B, nwin, T, h, w, C), wts (nwin, h, w) -> fp64 (B, T, Hc, Wc, C)"""
    e = torch.as_tensor(e).double()
    wts = torch.as_tensor(np.asarray(wts, dtype=np.float64))
    B, nwin, T, h, w, C = e.shape
    out = torch.zeros((B, T) + tuple(canvas) + (C,), dtype=torch.float64)
    for k, (y, x) in enumerate(org):
        out[:, :, y:y + h, x:x + w, :] += wts[k][None, None, :, :, None] * e[:, k]
    return out


def tiled_denoiser(denoiser, window, canvas, stride, blend_mode="feather"):
    """denoiser(z, t, zc) on windows -> the same signature on the canvas: fp64 gather -> the denoiser on the fp32 rounding of every window
    (each with its own condition window, t repeated) -> fp64 blend.  zc is a latent canvas (B, T_in, Hc, Wc, C)."""
    org = origins(window, canvas, stride)
    wts = weights(window, canvas, stride, blend_mode)

    def on_canvas(z, t, zc):
        zw, cw = gather(z.double(), window, org), gather(zc.double(), window, org)
        B, nwin = zw.shape[:2]
        e = denoiser(zw.reshape((B * nwin,) + tuple(zw.shape[2:])).float(), t.reshape(B, 1).expand(B, nwin).reshape(-1),
                     cw.reshape((B * nwin,) + tuple(cw.shape[2:])).float())
        return blend(e.reshape(zw.shape), wts, org, canvas)
    return on_canvas
