"""fp64 restatement of prediff_amd.spectrum's definition with numpy.fft.fft2 (not used by the product).

Bins: a brute-force double loop over Python integers -- b is the largest integer with (2 b - 1)^2 H^2 W^2 <= 4 L^2 (ky'^2 W^2 + kx'^2 H^2)
(b = 0 always holds).  State: sums (3, T', nb) fp64, frames (T',) int64, as the class keeps them."""
import functools
import math

import numpy as np


@functools.lru_cache(maxsize=None)
def bins_bruteforce(H, W):
    """bin of every cell, (H, W) int64, in Python integers (corners keep their bin > L / 2): a double loop over the cells; each cell's b
    is proposed by math.isqrt and then held against the definition itself -- (2 b - 1)^2 H^2 W^2 <= q (not tested for b = 0) and
    (2 (b + 1) - 1)^2 H^2 W^2 > q."""
    L = max(H, W)
    out = np.zeros((H, W), np.int64)
    hw2 = H * H * W * W
    for ky in range(H):
        sy = ky if ky < H // 2 else ky - H
        for kx in range(W):
            sx = kx if kx < W // 2 else kx - W
            q = 4 * L * L * (sy * sy * W * W + sx * sx * H * H)
            b = (math.isqrt(q // hw2) + 1) // 2
            assert (b == 0 or (2 * b - 1) ** 2 * hw2 <= q) and (2 * b + 1) ** 2 * hw2 > q
            out[ky, kx] = b
    out.setflags(write=False)
    return out


def hann2d(H, W):
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(H) / H)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)
    return h[:, None] * w[None, :]


def canon(x, layout):
    """numpy x in `layout` -> (N, T, C, H, W)."""
    for a in "NTHWC":
        if a not in layout:
            x, layout = x[..., None], layout + a
    return np.transpose(x, [layout.index(a) for a in "NTCHW"])


def pair_sums(p, t, bins, nb, window="none"):
    """p, t: (..., H, W) float arrays -> (3, ..., nb) fp64: S_p, S_t, S_x of every leading index."""
    H, W = p.shape[-2:]
    p, t = p.astype(np.float64), t.astype(np.float64)
    if window == "hann":
        p, t = p * hann2d(H, W), t * hann2d(H, W)
    P, T = np.fft.fft2(p), np.fft.fft2(t)
    s = 1.0 / (H * W)
    q = np.stack([s * np.abs(P) ** 2, s * np.abs(T) ** 2, s * (P * np.conj(T)).real])         # (3, ..., H, W)
    idx = np.flatnonzero(bins.reshape(-1) < nb)
    bi = bins.reshape(-1)[idx]
    rows = q.reshape(-1, H * W)
    out = np.stack([np.bincount(bi, weights=r[idx], minlength=nb) for r in rows])
    return out.reshape(q.shape[:-2] + (nb,))


def restate(updates, layout, keep_seq, window="none"):
    """The state after `updates` ((pred, target) numpy arrays in `layout`; pred may carry a leading member axis): sums (3, T', nb) fp64,
    frames (T',) int64."""
    sums = frames = None
    for p, t in updates:
        t = canon(np.asarray(t, np.float32), layout)
        p = np.asarray(p, np.float32)
        p = np.stack([canon(m, layout) for m in p]) if p.ndim == len(layout) + 1 else canon(p, layout)[None]
        M, N, T, C, H, W = p.shape
        nb = max(H, W) // 2 + 1
        s = pair_sums(p, np.broadcast_to(t, p.shape), bins_bruteforce(H, W), nb, window)       # (3, M, N, T, C, nb)
        s = s.sum(axis=(1, 2, 4))                                                             # (3, T, nb)
        n = np.full((T,), M * N * C, np.int64)
        if not keep_seq:
            s, n = s.sum(axis=1, keepdims=True), n.sum(keepdims=True)
        sums, frames = (s, n) if sums is None else (sums + s, frames + n)
    return sums, frames


def compute(sums, frames, cells):
    """psd_pred, psd_target, coherence (T', nb) and lsd (T',) of a state."""
    den = frames.astype(np.float64)[:, None] * cells.astype(np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        pp, pt = sums[0] / den, sums[1] / den
        coh = sums[2] / np.sqrt(sums[0] * sums[1])
        db = 10.0 * np.log10(pp[:, 1:] / pt[:, 1:])
        lsd = np.sqrt(np.mean(db * db, axis=1))
    return pp, pt, coh, lsd
