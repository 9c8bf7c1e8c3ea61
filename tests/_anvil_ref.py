"""NumPy restatement of prediff_amd.anvil's definition (not used by the product; the step numbers are those of the module docstring of
prediff_amd/anvil.py).  `dtype=np.float64` is the reference, `dtype=np.float32` the same operations in the same order in the kernels'
precision (np.fft keeps complex64); e32 = max |fp32 - fp64| of a quantity of a case is the rounding estimate the GPU tests multiply by 8.
fp64 in both: mean(A_0^2), W0 and the product that delta is rounded from, as the definition says.

Also the test inputs: `sequence`, translating Gaussian blobs whose amplitudes grow or decay linearly, with the frames that follow the
context, and the cases of the GPU tests."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import _extrapolation_ref as X
import _steps_ref as S

EPS = 1e-3
THR = 16 / 255


def window(sigma):
    """step 6: (g (2 r + 1,) float32, r, W0 = (sum g)^2 in fp64 of the rounded weights)"""
    r = int(math.ceil(3 * sigma))
    d = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-d * d / (2.0 * float(sigma) ** 2)).astype(np.float32)
    return g, r, float(g.astype(np.float64).sum()) ** 2


def gsum(f, g):
    """G[f] over the last two axes in f's dtype: the weighted row pass, then the same pass down the columns, taps ascending; a tap
    outside the frame adds nothing (a zero, which leaves the sum as it is)"""
    H, W = f.shape[-2:]
    r = (len(g) - 1) // 2
    gw = g.astype(f.dtype)
    pad = np.zeros(f.shape[:-1] + (W + 2 * r,), f.dtype)
    pad[..., r:r + W] = f
    h = np.zeros(f.shape, f.dtype)
    for t in range(2 * r + 1):
        h = h + gw[t] * pad[..., t:t + W]
    pad = np.zeros(f.shape[:-2] + (H + 2 * r, W), f.dtype)
    pad[..., r:r + H, :] = h
    s = np.zeros(f.shape, f.dtype)
    for t in range(2 * r + 1):
        s = s + gw[t] * pad[..., t:t + H, :]
    return s


def lagrangian_frames(ctx, motion, ar_order, dtype):
    """step 2: (B, ar_order + 2, H, W), A_j at [:, j]; no floor"""
    x = np.asarray(ctx)[..., 0].astype(dtype)
    v = np.asarray(motion).astype(dtype)
    B, T, H, W = x.shape
    yy = np.arange(H, dtype=dtype)[None, :, None]
    xx = np.arange(W, dtype=dtype)[None, None, :]
    A = [x[:, T - 1]]
    for j in range(1, ar_order + 2):
        A.append(X.bil_fill(x[:, T - 1 - j], yy - dtype(j) * v[:, 0], xx - dtype(j) * v[:, 1], 0.0))
    return np.stack(A, axis=1).astype(dtype)


def analyse(ctx, motion, w, ar_order, sigma, dtype=np.float64):
    """steps 2 .. 8.  w: the (L, H, W) float32 bands the device reads.  Returns phi, gamma (B, L, 2, H, W), Y0 (B, L, H, W),
    D (B, L, ar_order + 1, H, W) and A (B, ar_order + 2, H, W)."""
    g, r, W0 = window(sigma)
    A = lagrangian_frames(ctx, motion, ar_order, dtype)
    wl = w.astype(dtype)
    F = np.fft.fft2(A)                                                             # (B, J, H, W), complex of dtype
    Y = np.fft.ifft2(wl[None, :, None] * F[:, None]).real.astype(dtype)            # (B, L, J, H, W)
    D = (Y[:, :, :-1] - Y[:, :, 1:]).astype(dtype)                                 # (B, L, p + 1, H, W)
    ms = np.maximum((A[:, 0].astype(np.float64) ** 2).mean(axis=(-2, -1)), 1e-20)  # (B,), fp64
    delta = (1e-6 * W0 * ms).astype(np.float32).astype(dtype)[:, None, None, None]
    one, eps = dtype(1), dtype(EPS)
    c00, c11, c01 = gsum(D[:, :, 0] * D[:, :, 0], g), gsum(D[:, :, 1] * D[:, :, 1], g), gsum(D[:, :, 0] * D[:, :, 1], g)
    s0 = np.sqrt(c00 + delta)
    g1 = c01 / (s0 * np.sqrt(c11 + delta))
    g1 = np.minimum(np.maximum(g1, -(one - eps)), one - eps)
    if ar_order == 2:
        c22, c02 = gsum(D[:, :, 2] * D[:, :, 2], g), gsum(D[:, :, 0] * D[:, :, 2], g)
        g2 = c02 / (s0 * np.sqrt(c22 + delta))
        g2 = np.minimum(np.maximum(g2, dtype(2) * g1 * g1 - one + eps), one - eps)
        den = one - g1 * g1
        p1, p2 = g1 * (one - g2) / den, (g2 - g1 * g1) / den
    else:
        g2, p1, p2 = np.zeros_like(g1), g1, np.zeros_like(g1)
    out = SimpleNamespace(phi=np.stack([p1, p2], axis=2), gamma=np.stack([g1, g2], axis=2), Y0=Y[:, :, 0], D=D, A=A)
    assert all(a.dtype == dtype for a in vars(out).values())
    return out


def evolve(an, K):
    """step 9: R (B, K, H, W) in the dtype of the analysis"""
    dtype = an.Y0.dtype.type
    B, L, H, W = an.Y0.shape
    Y, d1, d2 = an.Y0.copy(), an.D[:, :, 0], an.D[:, :, 1]
    p1, p2 = an.phi[:, :, 0], an.phi[:, :, 1]
    R = np.zeros((B, K, H, W), dtype)
    for k in range(K):
        d = p1 * d1 + p2 * d2
        d2, d1 = d1, d
        Y = Y + d
        acc = np.zeros((B, H, W), dtype)
        for l in range(L):
            acc = acc + Y[:, l]
        R[:, k] = acc
    return R


def finish(R, motion, thr=THR, dtype=np.float64):
    """step 10 on the given R (B, K, H, W) in `dtype`: out (B, K, H, W, 1)"""
    R = np.asarray(R).astype(dtype)
    Q = np.where(R > dtype(np.float32(thr)), R, dtype(0))
    return np.stack([X.advect(Q[:, k], motion, k + 1, 0.0, dtype)[:, k] for k in range(R.shape[1])], axis=1)


def forecast(ctx, motion, w, ar_order, sigma, K, thr=THR, dtype=np.float64):
    return finish(evolve(analyse(ctx, motion, w, ar_order, sigma, dtype), K), motion, thr)


# ------------------------------------------------------------------------------------------------ inputs
VEL = ((0.75, -0.5), (-0.5, 0.625))
RATE = 0.08


def sequence(H, W, B, T, K, seed, nblob=3, sigma=(7.0, 9.0), wobble=0.3):
    """(ctx (B, T, H, W, 1), tgt (B, K, H, W, 1), motion (B, 2, H, W)) fp32: per sequence `nblob` Gaussian blobs on a zero background
    (sigma drawn from `sigma` times min(H, W) / 64) that translate by VEL[b] pixels per frame, evaluated in fp64 at the exact sub-pixel
    centres; blob n has the amplitude a_n (1 + RATE s_n t) at frame t with s_n = +1, -1, +1, ...: alternate blobs grow and decay.
    Every centre stays 3 sigma inside the frame over all T + K frames.  The motion handed to the forecast is VEL[b] plus a smooth
    wobble of `wobble` pixels, as in _steps_ref.context."""
    rng = np.random.default_rng(9000 + seed)
    scale = min(1.0, min(H, W) / 64.0)
    vel = scale * np.array(VEL)[:B]
    n = T + K
    yy, xx = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    out = np.zeros((B, n, H, W))
    for b in range(B):
        for k in range(nblob):
            s = rng.uniform(*sigma) * min(H, W) / 64.0
            amp = rng.uniform(0.5, 1.0)
            sign = 1.0 if k % 2 == 0 else -1.0
            c0 = []
            for size, vv in ((H, vel[b, 0]), (W, vel[b, 1])):
                lo, hi = 3 * s - min(0.0, vv * (n - 1)), size - 1 - 3 * s - max(0.0, vv * (n - 1))
                if lo > hi:
                    raise ValueError(f"a blob of sigma {s:.2f} moving {vv} px / frame for {n} frames does not fit {size} pixels")
                c0.append(rng.uniform(lo, hi))
            for t in range(n):
                cy, cx = c0[0] + vel[b, 0] * t, c0[1] + vel[b, 1] * t
                out[b, t] += amp * (1.0 + RATE * sign * t) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    seq = out.astype(np.float32)[..., None]
    fy, fx = np.arange(H)[:, None] / H, np.arange(W)[None, :] / W
    wob = wobble * scale * np.stack([np.sin(2 * np.pi * (fy + fx)), np.cos(2 * np.pi * (fy - 2 * fx))])
    motion = np.ascontiguousarray((vel[:, :, None, None] + wob[None]).astype(np.float32))
    ctx, tgt = np.ascontiguousarray(seq[:, :T]), np.ascontiguousarray(seq[:, T:])
    for a in (ctx, tgt, motion):
        a.setflags(write=False)
    return ctx, tgt, motion


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# T = ar + 2, the fewest frames, except on 32 x 64, which has more than it needs
CASES = {
    "16x16-ar1": dict(H=16, W=16, L=3, window=2.0, ar=1, B=2, T=3, K=3, seed=1),
    "16x16-ar2": dict(H=16, W=16, L=3, window=2.0, ar=2, B=2, T=4, K=3, seed=1),
    "12x12-ar2": dict(H=12, W=12, L=2, window=2.0, ar=2, B=2, T=4, K=3, seed=1),   # a side that is no multiple of 8, two levels
    "24x16-ar2": dict(H=24, W=16, L=3, window=2.0, ar=2, B=2, T=4, K=3, seed=1),
    "32x64-ar2": dict(H=32, W=64, L=4, window=3.0, ar=2, B=2, T=6, K=3, seed=1),
    "128x128-ar2": dict(H=128, W=128, L=6, window=16.0, ar=2, B=1, T=4, K=2, seed=1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """everything the tests need of a case, computed once: inputs (read-only), the fp64 results and e32 per quantity"""
    c = CASES[name]
    ctx, tgt, motion = sequence(c["H"], c["W"], c["B"], c["T"], c["K"], c["seed"])
    w = S.bands(c["H"], c["W"], c["L"]).astype(np.float32)
    g, r, W0 = window(c["window"])
    for a in (w, g):
        a.setflags(write=False)
    out = SimpleNamespace(ctx=ctx, tgt=tgt, motion=motion, w=w, g=g, r=r, W0=W0, thr=THR, e32={}, **c)
    res = {}
    for dt in (np.float64, np.float32):
        an = analyse(ctx, motion, w, c["ar"], c["window"], dt)
        res[dt] = dict(gamma=an.gamma, phi=an.phi, R=evolve(an, c["K"]))
        assert all(v.dtype == dt for v in res[dt].values())
        if dt is np.float64:
            out.an = an
    for k, v in res[np.float64].items():
        v.setflags(write=False)
        setattr(out, k, v)
        out.e32[k] = float(np.abs(res[np.float32][k].astype(np.float64) - v).max())
    out.forecast = finish(out.R, motion, THR)                                       # (B, K, H, W, 1), fp64
    out.forecast32 = finish(res[np.float32]["R"], motion, THR, np.float32)          # the whole forecast restated in fp32
    out.persistence = X.advect(ctx[:, -1], motion, c["K"])                          # Lagrangian persistence with the same motion
    return out
