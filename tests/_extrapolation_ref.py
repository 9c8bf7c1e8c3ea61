"""NumPy restatement of prediff_amd.extrapolation's definition (not used by the product): `dtype=np.float64` is the reference,
`dtype=np.float32` the same arithmetic in the kernels' precision, whose distance from the reference is the rounding estimate the GPU
bound is made of.  Frames are (B, T, H, W, 1); motion is (B, 2, H, W) = (v_y, v_x) in pixels per frame.

Also the test inputs: `blobs`, a seeded generator of translating Gaussian blobs evaluated analytically at sub-pixel shifts, whose
centres stay 3 sigma inside the frame over the context and every lead, so that a full-frame comparison with persistence is fair."""
import functools

import numpy as np

FAR = float(2 ** 20)


def down2(x):
    """the mean of each 2 x 2 block of the last two axes: ((a + b) + (c + d)) / 4"""
    return ((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + (x[..., 1::2, 0::2] + x[..., 1::2, 1::2])) * x.dtype.type(0.25)


def gradients(I):
    """central differences with a replicate border over the last two axes: (gy, gx)"""
    H, W = I.shape[-2:]
    yp, ym = np.minimum(np.arange(H) + 1, H - 1), np.maximum(np.arange(H) - 1, 0)
    xp, xm = np.minimum(np.arange(W) + 1, W - 1), np.maximum(np.arange(W) - 1, 0)
    half = I.dtype.type(0.5)
    return (I[..., yp, :] - I[..., ym, :]) * half, (I[..., :, xp] - I[..., :, xm]) * half


def box(f, r):
    """the truncated box sum S[f] over the last two axes: along x, then along y, offsets ascending; cells outside the frame add nothing"""
    H, W = f.shape[-2:]
    pad = np.zeros(f.shape[:-1] + (W + 2 * r,), f.dtype)
    pad[..., r:r + W] = f
    h = pad[..., 0:W].copy()
    for i in range(1, 2 * r + 1):
        h += pad[..., i:i + W]
    pad = np.zeros(f.shape[:-2] + (H + 2 * r, W), f.dtype)
    pad[..., r:r + H, :] = h
    s = pad[..., 0:H, :].copy()
    for i in range(1, 2 * r + 1):
        s += pad[..., i:i + H, :]
    return s


def _lerp2(I00, I01, I10, I11, fy, fx):
    top = I00 + fx * (I01 - I00)
    bot = I10 + fx * (I11 - I10)
    return top + fy * (bot - top)


def bil_clamp(I, cy, cx):
    """I (B, H, W) at (cy, cx) (B, H, W): the coordinate clamped to the frame, bilinear from floor, the upper taps clamped too"""
    B, H, W = I.shape
    one = I.dtype.type
    cy = np.minimum(np.maximum(cy, one(0)), one(H - 1))
    cx = np.minimum(np.maximum(cx, one(0)), one(W - 1))
    y0f, x0f = np.floor(cy), np.floor(cx)
    fy, fx = cy - y0f, cx - x0f
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    b = np.arange(B)[:, None, None]
    return _lerp2(I[b, y0, x0], I[b, y0, x1], I[b, y1, x0], I[b, y1, x1], fy, fx)


def bil_fill(I, cy, cx, fill):
    """I (B, H, W) at (cy, cx): bilinear from floor, a tap outside the frame reads `fill`; a non-finite coordinate, or one further than
    2^20 from the frame, gives `fill`"""
    B, H, W = I.shape
    one = I.dtype.type
    fill = one(fill)
    with np.errstate(invalid="ignore"):
        ok = (cy >= one(-FAR)) & (cy <= one(H - 1 + FAR)) & (cx >= one(-FAR)) & (cx <= one(W - 1 + FAR))
    cy, cx = np.where(ok, cy, one(0)), np.where(ok, cx, one(0))
    y0f, x0f = np.floor(cy), np.floor(cx)
    fy, fx = cy - y0f, cx - x0f
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    b = np.arange(B)[:, None, None]

    def tap(y, x):
        inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        return np.where(inside, I[b, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], fill)

    out = _lerp2(tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), fy, fx)
    return np.where(ok, out, fill)


def motion(ctx, levels=4, iters=3, radius=7, damping=1e-2, pairs=3, dtype=np.float64):
    """ctx (B, T, H, W, 1) -> (B, 2, H, W) of `dtype`: the pyramidal, iterated, damped Lucas-Kanade motion of the definition"""
    x = np.asarray(ctx)[..., 0].astype(dtype)
    B, T, H, W = x.shape
    P = min(int(pairs), T - 1)
    lam = dtype(damping)
    pyr = [x[:, T - 1 - P:]]                          # frame f of the pyramid is ctx[:, T - 1 - P + f]
    for _ in range(1, levels):
        pyr.append(down2(pyr[-1]))
    v = None
    for lvl in range(levels - 1, -1, -1):
        F = pyr[lvl]
        Hl, Wl = F.shape[-2:]
        if v is None:
            v = np.zeros((B, 2, Hl, Wl), dtype)
        else:
            v = dtype(2) * v[:, :, np.arange(Hl) // 2][:, :, :, np.arange(Wl) // 2]
        I0 = [F[:, P - 1 - p] for p in range(P)]
        I1 = [F[:, P - p] for p in range(P)]
        g = [gradients(i) for i in I0]
        Gyy = box(sum(gy * gy for gy, gx in g), radius)
        Gyx = box(sum(gy * gx for gy, gx in g), radius)
        Gxx = box(sum(gx * gx for gy, gx in g), radius)
        yy = np.arange(Hl, dtype=dtype)[None, :, None]
        xx = np.arange(Wl, dtype=dtype)[None, None, :]
        a, c = Gyy + lam, Gxx + lam
        det = a * c - Gyx * Gyx
        for _ in range(iters):
            It = [bil_clamp(I1[p], yy + v[:, 0], xx + v[:, 1]) - I0[p] for p in range(P)]
            by = box(sum(g[p][0] * It[p] for p in range(P)), radius)
            bx = box(sum(g[p][1] * It[p] for p in range(P)), radius)
            dy = (c * by - Gyx * bx) / det
            dx = (a * bx - Gyx * by) / det
            v = np.stack([v[:, 0] - dy, v[:, 1] - dx], axis=1)
    return v


def advect(frame, mot, out_len, fill=0.0, dtype=np.float64):
    """frame (B, H, W[, 1]), mot (B, 2, H, W) -> (B, out_len, H, W, 1) of `dtype`: F_k = bil_fill(frame, y - k v_y, x - k v_x)"""
    I = np.asarray(frame)
    I = (I[..., 0] if I.ndim == 4 else I).astype(dtype)
    v = np.asarray(mot).astype(dtype)
    B, H, W = I.shape
    yy = np.arange(H, dtype=dtype)[None, :, None]
    xx = np.arange(W, dtype=dtype)[None, None, :]
    out = np.empty((B, out_len, H, W, 1), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, out_len + 1):
            out[:, k - 1, :, :, 0] = bil_fill(I, yy - dtype(k) * v[:, 0], xx - dtype(k) * v[:, 1], fill)
    return out


def forecast(ctx, out_len=6, fill=0.0, dtype=np.float64, **kw):
    return advect(np.asarray(ctx)[:, -1], motion(ctx, dtype=dtype, **kw), out_len, fill, dtype)


@functools.lru_cache(maxsize=None)
def blobs(B, T, K, H, W, vel, seed=0, nblob=3, sigma=(2.5, 3.5)):
    """(ctx (B, T, H, W, 1), tgt (B, K, H, W, 1)) fp32, read-only: per sequence `nblob` Gaussian blobs (amplitude 0.4 .. 1, sigma drawn
    from `sigma` times min(H, W) / 64) that translate by `vel` = (v_y, v_x) pixels per frame -- one pair for all sequences or one per
    sequence --, evaluated in fp64 at the exact sub-pixel centres.  Every centre stays 3 sigma inside the frame over all T + K frames."""
    rng = np.random.default_rng(7000 + seed)
    vel = np.broadcast_to(np.asarray(vel, np.float64), (B, 2))
    n = T + K
    yy = np.arange(H, dtype=np.float64)[:, None]
    xx = np.arange(W, dtype=np.float64)[None, :]
    out = np.zeros((B, n, H, W))
    for b in range(B):
        for _ in range(nblob):
            s = rng.uniform(*sigma) * min(H, W) / 64.0
            amp = rng.uniform(0.4, 1.0)
            c0 = []
            for size, vv in ((H, vel[b, 0]), (W, vel[b, 1])):
                lo = 3 * s - min(0.0, vv * (n - 1))
                hi = size - 1 - 3 * s - max(0.0, vv * (n - 1))
                if lo > hi:
                    raise ValueError(f"a blob of sigma {s:.2f} moving {vv} px / frame for {n} frames does not fit {size} pixels")
                c0.append(rng.uniform(lo, hi))
            for t in range(n):
                cy, cx = c0[0] + vel[b, 0] * t, c0[1] + vel[b, 1] * t
                out[b, t] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    seq = out.astype(np.float32)[..., None]
    ctx, tgt = np.ascontiguousarray(seq[:, :T]), np.ascontiguousarray(seq[:, T:])
    ctx.setflags(write=False), tgt.setflags(write=False)
    return ctx, tgt


# The motion cases the device is held to: name -> (blobs arguments, estimator options).  test_extrapolation_host.py proves e32 < 1e-4 px
# for each, test_extrapolation.py holds the kernels to 8 * e32.
MOTION_CASES = {
    "16x24": (dict(B=3, T=4, K=0, H=16, W=24, vel=((0.5, -0.75), (-0.5, 0.25), (0.75, 1.0)), seed=3, nblob=2, sigma=(6.0, 8.0)),
              dict(levels=2, iters=3, radius=2, damping=1e-2, pairs=3)),
    "40x72": (dict(B=2, T=3, K=0, H=40, W=72, vel=((1.5, -0.75), (-2.0, 1.0)), seed=4, sigma=(4.0, 5.0)),
              dict(levels=3, iters=3, radius=4, damping=1e-2, pairs=2)),
    "64x64": (dict(B=1, T=2, K=0, H=64, W=64, vel=(1.5, -0.75), seed=5),
              dict(levels=3, iters=3, radius=7, damping=1e-2, pairs=3)),
    "32x40-r9": (dict(B=1, T=3, K=0, H=32, W=40, vel=(1.0, -0.75), seed=7, nblob=2, sigma=(4.0, 5.0)),        # the largest radius and LDS
                 dict(levels=2, iters=2, radius=9, damping=1e-2, pairs=2)),
    "128x128": (dict(B=2, T=7, K=0, H=128, W=128, vel=((1.5, -0.75), (-3.0, 2.0)), seed=6),
                dict(levels=4, iters=3, radius=7, damping=1e-2, pairs=3)),
}


@functools.lru_cache(maxsize=None)
def motion_case(name):
    """(ctx fp32 (B, T, H, W, 1), estimator options, fp64 motion, e32 = max |fp32 motion - fp64 motion|), all read-only"""
    args, opts = MOTION_CASES[name]
    args = dict(args, vel=tuple(args["vel"]))
    ctx, _ = blobs(**args)
    m64 = motion(ctx, dtype=np.float64, **opts)
    m32 = motion(ctx, dtype=np.float32, **opts)
    assert m32.dtype == np.float32 and m64.dtype == np.float64
    m64.setflags(write=False)
    return ctx, opts, m64, float(np.abs(m32.astype(np.float64) - m64).max())


# The sequences on which the forecast is compared with Eulerian persistence (host: the restatement; device: through the scores):
# name -> (blobs arguments, levels)
SKILL_CASES = {
    "64-slow": (dict(B=4, T=7, K=6, H=64, W=64, vel=(1.5, -0.75), seed=1), 3),
    "64-fast": (dict(B=4, T=7, K=6, H=64, W=64, vel=(-3.0, 2.0), seed=8), 3),
    "128-slow": (dict(B=2, T=7, K=6, H=128, W=128, vel=(1.5, -0.75), seed=1), 4),
    "128-fast": (dict(B=2, T=7, K=6, H=128, W=128, vel=(-3.0, 2.0), seed=0), 4),
}


@functools.lru_cache(maxsize=None)
def skill_case(name):
    """(ctx, tgt, levels, fp64 motion, fp64 forecast (B, 6, H, W, 1), fp32 forecast: motion and advection restated in fp32), read-only"""
    args, levels = SKILL_CASES[name]
    ctx, tgt = blobs(**args)
    m64 = motion(ctx, levels=levels)
    f64 = advect(ctx[:, -1], m64, tgt.shape[1])
    f32 = forecast(ctx, tgt.shape[1], dtype=np.float32, levels=levels)
    assert f32.dtype == np.float32
    m64.setflags(write=False), f64.setflags(write=False), f32.setflags(write=False)
    return ctx, tgt, levels, m64, f64, f32
