"""NumPy restatement of prediff_amd.probability_matching (the module docstring there is the definition): rank_frames, match_cdf and
probability_matched_mean on float32 arrays whose last three axes are (H, W, 1).  Everything is a selection of input values, so the
device results are compared with np.array_equal, NaN frames with equal_nan.

ORDER is np.argsort(frame.ravel(), kind="stable") on FINITE frames: ascending by value, ties (-0.0 and +0.0 among them) by pixel index.
NumPy compares float32 denormals by their exact value.  A frame with a non-finite pixel is never ordered.
"""
import numpy as np

NAN = np.float32(np.nan)


def finite(frame):
    return bool(np.isfinite(frame).all())


def order_of(flat):
    """the stable ascending order of a finite 1-d float32 array"""
    assert flat.dtype == np.float32 and flat.ndim == 1
    return np.argsort(flat, kind="stable")


def plus_zero(a):
    """-0.0 read as +0.0, every other value as it is"""
    a = a.copy()
    a[a == 0] = np.float32(0.0)
    return a


def rank_frames(x):
    """x (..., H, W, 1) float32 -> (sorted float32 (..., n), order int32 (..., n))"""
    assert x.dtype == np.float32 and x.shape[-1] == 1
    n = x.shape[-3] * x.shape[-2]
    flat = x.reshape(-1, n)
    srt, order = np.full(flat.shape, NAN, np.float32), np.full(flat.shape, -1, np.int32)
    for f in range(flat.shape[0]):
        if finite(flat[f]):
            o = order_of(flat[f])
            order[f], srt[f] = o, flat[f][o]
    lead = x.shape[:-3]
    return srt.reshape(lead + (n,)), order.reshape(lead + (n,))


def match_frame(xf, rf, threshold=None):
    """one frame: xf, rf flat float32 of equal length -> flat float32"""
    n = xf.size
    if not (finite(xf) and finite(rf)):
        return np.full(n, NAN, np.float32)
    s = np.sort(plus_zero(rf))                          # ties are equal bits after plus_zero: any sort gives the same array
    if threshold is not None:
        thr = np.float32(threshold)
        n_x = int((xf > thr).sum())
        head = s[:n - n_x]
        s[:n - n_x] = np.where(head > thr, thr, head)
    out = np.empty(n, np.float32)
    out[order_of(xf)] = s
    return out


def match_cdf(x, ref, threshold=None):
    """x (B, T, H, W, 1) or (M, B, T, H, W, 1), ref (B, T, H, W, 1) or (B, 1, H, W, 1) -> like x"""
    assert x.dtype == np.float32 and ref.dtype == np.float32
    x6 = x if x.ndim == 6 else x[None]
    M, B, T, H, W, _ = x6.shape
    assert ref.shape in ((B, T, H, W, 1), (B, 1, H, W, 1))
    out = np.empty_like(x6)
    for m in range(M):
        for b in range(B):
            for t in range(T):
                rf = ref[b, t if ref.shape[1] == T else 0].ravel()
                out[m, b, t] = match_frame(x6[m, b, t].ravel(), rf, threshold).reshape(H, W, 1)
    return out.reshape(x.shape)


def pmm_parts(members):
    """members (M, n) float32, all finite -> (mean float32 (n,), q float32 (n,))"""
    M, n = members.shape
    acc = np.zeros(n, np.float64)
    for m in range(M):                                  # member order 0 .. M-1
        acc = acc + members[m].astype(np.float64)
    mean = (acc / np.float64(M)).astype(np.float32)
    P = np.sort(plus_zero(members.ravel()))
    return mean, P[np.arange(n) * M + M // 2]


def probability_matched_mean(ens):
    """ens (M, B, T, H, W, 1) float32 -> (B, T, H, W, 1)"""
    assert ens.dtype == np.float32 and ens.ndim == 6 and ens.shape[-1] == 1
    M, B, T, H, W, _ = ens.shape
    out = np.empty((B, T, H, W, 1), np.float32)
    for b in range(B):
        for t in range(T):
            members = ens[:, b, t].reshape(M, H * W)
            if not finite(members):
                out[b, t] = NAN
                continue
            mean, q = pmm_parts(members)
            o = np.empty(H * W, np.float32)
            o[order_of(mean)] = q
            out[b, t] = o.reshape(H, W, 1)
    return out
