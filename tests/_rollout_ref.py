"""CPU restatement (numpy, float32: plain cat / slice / scale) of the rolling-forecast rule of DESIGN.md §7, written from the formulas and
independent of prediff_amd.rollout:

    segments: n = 1 if horizon <= out_len else ceil((horizon - out_len) / s) + 1; segment j forecasts the frames [j s, j s + out_len)
    result frame f = frame f - j s of segment j = min(f // s, n - 1)
    cat_j = [ctx_j ; z_scale * z_j] along T (in_len + out_len frames);  ctx_{j+1} = cat_j[s : s + in_len]
    windowed: ctx is (B, nwin, T_in, h, w, C) and window k of z is z[:, :, y_k : y_k + h, x_k : x_k + w]; the plain module is one window
    at (0, 0) of the canvas's own size
"""
import numpy as np


def n_segments(out_len, horizon, s):
    return 1 if horizon <= out_len else -(-(horizon - out_len) // s) + 1


def windows(z, window, origins):
    """(B, T, Hc, Wc, C) -> (B, nwin, T, h, w, C) by index slices"""
    return np.stack([z[:, :, y:y + window[0], x:x + window[1], :] for y, x in origins], axis=1)


def advance(ctx, z, z_scale, s, origins=((0, 0),)):
    """ctx (B, nwin, T_in, h, w, C), z (B, T_out, Hc, Wc, C), both float32 -> the next context, float32; one fp32 multiply per fed-back value"""
    ctx, z = np.asarray(ctx, dtype=np.float32), np.asarray(z, dtype=np.float32)
    zw = windows(z, ctx.shape[3:5], origins) * np.float32(z_scale)
    assert zw.dtype == np.float32
    cat = np.concatenate([ctx, zw], axis=2)
    return np.ascontiguousarray(cat[:, :, s:s + ctx.shape[2]])


def assemble(segments, out_len, horizon, s):
    """per-segment outputs (B, out_len, ...) -> (B, horizon, ...)"""
    n = n_segments(out_len, horizon, s)
    assert len(segments) == n
    frames = []
    for f in range(horizon):
        j = min(f // s, n - 1)
        frames.append(np.asarray(segments[j])[:, f - j * s])
    return np.stack(frames, axis=1)
