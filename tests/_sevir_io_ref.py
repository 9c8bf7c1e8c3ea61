"""numpy restatement of the SEVIR pixel chain the reference runs in two places (no reference code is imported; the lines are cited).

Offline, save_downsampled_dataset (datasets/sevir/sevir_dataloader.py:460-467):
    data[..., ::ft]                                    # layout NHWT: frames 0, ft, 2 ft, ...
    block_reduce(data, (1, fh, fw, 1), np.max)         # non-overlapping blocks, on the bytes (H, W divisible: no padding enters)
At load time, preprocess_data_dict (:639-647):
    scale * (data.astype(np.float32) + offset)         # Python scalars meet a float32 array: both are rounded to fp32 once; one fp32
                                                       # add, then one fp32 multiply
    change_layout NHWT -> NTHWC
Back, process_data_dict_back (:679):
    data.float() / scale - offset                      # one fp32 divide by the fp32 scale, then one fp32 subtract
The scalars are made np.float32 explicitly so the arithmetic below is fp32 whatever numpy's promotion rules are."""
import numpy as np

# PREPROCESS_SCALE_* / PREPROCESS_OFFSET_* for 'vil' (sevir_dataloader.py:25-44)
RESCALE = {"01": (1 / 255, 0), "sevir": (1 / 47.54, -33.44)}


def pool(raw, factors):
    """uint8 (N, H, W, T) -> uint8 (N, H / fh, W / fw, ceil(T / ft)): temporal stride, then the block maximum"""
    ft, fh, fw = factors
    x = raw[..., ::ft]
    N, H, W, T = x.shape
    assert H % fh == 0 and W % fw == 0
    return x.reshape(N, H // fh, fh, W // fw, fw, T).max(axis=(2, 4))


def forward(x_u8, rescale):
    scale, offset = (np.float32(v) for v in RESCALE[rescale])
    y = x_u8.astype(np.float32) + offset
    assert y.dtype == np.float32
    y = scale * y
    assert y.dtype == np.float32
    return y


def back(x_f32, rescale):
    scale, offset = (np.float32(v) for v in RESCALE[rescale])
    assert x_f32.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        y = x_f32 / scale - offset
    assert y.dtype == np.float32
    return y


def ingest(raw, factors, rescale, in_len, out_len, starts):
    """(ctx, tgt): float32 (N * len(starts), in_len | out_len, H', W', 1), sequence n * len(starts) + k = window k of event n"""
    lr = forward(pool(raw, factors), rescale)                    # (N, H', W', T')
    lr = np.ascontiguousarray(np.transpose(lr, (0, 3, 1, 2)))[..., None]      # NTHWC
    N = lr.shape[0]
    seqs = np.stack([lr[:, s:s + in_len + out_len] for s in starts], axis=1)
    assert seqs.shape[2] == in_len + out_len, "a window runs past the event"
    seqs = seqs.reshape((N * len(starts), in_len + out_len) + lr.shape[2:])
    return np.ascontiguousarray(seqs[:, :in_len]), np.ascontiguousarray(seqs[:, in_len:])


def to_bytes(v):
    """clamp to [0, 255], round half to even (torch.round, np.rint), uint8; NaN-free input"""
    return np.rint(np.clip(v, np.float32(0), np.float32(255))).astype(np.uint8)


def export(frames, rescale, dtype="uint8", layout="NTHW"):
    """frames float32 (B, T, H, W, 1) -> float32 NTHWC on the VIL scale, or uint8 (B, T, H, W) / (B, H, W, T)"""
    v = back(frames, rescale)
    if dtype == "float32":
        return v
    b = to_bytes(v[..., 0])
    return b if layout == "NTHW" else np.ascontiguousarray(np.transpose(b, (0, 2, 3, 1)))
