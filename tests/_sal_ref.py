"""CPU restatement of prediff_amd.object_score (storm objects and SAL, Wernli et al. 2008) on numpy and scipy.ndimage.label: the
yardstick of tests/test_object_score.py.  All arithmetic is fp64 except the threshold, which is the fp32 value the device uses:
float32(threshold), or the ONE fp32 product float32(thr_factor) * max(frame)."""
import numpy as np
from scipy import ndimage

STRUCTURE = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]), 8: np.ones((3, 3), int)}


def frame_threshold(frame, threshold=None, thr_factor=1.0 / 15.0):
    frame = np.asarray(frame, np.float32)
    if threshold is not None:
        return np.float32(threshold)
    with np.errstate(invalid="ignore"):
        return np.float32(thr_factor) * np.max(frame)         # NaN when the frame holds one: no object pixel then


def object_mask(frame, threshold=None, thr_factor=1.0 / 15.0):
    frame = np.asarray(frame, np.float32)
    with np.errstate(invalid="ignore"):
        return (frame >= frame_threshold(frame, threshold, thr_factor)) & (frame > 0)


def canonical_labels(frame, threshold=None, thr_factor=1.0 / 15.0, connectivity=8, min_pixels=1):
    """(labels int32 (H, W), n): background 0, the components with at least min_pixels pixels numbered 1 .. n in raster order of their
    first pixel -- scipy's labels brought to that form."""
    raw, n = ndimage.label(object_mask(frame, threshold, thr_factor), structure=STRUCTURE[connectivity])
    flat = raw.ravel()
    area = np.bincount(flat, minlength=n + 1)
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    keep = [k for k in range(1, n + 1) if area[k] >= min_pixels]
    keep.sort(key=lambda k: first[k])
    lut = np.zeros(n + 1, np.int32)
    for new, k in enumerate(keep):
        lut[k] = new + 1
    return lut[raw].astype(np.int32), len(keep)


def object_table(frame, **kw):
    """(labels, table (n, 6) fp64): mass, peak, area, row centroid, col centroid, first-pixel index of every object."""
    labels, n = canonical_labels(frame, **kw)
    v = np.asarray(frame, np.float32).astype(np.float64)
    H, W = v.shape
    rows, cols = np.mgrid[0:H, 0:W]
    flat = labels.ravel()
    table = np.zeros((n, 6))
    if n:
        v0 = np.where(labels > 0, v, 0.0)                      # background values (a NaN among them) stay out of the sums
        R = np.bincount(flat, weights=v0.ravel(), minlength=n + 1)[1:]
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        table[:, 0] = R
        table[:, 1] = ndimage.maximum(v0, labels, index=np.arange(1, n + 1))
        table[:, 2] = np.bincount(flat, minlength=n + 1)[1:]
        table[:, 3] = np.bincount(flat, weights=(v0 * rows).ravel(), minlength=n + 1)[1:] / R
        table[:, 4] = np.bincount(flat, weights=(v0 * cols).ravel(), minlength=n + 1)[1:] / R
        table[:, 5] = first[1:]
    return labels, table


def frame_record(frame, **kw):
    """What SAL needs of one frame: D, the mass centre x (None when sum v = 0), V and r (None without objects), the object count, and
    whether the frame is finite."""
    f32 = np.asarray(frame, np.float32)
    if not np.isfinite(f32).all():
        return {"finite": False}
    v = f32.astype(np.float64)
    H, W = v.shape
    rows, cols = np.mgrid[0:H, 0:W]
    sv = v.sum()
    x = None if sv == 0 else np.array([(v * rows).sum() / sv, (v * cols).sum() / sv])
    _, table = object_table(f32, **kw)
    n = table.shape[0]
    V = r = None
    if n:
        R, P = table[:, 0], table[:, 1]
        V = (R * (R / P)).sum() / R.sum()
        if x is not None:
            r = (R * np.hypot(table[:, 3] - x[0], table[:, 4] - x[1])).sum() / R.sum()
    return {"finite": True, "D": sv / (H * W), "x": x, "V": V, "r": r, "n": n, "d": float(np.hypot(H - 1, W - 1))}


def sal_pair(pred, target, **kw):
    """{"skipped": bool, "S", "A", "L1", "L2", "L" (None where undefined), "n_pred", "n_target"} of one (forecast, observation) pair."""
    F, O = frame_record(pred, **kw), frame_record(target, **kw)
    if not (F["finite"] and O["finite"]):
        return {"skipped": True}
    out = {"skipped": False, "S": None, "A": None, "L1": None, "L2": None, "L": None, "n_pred": F["n"], "n_target": O["n"]}
    d = F["d"]
    if F["D"] + O["D"] != 0:
        out["A"] = (F["D"] - O["D"]) / (0.5 * (F["D"] + O["D"]))
    if F["V"] is not None and O["V"] is not None:
        out["S"] = (F["V"] - O["V"]) / (0.5 * (F["V"] + O["V"]))
    if F["x"] is not None and O["x"] is not None and d > 0:
        out["L1"] = float(np.hypot(*(F["x"] - O["x"]))) / d
        if F["r"] is not None and O["r"] is not None:
            out["L2"] = 2.0 * abs(F["r"] - O["r"]) / d
            out["L"] = out["L1"] + out["L2"]
    return out


SUMS = ("S", "A", "L1", "L2", "L", "abs_S", "abs_A")
COUNTS = ("pairs", "skipped", "n_S", "n_A", "n_L1", "n_L", "obj_pred", "obj_target")


def sal_state(updates, keep_seq, **kw):
    """The state after `updates`, each (pred (N, T, H, W), target (N, T, H, W)): sums fp64 (7, T') and counts int64 (8, T')."""
    T = updates[0][1].shape[1]
    Tk = T if keep_seq else 1
    sums, counts = np.zeros((7, Tk)), np.zeros((8, Tk), np.int64)
    for pred, target in updates:
        for n in range(target.shape[0]):
            for t in range(T):
                tk = t if keep_seq else 0
                p = sal_pair(pred[n, t], target[n, t], **kw)
                if p["skipped"]:
                    counts[1, tk] += 1
                    continue
                counts[0, tk] += 1
                counts[6, tk] += p["n_pred"]
                counts[7, tk] += p["n_target"]
                if p["S"] is not None:
                    sums[0, tk] += p["S"]; sums[5, tk] += abs(p["S"]); counts[2, tk] += 1
                if p["A"] is not None:
                    sums[1, tk] += p["A"]; sums[6, tk] += abs(p["A"]); counts[3, tk] += 1
                if p["L1"] is not None:
                    sums[2, tk] += p["L1"]; counts[4, tk] += 1
                if p["L"] is not None:
                    sums[3, tk] += p["L2"]; sums[4, tk] += p["L"]; counts[5, tk] += 1
    return sums, counts
