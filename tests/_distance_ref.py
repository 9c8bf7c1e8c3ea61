"""CPU restatement of prediff_amd.distance_score (distance maps, mean error distances, Hausdorff, Baddeley's Delta; Gilleland 2011 / 2017)
on numpy: the yardstick of tests/test_distance_score.py.  The squared distance map is the brute-force minimum over the event pixels, on
integers; everything after it is fp64.  The event test is the fp32 division and comparison the device uses.  Empty sets are handled
apart (scipy's distance_transform_edt has no meaningful answer for them)."""
import numpy as np

NO_EVENT = 2 ** 31 - 1
SUMS = ("med_miss", "med_false", "hausdorff", "baddeley")
COUNTS = ("pairs", "skipped", "both", "baddeley", "events_pred", "events_target")


def event_mask(x, threshold, scaled=True):
    """float32(x) / float32(1/255) >= float32(threshold) (scaled) or float32(x) >= float32(threshold); a NaN is never an event"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x / np.float32(1.0 / 255.0) if scaled else x
        return v >= np.float32(threshold)


def d2_of_mask(mask):
    """int64 (H, W): min over the events a of (row - row_a)^2 + (col - col_a)^2; NO_EVENT everywhere for an empty mask"""
    H, W = mask.shape
    er, ec = np.nonzero(mask)
    if er.size == 0:
        return np.full((H, W), NO_EVENT, np.int64)
    dr2 = ((np.arange(H)[:, None] - er[None, :]) ** 2).astype(np.int32)          # (H, E)
    dc2 = ((np.arange(W)[:, None] - ec[None, :]) ** 2).astype(np.int32)          # (W, E)
    return np.stack([(dc2 + dr2[y][None, :]).min(axis=1) for y in range(H)]).astype(np.int64)


def distance_map(frames, threshold, scaled=True):
    """frames (..., H, W) -> int64 d2 of the same shape"""
    frames = np.asarray(frames, np.float32)
    flat = frames.reshape((-1,) + frames.shape[-2:])
    return np.stack([d2_of_mask(event_mask(f, threshold, scaled)) for f in flat]).reshape(frames.shape)


def metrics_of_maps(d2f, d2o, cutoff=None):
    """The values of one pair at one threshold from the two int64 maps: a dict with n_pred, n_target, both, and med_miss, med_false,
    hausdorff, baddeley (None where undefined), hausdorff_d2 (the integer under the root)."""
    F, O = d2f == 0, d2o == 0
    nf, no = int(F.sum()), int(O.sum())
    both = nf > 0 and no > 0
    out = {"n_pred": nf, "n_target": no, "both": both, "med_miss": None, "med_false": None, "hausdorff": None, "baddeley": None,
           "hausdorff_d2": None}
    df = np.sqrt(d2f.astype(np.float64)) if nf else None
    do = np.sqrt(d2o.astype(np.float64)) if no else None
    if both:
        out["med_miss"] = float(df[O].sum() / no)
        out["med_false"] = float(do[F].sum() / nf)
        out["hausdorff_d2"] = int(max(d2f[O].max(), d2o[F].max()))
        out["hausdorff"] = float(np.sqrt(np.float64(out["hausdorff_d2"])))
    if cutoff is not None:
        c = np.float64(cutoff)
        wf = np.minimum(df, c) if nf else np.full(d2f.shape, c)
        wo = np.minimum(do, c) if no else np.full(d2o.shape, c)
        out["baddeley"] = float(np.sqrt(((wf - wo) ** 2).sum() / d2f.size))
    elif both:
        out["baddeley"] = float(np.sqrt(((df - do) ** 2).sum() / d2f.size))
    return out


def pair_metrics(pred, target, threshold, cutoff=None, scaled=True):
    """One pair of (H, W) frames at one threshold; {"skipped": True} when either frame holds a non-finite pixel."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    if not (np.isfinite(pred).all() and np.isfinite(target).all()):
        return {"skipped": True}
    out = metrics_of_maps(d2_of_mask(event_mask(pred, threshold, scaled)), d2_of_mask(event_mask(target, threshold, scaled)), cutoff)
    out["skipped"] = False
    return out


def frame_maps(frames, thresholds, scaled=True):
    """frames (..., H, W) -> (finite bool (...), d2 int64 (..., K, H, W)): what distance_state needs of a stack of frames, made once"""
    frames = np.asarray(frames, np.float32)
    lead = frames.shape[:-2]
    finite = np.isfinite(frames).all(axis=(-2, -1))
    d2 = np.stack([distance_map(frames, t, scaled) for t in thresholds], axis=len(lead))
    return finite, d2


def distance_state(ens_maps, target_maps, cutoff, keep_seq):
    """The state after update_members: ens_maps = frame_maps of (M, N, T, H, W), target_maps of (N, T, H, W) ->
    sums fp64 [4, K, T'], counts int64 [6, K, T']"""
    (fin_e, d2_e), (fin_t, d2_t) = ens_maps, target_maps
    M, N, T, K = d2_e.shape[:4]
    Tk = T if keep_seq else 1
    sums, counts = np.zeros((4, K, Tk)), np.zeros((6, K, Tk), np.int64)
    for m in range(M):
        for n in range(N):
            for t in range(T):
                tk = t if keep_seq else 0
                if not (fin_e[m, n, t] and fin_t[n, t]):
                    counts[1, :, tk] += 1
                    continue
                for k in range(K):
                    p = metrics_of_maps(d2_e[m, n, t, k], d2_t[n, t, k], cutoff)
                    counts[0, k, tk] += 1
                    counts[4, k, tk] += p["n_pred"]
                    counts[5, k, tk] += p["n_target"]
                    if p["both"]:
                        counts[2, k, tk] += 1
                        for j in range(3):
                            sums[j, k, tk] += p[SUMS[j]]
                    if p["baddeley"] is not None:
                        counts[3, k, tk] += 1
                        sums[3, k, tk] += p["baddeley"]
    return sums, counts


def compute(sums, counts, mode):
    """SEVIRDistanceScore.compute() of a state: metric -> (K,) for modes "0" and "2", (T', K) for mode "1" """
    s, n = sums.transpose(0, 2, 1), counts.astype(np.float64).transpose(0, 2, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        per = {"med_miss": s[0] / n[2], "med_false": s[1] / n[2], "hausdorff": s[2] / n[2], "baddeley": s[3] / n[3], "frac_both": n[2] / n[0]}
    return {k: v[0] if mode == "0" else v if mode == "1" else v.mean(axis=0) for k, v in per.items()}
