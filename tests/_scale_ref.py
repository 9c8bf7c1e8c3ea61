"""CPU restatement of prediff_amd.scale_score (the intensity-scale skill score and the Haar energies; Casati et al. 2004, Casati 2010) on
numpy: the yardstick of tests/test_scale_score.py.  Q_l comes from reshaped integer block sums; the state is int64; compute() is fp64 with
the subtraction 4 Q_{l-1} - Q_l made in int64 first.  `explicit_components` is the decomposition spelled out (block-mean fields, their
differences, the mean squares): it is used only to check the integer form, in tests/test_scale_score_host.py."""
import numpy as np

MAX_LEVELS = 8
METRICS = ("mse", "mse_random", "iss", "energy_pred", "energy_target", "energy_bias", "base_rate", "freq_bias")


def event_mask(x, threshold, scaled=True):
    """float32(x) / float32(1/255) >= float32(threshold) (scaled) or float32(x) >= float32(threshold); a NaN is never an event"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x / np.float32(1.0 / 255.0) if scaled else x
        return v >= np.float32(threshold)


def top_level(H, W):
    """n with 2^n the smallest power of two >= max(H, W, 2)"""
    n = 1
    while 2 ** n < max(H, W):
        n += 1
    return n


def pad(field):
    """(H, W) -> int64 (S, S): the field at the top-left corner of zeros"""
    H, W = field.shape
    S = 2 ** top_level(H, W)
    out = np.zeros((S, S), np.int64)
    out[:H, :W] = field
    return out


def block_sums(padded, l):
    """int64 (S / 2^l, S / 2^l): the sums over the 2^l x 2^l blocks"""
    S, b = padded.shape[0], 2 ** l
    return padded.reshape(S // b, b, S // b, b).sum(axis=(1, 3))


def q_levels(field):
    """Q_l, l = 0 .. n, of an integer (H, W) field (a 0 / 1 mask, or a difference of two): int64 (n + 1,)"""
    p = pad(np.asarray(field).astype(np.int64))
    n = top_level(*np.asarray(field).shape)
    return np.array([(block_sums(p, l) ** 2).sum() for l in range(n + 1)], np.int64)


def scale_energy(frames, threshold, scaled=True):
    """frames (..., H, W) -> int64 (..., n + 1)"""
    frames = np.asarray(frames, np.float32)
    flat = frames.reshape((-1,) + frames.shape[-2:])
    q = np.stack([q_levels(event_mask(f, threshold, scaled)) for f in flat])
    return q.reshape(frames.shape[:-2] + (q.shape[-1],))


def explicit_components(field):
    """fp64 (n + 1,): mean(W_l^2) for l = 1 .. n and mean(F_n^2) over the padded field, from the block-mean fields themselves"""
    p = pad(np.asarray(field).astype(np.int64)).astype(np.float64)
    S = p.shape[0]
    n = top_level(*np.asarray(field).shape)

    def smooth(l):
        b = 2 ** l
        return np.kron(p.reshape(S // b, b, S // b, b).mean(axis=(1, 3)), np.ones((b, b)))

    fathers = [smooth(l) for l in range(n + 1)]
    comps = [fathers[l - 1] - fathers[l] for l in range(1, n + 1)] + [fathers[n]]
    assert np.abs(sum(comps) - p).max() <= 1e-12                       # the components sum to the field
    return np.array([(c ** 2).mean() for c in comps])


def component_means(q, n, area_pairs):
    """q int64 (..., n + 1); area_pairs int64 (...) = N P -> fp64 (..., n + 1): (4 Q_{l-1} - Q_l) / (4^l N P), l = 1 .. n; Q_n / (4^n N P)"""
    q = np.asarray(q, np.int64)
    num = np.concatenate([4 * q[..., :-1] - q[..., 1:], q[..., -1:]], axis=-1)
    den = np.asarray(area_pairs, np.int64)[..., None] * np.array([4 ** l for l in range(1, n + 1)] + [4 ** n], np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return num.astype(np.float64) / den.astype(np.float64)


def parseval_holds(q, n):
    """sum over l = 1 .. n of (4 Q_{l-1} - Q_l) 4^(n-l), plus Q_n, equals 4^n Q_0: on Python integers"""
    q = [int(v) for v in q[:n + 1]]
    return sum((4 * q[l - 1] - q[l]) * 4 ** (n - l) for l in range(1, n + 1)) + q[n] == 4 ** n * q[0]


def pair_records(ens, target, thresholds, scaled=True):
    """ens (M, N, T, H, W), target (N, T, H, W) -> (scored bool (M, N, T), q int64 (M, N, T, K, 3, 8)): per pair and threshold, Q_l of
    I_F, I_O and Z (zero above n, and zero for a pair that is skipped: one with a non-finite pixel in either frame), made once"""
    ens, target = np.asarray(ens, np.float32), np.asarray(target, np.float32)
    M, N, T, H, W = ens.shape
    K, n = len(thresholds), top_level(H, W)
    scored = np.isfinite(ens).all(axis=(-2, -1)) & np.isfinite(target).all(axis=(-2, -1))[None]
    q = np.zeros((M, N, T, K, 3, MAX_LEVELS), np.int64)
    for i in range(N):
        for t in range(T):
            for k, thr in enumerate(thresholds):
                o = event_mask(target[i, t], thr, scaled).astype(np.int64)
                qo = q_levels(o)
                for m in range(M):
                    if scored[m, i, t]:
                        f = event_mask(ens[m, i, t], thr, scaled).astype(np.int64)
                        q[m, i, t, k, :, :n + 1] = [q_levels(f), qo, q_levels(f - o)]
    return scored, q


def state_of_records(scored, q, keep_seq):
    """The state after update_members with these pairs: energy int64 [3, K, 8, T'], counts int64 [2, T'] (pairs scored, skipped)"""
    energy = q.sum(axis=(0, 1)).transpose(2, 1, 3, 0)                                  # (T, K, 3, 8) -> (3, K, 8, T)
    counts = np.stack([scored.sum(axis=(0, 1)), (~scored).sum(axis=(0, 1))]).astype(np.int64)
    if not keep_seq:
        energy, counts = energy.sum(axis=3, keepdims=True), counts.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(energy), counts


def scale_state(ens, target, thresholds, keep_seq, scaled=True):
    """The state after update_members: ens (M, N, T, H, W), target (N, T, H, W) -> energy int64 [3, K, 8, T'], counts int64 [2, T']"""
    return state_of_records(*pair_records(ens, target, thresholds, scaled), keep_seq)


def compute(energy, counts, n, mode):
    """SEVIRScaleScore.compute() of a state: metric -> (K[, L]) for modes "0" and "2", (T', K[, L]) for mode "1" """
    energy, counts = np.asarray(energy, np.int64), np.asarray(counts, np.int64)
    K, Tk = energy.shape[1], energy.shape[3]
    L = n + 1
    q = energy.transpose(0, 3, 1, 2)[..., :L]                                          # (3, T', K, L)
    area_pairs = np.broadcast_to((counts[0] * 4 ** n)[:, None], (Tk, K))               # N P, N = 4^n
    comp = [component_means(q[a], n, area_pairs) for a in range(3)]
    q0 = q[..., 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bf, bo = q0[0] / area_pairs.astype(np.float64), q0[1] / area_pairs.astype(np.float64)
        rnd = bf * (1.0 - bo) + bo * (1.0 - bf)
        per = {"mse": comp[2], "mse_random": rnd, "iss": 1.0 - L * comp[2] / rnd[..., None], "energy_pred": comp[0],
               "energy_target": comp[1], "energy_bias": (comp[0] - comp[1]) / (comp[0] + comp[1]), "base_rate": bo,
               "freq_bias": np.where(q0[1] > 0, q0[0] / q0[1], np.nan)}
    return {k: v[0] if mode == "0" else v if mode == "1" else v.mean(axis=0) for k, v in per.items()}
