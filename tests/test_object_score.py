"""prediff_amd.object_score (label_objects, SEVIRObjectScore: storm objects and SAL on the device) against tests/_sal_ref.py, the fp64
restatement on numpy and scipy.ndimage.label, which is itself pinned against hand-computed and analytic cases.

Tolerances.  Labels, counts, areas and first-pixel indices: equal.  Peaks: equal.  Masses and centroids: 1e-12 relative.  S, A, L1, L2
of a pair: 1e-9 absolute -- an fp64 sum of <= 16384 non-negative terms carries <= 16384 * 2^-53 ~ 2e-12 relative error and S, A, L are
bounded ratios of such sums, which leaves two orders for the summation order and fails an fp32 accumulation.  Analytic identities that
hold for the mathematical definitions but not bit for bit in fp64 (a shifted frame sums the same values in another order) are held to
1e-12, from the same 2e-12-relative bound on the sums (the quantities are O(1) or below)."""
import math
import os
import socket
from functools import lru_cache

import numpy as np
import pytest
import torch
from scipy import ndimage

import _sal_ref as R
from prediff_amd import SEVIRObjectScore, label_objects
from prediff_amd._lib import PrediffHipError
from prediff_amd.object_score import METRICS

SHAPES = [(1, 1), (1, 128), (128, 1), (5, 7), (37, 53), (128, 128)]
DENSITIES = (0.3, 0.45, 0.55, 0.6)
THR = 0.1                                     # the pattern frames hold 0 or values in [0.2, 1): every set pixel is an object pixel


# ------------------------------------------------------------------------------------------------ frames
def checkerboard(H, W):
    r, c = np.mgrid[0:H, 0:W]
    return (r + c) % 2 == 0


def serpentine(H, W):
    """even rows full, odd rows one pixel alternately at the last and the first column: one 4-connected snake"""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


@lru_cache(maxsize=None)
def pattern_frames(H, W):
    """(names, frames (P, H, W) fp32): the mask patterns with values in [0.2, 1) on them"""
    rng = np.random.default_rng(1000 * H + W)
    masks = {f"bernoulli {d}": rng.random((H, W)) < d for d in DENSITIES}
    masks.update({"checkerboard": checkerboard(H, W), "serpentine": serpentine(H, W), "full": np.ones((H, W), bool),
                  "empty": np.zeros((H, W), bool)})
    vals = (0.2 + 0.8 * rng.random((len(masks), H, W))).astype(np.float32)
    return tuple(masks), np.stack(list(masks.values())) * vals


@lru_cache(maxsize=None)
def pattern_reference(H, W, connectivity, min_pixels=1):
    _, frames = pattern_frames(H, W)
    return [R.object_table(f, threshold=THR, connectivity=connectivity, min_pixels=min_pixels) for f in frames]


def blob(H, W, cy, cx, sigma, amp):
    """a Gaussian bump of compact support (zero beyond 3 sigma)"""
    r, c = np.mgrid[0:H, 0:W]
    d2 = (r - cy) ** 2 + (c - cx) ** 2
    return np.where(d2 <= (3 * sigma) ** 2, amp * np.exp(-d2 / (2.0 * sigma ** 2)), 0.0)


def blob_frames(shape, seed, speckle=0.01):
    """(N, T, H, W) fp32: sums of 1 .. 5 blobs plus a sparse speckle, so that every frame has mass and objects"""
    N, T, H, W = shape
    rng = np.random.default_rng(seed)
    out = np.zeros(shape)
    for n in range(N):
        for t in range(T):
            for _ in range(rng.integers(1, 6)):
                s = rng.uniform(1.5, min(H, W) / 10.0)
                out[n, t] += blob(H, W, rng.uniform(3 * s, H - 1 - 3 * s), rng.uniform(3 * s, W - 1 - 3 * s), s, rng.uniform(0.3, 1.0))
            out[n, t] += (rng.random((H, W)) < speckle) * rng.uniform(0.0, 0.5, (H, W))
    return out.astype(np.float32)


def two_blobs(H=64, W=64):
    return (blob(H, W, 20, 22, 3.0, 1.0) + blob(H, W, 40, 41, 4.0, 0.7)).astype(np.float32)


def cuda5(x):
    """(N, T, H, W) numpy -> NTHWC tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(x))[..., None].cuda()


def one_pair(pred, target, **kw):
    """compute() and counts of a fresh score after one update with the (H, W) frames pred, target"""
    m = SEVIRObjectScore(**kw)
    m.update(cuda5(pred[None, None]), cuda5(target[None, None]))
    return m.compute(), dict(zip(R.COUNTS, m.counts[:, 0].tolist()))


# ------------------------------------------------------------------------------------------------ CPU: the reference
def test_reference_corner_touching_pixels():
    f = np.zeros((5, 7), np.float32)
    f[1, 2], f[2, 3] = 1.0, 0.5
    l8, n8 = R.canonical_labels(f, threshold=0.25, connectivity=8)
    l4, n4 = R.canonical_labels(f, threshold=0.25, connectivity=4)
    assert n8 == 1 and n4 == 2
    assert l8[1, 2] == 1 and l8[2, 3] == 1 and l8.sum() == 2
    assert l4[1, 2] == 1 and l4[2, 3] == 2 and l4.sum() == 3
    _, t8 = R.object_table(f, threshold=0.25, connectivity=8)
    assert t8.shape == (1, 6) and np.array_equal(t8[0], [1.5, 1.0, 2.0, 2.0 / 1.5, 3.5 / 1.5, 9.0])
    _, t4 = R.object_table(f, threshold=0.25, connectivity=4)
    assert np.array_equal(t4, [[1.0, 1.0, 1.0, 1.0, 2.0, 9.0], [0.5, 0.5, 1.0, 2.0, 3.0, 17.0]])
    # threshold=None: max / 15 in fp32 keeps both; min_pixels = 2 drops the two single pixels of the 4-connected case
    assert R.canonical_labels(f, connectivity=8)[1] == 1 and R.canonical_labels(f, connectivity=4, min_pixels=2)[1] == 0
    # raster order of the first pixel, not of scipy's discovery
    g = np.zeros((3, 5), np.float32)
    g[0, 4] = g[1, 4] = g[1, 0] = g[2, 0] = 1.0
    lg, _ = R.canonical_labels(g, threshold=0.5)
    assert lg[0, 4] == 1 and lg[1, 0] == 2
    # hand-computed SAL: F holds one pixel of 3 at (1, 2); O the pixels 2 and 1 at (4, 5) and (4, 6) (one object, R = 3, P = 2)
    a, b = np.zeros((5, 7), np.float32), np.zeros((5, 7), np.float32)
    a[1, 2], b[4, 5], b[4, 6] = 3.0, 2.0, 1.0
    p = R.sal_pair(a, b)
    # D_F = D_O = 3 / 35; V_F = 3 (3 / 3) / 3 = 1, V_O = 3 (3 / 2) / 3 = 1.5; x_F = (1, 2), x_O = (4, 16 / 3); r = 0 (one object each)
    assert p["A"] == 0.0 and abs(p["S"] - (-0.5 / 1.25)) <= 1e-15 and p["L2"] == 0.0 and p["n_pred"] == p["n_target"] == 1
    assert abs(p["L1"] - math.hypot(3.0, 10.0 / 3.0) / math.hypot(4, 6)) <= 1e-15 and p["L"] == p["L1"]
    # two objects in O: r_O = sum R_n |x - x_n| / sum R_n with x = (4, 3), the objects at (4, 0) and (4, 6), masses 1 and 1
    c = np.zeros((5, 7), np.float32)
    c[4, 0], c[4, 6] = 1.0, 1.0
    p = R.sal_pair(a, c, connectivity=4)
    assert p["n_target"] == 2 and abs(p["L2"] - 2.0 * 3.0 / math.hypot(4, 6)) <= 1e-15 and abs(p["A"] - 0.4) <= 1e-15


def test_reference_analytic_cases():
    t = two_blobs()
    d = math.hypot(63, 63)
    same = R.sal_pair(t, t)
    assert (same["S"], same["A"], same["L1"], same["L2"]) == (0.0, 0.0, 0.0, 0.0)
    dbl = R.sal_pair(2 * t, t)
    assert abs(dbl["S"]) <= 1e-15 and abs(dbl["L"]) <= 1e-15 and abs(dbl["A"] - 2.0 / 3.0) <= 1e-15
    sh = R.sal_pair(np.roll(t, (5, 7), (0, 1)), t)
    assert max(abs(sh["S"]), abs(sh["A"]), abs(sh["L2"])) <= 1e-12 and abs(sh["L1"] - math.sqrt(74.0) / d) <= 1e-12
    bl = R.sal_pair(ndimage.gaussian_filter(t.astype(np.float64), 3.0, mode="constant").astype(np.float32), t)
    assert bl["S"] > 0.1 and abs(bl["A"]) < 1e-3
    z = np.zeros_like(t)
    pz = R.sal_pair(z, t)
    assert pz["A"] == -2.0 and pz["S"] is None and pz["L1"] is None and pz["L2"] is None and pz["n_pred"] == 0
    zz = R.sal_pair(z, z)
    assert not zz["skipped"] and all(zz[k] is None for k in ("S", "A", "L1", "L2", "L"))
    tn = t.copy()
    tn[3, 3] = np.nan
    assert R.sal_pair(tn, t) == {"skipped": True} and R.sal_pair(t, tn) == {"skipped": True}
    assert R.canonical_labels(tn)[1] == 0 and R.canonical_labels(tn, threshold=0.1)[1] == 2      # a NaN is never an object pixel
    sums, counts = R.sal_state([(np.stack([t, tn, z])[None], np.stack([t, t, t])[None])], True)
    assert counts.tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 0, 0], [1, 0, 0], [2, 0, 0], [2, 0, 2]]
    assert sums[1].tolist() == [0.0, 0.0, -2.0]


# ------------------------------------------------------------------------------------------------ CPU: the class
def test_constructor_and_argument_refusals():
    for layout in ("NTHWX", "NTHHW", "THWC", "NTWC", "NTHC", "NT"):
        with pytest.raises(ValueError):
            SEVIRObjectScore(layout=layout)
    with pytest.raises(NotImplementedError):
        SEVIRObjectScore(mode="3")
    for mode in ("1", "2"):
        with pytest.raises(ValueError):
            SEVIRObjectScore(mode=mode)
    with pytest.raises(ValueError):
        SEVIRObjectScore(metrics_list=("S", "csi"))
    x = torch.zeros((1, 2, 16, 16, 1))
    for kw in ({"connectivity": 6}, {"thr_factor": 0.0}, {"thr_factor": -1.0}, {"min_pixels": 0}):
        with pytest.raises(ValueError):
            SEVIRObjectScore(**kw)
        with pytest.raises(ValueError):
            label_objects(x, **kw)
    with pytest.raises(ValueError):
        label_objects(x, max_objects=0)
    with pytest.raises(ValueError):
        label_objects(x, layout="NTC")
    with pytest.raises(PrediffHipError):
        label_objects(x)                                                     # a CPU tensor
    with pytest.raises(PrediffHipError):
        SEVIRObjectScore().update(x, x)
    with pytest.raises(PrediffHipError):
        SEVIRObjectScore().update_members(x[None], x)
    with pytest.raises(ValueError):
        SEVIRObjectScore().update(x, x[:, :1])
    with pytest.raises(ValueError):
        SEVIRObjectScore().update_members(x, x)                              # not (M,) + target.shape
    m = SEVIRObjectScore(layout="NHWT", mode="1", seq_len=6, metrics_list=("S", "L"), threshold=16, connectivity=4, min_pixels=3)
    assert m.keep_seq_len_dim and m.threshold == 16.0 and m.connectivity == 4 and m.min_pixels == 3
    assert SEVIRObjectScore.METRICS == METRICS == ("S", "A", "L", "L1", "L2", "abs_S", "abs_A", "n_obj_pred", "n_obj_target")
    assert SEVIRObjectScore().thr_factor == 1.0 / 15.0 and SEVIRObjectScore().threshold is None


_SUMS = [[1.0, 0.0, -2.0], [0.5, 0.0, 3.0], [0.25, 0.0, 0.5], [0.5, 0.0, 1.5], [0.75, 0.0, 2.0], [3.0, 0.0, 2.0], [1.5, 0.0, 3.0]]
_COUNTS = [[4, 0, 8], [1, 2, 0], [2, 0, 4], [4, 0, 6], [1, 0, 2], [1, 0, 2], [8, 0, 4], [6, 0, 16]]


def test_compute_from_hand_set_state():
    sums, counts = torch.tensor(_SUMS, dtype=torch.float64), torch.tensor(_COUNTS, dtype=torch.int64)
    m = SEVIRObjectScore(mode="1", seq_len=3)
    m.sums, m.counts = sums, counts
    r = m.compute()
    assert tuple(r) == METRICS
    exp = {"S": [0.5, math.nan, -0.5], "A": [0.125, math.nan, 0.5], "L1": [0.25, math.nan, 0.25], "L2": [0.5, math.nan, 0.75],
           "L": [0.75, math.nan, 1.0], "abs_S": [1.5, math.nan, 0.5], "abs_A": [0.375, math.nan, 0.5],
           "n_obj_pred": [2.0, math.nan, 0.5], "n_obj_target": [1.5, math.nan, 2.0]}
    for k in METRICS:
        assert np.array_equal(r[k], exp[k], equal_nan=True), (k, r[k])
    m2 = SEVIRObjectScore(mode="2", seq_len=2, metrics_list=("L", "S"))
    m2.sums, m2.counts = sums[:, [0, 2]], counts[:, [0, 2]]
    r2 = m2.compute()
    assert list(r2) == ["L", "S"] and r2 == {"L": 0.875, "S": 0.0}
    m0 = SEVIRObjectScore(mode="0")
    m0.sums, m0.counts = sums.sum(dim=1, keepdim=True), counts.sum(dim=1, keepdim=True)
    r0 = m0.compute()
    assert r0["S"] == -1.0 / 6.0 and r0["A"] == 0.35 and r0["n_obj_pred"] == 1.0 and r0["L2"] == 2.0 / 3.0
    # no update: NaNs of the mode's shape
    e0, e1, e2 = SEVIRObjectScore().compute(), SEVIRObjectScore(mode="1", seq_len=4).compute(), SEVIRObjectScore(mode="2", seq_len=4).compute()
    assert all(isinstance(e0[k], float) and math.isnan(e0[k]) for k in METRICS)
    assert all(e1[k].shape == (4,) and np.isnan(e1[k]).all() for k in METRICS)
    assert all(isinstance(e2[k], float) and math.isnan(e2[k]) for k in METRICS)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = SEVIRObjectScore(mode="1", seq_len=3)
        if rank == 0:                                   # rank 1 made no update: it takes part with a zero state
            m.sums, m.counts = torch.tensor(_SUMS, dtype=torch.float64), torch.tensor(_COUNTS, dtype=torch.int64)
        m.sync()
        q.put((rank, m.sums.tolist(), m.counts.tolist(), m.compute()["S"].tolist()[::2]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sync_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r[0]: r[1:] for r in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        assert got[r][0] == _SUMS and got[r][1] == _COUNTS and got[r][2] == [0.5, -0.5], (r, got[r])
    SEVIRObjectScore().sync()                           # no process group: a no-op


# ------------------------------------------------------------------------------------------------ GPU: labels and the table
def check_objects(label, got, ref, max_objects):
    """(labels (H, W), n, table (max_objects, 6)) of one frame against the reference's (labels, table)"""
    labels, n, table = got
    rl, rt = ref
    assert n == rt.shape[0], (label, n, rt.shape[0])
    assert np.array_equal(labels, rl), (label, int((labels != rl).sum()))
    k = min(n, max_objects)
    assert np.array_equal(table[:k, 2], rt[:k, 2]) and np.array_equal(table[:k, 5], rt[:k, 5]), label       # area, first pixel
    assert np.array_equal(table[:k, 1], rt[:k, 1]), label                                                   # peak
    for col, name in ((0, "mass"), (3, "row"), (4, "col")):
        err = np.abs(table[:k, col] - rt[:k, col])
        assert (err <= 1e-12 * np.abs(rt[:k, col])).all(), (label, name, float(err.max()))
    assert not table[k:].any(), label


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hip_labels_and_table_of_the_patterns(shape, connectivity):
    H, W = shape
    names, frames = pattern_frames(H, W)
    ref = pattern_reference(H, W, connectivity)
    cap = max(1, max(t.shape[0] for _, t in ref))
    labels, n, table = label_objects(cuda5(frames[:, None]), threshold=THR, connectivity=connectivity, max_objects=cap)
    assert labels.dtype == torch.int32 and labels.shape == (len(names), 1, H, W) and n.dtype == torch.int32 and n.shape == (len(names), 1)
    assert table.dtype == torch.float64 and table.shape == (len(names), 1, cap, 6)
    labels, n, table = labels.cpu().numpy(), n.cpu().numpy(), table.cpu().numpy()
    for i, name in enumerate(names):
        check_objects(f"{name} {H}x{W} c{connectivity}", (labels[i, 0], int(n[i, 0]), table[i, 0]), ref[i], cap)
    count = dict(zip(names, n[:, 0].tolist()))
    assert count["empty"] == 0 and count["full"] == 1 and count["serpentine"] == 1
    assert count["checkerboard"] == ((H * W + 1) // 2 if connectivity == 4 or min(H, W) == 1 else 1)
    if shape == (128, 128) and connectivity == 4:
        assert count["checkerboard"] == 8192            # the worst case: more objects than one batch of slots, by a factor of 16


@pytest.mark.gpu
def test_hip_labels_checkerboard_64_and_isolated_pixels():
    f = (checkerboard(64, 64) * 0.5).astype(np.float32)
    iso = np.zeros((128, 128), np.float32)
    iso[0::2, 0::2] = 0.75                              # 4096 pixels that no 8-neighbourhood joins
    for conn, want in ((4, 2048), (8, 1)):
        labels, n, _ = label_objects(cuda5(f[None, None]), threshold=THR, connectivity=conn, max_objects=1)
        assert int(n[0, 0]) == want and np.array_equal(labels[0, 0].cpu().numpy(), R.canonical_labels(f, threshold=THR, connectivity=conn)[0])
    labels, n, table = label_objects(cuda5(iso[None, None]), connectivity=8, max_objects=4096)
    rl, rt = R.object_table(iso, connectivity=8)
    check_objects("4096 isolated pixels", (labels[0, 0].cpu().numpy(), int(n[0, 0]), table[0, 0].cpu().numpy()), (rl, rt), 4096)
    assert int(n[0, 0]) == 4096


@pytest.mark.gpu
def test_hip_labels_strided_view_bf16_min_pixels_and_truncated_table():
    names, frames = pattern_frames(37, 53)
    x = cuda5(frames.reshape(2, 4, 37, 53))
    base = label_objects(x, threshold=THR, connectivity=4, max_objects=600)
    # layout "NHWT" as a view of the same memory, read in place
    view = x[..., 0].permute(0, 2, 3, 1)
    assert not view.is_contiguous()
    got = label_objects(view, layout="NHWT", threshold=THR, connectivity=4, max_objects=600)
    assert all(torch.equal(a, b) for a, b in zip(base, got))
    # bf16 input is read as its float values
    xb = x.bfloat16()
    a, b = label_objects(xb, connectivity=8), label_objects(xb.float(), connectivity=8)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    fb = xb.float().cpu().numpy()[..., 0]
    for i in range(2):
        ref = R.object_table(fb[i, 0], connectivity=8)
        check_objects(f"bf16 frame {i}", (a[0][i, 0].cpu().numpy(), int(a[1][i, 0]), a[2][i, 0].cpu().numpy()), ref, 256)
    # min_pixels = 4 on the density-0.3 masks; max_objects below the count truncates the table only
    for H, W in ((37, 53), (128, 128)):
        f = pattern_frames(H, W)[1][0]
        for conn in (4, 8):
            ref = R.object_table(f, threshold=THR, connectivity=conn, min_pixels=4)
            full = R.canonical_labels(f, threshold=THR, connectivity=conn)[1]
            assert 0 < ref[1].shape[0] < full
            labels, n, table = label_objects(cuda5(f[None, None]), threshold=THR, connectivity=conn, min_pixels=4, max_objects=7)
            assert ref[1].shape[0] > 7 and table.shape == (1, 1, 7, 6)
            check_objects(f"min_pixels 4 {H}x{W} c{conn}", (labels[0, 0].cpu().numpy(), int(n[0, 0]), table[0, 0].cpu().numpy()), ref, 7)


@pytest.mark.gpu
def test_hip_threshold_is_the_fp32_product():
    """threshold=None: pixels one ulp either side of float32(thr_factor) * max decide the mask exactly as the fp32 product does."""
    rng = np.random.default_rng(5)
    frames = []
    for mx in (1.0, 0.7312345, 254.99, 3.0e-3):
        mx = np.float32(mx)
        for factor in (1.0 / 15.0, 0.3):
            thr = np.float32(factor) * mx
            near = np.array([thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(np.inf))], np.float32)
            f = near[rng.integers(0, 3, (16, 24))]
            f[rng.integers(0, 16), rng.integers(0, 24)] = mx
            frames.append((f, factor))
    for f, factor in frames:
        labels, n, _ = label_objects(cuda5(f[None, None]), thr_factor=factor, connectivity=4, max_objects=1)
        rl, rn = R.canonical_labels(f, thr_factor=factor, connectivity=4)
        assert 1 < rn and int(n[0, 0]) == rn and np.array_equal(labels[0, 0].cpu().numpy(), rl)
        assert np.array_equal(rl > 0, f >= np.float32(factor) * f.max())


# ------------------------------------------------------------------------------------------------ GPU: SAL
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 2, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_hip_sal_values_against_the_reference(shape):
    N, T, H, W = shape
    pred, target = blob_frames(shape, 31), blob_frames(shape, 32)
    for conn in (8, 4):
        worst = dict.fromkeys(("S", "A", "L1", "L2"), 0.0)
        for n in range(N):                              # one n per update and mode "1": the state holds single pairs
            m = SEVIRObjectScore(mode="1", seq_len=T, connectivity=conn)
            m.update(cuda5(pred[n:n + 1]), cuda5(target[n:n + 1]))
            counts, r = m.counts.cpu().numpy(), m.compute()
            assert (counts[0] == 1).all() and (counts[1] == 0).all() and (counts[2:6] == 1).all(), counts       # every pair fully defined
            for t in range(T):
                ref = R.sal_pair(pred[n, t], target[n, t], connectivity=conn)
                assert counts[6, t] == ref["n_pred"] and counts[7, t] == ref["n_target"]
                for k in worst:
                    worst[k] = max(worst[k], abs(r[k][t] - ref[k]))
                assert abs(r["L"][t] - ref["L"]) <= 2e-9 and r["abs_S"][t] == abs(r["S"][t]) and r["abs_A"][t] == abs(r["A"][t])
        print(f"[object_score parity] {shape} c{conn}: max |delta| " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert all(v <= 1e-9 for v in worst.values()), worst
    # the batched state in mode "0" is the sum of those pairs
    m = SEVIRObjectScore(mode="0")
    m.update(cuda5(pred), cuda5(target))
    sums, counts = R.sal_state([(pred, target)], False)
    assert np.array_equal(m.counts.cpu().numpy(), counts)
    assert (np.abs(m.sums.cpu().numpy() - sums) <= 1e-9 * N * T).all()


@pytest.mark.gpu
def test_hip_sal_analytic_cases():
    t = two_blobs()
    d = math.hypot(63, 63)
    r, c = one_pair(t, t)
    assert r["S"] == 0.0 and r["A"] == 0.0 and r["L1"] == 0.0 and r["L2"] == 0.0 and r["L"] == 0.0
    assert c["pairs"] == 1 and c["n_S"] == c["n_A"] == c["n_L1"] == c["n_L"] == 1 and r["n_obj_pred"] == r["n_obj_target"] == 2.0
    r, _ = one_pair(2 * t, t)                           # a power of two scales every fixed-point sum exactly
    assert r["S"] == 0.0 and r["L"] == 0.0 and abs(r["A"] - 2.0 / 3.0) <= 1e-15
    r, _ = one_pair(np.roll(t, (5, 7), (0, 1)), t)
    assert max(abs(r["S"]), abs(r["A"]), abs(r["L2"])) <= 1e-12 and abs(r["L1"] - math.sqrt(74.0) / d) <= 1e-12
    r, _ = one_pair(ndimage.gaussian_filter(t.astype(np.float64), 3.0, mode="constant").astype(np.float32), t)
    assert r["S"] > 0.1 and abs(r["A"]) < 1e-3
    z = np.zeros_like(t)
    r, c = one_pair(z, t)
    assert r["A"] == -2.0 and math.isnan(r["S"]) and math.isnan(r["L1"]) and math.isnan(r["L2"]) and math.isnan(r["L"])
    assert (c["pairs"], c["skipped"], c["n_S"], c["n_A"], c["n_L1"], c["n_L"], c["obj_pred"], c["obj_target"]) == (1, 0, 0, 1, 0, 0, 0, 2)
    r, c = one_pair(z, z)
    assert all(math.isnan(r[k]) for k in ("S", "A", "L", "L1", "L2")) and r["n_obj_pred"] == 0.0
    assert (c["pairs"], c["skipped"], c["n_S"], c["n_A"], c["n_L1"], c["n_L"]) == (1, 0, 0, 0, 0, 0)


@pytest.mark.gpu
def test_hip_sal_nan_pair_is_skipped_and_stays_in_its_lead_time():
    pred, target = blob_frames((2, 3, 37, 53), 41), blob_frames((2, 3, 37, 53), 42)
    clean = SEVIRObjectScore(mode="1", seq_len=3)
    clean.update(cuda5(pred), cuda5(target))
    for which in ("pred", "target"):
        p, t = pred.copy(), target.copy()
        (p if which == "pred" else t)[1, 1, 20, 30] = np.nan
        m = SEVIRObjectScore(mode="1", seq_len=3)
        m.update(cuda5(p), cuda5(t))
        assert torch.equal(m.sums[:, [0, 2]], clean.sums[:, [0, 2]]) and torch.equal(m.counts[:, [0, 2]], clean.counts[:, [0, 2]])
        sums, counts = R.sal_state([(p, t)], True)
        assert np.array_equal(m.counts.cpu().numpy(), counts) and counts[0, 1] == 1 and counts[1, 1] == 1
        assert np.isfinite(m.sums.cpu().numpy()).all() and (np.abs(m.sums.cpu().numpy() - sums) <= 2e-9).all()
        assert all(np.isfinite(v).all() for v in m.compute().values())
    # an infinite pixel is skipped the same way; a NaN is never an object pixel of label_objects
    p = pred.copy()
    p[0, 0, 5, 5] = np.inf
    m = SEVIRObjectScore(mode="1", seq_len=3)
    m.update(cuda5(p), cuda5(target))
    assert m.counts[:2].tolist() == [[1, 2, 2], [1, 0, 0]]
    p = pred.copy()
    p[0, 0, 5, 5] = np.nan
    labels, n, _ = label_objects(cuda5(p[:1, :1]), threshold=0.05)
    rl, rn = R.canonical_labels(p[0, 0], threshold=0.05)
    assert rn > 0 and int(n[0, 0]) == rn and np.array_equal(labels[0, 0].cpu().numpy(), rl)
    assert int(label_objects(cuda5(p[:1, :1]))[1][0, 0]) == 0           # threshold=None: max(frame) is NaN


# ------------------------------------------------------------------------------------------------ GPU: state handling
@pytest.mark.gpu
@pytest.mark.parametrize("M", [5, 32])
def test_hip_sal_members_equal_sequential_updates(M):
    shape = (2, 3, 37, 53)
    target = blob_frames(shape, 50)
    ens = np.stack([blob_frames(shape, 51 + i) for i in range(M)])
    ec, tc = torch.from_numpy(ens)[..., None].cuda(), cuda5(target)
    for mode in ("1", "0"):
        a, b = (SEVIRObjectScore(mode=mode, seq_len=3) for _ in range(2))
        a.update_members(ec, tc)
        for i in range(M):
            b.update(ec[i], tc)
        assert torch.equal(a.counts, b.counts) and int(a.counts[0].sum()) == M * 6
        sa, sb = a.sums.cpu().numpy(), b.sums.cpu().numpy()
        assert (np.abs(sa - sb) <= 1e-12 * np.abs(sb)).all(), (sa, sb)
        again = SEVIRObjectScore(mode=mode, seq_len=3)
        again.update_members(ec, tc)
        assert torch.equal(again.sums, a.sums)          # the same call gives the same bits
    with pytest.raises(ValueError):
        SEVIRObjectScore().update_members(torch.zeros((513, 1, 1, 8, 8, 1), device="cuda"), torch.zeros((1, 1, 8, 8, 1), device="cuda"))


@pytest.mark.gpu
def test_hip_sal_state_accumulates_resets_and_refuses():
    p1, t1 = blob_frames((2, 3, 37, 53), 60), blob_frames((2, 3, 37, 53), 61)
    p2, t2 = blob_frames((1, 3, 37, 53), 62), blob_frames((1, 3, 37, 53), 63)
    m = SEVIRObjectScore(mode="1", seq_len=3, min_pixels=2, connectivity=4)
    m.update(cuda5(p1), cuda5(t1))
    first = m.sums.clone()
    m.update(cuda5(p2), cuda5(t2))
    sums, counts = R.sal_state([(p1, t1), (p2, t2)], True, min_pixels=2, connectivity=4)
    assert np.array_equal(m.counts.cpu().numpy(), counts) and (np.abs(m.sums.cpu().numpy() - sums) <= 3e-9).all()
    m.reset()
    assert m.sums is None and m.counts is None and math.isnan(m.compute()["S"][0])
    m.update(cuda5(p1), cuda5(t1))
    assert torch.equal(m.sums, first)
    # refusals: a side above 128 before any launch (the state stays zero), C > 1
    for shape in ((1, 1, 129, 16, 1), (1, 1, 16, 129, 1)):
        x = torch.rand(shape).cuda()
        s = SEVIRObjectScore()
        with pytest.raises(PrediffHipError, match="128"):
            s.update(x, x)
        assert float(s.sums.abs().sum()) == 0.0 and int(s.counts.sum()) == 0
        with pytest.raises(PrediffHipError, match="128"):
            label_objects(x)
    x = torch.rand((1, 1, 16, 16, 2)).cuda()
    with pytest.raises(ValueError):
        SEVIRObjectScore().update(x, x)
    with pytest.raises(ValueError):
        label_objects(x)
    labels, n, _ = label_objects(torch.rand((2, 3, 16, 16)).cuda(), layout="NTHW")      # C absent from the layout
    assert labels.shape == (2, 3, 16, 16) and n.shape == (2, 3)


@pytest.mark.gpu
def test_evaluate_context_updates_object_scores():
    """evaluate_context on the tiny latent-diffusion model of the config tests: the object scores see every sample where the frame scores
    do, and a call without the keywords returns what it returned before."""
    import _templates as TP
    from _cases import TINY_UNET_CFGS, TINY_VAE_CFG
    from _weights import seeded_input, seeded_state_dict
    from test_alignment import _tiny_alignment
    from prediff_amd import config as CFG
    from prediff_amd.autoencoder_kl import AutoencoderKL
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.latent_diffusion import LatentDiffusion
    vae = AutoencoderKL(**TINY_VAE_CFG, precision="fp32")
    vae.load_state_dict(seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 601))
    cfg = TINY_UNET_CFGS["axial"]
    net = CuboidTransformerUNet(**cfg, precision="fp32")
    net.load_state_dict(seeded_state_dict(TP.unet_template(cfg, "tiny_unet_schema.json", "axial"), 600))
    T_in, (T_out, H, W, _) = cfg["input_shape"][0], cfg["target_shape"]
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(T_out, H * 4, W * 4, 1), timesteps=1000, use_ema=False,
                          latent_shape=tuple(cfg["target_shape"]), first_stage_model=vae.cuda(),
                          cond_stage_model="__is_first_stage__").cuda().eval()
    al = _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    B, K = 2, 2
    seq = seeded_input("osseq", (B, T_in + T_out, H * 4, W * 4, 1), 23, kind="uniform").cuda()
    run_cfg = {"layout": {"in_len": T_in, "out_len": T_out}, "eval": {"num_samples_per_context": K}}
    os_, aos = (SEVIRObjectScore(layout="NTHWC", mode="1", seq_len=T_out, threshold=0.5) for _ in range(2))
    torch.manual_seed(7)
    out = CFG.evaluate_context(ldm, seq, run_cfg, object_score=os_, aligned_object_score=aos, timesteps=3)
    torch.manual_seed(7)
    plain = CFG.evaluate_context(ldm, seq, run_cfg, timesteps=3)
    assert set(out) == set(plain) == {"pred", "aligned_pred"}
    for k in out:
        assert len(out[k]) == len(plain[k]) == K and all(torch.equal(a, b) for a, b in zip(out[k], plain[k])), k
    tgt = seq[:, T_in:]
    for metric, preds in ((os_, out["pred"]), (aos, out["aligned_pred"])):
        manual = SEVIRObjectScore(layout="NTHWC", mode="1", seq_len=T_out, threshold=0.5)
        for pr in preds:
            manual.update(pr.float(), tgt)
        assert torch.equal(metric.sums, manual.sums) and torch.equal(metric.counts, manual.counts)
        assert int(metric.counts[:2, 0].sum()) == B * K
        sums, counts = R.sal_state([(pr.float().cpu().numpy()[..., 0], tgt.cpu().numpy()[..., 0]) for pr in preds], True, threshold=0.5)
        assert np.array_equal(metric.counts.cpu().numpy(), counts) and (np.abs(metric.sums.cpu().numpy() - sums) <= 1e-9 * B * K).all()
