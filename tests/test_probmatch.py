"""prediff_amd.probability_matching on the device against the NumPy restatement of tests/_probmatch_ref.py.

Every result is a selection of input values, so every comparison is for equality: np.array_equal (NaN frames with equal_nan) and, on top,
the same bit patterns (a -0.0 is not a +0.0 here).  No tolerance appears in this file.

Sizes: n = 1, 2, 3; the wave boundary 63, 64, 65; the workgroup boundary 1023, 1024, 1025; non-powers of two; degenerate sides; the
largest frame both ways.  Value patterns: continuous, radar-like (mostly ties: stability is what is tested), all equal, sorted both ways,
signed zeros with denormals, and one NaN / one +inf in one frame of the batch.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import _probmatch_ref as R
from prediff_amd import StochasticExtrapolation, match_cdf, probability_matched_mean, rank_frames
from prediff_amd import _lib as L
from prediff_amd import probability_matching as PM
from prediff_amd._lib import PrediffHipError

pytestmark = pytest.mark.gpu

THR = 16 / 255
GUARD = 1024
SIZES = ((1, 1), (1, 2), (3, 1), (7, 9), (8, 8), (5, 13), (33, 31), (32, 32), (25, 41), (5, 7), (37, 53), (1, 128), (128, 1), (128, 128),
         (1, 16384))
LEVELS = np.asarray([0.02, 0.05, 0.08, 0.11, 0.2, 0.35, 0.6, 0.9], np.float32)
FINITE = 8                  # frames 0 .. 7 of frames_of are finite, 8 holds a NaN, 9 a +inf


def radar(rng, shape, zeros):
    v = LEVELS[rng.integers(0, 8, shape)]
    return np.where(rng.random(shape) < zeros, np.float32(0), v).astype(np.float32)


@lru_cache(maxsize=None)
def frames_of(H, W):
    """(10, H, W, 1) float32: continuous, radar 70 % zeros, radar 90 % zeros, all equal, all zero, ascending, descending, signed zeros and
    denormals, the continuous frame with one NaN, the radar frame with one +inf"""
    rng = np.random.default_rng(H * 100003 + W)
    n = H * W
    cont = rng.random(n, dtype=np.float32)
    asc = np.sort(rng.random(n, dtype=np.float32))
    tiny = np.asarray([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, -1.1754944e-38, 0.5, -0.5],
                      np.float32)
    mix = tiny[rng.integers(0, tiny.size, n)]
    bad_nan, bad_inf = cont.copy(), radar(rng, n, 0.7)
    bad_nan[rng.integers(0, n)] = np.nan
    bad_inf[rng.integers(0, n)] = np.inf
    F = np.stack([cont, radar(rng, n, 0.7), radar(rng, n, 0.9), np.full(n, 0.3, np.float32), np.zeros(n, np.float32), asc, asc[::-1].copy(),
                  mix, bad_nan, bad_inf]).reshape(10, H, W, 1)
    F.setflags(write=False)
    return F


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def same(got, want):
    """equal values (NaN = NaN) and equal bits"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")
    if got.dtype == np.float32:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


class Guarded:
    """a device tensor of `shape` between two NaN guards of GUARD floats, NaN itself until written (int32: the NaN bit pattern)"""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def ws_of(need):
    g = Guarded((max(need, 8) // 4,))
    return g, g.t.view(torch.uint8)[:max(need, 1)]


# ------------------------------------------------------------------------------------------------ rank_frames
@pytest.mark.parametrize("H,W", SIZES)
def test_rank_frames(H, W):
    F = frames_of(H, W)
    x = F.reshape(2, 5, H, W, 1)
    want_sorted, want_order = R.rank_frames(x)
    for f in range(FINITE):                 # the restatement is the stable argsort and the gathered bits
        assert np.array_equal(want_order.reshape(10, -1)[f], np.argsort(F[f].ravel(), kind="stable"))
    assert (want_order.reshape(10, -1)[FINITE:] == -1).all() and np.isnan(want_sorted.reshape(10, -1)[FINITE:]).all()
    srt, order = rank_frames(dev(x))
    assert order.dtype == torch.int32 and tuple(order.shape) == (2, 5, H * W)
    same(order, want_order)
    same(srt, want_sorted)
    # a frame alone gives the bits it gives in the batch; a bare (H, W, 1) frame is a frame
    for f in (0, 1, 7):
        s1, o1 = rank_frames(dev(F[f]))
        same(o1, want_order.reshape(10, -1)[f])
        same(s1, want_sorted.reshape(10, -1)[f])


# ------------------------------------------------------------------------------------------------ match_cdf
@pytest.mark.parametrize("H,W", SIZES)
def test_match_cdf(H, W):
    F = frames_of(H, W)
    x = F.reshape(2, 5, H, W, 1)
    ref = np.ascontiguousarray(np.roll(F, 3, axis=0)[::-1]).reshape(2, 5, H, W, 1)          # another frame for every frame, both NaN kinds
    ref1 = np.ascontiguousarray(F[[1, 0]]).reshape(2, 1, H, W, 1)
    x6 = np.stack([x, np.ascontiguousarray(np.roll(F, 1, axis=0)).reshape(2, 5, H, W, 1), x[::-1]])
    dx, dx6, dref, dref1 = dev(x), dev(x6), dev(ref), dev(ref1)
    keep = [t.clone() for t in (dx, dx6, dref, dref1)]
    for thr in (None, THR):
        same(match_cdf(dx, dref, threshold=thr), R.match_cdf(x, ref, thr))
        same(match_cdf(dx, dref1, threshold=thr), R.match_cdf(x, ref1, thr))
        same(match_cdf(dx6, dref1, threshold=thr), R.match_cdf(x6, ref1, thr))
    same(match_cdf(dx6, dref, threshold=THR), R.match_cdf(x6, ref, THR))
    for t, k in zip((dx, dx6, dref, dref1), keep):                                          # the inputs are read only
        assert np.array_equal(t.cpu().numpy().view(np.uint32), k.cpu().numpy().view(np.uint32))
    # idempotence, bit for bit, on the finite frames without a -0.0
    idem = np.ascontiguousarray(F[[0, 1, 2, 3, 4, 5, 6, 0]]).reshape(2, 4, H, W, 1)
    same(match_cdf(dev(idem), dev(idem)), idem)
    same(match_cdf(dev(idem), dev(idem), threshold=THR), idem)


def test_match_cdf_threshold_branches():
    H, W = 37, 53
    F = frames_of(H, W)
    thr = np.float32(THR)
    wet = [(F[f] > thr).sum() for f in range(FINITE)]
    # (x, ref): the reference is wetter (the cap acts), drier (a no-op), and a dry forecast (everything above thr is capped)
    pairs = ((2, 0), (0, 2), (4, 0), (4, 4), (1, 1))
    assert wet[0] > wet[2] > 0 and wet[4] == 0
    x = np.ascontiguousarray(F[[p[0] for p in pairs]]).reshape(1, 5, H, W, 1)
    ref = np.ascontiguousarray(F[[p[1] for p in pairs]]).reshape(1, 5, H, W, 1)
    want, plain = R.match_cdf(x, ref, THR), R.match_cdf(x, ref)
    got = match_cdf(dev(x), dev(ref), threshold=THR)
    same(got, want)
    same(match_cdf(dev(x), dev(ref)), plain)
    got = got.cpu().numpy()
    assert not np.array_equal(want[0, 0], plain[0, 0]) and (got[0, 0] > thr).sum() == wet[2]    # capped down to the forecast's wet area
    assert (got[0, 0] == thr).sum() == wet[0] - wet[2]
    assert np.array_equal(want[0, 1], plain[0, 1])                                              # no-op
    assert (got[0, 2] > thr).sum() == 0 and (got[0, 2] == thr).sum() == wet[0]                  # n_x = 0
    # a threshold given as a Python float is rounded to fp32 once
    same(match_cdf(dev(x), dev(ref), threshold=float(np.float32(THR))), want)


def test_match_cdf_nan_in_a_shared_reference_frame():
    H, W = 5, 7
    F = frames_of(H, W)
    x6 = np.ascontiguousarray(F[[0, 1, 2, 3, 5, 6, 7, 0, 1, 2, 5, 6]]).reshape(3, 2, 2, H, W, 1)       # M = 3, B = 2, T = 2: all finite
    ref1 = np.ascontiguousarray(F[[1, 8]]).reshape(2, 1, H, W, 1)                                       # the second sequence's holds a NaN
    got = match_cdf(dev(x6), dev(ref1), threshold=THR)
    same(got, R.match_cdf(x6, ref1, THR))
    got = got.cpu().numpy()
    assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, 0]).all()                                   # exactly the M T frames that share it


# ------------------------------------------------------------------------------------------------ probability_matched_mean
def ensemble(M, H, W, seed=0):
    """(M, 1, 3, H, W, 1): a continuous frame, a radar frame (ties), and a radar frame with a NaN in member M // 2"""
    rng = np.random.default_rng(seed + M * 7919 + H * 131 + W)
    ens = np.stack([rng.random((M, H, W, 1), dtype=np.float32), radar(rng, (M, H, W, 1), 0.7), radar(rng, (M, H, W, 1), 0.7)], axis=1)
    ens[M // 2, 2, rng.integers(0, H), rng.integers(0, W), 0] = np.nan
    return ens[:, None]


@pytest.mark.parametrize("H,W", ((5, 7), (37, 53), (128, 128)))
@pytest.mark.parametrize("M", (1, 2, 3, 7, 32))
def test_pmm(M, H, W):
    ens = ensemble(M, H, W)
    want = R.probability_matched_mean(ens)
    assert np.isnan(want[0, 2]).all() and np.isfinite(want[0, :2]).all()
    d = dev(ens)
    got = probability_matched_mean(d)
    assert tuple(got.shape) == (1, 3, H, W, 1)
    same(got, want)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), ens.view(np.uint32))
    if M == 1:
        same(got[:, :2], ens[0, :, :2])                                                    # M = 1: the member
    # a frame alone gives the bits it gives in the batch
    same(probability_matched_mean(dev(ens[:, :, 1:2])), want[:, 1:2])


def test_pmm_512_members():
    ens = ensemble(512, 8, 8)
    same(probability_matched_mean(dev(ens)), R.probability_matched_mean(ens))


@pytest.mark.parametrize("H,W", ((5, 7), (37, 53), (128, 128)))
def test_pmm_identities(H, W):
    F = frames_of(H, W)
    one = np.ascontiguousarray(F[[0, 1, 5]]).reshape(1, 3, H, W, 1)
    same(probability_matched_mean(dev(one[None])), one)                                    # one member
    for M in (2, 5):
        same(probability_matched_mean(dev(np.stack([one] * M))), one)                      # identical members
    # k / 256 values: every fp64 sum is exact, so a permutation of the members changes no bit
    rng = np.random.default_rng(H + W)
    ens = (rng.integers(0, 256, (7, 1, 2, H, W, 1)) / 256).astype(np.float32)
    want = R.probability_matched_mean(ens)
    same(probability_matched_mean(dev(ens)), want)
    same(probability_matched_mean(dev(ens[rng.permutation(7)])), want)


# ------------------------------------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("H,W", ((5, 7), (25, 41), (128, 128)))
def test_bindings_write_only_their_outputs(H, W):
    """the three entry points through the bindings into NaN-guarded outputs and a NaN-guarded workspace of exactly the size asked for"""
    F = frames_of(H, W)
    n = H * W
    x = np.ascontiguousarray(F[:FINITE]).reshape(2, 4, H, W, 1)
    ref1 = np.ascontiguousarray(F[[1, 0]]).reshape(2, 1, H, W, 1)
    dx, dref1 = dev(x), dev(ref1)
    srt, order = Guarded((8, n)), Guarded((8, n), torch.int32)
    assert L.pm_ws_bytes(L.PM_RANK, 1, 8, H, W) == 0
    L.rank_frames(dx, 8, H, W, srt.t, order.t)
    torch.cuda.synchronize()
    assert srt.intact() and order.intact()
    want_sorted, want_order = R.rank_frames(x)
    same(srt.t, want_sorted.reshape(8, n))
    same(order.t, want_order.reshape(8, n))

    need = L.pm_ws_bytes(L.PM_CDF, 1, 2, H, W)
    assert need >= 2 * n * 4 + 8 and need % 8 == 0
    (wg, ws), out = ws_of(need), Guarded(x.shape)
    L.cdf_match(dx, dref1, 1, 2, 4, 1, H, W, THR, out.t, ws)
    torch.cuda.synchronize()
    assert wg.intact() and out.intact()
    same(out.t, R.match_cdf(x, ref1, THR))

    ens = x.reshape(4, 1, 2, H, W, 1)
    need = L.pm_ws_bytes(L.PM_PMM, 4, 2, H, W)
    assert need == 2 * ((4 * 2 * n * 4 + 7) // 8 * 8)
    (wg, ws), out = ws_of(need), Guarded((1, 2, H, W, 1))
    L.pmm(dev(ens), 4, 2, H, W, out.t, ws)
    torch.cuda.synchronize()
    assert wg.intact() and out.intact()
    same(out.t, R.probability_matched_mean(ens))


def test_unsupported_shapes_have_no_workspace_size():
    for args in ((L.PM_CDF, 1, 1, 129, 128), (L.PM_PMM, 513, 1, 8, 8), (L.PM_PMM, 0, 1, 8, 8), (L.PM_RANK, 1, 0, 8, 8), (3, 1, 1, 8, 8),
                 (L.PM_PMM, 512, 1 << 20, 128, 128)):
        assert L.pm_ws_bytes(*args) == -1, args


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    H, W = 37, 53
    F = frames_of(H, W)
    x6 = np.ascontiguousarray(F[[0, 1, 2, 3, 5, 6, 7, 0, 1, 2, 5, 6]]).reshape(3, 2, 2, H, W, 1)
    ref1 = np.ascontiguousarray(F[[1, 0]]).reshape(2, 1, H, W, 1)
    other6, other1 = np.ascontiguousarray(x6[::-1]), np.ascontiguousarray(ref1[::-1])

    def run(a, b):
        srt, order = rank_frames(a)
        return srt, order, match_cdf(a, b, threshold=THR), probability_matched_mean(a)

    eager = [[t.clone() for t in run(dev(a), dev(b))] for a, b in ((x6, ref1), (other6, other1))]      # the first call allocates the workspace
    again = run(dev(x6), dev(ref1))
    for t, u in zip(eager[0], again):
        same(t, u.cpu().numpy())
    assert not torch.equal(eager[0][2], eager[1][2])
    held = PM._WS[str(again[0].device)]
    static = [dev(x6), dev(ref1)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(*static)
    assert PM._WS[str(again[0].device)] is held                                                         # a call that fits only launches
    for src, want in (((other6, other1), eager[1]), ((x6, ref1), eager[0])):
        for dst, a in zip(static, src):
            dst.copy_(dev(a))
        graph.replay()
        torch.cuda.synchronize()
        for t, u in zip(outs, want):
            same(t, u.cpu().numpy())


def test_short_workspace_and_aliased_outputs_are_refused_and_nothing_is_written():
    H, W = 25, 41
    F = frames_of(H, W)
    n = H * W
    x = np.ascontiguousarray(F[:FINITE]).reshape(2, 4, H, W, 1)
    dx, dref1 = dev(x), dev(np.ascontiguousarray(F[[1, 0]]).reshape(2, 1, H, W, 1))
    need = L.pm_ws_bytes(L.PM_CDF, 1, 2, H, W)
    (wg, ws), out = ws_of(need), Guarded(x.shape)
    with pytest.raises(PrediffHipError, match=r"status -1\).*workspace"):
        L.cdf_match(dx, dref1, 1, 2, 4, 1, H, W, THR, out.t, ws[:need - 1])                # one byte short
    dens = dev(x.reshape(4, 1, 2, H, W, 1))
    need = L.pm_ws_bytes(L.PM_PMM, 4, 2, H, W)
    (wg2, ws2), out2 = ws_of(need), Guarded((1, 2, H, W, 1))
    with pytest.raises(PrediffHipError, match=r"status -1\).*workspace"):
        L.pmm(dens, 4, 2, H, W, out2.t, ws2[:need - 1])
    torch.cuda.synchronize()
    assert wg.untouched() and out.untouched() and wg2.untouched() and out2.untouched()
    # an output that is an input
    before = dx.clone()
    with pytest.raises(PrediffHipError, match=r"status -1\).*aliases an input"):
        L.cdf_match(dx, dref1, 1, 2, 4, 1, H, W, THR, dx, ws)
    with pytest.raises(PrediffHipError, match=r"status -1\).*aliases an input"):
        L.rank_frames(dx, 8, H, W, dx.view(8, n), torch.empty((8, n), dtype=torch.int32, device="cuda"))
    with pytest.raises(PrediffHipError, match=r"status -1\).*aliases an input"):
        L.pmm(dens, 4, 2, H, W, dens.view(-1)[n:3 * n].view(1, 2, H, W, 1), ws2)
    torch.cuda.synchronize()
    assert torch.equal(dx, before) and wg.untouched() and wg2.untouched()
    for fn in (rank_frames, lambda t: match_cdf(t, t), lambda t: probability_matched_mean(t[None])):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(torch.zeros((1, 1, 4, 4, 1)))


# ------------------------------------------------------------------------------------------------ composition
def test_cdf_matched_steps_forecast():
    """the STEPS composition of the module docstring at 16 x 16: every value above the threshold comes from the last observation"""
    H = W = 16
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    ctx = np.stack([0.9 * np.exp(-((yy - 6 - 0.5 * t) ** 2 + (xx - 5 - t) ** 2) / 8) + 0.5 * np.exp(-((yy - 11) ** 2 + (xx - 10 + 0.5 * t) ** 2) / 5)
                    for t in range(4)]).astype(np.float32)
    ctx = np.where(ctx > 0.03, ctx, 0).astype(np.float32).reshape(1, 4, H, W, 1)
    dctx = dev(ctx)
    se = StochasticExtrapolation(out_len=3, levels=3, match=None)
    g = torch.Generator(device="cuda").manual_seed(11)
    motion = torch.tensor([0.5, 1.0], device="cuda").view(1, 2, 1, 1).expand(1, 2, H, W).contiguous()
    fc = se.forecast(dctx, members=3, generator=g, motion=motion)
    assert tuple(fc.shape) == (3, 1, 3, H, W, 1) and bool(torch.isfinite(fc).all())
    last = dctx[:, -1:].contiguous()
    out = match_cdf(fc, last, threshold=THR)
    same(out, R.match_cdf(fc.cpu().numpy(), ctx[:, -1:], THR))
    out = out.cpu().numpy()
    wet = out > np.float32(THR)
    assert np.isin(out[wet], ctx[:, -1]).all()
    assert (wet.reshape(9, -1).sum(1) <= (fc.cpu().numpy() > np.float32(THR)).reshape(9, -1).sum(1)).all()
