"""prediff_amd.scale_score without a GPU: the constructor and argument refusals, compute() on hand-written states, the agreement of the
ranks on the padded side, and the properties of tests/_scale_ref.py, the restatement that tests/test_scale_score.py holds the device to."""
import os
import socket

import numpy as np
import pytest
import torch

import _scale_ref as R
from prediff_amd import SEVIRScaleScore, scale_energy
from prediff_amd._lib import PrediffHipError
from prediff_amd.scale_score import METRICS, component_means, top_level

NAN = np.nan


def disc(H, W, cy, cx, radius):
    r, c = np.mgrid[0:H, 0:W]
    return ((r - cy) ** 2 + (c - cx) ** 2 <= radius ** 2).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the class
def test_constructor_refusals():
    for layout in ("NTHWX", "NTHHW", "THWC", "NTWC", "NTHC", "NT"):
        with pytest.raises(ValueError):
            SEVIRScaleScore(layout=layout)
    with pytest.raises(NotImplementedError):
        SEVIRScaleScore(mode="3")
    for mode in ("1", "2"):
        with pytest.raises(ValueError):
            SEVIRScaleScore(mode=mode)
    with pytest.raises(ValueError):
        SEVIRScaleScore(metrics_list=("iss", "csi"))
    with pytest.raises(ValueError):
        SEVIRScaleScore(threshold_list=())
    with pytest.raises(ValueError):
        SEVIRScaleScore(threshold_list=tuple(range(10, 100, 10)))             # nine
    m = SEVIRScaleScore(layout="NHWT", mode="1", seq_len=6, threshold_list=(16, 74), metrics_list=("iss",))
    assert m.keep_seq_len_dim and m.Tk == 6 and m.threshold_list == (16.0, 74.0) and m.metrics_list == ("iss",) and m.levels is None
    d = SEVIRScaleScore()
    assert d.threshold_list == (16.0, 74.0, 133.0, 160.0, 181.0, 219.0) and d.mode == "0" and d.layout == "NTHWC" and d.seq_len is None
    assert SEVIRScaleScore.METRICS == METRICS == R.METRICS and d.metrics_list == METRICS
    assert len(SEVIRScaleScore(threshold_list=range(8)).threshold_list) == 8
    assert [(n, dt) for n, dt, _ in SEVIRScaleScore.STATE] == [("energy", torch.int64), ("counts", torch.int64)]
    assert [shape(m, 6) for _, _, shape in SEVIRScaleScore.STATE] == [(3, 2, 8, 6), (2, 6)]
    assert [top_level(*s) for s in ((1, 1), (2, 2), (3, 2), (4, 4), (5, 1), (64, 64), (65, 3), (128, 128))] == [1, 1, 2, 2, 3, 6, 7, 7]
    assert all(top_level(h, w) == R.top_level(h, w) for h in range(1, 129) for w in (1, 2, 3, 64, 65, 128))


def test_cpu_tensors_and_shapes_are_refused():
    x = torch.rand((1, 2, 8, 8, 1))
    with pytest.raises(PrediffHipError):
        scale_energy(x, 16)
    with pytest.raises(PrediffHipError):
        SEVIRScaleScore().update(x, x)
    with pytest.raises(PrediffHipError):
        SEVIRScaleScore().update_members(x[None], x)
    with pytest.raises(ValueError):
        SEVIRScaleScore().update(x, x[:, :1])
    with pytest.raises(ValueError):
        SEVIRScaleScore().update_members(x, x)                                # not (M,) + target.shape
    with pytest.raises(ValueError):
        scale_energy(x, 16, layout="NTC")
    with pytest.raises(ValueError):
        scale_energy(x, 16, layout="NTHW")                                    # one letter per axis
    SEVIRScaleScore().sync()                                                  # no process group: a no-op


def hand_state():
    """2 x 2 frames (n = 1, N = 4, L = 2), K = 2, T = 3, written out by hand.
    step 0, one pair.   k = 0: F = [[1, 0], [0, 0]], O = [[0, 1], [0, 0]]: Q(F) = Q(O) = (1, 1), Z = [[1, -1], [0, 0]]: Q(Z) = (2, 0).
                        k = 1: F = [[1, 1], [0, 0]]: Q(F) = (2, 4), O = [[1, 0], [0, 0]]: Q(O) = (1, 1), Z = [[0, 1], [0, 0]]: Q(Z) = (1, 1).
    step 1, two pairs.  k = 0: no events at all;  k = 1: the pair of step 0 twice.
    step 2: one skipped pair, none scored."""
    e = np.zeros((3, 2, 8, 3), np.int64)
    c = np.array([[1, 2, 0], [0, 0, 1]], np.int64)
    e[:, 0, :2, 0] = [[1, 1], [1, 1], [2, 0]]
    e[:, 1, :2, 0] = [[2, 4], [1, 1], [1, 1]]
    e[:, 1, :2, 1] = [[4, 8], [2, 2], [2, 2]]
    return e, c


def test_compute_on_a_hand_written_state():
    e, c = hand_state()
    m1 = SEVIRScaleScore(mode="1", seq_len=3, threshold_list=(16, 74))
    m1.energy, m1.counts, m1._n = torch.from_numpy(e), torch.from_numpy(c), 1
    assert m1.levels == 2
    r = m1.compute()
    assert set(r) == set(METRICS)
    assert all(r[k].shape == (3, 2, 2) for k in ("mse", "iss", "energy_pred", "energy_target", "energy_bias"))
    assert all(r[k].shape == (3, 2) for k in ("mse_random", "base_rate", "freq_bias"))
    k1 = {"mse": [0.1875, 0.0625], "iss": [0.25, 0.75], "energy_pred": [0.25, 0.25], "energy_target": [0.1875, 0.0625],
          "energy_bias": [0.0625 / 0.4375, 0.1875 / 0.3125]}
    want = {"mse": [[[0.5, 0.0], k1["mse"]], [[0.0, 0.0], k1["mse"]], [[NAN, NAN]] * 2],
            "mse_random": [[0.375, 0.5], [0.0, 0.5], [NAN, NAN]],
            "iss": [[[1.0 - 2 * 0.5 / 0.375, 1.0], k1["iss"]], [[NAN, NAN], k1["iss"]], [[NAN, NAN]] * 2],
            "energy_pred": [[[0.1875, 0.0625], k1["energy_pred"]], [[0.0, 0.0], k1["energy_pred"]], [[NAN, NAN]] * 2],
            "energy_target": [[[0.1875, 0.0625], k1["energy_target"]], [[0.0, 0.0], k1["energy_target"]], [[NAN, NAN]] * 2],
            "energy_bias": [[[0.0, 0.0], k1["energy_bias"]], [[NAN, NAN], k1["energy_bias"]], [[NAN, NAN]] * 2],
            "base_rate": [[0.25, 0.25], [0.0, 0.25], [NAN, NAN]],
            "freq_bias": [[1.0, 2.0], [NAN, 2.0], [NAN, NAN]]}
    for k, v in want.items():
        assert np.array_equal(r[k], np.array(v), equal_nan=True), (k, r[k])
    for k, v in R.compute(e, c, 1, "1").items():
        assert np.array_equal(v, r[k], equal_nan=True), k
    # mode "2": the mean over the lead times (NaN wherever one of them is)
    m2 = SEVIRScaleScore(mode="2", seq_len=3, threshold_list=(16, 74), metrics_list=("mse", "base_rate"))
    m2.energy, m2.counts, m2._n = torch.from_numpy(e[..., :2].copy()), torch.from_numpy(c[:, :2].copy()), 1
    m2.seq_len = 2
    r2 = m2.compute()
    assert list(r2) == ["mse", "base_rate"] and np.array_equal(r2["mse"], [[0.25, 0.0], k1["mse"]]) and np.array_equal(r2["base_rate"], [0.125, 0.25])
    # mode "0": one pooled step; the three pairs of k = 1 pool to the same values, k = 0 to 3 pairs with the events of one
    m0 = SEVIRScaleScore(mode="0", threshold_list=(16, 74))
    m0.energy, m0.counts, m0._n = torch.from_numpy(e.sum(axis=3, keepdims=True)), torch.from_numpy(c.sum(axis=1, keepdims=True)), 1
    r0 = m0.compute()
    assert r0["mse"].shape == (2, 2) and r0["mse_random"].shape == (2,)
    assert np.array_equal(r0["mse"][1], k1["mse"]) and np.array_equal(r0["iss"][1], k1["iss"]) and r0["freq_bias"].tolist() == [1.0, 2.0]
    assert np.array_equal(r0["mse"][0], [8.0 / 48.0, 0.0]) and r0["base_rate"].tolist() == [1.0 / 12.0, 0.25]
    assert np.array_equal(r0["mse_random"], [2 * (1.0 / 12.0) * (1.0 - 1.0 / 12.0), 0.5])


def test_compute_before_any_update_is_nan_with_an_empty_level_axis():
    e0 = SEVIRScaleScore().compute()
    e1 = SEVIRScaleScore(mode="1", seq_len=4, threshold_list=(16, 74, 133)).compute()
    e2 = SEVIRScaleScore(mode="2", seq_len=4, threshold_list=(16,)).compute()
    assert set(e0) == set(e1) == set(e2) == set(METRICS)
    for met in ("mse_random", "base_rate", "freq_bias"):
        assert e0[met].shape == (6,) and e1[met].shape == (4, 3) and e2[met].shape == (1,)
        assert np.isnan(e0[met]).all() and np.isnan(e1[met]).all() and np.isnan(e2[met]).all()
    for met in ("mse", "iss", "energy_pred", "energy_target", "energy_bias"):
        assert e0[met].shape == (6, 0) and e1[met].shape == (4, 3, 0) and e2[met].shape == (1, 0)
    m = SEVIRScaleScore()
    m.reset()
    assert m.energy is None and m.counts is None and m.levels is None
    # a state with a level but no scored pair: NaN everywhere
    m.energy, m.counts, m._n = torch.zeros((3, 6, 8, 1), dtype=torch.int64), torch.tensor([[0], [2]]), 3
    r = m.compute()
    assert r["iss"].shape == (6, 4) and all(np.isnan(v).all() for v in r.values())


# ------------------------------------------------------------------------------------------------ sync
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
        e, c = hand_state()
        m = SEVIRScaleScore(mode="1", seq_len=3, threshold_list=(16, 74))
        if rank == 0:                                   # rank 1 made no update: a zero state, and it takes rank 0's n
            m.energy, m.counts, m._n = torch.from_numpy(e), torch.from_numpy(c), 1
        m.sync()
        bad = SEVIRScaleScore(mode="1", seq_len=3, threshold_list=(16, 74))
        bad.energy, bad.counts, bad._n = torch.from_numpy(e.copy()), torch.from_numpy(c.copy()), 1 + rank
        try:
            bad.sync()
            raised = False
        except ValueError:
            raised = True
        q.put((rank, m.energy.tolist(), m.counts.tolist(), m.levels, m.compute()["iss"].tolist(), raised))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sync_world2_gloo_agrees_on_the_padded_side():
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
    e, c = hand_state()
    iss = R.compute(e, c, 1, "1")["iss"]
    for r in range(2):
        assert got[r][0] == e.tolist() and got[r][1] == c.tolist() and got[r][2] == 2 and got[r][4], (r, got[r])
        assert np.array_equal(np.array(got[r][3]), iss, equal_nan=True)


# ------------------------------------------------------------------------------------------------ evaluate_context
class _StubSampler:
    """What evaluate_context asks of a latent-diffusion model: alignment_fn and sample()."""
    alignment_fn = staticmethod(lambda *a, **k: None)

    def __init__(self, shape):
        self.shape, self.calls = shape, []

    def sample(self, cond, batch_size, use_alignment=False, **kwargs):
        self.calls.append(use_alignment)
        return torch.full(self.shape, float(len(self.calls)))


class _StubScore:
    def __init__(self):
        self.seen = []

    def update(self, pred, target):
        self.seen.append((float(pred.flatten()[0]), pred.dtype, tuple(pred.shape), tuple(target.shape)))


def test_evaluate_context_updates_the_scale_scores_once_per_sample():
    from prediff_amd import config as CFG
    B, T_in, T_out, S = 2, 3, 2, 3
    seq = torch.rand((B, T_in + T_out, 8, 8, 1))
    cfg = {"layout": {"in_len": T_in, "out_len": T_out}, "eval": {"num_samples_per_context": S}}
    shape = (B, T_out, 8, 8, 1)
    ldm, ss, ass, ds, ads = _StubSampler(shape), _StubScore(), _StubScore(), _StubScore(), _StubScore()
    out = CFG.evaluate_context(ldm, seq, cfg, scale_score=ss, aligned_scale_score=ass, distance_score=ds, aligned_distance_score=ads)
    assert ldm.calls == [True, False] * S and len(out["pred"]) == len(out["aligned_pred"]) == S
    # the aligned sample of round i is call 2 i + 1, the plain one call 2 i + 2; each score sees its own, once, where the distance one does
    assert [s[0] for s in ass.seen] == [1.0, 3.0, 5.0] and [s[0] for s in ss.seen] == [2.0, 4.0, 6.0]
    assert ss.seen == ds.seen and ass.seen == ads.seen and all(s[1:] == (torch.float32, shape, shape) for s in ss.seen + ass.seen)
    # without the keywords nothing else changes; one of the two alone is updated alone
    ldm2, only = _StubSampler(shape), _StubScore()
    out2 = CFG.evaluate_context(ldm2, seq, cfg, scale_score=only)
    assert ldm2.calls == ldm.calls and [s[0] for s in only.seen] == [2.0, 4.0, 6.0]
    assert all(torch.equal(a, b) for k in out for a, b in zip(out[k], out2[k]))


# ------------------------------------------------------------------------------------------------ the restatement
SHAPES = [(1, 1), (2, 2), (3, 5), (4, 4), (8, 8), (9, 1), (33, 40), (64, 64), (63, 65), (128, 3), (128, 128)]


def fields_of(H, W, seed):
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:H, 0:W]
    return [np.zeros((H, W), np.int64), np.ones((H, W), np.int64), ((r + c) % 2 == 0).astype(np.int64),
            (rng.random((H, W)) < 0.3).astype(np.int64), (rng.random((H, W)) < 0.5).astype(np.int64) - (rng.random((H, W)) < 0.5)]


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_integer_form_equals_the_explicit_decomposition(shape):
    H, W = shape
    n = R.top_level(H, W)
    for a in fields_of(H, W, 7 * H + W):
        q = R.q_levels(a)
        assert q.shape == (n + 1,) and q[0] == (a ** 2).sum() and q[n] == a.sum() ** 2 and R.parseval_holds(q, n)
        got, want = R.component_means(q, n, np.int64(4 ** n)), R.explicit_components(a)
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (shape, got, want)
        assert abs(got.sum() - (a ** 2).sum() / 4.0 ** n) <= 1e-12 * got.sum()                   # the components' energies sum to the field's
        assert np.array_equal(got, component_means(q, n, np.int64(4 ** n)))                      # the package's own helper


def test_reference_event_sets_and_padding():
    d = np.float32(1.0 / 255.0)
    v = np.float32(16.0) * d
    while v / d >= np.float32(16.0):                          # the smallest fp32 whose quotient reaches 16
        v = np.nextafter(v, np.float32(0.0))
    below, on = v, np.nextafter(v, np.float32(1.0))
    f = np.array([[below, on, np.nan, np.inf, -np.inf, 0.0]], np.float32)
    assert R.event_mask(f, 16).tolist() == [[False, True, False, True, False, False]]
    assert R.scale_energy(f, 16).tolist() == [2, 2, 4, 4]     # 1 x 6 pads to 8 x 8: two single events in two 2-blocks of one 4-block
    assert R.pad(np.ones((3, 5))).shape == (8, 8) and R.pad(np.ones((3, 5))).sum() == 15 and R.pad(np.ones((1, 1))).shape == (2, 2)
    assert R.q_levels(np.ones((128, 128), np.int64)).tolist() == [4 ** (7 + l) for l in range(8)]


def test_reference_identity_swap_and_shift():
    rng = np.random.default_rng(3)
    a = (rng.random((1, 2, 3, 33, 40)) ** 3).astype(np.float32)
    b = (rng.random((2, 3, 33, 40)) ** 3).astype(np.float32)
    thr = (16, 74, 133)
    e, c = R.scale_state(b[None], b, thr, True)
    assert (e[2] == 0).all() and np.array_equal(e[0], e[1]) and c.tolist() == [[2, 2, 2], [0, 0, 0]] and (e[:, :, 7:] == 0).all()
    r = R.compute(e, c, 6, "1")
    assert (r["mse"] == 0).all() and (r["mse_random"] > 0).all() and (r["iss"] == 1).all() and (r["energy_bias"] == 0).all()
    ab, ba = R.scale_state(a, b, thr, False), R.scale_state(b[None], a[0], thr, False)
    assert np.array_equal(ab[0][0], ba[0][1]) and np.array_equal(ab[0][1], ba[0][0]) and np.array_equal(ab[0][2], ba[0][2])
    assert (ab[0][2, :, 0] > 0).all() and np.array_equal(ab[1], ba[1])
    # a cyclic shift of a dyadic frame by a multiple of 2^l leaves Q_j, j <= l, unchanged
    m = (rng.random((64, 64)) < 0.2).astype(np.int64)
    q = R.q_levels(m)
    for l in range(7):
        for dy, dx in ((2 ** l, 0), (0, 3 * 2 ** l), (5 * 2 ** l, 2 ** l)):
            assert np.array_equal(R.q_levels(np.roll(m, (dy, dx), axis=(0, 1)))[:l + 1], q[:l + 1]), (l, dy, dx)
    assert not np.array_equal(R.q_levels(np.roll(m, 1, axis=1))[1:6], q[1:6])
    # a non-finite pixel in either frame skips the pair
    bad = b.copy()
    bad[1, 2, 0, 0] = np.inf
    e2, c2 = R.scale_state(a, bad, thr, True)
    assert c2.tolist() == [[2, 2, 1], [0, 0, 1]]


def test_reference_displaced_disc_loses_skill_at_the_scale_of_the_displacement():
    """A disc of radius 10 displaced by 8 pixels in a 128 x 128 frame: the smallest iss falls on component 4 (scale 8 px), and the
    components 6 .. 8 stay above 0.98 (measured: 0.556 0.394 0.614 -0.700 0.187 0.987 1.000 1.000).  The disc is centred on a corner of
    the 16-pixel grid, (80, 80), and moves to (80, 88); the values of the components 3 .. 5 depend on that alignment."""
    o, f = disc(128, 128, 80, 80, 10), disc(128, 128, 80, 88, 10)
    e, c = R.scale_state(f[None, None, None], o[None, None], (74,), False)
    iss = R.compute(e, c, 7, "0")["iss"][0]
    print("iss of the displaced disc:", " ".join(f"{v:.2f}" for v in iss))
    assert iss.shape == (8,) and int(np.argmin(iss)) == 3 and iss[3] < 0 and (iss[5:] > 0.98).all()
