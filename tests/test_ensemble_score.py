"""SEVIREnsembleScore (not in the reference): CRPS, fair CRPS, Brier, ensemble-mean RMSE and spread of M members.  An fp64 numpy oracle
(its identities checked on CPU) vs pd_ensemble_score_update on GPU: integer state exact, float metrics within 1e-5, deterministic bits."""
import numpy as np
import pytest
import torch

THR = (16, 74, 133, 160, 181, 219)
SCALE = np.float32(1.0 / 255.0)


# ------------------------------------------------------------------------------------------------------------------ fp64 oracle
def to_nthwc(x, layout, lead=0):
    """x in `layout` (after `lead` leading axes) -> (..., N, T, H, W, C), missing axes of size 1."""
    for a in "NTHWC":
        if a not in layout:
            x = x[..., None]
            layout = layout + a
    perm = list(range(lead)) + [lead + layout.index(a) for a in "NTHWC"]
    return np.transpose(x, perm)


def preprocess(x, s):
    """(..., N, T, H, W, C): fp32 / fp32(1/255), then max-pool over (H, W) with kernel = stride = s (floor mode, NaN propagating)."""
    x = x.astype(np.float32) / SCALE
    if s == 1:
        return x
    *lead, N, T, H, W, C = x.shape
    Ho, Wo = H // s, W // s
    x = x[..., :Ho * s, :Wo * s, :].reshape(*lead, N, T, Ho, s, Wo, s, C)
    return x.max(axis=(-4, -2))


def pairwise_sum(x):
    """sum_ij |x_i - x_j| over axis 0, directly (M^2 terms)."""
    return np.abs(x[:, None] - x[None, :]).sum(axis=(0, 1))


def sorted_pairwise_sum(x):
    """The same from the sorted members: sum_ij |x_i - x_j| = 2 sum_k (2k - M + 1) x_(k)."""
    M = x.shape[0]
    w = (2.0 * np.arange(M) - M + 1).reshape((M,) + (1,) * (x.ndim - 1))
    return 2.0 * (np.sort(x, axis=0) * w).sum(axis=0)


def oracle_state(ens, target, layout, s=1, keep_seq=True, thresholds=THR):
    """n_valid [T'], brier int64 [thr, T'], fp64 sums [4, T'] as the kernel accumulates them."""
    x = preprocess(to_nthwc(ens, layout, 1), s).astype(np.float64)          # (M, N, T, h, w, C)
    y = preprocess(to_nthwc(target, layout), s).astype(np.float64)           # (N, T, h, w, C)
    M = x.shape[0]
    valid = ~np.isnan(y) & ~np.isnan(x).any(axis=0)
    x = np.where(valid[None], x, 0.0)
    y = np.where(valid, y, 0.0)
    m = x.mean(axis=0)
    per = [np.abs(x - y[None]).sum(axis=0), sorted_pairwise_sum(x), (m - y) ** 2,
           ((x - m[None]) ** 2).sum(axis=0) / (M - 1) if M > 1 else np.zeros_like(m)]
    axes = (0, 2, 3, 4) if keep_seq else (0, 1, 2, 3, 4)
    sums = np.stack([np.where(valid, v, 0.0).sum(axis=axes) for v in per]).reshape(4, -1)
    n_valid = valid.sum(axis=axes).astype(np.int64).reshape(-1)
    brier = []
    for thr in thresholds:
        c = (x >= thr).sum(axis=0).astype(np.int64)
        o = (y >= thr).astype(np.int64)
        brier.append(np.where(valid, (c - M * o) ** 2, 0).sum(axis=axes).reshape(-1))
    return n_valid, np.asarray(brier, dtype=np.int64), sums, M


def oracle_scores(n_valid, brier, sums, M, mode):
    n = n_valid.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        per = {"crps": (sums[0] / M - sums[1] / (2.0 * M * M)) / n,
               "crps_fair": (sums[0] / M - sums[1] / (2.0 * M * (M - 1))) / n if M > 1 else np.full(n.shape, np.nan),
               "rmse": np.sqrt(sums[2] / n),
               "spread": np.sqrt(sums[3] / n) if M > 1 else np.full(n.shape, np.nan)}
        bs = brier / (float(M) * M * n)
    fin = (lambda v: v[0]) if mode == "0" else ((lambda v: v) if mode == "1" else (lambda v: np.mean(v)))
    ret = {k: fin(v) for k, v in per.items()}
    ret["brier"] = [fin(b) for b in bs]
    ret["brier_avg"] = fin(bs.mean(axis=0))
    return ret


def make_case(M, layout, seed, N=2, T=6, H=32, W=32, nan=True):
    """Members around a VIL-like target in `layout` (4- or 5-letter), exact k/255 values and NaNs in members and target."""
    g = np.random.default_rng(seed)
    tgt = (g.integers(0, 256, (N, T, H, W, 1)) / 255.0).astype(np.float32) * (g.random((N, T, H, W, 1)) > 0.4)
    ens = np.clip(tgt[None] + 0.15 * g.standard_normal((M, N, T, H, W, 1)), 0, 1).astype(np.float32)
    ens[:, :, :, :4] = (np.round(ens[:, :, :, :4] * 255) / 255).astype(np.float32)            # exact threshold values
    if nan:
        ens[M - 1, 0, 1, 5, 7, 0] = np.nan
        tgt[N - 1, 2, 9, 20, 0] = np.nan
    nthwc = "NTHWC"
    if len(layout) == 4:
        ens, tgt, nthwc = ens[..., 0], tgt[..., 0], "NTHW"
    perm = [nthwc.index(a) for a in layout]
    return np.ascontiguousarray(np.transpose(ens, [0] + [p + 1 for p in perm])), np.ascontiguousarray(np.transpose(tgt, perm))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_oracle_identities():
    g = np.random.default_rng(0)
    x = g.random((7, 5, 3)) * 255
    assert np.allclose(pairwise_sum(x), sorted_pairwise_sum(x), rtol=1e-12)
    # M = 1: CRPS is the absolute error, RMSE of the single member
    ens, tgt = make_case(1, "NTHWC", 1, nan=False)
    n, b, s, M = oracle_state(ens, tgt, "NTHWC", keep_seq=False)
    sc = oracle_scores(n, b, s, M, "0")
    xv, yv = (ens[0] / SCALE).astype(np.float64), (tgt / SCALE).astype(np.float64)
    mae = np.abs(xv - yv).mean()
    assert np.isclose(sc["crps"], mae, rtol=1e-12) and np.isnan(sc["crps_fair"]) and np.isnan(sc["spread"])
    # a deterministic ensemble (M identical members): Brier = misclassified fraction, CRPS = MAE, spread 0
    ens4 = np.repeat(ens, 4, axis=0)
    n, b, s, M = oracle_state(ens4, tgt, "NTHWC", keep_seq=False)
    sc4 = oracle_scores(n, b, s, M, "0")
    for i, thr in enumerate(THR):
        assert np.isclose(sc4["brier"][i], np.mean((xv >= thr) != (yv >= thr)), rtol=1e-12)
    assert np.isclose(sc4["crps"], mae, rtol=1e-12) and sc4["spread"] == 0.0
    # a NaN in one member or in the target removes that pixel (before pooling: its whole window); fair CRPS <= CRPS
    ens, tgt = make_case(5, "NHWT", 2)
    n, b, s, M = oracle_state(ens, tgt, "NHWT", s=1)
    assert n.shape == (6,) and b.shape == (6, 6) and list(n) == [2048, 2047, 2047, 2048, 2048, 2048]
    n4, _, _, _ = oracle_state(ens, tgt, "NHWT", s=4)
    assert list(n4) == [128, 127, 127, 128, 128, 128]
    sc = oracle_scores(n, b, s, M, "1")
    assert np.all(sc["crps_fair"] <= sc["crps"])


def test_constructor_validation():
    from prediff_amd.ensemble_score import SEVIREnsembleScore
    m = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=6, preprocess_type="sevir_pool4")
    assert m.pool_scale == 4 and m.metrics_list == ("crps", "crps_fair", "brier", "rmse", "spread")
    assert SEVIREnsembleScore().layout == "NHWT"          # SEVIRSkillScore's defaults
    with pytest.raises(ValueError):
        SEVIREnsembleScore(layout="NHWT", preprocess_type="sevir_pool4")
    with pytest.raises(ValueError):
        SEVIREnsembleScore(layout="NTHWC", metrics_list=("crps", "csi"))
    with pytest.raises(ValueError):
        SEVIREnsembleScore(layout="NTHWX")
    with pytest.raises(NotImplementedError):
        SEVIREnsembleScore(layout="NTHWC", mode="3")
    with pytest.raises(NotImplementedError):
        SEVIREnsembleScore(layout="NTHWC", preprocess_type="other")
    with pytest.raises(AssertionError):
        SEVIREnsembleScore(layout="NTHWC", mode="1")          # seq_len required
    ret = SEVIREnsembleScore(layout="NTHWC").compute()          # nothing accumulated: NaN, not an exception
    assert np.isnan(ret["crps"]) and np.isnan(ret["avg"]["brier"])
    # the member count is checked before anything touches a device
    with pytest.raises(ValueError):
        m.update(torch.zeros(513, 1, 6, 8, 8, 1), torch.zeros(1, 6, 8, 8, 1))
    with pytest.raises(ValueError):
        m.update(torch.zeros(2, 1, 6, 8, 8, 1), torch.zeros(1, 6, 8, 9, 1))


def _free_port():
    import socket
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    return port


def _sync_worker(rank, world, port, q, done):
    """Rank 0 holds state (as after its updates), rank 1 made none; both call sync().  Then both hold state with different M."""
    import os
    import torch.distributed as dist
    from prediff_amd.ensemble_score import SEVIREnsembleScore
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        es = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=6, threshold_list=(16, 74))
        if rank == 0:
            es._alloc_state("cpu")
            es.n_valid += torch.arange(1, 7)
            es.brier_sums += torch.arange(12).view(2, 6)
            es.sums += torch.linspace(1.0, 2.0, 24, dtype=torch.float64).view(4, 6)
            es.num_members = 4
        es.sync()
        first = (es.num_members, es.n_valid.clone(), es.brier_sums.clone(), es.sums.clone(), es.compute()["crps"])
        es2 = SEVIREnsembleScore(layout="NTHWC", mode="0")
        es2._alloc_state("cpu")
        es2.num_members = 4 + rank
        try:
            es2.sync()
            second = None
        except ValueError as err:
            second = str(err)
        q.put((rank, first, second))
        done.wait(120)        # the tensors travel as shared-memory fds that this process serves: stay until they are received
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sync_with_state_on_one_rank():
    """sync() is a collective on every rank: a rank that made no update takes part with a zero state and learns M."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q, done = ctx.Queue(), ctx.Event()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q, done)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (a, b)) for r, a, b in (q.get(timeout=120) for _ in range(2)))
    done.set()
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (m0, n0, b0, s0, c0), e0 = got[0]
    (m1, n1, b1, s1, c1), e1 = got[1]
    assert m0 == m1 == 4
    assert torch.equal(n0, torch.arange(1, 7)) and torch.equal(n1, n0) and torch.equal(b1, b0) and torch.equal(s1, s0)
    assert np.array_equal(c0, c1)
    assert e0 is not None and e1 is not None and "member counts" in e0


# ------------------------------------------------------------------------------------------------------------------ GPU
def _state(m):
    return m.n_valid.cpu().numpy(), m.brier_sums.cpu().numpy(), m.sums.cpu().numpy()


def _check(m, ens, tgt, layout, s, mode):
    n, b, sums, M = oracle_state(ens, tgt, layout, s, keep_seq=mode != "0")
    gn, gb, gs = _state(m)
    assert np.array_equal(gn, n) and np.array_equal(gb, b), (M, layout, s, mode)              # exact
    assert np.allclose(gs, sums, rtol=1e-5, atol=1e-6), (M, layout, s, mode)
    want, got = oracle_scores(n, b, sums, M, mode), m.compute()
    for k in ("crps", "crps_fair", "rmse", "spread"):
        assert np.allclose(np.asarray(got[k], dtype=np.float64), want[k], rtol=1e-5, equal_nan=True), (k, M, layout, s, mode)
    for i, thr in enumerate(THR):
        assert np.allclose(np.asarray(got[thr]["brier"], dtype=np.float64), want["brier"][i], rtol=1e-12), (thr, M, mode)
    assert np.allclose(np.asarray(got["avg"]["brier"], dtype=np.float64), want["brier_avg"], rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 5, 64, 512])
@pytest.mark.parametrize("layout,pre", [("NTHWC", "sevir"), ("NTHWC", "sevir_pool4"), ("NTHWC", "sevir_pool3"), ("NHWT", "sevir")])
def test_hip_ensemble_score_matches_oracle(M, layout, pre):
    """sevir_pool3: 3 does not divide the 32 x 32 frame (trailing rows / columns dropped) and a window spans a partial lane group."""
    from prediff_amd.ensemble_score import SEVIREnsembleScore
    s = {"sevir": 1, "sevir_pool4": 4, "sevir_pool3": 3}[pre]
    ens, tgt = make_case(M, layout, 10 + M, N=1 if M == 512 else 2)
    e, t = torch.from_numpy(ens).cuda(), torch.from_numpy(tgt).cuda()
    for mode in ("0", "1", "2"):
        m = SEVIREnsembleScore(layout=layout, mode=mode, seq_len=6, preprocess_type=pre, threshold_list=THR)
        m.update(e, t)
        _check(m, ens, tgt, layout, s, mode)
        if mode == "1":
            m2 = SEVIREnsembleScore(layout=layout, mode=mode, seq_len=6, preprocess_type=pre, threshold_list=THR)
            m2.update(e, t)
            for a, b in zip(_state(m), _state(m2)):                                             # same inputs, same bits
                assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("pre", ["sevir", "sevir_pool4"])
def test_hip_ensemble_score_two_updates_equal_one(pre):
    from prediff_amd import _lib as L
    from prediff_amd.ensemble_score import SEVIREnsembleScore
    s = 4 if pre == "sevir_pool4" else 1
    ens, tgt = make_case(16, "NTHWC", 7, N=3)
    e, t = torch.from_numpy(ens).cuda(), torch.from_numpy(tgt).cuda()
    if s == 1:
        # the kernel's tile (pixels per block, hence threads per pixel) differs between the three launches: workspace per slab
        per_slab = [L.ensemble_score_ws_doubles(16, [n, 6, 32, 32, 1], 1) // (6 * n) for n in (1, 2, 3)]
        assert len(set(per_slab)) == 3, per_slab
    one = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=6, preprocess_type=pre)
    one.update(e, t)
    two = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=6, preprocess_type=pre)
    two.update(e[:, :1], t[:1])
    two.update(e[:, 1:], t[1:])                 # strided view of the members: read in place
    a, b = _state(one), _state(two)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.allclose(a[2], b[2], rtol=1e-12, atol=0)
    _check(two, ens, tgt, "NTHWC", s, "1")
    with pytest.raises(ValueError):
        two.update(e[:8], t)                    # another member count without reset()
    two.reset()
    two.update(e[:8], t)
    assert two.num_members == 8


@pytest.mark.gpu
def test_hip_ensemble_score_full_size():
    """One context of a 64-member ensemble at SEVIR-LR size (64 x 1 x 6 x 128 x 128 x 1), as sample_ensemble returns it, pools 1 and 16."""
    from prediff_amd.ensemble_score import SEVIREnsembleScore
    ens, tgt = make_case(64, "NTHWC", 5, N=1, H=128, W=128)
    e, t = torch.from_numpy(ens[:, 0]).cuda(), torch.from_numpy(tgt).cuda()     # (M, T, H, W, C): a sample_ensemble result
    for pre, s in (("sevir", 1), ("sevir_pool16", 16)):
        m = SEVIREnsembleScore(layout="NTHWC", mode="2", seq_len=6, preprocess_type=pre)
        m.update(e.unsqueeze(1), t)
        _check(m, ens, tgt, "NTHWC", s, "2")


@pytest.mark.gpu
def test_evaluate_context_updates_ensemble_score():
    from prediff_amd import config as CFG
    from prediff_amd.ensemble_score import SEVIREnsembleScore
    g = torch.Generator().manual_seed(4)
    B, K = 2, 3
    seq = torch.rand((B, 7 + 6, 16, 16, 1), generator=g).cuda()
    samples = [torch.rand((B, 6, 16, 16, 1), generator=g).cuda() for _ in range(K)]

    class StubLDM:
        alignment_fn = None

        def __init__(self):
            self.calls = 0

        def sample(self, cond, batch_size, **kw):
            out = samples[self.calls % K]
            self.calls += 1
            return out

    cfg = {"layout": {"in_len": 7, "out_len": 6}, "eval": {"num_samples_per_context": K, "eval_unaligned": True}}
    es = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=6)
    out = CFG.evaluate_context(StubLDM(), seq, cfg, ensemble_score=es)
    assert len(out["pred"]) == K and es.num_members == K
    ens = torch.stack(samples).cpu().numpy()
    _check(es, ens, seq[:, 7:].cpu().numpy(), "NTHWC", 1, "1")
    # without an ensemble score nothing changes
    assert len(CFG.evaluate_context(StubLDM(), seq, cfg)["pred"]) == K
