"""SEVIRSkillScore with preprocess_type "sevir_pool{s}" (reference evaluation.py:220-231, the CSI-pool4 / CSI-pool16 scores): a numpy
oracle vs the reference golden on CPU (integer counts: bit exact), pd_sevir_skill_counts_pooled vs both on GPU, in place in any 5-letter
layout."""
import numpy as np
import pytest
import torch

from _inputs import skill_inputs
from oracle import skill as OS

THR = (16, 74, 133, 160, 181, 219)
POOLS = (4, 16, 3)
MODES = ("0", "1", "2")


def pool_np(x, s):
    """(N, T, H, W, C) fp32 / fp32(1/255), then F.max_pool2d over (H, W), kernel = stride = s, floor mode, NaN propagating."""
    x = x.astype(np.float32) / np.float32(1.0 / 255.0)
    N, T, H, W, C = x.shape
    Ho, Wo = H // s, W // s
    x = x[:, :, :Ho * s, :Wo * s].reshape(N, T, Ho, s, Wo, s, C)
    return x.max(axis=(3, 5))                                          # np.max propagates NaN


def pooled_counts(pred, target, s, keep_seq):
    """hits / misses / false alarms of the pooled frames (N T H W C), (thr, T) if keep_seq else (thr,)."""
    p, t = pool_np(pred, s), pool_np(target, s)
    nan = np.isnan(p) | np.isnan(t)
    axes = (0, 2, 3, 4) if keep_seq else (0, 1, 2, 3, 4)
    out = []
    for T in THR:
        tb, pb = (t >= T) & ~nan, (p >= T) & ~nan
        out.append([np.sum(tb & pb, axis=axes), np.sum(tb & ~pb, axis=axes), np.sum(~tb & pb, axis=axes)])
    out = np.asarray(out, dtype=np.int64)
    return out[:, 0], out[:, 1], out[:, 2]


def golden_counts(g, s, mode):
    return [g[f"p{s}_{name}_{mode}"].astype(np.int64) for name in ("hits", "misses", "fas")]


@pytest.mark.parametrize("s", POOLS)
def test_pooled_oracle_matches_reference(golden, s):
    g = golden("skill_score_pool")
    pred, target = skill_inputs()
    for mode in MODES:
        keep = mode != "0"
        a = pooled_counts(pred.numpy(), target.numpy(), s, keep)
        b = pooled_counts(pred.flip(0).numpy(), target.numpy(), s, keep)
        tot = [x + y for x, y in zip(a, b)]
        for got, want in zip(tot, golden_counts(g, s, mode)):
            assert np.array_equal(got, want), (s, mode)
        sc = OS.scores(*tot)
        for i, thr in enumerate(THR):
            for met in ("csi", "pod", "sucr", "bias"):
                want = g[f"p{s}_score_{mode}_{thr}_{met}"]
                got = np.mean(sc[met][i]) if mode == "2" else sc[met][i]
                assert np.allclose(got, want, rtol=1e-6, atol=1e-9), (s, mode, thr, met)
    # pooling the raw values and dividing once is the same thing (division by a positive constant is monotone)
    raw = pred.numpy()[:, :, :32 // s * s, :32 // s * s]
    N, T, H, W, C = raw.shape
    mx = raw.reshape(N, T, H // s, s, W // s, s, C).max(axis=(3, 5)) / np.float32(1.0 / 255.0)
    assert np.array_equal(mx, pool_np(pred.numpy(), s), equal_nan=True)


def test_pooled_construction_and_state_shapes():
    from prediff_amd.sevir_skill import SEVIRSkillScore
    m0 = SEVIRSkillScore(layout="NTHWC", mode="0", preprocess_type="sevir_pool4")
    assert m0.pool_scale == 4 and tuple(m0.hits.shape) == (6,) and tuple(m0.fas.shape) == (6,)
    m1 = SEVIRSkillScore(layout="NTHWC", mode="1", seq_len=6, preprocess_type="sevir_pool16")
    assert m1.pool_scale == 16 and tuple(m1.hits.shape) == (6, 6) and tuple(m1.misses.shape) == (6, 6)
    assert SEVIRSkillScore(layout="TCNHW", preprocess_type="sevir_pool3x").pool_scale == 3     # the first integer, as re.search(r'\d+')
    with pytest.raises(ValueError):
        SEVIRSkillScore(layout="NHWT", preprocess_type="sevir_pool4")    # the reference's rearrange needs N, T, H, W and C
    with pytest.raises(ValueError):
        SEVIRSkillScore(layout="NTHW", mode="1", seq_len=6, preprocess_type="sevir_pool16")
    with pytest.raises(ValueError):
        SEVIRSkillScore(layout="NTHWC", preprocess_type="sevir_pool")
    with pytest.raises(NotImplementedError):
        SEVIRSkillScore(layout="NTHWC", preprocess_type="other")


def _check_scores(m, g, s, mode):
    res = m.compute()
    for thr in THR + ("avg",):
        for met in ("csi", "pod", "sucr", "bias"):
            assert np.allclose(np.asarray(res[thr][met], dtype=np.float64), g[f"p{s}_score_{mode}_{thr}_{met}"], rtol=1e-6, atol=1e-9), \
                (s, mode, thr, met)


@pytest.mark.gpu
@pytest.mark.parametrize("s", POOLS)
def test_hip_pooled_skill_matches_reference(golden, s):
    from prediff_amd.sevir_skill import SEVIRSkillScore
    g = golden("skill_score_pool")
    pred, target = skill_inputs()
    for mode in MODES:
        m = SEVIRSkillScore(layout="NTHWC", mode=mode, seq_len=6, preprocess_type=f"sevir_pool{s}", threshold_list=THR,
                            metrics_list=("csi", "pod", "sucr", "bias"))
        m.update(pred.cuda(), target.cuda())
        m.update(pred.flip(0).cuda(), target.cuda())
        for st, want in zip((m.hits, m.misses, m.fas), golden_counts(g, s, mode)):
            assert np.array_equal(st.cpu().numpy().astype(np.int64), want), (s, mode)          # bit exact
        _check_scores(m, g, s, mode)
        m.reset()
        assert float(m.hits.sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["TCNHW", "NWHCT"])
def test_hip_pooled_skill_other_layouts(golden, layout):
    """The same frames permuted into other 5-letter layouts -- strided views, read in place -- give the golden counts."""
    from prediff_amd.sevir_skill import SEVIRSkillScore
    g = golden("skill_score_pool")
    pred, target = skill_inputs()
    perm = ["NTHWC".index(c) for c in layout]
    for s in (4, 3):
        for mode in ("0", "1"):
            m = SEVIRSkillScore(layout=layout, mode=mode, seq_len=6, preprocess_type=f"sevir_pool{s}", threshold_list=THR)
            m.update(pred.cuda().permute(*perm), target.cuda().permute(*perm))                        # non-contiguous views
            m.update(pred.flip(0).permute(*perm).contiguous().cuda(), target.permute(*perm).contiguous().cuda())
            for st, want in zip((m.hits, m.misses, m.fas), golden_counts(g, s, mode)):
                assert np.array_equal(st.cpu().numpy().astype(np.int64), want), (layout, s, mode)


@pytest.mark.gpu
def test_hip_pooled_skill_full_size():
    """Real frame size (8 x 6 x 128 x 128 x 1), pool 4 and 16, against the numpy oracle; NaNs included."""
    from prediff_amd.sevir_skill import SEVIRSkillScore
    gen = torch.Generator().manual_seed(3)
    target = (torch.randint(0, 256, (8, 6, 128, 128, 1), generator=gen).float() / 255) * (torch.rand(8, 6, 128, 128, 1, generator=gen) > 0.6)
    pred = (target + 0.1 * torch.randn(target.shape, generator=gen)).clamp(0, 1)
    pred[1, 2, 40, 77, 0] = float("nan")
    target[5, 0, 3, 3, 0] = float("nan")
    for s in (4, 16):
        m = SEVIRSkillScore(layout="NTHWC", mode="1", seq_len=6, preprocess_type=f"sevir_pool{s}", threshold_list=THR)
        m.update(pred.cuda(), target.cuda())
        want = pooled_counts(pred.numpy(), target.numpy(), s, True)
        for st, w in zip((m.hits, m.misses, m.fas), want):
            assert np.array_equal(st.cpu().numpy().astype(np.int64), w), s
