"""prediff_amd.steps without a GPU: the band weights, the identities of the NumPy restatement (tests/_steps_ref.py), the rounding error
e32 of every case the GPU tests run, the share of near-threshold pixels of those cases, and the host's argument checks."""
import numpy as np
import pytest
import torch

import _steps_ref as S
from prediff_amd import StochasticExtrapolation, steps_bands
from prediff_amd import _lib as L


# ------------------------------------------------------------------------------------------------ steps_bands
@pytest.mark.parametrize("H,W,levels", [(16, 16, 3), (24, 16, 3), (128, 128, 6)])
def test_bands_sum_to_one_and_are_even(H, W, levels):
    w = steps_bands(H, W, levels)
    assert w.dtype == torch.float32 and tuple(w.shape) == (levels, H, W) and not w.is_cuda
    w = w.numpy()
    assert np.abs(w.astype(np.float64).sum(axis=0) - 1).max() <= 1e-6
    assert (w >= 0).all()
    neg = w[:, (-np.arange(H)) % H][:, :, (-np.arange(W)) % W]
    assert np.array_equal(w, neg)                                                  # w(k) = w(-k)
    assert np.array_equal(w, S.bands(H, W, levels).astype(np.float32))            # the restatement's, rounded once
    assert w[:, 0, 0].argmax() == 0 and w[:, H // 2, W // 2].argmax() == levels - 1   # the mean sits in level 0, the corner in the last


@pytest.mark.parametrize("H,W,levels", [(16, 16, 1), (16, 16, 4), (128, 128, 7), (24, 16, 0), (20, 16, 3), (256, 256, 6), (4, 16, 2)])
def test_bands_refuse_levels_and_frames_out_of_range(H, W, levels):
    with pytest.raises(ValueError):
        steps_bands(H, W, levels)
    assert L.steps_ws_bytes(1, 1, H, W, levels, 2) == -1


def test_workspace_size_is_host_arithmetic():
    assert L.steps_ws_bytes(1, 1, 128, 128, 6, 2) > L.steps_ws_bytes(1, 0, 128, 128, 6, 2) > 0
    assert L.steps_ws_bytes(2, 3, 24, 16, 3, 1) % 8 == 0
    assert L.steps_ws_bytes(1, 1, 16, 16, 3, 3) == -1 and L.steps_ws_bytes(0, 1, 16, 16, 3, 2) == -1


# ------------------------------------------------------------------------------------------------ identities of the restatement
@pytest.mark.parametrize("name", list(S.CASES))
def test_restatement_recomposes_the_last_frame(name):
    """R^(0) = A_0 to 1e-12 relative, with the bands in fp64 (rounded to fp32 they sum to one within 1e-7 only)"""
    c = S.case(name)
    an = S.analyse(c.ctx, c.motion, S.bands(c.H, c.W, c.L), c.ar, c.thr, np.float64)
    A0 = an.A[:, 0]
    assert np.abs(S.recompose0(an) - A0).max() <= 1e-12 * np.abs(A0).max()
    wet = (A0 > np.float32(c.thr)).mean(axis=(-2, -1))
    assert (wet > 0.02).all() and (wet < 0.9).all()                               # wet0 neither empty nor full


@pytest.mark.parametrize("name", list(S.CASES))
def test_restatement_noise_is_normalised_and_ar_is_stationary(name):
    c = S.case(name)
    eh = S.shaped_noise(c.an, c.w, c.noise, np.float64)
    mean, var = eh.mean(axis=(-2, -1)), eh.var(axis=(-2, -1))
    zero = (eh == 0).all(axis=(-2, -1))
    assert ((np.abs(mean) < 1e-12) & (np.abs(np.sqrt(var) - 1) < 1e-12) | zero).all()
    p1, p2 = c.phi[..., 0].astype(np.float64), c.phi[..., 1].astype(np.float64)
    assert (np.abs(p2) < 1).all() and (p2 + p1 < 1).all() and (p2 - p1 < 1).all()
    assert (c.phi[..., 2] >= 0).all() and (c.sigma > 0).all()
    if c.ar == 1:
        assert (p2 == 0).all()


def test_restatement_zero_context_shapes_no_noise():
    """a constant field: every level is dead, P = 0, e^ = 0 exactly, R = thr up to rounding, and the finished forecast is exactly 0"""
    c = S.case("16x16-ar2")
    ctx = np.zeros_like(c.ctx)
    an = S.analyse(ctx, c.motion, c.w, 2, c.thr, np.float64)
    assert (an.sigma == 0).all() and (an.gamma == 0).all() and (an.P == 0).all()
    assert (S.shaped_noise(an, c.w, c.noise, np.float64) == 0).all()
    R = S.evolve(an, c.w, c.noise, c.K)
    assert np.abs(R - np.float32(c.thr)).max() < 1e-7
    assert (S.finish(R, ctx, c.motion, c.thr) == 0).all()


def test_restatement_persistence_limit():
    """identical frames, zero motion, no noise: |R^(k) - A_0| <= K eps sum_l sigma_l (phi1 + phi2 = 1 - eps / 2 + O(eps^2), |N_l| < 2)"""
    p = S.persistence_case()
    d = np.abs(p.R - p.A0[None, :, None]).max(axis=(0, 1, 3, 4))
    print(f"[steps] persistence: |R^(k) - A_0| = {d}, bound {p.K * S.EPS * p.sum_sigma:.3e}")
    assert d.shape == (p.K,) and (d > 0).all() and (d <= p.K * S.EPS * p.sum_sigma).all()


# ------------------------------------------------------------------------------------------------ the rounding error of the GPU cases
# twice the e32 measured here (NumPy 2.2, fp32 pocketfft); the measured values are in the docstring below
E32_BOUND = {"16x16-ar1":   dict(mu=7.0e-9, sigma=1.3e-8, gamma=2.6e-7, phi=1.1e-6, R=5.7e-7, R0=4.4e-7),
             "16x16-ar2":   dict(mu=7.0e-9, sigma=1.3e-8, gamma=4.8e-7, phi=8.2e-5, R=9.4e-6, R0=6.5e-6),
             "24x16-ar1":   dict(mu=5.3e-9, sigma=8.3e-9, gamma=2.4e-7, phi=1.9e-6, R=7.1e-7, R0=1.9e-7),
             "24x16-ar2":   dict(mu=5.3e-9, sigma=8.3e-9, gamma=4.1e-7, phi=9.1e-5, R=3.8e-6, R0=3.4e-6),
             "32x64-ar1":   dict(mu=4.9e-9, sigma=1.3e-8, gamma=2.0e-7, phi=1.6e-6, R=4.9e-7, R0=3.1e-7),
             "32x64-ar2":   dict(mu=4.9e-9, sigma=1.3e-8, gamma=2.0e-7, phi=6.0e-5, R=1.0e-5, R0=8.3e-6),
             "128x128-ar2": dict(mu=6.1e-9, sigma=1.3e-8, gamma=1.4e-6, phi=1.3e-3, R=1.8e-5, R0=6.0e-6)}


@pytest.mark.parametrize("name", list(S.CASES))
def test_rounding_error_of_the_gpu_cases(name):
    """e32 = max |fp32 restatement - fp64 restatement| per quantity; the GPU tests hold the kernels to 8 e32, and E32_BOUND is twice the
    value measured here:
                     mu        sigma     gamma     phi       R         R (no noise)
      16x16-ar1      3.49e-9   6.26e-9   1.28e-7   5.16e-7   2.83e-7   2.16e-7
      16x16-ar2      3.49e-9   6.26e-9   2.35e-7   4.09e-5   4.66e-6   3.23e-6
      24x16-ar1      2.62e-9   4.12e-9   1.16e-7   9.37e-7   3.50e-7   9.44e-8
      24x16-ar2      2.62e-9   4.12e-9   2.05e-7   4.51e-5   1.85e-6   1.67e-6
      32x64-ar1      2.41e-9   6.39e-9   9.53e-8   7.67e-7   2.45e-7   1.54e-7
      32x64-ar2      2.41e-9   6.39e-9   9.53e-8   2.97e-5   4.96e-6   4.14e-6
      128x128-ar2    3.01e-9   6.34e-9   6.92e-7   6.03e-4   8.71e-6   2.98e-6
    (AR(2) divides by 1 - gamma_1^2 with gamma_1 up to 0.99999 on these smooth fields: phi carries that amplification, and R inherits it.)
    mu, sigma, phi and gamma are a handful of fp32 numbers per case, and an e32 that happened to fall below the rounding of the fp32
    format itself (a quarter of an ulp of the largest value, 2^-26 of it at least) would measure luck, not arithmetic: the seeds of
    the cases were chosen so that none of the values above does."""
    c = S.case(name)
    print(f"[steps] e32 {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in c.e32.items()))
    for k, v in c.e32.items():
        assert 0 < v < E32_BOUND[name][k], (k, v)


@pytest.mark.parametrize("name,mask,match", S.FINISH_RUNS)
def test_few_pixels_sit_near_the_threshold(name, mask, match):
    """Step 9 cuts at thr: a pixel whose R lies within delta = 8 e32(R) of thr may fall on either side on the device, so the GPU test
    leaves such pixels out -- and must leave out at most 1 %.  Counted here on the fp64 R after mask and match; the pixels the mask
    itself set to thr are on the threshold by definition, in the restatement and on the device alike, and are not counted.  Without
    the mask the floored background itself hovers about thr as soon as noise is added, so mask=None runs on the 16 x 16 case, whose
    noise lifts it clear."""
    c = S.case(name)
    Rm, forced = S.mask_match(c.R, c.ctx, c.thr, mask, match)
    near = (np.abs(Rm - float(np.float32(c.thr))) <= 8 * c.e32["R"]) & ~forced
    print(f"[steps] {name} mask={mask} match={match}: {int(near.sum())} of {near.size} pixels within {8 * c.e32['R']:.1e} of thr")
    assert near.mean() <= 0.01
    assert 0.02 < (Rm > float(np.float32(c.thr))).mean() < 0.98


# ------------------------------------------------------------------------------------------------ arguments
def test_constructor_refuses_bad_options():
    for kw, msg in ((dict(ar_order=3), "ar_order must be 1 or 2"), (dict(ar_order=0), "ar_order must be 1 or 2"),
                    (dict(ar_order=1.5), "ar_order must be an integer"), (dict(mask="sprog"), "mask must be"),
                    (dict(mask="incremental"), "mask must be"), (dict(match="cdf"), "match must be"), (dict(levels=1), "levels must be >= 2"),
                    (dict(levels=True), "levels must be an integer"), (dict(out_len=0), "out_len must be >= 1"),
                    (dict(threshold=float("nan")), "threshold must be finite"), (dict(threshold=float("inf")), "threshold must be finite"),
                    (dict(threshold="x"), "threshold must be a finite number"), (dict(motion=object()), "motion must be a LagrangianPersistence")):
        with pytest.raises(ValueError, match=msg):
            StochasticExtrapolation(**kw)
    se = StochasticExtrapolation()
    assert (se.out_len, se.levels, se.ar_order, se.mask, se.match) == (6, 6, 2, "obs", "mean") and se.threshold == 16 / 255


def test_calls_refuse_bad_tensors_on_the_host():
    """every check of the context by its own message: all the tensors are on the CPU, which alone would be refused, last"""
    se = StochasticExtrapolation(levels=3)
    ok = torch.zeros((1, 3, 16, 16, 1))
    bad = [(ok.double(), "ctx must be a float32 tensor"),
           (ok.numpy(), "ctx must be a float32 tensor"),
           (ok[:, :0], "the empty shape"),
           (ok[..., 0], r"ctx must be \(B, T, H, W, 1\)"),                          # rank
           (torch.zeros((1, 3, 16, 16, 2)), r"ctx must be \(B, T, H, W, 1\)"),      # channels
           (ok[:, :2], r"AR\(2\) needs T >= 3 context frames, got 2"),
           (torch.zeros((1, 3, 20, 16, 1)), "frames of 20 x 16 are not supported"),
           (torch.zeros((1, 3, 256, 256, 1)), "frames of 256 x 256 are not supported"),
           (torch.zeros((1, 3, 4, 16, 1)), "frames of 4 x 16 are not supported"),
           (torch.zeros((1, 3, 16, 32, 1))[:, :, :, ::2], "ctx must be contiguous"),
           (ok, "no CPU path")]
    for x, msg in bad:
        for call in (se.analyse, se.evolve, se.forecast):
            with pytest.raises(ValueError, match=msg):
                call(x)
    with pytest.raises(ValueError, match=r"AR\(1\) needs T >= 2 context frames, got 1"):
        StochasticExtrapolation(levels=3, ar_order=1).forecast(ok[:, :1])
    with pytest.raises(ValueError, match="no CPU path"):
        StochasticExtrapolation(levels=3, ar_order=1).forecast(ok[:, :2])          # two frames are enough for AR(1)
    with pytest.raises(ValueError, match=r"levels must be 2 \.\. floor\(log2\(max\(H, W\)\)\) - 1 = 3"):
        StochasticExtrapolation(levels=4).forecast(ok)
    with pytest.raises(ValueError, match="members or noise, not both"):
        se.forecast(ok, members=2, noise=torch.zeros((2, 1, 6, 16, 16)))
    for m, msg in ((0, "members must be 1 .. 512"), (513, "members must be 1 .. 512"), (1.5, "members must be an integer")):
        with pytest.raises(ValueError, match=msg):
            se.forecast(ok, members=m)
    for call in (se.evolve, se.forecast):
        with pytest.raises(ValueError, match="out_len must be >= 1"):
            call(ok, out_len=0)
        with pytest.raises(ValueError, match="out_len must be an integer"):
            call(ok, out_len=2.5)
