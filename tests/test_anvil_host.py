"""prediff_amd.anvil without a GPU: the identities of the NumPy restatement (tests/_anvil_ref.py), the rounding error e32 of every case
the GPU tests run, the skill of the restatement on those cases against Lagrangian persistence, the share of near-threshold pixels, and
the host's argument checks."""
import numpy as np
import pytest
import torch

import _anvil_ref as A
import _steps_ref as S
from prediff_amd import AutoregressiveExtrapolation, LagrangianPersistence
from prediff_amd import _lib as L
from prediff_amd.anvil import anvil_window

AX = (0, 2, 3, 4)


# ------------------------------------------------------------------------------------------------ identities of the restatement
@pytest.mark.parametrize("name", list(A.CASES))
def test_restatement_levels_sum_to_the_last_frame(name):
    """sum_l Y_l0 = A_0 to 1e-12 relative with the bands in fp64 (rounded to fp32 they sum to one within 1e-7 only)"""
    c = A.case(name)
    an = A.analyse(c.ctx, c.motion, S.bands(c.H, c.W, c.L), c.ar, c.window, np.float64)
    A0 = an.A[:, 0]
    assert np.array_equal(A0, c.ctx[:, -1, :, :, 0].astype(np.float64))
    assert np.abs(an.Y0.sum(axis=1) - A0).max() <= 1e-12 * np.abs(A0).max()
    assert an.D.shape == (c.B, c.L, c.ar + 1, c.H, c.W) and an.phi.shape == an.gamma.shape == (c.B, c.L, 2, c.H, c.W)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_zero_context_gives_zeros(dtype):
    c = A.case("16x16-ar2")
    an = A.analyse(np.zeros_like(c.ctx), c.motion, c.w, 2, c.window, dtype)
    assert all((getattr(an, k) == 0).all() for k in ("phi", "gamma", "Y0", "D"))
    R = A.evolve(an, c.K)
    assert R.dtype == dtype and (R == 0).all() and (A.finish(R, c.motion) == 0).all()


def test_restatement_persistence_limit():
    """identical frames, zero motion: every difference is exactly zero and R^(k) is sum_l Y_l0, A_0 up to the rounding of the bands"""
    p = S.persistence_case()
    ctx = np.ascontiguousarray(np.broadcast_to(p.ctx[:, :1], (1, 4, 16, 16, 1)))
    for dtype, tol in ((np.float64, 1e-6), (np.float32, 1e-6)):
        an = A.analyse(ctx, p.motion, p.w, 2, 2.0, dtype)
        assert (an.D == 0).all() and (an.phi == 0).all()
        R = A.evolve(an, p.K)
        d = np.abs(R.astype(np.float64) - p.A0[:, None]).max()
        print(f"[anvil] persistence {np.dtype(dtype).name}: max |R^(k) - A_0| = {d:.2e}")
        assert R.shape == (1, p.K, 16, 16) and d <= tol


@pytest.mark.parametrize("name", list(A.CASES))
def test_restatement_parameters_are_stationary(name):
    c = A.case(name)
    g1, g2 = c.gamma[:, :, 0], c.gamma[:, :, 1]
    p1, p2 = c.phi[:, :, 0], c.phi[:, :, 1]
    assert np.abs(g1).max() <= 1 - A.EPS and np.abs(g1).max() > 0.5             # the trend is seen: the clamp is reached near the blobs
    if c.ar == 1:
        assert np.array_equal(p1, g1) and (p2 == 0).all() and (g2 == 0).all()
    else:
        assert (g2 <= 1 - A.EPS).all() and (g2 >= 2 * g1 * g1 - 1 + A.EPS - 1e-15).all()
        assert (np.abs(p2) < 1).all() and (p2 + p1 < 1).all() and (p2 - p1 < 1).all()   # the stationarity triangle


# ------------------------------------------------------------------------------------------------ the rounding error of the GPU cases
# twice the e32 measured here (NumPy 2.2, fp32 pocketfft); the measured values are in the docstring below and in DESIGN.md §7
E32_BOUND = {"16x16-ar1":   dict(gamma=1.2e-5, phi=1.2e-5, R=2.5e-6),
             "16x16-ar2":   dict(gamma=2.4e-5, phi=3.6e-4, R=9.3e-6),
             "12x12-ar2":   dict(gamma=7.0e-6, phi=2.4e-4, R=1.2e-5),
             "24x16-ar2":   dict(gamma=2.6e-5, phi=5.9e-4, R=8.6e-6),
             "32x64-ar2":   dict(gamma=4.8e-5, phi=8.8e-4, R=1.1e-5),
             "128x128-ar2": dict(gamma=3.8e-6, phi=1.6e-3, R=2.9e-6)}


@pytest.mark.parametrize("name", list(A.CASES))
def test_rounding_error_of_the_gpu_cases(name):
    """e32 = max |fp32 restatement - fp64 restatement| per quantity; the GPU tests hold the kernels to 8 e32, and E32_BOUND is twice the
    value measured here:
                     gamma     phi       R
      16x16-ar1      5.77e-6   5.77e-6   1.23e-6
      16x16-ar2      1.16e-5   1.80e-4   4.61e-6
      12x12-ar2      3.50e-6   1.16e-4   5.76e-6
      24x16-ar2      1.26e-5   2.93e-4   4.26e-6
      32x64-ar2      2.39e-5   4.37e-4   5.29e-6
      128x128-ar2    1.88e-6   7.93e-4   1.44e-6
    (gamma is a ratio of windowed sums that both shrink away from the blobs, down to the regulariser delta; AR(2) divides by
    1 - gamma_1^2 >= 2e-3: phi carries that amplification.)  An e32 below the rounding of the fp32 format itself (2^-26 of the
    quantity's size) would measure luck, not arithmetic: none of the values above is."""
    c = A.case(name)
    print(f"[anvil] e32 {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in c.e32.items()))
    for k, v in c.e32.items():
        assert 2.0 ** -26 * np.abs(getattr(c, k)).max() < v < E32_BOUND[name][k], (k, v)


@pytest.mark.parametrize("name", list(A.CASES))
def test_restatement_beats_lagrangian_persistence(name):
    """The skill condition, a condition on the inputs: on each case the restatement forecast's MSE against the true future frames is
    below 0.75 of that of Lagrangian persistence with the same motion at every lead, and below 0.5 of it at the last lead.  Measured:
    16x16-ar1 0.29 0.12 0.15; 16x16-ar2 0.29 0.18 0.28; 12x12-ar2 0.21 0.10 0.19; 24x16-ar2 0.47 0.19 0.25; 32x64-ar2 0.40 0.13 0.08; 128x128-ar2 0.47 0.12.
    (Lead 1 is the worst: there persistence errs by one step of growth only, while the forecast pays for the cut of step 10, which
    persistence does not make.)"""
    c = A.case(name)
    mse_f, mse_p = ((c.forecast - c.tgt) ** 2).mean(axis=AX), ((c.persistence - c.tgt) ** 2).mean(axis=AX)
    print(f"[anvil] {name}: MSE / Lagrangian persistence's per lead {np.round(mse_f / mse_p, 3).tolist()}")
    assert mse_f.shape == (c.K,) and (mse_f < 0.75 * mse_p).all() and mse_f[-1] < 0.5 * mse_p[-1]
    wet = (c.forecast > 0).mean()
    assert 0.02 < wet < 0.98


@pytest.mark.parametrize("name", list(A.CASES))
def test_few_pixels_sit_near_the_threshold(name):
    """Step 10 cuts at thr: a pixel whose R lies within 8 e32(R) of thr may fall on either side on the device, so the GPU test leaves out
    the output pixels that have such a pixel among their taps -- and must leave out at most 1 %."""
    c = A.case(name)
    near = np.abs(c.R - float(np.float32(c.thr))) <= 8 * c.e32["R"]
    left_out = S.advect_leads(near[None].astype(np.float64), c.motion)[0] > 0
    print(f"[anvil] {name}: {int(near.sum())} of {near.size} pixels within {8 * c.e32['R']:.1e} of thr, {left_out.mean():.3%} of the output")
    assert left_out.mean() <= 0.01


# ------------------------------------------------------------------------------------------------ arguments
def test_window_table():
    g, w0 = anvil_window(16.0)
    assert g.dtype == torch.float32 and tuple(g.shape) == (97,) and float(g[48]) == 1.0 and torch.equal(g, g.flip(0))
    ref, r, W0 = A.window(16.0)
    assert r == 48 and np.array_equal(g.numpy(), ref) and w0 == W0
    assert tuple(anvil_window(0.5)[0].shape) == (5,) and tuple(anvil_window(32.0)[0].shape) == (193,)


def test_workspace_size_is_host_arithmetic():
    per = (2 * 8 + 6 * (1 + 3 + 5) * 4) * 128 * 128               # two spectra, then Y_l0, three D and five moments per level
    assert L.anvil_ws_bytes(1, 128, 128, 6, 2) == per + 16 and L.anvil_ws_bytes(2, 128, 128, 6, 2) == 2 * per + 16   # + mean(A_0^2)
    assert L.anvil_ws_bytes(3, 24, 16, 3, 1) % 16 == 0 and L.anvil_ws_bytes(1, 12, 8, 2, 2) % 16 == 0 and L.anvil_ws_bytes(1, 12, 12, 2, 1) > 0
    for args in ((1, 16, 16, 3, 3), (0, 16, 16, 3, 2), (1, 16, 16, 4, 2), (1, 20, 16, 3, 2), (1, 256, 256, 6, 2), (1, 4, 16, 2, 2)):
        assert L.anvil_ws_bytes(*args) == -1


def test_constructor_refuses_bad_options():
    for kw, msg in ((dict(ar_order=3), "ar_order must be 1 or 2"), (dict(ar_order=0), "ar_order must be 1 or 2"),
                    (dict(ar_order=1.5), "ar_order must be an integer"), (dict(levels=1), "levels must be >= 2"),
                    (dict(levels=True), "levels must be an integer"), (dict(out_len=0), "out_len must be >= 1"),
                    (dict(window=0.25), r"window must be 0\.5 \.\. 32\.0 pixels"), (dict(window=33), r"window must be 0\.5 \.\. 32\.0 pixels"),
                    (dict(window=float("nan")), "window must be"), (dict(window="x"), "window and threshold must be finite numbers"),
                    (dict(threshold=float("nan")), "threshold must be finite"), (dict(threshold=float("inf")), "threshold must be finite"),
                    (dict(threshold=None), "window and threshold must be finite numbers"),
                    (dict(motion=object()), "motion must be a LagrangianPersistence")):
        with pytest.raises(ValueError, match=msg):
            AutoregressiveExtrapolation(**kw)
    ae = AutoregressiveExtrapolation()
    assert (ae.out_len, ae.levels, ae.ar_order, ae.window) == (6, 6, 2, 16.0) and ae.threshold == 16 / 255
    assert isinstance(ae.motion, LagrangianPersistence)


def test_calls_refuse_bad_tensors_on_the_host():
    """every check of the context by its own message: all the tensors are on the CPU, which alone would be refused, last"""
    ae = AutoregressiveExtrapolation(levels=3)
    ok = torch.zeros((1, 4, 16, 16, 1))
    bad = [(ok.double(), "ctx must be a float32 tensor"),
           (ok.numpy(), "ctx must be a float32 tensor"),
           (ok[:, :0], "the empty shape"),
           (ok[..., 0], r"ctx must be \(B, T, H, W, 1\)"),                          # rank
           (torch.zeros((1, 4, 16, 16, 2)), r"ctx must be \(B, T, H, W, 1\)"),      # channels
           (ok[:, :3], r"AR\(2\) on first differences needs T >= 4 context frames, got 3"),
           (torch.zeros((1, 4, 20, 16, 1)), "frames of 20 x 16 are not supported"),
           (torch.zeros((1, 4, 256, 256, 1)), "frames of 256 x 256 are not supported"),
           (torch.zeros((1, 4, 4, 16, 1)), "frames of 4 x 16 are not supported"),
           (torch.zeros((1, 4, 16, 32, 1))[:, :, :, ::2], "ctx must be contiguous"),
           (ok, "no CPU path")]
    for x, msg in bad:
        for call in (ae.analyse, ae.evolve, ae.forecast):
            with pytest.raises(ValueError, match=msg):
                call(x)
    with pytest.raises(ValueError, match=r"AR\(1\) on first differences needs T >= 3 context frames, got 2"):
        AutoregressiveExtrapolation(levels=3, ar_order=1).forecast(ok[:, :2])
    with pytest.raises(ValueError, match="no CPU path"):
        AutoregressiveExtrapolation(levels=3, ar_order=1).forecast(ok[:, :3])      # three frames are enough for AR(1)
    with pytest.raises(ValueError, match=r"levels must be 2 \.\. floor\(log2\(max\(H, W\)\)\) - 1 = 3"):
        AutoregressiveExtrapolation(levels=4).forecast(ok)
    for call in (ae.evolve, ae.forecast):
        with pytest.raises(ValueError, match="out_len must be >= 1"):
            call(ok, out_len=0)
        with pytest.raises(ValueError, match="out_len must be an integer"):
            call(ok, out_len=2.5)
