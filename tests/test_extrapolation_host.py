"""prediff_amd.extrapolation on the host: what the NumPy restatement of its definition (tests/_extrapolation_ref.py) achieves on
translating Gaussian blobs -- the conditions the device tests then rely on --, the rounding estimate the GPU bound is made of, and the
argument checks of the class, none of which reaches the library."""
import numpy as np
import pytest
import torch

import _extrapolation_ref as R
from prediff_amd import LagrangianPersistence
from prediff_amd import _lib as L
from prediff_amd import extrapolation as EX

SKILL = sorted(R.SKILL_CASES)


def test_restatement_pieces_by_hand():
    """the box sum, the gradients and the two samplers against direct loops on a small frame"""
    rng = np.random.default_rng(0)
    f = rng.standard_normal((1, 5, 7))
    r = 2
    direct = np.zeros_like(f)
    for y in range(5):
        for x in range(7):
            direct[0, y, x] = f[0, max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].sum()
    assert np.allclose(R.box(f, r), direct, rtol=1e-13, atol=1e-13)
    gy, gx = R.gradients(f)
    assert gy[0, 0, 3] == (f[0, 1, 3] - f[0, 0, 3]) / 2 and gy[0, 4, 3] == (f[0, 4, 3] - f[0, 3, 3]) / 2
    assert gx[0, 2, 0] == (f[0, 2, 1] - f[0, 2, 0]) / 2 and gx[0, 2, 3] == (f[0, 2, 4] - f[0, 2, 2]) / 2
    assert R.down2(f[:, :4, :6])[0, 1, 2] == pytest.approx(f[0, 2:4, 4:6].mean(), rel=1e-14)
    cy, cx = np.full((1, 5, 7), 1.25), np.full((1, 5, 7), 7.5)               # x beyond the frame: clamped to column 6
    assert R.bil_clamp(f, cy, cx)[0, 0, 0] == pytest.approx(0.75 * f[0, 1, 6] + 0.25 * f[0, 2, 6], rel=1e-14)
    cx = np.full((1, 5, 7), 6.5)                                             # half inside: the outer tap reads the fill
    assert R.bil_fill(f, cy, cx, -1.5)[0, 0, 0] == pytest.approx(0.5 * (0.75 * f[0, 1, 6] + 0.25 * f[0, 2, 6]) + 0.5 * -1.5, rel=1e-14)
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        assert R.bil_fill(f, np.full((1, 5, 7), bad), cx, -1.5)[0, 0, 0] == -1.5


def test_blobs_stay_three_sigma_inside():
    ctx, tgt = R.blobs(B=2, T=7, K=6, H=64, W=64, vel=(-3.0, 2.0), seed=8)
    assert ctx.shape == (2, 7, 64, 64, 1) and tgt.shape == (2, 6, 64, 64, 1) and ctx.dtype == np.float32
    seq = np.concatenate([ctx, tgt], axis=1)[..., 0]
    border = np.concatenate([seq[..., 0, :], seq[..., -1, :], seq[..., :, 0], seq[..., :, -1]], axis=-1)
    assert border.max() <= 3 * np.exp(-4.5) and seq.max() > 0.3              # three blobs of amplitude <= 1, each 3 sigma away
    with pytest.raises(ValueError):
        R.blobs(B=1, T=7, K=6, H=16, W=16, vel=(-3.0, 2.0), seed=0)


@pytest.mark.parametrize("name", SKILL)
def test_restatement_recovers_the_motion(name):
    ctx, tgt, levels, m64, f64, f32 = R.skill_case(name)
    vel = np.asarray(R.SKILL_CASES[name][0]["vel"])
    err = np.sqrt((m64[:, 0] - vel[0]) ** 2 + (m64[:, 1] - vel[1]) ** 2)
    med = float(np.median(err[ctx[:, -1, :, :, 0] > 0.1]))
    print(f"[extrapolation host] {name}: median motion error in echo {med:.3f} px")
    assert med < 0.5


@pytest.mark.parametrize("name", SKILL)
def test_restatement_beats_eulerian_persistence(name):
    ctx, tgt, levels, m64, f64, f32 = R.skill_case(name)
    pers = R.advect(ctx[:, -1], np.zeros_like(m64), tgt.shape[1])
    assert np.array_equal(pers, np.repeat(ctx[:, -1:].astype(np.float64), tgt.shape[1], axis=1))
    mse_f = ((f64 - tgt) ** 2).mean(axis=(0, 2, 3, 4))
    mse_p = ((pers - tgt) ** 2).mean(axis=(0, 2, 3, 4))
    print(f"[extrapolation host] {name}: MSE / persistence's per lead {np.round(mse_f / mse_p, 4).tolist()}")
    assert mse_f.shape == (6,) and (mse_f < 0.25 * mse_p).all()


@pytest.mark.parametrize("name", sorted(R.MOTION_CASES))
def test_fp32_rounding_of_the_gpu_motion_cases(name):
    """e32 = max |motion_fp32 - motion_fp64| of the restatement: the device bound is 8 e32 (tests/test_extrapolation.py)"""
    ctx, opts, m64, e32 = R.motion_case(name)
    print(f"[extrapolation host] {name}: e32 = {e32:.2e} px, largest |v| {np.abs(m64).max():.2f} px / frame")
    assert np.isfinite(m64).all() and np.abs(m64).max() > 0.25               # the case does measure a motion
    assert 0 < e32 < 1e-4


def test_zero_context_and_zero_motion_are_exact():
    z = np.zeros((2, 3, 16, 16, 1), np.float32)
    for dt in (np.float32, np.float64):
        assert (R.motion(z, levels=2, radius=2, dtype=dt) == 0).all()
    f = np.random.default_rng(1).standard_normal((2, 5, 7)).astype(np.float32)
    out = R.advect(f, np.zeros((2, 2, 5, 7)), 3, fill=-1.5, dtype=np.float32)
    assert all(np.array_equal(out[:, k, :, :, 0], f) for k in range(3))


# ------------------------------------------------------------------------------------------------ argument checks: no library call
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("an argument check reached the library")
    for fn in ("lib", "lk_ws_bytes", "lk_motion", "advect"):
        monkeypatch.setattr(L, fn, refuse)


@pytest.mark.parametrize("kw", [dict(out_len=0), dict(out_len=2.5), dict(levels=0), dict(levels=9), dict(iters=0), dict(radius=0),
                                dict(radius=10), dict(radius=True), dict(pairs=0), dict(damping=0.0), dict(damping=-1.0),
                                dict(damping=float("nan")), dict(fill=float("inf")), dict(fill=float("nan"))])
def test_constructor_validation(kw, no_library):
    with pytest.raises(ValueError):
        LagrangianPersistence(**kw)


def test_constructor_defaults(no_library):
    lp = LagrangianPersistence()
    assert (lp.out_len, lp.levels, lp.iters, lp.radius, lp.damping, lp.pairs, lp.fill) == (6, 4, 3, 7, 1e-2, 3, 0.0)
    assert lp._check_context((32, 7, 128, 128, 1)) == (32, 7, 128, 128) and lp._check_context((4, 13, 384, 384, 1)) == (4, 13, 384, 384)
    assert EX.MAX_RADIUS == 9 and EX.MAX_SIDE == 512


def test_method_validation_needs_no_library(no_library):
    lp = LagrangianPersistence(levels=3)
    ok = torch.zeros((2, 3, 16, 24, 1))
    for bad in (ok.double(), ok[..., 0], torch.zeros((2, 1, 16, 24, 1)), torch.zeros((2, 3, 16, 24, 2)), torch.zeros((2, 3, 18, 24, 1)),
                torch.zeros((2, 3, 12, 24, 1)), torch.zeros((2, 3, 16, 516, 1)), torch.zeros((0, 3, 16, 24, 1)),
                torch.zeros((2, 3, 24, 16, 1)).transpose(2, 3), ok.numpy(), ok):          # the last: a CPU tensor
        with pytest.raises(ValueError):
            lp.motion(bad)
        with pytest.raises(ValueError):
            lp.forecast(bad)
    frame, mot = torch.zeros((2, 16, 24, 1)), torch.zeros((2, 2, 16, 24))
    for f, m, k in ((frame, mot, 0), (frame, mot, 1.5), (frame.double(), mot, 1), (frame, mot.double(), 1), (frame[0], mot, 1),
                    (frame, mot[:, :1], 1), (frame, torch.zeros((2, 2, 24, 16)), 1), (frame, torch.zeros((2, 2, 24, 16)).transpose(2, 3), 1),
                    (torch.zeros((2, 24, 16)).transpose(1, 2), mot, 1), (torch.zeros((2, 16, 600)), torch.zeros((2, 2, 16, 600)), 1),
                    (frame, mot, 1), (frame[..., 0], mot, None)):                         # the last two: CPU tensors
        with pytest.raises(ValueError):
            lp.advect(f, m, k)
    with pytest.raises(ValueError):
        lp.forecast(ok, out_len=0)
    with pytest.raises(ValueError, match="pairs"):
        LagrangianPersistence(levels=1, pairs=40)._check_context((1, 40, 16, 16, 1))


def test_binding_refuses_cpu_tensors():
    z = torch.zeros((1, 2, 8, 8, 1))
    with pytest.raises(L.PrediffHipError):
        L.lk_motion(z, torch.zeros((1, 2, 8, 8)), 1, 2, 8, 8, 1, 1, 1, 1e-2, 1, torch.zeros(64))
    with pytest.raises(L.PrediffHipError):
        L.advect(z[:, -1, :, :, 0], torch.zeros((1, 2, 8, 8)), torch.zeros((1, 1, 8, 8, 1)), 1, 1, 8, 8, 64, 0.0)


def test_workspace_size_is_host_arithmetic():
    """pd_lk_ws_bytes: the pyramid above level 0 and two flow buffers per level; -1 for what pd_lk_motion refuses"""
    B, T, H, W = 3, 4, 16, 24
    assert L.lk_ws_bytes(B, T, H, W, 2, 3, 2, 3) == 4 * (B * 4 * 8 * 12 + 2 * B * 2 * (16 * 24 + 8 * 12))
    assert L.lk_ws_bytes(1, 2, 64, 64, 3, 3, 7, 3) == 4 * (2 * (32 * 32 + 16 * 16) + 4 * (64 * 64 + 32 * 32 + 16 * 16))   # P clipped to 1
    for bad in ((1, 1, 16, 16, 1, 3, 2, 3), (1, 4, 18, 16, 3, 3, 2, 3), (1, 4, 8, 8, 3, 3, 2, 3), (1, 4, 516, 16, 1, 3, 2, 3),
                (1, 4, 16, 16, 1, 3, 10, 3), (1, 4, 16, 16, 1, 0, 2, 3), (0, 4, 16, 16, 1, 3, 2, 3), (1, 40, 16, 16, 1, 3, 2, 17)):
        assert L.lk_ws_bytes(*bad) == -1, bad
