"""FVD on the device: the kernels of csrc/fvd.hip, the I3D feature engine and FrechetVideoDistance against the plain-torch restatement
tests/_i3d_ref.py (pinned on the reference's fixtures by tests/test_fvd_host.py).  Weights are seeded (no published checkpoint on hand)."""
import os

import pytest
import torch

import _i3d_ref as R
from prediff_amd import FrechetVideoDistance, InceptionI3d
from prediff_amd import _lib as L
from prediff_amd.packing import pad64, split_bf16
from prediff_amd.seeding import seeded_input

pytestmark = pytest.mark.gpu

# rel-L2 per video of the features against the restatement in float64, seeded weights.  Measured on the MI355X (profiles/fvd_accuracy.log):
# the restatement in fp32 on the CPU against itself in fp64 (the floor of the reference's own arithmetic) 4.8e-7 .. 1.2e-6; the fp32-class
# engine 5.8e-6 .. 6.12e-6 (the hi/lo products drop lo x lo, 2^-16 per product).  Bound = 3 x the worst, rounded up to one digit; it may
# not exceed 2e-4 (tests/test_hip_unet.py HEAVY_BOUND["fp32"]).  The single-pass engines measured 4.9e-4 (fp16) and 3.9e-3 (bf16).
FP32_BOUND = 2e-5
# the single-pass engines: finite and under the same-named entries of tests/test_hip_unet.py HEAVY_BOUND
SINGLE_PASS_BOUND = {"fp16": 7e-3, "bf16": 6e-2}
# end to end: |FVD_device - FVD_fp64| / FVD_fp64 measured 2.59e-6 (FVD 5.9124 against traces of 2.7214); bound 3 x that, rounded up to
# one digit; it may not exceed 1e-3
E2E_BOUND = 8e-6

_CACHE = {}


def weights(classes=400):
    if ("sd", classes) not in _CACHE:
        _CACHE[("sd", classes)] = R.seeded_weights(InceptionI3d(classes).state_dict())
    return _CACHE[("sd", classes)]


def engine(classes=400, precision="fp32"):
    key = ("net", classes, precision)
    if key not in _CACHE:
        net = InceptionI3d(classes, precision=precision)
        net.load_state_dict(weights(classes))
        _CACHE[key] = net.cuda()
    return _CACHE[key]


FEATURE_CASES = {"T9_B2": ("a", 400), "T24_B1": ((1, 24, 3, 40, 40), 400), "T12_600": ("b", 600)}


def case_input(case):
    src = FEATURE_CASES[case][0]
    return R.fixture_input(src) if isinstance(src, str) else seeded_input("fvd." + case, src, 4101, kind="uniform")


def reference_features(case):
    """the restatement in float64 (and, for the record, in fp32) -- computed once per session"""
    if ("ref", case) not in _CACHE:
        sd, v = weights(FEATURE_CASES[case][1]), case_input(case)
        _CACHE[("ref", case)] = (R.features_of(sd, v), R.features_of(sd, v, dtype=torch.float32))
    return _CACHE[("ref", case)]


# ---------------------------------------------------------------------------------------------------- max-pool
POOLS = [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((2, 2, 2), (2, 2, 2))]


@pytest.mark.parametrize("negative", [True, False])
@pytest.mark.parametrize("shape", [(2, 5, 7, 9, 24), (1, 6, 8, 8, 64)])
@pytest.mark.parametrize("kernel,stride", POOLS)
def test_maxpool_same_bit_equal(kernel, stride, shape, negative):
    """zero padding takes part in the max: an all-negative input shows it (border outputs are 0, not the largest negative value)"""
    B, T, H, W, C = shape
    x = seeded_input(f"pool{shape}{negative}", shape, 4104)
    x = -x.abs() - 0.01 if negative else x
    want = R.maxpool_same(x.permute(0, 4, 1, 2, 3), kernel, stride).permute(0, 2, 3, 4, 1).contiguous()
    rows = want.numel() // C
    of = torch.full((rows, C), float("nan"), device="cuda")
    both = torch.zeros((2, rows, pad64(C)), dtype=torch.bfloat16, device="cuda")
    out_thw = L.maxpool3d_same(x.cuda(), B, (T, H, W), C, kernel, stride, out_f32=of, outb=both[0], outb_lo=both[1])
    assert out_thw == tuple(want.shape[1:4])
    assert torch.equal(of.cpu().view(want.shape), want)
    hi, lo = split_bf16(want.view(rows, C), True)
    assert torch.equal(both[0, :, :C].cpu(), hi) and torch.equal(both[1, :, :C].cpu(), lo)
    assert float(both[:, :, C:].abs().max() if pad64(C) > C else 0) == 0
    if negative and any(L.same_pad(k, s, n) for k, s, n in zip(kernel, stride, (T, H, W))):
        assert float(want.max()) == 0.0          # a padded window of negative values gives the padding's 0
    half = torch.zeros((rows, pad64(C)), dtype=torch.float16, device="cuda")
    L.maxpool3d_same(x.cuda(), B, (T, H, W), C, kernel, stride, outb=half, opts=L.CallOpts("fp16"))
    assert torch.equal(half[:, :C].cpu(), want.view(rows, C).to(torch.float16))


# ---------------------------------------------------------------------------------------------------- preprocess
def _strided_nthwc():
    big = seeded_input("fvd.strided", (3, 5, 40, 52, 3), 4105, kind="uniform") * 255.0
    return big, (slice(1, 3), slice(0, 5), slice(4, 36), slice(2, 50), slice(0, 3))


@pytest.mark.parametrize("case", ["a", "b", "strided"])
def test_preprocess(case):
    if case == "strided":                          # an NTHWC view of a larger tensor, [0, 255] frames, every frame twice
        big, sl = _strided_nthwc()
        dev_in, layout, normalize, auto_t = big.cuda()[sl], "NTHWC", True, True
        ntchw = big[sl].permute(0, 1, 4, 2, 3)
        assert not dev_in.is_contiguous()
    else:
        ntchw, layout, normalize, auto_t = R.fixture_input(case), "NTCHW", False, False
        dev_in = ntchw.cuda()
    want = R.preprocess(R.prepare(ntchw, normalize, auto_t)).permute(0, 2, 3, 4, 1).contiguous()      # (N, T2, 224, 224, 3)
    N, T2 = want.shape[:2]
    from prediff_amd.sevir_skill import axes_of
    sizes, strides = axes_of(layout, dev_in)
    both = torch.full((2, N * T2 * 224 * 112, 64), 7.0, dtype=torch.bfloat16, device="cuda")
    f32 = torch.full((N, T2, 224, 224, 3), float("nan"), device="cuda")
    L.i3d_preprocess(dev_in, sizes, strides, normalize, auto_t, both[0], both[1], out_f32=f32)
    err = float((f32.cpu() - want).abs().max())
    # the operand: hi + lo of column 3 dw + c of row (n, t, y, ow) is frame[y][2 ow - 2 + dw][c], zero outside the frame and from column 21
    padded = torch.nn.functional.pad(want, (0, 0, 2, 3))                                           # W: 2 in front, 3 behind
    cols = padded.unfold(3, 7, 2).permute(0, 1, 2, 3, 5, 4).reshape(N * T2 * 224 * 112, 21)       # (.., ow, c, dw) -> (dw, c)
    op = (both[0].float() + both[1].float()).cpu()
    err_op = float((op[:, :21] - cols).abs().max())
    print(f"[preprocess {case}] fp32 output {err:.2e}, hi + lo operand {err_op:.2e} (max abs vs the restatement)")
    assert err < 1e-5 and err_op < 1e-5
    assert float(op[:, 21:].abs().max()) == 0
    half = torch.zeros((N * T2 * 224 * 112, 64), dtype=torch.float16, device="cuda")
    L.i3d_preprocess(dev_in, sizes, strides, normalize, auto_t, half, None, opts=L.CallOpts("fp16"))
    assert float((half[:, :21].float().cpu() - cols).abs().max()) < 1e-3                          # one rounding to 11 bits of values in [-1, 1]


# ---------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("n,d", [(1, 400), (5, 400), (33, 600)])
def test_feature_moments(n, d):
    runs = []
    fs = [seeded_input(f"mom{n}x{d}.{i}", (n, d), 4106) * 3.0 + 0.5 for i in range(2)]
    for _ in range(2):
        s = torch.zeros(d, dtype=torch.float64, device="cuda")
        c = torch.zeros((d, d), dtype=torch.float64, device="cuda")
        for f in fs:                                                   # two successive updates
            L.feature_moments_update(f.cuda(), s, c)
        runs.append((s.cpu(), c.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])         # the same inputs, the same bits
    F64 = torch.cat(fs).double()
    s, c = runs[0]
    # each entry within the rounding of an n-term fp64 sum in any order: 1e-12 x the sum of the terms' magnitudes
    assert bool(((s - F64.sum(0)).abs() <= 1e-12 * F64.abs().sum(0)).all())
    assert bool(((c - F64.T @ F64).abs() <= 1e-12 * (F64.abs().T @ F64.abs())).all())
    assert torch.equal(c, c.T)


# ---------------------------------------------------------------------------------------------------- features
@pytest.mark.parametrize("case", ["T9_B2", "T24_B1"])
def test_features_fp32(case):
    """T = 9: odd SAME padding in time; T = 24: two time positions for the head's mean"""
    f64, f32 = reference_features(case)
    got = engine().features(case_input(case).cuda())
    floor, err = R.rel_l2(f32, f64), R.rel_l2(got, f64)
    print(f"[features fp32 {case}] engine vs float64 {['%.2e' % e for e in err]}; the restatement in fp32 vs float64 {['%.2e' % e for e in floor]}")
    assert got.shape == f64.shape and bool(torch.isfinite(got).all())
    assert max(err) < FP32_BOUND


def test_forward_takes_the_preprocessed_video():
    f64, _ = reference_features("T9_B2")
    x = R.preprocess(R.prepare(case_input("T9_B2")))
    got = engine()(x.cuda())
    assert max(R.rel_l2(got, f64)) < FP32_BOUND


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_features_single_pass(precision):
    f64, _ = reference_features("T9_B2")
    got = engine(precision=precision).features(case_input("T9_B2").cuda())
    err = R.rel_l2(got, f64)
    print(f"[features {precision} T9_B2] engine vs float64 {['%.2e' % e for e in err]}")
    assert bool(torch.isfinite(got).all()) and max(err) < SINGLE_PASS_BOUND[precision]


def test_features_600_classes():
    f64, _ = reference_features("T12_600")
    got = engine(600).features(case_input("T12_600").cuda())
    err = R.rel_l2(got, f64)
    print(f"[features fp32 600 classes, T = 12] engine vs float64 {['%.2e' % e for e in err]}")
    assert got.shape == (1, 600) and max(err) < FP32_BOUND


# ---------------------------------------------------------------------------------------------------- end to end
def test_fvd_end_to_end():
    """16 real + 16 fake videos of 6 frames (auto_t), two updates of 8 each, against the restatement pipeline in float64 (the float64
    restatement of the 32 videos on the CPU is nearly all of this test's ~18 s; the device side takes under 0.1 s)"""
    real, fake = R.e2e_videos()
    sd = weights()
    fr = torch.cat([R.features_of(sd, real[i:i + 8], auto_t=True) for i in (0, 8)])
    ff = torch.cat([R.features_of(sd, fake[i:i + 8], auto_t=True) for i in (0, 8)])
    want, traces = R.frechet(fr, ff)
    assert want >= 0.01 * traces                  # a relative error means something (measured: FVD = 2.2 x the traces)
    m = FrechetVideoDistance(feature=400, weights=sd, auto_t=True)
    for i in (0, 8):
        m.update(real[i:i + 8].cuda(), real=True)
        m.update(fake[i:i + 8].cuda(), real=False)
    assert int(m.real_features_num_samples) == 16 and int(m.fake_features_num_samples) == 16 and m.real_features_cov_sum.is_cuda
    got = float(m.compute())
    rel = abs(got - want) / want
    print(f"[FVD end to end] device {got:.9f}, float64 restatement {want:.9f}, relative difference {rel:.2e} (traces {traces:.4f})")
    assert rel < E2E_BOUND
    m.reset()
    assert int(m.real_features_num_samples) == 0 and float(m.fake_features_cov_sum.abs().sum()) == 0


class _Mean(torch.nn.Module):
    def forward(self, v):
        return v.float().mean(dim=(1, 3, 4)).repeat(1, 4)[:, :8]


def test_custom_extractor_goes_through_the_moments_kernel():
    m = FrechetVideoDistance(feature=_Mean(), layout="NTHWC")
    v = seeded_input("fvd.custom", (5, 9, 16, 16, 1), 4107, kind="uniform")
    m.update(v.cuda(), real=True)
    f = _Mean()(v.permute(0, 1, 4, 2, 3).repeat(1, 1, 3, 1, 1)).double()
    assert m.real_features_sum.is_cuda and int(m.real_features_num_samples) == 5
    assert torch.allclose(m.real_features_sum.cpu(), f.sum(0), rtol=1e-12, atol=0)
    assert torch.allclose(m.real_features_cov_sum.cpu(), f.T @ f, rtol=1e-12, atol=0)


def test_sync_rccl_world1():
    """a world of one on "nccl" (= RCCL): the all-reduce really runs on the device state, also with no update made"""
    import torch.distributed as dist
    m = FrechetVideoDistance(feature=_Mean())
    idle = FrechetVideoDistance(feature=_Mean())
    v = seeded_input("fvd.sync", (3, 9, 3, 16, 16), 4108, kind="uniform")
    m.update(v.cuda(), real=False)
    before = [t.clone() for t in m._state("fake")]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29537")
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        m.sync()
        idle.sync()
    finally:
        dist.destroy_process_group()
    assert all(torch.equal(a, b) for a, b in zip(before, m._state("fake")))
    assert idle.real_features_sum.is_cuda and int(idle.fake_features_num_samples) == 0 and float(idle.real_features_cov_sum.abs().sum()) == 0
