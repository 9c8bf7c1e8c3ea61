"""GPU: the MX (block-scaled e4m3) kernels -- pd_quantize_mx and the two norm producers against the numpy restatement of the format
(tests/_mx_ref.py), pd_igemm_mx against the fp64 product of the dequantised operands with an independent random exponent on every
block of both operands (a misrouted scale byte is invisible with equal scales), and the unit-scale e4m3 launch around an MX launch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _mx_ref as R  # noqa: E402
from prediff_amd import _lib as L  # noqa: E402
from prediff_amd.packing import dequantize_mx, pack_conv_fp8, pad128, quantize_mx, to_fp8  # noqa: E402
from test_mx_host import adversarial_rows  # noqa: E402

DEV = "cuda"


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("K", [32, 96, 160])
@pytest.mark.parametrize("rows", [1, 3, 65])
def test_quantize_mx_equals_the_reference(rows, K):
    x = adversarial_rows(rows, K, seed=rows + K)
    ld = pad128(K)
    q = torch.full((rows, ld), 0x55, dtype=torch.uint8, device=DEV)
    s = torch.full((rows, ld // 32), 0x55, dtype=torch.uint8, device=DEV)
    L.quantize_mx(torch.from_numpy(x).to(DEV), q, s, rows, K)
    rq, rs = R.quantize(x, ld=ld)
    assert np.array_equal(s.cpu().numpy(), rs) and np.array_equal(q.cpu().numpy(), rq)
    with pytest.raises(L.PrediffHipError):                     # K % 32 != 0
        L.quantize_mx(torch.zeros(rows, 48, device=DEV), q, s, rows, 48, ld=ld)


def _producer_check(what, y32, q, s, C, cap):
    """payload / scales of a norm producer against _mx_ref on the fp32 reference of the norm: a payload byte may differ where the norm's own
    rounding moved the value across an e4m3 rounding boundary (share <= cap), a scale byte only where the block's amax element is such a byte"""
    ld = q.shape[1]
    rq, rs = R.quantize(y32.cpu().numpy(), ld=ld)
    q, s = q.cpu().numpy(), s.cpu().numpy()
    diff = q != rq
    share = diff[:, :C].mean()
    print(f"[{what}] payload bytes that differ from the reference: {int(diff.sum())} of {diff[:, :C].size} = {share:.2e} (cap {cap:.2e}); scale bytes {int((s != rs).sum())}")
    assert not diff[:, C:].any() and not s[:, C // 32:].any()          # padding: zero payload, scale byte 0
    assert share <= cap
    amax_at = np.abs(y32.cpu().numpy()).reshape(y32.shape[0], C // 32, 32).argmax(-1)
    amax_diff = np.take_along_axis(diff[:, :C].reshape(y32.shape[0], C // 32, 32), amax_at[..., None], -1)[..., 0]
    assert not ((s != rs)[:, :C // 32] & ~amax_diff).any()
    assert rel_l2(R.dequantize(q, s)[:, :C], y32) < 4e-2               # e4m3: three mantissa bits


# The share of payload bytes that the norm's own fp32 rounding moves across an e4m3 rounding boundary, measured on the CPU for each case
# below (torch's fp32 against its fp64 statement of the norm on the same inputs, both through _mx_ref.quantize; about 2 M elements per
# case, so that the counts mean something; no scale byte differed in any case).  A case's cap is 3x its measured share; the reference of
# the comparison is the same CPU fp32 statement.
LN_SHARE = {(4096, 512): 1.9e-6, (2048, 1024): 9.5e-7, (20001, 96): 1.0e-6}
GN_SHARE = {(4, 2048, 256, 32, False): 1.9e-6, (4, 2048, 256, 32, True): 2.4e-6, (8, 4001, 64, 16, False): 2.9e-6}


@pytest.mark.parametrize("rows,C", list(LN_SHARE))
def test_layernorm_mx(rows, C):
    g = torch.Generator(device="cpu").manual_seed(rows + C)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV), (0.3 * torch.randn(C, generator=g)).to(DEV)
    gamma[3] = 40.0                                            # an outlier channel: its block gets its own scale, nothing saturates
    ld = pad128(C)
    q = torch.full((rows, ld), 0x55, dtype=torch.uint8, device=DEV)
    s = torch.full((rows, ld // 32), 0x55, dtype=torch.uint8, device=DEV)
    L.layernorm_mx(x, gamma, beta, q, s, rows, C)
    _producer_check(f"layernorm mx C={C}", F.layer_norm(x.cpu(), (C,), gamma.cpu(), beta.cpu(), 1e-5), q, s, C, 3 * LN_SHARE[rows, C])


@pytest.mark.parametrize("B,S,C,G,ss", list(GN_SHARE))
def test_groupnorm_silu_mx(B, S, C, G, ss):
    g = torch.Generator(device="cpu").manual_seed(B + S + C)
    x = (torch.randn(B, S, C, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV), (0.3 * torch.randn(C, generator=g)).to(DEV)
    gamma[5] = 30.0
    emb = (0.3 * torch.randn(B, 2 * C, generator=g)).to(DEV) if ss else None
    ld = pad128(C)
    part = torch.empty(B * L.groupnorm_nchunk(S, C) * G * 2, dtype=torch.float64, device=DEV)
    q = torch.full((B * S, ld), 0x55, dtype=torch.uint8, device=DEV)
    s = torch.full((B * S, ld // 32), 0x55, dtype=torch.uint8, device=DEV)
    kw = dict(ss_scale=emb, ss_shift=emb[:, C:], ld_ss=2 * C) if ss else {}
    L.groupnorm_silu_mx(x, gamma, beta, part, q, s, B, S, C, G, 1e-5, silu=True, **kw)
    y = F.group_norm(x.cpu().permute(0, 2, 1), G, gamma.cpu(), beta.cpu(), 1e-5).permute(0, 2, 1)
    if ss:
        y = y * (1 + emb.cpu()[:, None, :C]) + emb.cpu()[:, None, C:]
    _producer_check(f"groupnorm silu mx C={C}", F.silu(y).reshape(B * S, C), q, s, C, 3 * GN_SHARE[B, S, C, G, ss])


def _random_mx(shape_rows, K, gen):
    """an MX operand with an independent random exponent in [-12, 12] on every block: (payload, scales) on the GPU, padded to 128.  The
    payload is what the quantiser emits for asymmetric Gaussian rows (every block's largest element in (224, 448]); the random exponents
    replace its scale bytes."""
    x = torch.randn(shape_rows + (K,), generator=gen) + torch.linspace(-1, 1, K) * 0.5
    q, s = quantize_mx(x)
    s[..., :K // 32] = (127 + torch.randint(-12, 13, shape_rows + (K // 32,), generator=gen)).to(torch.uint8)
    return q.to(DEV), s.to(DEV)


IGEMM_TOL = 3e-5          # the bound of test_hip_kernels.py::test_igemm_linear_fp8 for the same comparison (same operands, fp32 accumulation)


@pytest.mark.parametrize("K", [128, 384, 416])
@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("M", [16, 272])
def test_igemm_mx_linear(M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M * 3 + N + K)
    a, sa = _random_mx((M,), K, g)
    w, sw = _random_mx((N,), K, g)
    bias = torch.randn(N, generator=g).to(DEV)
    out = torch.full((M, N), float("nan"), device=DEV)
    L.igemm_mx(a, sa, w, sw, M=M, N=N, bias=bias, out_f32=out)
    ref = dequantize_mx(a, sa) @ dequantize_mx(w, sw).T + bias.double()
    e = rel_l2(out, ref)
    print(f"[igemm mx linear {M}x{N}x{K}] vs the fp64 product of the dequantised operands: rel-L2 {e:.2e}")
    assert e < IGEMM_TOL
    if (M, N, K) == (272, 256, 416):                           # the split-K form (debug_flags bit 128: slices whatever the grid)
        ws = torch.full((4 * M * N,), float("nan"), device=DEV)
        out_sk = torch.full((M, N), float("nan"), device=DEV)
        L.igemm_mx(a, sa, w, sw, M=M, N=N, bias=bias, out_f32=out_sk, splitk_ws=ws, debug_flags=128)
        assert bool(torch.isfinite(ws).all())                  # four slices of one K-tile each wrote their slabs
        assert rel_l2(out_sk, ref) < IGEMM_TOL and rel_l2(out_sk, out) < 3e-6      # (slabs summed in slice order: another fp32 order)


@pytest.mark.parametrize("Cin", [32, 64])
def test_igemm_mx_conv3d(Cin):
    B, T, H, W, Cout = 2, 2, 4, 4, 64
    M = B * T * H * W
    g = torch.Generator(device="cpu").manual_seed(Cin)
    a, sa = _random_mx((M,), Cin, g)
    w, sw = _random_mx((27, Cout), Cin, g)
    bias = torch.randn(Cout, generator=g).to(DEV)
    emb = torch.randn(B, Cout, generator=g).to(DEV)
    geom = L.conv_geom(B, (T, H, W), (3, 3, 3))
    kw = dict(M=M, N=Cout, taps=27, geom=geom, bias=bias, rowvec=emb, rows_per_sample=T * H * W)
    out = torch.full((M, Cout), float("nan"), device=DEV)
    L.igemm_mx(a, sa, w, sw, out_f32=out, **kw)
    x = dequantize_mx(a, sa)[:, :Cin].reshape(B, T, H, W, Cin)
    wd = dequantize_mx(w, sw)[:, :, :Cin].permute(1, 2, 0).reshape(Cout, Cin, 3, 3, 3)
    ref = F.conv3d(x.permute(0, 4, 1, 2, 3), wd, bias.double(), padding=1) + emb.double()[:, :, None, None, None]
    ref = ref.permute(0, 2, 3, 4, 1).reshape(M, Cout)
    e = rel_l2(out, ref)
    print(f"[igemm mx conv3d {Cin}->{Cout}] vs the fp64 convolution of the dequantised operands: rel-L2 {e:.2e}")
    assert e < IGEMM_TOL
    ws = torch.full((4 * M * Cout,), float("nan"), device=DEV)
    out_sk = torch.full((M, Cout), float("nan"), device=DEV)
    L.igemm_mx(a, sa, w, sw, out_f32=out_sk, splitk_ws=ws, debug_flags=128, **kw)
    assert bool(torch.isfinite(ws).all())
    assert rel_l2(out_sk, ref) < IGEMM_TOL and rel_l2(out_sk, out) < 3e-6


def test_igemm_mx_conv3d_splits_by_itself():
    """Cin = 256: 54 K-tiles on one 256 x 256 tile, so pd_igemm_mx takes the split-K form (six slices) with no debug flag, as pd_igemm
    does for its e4m3 operands; against the same bound, and against the single-pass form (no workspace)."""
    B, T, H, W, Cin, Cout = 2, 2, 4, 4, 256, 64
    M = B * T * H * W
    g = torch.Generator(device="cpu").manual_seed(Cin)
    a, sa = _random_mx((M,), Cin, g)
    w, sw = _random_mx((27, Cout), Cin, g)
    bias = torch.randn(Cout, generator=g).to(DEV)
    kw = dict(M=M, N=Cout, taps=27, geom=L.conv_geom(B, (T, H, W), (3, 3, 3)), bias=bias)
    out = torch.full((M, Cout), float("nan"), device=DEV)
    L.igemm_mx(a, sa, w, sw, out_f32=out, **kw)
    ws = torch.full((6 * M * Cout,), float("nan"), device=DEV)
    out_sk = torch.full((M, Cout), float("nan"), device=DEV)
    L.igemm_mx(a, sa, w, sw, out_f32=out_sk, splitk_ws=ws, **kw)
    assert bool(torch.isfinite(ws).all())                      # min(CUs / tiles, 54 / 8) = 6 slices, each wrote its slab
    x = dequantize_mx(a, sa).reshape(B, T, H, W, Cin)
    wd = dequantize_mx(w, sw).permute(1, 2, 0).reshape(Cout, Cin, 3, 3, 3)
    ref = F.conv3d(x.permute(0, 4, 1, 2, 3), wd, bias.double(), padding=1).permute(0, 2, 3, 4, 1).reshape(M, Cout)
    print(f"[igemm mx conv3d {Cin}->{Cout}, split by itself] rel-L2 {rel_l2(out_sk, ref):.2e}, single pass {rel_l2(out, ref):.2e}")
    assert rel_l2(out, ref) < IGEMM_TOL and rel_l2(out_sk, ref) < IGEMM_TOL and rel_l2(out_sk, out) < 3e-6


def test_unit_scale_e4m3_launch_is_unchanged_around_an_mx_launch():
    """pd_igemm(fp8=True) gives the same bits before and after an MX launch of the same process (no shared state leaks), and an MX launch
    with every scale byte 127 (2^0) gives those bits too."""
    B, T, H, W, C, Cout = 1, 3, 8, 8, 128, 64
    M = B * T * H * W
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(M, C, generator=g).to(DEV)
    wt = (torch.randn(Cout, C, 3, 3, 3, generator=g) / math.sqrt(27 * C)).to(DEV)
    a8 = to_fp8(x, 16.0)
    w8, sw = pack_conv_fp8(wt)
    geom = L.conv_geom(B, (T, H, W), (3, 3, 3))
    kw = dict(M=M, N=Cout, taps=27, geom=geom, alpha=1.0 / (16.0 * sw))

    def unit():
        o = torch.full((M, Cout), float("nan"), device=DEV)
        L.igemm(a8, w8, Cin=C, w_tap_stride=Cout * C, out_f32=o, fp8=True, **kw)
        return o

    before = unit()
    ones_a = torch.full((M, C // 32), 127, dtype=torch.uint8, device=DEV)
    ones_w = torch.full((27, Cout, C // 32), 127, dtype=torch.uint8, device=DEV)
    o_mx = torch.full((M, Cout), float("nan"), device=DEV)
    L.igemm_mx(a8, ones_a, w8, ones_w, out_f32=o_mx, **kw)
    after = unit()
    assert torch.equal(before, after)
    assert torch.equal(o_mx, before)            # (the fragment layout is the unit-scale kernel's: the same products in the same order)


def test_igemm_mx_refuses_what_it_does_not_run():
    a = torch.zeros(16, 96, dtype=torch.float8_e4m3fn, device=DEV)
    with pytest.raises(L.PrediffHipError):                     # rows of 96 bytes: not whole 128-element K-tiles
        L.igemm_mx(a, torch.zeros(16, 3, dtype=torch.uint8, device=DEV), a, torch.zeros(16, 3, dtype=torch.uint8, device=DEV), M=16, N=16,
                   out_f32=torch.zeros(16, 16, device=DEV))
    a = torch.zeros(16, 128, dtype=torch.float8_e4m3fn, device=DEV)
    with pytest.raises(L.PrediffHipError):                     # scales that do not match the payload
        L.igemm_mx(a, torch.zeros(16, 3, dtype=torch.uint8, device=DEV), a, torch.zeros(16, 4, dtype=torch.uint8, device=DEV), M=16, N=16,
                   out_f32=torch.zeros(16, 16, device=DEV))
