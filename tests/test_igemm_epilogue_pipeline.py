"""GPU: the pipelined row passes of the pd_igemm epilogue (csrc/igemm_epilogue.h) against the serial loop they replace.

Every case runs one launch twice -- the default, and debug_flags = 32, which keeps the serial loop -- and asserts (a) torch.equal of
every output: the same operations in the same order per element, so the same bits; (b) the default output against an fp64 torch
evaluation of the same rounded operands, within the bound tests/test_hip_kernels.py uses for that operand type (written at each check).
The shapes are the smallest that reach each path: both fp32 residual-stream writers (in-place residual; per-sample row vector, uniform
and per row), a last tile that ends inside a batch of passes, the modulo of a periodic residual, the scalar column tail, and the
instantiations that keep the loop (gate multiply, 16-bit-only, hi + lo, e4m3 outputs), on the halo-staged, tap-streamed and 128 x 128 kernels.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from prediff_amd import _lib as L  # noqa: E402
from prediff_amd.packing import pack_conv, pack_linear, split_bf16  # noqa: E402

DEV = "cuda"
SERIAL = 32          # debug_flags bit 32: the serial row loop


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def both(launch):
    """launch(debug_flags) -> tuple of output tensors; run the default and the serial arm, assert the same bits, return the default's"""
    new = launch(0)
    old = launch(SERIAL)
    torch.cuda.synchronize()
    for a, b in zip(new, old):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype == torch.float8_e4m3fn else a,
                                                  b.view(torch.uint8) if b.dtype == torch.float8_e4m3fn else b)
        if a.is_floating_point() and a.dtype != torch.float8_e4m3fn:
            assert bool(torch.isfinite(a).all())
    return new


def conv_case(B, T, H, W, Cin, Cout, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, T, H, W, Cin, generator=g)
    x += torch.linspace(-1, 1, W)[:, None] * 0.5 + torch.arange(T)[:, None, None, None] * 0.03
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(27 * Cin)
    w += torch.arange(27).reshape(3, 3, 3) * (0.02 / math.sqrt(27 * Cin))          # asymmetric taps
    bias = torch.randn(Cout, generator=g).to(DEV)
    x, w = x.to(DEV), w.to(DEV)
    a = x.reshape(-1, Cin).to(torch.bfloat16).contiguous()
    w_p, _ = pack_conv(w, False)
    M = B * T * H * W
    conv = F.conv3d(a.double().reshape(B, T, H, W, Cin).permute(0, 4, 1, 2, 3), w.to(torch.bfloat16).double(), bias.double(), padding=1)
    conv = conv.permute(0, 2, 3, 4, 1).reshape(M, Cout)
    kw = dict(M=M, N=Cout, Cin=Cin, taps=27, w_tap_stride=Cout * Cin, geom=L.conv_geom(B, (T, H, W), (3, 3, 3)), bias=bias)
    return a, w_p, kw, conv, g


def linear_case(M, N, K, seed, split=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(M, K, generator=g) + torch.linspace(-1, 1, K)[None, :] * 0.5 + torch.arange(M)[:, None] * 1e-3).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K) + torch.arange(N)[:, None] * 1e-3).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    a_hi, a_lo = split_bf16(x, split)
    w_hi, w_lo = pack_linear(w, split)
    xa = a_hi.double() + (a_lo.double() if split else 0.0)
    wa = w_hi.double() + (w_lo.double() if split else 0.0)
    prod = xa @ wa.reshape(N, -1)[:, :K].t() + bias.double()
    kw = dict(M=M, N=N, Cin=K, bias=bias, A_lo=a_lo, W_lo=w_lo)
    return a_hi, w_hi, kw, prod, g


# ------------------------------------------------------------------------------------------------ the two fp32 residual-stream writers
@pytest.mark.parametrize("tile", [10, 7])
def test_conv3d_l0_in_place_residual(tile):
    """Level-0 Conv3d, out += conv (conv-2 of a residual block): 6 tiles of one frame each, first and last frames tap-skipped; tile 10 =
    halo-staged, tile 7 = the tap-streamed 256 x 256 kernel.  Bound: 3e-6, test_igemm_conv3d (one-product operands)."""
    B, T, H, W, Cin, Cout = 2, 3, 16, 16, 64, 256
    a, w_p, kw, conv, g = conv_case(B, T, H, W, Cin, Cout, 1)
    res = torch.randn(B * T * H * W, Cout, generator=g).to(DEV)

    def launch(flags):
        out = res.clone()
        L.igemm(a, w_p, residual=out, out_f32=out, tile=tile, debug_flags=flags, **kw)
        return (out,)

    out, = both(launch)
    err = rel_l2(out, conv + res.double())
    print(f"[epilogue pipeline: conv3d L0 in place, tile {tile}] rel-L2 vs fp64 {err:.2e}")
    assert err < 3e-6


@pytest.mark.parametrize("tile", [11, 7])
def test_conv3d_l1_rowvec_straddling_samples(tile):
    """Level-1 Conv3d + timestep embedding (conv-1): M = 576, rows_per_sample = 192 -- the 256-row tiles straddle samples (per-row row
    vector), the wave slabs of 128 rows lie inside one sample or not, the last tile stores 64 of 256 rows.  Bound: 3e-6 as above."""
    B, T, H, W, Cin, Cout = 3, 3, 8, 8, 64, 512
    a, w_p, kw, conv, g = conv_case(B, T, H, W, Cin, Cout, 2)
    emb = torch.randn(B, Cout, generator=g).to(DEV)
    M = B * T * H * W

    def launch(flags):
        out = torch.full((M, Cout), float("nan"), device=DEV)
        L.igemm(a, w_p, rowvec=emb, rows_per_sample=T * H * W, out_f32=out, tile=tile, debug_flags=flags, **kw)
        return (out,)

    out, = both(launch)
    err = rel_l2(out, conv + emb.double().repeat_interleave(T * H * W, 0))
    print(f"[epilogue pipeline: conv3d L1 rowvec, tile {tile}] rel-L2 vs fp64 {err:.2e}")
    assert err < 3e-6


@pytest.mark.parametrize("N", [72, 70])
@pytest.mark.parametrize("tile", [1, 0, 5, 7])
def test_linear_row_tail(N, tile):
    """M = 200 on the 128 x 128 kernels (tile 1: batches of 4 passes x 4 rows, the last wave slab stores 8 of 64 rows; tile 5: two
    slabs per wave, four workgroups per CU), the 256 x 256 kernel (tile 7) and the automatic choice (tile 0); N = 72: a partial column tile, N = 70: the scalar
    path.  In place and with a separate residual.  Bound: 2e-6, test_igemm_linear (one-product operands, fp32 output)."""
    M, K = 200, 128
    a, w, kw, prod, g = linear_case(M, N, K, 3)
    res = torch.randn(M, N, generator=g).to(DEV)

    def launch(flags):
        out, out2 = res.clone(), torch.full((M, N), float("nan"), device=DEV)
        L.igemm(a, w, residual=out, out_f32=out, tile=tile, debug_flags=flags, **kw)
        L.igemm(a, w, residual=res, out_f32=out2, tile=tile, debug_flags=flags, **kw)
        return out, out2

    out, out2 = both(launch)
    assert torch.equal(out, out2)
    err = rel_l2(out, prod + res.double())
    print(f"[epilogue pipeline: linear {M}x{N}x{K} tile {tile}] rel-L2 vs fp64 {err:.2e}")
    assert err < 2e-6


@pytest.mark.parametrize("tile", [1, 7])
def test_linear_periodic_residual_and_per_row_rowvec(tile):
    """res_period > 0 with a residual table shorter than M (a positional table), and a per-sample row vector whose samples (50 rows)
    end inside a pass.  Bound: 2e-6, test_igemm_rowvec_alpha_mul_period."""
    M, N, K = 200, 72, 128
    a, w, kw, prod, g = linear_case(M, N, K, 4)
    table = torch.randn(64, N, generator=g).to(DEV)
    emb = torch.randn(4, N, generator=g).to(DEV)

    def launch(flags):
        o1, o2 = (torch.full((M, N), float("nan"), device=DEV) for _ in range(2))
        L.igemm(a, w, residual=table, res_period=64, alpha=0.25, out_f32=o1, tile=tile, debug_flags=flags, **kw)
        L.igemm(a, w, rowvec=emb, rows_per_sample=50, alpha=0.25, out_f32=o2, tile=tile, debug_flags=flags, **kw)
        return o1, o2

    o1, o2 = both(launch)
    bias = kw["bias"].double()
    core = 0.25 * (prod - bias) + bias
    e1 = rel_l2(o1, core + table.double().repeat(4, 1)[:M])
    e2 = rel_l2(o2, core + emb.double().repeat_interleave(50, 0))
    print(f"[epilogue pipeline: periodic residual / per-row rowvec, tile {tile}] rel-L2 vs fp64 {e1:.2e} / {e2:.2e}")
    assert e1 < 2e-6 and e2 < 2e-6


# ------------------------------------------------------------------------------------------------ the instantiations that keep the loop
def test_linear_mul_gate():
    """rowvec, SiLU, gate multiply and residual in one launch (the generic instantiation).  Bound: 2e-6, test_igemm_rowvec_alpha_mul_period."""
    M, N, K = 200, 72, 128
    a, w, kw, prod, g = linear_case(M, N, K, 5)
    mul = torch.randn(M, N, generator=g).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    emb = torch.randn(2, N, generator=g).to(DEV)

    def launch(flags):
        out = torch.full((M, N), float("nan"), device=DEV)
        L.igemm(a, w, rowvec=emb, rows_per_sample=100, mul=mul, residual=res, act="silu", out_f32=out, tile=1, debug_flags=flags, **kw)
        return (out,)

    out, = both(launch)
    ref = F.silu(prod + emb.double().repeat_interleave(100, 0)) * mul.double() + res.double()
    err = rel_l2(out, ref)
    print(f"[epilogue pipeline: mul gate] rel-L2 vs fp64 {err:.2e}")
    assert err < 2e-6


@pytest.mark.parametrize("act", ["none", "gelu"])
def test_linear_16bit_only_output(act):
    """A 16-bit-only producer (8 columns per lane), with and without GELU.  Bound: 4e-3, the bf16 output rounding of test_igemm_linear."""
    M, N, K = 200, 72, 128
    a, w, kw, prod, g = linear_case(M, N, K, 6)

    def launch(flags):
        ob = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        L.igemm(a, w, act=act, out_bf16=ob, tile=1, debug_flags=flags, **kw)
        return (ob,)

    ob, = both(launch)
    ref = F.gelu(prod) if act == "gelu" else prod
    err = rel_l2(ob.float(), ref)
    print(f"[epilogue pipeline: 16-bit only, {act}] rel-L2 vs fp64 {err:.2e}")
    assert err < 4e-3


@pytest.mark.parametrize("tile", [1, 7])
def test_linear_hi_lo_outputs(tile):
    """The precision="fp32" form: hi/lo operands, fp32 and hi + lo 16-bit outputs, residual.  Bounds: 2e-5 (test_igemm_linear, split) for
    the fp32 output, 3e-5 (test_igemm256_hi_lo_bit_equal_to_128) for hi + lo."""
    M, N, K = 200, 72, 128
    a, w, kw, prod, g = linear_case(M, N, K, 7, split=True)
    res = torch.randn(M, N, generator=g).to(DEV)

    def launch(flags):
        out = torch.full((M, N), float("nan"), device=DEV)
        ob = torch.full((2, M, N), 7.0, dtype=torch.bfloat16, device=DEV)
        L.igemm(a, w, residual=res, out_f32=out, out_bf16=ob[0], out_bf16_lo=ob[1], tile=tile, debug_flags=flags, **kw)
        return out, ob

    out, ob = both(launch)
    ref = prod + res.double()
    e1, e2 = rel_l2(out, ref), rel_l2(ob[0].double() + ob[1].double(), ref)
    print(f"[epilogue pipeline: hi + lo outputs, tile {tile}] rel-L2 vs fp64: fp32 {e1:.2e}, hi + lo {e2:.2e}")
    assert e1 < 2e-5 and e2 < 3e-5


def test_linear_e4m3_output():
    """e4m3 operands, e4m3 output (out_fp8_log2 = 4) with GELU.  Bound: test_igemm_fp8_output -- more than 98 % identical bytes and
    2e-2 on the dequantised values against the same statement quantised by torch."""
    from prediff_amd.packing import pack_linear_fp8, to_fp8
    M, N, K = 200, 72, 128
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    bias = (0.2 * torch.randn(N, generator=g)).to(DEV)
    a8, sa = to_fp8(x, 16.0), 16.0
    w8, sw = pack_linear_fp8(w)

    def launch(flags):
        o8 = torch.empty(M, N, dtype=torch.float8_e4m3fn, device=DEV)
        L.igemm(a8, w8, M=M, N=N, Cin=K, bias=bias, act="gelu", alpha=1.0 / (sa * sw), out_bf16=o8, ld_outb=N, fp8=True, out_fp8_log2=4,
                debug_flags=flags)
        return (o8,)

    o8, = both(launch)
    y = F.gelu((a8.float().double() @ w8.float().double().reshape(N, -1)[:, :K].T) / (sa * sw) + bias.double())
    ref = (y * 16.0).clamp(-448, 448).float().to(torch.float8_e4m3fn)
    same = float((o8.view(torch.uint8) == ref.view(torch.uint8)).float().mean())
    err = rel_l2(o8.float(), ref.float())
    print(f"[epilogue pipeline: e4m3 output] identical bytes {same:.4f}, rel-L2 of the dequantised values {err:.2e}")
    assert same > 0.98 and err < 2e-2
