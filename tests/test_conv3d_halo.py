"""The halo-staged Conv3d form of pd_igemm (tile 10, csrc/conv3d_halo.hip): the 256 x 256 kernel with the 18 x 18 input halo of a
(channel chunk, temporal tap) staged once in LDS and read at nine row shifts, instead of one A tile per filter tap.

No GPU: the LDS layout on paper -- every fragment read of every tap is bank-conflict free under the ds_read_b128 lane groups, the DMA
pieces tile the halo exactly, the LDS budget holds.  GPU: against F.conv3d on the rounded operands and against the tap-streamed kernel
(tile 7), at the one-product tolerance of test_hip_kernels.test_igemm_conv3d (rel-L2 < 3e-6); the automatic choice and its fallbacks.
"""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "prediff_amd", "csrc", "conv3d_halo.hip")
TOL = 3e-6      # test_igemm_conv3d, one-product operands: same 16-bit operands, fp32 accumulate -- only the summation order differs


def _const(name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(SRC).read())
    assert m, name
    return int(m.group(1))


# ---------------------------------------------------------------------------------------------------- layout (no GPU)
# ds_read_b128 is served in four groups of 16 lanes, one LDS cycle each when the 16 lanes touch 64 different banks
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)), list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def _conflicts(addr_of_lane):
    """extra LDS cycles of one ds_read_b128: per lane group, (addresses on the busiest bank) - 1"""
    extra = 0
    for grp in B128_GROUPS:
        banks = {}
        for lane in grp:
            a = addr_of_lane(lane)
            assert a % 16 == 0
            for d in range(4):
                banks.setdefault((a // 4 + d) % 64, set()).add(a)
        extra += max(len(v) for v in banks.values()) - 1
    return extra


def test_halo_fragment_reads_are_conflict_free_for_every_tap():
    plrows, hw = _const("PLROWS"), _const("FW") + 2
    plane = plrows * 16
    assert plane % 256 == 0 and plrows >= hw * hw
    for wr in range(2):
        for i in range(8):
            for kh in range(3):
                for kw in range(3):
                    for ks in range(2):
                        row0 = (wr * 8 + i + kh) * hw + kw
                        assert row0 + 15 < hw * hw
                        assert _conflicts(lambda l: (row0 + (l & 15)) * 16 + (4 * ks + (l >> 4)) * plane) == 0
    # the row-major halo with the W tile's XOR swizzle keyed on the halo row, for comparison: conflict-free only at shifts that are multiples of 4
    xor = lambda r0, ks: _conflicts(lambda l: (r0 + (l & 15)) * 128 + (((4 * ks + (l >> 4)) ^ (((r0 + (l & 15)) >> 1) & 7)) * 16))
    assert xor(0, 0) == 0 and xor(36, 1) == 0 and xor(hw + 1, 0) > 0


def test_halo_pieces_tile_the_buffer_and_fit_lds():
    plrows, fw = _const("PLROWS"), _const("FW")
    hw, halo = fw + 2, 8 * plrows * 16
    assert halo % 1024 == 0
    npiece = halo // 1024
    assert 40 < npiece <= 48                       # waves 0 .. 7 take pieces w + 8 n, n < 5; the rest (n = 5) goes to waves 0 .. npiece - 41
    seen = set()
    for wave in range(8):
        for n in range(6):
            if wave + 8 * n >= npiece:
                continue
            for lane in range(64):
                cell = (wave + 8 * n) * 64 + lane
                s, r = divmod(cell, plrows)
                assert s < 8 and (s, r) not in seen
                seen.add((s, r))
    assert len(seen) == 8 * plrows
    # interior pixels: halo row hr * 18 + hc <-> pixel (hr - 1, hc - 1); everything else (ring, spare rows) is zero-filled
    interior = {(s, r) for (s, r) in seen if r < hw * hw and 1 <= r // hw <= fw and 1 <= r % hw <= fw}
    assert len(interior) == 8 * fw * fw
    lds = 2 * halo + 2 * 2 * 128 * 128             # two halos, two W K-tile buffers
    assert 8 * 128 * 32 * 4 <= lds <= 160 * 1024   # the epilogue's accumulator slabs fit; one CU has 160 KB


# ---------------------------------------------------------------------------------------------------- kernel (GPU)
DEV = "cuda"


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _operands(B, T, H, W, Cin, Cout, dtype, seed=0):
    from prediff_amd.packing import pack_conv
    g = torch.Generator(device="cpu").manual_seed(B + T + Cin + seed)
    x = torch.randn(B, T, H, W, Cin, generator=g)
    x += torch.linspace(-1, 1, W)[:, None] * 0.5 + torch.arange(H)[:, None, None] * 0.05 + torch.arange(T)[:, None, None, None] * 0.03   # position dependent
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(27 * Cin)
    w += torch.arange(27).reshape(3, 3, 3) * (0.02 / math.sqrt(27 * Cin))     # asymmetric taps: a swapped or mirrored shift shows
    x, w = x.to(DEV), w.to(DEV)
    a = x.reshape(-1, Cin).to(dtype).contiguous()
    w_p, _ = pack_conv(w, False, dtype=dtype)
    return x, w, a, w_p


def _run(a, w_p, B, T, H, W, Cin, Cout, dtype, **kw):
    from prediff_amd import _lib as L
    M = B * T * H * W
    out = torch.full((M, Cout), float("nan"), device=DEV)
    opts = L.CallOpts("fp16") if dtype == torch.float16 else None
    L.igemm(a, w_p, M=M, N=Cout, Cin=Cin, taps=27, w_tap_stride=Cout * Cin, geom=L.conv_geom(B, (T, H, W), (3, 3, 3)), out_f32=out, opts=opts, **kw)
    torch.cuda.synchronize()
    return out


# (B, T, H, W, Cin, Cout): the level-0 shape, the skip-concatenated width, an odd tile count with a partial last column tile (N = 320:
# a 64-column remainder; M = B * T * 256 is always whole tiles), T = 1 and T = 2 (every / nearly every temporal tap out of range)
SHAPES = [(1, 13, 16, 16, 256, 256), (2, 13, 16, 16, 512, 256), (3, 5, 16, 16, 128, 320), (2, 1, 16, 16, 128, 256), (3, 2, 16, 16, 64, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,T,H,W,Cin,Cout", SHAPES)
def test_conv3d_halo_vs_torch_and_tap_streamed(B, T, H, W, Cin, Cout, dtype):
    x, w, a, w_p = _operands(B, T, H, W, Cin, Cout, dtype)
    M = B * T * H * W
    g = torch.Generator(device="cpu").manual_seed(Cout)
    bias, emb, res = torch.randn(Cout, generator=g).to(DEV), torch.randn(B, Cout, generator=g).to(DEV), torch.randn(M, Cout, generator=g).to(DEV)
    kw = dict(bias=bias, rowvec=emb, rows_per_sample=T * H * W, residual=res)
    out = _run(a, w_p, B, T, H, W, Cin, Cout, dtype, tile=10, **kw)
    old = _run(a, w_p, B, T, H, W, Cin, Cout, dtype, tile=7, **kw)
    xs, ws = x.to(dtype).float(), w.to(dtype).float()
    ref = F.conv3d(xs.permute(0, 4, 1, 2, 3), ws, bias, padding=1) + emb[:, :, None, None, None]
    ref = ref.permute(0, 2, 3, 4, 1).reshape(M, Cout) + res
    e_ref, e_old, d = rel_l2(out, ref), rel_l2(old, ref), rel_l2(out, old)
    print(f"[conv3d halo {dtype} B={B} {T}x{H}x{W} {Cin}->{Cout}] vs F.conv3d: halo-staged {e_ref:.2e}, tap-streamed {e_old:.2e}; halo vs tap-streamed {d:.2e}")
    assert bool(torch.isfinite(out).all())
    assert e_ref < TOL
    assert d < TOL                                  # a summation-order effect only


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,W,Cin,Cout", SHAPES)
def test_conv3d_halo_tap_skip_equals_dense(B, T, H, W, Cin, Cout):
    """Temporal taps whose input frame is outside the sample are left out as whole (chunk, kt) groups; debug_flags bit 8 streams them as zero
    halos instead: exact zeros added in the same order -- the same bits."""
    _, _, a, w_p = _operands(B, T, H, W, Cin, Cout, torch.bfloat16, seed=1)
    skip = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=10)
    dense = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=10, debug_flags=8)
    assert bool(torch.isfinite(skip).all()) and torch.equal(skip, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,W,Cin,Cout", [(1, 13, 8, 8, 512, 512), (2, 5, 7, 9, 64, 192), (1, 3, 32, 16, 64, 256)])
def test_conv3d_halo_unsupported_shape_falls_back(B, T, H, W, Cin, Cout):
    """Frames that are not 16 x 16: tile 10 runs what tile 7 runs (the tap-streamed kernel) -- the same bits, and right."""
    x, w, a, w_p = _operands(B, T, H, W, Cin, Cout, torch.bfloat16)
    out = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=10)
    old = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=7)
    assert torch.equal(out, old)
    ref = F.conv3d(x.bfloat16().float().permute(0, 4, 1, 2, 3), w.bfloat16().float(), None, padding=1).permute(0, 2, 3, 4, 1).reshape(-1, Cout)
    assert rel_l2(out, ref) < TOL


@pytest.mark.gpu
def test_conv3d_halo_automatic_choice_and_fallback_bit():
    """At 32 trajectories the automatic choice (tile 0) gives the level-0 Conv3d to the 256 x 256 kernel: now its halo-staged form (the bits
    of tile 10); debug_flags bit 16 keeps the tap-streamed kernel (the bits of tile 7).  The two differ (another summation order), so the
    comparison tells them apart."""
    B, T, H, W, Cin, Cout = 32, 13, 16, 16, 256, 256
    _, _, a, w_p = _operands(B, T, H, W, Cin, Cout, torch.bfloat16)
    halo = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=10)
    old = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=7)
    auto = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16)
    auto16 = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, debug_flags=16)
    assert not torch.equal(halo, old) and rel_l2(halo, old) < TOL
    assert torch.equal(auto, halo)
    assert torch.equal(auto16, old)
