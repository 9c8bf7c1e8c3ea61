"""The border-row skip of the halo-staged Conv3d kernels (csrc/conv3d_halo.hip, tiles 10 and 11): the MFMA row tiles whose sixteen A rows are
all cells of the zero ring (image row 0 at kh = 0, the last image row at kh = 2) are left out of the K-tile loop; debug_flags bit 256 keeps
the dense MFMA schedule.

No GPU: the rule follows from the LDS layout -- from the restated fragment addresses, exactly the (wave row, row tile, kh) the kernel leaves
out read nothing but zero cells for all three kw, and no other does.  GPU: the default launch against the dense one, bit for bit (the
products left out are 0 * w onto accumulators that are never -0), and against F.conv3d at the tolerance of test_conv3d_halo.
"""
import pytest
import torch
import torch.nn.functional as F

from test_conv3d_halo import DEV, TOL, _const, _operands, _run, rel_l2
from test_conv3d_halo_l1 import _cell_pixel, _layout


# ---------------------------------------------------------------------------------------------------- layout (no GPU)
def _all_zero_row_tiles(cell_is_zero, cell_of):
    """{(wave row, row tile, kh)} whose sixteen MFMA rows are zero cells for all three kw"""
    return {(wr, i, kh) for wr in range(2) for i in range(8) for kh in range(3)
            if all(cell_is_zero(cell_of(wr, i, kh, kw, l16)) for kw in range(3) for l16 in range(16))}


def test_level0_zero_row_tiles_follow_from_the_layout():
    fw = _const("FW")
    hw = fw + 2
    assert fw == 16

    def cell_of(wr, i, kh, kw, l16):               # a_rd / 16 + the compile-time offset of LOAD_A: (oh + kh) * 18 + kw + l16
        return (8 * wr + i + kh) * hw + kw + l16

    def is_zero(cell):                             # rows 0 and 17, columns 0 and 17 are the ring
        hr, hc = divmod(cell, hw)
        assert hr < hw
        return hr in (0, hw - 1) or hc in (0, hw - 1)

    # wave row 0 drops its local row tile 0 in phase A of kh = 0, wave row 1 its local row tile 7 (phase B, local 3) in phase B of kh = 2
    assert _all_zero_row_tiles(is_zero, cell_of) == {(0, 0, 0), (1, 7, 2)}


def test_level1_zero_row_tiles_follow_from_the_layout():
    c = _layout()
    rp = c["RP1"]

    def cell_of(wr, i, kh, kw, l16):               # as addr() of test_l1_fragment_reads_hit_the_right_cell_and_are_conflict_free, in cells
        return wr * c["WROW1"] + (l16 >> 3) * c["FPAIR1"] + (l16 & 7) + (i + kh) * rp + kw

    def is_zero(cell):
        assert cell < c["PLROWS1"]
        return _cell_pixel(c, cell) is None

    # both wave rows: row tile 0 in phase A of kh = 0, row tile 7 in phase B of kh = 2
    assert _all_zero_row_tiles(is_zero, cell_of) == {(wr, 0, 0) for wr in range(2)} | {(wr, 7, 2) for wr in range(2)}


# ---------------------------------------------------------------------------------------------------- kernel (GPU)
# (B, T, H, W, Cin, Cout, border_only).  Level 0: both temporal edges in one sample; three samples; T = 1 (every kt but one is skipped as a
# whole group).  Level 1: half a tile (two slots never valid); B * T = 15 (tiles straddle samples) with a ragged N; T = 1.
# border_only: the first and the last image row of every frame are the only non-zero rows -- the row tiles next to the ones left out
# (kh = 1, 2 on row 0; kh = 0, 1 on the last row) then carry all the signal
L0_SHAPES = [(1, 2, 16, 16, 64, 128, False), (3, 2, 16, 16, 64, 128, False), (1, 1, 16, 16, 128, 256, False), (3, 2, 16, 16, 64, 128, True)]
L1_SHAPES = [(1, 2, 8, 8, 64, 128, False), (3, 5, 8, 8, 128, 320, False), (2, 1, 8, 8, 128, 256, False), (3, 5, 8, 8, 128, 320, True)]


def _case(B, T, H, W, Cin, Cout, dtype, border_only):
    x, w, a, w_p = _operands(B, T, H, W, Cin, Cout, dtype)
    if border_only:
        x = x.clone()
        x[:, :, 1:H - 1] = 0
        a = x.reshape(-1, Cin).to(dtype).contiguous()
    ref = F.conv3d(x.to(dtype).float().permute(0, 4, 1, 2, 3), w.to(dtype).float(), None, padding=1).permute(0, 2, 3, 4, 1).reshape(-1, Cout)
    return a, w_p, ref


def _check(tile, dense_flags, B, T, H, W, Cin, Cout, dtype, border_only):
    a, w_p, ref = _case(B, T, H, W, Cin, Cout, dtype, border_only)
    out = _run(a, w_p, B, T, H, W, Cin, Cout, dtype, tile=tile)
    assert bool(torch.isfinite(out).all())
    for flags in dense_flags:
        dense = _run(a, w_p, B, T, H, W, Cin, Cout, dtype, tile=tile, debug_flags=flags)
        assert torch.equal(out, dense), f"debug_flags={flags}"
    e = rel_l2(out, ref)
    print(f"[conv3d border skip tile {tile} {dtype} B={B} {T}x{H}x{W} {Cin}->{Cout} border_only={border_only}] vs F.conv3d {e:.2e}")
    assert e < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,T,H,W,Cin,Cout,border_only", L0_SHAPES)
def test_conv3d_border_skip_level0_equals_dense(B, T, H, W, Cin, Cout, border_only, dtype):
    """bit 256: the dense MFMA schedule; 8 | 256: that and the dense temporal loop (zero halos streamed) -- the same bits all three"""
    _check(10, (256, 8 | 256), B, T, H, W, Cin, Cout, dtype, border_only)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,T,H,W,Cin,Cout,border_only", L1_SHAPES)
def test_conv3d_border_skip_level1_equals_dense(B, T, H, W, Cin, Cout, border_only, dtype):
    _check(11, (256,), B, T, H, W, Cin, Cout, dtype, border_only)
