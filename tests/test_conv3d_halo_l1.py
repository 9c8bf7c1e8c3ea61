"""The level-1 halo-staged Conv3d form of pd_igemm (tile 11, csrc/conv3d_halo.hip, conv3d_halo_kernel<1>): 8 x 8 frames, a 256-row tile is
four frame slots that may belong to two samples, the halo of a (channel chunk, temporal tap) is the four input frames of that tap.

No GPU: the LDS layout on paper, with the constants read out of the source -- the DMA pieces tile a halo buffer exactly once and every
pixel of the four frames is staged once, every fragment read of every (wave row, row tile, tap, k-step) lands on the cell of the right
(frame slot, image row + kh, column + kw) or on a zero cell, ZERO bank conflicts per ds_read_b128 lane group, the accumulator rows go
back to the right output rows, the LDS budget holds.  GPU: against F.conv3d on the rounded operands and against the tap-streamed kernel
(tile 7) at the tolerance of test_conv3d_halo (TOL = 3e-6, a summation-order effect only); the automatic choice and its A/B switch.
"""
import pytest
import torch
import torch.nn.functional as F

from test_conv3d_halo import DEV, TOL, _conflicts, _const, _operands, _run, rel_l2


# ---------------------------------------------------------------------------------------------------- layout (no GPU)
def _layout():
    c = {k: _const(k) for k in ("FW1", "RP1", "FR1", "FPAIR1", "WROW1", "FREACH1", "PLROWS1")}
    c["base"] = [(f >> 1) * c["WROW1"] + (f & 1) * c["FPAIR1"] for f in range(4)]       # frame_base1()
    return c


def _cell_pixel(c, r):
    """what the staging loop of the kernel puts into halo cell r of a plane: (frame slot, ih, iw), or None = a zero cell"""
    hit = None
    for f in range(4):
        rel = r - c["base"][f]
        hr, hc = divmod(rel, c["RP1"])
        if 0 <= rel < c["FR1"] and hr >= 1 and hc >= 1:
            assert hit is None                      # the interiors of two frames never share a cell
            hit = (f, hr - 1, hc - 1)
    return hit


def test_l1_constants_are_consistent():
    c = _layout()
    fw, rp = c["FW1"], c["RP1"]
    assert fw == 8 and rp == fw + 1 and c["FR1"] == rp * rp and c["WROW1"] == c["FPAIR1"] + c["FR1"]
    assert c["FREACH1"] == (fw + 1) * rp + (fw + 1) + 1                # cell of (hr = 9, hc = 9), plus one
    assert c["FPAIR1"] % 16 == 8                                       # the two image rows of an MFMA row tile: bank quads R .. R+7, R+8 .. R+15
    assert c["base"][3] + c["FREACH1"] <= c["PLROWS1"]


def test_l1_pieces_tile_the_buffer_and_fit_lds():
    c = _layout()
    plrows, fw = c["PLROWS1"], c["FW1"]
    halo = 8 * plrows * 16
    assert (plrows * 16) % 256 == 0 and halo % 1024 == 0
    npiece = halo // 1024
    assert 40 <= npiece <= 48                      # waves 0 .. 7 take pieces w + 8 n, n < 5; the rest (n = 5) goes to waves 0 .. npiece - 41
    seen = set()
    for wave in range(8):
        for n in range(6):
            if wave + 8 * n >= npiece:
                continue
            for lane in range(64):
                s, r = divmod((wave + 8 * n) * 64 + lane, plrows)
                assert s < 8 and (s, r) not in seen
                seen.add((s, r))
    assert len(seen) == 8 * plrows
    pixels = [_cell_pixel(c, r) for r in range(plrows)]
    staged = [p for p in pixels if p is not None]
    assert len(staged) == len(set(staged)) == 4 * fw * fw              # every pixel of the four frames, once per plane
    lds = 2 * halo + 2 * 2 * 128 * 128             # two halos, two W K-tile buffers
    assert 8 * 128 * 32 * 4 <= lds <= 160 * 1024   # the epilogue's accumulator slabs fit; one CU has 160 KB


def test_l1_fragment_reads_hit_the_right_cell_and_are_conflict_free():
    c = _layout()
    fw, rp, plane = c["FW1"], c["RP1"], c["PLROWS1"] * 16

    def addr(wr, i, kh, kw, ks, lane):             # a_rd + the compile-time offset of LOAD_A
        l16, lg = lane & 15, lane >> 4
        return (wr * c["WROW1"] + (l16 >> 3) * c["FPAIR1"] + (l16 & 7)) * 16 + lg * plane + ((i + kh) * rp + kw) * 16 + ks * 4 * plane

    for wr in range(2):
        for i in range(8):
            for kh in range(3):
                for kw in range(3):
                    for ks in range(2):
                        for lane in range(64):
                            s, r = divmod(addr(wr, i, kh, kw, ks, lane) // 16, c["PLROWS1"])
                            assert s == 4 * ks + (lane >> 4) and r < c["PLROWS1"]
                            f, ih, iw = 2 * wr + ((lane & 15) >> 3), i + kh - 1, (lane & 7) + kw - 1
                            want = (f, ih, iw) if 0 <= ih < fw and 0 <= iw < fw else None
                            assert _cell_pixel(c, r) == want
                        assert _conflicts(lambda l: addr(wr, i, kh, kw, ks, l)) == 0
    # the neighbouring-rows form the layout replaces (one row tile = image rows 2 i, 2 i + 1 of one frame at pitch 9): one quad hit twice
    assert _conflicts(lambda l: (((l & 15) >> 3) * rp + (l & 7)) * 16 + (l >> 4) * plane) == 4


def test_l1_accumulator_rows_go_back_to_their_output_rows():
    """MFMA row 4 lg + r of row tile i is pixel (i, (4 lg + r) & 7) of the wave row's frame (4 lg + r) >> 3: row f * 64 + i * 8 + ow of
    the wave row's 128-row slab (c_row + i * 8 + r in the kernel)."""
    rows = set()
    for i in range(8):
        for lg in range(4):
            for r in range(4):
                rho = 4 * lg + r
                row = ((lg >> 1) * 64 + (lg & 1) * 4) + i * 8 + r
                assert row == (rho >> 3) * 64 + i * 8 + (rho & 7)
                rows.add(row)
    assert rows == set(range(128))


# ---------------------------------------------------------------------------------------------------- kernel (GPU)
# (B, T, H, W, Cin, Cout): the level-1 shape at 32 trajectories (104 tiles of four frames, 13 frames per sample: most tiles straddle two
# samples); B = 4, T = 13 (13 whole tiles); T = 1, 2, 3 (every tile straddles, most temporal taps out of range); a partial last column
# tile (N = 320); Cin = 64; B * T no multiple of 4: 15 frames, 13 frames, and 2 / 1 frames (wave row 1 of the only tile at / past M)
SHAPES = [(32, 13, 8, 8, 512, 512), (4, 13, 8, 8, 128, 256), (4, 1, 8, 8, 64, 128), (6, 2, 8, 8, 128, 256), (4, 3, 8, 8, 64, 256),
          (4, 5, 8, 8, 128, 320), (3, 5, 8, 8, 128, 256), (1, 13, 8, 8, 64, 128), (1, 2, 8, 8, 64, 128), (1, 1, 8, 8, 64, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,T,H,W,Cin,Cout", SHAPES)
def test_conv3d_halo_l1_vs_torch_and_tap_streamed(B, T, H, W, Cin, Cout, dtype):
    """Measured on an MI355X, largest of the twenty cases (the level-1 shape, K = 13824, fp16): 1.32e-6 against F.conv3d (the tap-streamed
    kernel: 1.27e-6) and 6.2e-7 against the tap-streamed kernel; TOL of the existing file holds without a wider bound."""
    x, w, a, w_p = _operands(B, T, H, W, Cin, Cout, dtype)
    M = B * T * H * W
    g = torch.Generator(device="cpu").manual_seed(Cout)
    bias, emb, res = torch.randn(Cout, generator=g).to(DEV), torch.randn(B, Cout, generator=g).to(DEV), torch.randn(M, Cout, generator=g).to(DEV)
    kw = dict(bias=bias, rowvec=emb, rows_per_sample=T * H * W, residual=res)
    out = _run(a, w_p, B, T, H, W, Cin, Cout, dtype, tile=11, **kw)
    old = _run(a, w_p, B, T, H, W, Cin, Cout, dtype, tile=7, **kw)
    xs, ws = x.to(dtype).float(), w.to(dtype).float()
    ref = F.conv3d(xs.permute(0, 4, 1, 2, 3), ws, bias, padding=1) + emb[:, :, None, None, None]
    ref = ref.permute(0, 2, 3, 4, 1).reshape(M, Cout) + res
    e_ref, e_old, d = rel_l2(out, ref), rel_l2(old, ref), rel_l2(out, old)
    print(f"[conv3d halo L1 {dtype} B={B} {T}x{H}x{W} {Cin}->{Cout}] vs F.conv3d: halo-staged {e_ref:.2e}, tap-streamed {e_old:.2e}; halo vs tap-streamed {d:.2e}")
    assert bool(torch.isfinite(out).all())
    assert e_ref < TOL
    assert d < TOL                                  # a summation-order effect only


@pytest.mark.gpu
def test_conv3d_halo_l1_dense_bit_is_a_no_op():
    """Level 1 skips no group (a temporal tap is out of range for all four slots of a tile only when T = 1): debug_flags bit 8 changes nothing."""
    B, T, H, W, Cin, Cout = 4, 1, 8, 8, 64, 128
    _, _, a, w_p = _operands(B, T, H, W, Cin, Cout, torch.bfloat16, seed=1)
    out = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=11)
    dense = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=11, debug_flags=8)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,W,Cin,Cout", [(1, 13, 16, 16, 256, 256), (2, 5, 7, 9, 64, 192)])
def test_conv3d_halo_l1_unsupported_shape_falls_back(B, T, H, W, Cin, Cout):
    """Frames that are not 8 x 8 (16 x 16 ones included): tile 11 runs what tile 7 runs -- the same bits."""
    _, _, a, w_p = _operands(B, T, H, W, Cin, Cout, torch.bfloat16)
    out = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=11)
    old = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=7)
    assert torch.equal(out, old)


@pytest.mark.gpu
def test_conv3d_halo_l1_automatic_choice_and_fallback_bit():
    """At 32 trajectories the automatic choice (tile 0) gives the level-1 Conv3d to the halo-staged form (the bits of tile 11); debug_flags
    bit 16 keeps the tap-streamed kernel (the bits of tile 7).  The two differ (another summation order), so the comparison tells them apart."""
    B, T, H, W, Cin, Cout = 32, 13, 8, 8, 512, 512
    _, _, a, w_p = _operands(B, T, H, W, Cin, Cout, torch.bfloat16)
    halo = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=11)
    old = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, tile=7)
    auto = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16)
    auto16 = _run(a, w_p, B, T, H, W, Cin, Cout, torch.bfloat16, debug_flags=16)
    assert not torch.equal(halo, old) and rel_l2(halo, old) < TOL
    assert torch.equal(auto, halo)
    assert torch.equal(auto16, old)
