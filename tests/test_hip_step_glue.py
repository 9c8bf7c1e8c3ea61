"""GPU: the glue launches of a denoiser step folded into their neighbours -- every new path against the launches it replaces.

  * the stem GroupNorm (65 channels, one group each) in one launch (gn_narrow_kernel) against the statistics + apply pair;
  * one pd_igemm launch writing the fp32 rows and their 16-bit copy against pd_cast_rows of the fp32 rows; the stem's input builder
    writing its 16-bit copy itself against pd_unet_build_input + pd_cast_rows; the four-column pd_cast_rows against torch's rounding;
  * pd_time_embed against the chain of pd_timestep_embedding / pd_linear_small launches (bit-equal);
  * the per-row table in the convolution epilogue against the convolution followed by pd_add_rowtable (bit-equal);
  * a v1 forward with the Python-side changes (no skip copy, target-frame cuboids only in the last two pairs, and all of the above)
    against the same forward with every switch off, as 32-bit patterns.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------- stem GroupNorm, one launch
def _gn_fp64(x, gamma, beta, G, eps, silu):
    B, S, C = x.shape
    xd = x.double().reshape(B, S, G, C // G)
    mean = xd.mean(dim=(1, 3), keepdim=True)
    var = xd.var(dim=(1, 3), unbiased=False, keepdim=True)
    y = ((xd - mean) / torch.sqrt(var + eps)).reshape(B, S, C) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("S", [3 * 256, 13 * 256])
def test_stem_groupnorm_one_launch_vs_two_launches(S, silu):
    """C = 65 with the stem's 65 groups, B = 2: the one-launch kernel against the two-launch fallback (CallOpts.groupnorm_two_launches),
    both against an fp64 host GroupNorm of the same inputs.  Bound: twice the fallback's own error against that reference (the margin
    covers the other statistics form: fp32 mean and centred squares here, fp64 sums of x and x^2 there).  Both errors are the rounding
    of the result to bfloat16.  Measured on MI355X, rel-L2 against fp64, one launch / two launches:
        S =  768: SiLU 1.643e-03 / 1.643e-03, none 1.653e-03 / 1.653e-03
        S = 3328: SiLU 1.662e-03 / 1.662e-03, none 1.644e-03 / 1.644e-03
    The pad columns [65, 128) are zero in both, and `partials` gives pd_groupnorm_silu_bwd the same (sample, group) statistics."""
    from prediff_amd import _lib as L
    B, C, G, ld, eps = 2, 65, 65, 128, 1e-5
    g = torch.Generator(device="cpu").manual_seed(S + int(silu))
    x = torch.randn(B, S, C, generator=g) * (0.5 + torch.arange(C) * 0.05) + torch.linspace(-3, 3, C)     # per-channel scale and offset
    x[1] += 10.0                                                                                           # a mean far from zero: cancellation shows
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = _gn_fp64(x, gamma, beta, G, eps, silu)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    res = {}
    for name, opts in (("one", L.CallOpts("bf16")), ("two", L.CallOpts("bf16", groupnorm_two_launches=1))):
        out = torch.full((B * S, ld), float("nan"), dtype=torch.bfloat16, device=DEV)
        part = torch.full((B * L.groupnorm_nchunk(S, C) * G * 2,), float("nan"), dtype=torch.float64, device=DEV)
        L.groupnorm_silu(xd, gd, bd, part, out, None, B, S, C, G, ld, eps, silu=silu, opts=opts)
        torch.cuda.synchronize()
        res[name] = (out.float().cpu().reshape(B, S, ld), part.cpu().reshape(B, -1, G, 2).sum(dim=1))
    e_one, e_two = rel_l2(res["one"][0][..., :C], ref), rel_l2(res["two"][0][..., :C], ref)
    print(f"[stem GroupNorm S={S} silu={silu}] rel-L2 vs fp64: one launch {e_one:.3e}, two launches {e_two:.3e}")
    for out, _ in res.values():
        assert bool(torch.isfinite(out).all()) and bool((out[..., C:] == 0).all())
    assert e_one <= 2.0 * e_two
    # the statistics contract: sum and sum of squares per (sample, group), all chunks added
    cnt = S * (C // G)
    for name in ("one", "two"):
        p = res[name][1]
        mean, var = p[..., 0] / cnt, p[..., 1] / cnt - (p[..., 0] / cnt) ** 2
        xr = x.double().reshape(B, S, G, C // G)
        assert torch.allclose(mean, xr.mean(dim=(1, 3)), rtol=0, atol=2e-6 * float(x.abs().max())), name
        assert torch.allclose(var, xr.var(dim=(1, 3), unbiased=False), rtol=2e-5, atol=0), name


# ---------------------------------------------------------------------------------------------------- fp32 rows + their 16-bit copy
@pytest.mark.parametrize("N", [64, 256])
def test_igemm_f32_and_16bit_outputs_in_one_launch(N):
    """M = 300 (a ragged last tile): the 16-bit copy a pd_igemm launch writes next to its fp32 rows is pd_cast_rows of those rows, bit for bit."""
    from prediff_amd import _lib as L
    M, K = 300, 128
    g = torch.Generator(device="cpu").manual_seed(N)
    a = torch.randn(M, K, generator=g).to(DEV).bfloat16().contiguous()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV).bfloat16().contiguous()
    bias, res = torch.randn(N, generator=g).to(DEV), torch.randn(M, N, generator=g).to(DEV)
    o32 = torch.full((M, N), float("nan"), device=DEV)
    o16 = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    L.igemm(a, w, M=M, N=N, Cin=K, bias=bias, residual=res, out_f32=o32, out_bf16=o16)
    c16 = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    L.cast_rows(o32, c16, None, 1, M, 0, M, N, N, N)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o32).all())
    assert rel_l2(o32, a.float() @ w.float().T + bias + res) < 3e-6
    assert torch.equal(o16.view(torch.int16), c16.view(torch.int16))


@pytest.mark.parametrize("B", [1, 3])
def test_build_input16_equals_build_input_then_cast_rows(B):
    """cat([cond, x]) + indicator channel (65 fp32 columns) and, in the same launch, its bfloat16 copy in rows of 128: both equal what
    pd_unet_build_input and pd_cast_rows of its output write, bit for bit (pad columns zero)."""
    from prediff_amd import _lib as L
    T_in, T_out, HW, C, ld16 = 7, 6, 256, 64, 128
    g = torch.Generator(device="cpu").manual_seed(B)
    x, cond = torch.randn(B, T_out, HW, C, generator=g).to(DEV), torch.randn(B, T_in, HW, C, generator=g).to(DEV)
    rows = B * (T_in + T_out) * HW
    ref = torch.full((rows, C + 1), float("nan"), device=DEV)
    L.unet_build_input(x, cond, ref, B, T_in, T_out, HW, C, C + 1)
    ref16 = torch.full((rows, ld16), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.cast_rows(ref, ref16, None, B, (T_in + T_out) * HW, 0, (T_in + T_out) * HW, C + 1, C + 1, ld16)
    out = torch.full((rows, C + 1), float("nan"), device=DEV)
    out16 = torch.full((rows, ld16), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.unet_build_input16(x, cond, out, out16, B, T_in, T_out, HW, C, C + 1, ld16)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(out16.view(torch.int16), ref16.view(torch.int16))
    assert bool((out16[:, C + 1:] == 0).all()) and float(out16[0, C]) == 1.0 and float(out16[-1, C]) == 0.0


@pytest.mark.parametrize("C,ld_out", [(256, 256), (512, 512), (64, 128), (65, 128)])
def test_cast_rows_four_columns_per_thread_rounds_like_torch(C, ld_out):
    """pd_cast_rows on the target rows of each sample (row offset, zero padded columns): round to nearest even, as torch's .bfloat16().
    (65 columns: the scalar kernel; the others: four columns per thread.)"""
    from prediff_amd import _lib as L
    n, rows_in, off, rows_out = 3, 13 * 16, 7 * 16, 6 * 16
    g = torch.Generator(device="cpu").manual_seed(C)
    x = (torch.randn(n, rows_in, C, generator=g) * 3.0).to(DEV)
    x[0, off, :4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.3895e38])      # ties: to even, away from 1.0; a value that rounds to inf
    out = torch.full((n * rows_out, ld_out), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.cast_rows(x, out, None, n, rows_in, off, rows_out, C, C, ld_out)
    torch.cuda.synchronize()
    ref = torch.zeros((n, rows_out, ld_out), dtype=torch.bfloat16, device=DEV)
    ref[..., :C] = x[:, off:off + rows_out].bfloat16()
    assert torch.equal(out.view(torch.int16), ref.reshape(-1, ld_out).view(torch.int16))


# ---------------------------------------------------------------------------------------------------- timestep embedding
@pytest.mark.parametrize("B", [1, 3, 32])
def test_time_embed_bit_equal_to_the_chain(B):
    """sinusoid -> Linear + SiLU -> Linear -> four SiLU -> Linear projections (the v1 widths), t = 0 and t = 999 among the rows: every
    buffer of pd_time_embed equals the chain's, bit for bit."""
    from prediff_amd import _lib as L
    D, E, NS = 256, 1024, (256, 256, 512, 512)
    assert L.time_embed_supported(D, E, len(NS))
    g = torch.Generator(device="cpu").manual_seed(B)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0] = 0
    t[-1] = 999 if B > 1 else 0
    if B == 3:
        t[1] = 999
    t = t.to(DEV)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    freqs = L.timestep_freqs(D, device=DEV)
    w0, b0, w2, b2 = rnd(E, D) / math.sqrt(D), rnd(E), rnd(E, E) / math.sqrt(E), rnd(E)
    proj = [(rnd(n, E) / math.sqrt(E), rnd(n) if i != 1 else None) for i, n in enumerate(NS)]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    # the chain
    sin, h1, temb, outs = nan(B, D), nan(B, E), nan(B, E), [nan(B, n) for n in NS]
    L.timestep_embedding(t, freqs, sin, B, D)
    L.linear_small(sin, w0, b0, h1, B, D, E, act_out="silu")
    L.linear_small(h1, w2, b2, temb, B, E, E)
    for (w, b), o in zip(proj, outs):
        L.linear_small(temb, w, b, o, B, E, o.shape[1], act_in="silu")
    # the fused form
    sin2, h12, temb2, outs2 = nan(B, D), nan(B, E), nan(B, E), [nan(B, n) for n in NS]
    L.time_embed(t, freqs, w0, b0, w2, b2, [(w, b, o) for (w, b), o in zip(proj, outs2)], sin2, h12, temb2, B, D, E)
    torch.cuda.synchronize()
    for name, x, y in [("sin", sin, sin2), ("h1", h1, h12), ("temb", temb, temb2)] + [(f"proj{i}", x, y) for i, (x, y) in enumerate(zip(outs, outs2))]:
        assert bool(torch.isfinite(y).all()), name
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{name}: {int((x != y).sum())} of {x.numel()} values differ"
    assert float(sin[0, 0]) == 1.0 and float(sin[0, D // 2]) == 0.0      # t = 0: cos 1, sin 0


# ---------------------------------------------------------------------------------------------------- row table in the conv epilogue
def _conv_operands(B, T, Cin, Cout, seed):
    from prediff_amd.packing import pack_conv
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B * T * 256, Cin, generator=g).to(DEV).bfloat16().contiguous()
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(27 * Cin)).to(DEV)
    w_p, _ = pack_conv(w, False, dtype=torch.bfloat16)
    bias, res, tab = torch.randn(Cout, generator=g).to(DEV), torch.randn(B * T * 256, Cout, generator=g).to(DEV), torch.randn(T * 256, Cout, generator=g).to(DEV)
    return x, w_p, bias, res, tab


# tile 10: the halo-staged kernel (pipelined epilogue, the launch of the denoiser's stem); 7: the tap-streamed 256 x 256 kernel;
# 1: a 128 x 128 tile (serial epilogue); Cout = 320: a partial last column tile
@pytest.mark.parametrize("tile,Cout", [(10, 256), (7, 256), (1, 256), (10, 320), (0, 64)])
def test_conv_epilogue_row_table_bit_equal_to_add_rowtable(tile, Cout):
    """A 3x3x3 convolution with bias and residual, B = 2, T = 3, 16 x 16 frames: the row table added in the epilogue (row m takes table row
    m % (T * 256)) equals pd_add_rowtable behind the launch, bit for bit -- also in place (residual == output), as the stem runs it."""
    from prediff_amd import _lib as L
    B, T, Cin = 2, 3, 64
    M = B * T * 256
    x, w_p, bias, res, tab = _conv_operands(B, T, Cin, Cout, tile + Cout)
    kw = dict(M=M, N=Cout, Cin=Cin, taps=27, w_tap_stride=Cout * Cin, geom=L.conv_geom(B, (T, 16, 16), (3, 3, 3)), bias=bias, tile=tile)
    two = torch.full((M, Cout), float("nan"), device=DEV)
    L.igemm(x, w_p, residual=res, out_f32=two, **kw)
    plain = two.clone()
    L.add_rowtable(two, tab, B, T * 256, Cout)
    one = torch.full((M, Cout), float("nan"), device=DEV)
    L.igemm(x, w_p, residual=res, out_f32=one, rowtab=tab, **kw)
    inplace = res.clone()
    L.igemm(x, w_p, residual=inplace, out_f32=inplace, rowtab=tab, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(one).all()) and not torch.equal(plain, two)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)), f"{int((one != two).sum())} of {one.numel()} values differ"
    assert torch.equal(inplace.view(torch.int32), two.view(torch.int32))


def test_conv_epilogue_row_table_is_refused_with_a_splitk_workspace():
    from prediff_amd import _lib as L
    B, T, Cin, Cout = 1, 3, 64, 256
    x, w_p, bias, res, tab = _conv_operands(B, T, Cin, Cout, 5)
    out = torch.zeros((B * T * 256, Cout), device=DEV)
    with pytest.raises(L.PrediffHipError, match="row table"):
        L.igemm(x, w_p, M=B * T * 256, N=Cout, Cin=Cin, taps=27, w_tap_stride=Cout * Cin, geom=L.conv_geom(B, (T, 16, 16), (3, 3, 3)), residual=res,
                out_f32=out, rowtab=tab, splitk_ws=torch.zeros(1 << 20, device=DEV))


# ---------------------------------------------------------------------------------------------------- the forward, new paths on / off
SWITCHES = ("fuse_time_embed", "fuse_input_cast", "fuse_pos_epilogue", "skip_no_copy", "tail_target_only")


@pytest.mark.parametrize("split_k", [True, False])
def test_v1_forward_same_bits_with_the_glue_paths_off(split_k):
    """The v1 architecture, B = 2, seeded weights, bf16 engine: the forward with every new path on against the forward with all of them
    switched off (the launches of the parent: the seven-launch embedding chain, pd_add_rowtable, the skip copy, all 13 frames in the
    last two pairs), as 32-bit patterns.  split_k = False is the form large batches run (no split-K workspace: the positional table
    rides in the convolution epilogue); the stem GroupNorm is the same launch in both arms."""
    import _templates as TP
    from _cases import V1_UNET_CFG
    from _weights import seeded_input, seeded_state_dict
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    sd = seeded_state_dict(TP.unet_template(V1_UNET_CFG, "v1_unet_schema.json"), 1234)
    net = CuboidTransformerUNet(**V1_UNET_CFG, precision="bf16")
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.split_k = split_k
    x = seeded_input("gx", (2, 6, 16, 16, 64), 2).cuda()
    cond = seeded_input("gc", (2, 7, 16, 16, 64), 3).cuda()
    t = torch.tensor([999, 0]).cuda()
    assert all(getattr(net, s) is True for s in SWITCHES)
    new = net(x, t, cond).clone()
    for s in SWITCHES:
        setattr(net, s, False)
    old = net(x, t, cond).clone()
    for s in SWITCHES:
        setattr(net, s, True)
    again = net(x, t, cond)
    assert bool(torch.isfinite(new).all())
    assert torch.equal(new.view(torch.int32), old.view(torch.int32)), f"{int((new != old).sum())} of {new.numel()} values differ"
    assert torch.equal(again.view(torch.int32), new.view(torch.int32))
    # the last stack's H-axis and W-axis pairs have a table of the target frames' cuboids: 6 of 13 frames
    tabs = net._tables_dev[x.device][0]
    assert [("tok_tail" in tb, tb["tok_tail"].shape[0] * 13 == tb["tok"].shape[0] * 6 if "tok_tail" in tb else None) for tb in tabs] == \
        [(False, None), (True, True), (True, True)]
