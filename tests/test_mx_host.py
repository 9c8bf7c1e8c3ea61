"""CPU: the MX (block-scaled e4m3) format and its host side -- the numpy restatement (tests/_mx_ref.py), the weight packers against it
bit for bit, the two precision names of CuboidTransformerUNet and the refusal of widths that are no multiple of 32."""
import numpy as np
import pytest
import torch

import _mx_ref as R
from _cases import TINY_UNET_CFGS
from prediff_amd import _lib as L
from prediff_amd.packing import dequantize_mx, pack_conv_mx, pack_linear_mx, pad128, quantize_mx


def adversarial_rows(rows, K, seed=0):
    """fp32 rows whose 32-element blocks spread over 2^+-20 in magnitude, with an all-zero block, a block whose amax is an exact power of
    two, a block with one 1000x outlier and a block whose amax has a significand above 1.75 (the step of the scale rule)."""
    rng = np.random.default_rng(seed)
    nb = K // 32
    x = rng.standard_normal((rows * nb, 32)) * np.exp2(rng.integers(-20, 21, (rows * nb, 1)))
    n = rows * nb
    slot = (lambda i: i * (n // 4)) if n >= 4 else (lambda i: i)      # the four special blocks, spread over the tensor (fewer where it has fewer blocks)
    if slot(3) < n:
        x[slot(3)] = np.linspace(-1.9, 1.9, 32) * 2.0 ** 5  # amax = 1.9 * 2^5: significand above 1.75
    if slot(2) < n:
        x[slot(2), 3] *= 1000.0                             # one 1000x outlier
    if slot(1) < n:
        x[slot(1)] = rng.uniform(-1, 1, 32)
        x[slot(1), 7] = -4.0                                # amax an exact power of two
    x[0] = 0.0                                              # all-zero block: block 0 of row 0
    return x.reshape(rows, K).astype(np.float32)


@pytest.mark.parametrize("rows,K", [(2, 64), (3, 96), (65, 160)])
def test_mx_ref_round_trip(rows, K):
    x = adversarial_rows(rows, K)
    q, s = R.quantize(x)
    assert q.shape == (rows, K) and s.shape == (rows, K // 32) and q.dtype == s.dtype == np.uint8
    assert not ((q & 0x7F) == 0x7F).any()                   # no NaN code
    assert s.max() <= 254
    d = R.dequantize(q, s)
    scale = np.repeat(np.exp2(s.astype(np.float64) - 127.0), 32, axis=-1)
    xs = x.astype(np.float64) / scale                       # the value the payload rounds
    # no payload saturates: every scaled value lies inside +-448, the block's largest in (224, 448] unless the scale is clamped at byte 0
    assert np.abs(xs).max() <= 448.0
    amax_s = np.abs(xs).reshape(rows, K // 32, 32).max(-1)
    live = (s > 0) & (amax_s > 0)
    assert (amax_s[live] > 224.0).all()
    # e4m3's normal range at that scale (|x| 2^-e >= 2^-6): three mantissa bits, half an ulp = 2^-4 relative
    normal = np.abs(xs) >= 2.0 ** -6
    assert normal.any() and (np.abs(x - d)[normal] <= 2.0 ** -4 * np.abs(x)[normal]).all()
    assert (np.abs(x - d)[~normal] <= 2.0 ** -10 * scale[~normal]).all()      # subnormals: half the quantum 2^-9
    assert (s[0, 0] == 0) and not q[0, :32].any()           # the all-zero block: smallest scale, zero payload
    assert R.dequantize(*R.quantize(d.astype(np.float32)))[normal].tolist() == d[normal].tolist()     # idempotent


def test_mx_ref_padding_and_e4m3_codes():
    x = adversarial_rows(3, 96)
    q, s = R.quantize(x, ld=128)
    assert q.shape == (3, 128) and s.shape == (3, 4) and not q[:, 96:].any() and not s[:, 3].any()
    codes = np.array([b for b in range(256) if (b & 0x7F) != 0x7F], np.uint8)
    assert (R.e4m3_encode(R.e4m3_decode(codes).astype(np.float32)) == codes).all()
    assert (torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy() == R.e4m3_decode(codes)).all()
    # ties go to the even code; values past the top saturate
    assert R.e4m3_encode(np.float32([1.0625, 1.1875, 464.0, 1e9, -1e9])).tolist() == [0x38, 0x3A, 0x7E, 0x7E, 0xFE]


def test_weight_packers_equal_the_reference_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    lw = torch.randn(24, 96, generator=g) * torch.exp2(torch.randint(-12, 13, (24, 1), generator=g).float())
    lw[5, 32:64] = 0.0
    q, s = pack_linear_mx(lw)
    rq, rs = R.quantize(lw.numpy(), ld=128)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.uint8 and tuple(q.shape) == (24, pad128(96)) and tuple(s.shape) == (24, 4)
    assert (q.view(torch.uint8).numpy() == rq).all() and (s.numpy() == rs).all()
    cw = torch.randn(16, 32, 3, 3, 3, generator=g) * torch.exp2(torch.randint(-8, 9, (16, 1, 3, 3, 3), generator=g).float())
    q, s = pack_conv_mx(cw)
    taps = cw.reshape(16, 32, 27).permute(2, 0, 1).contiguous()               # (tap, N, C), taps (kt, kh, kw)-major like pack_conv
    rq, rs = R.quantize(taps.numpy(), ld=128)
    assert tuple(q.shape) == (27, 16, 128) and tuple(s.shape) == (27, 16, 4)
    assert (q.view(torch.uint8).numpy() == rq).all() and (s.numpy() == rs).all()
    assert np.array_equal(dequantize_mx(q, s).numpy(), R.dequantize(rq, rs))
    q2, s2 = quantize_mx(lw, ld=96)
    assert (q2.view(torch.uint8).numpy() == R.quantize(lw.numpy())[0]).all() and (s2.numpy() == R.quantize(lw.numpy())[1]).all()


def test_width_not_a_multiple_of_32_is_refused_naming_the_layer():
    with pytest.raises(L.PrediffHipError, match=r"dte0\.conv1.*multiple of 32"):
        pack_conv_mx(torch.randn(8, 48, 3, 3, 3), "dte0.conv1")
    with pytest.raises(L.PrediffHipError, match=r"ds1\.0\.ffn0\.fc1.*multiple of 32"):
        pack_linear_mx(torch.randn(8, 100), "ds1.0.ffn0.fc1")


def test_precision_mxfp8_constructs_and_packs_wmx_records():
    from prediff_amd import AutoencoderKL, CuboidTransformerUNet
    from _cases import TINY_VAE_CFG
    cpu = torch.device("cpu")
    cfg = dict(TINY_UNET_CFGS["axial"], base_units=256, scale_alpha=1.0, num_heads=4)      # level 1: 512 units, so K >= 512 linears exist
    nets = {p: CuboidTransformerUNet(**cfg, precision=p) for p in ("mxfp8", "mxfp8_conv", "bf16", "fp8", "fp8_conv", "fp16")}
    assert nets["mxfp8"].mx_conv and nets["mxfp8"].mx_linear and nets["mxfp8"].precision == "bf16"
    assert nets["mxfp8_conv"].mx_conv and not nets["mxfp8_conv"].mx_linear and nets["mxfp8_conv"].precision == "bf16"
    assert not nets["mxfp8"].fp8_conv and not nets["mxfp8"].fp8_linear and nets["mxfp8"].op_dtype == torch.bfloat16
    recs = {p: sorted(k for k in n._pack(cpu) if k.endswith(".wmx")) for p, n in nets.items()}
    for p in ("bf16", "fp8", "fp8_conv", "fp16"):
        assert not nets[p].mx_conv and not nets[p].mx_linear and recs[p] == []
    conv = [k for k in recs["mxfp8_conv"]]
    assert conv and all(k.endswith((".conv1.wmx", ".conv2.wmx")) for k in conv)
    assert "dte0.conv1.wmx" in conv and "ute1.conv2.wmx" in conv and "first.conv1.wmx" not in conv      # first.conv1 reads 5 channels: 16-bit
    lin = sorted(set(recs["mxfp8"]) - set(conv))
    assert set(conv) <= set(recs["mxfp8"]) and lin and all(k.endswith((".qkv.wmx", ".fc1.wmx")) for k in lin)      # LayerNorm-fed, K >= 512 only
    assert all(k.startswith(("ds1.", "us1.")) for k in lin)
    P = nets["mxfp8"]._pack(cpu)
    q, s = P["dte1.conv1.wmx"]
    assert q.dtype == torch.float8_e4m3fn and tuple(q.shape) == (27, 512, 512) and tuple(s.shape) == (27, 512, 16) and s.dtype == torch.uint8
    assert not any(k.endswith(".w8") for k in P)
    # the tiny configurations of the GPU tests construct too; the VAE implements neither name
    for p in ("mxfp8", "mxfp8_conv"):
        assert [k for k in CuboidTransformerUNet(**TINY_UNET_CFGS["axial"], precision=p)._pack(cpu) if k.endswith(".wmx")]
        with pytest.raises(ValueError):
            AutoencoderKL(**TINY_VAE_CFG, precision=p)
