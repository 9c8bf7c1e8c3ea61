"""prediff_amd.spectrum.SEVIRSpectralScore on the device against the fp64 restatement of tests/_spectrum_ref.py (numpy.fft.fft2).

Bound on each of the three sums, per lead time: with beta = 16 * 2^-24 * log2(H W) -- the O(eps log N) normwise error of a floating-point
Cooley-Tukey FFT, doubled for the square, with a constant of 8 --
    sum_b |S - S_ref| <= beta sum_b |S_ref|          and per bin          |S_b - S_ref,b| <= beta (|S_ref,b| + mean_b |S_ref|).
Every parity case prints the kernel's two figures (as fractions of those right sides' unit: normwise relative error, and the largest
per-bin ratio) beside the same figures of torch.fft.fft2 in fp32 on the CPU, and appends the line to the file SPECTRUM_PARITY_LOG names
(scripts/spectrum_parity.py -> profiles/spectrum_parity.log)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import _spectrum_ref as R
from prediff_amd import SEVIRSpectralScore
from prediff_amd import _lib as L
from prediff_amd import spectrum as SP

pytestmark = pytest.mark.gpu


def beta(H, W):
    return 16.0 * 2.0 ** -24 * math.log2(H * W)


@functools.lru_cache(maxsize=None)
def noise(shape, seed=0):
    """seeded uniform noise (pred, target), CPU fp32; shared by the tests, never written to"""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)


@functools.lru_cache(maxsize=None)
def reference(shape, window, keep_seq=True, seed=0):
    p, t = noise(shape, seed)
    s, n = R.restate([(p.numpy(), t.numpy())], "NTHWC", keep_seq, window)
    s.setflags(write=False), n.setflags(write=False)
    return s, n


def fp32_sums(p, t, window):
    """the same sums with torch.fft.fft2 in fp32 on the CPU (products in fp32, the bin sums in fp64): (3, T, nb) for NTHWC, C = 1"""
    N, T, H, W, _ = p.shape
    x, y = p[..., 0].float(), t[..., 0].float()
    if window == "hann":
        w = torch.tensor(R.hann2d(H, W), dtype=torch.float32)
        x, y = x * w, y * w
    P, Tt = torch.fft.fft2(x), torch.fft.fft2(y)
    s = 1.0 / (H * W)
    q = torch.stack([s * (P.real ** 2 + P.imag ** 2), s * (Tt.real ** 2 + Tt.imag ** 2), s * (P.real * Tt.real + P.imag * Tt.imag)])
    bins, nb = R.bins_bruteforce(H, W), max(H, W) // 2 + 1
    idx = np.flatnonzero(bins.reshape(-1) < nb)
    bi = bins.reshape(-1)[idx]
    rows = q.double().numpy().reshape(3 * N * T, H * W)
    out = np.stack([np.bincount(bi, weights=r[idx], minlength=nb) for r in rows]).reshape(3, N, T, nb)
    return out.sum(axis=1)


def figures(got, ref):
    """(normwise relative error, largest per-bin |d| / (|ref_b| + mean |ref|)) over the (3, T') rows of sums"""
    d, a = np.abs(got - ref), np.abs(ref)
    return float((d.sum(axis=-1) / a.sum(axis=-1)).max()), float((d / (a + a.mean(axis=-1, keepdims=True))).max())


def run(shape, window="none", mode="1", seed=0, layout="NTHWC"):
    p, t = noise(shape, seed)
    m = SEVIRSpectralScore(layout=layout, mode=mode, seq_len=shape[1] if mode != "0" else None, window=window)
    m.update(p.cuda(), t.cuda())
    return m


PARITY = [((2, 3, 8, 8, 1), "none"), ((2, 3, 16, 32, 1), "none"), ((2, 3, 16, 32, 1), "hann"), ((2, 3, 12, 8, 1), "none"),
          ((2, 3, 48, 32, 1), "none"), ((2, 3, 128, 128, 1), "none"), ((2, 3, 128, 128, 1), "hann"), ((2, 3, 192, 128, 1), "none"),
          ((1, 1, 384, 384, 1), "none"), ((2, 3, 512, 256, 1), "none")]


@pytest.mark.parametrize("shape,window", PARITY, ids=[f"{s[2]}x{s[3]}-{w}" for s, w in PARITY])
def test_hip_spectrum_parity(shape, window):
    H, W = shape[2], shape[3]
    m = run(shape, window)
    ref, nref = reference(shape, window)
    got = m.sums.cpu().numpy()
    assert got.shape == ref.shape == (3, shape[1], max(H, W) // 2 + 1)
    assert np.array_equal(m.frames.cpu().numpy(), nref)
    kn, kb = figures(got, ref)
    fn, fb = figures(fp32_sums(*noise(shape), window), ref)
    b = beta(H, W)
    line = (f"[spectrum parity] {H}x{W} window={window} N={shape[0]} T={shape[1]}: beta {b:.2e}  kernel normwise {kn:.2e} per-bin {kb:.2e}"
            f"  |  torch.fft.fft2 fp32 (CPU) normwise {fn:.2e} per-bin {fb:.2e}")
    print(line)
    if os.environ.get("SPECTRUM_PARITY_LOG"):
        with open(os.environ["SPECTRUM_PARITY_LOG"], "a") as f:
            f.write(line + "\n")
    assert np.isfinite(got).all()
    assert kn <= b, line
    assert kb <= b, line


# ------------------------------------------------------------------------------------------------ orientation, separation
def _waves(H, W):
    h, w = torch.arange(H, dtype=torch.float64)[:, None], torch.arange(W, dtype=torch.float64)[None, :]
    p = torch.cos(2 * math.pi * (3 * h / H + 5 * w / W)).float()
    t = torch.cos(2 * math.pi * (6 * h / H + 2 * w / W)).float()
    return p.expand(2, 3, H, W)[..., None].contiguous(), t.expand(2, 3, H, W)[..., None].contiguous()


@pytest.mark.parametrize("H,W", [(16, 32), (48, 32)])
def test_hip_spectrum_orientation_and_pair_separation(H, W):
    bins = R.bins_bruteforce(H, W)
    bp, bt = int(bins[3, 5]), int(bins[6, 2])
    assert bp != int(bins[5, 3]) and bp != bt                          # swapping ky and kx moves the bin: the test can see it
    p, t = _waves(H, W)
    ref, _ = R.restate([(p.numpy(), t.numpy())], "NTHWC", False)
    # the reference: H W / 4 per cell, two cells (k and -k), in exactly one bin; 6 pairs
    assert ref[0, 0, bp] == pytest.approx(6 * H * W / 2, rel=1e-6) and ref[1, 0, bt] == pytest.approx(6 * H * W / 2, rel=1e-6)
    m = SEVIRSpectralScore(mode="0")
    m.update(p.cuda(), t.cuda())
    s = m.sums.cpu().numpy()[:, 0]
    assert int(np.argmax(s[0])) == bp and int(np.argmax(s[1])) == bt
    assert s[0, bp] == pytest.approx(ref[0, 0, bp], rel=1e-5) and s[1, bt] == pytest.approx(ref[1, 0, bt], rel=1e-5)
    # a wrong -k index or conjugate in the pair split leaks one field's line into the other's spectrum
    print(f"[spectrum separation] {H}x{W}: S_p at the target's bin / total {abs(s[0, bt]) / s[0].sum():.2e}, "
          f"S_t at the pred's bin / total {abs(s[1, bp]) / s[1].sum():.2e}")
    assert abs(s[0, bt]) <= 1e-9 * s[0].sum()
    assert abs(s[1, bp]) <= 1e-9 * s[1].sum()


def test_hip_spectrum_coherence_and_lsd():
    _, t = noise((2, 3, 16, 32, 1))
    t = t.cuda()
    m = SEVIRSpectralScore(mode="1", seq_len=3)
    m.update(t, t)
    out = m.compute()
    assert np.abs(out["coherence"] - 1.0).max() <= 1e-5 and out["lsd"].max() < 1e-4
    np.testing.assert_allclose(m.wavenumber, np.arange(17) / 32.0)
    assert m.wavelength_px[1] == 32.0 and math.isinf(m.wavelength_px[0])
    m.reset()
    m.update(-t, t)
    assert np.abs(m.compute()["coherence"] + 1.0).max() <= 1e-5
    m.reset()
    m.update(2.0 * t, t)
    out = m.compute()
    assert np.abs(out["lsd"] - 20.0 * math.log10(2.0)).max() <= 1e-4
    assert np.abs(out["coherence"] - 1.0).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ plumbing
def _state(m):
    return m.sums.cpu().numpy(), m.frames.cpu().numpy()


def _close(a, b, rel=1e-12):
    return bool((np.abs(a - b) <= rel * np.abs(b)).all())


def test_hip_spectrum_layouts_are_read_in_place():
    shape = (2, 3, 16, 32, 1)
    p, t = noise(shape)
    base, _ = _state(run(shape))
    # NHWT: the same frames, T innermost
    a = SEVIRSpectralScore(layout="NHWT", mode="1", seq_len=3)
    a.update(p[..., 0].permute(0, 2, 3, 1).contiguous().cuda(), t[..., 0].permute(0, 2, 3, 1).contiguous().cuda())
    assert np.array_equal(_state(a)[0], base)
    # a non-contiguous NTHWC view: every other column and lead time of a wider tensor
    big_p, big_t = torch.zeros((2, 6, 16, 64, 1)), torch.full((2, 6, 16, 64, 1), 7.0)
    big_p[:, ::2, :, ::2], big_t[:, ::2, :, ::2] = p, t
    vp, vt = big_p.cuda()[:, ::2, :, ::2], big_t.cuda()[:, ::2, :, ::2]
    assert not vp.is_contiguous()
    b = SEVIRSpectralScore(mode="1", seq_len=3)
    b.update(vp, vt)
    assert np.array_equal(_state(b)[0], base)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hip_spectrum_16_bit_inputs_are_read_as_float(dtype):
    p, t = noise((2, 3, 16, 32, 1))
    p, t = p.to(dtype).cuda(), t.to(dtype).cuda()
    a, b = (SEVIRSpectralScore(mode="1", seq_len=3) for _ in range(2))
    a.update(p, t)
    b.update(p.float(), t.float())
    assert np.array_equal(_state(a)[0], _state(b)[0])
    ref, _ = R.restate([(p.float().cpu().numpy(), t.float().cpu().numpy())], "NTHWC", True)
    assert figures(_state(a)[0], ref)[0] <= beta(16, 32)


def test_hip_spectrum_channels_are_frames():
    g = torch.Generator().manual_seed(7)
    p, t = torch.rand((2, 3, 16, 32, 2), generator=g), torch.rand((2, 3, 16, 32, 2), generator=g)
    m = SEVIRSpectralScore(mode="1", seq_len=3)
    m.update(p.cuda(), t.cuda())
    s, n = _state(m)
    ref, nref = R.restate([(p.numpy(), t.numpy())], "NTHWC", True)
    assert np.array_equal(n, nref) and np.array_equal(n, [4, 4, 4])
    kn, kb = figures(s, ref)
    assert kn <= beta(16, 32) and kb <= beta(16, 32)


def test_hip_spectrum_modes_are_consistent():
    shape = (2, 3, 16, 32, 1)
    m0, m1, m2 = run(shape, mode="0"), run(shape, mode="1"), run(shape, mode="2")
    (s0, n0), (s1, n1), (s2, n2) = _state(m0), _state(m1), _state(m2)
    assert s0.shape == (3, 1, 17) and s1.shape == (3, 3, 17) and np.array_equal(s1, s2)
    assert n0.tolist() == [6] and n1.tolist() == [2, 2, 2]
    assert _close(s1.sum(axis=1, keepdims=True), s0)
    o0, o1, o2 = m0.compute(), m1.compute(), m2.compute()
    assert o0["psd_pred"].shape == (17,) and o1["psd_pred"].shape == (3, 17) and o1["lsd"].shape == (3,)
    for k in ("psd_pred", "psd_target", "coherence"):
        np.testing.assert_allclose(o2[k], o1[k].mean(axis=0), rtol=1e-14)
    assert o2["lsd"] == pytest.approx(float(o1["lsd"].mean()), rel=1e-14)
    np.testing.assert_allclose(o0["psd_pred"], o1["psd_pred"].mean(axis=0), rtol=1e-12)      # equal frames per lead time


def test_hip_spectrum_accumulation_members_and_bits():
    shape = (2, 3, 16, 32, 1)
    p, t = (x.cuda() for x in noise(shape))
    p2, t2 = (x.cuda() for x in noise(shape, seed=1))
    a, b = (SEVIRSpectralScore(mode="1", seq_len=3) for _ in range(2))
    a.update(p, t)
    a.update(p2, t2)
    b.update(torch.cat([p, p2]), torch.cat([t, t2]))
    assert _close(_state(a)[0], _state(b)[0]) and np.array_equal(_state(a)[1], _state(b)[1]) and _state(a)[1].tolist() == [4, 4, 4]
    # three members against one target = three updates
    p3 = noise(shape, seed=2)[0].cuda()
    ens = torch.stack([p, p2, p3])
    c, d = (SEVIRSpectralScore(mode="1", seq_len=3) for _ in range(2))
    c.update_members(ens, t)
    for i in range(3):
        d.update(ens[i], t)
    assert _close(_state(c)[0], _state(d)[0]) and np.array_equal(_state(c)[1], _state(d)[1]) and _state(c)[1].tolist() == [6, 6, 6]
    ref, _ = R.restate([(ens.cpu().numpy(), t.cpu().numpy())], "NTHWC", True)
    assert figures(_state(c)[0], ref)[0] <= beta(16, 32)
    with pytest.raises(ValueError):
        c.update_members(torch.zeros((513, 1, 1, 8, 8, 1), device="cuda"), torch.zeros((1, 1, 8, 8, 1), device="cuda"))
    # the same call twice from reset(): the same bits
    first = _state(c)[0].copy()
    c.reset()
    assert c.sums is None and math.isnan(c.compute()["lsd"][0])
    c.update_members(ens, t)
    assert np.array_equal(_state(c)[0], first)


def test_hip_spectrum_strip_form_in_two_chunks(monkeypatch):
    """A strip-form call whose workspace cap holds 3 of its 6 pairs equals the same pairs given in two calls."""
    shape = (2, 3, 192, 128, 1)
    p, t = (x.cuda() for x in noise(shape))
    one = L.spectrum_ws_bytes(1, [1, 1, 192, 128, 1])
    assert one > 8 * 192 * 128 and L.spectrum_ws_bytes(1, list(shape)) == 6 * one
    whole, _ = _state(run(shape))
    monkeypatch.setattr(SP, "WS_CAP_BYTES", 3 * one + 8)
    a, b = (SEVIRSpectralScore(mode="1", seq_len=3) for _ in range(2))
    a.update(p, t)
    assert a._ws.numel() * 8 < 4 * one                                 # the workspace holds 3 pairs: two chunks
    b.update(p[:1], t[:1])                                             # pairs are ordered n-major: these are the first chunk's
    b.update(p[1:], t[1:])
    assert _close(_state(a)[0], _state(b)[0]) and np.array_equal(_state(a)[1], _state(b)[1])
    assert _close(_state(a)[0], whole)
    ref, nref = reference(shape, "none")
    assert np.array_equal(_state(a)[1], nref) and figures(_state(a)[0], ref)[0] <= beta(192, 128)


def test_hip_spectrum_nan_stays_in_its_lead_time():
    shape = (2, 3, 16, 32, 1)
    p, t = noise(shape)
    clean, _ = _state(run(shape))
    q = p.clone()
    q[1, 1, 5, 7, 0] = float("nan")
    m = SEVIRSpectralScore(mode="1", seq_len=3)
    m.update(q.cuda(), t.cuda())
    s, _ = _state(m)
    assert np.isnan(s[:, 1]).all()                                     # pred and target travel as one complex frame: all three sums
    assert np.array_equal(s[:, 0], clean[:, 0]) and np.array_equal(s[:, 2], clean[:, 2])
    out = m.compute()
    assert np.isnan(out["lsd"]).tolist() == [False, True, False]


def test_hip_spectrum_refuses_side_20():
    x = torch.zeros((1, 1, 20, 16, 1), device="cuda")
    m = SEVIRSpectralScore()
    with pytest.raises(L.PrediffHipError, match="20"):
        m.update(x, x)
    assert m.sums is None
