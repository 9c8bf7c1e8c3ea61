"""Host side of prediff_amd.spectrum (no GPU): the integer binning against a brute-force loop in Python integers and against the
pysteps convention, the constructor's refusals, compute() from a hand-set state, the host-only workspace query, and self-checks of the
fp64 restatement the GPU tests compare against (tests/_spectrum_ref.py)."""
import math
import os
import socket

import numpy as np
import pytest
import torch

import _spectrum_ref as R
from prediff_amd import SEVIRSpectralScore
from prediff_amd import _lib as L
from prediff_amd.spectrum import METRICS, spectrum_bins

SHAPES = [(8, 8), (12, 8), (16, 32), (48, 32), (128, 128), (192, 128), (512, 256)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_spectrum_bins_against_bruteforce(H, W):
    ref = R.bins_bruteforce(H, W)
    bins, order, start, cells = spectrum_bins(H, W)
    nb = max(H, W) // 2 + 1
    assert bins.dtype == np.int64 and bins.shape == (H, W) and np.array_equal(bins, ref)
    assert order.dtype == np.int32 and start.dtype == np.int32 and cells.dtype == np.int64
    assert start.shape == (nb + 1,) and cells.shape == (nb,) and start[0] == 0 and start[-1] == order.size
    assert (cells > 0).all()                                           # no bin is empty at any of these shapes
    assert np.array_equal(np.diff(start), cells)
    kept = np.flatnonzero(ref.reshape(-1) < nb)
    assert np.array_equal(np.sort(order), kept)                        # a permutation of the kept cells ...
    for b in (0, 1, nb // 2, nb - 1):                                  # ... grouped by bin
        assert (ref.reshape(-1)[order[start[b]:start[b + 1]]] == b).all()
    assert (np.diff(ref.reshape(-1)[order]) >= 0).all()
    assert bins[0, 0] == 0 and cells[0] == 1


def test_spectrum_bins_tie_cell():
    """rho = 1.5 exactly: on the 48 x 32 frame the first harmonic of the SHORT side (L / 32 = 1.5) -- floor(rho + 1/2) = 2, which a
    floating-point square root may or may not give.  Both orientations of the frame."""
    assert spectrum_bins(48, 32)[0][0, 1] == 2 and spectrum_bins(48, 32)[0][0, 31] == 2
    assert spectrum_bins(32, 48)[0][1, 0] == 2 and spectrum_bins(32, 48)[0][31, 0] == 2
    assert spectrum_bins(48, 32)[0][1, 0] == 1                         # the long side's first harmonic: rho = 1


@pytest.mark.parametrize("n", [8, 128, 384])
def test_spectrum_bins_square_is_the_pysteps_convention(n):
    """pysteps' rapsd: round(sqrt(xc^2 + yc^2)) on the centred grid; equal below L / 2 (half-integers do not occur: x^2 + y^2 is never
    (m + 1/2)^2)."""
    bins = spectrum_bins(n, n)[0]
    c = np.arange(n) - n // 2                                          # centred (fftshift) coordinates
    rr = np.round(np.sqrt(c[:, None] ** 2.0 + c[None, :] ** 2.0)).astype(np.int64)
    rr = np.fft.ifftshift(rr)
    sel = (bins < n // 2) | (rr < n // 2)
    assert np.array_equal(bins[sel], rr[sel])


def test_spectrum_bins_refuses_odd_sides():
    with pytest.raises(ValueError):
        spectrum_bins(7, 8)


def test_constructor_refusals():
    with pytest.raises(ValueError):
        SEVIRSpectralScore(metrics_list=("psd_pred", "psnr"))
    for layout in ("NTC", "NTHC", "NTWC"):
        with pytest.raises(ValueError):
            SEVIRSpectralScore(layout=layout)
    with pytest.raises(NotImplementedError):
        SEVIRSpectralScore(mode="3")
    for mode in ("1", "2"):
        with pytest.raises(ValueError):
            SEVIRSpectralScore(mode=mode)
    with pytest.raises(ValueError):
        SEVIRSpectralScore(window="hamming")
    m = SEVIRSpectralScore(layout="NHWT", mode="1", seq_len=6, metrics_list=("lsd",), window="hann")
    assert m.metrics_list == ("lsd",) and m.keep_seq_len_dim and m.sums is None
    assert SEVIRSpectralScore().metrics_list == METRICS == ("psd_pred", "psd_target", "coherence", "lsd")


def _hand_state(m, T):
    nb = 5
    rng = np.random.default_rng(3)
    sp, st = rng.uniform(1.0, 2.0, (T, nb)), rng.uniform(1.0, 2.0, (T, nb))
    sx = 0.5 * np.sqrt(sp * st)
    m.sums = torch.tensor(np.stack([sp, st, sx]))
    m.frames = torch.arange(2, 2 + T, dtype=torch.int64)
    m.hw, m.cells = (8, 8), spectrum_bins(8, 8)[3]
    return sp, st, sx


def test_compute_from_a_hand_set_state():
    m1 = SEVIRSpectralScore(mode="1", seq_len=3)
    sp, st, sx = _hand_state(m1, 3)
    cells = m1.cells.astype(np.float64)
    fr = np.array([2.0, 3.0, 4.0])
    out = m1.compute()
    assert set(out) == set(METRICS)
    np.testing.assert_allclose(out["psd_pred"], sp / (fr[:, None] * cells[None]), rtol=1e-15)
    np.testing.assert_allclose(out["psd_target"], st / (fr[:, None] * cells[None]), rtol=1e-15)
    np.testing.assert_allclose(out["coherence"], np.full((3, 5), 0.5), rtol=1e-14)
    lsd = np.sqrt(np.mean((10 * np.log10(sp[:, 1:] / st[:, 1:])) ** 2, axis=1))
    np.testing.assert_allclose(out["lsd"], lsd, rtol=1e-13)
    assert out["psd_pred"].shape == (3, 5) and out["lsd"].shape == (3,)

    m2 = SEVIRSpectralScore(mode="2", seq_len=3, metrics_list=("lsd", "psd_pred"))
    m2.sums, m2.frames, m2.hw, m2.cells = m1.sums, m1.frames, m1.hw, m1.cells
    out2 = m2.compute()
    assert list(out2) == ["lsd", "psd_pred"]
    assert out2["lsd"] == pytest.approx(float(lsd.mean()), rel=1e-13) and out2["psd_pred"].shape == (5,)
    np.testing.assert_allclose(out2["psd_pred"], out["psd_pred"].mean(axis=0), rtol=1e-15)

    m0 = SEVIRSpectralScore(mode="0")
    sp, st, sx = _hand_state(m0, 1)
    out0 = m0.compute()
    assert out0["psd_pred"].shape == (5,) and isinstance(out0["lsd"], float)
    np.testing.assert_allclose(out0["psd_target"], st[0] / (2.0 * cells), rtol=1e-15)
    np.testing.assert_allclose(m0.wavenumber, np.arange(5) / 8.0)
    assert math.isinf(m0.wavelength_px[0]) and m0.wavelength_px[2] == 4.0


def test_empty_state_gives_nan():
    e0 = SEVIRSpectralScore().compute()
    e1 = SEVIRSpectralScore(mode="1", seq_len=4).compute()
    e2 = SEVIRSpectralScore(mode="2", seq_len=4).compute()
    assert math.isnan(e0["lsd"]) and np.isnan(e0["psd_pred"]).all() and np.isnan(e0["coherence"]).all()
    assert e1["lsd"].shape == (4,) and np.isnan(e1["lsd"]).all() and np.isnan(e1["psd_target"]).all()
    assert math.isnan(e2["lsd"])


def test_ws_bytes_without_a_gpu():
    for side in (7, 20, 1024):
        assert L.spectrum_ws_bytes(1, [2, 3, side, 16, 1]) == -1
        assert L.spectrum_ws_bytes(1, [2, 3, 16, side, 1]) == -1
    for H, W in SHAPES:
        one = L.spectrum_ws_bytes(1, [1, 1, H, W, 1])
        assert 0 < one <= L.spectrum_ws_bytes(3, [2, 3, H, W, 2])
        # the partials, and in the strip form (H W > 16384) a complex fp32 frame
        assert one == 24 * (max(H, W) // 2 + 1) + (8 * H * W if H * W > 16384 else 0)
    assert L.spectrum_ws_bytes(0, [2, 3, 16, 16, 1]) == -1 and L.spectrum_ws_bytes(513, [2, 3, 16, 16, 1]) == -1
    assert L.spectrum_ws_bytes(512, [64, 6, 512, 512, 1]) <= 256 << 20           # capped


def test_cpu_tensors_are_refused():
    x = torch.zeros((2, 3, 16, 16, 1))
    with pytest.raises(L.PrediffHipError):
        SEVIRSpectralScore().update(x, x)
    with pytest.raises(L.PrediffHipError):
        SEVIRSpectralScore().update_members(x[None], x)
    with pytest.raises(ValueError):
        SEVIRSpectralScore().update(x, x[:, :1])
    with pytest.raises(ValueError):
        SEVIRSpectralScore().update_members(x, x)
    SEVIRSpectralScore().sync()                                        # no process group: a no-op


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = SEVIRSpectralScore(mode="1", seq_len=2)
        m.hw = (8, 8)                                   # rank 1 made no update: it takes part with a zero state of the group's bins
        if rank == 0:
            m.sums = torch.arange(30, dtype=torch.float64).reshape(3, 2, 5) + 1.0
            m.frames, m.cells = torch.tensor([2, 4], dtype=torch.int64), spectrum_bins(8, 8)[3]
        m.sync()
        q.put((rank, m.sums.tolist(), m.frames.tolist(), m.compute()["psd_pred"].tolist()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sync_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r[0]: r[1:] for r in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sums = (np.arange(30, dtype=np.float64).reshape(3, 2, 5) + 1.0)
    psd = sums[0] / (np.array([2.0, 4.0])[:, None] * spectrum_bins(8, 8)[3][None, :])
    for r in range(2):
        assert got[r][0] == sums.tolist() and got[r][1] == [2, 4], (r, got[r])
        np.testing.assert_allclose(np.array(got[r][2]), psd, rtol=1e-15)


@pytest.mark.parametrize("H,W,window", [(16, 32, "none"), (48, 32, "none"), (12, 8, "hann")])
def test_reference_parseval(H, W, window):
    """sum_b S[b] plus the dropped corners equals sum x^2 (of the windowed frame)."""
    rng = np.random.default_rng(H * W)
    x = rng.uniform(size=(2, H, W)).astype(np.float32)
    bins, nb = R.bins_bruteforce(H, W), max(H, W) // 2 + 1
    s = R.pair_sums(x, x, bins, nb, window)[0]                         # (2, nb)
    xw = x.astype(np.float64) * (R.hann2d(H, W) if window == "hann" else 1.0)
    spec = np.abs(np.fft.fft2(xw)) ** 2 / (H * W)
    corners = spec[:, bins >= nb].sum(axis=1)
    np.testing.assert_allclose(s.sum(axis=1) + corners, (xw ** 2).sum(axis=(1, 2)), rtol=1e-12)
    # ... and through restate / compute: psd * cells * frames is the same sum
    sums, frames = R.restate([(x[:, None, :, :, None], x[:, None, :, :, None])], "NTHWC", False, window)
    cells = np.bincount(bins[bins < nb], minlength=nb)
    pp = R.compute(sums, frames, cells)[0]
    np.testing.assert_allclose((pp * cells * frames[:, None]).sum() + corners.sum(), (xw ** 2).sum(), rtol=1e-12)


def test_reference_identical_frames_are_coherent():
    rng = np.random.default_rng(5)
    x = rng.uniform(size=(2, 3, 16, 32, 1)).astype(np.float32)
    sums, frames = R.restate([(x, x)], "NTHWC", True)
    assert sums.shape == (3, 3, 17) and np.array_equal(frames, [2, 2, 2])
    _, _, coh, lsd = R.compute(sums, frames, spectrum_bins(16, 32)[3])
    np.testing.assert_allclose(coh, 1.0, rtol=1e-12)
    np.testing.assert_allclose(lsd, 0.0, atol=1e-12)
