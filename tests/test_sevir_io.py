"""The SEVIR pixel front end on the device (prediff_amd/sevir_io.py, csrc/sevir_io.hip): pd_sevir_ingest and pd_sevir_export
against the numpy restatement in tests/_sevir_io_ref.py (and the reference's own outputs in tests/golden/sevir_io.npz), bit for bit:
every comparison is torch.equal / np.array_equal, since each value is one rounding per operation.  Outputs the wrapper allocates cannot
carry guard rows; the kernel-level cases below call the binding on NaN-filled buffers between guards."""
import functools

import numpy as np
import pytest
import torch

import _sevir_io_ref as R
import _templates as TP
from _cases import TINY_UNET_CFGS, TINY_VAE_CFG
from _weights import seeded_state_dict
from prediff_amd import SEVIRFrontEnd

pytestmark = pytest.mark.gpu

RESCALES = ("01", "sevir")
GUARD = 64


def _events(shape, seed, block=(3, 3)):
    """uint8 events (N, H, W, T) holding every byte value (when they have 256 cells) in a seeded order, and, in frame 0 of event 0, fh x fw
    blocks of small values whose maximum (255) sits in each of the fh * fw positions in turn (as many as the frame has blocks)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    raw = rng.permutation(np.arange(n) % 256).astype(np.uint8).reshape(shape)
    fh, fw = block
    by, bx = shape[1] // fh, shape[2] // fw
    for p in range(min(fh * fw, by * bx)):
        y0, x0 = (p // bx) * fh, (p % bx) * fw
        raw[0, y0:y0 + fh, x0:x0 + fw, 0] = rng.integers(0, 200, size=(fh, fw))
        raw[0, y0 + p // fw, x0 + p % fw, 0] = 255
    return raw


def _check_ingest(raw, factors, in_len, out_len, starts, rescale, offset_bytes=0):
    """fe.ingest on a device copy of `raw` that starts `offset_bytes` past an allocation, against the restatement"""
    fe = SEVIRFrontEnd(in_len=in_len, out_len=out_len, factors=factors, rescale=rescale)
    flat = torch.zeros(offset_bytes + raw.size, dtype=torch.uint8, device="cuda")
    dev = flat[offset_bytes:].view(raw.shape)
    dev.copy_(torch.from_numpy(raw))
    ctx, tgt = fe.ingest(dev, starts=starts)
    rc, rt = R.ingest(raw, factors, rescale, in_len, out_len, starts)
    label = (raw.shape, factors, in_len, out_len, starts, rescale, offset_bytes)
    assert ctx.dtype == tgt.dtype == torch.float32 and ctx.shape == rc.shape and tgt.shape == rt.shape, label
    assert torch.equal(ctx.cpu(), torch.from_numpy(rc)), label
    assert torch.equal(tgt.cpu(), torch.from_numpy(rt)), label
    assert torch.equal(dev.cpu(), torch.from_numpy(raw)), label               # the events are only read
    return ctx, tgt


# ------------------------------------------------------------------------------------------------ ingest
@pytest.mark.parametrize("rescale", RESCALES)
def test_ingest_nothing_aligned(rescale):
    """raw (2, 6, 9, 5), factors (2, 3, 3): odd T, one block row, three segments of 45 bytes; the events at every offset 0 .. 16 inside a
    16-byte granule (heads of 0 .. 15 bytes, tails likewise; one chunk per row).  The six blocks of frame 0 carry their maximum in positions 0 .. 5."""
    raw = _events((2, 6, 9, 5), 1)
    assert [int(np.argmax(raw[0, (p // 3) * 3:(p // 3) * 3 + 3, (p % 3) * 3:(p % 3) * 3 + 3, 0])) for p in range(6)] == list(range(6))
    for off in range(17):
        _check_ingest(raw, (2, 3, 3), 2, 1, (0,), rescale, offset_bytes=off)


def test_ingest_max_in_each_block_position():
    """All 9 positions of a 3 x 3 block (the 6 x 9 case above has six blocks): a 9 x 9 frame."""
    raw = _events((1, 9, 9, 3), 2)
    assert sorted(int(np.argmax(raw[0, (p // 3) * 3:(p // 3) * 3 + 3, (p % 3) * 3:(p % 3) * 3 + 3, 0])) for p in range(9)) == list(range(9))
    for rescale in RESCALES:
        ctx, _ = _check_ingest(raw, (2, 3, 3), 2, 0, (0,), rescale)
        assert torch.equal(ctx[0, 0, :, :, 0].cpu(), torch.from_numpy(R.forward(np.full((3, 3), 255, np.uint8), rescale)))


@pytest.mark.parametrize("rescale", RESCALES)
def test_ingest_three_windows(rescale):
    """raw (1, 12, 12, 49): 25 LR frames, windows at 0, 6 and 12 of 7 + 6 frames, the last ending on LR frame 24 (raw frame 48, the last)."""
    raw = _events((1, 12, 12, 49), 3)
    assert len(np.unique(raw)) == 256
    ctx, tgt = _check_ingest(raw, (2, 3, 3), 7, 6, (0, 6, 12), rescale)
    assert ctx.shape == (3, 7, 4, 4, 1) and tgt.shape == (3, 6, 4, 4, 1)
    assert torch.equal(ctx[1, :1], ctx[0, -1:]) and torch.equal(ctx[2, :1], tgt[0, -1:])       # LR frames 6 and 12, seen by two windows


@pytest.mark.parametrize("factors", [(1, 1, 1), (3, 2, 4)])
@pytest.mark.parametrize("rescale", RESCALES)
def test_ingest_identity_and_unequal_factors(factors, rescale):
    """raw (3, 8, 16, 7): the full-resolution path (1, 1, 1) and unequal factors (3, 2, 4) (T_lr = 3); N = 3; with and without a target."""
    raw = _events((3, 8, 16, 7), 4, block=factors[1:])
    T_lr = -(-7 // factors[0])
    _check_ingest(raw, factors, T_lr - 1, 1, (0,), rescale)
    _check_ingest(raw, factors, 1, 1, tuple(range(T_lr - 1)), rescale, offset_bytes=5)
    ctx, tgt = _check_ingest(raw, factors, T_lr, 0, (0,), rescale)             # out_len = 0: the library gets a null target
    assert tgt.shape == (3, 0, 8 // factors[1], 16 // factors[2], 1) and tgt.numel() == 0


def test_ingest_reference_fixture(golden):
    """The reference's own preprocess_data_dict output (tests/golden/sevir_io.npz), factors (1, 1, 1)."""
    g = golden("sevir_io")
    for rescale in RESCALES:
        fe = SEVIRFrontEnd(in_len=10, out_len=6, factors=(1, 1, 1), rescale=rescale)
        ctx, tgt = fe.ingest(torch.from_numpy(g["raw"]).cuda())
        assert torch.equal(torch.cat([ctx, tgt], dim=1).cpu(), torch.from_numpy(g[f"pre_{rescale}"])), rescale
        back = fe.export(torch.from_numpy(g["frames"]).cuda(), dtype=torch.float32)
        assert torch.equal(back.cpu(), torch.from_numpy(g[f"back_{rescale}"])), rescale


def test_ingest_wide_rows_take_the_chunked_path():
    """Rows of W T = 1404 * 49 = 68 796 bytes: the kernel cuts the row along W into pieces whose fh segments fit its LDS budget (two
    segments per workgroup, each with its own head and tail; W' = 702 cells in six chunks of 101 and one of 96) -- at offsets 0 and 7."""
    raw = _events((1, 4, 1404, 49), 5, block=(2, 2))
    for off in (0, 7):
        _check_ingest(raw, (2, 2, 2), 7, 6, (0, 12), "01", offset_bytes=off)
    raw1 = _events((2, 2, 1400, 49), 6, block=(1, 1))                          # fh = 1: one segment per workgroup, four chunks of 350
    _check_ingest(raw1, (1, 1, 1), 2, 1, (46,), "sevir", offset_bytes=3)


def test_ingest_guards_and_bad_window():
    """The binding on NaN-filled outputs between guards: every element written, nothing around them; a window outside the event (the
    library cannot read the table) is written as zeros."""
    from prediff_amd import _lib as L
    raw = _events((2, 6, 9, 5), 7)
    dev = torch.from_numpy(raw).cuda()
    N, nwin, in_len, out_len, Hl, Wl = 2, 3, 2, 1, 2, 3
    starts = torch.tensor([0, 1, -1], dtype=torch.int32, device="cuda")       # T_lr = 3: only 0 is inside
    bufs = []
    for T in (in_len, out_len):
        n = N * nwin * T * Hl * Wl
        flat = torch.full((GUARD + n + GUARD,), float("nan"), device="cuda")
        bufs.append((flat, flat[GUARD:GUARD + n].view(N * nwin, T, Hl, Wl, 1)))
    (cf, ctx), (tf, tgt) = bufs
    L.sevir_ingest(dev, starts, ctx, tgt, 2, 6, 9, 5, (2, 3, 3), nwin, in_len, out_len, 1 / 255, 0.0)
    rc, rt = R.ingest(raw, (2, 3, 3), "01", in_len, out_len, (0,))
    for flat, out, ref in ((cf, ctx, rc), (tf, tgt, rt)):
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
        o = out.view(N, nwin, *out.shape[1:]).cpu()
        assert torch.equal(o[:, 0], torch.from_numpy(ref)) and bool((o[:, 1:] == 0).all())


@pytest.mark.parametrize("rescale", RESCALES)
def test_ingest_v1_size(rescale):
    """Two events at the public size, (384, 384, 49), default factors: 128 x 128 cells, rows cut into chunks of 43, 43 and 42 cells."""
    rng = np.random.default_rng(8)
    raw = rng.integers(0, 256, size=(2, 384, 384, 49), dtype=np.uint8)
    ctx, tgt = _check_ingest(raw, (2, 3, 3), 7, 6, (12,), rescale, offset_bytes=9)
    assert ctx.shape == (2, 7, 128, 128, 1) and tgt.shape == (2, 6, 128, 128, 1)


# ------------------------------------------------------------------------------------------------ export
def _export_values(rescale, shape=(2, 3, 7, 11, 1)):
    """fp32 frames whose VIL value is: k + 0.5 for k = -2 .. 257, built on the VIL scale (scale * (k + 0.5 + offset), or the float within
    4 ulps of it that the restatement takes back to k + 0.5 exactly, where there is one), values below 0 and above 255, the largest finite
    floats, infinities, a subnormal, and seeded values around [0, 1]."""
    scale, offset = (np.float32(v) for v in R.RESCALE[rescale])
    want = np.arange(-2, 258, dtype=np.float32) + np.float32(0.5)
    ties = scale * (want + offset)
    for d in (1, 2, 3, 4):
        for side in (np.float32(np.inf), np.float32(-np.inf)):
            cand = ties.copy()
            for _ in range(d):
                cand = np.nextafter(cand, side)
            fix = (R.back(ties, rescale) != want) & (R.back(cand, rescale) == want)
            ties[fix] = cand[fix]
    extremes = np.array([-1.0, -1e-3, 0.0, 1.0, 1.0001, 2.0, 300.0, -300.0, 3.4e38, -3.4e38, np.inf, -np.inf, 1e-45, 255.0, 254.5 / 255],
                        dtype=np.float32)
    rng = np.random.default_rng(9)
    n = int(np.prod(shape))
    body = rng.uniform(-0.1, 1.1, size=n).astype(np.float32)
    if rescale == "sevir":
        body = scale * (body * np.float32(255) + offset)
    head = np.concatenate([ties, extremes])
    body[:head.size] = head[:n]
    return body.reshape(shape)


@pytest.mark.parametrize("rescale", RESCALES)
def test_export_ties_extremes_layouts(rescale):
    """(2, 3, 7, 11, 1) = 462 elements: not a multiple of 4 (the tail group), both byte layouts and fp32, at an aligned base and one float off."""
    fe = SEVIRFrontEnd(rescale=rescale)
    x = _export_values(rescale)
    v = R.back(x, rescale)
    fin = v[np.isfinite(v)]
    print(f"export {rescale}: {int(((fin - np.floor(fin)) == 0.5).sum())} exact ties of 260")
    assert int(((fin - np.floor(fin)) == 0.5).sum()) >= 200 and bool((v < 0).any()) and bool((v > 255).any())   # ties reach the rounding
    for mis in (0, 1):
        flat = torch.zeros(x.size + 4 + mis, device="cuda")
        dev = flat[4 + mis:].view(x.shape)
        dev.copy_(torch.from_numpy(x))
        assert dev.data_ptr() % 16 == 4 * mis
        for layout in ("NTHW", "NHWT"):
            out = fe.export(dev, dtype=torch.uint8, layout=layout)
            ref = R.export(x, rescale, "uint8", layout)
            assert out.dtype == torch.uint8 and out.shape == ref.shape and torch.equal(out.cpu(), torch.from_numpy(ref)), (layout, mis)
        assert torch.equal(fe.export(dev).cpu(), torch.from_numpy(R.export(x, rescale)))                     # the defaults: uint8 NTHW
        f = fe.export(dev, dtype=torch.float32)
        ref = R.export(x, rescale, "float32")
        assert f.shape == x.shape and np.array_equal(f.cpu().numpy(), ref, equal_nan=True), mis
        assert torch.equal(dev.cpu(), torch.from_numpy(x))


def test_export_guards():
    """The binding on guarded outputs at byte offsets 0 .. 4 (the packed store needs 4-byte alignment, the others go byte by byte)."""
    from prediff_amd import _lib as L
    x = _export_values("01", (1, 6, 5, 11, 1))
    dev = torch.from_numpy(x).cuda()
    for mode, layout in ((1, "NTHW"), (2, "NHWT")):
        ref = torch.from_numpy(R.export(x, "01", "uint8", layout)).reshape(-1)
        for off in range(5):
            flat = torch.full((GUARD + off + x.size + GUARD,), 77, dtype=torch.uint8, device="cuda")
            out = flat[GUARD + off:GUARD + off + x.size]
            L.sevir_export(dev, out, 1, 6, 5, 11, 1 / 255, 0.0, mode)
            assert torch.equal(out.cpu(), ref), (layout, off)
            assert bool((flat[:GUARD + off] == 77).all()) and bool((flat[GUARD + off + x.size:] == 77).all()), (layout, off)
    flat = torch.full((GUARD + x.size + GUARD,), float("nan"), device="cuda")
    L.sevir_export(dev, flat[GUARD:GUARD + x.size], 1, 6, 5, 11, 1 / 255, 0.0, 0)
    assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
    assert np.array_equal(flat[GUARD:GUARD + x.size].cpu().numpy(), R.export(x, "01", "float32").reshape(-1))


@pytest.mark.parametrize("rescale", RESCALES)
def test_round_trip(rescale):
    """export(ingest(raw)) returns the pooled bytes exactly, in both layouts.  Asserted for "sevir" too: the restatement round-trips all
    256 values in both modes (tests/test_sevir_io_host.py::test_restatement_round_trip)."""
    raw = _events((2, 12, 12, 49), 10)
    fe = SEVIRFrontEnd(in_len=25, out_len=0, rescale=rescale)
    ctx, _ = fe.ingest(torch.from_numpy(raw).cuda())
    pooled = R.pool(raw, (2, 3, 3))                                            # (N, H', W', T')
    assert torch.equal(fe.export(ctx, layout="NHWT").cpu(), torch.from_numpy(pooled))
    assert torch.equal(fe.export(ctx, layout="NTHW").cpu(), torch.from_numpy(np.ascontiguousarray(np.transpose(pooled, (0, 3, 1, 2)))))
    full = SEVIRFrontEnd(in_len=1, out_len=0, factors=(1, 1, 1), rescale=rescale)      # every byte value, unpooled
    b = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).cuda()
    assert torch.equal(full.export(full.ingest(b)[0], layout="NHWT"), b)


# ------------------------------------------------------------------------------------------------ capture, end to end
def test_graph_capture():
    """Both launches captured in one graph and replayed on new input give the eager result (the start table is uploaded by the eager
    call before the capture; outputs come from the graph's pool)."""
    fe = SEVIRFrontEnd(in_len=2, out_len=1)
    a, b = (torch.from_numpy(_events((2, 6, 9, 9), s)).cuda() for s in (11, 12))
    eager = [(*fe.ingest(r, starts=(0, 2)), fe.export(fe.ingest(r, starts=(0, 2))[1], layout="NHWT")) for r in (a, b)]
    assert not torch.equal(eager[0][0], eager[1][0])
    static = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx, tgt = fe.ingest(static, starts=(0, 2))
        vil = fe.export(tgt, layout="NHWT")
    for r, ref in ((b, eager[1]), (a, eager[0])):
        static.copy_(r)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ctx, ref[0]) and torch.equal(tgt, ref[1]) and torch.equal(vil, ref[2])


@functools.lru_cache(maxsize=None)
def _tiny_ldm():
    from prediff_amd.autoencoder_kl import AutoencoderKL
    from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet
    from prediff_amd.latent_diffusion import LatentDiffusion
    cfg = TINY_UNET_CFGS["axial"]                                              # T_in = 3, T_out = 2, latent 8 x 8 x 4: 32 x 32 pixels
    net = CuboidTransformerUNet(**cfg, precision="bf16")
    net.load_state_dict(seeded_state_dict(TP.unet_template(cfg, "tiny_unet_schema.json", "axial"), 600))
    vae = AutoencoderKL(**TINY_VAE_CFG, precision="bf16")
    vae.load_state_dict(seeded_state_dict(TP.from_schema("tiny_vae_schema.json"), 601))
    ldm = LatentDiffusion(torch_nn_module=net, layout="NTHWC", data_shape=(2, 32, 32, 1), timesteps=1000, use_ema=False,
                          latent_shape=tuple(cfg["target_shape"]), first_stage_model=vae, cond_stage_model="__is_first_stage__",
                          scale_factor=0.18215).cuda().eval()
    ldm.num_streams = 1
    return ldm


def test_end_to_end_context():
    """Raw events (2, 96, 96, 9) -> fe.ingest -> sample(): the module gets the restatement's context, bit for bit (the contexts are
    compared; one sampling run shows the tensor is accepted as it is), and the forecast goes back to bytes."""
    ldm = _tiny_ldm()
    fe = SEVIRFrontEnd(in_len=3, out_len=2)
    raw = _events((2, 96, 96, 9), 13)
    ctx, tgt = fe.ingest(torch.from_numpy(raw).cuda())
    rc, rt = R.ingest(raw, (2, 3, 3), "01", 3, 2, (0,))
    assert ctx.shape == (2, 3, 32, 32, 1) and torch.equal(ctx.cpu(), torch.from_numpy(rc)) and torch.equal(tgt.cpu(), torch.from_numpy(rt))
    g = torch.Generator().manual_seed(14)
    tape = [torch.randn(tuple(ldm.get_batch_latent_shape(2)), generator=g) for _ in range(5)]
    out = ldm.sample(cond={"y": ctx}, batch_size=2, sampler="ddim", ddim_steps=2, eta=0.0, noise_tape=tape)
    assert out.shape == tgt.shape and bool(torch.isfinite(out).all())
    vil = fe.export(out.contiguous())
    assert vil.shape == (2, 2, 32, 32) and torch.equal(vil.cpu(), torch.from_numpy(R.export(out.cpu().numpy(), "01")))
