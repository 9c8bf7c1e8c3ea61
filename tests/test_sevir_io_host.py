"""The SEVIR pixel front end, host side (prediff_amd/sevir_io.py; no GPU): refusals, the window arithmetic, and the numpy restatement
(tests/_sevir_io_ref.py) against the reference's own two static methods (tests/golden/sevir_io.npz, written by gen_golden_sevir_io.py)."""
import numpy as np
import pytest
import torch

import _sevir_io_ref as R
from prediff_amd import SEVIRFrontEnd
from prediff_amd.sevir_io import RESCALE


def _raw(shape=(2, 6, 9, 5), dtype=torch.uint8):
    return torch.zeros(shape, dtype=dtype)


def test_constructor_refusals():
    for dt in ("vis", "ir069", "ir107", "lght"):
        with pytest.raises(NotImplementedError):
            SEVIRFrontEnd(data_type=dt)
    with pytest.raises(NotImplementedError):
        SEVIRFrontEnd(pool="mean")
    for kw in (dict(rescale="0255"), dict(data_type="radar"), dict(pool="min"), dict(factors=(2, 3)), dict(factors=(2, 0, 3)),
               dict(factors=(2, 3, 1.5)), dict(in_len=0), dict(out_len=-1), dict(in_len=2.5)):
        with pytest.raises(ValueError):
            SEVIRFrontEnd(**kw)
    fe = SEVIRFrontEnd()
    assert (fe.in_len, fe.out_len, fe.factors, fe.rescale, fe.data_type) == (7, 6, (2, 3, 3), "01", "vil")
    assert (fe.scale, fe.offset) == (1 / 255, 0.0)
    assert (SEVIRFrontEnd(rescale="sevir").scale, SEVIRFrontEnd(rescale="sevir").offset) == (1 / 47.54, -33.44)


def test_tables_match_the_restatement():
    assert {k: v["vil"] for k, v in RESCALE.items()} == R.RESCALE


def test_ingest_refusals():
    fe = SEVIRFrontEnd(in_len=2, out_len=1)
    with pytest.raises(ValueError, match="divisible"):
        fe.ingest(_raw((2, 7, 9, 5)))                       # H % fh
    with pytest.raises(ValueError, match="divisible"):
        fe.ingest(_raw((2, 6, 10, 5)))                      # W % fw
    with pytest.raises(ValueError, match="uint8"):
        fe.ingest(_raw(dtype=torch.float32))
    with pytest.raises(ValueError, match="uint8"):
        fe.ingest(_raw(dtype=torch.int16))
    with pytest.raises(ValueError, match=r"\(N, H, W, T\)"):
        fe.ingest(_raw((6, 9, 5)))
    with pytest.raises(ValueError, match="contiguous"):
        fe.ingest(_raw((2, 9, 6, 5)).transpose(1, 2))       # the right shape, the wrong strides
    with pytest.raises(ValueError, match="runs past"):
        fe.ingest(_raw(), starts=(1,))                      # T = 5 -> 3 LR frames = one window at 0
    with pytest.raises(ValueError, match="runs past"):
        fe.ingest(_raw(), starts=(0, -1))
    for bad in ((), 0, (0.5,), torch.tensor([0])):
        with pytest.raises(ValueError):
            fe.ingest(_raw(), starts=bad)
    with pytest.raises(ValueError, match="no CPU path"):
        fe.ingest(_raw())                                   # everything right but the device: there is no fallback


def test_export_refusals():
    fe = SEVIRFrontEnd()
    x = torch.zeros(2, 3, 4, 8, 1)
    with pytest.raises(ValueError, match="no CPU path"):
        fe.export(x)
    with pytest.raises(ValueError, match="float32"):
        fe.export(x.double())
    with pytest.raises(ValueError, match=r"\(B, T, H, W, 1\)"):
        fe.export(x[..., 0])
    with pytest.raises(ValueError, match=r"\(B, T, H, W, 1\)"):
        fe.export(torch.zeros(2, 3, 4, 8, 2))
    with pytest.raises(ValueError, match="contiguous"):
        fe.export(torch.zeros(2, 3, 8, 4, 1).transpose(2, 3))
    for dtype, layout in ((torch.float32, "NTHW"), (torch.uint8, "NTHWC"), (torch.float16, None), (torch.uint8, "NCHW")):
        with pytest.raises(ValueError, match="export writes"):
            fe.export(x, dtype=dtype, layout=layout)


def test_window_arithmetic_T49():
    """T = 49 at ft = 2 is frames 0, 2, ..., 48: 25 LR frames (SEVIR_LR_RAW_SEQ_LEN); a 7 + 6 window starts at 0 .. 12."""
    fe = SEVIRFrontEnd()
    assert fe.lr_shape((3, 384, 384, 49)) == (3, 25, 128, 128)
    assert fe.check_windows((3, 384, 384, 49), (0, 6, 12)) == (0, 6, 12)
    assert fe.check_windows((3, 384, 384, 49), [12]) == (12,)           # the last valid index: frames 12 .. 24
    with pytest.raises(ValueError, match="last valid start is 12"):
        fe.check_windows((3, 384, 384, 49), (13,))                      # one past it
    with pytest.raises(ValueError, match="runs past"):
        fe.check_windows((3, 384, 384, 49), (0, 13))
    assert fe.lr_shape((1, 384, 384, 48))[1] == 24 and fe.lr_shape((1, 384, 384, 1))[1] == 1
    full = SEVIRFrontEnd(in_len=13, out_len=12, factors=(1, 1, 1))
    assert full.lr_shape((1, 384, 384, 49)) == (1, 49, 384, 384)
    assert full.check_windows((1, 384, 384, 49), (24,)) == (24,)
    with pytest.raises(ValueError):
        full.check_windows((1, 384, 384, 49), (25,))
    assert SEVIRFrontEnd(in_len=25, out_len=0).check_windows((1, 384, 384, 49), (0,)) == (0,)


@pytest.mark.parametrize("rescale", ["01", "sevir"])
def test_restatement_vs_reference_fixture(golden, rescale):
    """preprocess_data_dict / process_data_dict_back themselves, run by gen_golden_sevir_io.py, against the restatement: bit for bit."""
    g = golden("sevir_io")
    assert sorted(np.unique(g["raw"]).tolist()) == list(range(256))
    pre = np.transpose(R.forward(g["raw"], rescale), (0, 3, 1, 2))[..., None]
    assert pre.dtype == np.float32 and np.array_equal(pre, g[f"pre_{rescale}"])
    assert np.array_equal(R.back(g["frames"], rescale), g[f"back_{rescale}"])
    ctx, tgt = R.ingest(g["raw"], (1, 1, 1), rescale, 10, 6, (0,))
    assert np.array_equal(np.concatenate([ctx, tgt], axis=1), g[f"pre_{rescale}"])


@pytest.mark.parametrize("rescale", ["01", "sevir"])
def test_restatement_round_trip(rescale):
    """back(forward(b)) rounds to b for all 256 bytes in both modes (in fp32 it is b only to about 2e-5: the bytes are what round-trips).
    tests/test_sevir_io.py asserts the device round trip for both modes on the strength of this."""
    b = np.arange(256, dtype=np.uint8)
    v = R.back(R.forward(b, rescale), rescale)
    assert np.array_equal(R.to_bytes(v), b)
    assert float(np.abs(v - b.astype(np.float32)).max()) < 1e-4


def test_restatement_pool():
    raw = np.zeros((1, 4, 6, 3), dtype=np.uint8)
    raw[0, 1, 2, 0], raw[0, 2, 3, 2], raw[0, 3, 5, 1] = 9, 7, 200          # frame 1 is skipped at ft = 2
    p = R.pool(raw, (2, 2, 3))
    assert p.shape == (1, 2, 2, 2) and p.dtype == np.uint8
    assert p[0, :, :, 0].tolist() == [[9, 0], [0, 0]] and p[0, :, :, 1].tolist() == [[0, 0], [0, 7]]
