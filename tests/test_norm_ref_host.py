"""CPU: tests/_norm_ref.py checked against itself before any kernel is.  Every case of tests/test_norm_bits.py and every input family of
tests/test_norm_values.py is run with the kernel calls replaced by nothing; the buffers a perfect kernel would return (q(fp64 reference),
encoded into each format) must pass `verify` with no element and no buffer left out -- the reference sits inside its own bound -- and a
localised error put into those buffers must fail it, with the element named."""
import pytest
import torch

import _norm_ref as R
import test_norm_bits as TB
import test_norm_values as TV


_LIB = TB.L


class _NoKernels:
    """prediff_amd._lib with every kernel launch a no-op (host helpers pass through)"""

    def __getattr__(self, name):
        if name in ("CallOpts", "groupnorm_nchunk"):
            return getattr(_LIB, name)
        return lambda *a, **k: None


@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(TB, "DEV", "cpu")
    monkeypatch.setattr(TB, "L", _NoKernels())


@pytest.mark.parametrize("name", sorted(TB.CASES))
def test_reference_inside_its_bound(name, on_cpu):
    spec, bufs, _ = TV.run_case(name)
    synth = R.synthesize(spec)
    assert set(synth) == {k for k, v in bufs.items() if v is not None}
    for k, v in synth.items():
        assert v.dtype == bufs[k].dtype and v.numel() == bufs[k].numel(), k
    R.verify(name, spec, synth)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name,cpg", TV.FAMILY_CASES, ids=[n for n, _ in TV.FAMILY_CASES])
def test_reference_inside_its_bound_family(name, cpg, family, on_cpu, monkeypatch):
    spec, _, _ = TV.run_family_case(name, cpg, family, monkeypatch)
    R.verify(name, spec, R.synthesize(spec))


def _synth(name):
    spec, _, _ = TV.run_case(name)
    return spec, R.synthesize(spec)


def test_one_wrong_element_is_named(on_cpu):
    name = "groupnorm_silu[scalar,2x70x64,G32,ld64,bf16,ss1,silu1]"
    spec, bufs = _synth(name)
    bits = bufs["out"].view(torch.int16)
    bits[93, 37] += 2                                       # two bf16 ulps, one element of 8960
    with pytest.raises(AssertionError, match=r"1 elements out of bound .* row 93, channel 37, group 18: got"):
        R.verify(name, spec, bufs)


def test_pad_column_and_unowned_byte_are_named(on_cpu):
    name = "layernorm_mx[5x96,ld128]"
    spec, bufs = _synth(name)
    bufs["scales"][2, 3] = 1
    with pytest.raises(AssertionError, match=r"scales: pad byte at row 2, column 3 is 0x1"):
        R.verify(name, spec, bufs)
    spec, bufs = _synth(name)
    guard = torch.full((TB.GUARD,), 0x55, dtype=torch.uint8)
    guard[7] = 0
    with pytest.raises(AssertionError, match=r"byte 7 behind the buffer overwritten"):
        R.verify(name, spec, bufs, [("out", guard)])


def test_nearest_by_integer_floor_is_caught(on_cpu):
    """H = 7 padded to 8: torch reads source row min(floor(p * float32(7 / 8)), 6); row 7 of the padded grid reads 6, and a gather that
    took the zero padding's rows instead differs in the last row of patches"""
    name = "patch_merge_layernorm[hilo,nearest]"
    spec, _ = _synth(name)
    wrong = dict(spec, nearest=False)
    with pytest.raises(AssertionError, match=r"out\+lo: .* worst at row \d+, channel \d+: got"):
        R.verify(name, spec, R.synthesize(wrong))


def test_statistics_with_a_wrong_count_are_caught(on_cpu):
    name = "groupnorm_stats[2x100x128,G32]"
    spec, bufs = _synth(name)
    bufs["stats"][1, 5, 1] *= 1 + 2.0 ** -20
    with pytest.raises(AssertionError, match=r"stats: .* sample 1, group 5, rstd"):
        R.verify(name, spec, bufs)
