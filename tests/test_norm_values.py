"""GPU: the output VALUES of every entry point of csrc/norm.hip, element by element against fp64.  The pair of tests/test_norm_bits.py:
that file pins the bytes of its CASES, this one runs the same CASES and says the bytes are right.

Every buffer a case returns is decoded (16-bit operand, bf16 hi + lo, e4m3 / fp8_scale, MX payload x 2^(scale byte - 127), fp32, the
fp64 partial sums) and compared with the fp64 reference of the case's own inputs (tests/_norm_ref.py: the references, the decoders and
the criterion).  Per element, no norm over the tensor:
    |decode(got_i) - ref_i| <= |q(ref_i) - ref_i| + 4 * e32
q = the CPU cast of the reference into the buffer's format, e32 = the largest error of torch's own fp32 CPU evaluation of the same op on
the same input.  Statistics: rstd within 2^-22 relative, mean within 2^-22 max|x|.  Pad columns are exactly zero, the guard bytes behind
every buffer are untouched, and no buffer and no element is left out.  A failure names the case, the buffer and the worst element's
(row, channel, group) with got / ref / bound; every case prints its max err / bound (pytest -s).

test_norm_family_values swaps only x of one case per GroupNorm dispatch path (and one LayerNorm / patch-merge shape per vector count) for
inputs that stress the statistics: a mean of 30 and 100 standard deviations, a near-constant group, channel means that differ inside a
group, one exactly constant group, a sample of zeros beside an ordinary one.

Measured on the MI355X: max err / bound at mean/std = 30 | 100 | near-constant, before -> after the two-launch statistics kernels carried
their per-thread sums in fp64 (they summed x and x^2 in fp32 and only then widened; DESIGN.md, "GroupNorm statistics"):
    (mean, rstd) from the partial sums   vec / fp8 / stats 79 | 1250 | 5.3e4,  scalar C = 64  147 | 2350 | 8.3e4,
                                         scalar C = 512  703 | 9620 | 4.3e5,  mx 38..108 | 491..1260 | 4.9e4..6.8e4   -> all < 1e-3
    stats buffer (vec)                   117 | 1840 | 6.5e4 -> 0.24
    hi/lo output                         3.65 | 15 | 74 -> 0.58 | 0.37 | 0.29
    bf16 two launches, fp8, mx outputs   1.01 | 3.9 | 52,  - | 4.8 | 17,  1.0 | 2.1 | 21  -> <= 1 (the format's own rounding)
    scalar outputs C = 64 / 512          1.19 | 5.9 | 41,  8.3 | 65 | 301 -> <= 1
    one-pass (three instantiations), general scalar (C = 5), backward: unchanged, 0.2 .. 1.0
The backward failed one family before its kernel formed n from the centred xh: constant group, sum dxh 4.1e-4 off, 7.5 x its bound.
"""
import pytest
import torch

import _norm_ref as R
import test_norm_bits as TB

pytestmark = pytest.mark.gpu


def run_case(name):
    del TB.GUARDS[:]
    TB.SPECS.pop(name, None)
    bufs = TB.CASES[name]()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return TB.SPECS[name], bufs, [(f"buffer {i}", g) for i, g in enumerate(TB.GUARDS)]


@pytest.mark.parametrize("name", sorted(TB.CASES))
def test_norm_values(name):
    spec, bufs, guards = run_case(name)
    print("\n" + "\n".join(R.verify(name, spec, bufs, guards)))


def test_family_cases_cover_every_groupnorm_path():
    """bookkeeping, like test_fixture_has_no_stale_case: every name below is a pinned case, and every GroupNorm entry point and every
    dispatch tag of groupnorm_silu among the pinned cases has one (test_norm_values itself is parametrised over all of CASES)"""
    names = [n for n, _ in FAMILY_CASES]
    assert all(n in TB.CASES for n in names) and len(set(names)) == len(names)
    paths = {n.split(",")[0] if n.startswith("groupnorm_silu[") else n.split("[")[0] for n in TB.CASES if n.startswith("groupnorm")}
    assert paths == {n.split(",")[0] if n.startswith("groupnorm_silu[") else n.split("[")[0] for n in names if n.startswith("groupnorm")}


# ------------------------------------------------------------------------------------------------ ill-conditioned inputs
def _gn(tag, B, S, C, G, ld, fmt="bf16"):
    return f"groupnorm_silu[{tag},{B}x{S}x{C},G{G},ld{ld},{fmt},ss1,silu1]", C // G


# one case per GroupNorm dispatch path, with its channels per group
FAMILY_CASES = [
    _gn("scalar", 2, 70, 5, 5, 64),                         # gn_stats_kernel, general branch
    _gn("scalar", 2, 70, 64, 32, 64),                       #                  C divides 256
    _gn("scalar", 1, 70, 512, 256, 512),                    #                  C a multiple of 256
    _gn("vec", 2, 100, 128, 32, 128, "hilo"),               # gn_stats_vec_kernel + apply, hi/lo
    _gn("vec_two_launches", 2, 100, 128, 32, 128),
    _gn("onepass", 2, 70, 128, 32, 128),
    _gn("onepass_small_grid", 1, 70, 128, 32, 128),
    _gn("onepass_long", 1, 1100, 128, 32, 128),
    ("groupnorm_silu_fp8[2x100x128,G32,ss1]", 4),
    ("groupnorm_silu_mx[2x100x64,G16,ld128,ss1]", 4),
    ("groupnorm_silu_mx[1x70x256,G32,ld256,ss1]", 8),
    ("groupnorm_stats[2x100x128,G32]", 4),
    ("groupnorm_stats[2x70x5,G5]", 1),
    ("groupnorm_silu_bwd[2x100x64,G16]", 4),
    # LayerNorm: one shape per vector count NV = 1, 2, 4, 8, 16; the patch-merge gather with both paddings
    ("layernorm[hilo,7x32,ld64]", 4),
    ("layernorm[bf16,5x512,ld512]", 4),
    ("layernorm[hilo,3x1024,ld1024]", 4),
    ("layernorm[fp16,2x2048,ld2048]", 4),
    ("layernorm[hilo,2x4096,ld4096]", 4),
    ("patch_merge_layernorm[hilo,nearest]", 4),
    ("patch_merge_layernorm[hilo,zeros]", 4),
]


def run_family_case(name, cpg, family, monkeypatch):
    seed = 1000 + R.FAMILIES.index(family)
    monkeypatch.setattr(TB, "X_SOURCE", lambda shape: R.family_input(family, shape, cpg, seed))
    return run_case(name)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name,cpg", FAMILY_CASES, ids=[n for n, _ in FAMILY_CASES])
def test_norm_family_values(name, cpg, family, monkeypatch):
    assert name in TB.CASES, name
    spec, bufs, guards = run_family_case(name, cpg, family, monkeypatch)
    print("\n" + "\n".join(R.verify(f"{name} <- {family}", spec, bufs, guards)))
