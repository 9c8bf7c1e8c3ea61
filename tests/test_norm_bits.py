"""GPU: the output BYTES of every entry point of csrc/norm.hip, pinned.  No tolerance: the SHA-256 of the raw bytes of each output buffer
(payload, lo half, scale bytes, the fp64 partial sums, stats, dx) equals the digest in tests/golden/norm_digests.json, which was recorded
from the library of the commit before the writers and statistics prologues of norm.hip were shared.  A change of these kernels that is
meant to be neutral keeps every digest; one that is meant to change bits rewrites the fixture and says so.  (Rewritten once since: the
two-launch statistics kernels carry their sums in fp64 from the first add and the backward forms n from the centred xh -- 34 buffers of
21 cases, all downstream of gn_stats_vec_kernel, the two fast branches of gn_stats_kernel or gn_silu_bwd_kernel; every LayerNorm,
patch-merge, cast_rows, one-pass and general-scalar digest is the first recording's.)

Inputs are a closed-form integer hash -> fp32 in [-4, 4) (numpy integer arithmetic: no library RNG, whose stream may differ between
versions).  Output buffers are pre-filled with 0x55, so bytes a kernel leaves untouched are pinned as well.  The cases are the smallest
shapes that reach each instantiation and each tail; each runs in milliseconds.

This file says the bits are STABLE; tests/test_norm_values.py says they are RIGHT: it runs the same CASES and compares every element of
every buffer with an fp64 reference (tests/_norm_ref.py).  For that each case records its inputs and parameters in SPECS while it runs,
every buffer has GUARD bytes of 0x55 behind it (outside what is hashed), and X_SOURCE swaps a case's x for another input.

As a script (needs an MI355X), with PD_LIB_PATH naming the library to run:
    python tests/test_norm_bits.py --write tests/golden/norm_digests.json      record the fixture
    python tests/test_norm_bits.py                                             every buffer as fixture / this library / identical
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from prediff_amd import _lib as L  # noqa: E402

DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_digests.json")


# ------------------------------------------------------------------------------------------------ inputs and buffers
def hashed(shape, salt, scale=1.0, offset=0.0):
    """fp32 `offset + scale * u`, u in [-4, 4) on a 2^-21 grid from a 32-bit integer hash of (index, salt); scale a power of two: exact"""
    n = int(np.prod(shape))
    h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32((salt * 40503 + 12345) & 0xFFFFFFFF)
    h ^= h >> np.uint32(15)
    h *= np.uint32(2246822519)
    h ^= h >> np.uint32(13)
    h *= np.uint32(3266489917)
    h ^= h >> np.uint32(16)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -21) - np.float32(4.0)
    v = np.float32(offset) + np.float32(scale) * u
    return torch.from_numpy(v.astype(np.float32).reshape(shape)).to(DEV)


def affine(C, salt):
    """gamma in [0.5, 1.5), beta in [-1, 1)"""
    return hashed((C,), salt, 0.125, 1.0), hashed((C,), salt + 1, 0.25)


GUARD = 256          # bytes of 0x55 behind every buffer: not part of the buffer, not hashed
GUARDS = []          # the guard regions of the buffers made since the list was last cleared
SPECS = {}           # name -> the inputs and parameters of the case's last run (tests/_norm_ref.py reads them)
X_SOURCE = None      # None: the hashed x.  (shape) -> fp32 CPU tensor: another x for the same case (no digest is recorded for those)


def buf(shape, dtype):
    """an output buffer whose every byte is 0x55"""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((n + GUARD,), 0x55, dtype=torch.uint8, device=DEV)
    GUARDS.append(raw[n:])
    return raw[:n].view(dtype).reshape(shape)


def input_x(shape, salt):
    return hashed(shape, salt) if X_SOURCE is None else X_SOURCE(tuple(shape)).to(device=DEV, dtype=torch.float32).contiguous()


def opts_of(operand, **kw):
    return L.CallOpts(operand, **kw) if (operand == "fp16" or kw) else None


def op_dtype(operand):
    return torch.float16 if operand == "fp16" else torch.bfloat16


# ------------------------------------------------------------------------------------------------ the cases: name -> () -> {buffer: tensor}
CASES = {}


def case(name):
    def reg(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return reg


def add_layernorm(variant, rows, C, ld):
    operand = "fp16" if variant == "fp16" else "bf16"

    name = f"layernorm[{variant},{rows}x{C},ld{ld}]"

    @case(name)
    def _():
        x, (g, b) = input_x((rows, C), 1), affine(C, 2)
        SPECS[name] = dict(op="layernorm", x=x, gamma=g, beta=b, eps=1e-5, ld=ld, fmt=variant)
        out = buf((rows, ld), op_dtype(operand))
        lo = buf((rows, ld), torch.bfloat16) if variant == "hilo" else None
        L.layernorm(x, g, b, out, lo, rows, C, ld, opts=opts_of(operand))
        return {"out": out, "lo": lo}


for _shape in ((7, 32, 64), (5, 512, 512), (3, 1024, 1024), (2, 2048, 2048), (2, 4096, 4096)):      # NV = 1, 2, 4, 8, 16; R = 4, 2 row tails; pads
    for _variant in ("bf16", "hilo", "fp16"):
        add_layernorm(_variant, *_shape)


def add_layernorm_fp8(rows, C, ld):
    name = f"layernorm_fp8[{rows}x{C},ld{ld}]"

    @case(name)
    def _():
        x, (g, b) = input_x((rows, C), 3), affine(C, 4)
        g[3] = 40.0                                         # one gain of 40: 40 * |xhat| * 16 passes 448, the store saturates
        SPECS[name] = dict(op="layernorm", x=x, gamma=g, beta=b, eps=1e-5, ld=ld, fmt="e4m3", fp8_scale=16.0)
        out = buf((rows, ld), torch.uint8)
        L.layernorm_fp8(x, g, b, out, rows, C, ld, 16.0)
        return {"out": out}


for _shape in ((7, 32, 32), (5, 512, 512), (3, 1024, 1024)):
    add_layernorm_fp8(*_shape)


def add_layernorm_mx(rows, C, ld):
    name = f"layernorm_mx[{rows}x{C},ld{ld}]"

    @case(name)
    def _():
        x, (g, b) = input_x((rows, C), 5), affine(C, 6)
        SPECS[name] = dict(op="layernorm", x=x, gamma=g, beta=b, eps=1e-5, ld=ld, fmt="mx")
        out, scales = buf((rows, ld), torch.uint8), buf((rows, ld // 32), torch.uint8)
        L.layernorm_mx(x, g, b, out, scales, rows, C)
        return {"out": out, "scales": scales}


for _shape in ((7, 32, 128), (5, 96, 128), (3, 512, 512), (2, 1024, 1024), (2, 4096, 4096)):
    add_layernorm_mx(*_shape)


def add_patch_merge(variant, nearest):
    operand = "fp16" if variant == "fp16" else "bf16"

    name = f"patch_merge_layernorm[{variant},{'nearest' if nearest else 'zeros'}]"

    @case(name)
    def _():
        B, T, H, W, C, ds, ld = 2, 3, 7, 6, 16, (1, 2, 2), 64       # H = 7 is padded to 8: the last row of patches reads padding
        Cm, rows = C * ds[0] * ds[1] * ds[2], B * 3 * 4 * 3
        x, (g, b) = input_x((B, T, H, W, C), 7), affine(Cm, 8)
        SPECS[name] = dict(op="patch_merge_layernorm", x=x, gamma=g, beta=b, eps=1e-5, ld=ld, fmt=variant, ds=ds, nearest=nearest)
        out = buf((rows, ld), op_dtype(operand))
        lo = buf((rows, ld), torch.bfloat16) if variant == "hilo" else None
        L.patch_merge_layernorm(x, g, b, out, lo, B, T, H, W, C, ds, ld, pad_nearest=nearest, opts=opts_of(operand))
        return {"out": out, "lo": lo}


for _variant in ("bf16", "hilo", "fp16"):
    for _nearest in (False, True):
        add_patch_merge(_variant, _nearest)


def gn_inputs(B, S, C, G, ss, salt):
    x, (g, b) = input_x((B, S, C), salt), affine(C, salt + 1)
    kw = dict(ss_scale=hashed((B, C), salt + 3, 0.125), ss_shift=hashed((B, C), salt + 4, 0.25), ld_ss=C) if ss else {}
    partials = buf((B * L.groupnorm_nchunk(S, C) * G * 2,), torch.float64)
    return x, g, b, partials, kw


def gn_spec(x, g, b, kw, G, **more):
    return dict(x=x, gamma=g, beta=b, ss_scale=kw.get("ss_scale"), ss_shift=kw.get("ss_shift"), G=G, eps=1e-6,
                nchunk=L.groupnorm_nchunk(x.shape[1], x.shape[2]), **more)


def add_groupnorm(tag, B, S, C, G, ld, lo=False, operand="bf16", ss=True, silu=True, **opt_kw):
    name = f"groupnorm_silu[{tag},{B}x{S}x{C},G{G},ld{ld},{'hilo' if lo else operand},ss{int(ss)},silu{int(silu)}]"

    @case(name)
    def _():
        x, g, b, partials, kw = gn_inputs(B, S, C, G, ss, 9)
        SPECS[name] = gn_spec(x, g, b, kw, G, op="groupnorm", ld=ld, fmt="hilo" if lo else operand, silu=silu)
        out = buf((B * S, ld), op_dtype(operand))
        out_lo = buf((B * S, ld), torch.bfloat16) if lo else None
        L.groupnorm_silu(x, g, b, partials, out, out_lo, B, S, C, G, ld, 1e-6, silu=silu, opts=opts_of(operand, **opt_kw), **kw)
        return {"out": out, "lo": out_lo, "partials": partials}


# scalar paths: the general one (ld > C: pad columns), C <= 256 dividing 256 with 2 channels per group, C % 256 == 0
for _shape in ((2, 70, 5, 5, 64), (2, 70, 64, 32, 64), (1, 70, 512, 256, 512)):
    add_groupnorm("scalar", *_shape)
    add_groupnorm("scalar", *_shape, lo=True, ss=False, silu=False)
add_groupnorm("scalar", 2, 70, 5, 5, 64, operand="fp16")
# the vectorised pair of launches (with a lo half; without one only under groupnorm_two_launches) and the one-pass kernel's three
# instantiations <16, 512, 32>, <8, 512, 16> (small_grid), <26, 512, 16> (more than 1024 rows), each with scale-shift / SiLU on and off
for _ss in (True, False):
    for _silu in (True, False):
        add_groupnorm("vec", 2, 100, 128, 32, 128, lo=True, ss=_ss, silu=_silu)
        add_groupnorm("vec_two_launches", 2, 100, 128, 32, 128, ss=_ss, silu=_silu, groupnorm_two_launches=1)
        add_groupnorm("onepass", 2, 70, 128, 32, 128, ss=_ss, silu=_silu)
add_groupnorm("onepass_small_grid", 1, 70, 128, 32, 128, small_grid=1)
add_groupnorm("onepass_long", 1, 1100, 128, 32, 128)
add_groupnorm("vec_two_launches", 2, 100, 128, 32, 128, operand="fp16", groupnorm_two_launches=1)
add_groupnorm("onepass", 2, 70, 128, 32, 128, operand="fp16")
add_groupnorm("onepass_small_grid", 1, 70, 128, 32, 128, operand="fp16", small_grid=1)
add_groupnorm("onepass_long", 1, 1100, 128, 32, 128, operand="fp16")


def add_groupnorm_fp8(ss):
    name = f"groupnorm_silu_fp8[2x100x128,G32,ss{int(ss)}]"

    @case(name)
    def _():
        B, S, C, G = 2, 100, 128, 32
        x, g, b, partials, kw = gn_inputs(B, S, C, G, ss, 15)
        SPECS[name] = gn_spec(x, g, b, kw, G, op="groupnorm", ld=C, fmt="e4m3", fp8_scale=16.0, silu=True)
        out = buf((B * S, C), torch.uint8)
        L.groupnorm_silu_fp8(x, g, b, partials, out, B, S, C, G, 1e-6, 16.0, **kw)
        return {"out": out, "partials": partials}


def add_groupnorm_mx(B, S, C, G, ld, ss):
    name = f"groupnorm_silu_mx[{B}x{S}x{C},G{G},ld{ld},ss{int(ss)}]"

    @case(name)
    def _():
        x, g, b, partials, kw = gn_inputs(B, S, C, G, ss, 21)
        SPECS[name] = gn_spec(x, g, b, kw, G, op="groupnorm", ld=ld, fmt="mx", silu=True)
        out, scales = buf((B * S, ld), torch.uint8), buf((B * S, ld // 32), torch.uint8)
        L.groupnorm_silu_mx(x, g, b, partials, out, scales, B, S, C, G, 1e-6, **kw)
        return {"out": out, "scales": scales, "partials": partials}


for _ss in (True, False):
    add_groupnorm_fp8(_ss)
    add_groupnorm_mx(2, 100, 64, 16, 128, _ss)              # ld > C: pad columns are written
    add_groupnorm_mx(1, 70, 256, 32, 256, _ss)


def add_groupnorm_stats(B, S, C, G):
    name = f"groupnorm_stats[{B}x{S}x{C},G{G}]"

    @case(name)
    def _():
        x = input_x((B, S, C), 27)
        SPECS[name] = dict(op="groupnorm_stats", x=x, G=G, eps=1e-6, nchunk=L.groupnorm_nchunk(S, C))
        partials, stats = buf((B * L.groupnorm_nchunk(S, C) * G * 2,), torch.float64), buf((B, G, 2), torch.float32)
        L.groupnorm_stats(x, partials, stats, B, S, C, G, 1e-6)
        return {"partials": partials, "stats": stats}


add_groupnorm_stats(2, 100, 128, 32)
add_groupnorm_stats(2, 70, 5, 5)


@case("groupnorm_silu_bwd[2x100x64,G16]")
def _():
    B, S, C, G = 2, 100, 64, 16
    x, g, b, fwd, _ = gn_inputs(B, S, C, G, False, 31)
    dy = hashed((B, S, C), 35, 0.25)
    SPECS["groupnorm_silu_bwd[2x100x64,G16]"] = gn_spec(x, g, b, {}, G, op="groupnorm_bwd", dy=dy)
    y = buf((B * S, C), torch.bfloat16)
    L.groupnorm_silu(x, g, b, fwd, y, None, B, S, C, G, C, 1e-6)         # the forward whose partial sums the backward reduces again
    bwd, dx = buf(tuple(fwd.shape), torch.float64), buf((B, S, C), torch.float32)
    L.groupnorm_silu_bwd(x, dy, g, b, fwd, bwd, dx, B, S, C, G, 1e-6)
    return {"fwd_partials": fwd, "bwd_partials": bwd, "dx": dx}


def add_cast_rows(variant):
    operand = "fp16" if variant == "fp16" else "bf16"

    name = f"cast_rows[{variant}]"

    @case(name)
    def _():
        x = input_x((3, 13, 10), 41)                         # the shape of test_cast_rows_slice: 3 samples x 13 rows x 10 channels, rows 7..12
        SPECS[name] = dict(op="cast_rows", x=x, row_off=7, rows_out=6, ld=64, fmt=variant)
        out = buf((3 * 6, 64), op_dtype(operand))
        lo = buf((3 * 6, 64), torch.bfloat16) if variant == "hilo" else None
        L.cast_rows(x, out, lo, 3, 13, 7, 6, 10, 10, 64, opts=opts_of(operand))
        return {"out": out, "lo": lo}


for _variant in ("bf16", "hilo", "fp16"):
    add_cast_rows(_variant)


# ------------------------------------------------------------------------------------------------ digests
def digests(name):
    bufs = CASES[name]()
    torch.cuda.synchronize()
    return {k: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest() for k, t in bufs.items() if t is not None}


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_norm_bits(name):
    want = fixture()["digests"]
    assert name in want, f"{name}: not in {FIXTURE}"
    got = digests(name)
    assert got == want[name], f"{name}: output bytes differ from the recorded ones in {[k for k in want[name] if got.get(k) != want[name][k]]}"


def test_fixture_has_no_stale_case():
    assert sorted(fixture()["digests"]) == sorted(CASES)


def main():
    with open(L.LIB_PATH, "rb") as f:
        lib_sha = hashlib.sha256(f.read()).hexdigest()
    if len(sys.argv) == 3 and sys.argv[1] == "--write":
        out = {"library_sha256": lib_sha, "digests": {name: digests(name) for name in sorted(CASES)}}
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(out['digests'])} cases from library {lib_sha}")
        return 0
    want = fixture()
    print(f"library  fixture {want['library_sha256']}\n         this    {lib_sha}")
    bad = n = 0
    for name in sorted(CASES):
        got = digests(name)
        for k in sorted(set(got) | set(want["digests"].get(name, {}))):
            w, g = want["digests"].get(name, {}).get(k), got.get(k)
            n += 1
            bad += w != g
            print(f"{name} {k}\n    fixture {w}\n    this    {g}   {'identical' if w == g else 'DIFFERENT'}")
    print(f"{n} buffers of {len(CASES)} cases: " + ("all identical" if not bad else f"{bad} DIFFERENT"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
