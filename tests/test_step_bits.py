"""GPU: the output BYTES of the sampler-step entry points of csrc/elementwise.hip, pinned.  No tolerance: the SHA-256 of the raw bytes of
`out`, and of `hist` where the form has one, equals the digest in tests/golden/step_digests.json, which was recorded from the library of
the commit before the nine step kernels became instantiations of one body.  A change of these kernels that is meant to be neutral keeps
every digest; one that is meant to change bits rewrites the fixture and says so.

The ten entry points: pd_ddim_step, pd_dpmpp_2m_step, pd_dpmpp_2m_sde_step, each plain, guided and held, and pd_hold_blend.  DDIM runs with
a noise tensor and without, every held form with a shift and without, pd_hold_blend out of place and in place.  Sizes: 96 (one partial
block), 1000 (four blocks and a ragged tail), both with B = 3, and 8192 * 256 + 300 with B = 1: the grid stops at 8192 blocks, so there,
and only there, the grid-stride loop takes a second trip.  At B = 3 sample 0 has w = 0 and a history of NaN, sample 1 has c_n = 0 and
k_n = 0 and a step noise (2M-SDE; DDIM reads its noise at every sigma) and a hold noise of NaN, sample 2 is generic; the B = 1 sample is
the generic one.  The mask is 0, 1 and 0.25 mixed within a sample.

Inputs are the closed-form integer hash of tests/test_norm_bits.py (no library RNG), the coefficient rows are fixed with a_t in (0, 1) as in
tests/test_hold.py::_rows.  Output buffers are pre-filled with 0x55 and have GUARD bytes of 0x55 behind them, which must still be there
afterwards.

As a script (needs an MI355X), with PD_LIB_PATH naming the library to run:
    python tests/test_step_bits.py --write tests/golden/step_digests.json      record the fixture
    python tests/test_step_bits.py                                             every buffer as fixture / this library / identical
"""
import hashlib
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from prediff_amd import _lib as L  # noqa: E402
from test_norm_bits import GUARDS, buf, hashed  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_digests.json")

WIDTH = {"ddim": 3, "dpmpp_2m": 4, "dpmpp_2m_sde": 5}
ROWS = {"ddim": [[0.05, 0.20, 0.30], [0.60, 0.80, 0.0], [0.97, 0.99, 0.05]],                                 # a_t, a_prev, sigma
        "dpmpp_2m": [[0.05, 0.90, 0.40, 0.0], [0.60, 0.80, 0.30, 1.9], [0.97, 0.50, 0.60, 0.5]],             # a_t, c_x, c_d, w
        "dpmpp_2m_sde": [[0.05, 0.90, 0.40, 0.0, 0.7], [0.60, 0.80, 0.30, 1.9, 0.0], [0.97, 0.50, 0.60, 0.5, 0.2]]}    # ..., c_n
TAIL = [[2.5, 0.8, 0.6], [0.01, 1.0, 0.0], [0.3, 0.3, 0.9375]]                                               # gamma, k_x, k_n
SIZES = {"3x96": ((0, 1, 2), 96), "3x1000": ((0, 1, 2), 1000), "1x2097452": ((2,), 8192 * 256 + 300)}      # the samples' rows, per_sample
NAN = float("nan")


def rows(solver, samples, form):
    width = WIDTH[solver] + {"plain": 0, "guided": 1, "held": 3}[form]
    return torch.tensor([(ROWS[solver][s] + TAIL[s])[:width] for s in samples], dtype=torch.float32, device="cuda")


def operands(samples, per):
    shape = (len(samples), per)
    o = {k: hashed(shape, 51 + i) for i, k in enumerate(("zt", "eps", "noise", "hist", "shift", "x0", "hnoise", "sde_noise"))}
    u = hashed(shape, 60)                                    # u in [-4, 4): about a third each of mask 0, 0.25 and 1
    o["mask"] = torch.full_like(u, 0.25)
    o["mask"][u < -1.25] = 0.0
    o["mask"][u >= 1.25] = 1.0
    if len(samples) == 3:
        o["hist"][0] = NAN                                   # w = 0: not read
        o["sde_noise"][1] = NAN                              # c_n = 0: not read
        o["hnoise"][1] = NAN                                 # k_n = 0: not read
    return o


def filled(x):
    """`x` in a buffer with a guard behind it: an operand the kernel writes as well"""
    b = buf(tuple(x.shape), torch.float32)
    b.copy_(x)
    return b


# ------------------------------------------------------------------------------------------------ the cases: name -> () -> {buffer: tensor}
CASES = {}


def add_step(solver, form, size, with_noise=True, with_shift=True):
    name = f"{solver}_step[{form},{size}{'' if with_noise else ',no noise'}{'' if with_shift else ',no shift'}]"

    def run():
        samples, per = SIZES[size]
        o = operands(samples, per)
        out, hist = buf((len(samples), per), torch.float32), filled(o["hist"])
        args = [o["zt"], o["eps"]]
        if solver == "ddim":
            args.append(o["noise"] if with_noise else None)
        if solver == "dpmpp_2m_sde":
            args.append(o["sde_noise"])
        if solver != "ddim":
            args.append(hist)
        if form != "plain":
            args.append(o["shift"] if with_shift else None)
        if form == "held":
            args += [o["x0"], o["mask"], o["hnoise"]]
        fn = getattr(L, f"{solver}_step" + {"plain": "", "guided": "_guided", "held": "_held"}[form])
        fn(*args, rows(solver, samples, form), out, len(samples), per)
        return {"out": out, "hist": hist if solver != "ddim" else None}

    assert name not in CASES, name
    CASES[name] = run


def add_hold_blend(size, in_place):
    name = f"hold_blend[{'in place' if in_place else 'out of place'},{size}]"

    def run():
        samples, per = SIZES[size]
        o = operands(samples, per)
        coef2 = torch.tensor([TAIL[s][1:] for s in samples], dtype=torch.float32, device="cuda")
        if in_place:                                         # the start rule as the loops call it: the latent is the hold noise and the output
            z = filled(o["zt"])
            L.hold_blend(z, o["x0"], o["mask"], z, coef2, z, len(samples), per)
            return {"out": z}
        out = buf((len(samples), per), torch.float32)
        L.hold_blend(o["zt"], o["x0"], o["mask"], o["hnoise"], coef2, out, len(samples), per)
        return {"out": out}

    assert name not in CASES, name
    CASES[name] = run


for _size in SIZES:
    for _solver in WIDTH:
        for _form in ("plain", "guided", "held"):
            for _shift in ((True, False) if _form == "held" else (True,)):
                for _noise in ((True, False) if _solver == "ddim" else (True,)):
                    add_step(_solver, _form, _size, _noise, _shift)
    add_hold_blend(_size, False)
    add_hold_blend(_size, True)


# ------------------------------------------------------------------------------------------------ digests
def digests(name):
    del GUARDS[:]
    bufs = CASES[name]()
    torch.cuda.synchronize()
    assert all(bool((g == 0x55).all()) for g in GUARDS), f"{name}: bytes written behind an output buffer"
    assert all(bool(torch.isfinite(t).all()) for t in bufs.values() if t is not None), f"{name}: a NaN that must not be read reached an output"
    return {k: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest() for k, t in bufs.items() if t is not None}


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_bits(name):
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
