"""The step-rule table and its launcher, host side (prediff_amd/step_rules.py; DESIGN.md §7, "Step rules"): for every rule and every
form of its step (plain, guided, held) the launcher hands each parameter of the `_lib` wrapper, by the wrapper's own parameter names,
the tensor meant for it, and the drivers allocate coefficient rows of the width the wrapper's `coefN` states.  CPU tensors and
recording stubs: no kernel runs."""
import contextlib
import inspect

import pytest
import torch

from prediff_amd import _lib as L
from prediff_amd import rollout
from prediff_amd import step_rules as SR
from prediff_amd.latent_diffusion import LatentDiffusion

B, PER = 2, 3
FORMS = ("", "_guided", "_held")
RULES = list(SR.RULES.values())


# the real wrappers' parameter names, read before any test replaces a wrapper
PARAMS = {r.stem + f: list(inspect.signature(getattr(L, r.stem + f)).parameters) for r in RULES for f in FORMS}


def _params(rule, form):
    return PARAMS[rule.stem + form]


def _stated_width(rule, form):
    """The N of the wrapper's `coefN` parameter; pd_ddim_step's plain `coef` is its three-column row (a_t, a_prev, sigma)."""
    name, = [p for p in _params(rule, form) if p.startswith("coef")]
    return int(name[4:]) if name[4:] else 3


def _record(monkeypatch, rule, form):
    """Replace the wrapper by a recorder: {parameter name: argument} of its one call."""
    params, got = _params(rule, form), {}

    def recorder(*args):
        assert not got and len(args) == len(params), (len(args), params)
        got.update(zip(params, args))
    monkeypatch.setattr(L, rule.stem + form, recorder)
    return got


def _launch(rule, form, *, noise=True, hold_noise=True, shift=True):
    """launch_step with a distinct tensor per operand; the tensors by parameter name."""
    names = ("zt", "eps", "noise", "hist", "shift", "hold_x0", "hold_mask", "hold_noise", "out")
    t = {n: torch.full((B, PER), float(i)) for i, n in enumerate(names)}
    t["coef"] = torch.zeros(B, rule.row_width(form == "_guided", form == "_held"))
    if not noise:
        t["noise"] = None
    if not hold_noise:
        t["hold_noise"] = None
    if not (shift and form):
        t["shift"] = None
    hold = (t["hold_x0"], t["hold_mask"], t["hold_noise"]) if form == "_held" else None
    SR.launch_step(rule, t["zt"], t["eps"], t["noise"], t["hist"], t["shift"], hold, t["coef"], t["out"])
    return t


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rule", RULES, ids=list(SR.RULES))
def test_every_parameter_gets_its_tensor(monkeypatch, rule, form):
    got = _record(monkeypatch, rule, form)
    t = _launch(rule, form)
    assert list(got) == _params(rule, form)
    assert ("noise" in got) == (rule.noise is not None) and ("hist" in got) == rule.hist
    assert ("shift" in got) == (form != "") and ("hold_x0" in got) == ("hold_mask" in got) == ("hold_noise" in got) == (form == "_held")
    for name, arg in got.items():
        if name in ("B", "per_sample"):
            continue
        assert arg is t["coef" if name.startswith("coef") else name], name
    assert got["B"] == B and got["per_sample"] == PER
    # the rows of this form, as the graph driver (un-guided) and the eager / aligned driver allocate them
    assert t["coef"].shape[1] == _stated_width(rule, form)


@pytest.mark.parametrize("rule", RULES, ids=list(SR.RULES))
def test_stand_ins_for_operands_no_kernel_reads(monkeypatch, rule):
    for form in FORMS:
        got = _record(monkeypatch, rule, form)
        t = _launch(rule, form, noise=False, hold_noise=False, shift=form == "_guided")
        if rule.noise == "pointer":          # the SDE step at eta = 0 demands the pointer: the latent stands in
            assert got["noise"] is t["zt"], form
        elif rule.noise == "nullable":       # DDIM at eta = 0: the kernels take a null pointer
            assert got["noise"] is None, form
        if form == "_held":                  # the last held step draws nothing; an un-guided held step has no shift
            assert got["hold_noise"] is t["zt"] and got["shift"] is None
        assert all(isinstance(got[n], torch.Tensor) for n in got if n not in ("B", "per_sample", "noise", "shift")), form


class _ZeroDenoiser(torch.nn.Module):
    def forward(self, x, t, c):
        return torch.zeros_like(x)


@pytest.mark.parametrize("rule", RULES, ids=list(SR.RULES))
def test_loops_allocate_rows_of_the_stated_width(monkeypatch, rule):
    """`sample` on the CPU (the eager driver) with every wrapper a recorder: plain, guided, held and guided + held runs launch the
    form meant for them with (B, N) rows, N as the wrapper's `coefN` states."""
    seen = []
    monkeypatch.setattr(L, "on_device", lambda t: contextlib.nullcontext())
    monkeypatch.setattr(L, "hold_blend", lambda z, x0, mask, noise, coef2, out, B, per: out.copy_(z))
    for form in FORMS:
        params = _params(rule, form)

        def stub(*args, form=form, params=params):
            a = dict(zip(params, args))
            coef, = [v for k, v in a.items() if k.startswith("coef")]
            seen.append((form, tuple(coef.shape)))
            a["out"].copy_(a["zt"])
        monkeypatch.setattr(L, rule.stem + form, stub)
    ldm = LatentDiffusion(_ZeroDenoiser(), layout="NTHWC", data_shape=(2, 8, 8, 1), timesteps=1000, use_ema=False, latent_shape=(2, 4, 4, 1))
    ldm.set_alignment(lambda zt, t, zc=None, y=None, **kw: torch.zeros_like(zt))
    shape = ldm.get_batch_latent_shape(B)
    mask = torch.zeros(1, 2, 1, 1, 1)
    mask[:, 0] = 1.0
    hold = dict(hold_mask=mask, hold_x0=torch.ones(shape))
    kw = dict(cond=torch.zeros(B, 3, 4, 4, 1), batch_size=B, return_decoded=False, sampler=rule.name, ddim_steps=3, x_T=torch.zeros(shape))
    for run, form in (({}, ""), (dict(use_alignment=True), "_guided"), (hold, "_held"), (dict(hold, use_alignment=True), "_held")):
        seen.clear()
        ldm.sample(**kw, **run)
        assert seen and set(seen) == {(form, (B, _stated_width(rule, form)))}, (run.keys(), seen)


def test_one_set_of_fast_sampler_names():
    assert set(SR.FAST_SAMPLERS) == set(SR.RULES) == {r.name for r in RULES} and len(SR.FAST_SAMPLERS) == 3
    assert rollout.FAST_SAMPLERS is SR.FAST_SAMPLERS
    assert set(SR.GRAPH_KINDS) == {r.kind for r in RULES} and len(SR.GRAPH_KINDS) == 3 and SR.GRAPH_KINDS["ddim"] is SR.DDIM
    m = x = torch.zeros(1)
    accepted = set()
    for name in list(SR.FAST_SAMPLERS) + ["ddpm", "dpmpp_3m"]:
        try:
            assert LatentDiffusion._check_hold(m, x, "fresh", name) is True
            accepted.add(name)
        except NotImplementedError:
            pass
    assert accepted == set(SR.FAST_SAMPLERS)
    for rule in RULES:
        assert callable(getattr(LatentDiffusion, rule.name + "_sample_loop"))
        for form in FORMS:
            assert callable(getattr(L, rule.stem + form))
