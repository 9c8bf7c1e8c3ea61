"""The fast samplers as data: one `StepRule` per sampler states what its step kernels take and how its loop is set up, and
`launch_step` is the one place that turns a rule and a step's tensors into a call of `_lib`'s step wrappers ("Step rules").
A sampler is one rule here, its three wrappers (<stem>, <stem>_guided, <stem>_held) in `_lib` and the kernels behind them."""
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import _lib as L
from .schedule import (make_ddim_sampling_parameters, make_ddim_timesteps, make_dpmpp_2m_coefficients, make_dpmpp_2m_sde_coefficients,
                       make_logsnr_timesteps)


class StepRule(NamedTuple):
    name: str                    # `sample`'s sampler=...; the loop method is <name>_sample_loop
    kind: str                    # the graph kind `_graph_step` / `_lanes` know the un-held step by
    stem: str                    # `_lib` wrappers <stem>, <stem>_guided, <stem>_held
    width: int                   # fp32 columns of an un-held, un-guided coefficient row
    noise: Optional[str]         # the step-noise operand: None (there is none), "nullable" (a null pointer reads as zero) or "pointer"
    hist: bool                   # the kernels keep the previous step's x0
    tape_without_eta: bool       # the step reads a tape entry of its own even at eta = 0 (else only a stochastic step does)
    label: str                   # the sampler's name in a refusal
    steps_kw: str                # the loop's step-count keyword
    default_steps: int
    eta_default: float           # `sample`'s default eta
    loop_kw: tuple               # those of `sample`'s eta / discretize / lower_order_final that the loop takes; no "eta": eta must be 0
    schedule: Callable           # (ldm, n_steps, eta, discretize, lower_order_final) -> (table, grid, visited), see _ddim_schedule

    def row_width(self, guided, held):
        """Columns of a coefficient row: gamma behind the un-held row when guided; (gamma, k_x, k_n) when held, guided or not."""
        return self.width + (3 if held else 1 if guided else 0)

    def stochastic(self, eta):
        return self.noise is not None and float(eta) > 0

    def reads_tape(self, eta):
        """Whether the sampler's own step reads a noise-tape entry (a hold's draw then follows it, else stands in its place)."""
        return self.tape_without_eta or self.stochastic(eta)


def _alphas_cumprod(ldm):
    return ldm._alphas_cumprod_f64.astype(np.float32).astype(np.float64)          # the fp32 buffer's values


def _ddim_schedule(ldm, n_steps, eta, discretize, lower_order_final):
    """(table, grid, visited): the coefficient rows in visiting order, rounded to fp32 by the caller or already fp32 values; the grid of
    timesteps; the grid index of every visited step (the step's t is grid[visited[k]]).  DDIM rows: (a_t, a_prev, sigma)."""
    grid = np.minimum(make_ddim_timesteps(discretize, n_steps, ldm.num_timesteps), ldm.num_timesteps - 1)
    sig, a, a_prev = make_ddim_sampling_parameters(_alphas_cumprod(ldm), grid, eta)
    visited = np.arange(len(grid) - 1, -1, -1)
    return np.stack([a, a_prev, sig], axis=1)[visited], grid, visited


def _multistep_schedule(coefficients):
    """The 2M solvers': rows (a_t, c_x, c_d, w[, c_n]); `discretize` may be "logsnr", and repeated grid points are not visited."""
    def schedule(ldm, n_steps, eta, discretize, lower_order_final):
        ac = _alphas_cumprod(ldm)
        grid = make_logsnr_timesteps(n_steps, ac) if discretize == "logsnr" else \
            np.minimum(make_ddim_timesteps(discretize, n_steps, ldm.num_timesteps), ldm.num_timesteps - 1)
        table, visited = coefficients(ac, grid, eta, lower_order_final)
        return table, grid, visited
    return schedule


_2M = dict(hist=True, tape_without_eta=False, label="DPM-Solver++", steps_kw="steps", default_steps=20)
DDIM = StepRule(name="ddim", kind="ddim", stem="ddim_step", width=3, noise="nullable", hist=False, tape_without_eta=True, label="DDIM",
                steps_kw="ddim_steps", default_steps=50, eta_default=0.0, loop_kw=("eta",), schedule=_ddim_schedule)
DPMPP_2M = StepRule(name="dpmpp_2m", kind="dpmpp", stem="dpmpp_2m_step", width=4, noise=None, eta_default=0.0,
                    loop_kw=("discretize", "lower_order_final"), **_2M,
                    schedule=_multistep_schedule(lambda ac, grid, eta, lof: make_dpmpp_2m_coefficients(ac, grid, lof)))
DPMPP_2M_SDE = StepRule(name="dpmpp_2m_sde", kind="dpmpp_sde", stem="dpmpp_2m_sde_step", width=5, noise="pointer", eta_default=1.0,
                        loop_kw=("eta", "discretize", "lower_order_final"), **_2M,
                        schedule=_multistep_schedule(make_dpmpp_2m_sde_coefficients))
RULES = {r.name: r for r in (DDIM, DPMPP_2M, DPMPP_2M_SDE)}
FAST_SAMPLERS = tuple(RULES)
GRAPH_KINDS = {r.kind: r for r in RULES.values()}


def launch_step(rule, z, eps, noise, hist, shift, hold, coef, out):
    """One step of `rule` on the current stream: out = step(z, eps, ...) with the rows `coef`, one per sample.  noise / hist are used
    where the rule has them; shift: the guidance shift or None; hold: None or (x0, mask, hold_noise) of a held-region run.  A shift
    alone picks the "_guided" wrapper, any hold the "_held" one (which takes the shift, None included).  The wrapper is looked up on
    `_lib` at call time, so a replaced module attribute is honoured."""
    args = [z, eps]
    if rule.noise is not None:
        # no noise (eta = 0): sigma / c_n is 0 on every row and nothing is read.  A "pointer" kernel still demands the operand, and
        # the latent stands in; a "nullable" one takes the null pointer
        args.append(z if noise is None and rule.noise == "pointer" else noise)
    if rule.hist:
        args.append(hist)
    suffix = ""
    if hold is not None:
        x0, mask, hold_noise = hold
        # the last step has k_n = 0 and draws nothing: the latent stands in for the hold's noise, which the kernel does not read
        args += [shift, x0, mask, z if hold_noise is None else hold_noise]
        suffix = "_held"
    elif shift is not None:
        args.append(shift)
        suffix = "_guided"
    return getattr(L, rule.stem + suffix)(*args, coef, out, z.shape[0], z[0].numel())
