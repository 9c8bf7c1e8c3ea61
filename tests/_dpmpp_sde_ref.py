"""CPU restatement (torch, fp64) of the stochastic DPM-Solver++(2M) sampler, written from the formulas of DESIGN.md §7 on top of
tests/_dpmpp_ref.py (grid, visit list, h_k, w_k, guidance coefficients) and independent of prediff_amd.schedule:

    x0 = (z - sigma eps) / alpha;  D = x0 + w_k (x0 - x0_prev)
    z_prev = (sigma_prev / sigma) exp(-eta h_k) z - alpha_prev expm1(-(1 + eta) h_k) D + sigma_prev sqrt(-expm1(-2 eta h_k)) n_k

Noise tape: tape[0] = x_T, tape[1 + k] = n_k of the k-th visited step."""
import math

import torch

import _dpmpp_ref as R


def coefficients(v, eta):
    """(c_x, c_d, c_n) of one visited step (a dict of _dpmpp_ref.visits) in Python floats."""
    sigma, alpha_prev, sigma_prev = math.sqrt(1.0 - v["a"]), math.sqrt(v["a_prev"]), math.sqrt(1.0 - v["a_prev"])
    h = v["h"]
    return ((sigma_prev / sigma) * math.exp(-eta * h), -alpha_prev * math.expm1(-(1.0 + eta) * h),
            sigma_prev * math.sqrt(-math.expm1(-2.0 * eta * h)))


def step(z, eps, noise, x0_prev, v, eta):
    """One step in fp64: (z_prev, x0).  x0_prev is not touched where w = 0, noise not where eta = 0."""
    z, eps = z.double(), eps.double()
    alpha, sigma = math.sqrt(v["a"]), math.sqrt(1.0 - v["a"])
    c_x, c_d, c_n = coefficients(v, eta)
    x0 = (z - sigma * eps) / alpha
    D = x0 + v["w"] * (x0 - x0_prev.double()) if v["w"] != 0.0 else x0
    out = c_x * z + c_d * D
    if eta != 0.0:
        out = out + c_n * noise.double()
    return out, x0


def sample_loop(ac, denoiser, zc, tape, n, eta=1.0, method="quad", lower_order_final=None, align_fn=None, logvar_clipped=None):
    """The sampler: fp64 state, the denoiser (and the alignment function) called on the fp32 rounding of it, as the engine's see it.
    align_fn(z, t) -> shift: the guided form, z_prev -= gamma_idx * shift."""
    steps = R.grid(n, ac, method)
    vs = R.visits(ac, steps, lower_order_final)
    gamma = R.gamma_f64(logvar_clipped, steps) if align_fn is not None else None
    z, x0_prev = tape[0].double(), None
    B = z.shape[0]
    for k, v in enumerate(vs):
        t = torch.full((B,), v["t"], dtype=torch.long)
        with torch.no_grad():
            eps = denoiser(z.float(), t, zc)
        shift = align_fn(z.float(), t).detach() if align_fn is not None else None
        z, x0_prev = step(z, eps, tape[1 + k] if eta != 0.0 else None, x0_prev, v, eta)
        if shift is not None:
            z = z - gamma[v["idx"]] * shift.double()
    return z
