"""Stochastic DPM-Solver++(2M) sampler, sampler="dpmpp_2m_sde" (DESIGN.md §7): the coefficient table and its two reductions, the step
kernel, the driver modes of the loop, the guided form and the front ends, against the fp64 restatement in tests/_dpmpp_sde_ref.py, and
the calibration of the final variance on Gaussian data (the quantity an ensemble's spread reports).  Bounds and the tiny model are those
of tests/test_dpmpp_2m.py."""
import math

import numpy as np
import pytest
import torch

import _dpmpp_ref as R
import _dpmpp_sde_ref as RS
import test_dpmpp_2m as D
from _weights import seeded_input
from oracle import diffusion as OD
from oracle import unet as OU
from prediff_amd import schedule as S

T = D.T
rel_l2 = D.rel_l2


def _ac(schedule):
    return np.cumprod(1.0 - OD.beta_schedule(schedule, T, linear_start=1e-4, linear_end=2e-2)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ CPU: schedule
@pytest.mark.parametrize("method,n", [("quad", 10), ("quad", 20), ("quad", 50), ("uniform", 10), ("logsnr", 10)])
@pytest.mark.parametrize("schedule", ["linear", "sqrt_linear"])
def test_table_eta0_is_the_deterministic_table(schedule, method, n):
    ac = _ac(schedule)
    steps = D._product_grid(n, ac, method)
    for lof in (None, True, False):
        table, visited = S.make_dpmpp_2m_sde_coefficients(ac, steps, 0.0, lower_order_final=lof)
        det, det_visited = S.make_dpmpp_2m_coefficients(ac, steps, lower_order_final=lof)
        assert table.dtype == np.float32 and table.shape == (len(det), 5)
        assert np.array_equal(visited, det_visited)
        assert np.array_equal(table[:, :4], det) and (table[:, 4] == 0).all()


@pytest.mark.parametrize("method,n,lof", [("quad", 10, None), ("quad", 20, None), ("quad", 50, None), ("uniform", 10, False),
                                          ("logsnr", 10, True)])
def test_table_eta1(method, n, lof):
    """eta = 1: the restated coefficients, and the first-order member is DDIM at eta = 1 (make_ddim_sampling_parameters' sigma):
    z_prev = alpha_prev x0 + dir eps + sigma n with eps = (z - alpha x0) / sigma_t gives z's coefficient dir / sigma_t and x0's
    alpha_prev - dir alpha / sigma_t.  1e-6 relative: the table is fp32 (2^-24 relative rounding)."""
    ac = _ac("linear")
    steps = D._product_grid(n, ac, method)
    table, visited = S.make_dpmpp_2m_sde_coefficients(ac, steps, 1.0, lower_order_final=lof)
    det, det_visited = S.make_dpmpp_2m_coefficients(ac, steps, lower_order_final=lof)
    vs = R.visits(ac, R.grid(n, ac, method), lof)
    assert table.dtype == np.float32 and table.shape == (len(vs), 5) and np.isfinite(table).all()
    # dropped grid points and lower_order_final as in the deterministic table: the same visit list, a and w columns
    assert np.array_equal(visited, det_visited) and [int(i) for i in visited] == [v["idx"] for v in vs]
    assert np.array_equal(table[:, 0], det[:, 0]) and np.array_equal(table[:, 3], det[:, 3])
    ref = np.asarray([RS.coefficients(v, 1.0) for v in vs])
    assert np.allclose(table[:, [1, 2, 4]].astype(np.float64), ref, rtol=1e-6, atol=0)
    sig, a, a_prev = S.make_ddim_sampling_parameters(ac.astype(np.float64), steps, 1.0)
    sig, a, a_prev = sig[visited], a[visited], a_prev[visited]
    direction = np.sqrt(1.0 - a_prev - sig ** 2)
    t64 = table.astype(np.float64)
    assert np.allclose(t64[:, 1], direction / np.sqrt(1.0 - a), rtol=1e-6, atol=0)
    assert np.allclose(t64[:, 2], np.sqrt(a_prev) - direction * np.sqrt(a) / np.sqrt(1.0 - a), rtol=1e-6, atol=0)
    assert np.allclose(t64[:, 4], sig, rtol=1e-6, atol=0)
    assert (table[:, 4] > 0).all()


def test_table_dropped_points_and_eta_range():
    ac = _ac("linear")
    steps = D._product_grid(50, ac, "quad")
    table, visited = S.make_dpmpp_2m_sde_coefficients(ac, steps, 1.0)
    assert len(np.unique(steps)) < 50 and table.shape == (len(np.unique(steps)), 5) and np.isfinite(table).all()
    assert np.array_equal(np.sort(steps[visited]), np.unique(steps))
    one, _ = S.make_dpmpp_2m_sde_coefficients(ac, np.asarray([T - 1]), 0.5)
    assert one.shape == (1, 5) and one[0, 3] == 0.0 and one[0, 4] > 0
    with pytest.raises(ValueError, match="eta"):
        S.make_dpmpp_2m_sde_coefficients(ac, steps, -0.1)


# ------------------------------------------------------------------------------------------------ CPU: front ends
def test_refusals():
    zc = torch.zeros(2, 3, 4, 4, 1)
    shape = (2, 2, 4, 4, 1)
    kw = dict(cond=zc, batch_size=2, sampler="dpmpp_2m_sde", steps=5, return_decoded=False)
    rng = torch.get_rng_state()
    ldm = D._cpu_ldm(parameterization="x0")
    with pytest.raises(NotImplementedError, match="x0"):
        ldm.dpmpp_2m_sde_sample_loop(zc, shape, steps=5)
    with pytest.raises(NotImplementedError, match="x0"):
        ldm.sample(**kw)
    with pytest.raises(NotImplementedError, match="clip_denoised"):
        D._cpu_ldm(clip_denoised=True).sample(**kw)
    with pytest.raises(NotImplementedError, match="shorten_cond_schedule"):
        D._cpu_ldm(num_timesteps_cond=4).sample(**kw)
    ldm = D._cpu_ldm()
    with pytest.raises(NotImplementedError, match="inpainting"):
        ldm.sample(mask=torch.ones(shape), x0=torch.zeros(shape), **kw)
    for bad in (0, T + 1):
        with pytest.raises(ValueError, match="steps"):
            ldm.sample(**dict(kw, steps=bad))
    with pytest.raises(NotImplementedError, match="discretization"):
        ldm.sample(discretize="cubic", **kw)
    with pytest.raises(ValueError, match="eta"):
        ldm.sample(eta=-1.0, **kw)
    assert torch.equal(torch.get_rng_state(), rng)                         # refused before any draw
    with pytest.raises(NotImplementedError, match="eta"):                  # the deterministic sampler keeps its refusal
        ldm.sample(**dict(kw, sampler="dpmpp_2m", eta=0.5))


def test_sample_routes_keywords():
    ldm = D._cpu_ldm()
    seen = []
    ldm.dpmpp_2m_sde_sample_loop = lambda cond, shape, **kw: (seen.append(kw), torch.zeros(shape))[1]
    for name in ("p_sample_loop", "ddim_sample_loop", "dpmpp_2m_sample_loop"):
        setattr(ldm, name, lambda *a, **k: pytest.fail("another sampler's loop ran"))
    zc = torch.zeros(2, 3, 4, 4, 1)
    kw = dict(cond=zc, batch_size=2, sampler="dpmpp_2m_sde", return_decoded=False)
    ldm.sample(**kw)
    ldm.sample(steps=12, eta=0.5, discretize="logsnr", lower_order_final=False, **kw)
    ldm.sample(ddim_steps=7, eta=0.0, **kw)
    ldm.sample(ddim_steps=7, steps=9, **kw)
    assert [(s["steps"], s["eta"], s["discretize"], s["lower_order_final"]) for s in seen] == \
        [(20, 1.0, "quad", None), (12, 0.5, "logsnr", False), (7, 0.0, "quad", None), (9, 1.0, "quad", None)]


def test_sample_ensemble_forwards_keywords():
    from prediff_amd.ensemble import sample_ensemble

    class Stub:
        latent_shape = (2, 4, 4, 1)

        def __init__(self):
            self.calls = []

        def sample(self, cond, **kw):
            self.calls.append(kw)
            return torch.zeros((kw["batch_size"],) + self.latent_shape)

    ldm = Stub()
    y = torch.rand(1, 3, 4, 4, 1)
    out = sample_ensemble(ldm, {"y": y}, 3, sampler="dpmpp_2m_sde", steps=15, eta=1.0, discretize="uniform", lower_order_final=True,
                          micro_batch=2, return_decoded=False)
    assert out.shape == (3, 2, 4, 4, 1) and [c["batch_size"] for c in ldm.calls] == [2, 1]
    for kw in ldm.calls:
        assert (kw["sampler"], kw["steps"], kw["eta"], kw["discretize"], kw["lower_order_final"]) == \
            ("dpmpp_2m_sde", 15, 1.0, "uniform", True)
        assert "timesteps" not in kw and "ddim_steps" not in kw
    ldm.calls.clear()
    sample_ensemble(ldm, {"y": y}, 2, sampler="dpmpp_2m_sde", return_decoded=False)       # sample_ensemble's own eta default
    assert (ldm.calls[0]["steps"], ldm.calls[0]["eta"], ldm.calls[0]["discretize"]) == (20, 0.0, "quad")


# ------------------------------------------------------------------------------------------------ CPU: calibration
CALIBRATION_C2 = (0.25, 4.0)


def _variance_ratio(z, a0, c2):
    return float(z.var()) / (a0 * c2 + 1.0 - a0)


def _calibration_fp64(table, c2, d, seed):
    """x0 ~ N(0, c2 I) with its exact denoiser eps = sigma z / (a c2 + 1 - a), the loop in fp64 arithmetic on the product's fp32 rows."""
    rng = np.random.default_rng(seed)
    z, hist = rng.standard_normal(d), None
    for a, c_x, c_d, w, c_n in table.astype(np.float64):
        sigma = math.sqrt(1.0 - a)
        x0 = (z - sigma * (sigma * z / (a * c2 + 1.0 - a))) / math.sqrt(a)
        z = c_x * z + c_d * (x0 + w * (x0 - hist) if w != 0 else x0) + c_n * rng.standard_normal(d)
        hist = x0
    return z


@pytest.mark.parametrize("schedule", ["sqrt_linear", "linear"])
def test_calibration_fp64(schedule):
    """var(z_final) / (a_0 c^2 + 1 - a_0) on 2^18 dimensions (sampling error of the variance: sqrt(2 / d) = 0.003), quad-20, eta = 1: the
    sampler within 8 %, the same table with the w column zeroed (DDIM at eta = 1) more than 20 % off.
    Measured: sampler 0.999 - 1.051, first order 0.74 - 0.78."""
    ac = _ac(schedule)
    table, _ = S.make_dpmpp_2m_sde_coefficients(ac, D._product_grid(20, ac, "quad"), 1.0)
    first = table.copy()
    first[:, 3] = 0.0
    for c2 in CALIBRATION_C2:
        r2 = _variance_ratio(_calibration_fp64(table, c2, 2 ** 18, 1), float(ac[0]), c2)
        r1 = _variance_ratio(_calibration_fp64(first, c2, 2 ** 18, 1), float(ac[0]), c2)
        print(f"[calibration fp64 {schedule} c2 {c2}] second order {r2:.4f}, first order {r1:.4f}")
        assert abs(r2 - 1.0) < 0.08, (schedule, c2)
        assert abs(r1 - 1.0) > 0.2, (schedule, c2)


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def _f64_step(zt, eps, noise, hist, coef):
    """(out, x0) of one step from the rows (a_t, c_x, c_d, w, c_n[, gamma]) as the kernel gets them, in fp64; NaN in a buffer the row
    does not read stays out of it."""
    c = coef.double().reshape(coef.shape[0], coef.shape[1], *([1] * (zt.dim() - 1)))
    a, c_x, c_d, w, c_n = c[:, 0], c[:, 1], c[:, 2], c[:, 3], c[:, 4]
    x0 = (zt.double() - (1 - a).sqrt() * eps.double()) / a.sqrt()
    Dk = torch.where(w != 0, x0 + w * (x0 - hist.double()), x0)
    return c_x * zt.double() + c_d * Dk + torch.where(c_n != 0, c_n * noise.double(), torch.zeros_like(x0)), x0


# (a_t, c_x, c_d, w, c_n, gamma): every combination of w = 0 / != 0 and c_n = 0 / != 0 over the two sets
KERNEL_ROWS = {"set 1": [[0.05, 0.90, 0.40, 0.0, 0.0, 2.5], [0.60, 0.80, 0.30, 1.9, 0.35, 0.01], [0.97, 0.50, 0.60, 0.0, 0.15, 0.3]],
               "set 2": [[0.05, 0.90, 0.40, 0.5, 0.0, 2.5], [0.60, 0.80, 0.30, 0.0, 0.0, 0.01], [0.97, 0.50, 0.60, 0.7, 0.15, 0.3]]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KERNEL_ROWS))
def test_step_kernel(name):
    from prediff_amd import _lib as L
    B, per = 3, 1000                          # per_sample not a multiple of 256: the tail of the grid-stride loop
    g = torch.Generator().manual_seed(11)
    zt, eps, noise, hist0, shift = (torch.randn(B, per, generator=g) for _ in range(5))
    coef6 = torch.tensor(KERNEL_ROWS[name], dtype=torch.float32)
    coef5, coef4 = coef6[:, :5].contiguous(), coef6[:, :4].contiguous()
    det = coef6[:, 4] == 0                    # the rows without noise
    noise[det] = float("nan")                 # ... do not read the noise buffer,
    hist0[coef6[:, 3] == 0] = float("nan")    # and the first-order rows do not read the history
    ref, x0 = _f64_step(zt, eps, noise, hist0, coef5)
    dz, de, dn, ds = zt.cuda(), eps.cuda(), noise.cuda(), shift.cuda()
    out, h = torch.empty(B, per).cuda(), hist0.clone().cuda()
    L.dpmpp_2m_sde_step(dz, de, dn, h, coef5.cuda(), out, B, per)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(h).all())
    e, eh = rel_l2(out, ref), rel_l2(h, x0)
    print(f"[pd_dpmpp_2m_sde_step {name}] out rel-L2 {e:.2e}, hist vs x0 {eh:.2e}")
    assert e <= D.STEP_KERNEL_BOUND and eh <= D.STEP_KERNEL_BOUND
    # c_n = 0: pd_dpmpp_2m_step's result bit for bit on those rows (output and history)
    out_d, h_d = torch.empty(B, per).cuda(), hist0.clone().cuda()
    L.dpmpp_2m_step(dz, de, h_d, coef4.cuda(), out_d, B, per)
    assert bool(det.any()) and torch.equal(out[det.cuda()], out_d[det.cuda()]) and torch.equal(h, h_d)
    # guided: against fp64, and a zero shift is the un-guided step bit for bit
    outg, hg = torch.empty_like(out), hist0.clone().cuda()
    L.dpmpp_2m_sde_step_guided(dz, de, dn, hg, ds, coef6.cuda(), outg, B, per)
    eg = rel_l2(outg, ref - coef6[:, 5:6].double() * shift.double())
    print(f"[pd_dpmpp_2m_sde_step_guided {name}] out rel-L2 {eg:.2e}")
    assert eg <= D.STEP_KERNEL_BOUND and torch.equal(hg, h)
    out0, h0 = torch.empty_like(out), hist0.clone().cuda()
    L.dpmpp_2m_sde_step_guided(dz, de, dn, h0, torch.zeros_like(out), coef6.cuda(), out0, B, per)
    assert torch.equal(out0, out) and torch.equal(h0, h)
    with pytest.raises(L.PrediffHipError):
        L.dpmpp_2m_sde_step(dz, de, dn, h, coef5.cuda()[:2], out, B, per)
    with pytest.raises(L.PrediffHipError):
        L.dpmpp_2m_sde_step(dz, de, dn[:2], h, coef5.cuda(), out, B, per)


@pytest.mark.gpu
def test_first_order_member_is_ddim_eta1():
    """w = 0 and eta = 1 rows of the product table against pd_ddim_step at the matching (a, a_prev, sigma) rows: three visited steps of
    quad-10 (the first, a middle one and the last) as the three samples."""
    from prediff_amd import _lib as L
    B, per = 3, 1000
    ac = _ac("linear")
    steps = D._product_grid(10, ac, "quad")
    table, visited = S.make_dpmpp_2m_sde_coefficients(ac, steps, 1.0)
    sig, a, a_prev = S.make_ddim_sampling_parameters(ac.astype(np.float64), steps, 1.0)
    ks = [0, len(visited) // 2, len(visited) - 1]
    coef5 = torch.tensor(table[ks])
    coef5[:, 3] = 0.0
    coef3 = torch.tensor(np.stack([a[visited[ks]], a_prev[visited[ks]], sig[visited[ks]]], axis=1), dtype=torch.float32)
    g = torch.Generator().manual_seed(12)
    zt, eps, noise = (torch.randn(B, per, generator=g).cuda() for _ in range(3))
    out, ref = torch.empty(B, per).cuda(), torch.empty(B, per).cuda()
    L.dpmpp_2m_sde_step(zt, eps, noise, torch.full((B, per), float("nan")).cuda(), coef5.cuda(), out, B, per)
    L.ddim_step(zt, eps, noise, coef3.cuda(), ref, B, per)
    e = [rel_l2(out[b], ref[b]) for b in range(B)]
    print("[first-order member vs pd_ddim_step] rel-L2 per row " + ", ".join(f"{x:.2e}" for x in e))
    assert max(e) <= D.STEP_KERNEL_BOUND


@pytest.mark.gpu
def test_calibration_on_the_kernels():
    """test_calibration_fp64 through pd_dpmpp_2m_sde_step: the product's fp32 table, eps in fp32 torch on the device, 2 x 2^17 elements,
    the "sqrt_linear" schedule.  fp32 rounding (1e-7 per operation over 20 steps) is far below both margins."""
    from prediff_amd import _lib as L
    ac = _ac("sqrt_linear")
    table, _ = S.make_dpmpp_2m_sde_coefficients(ac, D._product_grid(20, ac, "quad"), 1.0)
    first = table.copy()
    first[:, 3] = 0.0
    B, per = 2, 2 ** 17

    def run(tab, c2):
        g = torch.Generator(device="cuda").manual_seed(1)
        coefs = torch.tensor(tab).cuda()
        z, hist = torch.randn(B, per, generator=g, device="cuda"), torch.full((B, per), float("nan")).cuda()
        for k in range(len(tab)):
            a = float(tab[k, 0])
            eps = (math.sqrt(1.0 - a) / (a * c2 + 1.0 - a)) * z
            out = torch.empty_like(z)
            L.dpmpp_2m_sde_step(z, eps, torch.randn(B, per, generator=g, device="cuda"), hist, coefs[k].expand(B, 5).contiguous(), out, B, per)
            z = out
        return _variance_ratio(z.double().cpu().numpy(), float(ac[0]), c2)
    for c2 in CALIBRATION_C2:
        r2, r1 = run(table, c2), run(first, c2)
        print(f"[calibration on the kernels c2 {c2}] second order {r2:.4f}, first order {r1:.4f}")
        assert abs(r2 - 1.0) < 0.08, c2
        assert abs(r1 - 1.0) > 0.2, c2


# ------------------------------------------------------------------------------------------------ GPU: the loop
def _tape(shape, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) for _ in range(n + 1)]


@pytest.mark.gpu
def test_tiny_sample_vs_restatement_loop():
    """sample(sampler="dpmpp_2m_sde", steps=10, eta=1) on the tiny model against the restatement loop driven by the CPU oracle denoiser,
    one noise tape for both.  Bound: the precision's DDIM-10 bound times (1 + 2 max_k w_k) of the grid, as for the deterministic
    solver (the first-order member is DDIM at eta = 1, which the DDIM-10 bound covers).  At eta = 0: sampler="dpmpp_2m" bit for bit."""
    B, n = 2, 10
    ac = D._ac_linear()
    for method in ("quad", "logsnr"):
        ref, factor = None, D._factor(n, method)
        for precision in ("fp32", "bf16"):
            ldm, cfg, sd = D._tiny_ldm(precision)
            zc = seeded_input("dzc", (B,) + tuple(cfg["input_shape"]), 5)
            tape = _tape(ldm.get_batch_latent_shape(B), n, 3)
            if ref is None:
                ref = RS.sample_loop(ac, lambda z, t, c: OU.unet_forward(sd, cfg, z, t, c), zc, tape, n, 1.0, method)
            kw = dict(cond=zc.cuda(), batch_size=B, return_decoded=False, steps=n, discretize=method)
            out = ldm.sample(sampler="dpmpp_2m_sde", eta=1.0, noise_tape=tape, **kw)
            e = rel_l2(out, ref)
            print(f"[tiny 2M-SDE-{n} {method} {precision}] rel-L2 vs the restatement loop {e:.3e} "
                  f"(bound {D.DDIM10_BOUND[precision]:.0e} x {factor:.3f})")
            assert e < D.DDIM10_BOUND[precision] * factor, (method, precision)
            det = ldm.sample(sampler="dpmpp_2m", x_T=tape[0].cuda(), **kw)
            assert torch.equal(ldm.sample(sampler="dpmpp_2m_sde", eta=0.0, noise_tape=tape, **kw), det), (method, precision)
            assert rel_l2(out, det) > 1e-1                                 # the noise is in the sample


@pytest.mark.gpu
def test_modes_agree_and_replays_are_clean():
    """Lanes, the single graph and the eager loop give the same latents bit for bit from one tape; the same graphs replayed with another
    tape equal that tape's eager run (no history or noise of the first run survives); without a tape a seed fixes the run."""
    ldm, cfg, _ = D._tiny_ldm("bf16")
    B, n = 4, 6
    zc = seeded_input("dzc4", (B,) + tuple(cfg["input_shape"]), 5).cuda()
    shape = ldm.get_batch_latent_shape(B)
    tapes = [_tape(shape, n, 17), _tape(shape, n, 18)]
    kw = dict(cond=zc, batch_size=B, return_decoded=False, sampler="dpmpp_2m_sde", steps=n, eta=1.0, lower_order_final=False)
    outs = {}
    for lanes in (2, 1):
        ldm.num_streams = lanes
        outs[lanes] = [ldm.sample(noise_tape=tp, **kw) for tp in tapes]   # the second tape replays the first one's graphs
        assert lanes == 1 or 1 in ldm._graphs                             # the second lane's graph: the batch did run as lanes
        assert torch.equal(ldm.sample(noise_tape=tapes[0], **kw), outs[lanes][0]), lanes
    graph, inter = ldm.dpmpp_2m_sde_sample_loop(zc, shape, steps=n, eta=1.0, lower_order_final=False, noise_tape=tapes[0],
                                                return_intermediates=True)
    assert len(inter) == n + 1 and torch.equal(inter[-1], graph)
    ldm.use_hip_graph = False
    eager = [ldm.sample(noise_tape=tp, **kw) for tp in tapes]
    assert bool(torch.isfinite(eager[0]).all()) and not torch.equal(eager[0], eager[1])
    for i in range(2):
        assert torch.equal(outs[2][i], eager[i]) and torch.equal(outs[1][i], eager[i]), i
    assert torch.equal(graph, eager[0])
    # device draws when no tape is given: x_T, then one whole-batch draw per step
    for lanes, graph_mode in ((2, True), (1, True), (1, False)):
        ldm.num_streams, ldm.use_hip_graph = lanes, graph_mode
        torch.manual_seed(5)
        a = ldm.sample(**kw)
        torch.manual_seed(5)
        assert torch.equal(a, ldm.sample(**kw)), (lanes, graph_mode)
        assert not torch.equal(a, ldm.sample(**kw))


@pytest.mark.gpu
def test_guided_runs():
    """A zero alignment function gives the un-guided run bit for bit (graphs and eager); the guided run against the guided restatement
    loop stays within the guided-DDIM bound times the grid's factor."""
    from test_alignment import _tiny_alignment
    ldm, cfg, sd = D._tiny_ldm("fp32")
    B, n = 2, 10
    zc = seeded_input("gdzc", (B,) + tuple(cfg["input_shape"]), 21)
    tape = _tape(ldm.get_batch_latent_shape(B), n, 22)
    kw = dict(cond=zc.cuda(), batch_size=B, return_decoded=False, sampler="dpmpp_2m_sde", steps=n, eta=1.0, noise_tape=tape)
    plain = ldm.sample(**kw)
    ldm.set_alignment(lambda zt, t, zc=None, y=None, **k: torch.zeros_like(zt))
    for graph in (True, False):
        ldm.use_hip_graph = graph
        assert torch.equal(ldm.sample(use_alignment=True, **kw), plain), graph
    ldm.use_hip_graph = True
    al_cpu, al = _tiny_alignment(), _tiny_alignment()
    al.model.cuda()
    ldm.set_alignment(al.get_mean_shift)
    avg = torch.tensor([[0.4], [0.1]])
    ak = {"avg_x_gt": avg.cuda()}
    lv = OD.schedule_buffers(OD.beta_schedule("linear", T))["posterior_log_variance_clipped"]
    ref = RS.sample_loop(D._ac_linear(), lambda z, t, c: OU.unet_forward(sd, cfg, z, t, c), zc, tape, n, 1.0, "quad",
                         align_fn=lambda z, t: al_cpu.get_mean_shift(z, t, avg_x_gt=avg), logvar_clipped=lv)
    out = ldm.sample(use_alignment=True, alignment_kwargs=ak, **kw)
    e, d, factor = rel_l2(out, ref), rel_l2(out, plain), D._factor(n, "quad")
    print(f"[tiny guided 2M-SDE-{n}] rel-L2 vs the restatement loop {e:.3e} (bound {D.GUIDED_DDIM10_BOUND:.0e} x {factor:.3f}); "
          f"guided vs un-guided {d:.3e}")
    assert e < D.GUIDED_DDIM10_BOUND * factor
    assert d > 3e-2                          # the guidance moves the sample far beyond the parity bar
    ldm.use_hip_graph = False
    assert torch.equal(ldm.sample(use_alignment=True, alignment_kwargs=ak, **kw), out)


@pytest.mark.gpu
def test_ensemble_is_batch_split_invariant():
    """A member depends on (base_seed, member id) only: its tape is its own generator's draws in step order."""
    from prediff_amd.ensemble import sample_ensemble
    ldm, cfg, _ = D._tiny_ldm("fp32")
    zc = seeded_input("dzc", (1,) + tuple(cfg["input_shape"]), 5).cuda()
    kw = dict(base_seed=1000, sampler="dpmpp_2m_sde", steps=5, return_decoded=False)
    a = sample_ensemble(ldm, zc, 4, eta=1.0, micro_batch=4, **kw)
    b = sample_ensemble(ldm, zc, 4, eta=1.0, micro_batch=2, **kw)
    det = sample_ensemble(ldm, zc, 4, eta=0.0, **kw)
    assert a.shape == (4,) + tuple(cfg["target_shape"]) and bool(torch.isfinite(a).all())
    print(f"[ensemble 2M-SDE-5] micro_batch 4 vs 2 rel-L2 {rel_l2(b, a):.3e}; eta 1 vs eta 0 {rel_l2(a, det):.3e}")
    assert torch.equal(a, b)
    assert rel_l2(a, det) > 1e-1 and rel_l2(a[0], a[1]) > 1e-2
    assert torch.equal(det, sample_ensemble(ldm, zc, 4, **dict(kw, sampler="dpmpp_2m")))
