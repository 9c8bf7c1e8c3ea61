"""The norm family of csrc/norm.hip restated on the CPU, and the per-element criterion its outputs are held to.  No GPU, no kernel code.

Three layers:
  references   each op in plain torch.float64 (ln_ref, gather_ref, gn_ref, gn_stats_ref, gn_bwd_ref, cast_rows_ref) and torch's OWN fp32
               evaluation of the same op (F.layer_norm, F.group_norm, fp32 autograd), whose error against fp64 is the yardstick e32
  formats      decode(buffers) -> fp64 and q(ref) = the CPU cast of the reference into the buffer's format, for the 16-bit operand, the
               bf16 hi/lo pair, unit-scale e4m3 and MX
  verify       every element of every buffer of a case (tests/test_norm_bits.py records each case's inputs as a `spec`):
                   |decode(got_i) - ref_i| <= |q(ref_i) - ref_i| + 4 * e32
               pad columns decode to exactly 0, guard bytes behind a buffer stay 0x55.  Rounding to a grid moves a value's distance to
               the grid by at most the value's own error, so a kernel whose fp32 result is within 2 * e32 of fp64 always passes: the 4
               covers another summation order and the hardware rsqrt / fast exp.
`synthesize` builds the buffers a perfect kernel would return (q(ref) encoded); tests/test_norm_ref_host.py runs `verify` on them.
"""
import torch
import torch.nn.functional as F

import _mx_ref as MX

F64, F32 = torch.float64, torch.float32
E4M3_MAX = 448.0
SLACK = 4.0                       # x e32
STAT_REL = 2.0 ** -22             # statistics: fp32 roundings of an fp64 computation (two half-ulps, twice)


# ------------------------------------------------------------------------------------------------ references
def ln_ref(x, gamma, beta, eps):
    """LayerNorm over the last axis: fp64 spelled out; fp32 = torch's own kernel"""
    if x.dtype == F32:
        return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def gather_ref(x, ds, nearest):
    """patch merge: (B, T, H, W, C) padded up to multiples of ds (zeros, or torch's nearest resize), ds-blocks -> rows of dt*dh*dw*C"""
    B, T, H, W, C = x.shape
    To, Ho, Wo = (-(-n // d) for n, d in zip((T, H, W), ds))
    Tp, Hp, Wp = To * ds[0], Ho * ds[1], Wo * ds[2]
    if nearest:
        xp = F.interpolate(x.permute(0, 4, 1, 2, 3), size=(Tp, Hp, Wp), mode="nearest").permute(0, 2, 3, 4, 1)
    else:
        xp = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H, 0, Tp - T))
    return xp.reshape(B, To, ds[0], Ho, ds[1], Wo, ds[2], C).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B * To * Ho * Wo, ds[0] * ds[1] * ds[2] * C)


def gn_stats_ref(x, G):
    """x (B, S, C) -> mean, biased variance, each (B, G)"""
    B, S, C = x.shape
    xg = x.reshape(B, S, G, C // G)
    mean = xg.mean((1, 3))
    return mean, ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))


def gn_ref(x, G, gamma, beta, eps, ss_scale=None, ss_shift=None, silu=False):
    """GroupNorm on channels-last (B, S, C) [-> (1 + scale) y + shift per sample] [-> SiLU]"""
    B, S, C = x.shape
    if x.dtype == F32:
        y = F.group_norm(x.permute(0, 2, 1), G, gamma, beta, eps).permute(0, 2, 1)
    else:
        mean, var = gn_stats_ref(x, G)
        cpg = C // G
        mean, rstd = (t.repeat_interleave(cpg, 1)[:, None, :] for t in (mean, 1.0 / torch.sqrt(var + eps)))
        y = (x - mean) * rstd * gamma + beta
    if ss_scale is not None:
        y = y * (1 + ss_scale[:, None, :]) + ss_shift[:, None, :]
    if silu:
        y = F.silu(y) if x.dtype == F32 else y / (1 + torch.exp(-y))
    return y


def gn_bwd_ref(x, dy, G, gamma, beta, eps):
    """dx of sum(dy * SiLU(GroupNorm(x))) by autograd in x's dtype"""
    xr = x.clone().requires_grad_(True)
    (gn_ref(xr, G, gamma, beta, eps, silu=True) * dy).sum().backward()
    return xr.grad


def gn_bwd_sums_ref(x, dy, G, gamma, beta, eps):
    """the backward's partial sums per (sample, group): sum dxh, sum dxh xh with xh = (x - mean) rstd, n = gamma xh + beta,
    dxh = dy SiLU'(n) gamma -- and sum |dxh|, sum |dxh xh| (the magnitude their fp32 terms are formed at).  (B, G) each"""
    B, S, C = x.shape
    mean, var = gn_stats_ref(x, G)
    cpg = C // G
    mean, rstd = (t.repeat_interleave(cpg, 1)[:, None, :] for t in (mean, 1.0 / torch.sqrt(var + eps)))
    xh = (x - mean) * rstd
    n = gamma * xh + beta
    sig = torch.sigmoid(n)
    dxh = dy * sig * (1 + n * (1 - sig)) * gamma
    red = lambda t: t.reshape(B, S, G, cpg).sum((1, 3))
    return red(dxh), red(dxh * xh), red(dxh.abs()), red((dxh * xh).abs())


def cast_rows_ref(x, row_off, rows_out):
    """(n, rows_in, C) -> rows [row_off, row_off + rows_out) of every sample, (n * rows_out, C)"""
    return x[:, row_off:row_off + rows_out].reshape(-1, x.shape[-1])


# ------------------------------------------------------------------------------------------------ formats
def _np(t):
    return t.detach().cpu().numpy()


def q16(ref, fmt):
    """ref (fp64 tensor) -> the buffers of the 16-bit kinds: {"out": ..} or {"out": hi, "lo": bf16(ref - hi)}"""
    if fmt == "hilo":
        hi = ref.to(torch.bfloat16)
        return {"out": hi, "lo": (ref - hi.double()).to(torch.bfloat16)}
    return {"out": ref.to(torch.float16 if fmt == "fp16" else torch.bfloat16)}


def q_e4m3(ref, scale):
    """bytes of e4m3(ref * scale), saturating at +-448 before rounding"""
    return (ref * scale).clamp(-E4M3_MAX, E4M3_MAX).to(F32).to(torch.float8_e4m3fn).view(torch.uint8)


def dec_e4m3(b, scale):
    return b.view(torch.float8_e4m3fn).double() / scale


def q_mx(ref, ld):
    payload, scales = MX.quantize(_np(ref.to(F32)), ld)
    return torch.from_numpy(payload), torch.from_numpy(scales)


def dec_mx(payload, scales):
    return torch.from_numpy(MX.dequantize(_np(payload), _np(scales)))


# ------------------------------------------------------------------------------------------------ a case's expectation
def _cpu(spec, dtype):
    return {k: (v.detach().cpu().to(dtype) if torch.is_tensor(v) else v) for k, v in spec.items()}


def _forward(s):
    """the value tensor of a forward case, (rows, C), in the dtype of s["x"]"""
    op = s["op"]
    if op == "layernorm":
        return ln_ref(s["x"], s["gamma"], s["beta"], s["eps"])
    if op == "patch_merge_layernorm":
        return ln_ref(gather_ref(s["x"], s["ds"], s["nearest"]), s["gamma"], s["beta"], s["eps"])
    if op == "groupnorm":
        return gn_ref(s["x"], s["G"], s["gamma"], s["beta"], s["eps"], s.get("ss_scale"), s.get("ss_shift"), s["silu"]).reshape(-1, s["x"].shape[-1])
    if op == "cast_rows":
        return cast_rows_ref(s["x"], s["row_off"], s["rows_out"])
    raise KeyError(op)


def _maxerr(a32, a64):
    return float((a32.double() - a64).abs().max())


class Check:
    """one comparison: `got` against `ref` with a per-element `bound`, all (rows, cols) fp64; `what` names the buffer(s).  cpg: channels
    per group of a (rows, channels) check; cols: the column names of a per-(sample, group) check, whose rows are sample * G + group"""

    def __init__(self, what, ref, bound, decode, cpg=None, cols=None):
        self.what, self.ref, self.bound, self.decode, self.cpg, self.cols = what, ref, bound, decode, cpg, cols


def expectation(spec):
    """spec (tensors anywhere) -> (checks, pads): checks = [Check]; pads = [(buffer, first pad column)] whose columns from there on are 0"""
    s64, s32 = _cpu(spec, F64), _cpu(spec, F32)
    op, fmt = spec["op"], spec.get("fmt")
    checks, pads = [], []
    if op in ("layernorm", "patch_merge_layernorm", "groupnorm", "cast_rows"):
        ref = _forward(s64)
        slack = SLACK * _maxerr(_forward(s32), ref)
        C = ref.shape[1]
        cpg = C // spec["G"] if op == "groupnorm" else None
        if fmt == "e4m3":
            sc = spec["fp8_scale"]
            ref = ref.clamp(-E4M3_MAX / sc, E4M3_MAX / sc)
            q = dec_e4m3(q_e4m3(ref, sc), sc)
            checks.append(Check("out", ref, (q - ref).abs() + slack, lambda b: dec_e4m3(b["out"], sc)[:, :C], cpg))
            pads.append(("out", C))
        elif fmt == "mx":
            q = dec_mx(*q_mx(ref, spec["ld"]))[:, :C]
            checks.append(Check("out*scales", ref, (q - ref).abs() + slack, lambda b: dec_mx(b["out"], b["scales"])[:, :C], cpg))
            pads += [("out", C), ("scales", C // 32)]
        else:
            qb = q16(ref, fmt)
            q = sum(t.double() for t in qb.values())
            checks.append(Check("+".join(qb), ref, (q - ref).abs() + slack, lambda b: sum(b[k].double() for k in qb)[:, :C], cpg))
            pads += [(k, C) for k in qb]
    if op in ("groupnorm", "groupnorm_stats", "groupnorm_bwd"):
        # (mean, rstd) per (sample, group): the stats buffer is an fp32 rounding of an fp64 computation; the partial sums, summed over
        # the chunks, are read as every consumer reads them (mean = sum / n, var = sumsq / n - mean^2 in fp64) and may carry the fp32
        # mean and variance of the one-pass kernels: torch's fp32 var_mean is their yardstick
        x64, G, eps = s64["x"], spec["G"], spec["eps"]
        mean, var = gn_stats_ref(x64, G)
        ref = torch.stack((mean, 1.0 / torch.sqrt(var + eps)), -1).reshape(-1, 2)
        bound = torch.stack((torch.full_like(mean, STAT_REL * float(x64.abs().max())), STAT_REL * ref[:, 1].reshape(mean.shape)), -1).reshape(-1, 2)
        xg = s32["x"].reshape(x64.shape[0], x64.shape[1], G, -1)
        v32, m32 = torch.var_mean(xg, dim=(1, 3), unbiased=False)
        e32 = (torch.stack((m32.double(), 1.0 / torch.sqrt(v32.double() + eps)), -1).reshape(-1, 2) - ref).abs().max(0).values
        nchunk, cnt = spec["nchunk"], x64.shape[1] * (x64.shape[2] // G)

        def from_partials(key):
            def dec(b):
                p = b[key].double().reshape(x64.shape[0], nchunk, G, 2).sum(1)
                m = p[..., 0] / cnt
                return torch.stack((m, 1.0 / torch.sqrt((p[..., 1] / cnt - m * m).clamp_min(0) + eps)), -1).reshape(-1, 2)
            return dec
        pkey = "fwd_partials" if op == "groupnorm_bwd" else "partials"
        checks.append(Check(pkey + "->(mean,rstd)", ref, bound + SLACK * e32, from_partials(pkey), cols=("mean", "rstd")))
        if op == "groupnorm_stats":
            checks.append(Check("stats", ref, bound, lambda b: b["stats"].double().reshape(-1, 2), cols=("mean", "rstd")))
    if op == "groupnorm_bwd":
        args = lambda s: (s["x"], s["dy"], spec["G"], s["gamma"], s["beta"], spec["eps"])
        ref = gn_bwd_ref(*args(s64))
        C = ref.shape[-1]
        slack = SLACK * _maxerr(gn_bwd_ref(*args(s32)), ref)
        checks.append(Check("dx", ref.reshape(-1, C), torch.full((ref.numel() // C, C), slack, dtype=F64), lambda b: b["dx"].double().reshape(-1, C), C // G))
        # the backward's own partial sums, fp64 sums of terms formed in fp32.  Format term: half an ulp of each term's magnitude (what
        # an fp32 term cannot hold, as q(ref) for a 16-bit output; same factor).  Slack: torch's fp32 evaluation of the same sums, as
        # everywhere -- it carries what the fp32 mean and rstd inside xh cost on this input
        s1, s2, a1, a2 = gn_bwd_sums_ref(*args(s64))
        t1, t2, _, _ = gn_bwd_sums_ref(*args(s32))
        e32 = torch.stack(((t1.double() - s1).abs().max(), (t2.double() - s2).abs().max()))
        checks.append(Check("bwd_partials", torch.stack((s1, s2), -1).reshape(-1, 2),
                            SLACK * (2.0 ** -24 * torch.stack((a1, a2), -1).reshape(-1, 2) + e32),
                            lambda b: b["bwd_partials"].double().reshape(x64.shape[0], nchunk, G, 2).sum(1).reshape(-1, 2), cols=("sum dxh", "sum dxh*xh")))
    assert checks, op
    return checks, pads


# ------------------------------------------------------------------------------------------------ verify / synthesize
def verify(name, spec, bufs, guards=()):
    """-> one report line per check; AssertionError naming the worst element.  bufs / guards: tensors on any device"""
    b = {k: v.detach().cpu() for k, v in bufs.items() if v is not None}
    checks, pads = expectation(spec)
    lines, failed, seen = [], [], set()
    for ch in checks:
        got = ch.decode(b)
        assert got.shape == ch.ref.shape, f"{name} {ch.what}: decoded {tuple(got.shape)}, reference {tuple(ch.ref.shape)}"
        err = (got - ch.ref).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
        ratio = torch.where(err == 0, torch.zeros_like(err), err / ch.bound)          # (a zero bound: 0 where exact, inf elsewhere)
        i = int(ratio.argmax())
        r, c = divmod(i, got.shape[1])
        if ch.cols:
            where = f"sample {r // spec['G']}, group {r % spec['G']}, {ch.cols[c]}"
        else:
            where = f"row {r}, channel {c}" + (f", group {c // ch.cpg}" if ch.cpg else "")
        line = (f"{name} {ch.what}: max err / bound {float(ratio.flatten()[i]):.3g} over {got.numel()} elements; worst at {where}: "
                f"got {float(got.flatten()[i]):.9g} ref {float(ch.ref.flatten()[i]):.9g} err {float(err.flatten()[i]):.3e} bound {float(ch.bound.flatten()[i]):.3e}")
        lines.append(line)
        if not bool((err <= ch.bound).all()):
            failed.append(f"{int((~(err <= ch.bound)).sum())} elements out of bound -- {line}")
        seen.update(ch.what.replace("->(mean,rstd)", "").replace("*", "+").split("+"))
    assert not failed, "\n".join(failed)
    for key, c0 in pads:
        raw = b[key].view(torch.uint8).reshape(b[key].shape[0], -1)
        pad = raw[:, c0 * b[key].element_size():]
        bad = pad.nonzero()
        assert bad.numel() == 0, f"{name} {key}: pad byte at row {int(bad[0, 0])}, column {c0 + int(bad[0, 1]) // b[key].element_size()} is {int(pad[tuple(bad[0])]):#x}, not 0"
        if pad.numel():
            lines.append(f"{name} {key}: {pad.numel()} pad bytes zero")
    assert seen == set(b), f"{name}: buffers never compared: {sorted(set(b) - seen)}"
    for key, g in guards:
        g = g.detach().cpu()
        bad = (g != 0x55).nonzero()
        assert bad.numel() == 0, f"{name} {key}: byte {int(bad[0])} behind the buffer overwritten with {int(g[int(bad[0])]):#x}"
    return lines


def synthesize(spec):
    """the buffers of a kernel that returns q(fp64 reference): the reference inside its own bound, nothing else"""
    s64 = _cpu(spec, F64)
    op, fmt, out = spec["op"], spec.get("fmt"), {}
    if op in ("layernorm", "patch_merge_layernorm", "groupnorm", "cast_rows"):
        ref = _forward(s64)
        rows, C, ld = ref.shape[0], ref.shape[1], spec["ld"]
        full = torch.zeros(rows, ld, dtype=F64)
        full[:, :C] = ref
        if fmt == "e4m3":
            out["out"] = q_e4m3(full, spec["fp8_scale"])
        elif fmt == "mx":
            out["out"], out["scales"] = q_mx(ref, ld)
        else:
            out.update(q16(full, fmt))
    if op in ("groupnorm", "groupnorm_stats", "groupnorm_bwd"):
        x, G, nchunk = s64["x"], spec["G"], spec["nchunk"]
        B, S, C = x.shape
        xg = x.reshape(B, S, G, C // G)
        p = torch.zeros(B, nchunk, G, 2, dtype=F64)
        p[:, 0, :, 0], p[:, 0, :, 1] = xg.sum((1, 3)), (xg * xg).sum((1, 3))
        out["fwd_partials" if op == "groupnorm_bwd" else "partials"] = p.reshape(-1)
        if op == "groupnorm_stats":
            mean, var = gn_stats_ref(x, G)
            out["stats"] = torch.stack((mean, 1.0 / torch.sqrt(var + spec["eps"])), -1).to(F32)
    if op == "groupnorm_bwd":
        args = (s64["x"], s64["dy"], spec["G"], s64["gamma"], s64["beta"], spec["eps"])
        out["dx"] = gn_bwd_ref(*args).to(F32)
        s1, s2, _, _ = gn_bwd_sums_ref(*args)
        p = torch.zeros(x.shape[0], spec["nchunk"], spec["G"], 2, dtype=F64)
        p[:, 0, :, 0], p[:, 0, :, 1] = s1, s2
        out["bwd_partials"] = p.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------ ill-conditioned inputs
FAMILIES = ("plus30", "plus100", "near_constant", "channel_means", "constant_group", "zero_sample")


def family_input(family, shape, cpg, seed):
    """fp32 x of `shape` (.., C), seeded on the CPU.  cpg: channels per group (LayerNorm rows: the whole row is the group, cpg = 4 is
    only the period of channel_means).  The first axis is the sample (GroupNorm, patch merge) or the row (LayerNorm)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.randn(shape, generator=gen, dtype=F64)
    C = shape[-1]
    if family == "plus30":
        x = r + 30
    elif family == "plus100":
        x = r + 100
    elif family == "near_constant":
        x = 1 + 1e-3 * r
    elif family == "channel_means":
        x = r + 50.0 * (torch.arange(C) % cpg)
    elif family == "constant_group":
        # 2.5: its multiples are exact in fp32 in every summation order, so an fp32 mean is 2.5 and the reference's `beta` is what fp32 can give
        x = r
        if len(shape) == 3:
            g = 1 if C // cpg > 1 else 0
            x[0, :, g * cpg:(g + 1) * cpg] = 2.5         # sample 0, group 1
        elif len(shape) == 5:
            x[0, 0, 0:2, 0:2, :] = 2.5                   # the four pixels of merged row 0
        else:
            x[1] = 2.5                                   # row 1
    elif family == "zero_sample":
        x = r
        x[0] = 0.0
    else:
        raise KeyError(family)
    return x.to(F32)
