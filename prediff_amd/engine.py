"""What CuboidTransformerUNet and AutoencoderKL share as HIP engines: the precision switch, the workspace, the packed-weight cache,
the GEMM activation operand and the one helper every weight launch (pd_igemm against a packed weight record) goes through."""
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from .packing import pad64


class Act(NamedTuple):
    """A operand of a pd_igemm launch: rows of `ld` elements.  scale None: 16-bit rows, `lo` the low halves of the hi/lo engine (else
    None).  scale a float: `hi` holds e4m3 rows of value * scale.  mx a tensor: `hi` holds the e4m3 payload of an MX operand and `mx`
    its E8M0 block scales (rows of ld / 32 bytes)."""
    hi: torch.Tensor
    lo: Optional[torch.Tensor]
    ld: int
    scale: Optional[float] = None
    mx: Optional[torch.Tensor] = None


class HipEngine:
    """Mixin of the two model engines (not an nn.Module).  A subclass supplies `_pack(device)` and may extend `_params_key` /
    `_after_pack`; a `_ws_slot` attribute, where it has one, selects the workspace set."""

    def _init_engine(self, precision, allowed):
        if precision not in allowed:
            raise ValueError(f"precision must be one of {', '.join(map(repr, allowed))}; got {precision!r}")
        self.operand = "fp16" if precision.startswith("fp16") else "bf16"
        # per-call options handed to every launch of this module (operand type + A/B switches: bench.py / scripts set attributes here;
        # nothing is process-global, two modules in one process do not see each other's settings)
        self.opts = L.CallOpts(self.operand)
        self.op_dtype = self.opts.dtype
        # "bf16" = the single-pass 16-bit-operand engine (whatever the operand type, e4m3 layers included), "fp32" = the hi/lo engine
        self.precision = precision if precision in ("bf16", "fp32") else "bf16"
        self._packed = self._packed_key = None
        self._ws = {}

    # ------------------------------------------------------------------------------------------------ packed weights
    def _params_key(self, device):
        return (str(device), self.precision, self.operand) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _after_pack(self, device):
        pass

    def _ensure_packed(self, device):
        key = self._params_key(device)
        if key != self._packed_key:
            L.lib()   # fail loudly before any work if the extension is missing
            self._packed = self._pack(device)
            self._packed_key = key
            self._after_pack(device)
        return self._packed

    # ------------------------------------------------------------------------------------------------ workspace
    def _buf(self, name, shape, dtype, device):
        key = (name, tuple(shape), dtype, str(device), getattr(self, "_ws_slot", 0))
        t = self._ws.get(key)
        if t is None:
            t = torch.zeros(shape, dtype=dtype, device=device)
            self._ws[key] = t
        return t

    def _bf(self, name, rows, cols, device):
        """16-bit operand buffer pair (hi, lo-or-None)."""
        if self.precision == "fp32":      # both halves in one allocation: the 256 x 256 hi/lo kernel reads them through one buffer descriptor
            both = self._buf(name + ".hilo", (2, rows, cols), torch.bfloat16, device)
            return both[0], both[1]
        return self._buf(name, (rows, cols), self.op_dtype, device), None

    # ------------------------------------------------------------------------------------------------ operand producers
    def _cast(self, x, name, rows, C, dev, samples=1, rows_in=None, row_off=0) -> Act:
        """`rows` fp32 rows of each sample (from row `row_off` of its `rows_in`) -> 16-bit operand rows."""
        ld = pad64(C)
        a = self._bf(name, samples * rows, ld, dev)
        L.cast_rows(x, *a, samples, rows if rows_in is None else rows_in, row_off, rows, C, C, ld, opts=self.opts)
        return Act(*a, ld)

    def _gn_args(self, B, S, C, G, dev, ss=None):
        """What every GroupNorm launch takes beside its output: the fp64 partial-sum workspace and the scale-shift keywords of `ss`
        ((B, 2 C) fp32 rows, scale then shift; None: no scale-shift)."""
        part = self._buf("gn.part", (B * L.groupnorm_nchunk(S, C) * G * 2,), torch.float64, dev)
        return part, (dict(ss_scale=ss, ss_shift=ss[:, C:], ld_ss=2 * C) if ss is not None else {})

    def _groupnorm(self, x, g, beta, B, S, C, G, name, dev, eps, silu=True, ss=None, opts=None) -> Act:
        """GroupNorm [-> scale-shift `ss`] [-> SiLU] of channels-last fp32 x (B, S, C) -> 16-bit operand rows."""
        ld = pad64(C)
        a = self._bf(name, B * S, ld, dev)
        part, kw = self._gn_args(B, S, C, G, dev, ss)
        L.groupnorm_silu(x, g, beta, part, *a, B, S, C, G, ld, eps, silu=silu, **kw, opts=opts or self.opts)
        return Act(*a, ld)

    # ------------------------------------------------------------------------------------------------ the weight launch
    def _gemm(self, P, name, act, /, *, M, N, taps=1, geom=None, alpha=1.0, **epilogue):
        """One pd_igemm launch of `act` against the packed weight record of layer `name` in P (+ its bias): the e4m3 record `.w8` where
        the operand is e4m3 (both tensor scales go into alpha), the MX record `.wmx` (pd_igemm_mx) where it is an MX operand, else `.w`.
        `epilogue`: the other keywords of `_lib.igemm`."""
        if act.mx is not None:
            w, ws = P[name + ".wmx"]                        # (e4m3 payload, E8M0 block scales)
            if epilogue.pop("out_bf16_lo", None) is not None or epilogue.pop("out_fp8_log2", 0):
                raise L.PrediffHipError(f"{name}: an MX launch writes fp32 or bfloat16 rows only (no low halves, no e4m3 output)")
            L.igemm_mx(act.hi, act.mx, w, ws, M=M, N=N, taps=taps, geom=geom, bias=P.get(name + ".b"), alpha=alpha, **epilogue, opts=self.opts)
            return
        fp8 = act.scale is not None
        w, w2 = P[name + (".w8" if fp8 else ".w")]          # (e4m3 weights, their scale) | (hi, lo-or-None)
        folded = not fp8 and w.dim() == 3 and w.shape[0] == 2 * taps
        if folded and not getattr(w, "_pd_fold", False):
            # `_lib.igemm` knows hi + lo slabs by this tag alone; a .clone() / .to() / view drops it, and the launch would read the hi half only
            raise L.PrediffHipError(f"{name}: the packed weight has the folded (hi + lo) shape {tuple(w.shape)} for {taps} tap(s) but has "
                                    f"lost its `_pd_fold` tag (a copy or a view of a packing.fold_weights result): pack it again")
        # the tap stride is N * ld for a convolution record (one (N, ld) slab per tap) and 0 for a linear layer's ((N, ld), or its folded
        # (2, N, ld) pair).  The rank test is there for the one-tap convolutions launched without a geometry (the VAE's 1x1 Conv2d, a
        # (1, N, ld) record): the library never reads the stride at one tap, but the launch keeps the arguments it always had
        per_tap = geom is not None or (w.dim() == 3 and not folded)
        if fp8:
            alpha, w2 = alpha / (act.scale * w2), None
        L.igemm(act.hi, w, A_lo=act.lo, W_lo=w2, M=M, N=N, Cin=act.ld, taps=taps, w_tap_stride=N * act.ld if per_tap else 0, geom=geom,
                bias=P.get(name + ".b"), alpha=alpha, fp8=fp8, **epilogue, opts=self.opts)
