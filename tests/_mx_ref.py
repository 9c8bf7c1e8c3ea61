"""The MX (OCP microscaling) e4m3 format of prediff_amd, restated in numpy.  Pure CPU, no torch.

A block is 32 consecutive elements along K.  Its scale is an E8M0 byte b standing for 2^(b - 127):
    e = floor(log2(amax)) - 8                 (8 = emax of e4m3),
    e += 1 where amax * 2^-e > 448            (448 = 1.75 * 2^8 is the largest e4m3 value: without the step a block whose amax has a
                                               significand above 1.75 would saturate its largest element),
    b = max(e + 127, 0)                       (an all-zero block -- and any amax below 2^-119 -- gets the smallest scale, byte 0).
The payload is x * 2^-(b - 127) rounded to nearest-even into OCP e4m3 (saturating at +-448, which the scale rule never reaches).
Scales are stored beside the payload as bytes [rows][ld / 32]; columns [K, ld) of a padded row hold zero payload and scale byte 0."""
import numpy as np

BLOCK = 32
E4M3_MAX = 448.0


def scale_bytes(amax):
    """E8M0 byte of a block from its amax (float32, >= 0, finite)."""
    bits = np.ascontiguousarray(amax, dtype=np.float32).view(np.uint32).astype(np.int64)
    e = (bits >> 23) - 8 + ((bits & 0x7FFFFF) > 0x600000)
    return np.maximum(e, 0).astype(np.uint8)


def e4m3_encode(v):
    """float32 -> OCP e4m3 bytes, round to nearest even, saturating at +-448; the sign of a value that rounds to zero is kept."""
    v = np.asarray(v, dtype=np.float32)
    sign = np.signbit(v).astype(np.uint8) << 7
    a = np.minimum(np.abs(v).astype(np.float64), E4M3_MAX)
    _, ex = np.frexp(a)                                  # a = m 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    E = np.maximum(ex - 1, -6)                           # below 2^-6: the subnormal quantum 2^-9
    r = np.rint(a / np.exp2(E - 3.0)) * np.exp2(E - 3.0)  # np.rint rounds halves to even
    r = np.minimum(r, E4M3_MAX)
    _, ex2 = np.frexp(r)
    E2 = ex2 - 1
    normal = r >= 2.0 ** -6
    expf = np.where(normal, E2 + 7, 0)
    mant = np.where(normal, np.rint((r / np.exp2(np.where(normal, E2, 0).astype(np.float64)) - 1.0) * 8.0), np.rint(r * 512.0))
    return (sign | (expf.astype(np.uint8) << 3) | mant.astype(np.uint8)).astype(np.uint8)


def e4m3_decode(b):
    b = np.asarray(b, dtype=np.uint8)
    s = np.where(b & 0x80, -1.0, 1.0)
    ef = ((b >> 3) & 0xF).astype(np.int64)
    m = (b & 7).astype(np.float64)
    return s * np.where(ef == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * np.exp2(ef - 7.0))


def quantize(x, ld=None):
    """x (..., K) float32, K % 32 == 0 -> (payload (..., ld) uint8, scales (..., ld / 32) uint8); ld defaults to K."""
    x = np.asarray(x, dtype=np.float32)
    K = x.shape[-1]
    assert K % BLOCK == 0, "MX operands need K % 32 == 0"
    ld = K if ld is None else ld
    assert ld % BLOCK == 0 and ld >= K
    xb = x.reshape(x.shape[:-1] + (K // BLOCK, BLOCK))
    sb = scale_bytes(np.abs(xb).max(-1))
    inv = ((254 - sb.astype(np.uint32)) << 23).astype(np.uint32).view(np.float32)      # 2^(127 - byte), exact
    q = e4m3_encode(np.clip(xb * inv[..., None], -E4M3_MAX, E4M3_MAX)).reshape(x.shape)
    payload = np.zeros(x.shape[:-1] + (ld,), np.uint8)
    payload[..., :K] = q
    scales = np.zeros(x.shape[:-1] + (ld // BLOCK,), np.uint8)
    scales[..., :K // BLOCK] = sb
    return payload, scales


def dequantize(payload, scales):
    """float64 values of an MX operand"""
    return e4m3_decode(payload) * np.repeat(np.exp2(scales.astype(np.float64) - 127.0), BLOCK, axis=-1)
