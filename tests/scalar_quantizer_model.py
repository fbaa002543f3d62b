"""Numpy restatement of the scalar quantizer's arithmetic contract (include/scann_hip.h "scalar
quantizer"): QuantizationStats::from_dataset (quantization/mod.rs:75-110) in the reference's sequential order AND in
the device's fixed order, ScalarQuantizer::calibrate / quantize_value / dequantize_value (quantization/scalar.rs:
103-172), and the library's SQ_SIGNED mode (hip.symmetric_int8).  Every f32 operation is one numpy float32 operation:
nothing is fused."""
import numpy as np

SQ_STDDEV, SQ_SYMMETRIC, SQ_RANGE, SQ_SIGNED = 0, 1, 2, 3
CHUNK, THREADS = 16384, 256          # kSqChunk, kSqThreads of csrc/scalarq.h
F32_MAX = np.float32(np.finfo(np.float32).max)
f32 = np.float32


def _tree(a):
    """[..., 256] -> [...]: s[t] += s[t + off] for off = 128, 64, ..., 1"""
    a = a.copy()
    off = THREADS // 2
    while off:
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
        off //= 2
    return a[..., 0]


def sums_sequential(values):
    """(sum, sum_sq) in f64, one value after the other: the reference's order"""
    s = s2 = np.float64(0.0)
    for v in np.asarray(values, np.float32).ravel().astype(np.float64):
        s = s + v
        s2 = s2 + v * v
    return s, s2


def sums_device(values):
    """(sum, sum_sq) in f64 in the device's order: chunks of 16384 logical values; in a chunk thread t adds the values
    4 g .. 4 g + 3 for g = t, t + 256, ... in order, the 256 thread sums are added as a tree; the chunk sums are then
    folded by thread t = chunk % 256 in ascending order and the same tree.  (Adding +0.0 for an absent value changes
    no f64 sum that started from +0.0.)"""
    v = np.asarray(values, np.float32).ravel().astype(np.float64)
    chunks = max(1, -(-v.size // CHUNK))
    pad = np.zeros(chunks * CHUNK, np.float64)
    pad[:v.size] = v
    g = pad.reshape(chunks, CHUNK // (4 * THREADS), THREADS, 4)     # [chunk][j][thread][element]
    out = []
    for x in (g, g * g):
        acc = np.zeros((chunks, THREADS), np.float64)
        for j in range(g.shape[1]):
            for e in range(4):
                acc = acc + x[:, j, :, e]
        part = _tree(acc)                                           # one sum per chunk
        rounds = -(-chunks // THREADS)
        pp = np.zeros(rounds * THREADS, np.float64)
        pp[:chunks] = part
        acc = np.zeros(THREADS, np.float64)
        for r in range(rounds):
            acc = acc + pp[r * THREADS:(r + 1) * THREADS]
        out.append(_tree(acc))
    return out[0], out[1]


def stats_from_sums(values, s, s2):
    """float32 [min, max, mean, std_dev] of quantization/mod.rs:96-110 from the f64 sums"""
    v = np.asarray(values, np.float32).ravel()
    count = v.size
    with np.errstate(all="ignore"):
        mn = np.fmin.reduce(np.concatenate([[F32_MAX], v]).astype(np.float32))
        mx = np.fmax.reduce(np.concatenate([[-F32_MAX], v]).astype(np.float32))
        mean = f32(s / np.float64(count)) if count else f32(0)
        var = f32((s2 - s * s / np.float64(count)) / np.float64(count - 1)) if count > 1 else f32(0)
        return np.array([mn, mx, mean, np.sqrt(var, dtype=np.float32)], np.float32)


def stats_reference(values):
    return stats_from_sums(values, *sums_sequential(values))


def stats_device(values):
    return stats_from_sums(values, *sums_device(values))


def roundf(x):
    """C roundf: half away from zero (numpy's round is half to even)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        return np.where(np.abs(x - t) >= f32(0.5), t + np.copysign(f32(1), x), t).astype(np.float32)


def as_i32(t):
    """Rust's `f32 as i32`: saturating, NaN -> 0"""
    t = np.asarray(t, np.float32)
    out = np.zeros(t.shape, np.int64)
    ok = ~np.isnan(t)
    out[ok] = np.clip(t[ok].astype(np.float64), -2147483648.0, 2147483647.0).astype(np.int64)
    return out


def calibrate(stats, bits=8, mode=SQ_STDDEV, a=3.0, b=0.0):
    """(params float32 [min, max, scale, inv_scale], zero_point) or None where the library refuses"""
    smin, smax, mean, std = (f32(x) for x in np.asarray(stats, np.float32))
    a, b = f32(a), f32(b)
    if mode == SQ_SIGNED:
        if bits != 8 or not (np.isfinite(smin) and np.isfinite(smax) and np.isfinite(mean)):
            return None
        m = np.fmax(np.abs(smin), np.abs(smax))
        s = f32(np.float64(m) / 127.0) if m > 0 else f32(1)
        with np.errstate(all="ignore"):
            return np.array([-m, m, s, f32(1) / s], np.float32), 0
    if bits not in (4, 8) or mode not in (SQ_STDDEV, SQ_SYMMETRIC, SQ_RANGE):
        return None
    levels = f32((1 << bits) - 1)
    with np.errstate(all="ignore"):
        if mode == SQ_RANGE:
            mn, mx = a, b
        elif mode == SQ_SYMMETRIC:
            am = np.fmax(np.abs(smin), np.abs(smax))
            mn, mx = -am, am
        else:
            r = a * std
            mn, mx = np.fmax(mean - r, smin), np.fmin(mean + r, smax)
        if not mn <= mx:
            return None
        rng = mx - mn
        if rng > f32(1e-10):
            scale, inv = rng / levels, levels / rng
            zp = int(as_i32(roundf(-mn * inv)))
        else:
            scale, inv, zp = f32(1), f32(1), 0
    return np.array([mn, mx, scale, inv], np.float32), zp


def quantize(values, params, bits=8, mode=SQ_STDDEV):
    """int8 codes, elementwise"""
    v = np.asarray(values, np.float32)
    mn, mx, scale, inv = (f32(x) for x in params)
    with np.errstate(all="ignore"):
        if mode == SQ_SIGNED:
            t = np.clip(np.rint(v / scale), -127, 127)
            return np.where(np.isnan(t), 0, t).astype(np.int8)
        c = np.where(v < mn, mn, np.where(v > mx, mx, v)).astype(np.float32)
        q = as_i32(roundf((c - mn) * inv))
    return np.clip(q, 0, (1 << bits) - 1).astype(np.uint8).view(np.int8)


def dequantize(codes, params, mode=SQ_STDDEV):
    c = np.asarray(codes, np.int8)
    mn, _, scale, _ = (f32(x) for x in params)
    with np.errstate(all="ignore"):
        if mode == SQ_SIGNED:
            return c.astype(np.float32) * scale
        return c.view(np.uint8).astype(np.float32) * scale + mn


def rows_int8(rows, out_stride, bits=8, mode=SQ_STDDEV, a=3.0, b=0.0, stats=None):
    """(codes [n, out_stride] int8 with pad columns 0, params, zero_point): what quantize_rows stores"""
    x = np.asarray(rows, np.float32)
    params, zp = calibrate(stats_device(x) if stats is None else stats, bits, mode, a, b)
    out = np.zeros((x.shape[0], out_stride), np.int8)
    out[:, :x.shape[1]] = quantize(x, params, bits, mode)
    return out, params, zp
