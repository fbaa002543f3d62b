"""Shapes and inputs shared by tests/test_scalar_quantizer_model.py (CPU) and tests/test_gpu_scalar_quantizer.py.

SHAPES are the smallest at which the kernels of csrc/scalarq.hip can go wrong: one value; the reference's 5 x 3 test
set; 257 x 50 (no 16-byte loads, a tail of the vector width, pad columns at strides 52 and 64); 1000 x 128 (the
16-byte path, several chunks); 4099 x 33 (odd everything, nine chunks); two shapes of exactly one 16384-value chunk of
the stats pass and one of a chunk plus one value.

PARITY inputs are those on which the device's summation order and the reference's sequential order give bit-equal
mean and std_dev (checked on the CPU by test_scalar_quantizer_model.py); CANCELLATION is the documented exception
(DESIGN.md 7): a large mean with a tiny spread, where sum_sq - sum^2 / count cancels down to the last f64 bits."""
import numpy as np

SHAPES = [(1, 1), (5, 3), (257, 50), (1000, 128), (4099, 33), (128, 128), (4096, 4), (113, 145)]
STRIDES_257x50 = (50, 52, 64)
KINDS = ("uniform01", "centred", "gauss37", "three")


def rows_of(kind, n, dim, seed=0):
    rng = np.random.default_rng([seed, n, dim, KINDS.index(kind) if kind in KINDS else 99])
    if kind == "uniform01":
        x = rng.random((n, dim), dtype=np.float32)
    elif kind == "centred":
        x = rng.random((n, dim), dtype=np.float32) - np.float32(0.5)
    elif kind == "gauss37":
        x = rng.standard_normal((n, dim), dtype=np.float32) * np.float32(37.0)
    elif kind == "three":
        x = rng.choice(np.array([-1.5, 0.25, 3.0], np.float32), size=(n, dim))
    elif kind == "cancellation":
        x = np.float32(100.0) + np.float32(0.01) * rng.random((n, dim), dtype=np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)


def parity_cases():
    """[(name, rows)]: every shape with one kind (cycling), and every kind at 1000 x 128"""
    out = []
    for i, (n, dim) in enumerate(SHAPES):
        kind = KINDS[i % len(KINDS)]
        out.append(("%dx%d-%s" % (n, dim, kind), rows_of(kind, n, dim)))
    for kind in KINDS:
        if not any(name == "1000x128-" + kind for name, _ in out):
            out.append(("1000x128-" + kind, rows_of(kind, 1000, 128)))
    return out


def cancellation_rows():
    return rows_of("cancellation", 3000, 24)


def strided(rows, stride, fill=np.nan):
    """[n, stride] f32 with the rows in the first dim columns and `fill` in the padding (NaN: a read of it would show
    in every statistic)"""
    n, dim = rows.shape
    out = np.full((n, stride), fill, np.float32)
    out[:, :dim] = rows
    return out


def adversarial_values(params, bits):
    """values around everything quantize_value branches on, for a calibrated [min, max, scale, inv_scale]: exact
    halves of the level grid, both ends and beyond, NaN, infinities, signed zeros, the 127 / 128 / 255 wrap"""
    mn, mx, scale, inv = (np.float32(x) for x in params)
    levels = (1 << bits) - 1
    ks = np.array([0, 1, 2, levels // 2 - 1, levels // 2, levels // 2 + 1, levels - 1, levels], np.float32)
    with np.errstate(all="ignore"):
        grid = (mn + ks * scale).astype(np.float32)
        halves = (mn + (ks + np.float32(0.5)) / inv).astype(np.float32)
        near = np.concatenate([np.nextafter(halves, np.float32(-np.inf)), halves, np.nextafter(halves, np.float32(np.inf))])
        ends = np.array([mn, mx, mn - np.float32(1), mx + np.float32(1), np.nextafter(mn, np.float32(-np.inf)),
                         np.nextafter(mx, np.float32(np.inf)), -3.0e38, 3.0e38], np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45], np.float32)
    return np.concatenate([grid, near, ends, special]).astype(np.float32)
