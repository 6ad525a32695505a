"""Inputs and plain NumPy references for the three single-pass streaming entries -- xrs_hotspots_classify_f32, xrs_nan_moments_f32
(xrspatial_amd/csrc/hotspots.hip) and xrs_nan_minmax_f32 (csrc/composite.hip) -- shared by tests/test_gpu_streaming_abi.py (the
kernels) and tests/test_hotspots_classes_host.py (the oracle's rule and the CPU emulation, no GPU).

The class rule restated here is the reference's `_calc_hotspots_numpy` (xrspatial/focal.py:881-915) as Numba types it: the float32
z-score meets the Python literals 2.33, 1.65, 1.29, 2.58 and 1.96 as float64 (Numba unifies float32 with a float64 constant to
float64; nobody has run Numba against this project, the claim rests on that typing rule).  NumPy under NEP 50 would compare in
float32 instead; `classes_f32` keeps that rule only to state where the two differ: at |z| == float32(1.96) and nowhere else."""
import numpy as np

F32 = np.float32
THRESHOLDS = (1.29, 1.65, 1.96, 2.33, 2.58)
FLT_MAX = np.finfo(F32).max
SUBNORMAL = np.finfo(F32).smallest_subnormal
SWEEP_CELLS = 12_582_913                        # every float32 in [1, 3]


def classes_f64(z):
    """int8 classes of float32 z-scores: |z| widened to float64, the ladder of focal.py:890-914 with Python-float thresholds, the
    sign from z."""
    z = np.asarray(z)
    assert z.dtype == F32
    a = np.abs(z).astype(np.float64)
    with np.errstate(invalid="ignore"):
        p = np.where(a >= 2.33, 0.0099, np.where(a >= 1.65, 0.0495, np.where(a >= 1.29, 0.0985, 1.0)))
        conf = np.where((a > 2.58) & (p < 0.01), 99, np.where((a > 1.96) & (p < 0.05), 95, np.where((a > 1.65) & (p < 0.1), 90, 0)))
        hot = np.where(z > 0, 1, np.where(z < 0, -1, 0))
    return (hot * conf).astype(np.int8)


def classes_f32(z):
    """The same ladder with every threshold rounded to float32 first: what a float32 comparison computes."""
    z = np.asarray(z)
    assert z.dtype == F32
    a = np.abs(z)
    t129, t165, t196, t233, t258 = (F32(t) for t in THRESHOLDS)
    with np.errstate(invalid="ignore"):
        p = np.where(a >= t233, 0.0099, np.where(a >= t165, 0.0495, np.where(a >= t129, 0.0985, 1.0)))
        conf = np.where((a > t258) & (p < 0.01), 99, np.where((a > t196) & (p < 0.05), 95, np.where((a > t165) & (p < 0.1), 90, 0)))
        hot = np.where(z > 0, 1, np.where(z < 0, -1, 0))
    return (hot * conf).astype(np.int8)


def zscore(m, gmean, gstd):
    """(m - gmean) / gstd in float32, each operation correctly rounded, as NumPy forms it from float32 operands"""
    m = np.asarray(m)
    assert m.dtype == F32
    with np.errstate(all="ignore"):
        return (m - F32(gmean)) / F32(gstd)


def stepped(value, ulps):
    """float32 `value` moved by each of `ulps` units in the last place (positive finite values: the bit pattern counts them)"""
    bits = np.array([value], F32).view(np.uint32)[0].astype(np.int64)
    return (bits + np.asarray(ulps, np.int64)).astype(np.uint32).view(F32)


def sweep():
    """every float32 in [1, 3], ascending"""
    lo, hi = (int(np.array([v], F32).view(np.uint32)[0]) for v in (1.0, 3.0))
    out = np.arange(lo, hi + 1, dtype=np.uint32).view(F32)
    assert out.size == SWEEP_CELLS and out[0] == 1.0 and out[-1] == 3.0
    return out


def neighbourhood():
    """float32(t) stepped -8 .. +8 ulp for each threshold t, both signs, then the specials"""
    near = np.concatenate([stepped(F32(t), np.arange(-8, 9)) for t in THRESHOLDS])
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, SUBNORMAL, -SUBNORMAL, FLT_MAX, -FLT_MAX], F32)
    return np.concatenate([near, -near, special])


def division_cells(gmean, gstd, seed=7):
    """Cells whose z-scores under (gmean, gstd) fall within a few ulp of every threshold (so a divide or a subtract that is one
    ulp off changes a class), followed by seeded normal cells with NaN holes.  70,001 + 1290 cells."""
    gmean, gstd = F32(gmean), F32(gstd)
    near = []
    for t in THRESHOLDS:
        for sign in (1.0, -1.0):
            centre = F32(F32(sign * t) * gstd + gmean)
            step = np.spacing(np.abs(centre))
            near.append((centre + np.arange(-64, 65, dtype=np.float64) * step).astype(F32))
    rng = np.random.default_rng(seed)
    bulk = rng.normal(50.3, 25.0, 70_001).astype(F32)
    bulk[rng.random(bulk.size) < 0.1] = np.nan
    return np.concatenate(near + [bulk])


# ---------------------------------------------------------------------------------------------------------------- moments
MOMENT_SIZES = (1, 3, 4, 5, 4096, 4097, 8 * 4096 + 5, 4 * (2 ** 21 + 1) + 3)


def moment_values(n, kind, seed=11):
    """`n` float32 cells: normal(250, 40) with 30 % NaN ('holes'), and what the other kinds change in it"""
    rng = np.random.default_rng(seed)
    x = rng.normal(250.0, 40.0, n).astype(F32)
    x[rng.random(n) < 0.3] = np.nan
    if kind == "holes":
        pass
    elif kind == "far shift":                   # the shift sample (the first 4096 cells) says nothing about the rest
        x[:4096] = -9999.0
    elif kind == "one inf":
        x[n // 2] = np.inf
    elif kind == "both inf":
        x[n // 3], x[2 * n // 3] = np.inf, -np.inf
    elif kind == "all nan":
        x[:] = np.nan
    else:
        raise KeyError(kind)
    return x


def moments_reference(x):
    """(count, mean, std) of the cells that are not NaN, in float64; (0, nan, nan) when there is none"""
    v = x[~np.isnan(x)].astype(np.float64)
    if not v.size:
        return 0, np.nan, np.nan
    with np.errstate(all="ignore"):
        return int(v.size), float(v.mean()), float(v.std())


# ----------------------------------------------------------------------------------------------------------------- minmax
MINMAX_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 8 * 1024 + 5, 2 ** 21 + 5)
MINMAX_BIG = 2 ** 21 + 5                        # 2048 workgroups (the cap), chunks of 2048 cells = two trips; chunk 1024 holds 5 cells


def minmax_reference(x):
    """(np.nanmin, np.nanmax), (nan, nan) for no cell or NaN cells only"""
    v = x[~np.isnan(x)]
    return (F32(v.min()), F32(v.max())) if v.size else (F32(np.nan), F32(np.nan))


def minmax_contents(n, seed=13):
    """name -> `n` float32 cells (n >= 8), for the big size and the unaligned one"""
    rng = np.random.default_rng(seed)
    base = rng.normal(10.0, 300.0, n).astype(F32)
    base[rng.random(n) < 0.2] = np.nan
    chunk0_last = min(n, 2048 if n > 2 ** 21 else 1024) - 1
    out = {"holes": base, "all nan": np.full(n, np.nan, F32)}
    assert n & 3                                # so that the last cell lies in the scalar remainder behind the last 16-byte slot
    for where, at in (("cell 0", 0), ("last cell of chunk 0", chunk0_last), ("last 16-byte slot", (n & ~3) - 1),
                      ("last cell, the scalar remainder", n - 1)):
        one = np.full(n, np.nan, F32)
        one[at] = -7.25
        out["one finite cell: " + where] = one
    out["negative only"] = -np.abs(base) - F32(1)
    with_inf = base.copy()
    with_inf[[n // 5, n // 2]] = np.inf, -np.inf
    out["inf mixed in"] = with_inf
    out["all +inf"] = np.full(n, np.inf, F32)
    out["all -inf"] = np.full(n, -np.inf, F32)
    tiny = (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(F32)   # subnormals, both signs
    out["subnormals"] = tiny
    extremes = tiny.copy()
    extremes[[n // 7, n // 3]] = FLT_MAX, -FLT_MAX
    out["subnormals and FLT_MAX"] = extremes
    ends = np.clip(base, -2000, 2000)
    ends[0], ends[-1] = 5000.0, -5000.0
    out["max in cell 0, min in the last cell"] = ends
    return out
