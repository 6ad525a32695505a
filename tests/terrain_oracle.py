"""CPU restatement of the reference's perlin / generate_terrain (NumPy path), vectorised and dtype-explicit: what
csrc/noise.hip is held to at the shapes the executed-reference fixture (tests/golden/terrain_exec.npz) does not hold.
Test infrastructure: never imported by the package.

Every step names its dtype:
  coordinates  np.linspace(a, b, n, endpoint=False, dtype=float32) -- restated as float32(float64(j) * ((b - a) / n) + a)
               in `linspace32`, which tests/test_terrain_host.py checks against NumPy's own;
  _perlin      xi = trunc(x) as int64, xf = float64(x) - xi, fade / gradient / lerp in float64.  The column part (xi, xf,
               fade(xf), p[xi], p[xi + 1]) is computed once per column and the row part once per row, then broadcast: the
               reference computes the same values on meshgrid planes;
  perlin       data[:] = noise (float64 -> dtype), (data - min) / ptp in dtype;
  terrain      h = dtype(float64(h) + noise_i * 2^-i) for i = 0 .. 15, h / dtype(1.00 + 0.50 + 0.25 + 0.13 + 0.06 + 0.03),
               h ** 3, (h - min) / ptp, h[h < dtype(0.3)] = 0, h * dtype(zfactor), all in dtype.
The table index is masked with 2^20 - 1 where the reference reads a doubled table: p2[k] == p[k - 2^20].
"""
import functools

import numpy as np

TABLE_SIZE = 1 << 20
MASK = TABLE_SIZE - 1
N_OCTAVES = 16
DIVISOR = 1.00 + 0.50 + 0.25 + 0.13 + 0.06 + 0.03


@functools.lru_cache(maxsize=40)
def table(seed):
    """np.random.seed(seed); np.random.permutation(2**20), without touching the global state"""
    p = np.random.RandomState(seed).permutation(TABLE_SIZE)
    p.setflags(write=False)
    return p


def linspace32(a, b, n, j0=0, count=None):
    """Elements [j0, j0 + count) of np.linspace(a, b, n, endpoint=False, dtype=np.float32)"""
    a, b = float(a), float(b)
    j = np.arange(j0, j0 + (n - j0 if count is None else count), dtype=np.float64)
    return (j * ((b - a) / n) + a).astype(np.float32)


def _fade(t):
    return 6 * t ** 5 - 15 * t ** 4 + 10 * t ** 3


def _gradient(h, x, y):
    """vectors[h % 4] . (x, y) with vectors (0, 1), (0, -1), (1, 0), (-1, 0)"""
    s = np.where(h & 2, x, y)
    return np.where(h & 1, 0.0 - s, s)


def _lerp(a, b, t):
    return a + t * (b - a)


def noise(p, x, y):
    """_perlin(p, *np.meshgrid(x, y)) for float32 vectors x (columns) and y (rows): float64, shape (len(y), len(x))"""
    assert x.dtype == np.float32 and y.dtype == np.float32
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    xf = (x.astype(np.float64) - xi)[None, :]
    yf = (y.astype(np.float64) - yi)[:, None]
    u, v = _fade(xf), _fade(yf)
    a0, a1 = p[xi & MASK][None, :], p[(xi + 1) & MASK][None, :]
    yi = yi[:, None]
    n00 = _gradient(p[(a0 + yi) & MASK], xf, yf)
    n01 = _gradient(p[(a0 + yi + 1) & MASK], xf, yf - 1)
    n11 = _gradient(p[(a1 + yi + 1) & MASK], xf - 1, yf - 1)
    n10 = _gradient(p[(a1 + yi) & MASK], xf - 1, yf)
    return _lerp(_lerp(n00, n10, u), _lerp(n01, n11, u), v)


def _normalised(d):
    with np.errstate(all="ignore"):
        return (d - np.min(d)) / np.ptp(d)


def perlin_raw(shape, dtype, freq, seed, row0=0, rows=None):
    """The plane before the normalisation (rows [row0, row0 + rows) of it)"""
    h, w = shape
    x = linspace32(0, freq[0], w)
    y = linspace32(0, freq[1], h, row0, rows)
    return noise(table(seed), x, y).astype(dtype)


def perlin(shape, dtype, freq=(1, 1), seed=5):
    return _normalised(perlin_raw(shape, dtype, freq, seed))


def scale(value, old_range, new_range):
    d = (value - old_range[0]) / (old_range[1] - old_range[0])
    return d * (new_range[1] - new_range[0]) + new_range[0]


def scaled_ranges(x_range, y_range, full_extent=None):
    fe = full_extent or (x_range[0], y_range[0], x_range[1], y_range[1])
    fx, fy = (fe[0], fe[2]), (fe[1], fe[3])
    return ((scale(x_range[0], fx, (0.0, 1.0)), scale(x_range[1], fx, (0.0, 1.0))),
            (scale(y_range[0], fy, (0.0, 1.0)), scale(y_range[1], fy, (0.0, 1.0))))


def terrain_raw(shape, dtype, seed, xr_scaled, yr_scaled, row0=0, rows=None, n_octaves=N_OCTAVES):
    """_gen_terrain: after the cube, before the normalisation (rows [row0, row0 + rows) of it)"""
    dtype = np.dtype(dtype)
    h, w = shape
    x = linspace32(xr_scaled[0], xr_scaled[1], w)
    y = linspace32(yr_scaled[0], yr_scaled[1], h, row0, rows)
    hm = np.zeros((y.size, w), dtype)
    for i in range(n_octaves):
        f = np.float32(2 ** i)
        hm = (hm.astype(np.float64) + noise(table(seed + i), x * f, y * f) * (1 / 2 ** i)).astype(dtype)
    hm = hm / dtype.type(DIVISOR)
    hm = hm ** 3
    assert hm.dtype == dtype
    return hm


def terrain_planes(shape, dtype, x_range=(0, 500), y_range=(0, 500), seed=10, zfactor=4000, full_extent=None):
    """(raw, normalised, final) of generate_terrain"""
    dtype = np.dtype(dtype)
    xr, yr = scaled_ranges(x_range, y_range, full_extent)
    raw = terrain_raw(shape, dtype, seed, xr, yr)
    norm = _normalised(raw)
    out = norm.copy()
    out[out < dtype.type(0.3)] = 0
    out = out * dtype.type(zfactor)
    assert norm.dtype == dtype and out.dtype == dtype
    return raw, norm, out


def cell_centres(lo, hi, n):
    return lo + (np.arange(n, dtype=np.float64) + 0.5) * (hi - lo) / n
