"""Outputs of the reference's OWN perlin / generate_terrain code, executed here: tests/golden/terrain_exec.npz.

Test infrastructure only, built like make_regions_exec.py: `_lerp`, `_fade`, `_gradient`, `_perlin`, `_perlin_numpy`
(xrspatial/perlin.py:28-91) and `_scale`, `_gen_terrain`, `_terrain_numpy` (xrspatial/terrain.py:31-80) are lifted with
`ast` from the reference where it lies, their `@jit` decorators stripped, `nb.prange` supplied as `range`, and RUN as plain
Python / NumPy on the cases of `cases()`.  Nothing of the reference is copied: the fixture holds outputs only (the inputs are
the few numbers in `cases()`).

Undecorated, the lifted functions are the same arithmetic as under Numba: every operand of `_lerp`, `_fade` and
`_gradient` is a float64 array (x - xi is float32 - int64 -> float64), and everything else is NumPy in both.

Keys: `<case>/out` (what `_perlin_numpy` / `_terrain_numpy` return), and for the terrain cases `<case>/raw` (what
`_gen_terrain` returns: after the cube, before the normalisation) and `<case>/norm` (the normalised plane before the water
line, recomputed from `raw` as `_terrain_numpy` does: (raw - min) / ptp).  `table/<seed>/...`: a digest of the permutation
the reference draws for that seed (`np.random.seed(seed); np.random.permutation(2**20)`): its first 64 entries, every
4096th entry and sum(p[k] * (k % 8191)).

Usage:  python tests/golden/make_terrain_exec.py            (writes tests/golden/terrain_exec.npz; about two minutes)
        python tests/golden/make_terrain_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "terrain_exec.npz")
TABLE_SEEDS = (5, 10, 25)


def cases():
    """[(name, parameters)], deterministic.  kind 'perlin': shape, dtype, freq, seed; kind 'terrain': shape, dtype,
    x_range, y_range, seed, zfactor, full_extent (None: the ranges themselves)."""
    f32, f64 = "float32", "float64"
    P = lambda shape, dtype, freq, seed: dict(kind="perlin", shape=shape, dtype=dtype, freq=freq, seed=seed)  # noqa: E731
    T = lambda shape, dtype, seed=10, zfactor=4000, x_range=(0, 500), y_range=(0, 500), full_extent=None: dict(  # noqa: E731
        kind="terrain", shape=shape, dtype=dtype, x_range=x_range, y_range=y_range, seed=seed, zfactor=zfactor,
        full_extent=full_extent)
    return [
        ("perlin_doc", P((3, 4), f32, (1, 1), 5)),                  # the docstring example of xrspatial.perlin
        ("perlin_50", P((50, 50), f32, (1, 1), 5)),                 # the shape of the reference's tests, default arguments
        ("perlin_freq", P((37, 53), f32, (3, 7.3), 7)),
        ("perlin_f64", P((21, 30), f64, (2, 5), 5)),
        ("perlin_1x1", P((1, 1), f32, (1, 1), 5)),                  # constant plane: 0 / 0
        ("terrain_50", T((50, 50), f32)),
        ("terrain_37x53_f32", T((37, 53), f32)),
        ("terrain_37x53_f64", T((37, 53), f64)),
        ("terrain_96x130_f32", T((96, 130), f32)),
        ("terrain_96x130_f64", T((96, 130), f64)),
        ("terrain_window", T((37, 53), f32, seed=10, zfactor=4000, x_range=(100, 300), y_range=(50, 450),
                             full_extent=(0, 0, 500, 500))),
        ("terrain_1x1", T((1, 1), f32, seed=3, zfactor=10)),
    ]


class _NumbaStandIn:
    prange = range


def ref_functions():
    p = rx.lift("perlin.py", ["_lerp", "_fade", "_gradient", "_perlin", "_perlin_numpy"], {"nb": _NumbaStandIn})
    t = rx.lift("terrain.py", ["_scale", "_gen_terrain", "_terrain_numpy"], {"_perlin": p["_perlin"]})
    return p, t


def scaled_ranges(c, scale):
    """x_range_scaled, y_range_scaled as generate_terrain (terrain.py:240-256) builds them, with the reference's `_scale`"""
    fe = c["full_extent"] or (c["x_range"][0], c["y_range"][0], c["x_range"][1], c["y_range"][1])
    fx, fy = (fe[0], fe[2]), (fe[1], fe[3])
    return ((scale(c["x_range"][0], fx, (0.0, 1.0)), scale(c["x_range"][1], fx, (0.0, 1.0))),
            (scale(c["y_range"][0], fy, (0.0, 1.0)), scale(c["y_range"][1], fy, (0.0, 1.0))))


def table_digest(p):
    p = np.asarray(p, dtype=np.int64)
    return {"head": p[:64].copy(), "strided": p[::4096].copy(),
            "checksum": np.array([int(np.sum(p * (np.arange(p.size, dtype=np.int64) % 8191)))], dtype=np.int64)}


def run_all():
    pn, tn = ref_functions()
    store = {}
    for name, c in cases():
        data = np.zeros(c["shape"], dtype=c["dtype"])
        with np.errstate(all="ignore"):
            if c["kind"] == "perlin":
                store[f"{name}/out"] = np.array(pn["_perlin_numpy"](data, c["freq"], c["seed"]))
                continue
            xr, yr = scaled_ranges(c, tn["_scale"])
            raw = np.array(tn["_gen_terrain"](data * 0, c["seed"], x_range=xr, y_range=yr))
            store[f"{name}/raw"] = raw
            store[f"{name}/norm"] = (raw - np.min(raw)) / np.ptp(raw)
            store[f"{name}/out"] = np.array(tn["_terrain_numpy"](data, c["seed"], xr, yr, c["zfactor"]))
        for k in ("raw", "norm", "out"):
            assert store[f"{name}/{k}"].dtype == data.dtype, (name, k)
    for seed in TABLE_SEEDS:
        np.random.seed(seed)
        for k, v in table_digest(np.random.permutation(2 ** 20)).items():
            store[f"table/{seed}/{k}"] = v
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def check():
    want = load()
    got = run_all()
    bad = sorted(set(want) ^ set(got))
    for k in set(want) & set(got):
        a, b = want[k], got[k]
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            bad.append(k)
    for k in sorted(bad)[:20]:
        print("MISMATCH", k)
    return not bad


if __name__ == "__main__":
    if not rx.have_reference():
        sys.exit("the reference is not present here")
    if sys.argv[1:] == ["--check"]:
        ok = check()
        print("terrain_exec.npz reproduces" if ok else "terrain_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")
