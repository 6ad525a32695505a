"""Witnesses for two mutations of tests/rasterize_oracle.py that no ordinary input tells apart: tests/golden/rasterize_witness.npz.

Test infrastructure only.  "fma" (the pixel-space mapping with its first product fused into the sum) and "no_canonical" (edges
evaluated in the direction they are walked) move a crossing by one unit in the last place at most; that shows only where an
edge passes within a rounding error of a cell centre.  A bounded, seeded search makes such edges: a centre c of an 8 x 8 raster,
a random direction d, and the triangle (c - m d, c + n d, a far third point) for small integers m, n, whose first edge passes
the centre up to the rounding of its ends.  The first triangle for which the mutated oracle burns another raster than the plain
one is kept, with the trial number that found it.

Keys: `<mutation>/points` ([3, 2] float64, world coordinates), `<mutation>/transform` (6 float64; absent = pixel space),
`<mutation>/trial` (int64), `seed`, `shape`.

Usage:  python tests/golden/make_rasterize_witness.py            (writes tests/golden/rasterize_witness.npz)
        python tests/golden/make_rasterize_witness.py --check    (exit 1 unless the stored witnesses still tell the mutations apart)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import rasterize_oracle as ro  # noqa: E402

OUT = os.path.join(HERE, "rasterize_witness.npz")
SEED = 20261021
SHAPE = (8, 8)
MAX_TRIALS = 20000
SHEAR = (0.1, 0.3, -0.7, 0.3, -0.7, 0.1)
TRANSFORMS = {"fma": SHEAR, "no_canonical": None}


def triangle(rng):
    """pixel-space triangle whose first edge passes a cell centre up to the rounding of its ends"""
    H, W = SHAPE
    c = np.array([rng.integers(1, W - 1) + 0.5, rng.integers(1, H - 1) + 0.5])
    d = rng.uniform(-1.0, 1.0, 2)
    m, n = rng.integers(1, 6, 2)
    far = np.array([rng.uniform(-3.0, W + 3.0), rng.choice([-3.0, H + 3.0])])
    tri = np.stack([c - m * d, c + n * d, far])
    return tri[::-1].copy() if rng.random() < 0.5 else tri


def to_world(tri, t):
    if t is None:
        return tri
    i, j = tri[:, 0], tri[:, 1]
    return np.stack([t[0] * i + t[1] * j + t[2], t[3] * i + t[4] * j + t[5]], axis=1)


def differs(points, transform, mutation):
    shapes = (points, np.array([0, 3]), np.array([0, 1]))
    return not np.array_equal(ro.rasterize(*shapes, SHAPE, transform=transform),
                              ro.rasterize(*shapes, SHAPE, transform=transform, mutate=mutation))


def search():
    store = {"seed": np.int64(SEED), "shape": np.array(SHAPE)}
    for mutation, transform in TRANSFORMS.items():
        rng = np.random.default_rng(SEED)
        for trial in range(MAX_TRIALS):
            points = to_world(triangle(rng), transform)
            if differs(points, transform, mutation):
                store[f"{mutation}/points"] = points
                store[f"{mutation}/trial"] = np.int64(trial)
                if transform is not None:
                    store[f"{mutation}/transform"] = np.asarray(transform, np.float64)
                print(f"{mutation}: trial {trial}")
                break
        else:
            print(f"{mutation}: no witness in {MAX_TRIALS} trials")
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def check():
    st = load()
    ok = True
    for mutation in TRANSFORMS:
        t = st.get(f"{mutation}/transform")
        good = f"{mutation}/points" in st and differs(st[f"{mutation}/points"], None if t is None else tuple(t), mutation)
        print(mutation, "witness holds" if good else "NO witness")
        ok &= bool(good)
    return ok


if __name__ == "__main__":
    if sys.argv[1:] == ["--check"]:
        sys.exit(0 if check() else 1)
    st = search()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")
