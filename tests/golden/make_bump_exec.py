"""Outputs of the reference's OWN bump loop, executed here: tests/golden/bump_exec.npz.

Test infrastructure only, built like make_local_exec.py: `_finish_bump` of xrspatial/bump.py is lifted with `ast` from the
reference where it lies and RUN as plain Python on the cases of `cases()`.  Nothing of the reference is copied: the fixture
holds the inputs of `cases()` and the outputs.

The locations are handed to the lifted function as int64.  Under Numba `uint16 - int64` widens to int64; as plain Python under
NumPy 2 a uint16 scalar minus a Python int wraps, which would not be the reference's arithmetic.  The fixture stores them as the
uint16 the public function makes.

Keys of a case: `<case>/size` (width, height, spread; int64), `<case>/locs` ((count, 2) uint16 of (x, y)), `<case>/heights`
(count values in the case's own dtype), `<case>/out` ((height, width) float64, the reference's result, inf and NaN included).

Usage:  python tests/golden/make_bump_exec.py            (writes tests/golden/bump_exec.npz; some seconds)
        python tests/golden/make_bump_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "bump_exec.npz")
MAX_BYTES = 600_000


def ref_finish_bump():
    return rx.lift("bump.py", ["_finish_bump"])["_finish_bump"]


# ------------------------------------------------------------------ cases
def _random(rng, width, height, count, heights="normal"):
    locs = np.stack([rng.integers(0, width, count), rng.integers(0, height, count)], axis=1).astype(np.uint16)
    if heights == "ones":
        z = np.ones(count)
    else:
        z = rng.normal(scale=3.0, size=count)                # full mantissas: another order of the adds shows
    return locs, z


def chain(n, forward):
    """n spread-1 bumps along row 1 of an n x 3 raster.  A spread-1 bump at x covers x - 1: placed right to left, every bump
    covers the NEXT bump's centre, so that bump cannot publish before this one has (a chain n deep); placed left to right,
    every bump covers the centre of the bump BEFORE it, and every centre is published in the first pass."""
    xs = np.arange(n - 1, -1, -1) if forward else np.arange(n)
    locs = np.stack([xs, np.ones(n, np.int64)], axis=1).astype(np.uint16)
    z = 1.0 + np.arange(n) / 7.0
    return locs, z


def cases():
    """[(name, dict(width, height, spread, locs, heights))], deterministic"""
    out = []
    rng = np.random.default_rng(20261019)

    def add(name, width, height, spread, locs, heights):
        out.append((name, dict(width=width, height=height, spread=spread, locs=np.ascontiguousarray(locs, dtype=np.uint16),
                               heights=np.ascontiguousarray(heights))))

    # the sizes of the design check: default density, spreads 1 .. 3
    add("r20x20_n40_s1", 20, 20, 1, *_random(rng, 20, 20, 40, "ones"))
    add("r64x48_n307_s1", 64, 48, 1, *_random(rng, 64, 48, 307))
    add("r64x48_n307_s2", 64, 48, 2, *_random(rng, 64, 48, 307))
    add("r37x29_n500_s3", 37, 29, 3, *_random(rng, 37, 29, 500))
    # clipping: one row, one column, one cell; every corner and edge of 9 x 7; a spread larger than the raster
    add("r1x1_s1", 1, 1, 1, np.zeros((5, 2)), rng.normal(size=5))
    add("r1x1_s3", 1, 1, 3, np.zeros((5, 2)), rng.normal(size=5))
    add("r1x17_s2", 1, 17, 2, *_random(rng, 1, 17, 30))
    add("r17x1_s2", 17, 1, 2, *_random(rng, 17, 1, 30))
    border = [(x, y) for x in (0, 4, 8) for y in (0, 3, 6) if (x, y) != (4, 3)]
    border = np.array(border + border[::-1])
    for spread in (1, 2, 3):
        add(f"border_9x7_s{spread}", 9, 7, spread, border, rng.normal(size=len(border)))
    add("spread9_in_5x4", 5, 4, 9, *_random(rng, 5, 4, 25))
    # per-cell order: 40 bumps on one cell, heights that cancel in one order only
    z = np.tile([1e16, 1.0, -1e16, 3.0], 10)
    add("one_cell_5x5_s1", 5, 5, 1, np.full((40, 2), 2), z)
    add("one_cell_5x5_s2", 5, 5, 2, np.full((40, 2), 2), z)
    # dependency chains
    add("chain_forward_300", 300, 3, 1, *chain(300, True))
    add("chain_reverse_300", 300, 3, 1, *chain(300, False))
    # dense: every bump depends on most of the earlier ones; the second overflows
    add("dense_8x8_n2000_s3", 8, 8, 3, *_random(rng, 8, 8, 2000, "ones"))
    add("dense_6x6_n8000_s3", 6, 6, 3, *_random(rng, 6, 6, 8000, "ones"))
    # an infinite centre: the cells walked before the centre's own `+ v * 0.0` take inf, the centre and those after it NaN
    add("inf_height_7x7_s2", 7, 7, 2, [(1, 1), (3, 3), (5, 4), (0, 6)], [2.5, np.inf, -1.25, 1.0])
    add("overflow_7x7_s2", 7, 7, 2, [(3, 3), (3, 3), (2, 3), (6, 6)], [1.5e308, 1.5e308, 1.0, -np.inf])
    # more than one workgroup of cells, odd widths (the other spreads of these shapes run against the oracle)
    add("seam_130x70_s2", 130, 70, 2, *_random(rng, 130, 70, 2000))
    add("seam_130x70_s9", 130, 70, 9, *_random(rng, 130, 70, 2000))
    add("seam_257x33_s1", 257, 33, 1, *_random(rng, 257, 33, 2000))
    add("seam_257x33_s5", 257, 33, 5, *_random(rng, 257, 33, 2000))
    # spread 0 and negative: the centre adds alone
    for spread in (0, -2):
        add(f"r12x9_s{spread}", 12, 9, spread, *_random(rng, 12, 9, 60))
    # the height dtypes
    locs, _ = _random(rng, 23, 11, 90)
    add("heights_u16", 23, 11, 2, locs, rng.integers(0, 60000, 90).astype(np.uint16))
    add("heights_f32", 23, 11, 2, locs, rng.normal(size=90).astype(np.float32))
    add("heights_f64", 23, 11, 2, locs, rng.normal(size=90))
    add("heights_i64_beyond_2p53", 23, 11, 2, locs, (rng.integers(-(1 << 62), 1 << 62, 90) | 1).astype(np.int64))
    return out


# ------------------------------------------------------------------ running the reference
def reference(fn, c):
    with np.errstate(all="ignore"):
        got = fn(c["width"], c["height"], c["locs"].astype(np.int64), c["heights"], c["spread"])
    assert got.dtype == np.float64 and got.shape == (c["height"], c["width"])
    return got


def complaints(name, c, got):
    bad = []
    if name == "dense_6x6_n8000_s3" and np.isfinite(got).all():
        bad.append(f"{name}: every cell is finite; raise the count until the sums overflow")
    if name == "dense_8x8_n2000_s3" and not (np.isfinite(got).all() and np.abs(got).max() > 1e100):
        bad.append(f"{name}: expected finite values beyond 1e100, largest is {np.abs(got).max()}")
    if name in ("inf_height_7x7_s2", "overflow_7x7_s2") and not (np.isinf(got).any() and np.isnan(got).any() and np.isfinite(got).any()):
        bad.append(f"{name}: expected inf, NaN and finite cells side by side")
    if name.startswith("one_cell") and got[2, 2] == np.asarray(c["heights"], np.float64).sum():
        bad.append(f"{name}: the order of the adds does not show")
    return bad


def run_all():
    fn = ref_finish_bump()
    store, bad = {}, []
    for name, c in cases():
        got = reference(fn, c)
        bad += complaints(name, c, got)
        store[f"{name}/size"] = np.array([c["width"], c["height"], c["spread"]], np.int64)
        store[f"{name}/locs"] = c["locs"]
        store[f"{name}/heights"] = c["heights"]
        store[f"{name}/out"] = got
    return store, bad


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def names(store):
    return sorted({k.split("/")[0] for k in store})


def case_of(store, name):
    """(width, height, spread, locs, heights, out) of a stored case"""
    width, height, spread = (int(v) for v in store[f"{name}/size"])
    return width, height, spread, store[f"{name}/locs"], store[f"{name}/heights"], store[f"{name}/out"]


def check():
    want = load()
    got, _ = run_all()
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
        print("bump_exec.npz reproduces" if ok else "bump_exec.npz differs")
        sys.exit(0 if ok else 1)
    st, bad = run_all()
    for line in bad:
        print("REFUSED", line)
    if bad:
        sys.exit(1)
    np.savez_compressed(OUT, **st)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {len(st)} arrays of {len(names(st))} cases, {size} bytes")
    if size > MAX_BYTES:
        sys.exit(f"{size} bytes is above the {MAX_BYTES} allowed")
