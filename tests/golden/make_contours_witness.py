"""contourpy's lines for seeded small rasters: tests/golden/contours_witness.npz.

Test infrastructure only.  The contour rule of DESIGN.md §6s is a written one (the reference has no contours); this fixture
records what an independent implementation draws, so that tests/contours_oracle.py, and through it the kernels, are held against
something that was not written here.  contourpy runs with name="serial", corner_mask=False, LineType.Separate, x and y at the
cell centres (c + 0.5, r + 0.5) and the cells that are not finite masked.  It orders the lines of a level its own way and starts
a closed line where it likes: the tests compare after matching lines and rotating closed ones.

contourpy treats a node or a saddle centre that equals a level differently, so the generator rejects such a case and draws the
next one from the same stream.

Keys: `n_cases`, `seed`, `max_diff` (the largest coordinate difference between contourpy and the oracle over all cases, as
measured when the fixture was written), and per case i: `<i>/z`, `<i>/levels` (float64), `<i>/points` ([N, 2] float64),
`<i>/line_offsets`, `<i>/level_offsets` (int64).

Usage:  python tests/golden/make_contours_witness.py      (needs contourpy; writes tests/golden/contours_witness.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import contours_oracle as co  # noqa: E402

OUT = os.path.join(HERE, "contours_witness.npz")
SEED = 20261021
N_CASES = 60
KINDS = ("float32", "float64", "saddles", "holes")


def draw(rng, kind):
    """(z, levels) of one case"""
    H, W = (int(v) for v in rng.integers(2, 14, 2))
    k = int(rng.integers(1, 6))
    if kind == "saddles":                                  # few integer values: most quads cross, many are saddles
        z = rng.integers(0, 4, (H, W)).astype((np.int8, np.uint16, np.int32, np.float32)[int(rng.integers(4))])
        levels = np.sort(rng.choice(np.arange(-0.5, 4.0, 0.125), k, replace=False))
    else:
        z = rng.normal(0.0, 1.0, (H, W)).astype(np.float32 if kind == "float32" else np.float64)
        if kind == "holes":
            z[rng.random((H, W)) < 0.1] = np.nan
        levels = np.sort(rng.uniform(-1.5, 1.5, k))
    return z, np.asarray(levels, np.float64)


def has_tie(z, levels):
    z = np.asarray(z).astype(np.float64)
    with np.errstate(all="ignore"):
        centre = ((z[:-1, :-1] + z[:-1, 1:]) + (z[1:, 1:] + z[1:, :-1])) * 0.25
    return any(np.any(z == level) or np.any(centre == level) or not np.all(np.diff(levels) > 0) for level in levels)


def contourpy_lines(z, levels):
    """per level, contourpy's list of (n, 2) float64 arrays"""
    from contourpy import LineType, contour_generator
    z = np.asarray(z).astype(np.float64)
    H, W = z.shape
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    gen = contour_generator(x, y, np.ma.masked_invalid(z), name="serial", corner_mask=False, line_type=LineType.Separate)
    return [[np.asarray(line, np.float64) for line in gen.lines(float(level))] for level in levels]


def is_closed(line):
    return len(line) > 1 and bool(np.all(line[0] == line[-1]))


def match(want, got, tol):
    """The largest coordinate difference after pairing every line of `want` with one of `got` of one level (same closed flag, same
    point count, same direction; a closed line rotated to the best start), or None when they do not pair up."""
    if len(want) != len(got):
        return None
    free, worst = list(range(len(got))), 0.0
    for a in want:
        best = None
        for j in free:
            b = got[j]
            if len(a) != len(b) or is_closed(a) != is_closed(b):
                continue
            if is_closed(a):
                n = len(a) - 1
                diffs = [np.abs(np.roll(b[:-1], -s, axis=0) - a[:-1]).max() for s in range(n)]
                d = float(min(diffs))
            else:
                d = float(np.abs(a - b).max())
            if d <= tol and (best is None or d < best[0]):
                best = (d, j)
        if best is None:
            return None
        free.remove(best[1])
        worst = max(worst, best[0])
    return worst


def build():
    rng = np.random.default_rng(SEED)
    store = {"n_cases": np.int64(N_CASES), "seed": np.int64(SEED)}
    worst, n_lines, i, rejected = 0.0, 0, 0, 0
    while i < N_CASES:
        z, levels = draw(rng, KINDS[i % len(KINDS)])
        if has_tie(z, levels):
            rejected += 1
            continue
        theirs = contourpy_lines(z, levels)
        ours = co.lines_of(co.contours(z, levels))
        for k in range(len(levels)):
            d = match(theirs[k], ours[k], 1e-9)
            assert d is not None, f"case {i}, level {levels[k]}: the oracle and contourpy draw different lines"
            worst = max(worst, d)
            n_lines += len(theirs[k])
        flat = [line for lines in theirs for line in lines]
        store[f"{i}/z"] = z
        store[f"{i}/levels"] = levels
        store[f"{i}/points"] = np.concatenate(flat).reshape(-1, 2) if flat else np.empty((0, 2), np.float64)
        store[f"{i}/line_offsets"] = np.concatenate([[0], np.cumsum([len(line) for line in flat])]).astype(np.int64)
        store[f"{i}/level_offsets"] = np.concatenate([[0], np.cumsum([len(lines) for lines in theirs])]).astype(np.int64)
        i += 1
    store["max_diff"] = np.float64(worst)
    print(f"{N_CASES} cases ({rejected} rejected for ties), {n_lines} lines, largest difference {worst:.3g}")
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def case_lines(st, i):
    """per level, the witness lines of case i"""
    return co.lines_of((st[f"{i}/points"], st[f"{i}/line_offsets"], st[f"{i}/level_offsets"], None))


if __name__ == "__main__":
    st = build()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")
