"""Outputs of the reference's OWN pathfinding code, executed here: tests/golden/astar_exec.npz.

Test infrastructure only, built like make_proximity_exec.py: `_is_not_crossable`, `_find_nearest_pixel`, `_distance`,
`_heuristic`, `_neighborhood_structure`, `_reconstruct_path`, `_min_cost_pixel_id` and `_a_star_search` of
xrspatial/pathfinding.py are lifted with `ast` from the reference where it lies, `ngjit` supplied as the identity, and RUN as plain
Python on the cases of `cases()`, in pixel space and in the order of the reference's `a_star_search`: snap, the two warnings, the
NaN image, the search unless the start snapped to nothing.  Nothing of the reference is copied: the fixture holds the inputs of
`cases()`, the output images, whether each warning was issued, and the names, kinds and defaults of `a_star_search`'s parameters.

Every pop of the reference's open list scans the raster, cells^2 per case as plain Python: no case has more than 40 x 40 cells.
A fixture in which fewer than 20 cases with a path have exactly one shortest path (tests/pathfinding_oracle.py counts them) is
not written: only there does the rule have to give the reference's image bit for bit.

Keys: `<case>/z`, `<case>/start`, `<case>/goal` (pixels), `<case>/barriers`, `<case>/args` (connectivity, snap_start, snap_goal),
`<case>/image` (float64), `<case>/warned` (start, goal); `signature` (JSON).

Usage:  python tests/golden/make_astar_exec.py            (writes tests/golden/astar_exec.npz; about a minute)
        python tests/golden/make_astar_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "astar_exec.npz")
MAX_SIDE = 40
MIN_UNIQUE = 20
LIFTED = ["NONE", "_is_not_crossable", "_distance", "_heuristic", "_min_cost_pixel_id", "_find_nearest_pixel", "_reconstruct_path",
          "_neighborhood_structure", "_a_star_search"]
DOC = np.array([[0, 1, 0, 0], [1, 1, 0, 0], [0, 1, 2, 2], [1, 0, 2, 0], [0, 2, 2, 2]])
DOC_NAN = np.array([[0, 1, 0, 0], [1, 1, np.nan, 0], [0, 1, 2, 2], [1, 0, 2, 0], [0, np.nan, 2, 2]])


def _case(z, start, goal, barriers=(), connectivity=8, snap_start=False, snap_goal=False):
    z = np.asarray(z)
    assert z.ndim == 2 and max(z.shape) <= MAX_SIDE
    bar = np.array(list(barriers)) if len(barriers) else np.array([])    # `np.array(barriers)` of the reference
    return dict(z=z, start=np.array(start, np.int64), goal=np.array(goal, np.int64), barriers=bar,
                args=np.array([connectivity, snap_start, snap_goal], np.int64))


def serpentine(h, w, dtype=np.int32, vertical=False):
    """one-cell corridors (1) between walls (0) that leave a gap at alternating ends: exactly one path"""
    z = np.ones((h, w), dtype)
    for k, r in enumerate(range(1, h, 2)):
        z[r, :] = 0
        z[r, -1 if k % 2 == 0 else 0] = 1
    return z.T.copy() if vertical else z


def maze(shape, seed, share, dtype=np.int32):
    """`share` of the cells are walls (0), the corners are open"""
    rng = np.random.default_rng(seed)
    z = (rng.random(shape) >= share).astype(dtype)
    z[0, 0] = z[-1, -1] = 1
    return z


def tree_maze(h, w, seed, dtype=np.int32):
    """a spanning tree of the odd-indexed cells (depth-first, seeded): between any two open cells exactly one 4-connected path"""
    rng = np.random.default_rng(seed)
    z = np.zeros((h, w), dtype)
    cells = [(r, c) for r in range(0, h, 2) for c in range(0, w, 2)]
    seen = {cells[0]}
    stack = [cells[0]]
    z[cells[0]] = 1
    while stack:
        r, c = stack[-1]
        nxt = [(r + dr, c + dc) for dr, dc in ((-2, 0), (2, 0), (0, -2), (0, 2))
               if 0 <= r + dr < h and 0 <= c + dc < w and (r + dr, c + dc) not in seen]
        if not nxt:
            stack.pop()
            continue
        n = nxt[rng.integers(len(nxt))]
        z[(r + n[0]) // 2, (c + n[1]) // 2] = 1
        z[n] = 1
        seen.add(n)
        stack.append(n)
    return z


def cases():
    """[(name, dict(z, start, goal, barriers, args))], deterministic"""
    out = []
    out.append(("doc_example", _case(DOC, (1, 0), (4, 1), [0])))
    # the reference's own test module: every pair without barriers on its 5 x 4 raster would be 400 cases; a spread of them
    for k, (s, g) in enumerate([((0, 0), (4, 3)), ((4, 0), (0, 3)), ((2, 1), (2, 1)), ((0, 3), (3, 0)), ((1, 2), (4, 2))]):
        out.append((f"upstream_no_barriers_{k}", _case(DOC, s, g)))
    for k, g in enumerate([(0, 0), (2, 3), (4, 1), (3, 1)]):              # barriers [1]: its start (2, 0) -> pixel (0, 0) is walled in
        out.append((f"upstream_barriers_{k}", _case(DOC, (0, 0), g, [1])))
    for name, ss, sg in (("none", 0, 0), ("start", 1, 0), ("goal", 0, 1)):   # start and goal on NaN cells
        out.append((f"upstream_snap_{name}", _case(DOC_NAN, (1, 2), (4, 1), (), 8, ss, sg)))
    out.append(("upstream_connectivity_8", _case(DOC_NAN, (1, 2), (4, 1), (), 8, 1, 1)))
    out.append(("upstream_connectivity_4", _case(DOC_NAN, (1, 2), (4, 1), (), 4, 1, 1)))

    # dtypes and connectivities on one random layout (values 0 .. 4, barriers 0 and 3)
    rng = np.random.default_rng(101)
    base = rng.integers(0, 5, (17, 23))
    base[0, 0] = base[-1, -1] = 1
    for dt in (np.int8, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.float32, np.float64):
        for conn in (4, 8):
            out.append((f"values_{np.dtype(dt).name}_c{conn}", _case(base.astype(dt), (0, 0), (16, 22), [0, 3] if conn == 8 else [3], conn)))
    # NaN cells, +-inf cells crossable, then inf as a barrier
    f = rng.integers(1, 5, (15, 19)).astype(np.float64)
    f[rng.random(f.shape) < 0.25] = np.nan
    f[rng.random(f.shape) < 0.10] = np.inf
    f[rng.random(f.shape) < 0.10] = -np.inf
    f[0, 0], f[-1, -1], f[7, 9] = 1.0, np.inf, -np.inf
    for conn in (4, 8):
        out.append((f"nan_inf_crossable_c{conn}", _case(f, (0, 0), (14, 18), (), conn)))
        out.append((f"nan_inf_barrier_c{conn}", _case(f.astype(np.float32), (0, 0), (7, 9), [np.inf], conn)))
        out.append((f"nan_inf_both_barriers_c{conn}", _case(f, (0, 0), (14, 17), [np.inf, -np.inf, 4.0], conn)))
    # integer barriers that float64 cannot tell apart
    big = 2 ** 53
    zi = np.where(rng.random((12, 16)) < 0.35, big + 1, big).astype(np.int64)
    zi[0, 0] = zi[-1, -1] = big
    assert np.float64(big) == np.float64(big + 1)
    for conn in (4, 8):
        out.append((f"int64_beyond_2_53_c{conn}", _case(zi, (0, 0), (11, 15), [big + 1], conn)))
    out.append(("int64_beyond_2_53_other_value", _case(zi, (0, 0), (11, 15), [big + 3, big + 2], 8)))
    # start == goal; start or goal on a barrier, with and without snapping
    m = maze((14, 18), 7, 0.3)
    m[5, 5] = m[9, 12] = 0
    out.append(("start_is_goal", _case(m, (0, 0), (0, 0), [0])))
    out.append(("start_is_goal_on_barrier", _case(m, (5, 5), (5, 5), [0])))
    out.append(("start_is_goal_on_barrier_snapped", _case(m, (5, 5), (5, 5), [0], 8, 1, 1)))
    for conn in (4, 8):
        out.append((f"start_on_barrier_c{conn}", _case(m, (5, 5), (13, 17), [0], conn)))
        out.append((f"start_on_barrier_snapped_c{conn}", _case(m, (5, 5), (13, 17), [0], conn, 1, 0)))
        out.append((f"goal_on_barrier_c{conn}", _case(m, (0, 0), (9, 12), [0], conn)))
        out.append((f"goal_on_barrier_snapped_c{conn}", _case(m, (0, 0), (9, 12), [0], conn, 0, 1)))
        out.append((f"both_on_barriers_snapped_c{conn}", _case(m, (5, 5), (9, 12), [0], conn, 1, 1)))
    # snapping finds nothing: an all-barrier raster, and the opposite corner, which the strict < of the first distance excludes
    out.append(("snap_all_barriers", _case(np.zeros((6, 7), np.int32), (2, 3), (4, 4), [0], 8, 1, 1)))
    corner = np.zeros((6, 7), np.float32)
    corner[-1, -1] = 1
    out.append(("snap_opposite_corner_start", _case(corner, (0, 0), (5, 6), [0], 8, 1, 0)))
    out.append(("snap_opposite_corner_goal", _case(corner, (5, 6), (0, 0), [0], 8, 0, 1)))
    corner2 = corner.copy()
    corner2[-1, -2] = 1
    out.append(("snap_next_to_opposite_corner", _case(corner2, (0, 0), (5, 6), [0], 8, 1, 0)))
    # walled-off goals
    wall = np.ones((16, 20), np.float32)
    wall[10:15, 12] = wall[10:15, 18] = wall[10, 12:19] = wall[14, 12:19] = 0
    for conn in (4, 8):
        out.append((f"walled_off_goal_c{conn}", _case(wall, (0, 0), (12, 15), [0], conn)))
    wall2 = np.ones((16, 20), np.float64)
    wall2[:, 9] = np.nan
    out.append(("nan_wall_across", _case(wall2, (3, 2), (12, 17))))
    diag = np.ones((12, 12), np.int16)
    np.fill_diagonal(diag, 0)
    out.append(("diagonal_wall_c4", _case(diag, (0, 11), (11, 0), [0], 4)))       # closed to 4-connectivity,
    out.append(("diagonal_wall_c8", _case(diag, (0, 11), (11, 0), [0], 8)))       # open to 8: diagonal steps pass between corners
    # serpentines and mazes on 4-connectivity: one shortest path each
    out.append(("serpentine_21x25_c4", _case(serpentine(21, 25), (0, 0), (20, 0), [0], 4)))
    out.append(("serpentine_25x21_vertical_c4", _case(serpentine(21, 25, np.float32, True), (0, 0), (0, 20), [0], 4)))
    out.append(("serpentine_39x40_c4", _case(serpentine(39, 40, np.uint8), (0, 0), (38, 39), [0], 4)))
    out.append(("serpentine_15x30_c8", _case(serpentine(15, 30), (0, 0), (14, 29), [0], 8)))
    for k, (h, w) in enumerate([(21, 21), (25, 31), (31, 25), (39, 39), (33, 39), (27, 35), (39, 29), (35, 35)]):
        z = tree_maze(h, w, 300 + k, (np.int32, np.float32, np.int64, np.uint8)[k % 4])
        out.append((f"tree_maze_{h}x{w}_c4", _case(z, (0, 0), (h - 1, w - 1), [0], 4)))
        out.append((f"tree_maze_{h}x{w}_inner_c4", _case(z, (h - 1, 0), (2 * (h // 4), 2 * (w // 4)), [0], 4)))
    for k, share in enumerate((0.40, 0.42, 0.44, 0.46, 0.48, 0.50, 0.40, 0.45)):
        z = maze((30 + k, 40 - k), 500 + k, share)
        out.append((f"random_maze_{k}_c4", _case(z, (0, 0), (z.shape[0] - 1, z.shape[1] - 1), [0], 4, 0, 0)))
        out.append((f"random_maze_{k}_snapped_c4", _case(z, (z.shape[0] // 2, 3), (3, z.shape[1] // 2), [0], 4, 1, 1)))
    for k in range(4):
        z = maze((26, 34), 600 + k, 0.30, np.float32)
        out.append((f"random_maze_{k}_c8", _case(z, (0, 0), (25, 33), [0], 8)))
    out.append(("open_ground_c8", _case(np.ones((12, 20), np.float32), (0, 0), (11, 19))))
    out.append(("open_ground_c4", _case(np.ones((12, 20), np.float32), (11, 0), (0, 19), (), 4)))
    out.append(("one_row", _case(np.array([[1, 1, 1, 0, 1, 1, 1, 1]], np.int32), (0, 0), (0, 7), [5])))
    out.append(("one_column_blocked", _case(np.array([[1, 1, 1, 0, 1, 1, 1, 1]], np.int32).T.copy(), (0, 0), (7, 0), [0])))
    return out


def ref_functions():
    return rx.lift("pathfinding.py", LIFTED, {"ngjit": lambda f: f})


def reference(ns, c):
    """(image, (warned at the start, warned at the goal)): `a_star_search` from the pixel ids on, with the lifted functions"""
    data, barriers = c["z"], c["barriers"]
    conn, snap_start, snap_goal = (int(v) for v in c["args"])
    start_py, start_px = (int(v) for v in c["start"])
    goal_py, goal_px = (int(v) for v in c["goal"])
    with np.errstate(all="ignore"):
        if snap_start:
            start_py, start_px = ns["_find_nearest_pixel"](start_py, start_px, data, barriers)
        warn_start = bool(ns["_is_not_crossable"](data[start_py, start_px], barriers))
        if snap_goal:
            goal_py, goal_px = ns["_find_nearest_pixel"](goal_py, goal_px, data, barriers)
        warn_goal = bool(ns["_is_not_crossable"](data[goal_py, goal_px], barriers))
        img = np.zeros_like(data, dtype=np.float64)
        img[:] = np.nan
        if start_py != ns["NONE"]:
            ys, xs = ns["_neighborhood_structure"](conn)
            ns["_a_star_search"](data, img, start_py, start_px, goal_py, goal_px, barriers, ys, xs)
    return img, np.array([warn_start, warn_goal])


def signature():
    """[[name, kind, default as JSON or null for none]] of the reference's `a_star_search`, read from its source"""
    with open(os.path.join(rx.REF_PKG, "pathfinding.py")) as fh:
        tree = ast.parse(fh.read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "a_star_search")
    assert not (fn.args.posonlyargs or fn.args.kwonlyargs or fn.args.vararg or fn.args.kwarg)
    names = [a.arg for a in fn.args.args]
    defaults = [None] * (len(names) - len(fn.args.defaults)) + [json.dumps(ast.literal_eval(d)) for d in fn.args.defaults]
    return [[n, "POSITIONAL_OR_KEYWORD", d] for n, d in zip(names, defaults)]


def run_all():
    ns = ref_functions()
    store = {"signature": np.array(json.dumps(signature()))}
    for name, c in cases():
        for k, v in c.items():
            store[f"{name}/{k}"] = v
        store[f"{name}/image"], store[f"{name}/warned"] = reference(ns, c)
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def names(store):
    return sorted({k.split("/")[0] for k in store if "/" in k})


def call_args(store, name):
    """(z, start, goal, barriers, connectivity, snap_start, snap_goal) of a stored case"""
    conn, ss, sg = (int(v) for v in store[f"{name}/args"])
    return (store[f"{name}/z"], tuple(int(v) for v in store[f"{name}/start"]), tuple(int(v) for v in store[f"{name}/goal"]),
            store[f"{name}/barriers"], conn, bool(ss), bool(sg))


def unique_cases(store):
    """the cases with a path that have exactly one shortest path, by the oracle's counter"""
    from tests import pathfinding_oracle as po
    return [n for n in names(store) if po.run(*call_args(store, n))["n_paths"] == 1]


def check():
    want, got = load(), run_all()
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
        print("astar_exec.npz reproduces" if ok else "astar_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    uniq = unique_cases(st)
    with_path = [n for n in names(st) if not np.isnan(st[f"{n}/image"]).all()]
    if len(uniq) < MIN_UNIQUE:
        sys.exit(f"REFUSED: only {len(uniq)} cases have exactly one shortest path, {MIN_UNIQUE} are needed")
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(names(st))} cases, {len(with_path)} with a path, {len(uniq)} of them with exactly one shortest path, "
          f"{os.path.getsize(OUT)} bytes")
