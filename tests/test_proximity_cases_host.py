"""CPU proof that the cases of tests/proximity_cases.py are what they claim: the scan references against a plain loop, the
row lists' lengths, the walks that the search's cases are named for (through the model `proximity_cases.walk`), the ties, the
cuts at equality, the tie runs that the nearest-left / nearest-right candidate set gets wrong, and the share of cells that the
great-circle cases leave out.  No GPU; tests/test_gpu_proximity_abi.py runs the same cases on the device."""
import numpy as np
import pytest

from tests import proximity_cases as pc
from tests import proximity_oracle as po

GC_GAP_ULP, GC_LEFT_OUT = 2, 0.005                                       # as tests/test_gpu_proximity.py


@pytest.fixture(scope="module")
def search_cases():
    return {c.name: c for c in pc.search_cases()}


def _winner_differs(case, metric, run, extend):
    w = pc.walk(case, metric, extend=extend)
    return (w["row"] != run["row"]) | (w["col"] != run["col"]), w


# ------------------------------------------------------------------------------------------------ the references themselves
def test_scan_reference_against_a_plain_loop():
    t = pc.width_raster(65) != 0
    ref = pc.scan_reference(t)
    for i in range(t.shape[0]):
        for j in range(t.shape[1]):
            at_or_left = [c for c in range(j + 1) if t[i, c]]
            beyond = [c for c in range(j + 1, t.shape[1]) if t[i, c]]
            assert ref["left"][i, j] == (at_or_left[-1] if at_or_left else -1), (i, j)
            assert ref["right"][i, j] == (beyond[0] if beyond else -1), (i, j)
    assert ref["flag"].tolist() == [0, 1, 1, 1, 1, 1, 1, int(t[7].any())]
    assert ref["list"].tolist() == [r for r in range(8) if t[r].any()] and ref["count"] == len(ref["list"])
    assert (ref["right"][:, -1] == -1).all()                              # exclusive: nothing lies right of the last column
    assert ref["left"][4].tolist() == list(range(65)) and ref["right"][4, :-1].tolist() == list(range(1, 65))


def test_layout_is_the_size_the_existing_test_states():
    for rows, cols in ((300, 400), (1, 1), (700, 5), (8, 769)):
        lay = pc.layout(rows, cols)
        assert lay["total"] == 2 * pc.up256(rows * cols * 4) + 2 * pc.up256(rows * 4) + 256
        order = [lay[k] for k in ("left", "right", "flag", "list", "count", "total")]
        assert order == sorted(order) and all(v % 256 == 0 for v in order)
        assert lay["right"] - lay["left"] >= rows * cols * 4 and lay["list"] - lay["flag"] >= rows * 4


def test_width_rasters_hold_every_kind_of_row():
    assert pc.WIDTHS == (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769)
    for cols in pc.WIDTHS:
        t = pc.width_raster(cols) != 0
        assert t.shape == (8, cols) and not t[0].any() and t[4].all()
        assert np.flatnonzero(t[1]).tolist() == [0] and np.flatnonzero(t[2]).tolist() == [cols - 1]
        assert np.flatnonzero(t[3]).tolist() == ([c for c in (255, 256) if c < cols] or [cols // 2])
        only5, only6 = np.flatnonzero(t[5]), np.flatnonzero(t[6])
        assert only5.size == 1 and only5[0] < pc.SPAN and only6.size == 1 and only6[0] >= cols - pc.SPAN
        if cols > 2 * pc.SPAN:                                            # the carry crosses at least two spans, each way
            assert (cols - 1) // pc.SPAN - only5[0] // pc.SPAN >= 2
            assert (cols - 1 - only6[0]) // pc.SPAN == 0 and (cols - 1) // pc.SPAN >= 2
    assert -(-769 // pc.SPAN) == 4 and 769 % pc.SPAN != 0                 # four steps; the two passes cut at different columns


def test_row_lists_have_the_lengths_that_matter():
    counts = set()
    for rows in pc.HEIGHTS:
        for pattern in pc.FLAG_PATTERNS:
            f = pc.flag_rows(rows, pattern)
            sc = pc.scan_reference(pc.flag_raster(rows, 3, pattern) != 0)
            assert np.array_equal(sc["flag"].astype(bool), f) and sc["count"] == int(f.sum()), (rows, pattern)
            counts.add(sc["count"])
    assert {0, 1, 255, 256, 257, 512, 513} <= counts, sorted(counts)
    assert any(580 <= c <= 620 for c in counts), sorted(counts)
    assert np.flatnonzero(pc.flag_rows(700, "seams")).tolist() == [255, 256, 511, 512]
    none = pc.flag_raster(700, 5, "none", np.float32)
    assert np.isnan(none).all() and not po.targets(none).any()


def test_dtype_rasters_hold_what_is_no_target():
    assert [np.dtype(d) for d in pc.DTYPES] == [np.dtype(n) for n in ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64",
                                                                      "uint64", "float64", "float32")]
    for dt in pc.DTYPES:
        z = pc.dtype_raster(dt)
        t = po.targets(z)
        assert z.shape == (5, 300) and z.dtype == np.dtype(dt) and t.any() and not t[1].any() and t[-1, -1]
        if np.dtype(dt).kind == "f":
            for v in (np.inf, -np.inf):
                assert (z == v).any() and not t[z == v].any()
            assert np.isnan(z).any() and not t[np.isnan(z)].any()
            assert (np.signbit(z) & (z == 0)).any() and not t[z == 0].any()
        else:
            assert (z == np.iinfo(dt).max).any() and t[z == np.iinfo(dt).max].all()


def test_value_cases_mean_what_numpy_means():
    cases = dict((n, (z, tv)) for n, z, tv in pc.value_cases())
    for name, (z, tv) in cases.items():
        t = po.targets(z, tv)
        assert np.array_equal(t, pc.exact_targets(z, tv)), name
        assert tv.dtype in pc.VALUES_KIND and (tv.dtype == np.float64 or z.dtype.kind in "iu"), name
    hits = {n: int(po.targets(z, tv).sum()) for n, (z, tv) in cases.items()}
    for f in ("float32", "float64"):
        z = cases[f"{f}_inf"][0]
        assert np.array_equal(po.targets(*cases[f"{f}_inf"]), z == np.inf) and hits[f"{f}_inf"] > 0 and (z == -np.inf).any()
        assert hits[f"{f}_nan"] == 0 and np.isnan(z).any()
        zero = po.targets(*cases[f"{f}_zero"])
        assert zero[np.signbit(z) & (z == 0)].all() and (np.signbit(z) & (z == 0)).any()
    assert hits["float32_tenth"] == 0 and (cases["float32_tenth"][0] == np.float32(0.1)).any() and hits["float64_tenth"] > 0
    z = cases["int64_beyond_2_53"][0]
    assert np.array_equal(po.targets(*cases["int64_beyond_2_53"]), z == 2 ** 53 + 1) and (z == 2 ** 53).any()
    for u in ("uint8", "uint16", "uint32", "uint64"):
        assert hits[f"{u}_negative_i64"] == 0 and (cases[f"{u}_negative_i64"][0] == np.iinfo(u).max).any()
        assert hits[f"{u}_negative_i64_and_7"] == int((cases[f"{u}_negative_i64"][0] == 7).sum()) > 0
    for s in ("int8", "int16", "int32", "int64"):
        z = cases[f"{s}_u64_above_2_63"][0]
        assert hits[f"{s}_u64_above_2_63"] == 0 and (z == -1).any() and (z == np.iinfo(s).min).any()
        assert hits[f"{s}_u64_above_2_63_and_7"] == int((z == 7).sum()) > 0
    assert hits["uint64_u64_above_2_63"] == int((cases["uint64_u64_above_2_63"][0] == 2 ** 63 + 5).sum()) > 0
    assert hits["uint64_u64_top"] > 0
    assert hits["int32_f64_two"] > 0 and hits["int32_f64_two_and_a_half"] == 0


# ------------------------------------------------------------------------------------------------ the walks
@pytest.mark.parametrize("name", ["far_40x300", "mixed_40x256", "ring", "ring_max5", "ring_max0", "order_y_rising_x_falling",
                                  "uneven_23x90_max6", "rows_513x9_seams"])
def test_the_model_finds_the_oracles_winner(search_cases, name):
    """the model is the kernel's algorithm: with the tie extension it names the rule's target at every cell"""
    case = search_cases[name]
    for metric in case.metrics:
        run = po.run(case.z, case.xs, case.ys, case.tv, case.md, metric)
        differ, _ = _winner_differs(case, metric, run, extend=True)
        assert not differ.any(), (name, metric, np.argwhere(differ)[:5].tolist())


def test_far_case_keeps_walking(search_cases):
    case = search_cases["far_40x300"]
    run = po.run(case.z, case.xs, case.ys)
    w = pc.walk(case, "EUCLIDEAN")
    corner = (slice(35, 40), slice(0, 10))
    assert (run["row"][corner] == 5).all() and (run["d32"][corner] >= 30).all()
    assert (w["up"][corner] >= 30).all()                                  # 30 rows whose candidates lose, then the winner's
    for r in range(6, 40):                                                # every nearer row holds one far-away target only
        cols = np.flatnonzero(case.z[r])
        assert cols.size == 1 and cols[0] >= 297


def test_mixed_block_closes_lanes_many_rows_apart(search_cases):
    case = search_cases["mixed_40x256"]
    assert case.z.shape[1] == pc.SPAN                                     # one block per row
    for metric in case.metrics:
        w = pc.walk(case, metric)
        by_bound = w["up_closed"][39] == pc.CLOSED_BY.index("bound")
        ran_out = w["up_closed"][39] == pc.CLOSED_BY.index("rows")
        assert by_bound.sum() >= 20 and ran_out.sum() >= 100, metric
        assert np.ptp(w["up"][39][by_bound]) > 8, metric
        assert np.ptp(w["up"][39][192:][by_bound[192:]]) > 8, metric      # and inside the block's last wave alone, too


def test_ring_has_the_ties_and_the_cuts(search_cases):
    ring = search_cases["ring"]
    ties = pc.tie_counts(ring, "EUCLIDEAN")
    for centre in pc.RING_CENTRES:
        assert ties[centre] == 12 and not ring.z[centre]
    assert {2, 4, 12} <= set(np.unique(ties).tolist())
    assert ties[15, 54] == 2 and ties[22, 62] == 2 and ties[24, 48] == 4
    cut = search_cases["ring_max5"]
    max2 = np.float64(cut.md) ** 2
    for metric in cut.metrics:
        run = po.run(cut.z, cut.xs, cut.ys, cut.tv, cut.md, metric)
        s = (run["d32"] * run["d32"]).astype(np.float64)
        at_cut = (s == max2) & (run["row"] >= 0)
        assert at_cut.sum() >= 4, metric                                  # kept at equality
        w = pc.walk(cut, metric)
        below_lone = (pc.LONE[0] + 5, pc.LONE[1])                         # its only target within 5 is 5 rows straight above
        assert run["row"][below_lone] == pc.LONE[0] and run["col"][below_lone] == pc.LONE[1] and at_cut[below_lone], metric
        assert w["at_cut"][below_lone] >= 1 and w["row"][below_lone] == pc.LONE[0], metric
        assert (w["up_closed"] == pc.CLOSED_BY.index("max_distance")).any() and (w["dn_closed"] == pc.CLOSED_BY.index("max_distance")).any()
        assert np.isnan(run["proximity"]).any()
    zero = search_cases["ring_max0"]
    run = po.run(zero.z, zero.xs, zero.ys, zero.tv, zero.md)
    assert np.array_equal(~np.isnan(run["proximity"]), zero.z != 0)


def test_row_cases_have_cells_above_and_below_every_row(search_cases):
    for shape in ("700x5", "513x9"):
        seams = search_cases[f"rows_{shape}_seams"]
        rows = np.flatnonzero((seams.z != 0).any(axis=1))
        assert rows[0] == 255 and rows[-1] == 512 and (seams.z.shape[0] > 513 or shape == "513x9")   # 700: cells below them too
        assert pc.scan_reference(search_cases[f"rows_{shape}_none"].z == 1)["count"] == 0
        assert not po.targets(search_cases[f"rows_{shape}_none"].z).any()
        assert po.targets(search_cases[f"rows_{shape}_row0"].z).any(axis=1).sum() == 1
        assert po.targets(search_cases[f"rows_{shape}_last"].z).any(axis=1).tolist()[-1]


def test_the_issues_cases_are_all_there(search_cases):
    names = set(search_cases)
    for shape in ("700x5", "513x9"):
        assert {f"rows_{shape}_{p}" for p in pc.FLAG_PATTERNS} <= names
    assert {"far_40x300", "mixed_40x256", "ring", "ring_max5", "ring_max0", "uneven_23x90", "width_257", "width_513", "alloc_int8",
            "alloc_uint16", "alloc_uint32"} <= names
    assert len([n for n in names if n.startswith("order_")]) == 4
    assert search_cases["ring_max5"].md == 5.0 and search_cases["ring_max0"].md == 0.0
    for n in ("order_y_falling_x_rising", "order_y_rising_x_falling"):
        c = search_cases[n]
        assert (np.diff(c.ys) > 0).all() == ("y_rising" in n) and (np.diff(c.xs) > 0).all() == ("x_rising" in n)
    steps = np.diff(search_cases["uneven_23x90"].xs)
    assert steps.min() > 0 and steps.max() > 2 * steps.min()
    assert search_cases["alloc_int8"].z.min() == -128 and search_cases["alloc_uint32"].z.max() == 2 ** 32 - 1
    assert search_cases["width_257"].z.shape[1] % pc.SPAN == 1 and search_cases["width_513"].z.shape[1] % pc.SPAN == 1


# ------------------------------------------------------------------------------------------------ the tie runs
@pytest.mark.parametrize("case", pc.tie_run_cases(), ids=lambda c: c.name)
def test_tie_runs_defeat_the_nearest_candidates(case):
    """Without the extension (the nearest target left and right of the cell only: the kernel before the fix) the winner differs
    from the rule's at 10 cells and more; with it, at none.  `proximity` itself is the same either way."""
    assert case.z.shape == (8, 40) and not case.z[1::2].any()
    for metric in case.metrics:
        with np.errstate(over="ignore"):                                 # (1e30 x 1e39 overflows float32 on purpose)
            run = po.run(case.z, case.xs, case.ys, case.tv, case.md, metric)
            plain, _ = _winner_differs(case, metric, run, extend=False)
            fixed, w = _winner_differs(case, metric, run, extend=True)
        alloc = case.z[run["row"], run["col"]]
        print(f"{case.name} {metric}: nearest-only winner differs at {int(plain.sum())} of {plain.size} cells, "
              f"extended at {int(fixed.sum())}; {int(w['extended'].sum())} cells extended a run")
        assert plain.sum() >= 10, (case.name, metric)
        assert not fixed.any() and w["extended"].sum() >= 10, (case.name, metric)
        assert np.array_equal(alloc.astype(np.float32), run["allocation"])
    if case.name == "tie_run_all_zero_1e-46":
        assert (po.run(case.z, case.xs, case.ys)["d32"] == 0).all()
    if case.name == "tie_run_inf_1e30x1e39":
        assert np.isinf(run["d32"][1::2]).all()
    if case.name == "tie_run_all_inf_1e39":
        assert np.isinf(run["d32"][case.z == 0]).all() and (run["d32"][case.z != 0] == 0).all()


@pytest.mark.parametrize("case", pc.margin_cases(), ids=lambda c: c.name)
def test_margin_cases_tie_at_the_widest_ratio(case):
    """two targets one float32 value apart from nothing: equal d32, the float64 ratio 0.99 of what float32 allows at most"""
    i, j = (1, 2) if case.name == "margin_above" else (0, 2)
    (r0, c0), (r1, c1) = np.argwhere(case.z != 0)
    for metric in case.metrics:
        m = po.METRICS[metric]
        near, far = sorted((abs(case.xs[c0]), abs(case.xs[c1])))
        d = [po.distance(case.xs[c], case.xs[j], case.ys[r], case.ys[i], m) for r, c in ((r0, c0), (r1, c1))]
        assert d[0] == d[1] == np.float32(1.0 + 2.0 ** -23), metric
        assert 0.98 * 2.0 ** -23 < far / near - 1 < 2.0 ** -23 and 2.3e-7 < (far / near) ** 2 - 1 < 2.0 ** -22
        run = po.run(case.z, case.xs, case.ys, (), np.inf, metric)
        plain, _ = _winner_differs(case, metric, run, extend=False)
        fixed, w = _winner_differs(case, metric, run, extend=True)
        assert plain[i, j] and not fixed.any() and w["extended"][i, j], metric
        assert abs(case.xs[run["col"][i, j]]) == far                     # the rule names the farther of the two


def test_square_cells_have_no_tie_runs():
    """the same raster on unit cells: the nearest candidates are the whole story (the issue's table, first row)"""
    case = pc.Case("square", pc.tie_run_raster(), *pc.tie_run_coords(1.0, 1.0), "")
    for metric in ("EUCLIDEAN", "MANHATTAN"):
        run = po.run(case.z, case.xs, case.ys, (), np.inf, metric)
        plain, w = _winner_differs(case, metric, run, extend=False)
        assert not plain.any(), metric


def test_great_circle_limit_is_real():
    """GREAT_CIRCLE does not extend: on degenerate longitudes its candidate set differs from the rule's winner"""
    case = pc.great_circle_tie_case()
    run = po.run(case.z, case.xs, case.ys, (), np.inf, "GREAT_CIRCLE")
    plain, _ = _winner_differs(case, "GREAT_CIRCLE", run, extend=True)     # (extend has no effect under GREAT_CIRCLE)
    assert plain.sum() >= 10
    assert len(np.unique(case.z[case.z != 0])) == int((case.z != 0).sum())  # allocation names the target


# ------------------------------------------------------------------------------------------------ great circle
@pytest.mark.parametrize("case", pc.great_circle_cases() + [pc.roundtrip_case()], ids=lambda c: c.name)
def test_great_circle_cases_leave_out_few_cells(case):
    run = po.run(case.z, case.xs, case.ys, case.tv, case.md, "GREAT_CIRCLE")
    close = np.isfinite(run["second"]) & (po.ulps(run["d32"], run["second"]) <= GC_GAP_ULP)
    print(f"{case.name}: {int(close.sum())} of {close.size} cells have a second target within {GC_GAP_ULP} ulp")
    assert close.mean() <= GC_LEFT_OUT
    assert np.abs(case.xs).max() <= 180 and np.abs(case.ys).max() <= 90
    if "wrap" in case.name:
        far = np.abs(case.xs[run["col"]] - case.xs[None, :]) > 180.0
        assert far.sum() >= 10 and case.z.shape[0] == 300
