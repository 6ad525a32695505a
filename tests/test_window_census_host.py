"""The census table (tests/window_census_cases.py) against the sources, without a GPU: it names every walker unit and every
dispatch branch, holds every annulus pair and radius, and builds the masks the walkers are instantiated for."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import window_census_cases as wc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xrspatial_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _entry_names():
    """The WindowEntryFn declarations of window_call.h, without `try_launch_`."""
    names = []
    for decl in re.findall(r"^WindowEntryFn\s+([^;]*);", _source("window_call.h"), flags=re.M):
        names += re.findall(r"\btry_launch_(\w+)", decl)
    return names


def _branch_tags():
    """The tags kxk.hip hands to the route witness (every string literal inside a `noted(...)` call), and boxsep's."""
    src = _source("kxk.hip")
    tags = []
    for m in re.finditer(r"\bnoted\(", src):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        tags += re.findall(r'"([a-z0-9_]+)"', src[m.end():i])
    tags += re.findall(r'route_note\("([a-z0-9_]+)"', _source("boxsep.hip"))
    return tags


def test_the_sources_name_what_the_census_expects_to_parse():
    entries, tags = _entry_names(), _branch_tags()
    assert len(entries) == len(set(entries)) >= 37, entries
    assert {"focal_mean_runs", "focal_mom_annulus12", "wide_annulus4", "focal_ext_annulus_c", "conv_wide_box"} <= set(entries)
    assert set(tags) == {"big", "pass", "strips3", "strips5", "lds_mean7", "tap0", "tap1", "tap2", "tap3", "tap4", "conv_strips3",
                         "conv_strips5", "conv_tap", "boxsep"}, tags


def test_census_routes_name_every_walker_unit_and_dispatch_branch():
    named = wc.all_route_names()
    missing = (set(_entry_names()) | set(_branch_tags())) - named
    assert not missing, f"no census case expects {sorted(missing)}: add one to tests/window_census_cases.py"
    unknown = named - set(_entry_names()) - set(_branch_tags())
    assert not unknown, f"the census expects routes the sources do not have: {sorted(unknown)}"


def test_census_holds_every_annulus_pair_and_radius():
    ids = [c.id for c in wc.CASES]
    assert len(ids) == len(set(ids))
    pairs = {(c.R, c.RI) for c in wc.CASES if c.kind == 'annulus'}
    assert pairs == {(R, RI) for R in range(4, 13) for RI in range(1, R)} and len(pairs) == 63
    for kind in ('circle', 'box'):
        assert {c.R for c in wc.CASES if c.kind == kind} >= set(range(2, 13))
    for c in wc.CASES:
        if c.kind == 'other' or not 2 <= c.R <= 12:
            continue
        flagged = c.kind != 'annulus' or (c.R, c.RI) in wc.FLAGGED_ANNULI
        for flags in (wc.FLAG_SETS if flagged else (0,)):
            got = {call.stats for call in c.calls if call.what == 'focal' and call.flags == flags and call.workspace == 'api'}
            assert got == set(wc.STAT_SETS), (c.id, flags)
        assert any(call.workspace == 'none' for call in c.calls), c.id
        assert any(call.what == 'conv' for call in c.calls) == (c.R >= 3), c.id


@pytest.mark.parametrize("case", [c for c in wc.CASES if c.kind != 'other'], ids=lambda c: c.id)
def test_masks_are_the_shapes_the_walkers_are_instantiated_for(case):
    """The row formulas of window_call.h (CircleShape::hw, annulus_hole_hw), ported, give the mask the test builds."""
    mask = wc.build_mask(case)
    np.testing.assert_array_equal(mask, wc.shape_mask(case.kind, case.R, case.RI))
    if case.kind == 'annulus':
        assert mask[case.R, case.R] == 0 and mask[case.R, case.R + case.RI] == 0 and mask[case.R, case.R + case.RI + 1] == 1


def test_ragged_masks_are_no_recognised_shape():
    for case in (c for c in wc.CASES if c.kind == 'other'):
        mask = wc.build_mask(case)
        assert set(np.unique(mask)) == {0.0, 1.0} and not wc.suits_run_kernels(mask)
        for kind in ('circle', 'box'):
            assert not np.array_equal(mask, wc.shape_mask(kind, case.R))


def test_route_text_parses_and_the_geometry_conditions_bite():
    text = "focal_ext_annulus_a(9,4)[wave=64,wg=256,rows=130,grid=5x4];focal_mom_annulus9(9,4)[wave=128,wg=512,rows=134,grid=3x4];tap3(9)"
    assert wc.route_names(text) == ["focal_ext_annulus_a(9,4)", "focal_mom_annulus9(9,4)", "tap3(9)"]
    ext, mom, tap = wc.parse_route(text)
    assert (ext.name, ext.R, ext.RI, ext.wave, ext.wgs_y) == ("focal_ext_annulus_a", 9, 4, 64, 4) and tap.wave is None
    assert wc.geometry_faults(ext, 420, 1100, 9) == [] and wc.geometry_faults(mom, 420, 1100, 9) == []
    # the raster the census replaced: one tile row
    one_row = wc.Item("focal_mom_circle", 9, None, 128, 512, 150, 1, 1)
    assert any("tile rows" in f for f in wc.geometry_faults(one_row, 150, 331, 9))
    assert any("workgroups across" in f for f in wc.geometry_faults(one_row, 150, 331, 9))
    # no partial last tile; and a raster whose only whole interior tiles hold decorations
    even = wc.Item("focal_wide_box", 12, None, 128, 512, 140, 3, 3)
    assert any("partial last tile row" in f for f in wc.geometry_faults(even, 420, 1100, 12))
    assert any("free of decorations" in f for f in wc.geometry_faults(wc.Item("focal_wide_box", 12, None, 512, 2048, 130, 1, 4), 420, 1100, 12))


def test_fake_hip_answers_the_route_witness(monkeypatch):
    from tests import fake_hip
    from xrspatial_amd import _lib
    fake_hip.install(monkeypatch)
    assert "xrs_debug_window_route" in _lib.EXPORTED
    z = np.arange(48, dtype=np.float32).reshape(6, 8)
    out = np.zeros_like(z)
    k = np.ones((3, 3))
    ptrs = (ctypes.c_void_p * 7)()
    ptrs[0] = out.ctypes.data
    _lib.call("xrs_focal_stats_f32", z.ctypes.data, ptrs, 1, 6, 8, 8, 8, k.ctypes.data, 3, 3, None, 0, 0, None)
    assert _lib.window_route() == "oracle:xrs_focal_stats_f32"
    buf = ctypes.create_string_buffer(8)
    assert _lib.load().xrs_debug_window_route(buf, 8) == len("oracle:xrs_focal_stats_f32") and buf.value == b"oracle:"
