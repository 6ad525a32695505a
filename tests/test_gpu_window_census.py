"""Census of the focal / convolve_2d window kernels: every instantiation of the large-window walkers (all 63 annulus pairs,
circles and boxes of radius 2..12, each statistic set, accuracy flag and workspace mode of tests/window_census_cases.py) on a
raster with interior tiles, against the C oracle -- and after every call the route witness (xrs_debug_window_route) must name
the kernels the dispatch table promises, with a tiling that really puts interior tiles, a rim and partial last tiles on the
raster.  One test per mask; the oracle runs once per mask."""
import ctypes
import time

import numpy as np
import pytest

import xrspatial_amd as xs
from oracle import c_oracle as corc
from tests import parity_log
from tests import window_census_cases as wc
from tests.test_gpu_parity import RIM_MOMENT_RTOL, check_window_sum, raster
from xrspatial_amd import _lib
from xrspatial_amd import focal as focal_mod
from xrspatial_amd.convolution import convolve_2d
from xrspatial_amd.focal import apply, focal_stats

pytestmark = pytest.mark.gpu

_rasters = {}


def _raster(shape):
    if shape not in _rasters:
        z = wc.census_raster(shape)
        z.setflags(write=False)
        _rasters[shape] = z
    return _rasters[shape]


def _check_route(case, call, rows, cols, what, **shard):
    text = _lib.window_route()
    assert wc.route_names(text) == list(call.route), f"{what}: served by {text!r}, the dispatch table promises {call.route}"
    tiled = [it for it in wc.parse_route(text) if it.wave]
    for it in tiled:
        faults = wc.geometry_faults(it, rows, cols, case.R, **shard)
        assert not faults, f"{what}: {rows}x{cols} under {it}: {faults}"
    return tiled


def _interior_cells(tiled, rows, cols, R):
    """Boolean plane: the cells of the clean, whole, interior wave tiles of every tiled launch of the call."""
    inside = np.zeros((rows, cols), bool)
    for it in tiled:
        for ty, tx in wc.clean_interior_wave_tiles(it, rows, cols, R):
            inside[ty * it.tile_rows:(ty + 1) * it.tile_rows, tx * it.wave:(tx + 1) * it.wave] = True
    return inside


def _check_planes(case, call, got, want, z, k, sum_abs, what, rows=slice(None), interior=None):
    """`got`: {stat: plane} of one call; `want`: the oracle's planes of the whole raster, `rows` of which the call produced."""
    exact, seq = call.flags & wc.EXACT, call.flags & wc.SEQ
    for st in call.stats:
        g, w, msg = got[st], want[st][rows], f"{what} {st}"
        if st in ('max', 'min', 'range'):
            np.testing.assert_array_equal(g, w, err_msg=msg)
        elif st == 'sum':
            if seq:
                np.testing.assert_array_equal(g, w, err_msg=msg)
            else:
                hatch = check_window_sum(g, z[rows], k, msg, want=w, sum_abs=sum_abs[rows])
                assert hatch == 0, f"{msg}: {hatch} windows beyond 1e-5 of the reference's sum"
        else:
            np.testing.assert_allclose(g, w, rtol=1e-6 if exact else 1e-5, atol=0, equal_nan=True, err_msg=msg)
            assert np.array_equal(np.isnan(g), np.isnan(w)), msg
            parity_log.record(f'census {z.shape[0]}x{z.shape[1]}', f'{case.id} {st}' + (' exact' if exact else ''), g, w)
            if interior is not None and interior.any() and not exact:
                # the documented float32 figures on decoration-free interior tiles: recorded, and reported when exceeded
                rel, _ = parity_log.record('census: decoration-free interior tiles', f'{case.id} {st}', g[interior], w[interior],
                                           tol=f"{RIM_MOMENT_RTOL if st == 'var' else RIM_MOMENT_RTOL / 2:g} documented")
                if rel > (RIM_MOMENT_RTOL if st == 'var' else RIM_MOMENT_RTOL / 2):
                    print(f"CENSUS FINDING {what} {st}: {rel:.3g} on interior tiles")
    if rows == slice(None):
        ly, lx = wc.lake_interior(case.R)
        if ly.start < ly.stop <= z.shape[0] and lx.start < lx.stop:
            if 'mean' in got:
                assert (got['mean'][ly, lx] == wc.LAKE_VALUE).all(), f"{what}: mean on the lake"
            for st in ('var', 'std'):
                if st in got:
                    assert (got[st][ly, lx] == 0).all(), f"{what}: {st} on the lake"


@pytest.mark.parametrize("case", wc.CASES, ids=[c.id for c in wc.CASES])
def test_window_census(case, monkeypatch):
    t0 = time.perf_counter()
    z = _raster(case.shape)
    rows, cols = z.shape
    k = wc.build_mask(case)
    K = k.shape[0]
    kk = np.ascontiguousarray(k, dtype=np.float64)
    with np.errstate(all='ignore'):
        want = {st: corc.focal_apply(z, k, st, nthreads=8) for st in wc.STATS}
        absz = np.abs(np.nan_to_num(z, nan=0.0, posinf=0.0, neginf=0.0)).astype(np.float32)
        sum_abs = corc.focal_apply(absz, k, 'sum', nthreads=8)
    agg = raster(z)
    full = None
    for call in case.calls:
        what = f"{case.id} {call.what} {'+'.join(call.stats)} flags={call.flags} workspace={call.workspace}"
        if call.what == 'conv':
            kn = k / k.sum()
            with np.errstate(all='ignore'):
                want_c = corc.convolve_2d(z, kn, nthreads=8)
            got_c = convolve_2d(z, kn)
            _check_route(case, call, rows, cols, what)
            np.testing.assert_allclose(got_c, want_c, rtol=2e-6, atol=0, equal_nan=True, err_msg=what)
            assert np.array_equal(np.isnan(got_c), np.isnan(want_c)), what
            parity_log.record(f'census {rows}x{cols}', f'{case.id} convolve_2d', got_c, want_c)
        elif call.workspace == 'api':
            monkeypatch.setitem(focal_mod.options, 'moments', 'exact' if call.flags & wc.EXACT else 'fast')
            monkeypatch.setitem(focal_mod.options, 'sum', 'sequential' if call.flags & wc.SEQ else 'rounded')
            if len(call.stats) == 1:                       # one statistic: focal.apply with the built-in reducer
                got = {call.stats[0]: apply(agg, k, getattr(focal_mod, '_calc_' + call.stats[0])).data}
            else:
                res = focal_stats(agg, k, stats_funcs=list(call.stats))
                got = {st: res.data[i] for i, st in enumerate(call.stats)}
            tiled = _check_route(case, call, rows, cols, what)
            _check_planes(case, call, got, want, z, k, sum_abs, what, interior=_interior_cells(tiled, rows, cols, case.R))
        else:
            # a row shard with halo rows and no workspace, at the C ABI: interior tiles reach into the halos
            if full is None:
                full = xs.DeviceArray.from_numpy(z)
            first, n = wc.SHARD_FIRST, wc.SHARD_ROWS
            ht = hb = K // 2
            outs = {st: xs.DeviceArray((n, cols), np.float32) for st in call.stats}
            ptrs = (ctypes.c_void_p * 7)()
            mask = 0
            for st, arr in outs.items():
                ptrs[wc.STATS.index(st)] = arr.ptr
                mask |= 1 << wc.STATS.index(st)
            _lib.call("xrs_focal_stats_f32", full.ptr + first * cols * 4, ptrs, mask, n, cols, cols, cols, kk.ctypes.data, K, K, None,
                      ht, hb, None)
            _lib.call("xrs_stream_sync", None)
            _check_route(case, call, n, cols, what, first_row=first, halo_top=ht, halo_bot=hb)
            _check_planes(case, call, {st: arr.get() for st, arr in outs.items()}, want, z, k, sum_abs, what,
                          rows=slice(first, first + n))
    parity_log.record('census: wall time per test (seconds, as max_abs)', case.id, [time.perf_counter() - t0], [0.0])
