"""CPU checks of viewshed(method='mesh'): every piece of the rule (tests/viewshed_mesh_oracle.py) that the reference computes
outside its OptiX trace, against the reference's own functions executed on the CPU (tests/golden/viewshed_mesh_exec.npz);
analytic cases for the brute force; and the argument checks and refusals, which run before any device work."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import hillshade_shadow_oracle as ho
from tests import viewshed_mesh_oracle as vo
from tests.golden import make_reference_exec as rx
from tests.golden import make_viewshed_mesh_exec as gen

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)
# the float32-arithmetic allowance of tests/test_hillshade_shadow_host.py (2^-24 per stored float32, fewer than ten per result),
# plus 1e-6 absolute: a direction component is a difference of float32 heights of magnitude up to max(H, W) = 11, each good
# to 2^-24 * 11 = 7e-7, and may itself be anywhere near zero
RTOL, ATOL = 1e-6, 1e-6


def _agg(a, **kw):
    import xrspatial_amd as xs
    return xs.DataArray(a, dims=["y", "x"], **kw)


def _case(name):
    view = tuple(int(v) for v in FIXTURE[f"{name}/view"])
    elev = tuple(float(v) for v in FIXTURE[f"{name}/elev"])
    res = tuple(float(v) for v in FIXTURE[f"{name}/res"])
    return FIXTURE[f"{name}/data"], view, elev, res


# ------------------------------------------------------------------ the rule against the executed reference
def test_fixture_covers_what_the_rule_distinguishes():
    dtypes, spots = set(), set()
    for name in CASES:
        data, (r, c), _, _ = _case(name)
        H, W = data.shape
        assert H <= 9 and W <= 11
        dtypes.add(data.dtype.name)
        spots.add(("last row" if r == H - 1 else "corner" if (r, c) == (0, 0) else "inside" if 0 < r < H - 1 and 0 < c < W - 1 else "",
                   "last column" if c == W - 1 else ""))
    assert dtypes == {"float32", "float64", "int16"}
    assert {("inside", ""), ("corner", ""), ("last row", ""), ("", "last column"), ("last row", "last column")} <= spots


@pytest.mark.parametrize("case", CASES)
def test_surface_origins_equal_the_primary_ray_kernel(case):
    """every cell, the stepped-back last row and column included"""
    want = FIXTURE[f"{case}/primary"]
    H, W = want.shape[:2]
    S, _ = vo.surface_points(ho.mesh(FIXTURE[f"{case}/data"])[1])
    assert np.array_equal(S[..., :2].astype(np.float32).view(np.uint32), want[..., :2].view(np.uint32))
    assert np.array_equal(S[..., :2], want[..., :2].astype(np.float64))              # (the rule's x0, y0 ARE the float32 origins)
    assert (want[:, W - 1, 0] < W - 1).all() and (want[H - 1, :, 1] < H - 1).all() and (want[:, :W - 1, 0] > np.arange(W - 1)).all()
    assert (want[..., 2] == 10000).all() and (want[..., 4:7] == [0, 0, -1]).all()


@pytest.mark.parametrize("case", CASES)
def test_rays_equal_the_viewshed_ray_kernel(case):
    """origin, direction and length of every target's ray to float32 rounding (RTOL of the component's magnitude + ATOL)"""
    data, view, elev, _ = _case(case)
    got = FIXTURE[f"{case}/vsrays"].astype(np.float64)
    scale, zv, _, _ = ho.mesh(data)
    assert scale == float(FIXTURE[f"{case}/scale"])
    origin, direction, length = vo.rays(zv, view[0], view[1], elev[0] * scale, elev[1] * scale)
    targets = np.ones(zv.shape, bool)
    targets[view] = False
    for what, a, b in (("origin", got[..., 0:3], origin), ("direction", got[..., 4:7], direction), ("length", got[..., 7], length)):
        err = np.abs(a[targets] - b[targets])
        print(f"{case} {what}: largest difference {err.max():.3g}, largest relative to RTOL * |value| + ATOL "
              f"{(err / (RTOL * np.abs(b[targets]) + ATOL)).max():.3g}")
        np.testing.assert_allclose(a[targets], b[targets], rtol=RTOL, atol=ATOL, err_msg=what)
    assert (got[..., 3][targets] == 0).all()                         # tmin = 0; tmax = the length (slot 7)
    unit = np.sqrt((direction[targets] ** 2).sum(axis=-1))
    np.testing.assert_allclose(unit, 1.0, rtol=1e-15, atol=1e-15)
    assert (FIXTURE[f"{case}/hits"][..., 3] < 0).all()               # the triangle's own normal points down: the kernel flips it


@pytest.mark.parametrize("case", CASES)
def test_values_equal_the_calc_viewshed_kernel(case):
    """rule 6 on the fixture's hit flags equals the executed kernel's float32 grid, bit for bit"""
    data, view, elev, res = _case(case)
    flags, want = FIXTURE[f"{case}/flags"][..., 0], FIXTURE[f"{case}/visgrid"]
    mask = flags >= 0
    assert mask.any() and not mask.all() and mask[0, 1] and flags[0, 1] == 0 and not mask[view]
    ang = vo.angles(data, view[0], view[1], elev[0], elev[1], res[0], res[1])
    got = vo.values(ang, mask)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want[view] == 180.0 and (want[mask] == -1).all() and (want[~mask] >= 0).all()


def test_fixture_takes_every_branch_of_the_angle():
    seen = set()
    for case in CASES:
        data, view, elev, _ = _case(case)
        z = np.asarray(data).astype(np.float64)
        diff = (z[view] + elev[0]) - (z + elev[1])
        visible = FIXTURE[f"{case}/flags"][..., 0] < 0
        visible[view] = False
        want = FIXTURE[f"{case}/visgrid"]
        seen |= {"level"} if (visible & (diff == 0)).any() else set()
        seen |= {"below"} if (visible & (diff > 0)).any() else set()
        seen |= {"above"} if (visible & (diff < 0)).any() else set()
        assert (want[visible & (diff == 0)] == 90).all() and (want[visible & (diff > 0)] < 90).all() and (want[visible & (diff < 0)] > 90).all()
    assert seen == {"level", "below", "above"}


@pytest.mark.skipif(not rx.have_reference(), reason="the reference is not present here")
def test_fixture_reproduces():
    assert gen.check()


# ------------------------------------------------------------------ analytic cases for the brute force
@pytest.mark.parametrize("elev", [(5, 0), (5, 1), (2, 0), (2, 1)], ids=lambda e: f"oe{e[0]}_te{e[1]}")
def test_level_plane_is_fully_visible(elev):
    """the reference's test_viewshed_flat: 5 x 4 cells of 1.3, xs = arange * 0.5, ys = arange * 1.5, the observer at (0, 0);
    the angles against that test's closed form at its own atol = 0.03 where < 90 -- and far closer"""
    ny, nx = 5, 4
    xs, ys = np.arange(nx) * 0.5, np.arange(ny) * 1.5
    out, mask, ang = vo.viewshed_mesh(np.full((ny, nx), 1.3), 0, 0, elev[0], elev[1], 0.5, 1.5)
    assert not mask.any() and out.dtype == np.float32 and out[0, 0] == 180
    xs2, ys2 = np.meshgrid(xs, ys)
    angle = np.rad2deg(np.arctan2(np.sqrt(xs2 ** 2 + ys2 ** 2), elev[0] - elev[1]))
    angle[0, 0] = out[0, 0]
    below = out < 90
    assert below.sum() == ny * nx - 1
    np.testing.assert_allclose(out[below], angle[below], rtol=0, atol=0.03)
    np.testing.assert_allclose(out, angle, rtol=1e-6, atol=0)
    for view in ((4, 3), (2, 1), (4, 0)):                            # ... and from the stepped-back corner, inside, an edge
        assert not vo.viewshed_mesh(np.full((ny, nx), 1.3), view[0], view[1], elev[0], elev[1])[1].any()
    assert not vo.viewshed_mesh(np.full((ny, nx), 1.3, np.float32), 2, 2, 0, 0)[1].any()       # level with the observer too


def test_wall_across_a_plane_hides_the_cells_behind_it():
    """a wall one vertex wide at column 25 of a 9 x 41 plane, 0.1 of the maximum above it: 4.1 mesh units after the scale
    max(H, W) / max.  The observer at column 5, oe above the plane (oe * 4.1 mesh units): the sight line of a target at column
    j > 25 crosses the ridge at oe * 4.1 * (j - 25) / (j - 5), whatever the row, and clears it iff oe (j - 25) > j - 5.  The
    wall's far face hides itself; everything on the observer's side is seen."""
    z = np.full((9, 41), 9.0)
    z[:, 25] = 10.0
    for oe, first_seen in ((2.5, 39), (4.0, 32)):                    # j > 38.33 and j > 31.67: no column sits on the edge
        for row in (4, 0, 8):
            out, mask, _ = vo.viewshed_mesh(z, row, 5, oe, 0)
            want = np.zeros(z.shape, bool)
            want[:, 25:first_seen] = True
            assert np.array_equal(mask, want), (oe, row, np.argwhere(mask != want)[:8].tolist())
            assert (out[mask] == -1).all() and out[row, 5] == 180 and (out[~mask] >= 0).all()
    _, mask, _ = vo.viewshed_mesh(z, 4, 35, 2.5, 0)                  # from the other side: 2.5 (25 - j) > 35 - j, j < 18.33
    want = np.zeros(z.shape, bool)
    want[:, 19:25] = True                                            # (column 24 is the wall's face turned away from x = 35)
    assert np.array_equal(mask, want), np.argwhere(mask != want)[:8].tolist()
    _, mask, _ = vo.viewshed_mesh(z, 4, 5, 2.5, 5.0)                 # targets raised above the wall's top are all seen
    assert not mask.any()


# ------------------------------------------------------------------ the host side of the public function
def test_argument_errors_come_before_device_work():
    import xrspatial_amd as xs
    good = np.random.default_rng(0).random((6, 7)).astype(np.float32) + 1
    coords = {"y": np.arange(6) * 2.0, "x": np.arange(7) + 10.0}
    with pytest.raises(ValueError, match="method"):
        xs.viewshed(_agg(good, coords=coords), x=12, y=2, method="rtx")
    with pytest.raises(ValueError, match="x argument outside of raster x_range"):
        xs.viewshed(_agg(good, coords=coords), x=9.9, y=2, method="mesh")
    with pytest.raises(ValueError, match="y argument outside of raster y_range"):
        xs.viewshed_mesh(_agg(good, coords=coords), 12, -0.5, 0, 0)
    with pytest.raises(ValueError, match="2-D"):
        xs.viewshed(xs.DataArray(np.ones((2, 3, 4), np.float32), dims=["b", "y", "x"]), x=1, y=0, method="mesh")
    for shape in ((1, 5), (5, 1)):
        with pytest.raises(ValueError, match="two cells"):
            xs.viewshed(_agg(np.ones(shape, np.float64)), x=0, y=0, method="mesh")
    with pytest.raises(ValueError, match="finite"):
        xs.viewshed(_agg(good), x=1, y=1, observer_elev=float("inf"), method="mesh")
    for value in (np.nan, np.inf, -np.inf):
        bad = good.astype(np.float64)
        bad[2, 3] = value
        with pytest.raises(ValueError, match=r"viewshed\(method='mesh'\).*1 non-finite"):
            xs.viewshed(_agg(bad), x=1, y=1, method="mesh")
    with pytest.raises(ValueError, match="positive"):
        xs.viewshed(_agg(-good), x=1, y=1, method="mesh")
    with pytest.raises(ValueError, match="positive"):
        xs.viewshed_mesh(_agg(np.zeros((6, 7), np.int16)), 1, 1, 0, 0)


def test_dask_backed_raster_is_refused(monkeypatch):
    import xrspatial_amd as xs
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.ones((8, 8), np.float32), (4, 4)))
    with pytest.raises(NotImplementedError, match="dask"):
        xs.viewshed(lazy, x=1, y=1, method="mesh")


def test_sweep_and_the_default_take_the_old_path(monkeypatch):
    import xrspatial_amd as xs
    mod = importlib.import_module("xrspatial_amd.viewshed")
    calls = []
    monkeypatch.setattr(mod, "_run", lambda data, *a: calls.append(("sweep",) + a) or np.full(data.shape, -1.0))
    monkeypatch.setattr(mod, "_run_mesh", lambda data, *a: calls.append(("mesh",) + a) or np.full(data.shape, -1.0, np.float32))
    agg = _agg(np.ones((4, 6), np.float32), coords={"y": [40.0, 30.0, 20.0, 10.0], "x": [0.0, 2.5, 5.0, 7.5, 10.0, 12.5]}, attrs={"crs": 3857})
    a = xs.viewshed(agg, x=7.4, y=21, observer_elev=3, target_elev=1.5)
    b = xs.viewshed(agg, 7.4, 21, 3, 1.5, method="sweep")
    c = xs.viewshed(agg, 7.4, 21, 3, 1.5, method="mesh")
    d = xs.viewshed_mesh(agg, 7.4, 21, 3, 1.5)
    args = (2, 3, 3.0, 1.5, 2.5, -10.0)
    assert calls == [("sweep",) + args, ("sweep",) + args, ("mesh",) + args, ("mesh",) + args]
    assert a.data.dtype == b.data.dtype == np.float64 and c.data.dtype == d.data.dtype == np.float32
    for out in (c, d):
        assert out.name == "viewshed" and tuple(out.dims) == ("y", "x") and out.attrs == {"crs": 3857}
        assert np.array_equal(np.asarray(out["y"].data), [40.0, 30.0, 20.0, 10.0]) and np.array_equal(np.asarray(out["x"].data), agg["x"].data)


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xs
    agg = _agg(np.random.default_rng(1).random((5, 6)).astype(np.float32) + 1)
    if xs.has_hip():
        assert xs.viewshed(agg, x=1, y=1, method="mesh").data.dtype == np.float32
        return
    for dt in (np.float32, np.float64, np.int32):
        with pytest.raises(xs.XrsError):
            xs.viewshed(_agg(agg.data.astype(dt) + 1), x=1, y=1, method="mesh")


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_viewshed_mesh_* validate on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    assert lib.xrs_viewshed_mesh_workspace_bytes(300, 400) == lib.xrs_hillshade_shadow_workspace_bytes(300, 400) > 300 * 400 * 4
    assert lib.xrs_viewshed_mesh_workspace_bytes(0, 5) == 0

    def call(fn=lib.xrs_viewshed_mesh_f32, data=fake, rows=4, cols=5, scale=1.0, zmin=0.0, zmax=5.0, vr=1, vc=2, obs=0.0, tgt=0.0, ew=1.0,
             ns=1.0, work=fake, out=fake):
        return fn(data, rows, cols, scale, zmin, zmax, vr, vc, obs, tgt, ew, ns, work, out, None)

    for kw, text in ((dict(rows=1), "2 x 2"), (dict(cols=1), "2 x 2"), (dict(rows=-3), "2 x 2"), (dict(rows=1 << 30), "too large"),
                     (dict(vr=4), "outside"), (dict(vc=-1), "outside"), (dict(data=None), "null"), (dict(work=None), "null"),
                     (dict(out=None), "null"), (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"),
                     (dict(scale=float("inf")), "scale"), (dict(scale=-1.0), "scale"), (dict(zmin=float("nan")), "bounds"),
                     (dict(zmin=6.0), "bounds"), (dict(obs=float("inf")), "finite"), (dict(tgt=float("nan")), "finite"),
                     (dict(ew=float("nan")), "resolutions"), (dict(fn=lib.xrs_viewshed_mesh_f64, vr=9), "outside")):
        assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    probe = lib.xrs_viewshed_mesh_probe_f32
    assert probe(fake, 4, 5, 1.0, 0.0, 5.0, 1, 2, 0.0, 0.0, 1.0, 1.0, 12, fake, fake, None, None) != 0 and "block" in _lib.last_error()
