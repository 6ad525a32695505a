"""The host glue of the whole-raster calls (proximity .. bump), without a device: the C-ABI calls each public function makes, in
order, with their integer and float arguments, and what each function refuses.

A recording stand-in replaces `_lib.call` / `_lib.load` / `_lib.require_device`: `xrs_malloc` hands out zero-filled host memory,
the copies are memmoves, every other entry point is logged and returns without touching its outputs, every `*_workspace_bytes`
answers WORK_BYTES.  Where the zero outputs stop a function early or make it raise, that is the trace.  The pool's own
bookkeeping (POOL_CALLS) is left out: its order depends on what the pool holds.  `python -m tests.test_whole_raster_host` prints
the traces as the literal below."""
import ctypes
import gc
import importlib
import warnings
from collections import OrderedDict

import numpy as np
import pytest

WORK_BYTES = 64
POOL_CALLS = ("xrs_malloc", "xrs_free", "xrs_event_create", "xrs_event_record", "xrs_event_sync")
_FLOATS = (ctypes.c_float, ctypes.c_double)
_SCALARS = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_float, ctypes.c_double)


class Recorder:
    """`_lib.call` and the object `_lib.load()` returns, in one."""

    def __init__(self, prototypes):
        self.prototypes = prototypes
        self.trace = []
        self.live = {}

    def _log(self, name, args):
        if name not in POOL_CALLS:
            kinds = self.prototypes[name]
            assert len(kinds) == len(args), (name, len(args))
            self.trace.append((name,) + tuple((float if k in _FLOATS else int)(a) for a, k in zip(args, kinds) if k in _SCALARS))

    def call(self, name, *args):
        self._log(name, args)
        if name == "xrs_malloc":
            buf = ctypes.create_string_buffer(int(args[1]) + 64)
            addr = (ctypes.addressof(buf) + 63) // 64 * 64
            self.live[addr] = buf
            args[0]._obj.value = addr
        elif name in ("xrs_memcpy_h2d", "xrs_memcpy_d2h", "xrs_memcpy_d2d"):
            ctypes.memmove(int(args[0]), int(args[1]), int(args[2]))
        elif name in ("xrs_event_create", "xrs_stream_create"):
            args[0]._obj.value = 1
        return 0

    def __getattr__(self, name):
        if not name.startswith("xrs_"):
            raise AttributeError(name)

        def entry(*args):
            self._log(name, args)
            if name == "xrs_free":
                self.live.pop(int(args[0]), None)
            return WORK_BYTES if name.endswith("_workspace_bytes") else 0
        return entry


def _install(monkeypatch):
    """The recorder in place of the library, an empty device pool and an empty table cache in place of the process's."""
    from xrspatial_amd import _lib, device
    perlin = importlib.import_module("xrspatial_amd.perlin")           # (the package's `perlin` is the function)
    rec = Recorder(_lib._PROTOTYPES)
    monkeypatch.setattr(_lib, "call", rec.call)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    monkeypatch.setattr(device, "_pool", {})
    monkeypatch.setattr(device, "_pool_bytes", 0)
    monkeypatch.setattr(device, "_spare_events", [])
    monkeypatch.setattr(perlin, "_tables", OrderedDict())
    monkeypatch.setattr(perlin, "host_table", lambda seed: np.zeros(perlin.TABLE_SIZE, np.int32))   # (0.13 s each, 16 per terrain)
    return rec


@pytest.fixture
def rec(monkeypatch):
    rec = _install(monkeypatch)
    yield rec
    gc.collect()                                     # every stand-in block is back in the stand-in pool before the real one returns


# ------------------------------------------------------------------ the inputs: 4 x 5
Z = (np.arange(20).reshape(4, 5) * 7 % 5 + 1)       # 1 .. 5: finite, positive maximum, some cells equal
XS, YS = np.arange(5, dtype=np.float64), np.arange(4, dtype=np.float64)


def _back(values, backend):
    from xrspatial_amd import DeviceArray
    values = np.ascontiguousarray(values)
    return DeviceArray.from_numpy(values) if backend == "device" else values


def _agg(values, backend="numpy", **kw):
    import xrspatial_amd as xa
    return xa.DataArray(_back(values, backend) if isinstance(values, np.ndarray) else values, dims=["y", "x"],
                        coords={"y": YS[:values.shape[0]], "x": XS[:values.shape[1]]}, attrs={"res": (1.0, 1.0)}, **kw)


def _ds(backend, mixed=False):
    import xrspatial_amd as xa
    zf = Z.astype(np.float32)
    planes = {"a": _back(zf, backend), "b": _back(zf[::-1], "numpy" if mixed else backend), "c": _back(zf.T.reshape(4, 5), backend),
              "r": _back((Z % 3 + 1).astype(np.int32), backend)}
    return xa.Dataset({k: xa.DataArray(v, dims=["y", "x"]) for k, v in planes.items()})


def _cases():
    """name -> f(backend): one public call each"""
    import xrspatial_amd as xa
    from xrspatial_amd.experimental import polygonize
    cases = {}
    for dt in ("float32", "int16", "bool", "float16"):
        cases[f"proximity-{dt}"] = lambda b, dt=dt: xa.proximity(_agg((Z % 3).astype(dt), b))
        cases[f"a_star_search-{dt}"] = lambda b, dt=dt: xa.a_star_search(_agg(Z.astype(dt), b), (0.0, 0.0), (3.0, 4.0), barriers=[2],
                                                                        snap_start=True)
    cases["allocation-float32"] = lambda b: xa.allocation(_agg((Z % 3).astype(np.float32), b), target_values=[1, 2], max_distance=3)
    cases["direction-float32"] = lambda b: xa.direction(_agg((Z % 3).astype(np.float32), b), distance_metric="GREAT_CIRCLE")
    for dt in ("float32", "int32"):
        cases[f"viewshed-{dt}"] = lambda b, dt=dt: xa.viewshed(_agg(Z.astype(dt), b), 2.0, 1.0, observer_elev=3)
        cases[f"viewshed_mesh-{dt}"] = lambda b, dt=dt: xa.viewshed(_agg(Z.astype(dt), b), 2.0, 1.0, observer_elev=3, method="mesh")
        cases[f"hillshade_shadows-{dt}"] = lambda b, dt=dt: xa.hillshade(_agg(Z.astype(dt), b), shadows=True)
        cases[f"flow_direction-{dt}"] = lambda b, dt=dt: xa.flow_direction(_agg(Z.astype(dt), b))
        cases[f"flow_accumulation-{dt}"] = lambda b, dt=dt: xa.flow_accumulation(_agg(np.zeros((4, 5), dt), b))
    cases["basins-float32"] = lambda b: xa.basins(_agg(np.zeros((4, 5), np.float32), b))
    cases["regions-uint8"] = lambda b: xa.zonal.regions(_agg(Z.astype(np.uint8), b), neighborhood=8)
    cases["polygonize-uint8"] = lambda b: polygonize(_agg(Z.astype(np.uint8), b))
    cases["polygonize-uint8-mask"] = lambda b: polygonize(_agg(Z.astype(np.uint8), b), mask=_agg(Z > 2, b), connectivity=8,
                                                         return_type="flat")
    cases["cell_stats"] = lambda b: xa.local.cell_stats(_ds(b), ["a", "b", "c"], func="mean")
    cases["cell_stats-mixed"] = lambda b: xa.local.cell_stats(_ds(b, mixed=True), ["a", "b", "c"])
    cases["combine"] = lambda b: xa.local.combine(_ds(b), ["a", "r"])
    for name in ("lesser_frequency", "equal_frequency", "greater_frequency", "popularity", "rank"):
        cases[name] = lambda b, name=name: getattr(xa.local, name)(_ds(b), "r")
    for name in ("lowest_position", "highest_position"):
        cases[name] = lambda b, name=name: getattr(xa.local, name)(_ds(b), ["a", "b"])
    cases["perlin"] = lambda b: xa.perlin(_agg(np.zeros((4, 5), np.float32), b), freq=(2, 3), seed=7)
    cases["generate_terrain"] = lambda b: xa.generate_terrain(_agg(np.zeros((4, 5), np.float64), b), seed=3, zfactor=100)
    cases["natural_breaks"] = lambda b: xa.natural_breaks(_agg(Z.astype(np.float32), b), k=3)
    cases["bump"] = lambda b: xa.bump(5, 4, count=2, spread=2)
    return cases


def _trace(rec, case, backend):
    """The calls of one case, the uploads that build its DeviceArray inputs first; an exception is the trace's last entry."""
    state = np.random.get_state()
    from xrspatial_amd import device
    importlib.import_module("xrspatial_amd.perlin").clear_table_cache()
    gc.collect()
    device._pool.clear()                             # (the stand-in pool: a recycled block is not zero-filled)
    device._pool_bytes = 0
    rec.trace.clear()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _cases()[case](backend)
    except Exception as e:                           # noqa: BLE001
        rec.trace.append(("raises", type(e).__name__, str(e)))
    finally:
        np.random.set_state(state)
    return list(rec.trace)


# EXPECTED-BEGIN
inf = float("inf")
EXPECTED = {
    'proximity-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 9, 4, 5, 0, 0, inf, 0, 0), ('xrs_memcpy_d2h', 80),
        ('xrs_stream_sync',)],
    'proximity-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 9, 4, 5, 0, 0, inf, 0, 0), ('xrs_stream_sync',)],
    'a_star_search-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8),
        ('xrs_stream_sync',), ('xrs_astar', 9, 4, 5, 0, 0, 3, 4, 0, 1, 8, 1), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'a_star_search-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8),
        ('xrs_stream_sync',), ('xrs_astar', 9, 4, 5, 0, 0, 3, 4, 0, 1, 8, 1)],
    'proximity-int16/numpy': [
        ('xrs_memcpy_h2d', 40), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 2, 4, 5, 0, 0, inf, 0, 0), ('xrs_memcpy_d2h', 80),
        ('xrs_stream_sync',)],
    'proximity-int16/device': [
        ('xrs_memcpy_h2d', 40), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 2, 4, 5, 0, 0, inf, 0, 0), ('xrs_stream_sync',)],
    'a_star_search-int16/numpy': [
        ('xrs_memcpy_h2d', 40), ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8),
        ('xrs_stream_sync',), ('xrs_astar', 2, 4, 5, 0, 0, 3, 4, 1, 1, 8, 1), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'a_star_search-int16/device': [
        ('xrs_memcpy_h2d', 40), ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8),
        ('xrs_stream_sync',), ('xrs_astar', 2, 4, 5, 0, 0, 3, 4, 1, 1, 8, 1)],
    'proximity-bool/numpy': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 1, 4, 5, 0, 0, inf, 0, 0), ('xrs_memcpy_d2h', 80),
        ('xrs_stream_sync',)],
    'proximity-bool/device': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 20), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 20),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',), ('xrs_proximity_workspace_bytes', 4, 5),
        ('xrs_proximity', 1, 4, 5, 0, 0, inf, 0, 0), ('xrs_stream_sync',)],
    'a_star_search-bool/numpy': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8),
        ('xrs_stream_sync',), ('xrs_astar', 1, 4, 5, 0, 0, 3, 4, 1, 1, 8, 1), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'a_star_search-bool/device': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 20), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 20),
        ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8), ('xrs_stream_sync',),
        ('xrs_astar', 1, 4, 5, 0, 0, 3, 4, 1, 1, 8, 1)],
    'proximity-float16/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 9, 4, 5, 0, 0, inf, 0, 0), ('xrs_memcpy_d2h', 80),
        ('xrs_stream_sync',)],
    'proximity-float16/device': [
        ('xrs_memcpy_h2d', 40), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 40), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 72), ('xrs_stream_sync',), ('xrs_proximity_workspace_bytes', 4, 5),
        ('xrs_proximity', 9, 4, 5, 0, 0, inf, 0, 0), ('xrs_stream_sync',)],
    'a_star_search-float16/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8),
        ('xrs_stream_sync',), ('xrs_astar', 9, 4, 5, 0, 0, 3, 4, 0, 1, 8, 1), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'a_star_search-float16/device': [
        ('xrs_memcpy_h2d', 40), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 40), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_astar_workspace_bytes', 4, 5), ('xrs_memcpy_h2d', 8), ('xrs_stream_sync',),
        ('xrs_astar', 9, 4, 5, 0, 0, 3, 4, 0, 1, 8, 1)],
    'allocation-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 88), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 9, 4, 5, 0, 2, 3.0, 0, 1), ('xrs_memcpy_d2h', 80),
        ('xrs_stream_sync',)],
    'allocation-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 88), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 9, 4, 5, 0, 2, 3.0, 0, 1), ('xrs_stream_sync',)],
    'direction-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 176), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 9, 4, 5, 0, 0, inf, 1, 2), ('xrs_memcpy_d2h', 80),
        ('xrs_stream_sync',)],
    'direction-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 176), ('xrs_stream_sync',),
        ('xrs_proximity_workspace_bytes', 4, 5), ('xrs_proximity', 9, 4, 5, 0, 0, inf, 1, 2), ('xrs_stream_sync',)],
    'viewshed-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_viewshed_workspace_bytes', 4, 5),
        ('xrs_viewshed_f32', 4, 5, 1, 2, 3.0, 0.0, 1.0, 1.0), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'viewshed-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_viewshed_workspace_bytes', 4, 5),
        ('xrs_viewshed_f32', 4, 5, 1, 2, 3.0, 0.0, 1.0, 1.0), ('xrs_stream_sync',)],
    'viewshed_mesh-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_viewshed_mesh_workspace_bytes', 4, 5),
        ('xrs_viewshed_mesh_f32', 4, 5, 1.0, 1.0, 5.0, 1, 2, 3.0, 0.0, 1.0, 1.0), ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',)],
    'viewshed_mesh-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_classify_workspace_bytes', 1, 0),
        ('xrs_classify_finite_stats_f32', 20), ('xrs_memcpy_d2h', 32), ('xrs_stream_sync',),
        ('raises', 'ValueError', "viewshed(method='mesh'): the raster holds 20 non-finite cells")],
    'hillshade_shadows-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_hillshade_shadow_workspace_bytes', 4, 5),
        ('xrs_hillshade_shadow_f32', 4, 5, 1.0, 1.0, 5.0, -0.6408563820557884, 0.6408563820557887, 0.42261826174069944, 1),
        ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',)],
    'hillshade_shadows-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_classify_workspace_bytes', 1, 0),
        ('xrs_classify_finite_stats_f32', 20), ('xrs_memcpy_d2h', 32), ('xrs_stream_sync',),
        ('raises', 'ValueError', 'hillshade(shadows=True): the raster holds 20 non-finite cells')],
    'flow_direction-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_flow_direction', 9, 4, 5, 1.0, 1.0, 1.4142135623730951),
        ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',)],
    'flow_direction-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_flow_direction', 9, 4, 5, 1.0, 1.0, 1.4142135623730951)],
    'flow_accumulation-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_flow_workspace_bytes', 4, 5, 1), ('xrs_flow_accumulate', 4, 5, 0),
        ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'flow_accumulation-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_flow_workspace_bytes', 4, 5, 1), ('xrs_flow_accumulate', 4, 5, 0),
        ('xrs_stream_sync',)],
    'viewshed-int32/numpy': [
        ('xrs_memcpy_h2d', 160), ('xrs_stream_sync',), ('xrs_viewshed_workspace_bytes', 4, 5),
        ('xrs_viewshed_f64', 4, 5, 1, 2, 3.0, 0.0, 1.0, 1.0), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'viewshed-int32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 160),
        ('xrs_stream_sync',), ('xrs_viewshed_workspace_bytes', 4, 5), ('xrs_viewshed_f64', 4, 5, 1, 2, 3.0, 0.0, 1.0, 1.0),
        ('xrs_stream_sync',)],
    'viewshed_mesh-int32/numpy': [
        ('xrs_memcpy_h2d', 160), ('xrs_stream_sync',), ('xrs_viewshed_mesh_workspace_bytes', 4, 5),
        ('xrs_viewshed_mesh_f64', 4, 5, 1.0, 1.0, 5.0, 1, 2, 3.0, 0.0, 1.0, 1.0), ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',)],
    'viewshed_mesh-int32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 160),
        ('xrs_stream_sync',), ('xrs_classify_workspace_bytes', 1, 1), ('xrs_classify_finite_stats_f64', 20),
        ('xrs_memcpy_d2h', 32), ('xrs_stream_sync',),
        ('raises', 'ValueError', "viewshed(method='mesh'): the raster holds 20 non-finite cells")],
    'hillshade_shadows-int32/numpy': [
        ('xrs_memcpy_h2d', 160), ('xrs_stream_sync',), ('xrs_hillshade_shadow_workspace_bytes', 4, 5),
        ('xrs_hillshade_shadow_f64', 4, 5, 1.0, 1.0, 5.0, -0.6408563820557884, 0.6408563820557887, 0.42261826174069944, 1),
        ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',)],
    'hillshade_shadows-int32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 160),
        ('xrs_stream_sync',), ('xrs_classify_workspace_bytes', 1, 1), ('xrs_classify_finite_stats_f64', 20),
        ('xrs_memcpy_d2h', 32), ('xrs_stream_sync',),
        ('raises', 'ValueError', 'hillshade(shadows=True): the raster holds 20 non-finite cells')],
    'flow_direction-int32/numpy': [
        ('xrs_memcpy_h2d', 160), ('xrs_stream_sync',), ('xrs_flow_direction', 8, 4, 5, 1.0, 1.0, 1.4142135623730951),
        ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',)],
    'flow_direction-int32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 160),
        ('xrs_stream_sync',), ('xrs_flow_direction', 8, 4, 5, 1.0, 1.0, 1.4142135623730951), ('xrs_stream_sync',)],
    'flow_accumulation-int32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_cast_f32', 4, 20), ('xrs_stream_sync',),
        ('xrs_flow_workspace_bytes', 4, 5, 1), ('xrs_flow_accumulate', 4, 5, 0), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160),
        ('xrs_stream_sync',)],
    'flow_accumulation-int32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_cast_f32', 4, 20), ('xrs_flow_workspace_bytes', 4, 5, 1),
        ('xrs_flow_accumulate', 4, 5, 0), ('xrs_stream_sync',)],
    'basins-float32/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_flow_workspace_bytes', 4, 5, 2), ('xrs_flow_accumulate', 4, 5, 0),
        ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'basins-float32/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_flow_workspace_bytes', 4, 5, 2), ('xrs_flow_accumulate', 4, 5, 0),
        ('xrs_stream_sync',)],
    'regions-uint8/numpy': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_regions_workspace_bytes', 4, 5), ('xrs_regions_link', 1, 4, 5, 8),
        ('xrs_regions_label', 1, 4, 5, 8), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 20), ('xrs_stream_sync',)],
    'regions-uint8/device': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_regions_workspace_bytes', 4, 5), ('xrs_regions_link', 1, 4, 5, 8),
        ('xrs_regions_label', 1, 4, 5, 8), ('xrs_stream_sync',)],
    'polygonize-uint8/numpy': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_polygonize_workspace_bytes', 4, 5),
        ('xrs_polygonize_census', 1, 0, 4, 5, 4)],
    'polygonize-uint8/device': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_polygonize_workspace_bytes', 4, 5),
        ('xrs_polygonize_census', 1, 0, 4, 5, 4)],
    'polygonize-uint8-mask/numpy': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',),
        ('xrs_polygonize_workspace_bytes', 4, 5), ('xrs_polygonize_census', 1, 1, 4, 5, 8)],
    'polygonize-uint8-mask/device': [
        ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 20), ('xrs_stream_sync',),
        ('xrs_polygonize_workspace_bytes', 4, 5), ('xrs_polygonize_census', 1, 1, 4, 5, 8)],
    'cell_stats/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_local_cells', 3, 3, 0, 20, 0), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160),
        ('xrs_stream_sync',)],
    'cell_stats/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 3, 3, 0, 20, 0)],
    'cell_stats-mixed/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_local_cells', 2, 3, 0, 20, 0), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160),
        ('xrs_stream_sync',)],
    'cell_stats-mixed/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 2, 3, 0, 20, 0),
        ('xrs_stream_sync',)],
    'combine/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',),
        ('xrs_local_combine_workspace_bytes', 20, 2), ('xrs_local_combine', 2, 20, 64, 0), ('xrs_stream_sync',),
        ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'combine/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_combine_workspace_bytes', 20, 2),
        ('xrs_local_combine', 2, 20, 64, 0), ('xrs_stream_sync',)],
    'lesser_frequency/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 6, 3, 4, 20, 0),
        ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'lesser_frequency/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 6, 3, 4, 20, 0)],
    'equal_frequency/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 7, 3, 4, 20, 0),
        ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'equal_frequency/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 7, 3, 4, 20, 0)],
    'greater_frequency/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 8, 3, 4, 20, 0),
        ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'greater_frequency/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 8, 3, 4, 20, 0)],
    'popularity/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 12, 3, 4, 20, 0),
        ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'popularity/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 12, 3, 4, 20, 0)],
    'rank/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 11, 3, 4, 20, 0),
        ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'rank/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 11, 3, 4, 20, 0)],
    'lowest_position/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',),
        ('xrs_local_cells', 9, 2, 0, 20, 0), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'lowest_position/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 9, 2, 0, 20, 0)],
    'highest_position/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',),
        ('xrs_local_cells', 10, 2, 0, 20, 0), ('xrs_stream_sync',), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'highest_position/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80),
        ('xrs_stream_sync',), ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_local_cells', 10, 2, 0, 20, 0)],
    'perlin/numpy': [
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_noise_raw_f32', 4, 5, 0, 4, 0.0, 2.0, 0.0, 3.0, 1, 0),
        ('xrs_memcpy_d2h', 16), ('xrs_stream_sync',), ('xrs_noise_finish_f32', 20, 0.0, 0.0, 0, 0.0, 0, 1.0),
        ('xrs_memcpy_d2h', 80), ('xrs_stream_sync',)],
    'perlin/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_noise_raw_f32', 4, 5, 0, 4, 0.0, 2.0, 0.0, 3.0, 1, 0), ('xrs_memcpy_d2h', 16), ('xrs_stream_sync',),
        ('xrs_noise_finish_f32', 20, 0.0, 0.0, 0, 0.0, 0, 1.0)],
    'generate_terrain/numpy': [
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_noise_raw_f64', 4, 5, 0, 4, 0.0, 1.0, 0.0, 1.0, 16, 1), ('xrs_memcpy_d2h', 16), ('xrs_stream_sync',),
        ('xrs_noise_finish_f64', 20, 0.0, 0.0, 1, 0.3, 1, 100.0), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'generate_terrain/device': [
        ('xrs_memcpy_h2d', 160), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',),
        ('xrs_memcpy_h2d', 4194304), ('xrs_stream_sync',), ('xrs_noise_raw_f64', 4, 5, 0, 4, 0.0, 1.0, 0.0, 1.0, 16, 1),
        ('xrs_memcpy_d2h', 16), ('xrs_stream_sync',), ('xrs_noise_finish_f64', 20, 0.0, 0.0, 1, 0.3, 1, 100.0)],
    'natural_breaks/numpy': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_classify_workspace_bytes', 1, 0),
        ('xrs_classify_finite_stats_f32', 20), ('xrs_memcpy_d2h', 32), ('xrs_stream_sync',),
        ('raises', 'ValueError', 'zero-size array to reduction operation maximum which has no identity')],
    'natural_breaks/device': [
        ('xrs_memcpy_h2d', 80), ('xrs_stream_sync',), ('xrs_classify_workspace_bytes', 1, 0),
        ('xrs_classify_finite_stats_f32', 20), ('xrs_memcpy_d2h', 32), ('xrs_stream_sync',),
        ('raises', 'ValueError', 'zero-size array to reduction operation maximum which has no identity')],
    'bump/numpy': [
        ('xrs_bump_workspace_bytes', 2, 5, 4, 2, 134217728), ('xrs_memcpy_h2d', 8), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 16),
        ('xrs_stream_sync',), ('xrs_bump_f64', 2, 5, 4, 2, 64, 134217728), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
    'bump/device': [
        ('xrs_bump_workspace_bytes', 2, 5, 4, 2, 134217728), ('xrs_memcpy_h2d', 8), ('xrs_stream_sync',), ('xrs_memcpy_h2d', 16),
        ('xrs_stream_sync',), ('xrs_bump_f64', 2, 5, 4, 2, 64, 134217728), ('xrs_memcpy_d2h', 160), ('xrs_stream_sync',)],
}
# EXPECTED-END


def test_every_case_has_a_recorded_trace():
    assert sorted(EXPECTED) == sorted(f"{c}/{b}" for c in _cases() for b in ("numpy", "device"))


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_the_call_sequence_is_the_recorded_one(rec, key):
    case, backend = key.split("/")
    assert _trace(rec, case, backend) == EXPECTED[key]


# ------------------------------------------------------------------ refusals: the texts, and where they stand among the checks
def _lazy(values, monkeypatch):
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    values = np.asarray(values)
    return fake_dask.from_array(values, tuple(max(n // 2, 1) for n in values.shape))


def _shard(values):
    import xrspatial_amd as xa
    shard = object.__new__(xa.ShardedArray)          # (its constructor wants a device; the refusals do not)
    shard.local = np.asarray(values)
    return shard


def _plain(what, suffix_sharded="", suffix_dask=""):
    return (f"{what}() does not support row-sharded (multi-GPU) DataArray" + suffix_sharded,
            f"{what}() does not support dask backed DataArray" + suffix_dask)


def _split_ds(data):
    import xrspatial_amd as xa
    zf = Z.astype(np.float32)
    return xa.Dataset({"a": xa.DataArray(zf, dims=["y", "x"]), "b": xa.DataArray(data, dims=["y", "x"]),
                       "r": xa.DataArray(Z.astype(np.int32), dims=["y", "x"])})


def _refusing():
    """name -> (f(data), (ShardedArray text, dask text)), `data` a 4 x 5 float32 raster of a split backend"""
    import xrspatial_amd as xa
    out = {name: (lambda d, name=name: getattr(xa, name)(_agg(d)), _plain(name))
           for name in ("proximity", "allocation", "direction", "flow_direction", "flow_accumulation", "basins", "perlin",
                        "generate_terrain")}
    out["a_star_search"] = (lambda d: xa.a_star_search(_agg(d), (0.0, 0.0), (3.0, 4.0)), _plain("a_star_search"))
    out["viewshed"] = (lambda d: xa.viewshed(_agg(d), 2.0, 1.0), _plain("viewshed"))
    out["viewshed_mesh"] = (lambda d: xa.viewshed(_agg(d), 2.0, 1.0, method="mesh"), _plain("viewshed"))
    out["hillshade_shadows"] = (lambda d: xa.hillshade(_agg(d), shadows=True),
                                ("hillshade(shadows=True) does not support row-sharded (multi-GPU) DataArray: rays cross shards",
                                 "hillshade(shadows=True) does not support dask backed DataArray: rays cross chunks"))
    out["regions"] = (lambda d: xa.zonal.regions(_agg(d)),
                      ("zonal.regions of a row-sharded (multi-GPU) raster: merging regions across shards is not implemented; "
                       "gather the raster on one GPU",
                       "zonal.regions of a dask-backed raster: the reference has no dask path either; compute the raster first"))
    out["natural_breaks"] = (lambda d: xa.natural_breaks(_agg(d)),
                             ("not implemented for row-sharded (multi-GPU) arrays", "not implemented for dask-backed arrays"))
    for name in ("cell_stats", "combine", "lowest_position", "highest_position"):
        out[name] = (lambda d, name=name: getattr(xa.local, name)(_split_ds(d)), _plain(name))
    for name in ("lesser_frequency", "equal_frequency", "greater_frequency", "popularity", "rank"):
        out[name] = (lambda d, name=name: getattr(xa.local, name)(_split_ds(d), "r"), _plain(name))
    return out


REFUSING = ("proximity", "allocation", "direction", "flow_direction", "flow_accumulation", "basins", "perlin", "generate_terrain",
            "a_star_search", "viewshed", "viewshed_mesh", "hillshade_shadows", "regions", "natural_breaks", "cell_stats", "combine",
            "lowest_position", "highest_position", "lesser_frequency", "equal_frequency", "greater_frequency", "popularity", "rank")


@pytest.mark.parametrize("name", REFUSING)
def test_split_backends_are_refused_in_these_words(monkeypatch, name):
    assert sorted(REFUSING) == sorted(_refusing())
    call, (sharded_text, dask_text) = _refusing()[name]
    zf = Z.astype(np.float32)
    with pytest.raises(NotImplementedError) as e:
        call(_shard(zf))
    assert str(e.value) == sharded_text
    with pytest.raises(NotImplementedError) as e:
        call(_lazy(zf, monkeypatch))
    assert str(e.value) == dask_text


def test_polygonize_names_the_type_it_refuses(monkeypatch):
    from xrspatial_amd.experimental import polygonize
    from tests import fake_dask
    for data in (_shard(Z.astype(np.uint8)), _lazy(Z.astype(np.uint8), monkeypatch)):
        with pytest.raises(TypeError) as e:
            polygonize(_agg(data))
        assert str(e.value) == f"Unsupported array type: {type(data)}"
    assert type(data) is fake_dask.Array


def test_where_the_refusal_stands_among_the_checks(monkeypatch):
    """A split-backend raster that also fails another check: which of the two errors the caller sees."""
    import xrspatial_amd as xa
    from xrspatial_amd.experimental import polygonize
    zf = Z.astype(np.float32)
    lazy, lazy3 = _lazy(zf, monkeypatch), _lazy(np.zeros((2, 4, 5), np.float32), monkeypatch)
    wrong_dims = xa.DataArray(lazy, dims=["lat", "lon"], coords={"lat": YS, "lon": XS})
    cube = xa.DataArray(lazy3, dims=["b", "y", "x"])
    refused, checked = pytest.raises(NotImplementedError), pytest.raises(ValueError)
    # the refusal first
    for fn in (xa.proximity, xa.allocation, xa.direction):
        with refused:
            fn(wrong_dims)                                               # (before "raster.coords should be named ...")
    for fn in (xa.flow_direction, xa.flow_accumulation, xa.basins, xa.zonal.regions):
        with refused:
            fn(cube)                                                     # (before "expected a 2D raster")
    with refused:
        xa.a_star_search(_agg(lazy), (9.0, 9.0), (3.0, 4.0))             # (before "start location outside ...")
    with refused:
        xa.hillshade(_agg(lazy), azimuth=np.nan, shadows=True)           # (before "azimuth and angle_altitude must be finite")
    with refused:
        xa.local.cell_stats(_split_ds(_lazy(np.zeros((3, 3), np.float32), monkeypatch)))      # (before the shape check)
    with refused:
        xa.local.rank(xa.Dataset({"r": xa.DataArray(lazy, dims=["y", "x"])}), "r")           # (before "no data variables")
    # the other check first
    with checked:
        xa.a_star_search(_agg(lazy), (0.0, 0.0), (3.0, 4.0), connectivity=5)
    with checked:
        xa.a_star_search(wrong_dims, (0.0, 0.0), (3.0, 4.0))
    for method in ("sweep", "mesh"):
        with checked:
            xa.viewshed(_agg(lazy), 99.0, 1.0, method=method)            # ("x argument outside of raster x_range")
        with checked:
            xa.viewshed(_agg(lazy), 2.0, 1.0, observer_elev=np.inf, method=method)
    with checked:
        xa.hillshade(cube, shadows=True)
    with checked:
        xa.zonal.regions(_agg(lazy), neighborhood=5)
    with checked:
        xa.local.cell_stats(_split_ds(lazy), func="mode")
    with checked:
        xa.local.rank(_split_ds(lazy), "r", ["r"])                       # ("ref_var must not be an element of data_vars")
    with checked:
        xa.perlin(_agg(lazy), freq=(1, 2, 3))
    with checked:
        xa.perlin(_agg(_lazy(Z.astype(np.int32), monkeypatch)))          # ("float32 or float64 data is needed")
    with checked:
        xa.generate_terrain(_agg(lazy), full_extent=(0, 0, 0, 500))      # ("the full extent is empty")
    with checked:
        polygonize(_agg(lazy), connectivity=5)
    with pytest.raises(TypeError):
        polygonize(_agg(lazy), return_type="wkt")                        # (the type is refused before the return type is read)


# ------------------------------------------------------------------ the ABI table
def test_workspace_sizes_and_nothing_else_return_size_t(monkeypatch):
    """`load()` on a stand-in for the shared object: every prototype gets its argtypes, the `*_workspace_bytes` names return
    size_t (an int would truncate them without an error), every other name int."""
    from types import SimpleNamespace
    from xrspatial_amd import _lib

    class Library:
        def __init__(self, path):
            self.entries = {}

        def __getattr__(self, name):
            return self.__dict__["entries"].setdefault(name, SimpleNamespace())

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", __file__)
    monkeypatch.setattr(_lib.ctypes, "CDLL", Library)
    entries = _lib.load().entries
    assert sorted(entries) == sorted(_lib._PROTOTYPES)
    sizes = sorted(name for name, fn in entries.items() if fn.restype is ctypes.c_size_t)
    assert sizes == sorted(name for name in _lib._PROTOTYPES if name.endswith("_workspace_bytes")) and len(sizes) == 18
    assert all(fn.restype is ctypes.c_int for name, fn in entries.items() if name not in sizes)
    assert all(entries[name].argtypes == argtypes for name, argtypes in _lib._PROTOTYPES.items())


if __name__ == "__main__":
    with pytest.MonkeyPatch.context() as mp:
        recorder = _install(mp)
        traces = {f"{c}/{b}": _trace(recorder, c, b) for c in _cases() for b in ("numpy", "device")}
        gc.collect()
    print("EXPECTED = {")
    for key, trace in traces.items():
        lines = [[]]
        for entry in trace:
            if lines[-1] and sum(len(e) + 2 for e in lines[-1]) + len(repr(entry)) > 120:
                lines.append([])
            lines[-1].append(repr(entry))
        print(f"    {key!r}: [\n" + ",\n".join(" " * 8 + ", ".join(ln) for ln in lines) + "],")
    print("}")
