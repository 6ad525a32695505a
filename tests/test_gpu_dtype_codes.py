"""The XRS_DT_* code of every C-ABI entry point that takes a raster in its own dtype as (const void *, int dtype) -- called
through `_lib`, never through a function of the package.

Two things per entry point, from one table (ENTRIES):
  * refusals: the codes -1 and 10 and every code the entry has no kernel for give a non-zero return and exactly the text
    below in xrs_last_error().  The texts were recorded from the library before its dispatch was gathered into
    csrc/dtype_dispatch.h and are literals here (with the code as %d);
  * every accepted code: one call on the values 0 .. 14 as a 3 x 5 raster of that dtype (8 x 8 for xrs_fill / xrs_flow_flats,
    which treat anything narrower than 3 as all rim) gives, bit for bit, what the same call gives on the same values as float64
    (float32 where the entry has no float64 kernel).  Every dtype holds these values exactly, so the reference is the library's
    own float path.  A result that has the raster's dtype (xrs_regions_label, the polygonize column, xrs_fill) is compared
    after `astype(float64)`, which is exact for these values.
A runner hands `code` to the entry under test only; the calls that prepare its input get the true code of the raster."""
import ctypes

import numpy as np
import pytest

import xrspatial_amd as xs
from xrspatial_amd import _lib
from xrspatial_amd._launch import get_stream, workspace
from xrspatial_amd.device import DTYPE_CODE

pytestmark = pytest.mark.gpu

ALL = [np.dtype(t) for t in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float64,
                             np.float32)]                                # in the order of their codes 0 .. 9
F32, F64, U64, I32 = (DTYPE_CODE[np.dtype(t)] for t in (np.float32, np.float64, np.uint64, np.int32))
VALUES = np.arange(15).reshape(3, 5)
FILL_VALUES = ((np.arange(64) * 27) % 64).reshape(8, 8)                  # a permutation of 0 .. 63: pits away from the rim
FLAT_VALUES = np.repeat(np.arange(4), 16).reshape(8, 8)                  # terraces two rows deep: cells without a lower neighbour
VALUES_F64 = 0                                                           # XRS_PROX_VALUES_F64
LOCAL_MAX, LOCAL_SUM, LOCAL_LESSER = 0, 2, 6                             # XRS_LOCAL_*
FILL_STATUS_WORDS = 256                                                  # XRS_FILL_STATUS_WORDS


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def _up(a):
    return xs.DeviceArray.from_numpy(np.ascontiguousarray(a), stream=get_stream())


def _true(z):
    return DTYPE_CODE[z.dtype]


# ------------------------------------------------------------------ one runner per entry point: (raster, code) -> host arrays
def cast_f32(z, code):
    src, out = _up(z), xs.DeviceArray(z.shape, np.float32)
    _lib.call("xrs_cast_f32", src.ptr, code, out.ptr, z.size, get_stream())
    return [out.get(get_stream())]


def classify_to_f64(z, code):
    src, out = _up(z), xs.DeviceArray(z.shape, np.float64)
    _lib.call("xrs_classify_to_f64", src.ptr, code, out.ptr, z.size, get_stream())
    return [out.get(get_stream())]


def true_color_u8(z, code):
    band, raw = _up(z.astype(np.float32)), _up(z)
    minmax, out = _up(np.array([0, 14] * 3, np.float32)), xs.DeviceArray((z.size, 4), np.uint8)
    _lib.call("xrs_true_color_u8", band.ptr, band.ptr, band.ptr, raw.ptr, code, z.size, minmax.ptr, 3.0, 10.0, 0.5, out.ptr,
              get_stream())                                              # nodata 3: alpha 0 at the cells 0 .. 3
    return [out.get(get_stream())]


def match_bbox(z, code):
    src, box = _up(z), xs.DeviceArray((4,), np.int32)
    wanted = np.array([6.0, 7.0, 13.0])
    _lib.call("xrs_match_bbox", src.ptr, code, z.shape[0], z.shape[1], z.shape[1], wanted.ctypes.data, wanted.size, 0, box.ptr,
              get_stream())
    return [box.get(get_stream())]


def regions_link(z, code):
    src, work, n_new = _up(z), workspace("regions", *z.shape), ctypes.c_uint64(0)
    _lib.call("xrs_regions_link", src.ptr, code, z.shape[0], z.shape[1], 8, work.ptr, ctypes.byref(n_new), get_stream())
    return [np.array([n_new.value])]


def regions_label(z, code):
    src, work, n_new = _up(z), workspace("regions", *z.shape), ctypes.c_uint64(0)
    out = xs.DeviceArray(z.shape, z.dtype)
    _lib.call("xrs_regions_link", src.ptr, _true(z), z.shape[0], z.shape[1], 8, work.ptr, ctypes.byref(n_new), get_stream())
    _lib.call("xrs_regions_label", src.ptr, code, z.shape[0], z.shape[1], 8, work.ptr, out.ptr, get_stream())
    return [out.get(get_stream()).astype(np.float64)]


def _census(z, code, mask=None, mask_code=0):
    src, work = _up(z), workspace("polygonize", *z.shape)
    mdev = _up(mask) if mask is not None else None
    n_regions, n_states = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.call("xrs_polygonize_census", src.ptr, code, mdev.ptr if mdev is not None else None, mask_code, z.shape[0], z.shape[1], 4,
              work.ptr, ctypes.byref(n_regions), ctypes.byref(n_states), get_stream())
    region = xs.DeviceArray(z.shape, np.uint32, _ptr=work.ptr, _base=work).get(get_stream())   # the region plane (ABI)
    return src, work, int(n_regions.value), int(n_states.value), region


def polygonize_census(z, code):
    _, _, n_regions, n_states, region = _census(z, code)
    return [np.array([n_regions, n_states]), region]


def polygonize_census_mask(m, code):
    """`m` is the mask (cell 0 is masked out); the raster is VALUES as float64."""
    _, _, n_regions, n_states, region = _census(VALUES.astype(np.float64), F64, m, code)
    return [np.array([n_regions, n_states]), region]


def polygonize_scatter(z, code):
    src, work, n_regions, n_states, _ = _census(z, _true(z))
    rings = xs.DeviceArray((_lib.workspace_bytes("polygonize_rings", n_states),), np.uint8)
    n_rings, n_points = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.call("xrs_polygonize_rings", z.shape[0], z.shape[1], work.ptr, rings.ptr, n_states, n_regions, ctypes.byref(n_rings),
              ctypes.byref(n_points), None, get_stream())
    n_rings, n_points = int(n_rings.value), int(n_points.value)
    points, column = xs.DeviceArray((n_points, 2), np.float64), xs.DeviceArray((n_regions,), z.dtype)
    ring_off, poly_off = xs.DeviceArray((n_rings + 1,), np.int64), xs.DeviceArray((n_regions + 1,), np.int64)
    _lib.call("xrs_polygonize_scatter", src.ptr, code, z.shape[0], z.shape[1], work.ptr, rings.ptr, n_states, n_regions, n_rings,
              None, points.ptr, ring_off.ptr, poly_off.ptr, column.ptr, get_stream())
    s = get_stream()
    return [column.get(s).astype(np.float64), points.get(s), ring_off.get(s), poly_off.get(s)]


def proximity(z, code):
    rows, cols = z.shape
    aux = _up(np.concatenate([np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64), [4.0, 7.0]]))
    src, work, out = _up(z), workspace("proximity", rows, cols), xs.DeviceArray((3, rows, cols), np.float32)
    _lib.call("xrs_proximity", src.ptr, code, rows, cols, aux.ptr, aux.ptr + 8 * cols, None, aux.ptr + 8 * (cols + rows), VALUES_F64,
              2, float("inf"), 0, 3, work.ptr, out.ptr, get_stream())    # EUCLIDEAN, all three planes: allocation reads the raster
    return [out.get(get_stream())]


def astar(z, code):
    rows, cols = z.shape
    src, work, out = _up(z), workspace("astar", rows, cols, at_least=1), xs.DeviceArray((rows, cols), np.float64)
    barriers, status = _up(np.array([6.0, 7.0])), (ctypes.c_int64 * 8)()
    _lib.call("xrs_astar", src.ptr, code, rows, cols, 0, 0, rows - 1, cols - 1, barriers.ptr, VALUES_F64, 2, 8, 0, work.ptr, out.ptr,
              status, get_stream())
    return [out.get(get_stream()), np.array(status[:7])]                 # (word 7 counts passes, not a result)


def _local(op, planes, codes, ref, ref_code):
    n, out = planes[0].size, xs.DeviceArray(planes[0].shape, np.float64)
    dev, ref_dev = [_up(p) for p in planes], _up(ref) if ref is not None else None
    _lib.call("xrs_local_cells", op, (ctypes.c_void_p * len(dev))(*[d.ptr for d in dev]), (ctypes.c_int * len(dev))(*codes), len(dev),
              ref_dev.ptr if ref_dev is not None else None, ref_code, n, out.ptr, 0, get_stream())
    return out.get(get_stream())


def local_cells_plane(z, code):
    """Plane 0 carries `code`; plane 1 is the raster reversed, in its true dtype.  MAX and SUM: both working types' loads."""
    planes, codes = [z, z[::-1, ::-1]], [code, _true(z)]
    return [_local(op, planes, codes, None, 0) for op in (LOCAL_MAX, LOCAL_SUM)]


def local_cells_ref(r, code):
    """`r` is the ref plane; the two planes are float64."""
    planes = [VALUES.astype(np.float64), VALUES[::-1, ::-1].astype(np.float64)]
    return [_local(LOCAL_LESSER, planes, [F64, F64], r, code)]


def flow_direction(z, code):
    src, out = _up(z), xs.DeviceArray(z.shape, np.float32)
    _lib.call("xrs_flow_direction", src.ptr, code, z.shape[0], z.shape[1], 1.0, 1.0, 2.0 ** 0.5, out.ptr, get_stream())
    return [out.get(get_stream())]


def fill(z, code):
    src, out, work = _up(z), xs.DeviceArray(z.shape, z.dtype), workspace("fill", *z.shape)
    status = (ctypes.c_int64 * FILL_STATUS_WORDS)()
    _lib.call("xrs_fill", src.ptr, code, z.shape[0], z.shape[1], out.ptr, work.ptr, status, 0, get_stream())
    return [out.get(get_stream()).astype(np.float64)]


def flow_flats(z, code):
    src, codes, work = _up(z), xs.DeviceArray(z.shape, np.float32), workspace("flow_flats", *z.shape)
    status = (ctypes.c_int64 * FILL_STATUS_WORDS)()
    _lib.call("xrs_flow_direction", src.ptr, _true(z), z.shape[0], z.shape[1], 1.0, 1.0, 2.0 ** 0.5, codes.ptr, get_stream())
    _lib.call("xrs_flow_flats", src.ptr, code, z.shape[0], z.shape[1], codes.ptr, work.ptr, status, 0, get_stream())
    return [codes.get(get_stream())]


# ------------------------------------------------------------------ the table
# (runner, values, codes the entry has no kernel for, the refusal with the code as %d)
FLOATS_ONLY = [c for c in range(10) if c not in (F32, F64)]
ENTRIES = {
    "xrs_cast_f32": (cast_f32, VALUES, [F32], "xrs_cast_f32: unknown source dtype code %d"),
    "xrs_classify_to_f64": (classify_to_f64, VALUES, [F64], "xrs_classify_to_f64: unsupported dtype code %d"),
    "xrs_true_color_u8": (true_color_u8, VALUES, [], "xrs_true_color_u8: unknown dtype code %d"),
    "xrs_match_bbox": (match_bbox, VALUES, [], "xrs_match_bbox: unknown dtype code %d"),
    "xrs_regions_link": (regions_link, VALUES, [], "xrs_regions_link: unsupported dtype code %d"),
    "xrs_regions_label": (regions_label, VALUES, [], "xrs_regions_label: unsupported dtype code %d"),
    "xrs_polygonize_census": (polygonize_census, VALUES, [], "xrs_polygonize_census: unsupported dtype code %d"),
    "xrs_polygonize_census mask": (polygonize_census_mask, VALUES, [], "xrs_polygonize_census: unsupported mask dtype code %d"),
    "xrs_polygonize_scatter": (polygonize_scatter, VALUES, [], "xrs_polygonize_scatter: unsupported dtype code %d"),
    "xrs_proximity": (proximity, VALUES, [], "xrs_proximity: unsupported dtype code %d"),
    "xrs_astar": (astar, VALUES, [], "xrs_astar: unsupported dtype code %d"),
    "xrs_local_cells plane": (local_cells_plane, VALUES, [U64], "xrs_local_cells: plane 0 has unsupported dtype code %d"),
    "xrs_local_cells ref": (local_cells_ref, VALUES, [U64], "xrs_local_cells: ref has unsupported dtype code %d"),
    "xrs_fill": (fill, FILL_VALUES, FLOATS_ONLY, "xrs_fill: unsupported dtype code %d (float32 or float64)"),
    "xrs_flow_flats": (flow_flats, FLAT_VALUES, FLOATS_ONLY, "xrs_flow_flats: unsupported dtype code %d (float32 or float64)"),
    "xrs_flow_direction": (flow_direction, VALUES, FLOATS_ONLY, "xrs_flow_direction: unsupported dtype code %d (float32 or float64)"),
}


def _reference_dtype(excluded):
    return np.dtype(np.float32 if F64 in excluded else np.float64)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_refusals(name):
    run, values, excluded, text = ENTRIES[name]
    z = values.astype(_reference_dtype(excluded))
    for code in [-1, 10] + excluded:
        with pytest.raises(_lib.XrsError):                               # (`_lib.call` raises on a non-zero return)
            run(z, code)
        assert _lib.last_error() == text % code, (name, code)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_accepted_code_gives_the_float_result(name):
    run, values, excluded, _ = ENTRIES[name]
    ref = _reference_dtype(excluded)
    want = run(values.astype(ref), DTYPE_CODE[ref])
    accepted = [dt for dt in ALL if DTYPE_CODE[dt] not in excluded and dt != ref]
    assert len(accepted) == 9 - len(excluded)
    for dt in accepted:
        got = run(values.astype(dt), DTYPE_CODE[dt])
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape, (name, dt, k)
            np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=f"{name} {dt} result {k}")
