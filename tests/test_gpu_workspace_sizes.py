"""What the `xrs_*_workspace_bytes` / `_size` entries answer, against the layouts written out again here from the layout
comments of the `carve` functions in csrc (every part starts on a 256-byte boundary: up(v) = v rounded up to 256).  No kernel
is launched.

  * entries without a hipCUB part: the answer equals the formula, refused shapes (0 or 256) included;
  * entries with a hipCUB part (its size is the vendor library's business): the answer is a multiple of 256 and at least the
    parts in front of the hipCUB block plus the least that block can be.
The cases are tests/workspace_cases.py; run as a script with XRS_LIB pointing at two builds, that file compares the
hipCUB-bearing totals exactly.  This file passes unmodified on the library from before the layouts were gathered into
csrc/workspace.h: that library defined the answers."""
import math

import pytest

import xrspatial_amd as xs
from tests import workspace_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def up(v):
    return (v + 255) & ~255


def tiles(rows, cols, th, tw):
    return math.ceil(rows / th) * math.ceil(cols / tw)


# ------------------------------------------------------------------ exact: no hipCUB part
def astar(rows, cols):
    if rows <= 0 or cols <= 0 or rows * cols > 1 << 30:
        return 0
    t = tiles(rows, cols, 32, 64)                                  # field | dirty x 2 | changed | status | partial
    return up(rows * cols * 8) + 2 * up(t * 4) + up(64 * 4) + up(16 * 8) + up(1024 * 4 * 8)


def proximity(rows, cols):
    if rows <= 0 or cols <= 0:
        return 0
    return 2 * up(rows * cols * 4) + 2 * up(rows * 4) + 256         # left | right | flag | list | count


def flow(rows, cols, want):
    if rows <= 0 or cols <= 0 or not want & 3:
        return 0
    head = ((32 + 1) * 64 * 64 + 64) * 4                           # MAX_ROUNDS + 1 rows of slots, the invalid-code word
    planes = 2 + (3 if want & 1 else 0) + (2 if want & 2 else 0)   # anc x 2 | S, D x 2 | root x 2
    return head + planes * up(rows * cols * 4)


def fill(rows, cols, with_d=False):
    if rows <= 0 or cols <= 0:
        return 0
    t = tiles(rows, cols, 64, 64)                                  # head | flags | list | d
    return up((64 * 64 + 64) * 4) + 2 * up(t * 4) + (up(rows * cols * 4) if with_d else 0)


def flow_flats(rows, cols):
    return fill(rows, cols, with_d=True)


def zonal_mode(n, nz, f64):
    if n < 0 or nz <= 0:
        return 256
    k = 8 if f64 else 4
    parts = 2 * (n // 1024 + 1) + nz
    chunks = ((n // 8192 + 1 + nz + 7) // 8) * 8 + 8
    return (256 + up(nz * 4) + up(parts * 4)                        # hdr | zone_count | part_count: cleared per call
            + up((nz + 1) * 4) + up(nz * 4) + 2 * up((nz + 1) * 4) + up(nz)   # key_off | zone_cursor | part_base | chunk_base | zone_B
            + 3 * up(parts * 4) + up(parts * k) + up(chunks * 2)    # part_off | part_cursor | best_count | best_key | chunk_zone
            + 2 * up(n * k))                                        # keys | parted


def jenks(n, k):
    if n < 1 or n >= 1 << 24 or k < 1:
        return 0
    return 2 * up((n + 1) * 4)                                      # two columns of n + 1 float32


def mesh(rows, cols):
    if rows < 1 or cols < 1:
        return 0
    by, bx = (rows - 1 + 7) >> 3, (cols - 1 + 7) >> 3              # blocks of 2^3 mesh cells: the largest table
    return up(rows * cols * 4) + up((max(by, 0) * max(bx, 0) + 1) * 4)


EXACT = {"astar": astar, "proximity": proximity, "flow": flow, "fill": fill, "flow_flats": flow_flats, "zonal_mode": zonal_mode,
         "jenks": jenks, "hillshade_shadow": mesh, "viewshed_mesh": mesh}


# ------------------------------------------------------------------ bounds: (parts in front of the hipCUB block, its least size)
def regions(rows, cols):
    if rows < 0 or cols < 0:
        return None
    words = rows * math.ceil(cols / 64)                            # parent | mask | cnt (+ the total) | cub: up(max(bytes, 1))
    return up(rows * cols * 4) + up(words * 8) + up((words + 1) * 4), 256


def polygonize(rows, cols):
    if rows < 1 or cols < 1:
        return None
    n = rows * cols
    words = (n + 63) // 64        # region | parent | mask | links | rootbits | cnt | sbits | scnt | cub: up(max(bytes, 1))
    return 2 * up(n * 4) + 2 * up(n) + up(words * 8) + up((words + 1) * 4) + up(words * 32) + up((words + 1) * 8), 256


def polygonize_rings(ns):
    if ns == 0 or ns > wc.MAX_STATES:
        return None
    rings = ns // 4 + 1           # next | buf x 4 | lead | emit | keys x 2 | count1 | ring_off | poly_off | words | cub
    return 6 * up(ns * 4) + up(ns) + 2 * up(rings * 8) + 3 * up((rings + 1) * 8) + up((8 + 2 * 32 + 8) * 4), 256


def zonal_majority(n, nz, f64):
    if n <= 0 or nz <= 0:
        return None
    k = 8 if f64 else 4           # vk x 2 | zk x 2 | flags | pos | nruns | best | cub: up(bytes) + 256
    return 2 * up(n * k) + 2 * up(n * 4) + up(n) + up(n * 4) + 256 + up(nz * 8), 256


def classify(n, f64):
    m, k = max(n, 1), 8 if f64 else 4
    select = up(3 * 64 * 8 + 64 * 4 + 8) + 64 * 2048 * 4           # SelState (n_dp padded to 8 bytes) | histograms
    # maximum_breaks: k x 2 | uk | flags | m | parts | bound | picked | cub: up(bytes) + 256
    breaks = 3 * up(m * k) + up(m) + 256 + up(512 * 16) + 256 + up(64 * 8)
    return max(select, up(1024 * 32), breaks + 256), 0             # the largest of the three users of the block


def local_combine(n, n_planes):
    if n <= 0 or n >= 1 << 31:
        return None               # idx x 2 | key x 2 (each up(8 n) + 256) | cls | scan | bad | small | cub: up(bytes) + 256
    return 2 * up(n * 4) + 2 * (up(n * 8) + 256) + 2 * up(n * 4) + up(n) + 256, 256


def bump(count, width, height, spread, max_events):
    box = min(2 * spread, width) * min(2 * spread, height)
    disc = sum(m + 1 + min(m, spread - 1) for m in (math.isqrt(spread * spread - dx * dx) for dx in range(-spread, spread)))
    footprint = min(disc, box) if spread > 0 else 1
    if footprint > max_events:
        return None
    n = max(count, 1)
    cap = min(max_events, n * footprint)
    chunk = min(cap // footprint, n)
    segs = min(cap, width * height)   # keys x 2 | seg | offs | v | flag | ctrl | cub: up(bytes), which may be 0
    return 2 * up(cap * 8) + up(segs * 4) + up((chunk + 1) * 4) + up(chunk * 8) + up(chunk * 4) + up(16), 0


BOUNDED = {"regions": regions, "polygonize": polygonize, "polygonize_rings": polygonize_rings, "zonal_majority": zonal_majority,
           "classify": classify, "local_combine": local_combine, "bump": bump}
REFUSED = {"regions": 0, "polygonize": 0, "polygonize_rings": 0, "zonal_majority": 256, "local_combine": 256, "bump": 0}


def _id(case):
    return case[0] + "-" + "x".join(str(a) for a in case[1])


def test_the_cases_cover_every_entry():
    assert {name for name, _ in wc.CASES} == set(EXACT) | set(BOUNDED)


@pytest.mark.parametrize("case", [c for c in wc.CASES if c[0] in EXACT], ids=_id)
def test_exact_total(case):
    name, args = case
    assert wc.answer(name, args) == EXACT[name](*args)


@pytest.mark.parametrize("case", [c for c in wc.CASES if c[0] in BOUNDED], ids=_id)
def test_total_with_a_hipcub_part(case):
    name, args = case
    got, plan = wc.answer(name, args), BOUNDED[name](*args)
    if plan is None:
        assert got == REFUSED[name]
        return
    front, least_tail = plan
    assert got % 256 == 0
    assert got >= front + least_tail
