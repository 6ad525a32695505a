"""What xrs_rasterize_workspace_size and xrs_rasterize_spans_workspace_size answer, against the layouts written out again
here from the `carve` functions of csrc/rasterize.hip, the way tests/test_gpu_workspace_sizes.py checks the other entries:
every part starts on a 256-byte boundary, the hipCUB block at the end is the vendor library's business, so the answer is a
multiple of 256 and at least the parts in front of that block plus the least it can be.  No kernel is launched."""
import pytest

import xrspatial_amd as xs
from xrspatial_amd import _lib

pytestmark = pytest.mark.gpu

MAX_POINTS = (1 << 31) - 1
MAX_CROSSINGS = (1 << 31) - 2


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def up(v):
    return (v + 255) & ~255


def census(n):
    if n == 0 or n > MAX_POINTS:
        return None
    return up((n + 1) * 8) + 2 * up(n * 4) + up(64 * 4), 256        # cnt (+ the total) | poly | next | flags | cub: up(max(bytes, 1))


def spans(c):
    if c == 0 or c > MAX_CROSSINGS:
        return None
    return 2 * up(c * 8) + up((c // 2 + 1) * 8) + up(64 * 4), 256    # keys x 2 | chunks (+ the total) | words | cub


@pytest.mark.parametrize("name,plan,sizes", [
    ("rasterize", census, (0, 1, 2, 31, 32, 33, 1000, 65537, 10**7, MAX_POINTS, MAX_POINTS + 1)),
    ("rasterize_spans", spans, (0, 2, 4, 62, 64, 66, 1000, 65538, 10**7, MAX_CROSSINGS, MAX_CROSSINGS + 2)),
])
def test_total_with_a_hipcub_part(name, plan, sizes):
    last = 0
    for n in sizes:
        got, want = _lib.workspace_bytes(name, n), plan(n)
        if want is None:
            assert got == 0, (name, n)
            continue
        front, least_tail = want
        assert got % 256 == 0 and got >= front + least_tail, (name, n, got, front)
        assert got >= last, (name, n)                            # more to hold never takes less
        last = got
