"""CPU statements of the reference's bump loop (xrspatial/bump.py:12-28), for tests only.

`finish_bump` restates the loop bump by bump; tests/test_bump_host.py pins it to what the reference's own code produced
(tests/golden/bump_exec.npz), and the GPU tests use it for live cases.  `fold_model` is the specification of csrc/bump.hip: the
same result from sorted (cell, bump) events folded in passes, with the chunk plan and the status words of the kernel."""
import numpy as np

MAX_EVENTS = (1 << 31) - 1
EXACT_FOOTPRINT = 4096


def footprint(spread):
    """[(dx, dy)] of an unclipped bump in the reference's order: nx outer, ny inner, both upper bounds exclusive."""
    s = spread * spread
    if spread <= 0:
        return []
    return [(dx, dy) for dx in range(-spread, spread) for dy in range(-spread, spread) if dx * dx + dy * dy <= s]


def _tables(spread, width, height):
    """the footprint's offsets that can fall inside a width x height raster at all, with their weights"""
    s = spread * spread
    cells = [(dx, dy) for dx in range(max(-spread, 1 - width), min(spread, width)) for dy in range(max(-spread, 1 - height), min(spread, height))
             if dx * dx + dy * dy <= s]
    dx = np.array([c[0] for c in cells], np.int64)
    dy = np.array([c[1] for c in cells], np.int64)
    weight = (dx * dx + dy * dy).astype(np.float64) / np.float64(s)          # int / int of the reference: one IEEE division
    after = (dx > 0) | ((dx == 0) & (dy > 0))                                # walked after the centre's own `+ v * 0.0`
    return dx, dy, weight, after


def finish_bump(width, height, locs, heights, spread):
    """The reference's loop.  Within one bump the footprint cells are distinct, so the inner loops are one indexed add; the
    centre is re-read for every cell, so the cells walked after it see what its own `+ v * 0.0` left (NaN for an infinite v)."""
    out = np.zeros((height, width))
    locs = np.asarray(locs).astype(np.int64)
    z = np.asarray(heights, dtype=np.float64)
    if spread >= 1:
        dx, dy, weight, after = _tables(spread, width, height)
    with np.errstate(all="ignore"):
        for i in range(len(z)):
            x, y = int(locs[i, 0]), int(locs[i, 1])
            out[y, x] = out[y, x] + z[i]
            if spread >= 1:
                nx, ny = x + dx, y + dy
                ok = (nx >= 0) & (nx < width) & (ny >= 0) & (ny < height)
                v = out[y, x]
                seen = np.where(after[ok], v + v * 0.0, v)
                out[ny[ok], nx[ok]] = out[ny[ok], nx[ok]] + seen * weight[ok]
    return out


def footprint_bound(width, height, spread):
    """most events of one bump (csrc/bump.hip `footprint_bound`)"""
    if spread <= 0:
        return 1
    box = min(2 * spread, width) * min(2 * spread, height)
    if spread > EXACT_FOOTPRINT:
        return box
    return min(len(footprint(spread)), box)


def plan(count, width, height, spread, max_events):
    """(events a chunk may hold, bumps of a chunk), as csrc/bump.hip `make_plan` has them"""
    f = footprint_bound(width, height, spread)
    n = max(count, 1)
    cap = min(max_events, MAX_EVENTS)
    if cap // f >= n:
        cap = n * f
    return cap, min(cap // f, n)


def fold_model(width, height, locs, heights, spread, max_events=1 << 27):
    """(out, status) of the event / fold scheme.  One event per (cell, bump) of every clipped footprint, sorted by cell and then
    bump.  Every touched cell is walked in order by its own cursor: the centre's event adds z, publishes v with the number of
    the pass and adds v * 0.0; any other event is ready only if v was published in an EARLIER pass, else the cell stops for
    this pass.  Passes repeat until every event is retired; a pass that retires none is an error."""
    locs = np.asarray(locs).astype(np.int64)
    z = [float(h) for h in np.asarray(heights, dtype=np.float64)]
    count = len(z)
    cells = footprint(spread) if spread >= 1 else [(0, 0)]
    s = spread * spread
    out = [0.0] * (width * height)
    cap, chunk = plan(count, width, height, spread, max_events)
    status = dict(chunks=0, events=0, passes=0, touched_cells=0)
    for b0 in range(0, count, chunk):
        nb = min(chunk, count - b0)
        jbits = max(1, (chunk - 1).bit_length())
        keys = []
        for j in range(nb):
            x, y = int(locs[b0 + j, 0]), int(locs[b0 + j, 1])
            assert 0 <= x < width and 0 <= y < height
            for dx, dy in cells:
                nx, ny = x + dx, y + dy
                if 0 <= nx < width and 0 <= ny < height:
                    keys.append(((ny * width + nx) << jbits) | j)
        keys.sort()
        total = len(keys)
        assert 0 < total <= cap
        cursors = [e for e in range(total) if e == 0 or keys[e - 1] >> jbits != keys[e] >> jbits]
        v, flag = [0.0] * nb, [0] * nb
        retired, n_pass = 0, 0
        while retired < total:
            n_pass += 1
            before = retired
            for slot, cur in enumerate(cursors):
                if cur is None:
                    continue
                cell = keys[cur] >> jbits
                cy, cx = divmod(cell, width)
                acc = out[cell]
                done = False
                while True:
                    j = keys[cur] & ((1 << jbits) - 1)
                    dx, dy = cx - int(locs[b0 + j, 0]), cy - int(locs[b0 + j, 1])
                    if dx == 0 and dy == 0:
                        acc = acc + z[b0 + j]
                        if spread >= 1:
                            v[j], flag[j] = acc, n_pass
                            acc = acc + acc * 0.0
                    else:
                        if flag[j] == 0 or flag[j] >= n_pass:
                            break
                        vi = v[j]
                        if dx > 0 or (dx == 0 and dy > 0):
                            vi = vi + vi * 0.0
                        acc = acc + vi * ((dx * dx + dy * dy) / s)
                    retired += 1
                    cur += 1
                    if cur == total or keys[cur] >> jbits != cell:
                        done = True
                        break
                out[cell] = acc
                cursors[slot] = None if done else cur
            assert retired > before, "a pass retired no event"
        status["chunks"] += 1
        status["events"] += total
        status["passes"] += n_pass
        status["touched_cells"] += len(cursors)
    return np.array(out, np.float64).reshape(height, width), status


def same_bits(got, want):
    """Equal as the issue defines it: NaN where NaN (sign and payload free), identical bits everywhere else."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float64 or want.dtype != np.float64:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if not np.array_equal(nan_g, nan_w):
        return False
    return np.array_equal(np.ascontiguousarray(got).view(np.uint64)[~nan_g], np.ascontiguousarray(want).view(np.uint64)[~nan_w])
