"""One list of (entry name, args) over every `xrs_<name>_workspace_bytes` / `_size` entry whose scratch block is laid out by a
`carve` (csrc/workspace.h), at the shapes where a layout can go wrong and no larger: the edges of the 64 x 32 and 64 x 64
tiles and of the 64-cell bit words for rasters, the 256-byte rounding for flat sizes, refused shapes among them.

    python tests/workspace_cases.py      prints one `name args bytes` line per case

With XRS_LIB pointing at another build of the library the output must not change: the totals that hold a hipCUB part, which
tests/test_gpu_workspace_sizes.py can only bound, are compared exactly that way."""

SHAPES = [(-1, 5), (0, 5), (1, 1), (1, 65), (33, 64), (65, 129), (257, 3)]     # rows x cols
FLAT_N = [0, 1, 255, 256, 257, 4097]
ZONES = [1, 64, 65]
FLOW_WANT = [1, 2, 3]                                 # XRS_FLOW_ACCUMULATION, XRS_FLOW_BASINS, both
MAX_STATES = 2147483647                               # XRS_POLYGONIZE_MAX_STATES
RING_STATES = [0, 1, 4, 1025, MAX_STATES + 1]
BUMP_REFUSED = (4, 8, 8, 3, 1)                        # count, width, height, spread, max_events: one footprint does not fit
BUMP_ACCEPTED = (4, 8, 8, 3, 1000)

RASTER_ENTRIES = ("regions", "polygonize", "proximity", "astar", "fill", "flow_flats", "hillshade_shadow", "viewshed_mesh")


def _cases():
    out = []
    for shape in SHAPES:
        out += [(name, shape) for name in RASTER_ENTRIES]
        out += [("flow", shape + (want,)) for want in FLOW_WANT]
    for n in FLAT_N:
        for f64 in (0, 1):
            out.append(("classify", (n, f64)))
            out += [(name, (n, nz, f64)) for name in ("zonal_mode", "zonal_majority") for nz in ZONES]
        out.append(("local_combine", (n, 2)))
        out.append(("jenks", (n, 5)))
    out += [("polygonize_rings", (n,)) for n in RING_STATES]
    out += [("bump", BUMP_REFUSED), ("bump", BUMP_ACCEPTED)]
    return out


CASES = _cases()


def answer(name, args):
    from xrspatial_amd import _lib
    return _lib.workspace_bytes(name, *args)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name, args in CASES:
        print(name, " ".join(str(a) for a in args), answer(name, args))
