"""A dtype-explicit NumPy model of csrc/jenks.hip -- TEST INFRASTRUCTURE.

The kernel runs one launch per class column j and one thread per row l; every thread walks m = 0 .. l-1 down the sorted
sample.  Here the threads of a launch are the elements of NumPy vectors and the walk is a Python loop over m, so every
operation below is one IEEE operation per row in a stated type (NumPy's element-wise float64 / float32 arithmetic neither fuses
nor reorders): float64 sums of float32 values, the square rounded to float32 first, one float64 division per step, the float32
running minimum replaced on `>=`.  tests/test_natural_breaks_host.py holds it against the tables the reference's own loop
produced (tests/golden/natural_breaks_exec.npz), bit for bit; the GPU tests hold the kernel against the same tables.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def initial_tables(n, k):
    limits = np.zeros((n + 1, k + 1), F32)
    limits[1, 1:] = 1.0
    var = np.zeros((n + 1, k + 1), F32)
    var[2:, 1:] = np.inf
    return limits, var


def column(data, prev, j):
    """Rows 2 .. n of column j of (limits, var) from column j-1 of var (`prev`, entries 0 .. n)."""
    n = data.shape[0]
    rows = np.arange(2, n + 1)
    total, squares, w = (np.zeros(rows.size, F64) for _ in range(3))
    variance = np.zeros(rows.size, F64)
    best = np.full(rows.size, np.inf, F32)
    limit = np.zeros(rows.size, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(n):
            on = slice(max(0, m - 1), None)                  # the rows with l - 1 - m >= 0
            i4 = rows[on] - 1 - m
            val = data[i4]                                   # float32
            w[on] += F64(1.0)
            total[on] += val.astype(F64)
            squares[on] += (val * val).astype(F64)           # a float32 product, then widened
            variance[on] = squares[on] - (total[on] * total[on]) / w[on]
            if j == 1:
                continue
            cls = slice(max(0, m), None)                     # ... and i4 != 0: a class can start at i4
            at = rows[cls] - 1 - m
            cand = variance[cls] + prev[at].astype(F64)
            take = best[cls].astype(F64) >= cand
            best[cls] = np.where(take, cand.astype(F32), best[cls])
            limit[cls] = np.where(take, (rows[cls] - m).astype(F32), limit[cls])
    if j == 1:
        return np.ones(rows.size, F32), variance.astype(F32)
    return limit, best


def jenks_tables(sorted_sample, k):
    """(lower_class_limits, var_combinations) as xrs_jenks_matrices_f32 writes them."""
    data = np.ascontiguousarray(sorted_sample, dtype=F32)
    n = data.shape[0]
    limits, var = initial_tables(n, k)
    if n >= 2:
        for j in range(1, k + 1):
            limits[2:, j], var[2:, j] = column(data, var[:, j - 1].copy(), j)
    return limits, var
