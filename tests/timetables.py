"""Non-uniform pose / IMU time tables and pose sequences for the table-search tests
(test_gpu_table_search.py, test_timetables_cpu.py).  A plain module, deterministic from its seeds.

k_prep looks a frame's times up in the 64 table entries around an interpolation guess
(kernels.hpp probe_base / probe_count) and takes the wave-cooperative full search only when that
window does not decide the answer.  On a uniform grid the guess is always right; these tables make
it wrong: curved (convex / concave), alternating dense and sparse blocks (bursty), one gap longer
than the rest of the table (dropout), runs of equal timestamps shorter than, equal to and longer
than the window (plateaus), and a table of one repeated value (flat).
"""
import numpy as np

T_FIRST = 3.25
SEED = 4                  # the tests' tables (bursty leaves the probe window for ~0.8 of the frames at T >= 4096)
MIN_GAP = 1e-5            # every gap of a table is exactly 0 or at least this (seconds)
KINDS = ("convex", "concave", "bursty", "dropout", "plateaus")     # "flat" besides, frame mode only
INCREASING = ("convex", "concave", "bursty", "dropout")           # strictly increasing tables
SIZES = (65, 127, 128, 129, 4096, 4097, 20011)
FLAT_T = 130
BURST = 97                # bursty: every other block of this many gaps is dense
RUN_LENGTHS = (2, 63, 64, 65, 200)    # plateaus: runs of equal timestamps, around the 64-entry window
RUN_FIRST, RUN_APART = 5, 37
PROBE = 64                # kernels.hpp: the probe window's entries; the guess sits at entry 31 of it


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def plateau_runs(T):
    """[(first index, length)] of the runs of equal timestamps in table("plateaus", T, .): the first
    starts at index RUN_FIRST, each next one RUN_APART entries after the previous one's last entry;
    a run that would reach the table's end is dropped (and every later one with it)."""
    runs, start = [], RUN_FIRST
    for n in RUN_LENGTHS:
        if start + n >= T:
            break
        runs.append((start, n))
        start += n - 1 + RUN_APART
    return runs


def table(kind, T, seed):
    """float64 non-decreasing times, time[0] = T_FIRST; gaps 10 ** uniform(-5, 0) s shaped by ``kind``
    (module docstring).  Every difference of neighbours is exactly 0 or >= MIN_GAP: metre-sized pose
    jumps over sub-nanosecond segments would let the kernels' integer-nanosecond segment boundaries
    and the oracle's float compare differ legitimately."""
    if kind == "flat":
        return np.full(T, T_FIRST)
    rng = _rng(seed, T, 1)
    gaps = 10.0 ** rng.uniform(-5.0, 0.0, T - 1)
    if kind == "convex":
        gaps = np.sort(gaps)
    elif kind == "concave":
        gaps = np.sort(gaps)[::-1]
    elif kind == "bursty":
        dense = (np.arange(T - 1) // BURST) % 2 == 1
        gaps[dense] = rng.uniform(1e-5, 2e-5, int(dense.sum()))
    elif kind == "dropout":
        mid = (T - 1) // 2
        gaps[mid] = 0.0
        gaps[mid] = 1.5 * gaps.sum()
    elif kind == "plateaus":
        gaps = np.full(T - 1, 0.01)
        for start, n in plateau_runs(T):
            gaps[start:start + n - 1] = 0.0
    else:
        raise ValueError(kind)
    # the running sum rounds each time to its own ulp (< 1e-12 s here): keep the rounded
    # differences at or above MIN_GAP
    gaps = np.where(gaps > 0.0, np.maximum(gaps, MIN_GAP * (1.0 + 1e-5)), 0.0)
    return T_FIRST + np.concatenate([[0.0], np.cumsum(gaps)])


def poses(T, seed, spiky=True):
    """(position (T, 3), rpy (T, 3)).

    spiky: positions a random walk with N(0, 5 m) steps, roll / pitch N(0, 0.02), yaw a running sum
    wrapped to +-pi whose steps are N(0, 1e-3) except about 5 % of +-U(2.0, 2.9) rad: isolated
    segments with quaternion angle Theta up to 1.45 between neighbours of Theta ~ 5e-4 (a polynomial
    tier taken from the neighbouring segment is grossly wrong), and no step near pi (the shortest arc
    is never ambiguous).
    not spiky (Path A index decoding): pos[k] = (k, -2k, 0.5k), exact in float32 up to T = 20011, so
    the origin's image names the pose that was used; rpy[k] i.i.d. U(-pi, pi)."""
    rng = _rng(seed, T, 2)
    if not spiky:
        k = np.arange(T, dtype=np.float64)
        return np.column_stack([k, -2.0 * k, 0.5 * k]), rng.uniform(-np.pi, np.pi, (T, 3))
    pos = np.cumsum(rng.normal(0.0, 5.0, (T, 3)), axis=0)
    step = rng.normal(0.0, 1e-3, T)
    big = rng.random(T) < 0.05
    step[big] = rng.choice([-1.0, 1.0], int(big.sum())) * rng.uniform(2.0, 2.9, int(big.sum()))
    yaw = (np.cumsum(step) + np.pi) % (2.0 * np.pi) - np.pi
    return pos, np.column_stack([rng.normal(0.0, 0.02, T), rng.normal(0.0, 0.02, T), yaw])


def frame_queries(kind, time):
    """Frame times for the Path A index test: up to 600 table entries spread over the table (exact
    ties), nextafter of each both ways, midpoints of neighbours, both ends +-1 s, -inf, +inf and NaN;
    plateaus: every run's value, nextafter of it both ways, and the entries before and after the
    run; dropout: times inside the long gap."""
    T = len(time)
    sel = np.unique(np.round(np.linspace(0, T - 1, min(T, 600))).astype(np.int64))
    extra = [np.array([time[0] - 1.0, time[-1] + 1.0, -np.inf, np.inf, np.nan])]
    if kind == "plateaus":
        for start, n in plateau_runs(T):
            v = time[start]
            extra.append(np.array([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf),
                                   time[start - 1], time[start + n]]))
    if kind == "dropout":
        mid = (T - 1) // 2
        extra.append(np.linspace(time[mid], time[mid + 1], 9)[1:-1])
    t = time[sel]
    nb = sel[sel < T - 1]
    return np.concatenate([t, np.nextafter(t, -np.inf), np.nextafter(t, np.inf),
                           0.5 * (time[nb] + time[nb + 1])] + extra)


def guess_misses(time, x):
    """True where the 64-entry probe window around the interpolation guess for x does NOT decide
    x's place in ``time``, i.e. where k_prep takes its full wave-cooperative search.

    Mirrors probe_base / probe_count in csrc/kernels.hpp (the window's first entry from the guess,
    and the rule by which the window decides) and must change with them.  Used only to qualify test
    inputs, never as a reference.  Stated for the strict compare (searchsorted 'left'); a NaN query
    makes the guess 0 there as here (fmax(NaN, 0) = 0) and compares false everywhere."""
    time = np.asarray(time, dtype=np.float64)
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    T = len(time)
    if T <= PROBE:
        return np.zeros(len(x), bool)
    span = time[-1] - time[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = (x - time[0]) / span * (T - 1) if span > 0.0 else np.zeros(len(x))
        g = np.where(np.isnan(g), 0.0, np.clip(g, 0.0, float(T - 1)))
        base = np.clip(g.astype(np.int64) - (PROBE // 2 - 1), 0, T - PROBE)
        lo_ok = (base == 0) | (time[base] < x)
        hi_ok = (base + PROBE >= T) | ~(time[base + PROBE - 1] < x)
    return ~(lo_ok & hi_ok)
