"""CPU: the non-uniform time tables of timetables.py are what they claim to be, and the oracle
(oracle.restatement.slerp_pose) can be trusted on them: against scipy's Slerp on the strictly
increasing tables, against a literal per-query loop on runs of equal timestamps."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation, Slerp

import timetables as tt
from oracle import restatement as R

CASES = [(k, T) for k in tt.KINDS for T in tt.SIZES] + [("flat", tt.FLAT_T)]


@pytest.mark.parametrize("kind,T", CASES)
def test_generator_invariants(kind, T):
    time = tt.table(kind, T, seed=tt.SEED)
    assert time.dtype == np.float64 and time.shape == (T,) and time[0] == 3.25
    assert np.array_equal(time, tt.table(kind, T, seed=tt.SEED))            # deterministic
    gaps = np.diff(time)
    assert np.all((gaps == 0.0) | (gaps >= tt.MIN_GAP)), gaps[(gaps != 0) & (gaps < tt.MIN_GAP)]
    if kind in tt.INCREASING:
        assert np.all(gaps > 0)
    if kind == "convex":          # the sorted gaps, up to the rounding of the running sum
        assert np.all(np.diff(gaps) >= -1e-11) and gaps[-1] > 100 * gaps[0]
    if kind == "concave":
        assert np.all(np.diff(gaps) <= 1e-11) and gaps[0] > 100 * gaps[-1]
    if kind == "bursty":
        dense = (np.arange(T - 1) // tt.BURST) % 2 == 1
        assert np.all(gaps[dense] <= 2e-5 + 1e-11)
        assert np.median(gaps[~dense]) > 1e-4
    if kind == "dropout":
        mid = (T - 1) // 2
        assert gaps[mid] == pytest.approx(1.5 * (gaps.sum() - gaps[mid]), rel=1e-9)
        assert np.all(np.delete(gaps, mid) <= 1.0 + 1e-9)
    if kind == "plateaus":
        # the runs of equal timestamps found in the table itself are the announced ones
        z = np.concatenate([[False], gaps == 0.0, [False]])
        first = np.flatnonzero(z[1:] & ~z[:-1])
        last = np.flatnonzero(~z[1:] & z[:-1])
        found = [(int(a), int(b - a + 1)) for a, b in zip(first, last)]
        assert found == tt.plateau_runs(T)
        assert first[0] == tt.RUN_FIRST
        want = [n for n in tt.RUN_LENGTHS if n + tt.RUN_FIRST < T][:len(found)]
        assert [n for _, n in found] == want
        assert len(found) == (5 if T >= 4096 else 2 if T >= 127 else 1)
        assert np.allclose(gaps[gaps > 0], 0.01, rtol=0, atol=1e-12)
    if kind == "flat":
        assert np.all(time == 3.25)


def test_pose_generators():
    pos, rpy = tt.poses(20011, 3, spiky=False)
    k = np.arange(20011)
    assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos)      # exact in float32
    assert np.array_equal(pos, np.column_stack([k, -2.0 * k, 0.5 * k]))
    assert np.all(np.abs(rpy) <= np.pi)
    pos, rpy = tt.poses(20011, 3, spiky=True)
    q = R.euler_xyz_quat(rpy)
    th = 2 * np.arccos(np.minimum(np.abs(np.sum(q[:-1] * q[1:], axis=1)), 1.0))    # rotation angle per step
    big = th > 1.0
    assert 0.03 < big.mean() < 0.07
    assert th[big].min() > 1.9 and th[big].max() < 3.0            # none near pi: the shortest arc is clear
    assert np.median(th[~big]) < 0.05
    # isolated: a large segment's neighbours are almost always small ones
    assert np.mean(big[1:] & big[:-1]) < 0.01
    assert np.all(np.abs(rpy[:, 2]) <= np.pi)


@pytest.mark.parametrize("kind,T", CASES)
def test_guess_misses_rule_and_share(kind, T):
    """Where guess_misses says the probe window decides, counting inside the window gives numpy's
    searchsorted (so the rule the kernel's probe_count states is sound on these tables), and on the
    long tables the frame test's queries leave the window for at least half the frames."""
    time = tt.table(kind, T, seed=tt.SEED)
    x = tt.frame_queries(kind, time)
    miss = tt.guess_misses(time, x)
    span = time[-1] - time[0]
    for xi, m in zip(x, miss):
        if m or np.isnan(xi):
            continue
        g = (xi - time[0]) / span * (T - 1) if span > 0 else 0.0
        base = int(np.clip(int(np.clip(g, 0, T - 1)) - 31, 0, T - 64))
        assert base + np.count_nonzero(time[base:base + 64] < xi) == np.searchsorted(time, xi, "left")
    share = float(miss.mean())
    print(f"guess_misses share {kind} T={T}: {share:.3f} of {len(x)} frames")
    if T >= 4096:
        assert share >= 0.5, (kind, T, share)


@pytest.mark.parametrize("T", [129, 4097, 20011])
@pytest.mark.parametrize("kind", tt.INCREASING)
def test_oracle_slerp_matches_scipy_on_nonuniform_tables(kind, T):
    time = tt.table(kind, T, seed=tt.SEED)
    pos, rpy = tt.poses(T, tt.SEED, spiky=True)
    rng = np.random.default_rng([T, 5])
    # half uniform in time (long segments), half a random segment at a random alpha (short ones too)
    k = rng.integers(0, T - 1, 2500)
    tq = np.concatenate([rng.uniform(time[0], time[-1], 2500),
                         time[k] + rng.uniform(0, 1, 2500) * (time[k + 1] - time[k])])
    tq = np.clip(tq, time[0], time[-1])
    Rm, p = R.slerp_pose(time, pos, rpy, tq)
    want = Slerp(time, Rotation.from_euler("xyz", rpy))(tq).as_matrix()
    err = float(np.abs(Rm - want).max())
    print(f"slerp_pose vs scipy Slerp {kind} T={T}: {err:.2e}")
    assert err <= 1e-13
    # position: np.interp's slope form against the oracle's alpha form, a few ulp of the largest
    # coordinate apart (|pos| up to ~2e3 m: 16 ulp = 7e-12 m)
    wp = np.column_stack([np.interp(tq, time, pos[:, c]) for c in range(3)])
    assert float(np.abs(p - wp).max()) <= 16 * np.finfo(np.float64).eps * np.abs(pos).max()


@pytest.mark.parametrize("T", [129, 4097])
def test_oracle_slerp_on_repeated_timestamps(T):
    """At a repeated timestamp slerp_pose gives the run's last sample, just before it the
    interpolation into the run's first; expected values from a per-query loop (linear scan for the
    last sample at or before t, scipy for the rotation between the two samples)."""
    time = tt.table("plateaus", T, seed=tt.SEED)
    pos, rpy = tt.poses(T, tt.SEED, spiky=True)
    rot = Rotation.from_euler("xyz", rpy)
    runs = tt.plateau_runs(T)
    assert runs
    q = []
    for s, n in runs:
        v = time[s]
        q += [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), v - 0.004, v + 0.004]
    q = np.array(q)
    Rm, p = R.slerp_pose(time, pos, rpy, q)
    for i, t in enumerate(q):
        k = -1
        for j in range(T):            # last sample with time <= t
            if time[j] <= t:
                k = j
        k = min(max(k, 0), T - 2)
        dt = time[k + 1] - time[k]
        al = 0.0 if dt == 0 else min(max((t - time[k]) / dt, 0.0), 1.0)
        rel = (rot[k].inv() * rot[k + 1]).as_rotvec()
        wantR = (rot[k] * Rotation.from_rotvec(al * rel)).as_matrix()
        wantp = pos[k] + al * (pos[k + 1] - pos[k])
        assert np.abs(Rm[i] - wantR).max() <= 1e-13, (i, t, k)
        assert np.abs(p[i] - wantp).max() <= 16 * np.finfo(np.float64).eps * np.abs(pos).max()
    for r, (s, n) in enumerate(runs):
        last = s + n - 1
        assert np.array_equal(p[5 * r], pos[last])                       # at the repeated timestamp
        assert np.abs(Rm[5 * r] - R.euler_xyz_matrix(rpy[last])).max() <= 1e-13
        # just before it: segment s - 1 at alpha = 1 - 2e-14, i.e. the run's first sample to within
        # that fraction of the step (5 m steps, Theta <= 1.45)
        assert np.abs(p[5 * r + 1] - pos[s]).max() <= 1e-10
        assert np.abs(Rm[5 * r + 1] - R.euler_xyz_matrix(rpy[s])).max() <= 1e-12
        assert not np.array_equal(pos[s], pos[last])
