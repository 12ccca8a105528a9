"""The evenly-timed rule on the device (csrc/time_rule.hpp, k_trange, k_deskew_points<.., RULE = true>):
the span pass's decisions against the NumPy restatement (tests/timerule.py), and every per-point call
path with the rule on bit-identical, on all valid points, to the same call with the loading kernels forced
(Context.time_rule(False)), which is held to the 1e-5 gate of oracle/restatement.py.

One batch shape for everything: frames of 0, 1 .. 5, 255 .. 257, 1023 .. 1025, 2047 .. 2049 and 4100
points — the group (4), block (256), sub-tile (1024) and tile (2048) edges of the layout — with empty frames
at both ends.  The pose and IMU tables tick every 5 ms, so the step dt of a frame's ramp chooses the path of
a 1024-point sub-tile: 1 us/point spans at most 2 segments (records in SGPRs), 50 us/point 3 .. 64 (the LDS
window), 500 us/point more than 64 (per-point search).  Each case asserts its class from the table.
"""
import numpy as np
import pytest

import relative as V
import timerule as TR
from conftest import assert_scaled_close
from oracle import restatement as R
from oracle import synth

pytestmark = pytest.mark.gpu

COUNTS = np.array([0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4100, 0])
OFF = np.concatenate([[0], np.cumsum(COUNTS)])
F = len(COUNTS)
TICK_NS = 5_000_000                                  # pose and IMU sample spacing
N_TAB = 1201                                         # 6 s of table
TIMES = 0.2 + 0.1 * np.arange(F)                     # frame times (s)
STARTS = (np.round(TIMES * 1e9)).astype(np.int64)    # frame starts (ns)
SUB = 1024                                           # points per sub-tile
# dt (ns per point) -> the path a full sub-tile takes, and the segments it may span
DT = {"sgpr": 1000, "lds": 50_000, "search": 500_000, "negative": -1000}
CLASS = {"sgpr": (1, 2), "lds": (3, 64), "search": (65, 10**9), "negative": (1, 2)}


def _tables():
    rng = np.random.default_rng(11)
    time = np.arange(N_TAB) * (TICK_NS * 1e-9)
    pos = np.cumsum(rng.normal(0, 0.05, (N_TAB, 3)), axis=0) + np.array([10.0, -20.0, 2.0])
    rpy = np.column_stack([0.05 * np.sin(1.3 * time), 0.04 * np.cos(0.7 * time), 0.6 * np.sin(0.5 * time)])
    tr = {"time": time, "position_gps": pos, "orientation_imu": rpy}
    ts = (np.arange(N_TAB, dtype=np.int64) * TICK_NS)
    gyro = rng.normal(0, 0.3, (N_TAB, 3))
    return tr, ts, gyro


TR_TAB, IMU_TS, GYRO = _tables()


def _rows(key):
    rng = np.random.default_rng(key)
    n = int(COUNTS.sum())
    return np.column_stack([rng.uniform(-60, 60, (n, 3)), rng.uniform(0, 1, n)]).astype(np.float32).astype(np.float64)


ROWS = _rows(3)


def ramps(kind):
    """Every frame a ramp of the case's step; t0 differs per frame, negative in some."""
    dt = DT[kind]
    out = []
    for f, n in enumerate(COUNTS):
        t0 = (f % 3 - 1) * 777 + (0 if dt >= 0 else (int(n) - 1) * -dt)
        out.append(TR.ramp(t0, dt, int(n)))
    return out


def segments_per_subtile(t_frames, mode):
    """Largest count of table segments one sub-tile of any frame spans (the kernel's window width)."""
    worst = 0
    for f, t in enumerate(t_frames):
        for s in range(0, len(t), SUB):
            c = t[s:s + SUB].astype(np.int64)
            if mode == "pose_slerp":
                q = TIMES[f] + np.array([c.min(), c.max()]) * 1e-9
                k = np.clip(np.searchsorted(TR_TAB["time"], q, "right") - 1, 0, N_TAB - 2)
            else:
                k = np.clip(np.searchsorted(IMU_TS, STARTS[f] + np.array([c.min(), c.max()]), "right") - 1, 0, N_TAB - 1)
            worst = max(worst, int(k[1] - k[0]) + 1)
    return worst


def expected_rule(t_frames):
    r = [TR.rule_of(t) for t in t_frames]
    return (np.array([x[0] for x in r]), np.array([x[1] for x in r], np.int32), np.array([x[2] for x in r], np.int32))


def assert_rule(b, t_frames, what=""):
    even, t0, dt = b.time_rule()
    we, w0, wd = expected_rule(t_frames)
    assert np.array_equal(even, we), (what, even, we)
    assert np.array_equal(t0, w0) and np.array_equal(dt, wd), what
    return even


_ORACLE = {}


def oracle(rows, t_frames, mode, key):
    """Per-point float64 oracle and scale of the whole batch, computed once per key."""
    if key in _ORACLE:
        return _ORACLE[key]
    ref, sc = np.zeros((len(rows), 3)), np.zeros(len(rows))
    for f, n in enumerate(COUNTS):
        if n == 0:
            continue
        s = slice(OFF[f], OFF[f + 1])
        p, t = rows[s, :3], t_frames[f]
        if mode == "pose_slerp":
            ref[s] = R.deskew_pose_slerp(p, t, TIMES[f], TR_TAB)
            _, tt = R.slerp_pose(TR_TAB["time"], TR_TAB["position_gps"], TR_TAB["orientation_imu"], TIMES[f] + t * 1e-9)
            sc[s] = np.linalg.norm(p, axis=1) + np.linalg.norm(tt, axis=1)
        else:
            ref[s] = R.compensate_arrays(p, STARTS[f] + t.astype(np.int64), STARTS[f], IMU_TS, GYRO)
            sc[s] = np.linalg.norm(p, axis=1)
    _ORACLE[key] = (ref, sc)
    return ref, sc


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    gpu_ctx.set_trajectory(TR_TAB["time"], TR_TAB["position_gps"], TR_TAB["orientation_imu"])
    gpu_ctx.set_imu(IMU_TS, GYRO)
    gpu_ctx.time_rule(True)
    yield gpu_ctx
    gpu_ctx.time_rule(True)


def make_batch(ctx, rows, t_frames, **kw):
    b = ctx.batch(COUNTS, with_time=True, **kw)
    b.upload_aos(rows)
    b.upload_time(np.concatenate(t_frames))
    b.set_frame_times(TIMES)
    b.set_frame_starts(STARTS)
    return b


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def both(ctx, fn):
    """fn() with the loading kernels forced, then with the rule on."""
    ctx.time_rule(False)
    try:
        off = fn()
    finally:
        ctx.time_rule(True)
    return off, fn()


# ---- decisions --------------------------------------------------------------------------------

def test_decisions_ramps_and_mixed(ctx):
    for kind in DT:
        t = ramps(kind)
        even = assert_rule(make_batch(ctx, ROWS, t), t, kind)
        assert even.all()
    # the near misses, one frame at a time and all at once: (frame, index)
    misses = [(9, 1), (13, 2047), (14, 1024), (15, 2048), (15, 4099), (15, 1)]
    base = ramps("sgpr")
    b = make_batch(ctx, ROWS, base)
    for f, i in misses:
        t = list(base)
        t[f] = TR.off_by_one(base[f], i)
        b.upload_time(np.concatenate(t))
        even = assert_rule(b, t, f"miss at frame {f} index {i}")
        assert not even[f] and even.sum() == F - 1
    t = list(base)
    for f, i in misses[:4]:
        t[f] = TR.off_by_one(base[f], i)
    t[6] = TR.synth_times(255)                                          # floor(i 1e8 / n): no ramp
    t[3] = TR.synth_times(3)                                            # ... a ramp
    t[8] = TR.wrap32(np.arange(257, dtype=np.int64) * (2**30 + 12345))  # wraps: evenly timed as stored
    b.upload_time(np.concatenate(t))
    even = assert_rule(b, t, "mixed")
    assert list(np.flatnonzero(~even)) == [6, 9, 13, 14, 15]
    b.upload_time(np.concatenate(base))
    assert assert_rule(b, base, "restored").all()


# ---- outputs ----------------------------------------------------------------------------------

CASES = [(k, m) for k in DT for m in ("pose_slerp", "imu")]


@pytest.mark.parametrize("kind,mode", CASES)
def test_rule_on_is_bit_identical(mc, ctx, kind, mode):
    t = ramps(kind)
    w = segments_per_subtile(t, mode)
    lo, hi = CLASS[kind]
    assert lo <= w <= hi, f"{kind}/{mode}: a sub-tile spans {w} segments, outside its class [{lo}, {hi}]"
    tcat = np.concatenate(t)
    b = make_batch(ctx, ROWS, t)
    assert assert_rule(b, t).all()
    ref, sc = oracle(ROWS, t, mode, (kind, mode))

    def gate(got, what):
        assert np.array_equal(got[:, 3], ROWS[:, 3]), what
        assert_scaled_close(got[:, :3], ref, sc, what=f"{kind}/{mode} {what}")

    # Context.deskew, three identical calls: the second launches fused with the next call's prep, the
    # third finds its tables ready
    def calls():
        o = ctx.batch(COUNTS)
        return [ctx.deskew(b, o, mode=mode).download_aos() for _ in range(3)]
    off, on = both(ctx, calls)
    gate(off[0], "deskew, loading kernel")
    for k in range(3):
        assert np.array_equal(bits(off[k]), bits(off[0])) and np.array_equal(bits(on[k]), bits(off[0])), f"call {k}"
    want = bits(off[0])

    # deskew_steps, 3 steps
    off, on = both(ctx, lambda: ctx.deskew_steps(b, ctx.batch(COUNTS), 3, mode=mode).download_aos())
    assert np.array_equal(bits(off), want) and np.array_equal(bits(on), want), "deskew_steps"

    # an output that keeps PCD text sums, and mc_deskew_pcd: the texts (laid out by the block sums) too
    def pcd():
        o = ctx.batch(COUNTS, with_pcd_len=True)
        ctx.deskew(b, o, mode=mode)
        assert o.pcd_len_current()
        a = mc.codecs.encode_pcd_batch(o)
        o2 = ctx.batch(COUNTS)
        return o.download_aos(), a, mc.codecs.deskew_pcd_frames(b, o2, mode=mode), o2.download_aos()
    off, on = both(ctx, pcd)
    for k in (0, 3):
        assert np.array_equal(bits(off[k]), want) and np.array_equal(bits(on[k]), want), "pcd outputs"
    assert off[1] == on[1] and off[2] == on[2] and on[1] == on[2], "pcd texts"

    # tune_order: one round ends on the XCD-contiguous order, two rounds on the dealt one
    for rounds in (1, 2):
        def tune():
            o = ctx.batch(COUNTS)
            ctx.tune_order(b, o, mode=mode, launches=1, rounds=rounds)
            return o.download_aos()
        off, on = both(ctx, tune)
        assert np.array_equal(bits(off), want) and np.array_equal(bits(on), want), f"tune_order rounds={rounds}"

    # an output with a time column (t_ns passed through), then used as the next input
    def chain():
        o = ctx.batch(COUNTS, with_time=True)
        ctx.deskew(b, o, mode=mode)
        o.set_frame_times(TIMES)
        o.set_frame_starts(STARTS)
        first, tt = o.download_aos(), o.download_time()
        even = o.time_rule()[0]
        return first, tt, even, ctx.deskew(o, ctx.batch(COUNTS), mode=mode).download_aos()
    off, on = both(ctx, chain)
    assert np.array_equal(bits(off[0]), want) and np.array_equal(bits(on[0]), want)
    assert np.array_equal(off[1], tcat) and np.array_equal(on[1], tcat), "t_ns not passed through"
    assert off[2].all() and on[2].all()
    assert np.array_equal(bits(off[3]), bits(on[3])), "second deskew of the chain"
    ref2, sc2 = oracle(off[0], t, mode, (kind, mode, "chain"))
    assert_scaled_close(off[3][:, :3], ref2, sc2, what=f"{kind}/{mode} chain")

    # the sensor frame at a reference time (SLERP only)
    if mode == "pose_slerp":
        for reference in ("end", 0.75):
            off, on = both(ctx, lambda: ctx.deskew(b, ctx.batch(COUNTS), mode=mode, reference=reference).download_aos())
            assert np.array_equal(bits(off), bits(on)), f"reference={reference}"
        t_ref = ctx.reference_times(b, 0.75)
        for f in (5, 10, 15):   # (off is the reference=0.75 output of the loading kernel)
            s = slice(OFF[f], OFF[f + 1])
            r = V.relative_oracle(ROWS[s, :3], t[f], TIMES[f], t_ref[f], TR_TAB)
            assert_scaled_close(off[s, :3], r, V.relative_scale(ROWS[s, :3], t[f], TIMES[f], t_ref[f], TR_TAB),
                                what=f"{kind} relative frame {f}")

    # in place (last: it overwrites the input's points)
    b2 = make_batch(ctx, ROWS, t)
    spare = [b, b2]
    off, on = both(ctx, lambda: (lambda x: ctx.deskew(x, x, mode=mode).download_aos())(spare.pop()))
    assert np.array_equal(bits(off), want) and np.array_equal(bits(on), want), "in place"
    assert np.array_equal(b.download_time(), tcat) and np.array_equal(b2.download_time(), tcat)


def test_mixed_batch_keeps_loading_kernel_results(ctx):
    """One frame off its ramp: the batch takes the loading kernel; outputs follow the stored times."""
    t = ramps("lds")
    t[15] = TR.off_by_one(t[15], 2048)
    b = make_batch(ctx, ROWS, t)
    assert not assert_rule(b, t)[15]
    for mode in ("pose_slerp", "imu"):
        off, on = both(ctx, lambda: ctx.deskew(b, ctx.batch(COUNTS), mode=mode).download_aos())
        assert np.array_equal(bits(off), bits(on))
        ref, sc = oracle(ROWS, t, mode, ("mixed", mode))
        assert_scaled_close(on[:, :3], ref, sc, what=f"mixed {mode}")


# ---- staleness --------------------------------------------------------------------------------

def _non_ramp(t):
    """Frame 15 far off its ramp (a deskew with the old ramp's times would miss the gate)."""
    u = list(t)
    v = u[15].copy()
    v[1000:] += 40_000_000          # 40 ms later: eight table ticks
    v[4099] -= 15_000_000
    u[15] = v
    return u


@pytest.mark.parametrize("mode", ["pose_slerp", "imu"])
def test_rule_goes_stale_with_the_time_column(ctx, mode):
    t = ramps("sgpr")
    bad = _non_ramp(t)
    b = make_batch(ctx, ROWS, t)
    o = ctx.batch(COUNTS)

    def run(rows, times, key, what, expect_even):
        even = assert_rule(b, times, what)
        assert bool(even.all()) == expect_even, what
        got = ctx.deskew(b, o, mode=mode).download_aos()
        ref, sc = oracle(rows, times, mode, key)
        assert_scaled_close(got[:, :3], ref, sc, what=f"{mode} {what}")
        ctx.time_rule(False)
        try:
            assert np.array_equal(bits(ctx.deskew(b, o, mode=mode).download_aos()), bits(got)), what
        finally:
            ctx.time_rule(True)
        return got

    first = run(ROWS, t, ("stale", mode, "ramp"), "ramp", True)
    # the oracle tells the two time columns apart: the test would see a deskew that kept the old ramp
    ref_bad, sc_bad = oracle(ROWS, bad, mode, ("stale", mode, "bad"))
    assert (np.abs(first[:, :3] - ref_bad).max(axis=1) / sc_bad).max() > 1e-4

    # a column upload
    b.upload_time(np.concatenate(bad))
    run(ROWS, bad, ("stale", mode, "bad"), "upload non-ramp", False)
    b.upload_time(np.concatenate(t))
    assert np.array_equal(bits(run(ROWS, t, ("stale", mode, "ramp"), "upload ramp", True)), bits(first))

    # synth: floor(i 1e8 / n) — no ramp for most of these counts — and new points
    b.synth(seed=5, frame_id_base=77)
    x, y, z, inten, ts = synth.synth_batch(COUNTS, seed=5, frame_id_base=77)
    srows = np.column_stack([x, y, z, inten]).astype(np.float64)
    st = [ts[OFF[f]:OFF[f + 1]].astype(np.int32) for f in range(F)]
    even = expected_rule(st)[0]
    assert even[[3, 4, 5, 7]].all() and not even[[6, 8, 9, 10, 15]].any()
    run(srows, st, ("stale", mode, "synth"), "synth", False)
    b.upload_time(np.concatenate(t))
    run(srows, t, ("stale", mode, "synth ramp"), "ramp after synth", True)

    # the AoS stager: new points, the time column (and the rule) stay
    rows2 = _rows(8)
    b.upload_aos(rows2)
    run(rows2, t, ("stale", mode, "stager"), "stager", True)

    # t_ns passed through from another batch (copy_t): this batch's time column is rewritten
    src_bad, src_ok = make_batch(ctx, ROWS, bad), make_batch(ctx, ROWS, t)
    ctx.deskew(src_bad, b, mode=mode)
    assert np.array_equal(b.download_time(), np.concatenate(bad))
    run(b.download_aos(), bad, ("stale", mode, "copy_t bad"), "copy_t non-ramp", False)
    ctx.deskew(src_ok, b, mode=mode)
    run(b.download_aos(), t, ("stale", mode, "copy_t ok"), "copy_t ramp", True)
