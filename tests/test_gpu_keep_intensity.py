"""The kernels that leave the intensity column alone (k_deskew_points<.., KEEPI = true>) and the host rule
that chooses them (csrc/batch_state.hpp holds_intensity_of, csrc/mcdeskew.hip begin_steps): every call path
byte-identical to the same calls on a second context with Context.keep_intensity(False), which always
launches the full kernels, and the held state gone after every writer of either batch.

Every case is a scenario: a function of a context that makes its own batches, runs its calls and takes a
snapshot of the output after each — the four columns (and t_ns where the output has one) as raw bits, the
batch checksum, and Batch.holds_intensity_of.  The scenario runs on both contexts; the snapshots must be
equal one by one, the held states must be what the scenario says, and the output's intensity must be the
input's bit for bit.  A new output batch is first filled with other intensities (its memory may be that of
an earlier output of the same shape, already holding the right bytes), and every writer in the staleness
cases changes the intensity values, so a launch that wrongly kept the column leaves wrong bytes.

One batch shape: frames of 1, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 0 and 4100 points — a last
group of 1 .. 3 valid points, the block (256), sub-tile (1024) and tile (2048) edges from both sides, an
empty frame, a frame of more than two tiles.  Intensities are distinct per point, with a NaN and a -0.0
among them.  Times: 1 us per point from a per-frame t0 (evenly timed: the kernels that generate t_ns), and
the same with one point off its ramp (the loading kernels).

Writers not exercised here: the LVX and LAS decoders, the ray and scan emits and the two gathers.  They
report through the same batch_columns_written(kWrotePoints) as the text decoder and the voxel emit that
are (tests/test_gpu_batch_state.py runs each of them into an existing batch).

Tried once against a library whose BatchState::points_written() does not move the points version: 10 of
the 37 cases fail (test_steps, test_writers_end_the_state, test_text_decoder_into_input,
test_voxel_emit_into_input: every case with a writer between two deskews of a pair).
"""
import ctypes
from ctypes import c_int64

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = np.array([1, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 0, 4100], np.int64)
OFF = np.concatenate([[0], np.cumsum(COUNTS)])
F, N = len(COUNTS), int(COUNTS.sum())
TICK_NS = 5_000_000                                    # pose and IMU sample spacing
N_TAB = 401                                            # 2 s of table
TIMES = 0.2 + 0.1 * np.arange(F)
STARTS = np.round(TIMES * 1e9).astype(np.int64)
MODES = ("pose_slerp", "imu")
KINDS = ("ramp", "off_ramp")
CASES = [(k, m) for k in KINDS for m in MODES]


def _tables():
    rng = np.random.default_rng(41)
    time = np.arange(N_TAB) * (TICK_NS * 1e-9)
    pos = np.cumsum(rng.normal(0, 0.05, (N_TAB, 3)), axis=0) + np.array([10.0, -20.0, 2.0])
    rpy = np.column_stack([0.05 * np.sin(1.3 * time), 0.04 * np.cos(0.7 * time), 0.6 * np.sin(0.5 * time)])
    return (time, pos, rpy), (np.arange(N_TAB, dtype=np.int64) * TICK_NS, rng.normal(0, 0.3, (N_TAB, 3)))


TRAJ, IMU = _tables()


def times_of(kind, counts=COUNTS):
    t = np.concatenate([(f + 1) * 777 + 1000 * np.arange(int(n), dtype=np.int64) for f, n in enumerate(counts)]
                       + [np.zeros(0, np.int64)])
    if kind == "off_ramp":
        t[-2] += 1        # one point of the last frame: the whole batch takes the loading kernels
    return t


def xyz_of(key, n=N):
    rng = np.random.default_rng(key)
    return (rng.integers(-30_000, 30_000, (n, 3)) / 1000.0).astype(np.float32)


def intensity_of(key, n=N):
    """n distinct float32 values in an order of their own per key, with a NaN and a -0.0 where n allows."""
    v = (np.random.default_rng(1000 + key).permutation(n) + 1 + 100_000 * key).astype(np.float32)
    if n > 8:
        v[n // 3] = np.float32("nan")
        v[n // 2] = np.float32(-0.0)
    return v


def fill(b, key, kind="ramp"):
    """Points and intensities of `key`, and (a batch with a time column) the times of `kind`."""
    p = xyz_of(key, b.n_points)
    b.upload_aos(np.column_stack([p, np.zeros(b.n_points)]).astype(np.float64))   # (the AoS stager)
    b.upload_columns(intensity=intensity_of(key, b.n_points))
    if b.with_time:
        b.upload_time(times_of(kind, b.counts))
    return b


def source(c, key, kind, counts=COUNTS, **kw):
    b = fill(c.batch(counts, with_time=True, **kw), key, kind)
    b.set_frame_times(TIMES[:len(counts)])
    b.set_frame_starts(STARTS[:len(counts)])
    return b


def output(c, counts=COUNTS, **kw):
    """An output batch holding other points and other intensities than any input."""
    o = c.batch(counts, **kw)
    fill(o, 77)
    return o


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def snap(what, o, src, held):
    """(label, raw column bits, checksum bits, held state) of o; asserts the state and, independently of
    the other context, that o's intensity is src's."""
    cols = o.download_columns()
    assert np.array_equal(u32(cols[3]), u32(src.download_columns()[3])), f"{what}: the intensity is not the input's"
    got = o.holds_intensity_of(src)
    assert got == held, f"{what}: holds_intensity_of is {got}"
    raw = [u32(c) for c in cols]
    if o.with_time:
        raw.append(u32(o.download_time()))
    return what, np.stack(raw), np.ascontiguousarray(o.checksum()).view(np.uint64), got


@pytest.fixture(scope="module")
def pair(mc, gpu_ctx):
    """(the suite's context with the keeping kernels allowed, a second one that never launches them)."""
    ref = mc.Context(0)
    for c in (gpu_ctx, ref):
        c.set_trajectory(*TRAJ)
        c.set_imu(*IMU)
        c.time_rule(True)
    gpu_ctx.keep_intensity(True)
    ref.keep_intensity(False)
    yield gpu_ctx, ref
    ref.close()


def both(pair, scenario):
    """scenario(context) -> snapshots, on both contexts: equal one by one.  Returns the first context's."""
    got, want = scenario(pair[0]), scenario(pair[1])
    assert [s[0] for s in got] == [s[0] for s in want]
    for g, w in zip(got, want):
        assert np.array_equal(g[1], w[1]), f"{g[0]}: columns differ from the full kernels'"
        assert np.array_equal(g[2], w[2]), f"{g[0]}: checksum differs"
        assert g[3] == w[3], f"{g[0]}: held state differs"
    return got


# ---- call sequences ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,mode", CASES)
def test_three_calls(pair, kind, mode):
    """mc_deskew three times: full, keeping (fused with the next call's prep), keeping on speculated tables."""
    def scenario(c):
        b, o = source(c, 1, kind), output(c)
        assert not o.holds_intensity_of(b)
        return [snap(f"call {k}", c.deskew(b, o, mode=mode), b, True) for k in range(3)]
    got = both(pair, scenario)
    for s in got[1:]:
        assert np.array_equal(s[1], got[0][1]), s[0]


@pytest.mark.parametrize("kind,mode", CASES)
def test_steps(pair, kind, mode):
    """mc_deskew_steps with 1, 2 and 5 steps on a fresh pair (step 0 full, the rest keeping) and again on
    the pair it leaves held (all keeping)."""
    def scenario(c):
        b, out = source(c, 2, kind), []
        for n in (1, 2, 5):
            o = output(c)
            out.append(snap(f"fresh n={n}", c.deskew_steps(b, o, n, mode=mode), b, True))
            out.append(snap(f"held n={n}", c.deskew_steps(b, o, n, mode=mode), b, True))
            fill(o, 78)   # a write between two runs: the next run starts in full again
            assert not o.holds_intensity_of(b)
            out.append(snap(f"written n={n}", c.deskew_steps(b, o, n, mode=mode), b, True))
        return out
    got = both(pair, scenario)
    for s in got[1:]:
        assert np.array_equal(s[1], got[0][1]), s[0]


@pytest.mark.parametrize("kind", KINDS)
def test_relative(pair, kind):
    """mc_deskew_relative with two references, between two global deskews, on one pair."""
    def scenario(c):
        b, o = source(c, 3, kind), output(c)
        out = [snap("end", c.deskew(b, o, mode="pose_slerp", reference="end"), b, True),
               snap("keyframe", c.deskew(b, o, mode="pose_slerp", reference=0.75), b, True),
               snap("global", c.deskew(b, o, mode="pose_slerp"), b, True),
               snap("start", c.deskew(b, o, mode="pose_slerp", reference="start"), b, True)]
        o2 = output(c)
        out.append(snap("keyframe, fresh pair", c.deskew(b, o2, mode="pose_slerp", reference=0.75), b, True))
        return out
    got = both(pair, scenario)
    assert np.array_equal(got[1][1], got[4][1])
    assert not np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("kind,mode", CASES)
def test_in_place(pair, kind, mode):
    """out == in keeps from the first call and records nothing."""
    def scenario(c):
        b = source(c, 4, kind)
        out = [snap("first", c.deskew(b, b, mode=mode), b, False), snap("second", c.deskew(b, b, mode=mode), b, False)]
        out.append(snap("steps", c.deskew_steps(b, b, 3, mode=mode), b, False))
        if mode == "pose_slerp":
            out.append(snap("relative", c.deskew(b, b, mode=mode, reference="end"), b, False))
        # the deskewed input into another batch: a fresh pair like any other
        out.append(snap("then out of place", c.deskew(b, output(c), mode=mode), b, True))
        assert np.array_equal(b.download_time(), times_of(kind))
        return out
    both(pair, scenario)


@pytest.mark.parametrize("kind,mode", CASES)
def test_output_with_time_column(pair, kind, mode):
    """copy_t: t_ns is passed through by the keeping kernels as by the full ones."""
    def scenario(c):
        b, o = source(c, 5, kind), output(c, with_time=True)
        out = [snap(f"call {k}", c.deskew(b, o, mode=mode), b, True) for k in range(2)]
        out.append(snap("steps", c.deskew_steps(b, o, 2, mode=mode), b, True))
        assert np.array_equal(o.download_time(), times_of(kind))
        return out
    both(pair, scenario)


@pytest.mark.parametrize("kind,mode", CASES)
def test_output_with_pcd_len(mc, pair, kind, mode):
    """An output that keeps PCD text sums stays on the kernels that write them: the sums are current after
    every call and the encoder's bytes are those of the other context."""
    texts = []

    def scenario(c):
        # (the other cases' intensities hold a NaN, which has no PCD text: finite columns for this one)
        b, o = source(c, 6, kind), c.batch(COUNTS, with_pcd_len=True)
        b.upload_columns(intensity=np.arange(1, N + 1, dtype=np.float32))
        o.upload_columns(intensity=np.arange(N, 0, -1, dtype=np.float32))
        out = []
        for k in range(2):
            out.append(snap(f"call {k}", c.deskew(b, o, mode=mode), b, True))
            assert o.pcd_len_current()
            texts.append(mc.codecs.encode_pcd_batch(o))
        out.append(snap("steps", c.deskew_steps(b, o, 3, mode=mode), b, True))
        assert o.pcd_len_current()
        texts.append(mc.codecs.encode_pcd_batch(o))
        return out
    both(pair, scenario)
    assert len(texts) == 6 and all(t == texts[0] for t in texts[1:])


@pytest.mark.parametrize("kind,mode", CASES)
def test_tune_order_then_deskew(pair, kind, mode):
    """mc_tune_order's launches follow the rule (the first in full on a fresh pair) and leave the pair held."""
    def scenario(c):
        b, out = source(c, 7, kind), []
        for rounds, launches in ((1, 1), (2, 3)):
            o = output(c)
            c.tune_order(b, o, mode=mode, launches=launches, rounds=rounds)
            out.append(snap(f"tuned {rounds}x{launches}", o, b, True))
            out.append(snap(f"deskew after {rounds}x{launches}", c.deskew(b, o, mode=mode), b, True))
            c.tune_order(b, o, mode=mode, launches=launches, rounds=rounds)
            out.append(snap(f"tuned again {rounds}x{launches}", o, b, True))
        return out
    got = both(pair, scenario)
    for s in got[1:]:
        assert np.array_equal(s[1], got[0][1]), s[0]


@pytest.mark.parametrize("kind", KINDS)
def test_mode_changes(pair, kind):
    """SLERP -> IMU -> frame -> SLERP on one pair: every mode passes the column through, so it stays held."""
    def scenario(c):
        b, o = source(c, 8, kind), output(c)
        return [snap(f"{k} {m}", c.deskew(b, o, mode=m), b, True)
                for k, m in enumerate(("pose_slerp", "imu", "frame", "pose_slerp", "frame", "imu"))]
    got = both(pair, scenario)
    assert np.array_equal(got[0][1], got[3][1]) and np.array_equal(got[1][1], got[5][1])


# ---- staleness -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_writers_end_the_state(pair, mode):
    def scenario(c):
        b, o = source(c, 10, "ramp"), output(c)
        out = [snap("first", c.deskew(b, o, mode=mode), b, True)]

        def again(what):
            assert not o.holds_intensity_of(b), what
            out.append(snap(what, c.deskew(b, o, mode=mode), b, True))
            out.append(snap(what + ", kept", c.deskew(b, o, mode=mode), b, True))

        b.upload_columns(intensity=intensity_of(11))
        again("column upload to in")
        o.upload_columns(intensity=intensity_of(12))
        again("column upload to out")
        b.upload_columns(x=xyz_of(13)[:, 0])     # (any point column moves the version)
        again("x upload to in")
        b.synth(seed=5, frame_id_base=77)
        b.upload_time(times_of("ramp"))          # (synth's own times reach past this test's table)
        again("synth on in")
        fill(b, 14)
        again("AoS stager into in")
        c.transform_affine(source(c, 15, "ramp"), o, mats=np.hstack([np.eye(3), [[1.0], [2.0], [3.0]]]))
        assert not np.array_equal(u32(o.download_columns()[3]), u32(b.download_columns()[3]))
        again("affine into out")
        b2 = source(c, 16, "ramp")
        out.append(snap("another input", c.deskew(b2, o, mode=mode), b2, True))
        again("the first input again")
        # the input into another output, then a write of the input: neither output holds it
        o2 = output(c)
        out.append(snap("second output", c.deskew(b, o2, mode=mode), b, True))
        assert o.holds_intensity_of(b) and o2.holds_intensity_of(b)
        b.upload_columns(intensity=intensity_of(17))
        assert not o2.holds_intensity_of(b)
        again("input written after two outputs")
        out.append(snap("second output again", c.deskew(b, o2, mode=mode), b, True))
        # in place moves the input's version too
        c.deskew(b, b, mode=mode)
        again("input deskewed in place")
        # a frame-mode deskew of another input
        out.append(snap("frame mode, another input", c.deskew(b2, o, mode="frame"), b2, True))
        again("after frame mode")
        return out
    both(pair, scenario)


@pytest.mark.parametrize("mode", MODES)
def test_new_batches_match_nothing(pair, mode):
    """A batch created after another of the same shape was closed (it may get the same memory, and with it
    the old bytes) neither holds anything nor is held."""
    def scenario(c):
        b, o = source(c, 20, "ramp"), output(c)
        out = [snap("first", c.deskew(b, o, mode=mode), b, True)]
        o.close()
        o = c.batch(COUNTS)
        assert not o.holds_intensity_of(b)
        o.upload_columns(intensity=intensity_of(21))
        out.append(snap("new output", c.deskew(b, o, mode=mode), b, True))
        b.close()
        b = source(c, 22, "ramp")
        assert not o.holds_intensity_of(b)
        out.append(snap("new input", c.deskew(b, o, mode=mode), b, True))
        out.append(snap("new input, kept", c.deskew(b, o, mode=mode), b, True))
        return out
    both(pair, scenario)


@pytest.mark.parametrize("mode", MODES)
def test_text_decoder_into_input(mc, pair, mode):
    """mc_text_decode_batch into an input whose column an output holds."""
    ing, ptr = mc.ingest, mc._lib.ptr
    t = times_of("ramp")
    rows = np.column_stack([xyz_of(31).astype(np.float64), np.arange(N) % 251 + 0.5, np.repeat(STARTS, COUNTS) + t])
    body = "".join(f"{r[0]:.3f},{r[1]:.3f},{r[2]:.3f},{r[3]:.1f},{int(r[4])}\n" for r in rows).encode()

    def scenario(c):
        b, o = source(c, 30, "ramp"), output(c)
        out = [snap("first", c.deskew(b, o, mode=mode), b, True)]
        d_text = ing._upload_file(c, body)
        used, bad = np.zeros(F, np.int64), c_int64()
        mc._lib.check(c.lib.mc_text_decode_batch(c.handle, ord(","), 5, d_text.ptr, len(body), b.handle,
                                                 ptr(STARTS, c_int64), ptr(used, c_int64), ctypes.byref(bad)),
                      "text_decode_batch")
        d_text.close()
        assert not o.holds_intensity_of(b)
        assert np.array_equal(b.download_columns()[3], rows[:, 3].astype(np.float32))
        out.append(snap("decoded", c.deskew(b, o, mode=mode), b, True))
        out.append(snap("decoded, kept", c.deskew(b, o, mode=mode), b, True))
        return out
    both(pair, scenario)


@pytest.mark.parametrize("mode", MODES)
def test_voxel_emit_into_input(mc, pair, mode):
    """mc_voxel_emit_batch into a one-frame input whose column an output holds."""
    pts = np.column_stack([xyz_of(41).astype(np.float64), np.arange(N) % 199 + 1.0])

    def scenario(c):
        src = c.batch(COUNTS)
        src.upload_aos(pts)
        cloud = c.voxel_downsample(src, 2.0)
        one = np.array([cloud.n_voxels], np.int64)
        assert 1024 < one[0] <= N
        b, o = source(c, 40, "ramp", counts=one), output(c, counts=one)
        out = [snap("first", c.deskew(b, o, mode=mode), b, True)]
        mc._lib.check(c.lib.mc_voxel_emit_batch(c.handle, b.handle), "voxel_emit_batch")
        assert not o.holds_intensity_of(b)
        assert not np.array_equal(u32(b.download_columns()[3]), u32(intensity_of(40, int(one[0]))))
        out.append(snap("emitted", c.deskew(b, o, mode=mode), b, True))
        out.append(snap("emitted, kept", c.deskew(b, o, mode=mode), b, True))
        return out
    both(pair, scenario)


def test_switch_and_query_arguments(mc, pair):
    """The switch takes effect on the next launch either way; the query refuses NULL."""
    c = pair[0]
    b, o = source(c, 50, "ramp"), output(c)
    want = snap("on", c.deskew(b, o, mode="pose_slerp"), b, True)
    c.keep_intensity(False)
    try:
        off = snap("off", c.deskew(b, o, mode="pose_slerp"), b, True)   # (the state is kept either way)
    finally:
        c.keep_intensity(True)
    on = snap("on again", c.deskew(b, o, mode="pose_slerp"), b, True)
    assert np.array_equal(off[1], want[1]) and np.array_equal(on[1], want[1])
    assert c.lib.mc_batch_holds_intensity_of(None, b.handle) < 0
    assert c.lib.mc_batch_holds_intensity_of(o.handle, None) < 0
