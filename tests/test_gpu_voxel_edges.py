"""The voxel-grid filter on the device where tests/test_gpu_voxel.py stops short (builders and their
conditions: tests/voxeledges.py, asserted in tests/test_voxel_edges_cpu.py): the rank scan past its first
pass of 256 chunks, probe chains that wrap around the table and are hundreds of slots long, per-voxel
sums past 2^53, hundreds of frames with runs of empty ones and the naming of a refused point among them,
random grids, rebuilds on one context, rows wider than four columns, a source batch with a time column,
and the phase timing.  Everything is compared bit for bit with the NumPy restatement of tests/voxel.py."""
import contextlib
import gc

import numpy as np
import pytest

import voxel as V
import voxeledges as E
from test_gpu_voxel import bits, both_sources, check_cloud

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def own_context(mc):
    """A context of the test's own, so that the session's gpu_ctx is not left holding the test's scratch.
    It is closed once the test has passed and nothing made in it is alive; after a failure, whose
    traceback may hold a batch, it goes when the last such object has gone (their finalizers hold it)."""
    ctx = mc.Context(0)
    yield ctx
    gc.collect()
    ctx.close()


def upload(ctx, counts, rows, with_time=False):
    b = ctx.batch(counts, with_time=with_time)
    b.upload_columns(*[rows[:, c].astype(np.float32) for c in range(4)])
    return b


# ---- A: the rank scan across passes ------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.SCAN_SIZES)
def test_rank_scan_across_passes(gpu_ctx, n):
    """256 chunks (one pass of k_vox_scan), 257 (the carry into a one-chunk pass) and 516 (three passes, a
    partial last pass, a 17-point last chunk), with first appearances in every pass; 11 uneven frames."""
    counts, rows, h = E.scan_case(n)
    _, cloud = both_sources(gpu_ctx, counts, rows, h, what=f"scan, n = {n}", want=E.scan_want(n))
    cloud.close()


# ---- B: long and wrapping probe chains ---------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(E.PROBE_CASES)))
def test_probe_chains_wrap_and_go_far(gpu_ctx, which):
    """Every key's first slot is in the last 96 of 4096 (the last 4 of 64) slots: the chains cross from slot
    ``mask`` to slot 0 and most lanes walk hundreds of taken slots."""
    counts, rows, h, k = E.probe_case(which)
    want, _ = both_sources(gpu_ctx, counts, rows, h, what=f"probe, {E.PROBE_CASES[which]}")
    assert len(want["rows"]) == len(set(V.pack(k).tolist()))


# ---- C: sums past 2^53 -------------------------------------------------------------------------------------
def test_sums_past_2_53(gpu_ctx, mc):
    """Two voxels of 2 200 001 points each whose sums are odd and beyond 2^53: the finaliser's double(S)
    rounds, to even.  Rows only (float32 cannot hold these values)."""
    rows, h, o = E.big_sum_case()
    cloud = mc.voxel_downsample(rows, h, o, context=gpu_ctx)
    try:
        check_cloud(cloud, E.big_sum_want(), "sums past 2^53")
    finally:
        cloud.close()


# ---- D: many frames, runs of empty frames, refusal naming --------------------------------------------------
@pytest.mark.parametrize("one_voxel", [True, False])
def test_frame_runs(gpu_ctx, one_voxel):
    rows, h = E.frame_run_rows(one_voxel)
    both_sources(gpu_ctx, E.frame_run_counts(), rows, h, what=f"910 frames, one voxel {one_voxel}")


def test_refusals_are_named_among_empty_frames(gpu_ctx, mc):
    ctx = gpu_ctx
    counts = E.frame_run_counts()
    good, h = E.frame_run_rows(False)
    places = E.refusal_places()

    def refuse(at, what):
        """at: {dense index: refused row}; the lowest is named, by frame and point and by row"""
        rows = np.array(good)
        for dense, row in at.items():
            rows[dense] = row
        f, i, dense = min(places.values(), key=lambda p: p[2] if p[2] in at else np.inf)
        assert dense == min(at)
        with pytest.raises(V.Refused) as e:
            V.downsample(rows, h)
        assert e.value.index == dense, what
        with pytest.raises(ValueError, match=rf"frame {f}, point {i} "):
            ctx.voxel_downsample(upload(ctx, counts, rows), h)
        with pytest.raises(ValueError, match=rf"row {dense} "):
            mc.voxel_downsample(rows, h, context=ctx)

    for k, (name, (f, i, dense)) in enumerate(places.items()):
        refuse({dense: E.REFUSED_ROWS[k]}, name)
    first, last, lone, p255, p256, p512 = (p[2] for p in places.values())
    refuse({p256: E.REFUSED_ROWS[0], last: E.REFUSED_ROWS[1]}, "two at once")
    refuse({lone: E.REFUSED_ROWS[3], p512: E.REFUSED_ROWS[2]}, "two at once, the lower in the one-point frame")
    refuse({first: E.REFUSED_ROWS[4], last: E.REFUSED_ROWS[5]}, "the first and the last point")


def test_batch_of_empty_frames(gpu_ctx):
    cloud = gpu_ctx.voxel_downsample(gpu_ctx.batch([0, 0, 0]), 0.1)
    b = check_cloud(cloud, V.downsample(np.zeros((0, 4)), 0.1), "three empty frames")
    assert cloud.n_voxels == 0 and cloud.rows().shape == (0, 4) and cloud.keys().shape == (0, 3) and b.n_points == 0


# ---- E: grid fuzz ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", E.FUZZ_SEEDS)
def test_grid_fuzz(gpu_ctx, mc, seed):
    h, o, rows64, rows32 = E.fuzz_case(seed)
    both_sources(gpu_ctx, E.FUZZ_COUNTS, rows32, h, o, what=f"fuzz {seed}: h {h}, origin {o}")
    check_cloud(mc.voxel_downsample(rows64, h, o, context=gpu_ctx), V.downsample(rows64, h, o), f"fuzz {seed}, float64")


# ---- F: rebuilds on one context ----------------------------------------------------------------------------
def test_rebuild_sequence_on_one_context(mc):
    """Large, small, empty, full-table, refused and other-source builds on a context of its own: the
    scratch is kept while it is large enough and only the current build's slots are reset."""
    with own_context(mc) as ctx:
        rng = np.random.default_rng(60)
        clouds = []

        def build(source, counts, rows, h, o):
            want = V.downsample(rows, h, o)
            cloud = ctx.voxel_downsample(upload(ctx, counts, rows), h, o) if source == "batch" else \
                mc.voxel_downsample(rows, h, o, context=ctx)
            void()
            check_cloud(cloud, want, f"rebuild {len(clouds)}: {len(rows)} points ({source})")
            clouds.append(cloud)
            return want

        def void():
            for old in clouds:
                for emit in (old.rows, old.point_counts, old.keys, old.batch):
                    with pytest.raises(ValueError):
                        emit()

        frames = [10000, 10001, 9999, 10003, 9998, 10000, 10000]
        centre = rng.integers(-40, 40, (9000, 3))
        big = E.f32(np.column_stack([(centre[rng.integers(0, 9000, 70001)] + rng.uniform(0.05, 0.95, (70001, 3))) * 0.2,
                                     rng.uniform(0, 1, 70001)]))
        assert len(build("batch", frames, big, 0.2, (0.0, 0.0, 0.0))["rows"]) > 5000
        build("rows", None, E.f32(rng.uniform(-2, 2, (5, 4))), 0.3, (0.1, -0.2, 0.05))
        assert len(build("rows", None, np.zeros((0, 4)), 0.7, (1.0, 2.0, 3.0))["rows"]) == 0
        own, _ = E.own_voxel_rows(2049, 0.125, (16.0, -8.0, 4.0))
        assert len(build("batch", [2000, 0, 49], own, 0.125, (16.0, -8.0, 4.0))["rows"]) == 2049
        bad = E.f32(rng.uniform(-2, 2, (700, 4)))
        bad[333, 1] = np.nan
        with pytest.raises(ValueError, match=r"row 333 "):
            mc.voxel_downsample(bad, 0.45, (0.0, 0.5, 0.0), context=ctx)
        void()
        buf = ctx.device_buffer(64)
        assert ctx.lib.mc_voxel_emit_f64(ctx.handle, buf.ptr, None, None) == mc._lib.MC_ERR_STATE
        buf.close()
        build("rows", None, E.f32(rng.uniform(-1, 1, (33, 4))), 0.05, (-0.3, 0.0, 0.3))
        clouds[-1].close()
        void()
        utm = (5.0e6, 4.4e5, 100.0)
        build("batch", [100, 200], E.f32(rng.normal(0, 3, (300, 4)) + [*utm, 0.0]), 1.5, utm)


@pytest.mark.parametrize("n", E.OWN_SIZES)
def test_own_voxel_small_sizes(gpu_ctx, n):
    """M = n around the four-voxel lanes of k_vox_emit_batch and the block ends, in the 64- and 128-slot tables."""
    rows, keys = E.own_voxel_rows(n)
    want, _ = both_sources(gpu_ctx, [n], rows, 0.25, what=f"own voxel, n = {n}")
    assert np.array_equal(want["keys"], keys)


# ---- G: layout variants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [6, 7])
def test_rows_wider_than_four_columns(gpu_ctx, mc, ld):
    rng = np.random.default_rng(ld)
    rows = np.empty((3001, ld))
    rows[:, :4] = rng.uniform(-4, 4, (3001, 4))
    rows[:, 4:] = rng.choice([np.nan, np.inf, -np.inf, 1e308], (3001, ld - 4))
    check_cloud(mc.voxel_downsample(rows, 0.3, (0.1, 0.2, 0.3), context=gpu_ctx),
                V.downsample(rows[:, :4], 0.3, (0.1, 0.2, 0.3)), f"rows of {ld} columns")


def test_source_batch_with_a_time_column(gpu_ctx):
    counts = [700, 0, 257, 1300]
    rng = np.random.default_rng(70)
    rows = E.f32(rng.uniform(-4, 4, (sum(counts), 4)))
    want = V.downsample(rows, 0.3)
    timed = upload(gpu_ctx, counts, rows, with_time=True)
    timed.upload_time(rng.integers(-2 ** 31, 2 ** 31, sum(counts)))
    assert timed.with_time
    got = check_cloud(gpu_ctx.voxel_downsample(timed, 0.3), want, "batch with a time column")
    timed_cols = np.stack(got.download_columns(), axis=1)
    plain = check_cloud(gpu_ctx.voxel_downsample(upload(gpu_ctx, counts, rows), 0.3), want, "the same points, four columns")
    assert np.array_equal(bits(timed_cols), bits(np.stack(plain.download_columns(), axis=1)))


# ---- H: the phase timing -----------------------------------------------------------------------------------
def test_read_timing_voxel(mc):
    """mc_timing_read_voxel: the event time of the four phases since the last read, and the timed regions."""
    with own_context(mc) as ctx:
        rows = np.random.default_rng(80).uniform(-20, 20, (50000, 4))
        phases = ("insert_ms", "rank_ms", "accumulate_ms", "finalise_ms")

        def run():
            cloud = mc.voxel_downsample(rows, 0.3, context=ctx)
            cloud.rows()
            return ctx.read_timing_voxel()

        off = run()
        assert off["regions"] == 0 and all(off[p] == 0.0 for p in phases)
        ctx.timing(True)
        t = run()
        print("voxel phases (ms):", {p: float(t[p]) for p in phases}, "regions", t["regions"])
        assert all(np.isfinite(t[p]) and t[p] >= 0.0 for p in phases)
        assert t["insert_ms"] > 0.0 and t["rank_ms"] > 0.0 and t["accumulate_ms"] > 0.0
        assert t["regions"] == 4           # one build: insert, rank, accumulate; one emit: finalise
        again = ctx.read_timing_voxel()
        assert again["regions"] == 0 and all(again[p] == 0.0 for p in phases)
        ctx.timing(False)
        off = run()
        assert off["regions"] == 0 and all(off[p] == 0.0 for p in phases)
