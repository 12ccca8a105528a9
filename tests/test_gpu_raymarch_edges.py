"""The ray-march scanner (csrc/raymarch.hpp) on its decision edges and past 256 rays, against the numpy
restatement of tests/raymarch.py (which equals the reference's recordings exactly).

Every scene uses R = R_inv = identity and an explicit direction table: R @ d is d exactly in any
summation order, so the expected decisions rest on nothing BLAS- or machine-dependent and every
discrete result, and under the identity every coordinate, is asserted bit for bit.

* edge scenes: per ray one point just outside the 0.1 hit radius at an earlier step and one just
  inside it at a later one, adjacent doubles of one coordinate: a fused multiply-add in ray_sample, a
  fused sum of squares in ray_exact, a sqrt that is not correctly rounded or a radius off by 1e-13
  changes rays here (tests/test_raymarch_cpu.py counts how many under numpy emulations of each);
* tie scenes: two points of one object within a coordinate ulp of the same distance, or exact
  duplicates, in different LDS tiles and, by the chunking, in the same or in different scene chunks;
* scene sizes around the 512-point tile, ray counts around the 256-lane workgroup across frames, and
  frames of 441 rays whose hits span two 256-ray groups and two 256-point batch blocks.
"""
import numpy as np
import pytest

import raymarch as RM
from raymarch import abi_count, abi_rows

pytestmark = pytest.mark.gpu
BAR = 3e-15      # the float64 bar of CSIM paths, as tests/test_gpu_raymarch.py


def want_hits(marches):
    return np.stack([np.column_stack([m["step"], m["object"], m["index"]]) for m in marches])


def count_with_grids(mc, ctx, grids, *args, **kw):
    """abi_count under each mc_set_launch cap of ``grids`` (0: the default chunking)."""
    out = []
    for i, g in enumerate(grids):
        ctx.set_max_grid(g)
        try:
            out.append(abi_count(mc, ctx, *args, set_scene=(i == 0), **kw))
        finally:
            ctx.set_max_grid(0)
    return out


@pytest.mark.parametrize("origin", RM.EDGE_ORIGINS, ids=["zero", "metres", "utm"])
def test_edge_decisions_match_reference_predicate(mc, gpu_ctx, origin):
    """Step, object and index of all 288 rays equal the restatement's under the default grid and in one
    scene chunk; the float64 rows under R_inv = identity without noise are hit_point - origin bit for bit."""
    sc = RM.edge_scene(origin, RM.EDGE_SEED)
    m = RM.march_scene(sc)
    assert np.array_equal(m["step"], sc["k2"]) and np.array_equal(m["scene_index"], sc["scene_in"])
    want = want_hits([m])
    for counts, hits, Rinv in count_with_grids(mc, gpu_ctx, (0, 1), {}, sc["origin"], RM.IDENTITY, sc["objects"],
                                               dirs=sc["dirs"], steps=sc["steps"]):
        wrong = np.flatnonzero((hits[0] != want[0]).any(axis=1))
        early = int((hits[0, :, 0] == sc["k1"]).sum())
        assert wrong.size == 0, (f"{wrong.size} of 288 rays differ ({early} accept the point just outside, "
                                 f"{int((hits[0, :, 0] < 0).sum())} miss the point just inside)")
        assert counts.tolist() == [288]
    assert np.array_equal(Rinv[0], np.eye(3))
    rows = abi_rows(mc, gpu_ctx, Rinv, None, 288)
    hit_point = sc["origin"] + sc["dirs"] * sc["steps"][sc["k2"]][:, None]
    assert np.array_equal(hit_point, m["hit_point"])
    assert np.array_equal(rows[:, :3], hit_point - sc["origin"])
    assert np.array_equal(rows[:, 3], m["intensity"]) and np.array_equal(rows[:, 4], np.arange(288.0))


@pytest.mark.parametrize("seed", RM.TIE_SEEDS)
def test_near_ties_and_duplicates_across_tiles_and_chunks(mc, gpu_ctx, seed):
    """The key's distance and index components: A and B of a ray are two LDS tiles apart, in different
    scene chunks under the default chunking (one tile per chunk), in one chunk under mc_set_launch(1)
    and in chunks of four tiles under mc_set_launch(48).  The three results are byte-equal and equal
    the restatement's."""
    sc = RM.tie_scene(seed)
    m = RM.march_scene(sc)
    assert np.array_equal(m["scene_index"], sc["winner"])
    want = want_hits([m])
    got = [hits for _, hits, _ in count_with_grids(mc, gpu_ctx, (0, 1, 48), {}, sc["origin"], RM.IDENTITY,
                                                   sc["objects"], dirs=sc["dirs"], steps=sc["steps"])]
    for hits in got:
        wrong = (hits[0] != want[0]).any(axis=1)
        assert not wrong.any(), (f"{int(wrong.sum())} of 288 rays differ: {int((wrong & sc['duplicate']).sum())} exact "
                                 f"duplicates, {int((wrong & ~sc['duplicate'] & sc['nearer']).sum())} with B just nearer")
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


@pytest.mark.parametrize("E", RM.TILE_SIZES)
def test_scene_sizes_around_the_lds_tile(mc, gpu_ctx, E):
    """Scenes of one point, of one tile +- 1 and of two tiles (+ 1) for case B's 7 rays: the hits are the
    scene's first and last point, the rest is filler behind the sensor."""
    objs = RM.tile_scene(E)
    m = RM.march_frame(np.zeros(3), RM.IDENTITY, RM.CFG_B, objs)
    want = want_hits([m])
    assert (want[0, :, 0] >= 0).sum() == min(E, 2)
    for counts, hits, _ in count_with_grids(mc, gpu_ctx, (0, 1), RM.CFG_B, np.zeros(3), RM.IDENTITY, objs):
        assert np.array_equal(hits, want) and counts.tolist() == [min(E, 2)]
    rows = abi_rows(mc, gpu_ctx, np.eye(3)[None], None, min(E, 2))
    hit = m["step"] >= 0
    assert np.array_equal(rows[:, :3], m["hit_point"][hit]) and np.array_equal(rows[:, 3], m["intensity"][hit])


@pytest.mark.parametrize("n_rays", RM.RAY_COUNTS)
def test_ray_counts_around_a_workgroup(mc, gpu_ctx, n_rays):
    """Three frames of n_rays rays in one count call: a 256-lane group of k_ray_count spans frames at
    every alignment (gr / n_rays, gr % n_rays), k_ray_emit's ray loop runs one to three times."""
    D, steps, objs = RM.count_scene(n_rays)
    ms = [RM.march_frame(o, RM.IDENTITY, {}, objs, dirs=D, steps=steps) for o in RM.COUNT_ORIGINS]
    want = want_hits(ms)
    ori = np.zeros((3, 3))
    counts, hits, Rinv = abi_count(mc, gpu_ctx, {}, RM.COUNT_ORIGINS, ori, objs, dirs=D, steps=steps)
    assert np.array_equal(hits, want)
    assert np.array_equal(counts, (want[:, :, 0] >= 0).sum(axis=1)) and counts.min() >= 1
    rows = abi_rows(mc, gpu_ctx, Rinv, None, int(counts.sum()))
    ref = np.concatenate([np.column_stack([(m["hit_point"] - o)[m["step"] >= 0], m["intensity"][m["step"] >= 0],
                                           np.flatnonzero(m["step"] >= 0)]) for m, o in zip(ms, RM.COUNT_ORIGINS)])
    assert np.array_equal(rows, ref)


@pytest.fixture(scope="module")
def block_case():
    objs, rays = RM.block_scene()
    flat = RM.flatten(objs)
    ms = [RM.march_frame(o, RM.IDENTITY, RM.CFG_BLOCK, objs, flat) for o in RM.BLOCK_ORIGINS]
    return objs, rays, ms


def test_frames_past_one_block(mc, gpu_ctx, block_case):
    """points_per_frame = 20000 (441 rays) through LiDARSimulator: six frames with 257, 0, 441, 1, 256 and
    255 hits, so k_ray_emit's ray loop runs twice with hits in both groups, a frame's points and text
    sums span two 256-point blocks and padding sits between frames."""
    objs, rays, ms = block_case
    cfg = dict(RM.CFG_BLOCK)
    pos, ori = RM.BLOCK_ORIGINS, np.zeros((6, 3))
    H = sum(RM.BLOCK_HITS)
    for f, m in enumerate(ms):
        assert np.array_equal(np.flatnonzero(m["step"] >= 0), rays[f]) and (not len(rays[f]) or m["edge_margin"] >= 0.0299)
    sim = mc.LiDARSimulator(dict(cfg), context=gpu_ctx)
    assert len(sim.directions()) == 441
    counts, rows = sim.scan_rows(pos, ori, objs)
    assert counts.tolist() == list(RM.BLOCK_HITS)
    assert np.array_equal(sim.hits(6, 441), want_hits(ms))
    rng = np.random.RandomState(RM.cfg_of(cfg)["random_seed"])
    want = np.concatenate([RM.emit_frame(m, o, RM.IDENTITY, cfg, RM.noise_of(rng, n, cfg), 0)["rows"]
                           for m, o, n in zip(ms, pos, RM.BLOCK_HITS)])
    assert np.array_equal(rows, want)                                   # bitwise under the identity
    assert np.array_equal(rows[:, 4], np.concatenate(rays))             # rays in order
    assert want[:, 3].min() == 0.0 and want[:, 3].max() == 255.0        # the scene takes both clips
    end = np.random.RandomState(RM.cfg_of(cfg)["random_seed"])
    end.standard_normal(4 * H)
    for a, b in ((sim.rng.get_state(), end.get_state()), (rng.get_state(), end.get_state())):
        assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]

    sim = mc.LiDARSimulator(dict(cfg), context=gpu_ctx)                  # the same generator again
    starts = 1_000_000_000 + 100_000_000 * np.arange(6, dtype=np.int64)
    batch, st = sim.scan_frames(pos, ori, objs, starts, with_pcd_len=True)
    assert np.array_equal(batch.counts, counts) and np.array_equal(st, starts) and batch.with_time
    assert batch.pcd_len_current()
    cols = np.column_stack(batch.download_columns())
    assert np.array_equal(cols, rows[:, :4].astype(np.float32))
    t_ns = batch.download_time()
    assert np.array_equal(t_ns, rows[:, 4].astype(np.int64) * 1000) and t_ns.max() == 440_000
    plain = gpu_ctx.batch(counts)
    plain.upload_columns(*batch.download_columns())
    assert mc.codecs.encode_pcd_batch(batch) == mc.codecs.encode_pcd_batch(plain)
    assert batch.pcd_len_current()
    ts = np.arange(0, 2_000_000_000, 5_000_000, dtype=np.int64)
    gyro = np.column_stack([0.3 * np.sin(ts * 2e-9), 0.2 * np.cos(ts * 3e-9), 0.5 + 0.1 * np.sin(ts * 1e-9)])
    gpu_ctx.set_imu(ts, gyro)
    out = gpu_ctx.deskew(batch, mode="imu").download_aos()
    assert out.shape == (H, 4) and np.isfinite(out).all() and np.array_equal(out[:, 3], cols[:, 3].astype(np.float64))

    # the same hits through mc_ray_emit_f64 with a rotation that is not the identity
    _, Rinv = RM.rotations([0.3, -0.2, 1.1])
    Rinv = np.ascontiguousarray(np.broadcast_to(Rinv, (6, 3, 3)))
    got = abi_rows(mc, gpu_ctx, Rinv, None, H)
    offs = np.concatenate([[0], np.cumsum(counts)])
    for f, (m, o) in enumerate(zip(ms, pos)):
        hit = m["step"] >= 0
        ref = np.array([Rinv[f] @ (p - o) for p in m["hit_point"][hit]]).reshape(-1, 3)
        sc = np.linalg.norm(o) + RM.steps_of(cfg)[m["step"][hit]]
        err = np.abs(got[offs[f]:offs[f + 1], :3] - ref).max(axis=1) if hit.any() else np.zeros(0)
        assert (err <= BAR * sc).all(), (f, float((err / sc).max()))
        assert np.array_equal(got[offs[f]:offs[f + 1], 3], m["intensity"][hit])
        assert np.array_equal(got[offs[f]:offs[f + 1], 4], rays[f])
