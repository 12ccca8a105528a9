"""The ray-march scanner on the GPU (k_ray_count / k_ray_merge / k_ray_emit, csrc/raymarch.hpp)
against the reference's recorded runs (tests/golden/csim_raymarch.npz) and, where there is no golden,
against the numpy restatement of tests/raymarch.py.

Bars.  Everything discrete is exact: each ray's step, object and point index, the hit counts, the
truncated intensities, timestamps, rings and tags (the fixtures keep every evaluated distance at least
1e-9 from the 0.1 hit radius and every point's range at least 1e-6 from the tag threshold, far above
float64 rounding at these coordinates).  Coordinates: the device forms the world direction R @ d in
numpy's one-row order itself, so a sample origin + direction * d_k may differ from the reference's by
the rounding of that product times d_k plus one rounding of the sum; the project's float64 bar for
CSIM paths is 3e-15 * scale, here scale = |origin| + d_k, the magnitude
of the terms that are summed.  The same absolute bar holds for the sensor-frame point R_inv (hit -
position), a rotation of that difference.
"""
from ctypes import c_double, c_int64

import numpy as np
import pytest

import raymarch as RM
from conftest import golden
from raymarch import abi_count, abi_rows, ptr as _p

pytestmark = pytest.mark.gpu
BAR = 3e-15


@pytest.fixture(scope="module")
def gold():
    return golden("csim_raymarch.npz")


@pytest.fixture(scope="module")
def frames():
    return RM.golden_frames()


def scales(cfg, position, steps_hit):
    return np.linalg.norm(position) + RM.steps_of(cfg)[steps_hit]


def check_points(cfg, rows_xyz, intensity, ray, stamp, gold, name, position):
    """rows of one frame against the golden LiDARPoint fields; returns whether x, y, z were bitwise."""
    hit = gold[f"{name}_step"] >= 0
    assert np.array_equal(ray, np.flatnonzero(hit)), name
    want = np.column_stack([gold[f"{name}_{k}"] for k in "xyz"])
    sc = scales(cfg, position, gold[f"{name}_step"][hit])
    err = np.abs(rows_xyz - want).max(axis=1) if len(want) else np.zeros(0)
    assert (err <= BAR * sc).all(), (name, float((err / sc).max()))
    assert np.array_equal(np.asarray(intensity, np.int64), gold[f"{name}_intensity"]), name
    assert np.array_equal(stamp + ray * 1000, gold[f"{name}_timestamp"]), name
    assert np.array_equal(ray % 16, gold[f"{name}_ring"]), name
    norm = np.array([np.linalg.norm(r) for r in rows_xyz]).reshape(-1)
    assert np.array_equal((norm > RM.cfg_of(cfg)["range_max"] * 0.9).astype(np.int64), gold[f"{name}_tag"]), name
    return bool(np.array_equal(rows_xyz, want))


@pytest.mark.parametrize("case", ["A", "B0", "B1", "C"])
def test_c_abi_matches_reference(mc, gpu_ctx, gold, frames, case):
    names = RM.CASES[case]
    cfg, _, _, objs, _ = frames[names[0]]
    pos = np.array([frames[n][1] for n in names])
    ori = np.array([frames[n][2] for n in names])
    counts, hits, Rinv = abi_count(mc, gpu_ctx, cfg, pos, ori, objs)
    for f, n in enumerate(names):
        for c, k in enumerate(("step", "object", "index")):
            assert np.array_equal(hits[f, :, c], gold[f"{n}_{k}"]), (n, k)
        assert counts[f] == int((gold[f"{n}_step"] >= 0).sum())
    offs = np.concatenate([[0], np.cumsum(counts)])
    H = int(offs[-1])
    # hit points: with R_inv = I and no noise the rows are hit_point - position (1 x + 0 y + 0 z is x)
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(3), (len(names), 3, 3)))
    rel = abi_rows(mc, gpu_ctx, eye, None, H)
    rng = np.random.RandomState(RM.cfg_of(cfg)["random_seed"])
    rows = abi_rows(mc, gpu_ctx, Rinv, RM.noise_of(rng, H, cfg), H)
    bitwise = []
    for f, n in enumerate(names):
        s = slice(offs[f], offs[f + 1])
        hit = gold[f"{n}_step"] >= 0
        want = gold[f"{n}_hit_point"][hit] - pos[f]
        sc = scales(cfg, pos[f], gold[f"{n}_step"][hit])
        err = np.abs(rel[s, :3] - want).max(axis=1) if hit.any() else np.zeros(0)
        assert (err <= BAR * sc).all(), (n, float((err / sc).max()))
        assert np.array_equal(rel[s, 3], gold[f"{n}_raw_intensity"][hit]), n
        bitwise.append(check_points(cfg, rows[s, :3], rows[s, 3], rows[s, 4].astype(np.int64), frames[n][4], gold, n,
                                    pos[f]) and np.array_equal(rel[s, :3], want))
    print(f"case {case}: hit and sensor points bitwise equal to the reference: {bitwise}")


@pytest.mark.parametrize("case", ["A", "B0", "B1"])
def test_simulate_scan_matches_reference(mc, gpu_ctx, gold, frames, case):
    names = RM.CASES[case]
    cfg = frames[names[0]][0]
    sim = mc.LiDARSimulator(dict(cfg), context=gpu_ctx)
    for n in names:
        _, pos, ori, objs, stamp = frames[n]
        pts = sim.simulate_scan(pos, ori, objs, stamp)
        assert all(isinstance(p, mc.LiDARPoint) for p in pts)
        xyz = np.array([[p.x, p.y, p.z] for p in pts]).reshape(-1, 3)
        ray = (np.array([p.timestamp for p in pts], np.int64) - stamp) // 1000
        check_points(cfg, xyz, [p.intensity for p in pts], ray, stamp, gold, n, pos)
        assert [p.ring for p in pts] == gold[f"{n}_ring"].tolist() and [p.tag for p in pts] == gold[f"{n}_tag"].tolist()
    if case == "A":   # the simulator's generator was consumed exactly as the reference's
        st = sim.rng.get_state()
        assert np.array_equal(st[1], gold["A_rng_keys"]) and st[2] == int(gold["A_rng_pos"])
        assert st[3] == int(gold["A_rng_has_gauss"]) and st[4] == float(gold["A_rng_cached"])


def test_simulate_lidar_frames_matches_reference(mc, gpu_ctx, gold, frames):
    """A's three poses as the knots of a trajectory (np.interp returns a knot's value exactly)."""
    pos, ori = RM.POSES_A
    t = np.append(np.arange(0, 0.25, 0.1), 0.25)
    mount = 0.5
    z = pos[:, 2] - mount
    assert np.array_equal(z + mount, pos[:, 2])
    ext = lambda v: np.append(v, v[-1])
    traj = {"time": t, "x": ext(pos[:, 0]), "y": ext(pos[:, 1]), "z": ext(z), "roll": ext(ori[:, 0]),
            "pitch": ext(ori[:, 1]), "yaw": ext(ori[:, 2])}
    sim = mc.LiDARSimulator(dict(RM.CFG_A), context=gpu_ctx)
    out = sim.simulate_lidar_frames(traj, frames["A0"][3], mount)
    assert [d["frame_id"] for d in out] == [0, 1, 2] and [d["timestamp"] for d in out] == list(RM.STAMPS_A)
    for f, (d, n) in enumerate(zip(out, RM.CASES["A"])):
        assert np.array_equal(d["sensor_position"], pos[f]) and np.array_equal(d["sensor_orientation"], ori[f])
        assert d["frame_duration_ns"] == 100_000_000
        pts = d["points"]
        xyz = np.array([[p.x, p.y, p.z] for p in pts]).reshape(-1, 3)
        ray = (np.array([p.timestamp for p in pts], np.int64) - d["timestamp"]) // 1000
        check_points(RM.CFG_A, xyz, [p.intensity for p in pts], ray, d["timestamp"], gold, n, pos[f])
    st = sim.rng.get_state()
    assert np.array_equal(st[1], gold["A_rng_keys"]) and st[2] == int(gold["A_rng_pos"])


@pytest.fixture(scope="module")
def case_d():
    objs = RM.scene_d()
    pos, ori = RM.poses_d()
    flat = RM.flatten(objs)
    ms = [RM.march_frame(p, o, RM.CFG_D, objs, flat) for p, o in zip(pos, ori)]
    return objs, pos, ori, ms


def test_many_chunks_and_objects_against_restatement(mc, gpu_ctx, case_d):
    """40 frames x 224 rays on 50 000 points of 65 objects (one empty, one without intensity): the scene
    spans many LDS tiles and scene chunks, every ray's candidates come from several objects spread over
    the whole scene, so the per-chunk keys must merge in key order.  Byte-equal when run again and
    when mc_set_launch caps the grid (another chunking)."""
    objs, pos, ori, ms = case_d
    assert len(objs) == 65 and sum(len(o) for o in objs) == 50_000 and len(pos) == 40
    assert min(m["edge_margin"] for m in ms) >= 1e-9
    want = np.stack([np.column_stack([m["step"], m["object"], m["index"]]) for m in ms])
    assert 0.25 <= np.mean(want[:, :, 0] >= 0) <= 0.9 and len(np.unique(want[:, :, 1])) > 40
    counts, hits, _ = abi_count(mc, gpu_ctx, RM.CFG_D, pos, ori, objs)
    assert np.array_equal(hits, want)
    assert np.array_equal(counts, (want[:, :, 0] >= 0).sum(axis=1))
    _, again, _ = abi_count(mc, gpu_ctx, RM.CFG_D, pos, ori, objs, set_scene=False)
    assert again.tobytes() == hits.tobytes()
    gpu_ctx.set_max_grid(48)
    try:
        _, small, _ = abi_count(mc, gpu_ctx, RM.CFG_D, pos, ori, objs, set_scene=False)
    finally:
        gpu_ctx.set_max_grid(0)
    assert small.tobytes() == hits.tobytes()


def test_scan_frames_feeds_imu_deskew(mc, gpu_ctx, frames):
    """scan_frames on A: the batch's columns are the float64 rows rounded once to float32, t_ns is
    1000 * ray index, the PCD text lengths are current, and Context.deskew(mode="imu") takes it."""
    from oracle import restatement as R
    objs = frames["A0"][3]
    pos, ori = RM.POSES_A
    starts = np.array(RM.STAMPS_A, np.int64) + 1_000_000_000
    sim = mc.LiDARSimulator(dict(RM.CFG_A), context=gpu_ctx)
    counts, rows = sim.scan_rows(pos, ori, objs)
    sim = mc.LiDARSimulator(dict(RM.CFG_A), context=gpu_ctx)      # the same generator again
    batch, st = sim.scan_frames(pos, ori, objs, starts, with_pcd_len=True)
    assert np.array_equal(batch.counts, counts) and np.array_equal(st, starts) and batch.with_time
    assert batch.pcd_len_current()
    cols = np.column_stack(batch.download_columns())
    assert np.array_equal(cols, rows[:, :4].astype(np.float32))
    t_ns = batch.download_time()
    assert np.array_equal(t_ns, rows[:, 4].astype(np.int64) * 1000)
    # the text lengths the emit kernel summed are those the encoder measures on a plain batch
    plain = gpu_ctx.batch(counts)
    plain.upload_columns(*batch.download_columns())
    assert mc.codecs.encode_pcd_batch(batch) == mc.codecs.encode_pcd_batch(plain)
    assert batch.pcd_len_current()
    ts = np.arange(0, 2_000_000_000, 5_000_000, dtype=np.int64)
    gyro = np.column_stack([0.3 * np.sin(ts * 2e-9), 0.2 * np.cos(ts * 3e-9), 0.5 + 0.1 * np.sin(ts * 1e-9)])
    gpu_ctx.set_imu(ts, gyro)
    out = gpu_ctx.deskew(batch, mode="imu").download_aos()
    offs = np.concatenate([[0], np.cumsum(counts)])
    for f in range(3):
        s = slice(offs[f], offs[f + 1])
        p = cols[s, :3].astype(np.float64)
        ref = R.compensate_arrays(p, starts[f] + t_ns[s].astype(np.int64), starts[f], ts, gyro)
        sc = np.linalg.norm(p, axis=1)
        assert (np.abs(out[s, :3] - ref).max(axis=1) <= 1e-6 * sc).all()
        assert np.array_equal(out[s, 3], cols[s, 3].astype(np.float64))


def test_emit_after_scene_change_is_refused(mc, gpu_ctx, frames):
    cfg, pos, ori, objs, _ = frames["B0"]
    counts, _, Rinv = abi_count(mc, gpu_ctx, cfg, pos, ori, objs)
    assert counts.sum() > 0
    other = frames["B1"][3]
    c2, r2 = mc.raymarch.scene_rows(other)
    mc._lib.check(gpu_ctx.lib.mc_set_ray_scene(gpu_ctx.handle, len(c2), _p(c2, c_int64), _p(r2, c_double), 4))
    rows = np.zeros((int(counts.sum()), 5))
    rc = gpu_ctx.lib.mc_ray_emit_f64(gpu_ctx.handle, _p(Rinv, c_double), None, _p(rows, c_double))
    assert rc == mc._lib.MC_ERR_STATE
    b = gpu_ctx.batch(counts, with_time=True)
    assert gpu_ctx.lib.mc_ray_emit(gpu_ctx.handle, b.handle, _p(Rinv, c_double), None) == mc._lib.MC_ERR_STATE
    # a new count on the new scene is accepted again
    counts, _, Rinv = abi_count(mc, gpu_ctx, cfg, pos, ori, other, set_scene=False)
    assert abi_rows(mc, gpu_ctx, Rinv, None, int(counts.sum())).shape == (7, 5)


def test_empty_frames(mc, gpu_ctx, frames):
    """An all-miss frame next to a frame with hits, and scenes without a point (no objects, only
    empty objects): empty frames, no noise drawn."""
    objs = frames["A0"][3]
    sim = mc.LiDARSimulator(dict(RM.CFG_A), context=gpu_ctx)
    pos = np.array([RM.POSES_A[0][0], [500.0, 500.0, 50.0]])
    ori = np.array([RM.POSES_A[1][0], [0.0, 0.0, 0.0]])
    counts, rows = sim.scan_rows(pos, ori, objs)
    assert counts[0] > 0 and counts[1] == 0 and len(rows) == counts[0]
    assert sim.hits(2, 224)[1].max() == -1
    before = sim.rng.get_state()
    for scene in ([], [np.zeros((0, 4)), np.zeros((0, 3))]):
        assert sim.simulate_scan(pos[0], ori[0], scene, 0) == []
        batch, _ = sim.scan_frames(pos, ori, scene, [0, 1])
        assert batch.n_points == 0 and batch.counts.tolist() == [0, 0]
    after = sim.rng.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    with pytest.raises(ValueError):
        sim.simulate_scan(pos[0], ori[0], [np.zeros((4, 2))], 0)
    with pytest.raises(ValueError):
        sim.scan_rows(pos, ori[:1], objs)
