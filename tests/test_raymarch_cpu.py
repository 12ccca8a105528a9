"""The ray-march scanner's contract on the CPU (no GPU): tests/raymarch.py's numpy restatement
against the reference's recorded runs (tests/golden/csim_raymarch.npz), the host-table rules the
Python layer relies on, the fixtures' own conditions, and the kernel's per-pair core
(csrc/raymarch_core.hpp) compiled for the host under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import re
import shutil

import numpy as np
import pytest

import hostbuild
import raymarch as RM
from conftest import golden, pkg

ROOT = hostbuild.ROOT
NEW_SYMBOLS = ("mc_set_ray_scene", "mc_ray_count", "mc_ray_hits", "mc_ray_emit", "mc_ray_emit_f64",
               "mc_timing_read_ray")


@pytest.fixture(scope="module")
def gold():
    return golden("csim_raymarch.npz")


@pytest.fixture(scope="module")
def frames():
    return RM.golden_frames()


@pytest.fixture(scope="module")
def marched(frames):
    return {name: RM.march_frame(pos, ori, cfg, objs) for name, (cfg, pos, ori, objs, _) in frames.items()}


@pytest.fixture(scope="module")
def edge_scenes():
    return [RM.edge_scene(o, RM.EDGE_SEED) for o in RM.EDGE_ORIGINS]


@pytest.fixture(scope="module")
def tie_scenes():
    return [RM.tie_scene(s) for s in RM.TIE_SEEDS]


@pytest.fixture(scope="module")
def edge_marched(edge_scenes):
    return [RM.march_scene(s) for s in edge_scenes]


@pytest.fixture(scope="module")
def tie_marched(tie_scenes):
    return [RM.march_scene(s) for s in tie_scenes]


def test_fixture_conditions(gold, frames):
    """Edge margin >= 1e-9 and tag margin >= 1e-6 in every case, 25-75 % of the rays hit in A and
    C, and the scene builders still build the scenes the reference scanned."""
    for case in RM.CASES:
        assert float(gold[f"{case}_edge_margin"]) >= 1e-9, case
        assert float(gold[f"{case}_tag_margin"]) >= 1e-6, case
    for case in ("A", "C"):
        steps = np.concatenate([gold[f"{n}_step"] for n in RM.CASES[case]])
        assert len(steps) == 224 * len(RM.CASES[case])
        assert 0.25 <= np.mean(steps >= 0) <= 0.75, (case, np.mean(steps >= 0))
    assert len(gold["B0_step"]) == 7
    for name, (_, _, _, objs, _) in frames.items():
        assert str(gold[f"{name}_scene_sha"]) == RM.scene_sha(objs), name
    a = frames["A0"][3]
    assert sorted(np.shape(o)[1] for o in a if len(o)) == [3, 4, 5] and any(len(o) == 0 for o in a)
    assert 2600 <= len(RM.steps_of(RM.CFG_C)) <= 2601


def test_restatement_matches_reference(gold, frames, marched):
    """Discrete fields, world directions, hit points and intensities equal the reference's exactly;
    the emitted points (one simulator per case, its generator carried across A's frames) too."""
    for case, names in RM.CASES.items():
        cfg = frames[names[0]][0]
        rng = np.random.RandomState(RM.cfg_of(cfg)["random_seed"])
        for name in names:
            _, pos, ori, _, stamp = frames[name]
            m = marched[name]
            for k in ("step", "object", "index"):
                assert np.array_equal(m[k], gold[f"{name}_{k}"]), (name, k)
            assert np.array_equal(m["world_dir"], gold[f"{name}_world_dir"]), name
            assert np.array_equal(m["hit_point"], gold[f"{name}_hit_point"], equal_nan=True), name
            assert np.array_equal(m["intensity"], gold[f"{name}_raw_intensity"], equal_nan=True), name
            assert m["edge_margin"] >= 1e-9
            n_hits = int((m["step"] >= 0).sum())
            e = RM.emit_frame(m, pos, ori, cfg, RM.noise_of(rng, n_hits, cfg), stamp)
            for c, k in enumerate("xyz"):
                assert np.array_equal(e["rows"][:, c], gold[f"{name}_{k}"]), (name, k)
            assert np.array_equal(e["intensity_int"], gold[f"{name}_intensity"]), name
            for k in ("timestamp", "ring", "tag"):
                assert np.array_equal(e[k], gold[f"{name}_{k}"]), (name, k)
        if case == "A":
            st = rng.get_state()
            assert np.array_equal(st[1], gold["A_rng_keys"]) and st[2] == int(gold["A_rng_pos"])
            assert st[3] == int(gold["A_rng_has_gauss"]) and st[4] == float(gold["A_rng_cached"])


def test_handmade_cases_decide_as_designed(gold):
    """Case B's features: earlier object wins over a nearer later one, the earlier step wins over a
    nearer later step, the lower index wins a tie, a point past range_max but within 0.1 of the last
    sample hits, points further out and behind the sensor miss; a point behind the sensor below
    range_min is hit by every ray's first sample."""
    K = len(RM.steps_of(RM.CFG_B))
    assert gold["B0_step"].tolist() == [30, 30, 30, K - 1, -1, -1, -1]
    assert gold["B0_object"].tolist() == [0, 0, 0, 0, -1, -1, -1]
    assert gold["B0_index"].tolist() == [0, 1, 2, 4, -1, -1, -1]
    assert gold["B0_raw_intensity"][:4].tolist() == [40.0, 60.0, 50.0, 70.0]
    assert gold["B1_step"].tolist() == [0] * 7 and gold["B1_object"].tolist() == [1] * 7


def test_edge_scenes_sit_on_the_hit_radius(edge_scenes, edge_marched):
    """Every edge ray's expected result is (k2, p_in): p_out at the earlier step is rejected, p_in
    accepted.  Both are within a coordinate ulp of the 0.1 radius (the opposite of the golden cases'
    >= 1e-9): edge_margin <= 1e-15 at the first two origins, <= 1e-9 at the UTM-scale one, and no single
    point farther from it than 4e-15 / 1e-9; no point is closer than 0.105 to a neighbouring step's
    sample, and the designed pairs alone decide a ray (decide_edges, the base of the mutation counts)."""
    for sc, m, bar, each in zip(edge_scenes, edge_marched, (1e-15, 1e-15, 1e-9), (4e-15, 4e-15, 1e-9)):
        o, D, steps = sc["origin"], sc["dirs"], sc["steps"]
        assert len(D) == 288 and np.array_equal(m["world_dir"], D)
        assert (sc["k1"] >= 30).all() and (sc["k2"] >= sc["k1"] + 6).all() and (sc["k2"] <= 110).all()
        assert np.array_equal(m["step"], sc["k2"]) and np.array_equal(m["scene_index"], sc["scene_in"])
        assert m["edge_margin"] <= bar
        assert (sc["d_out"] >= RM.STEP).all() and (sc["d_in"] < RM.STEP).all()
        assert max(np.abs(sc["d_out"] - RM.STEP).max(), np.abs(sc["d_in"] - RM.STEP).max()) <= each
        for k, P in ((sc["k1"], sc["p_out"]), (sc["k2"], sc["p_in"])):
            for dk in (-1, 1):
                assert (RM.pair_distance(o, D, steps[k + dk], P) > 0.105).all()
        flat = RM.flatten(sc["objects"])[0]
        assert np.array_equal(flat[sc["scene_in"]], sc["p_in"]) and np.array_equal(flat[sc["scene_out"]], sc["p_out"])
        assert np.array_equal(RM.decide_edges(sc), np.column_stack([sc["k2"], sc["scene_in"]]))
    cos = edge_scenes[0]["dirs"] @ edge_scenes[0]["dirs"].T
    np.fill_diagonal(cos, 0.0)
    assert np.arccos(cos.max()) >= 0.08


def test_tie_scenes_decide_as_designed(tie_scenes, tie_marched):
    """For every tie ray the expected point is the designed one: B where it is just nearer, A where it
    is just not (the lower index where that makes the distances equal), the lower index of exact
    duplicates.  A and B share an object, are >= 1024 scene indices apart and clearly inside the radius;
    the filler is farther than 0.3 from every ray."""
    for sc, m in zip(tie_scenes, tie_marched):
        o, D, steps = sc["origin"], sc["dirs"], sc["steps"]
        assert np.array_equal(m["step"], sc["k"]) and np.array_equal(m["scene_index"], sc["winner"])
        assert np.array_equal(m["object"], np.arange(288) // 8) and len(sc["objects"]) == 36
        assert np.array_equal(RM.decide_ties(sc), sc["winner"])
        dup, near, low = sc["duplicate"], sc["nearer"], sc["b_low"]
        assert dup.sum() == 32 and [int((~dup & (near == a) & (low == b)).sum()) for a in (0, 1) for b in (0, 1)] == [64] * 4
        assert np.array_equal(sc["A"][dup], sc["B"][dup]) and 8 <= low[dup].sum() <= 24
        assert (sc["d_b"] < sc["d_a"])[~dup & near].all() and (sc["d_b"] >= sc["d_a"])[~dup & ~near].all()
        assert (np.abs(sc["d_b"] - sc["d_a"]) <= 4e-15).all()
        assert np.array_equal(sc["winner"][~dup & near], sc["scene_b"][~dup & near])
        assert np.array_equal(sc["winner"][dup], np.minimum(sc["scene_a"], sc["scene_b"])[dup])
        for d in (sc["d_a"], sc["d_b"]):
            assert (d > 0.0299).all() and (d < 0.0701).all()
        for P in (sc["A"], sc["B"]):
            assert (RM.pair_distance(o, D, steps[sc["k"] - 1], P) > 0.104).all()
        assert (np.abs(sc["scene_a"] - sc["scene_b"]) >= 1024).all()
        assert np.array_equal(sc["scene_a"] // RM.TIE_OBJECT_POINTS, sc["scene_b"] // RM.TIE_OBJECT_POINTS)
        assert np.array_equal(sc["b_low"], sc["scene_b"] < sc["scene_a"])
        xyz, inten, _, _ = RM.flatten(sc["objects"])
        assert (inten[sc["scene_a"]] != inten[sc["scene_b"]]).all()
        assert len(xyz) == 36 * RM.TIE_OBJECT_POINTS and sc["filler"].sum() == len(xyz) - 576
        V = xyz[sc["filler"]] - o
        for i in range(0, len(V), 8192):      # distance to the marched segment of every ray
            v = V[i:i + 8192]
            s = np.clip(v @ D.T, 0.0, steps[-1] + 0.2)
            d2 = (v * v).sum(axis=1)[:, None] - 2 * s * (v @ D.T) + s * s
            assert d2.min() > 0.3 ** 2


def test_size_edge_scenes_hit_as_designed():
    """The scenes of the tile-size, ray-count and block tests, decided by the restatement: the tile
    scenes hit their first and last point, the ray-count scenes are clear of every edge and hit in every
    frame, the six 441-ray frames hit exactly their chosen 257, 0, 441, 1, 256, 255 rays (margin 0.03)."""
    for E in RM.TILE_SIZES:
        objs = RM.tile_scene(E)
        m = RM.march_frame(np.zeros(3), RM.IDENTITY, RM.CFG_B, objs)
        assert sum(len(o) for o in objs) == E and m["edge_margin"] >= 1e-3
        first = (20, 0 if E > 1 else 1, 0)
        last = (41, 1, E - E // 2 - 1)
        want = {1: first, 5: last} if E > 1 else {1: first}
        for ray in range(7):
            assert (m["step"][ray], m["object"][ray], m["index"][ray]) == want.get(ray, (-1, -1, -1)), (E, ray)
    for n in RM.RAY_COUNTS:
        D, steps, objs = RM.count_scene(n)
        assert len(D) == n
        for f, o in enumerate(RM.COUNT_ORIGINS):
            m = RM.march_frame(o, RM.IDENTITY, {}, objs, dirs=D, steps=steps)
            assert m["edge_margin"] >= 1e-3 and m["step"][f % n] >= 0
            assert set(np.unique(m["object"])) <= {-1, f}
            assert n < 63 or 0.4 <= np.mean(m["step"] >= 0) <= 0.9
    objs, rays = RM.block_scene()
    assert [len(r) for r in rays] == [257, 0, 441, 1, 256, 255]
    for f, o in enumerate(RM.BLOCK_ORIGINS):
        m = RM.march_frame(o, RM.IDENTITY, RM.CFG_BLOCK, objs)
        assert np.array_equal(np.flatnonzero(m["step"] >= 0), rays[f]), f
        assert m["edge_margin"] >= 0.0299 or len(rays[f]) == 0
        assert (m["step"][rays[f]] >= 560).all() and (m["step"][rays[f]] <= 640).all()


def test_emulated_mutations_change_decisions(edge_scenes, tie_scenes):
    """Sensitivity: deciding the same scenes with wrong arithmetic (a fused sample, a fused sum of
    squares, a radius off by 1e-13) changes at least 5 rays per mutation, summed over the three edge
    scenes and, for the two fused forms, over the tie scenes.  Counts measured here: DESIGN.md §5."""
    for name, variants in RM.predicate_mutations().items():
        n = sum(int((RM.decide_edges(sc, **kw) != RM.decide_edges(sc)).any(axis=1).sum())
                for sc in edge_scenes for kw in variants)
        print(f"{name}: {n} edge rays change")
        assert n >= 5, (name, n)
        if name == "radius":
            continue
        n = sum(int((RM.decide_ties(sc, **kw) != RM.decide_ties(sc)).sum()) for sc in tie_scenes for kw in variants)
        print(f"{name}: {n} tie rays change")
        assert n >= 5, (name, n)


def test_noise_draws_are_consecutive_standard_normals():
    """rng.normal(0, s, 3) then rng.normal(0, s_i) per hit (CSIM:1038-1039) = standard_normal(4 n)
    scaled, and both leave the generator in the same state (the cached second Gaussian included)."""
    for n in (1, 2, 7, 250):
        a, b = np.random.RandomState(42), np.random.RandomState(42)
        ref = np.array([np.append(a.normal(0, 0.02, 3), a.normal(0, 5.0)) for _ in range(n)])
        got = RM.noise_of(b, n, {})
        assert np.array_equal(ref, got)
        sa, sb = a.get_state(), b.get_state()
        assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def test_arange_step_table_rule():
    """np.arange(range_min, range_max, 0.1)[k] = range_min + k * delta with delta = (range_min + 0.1)
    - range_min: for range_min 0.05 that is not 0.1, and range_min + k * 0.1 gives other values, which
    is why the table is taken from numpy and uploaded."""
    for rmin, rmax in ((0.05, 90.0), (0.05, 260.0), (0.05, 12.0), (0.3, 40.0), (1.0, 25.0)):
        t = np.arange(rmin, rmax, 0.1)
        delta = (rmin + 0.1) - rmin
        k = np.arange(len(t), dtype=np.float64)
        assert np.array_equal(t, rmin + k * delta), (rmin, rmax)
    assert (0.05 + 0.1) - 0.05 != 0.1
    t = np.arange(0.05, 260.0, 0.1)
    assert np.count_nonzero(t != 0.05 + np.arange(len(t)) * 0.1) > 0


def dump_case(path, dirs, steps, objects, poses):
    """The harness' input: the tables, the flattened scene and one (origin, R) per frame."""
    xyz, _, oid, _ = RM.flatten(objects)
    with open(path, "wb") as f:
        f.write(np.array([len(poses), len(dirs), len(steps), len(xyz)], np.int64).tobytes())
        f.write(np.array([RM.STEP], np.float64).tobytes())
        for a in (steps, dirs, xyz):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        f.write(oid.astype(np.int64).tobytes())
        for origin, R in poses:
            f.write(np.concatenate([origin, np.asarray(R).ravel()]).astype(np.float64).tobytes())


@pytest.fixture(scope="module")
def host_core(tmp_path_factory):
    """The core in the harness, built once with g++ under ASan + UBSan; returns run(path) ->
    (per-ray "step object scene_index" rows, the last line)."""
    exe = hostbuild.build(tmp_path_factory.mktemp("raymarch_host"), "raymarch_host.cpp", "-ffp-contract=off", sanitize=True)

    def run(path):
        lines = hostbuild.run(exe, path).stdout.strip().splitlines()
        return np.array([ln.split() for ln in lines[:-1]], dtype=np.int64), lines[-1]
    return run


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_kernel_core_on_host_under_asan_ubsan(tmp_path, gold, frames, host_core):
    """ray_tube / ray_exact / ray_key_less as the kernel compiles them, on cases A-C: every ray's
    step, object and point equal the reference's; merging 777-point chunks by key order gives the
    same result as one chunk."""
    for case, names in RM.CASES.items():
        path = tmp_path / f"{case}.bin"
        cfg, objs = frames[names[0]][0], frames[names[0]][3]
        dump_case(path, RM.directions(cfg), RM.steps_of(cfg), objs,
                  [(frames[n][1], RM.rotations(frames[n][2])[0]) for n in names])
        got, last = host_core(path)
        assert last == "bad 0", last
        _, _, oid, idx = RM.flatten(objs)
        want = np.concatenate([np.column_stack([gold[f"{n}_step"], gold[f"{n}_object"], gold[f"{n}_index"]])
                               for n in names])
        hit = got[:, 0] >= 0
        assert np.array_equal(hit, want[:, 0] >= 0), case
        assert np.array_equal(got[hit, 0], want[hit, 0]) and np.array_equal(got[hit, 1], want[hit, 1]), case
        assert np.array_equal(oid[got[hit, 2]], want[hit, 1]) and np.array_equal(idx[got[hit, 2]], want[hit, 2]), case


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_kernel_core_on_host_decides_edge_and_tie_scenes(tmp_path, host_core, edge_scenes, tie_scenes, edge_marched,
                                                         tie_marched):
    """The same host build on the scenes within one coordinate ulp of a decision: every ray's step,
    object and scene index equal the restatement's, in one chunk and in merged 777-point chunks."""
    scenes = [(f"edge{i}", s, m) for i, (s, m) in enumerate(zip(edge_scenes, edge_marched))]
    scenes += [(f"tie{i}", s, m) for i, (s, m) in enumerate(zip(tie_scenes, tie_marched))]
    for name, sc, m in scenes:
        path = tmp_path / f"{name}.bin"
        dump_case(path, sc["dirs"], sc["steps"], sc["objects"], [(sc["origin"], np.eye(3))])
        got, last = host_core(path)
        assert last == "bad 0", (name, last)
        want = np.column_stack([m["step"], m["object"], m["scene_index"]])
        assert np.array_equal(got, want), (name, int((got != want).any(axis=1).sum()))


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "mcdeskew.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    m = pkg()
    lib = m._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in m._lib.EXPORTED, name
        assert hasattr(lib, name), name
    assert hasattr(m, "LiDARSimulator") and m.raymarch.LiDARSimulator is m.LiDARSimulator
