"""The scene scanner's visibility decision on the CPU (no GPU): tests/scanedges.py's fixtures
against oracle.restatement.scan_environment and their own conditions, and scan_visible's two tiers
(csrc/scan_core.hpp) compiled for the host under AddressSanitizer +
UndefinedBehaviorSanitizer: equal to the reference's mask on every row of every edge scene, and no
longer equal once any of its comparisons, margins or guards is altered."""
import shutil

import numpy as np
import pytest

import hostbuild
import scanedges as S
from oracle import restatement as R

FLAGS = ("-ffp-contract=off", "-Wno-unknown-pragmas")
EDGE_CLASSES = ("range_max", "range_min", "az_edge", "el_edge", "corner_az_rmin", "corner_el_rmax")

# (name, text of the core as the compiler reads it, its replacement); every mutant must change a decision on some
# fixture row.  "behind shortcut dropped" cannot: without `lx < -m -> az_in = 0` the exact tier
# decides those rows, and decides them alike; it is held to what it does change, rows behind the
# sensor reaching atan2, and its decision-changing form (the `lx < -m` condition alone dropped, so
# lx in [-m, m] is rejected unseen) is the mutant after it.
MUTANTS = [
    ("range_max <= to <", "if (!(d2 <= sp.range_max_sq))", "if (!(d2 < sp.range_max_sq))"),
    ("range_min >= to >", "if (!(r >= sp.range_min))", "if (!(r > sp.range_min))"),
    ("rmin2_lo / rmin2_hi swapped", "r_in = d2 > sp.rmin2_hi ? 1 : (d2 < sp.rmin2_lo ? 0 : -1);",
     "r_in = d2 > sp.rmin2_lo ? 1 : (d2 < sp.rmin2_hi ? 0 : -1);"),
    ("1e-6 clamp removed", "lz / fmax(r, 1e-6)", "lz / r"),
    ("d2 > 1e-10 guard removed", "if (d2 > 1e-10) {", "if (true) {"),
    ("fast bound 89 to 91", "par[2] < 89.0 && par[3] >= 0.0 && par[3] < 89.0",
     "par[2] < 91.0 && par[3] >= 0.0 && par[3] < 91.0"),
    ("behind shortcut dropped", "else if (lx < -m) az_in = 0;", ""),
    ("behind shortcut unconditional", "else if (lx < -m) az_in = 0;", "else az_in = 0;"),
    ("sin_v2 to sin v", "sp.sin_v2 = sv * sv;", "sp.sin_v2 = sv;"),
]
TIER_ONLY = {"behind shortcut dropped"}


@pytest.fixture(scope="module")
def scenes():
    """Every CONFIGS x poses_of edge scene with the reference's decision: (ci, pi, env, cls, keep, margins)."""
    out = []
    for ci, cfg in enumerate(S.CONFIGS):
        for pi, (pos, rpy) in enumerate(S.poses_of(ci)):
            env, cls = S.edge_scene(ci, pi)
            keep, m = S.mask(env, pos, rpy, cfg)
            out.append((ci, pi, env, cls, keep, m))
    return out


def test_mask_is_the_oracle_decision(scenes):
    """mask keeps exactly the rows oracle.restatement.scan_environment returns (uncapped, no noise), in
    order, on every edge scene and on the cap scene's 17 frames."""
    for ci, pi, env, _, keep, _ in scenes:
        pos, rpy = S.poses_of(ci)[pi]
        with np.errstate(all="ignore"):
            ref = R.scan_environment(env, S.pose_dict(pos, rpy), S.config_of(S.CONFIGS[ci]))
        assert np.array_equal(ref[:, 3], env[keep, 3]), (ci, pi)
    env, tr = S.cap_scene(), S.CAP_FRAMES
    for f in range(len(S.CAP_N)):
        pos, rpy = tr["position_gps"][f], tr["orientation_imu"][f]
        ref = R.scan_environment(env, S.pose_dict(pos, rpy), S.config_of(S.CAP_CONFIG))
        assert np.array_equal(ref[:, 3], env[S.mask(env, pos, rpy, S.CAP_CONFIG)[0], 3]), f


def test_fixture_conditions(scenes):
    """More than one scene tile and off the tile size; at most 1 % of a scene's rows below the GPU
    floor (rows exact by construction are not below it); in every fast config every edge class has
    kept and dropped rows (range_min only where there is one); the near-sensor rows are kept only
    where range_min <= 0, and there on both sides; non-finite rows are dropped."""
    for ci, pi, env, cls, keep, m in scenes:
        E = len(env)
        assert E > 1024 and E % 1024 and np.array_equal(env[:, 3], np.arange(E)), (ci, pi)
        below = int(S.below_floor(m).sum())
        exact = int((m["az_exact"] | m["el_exact"]).sum())
        print(f"config {ci} pose {pi}: {E} rows, {int(keep.sum())} kept, {below} below the floor, {exact} exact")
        assert below <= 0.01 * E and int((~S.gpu_asserted(m)).sum()) == below, (ci, pi, below)
        of = {name: keep[cls == S.CLASSES.index(name)] for name in S.CLASSES}
        assert len(of["nonfinite"]) == 3 and not of["nonfinite"].any()
        assert len(of["near"]) == len(S.NEAR_R) * 62
        if S.CONFIGS[ci][0] > 0:
            assert not of["near"].any(), (ci, pi)
        if ci not in S.FAST:
            continue
        for name in EDGE_CLASSES:
            if name == "range_min" and S.CONFIGS[ci][0] <= 0:
                assert of[name].all()
                continue
            assert of[name].any() and not of[name].all(), (ci, pi, name)
        if S.CONFIGS[ci][0] <= 0:
            assert of["near"].any() and not of["near"].all(), (ci, pi)
    # the dyadic config's exact on-edge points: d2 == range_max^2 and sqrt(d2) == range_min to the bit
    ci, pi, env, cls, keep, m = next(s for s in scenes if s[0] == S.DYADIC and s[1] == 0)
    ex = cls == S.CLASSES.index("exact")
    assert int((m["rmax"][ex] == 0).sum()) >= 6 and int((m["rmin"][ex] == 0).sum()) >= 2
    assert keep[ex & ((m["rmax"] == 0) | (m["rmin"] == 0))].all() and not keep[ex].all()


def test_cap_scene_counts():
    """The 17 cap frames see exactly CAP_N points (the subsample's boundaries for cap 700: n = cap,
    cap + 1, 2 cap - 1, 2 cap, ...), never a hidden row, and the visible rows span five scene tiles."""
    env, tr = S.cap_scene(), S.CAP_FRAMES
    assert len(S.CAP_N) == 17 and len(tr["time"]) == 17
    for n in (0, 1, 699, 700, 701, 1399, 1400, 1401, 2099, 2100, 2101, 2200):
        assert n in S.CAP_N
    for f, n in enumerate(S.CAP_N):
        keep, _ = S.mask(env, tr["position_gps"][f], tr["orientation_imu"][f], S.CAP_CONFIG)
        ids = np.flatnonzero(keep)
        assert len(ids) == n and not (ids % 2).any(), (f, n, len(ids))
        assert np.array_equal(ids, 2 * np.arange(S.N_CAP - n, S.N_CAP)), f
        for cap in S.CAPS:
            kept = S.subsample(ids, cap)
            assert len(kept) == S.subsample_count(n, cap) <= cap, (f, cap)
    assert len(env) == 4400 and (2 * S.N_CAP - 2) // 1024 == 4


def build_mutant(tmp, name, text):
    """The preprocessed harness with one alteration, built as the harness itself is."""
    ii = tmp / f"{name}.ii"
    ii.write_text(text)
    return hostbuild.build(tmp, ii, *FLAGS, sanitize=True)


def run_host(exe, path):
    """(visible, exact evaluations) per row of every case in ``path``, as its own process."""
    r = hostbuild.run(exe, path)
    out = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, 2)
    return out[:, 0].astype(bool), out[:, 1]


@pytest.fixture(scope="module")
def case_file(tmp_path_factory, scenes):
    """All edge scenes in the harness' input format, and the reference's decisions in the same order."""
    path = tmp_path_factory.mktemp("scan_host") / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(scenes)], np.float64).tobytes())
        for ci, pi, env, _, _, _ in scenes:
            pos, rpy = S.poses_of(ci)[pi]
            f.write(np.array(S.CONFIGS[ci], np.float64).tobytes())
            f.write(np.concatenate([R.euler_xyz_matrix(rpy).ravel(), pos]).astype(np.float64).tobytes())
            f.write(np.array([len(env)], np.float64).tobytes())
            f.write(np.ascontiguousarray(env[:, :3], dtype=np.float64).tobytes())
    return path, np.concatenate([s[4] for s in scenes])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_core_equals_mask_and_mutants_do_not(tmp_path, scenes, case_file):
    """scan_visible as the kernel compiles it equals the reference's mask on every row of every scene,
    with no floor (the same libm on both sides).  Each mutant of MUTANTS, built the same way, disagrees
    with the mask on at least one row; the decision-neutral one sends rows to atan2 that the core
    decides without."""
    path, want = case_file
    core = hostbuild.preprocessed("scan_host.cpp", *FLAGS, sanitize=True)
    got, exact = run_host(hostbuild.build(tmp_path, "scan_host.cpp", *FLAGS, sanitize=True), path)
    assert len(got) == len(want)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), bad[:10])
    # both tiers are in use: in a fast config some rows are decided without atan2 / asin and some
    # (the edge rows; with fov_horizontal 0 every row inside) with them
    offs = np.concatenate([[0], np.cumsum([len(s[2]) for s in scenes])])
    for k, (ci, pi, _, _, _, _) in enumerate(scenes):
        frac = float(np.mean(exact[offs[k]:offs[k + 1]] > 0))
        assert ci not in S.FAST or 0.0 < frac < 1.0, (ci, pi, frac)
    for k, (name, old, new) in enumerate(MUTANTS):
        assert core.count(old) == 1, name
        mgot, mexact = run_host(build_mutant(tmp_path, f"mutant{k}", core.replace(old, new)), path)
        n = int((mgot != want).sum())
        per = [int((mgot != want)[offs[j]:offs[j + 1]].sum()) for j in range(len(scenes))]
        hit = sorted({scenes[j][0] for j in range(len(scenes)) if per[j]})
        tier = int(((mexact > 0) != (exact > 0)).sum())
        print(f"mutant '{name}': {n} rows decided unlike the reference (configs {hit}), {tier} rows change tier")
        if name in TIER_ONLY:
            assert n == 0 and tier >= 1000, (name, n, tier)
        else:
            assert n >= 1, name
