"""The rays through a voxel cloud without a GPU: (1) csrc/rays_core.hpp compiles alone behind the stand-ins and has no
HIP include; (2) the scalar core, included by tests/host/rays_host.cpp, built with g++ plainly and under ASan + UBSan,
against the restatement of tests/rays.py on every case — every count, every `through` and the three stats — and what
the cases promise, on the restatement; (3) the restatement against code that does not share its definition: exact
rational arithmetic on the computed grid coordinates; (4) mutant cores, each different from the restatement on a named
case; (5) the module surface that needs no device."""
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hostbuild
import rays as R
import voxel as V
from conftest import pkg

ROOT = hostbuild.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


# ---- (1) the core header on its own --------------------------------------------------------------------------------
@needs_gxx
def test_core_header_is_self_contained(tmp_path):
    """tests/test_core_headers.py's line on rays_core.hpp itself."""
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "device_standins.hpp"\n#include "rays_core.hpp"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", hostbuild.CSRC, "-I", hostbuild.HOST,
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(os.path.join(hostbuild.CSRC, "rays_core.hpp")).read()
    assert not [i for i in re.findall(r"#include\s+[<\"]([^>\"]+)", text) if "hip" in i.lower()]


# ---- (2) the core under g++ ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rays_host")
    return tmp, [hostbuild.build(tmp, "rays_host.cpp", "-ffp-contract=off", sanitize=san) for san in (False, True)]


def run_host(exe, tmp, c):
    """One case through the harness -> (dict like the restatement's; the raw bytes)."""
    src, dst = tmp / "in.bin", tmp / "out.bin"
    M, n = len(c["keys"]), len(c["src"])
    origins = np.ascontiguousarray(c["origins"], np.float64).reshape(-1, 3)
    log2cap = 6
    while (1 << log2cap) < 2 * M:
        log2cap += 1
    par = np.array([c["h"], *c["origin"]], np.float64)
    dim = np.array([M, n, len(origins), c["guard"], c["max_steps"], log2cap], np.int64)
    src.write_bytes(par.tobytes() + dim.tobytes() + np.ascontiguousarray(c["keys"], np.int32).tobytes()
                    + np.ascontiguousarray(c["src"][:, :3], np.float64).tobytes() + origins.tobytes())
    hostbuild.run(exe, src, dst)
    raw = dst.read_bytes()
    assert len(raw) == 32 + 8 * M + 4 * n
    stats = np.frombuffer(raw, "<i8", 4, 0)
    assert stats[3] == 0
    return dict(passed=np.frombuffer(raw, "<i4", M, 32), ended=np.frombuffer(raw, "<i4", M, 32 + 4 * M),
                through=np.frombuffer(raw, "<i4", n, 32 + 8 * M), n_rays=int(stats[0]), n_skipped=int(stats[1]),
                steps=int(stats[2])), raw


@needs_gxx
def test_core_equals_the_restatement_on_every_case(exes):
    tmp, builds = exes
    for name in R.CASES:
        c, want = R.case(name), R.expect(name)
        seen = []
        for exe in builds:
            got, raw = run_host(exe, tmp, c)
            seen.append(raw)
            assert R.equal(got, want), (name, got, want)
        assert seen[0] == seen[1], name
        print(f"{name}: {want['n_rays']} rays, {want['n_skipped']} skipped, {want['steps']} steps, passed "
              f"{int(want['passed'].sum())}, ended {int(want['ended'].sum())}")


def grid_walk(s, e, max_steps=4096):
    return R.walk((np.array(s) * R.H).tolist(), (np.array(e) * R.H).tolist(), R.H, V.ZERO, max_steps)


def test_the_cases_hold_what_they_promise():
    """On the restatement, which the test above holds the core to."""
    # ties go to the lowest axis: x, then y, then z, in either direction
    assert grid_walk(*R.TIES[0]) == R.TIE_ORDER
    assert grid_walk(*R.TIES[3]) == [(3, 3, 3), (2, 3, 3), (2, 2, 3), (2, 2, 2), (1, 2, 2), (1, 1, 2), (1, 1, 1), (0, 1, 1),
                                     (0, 0, 1), (0, 0, 0)]
    assert grid_walk(*R.TIES[1]) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0), (3, 2, 0), (3, 3, 0)]
    assert grid_walk(*R.TIES[4]) == [(3, 3, 0), (2, 3, 0), (2, 2, 0), (1, 2, 0), (1, 1, 0), (0, 1, 0), (0, 0, 0)]
    # an axis alone
    assert grid_walk(*R.AXIS[0]) == [(k, 0, 0) for k in range(6)]
    assert grid_walk(*R.AXIS[1]) == [(0, -k, 0) for k in range(4)] and grid_walk(*R.AXIS[2]) == [(0, 0, k) for k in range(7)]
    # on a face: the endpoint's cell is floor(g), the cell an insert puts it in; an origin on a face starts in floor(g)
    assert grid_walk(*R.FACES[0]) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)]
    assert grid_walk(*R.FACES[2]) == [(3, 0, 0), (2, 0, 0), (1, 0, 0)]
    assert grid_walk(*R.FACES[7])[0] == (2, 2, 2) and grid_walk(*R.FACES[7])[-1] == (5, 5, 5)
    for name in R.CASES:
        c = R.case(name)
        if name in R.NOT_FINITE_ORIGINS:
            continue
        for s, e in zip(np.broadcast_to(np.reshape(c["origins"], (-1, 3)), c["src"].shape), c["src"]):
            w = R.walk(s.tolist(), e.tolist(), c["h"], c["origin"], 2 ** 22)
            if w is not None and np.isfinite(e).all():
                K = V.quantise(e[None], [0.0], c["h"], c["origin"])[0][0]
                assert w[-1] == tuple(K.tolist()) and len(set(w)) == len(w), name
    # negative keys: both walks cross key 0 on every axis
    c = R.case("negative keys")
    for s, e in zip(c["origins"], c["src"]):
        w = np.array(R.walk(s.tolist(), e.tolist(), c["h"], c["origin"], 4096))
        assert (w.min(axis=0) < 0).all() and (w.max(axis=0) > 0).all()
    # the same cell: ended + 1, never passed, whatever the guard
    for g in (0, 1, 255):
        w = R.expect(f"same cell, guard {g}")
        assert w["steps"] == 0 and not w["passed"].any() and w["ended"].sum() == 3 and not w["through"].any()
    # the guard on walks of 0, 1, 3, 4 steps (the box holds every cell of them)
    steps = [0, 1, 3, 4, 4, 5]
    for g in (0, 1, 3):
        assert R.expect(f"guard {g}")["through"].tolist() == [max(n - g, 0) for n in steps]
    # max_steps: exactly max_steps is walked, one more is skipped; a skipped ray ends nowhere
    w = R.expect("max_steps 5")
    assert w["through"].tolist() == [4, 5, -1, 4, 5] and w["n_skipped"] == 1 and w["ended"].sum() == 4 and w["steps"] == 18
    w = R.expect("max_steps 1")
    assert w["through"].tolist() == [0, 1, -1, -1] and w["n_skipped"] == 2 and w["ended"].sum() == 2
    # skipped: through is -1 exactly there
    w = R.expect("skipped")
    assert w["through"].tolist() == [6, -1, -1, -1, -1, -1, 13, -1, -1, -1] and w["n_skipped"] == 8 and w["ended"].sum() == 2
    w = R.expect("skipped origins")
    assert (w["through"] == -1).tolist() == [False] + [True] * 5 + [False] + [True] * 6 + [False] and w["n_skipped"] == 11
    # contention
    w, c = R.expect("contention"), R.case("contention")
    assert len(np.unique(c["origins"], axis=0)) == 4097
    assert c["keys"].tolist() == [[5, 0, 0], [10, 0, 0], [0, 0, 0]] and w["passed"].tolist() == [4097, 0, 4097]
    assert w["ended"].tolist() == [0, 4097, 0]
    # own points: every ray ends where its point was put
    c = R.case("own points")
    assert np.array_equal(R.expect("own points")["ended"], V.downsample(c["rows"], c["h"], c["origin"])["counts"])
    # the long ray: the accumulated walk leaves the restatement's
    c = R.case("long")
    s, e = c["origins"][0].tolist(), c["src"][0].tolist()
    assert R.accumulated_walk(s, e, c["h"], c["origin"]) != R.walk(s, e, c["h"], c["origin"], 4096)
    assert R.expect("long")["steps"] == 2932 and R.expect("long")["through"].tolist() == [2931]
    # an empty cloud still walks
    w = R.expect("empty cloud")
    assert w["through"].tolist() == [0, 0, 0, -1] and w["steps"] == 14 and len(w["passed"]) == 0


def test_the_ghost_is_seen_through():
    """The known answer, on the restatement: the scan sees the wall alone, so every voxel of the box has beams through
    it and none ending in it, and the wall's voxels have beams ending in them and, with guard 1, none through them."""
    c, w = R.case("ghost"), R.expect("ghost")
    wall = V.downsample(c["wall"], c["h"], c["origin"])
    both = V.downsample(c["rows"], c["h"], c["origin"])
    n_wall, n_box = len(wall["keys"]), len(c["box"])
    assert n_wall == 24 * 12 and n_box == 36 and len(both["keys"]) == n_wall + n_box
    assert np.array_equal(both["keys"][:n_wall], wall["keys"])             # the wall first, then the box
    assert (w["ended"][:n_wall] == 4).all() and not w["passed"][:n_wall].any()
    assert (w["passed"][n_wall:] >= 1).all() and not w["ended"][n_wall:].any()
    assert np.array_equal((w["passed"] >= 1) & (w["ended"] == 0), np.arange(n_wall + n_box) >= n_wall)
    assert w["n_skipped"] == 0 and w["through"].min() == 0 and w["through"].max() >= 1


# ---- (3) the restatement against exact rational arithmetic -----------------------------------------------------------
# The bound.  With |g| <= 1025 the three roundings of t_a(j) = fl(fl(b - gs_a) / fl(ge_a - gs_a)) — the two differences
# and the division, each within 2^-53 relative — leave the computed t within 4 x 2^-53 < 5e-16 of the exact crossing
# parameter (t <= 1).  Two crossings can therefore be taken in the wrong order only when their exact parameters differ
# by less than 1e-15; over such an interval the point of the segment moves less than |d| x 1e-15 <= 2050 x 1e-15 < 3e-12
# grid units.  So a cell the walk leaves out is crossed over an interval far below 1e-9, and a cell it visits without the
# exact segment entering it lies within 3e-12 < 1e-9 grid units of the segment.
EPS = Fraction(1, 10 ** 9)


def exact_check(s, e, h, o):
    (gs, ks), (ge, ke) = R.cell(s, h, o), R.cell(e, h, o)
    assert max(map(abs, gs + ge)) <= 1025
    cells = R.walk(s, e, h, o, 2 ** 22)
    steps = sum(abs(ke[a] - ks[a]) for a in range(3))
    assert len(cells) == steps + 1 and cells[0] == tuple(ks) and cells[-1] == tuple(ke) and len(set(cells)) == len(cells)
    G = [Fraction(x) for x in gs]
    D = [Fraction(ge[a]) - G[a] for a in range(3)]
    # every cell the exact segment crosses over an interval longer than 1e-9 is visited
    times = {Fraction(0), Fraction(1)}
    for a in range(3):
        if D[a] != 0:
            for b in range(min(ks[a], ke[a]), max(ks[a], ke[a]) + 2):
                tau = (b - G[a]) / D[a]
                if 0 < tau < 1:
                    times.add(tau)
    times = sorted(times)
    visited = set(cells)
    for t0, t1 in zip(times, times[1:]):
        if t1 - t0 > EPS:
            mid = (t0 + t1) / 2
            assert tuple(math.floor(G[a] + mid * D[a]) for a in range(3)) in visited
    # every visited cell lies within 1e-9 of the exact segment: where the segment meets the face it was entered by
    for prev, cur in zip(cells, cells[1:]):
        a = next(a for a in range(3) if prev[a] != cur[a])
        assert sum(abs(prev[c] - cur[c]) for c in range(3)) == 1
        tau = (max(prev[a], cur[a]) - G[a]) / D[a]
        assert 0 <= tau <= 1
        for c in range(3):
            assert cur[c] - EPS <= G[c] + tau * D[c] <= cur[c] + 1 + EPS
    return steps


def test_walk_against_exact_rational_arithmetic():
    rng = np.random.default_rng(21)
    h, o = 0.1, (0.3, -0.2, 0.1)
    total = 0
    for r in range(300):
        if r < 296:          # short rays anywhere in |g| <= 1024
            centre = rng.uniform(-1000.0, 1000.0, 3)
            gs, ge = centre + rng.uniform(-15.0, 15.0, 3), centre + rng.uniform(-15.0, 15.0, 3)
            if r % 4 == 0:   # some along an axis or a plane, some with an end on a face
                ge[rng.integers(3)] = gs[rng.integers(3)]
                gs[rng.integers(3)] = float(round(gs[0]))
        else:                # and a few across the whole range
            gs, ge = rng.uniform(-1024.0, 1024.0, 3), rng.uniform(-1024.0, 1024.0, 3)
        s = (np.array(o) + gs * h).tolist()
        e = (np.array(o) + ge * h).tolist()
        total += exact_check(s, e, h, o)
    # exact ties, where the rational order decides nothing and the rule does
    for s, e in R.TIES + R.FACES:
        total += exact_check((np.array(s) * R.H).tolist(), (np.array(e) * R.H).tolist(), R.H, V.ZERO)
    print(f"{total} transitions checked against exact arithmetic")
    assert total > 10000


# ---- (4) mutants ---------------------------------------------------------------------------------------------------
MUTANTS = {
    # name: (edits of the preprocessed core (old, new, occurrences), the case it must differ on, a case it still passes)
    "ties to the highest axis": ((("if (w->t[1] < best) {", "if (w->t[1] <= best) {", 1),
                                  ("if (w->t[2] < best) {", "if (w->t[2] <= best) {", 1)), "diagonal ties", "axis"),
    "t accumulated": ((("const double t = rays_crossing(k, dir, left, gs, d);",
                        "const double t = left == 0 ? __builtin_inf() : best + 1.0 / fabs(d);", 1),), "long", "axis"),
    # the crossing parameters from a g without the origin: equal on every case of the default origin, the blind spot the
    # cases on V.ORIGIN_GRIDS close
    "g forgets the origin": ((("const double d = v[a] - o[a];", "const double d = v[a];", 1),), "ties on fractional", "diagonal ties"),
    "guard off by one": ((("if (at < counted && rays_voxel(", "if (at <= counted && rays_voxel(", 1),), "guard 1", "same cell, guard 1"),
}


@needs_gxx
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_mutant_core_differs_on_its_case(tmp_path, mutant):
    edits, differs_on, passes = MUTANTS[mutant]
    core = hostbuild.preprocessed("rays_host.cpp", "-ffp-contract=off")
    for old, new, occurrences in edits:
        assert core.count(old) == occurrences, (old, core.count(old))
        core = core.replace(old, new)
    ii = tmp_path / "mutant.ii"
    ii.write_text(core)
    exe = hostbuild.build(tmp_path, ii, "-ffp-contract=off")
    got, _ = run_host(exe, tmp_path, R.case(passes))
    assert R.equal(got, R.expect(passes)), (mutant, passes)
    got, _ = run_host(exe, tmp_path, R.case(differs_on))
    want = R.expect(differs_on)
    assert not R.equal(got, want), (mutant, differs_on)
    print(f"{mutant}: on '{differs_on}' passed differs in {int((got['passed'] != want['passed']).sum())} voxels, through in "
          f"{int((got['through'] != want['through']).sum())} rays")
    if mutant == "t accumulated":       # and it is the accumulated walk of tests/rays.py that it walks
        c = R.case("long")
        acc = R.accumulated_walk(c["origins"][0].tolist(), c["src"][0].tolist(), c["h"], c["origin"])
        held = {tuple(k) for k in c["keys"].tolist()}
        assert int(got["through"][0]) == sum(cell in held for cell in acc[:-2])


# ---- (5) the module surface ----------------------------------------------------------------------------------------
NEW = ("mc_voxel_rays_batch", "mc_voxel_rays_f64", "mc_timing_read_voxel_rays")


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


def test_argument_errors_need_no_device():
    m = pkg()
    ctx = _NoDevice()
    cloud = m.VoxelCloud(ctx, 10, 7, 0.05, (0.0, 0.0, 0.0))
    rows, o = np.zeros((5, 3)), np.zeros(3)
    for src in (np.zeros((5, 2)), np.zeros(5), np.zeros((5, 3, 1))):
        with pytest.raises(ValueError, match=r"rows must be \(N, >= 3\)"):
            cloud.rays(src, o)
    for src in (np.zeros((0, 3)), np.zeros((0, 4))):
        with pytest.raises(ValueError, match="the source is empty"):
            cloud.rays(src, o)
    with pytest.raises(ValueError, match=r"fewer than 2\^31"):
        cloud.rays(np.broadcast_to(np.zeros((1, 3)), (2 ** 31, 3)), o)
    with pytest.raises(ValueError, match="frame names a frame of a Batch"):
        cloud.rays(rows, o, frame=0)
    nan, inf = np.zeros((5, 3)), np.zeros(3)
    nan[2, 1], inf[0] = np.nan, np.inf
    for bad in (np.zeros(2), np.zeros((4, 3)), np.zeros((5, 4)), np.zeros((3, 5)), np.zeros((1, 5, 3)), nan, inf, "x", None,
                [[0, 0, 0], [1, 1]], np.zeros(3, complex)):
        with pytest.raises(ValueError, match=r"origins must be finite float64 of shape \(3,\) or \(5, 3\), one per row"):
            cloud.rays(rows, bad)
    for g in (-1, 256, 1.0, "1", None, True):
        with pytest.raises(ValueError, match=r"guard must be an integer in 0\.\.255"):
            cloud.rays(rows, o, guard=g)
    for ms in (0, -1, 2 ** 22 + 1, 4096.0, "9", None, False):
        with pytest.raises(ValueError, match=r"max_steps must be an integer in 1\.\.4194304"):
            cloud.rays(rows, o, max_steps=ms)
    # arguments at the edge of what is allowed pass the checks and reach the liveness test
    closed = m.VoxelCloud(ctx, 10, 6, 0.05, (0.0, 0.0, 0.0))      # not the context's live generation
    for kw in (dict(guard=0, max_steps=1), dict(guard=np.int32(255), max_steps=np.int64(2 ** 22))):
        with pytest.raises(ValueError, match="closed or was replaced"):
            closed.rays(rows, o, **kw)
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.rays(np.zeros((5, 6)), [[1, 2, 3]] * 5)
    assert m.VoxelRays is m.voxel.VoxelRays
    assert m.VoxelRays._fields == ("passed", "ended", "through", "n_rays", "n_skipped", "steps")
    assert callable(m.VoxelCloud.rays) and callable(m.Context.read_timing_voxel_rays)
    assert "VoxelRays" in m.__doc__ and "Seeing through the cloud" in m.voxel.__doc__
    assert "remove((r.passed >= k) & (r.ended == 0))" in m.VoxelCloud.rays.__doc__.replace("\n        ", " ")


def test_symbols_exported_and_abi_unchanged():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    # the library refuses a NULL context itself, and clears the stats
    stats = np.ones(4, np.int64)
    p = m._lib.ptr(stats, m._lib.c_int64)
    assert lib.mc_voxel_rays_f64(None, None, 3, 1, None, 1, 1, 4096, None, None, None, p) == m._lib.MC_ERR_INVALID
    assert not stats.any()
    stats[:] = 1
    assert lib.mc_voxel_rays_batch(None, None, -1, None, 1, 1, 4096, None, None, None, p) == m._lib.MC_ERR_INVALID
    assert not stats.any()
    assert lib.mc_timing_read_voxel_rays(None, None, None) == m._lib.MC_ERR_INVALID
