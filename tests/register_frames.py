"""The cases of the frames of a batch registered together (VoxelCloud.register_frames; csrc/register.hpp
k_rg_frames_*), shared by tests/test_register_frames_cpu.py and tests/test_gpu_register_frames.py, and their
restatement: tests/registration.py's ``register`` on the rows of each frame, which every frame's result must equal
bit for bit.  Nothing here defines anything anew.

The cloud: tests/registration.py's corner cloud at H with, 25 m away, tests/normals.py's isolated voxels on the same
grid (cells ISOLATED_CELLS + 100: neighbour counts 1, 2, 2, 3, 3, 3 at the radius of 2 H, the ends of the three
collinear ones exactly the radius apart), so that one batch on one cloud can hold a frame that ends with five pairs
beside frames that converge: a call has one cloud and one max_distance.  The isolated voxels are further from the
corner than any window reaches, so the corner's normals and counts are what they are without them.

Every source holds the values a batch can hold (float32, as float64), so the host harness, the restatement and the
device see the same points."""
import numpy as np

import normals as N
import registration as G
import voxel as V

H = G.H
MAX_DISTANCE = 2 * H
RADIUS = 2 * H
MAX_NN = 30
FAR = 100                             # cells: where the isolated voxels are
STATUS = G.STATUS + ("empty",)

_cache = {}


def cloud():
    """-> dict(rows, h, origin, vox, keys, cent, n_corner); nobody writes into it"""
    if "cloud" not in _cache:
        lone = np.column_stack([(N.ISOLATED_CELLS + FAR + 0.5) * H, np.full(len(N.ISOLATED_CELLS), 0.5)])
        rows = np.concatenate([G.corner_rows(), lone])
        d = V.downsample(rows, H, V.ZERO)
        _cache["cloud"] = dict(rows=rows, h=H, origin=V.ZERO, vox=d, keys=d["keys"], cent=np.ascontiguousarray(d["rows"][:, :3]),
                               n_corner=len(d["keys"]) - len(lone))
    return _cache["cloud"]


def on_planes(n, seed, T):
    """n points on the corner's planes moved back by T, as a batch holds them."""
    return V.as_float32(G.moved_back(G.corner_source(n, seed), T))


def five_pairs(n_pairs=5):
    """tests/registration.py few_neighbours on this cloud: two points beside every isolated voxel with fewer than three
    neighbours, which find it and are dropped, and n_pairs beside the three that have them."""
    at = cloud()["cent"][cloud()["n_corner"]:]
    rng = np.random.default_rng(6)
    near = np.concatenate([np.repeat(at[:3], 2, axis=0), at[3 + np.arange(n_pairs) % 3]])
    return V.as_float32(near + rng.uniform(-0.1, 0.1, near.shape) * H)


def one_plane(n=300):
    """A source on the corner's z plane alone (exact in float32): the third pivot is exactly zero from NEARBY_FLAT."""
    return V.as_float32(G.corner_source(n, n, planes=(0,)))


POSES = (G.KNOWN, G.pose(-0.01, 0.02, 0.015, [-0.03, 0.02, 0.04]), G.pose(0.015, 0.01, -0.02, [0.05, 0.01, -0.02]),
         G.pose(0.0, -0.025, 0.005, [0.0, -0.045, 0.03]))


# the largest |T - known| entry of known_answers() on the restatement, as tests/test_register_frames_cpu.py measures
# and prints it (1.52e-09), rounded up in the second digit; both tests allow four times this
MEASURED = 1.6e-9


def _case(frames, inits=None, max_iterations=3):
    """frames: a list of (n, 3) arrays -> dict(counts, src (N, 3), inits None, (4, 4) or (F, 4, 4), max_iterations)"""
    counts = [len(f) for f in frames]
    src = np.concatenate([np.zeros((0, 3))] + [np.asarray(f, np.float64).reshape(-1, 3) for f in frames])
    return dict(counts=counts, src=np.ascontiguousarray(src), inits=None if inits is None else np.asarray(inits, np.float64),
                max_iterations=max_iterations)


def sizes():
    """Frames of 1, 255, 256, 257 and 1281 points: the tree's block edge and padded partials, frame by frame."""
    return _case([on_planes(n, n, G.KNOWN) for n in G.SIZES])


def with_an_empty_frame():
    """Counts 400, 0, 881 of one source, from one pose for all frames."""
    s = on_planes(1281, 1281, G.KNOWN)
    return _case([s[:400], s[:0], s[400:]], G.NEARBY)


MIXED = ("converged", "converged", "too_few_pairs", "singular", "empty")
MIXED_ITERATIONS = (1, 3, 1, 1, 0)


def mixed(max_iterations=30):
    """One batch with every ending: a frame that converges in one iteration (from the answer), one that needs three,
    one with five pairs, one on one plane (singular) and an empty one; max_iterations 1 or 2 puts max_iterations among
    them."""
    I = np.eye(4)
    frames = [on_planes(3000, 3000, G.KNOWN), on_planes(3000, 3001, G.KNOWN), five_pairs(), one_plane(), np.zeros((0, 3))]
    return _case(frames, np.stack([G.KNOWN, I, I, G.NEARBY_FLAT, G.NEARBY]), max_iterations)


def many_small(n_frames=300, n=7):
    """300 frames of 7 points, and empty frames at the start, in the middle (two in a row) and at the end: every block
    must find its frame, and an empty frame owns none."""
    s = on_planes(n_frames * n, 300, G.KNOWN)
    frames = [s[n * f:n * (f + 1)] for f in range(n_frames)]
    none = s[:0]
    frames = [none] + frames[:100] + [none, none] + frames[100:] + [none]
    return _case(frames, max_iterations=1)


def known_answers():
    """Four frames on the corner's planes, each moved back by a pose of its own: each is recovered."""
    return _case([on_planes(2000, 40 + k, T) for k, T in enumerate(POSES)], max_iterations=30)


def large_between_small():
    """65 537 points between frames of 3 and 300: the large frame has a second tree level, the small ones none."""
    return _case([on_planes(3, 3, G.KNOWN), on_planes(65537, 65537, G.KNOWN), on_planes(300, 300, G.KNOWN)], max_iterations=2)


CASES = {
    "sizes": (sizes, ()),
    "400, 0, 881": (with_an_empty_frame, ()),
    "mixed endings": (mixed, ()),
    "mixed endings, one iteration": (mixed, (1,)),
    "mixed endings, two iterations": (mixed, (2,)),
    "300 frames of 7": (many_small, ()),
    "known answers": (known_answers, ()),
}


def case(name):
    if ("case", name) not in _cache:
        builder, args = CASES[name]
        _cache[("case", name)] = builder(*args)
    return _cache[("case", name)]


def inits_of(c):
    """The case's inits as (F, 4, 4)."""
    F = len(c["counts"])
    if c["inits"] is None:
        return np.tile(np.eye(4), (F, 1, 1))
    return np.tile(c["inits"], (F, 1, 1)) if c["inits"].ndim == 2 else c["inits"]


def frame_rows(c, f):
    off = np.concatenate([[0], np.cumsum(c["counts"])])
    return c["src"][off[f]:off[f + 1]]


def expect(key, c, given, tol=1e-6):
    """The restatement of every frame of case c on the cloud `given` (with its normals): a list, None for an empty
    frame; computed once per key (nobody writes into it)."""
    if ("expect", key) not in _cache:
        T = inits_of(c)
        _cache[("expect", key)] = [
            G.register(given, frame_rows(c, f), MAX_DISTANCE, init=T[f], max_iterations=c["max_iterations"], tol_rotation=tol,
                       tol_translation=tol) if n else None for f, n in enumerate(c["counts"])]
    return _cache[("expect", key)]


def frame_of(r, f):
    """Row f of a VoxelFrameRegistrations (or of the harness's dict of arrays) as the dict G.equal compares."""
    g = r._asdict() if hasattr(r, "_asdict") else r
    it = int(g["iterations"][f])
    return dict(transformation=g["transformations"][f], fitness=float(g["fitness"][f]), inlier_rmse=float(g["inlier_rmse"][f]),
                pairs=int(g["pairs"][f]), iterations=it, status=STATUS[int(g["status"][f])], history=g["history"][f][:it])


def holds(r, c, want, what=""):
    """Every frame of r against its restatement: every field bit for bit; an empty frame: "empty", its init, zeros;
    the history rows past a frame's iterations +0.0.  -> None, or what differs."""
    g = r._asdict() if hasattr(r, "_asdict") else r
    T = inits_of(c)
    F = len(c["counts"])
    if not all(len(g[k]) == F for k in ("transformations", "fitness", "inlier_rmse", "pairs", "iterations", "status", "history")):
        return f"{what}: not {F} rows"
    if g["history"].shape[1:] != (int(max(g["iterations"], default=0)), 8):
        return f"{what}: history {g['history'].shape}"
    for f in range(F):
        got = frame_of(g, f)
        if G.bits(g["history"][f][got["iterations"]:]).any():
            return f"{what}: frame {f} has history past its iterations"
        if want[f] is None:
            if not (got["status"] == "empty" and got["iterations"] == 0 and got["pairs"] == 0 and G.bits(got["fitness"]) == 0
                    and G.bits(got["inlier_rmse"]) == 0 and np.array_equal(G.bits(got["transformation"]), G.bits(T[f]))):
                return f"{what}: empty frame {f}: {got}"
        elif not G.equal(got, want[f]):
            return (f"{what}: frame {f}: {got['status']} ({want[f]['status']}) after {got['iterations']} ({want[f]['iterations']}), "
                    f"pairs {got['pairs']} ({want[f]['pairs']})")
    return None
