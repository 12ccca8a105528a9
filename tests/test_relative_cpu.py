"""The relative (sensor-frame) SLERP deskew on the CPU (tests/relative.py): the oracle against scipy,
the bar on numpy emulations of what the device does and of what it must not do, and the fold of
csrc/relfold.hpp compiled for the host.  No GPU.

    p' = R_ref^T ( R(q(t)) p + pos(t) - pos_ref ),  (R_ref, pos_ref) = slerp_pose(table, t_ref)

Every case prints `case: d_ref ..., folded / two-pass outside the bar` (pytest -s); DESIGN §5 records them.
"""
import shutil
import struct

import numpy as np
import pytest

import hostbuild
import relative as V
import rounding as Q
from oracle import restatement as R


def test_oracle_matches_scipy_across_yaw_wrap():
    sp = pytest.importorskip("scipy.spatial.transform")
    rng = np.random.default_rng(5)
    T = 60
    time = np.cumsum(rng.uniform(0.05, 0.15, T))
    yaw = (np.cumsum(rng.uniform(0.2, 0.5, T)) + np.pi) % (2 * np.pi) - np.pi      # wraps several times
    rpy = np.column_stack([rng.normal(0, 0.05, T), rng.normal(0, 0.05, T), yaw])
    pos = np.array([4.0e5, 5.0e6, 100.0]) + np.cumsum(rng.normal(0, 0.5, (T, 3)), axis=0)
    tr = {"time": time, "position_gps": pos, "orientation_imu": rpy}
    assert np.count_nonzero(np.abs(np.diff(yaw)) > np.pi) >= 3
    slerp = sp.Slerp(time, sp.Rotation.from_euler("xyz", rpy))

    def pose(t):
        t = np.clip(t, time[0], time[-1])
        return slerp(t).as_matrix(), np.column_stack([np.interp(t, time, pos[:, c]) for c in range(3)])

    n = 500
    xyz = rng.uniform(-90, 90, (n, 3))
    for t_frame, t_ref in ((time[3], time[3]), (time[10] + 0.01, time[12] - 0.02), (time[-2], time[0] - 1.0),
                           (time[20], time[-1] + 5.0)):
        t_ns = rng.integers(-200_000_000, 400_000_000, n)
        Rt, pt = pose(t_frame + t_ns * 1e-9)
        Rr, pr = pose(np.array([t_ref]))
        want = (np.einsum("nij,nj->ni", Rt, xyz) + pt - pr[0]) @ Rr[0]
        got = V.relative_oracle(xyz, t_ns, t_frame, t_ref, tr)
        sc = V.relative_scale(xyz, t_ns, t_frame, t_ref, tr)
        assert (np.abs(got - want).max(axis=1) / sc).max() < 1e-13


def test_record_emulation_is_emu_slerp():
    """emu_slerp_records on the plain records is rounding.emu_slerp, bit for bit."""
    case, _, _ = V.relative_bundle("big", "sorted", True, "key")
    tr = case["tr"]
    sg = Q.pose_segments(tr)
    for f in (0, 1, 5):
        a = V.emu_slerp_records(sg, tr["time"], case["xyz"][f], case["t_ns"][f], case["times"][f])
        b = Q.emu_slerp(case["xyz"][f], case["t_ns"][f], case["times"][f], tr, 10)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("table,pattern,shifted,ref", V.CASES)
def test_bar_on_emulations(table, pattern, shifted, ref):
    """d_ref is small enough for the bar to mean something; the folded-record emulation passes it;
    the two-pass route (float32 global batch, then the inverse matrix) fails it on every shifted case;
    every mutant of the fold fails it."""
    case, frames, d = V.relative_bundle(table, pattern, shifted, ref)
    total = sum(3 * len(r) for r, _, _ in frames)
    folded = V.failures(case, frames, d, V.emu_folded)
    two = V.failures(case, frames, d, V.emu_two_pass)
    print(f"relative {table}/{pattern}/{'shifted' if shifted else 'as generated'}/{ref}: d_ref {d:.3e}, "
          f"outside the bar: folded {folded}, two-pass {two} of {total}")
    assert d <= Q.D_REF_MAX
    assert folded == 0
    if shifted:
        assert two > total // 2, "the bar does not see the two-pass route's double rounding"
    for m in V.MUTANTS:
        assert V.failures(case, frames, d, lambda *a, m=m: V.emu_folded(*a, mutant=m)) > total // 2, m


@pytest.mark.parametrize("shifted", [False, True])
def test_point_at_reference_time_maps_to_itself(shifted):
    case, frames, d = V.relative_bundle("big", "sorted", shifted, "start")
    tr = case["tr"]
    for f in (0, 2):
        xyz, tf = case["xyz"][f], case["times"][f]
        zero = np.zeros(len(xyz), np.int64)
        sc = V.relative_scale(xyz, zero, tf, tf, tr)
        for what, y in (("oracle", V.relative_oracle(xyz, zero, tf, tf, tr)), ("folded", V.emu_folded(xyz, zero, tf, tf, tr))):
            assert Q.rounded_once_failures(Q.f32(y), xyz, sc, Q.MARGIN * d) == 0, what


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_fold_compiled_for_the_host(tmp_path):
    """rel_fold of csrc/relfold.hpp through g++ -ffp-contract=off equals the numpy fold bit for bit, on
    the records of a shifted table and a reference pose between two samples."""
    exe = hostbuild.build(tmp_path, "relfold_host.cpp", "-ffp-contract=off")
    tr = dict(Q.pose_table("big"))
    tr["position_gps"] = tr["position_gps"] + V.SHIFT
    sg = Q.pose_segments(tr)
    q_ref, pos_ref = V.emu_pose(sg, tr["time"], 12.3456)
    rec = np.ascontiguousarray(np.column_stack([sg["q0"], sg["v"], sg["p0"], sg["dp"]]))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<q", len(rec)) + np.concatenate([q_ref, pos_ref]).tobytes() + rec.tobytes())
    hostbuild.run(exe, src, dst, timeout=120)
    got = np.frombuffer(dst.read_bytes(), np.float64).reshape(-1, 14)
    fd = V.fold_records(sg, q_ref, pos_ref)
    want = np.column_stack([fd["q0"], fd["v"], fd["p0"], fd["dp"]])
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
    # and it is a fold: the rotation part is orthonormal to rounding, the relative position small
    Rr, pr = R.slerp_pose(tr["time"], tr["position_gps"], tr["orientation_imu"], np.array([12.3456]))
    k = 1234
    assert np.allclose(got[k, 8:11], Rr[0].T @ (sg["p0"][k] - pr[0]), rtol=0, atol=1e-9)
