"""LAS 1.2 without a GPU (las.py; f8): the known answers of the restatement the GPU tests compare with
(tests/las.py), its header against struct.unpack_from at the literal offsets of the ASPRS LAS 1.2
table, and the module surface that needs no device — argument errors, an unknown variant, 2^32
points — with every existing default unchanged (``encode_text(..., "las")`` still raises)."""
import datetime
import os
import re
import struct

import numpy as np
import pytest

import las as LAS
from conftest import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livox-motion-compensation-sim_amd", "csrc")


@pytest.mark.parametrize("x,scale,want", [(0.005, 0.01, 0), (0.015, 0.01, 2), (0.025, 0.01, 2), (-0.5, 1.0, 0),
                                          (21474836.47, 0.01, 2147483647), (21474836.48, 0.01, None),
                                          (-21474836.485, 0.01, -2147483648)])
def test_rounding_known_answers(x, scale, want):
    X, bad = LAS.fix(np.array([x]), scale, 0.0)
    if want is None:
        assert bad[0]
        with pytest.raises(ValueError, match="row 0"):
            LAS.encode(np.array([[x, 0.0, 0.0, 0.0]]), "lmc", scale)
    else:
        assert not bad[0] and int(X[0]) == want
    if x == 21474836.47:
        assert (x - 0.0) / scale == 2147483646.9999998
    if x == -21474836.485:
        assert (x - 0.0) / scale == -2147483648.5   # a tie: to even, accepted


def test_intensity_known_answers():
    it, bad = LAS.intensity(np.array([0.5, 1.0, 0.9999999, 1e-5]), 65535.0)
    assert it.tolist() == [32767, 65535, 65534, 0] and not bad.any()
    it, bad = LAS.intensity(np.array([-0.5, 65535.9, 65536.0, -1.0, np.nan, np.inf]), 1.0)
    assert bad.tolist() == [False, False, True, True, True, True] and it[:2].tolist() == [0, 65535]


def test_header_at_the_literal_offsets():
    rows = np.array([[1.25, -2.5, 3.0, 0.5, 1e9], [-7.0, 8.0, -9.0, 1.0, 2e9], [0.5, 0.25, 0.125, 0.0, 3e9]])
    data = LAS.encode(rows, "lmc", None, [10.0, 20.0, 30.0], 3, b"mcdeskew 0.1.0", 2024, 61)
    assert len(data) == 227 + 3 * 34
    u = lambda fmt, at: struct.unpack_from(fmt, data, at)   # noqa: E731
    assert data[:4] == b"LASF" and u("<HH", 4) == (0, 0) and data[8:24] == bytes(16) and u("BB", 24) == (1, 2)
    assert data[26:58] == b"OTHER".ljust(32, b"\0") and data[58:90] == b"mcdeskew 0.1.0".ljust(32, b"\0")
    assert u("<HHH", 90) == (61, 2024, 227) and u("<II", 96) == (227, 0)
    assert u("<B", 104) == (3,) and u("<H", 105) == (34,) and u("<I", 107) == (3,) and u("<5I", 111) == (0,) * 5
    assert u("<3d", 131) == (0.01, 0.01, 0.01) and u("<3d", 155) == (10.0, 20.0, 30.0)
    X = np.array([[int(np.rint((r[k] - o) / 0.01)) for k, o in enumerate((10.0, 20.0, 30.0))] for r in rows])
    want = []
    for k, o in enumerate((10.0, 20.0, 30.0)):
        want += [float(X[:, k].max()) * 0.01 + o, float(X[:, k].min()) * 0.01 + o]
    assert u("<6d", 179) == tuple(want)
    # record 1 at 227 + 34: X, Y, Z, intensity, six zero bytes, gps_time 0.0 (lmc), RGB 0
    assert u("<3iH", 261) == (int(X[1, 0]), int(X[1, 1]), int(X[1, 2]), 65535)
    assert data[261 + 14:261 + 34] == bytes(20)
    # csim: intensity as is, gps_time = column 4 * 1e-9; format 1 is the first 28 bytes, format 0 the first 20
    rows[:, 3] = [7.9, 255.0, 0.0]
    c3, c1, c0 = (LAS.encode(rows, "csim", fmt=f) for f in (3, 1, 0))
    assert struct.unpack_from("<H", c3, 227 + 12) == (7,) and struct.unpack_from("<d", c3, 227 + 20) == (1e9 * 1e-9,)
    assert struct.unpack_from("<d", c3, 227 + 34 + 20) == (2e9 * 1e-9,)
    for i in range(3):
        assert c1[227 + 28 * i:227 + 28 * (i + 1)] == c3[227 + 34 * i:227 + 34 * i + 28]
        assert c0[227 + 20 * i:227 + 20 * (i + 1)] == c3[227 + 34 * i:227 + 34 * i + 20]
    c2 = LAS.encode(rows, "csim", fmt=2)
    assert c2[227:227 + 20] == c3[227:227 + 20] and c2[227 + 20:227 + 26] == bytes(6) and len(c2) == 227 + 3 * 26
    assert struct.unpack_from("<BH", c1, 104) == (1, 28) and struct.unpack_from("<BH", c0, 104) == (0, 20)
    # the restatement reads its own files back, padded ones included
    for d in (c3, LAS.encode(rows, "csim", fmt=1, reclen=30, offset_to_points=243)):
        h, got = LAS.decode(d)
        assert np.array_equal(got[:, 3], [7, 255, 0]) and np.array_equal(got[:, 4], rows[:, 4] * 1e-9)
        assert np.array_equal(LAS.bits(got[:, 0]), LAS.bits(np.rint(rows[:, 0] / 0.001) * 0.001 + 0.0))


def test_fused_multiply_add_would_show():
    rng = np.random.default_rng(1)
    X = rng.integers(-2 ** 31, 2 ** 31, 20000)
    assert LAS.fused_differs(X, 0.001, 500000.0) >= 1000
    assert LAS.fused_differs(X, 0.001, 0.0) == 0   # without an offset the set shows nothing


def test_kernel_tile_constants_match_the_module():
    src = open(os.path.join(CSRC, "las.hpp")).read()
    m = pkg().las
    assert int(re.search(r"constexpr int kLasTile = (\d+);", src).group(1)) == m.TILE_RECORDS
    assert int(re.search(r"constexpr int kLasDecTile = (\d+);", src).group(1)) == m.DECODE_TILE_RECORDS
    assert m.TILE_RECORDS % 8 == 0
    assert all(8 * n % 16 == 0 for n in m.RECORD_BYTES.values()) and m.RECORD_BYTES == LAS.NOMINAL
    head = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    for text in (m.__doc__, head):   # what is not claimed, in both places
        flat = " ".join(text.replace("*", " ").split())
        assert "neither promised nor tested" in flat and "from memory, unchecked" in flat


def test_module_surface_without_a_gpu():
    m = pkg()
    rows = np.zeros((3, 4))
    with pytest.raises(ValueError, match="Unknown LAS variant"):
        m.encode_las(rows, variant="laspy")
    with pytest.raises(ValueError, match="point_format"):
        m.encode_las(rows, point_format=4)
    with pytest.raises(ValueError, match="scale"):
        m.encode_las(rows, scale=0.0)
    with pytest.raises(ValueError, match="scale"):
        m.encode_las(rows, scale=[0.01, np.nan, 0.01])
    with pytest.raises(ValueError, match="offset"):
        m.encode_las(rows, offset=np.inf)
    with pytest.raises(IndexError, match=">= 4"):
        m.encode_las(np.zeros((3, 3)))
    with pytest.raises(IndexError, match=">= 5"):
        m.encode_las(rows, variant="csim")
    with pytest.raises(IndexError):
        m.encode_las(np.zeros(4))
    huge = np.broadcast_to(np.zeros((1, 4)), (2 ** 32, 4))   # no memory behind it
    with pytest.raises(ValueError, match="u32"):
        m.encode_las(huge)
    with pytest.raises(ValueError, match="u32"):
        m.write_las(os.devnull, huge)
    with pytest.raises(ValueError, match="creation_date"):
        m.las._creation((2024, 400))
    assert m.las._creation(datetime.date(2024, 3, 1)) == (2024, 61)
    assert m.las._creation(None)[0] >= 2024
    for name in ("mc_las_probe", "mc_las_encode", "mc_las_encode_batch", "mc_las_decode", "mc_las_decode_batch"):
        assert name in m._lib.EXPORTED
    with pytest.raises(ValueError, match="las must be"):
        m.LiDARMotionSimulator.save_results(None, {}, las="host")


def test_existing_defaults_are_unchanged():
    m = pkg()
    with pytest.raises(ValueError, match="Unsupported text format: las"):
        m.csim_export.encode_text(np.zeros((1, 5)), "las")
    import inspect
    assert inspect.signature(m.LiDARMotionSimulator.save_results).parameters["las"].default == "laspy"
    assert "las_writer" not in m.default_config()
