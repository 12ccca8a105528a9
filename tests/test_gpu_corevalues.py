"""The value classes of tests/corevalues.py through the kernels: the scalar cores under the text
writers (csrc/codecs.hpp, csim_codecs.hpp), the text parser (ingest.hpp) and the LAS codec (las.hpp) as
hipcc compiles them for the device, byte for byte / bit for bit against plain Python and numpy
("%.6f" % v, "%.0f" % v, float(token), tests/las.py) — no tolerance anywhere.  tests/test_corevalues_cpu.py
runs the same classes through the g++ builds of the same source and asserts how many values reach each
branch; a failure here alone therefore belongs to the device compile (a fused multiply-add, the inline
128-bit division, a conversion), not to the algorithm.  Also the two LDS staging limits, hit exactly
and one byte over at every alignment: k_csim_text_write (staged / direct) and k_text_parse.  Every
output of a C-ABI call sits between 256-byte guards of 0xA5 that must survive."""
import re
from ctypes import c_int64

import numpy as np
import pytest

import corevalues as CV
import csimexport as CE
import ingest as ING
import las as LAS
from test_gpu_ingest import eq_bits, guarded, inner, open_guard, text_guarded
from test_gpu_las import DATE, check_bounds, decode_guarded, encode_rows_guarded

pytestmark = pytest.mark.gpu

SEED = 20240611          # the seed and sizes of tests/test_corevalues_cpu.py: the same values
N_ROWS = 60_000
TILE, LDS = CV.TILE_LINES, CV.TILE_TEXT
START = 1_700_000_000_000_000_000


@pytest.fixture(scope="module")
def frows():
    return CV.formatter_rows(SEED, N_ROWS)


def first_difference(got, want):
    """the first differing line, for the assertion message"""
    if got == want:
        return None
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return i, a, b
    return min(len(g), len(w)), b"(length)", b"%d / %d lines" % (len(g), len(w))


# ---- the formatters ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["pcd", "xyz", "csv"])
def test_formatter_classes_from_rows(mc, gpu_ctx, frows, fmt):
    """60 000 rows x 5 columns of F1..F7 (every class in every column, F6 in the "%.0f" columns 3 and 4;
    tiles of short lines only, tiles with F4 mixed in, tiles beyond the LDS buffer) through
    encode_text, against "%.6f" / "%.0f" of Python."""
    want = CE.BODIES[fmt](frows)
    got = mc.csim_export.encode_text(frows, fmt, context=gpu_ctx)
    assert got == want, first_difference(got, want)
    if fmt == "csv":
        direct, _ = CV.writer_tile_direct([ln + b"\n" for ln in want.split(b"\n")[:-1]])
        assert direct.count(True) >= 20 and direct.count(False) >= 50   # both paths of k_csim_text_write ran


@pytest.mark.parametrize("fmt", ["pcd", "xyz", "csv"])
def test_formatter_classes_from_a_batch(mc, gpu_ctx, frows, fmt):
    """20 000 points whose x, y, z, intensity are the float32 roundings of every third row (the
    float32-representable values of the classes; |v| < 2^107 < FLT_MAX), in frames with empty ones
    between: the batch's row is [x, y, z, trunc(intensity), frame start + t_ns] widened exactly."""
    src = frows[::3]
    n = len(src)
    counts = np.array([0, 5000, 0, TILE, n - 5000 - TILE - 1, 1, 0], np.int64)
    with np.errstate(over="ignore", under="ignore"):
        cols = [np.ascontiguousarray(src[:, k], np.float32) for k in range(4)]
    top = np.nextafter(np.float32(2.0 ** 107), np.float32(0))   # the doubles just below 2^107 round up to it
    cols = [np.where(np.isfinite(c) & (np.abs(c) >= np.float32(2.0 ** 107)), np.copysign(top, c), c) for c in cols]
    assert all(np.isfinite(c[np.isfinite(src[:, k])]).all() for k, c in enumerate(cols))
    rng = np.random.default_rng(SEED)
    t = rng.integers(-2 ** 31, 2 ** 31, n)
    starts = START + 100_000_000 * np.arange(len(counts), dtype=np.int64)
    b = gpu_ctx.batch(counts, with_time=True)
    b.upload_columns(*cols)
    b.upload_time(t)
    b.set_frame_starts(starts)
    rows = np.empty((n, 5))
    for k in range(3):
        rows[:, k] = cols[k].astype(np.float64)
    rows[:, 3] = np.trunc(cols[3].astype(np.float64))
    rows[:, 4] = (np.repeat(starts, counts) + t).astype(np.float64)
    want = CE.BODIES[fmt](rows)
    got = b"".join(mc.csim_export.encode_text_batch(b, fmt))
    b.close()
    assert got == want, first_difference(got, want)


def test_formatter_classes_through_the_lmc_lines(mc, gpu_ctx, frows):
    """20 000 rows x 4 columns through codecs.encode_pcd_bodies: the LMC "%.6f %.6f %.6f %.6f" lines, which
    use fmt6_prepare alone (128-bit arithmetic from 4294 on)."""
    rows = np.ascontiguousarray(frows[1::3, [0, 1, 2, 4]])
    want = "".join("%.6f %.6f %.6f %.6f\n" % tuple(r) for r in rows.tolist()).encode()
    got = mc.codecs.encode_pcd_bodies([rows], gpu_ctx)[0]
    assert got == want, first_difference(got, want)


# ---- the writer's staging edge -------------------------------------------------------------------------------
def csv_rows_of_lengths(lengths):
    """rows whose CSV lines have exactly these lengths (45..135): five values 10^(d - 1) print
    sum(d) + 35 digits and points, 4 commas and the newline"""
    rows = np.empty((len(lengths), 5))
    for i, L in enumerate(lengths):
        q, r = divmod(L - 40, 5)
        rows[i] = [float(10 ** (q + (1 if c < r else 0) - 1)) for c in range(5)]
    return rows


def spread(n, total):
    base, rem = divmod(total, n)
    return [base + 1] * rem + [base] * (n - rem)


def text_encode_guarded(mc, ctx, fmt, rows=None, batch=None):
    """mc_csim_text_encode / _batch of one frame's rows (or a batch) into a guarded buffer -> bytes"""
    lib, P = ctx.lib, mc._lib.ptr
    code = mc.csim_export.FORMATS[fmt]
    if batch is None:
        counts = np.array([len(rows)], np.int64)
        d_rows = ctx.device_buffer(rows.nbytes)
        d_rows.from_host(np.ascontiguousarray(rows))
        call = lambda o, nb, pos: lib.mc_csim_text_encode(ctx.handle, code, d_rows.ptr, rows.shape[1], 1, P(counts, c_int64),
                                                          o, nb, P(pos, c_int64))   # noqa: E731
        pos = np.zeros(2, np.int64)
    else:
        d_rows = None
        call = lambda o, nb, pos: lib.mc_csim_text_encode_batch(ctx.handle, code, batch.handle, o, nb, P(pos, c_int64))   # noqa: E731
        pos = np.zeros(batch.n_frames + 1, np.int64)
    assert call(None, 0, pos) == mc._lib.MC_ERR_SPACE
    total = int(pos[-1])
    out = guarded(ctx, total)
    rc = call(inner(out), total, pos)
    if d_rows is not None:
        d_rows.close()
    text = open_guard(out, total).tobytes()   # the guards survived
    assert rc == 0, ctx.lib.mc_last_error()
    return text


@pytest.mark.parametrize("shift", range(16))
def test_writer_staging_limit_at_every_shift(mc, gpu_ctx, shift):
    """One frame of two tiles of 256 CSV lines: tile 0's 11 520 + shift bytes put tile 1 at offset
    `shift` modulo 16; tile 1's text is exactly 256 * 96 - shift bytes (staged, the LDS buffer full to
    its last byte), then one byte more (direct)."""
    for over, want_direct in ((0, False), (1, True)):
        lengths = spread(TILE, 45 * TILE + shift) + spread(TILE, LDS - shift + over)
        rows = csv_rows_of_lengths(lengths)
        want = CE.csv_body(rows)
        lines = [ln + b"\n" for ln in want.split(b"\n")[:-1]]
        assert [len(ln) for ln in lines] == lengths
        direct, shifts = CV.writer_tile_direct(lines)
        assert shifts == [0, shift] and direct == [False, want_direct]
        assert sum(lengths[TILE:]) + shift == LDS + over
        got = text_encode_guarded(mc, gpu_ctx, "csv", rows)
        assert got == want, (over, first_difference(got, want))


def test_writer_direct_and_staged_tiles_side_by_side(mc, gpu_ctx):
    """Three tiles in one frame: direct (one byte over at shift 0), staged, direct (exactly full but for the
    shift of 1); then a frame whose every tile is direct (135-byte lines), from rows and from a batch."""
    lengths = spread(TILE, LDS + 1) + spread(TILE, 12_000) + spread(TILE, LDS)
    rows = csv_rows_of_lengths(lengths)
    want = CE.csv_body(rows)
    direct, shifts = CV.writer_tile_direct([ln + b"\n" for ln in want.split(b"\n")[:-1]])
    assert direct == [True, False, True] and shifts == [0, 1, 1]
    got = text_encode_guarded(mc, gpu_ctx, "csv", rows)
    assert got == want, first_difference(got, want)

    rng = np.random.default_rng(SEED + 3)
    n = 2 * TILE
    cols = [rng.uniform(1e18, 9e18, n).astype(np.float32) * rng.choice([1, 1, 1, -1], n).astype(np.float32) for _ in range(4)]
    cols[3] = np.abs(cols[3])
    t = rng.integers(0, 2 ** 31, n)
    b = gpu_ctx.batch([n], with_time=True)
    b.upload_columns(*cols)
    b.upload_time(t)
    b.set_frame_starts([START])
    rows = np.column_stack([c.astype(np.float64) for c in cols] + [(START + t).astype(np.float64)])
    want = CE.csv_body(rows)
    lines = [ln + b"\n" for ln in want.split(b"\n")[:-1]]
    assert min(map(len, lines)) >= 135 and CV.writer_tile_direct(lines)[0] == [True, True]
    got = text_encode_guarded(mc, gpu_ctx, "csv", batch=b)
    b.close()
    assert got == want, first_difference(got, want)
    got = text_encode_guarded(mc, gpu_ctx, "csv", rows)
    assert got == want, first_difference(got, want)


# ---- the token parser ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pools():
    p = CV.token_pools(SEED)
    assert sum(not ING.in_window(t) for v in p.values() for t in v) == 0   # nothing filtered
    return p


def orders(pools):
    """The tokens mixed (lines of every length: staged tiles) and sorted longest first (tiles of long
    tokens only, beyond the LDS buffer at 5 and 8 columns)."""
    toks = [t for v in pools.values() for t in v]
    rng = np.random.default_rng(SEED + 5)
    mixed = [toks[i] for i in rng.permutation(len(toks))]
    return mixed, sorted(toks, key=len, reverse=True)


def check_tokens(mc, ctx, tokens, ncols, sep, eol=b"\n", final=True):
    body, lines = CV.text_body(tokens, ncols, sep, eol, final)
    want = ING.parse_lines(lines, sep, ncols)
    got = text_guarded(mc, ctx, body, sep.decode(), ncols)
    assert got.shape == want.shape
    differ = np.flatnonzero((ING.bits(got) != ING.bits(want)).any(axis=1))
    assert not len(differ), (len(differ), lines[differ[0]], got[differ[0]].tolist(), want[differ[0]].tolist())
    return lines


def test_token_classes_through_the_parser(mc, gpu_ctx, pools):
    """~22 000 tokens (P1..P4 of corevalues.py, nan / inf / -inf among them) as XYZ lines (3 columns,
    space) and CSV lines (5 columns, comma, empty fields sprinkled in for NaN), mixed and longest first,
    then at 8 columns with "\\r\\n" endings and no final newline: float(token) bit for bit.  P2 (the exact
    ties) and the 19-digit tokens sit both in tiles staged in LDS and in tiles read in place."""
    special = set(pools["P2"]) | {t for v in pools.values() for t in v if (CV.token_mk(t) or (0, 0))[0] >= 10 ** 18}
    seen = {True: 0, False: 0}
    for tokens in orders(pools):
        check_tokens(mc, gpu_ctx, tokens, 3, b" ")
        lines = check_tokens(mc, gpu_ctx, tokens, 5, b",")
        staged, _ = CV.parser_tile_staged(lines)
        for i, ln in enumerate(lines):
            if any(f in special for f in ln.split(b",")):
                seen[staged[i // TILE]] += 1
        lines = check_tokens(mc, gpu_ctx, tokens, 8, b" ", b"\r\n", False)   # the C-ABI's column limit
        assert not all(CV.parser_tile_staged(lines, 2)[0])
    assert seen[True] >= 500 and seen[False] >= 500, seen


def test_formatter_output_round_trips(mc, gpu_ctx):
    """P4 end to end on the device: read_points(encode_text(rows)) is float() of the reference text."""
    _, v = CV.p4(SEED + 4, 4000)
    rows = np.resize(v, (len(v) // 5 + 1, 5))
    ex, ing = mc.csim_export, mc.ingest
    for fmt, head, cols, sep in (("xyz", b"", 3, b" "), ("csv", ex.CSV_HEADER, 5, b",")):
        want_text = CE.BODIES[fmt](rows)
        text = ex.encode_text(rows, fmt, context=gpu_ctx)
        assert text == want_text
        got = ing.read_points(head + text, fmt, gpu_ctx)
        assert eq_bits(got, ING.parse_lines(ING.text_lines(want_text), sep, cols))


def padded(tok, zeros):
    return tok[:1] + b"0" * zeros + tok[1:] if tok[:1] in b"+-" else b"0" * zeros + tok


@pytest.mark.parametrize("shift", range(16))
def test_parser_staging_limit_at_every_shift(mc, gpu_ctx, pools, shift):
    """Three tiles of XYZ lines made of the P2 tokens: leading zeros pad tile 0 to `shift` bytes modulo
    16 and tile 1 to exactly 256 * 96 - shift bytes (staged, the LDS buffer full), then one byte more
    (read in place)."""
    toks = pools["P2"] + pools["P2off"]
    base = [[toks[(3 * i + c + 7 * shift) % len(toks)] for c in range(3)] for i in range(2 * TILE + 10)]
    for over, want_staged in ((0, True), (1, False)):
        lines = [list(f) for f in base]
        len0 = sum(len(b" ".join(f)) + 1 for f in lines[:TILE])
        lines[0][0] = padded(lines[0][0], (shift - len0) % 16)
        len1 = sum(len(b" ".join(f)) + 1 for f in lines[TILE:2 * TILE])
        for i, z in enumerate(spread(TILE, LDS - shift + over - len1)):
            lines[TILE + i][i % 3] = padded(lines[TILE + i][i % 3], z)
        lines = [b" ".join(f) for f in lines]
        body = b"\n".join(lines) + b"\n"
        staged, shifts = CV.parser_tile_staged(lines)
        assert shifts[1] == shift and staged == [True, want_staged, True]
        assert sum(len(ln) + 1 for ln in lines[TILE:2 * TILE]) + shift == LDS + over
        assert ING.first_outside(lines, b" ") is None
        got = text_guarded(mc, gpu_ctx, body, " ", 3)
        assert eq_bits(got, ING.parse_lines(lines, b" ", 3)), over


# ---- LAS -----------------------------------------------------------------------------------------------------
REFUSED = re.compile(rb"row (\d+) \(the first of (\d+)\)")


@pytest.mark.parametrize("scale", CV.LAS_SCALES)
def test_las_edge_classes_encode(mc, gpu_ctx, scale):
    """Per (scale, offset) pair and variant ~3 900 rows (random values, quotient ties with both neighbours,
    the int32 edges with their two .5 ties, the intensity edges) through mc_las_encode.  All rows at once:
    refused, naming the first refused row of tests/las.py and counting them all; in reverse order: the
    last one named; the accepted rows alone: the file of tests/las.py byte for byte, header bounds
    included.  Together: the kernel refuses exactly the rows the restatement refuses.  Each file is then
    decoded back into rows, bit for bit against tests/las.py (las_unscale at every scale and offset)."""
    software = f"mcdeskew {mc.__version__}".encode()
    for off in CV.LAS_OFFSETS:
        for variant, fmt in (("lmc", 1), ("csim", 3)):
            rows, kind = CV.las_rows(SEED, 300, scale, off, variant)
            _, bad = LAS.records(rows, variant, scale, off, fmt)
            assert bad[kind == "edge"].any() and not bad[kind == "edge"].all() and not bad[(kind == "random") | (kind == "tie")].any()
            for r, b in ((rows, bad), (np.ascontiguousarray(rows[::-1]), bad[::-1])):
                rc, _, named = encode_rows_guarded(mc, gpu_ctx, r, variant, fmt, software, scale, off)
                m = REFUSED.search(gpu_ctx.lib.mc_last_error())
                assert rc == mc._lib.MC_ERR_INVALID and named == int(np.flatnonzero(b)[0]), (scale, off, variant)
                assert m and (int(m.group(1)), int(m.group(2))) == (named, int(b.sum()))
            keep = np.ascontiguousarray(rows[~bad])
            rc, got, named = encode_rows_guarded(mc, gpu_ctx, keep, variant, fmt, software, scale, off)
            assert rc == 0 and named == -1, gpu_ctx.lib.mc_last_error()
            assert got == LAS.encode(keep, variant, scale, off, fmt, software, *DATE), (scale, off, variant)
            check_bounds(got)
            # and back: x = X * scale + offset as two rounded operations, never one fused multiply-add
            want = LAS.decode(got)[1]
            assert np.array_equal(LAS.bits(decode_guarded(mc, gpu_ctx, got)), LAS.bits(want)), (scale, off, variant)
            if (scale, off, variant) == (0.001, 500000.0, "csim"):
                # a fused decode cannot pass: it changes 97 of this file's first 1000 X (counted exactly)
                X = np.frombuffer(got, LAS.RECORD[fmt], 1000, 227)["X"]
                assert LAS.fused_differs(X, scale, off) >= 50


def gps_file(gps):
    rec = np.zeros(len(gps), LAS.RECORD[3])
    rec["X"] = np.arange(len(gps))
    rec["gps_time"] = gps
    s, o = np.full(3, 0.01), np.zeros(3)
    return LAS.header(rec, 3, s, o, b"test", *DATE).tobytes() + rec.tobytes()


def test_las_times_off_the_nanosecond_grid(mc, gpu_ctx):
    """2 400 gps times off the nanosecond grid in 48 frames from 2^-6 s to 2^33 s (2^63 ns = 2^33.1 s),
    both signs, and the times on the accepted side of the int64 edges, decoded into a batch: t_ns =
    rint(gps * 1e9) - frame start, as tests/las.py.  The times on the refused side (the int64 edges,
    2^34 .. 2^40 s, NaN, inf) are refused, naming the point."""
    frames, refused, (pos, neg) = CV.las_gps(SEED, 2000)
    frames = frames + [pos, neg]
    counts = np.array([len(f) for f in frames], np.int64)
    gps = np.concatenate(frames)
    t, ok = LAS.time_ns(gps)
    assert ok.all() and t.max() == 2 ** 63 - 1024 and t.min() == -2 ** 63
    off = np.concatenate([[0], np.cumsum(counts)])
    starts = t[off[:-1]]
    batch, _ = mc.read_las_batch(gps_file(gps), counts=counts, context=gpu_ctx)
    assert np.array_equal(batch.frame_starts, starts)
    assert np.array_equal(batch.download_time(), t - np.repeat(starts, counts))
    batch.close()
    for k, r in enumerate(refused.tolist()):
        at = 5 + 37 * k
        bad = np.insert(gps, at, r)
        f = int(np.searchsorted(off, at, "right")) - 1
        c = counts.copy()
        c[f] += 1
        with pytest.raises(ValueError, match=rf"point {at} \(the first of 1\)"):
            mc.read_las_batch(gps_file(bad), counts=c, context=gpu_ctx)
