"""The value classes of tests/corevalues.py through the g++ builds of the scalar cores (no GPU): the
"%.6f" / "%.0f" formatters, the text token parser and the LAS record cores, included by the harnesses
of tests/host/ as the existing host tests build them, fed from files and compared here with
"%.6f" % v / "%.0f" % v, float(token) and tests/las.py.  The branch predicates of corevalues.py count
how many inputs reach each branch of each core, and the counts are asserted: a class that stops
reaching its branch fails here, before a GPU sees the generator.  tests/test_gpu_corevalues.py sends the
same classes through the kernels; if it fails while this passes, the device compile is at fault, not
the algorithm."""
import collections
import shutil

import numpy as np
import pytest

import corevalues as CV
import csimexport as CE
import hostbuild
import ingest as ING
import las as LAS
from test_las_host import DEC_OUT, ENC_OUT

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

N_ROWS = 60_000      # formatter rows (x 5 columns), the rows the GPU test encodes
SEED = 20240611


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("corevalues")
    return (tmp, hostbuild.build(tmp, "csim_text_host.cpp"), hostbuild.build(tmp, "ingest_host.cpp"),
            hostbuild.build(tmp, "las_host.cpp", "-ffp-contract=off"))


def run(exe, tmp, mode, data):
    src, dst = tmp / "in.bin", tmp / "out.bin"
    src.write_bytes(data)
    hostbuild.run(exe, mode, src, dst, timeout=120)
    return dst.read_bytes()


# ---- the formatters ------------------------------------------------------------------------------------------
def test_formatters_on_the_value_classes(exes):
    """300 000 values (the 60 000 x 5 rows of the GPU test): every value through fmt6_prepare,
    fmt0_prepare and csim_fmt6_prepare, against "%.6f" % v and "%.0f" % v; at least 1000 values in each
    formatter branch."""
    tmp, exe, _, _ = exes
    rows = CV.formatter_rows(SEED, N_ROWS)
    vals = rows.ravel()
    fin = np.isfinite(vals)
    assert np.abs(vals[fin]).max() < 2.0 ** 107 and (np.abs(vals[fin]) >= 2.0 ** 106).any()
    out = run(exe, tmp, "file", vals.tobytes()).decode().split("\n")
    assert out.pop() == "" and len(out) == len(vals)
    wrong = []
    for v, line in zip(vals.tolist(), out):
        want = ("%.6f" % v, "%.0f" % v, "%.6f" % v)
        if tuple(line.split("\t")) != want:
            wrong.append((v.hex() if v == v else "nan", line, want))
    assert not wrong, (len(wrong), wrong[:5])

    # the branch counts, from the predicates alone
    lmc = collections.Counter(CV.fmt6_branch(vals).tolist())
    csim = collections.Counter(CV.csim_fmt6_branch(vals).tolist())
    groups = collections.Counter()
    for c in range(5):   # the PCD lines print columns 3 and 4 "%.0f"; the CSV lines print every column "%.6f"
        groups.update(CV.digit_groups(v, c >= 3) for v in rows[:, c].tolist())
    counts = {"fast": csim["fast"], "exact below 4294": csim["exact"], "split": csim["split"], "integer-only": csim["int"],
              "128-bit": csim["wide128"], "fmt6_prepare wide": lmc["wide"], "fmt6_prepare 128-bit": lmc["wide128"],
              "put_digits x1": groups[1], "put_digits x2": groups[2], "put_digits x3": groups[3]}
    print("formatter branches:", counts)
    assert all(n >= 1000 for n in counts.values()), counts
    # every class in every column, F6 in columns 3 and 4
    pools = CV.formatter_pools(SEED, max(N_ROWS // 4, 2000))
    for c in range(5):
        col = rows[:, c]
        for k, p in enumerate(pools):
            p = p[~np.isnan(p)]
            assert np.isin(col, p).sum() >= (2 if k == 6 else 500), (c, k)
    # the lines' tiles: some staged (short lines only), some direct, as the CSV writer sees them
    lines = CE.csv_body(rows).split(b"\n")[:-1]
    direct, _ = CV.writer_tile_direct([ln + b"\n" for ln in lines])
    print("CSV tiles: staged", direct.count(False), "direct", direct.count(True))
    assert direct.count(False) >= 50 and direct.count(True) >= 20


# ---- the token parser ----------------------------------------------------------------------------------------
TOK_OUT = np.dtype([("bits", "<u8"), ("bad", "<i4"), ("len", "<i4")])


def test_parser_on_the_token_classes(exes):
    """About 22 000 tokens (P1 13 500, P2 1 600 ties + 3 200 off-ties, P3 90, P4 ~3 000): none outside the
    window, every P2 tie exact, every value float(token) bit for bit; at least 2000 tokens in each
    of M < 2^53, k == 0 and ingest_div, the last with s >= 0 and s < 0 and sh = 2 and 3."""
    tmp, _, exe, _ = exes
    pools = CV.token_pools(SEED)
    toks = [t for p in pools.values() for t in p]
    assert sum(not ING.in_window(t) for t in toks) == 0          # nothing filtered
    assert all(CV.is_exact_tie(t) for t in pools["P2"]) and not any(CV.is_exact_tie(t) for t in pools["P2off"])
    got = np.frombuffer(run(exe, tmp, "file", b"\n".join(toks) + b"\n"), TOK_OUT)
    assert len(got) == len(toks)
    want = np.array([float(t) for t in toks])
    assert not got["bad"].any() and np.array_equal(got["len"], [len(t) for t in toks])
    assert np.array_equal(ING.bits(got["bits"].view(np.float64)), ING.bits(want))
    br = [CV.token_branch(t) for t in toks]
    kinds = collections.Counter(b[0] for b in br)
    div = collections.Counter((b[1] >= 0, b[2]) for b in br if b[0] == "div")
    print("parser branches:", dict(kinds), "ingest_div (s >= 0, sh):", dict(div))
    assert min(kinds["small"], kinds["int"], kinds["div"]) >= 2000, kinds
    assert set(sh for _, sh in div) == {2, 3} and set(s for s, _ in div) == {True, False}, div
    assert all(CV.token_branch(t)[0] == "div" for t in pools["P2"] + pools["P2off"])
    # the round trip class: the dyadic values, which six decimals hold exactly, parse back to themselves
    trip, v = CV.p4(SEED + 4, 4000)
    back = np.array([float(t) for t in trip])
    assert trip == pools["P4"] and (back == v).sum() >= 500 and np.abs(back - v).max() <= 1e-6


# ---- the LAS record cores ------------------------------------------------------------------------------------
def test_las_cores_on_the_edge_classes(exes):
    """Every (scale, offset) pair x both variants, ~3 900 rows each: random values, quotient ties with
    both neighbours, the int32 edges (quotients rounding to -2^31 - 1, -2^31, 2^31 - 1, 2^31, the two .5
    ties among them) and the intensity edges, against tests/las.py; then gps times off the nanosecond
    grid and on the int64 edges through las_time_ns."""
    tmp, _, _, exe = exes
    plus = minus = refused = accepted = 0
    for scale in CV.LAS_SCALES:
        for off in CV.LAS_OFFSETS:
            _, _, edge = CV.las_coords(SEED, 300, scale, off)
            q = CV.las_quotient(edge, scale, off)
            assert set(np.rint(q).tolist()) == set(CV.LAS_EDGE_Q)
            X, b = LAS.fix(edge, scale, off)
            assert np.array_equal(b, (np.rint(q) == 2.0 ** 31) | (np.rint(q) == -2.0 ** 31 - 1))
            plus += int((q == 2147483647.5).sum())
            minus += int((q == -2147483648.5).sum())
            assert b[q == 2147483647.5].all() and not b[q == -2147483648.5].any()
            for variant in ("lmc", "csim"):
                imul, tmul, _ = LAS.VARIANTS[variant]
                rows, kind = CV.las_rows(SEED, 300, scale, off, variant)
                head = np.array([scale] * 3 + [off] * 3 + [imul, tmul]).tobytes()
                got = np.frombuffer(run(exe, tmp, "enc", head + np.ascontiguousarray(rows).tobytes()), ENC_OUT)
                bad = np.zeros(len(rows), bool)
                for k in range(3):
                    X, b = LAS.fix(rows[:, k], scale, off)
                    assert np.array_equal(got["X"][:, k], X), (scale, off, k)
                    bad |= b
                it, b = LAS.intensity(rows[:, 3], imul)
                assert np.array_equal(got["intensity"], it) and np.array_equal(got["bad"] != 0, bad | b)
                assert b[kind == "intensity"].tolist() == [True, False, False, True]
                assert not bad[kind != "edge"].any()
                refused += int((bad | b).sum())
                accepted += int((~(bad | b)).sum())
    print("LAS: accepted", accepted, "refused", refused, "exact ties at +2^31 - 0.5:", plus, "at -2^31 - 0.5:", minus)
    assert plus >= 10 and minus >= 10 and refused >= 2000 and accepted >= 100_000

    frames, no, (pos, neg) = CV.las_gps(SEED, 2000)
    gps = np.concatenate(frames + [no, pos, neg])
    assert (np.rint(np.concatenate(frames) * 1e9) != np.concatenate(frames) * 1e9).mean() > 0.5   # off the grid
    rec = np.zeros(len(gps), LAS.RECORD[3])
    rec["gps_time"] = gps
    head = np.array([3, 34], np.int64).tobytes() + np.array([0.01] * 3 + [0.0] * 3).tobytes()
    got = np.frombuffer(run(exe, tmp, "dec", head + rec.tobytes()), DEC_OUT)
    t, ok = LAS.time_ns(gps)
    assert np.array_equal(got["fits"] != 0, ok) and np.array_equal(got["t"][ok], t[ok])
    n_ok = sum(map(len, frames))
    assert ok[:n_ok].all() and not ok[n_ok:n_ok + len(no)].any() and ok[n_ok + len(no):].all()
    assert t[ok].max() == 2 ** 63 - 1024 and t[ok].min() == -2 ** 63
