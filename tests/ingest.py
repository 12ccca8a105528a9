"""A plain numpy / Python statement of what the ingest decoders (f7) must return, written from the
format descriptions alone: a structured-dtype ``np.frombuffer`` walk over the three LVX layouts and
``float(token)`` per text field.  The GPU tests compare the kernels with it bit for bit; the CPU
tests compare the host index walk with it.  (oracle/ is frozen; this mirrors tests/csimexport.py.)

Rows are (N, 5) float64 = x, y, z, intensity, timestamp_ns.
"""
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

V11, LEGACY, LVX2 = 0, 1, 2
REC_MM = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("i", "u1"), ("tag", "u1")])
REC_F32 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("i", "u1"), ("tag", "u1")])
PKG = np.dtype([("hdr", "u1", 14), ("ts", "<u8"), ("rec", REC_MM, 96)])
assert REC_MM.itemsize == 14 and PKG.itemsize == 1366


def sniff(data: bytes) -> int:
    if data[:10] == b"livox_file":
        return LEGACY
    if data[:10] == b"livox_tech":
        return LVX2 if data[10:16] == b"2.0.0\x00" else V11
    raise ValueError("unknown signature")


def lvx_walk(data: bytes):
    """-> dict(format, frame_pos (F + 1), slots, ids, ts, recs: per frame a structured array of its
    record slots, pkg_ts: per frame the timestamp of each slot's package (V11) or None)."""
    fmt = sniff(data)
    pos = 60 if fmt == LEGACY else 88
    fp, slots, ids, ts, recs, pkg_ts = [], [], [], [], [], []
    while pos < len(data):
        fp.append(pos)
        if fmt == V11:
            own, nxt, fid = np.frombuffer(data, "<u8", 3, pos)
            assert own == pos
            end = int(nxt) if nxt else len(data)
            k = (end - pos - 24) // 1366
            pk = np.frombuffer(data, PKG, k, pos + 24)
            recs.append(pk["rec"].reshape(-1))
            pkg_ts.append(np.repeat(pk["ts"].astype(np.int64), 96))
            slots.append(96 * k); ids.append(int(fid)); ts.append(int(pk["ts"][0]) if k else -1)
            pos = end
        elif fmt == LEGACY:
            t = int(np.frombuffer(data, "<u8", 1, pos)[0]); n = int(np.frombuffer(data, "<u4", 1, pos + 8)[0])
            recs.append(np.frombuffer(data, REC_F32, n, pos + 12)); pkg_ts.append(None)
            slots.append(n); ids.append(len(ids)); ts.append(t)
            pos += 12 + 14 * n
        else:
            fid = int(np.frombuffer(data, "<u4", 1, pos)[0]); t = int(np.frombuffer(data, "<u8", 1, pos + 4)[0])
            n = int(np.frombuffer(data, "<u4", 1, pos + 12)[0])
            recs.append(np.frombuffer(data, REC_MM, n, pos + 45)); pkg_ts.append(None)
            slots.append(n); ids.append(fid); ts.append(t)
            pos += 45 + 14 * n
    fp.append(len(data))
    return dict(format=fmt, frame_pos=np.array(fp, np.int64), slots=np.array(slots, np.int64),
                ids=np.array(ids, np.uint64), ts=np.array(ts, np.int64), recs=recs, pkg_ts=pkg_ts)


def device_block(data: bytes):
    """-> (sn, device_type, extrinsic_enable, 6 float32)."""
    fmt = sniff(data)
    o_sn, o_ty, o_en, o_ext = {V11: (29, 62, 63, 64), LEGACY: (28, 44, None, None), LVX2: (32, 48, 49, 50)}[fmt]
    sn = data[o_sn:o_sn + 16].split(b"\x00")[0].decode("ascii")
    en = bool(data[o_en]) if o_en is not None else False
    ext = np.frombuffer(data, "<f4", 6, o_ext) if o_ext is not None else np.zeros(6, np.float32)
    return sn, data[o_ty], en, ext


def lvx_trimmed(recs: np.ndarray) -> int:
    """V11: the slots of a frame less the trailing all-zero records of its last package."""
    if len(recs) == 0:
        return 0
    last = recs[-96:]
    nz = np.flatnonzero((last["x"] != 0) | (last["y"] != 0) | (last["z"] != 0) | (last["i"] != 0) | (last["tag"] != 0))
    return len(recs) - 96 + (int(nz[-1]) + 1 if len(nz) else 0)


def lvx_rows(data: bytes, keep_padding=False, point_period_ns=0):
    """-> (walk, counts, rows (N, 5) float64, tags (N,) uint8)."""
    w = lvx_walk(data)
    fmt = w["format"]
    counts, rows, tags = [], [], []
    for f, rec in enumerate(w["recs"]):
        n = len(rec) if (fmt != V11 or keep_padding) else lvx_trimmed(rec)
        rec = rec[:n]
        r = np.empty((n, 5), np.float64)
        for k, name in enumerate("xyz"):
            r[:, k] = rec[name].astype(np.float64) if fmt == LEGACY else rec[name].astype(np.float64) / 1000.0
        r[:, 3] = rec["i"].astype(np.float64) / 255.0 if fmt == V11 else rec["i"].astype(np.float64)
        base = w["pkg_ts"][f][:n] if fmt == V11 else np.full(n, w["ts"][f], np.int64)
        r[:, 4] = (base + np.arange(n, dtype=np.int64) * int(point_period_ns)).astype(np.float64)
        counts.append(n); rows.append(r); tags.append(rec["tag"].copy())
    rows = np.concatenate(rows) if rows else np.zeros((0, 5))
    tags = np.concatenate(tags) if tags else np.zeros(0, np.uint8)
    return w, np.array(counts, np.int64), rows, tags


# ---- text ------------------------------------------------------------------------------------------
TOKEN = re.compile(rb"[+-]?\d+(\.\d*)?$")


def in_window(tok: bytes) -> bool:
    """The device parser's window: [+-]digits[.digits] with, after stripping the sign, the leading zeros
    and the fraction's trailing zeros, at most 19 significant and 19 fractional digits; nan, inf, -inf."""
    if tok in (b"nan", b"inf", b"-inf", b"+inf"):
        return True
    if not TOKEN.match(tok):
        return False
    t = tok.lstrip(b"+-")
    ip, _, fr = t.partition(b".")
    fr = fr.rstrip(b"0")
    return len(fr) <= 19 and len((ip + fr).lstrip(b"0")) <= 19


def body_of(data: bytes, fmt: str) -> bytes:
    if fmt == "pcd":
        return data[data.index(b"DATA ascii\n") + 11:]
    if fmt == "csv":
        return data[data.index(b"\n") + 1:]
    return data


def text_lines(body: bytes):
    """The non-empty lines (a line holding nothing or a lone '\\r' is skipped), without '\\n' / trailing '\\r'."""
    out = []
    for ln in body.split(b"\n"):
        if ln in (b"", b"\r"):
            continue
        out.append(ln[:-1] if ln.endswith(b"\r") else ln)
    return out


def line_fields(line: bytes, sep: bytes):
    return line.split(sep)


def parse_lines(lines, sep: bytes, ncols: int) -> np.ndarray:
    """float(token) per field; an empty CSV field is NaN."""
    out = np.empty((len(lines), ncols), np.float64)
    for i, ln in enumerate(lines):
        fs = ln.split(sep)
        assert len(fs) == ncols, (i, ln)
        out[i] = [float("nan") if (f == b"" and sep == b",") else float(f) for f in fs]
    return out


def first_outside(lines, sep: bytes):
    """1-based index of the first line holding a token outside the window, or None."""
    for i, ln in enumerate(lines):
        if any(not (in_window(f) or (f == b"" and sep == b",")) for f in ln.split(sep)):
            return i + 1
    return None


def bits(a) -> np.ndarray:
    """float64 -> uint64 bit patterns with every NaN folded to one pattern (NaN by position)."""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = 0x7FF8000000000000
    return b
