"""Time the ingest decoders (ingest; csrc/ingest.hpp, f7): LVX v1.1 / CSIM lvx / lvx2 files and PCD /
XYZ / CSV text back into device rows or a batch.

Workload: 600 frames x 100 000 synthetic points (mc_batch_synth, MC_BATCH_WITH_TIME, frame starts at
10 Hz).  Each file is first written on the device by the existing encoders (mc_lvx_encode_batch,
mc_csim_lvx_encode_batch, mc_csim_text_encode_batch) and then decoded from that device copy.

    python tools/bench_ingest.py [--frames 600] [--points 100000] [--repeat 3] [--json out.json]

Per decoder: kernel time from HIP events (mc_timing_read_codec; median of --repeat), and once the wall
time of "host bytes -> H2D -> decode" (the file already read into memory; LVX: the host index walk
included).  Algorithmic bytes: LVX 14 B read per record + 41 B (rows and tag) or 20 B (batch) written;
text = the file read twice + 8 B per line of starts written and read + the output (8 B x columns, or
16 / 20 B per batch point) — the decode call itself reads the text three times (it repeats the count
pass of mc_text_lines), so its achieved traffic is higher than the algorithmic figure it is held to.
GB/s = algorithmic bytes over kernel time, set against 8 TB/s.  Beside each: this box's numpy decode
(np.frombuffer with a structured dtype; np.loadtxt, and pandas.read_csv when installed) timed on one
frame and multiplied by the frame count — labelled extrapolated.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys
import time
from ctypes import c_float, c_int64, c_uint8, c_uint64

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ex, ing, ptr = m.csim_export, m.ingest, m._lib.ptr
    ctx = m.Context(0)
    lib, h = ctx.lib, ctx.handle
    F = args.frames
    counts = np.full(F, args.points, np.int64)
    n = int(counts.sum())
    b = ctx.batch(counts, with_time=True)
    b.synth(seed=0, frame_id_base=1000)
    starts = np.array([int((1.7e9 + 0.1 * f) * 1e9) for f in range(F)], np.int64)
    b.set_frame_starts(starts)
    ts, ids = starts.astype(np.uint64), np.arange(F, dtype=np.uint64)
    sn, dtype, ext_on, ext = ex._device_fields(ex.DeviceInfo("3JEDK7M00100451", 1, "", True, 0.01, -0.02, 1.5, 1.2, -0.3, 1.8))
    cp = ptr(counts, c_int64)
    out = ctx.batch(counts, with_time=True)
    d_rows, d_tags = ctx.device_buffer(n * 40), ctx.device_buffer(n)
    result = {"frames": F, "points": n, "repeat": args.repeat, "cases": {}}

    def kernel_ms(call):
        rc = call()   # warm-up: scratch allocation, first launch
        if rc != 0:
            raise RuntimeError(f"decoder returned {rc}: {lib.mc_last_error().decode()}")
        ctx.timing(True)
        ctx.read_timing()
        ms = []
        for _ in range(args.repeat):
            call()
            ms.append(ctx.read_timing()["codec_ms"])
        ctx.timing(False)
        return float(np.median(ms)), ms

    def report(name, call, alg_bytes, wall_s=None, cpu=None):
        ms, all_ms = kernel_ms(call)
        gbs = alg_bytes / (ms * 1e-3) / 1e9
        r = {"us": ms * 1e3, "us_all": [v * 1e3 for v in all_ms], "algorithmic_bytes": alg_bytes, "GBps": gbs,
             "hbm_fraction": gbs * 1e9 / HBM_PEAK}
        if wall_s is not None:
            r["wall_ms_with_h2d"] = wall_s * 1e3
        if cpu:
            r["cpu_extrapolated_ms"] = cpu
        result["cases"][name] = r
        print(f"{name:22s} {ms * 1e3:10.1f} us {gbs:8.1f} GB/s {100 * gbs * 1e9 / HBM_PEAK:6.1f} % of 8 TB/s"
              + (f"   wall with H2D {wall_s * 1e3:8.1f} ms" if wall_s is not None else "")
              + ("".join(f"   {k} {v:.0f} ms (extrapolated)" for k, v in cpu.items()) if cpu else ""))

    print(f"{F} frames x {args.points} points = {n} points; median of {args.repeat}")
    # ---- LVX ----------------------------------------------------------------------------------------
    for name in ("lvx v1.1", "lvx", "lvx2"):
        if name == "lvx v1.1":
            size = int(m.codecs.lvx_layout(counts)[-1])
            enc = lambda o: lib.mc_lvx_encode_batch(h, b.handle, ptr(ids, c_uint64), ptr(ts, c_uint64), o, size)  # noqa: E731
        else:
            size = int(ex.lvx_layout(counts, name)[-1])
            enc = lambda o, v=ex.VERSIONS[name]: lib.mc_csim_lvx_encode_batch(  # noqa: E731
                h, v, b.handle, ptr(ts, c_uint64), None, ptr(sn, c_uint8), dtype, ext_on, ptr(ext, c_float), o, size)
        padded = (size + 15) // 16 * 16
        d_file = ctx.device_buffer(padded)
        assert enc(d_file.ptr) == 0, lib.mc_last_error()
        host = d_file.to_host(np.uint8)
        data = host[:size].tobytes()
        t0 = time.perf_counter()
        fmt, pos, slots, fids, fts, _ = ing._lvx_index(data)
        walk_ms = (time.perf_counter() - t0) * 1e3
        dcounts = ing._lvx_counts(ctx, fmt, d_file, size, pos, slots, False)
        assert np.array_equal(dcounts, counts), "the decoded counts differ from the encoded ones"
        pp, sp, dp, tp = ptr(pos, c_int64), ptr(slots, c_int64), ptr(dcounts, c_int64), ptr(fts, c_int64)
        cnt = np.zeros(F, np.int64)
        # this box's numpy decode of one frame's records
        rec = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("i", "u1"), ("t", "u1")]) if fmt != 1 else \
            np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("i", "u1"), ("t", "u1")])
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            if fmt == 0:
                pk = np.frombuffer(data, np.dtype([("h", "u1", 22), ("r", rec, 96)]), int(slots[0]) // 96,
                                   int(pos[0]) + 24)["r"].reshape(-1)
            else:
                pk = np.frombuffer(data, rec, int(slots[0]), int(pos[0]) + (12 if fmt == 1 else 45))
            one = np.empty((len(pk), 5))
            for k, c in enumerate("xyz"):
                one[:, k] = pk[c] / 1000.0 if fmt != 1 else pk[c]
            one[:, 3] = pk["i"] / 255.0 if fmt == 0 else pk["i"]
            one[:, 4] = float(fts[0])
            best = min(best, time.perf_counter() - t0)
        cpu = {"numpy frombuffer": best * 1e3 * F}

        def wall():
            t0 = time.perf_counter()
            d_file.from_host(host)
            f2, p2, s2, _, t2, _ = ing._lvx_index(data)
            c2 = ing._lvx_counts(ctx, f2, d_file, size, p2, s2, False)
            rc = lib.mc_lvx_decode_batch(h, f2, d_file.ptr, size, F, ptr(p2, c_int64), ptr(c2, c_int64), ptr(t2, c_int64),
                                         1000, out.handle, None)
            assert rc == 0, lib.mc_last_error()
            return time.perf_counter() - t0

        if fmt == 0:
            report(f"{name} trim", lambda: lib.mc_lvx_count(h, fmt, d_file.ptr, size, F, pp, sp, 0, ptr(cnt, c_int64)),
                   F * 96 * 14)
        report(f"{name} -> rows", lambda: lib.mc_lvx_decode(h, fmt, d_file.ptr, size, F, pp, dp, tp, 1000, d_rows.ptr, 5,
                                                             d_tags.ptr), n * (14 + 41))
        report(f"{name} -> batch", lambda: lib.mc_lvx_decode_batch(h, fmt, d_file.ptr, size, F, pp, dp, tp, 1000,
                                                                   out.handle, None), n * (14 + 20), wall(), cpu)
        result["cases"][f"{name} -> batch"]["host_index_walk_ms"] = walk_ms
        d_file.close()
        del host, data

    # ---- text -----------------------------------------------------------------------------------------
    bpos = np.zeros(F + 1, np.int64)
    for name, code in ex.FORMATS.items():
        cols, sep = (3, " ") if name == "xyz" else (5, "," if name == "csv" else " ")
        rc = lib.mc_csim_text_encode_batch(h, code, b.handle, None, 0, ptr(bpos, c_int64))
        assert rc == m._lib.MC_ERR_SPACE, rc
        size = int(bpos[-1])
        d_text = ctx.device_buffer((size + 15) // 16 * 16)
        assert lib.mc_csim_text_encode_batch(h, code, b.handle, d_text.ptr, size, ptr(bpos, c_int64)) == 0
        host = d_text.to_host(np.uint8)
        frame0 = host[:int(bpos[1])].tobytes()
        cpu = {}
        import io
        t0 = time.perf_counter()
        np.loadtxt(io.BytesIO(frame0.replace(b",,", b",nan,")), delimiter=None if sep == " " else ",")
        cpu["numpy loadtxt"] = (time.perf_counter() - t0) * 1e3 * F
        try:
            import pandas
            t0 = time.perf_counter()
            pandas.read_csv(io.BytesIO(frame0), sep=sep, header=None)
            cpu["pandas read_csv"] = (time.perf_counter() - t0) * 1e3 * F
        except ImportError:
            pass
        nl, bad = c_int64(), c_int64()
        d_out = ctx.device_buffer(n * cols * 8)
        tout = ctx.batch(counts, with_time=cols == 5)

        def wall():
            t0 = time.perf_counter()
            d_text.from_host(host)
            rc = lib.mc_text_decode_batch(h, ord(sep), cols, d_text.ptr, size, tout.handle, ptr(starts, c_int64), None,
                                          ctypes.byref(bad))
            assert rc == 0, lib.mc_last_error()
            return time.perf_counter() - t0

        report(f"{name} lines", lambda: lib.mc_text_lines(h, d_text.ptr, size, ctypes.byref(nl)), size)
        assert nl.value == n
        base = 2 * size + 16 * n
        report(f"{name} -> rows", lambda: lib.mc_text_decode(h, ord(sep), cols, d_text.ptr, size, n, d_out.ptr, cols,
                                                              ctypes.byref(bad)), base + 8 * cols * n)
        report(f"{name} -> batch", lambda: lib.mc_text_decode_batch(h, ord(sep), cols, d_text.ptr, size, tout.handle,
                                                                    ptr(starts, c_int64), None, ctypes.byref(bad)),
               base + (20 if cols == 5 else 16) * n, wall(), cpu)
        result["cases"][f"{name} -> batch"]["file_bytes"] = size
        for x in (d_text, d_out, tout):
            x.close()
        del host

    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    for x in (d_rows, d_tags, b, out):
        x.close()


if __name__ == "__main__":
    main()
