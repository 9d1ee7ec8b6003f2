#!/usr/bin/env python3
"""Saving a session (vtmc_terrain_save / vtmc_terrain_load), measured in one run on a --size^3 terrain (default 1024: a plane, one
whole-grid fBm noise modifier and --edits sphere edits):

  read_stream  tools/calib/calib read: a plain float4 read stream of the grid's byte count (its own HIP events, best of 5)
  save / load  wall time of terrain_save and terrain_load (without and with the full extract), default and exact, and the file sizes
  dense        the route a host has without the brick file: terrain_read_samples + ndarray.tofile, np.fromfile + terrain_write_samples
  kernels      with --kernel-stats CSV (the kernel statistics of a `rocprofv3 --kernel-trace --stats` run over this tool): the
               brick-flag kernel's time and the TB/s that is of the grid's bytes, beside read_stream

Prints one JSON line per record; --out DIR also writes them to DIR/<record>.json."""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import volumetricterrain_amd as vt
from volumetricterrain_amd import terrainfile as tf


def emit(out, name, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name + ".json"), "w") as f:
            f.write(line + "\n")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, round((time.perf_counter() - t0) * 1e3, 1)


def kernel_stats(path, grid_bytes):
    """The brick kernels' rows of rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, MinNs, MaxNs, ...)."""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        for k in ("brick_flags_kernel", "brick_kinds_kernel", "brick_pack_kernel", "brick_unpack_kernel", "brick_redraw_kernel", "scan_fused_kernel"):
            if k in name:
                out[k] = {"calls": int(row["Calls"]), "avg_ms": round(float(row["AverageNs"]) / 1e6, 4), "min_ms": round(float(row["MinNs"]) / 1e6, 4),
                          "max_ms": round(float(row["MaxNs"]) / 1e6, 4)}
    if "brick_flags_kernel" in out:
        f = out["brick_flags_kernel"]
        f["grid_bytes"] = grid_bytes
        f["TBps_avg"] = round(grid_bytes / (f["avg_ms"] * 1e-3) / 1e12, 3)
        f["TBps_best"] = round(grid_bytes / (f["min_ms"] * 1e-3) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--edits", type=int, default=300)
    ap.add_argument("--dir", help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--kernel-stats", help="fold a rocprofv3 kernel statistics CSV of an earlier run of this tool into kernels.json and exit")
    ap.add_argument("--out")
    a = ap.parse_args()
    n = a.size
    grid_bytes = 4 * (n + 2) ** 3
    if a.kernel_stats:
        rec = {"what": "terrain_io kernels, rocprofv3 --kernel-trace --stats", "size": n, "kernels": kernel_stats(a.kernel_stats, grid_bytes)}
        stream = os.path.join(a.out or ".", "read_stream.json")
        if os.path.exists(stream) and "brick_flags_kernel" in rec["kernels"]:
            s = json.load(open(stream))
            rec["read_stream_TBps"] = s["TBps"]
            rec["flags_over_read_stream_best"] = round(rec["kernels"]["brick_flags_kernel"]["TBps_best"] / s["TBps"], 3)
            rec["flags_over_read_stream_avg"] = round(rec["kernels"]["brick_flags_kernel"]["TBps_avg"] / s["TBps"], 3)
        emit(a.out, "kernels", rec)
        return
    calib = os.path.join(ROOT, "tools", "calib", "calib")
    p = subprocess.run([calib, "read", str((grid_bytes + (1 << 20) - 1) >> 20)], capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit("tools/calib/calib read failed: " + p.stderr[-300:])
    emit(a.out, "read_stream", json.loads(p.stdout.strip().splitlines()[-1]))

    own_dir = None if a.dir else tempfile.TemporaryDirectory()
    d = a.dir or own_dir.name
    os.makedirs(d, exist_ok=True)
    path = lambda name: os.path.join(d, name)   # noqa: E731
    rng = np.random.default_rng(1)
    rec = {"what": "vtmc_terrain_save / vtmc_terrain_load, wall ms", "size": n, "grid_bytes": grid_bytes, "edits": a.edits}
    with vt.Extractor(0) as ex:
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 1)
        _, rec["build_plane_ms"] = timed(lambda: ex.terrain_update([vt.PlaneModifier(0.4 * n + 0.5, (-1, -1), (n + 8, n + 8), True)]))
        _, rec["build_noise_ms"] = timed(lambda: ex.terrain_update([vt.NoiseModifier(7, 6, 4.0 / n, amplitude=0.12 * n, ramp_scale=1.0, ramp_center=0.45 * n,
                                                                                     upper=(n + 8.0, n + 8.0, n + 8.0))]))
        for i in range(a.edits):
            c = (float(rng.uniform(0.1, 0.9) * n), float(rng.uniform(0.35, 0.55) * n), float(rng.uniform(0.1, 0.9) * n))
            ex.terrain_update([vt.SphereModifier(c, float(rng.uniform(6.0, 24.0)), bool(i & 1))])
        print("world built", flush=True)
        for exact in (False, True):
            key = "exact" if exact else "default"
            f = path(key + ".vtmt")
            ms = []
            for _ in range(3 if not exact else 1):
                size, t = timed(lambda: ex.terrain_save(f, exact=exact))
                ms.append(t)
            hdr = tf.read_header(f)
            nb = tf.brick_counts(hdr["dims"])
            rec["save_" + key] = {"ms": ms, "file_bytes": size, "n_raw": hdr["n_raw"], "bricks": nb[0] * nb[1] * nb[2],
                                  "grid_over_file": round(grid_bytes / size, 2)}
            print("saved", key, flush=True)
        if not a.no_dense:
            def dense_out():
                ex.terrain_read_samples().transpose(2, 1, 0).tofile(path("dense.f32"))
            _, t = timed(dense_out)
            rec["dense_save"] = {"ms": [t], "file_bytes": os.path.getsize(path("dense.f32")), "route": "terrain_read_samples + ndarray.tofile"}
            print("dense saved", flush=True)
    with vt.Extractor(0) as ex:
        for key in ("default", "exact"):
            (nd, T), t0 = timed(lambda: ex.terrain_load(path(key + ".vtmt"), extract=False))
            (nd, T), t1 = timed(lambda: ex.terrain_load(path(key + ".vtmt")))
            rec["load_" + key] = {"ms_no_extract": [t0], "ms_with_extract": [t1], "dirty_blocks": nd, "triangles": T}
            print("loaded", key, flush=True)
        if not a.no_dense:
            def dense_in():
                g = np.fromfile(path("dense.f32"), np.float32).reshape(n + 2, n + 2, n + 2).transpose(2, 1, 0)
                ex.terrain_write_samples(g)
            _, t = timed(dense_in)
            rec["dense_load"] = {"ms": [t], "route": "np.fromfile + terrain_write_samples (no extract)"}
    rec["save_default_over_dense"] = round(rec["dense_save"]["ms"][0] / min(rec["save_default"]["ms"]), 2) if not a.no_dense else None
    rec["load_default_over_dense"] = round(rec["dense_load"]["ms"][0] / rec["load_default"]["ms_no_extract"][0], 2) if not a.no_dense else None
    vt.release_streams()
    emit(a.out, "terrain_io_bench", rec)
    if own_dir:
        own_dir.cleanup()


if __name__ == "__main__":
    main()
