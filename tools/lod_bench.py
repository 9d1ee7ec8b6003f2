#!/usr/bin/env python3
"""Level-of-detail extraction (vtmc_terrain_extract_lod) measured on a world build, beside the full-resolution extract of the same grid in
the same process with the same library:

  world   a resident terrain of 1024 x 256 x 1024 cells (--quick: 256 x 64 x 256): the island heightmap of tools/world_build_bench.py
          plus one whole-grid fBm NoiseModifier, one vtmc_terrain_update
  full    every block at full resolution: vtmc_extract_volumes_device on the resident grid itself (vtmc_terrain_device_grid), the dense
          route a full rebuild or vtmc_terrain_load takes -- wall time of the call (median and best of --reps), stage times, triangles and
          the bytes of their 76-byte records
  lod     vtmc_terrain_extract_lod with the viewer at the terrain's centre, split 2, max_level 0 .. 4: nodes (and how many per level),
          triangles, record bytes, bytes of the gathered tiles, wall time of the whole call, device time of lod_gather_kernel
          (vtmc_debug_lod_gather_ms), the extraction's stage times, the gather's bytes per second (4000 bytes stored per node, and
          4000 bytes of samples loaded), and the ratios against `full`: time, triangles, bytes
  box     tools/calib/mix2 4 box in a fresh process after the context is closed: the plain read / write / copy streams of this machine;
          every gather rate is also given as a fraction of the copy stream (the gather loads and stores the same number of bytes)

Prints one JSON line per record; --out DIR also appends them to DIR/lod_bench.jsonl."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import volumetricterrain_amd as vt
from world_build_bench import heightmap

LEVELS = (0, 1, 2, 3, 4)


def emit(out, name, rec):
    rec = dict(record=name, **rec)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "lod_bench.jsonl"), "a") as f:
            f.write(line + "\n")
    return rec


def timed_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "best_ms": round(float(min(ms)), 3), "reps": len(ms)}


def device_grid(ex):
    p, strides, dims = ctypes.c_void_p(), (ctypes.c_int64 * 3)(), (ctypes.c_int32 * 3)()
    ex._check(ex._L.vtmc_terrain_device_grid(ex._h, ctypes.byref(p), ctypes.byref(strides), ctypes.byref(dims)))
    return p.value, tuple(strides), tuple(d - 2 for d in dims)


def gather_ms(ex):
    ms = ctypes.c_float()
    ex._check(ex._L.vtmc_debug_lod_gather_ms(ex._h, ctypes.byref(ms)))
    return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="256 x 64 x 256 cells instead of 1024 x 256 x 1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--split", type=float, default=2.0)
    ap.add_argument("--no-box", action="store_true", help="skip tools/calib/mix2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, E, H = (256, 64, 256) if a.quick else (1024, 256, 1024)
    hm = heightmap(512)
    island = vt.IslandModifier(hm * (E * 0.6), float(W), float(H), float(E), True)
    noise = vt.NoiseModifier(1337, 6, 6.0 / W, 2.0, 0.5, "fbm", amplitude=E / 8.0, ramp_scale=1.0, ramp_center=E * 0.35, lower=(0.0, 0.0, 0.0),
                             upper=(W + 2.0, E + 2.0, H + 2.0))
    copy_TBps = None
    with vt.Extractor(0) as ex:
        ex.terrain_init(W, E, H, 1.0, (0.0, 0.0, 0.0), 5)
        n_dirty, T_build = ex.terrain_update([island, noise])
        emit(a.out, "world", {"cells": [W, E, H], "what": "island heightmap (512^2) + one whole-grid fBm noise modifier (6 octaves), one update",
                              "dirty_blocks": int(n_dirty), "triangles": int(T_build), "quick": bool(a.quick)})
        d_grid, strides, cells = device_grid(ex)
        ms, T_full = timed_ms(lambda: ex.extract_volumes_device(d_grid, cells, strides), a.reps + 1)
        full_ms = ms[1:]
        full = emit(a.out, "full", dict(summary(full_ms), triangles=int(T_full), record_bytes=76 * int(T_full), stage_ms=ex.last_stage_ms(),
                                        blocks=(W // 8) * (E // 8) * (H // 8)))
        assert T_full == T_build
        viewer = (W / 2.0, E / 2.0, H / 2.0)
        lods = []
        for level in LEVELS:
            if W % (8 << level) or E % (8 << level) or H % (8 << level):
                continue
            params = vt.LodParams(viewer, level, a.split, 1 << 20)
            ms, (n, T) = timed_ms(lambda: ex.terrain_extract_lod(params), a.reps + 1)
            ms = ms[1:]   # the first call allocates the tiles and, maybe, grows the output
            g = [gather_ms(ex)]
            for _ in range(a.reps - 1):
                ex.terrain_extract_lod(params)
                g.append(gather_ms(ex))
            nodes = ex.terrain_lod_nodes()
            best_g = min(g)
            rec = dict(summary(ms), max_level=level, split=a.split, nodes=int(n), nodes_per_level=np.bincount(nodes[:, 3], minlength=level + 1).tolist(),
                       triangles=int(T), record_bytes=76 * int(T), tile_bytes=4000 * int(n), stage_ms=ex.last_stage_ms(),
                       gather_ms={"median": round(float(np.median(g)), 4), "best": round(best_g, 4)},
                       gather_TBps_stored_plus_loaded=round(8000.0 * n / (best_g * 1e-3) / 1e12, 3) if best_g > 0 else None,
                       time_over_full=round(float(np.median(ms)) / full["median_ms"], 4), triangles_over_full=round(T / max(T_full, 1), 4),
                       record_bytes_over_full=round(T / max(T_full, 1), 4))
            lods.append(rec)
    vt.release_streams()
    if not a.no_box:
        exe = os.path.join(ROOT, "tools", "calib", "mix2")
        if os.path.exists(exe):
            p = subprocess.run([exe, "4", "box"], capture_output=True, text=True, timeout=300)
            rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode == 0 and rows:
                box = rows[-1]
                copy_TBps = box["copy_TBps"]
                emit(a.out, "box", {k: box[k] for k in ("read_TBps", "write_TBps", "copy_TBps", "device") if k in box})
            else:
                emit(a.out, "box", {"error": "tools/calib/mix2 4 box: exit code %d: %s" % (p.returncode, p.stderr.strip()[-300:])})
        else:
            emit(a.out, "box", {"error": "tools/calib/mix2 is not built (python -c 'import __graft_entry__ as g; g.build()')"})
    for rec in lods:
        if copy_TBps and rec["gather_TBps_stored_plus_loaded"]:
            rec["gather_over_copy_stream"] = round(rec["gather_TBps_stored_plus_loaded"] / copy_TBps, 3)
        emit(a.out, "lod", rec)


if __name__ == "__main__":
    main()
