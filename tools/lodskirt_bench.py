#!/usr/bin/env python3
"""The level-of-detail skirts (vtmc_lod_skirts, include/vtmc_lodskirt.h) measured on a --cells^3 terrain (1024: 1026^3 samples, 4.3 GB):
the fBm-over-a-ramp terrain of the other benches, whose surface lies about the middle plane, meshed by vtmc_terrain_extract_lod with the
viewer at the terrain's centre, roots of --max-level (4) and splits 1 and 2, in soup and in indexed mode.

Per split and mode, medians of --reps calls:
  extract_lod   the vtmc_terrain_extract_lod of the same run (host wall time)
  record_read   a plain device read of the result's records, 16 bytes a lane (vtmc_debug_lodskirt_read_ms)
  skirts        vtmc_lod_skirts at depth 1, for both store variants of the emit kernel, called alternately in this one process (direct: a
                lane stores its records dword by dword; staged: the tile's records are put together in LDS and leave as 16-byte pieces):
                host wall time and the device time of the four stages (count kernel, scan, emit kernel, node offsets)
and the node, flagged-node, triangle and skirt counts.  all_faces is measured once per split with the direct stores.

Prints one JSON line; --out DIR also writes it to DIR/lodskirt_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import volumetricterrain_amd as vt

STAGES = ("count", "scan", "emit", "offsets")


def timed_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--max-level", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    samples = (n + 2) ** 3
    rec = {"tool": "tools/lodskirt_bench.py", "terrain": "%d^3 cells, %d samples, %.2f GB" % (n, samples, 4 * samples / 1e9), "max_level": a.max_level, "depth": a.depth,
           "reps": a.reps, "cases": []}
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        viewer = (n / 2.0, n / 2.0, n / 2.0)

        def skirts(staged, all_faces=False):
            """medians of --reps calls: wall time and the four stages"""
            ex._check(L.vtmc_debug_lodskirt_store(h, int(staged)))
            wall, stages, count = [], [], 0
            for _ in range(a.reps):
                t, count = timed_ms(lambda: ex.lod_skirts(a.depth, all_faces), 1)
                ms = (ctypes.c_float * 4)()
                ex._check(L.vtmc_debug_lodskirt_ms(h, ms))
                wall += t
                stages.append(list(ms))
            p = np.median(np.asarray(stages), axis=0)
            return {"ms_median": round(float(np.median(wall)), 3), "ms_best": round(float(np.min(wall)), 3),
                    "device_ms": {k: round(float(v), 4) for k, v in zip(STAGES, p)}, "skirt_triangles": int(count)}

        for split in (1.0, 2.0):
            for indexed in (False, True):
                ex.set_output_mode(indexed)
                params = vt.LodParams(viewer, a.max_level, split, 1 << 20)
                ex.terrain_extract_lod(params, a.max_level)   # the warm-up: the tiles and the output are allocated here
                ms, (nodes, T) = timed_ms(lambda: ex.terrain_extract_lod(params, a.max_level), a.reps)
                read_ms = ctypes.c_float()
                ex._check(L.vtmc_debug_lodskirt_read_ms(h, a.reps, ctypes.byref(read_ms)))
                levels = np.bincount(ex.terrain_lod_nodes()[:, 3], minlength=a.max_level + 1).tolist()
                ex.lod_skirts(a.depth)           # the warm-up of the skirts' own buffers
                ex._check(L.vtmc_debug_lodskirt_store(h, 1))
                ex.lod_skirts(a.depth)
                direct, staged = skirts(False), skirts(True)
                direct2, staged2 = skirts(False), skirts(True)   # the two variants alternate: a second round of each
                case = {"split": split, "mode": "indexed" if indexed else "soup", "nodes": int(nodes), "nodes_per_level": levels, "flagged_nodes": ex.lodskirt_info()[1],
                        "triangles": int(T), "record_bytes": int(ex.last_counts()[1]) * 76 if not indexed else None,
                        "extract_lod_ms_median": round(float(np.median(ms)), 3), "record_read_ms": round(read_ms.value, 4),
                        "skirts_direct": [direct, direct2], "skirts_staged": [staged, staged2]}
                if not indexed:
                    case["skirts_all_faces_direct"] = skirts(False, True)
                    case["all_faces_flagged_nodes"] = ex.lodskirt_info()[1]
                rec["cases"].append(case)
        ex._check(L.vtmc_debug_lodskirt_store(h, 0))
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "lodskirt_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
