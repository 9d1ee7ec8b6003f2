#!/usr/bin/env python3
"""Per-vertex ambient occlusion (vtmc_ao_*) measured on the benchmark's field:

  full   a resident terrain of N^3 cells (N = 1024; --quick: 256) filled by one fBm NoiseModifier with bench.py's fbm8 parameters
         (8 octaves, f = 4/N, ramp 2/N around N/2), every block extracted; then vtmc_ao_vertices on that result, in soup and in indexed
         mode, at (radius, steps) = (2 cells, 2), (4, 4) and (6, 8): time of the call (launch + wait on the device; median and best of
         --reps), vertices per second at the best time, the LDS bytes of a workgroup (tile + record chunk + output bytes), and how many
         workgroups staged a tile or took the direct route.  For scale: vtmc_material_vertices (C = 128) on the same result.
         --direct-max N also runs (4, 4) with blocks of up to N vertices on the direct route (0: none; a large N: all), one entry each.
  edit   one SphereModifier dig of 64 dirty blocks (radius 1.4 blocks at the surface): time of vtmc_terrain_update alone, and of the
         update followed by vtmc_ao_vertices at (4, 4): the latency the call adds to an edit

Prints one JSON line; --out DIR also writes it to DIR/ao_bench.json."""
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

CASES = [(2.0, 2), (4.0, 4), (6.0, 8)]   # (radius in cells, steps)
RECORD_LDS = {False: (128 * 19 + 4) * 4 + (384 // 4 + 2) * 4, True: (256 * 6 + 4) * 4 + (256 // 4 + 2) * 4}   # csrc/terrain_ao.hip


def timed_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "best_ms": round(float(min(ms)), 3), "reps": len(ms)}


def fbm_world(ex, n):
    ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 1)
    m = vt.NoiseModifier(1337, 8, 4.0 / n, 2.0, 0.5, "fbm", ramp_scale=2.0 / n, ramp_center=n / 2.0, lower=(0.0, 0.0, 0.0),
                         upper=(n + 2.0, n + 2.0, n + 2.0))
    return ex.terrain_update([m])


def routes(ex, direct_max=-2):
    c = (ctypes.c_uint32 * 2)()
    ex._L.vtmc_debug_ao_routes(ex._h, ctypes.byref(c), direct_max)
    return {"tile_workgroups": int(c[0]), "direct_workgroups": int(c[1])}


def ao_case(ex, radius, steps, reps, indexed):
    p = vt.AmbientOcclusion(radius, 1.0, steps)
    ms, count = timed_ms(lambda: ex.ao_vertices(p), reps + 1)
    ms = ms[1:]   # the first call allocates the bytes
    r = summary(ms)
    reach = int(np.ceil(radius))
    r.update({"radius_cells": radius, "steps": steps, "vertices": int(count), "gvertices_per_s_at_best": round(count / (min(ms) * 1e-3) / 1e9, 3),
              "lds_bytes_per_workgroup": 4 * (10 + 2 * reach) ** 3 + RECORD_LDS[indexed]})
    r.update(routes(ex))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="256^3 cells instead of 1024^3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--direct-max", type=int, nargs="*", default=[], help="extra runs of (4 cells, 4 steps) with this route threshold")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = 256 if args.quick else 1024
    rec = {"tool": "tools/ao_bench.py", "quick": bool(args.quick), "cells": n,
           "world": "%d^3 cells, one fBm NoiseModifier (8 octaves, f = 4/N, ramp 2/N around N/2), every block extracted" % n}
    for indexed in (False, True):
        with vt.Extractor(0) as ex:
            ex.set_output_mode(indexed)
            n_dirty, T = fbm_world(ex, n)
            r = {"triangles": int(T), "dirty_blocks": int(n_dirty), "emit_stage_ms": round(float(ex.last_stage_ms()["emit"]), 3)}
            r["cases"] = [ao_case(ex, radius, steps, args.reps, indexed) for radius, steps in CASES]
            r["direct_max"] = []
            for dm in args.direct_max:
                routes(ex, dm)
                c = ao_case(ex, 4.0, 4, args.reps, indexed)
                c["direct_max"] = dm
                r["direct_max"].append(c)
            routes(ex, -1)
            ex.material_init(8)
            ms, _ = timed_ms(ex.material_vertices, args.reps + 1)
            r["material_vertices"] = summary(ms[1:])
            if not indexed:
                # a dig at the surface (the ramp's centre) that dirties 4 x 4 x 4 blocks: alternate add / erode so that every update edits
                c, rad = (n / 2.0 + 0.5, n / 2.0 + 0.5, n / 2.0 + 0.5), 11.0
                p = vt.AmbientOcclusion(4.0, 1.0, 4)
                alone, both, dirty = [], [], 0
                for k in range(2 * (args.reps + 1)):
                    mod = vt.SphereModifier(c, rad, k % 2 == 1)
                    t0 = time.perf_counter()
                    dirty, _ = ex.terrain_update([mod])
                    t1 = time.perf_counter()
                    nv = ex.ao_vertices(p)
                    t2 = time.perf_counter()
                    if k >= 2:
                        alone.append((t1 - t0) * 1e3)
                        both.append((t2 - t1) * 1e3)
                rec["edit"] = {"dirty_blocks": int(dirty), "vertices": int(nv), "terrain_update": summary(alone), "ao_vertices_after_it": summary(both)}
            rec["indexed" if indexed else "soup"] = r
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "ao_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
