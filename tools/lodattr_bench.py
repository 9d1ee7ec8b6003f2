#!/usr/bin/env python3
"""The level-of-detail materials and occlusion (vtmc_lod_material_vertices, vtmc_lod_ao_vertices, include/vtmc_lodattr.h) measured on the
scene of tools/lodskirt_bench.py: a --cells^3 terrain (1024: 1026^3 samples, 4.3 GB) of fBm over a ramp, meshed by
vtmc_terrain_extract_lod with the viewer at the terrain's centre, roots of --max-level (4) and splits 1 and 2, in soup and indexed mode.

Per split and mode, medians of --reps calls after one call that is not timed:
  extract_lod, lod_skirts   of the same run (host wall time), and record_read, a plain device read of the result's records
  materials, ao             each compute call (host wall time); for the occlusion also the device time of the nodes' kernel and of the
                            skirts' pass, and the route counters
  ab_routes                 the occlusion with every node on the strided LDS staging against every node on the direct route
  ab_skirts                 the skirt quads in a pass of their own against the node's own workgroup taking them (the library's choice)
The two A/B comparisons alternate in this one process, two rounds of each.  The direct route is forced for every node, level 0 included:
the threshold is one number for all levels; nodes_per_level says how many of them are of level >= 1.
Once per run: the device time of the occlusion's nodes' kernel on selections of one level each (the viewer far away, roots of level L).

Prints one JSON line; --out DIR also writes it to DIR/lodattr_bench.json."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--max-level", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=4.0, help="occlusion radius in world units (the voxel scale is 1)")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    samples = (n + 2) ** 3
    rec = {"tool": "tools/lodattr_bench.py", "terrain": "%d^3 cells, %d samples, %.2f GB" % (n, samples, 4 * samples / 1e9), "max_level": a.max_level,
           "radius": a.radius, "steps": a.steps, "reps": a.reps, "cases": [], "ao_kernel_ms_per_level": {}}
    occlusion = vt.AmbientOcclusion(a.radius, 1.0, a.steps)
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        ex.material_init(8)
        viewer = (n / 2.0, n / 2.0, n / 2.0)

        def wall(fn):
            """the median and the best of --reps calls, milliseconds, after one call that is not timed"""
            fn()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            return {"ms_median": round(float(np.median(t)), 3), "ms_best": round(float(np.min(t)), 3)}

        def ao(direct_max=-1, in_node=1):
            """the occlusion call under a route threshold and a skirt variant: wall time, the two device times, the routes"""
            counts, ms = (ctypes.c_uint32 * 2)(), (ctypes.c_float * 2)()
            ex._check(L.vtmc_debug_lodattr_routes(h, None, direct_max))
            ex._check(L.vtmc_debug_lodattr_skirts_in_node(h, in_node))
            ex.lod_ao_vertices(occlusion)
            t, dev = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ex.lod_ao_vertices(occlusion)
                t.append((time.perf_counter() - t0) * 1e3)
                ex._check(L.vtmc_debug_lodattr_ms(h, ms))
                dev.append(list(ms))
            ex._check(L.vtmc_debug_lodattr_routes(h, counts, -1))
            ex._check(L.vtmc_debug_lodattr_skirts_in_node(h, 1))
            d = np.median(np.asarray(dev), axis=0)
            return {"ms_median": round(float(np.median(t)), 3), "ms_best": round(float(np.min(t)), 3), "nodes_kernel_ms": round(float(d[0]), 4),
                    "skirts_pass_ms": round(float(d[1]), 4), "staged": int(counts[0]), "direct": int(counts[1])}

        for split in (1.0, 2.0):
            for indexed in (False, True):
                ex.set_output_mode(indexed)
                params = vt.LodParams(viewer, a.max_level, split, 1 << 20)
                extract = wall(lambda: ex.terrain_extract_lod(params, a.max_level))
                nodes, T = ex.last_counts()
                read_ms = ctypes.c_float()
                ex._check(L.vtmc_debug_lodskirt_read_ms(h, a.reps, ctypes.byref(read_ms)))
                skirts = wall(lambda: ex.lod_skirts(1.0))
                case = {"split": split, "mode": "indexed" if indexed else "soup", "nodes": int(nodes), "triangles": int(T),
                        "nodes_per_level": np.bincount(ex.terrain_lod_nodes()[:, 3], minlength=a.max_level + 1).tolist(), "skirt_triangles": ex.lodskirt_info()[2],
                        "extract_lod": extract, "lod_skirts": skirts, "record_read_ms": round(read_ms.value, 4),
                        "materials": wall(ex.lod_material_vertices), "ao": ao()}
                case["vertices"], case["skirt_vertices"] = ex.lodattr_info(vt._lib.LODATTR_AO)
                case["ab_routes"] = [{"staged": ao(0), "direct": ao(1 << 30)} for _ in range(2)]
                case["ab_skirts"] = [{"own_pass": ao(-1, 0), "in_node": ao(-1, 1)} for _ in range(2)]
                rec["cases"].append(case)
        # one level at a time: the viewer far away, so no root splits
        ex.set_output_mode(False)
        for level in range(a.max_level + 1):
            ex.terrain_extract_lod(vt.LodParams((1e7, 1e7, 1e7), level, 1.0, 1 << 24), level)
            r = ao(0)
            rec["ao_kernel_ms_per_level"][str(level)] = {"nodes": ex.last_counts()[0], "vertices": ex.lodattr_info(vt._lib.LODATTR_AO)[0], "nodes_kernel_ms": r["nodes_kernel_ms"]}
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "lodattr_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
