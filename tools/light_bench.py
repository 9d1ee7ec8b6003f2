#!/usr/bin/env python3
"""The voxel lighting (vtmc_terrain_light, include/vtmc_light.h) measured on a --cells^3 terrain (1024: 1026^3 samples, 4.3 GB): the
fBm-over-a-ramp terrain of the other benches, whose surface lies about the middle plane, so the upper half of the box is open sky.

  box_read       a plain device read of the box (vtmc_debug_nav_box_read_ms): what one read of the grid costs here
  flood          vtmc_terrain_flood of the same box, one level, 16 sources: another non-local pass over the open samples, in the same run
  whole_grid     a light call on the whole grid with sky (level 255, falloff 16) and 16 torches of level 255 (falloff 16) just above the
                 surface: host wall time (median and best of --reps), the round count, the device time of its three phases
  variants       the tiled rounds and the plain one-hop rounds ALTERNATED in one process, --reps calls each, and rounds per read-back
                 1, 4 and 16 for the variant the library keeps
  vertex_pass    vtmc_light_vertices on the extract of the same run (every block of the terrain)
  probe_100000   100 000 probes with their copies
  relight_64     an edit (a sphere dug at the surface), then a light call on a box of 64^3 cells around it: what a host pays in place of
                 an incremental update; beside it a plain read and a flood of that box, and the vertex pass on the edit's dirty blocks

Prints one JSON line; --out DIR also writes it to DIR/light_bench.json."""
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


def timed_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_best": round(float(np.min(ms)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    samples = (n + 2) ** 3
    rec = {"tool": "tools/light_bench.py", "terrain": "%d^3 cells, %d samples, %.2f GB" % (n, samples, 4 * samples / 1e9), "reps": a.reps}
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        _, tris = ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        rec["extract_triangles"] = tris

        def box_read(lower, upper):
            lo, up, ms = (ctypes.c_float * 3)(*lower), (ctypes.c_float * 3)(*upper), ctypes.c_float()
            ex._check(L.vtmc_debug_nav_box_read_ms(h, ctypes.byref(lo), ctypes.byref(up), 5, ctypes.byref(ms)))
            return round(ms.value, 3)

        def flood(lower, upper, level, places):
            src = np.zeros(len(places), vt.WATER_SOURCE_DTYPE)
            src["position"], src["level"] = np.asarray(places, np.float32), level
            ex.terrain_flood(src, lower, upper)   # the warm-up: the buffers are allocated here
            ms, (_, bodies) = timed_ms(lambda: ex.terrain_flood(src, lower, upper), a.reps)
            return dict(summary(ms), bodies=bodies, wet_samples=ex.water_info()[4])

        def light(params, src, lower, upper, reps):
            wall, phases = [], []
            for _ in range(reps):
                t, lit = timed_ms(lambda: ex.terrain_light(params, src, lower, upper), 1)
                stage = (ctypes.c_float * 3)()
                ex._check(L.vtmc_debug_light_ms(h, stage))
                wall += t
                phases.append(list(stage))
            p = np.median(np.asarray(phases), axis=0)
            info = ex.light_info()
            return dict(summary(wall), rounds=info[4], lit_sources=int(lit.sum()), sky_samples=info[2], torch_samples=info[3],
                        device_ms={"seeds": round(float(p[0]), 3), "relaxation": round(float(p[1]), 3), "count": round(float(p[2]), 3)})

        rng = np.random.default_rng(11)
        places = [(n * (i + 0.5) / 4, n / 2.0 + 0.03 * n, n * (j + 0.5) / 4) for i in range(4) for j in range(4)]
        torches = np.zeros(16, vt.LIGHT_SOURCE_DTYPE)
        torches["position"], torches["level"] = np.asarray(places, np.float32), 255
        params = vt.LightParams(255, 16, 16)
        rec["box_read_ms"] = box_read(**everything)
        rec["flood"] = flood(everything["lower"], everything["upper"], n / 2.0 + 0.02 * n, [(x, y - 0.02 * n, z) for x, y, z in places])

        # the two variants alternated in one process; the library's default is variant 0 with 4 rounds per read-back
        ex.terrain_light(params, torches, **everything)   # the warm-up: the buffers are allocated here
        variants = {"tiled": [], "plain": []}
        for _ in range(a.reps):
            for name, plain in (("tiled", 0), ("plain", 1)):
                ex._check(L.vtmc_debug_light_variant(h, plain, 4))
                variants[name].append(light(params, torches, everything["lower"], everything["upper"], 1))
        rec["variants"] = {}
        for name, runs in variants.items():
            rec["variants"][name] = dict(summary([r["ms_median"] for r in runs]), rounds=runs[0]["rounds"],
                                         relaxation_device_ms_median=round(float(np.median([r["device_ms"]["relaxation"] for r in runs])), 3))
        keeps = min(rec["variants"], key=lambda k: rec["variants"][k]["ms_median"])
        rec["variants"]["faster_end_to_end"] = keeps
        rec["rounds_per_read_back"] = {}
        for batch in (1, 4, 16):
            ex._check(L.vtmc_debug_light_variant(h, 0, batch))
            r = light(params, torches, everything["lower"], everything["upper"], 3)
            rec["rounds_per_read_back"][str(batch)] = {"ms_median": r["ms_median"], "ms_best": r["ms_best"], "rounds": r["rounds"]}
        ex._check(L.vtmc_debug_light_variant(h, 0, 4))
        rec["whole_grid"] = light(params, torches, everything["lower"], everything["upper"], a.reps)
        rec["whole_grid"]["times_the_box_read"] = round(rec["whole_grid"]["ms_median"] / rec["box_read_ms"], 1)
        rec["whole_grid"]["times_the_flood"] = round(rec["whole_grid"]["ms_median"] / rec["flood"]["ms_median"], 2)

        ex.light_vertices()
        ms, nv = timed_ms(ex.light_vertices, a.reps)
        rec["vertex_pass"] = dict(summary(ms), vertices=nv)
        q = np.stack([rng.uniform(0, n, 100000), rng.uniform(n / 2.0 - 0.05 * n, n / 2.0 + 0.1 * n, 100000), rng.uniform(0, n, 100000)], axis=1).astype(np.float32)
        ex.light_probe(q[:16])
        ms, (sky, torch) = timed_ms(lambda: ex.light_probe(q), 3)
        rec["probe_100000"] = dict(summary(ms), sky_lit=int((sky > 0).sum()), torch_lit=int((torch > 0).sum()))

        # an edit, and the relight of a box of 64^3 cells around it
        centre = (n / 2.0, n / 2.0, n / 2.0)
        n_dirty, t_edit = ex.terrain_update([vt.SphereModifier(centre, 6.0, False)])
        lower, upper = tuple(c - 32.0 for c in centre), tuple(c + 32.0 for c in centre)
        torch = np.zeros(1, vt.LIGHT_SOURCE_DTYPE)
        torch["position"], torch["level"] = np.asarray(centre, np.float32), 255
        ex.terrain_light(params, torch, lower, upper)
        rec["relight_64"] = light(params, torch, lower, upper, a.reps)
        rec["relight_64"].update(dirty_blocks=n_dirty, edit_triangles=t_edit, box_read_ms=box_read(lower, upper),
                                 flood=flood(lower, upper, n / 2.0, [(centre[0], centre[1] - 3.0, centre[2])]))
        ex.light_vertices()
        ms, nv = timed_ms(ex.light_vertices, a.reps)
        rec["relight_64"]["vertex_pass"] = dict(summary(ms), vertices=nv)
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "light_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
