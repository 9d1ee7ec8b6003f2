#!/usr/bin/env python3
"""The flood (vtmc_terrain_flood, include/vtmc_water.h) measured on a full-grid box of a --cells^3 terrain (1024: 1026^3 samples,
4.3 GB): the fBm-over-a-ramp terrain of the other benches, whose surface lies about the middle plane.

  box_read       a plain device read of the box (vtmc_debug_nav_box_read_ms): what one read of the grid costs here
  fragments      vtmc_terrain_fragments with dst = NULL on the same box: the same labelling scheme on the solid samples, one pass
  sea            one level a little above the middle plane, 64 sources on a grid of places just under it (those in rock are dry): one
                 labelling pass over the open samples under the level, then the statistics and the volume
  lakes          eight levels around the middle plane, 32 sources each at seeded places just under their level: eight labelling passes
Each flood is given as host wall time (median and best of --reps), as the device time of its three phases (the levels' labelling with
numbering and assignment, the statistics, the volume kernel; medians) and as a multiple of the fragment query.  water_extract of the
sea's volume and 100 000 probes are timed once.

Prints one JSON line; --out DIR also writes it to DIR/water_bench.json."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    samples = (n + 2) ** 3
    rec = {"tool": "tools/water_bench.py", "terrain": "%d^3 cells, %d samples, %.2f GB" % (n, samples, 4 * samples / 1e9), "reps": a.reps}
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        lo, up = (ctypes.c_float * 3)(*everything["lower"]), (ctypes.c_float * 3)(*everything["upper"])
        read_ms = ctypes.c_float()
        ex._check(L.vtmc_debug_nav_box_read_ms(h, ctypes.byref(lo), ctypes.byref(up), 5, ctypes.byref(read_ms)))
        rec["box_read_ms"] = round(read_ms.value, 3)
        count = ctypes.c_int32()

        def fragments():
            ex._check(L.vtmc_terrain_fragments(h, ctypes.byref(lo), ctypes.byref(up), 0, 0, None, 0, ctypes.byref(count)))
            return count.value
        fragments()   # the warm-up: the scratch is allocated here
        ms, found = timed_ms(fragments, a.reps)
        frag_ms = float(np.median(ms))
        rec["fragments_count_only"] = {"ms_median": round(frag_ms, 2), "ms_best": round(float(np.min(ms)), 2), "fragments": found}

        rng = np.random.default_rng(11)
        sea_level = n / 2.0 + 0.02 * n
        places = [(n * (i + 0.5) / 8, n * (j + 0.5) / 8) for i in range(8) for j in range(8)]
        sea = [(x, sea_level - 1.0, z, sea_level) for x, z in places]
        lakes = []
        for k in range(8):
            level = n / 2.0 + (k - 4) * 0.015 * n + 0.25
            lakes += [(float(rng.uniform(0.05, 0.95) * n), level - 1.0, float(rng.uniform(0.05, 0.95) * n), level) for _ in range(32)]
        for name, sources in (("sea", sea), ("lakes", lakes)):
            src = np.zeros(len(sources), vt.WATER_SOURCE_DTYPE)
            rows = np.asarray(sources, np.float32)
            src["position"], src["level"] = rows[:, :3], rows[:, 3]
            ex.terrain_flood(src, **everything)   # the warm-up: the buffers are allocated here
            wall, phases = [], []
            for _ in range(a.reps):
                t, (source_body, bodies) = timed_ms(lambda: ex.terrain_flood(src, **everything), 1)
                stage = (ctypes.c_float * 3)()
                ex._check(L.vtmc_debug_water_ms(h, stage))
                wall += t
                phases.append(list(stage))
            med = float(np.median(wall))
            p = np.median(np.asarray(phases), axis=0)
            info = ex.water_info()
            recs = ex.water_bodies()
            rec[name] = {"sources": len(src), "levels": len(set(rows[:, 3].tolist())), "bodies": bodies, "dry_sources": int((source_body < 0).sum()), "wet_samples": info[4],
                         "largest_body_samples": int(recs["n_samples"].max()) if len(recs) else 0, "at_a_face": int((recs["flags"] & 1).sum()),
                         "ms_median": round(med, 2), "ms_best": round(float(np.min(wall)), 2),
                         "device_ms": {"levels": round(float(p[0]), 2), "statistics": round(float(p[1]), 2), "volume": round(float(p[2]), 2)},
                         "times_the_fragment_query": round(med / frag_ms, 2), "times_the_box_read": round(med / read_ms.value, 1)}
            if name == "sea":
                t, tris = timed_ms(ex.water_extract, 1)
                rec["sea"]["water_extract"] = {"ms": round(t[0], 2), "triangles": tris}
                q = np.stack([rng.uniform(0, n, 100000), rng.uniform(n / 2.0 - 0.05 * n, sea_level, 100000), rng.uniform(0, n, 100000)], axis=1).astype(np.float32)
                ex.water_probe(q[:16])
                t, (body, depth) = timed_ms(lambda: ex.water_probe(q), 3)
                rec["sea"]["probe_100000"] = {"ms_median": round(float(np.median(t)), 3), "wet": int((body >= 0).sum())}
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "water_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
