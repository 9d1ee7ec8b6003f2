#!/usr/bin/env python3
"""The fragment query (vtmc_terrain_fragments) and the detach modifier (VTMC_MOD_DETACH) measured on a full-grid box of a
1024 x 1024 x 1024-cell terrain (1026^3 samples, 4.3 GB): an fBm terrain after --digs sphere erodes at seeded places.

  read_stream   tools/calib/calib read: a plain float4 read stream of the grid's byte count (its own HIP events, best of 5), in the same
                run: what one read of the grid costs on this machine
  query_count   vtmc_terrain_fragments with dst = NULL over the whole grid: the labelling (local, merge, anchors, flatten + counts), the
                fragment count and the read-back of the control words; host wall time, median and best of --reps
  query_list    the same with the records: two more passes over the labels (select, bounds) and the copy of the records
  detach        VTMC_MOD_DETACH over the whole grid, as a difference: a queue of 3 against a queue of 1 (a vtmc_terrain_update also
                extracts the dirty blocks, here all of them; the kernels of a queue run back to back on one stream),
                (median t3 - median t1) / 2.  The first detach removes the fragments; the timed ones find none and still label, read and
                test every sample.
Each time is also given as a multiple of the read stream's time for the grid.

Prints one JSON line; --out DIR also writes it to DIR/fragments_bench.json."""
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


def timed_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def summary(ms, read_ms):
    med, best = float(np.median(ms)), float(np.min(ms))
    return {"ms_median": round(med, 2), "ms_best": round(best, 2), "reads_of_the_grid_median": round(med / read_ms, 2),
            "reads_of_the_grid_best": round(best / read_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--digs", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.cells
    samples = (n + 2) ** 3
    grid_bytes = 4 * samples
    rec = {"tool": "tools/fragments_bench.py", "terrain": "%d^3 cells, %d samples, %.2f GB" % (n, samples, grid_bytes / 1e9), "digs": a.digs, "reps": a.reps,
           "scratch_GB": round(8 * samples / 1e9, 2)}

    calib = os.path.join(ROOT, "tools", "calib", "calib")
    p = subprocess.run([calib, "read", str((grid_bytes + (1 << 20) - 1) >> 20)], capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit("tools/calib/calib read failed (build it with hipcc from tools/calib/calib.hip): " + p.stderr[-300:])
    stream = json.loads(p.stdout.strip().splitlines()[-1])
    read_ms = grid_bytes / (stream["TBps"] * 1e12) * 1e3
    rec["read_stream"] = {"TBps": stream["TBps"], "ms_for_the_grid": round(read_ms, 3)}

    with vt.Extractor(0) as ex:
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        rng = np.random.default_rng(3)
        digs = []
        for _ in range(a.digs):   # around the surface, where a dig can cut something loose
            c = (rng.uniform(0.05, 0.95) * n, n / 2.0 + rng.uniform(-0.2, 0.2) * n, rng.uniform(0.05, 0.95) * n)
            digs.append(vt.SphereModifier(c, float(rng.uniform(0.01, 0.04) * n), False))
        for i in range(0, len(digs), 50):
            ex.terrain_update(digs[i:i + 50])

        lo, up = (ctypes.c_float * 3)(*everything["lower"]), (ctypes.c_float * 3)(*everything["upper"])
        count = ctypes.c_int32()

        def count_only():
            ex._check(ex._L.vtmc_terrain_fragments(ex._h, ctypes.byref(lo), ctypes.byref(up), 0, 0, None, 0, ctypes.byref(count)))
            return count.value

        buf = np.zeros(max(count_only(), 1), vt.FRAGMENT_DTYPE)   # also the warm-up: the scratch is allocated here

        def listed():
            ex._check(ex._L.vtmc_terrain_fragments(ex._h, ctypes.byref(lo), ctypes.byref(up), 0, 0, buf.ctypes.data, len(buf), ctypes.byref(count)))
            return count.value

        ms, found = timed_ms(count_only, a.reps)
        rec["query_count"] = dict(summary(ms, read_ms), fragments=found)
        ms, found = timed_ms(listed, a.reps)
        rec["query_list"] = dict(summary(ms, read_ms), fragments=found,
                                 largest_fragment_samples=int(buf["n_samples"][:found].max()) if found else 0,
                                 fragment_samples=int(buf["n_samples"][:found].astype(np.int64).sum()) if found else 0)

        one = [vt.DetachModifier(**everything).to_struct()]
        three = [vt.DetachModifier(**everything).to_struct() for _ in range(3)]
        t0 = time.perf_counter()
        ex.terrain_update(one)                                      # removes the fragments
        rec["first_detach_update_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["fragments_after_detach"] = count_only()
        t1, t3 = [], []
        for _ in range(a.reps):
            t1 += timed_ms(lambda: ex.terrain_update(one), 1)[0]
            t3 += timed_ms(lambda: ex.terrain_update(three), 1)[0]
        per = (float(np.median(t3)) - float(np.median(t1))) / 2
        rec["detach"] = {"device_ms_per_modifier": round(per, 2), "reads_of_the_grid": round(per / read_ms, 2),
                         "update_ms_queue_of_1": round(float(np.median(t1)), 1), "update_ms_queue_of_3": round(float(np.median(t3)), 1)}
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "fragments_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
