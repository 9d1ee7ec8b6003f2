#!/usr/bin/env python3
"""The material layer (vtmc_material_*) measured on the benchmark's field:

  vertices  a resident terrain of N^3 cells (N = 1024; --quick: 256) filled by one fBm NoiseModifier with bench.py's fbm8 parameters
            (8 octaves, f = 4/N, ramp 2/N around N/2), every block extracted; then vtmc_material_vertices on that result, in soup and in
            indexed mode, at C = 128: host time of the call (launch + wait; median and best of --reps), beside the emit stage's device
            time of the same result (vtmc_last_stage_ms) and the bytes the kernel must move -- 76 T read + 24 T written (soup),
            24 V + 8 V (indexed) -- and the rate those bytes and the best time give
  paint     VTMC_MATERIAL_MAX_STROKES = 4096 strokes (r = 2 % ... 8 % of the world, seeded) in one vtmc_material_paint at C = 128, and one
            stroke of the same kind: host time of the call

Prints one JSON line; --out DIR also writes it to DIR/material_bench.json."""
import argparse
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
    return {"median_ms": round(float(np.median(ms)), 3), "best_ms": round(float(min(ms)), 3), "reps": len(ms)}


def fbm_world(ex, n):
    ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 1)
    m = vt.NoiseModifier(1337, 8, 4.0 / n, 2.0, 0.5, "fbm", ramp_scale=2.0 / n, ramp_center=n / 2.0, lower=(0.0, 0.0, 0.0),
                         upper=(n + 2.0, n + 2.0, n + 2.0))
    return ex.terrain_update([m])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="256^3 cells instead of 1024^3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = 256 if args.quick else 1024
    rec = {"tool": "tools/material_bench.py", "quick": bool(args.quick), "cells": n, "layer": 128,
           "world": "%d^3 cells, one fBm NoiseModifier (8 octaves, f = 4/N, ramp 2/N around N/2), every block extracted" % n}
    rng = np.random.default_rng(1)
    strokes = [vt.MaterialStroke(tuple(rng.uniform(0, n, 3)), float(rng.uniform(0.02 * n, 0.08 * n)), int(rng.integers(0, 8)),
                                 float(rng.uniform(0.2, 1.0))) for _ in range(4096)]
    for indexed in (False, True):
        with vt.Extractor(0) as ex:
            ex.set_output_mode(indexed)
            n_dirty, T = fbm_world(ex, n)
            emit_ms = ex.last_stage_ms()["emit"]
            ex.material_init(8)
            if not indexed:
                one, _ = timed_ms(lambda: ex.paint(strokes[:1]), args.reps)
                many, _ = timed_ms(lambda: ex.paint(strokes), max(args.reps // 2, 2))
                rec["paint"] = {"one_stroke": summary(one), "strokes_4096": summary(many), "texels": 128 ** 3}
            else:
                ex.paint(strokes[:64])
            ms, count = timed_ms(ex.material_vertices, args.reps + 1)
            ms = ms[1:]   # the first call allocates the weights
            V = ex.last_vertex_count() if indexed else 0
            moved = (24 + 8) * V if indexed else (76 + 24) * T
            r = summary(ms)
            r.update({"triangles": int(T), "vertices": int(count), "dirty_blocks": int(n_dirty), "emit_stage_ms": round(float(emit_ms), 3),
                      "bytes_moved": int(moved), "tb_per_s_at_best": round(moved / (min(ms) * 1e-3) / 1e12, 3)})
            rec["vertices_indexed" if indexed else "vertices_soup"] = r
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "material_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
