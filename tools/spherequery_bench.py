#!/usr/bin/env python3
"""Sphere casts and closest points on the device (vtmc_terrain_spherecast / _closest_point, vtmc_spherecast_device), measured:

  step        median host time of one vtmc_terrain_spherecast of one sweep (r = 0.5 cells, 2 cells long: a character step) on the demo
              world (256 x 72 x 256 cells, SceneManager.cs:23-24, built as tools/raycast_bench.py builds it), beside the median
              vtmc_terrain_raycast of one pick in the same process
  closest     the same for one vtmc_terrain_closest_point with r = 0.5
  batch       --batch sweeps with r = 1 and length 16 cells aimed down onto the demo world through vtmc_spherecast_device: Msweeps/s
              (HIP events on a stream of the tool's own)
  diagonal    one sweep with r = 4 along the diagonal of a 1024^3-cell perlin3d grid (HIP events, median)

Kernel times to quote come from `rocprofv3 --kernel-trace --stats` over a run of this tool (--quick keeps that run short); the events
here are the in-process view.  Prints one JSON line; --out DIR also writes it to DIR/spherequery_bench.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import volumetricterrain_amd as vt
from raycast_bench import demo_world, terrain_grid_args

HIT = vt.SPHERE_HIT_DTYPE.itemsize


def host_median(fn, calls):
    for _ in range(20):
        fn()
    us = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us)), float(np.percentile(us, 90)), out


def timed_sweeps(ex, grid_args, o, d, r, max_distance, reps):
    """Median device time (ms) of `reps` launches of vtmc_spherecast_device on a stream of their own, and the hits of the last one."""
    d_o = torch.from_numpy(np.ascontiguousarray(o, np.float32)).cuda()
    d_d = torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda()
    d_r = torch.from_numpy(np.full(len(o), r, np.float32)).cuda()
    d_h = torch.empty(len(o) * HIT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ms = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        ex.spherecast_device(*grid_args, d_o.data_ptr(), d_d.data_ptr(), d_r.data_ptr(), len(o), d_h.data_ptr(), max_distance,
                             stream=s.cuda_stream)
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    s.synchronize()
    return float(np.median(ms[3:])), d_h.cpu().numpy().view(vt.SPHERE_HIT_DTYPE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--edits", type=int, default=100)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--quick", action="store_true", help="few repetitions (for the rocprofv3 run)")
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.quick:
        a.calls, a.edits = 20, 20
    rng = np.random.default_rng(1)
    res = {"what": "sphere queries: vtmc_terrain_spherecast / _closest_point / vtmc_spherecast_device (sphere_query_kernel)"}
    with vt.Extractor(0) as ex:
        demo_world(ex, rng, a.edits)
        # a character standing on the ground (the plane at 30.5 and the edits around it), stepping 2 cells forward and down
        hit = ex.terrain_raycast(np.float32([[100.0, 60.0, 120.0]]), np.float32([[0.0, -1.0, 0.0]]))
        ground = float(hit["point"][0][1]) if hit["triangle"][0] >= 0 else 30.5
        po = np.float32([[100.0, ground + 0.6, 120.0]])
        pd = np.float32([[2.0, -0.25, 0.0]])
        pick_o = np.float32([[128.0, 110.0, -40.0]])
        pick_d = (np.float32([[140.0, 30.0, 150.0]]) - pick_o).astype(np.float32)
        pick = host_median(lambda: ex.terrain_raycast(pick_o, pick_d), a.calls)
        step = host_median(lambda: ex.terrain_spherecast(po, pd, 0.5, max_distance=float(np.linalg.norm(pd))), a.calls)
        near = host_median(lambda: ex.terrain_closest_point(po - [0, 0.3, 0], 0.5), a.calls)
        res["step"] = {"host_us_median": round(step[0], 1), "host_us_p90": round(step[1], 1), "calls": a.calls,
                       "distance": float(step[2]["distance"][0]), "raycast_pick_host_us_median_same_process": round(pick[0], 1),
                       "raycast_pick_host_us_p90": round(pick[1], 1)}
        res["closest"] = {"host_us_median": round(near[0], 1), "host_us_p90": round(near[1], 1), "calls": a.calls,
                          "distance": float(near[2]["distance"][0])}
        # the batch: sweeps from 16 cells above the ground straight down-ish, r = 1, 16 cells long
        k = a.batch
        o = np.stack([rng.uniform(8, 248, k), np.full(k, ground + 16.0), rng.uniform(8, 248, k)], 1).astype(np.float32)
        d = np.stack([rng.uniform(-0.3, 0.3, k), -np.ones(k), rng.uniform(-0.3, 0.3, k)], 1).astype(np.float32)
        ga = terrain_grid_args(ex)
        ms, hb = timed_sweeps(ex, ga, o, d, 1.0, 16.0, 5 if a.quick else 20)
        res["batch"] = {"sweeps": k, "radius_cells": 1.0, "length_cells": 16.0, "event_ms_median": round(ms, 3),
                        "msweeps_per_s": round(k / ms / 1e3, 2), "hit_fraction": round(float((hb["triangle"] >= 0).mean()), 4)}
    if not a.no_1024:
        with vt.Extractor(0) as ex:
            n, dim = 1024, 1026
            g = torch.empty(dim ** 3, dtype=torch.float32, device="cuda")
            ex.density_fill_device(vt.density_params("perlin3d", n), [[0, 0, 0]], (dim, dim, dim), (1, dim, dim * dim), 0, g.data_ptr())
            ga = (g.data_ptr(), (n, n, n), (1, dim, dim * dim), (0.0, 0.0, 0.0), 1.0)
            o = np.float32([[-5.0, -5.0, -5.0]])
            d = np.float32([[1.0, 1.0, 1.0]])
            ms, hd = timed_sweeps(ex, ga, o, d, 4.0, float("inf"), a.calls)
            res["diagonal_1024"] = {"radius_cells": 4.0, "event_us_median": round(ms * 1e3, 2), "distance": float(hd["distance"][0])}
            g.fill_(-1.0)   # no surface anywhere: the sweep crosses the whole grid
            ms, hd = timed_sweeps(ex, ga, o, d, 4.0, float("inf"), a.calls)
            res["diagonal_1024_no_surface"] = {"radius_cells": 4.0, "event_us_median": round(ms * 1e3, 2)}
            del g
    vt.release_streams()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "spherequery_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
