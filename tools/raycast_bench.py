#!/usr/bin/env python3
"""Ray picking on the device (vtmc_terrain_raycast / vtmc_raycast_device), measured:

  pick        median host time of one vtmc_terrain_raycast of one ray on the demo world (256 x 72 x 256 cells, SceneManager.cs:23-24)
              over --calls calls after warm-up, beside the median vtmc_terrain_update of one sphere edit in the same process (the loop
              of tools/edit_latency.py: the whole interactive edit is pick + edit)
  one_ray     device time (HIP events around each launch, median) of one ray across the demo world and along the diagonal of a
              1024^3-cell perlin3d grid
  batch       --batch camera rays (a 1024 x 1024 pinhole, 60 degrees field of view) looking down at 30 degrees onto the demo world:
              Mrays/s, the mean number of cells a ray visits (box entry to its hit, or to its exit) and the sample bytes that implies
              (8 corner samples of 4 bytes per visited cell, as the kernel loads them)

Kernel times to quote come from `rocprofv3 --kernel-trace --stats` over a run of this tool (--quick keeps that run short); the events
here are the in-process view.  Prints one JSON line; --out DIR also writes it to DIR/raycast_bench.json."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import volumetricterrain_amd as vt

HIT = vt.RAY_HIT_DTYPE.itemsize


def demo_world(ex, rng, n_edits):
    """tools/edit_latency.py's world and edit loop; returns the edit latencies (us) after 20 warm-up edits."""
    ex.terrain_init(256, 72, 256, 1.0, (0.0, 0.0, 0.0), 1)
    ex.terrain_update([vt.PlaneModifier(30.5, (-1, -1), (300, 300), True)])
    lat = []
    for i in range(n_edits + 20):
        c = (float(rng.uniform(20, 236)), 30.0 + float(rng.uniform(-4, 4)), float(rng.uniform(20, 236)))
        t0 = time.perf_counter()
        ex.terrain_update([vt.SphereModifier(c, 10.0, bool(i & 1))])
        if i >= 20:
            lat.append((time.perf_counter() - t0) * 1e6)
    return np.array(lat)


def camera_rays(w, h, pos, pitch_deg, fov_deg=60.0):
    """Pinhole camera at `pos` looking along +z, pitched down by pitch_deg."""
    p = np.radians(pitch_deg)
    fwd = np.array([0.0, -np.sin(p), np.cos(p)])
    right = np.array([1.0, 0.0, 0.0])
    up = np.cross(fwd, right)
    s = np.tan(np.radians(fov_deg) / 2)
    u = (np.arange(w) + 0.5) / w * 2 - 1
    v = (np.arange(h) + 0.5) / h * 2 - 1
    uu, vv = np.meshgrid(u * s, v * s)
    d = fwd + uu[..., None] * right + vv[..., None] * up
    d = d.reshape(-1, 3)
    return np.tile(np.asarray(pos, np.float32), (len(d), 1)), d.astype(np.float32)


def cells_visited(o, d, dist, n):
    """Cells a ray's DDA walks from its entry into [0, n] to its hit (or its exit)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (0.0 - o) / d, (np.asarray(n, float) - o) / d
        tin = np.maximum(np.nanmax(np.minimum(t0, t1), axis=1), 0.0)
        tout = np.nanmin(np.maximum(t0, t1), axis=1)
    ok = tin <= tout
    tend = np.where(dist >= 0, dist, tout)
    a = np.clip(np.floor(o + tin[:, None] * d), 0, np.asarray(n) - 1)
    b = np.clip(np.floor(o + tend[:, None] * d), 0, np.asarray(n) - 1)
    return np.where(ok, np.abs(b - a).sum(axis=1) + 1, 0)


def device_rays(o, d):
    return torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()


def timed_casts(ex, grid_args, o, d, reps):
    """Median device time (ms) of `reps` launches of vtmc_raycast_device on a stream of their own, and the hits of the last one."""
    d_o, d_d = device_rays(o, d)
    d_h = torch.empty(len(o) * HIT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()   # a stream of its own (torch's default one is the NULL handle, which the library reads as its context's stream)
    ms = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        ex.raycast_device(*grid_args, d_o.data_ptr(), d_d.data_ptr(), len(o), d_h.data_ptr(), stream=s.cuda_stream)
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    s.synchronize()
    hits = d_h.cpu().numpy().view(vt.RAY_HIT_DTYPE)
    return float(np.median(ms[3:])), hits


def terrain_grid_args(ex):
    p, st, dims = ctypes.c_void_p(), (ctypes.c_int64 * 3)(), (ctypes.c_int32 * 3)()
    ex._check(ex._L.vtmc_terrain_device_grid(ex._h, ctypes.byref(p), ctypes.byref(st), ctypes.byref(dims)))
    return (p.value, (dims[0] - 2, dims[1] - 2, dims[2] - 2), tuple(st), (0.0, 0.0, 0.0), 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--edits", type=int, default=200)
    ap.add_argument("--batch-side", type=int, default=1024, help="the camera batch is side x side rays")
    ap.add_argument("--quick", action="store_true", help="few repetitions (for the rocprofv3 run)")
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.quick:
        a.calls, a.edits = 20, 20
    rng = np.random.default_rng(1)
    res = {"what": "ray picking: vtmc_terrain_raycast / vtmc_raycast_device (raycast_kernel)"}
    with vt.Extractor(0) as ex:
        edit = demo_world(ex, rng, a.edits)
        # one pick: a cursor ray from a camera above the world's edge to a point of the ground
        po = np.array([[128.0, 110.0, -40.0]], np.float32)
        pd = (np.array([[140.0, 30.0, 150.0]], np.float32) - po).astype(np.float32)
        for _ in range(20):
            ex.terrain_raycast(po, pd)
        host = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            h = ex.terrain_raycast(po, pd)
            host.append((time.perf_counter() - t0) * 1e6)
        res["pick"] = {"host_us_median": round(float(np.median(host)), 1), "host_us_p90": round(float(np.percentile(host, 90)), 1),
                       "calls": a.calls, "hit_distance": float(h["distance"][0]),
                       "cells_visited": int(cells_visited(po, pd, h["distance"], (256, 72, 256))[0]),
                       "edit_us_median_same_process": round(float(np.median(edit)), 1), "edits": len(edit)}
        ga = terrain_grid_args(ex)
        ms, h1 = timed_casts(ex, ga, po, pd, a.calls)
        res["one_ray_demo_world"] = {"event_us_median": round(ms * 1e3, 2), "distance": float(h1["distance"][0])}
        # the camera batch, 30 degrees down onto the demo world
        o, d = camera_rays(a.batch_side, a.batch_side, (128.0, 100.0, -60.0), 30.0)
        ms, hb = timed_casts(ex, ga, o, d, 5 if a.quick else 20)
        cells = cells_visited(o, d, hb["distance"], (256, 72, 256))
        res["batch"] = {"rays": len(o), "camera": "(128, 100, -60), pitch -30 deg, fov 60 deg, 1024 x 1024" if a.batch_side == 1024 else a.batch_side,
                        "event_ms_median": round(ms, 3), "mrays_per_s": round(len(o) / ms / 1e3, 1),
                        "hit_fraction": round(float((hb["triangle"] >= 0).mean()), 4), "mean_cells_visited": round(float(cells.mean()), 1),
                        "sample_gb_per_s": round(float(cells.sum()) * 32 / (ms * 1e-3) / 1e9, 1)}
    if not a.no_1024:
        with vt.Extractor(0) as ex:
            n, dim = 1024, 1026
            g = torch.empty(dim ** 3, dtype=torch.float32, device="cuda")
            ex.density_fill_device(vt.density_params("perlin3d", n), [[0, 0, 0]], (dim, dim, dim), (1, dim, dim * dim), 0, g.data_ptr())
            o = np.array([[-1.0, -1.0, -1.0]], np.float32)
            d = np.array([[1.0, 1.0, 1.0]], np.float32)
            ga = (g.data_ptr(), (n, n, n), (1, dim, dim * dim), (0.0, 0.0, 0.0), 1.0)
            ms, hd = timed_casts(ex, ga, o, d, a.calls)
            res["one_ray_1024_diagonal"] = {"event_us_median": round(ms * 1e3, 2), "distance": float(hd["distance"][0]),
                                            "cells_visited": int(cells_visited(o, d, hd["distance"], (n, n, n))[0])}
            # the same diagonal on a field without any surface on it: every cell of the ray is walked
            g.fill_(-1.0)
            ms, hd = timed_casts(ex, ga, o, d, a.calls)
            res["one_ray_1024_diagonal_no_surface"] = {"event_us_median": round(ms * 1e3, 2), "cells_visited": int(cells_visited(o, d, hd["distance"], (n, n, n))[0])}
            del g
    vt.release_streams()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "raycast_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
