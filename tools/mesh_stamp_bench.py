#!/usr/bin/env python3
"""vtmc_stamp_from_mesh measured: an icosphere of 1 280, 20 480 and 327 680 triangles voxelized into a 128^3 and a 256^3 stamp that holds
it with a margin of four samples.  Per case:

  call_ms            host time of one call (closed-mesh check, records, two uploads, the kernel, the wait): median after two warm-up calls
  event_ms           the time between two HIP events recorded on the context's stream around the same call
  trusted_call_ms    call_ms with VTMC_MESH_TRUST_CLOSED: without the host's edge sort
  survivors_distance, survivors_parity
                     mean triangles per 64 x 16 x 4 tile that pass the kernel's two pruning tests, computed here from the same bounds
                     (the triangle's AABB grown by g against the tile's AABB; its (y, z) AABB and max_x against the tile's)

Prints one JSON line; --out DIR also writes it to DIR/mesh_stamp_bench.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import volumetricterrain_amd as vt
from mesh_twin import icosphere, positions, reach_box_grow

TILE = (64, 16, 4)


def survivors(v, t, first, pitch, dims):
    """Mean triangles per tile that survive the distance test and the parity test of stamp_mesh_kernel."""
    tv = v[t]
    lo, hi = tv.min(axis=1), tv.max(axis=1)
    g = reach_box_grow(tv, first, pitch, dims)
    P = positions(first, pitch, dims)
    tlo = [P[k][::TILE[k]] for k in range(3)]
    thi = [P[k][np.minimum(np.arange(TILE[k] - 1, dims[k] + TILE[k] - 1, TILE[k]), dims[k] - 1)] for k in range(3)]
    # per axis [tiles along the axis, triangles]: the tests are separable, so the counts are sums of products of the axis masks
    near = [~((thi[k][:, None] < lo[None, :, k] - g) | (tlo[k][:, None] > hi[None, :, k] + g)) for k in range(3)]
    over = [tlo[0][:, None] < hi[None, :, 0], ~((thi[1][:, None] < lo[None, :, 1]) | (tlo[1][:, None] > hi[None, :, 1])),
            ~((thi[2][:, None] < lo[None, :, 2]) | (tlo[2][:, None] >= hi[None, :, 2]))]
    n_tiles = len(tlo[0]) * len(tlo[1]) * len(tlo[2])
    count = lambda m: float(np.einsum("xt,yt,zt->", *(a.astype(np.float64) for a in m))) / n_tiles   # noqa: E731
    return round(count(near), 2), round(count(over), 2)


def timed_calls(ex, stream, v, t, first, pitch, dims, trust, reps):
    wall, event = [], []
    for r in range(reps + 2):   # two warm-up calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        sid = ex.stamp_from_mesh(v, t, first, pitch, dims, trust_closed=trust)
        t1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        ex.stamp_destroy(sid)
        if r >= 2:
            wall.append((t1 - t0) * 1e3)
            event.append(e0.elapsed_time(e1))
        del e0, e1
    return round(float(np.median(wall)), 3), round(float(np.median(event)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"tool": "tools/mesh_stamp_bench.py", "reps": args.reps, "cases": []}
    with vt.Extractor(0) as ex:
        stream = torch.cuda.ExternalStream(ex.stream_handle(own_queue=False))
        for n in (128, 256):
            for sub, n_tri in ((3, 1280), (5, 20480), (7, 327680)):
                v, t = icosphere(sub, (n - 9) / 2.0, ((n - 1) / 2.0,) * 3)   # pitch 1: the sphere fills the stamp but for a margin of 4
                assert len(t) == n_tri
                first, pitch, dims = (0.0, 0.0, 0.0), 1.0, (n, n, n)
                call_ms, event_ms = timed_calls(ex, stream, v, t, first, pitch, dims, False, args.reps)
                trusted_ms, _ = timed_calls(ex, stream, v, t, first, pitch, dims, True, args.reps)
                sd, sp = survivors(v, t, first, pitch, dims)
                rec["cases"].append({"stamp": n, "triangles": n_tri, "call_ms": call_ms, "event_ms": event_ms, "trusted_call_ms": trusted_ms,
                                     "survivors_distance": sd, "survivors_parity": sp})
        del stream
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "mesh_stamp_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
