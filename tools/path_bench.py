#!/usr/bin/env python3
"""The path modifier (VTMC_MOD_PATH) measured on a 1024 x 128 x 1024-cell terrain (1026 x 130 x 1026 samples) that holds a plane plus
noise, carving one deterministic branching river tree of about 2000 segments (SplitMix64, no library RNG) that spans the map:

  a  path        one PathModifier erode of the whole tree: one launch over one box, one event number, one journal box
  b  cylinders   the same tree as a queue of one eroding CylinderModifier per segment in ONE vtmc_terrain_update, radius = the upstream
                 node's: the reference's route (RiverRenderer.cs:151-170, TerrainEngine.cs:97-99).  Another shape, the same job
  c  flatten0    VTMC_MOD_FLATTEN with strength 0 on the path's box, as the issue asked.  With history off that kernel skips a sample of
                 weight 0 before it reads it, so it moves no bytes; with history on it reads the box and writes the image
  d  plane       a PlaneModifier add far below the terrain on the path's box: the pointwise kernel that reads and writes every sample
                 of the box (8 bytes per sample, 12 with history on) -- the read-write floor the path kernel is to be compared with

Each with history off and on.  wall_ms is the host time of one vtmc_terrain_update holding the queue once (it includes the extraction
of the dirty blocks, which is every block for a, c and d); device_ms is the difference method of the other terrain tools: the median
update holding the queue k times minus the median update holding it once, over k - 1.  For a path that difference also holds the
staging of its segments (a stream drain and a copy of 64 bytes per segment).  The queues are prebuilt vtmc_modifier arrays and the call
is the C entry point, so no Python marshalling is in the times.

Prints one JSON line; --out DIR also writes it to DIR/path_bench.json."""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import volumetricterrain_amd as vt
from volumetricterrain_amd._lib import Modifier
from history_bench import timed

DIMS = (1024, 128, 1024)
SAMPLES = (DIMS[0] + 2) * (DIMS[1] + 2) * (DIMS[2] + 2)
M64 = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def uniform(self, lo=0.0, hi=1.0):
        return lo + (hi - lo) * (self.next() >> 11) / float(1 << 53)


def river_tree(n_segments=2000, seed=2024):
    """(positions, radii, parent) of a river tree grown upstream from its mouth at the middle of the map's z = 1000 edge, breadth first
    as RiverRenderer walks it: a node has one or two upstream nodes 16..30 units away, turned a little from its own heading; the
    radius (the reference's flux) falls from 7 at the mouth to 1.2 at the springs; the bed wanders about y = 60."""
    rng = SplitMix64(seed)
    pos, rad, parent, heading = [(512.0, 58.0, 1000.0)], [7.0], [-1], [-math.pi / 2]   # heading: angle in the x-z plane; upstream is -z
    frontier = [0]
    while len(pos) - 1 < n_segments and frontier:
        nxt = []
        for k in frontier:
            kids = 2 if rng.uniform() < 0.09 or k == 0 else 1
            for c in range(kids):
                if len(pos) - 1 >= n_segments:
                    break
                turn = rng.uniform(-0.45, 0.45) + (0.0 if kids == 1 else (0.6 if c else -0.6))
                h = heading[k] + turn
                step = rng.uniform(16.0, 30.0)
                x, y, z = pos[k]
                x2, z2 = x + step * math.cos(h), z + step * math.sin(h)
                if not (20.0 < x2 < 1004.0 and 20.0 < z2 < 1004.0):   # turn back into the map
                    h = math.atan2(512.0 - z, 512.0 - x) + rng.uniform(-0.3, 0.3)
                    x2, z2 = x + step * math.cos(h), z + step * math.sin(h)
                y2 = min(max(y + rng.uniform(-1.2, 1.6), 40.0), 90.0)
                pos.append((x2, y2, z2))
                rad.append(max(1.2, rad[k] * rng.uniform(0.93, 0.995) * (0.8 if kids == 2 else 1.0)))
                parent.append(k)
                heading.append(h)
                nxt.append(len(pos) - 1)
        frontier = nxt
    return np.array(pos), np.array(rad), np.array(parent)


def queue_of(mods, times=1):
    structs = [m.to_struct() if hasattr(m, "to_struct") else m for m in mods] * times
    arr = (Modifier * len(structs))()
    for i, m in enumerate(structs):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(m), ctypes.sizeof(Modifier))
    return arr, len(structs), structs   # structs: what keeps borrowed arrays alive


def update(ex, q):
    nd, t = ctypes.c_int32(), ctypes.c_int32()
    ex._check(ex._L.vtmc_terrain_update(ex._h, ctypes.cast(q[0], ctypes.c_void_p), q[1], ctypes.byref(nd), ctypes.byref(t)))
    return nd.value, t.value


def measure(ex, mods, k, reps, history):
    """One queue: wall of the queue once, device time by the difference against the queue k times; with history on, what one update
    of the queue once records."""
    once, many = queue_of(mods), queue_of(mods, k)
    t1, tk = [], []
    out = {}
    for r in range(reps + 2):   # two warm-up rounds
        d1, (nd, T) = timed(lambda: update(ex, once))
        if history and r == 0:
            n_undo, _, used = ex.terrain_history()
            out.update(steps_recorded=n_undo, journal_bytes=int(used), journal_boxes=len(mods))
            ex.terrain_set_history(history)   # start every measured update from an empty arena
        dk, _ = timed(lambda: update(ex, many))
        if history:
            ex.terrain_set_history(history)
        if r >= 2:
            t1.append(d1)
            tk.append(dk)
    out.update(wall_ms=round(float(np.median(t1)) / 1e3, 3), wall_ms_min=round(float(np.min(t1)) / 1e3, 3), wall_ms_max=round(float(np.max(t1)) / 1e3, 3),
               device_ms=round((float(np.median(tk)) - float(np.median(t1))) / 1e3 / (k - 1), 3), queue_times=k, modifiers=len(mods),
               dirty_blocks=int(nd), triangles=int(T))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--segments", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pos, rad, parent = river_tree(args.segments)
    path = vt.PathModifier.from_tree(pos, rad, parent)
    seg = path.segments.astype(np.float64)
    cylinders = [vt.CylinderModifier(s[0:3], s[4:7] - s[0:3], float(np.linalg.norm(s[4:7] - s[0:3])), s[7], False) for s in seg]
    lo, hi = path.LowerBound.astype(np.float64), path.UpperBound.astype(np.float64)
    flatten0 = vt.FlattenModifier((512.0, 60.0, 512.0), (0.0, 1.0, 0.0), 100.0, 0.0).to_struct()
    plane = vt.PlaneModifier(-1.0e6, (lo[0], lo[2]), (hi[0], hi[2]), True).to_struct()
    for m in (flatten0, plane):
        m.lower[:], m.upper[:] = tuple(lo), tuple(hi)
    rec = {"tool": "tools/path_bench.py", "terrain": "%dx%dx%d cells, %d samples" % (DIMS + (SAMPLES,)), "reps": args.reps, "segments": len(seg),
           "path_box_lower": [round(float(v), 2) for v in lo], "path_box_upper": [round(float(v), 2) for v in hi],
           "segment_length_mean": round(float(np.linalg.norm(seg[:, 4:7] - seg[:, 0:3], axis=1).mean()), 2),
           "radius_min_max": [round(float(seg[:, [3, 7]].min()), 2), round(float(seg[:, [3, 7]].max()), 2)]}
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, 1.0, (0.0, 0.0, 0.0), 5)
        ex.terrain_update([vt.PlaneModifier(64.0, (-10.0, -10.0), (2000.0, 2000.0), True),
                           vt.NoiseModifier(seed=11, octaves=5, frequency=1.0 / 160, amplitude=14.0, ramp_scale=1.0, ramp_center=64.0,
                                            lower=(-10.0, 30.0, -10.0), upper=(2000.0, 100.0, 2000.0))])
        box_samples = None
        for name, history in (("history_off", 0), ("history_on", 3 << 30)):
            ex.terrain_set_history(history)
            r = {"path": measure(ex, [path], 2, args.reps, history), "cylinders": measure(ex, cylinders, 2, args.reps, history),
                 "flatten0": measure(ex, [flatten0], 5, args.reps, history), "plane": measure(ex, [plane], 5, args.reps, history)}
            if history:
                box_samples = r["path"]["journal_bytes"] // 4
            for what in ("device_ms", "wall_ms"):
                a, b, c, d = (r[k][what] for k in ("path", "cylinders", "flatten0", "plane"))
                r["ratios_" + what] = {"a_over_b": round(a / b, 4) if b > 0 else None, "a_over_c": round(a / c, 3) if c > 0 else None,
                                       "a_over_d": round(a / d, 3) if d > 0 else None}
            rec[name] = r
        ex.terrain_set_history(0)
    rec["path_box_samples"] = box_samples
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "path_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
