#!/usr/bin/env python3
"""The stamp modifier (VTMC_MOD_STAMP) measured on a 512^3-cell terrain (514^3 samples, voxel scale 1):

  stamp64_identity   a 64^3 stamp pasted unturned at pitch 1
  stamp64_skew       the same stamp turned by the quaternion (0.3, -0.5, 0.2, 0.79)
  stamp256_skew      a 256^3 stamp (64 MB: beyond an XCD's L2) turned the same way

each in replace mode (a paste leaves what the one before it left, so every repetition does the same work), with history off and on, and
beside each the parent's pointwise kernel: a SphereModifier handed the same lower / upper, so the same sample box, in the same process;
and vtmc_stamp_capture of a 64^3 and a 256^3 box (host time of the call: allocation, the device copy, the wait).

A vtmc_terrain_update also extracts the dirty blocks, so a modifier's device time is taken as a difference, as tools/noise_bench.py does:
a queue of 5 copies against a queue of 1, (median t5 - median t1) / 4 over --reps updates each, alternating, after one warm-up round.
GB/s-equivalent counts 8 bytes per sample of the box (one read, one write); the stamp's own reads and the journal's image come on top.

Prints one JSON line; --out DIR also writes it to DIR/stamp_bench.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import volumetricterrain_amd as vt
from history_bench import timed

DIMS = (512, 512, 512)
CENTRE = (257.0, 257.0, 257.0)
SKEW = (0.3, -0.5, 0.2, 0.79)


def field(n, seed):
    rng = np.random.default_rng(seed)
    a = np.arange(n, dtype=np.float32)
    k = rng.uniform(0.02, 0.2, 3).astype(np.float32)
    return (1.5 * np.sin(k[0] * a)[:, None, None] * np.cos(k[1] * a)[None, :, None] * np.sin(k[2] * a + 1.0)[None, None, :]).astype(np.float32)


def per_modifier(ex, struct, reps):
    one, five = [struct], [struct] * 5
    t1, t5 = [], []
    for r in range(reps + 1):   # the first round is the warm-up
        d1, (nd, T) = timed(lambda: ex.terrain_update(one))
        d5, _ = timed(lambda: ex.terrain_update(five))
        if r:
            t1.append(d1)
            t5.append(d5)
    return (float(np.median(t5)) - float(np.median(t1))) / 4e3, float(np.median(t1)) / 1e3, int(nd), int(T)


def case(ex, sid, n, rotation, reps):
    mod = vt.StampModifier(sid, (n, n, n), CENTRE, rotation, 1.0, "replace").to_struct()
    sphere = vt.SphereModifier(CENTRE, 0.45 * n, True).to_struct()
    sphere.lower[:], sphere.upper[:] = list(mod.lower), list(mod.upper)   # the stamp's sample box
    box = [int(np.ceil(mod.upper[k])) - int(np.floor(mod.lower[k])) + 1 for k in range(3)]
    samples = box[0] * box[1] * box[2]
    rec = {"box_samples": box, "footprint_share": round(n ** 3 / samples, 3)}
    for name, history in (("history_off", 0), ("history_on", 1 << 32)):
        ex.terrain_set_history(history)
        ms, whole, nd, T = per_modifier(ex, mod, reps)
        ms_sphere, _, _, _ = per_modifier(ex, sphere, reps)
        rec[name] = {"device_ms_per_paste": round(ms, 4), "update_ms_queue_of_1": round(whole, 3), "dirty_blocks": nd, "triangles": T,
                     "gb_per_s_equivalent": round(8 * samples / ms / 1e6, 1), "sphere_same_box_ms": round(ms_sphere, 4),
                     "ratio_to_sphere": round(ms / ms_sphere, 2)}
    ex.terrain_set_history(0)
    return rec


def capture_ms(ex, n, reps):
    t = []
    for _ in range(reps + 1):
        dt, sid = timed(lambda: ex.stamp_capture((100, 100, 100), (n, n, n)))
        ex.stamp_destroy(sid)
        t.append(dt)
    return round(float(np.median(t[1:])) / 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"tool": "tools/stamp_bench.py", "terrain": "%dx%dx%d cells, voxel scale 1" % DIMS, "reps": args.reps, "mode": "replace", "pitch": 1.0}
    with vt.Extractor(0) as ex:
        ex.terrain_init(*DIMS, 1.0, (0.0, 0.0, 0.0), 5)
        ex.terrain_update([vt.PlaneModifier(250.5, (-1, -1), (600, 600), True)])
        s64, s256 = ex.stamp_create(field(64, 1)), ex.stamp_create(field(256, 2))
        rec["stamp64_identity"] = case(ex, s64, 64, (0.0, 0.0, 0.0, 1.0), args.reps)
        rec["stamp64_skew"] = case(ex, s64, 64, SKEW, args.reps)
        rec["stamp256_skew"] = case(ex, s256, 256, SKEW, args.reps)
        rec["stamp_capture_host_ms"] = {"64^3": capture_ms(ex, 64, args.reps), "256^3": capture_ms(ex, 256, args.reps)}
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "stamp_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
