#!/usr/bin/env python3
"""VTMC_MOD_EROSION (include/vtmc_erosion.h) measured on a --cells^3 terrain (1024: 1026^3 samples, 4.3 GB; the fBm-over-a-ramp terrain
of the other benches) with a whole-grid box, 1026 x 1026 columns, and the same step on a box of --small x --small columns.

  box_read         a plain device read of the box (vtmc_debug_nav_box_read_ms): what one read of the grid costs here
  heights          the height pass of an erosion of one step (vtmc_debug_erosion_ms), against that read
  write_back       its finish and write-back, history off, against that read
  step_in_a_call   an erosion of --steps steps: the device time of its steps divided by --steps
  step, per variant  vtmc_debug_erosion_step_ms: --steps more steps on the state the erosion left, divided by --steps, the variants
                   alternating in this one process, --reps rounds: direct (neighbour loads through the caches), lds (the planes read at a
                   neighbour staged in LDS), empty (three empty launches of the same shape)
  state_copy       a device-to-device copy of as many bytes as the state holds (45 per column), the same way
No threshold: the times have no predecessor.  The record says which of the three references -- the copy of the state, the empty launches,
the box read -- a step sits nearest to.

Prints one JSON line and writes it to DIR/erosion_bench.json (--out DIR, by default profiles/r28/erosion; --out "" writes nothing)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import volumetricterrain_amd as vt

PARAMS = dict(rain=0.02, evaporation=0.05, capacity=1.0, dissolve=0.3, deposit=0.3, dt=0.25, talus=0.5, thermal_rate=0.1)
VARIANTS = ("direct", "lds", "empty")


def copy_ms(n_bytes, reps):
    """Median device time of a device-to-device copy of n_bytes, or None without torch."""
    try:
        import torch
    except Exception:
        return None
    src, dst = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    dst.copy_(src)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def steps_of(ex, steps, reps):
    """Per-step device time of every variant, alternating, as {variant: [ms per step, one per round]}."""
    ms, out = ctypes.c_float(), {v: [] for v in VARIANTS}
    for v in range(3):   # warm-up, every variant once
        ex._check(ex._L.vtmc_debug_erosion_step_ms(ex._h, v, 8, ctypes.byref(ms)))
    for _ in range(reps):
        for v, name in enumerate(VARIANTS):
            ex._check(ex._L.vtmc_debug_erosion_step_ms(ex._h, v, steps, ctypes.byref(ms)))
            out[name].append(ms.value / steps)
    return out


def summary(rounds):
    return {name: {"us_median": round(1e3 * float(np.median(v)), 2), "us_min": round(1e3 * float(np.min(v)), 2), "us_max": round(1e3 * float(np.max(v)), 2)}
            for name, v in rounds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--small", type=int, default=128)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28", "erosion"))
    a = ap.parse_args()
    n = a.cells
    samples = (n + 2) ** 3
    rec = {"tool": "tools/erosion_bench.py", "terrain": "%d^3 cells, %d samples, %.2f GB" % (n, samples, 4 * samples / 1e9), "reps": a.reps, "steps": a.steps,
           "params": PARAMS}
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        ex.terrain_init(n, n, n, 1.0, (0.0, 0.0, 0.0), 5)
        everything = dict(lower=(-10.0,) * 3, upper=(float(n) + 10.0,) * 3)
        ex.terrain_update([vt.NoiseModifier(seed=1337, octaves=6, frequency=4.0 / n, amplitude=1.0, ramp_scale=4.0 / n, ramp_center=n / 2.0, **everything)])
        lo, up = (ctypes.c_float * 3)(*everything["lower"]), (ctypes.c_float * 3)(*everything["upper"])
        read_ms = ctypes.c_float()
        ex._check(L.vtmc_debug_nav_box_read_ms(h, ctypes.byref(lo), ctypes.byref(up), 5, ctypes.byref(read_ms)))
        rec["box_read_ms"] = round(read_ms.value, 3)

        def erode(iterations, **box):
            ex.terrain_update([vt.ErosionModifier(iterations=iterations, **box, **PARAMS)])
            ms = (ctypes.c_float * 3)()
            ex._check(L.vtmc_debug_erosion_ms(h, ms))
            return list(ms)

        erode(1, **everything)   # the warm-up: the state is allocated here
        one = np.median(np.asarray([erode(1, **everything) for _ in range(a.reps)]), axis=0)
        info = ex.erosion_info()
        columns = info["nx"] * info["nz"]
        rec["whole_grid"] = {"columns": columns, "n_active": info["n_active"], "n_rewritten": info["n_rewritten"], "n_clamped": info["n_clamped"],
                             "heights_ms": round(float(one[0]), 3), "heights_over_box_read": round(float(one[0]) / read_ms.value, 2),
                             "write_back_ms": round(float(one[2]), 3), "write_back_over_box_read": round(float(one[2]) / read_ms.value, 2)}
        many = erode(a.steps, **everything)
        rec["whole_grid"]["step_in_a_call_us"] = round(1e3 * many[1] / a.steps, 2)
        rec["whole_grid"]["step"] = summary(steps_of(ex, a.steps, a.reps))
        state_bytes = 45 * columns
        c = copy_ms(state_bytes, a.reps)
        rec["whole_grid"]["state_bytes"] = state_bytes
        rec["whole_grid"]["state_copy_us"] = None if c is None else round(1e3 * c, 2)

        small = dict(lower=(n / 2.0, -10.0, n / 2.0), upper=(n / 2.0 + a.small - 1, float(n) + 10.0, n / 2.0 + a.small - 1))
        erode(1, **small)
        info = ex.erosion_info()
        columns = info["nx"] * info["nz"]
        many = erode(a.steps, **small)
        rec["small_box"] = {"columns": columns, "n_active": info["n_active"], "step_in_a_call_us": round(1e3 * many[1] / a.steps, 2),
                            "step": summary(steps_of(ex, a.steps, a.reps))}
        c = copy_ms(45 * columns, a.reps)
        rec["small_box"]["state_copy_us"] = None if c is None else round(1e3 * c, 2)

        for name in ("whole_grid", "small_box"):
            r = rec[name]
            direct = r["step"]["direct"]["us_median"]
            refs = {"three empty launches": r["step"]["empty"]["us_median"], "a copy of the state": r["state_copy_us"],
                    "a read of the box": 1e3 * read_ms.value if name == "whole_grid" else None}
            refs = {k: v for k, v in refs.items() if v}
            r["faster_variant"] = "lds" if r["step"]["lds"]["us_median"] < direct else "direct"
            r["a_step_sits_nearest_to"] = min(refs, key=lambda k: abs(np.log(direct / refs[k])))
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "erosion_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
