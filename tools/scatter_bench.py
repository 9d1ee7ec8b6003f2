#!/usr/bin/env python3
"""The surface scatter (vtmc_scatter_*) measured on the benchmark's field, against the extract that wrote the records it reads:

  a resident terrain of N^3 cells (N = 1024; --quick: 256) filled by one fBm NoiseModifier with bench.py's fbm8 parameters (8 octaves,
  f = 4/N, ramp 2/N around N/2), every block extracted (tools/ao_bench.py's world); then vtmc_scatter_surface on that result, in soup and
  in indexed mode, per case (density in instances per cell^2, filters): the device time of the count, scan, emit and block-offset kernels
  (HIP events, vtmc_debug_scatter_ms; median of --reps, the first call, which allocates, left out) and the time of the whole call on the
  host; T and the number of instances; the bytes the pass moves at the least; the rate that gives over the four kernels, beside the read
  stream of the project's box calibration (profiles/r04/memory_ceilings.json: 6.8 TB/s); and the ratio of the scatter's device time to the
  extract of the same run (vtmc_last_stage_ms, `total`).

Bytes moved, soup: 76 T (count) + T (masks out) + T (masks in) + 76 T (emit, when every tile has a survivor) + 32 N.  Indexed: the index
triples (12 T) and every vertex once (24 V) per pass, in place of the records.

Prints one JSON line; --out DIR also writes it to DIR/scatter_bench.json."""
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
from ao_bench import fbm_world

BOX_READ_TBPS = 6.8   # DESIGN.md, "What the memory system gives": one float4 per thread, 2-8 GiB
CASES = [("density 1", dict(density=1.0)), ("density 8", dict(density=8.0)),
         ("density 1, up >= 0.7, upper half", dict(density=1.0, min_up=0.7, min_y=None))]   # min_y: filled in with N / 2


def kernel_ms(ex):
    ms = (ctypes.c_float * 4)()
    ex._check(ex._L.vtmc_debug_scatter_ms(ex._h, ctypes.byref(ms)))
    return [float(v) for v in ms]


def scatter_case(ex, kw, reps, T, V, indexed):
    p = vt.ScatterParams(seed=7, max_instances=(1 << 31) - 1, **kw).to_struct()
    n = ctypes.c_int64()
    dev, host = [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        ex._check(ex._L.vtmc_scatter_surface(ex._h, ctypes.byref(p), ctypes.byref(n)))
        t1 = time.perf_counter()
        if k:   # the first call grows the buffers
            dev.append(kernel_ms(ex))
            host.append((t1 - t0) * 1e3)
    med = np.median(np.array(dev), axis=0)
    N = int(n.value)
    per_pass = (12 * T + 24 * V) if indexed else 76 * T
    moved = 2 * per_pass + 2 * T + 32 * N
    total = float(med.sum())
    return {"count_ms": round(float(med[0]), 4), "scan_ms": round(float(med[1]), 4), "emit_ms": round(float(med[2]), 4),
            "block_offsets_ms": round(float(med[3]), 4), "kernels_ms": round(total, 4), "call_host_ms": round(float(np.median(host)), 3),
            "instances": N, "bytes_moved": int(moved), "tbps": round(moved / (total * 1e-3) / 1e12, 3), "box_read_tbps": BOX_READ_TBPS,
            "count_tbps": round((per_pass + T) / (float(med[0]) * 1e-3) / 1e12, 3),
            "emit_tbps": round((per_pass + T + 32 * N) / (float(med[2]) * 1e-3) / 1e12, 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="256^3 cells instead of 1024^3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = 256 if args.quick else 1024
    rec = {"tool": "tools/scatter_bench.py", "quick": bool(args.quick), "cells": n,
           "world": "%d^3 cells, one fBm NoiseModifier (8 octaves, f = 4/N, ramp 2/N around N/2), every block extracted" % n}
    for indexed in (False, True):
        with vt.Extractor(0) as ex:
            ex.set_output_mode(indexed)
            n_dirty, T = fbm_world(ex, n)
            stages = ex.last_stage_ms()
            V = ex.last_vertex_count() if indexed else 0
            r = {"triangles": int(T), "vertices": int(V), "dirty_blocks": int(n_dirty),
                 "extract_ms": {k: round(float(v), 4) for k, v in stages.items()}, "cases": []}
            for name, kw in CASES:
                kw = {k: (n / 2.0 if v is None else v) for k, v in kw.items()}
                c = scatter_case(ex, kw, args.reps, int(T), int(V), indexed)
                c["case"] = name
                c["scatter_over_extract"] = round(c["kernels_ms"] / float(stages["total"]), 3)
                r["cases"].append(c)
            rec["indexed" if indexed else "soup"] = r
    vt.release_streams()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "scatter_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
