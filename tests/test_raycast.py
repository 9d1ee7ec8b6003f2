"""Ray picking (vtmc_terrain_raycast / vtmc_raycast_device): the Physics.Raycast of the interactive edit (SceneManager.cs:114-131)
against the surface vtmc_extract_grid emits in exact mode, checked against the CPU reference of surface_twin.py (the oracle's triangles
of the same grid, Moller-Trumbore in float64), under the agreement rule and the float32-precision tight check its docstrings state.
The CPU tests here hold that reference to known answers.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fields
from surface_twin import RAY_HIT_BYTES, Surface, _cast, _device, _long_rays, _rays_perlin, check_tight, compare, reference, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests: the ABI surface and the reference itself
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_ray_calls():
    import volumetricterrain_amd as vt
    text = open(os.path.join(ROOT, "include", "vtmc.h")).read()
    lib = vt.load()
    for name in ("vtmc_terrain_raycast", "vtmc_raycast_device"):
        assert re.search(r"int32_t\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
    assert "#define VTMC_RAY_TWO_SIDED 1u" in text
    assert vt.RAY_HIT_DTYPE.itemsize == RAY_HIT_BYTES
    assert [vt.RAY_HIT_DTYPE.fields[f][1] for f in ("distance", "point", "normal", "barycentric", "block", "cell", "triangle")] == \
        [0, 4, 16, 28, 36, 48, 52]


def test_ray_hit_layout_and_argument_rules_from_c(tmp_path):
    """A pedantic C99 host: the 56-byte record and its offsets, and null / negative arguments answered with status codes."""
    import volumetricterrain_amd as vt
    if not shutil.which("gcc"):
        pytest.skip("gcc not installed")
    vt.load()
    src = tmp_path / "ray_host.c"
    src.write_text("""
#include "vtmc.h"
#include <stddef.h>
#include <stdio.h>
int main(void)
{
    float o[3] = {0, 0, 0}, d[3] = {0, -1, 0};
    vtmc_ray_hit h;
    if (sizeof h != 56) return 2;
    if (offsetof(vtmc_ray_hit, distance) != 0 || offsetof(vtmc_ray_hit, point) != 4 || offsetof(vtmc_ray_hit, normal) != 16 ||
        offsetof(vtmc_ray_hit, barycentric) != 28 || offsetof(vtmc_ray_hit, block) != 36 || offsetof(vtmc_ray_hit, cell) != 48 ||
        offsetof(vtmc_ray_hit, triangle) != 52) return 3;
    if (vtmc_terrain_raycast(NULL, o, d, 1, 1.0f, 0u, &h) != VTMC_ERR_INVALID_ARG) return 4;
    if (vtmc_terrain_raycast(NULL, NULL, NULL, -1, 1.0f, 0u, NULL) != VTMC_ERR_INVALID_ARG) return 5;
    if (vtmc_raycast_device(NULL, NULL, 8, 8, 8, 1, 10, 100, o, 1.0f, NULL, NULL, 1, 1.0f, VTMC_RAY_TWO_SIDED, NULL, NULL) != VTMC_ERR_INVALID_ARG)
        return 6;
    if (vtmc_raycast_device(NULL, NULL, 8, 8, 8, 1, 10, 100, o, 1.0f, NULL, NULL, -3, 1.0f, 0u, NULL, NULL) != VTMC_ERR_INVALID_ARG) return 7;
    puts("ok");
    return 0;
}
""")
    inc, lib = os.path.join(ROOT, "include"), vt.library_path()
    exe = tmp_path / "ray_host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", str(exe), lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-500:])


def test_integration_has_the_raycast_stub():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\[DllImport\([^\]]*\)\]\s*public static extern int vtmc_terrain_raycast\s*\(", text)


def test_reference_plane_known_answers(oracle_mod):
    """f = h - y: the linear field puts every vertex at y = h exactly.  Down from above hits at o.y - h with normal +y; up from
    below hits nothing single-sided (the faces look up) and the same plane two-sided."""
    h = 9.375
    surf = Surface.of_grid(oracle_mod, fields.plane((32, 16, 24), h))
    rng = np.random.default_rng(3)
    o = np.stack([rng.uniform(0.5, 31.5, 64), np.full(64, 15.75), rng.uniform(0.5, 23.5, 64)], 1)
    down = reference(surf, o, np.tile([0.0, -1.0, 0.0], (64, 1)))
    for oo, r in zip(o, down):
        if r["ambiguous"]:
            continue
        assert r["hit"] and abs(r["t"] - (oo[1] - h)) < 1e-9 and np.allclose(r["normal"], [0, 1, 0])
    assert sum(r["ambiguous"] for r in down) <= 2
    below = o.copy()
    below[:, 1] = 0.5
    up = reference(surf, below, np.tile([0.0, 1.0, 0.0], (64, 1)))
    assert not any(r["hit"] for r in up)
    up2 = reference(surf, below, np.tile([0.0, 1.0, 0.0], (64, 1)), two_sided=True)
    assert all(r["hit"] and abs(r["t"] - (h - 0.5)) < 1e-9 for r in up2 if not r["ambiguous"])
    # max_distance cuts it
    assert not any(r["hit"] for r in reference(surf, o[:8], np.tile([0.0, -1.0, 0.0], (8, 1)), max_distance=1.0))


def test_reference_sphere_known_answer(oracle_mod):
    """f = r - |x - c|: a ray through the centre hits within the marching-cubes error of |c - o| - r, from outside; from the centre,
    single-sided, it leaves through back faces and hits nothing."""
    c, rad = np.array([16.3, 15.7, 16.1]), 9.5
    surf = Surface.of_grid(oracle_mod, fields.sphere((32, 32, 32), c, rad))
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(48, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    o = c + 40.0 * dirs
    res = reference(surf, o, -dirs)
    for r in res:
        assert r["hit"] and abs(r["t"] - (40.0 - rad)) < 0.1, r["t"]
        assert r["normal"] @ (r["point"] - c) > 0.9 * np.linalg.norm(r["point"] - c)   # outward
    assert not any(r["hit"] for r in reference(surf, np.tile(c, (16, 1)), dirs[:16]))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_perlin64_device_rays_both_layouts(oracle_mod):
    """4096 seeded rays through vtmc_raycast_device on a 64^3 perlin3d field filled on the device, x-fastest and z-fastest: both
    layouts give bit-identical hits, and the hits agree with the reference; again two-sided, and at voxel_scale 0.5 off the origin."""
    import torch
    import volumetricterrain_amd as vt
    n, dim = 64, 66
    prm = vt.density_params("perlin3d", n)
    with vt.Extractor(0) as ex:
        gx = torch.empty(dim ** 3, dtype=torch.float32, device="cuda")
        gz = torch.empty(dim ** 3, dtype=torch.float32, device="cuda")
        ex.density_fill_device(prm, [[0, 0, 0]], (dim, dim, dim), (1, dim, dim * dim), 0, gx.data_ptr())
        ex.density_fill_device(prm, [[0, 0, 0]], (dim, dim, dim), (dim * dim, dim, 1), 0, gz.data_ptr())
        grid = gx.cpu().numpy().reshape(dim, dim, dim).transpose(2, 1, 0)
        assert np.array_equal(gz.cpu().numpy().reshape(dim, dim, dim).view(np.uint32), grid.view(np.uint32))
        O, D = _rays_perlin(n, 4096, 11)
        for scale, origin, two_sided in ((1.0, (0.0, 0.0, 0.0), False), (1.0, (0.0, 0.0, 0.0), True), (0.5, (3.25, -7.5, 1.0), False)):
            o = (np.float32(origin) + O * np.float32(scale)).astype(np.float32)
            hx = _cast(ex, gx.data_ptr(), (n, n, n), (1, dim, dim * dim), origin, scale, o, D, two_sided=two_sided)
            hz = _cast(ex, gz.data_ptr(), (n, n, n), (dim * dim, dim, 1), origin, scale, o, D, two_sided=two_sided)
            assert hx.tobytes() == hz.tobytes(), "x-fastest and z-fastest grids give different hits"
            surf = Surface.of_grid(oracle_mod, grid, origin, scale)
            ref = reference(surf, o, D, two_sided=two_sided)
            label = "scale %g two_sided %d" % (scale, two_sided)
            n_amb = compare(hx, ref, scale, label)
            report("perlin64 " + label, len(o), n_amb, check_tight(hx, ref, surf, label))
            assert n_amb < 0.01 * len(o), n_amb
            assert (hx["triangle"] >= 0).sum() > len(o) // 3


def _demo_world_edits(rng, k):
    import volumetricterrain_amd as vt
    mods = []
    for i in range(k):
        c = (float(rng.uniform(24, 232)), float(rng.uniform(22, 40)), float(rng.uniform(24, 232)))
        mods.append(vt.SphereModifier(c, float(rng.uniform(4, 12)), bool(i % 3 == 0)))
    return mods


@pytest.mark.gpu
def test_demo_world_terrain_raycast_follows_the_edits(oracle_mod):
    """The demo world (256 x 72 x 256 cells, SceneManager.cs:23-24): a plane, an island heightmap, sphere adds and erodes (some of
    them caves under the ground).  1024 rays through vtmc_terrain_raycast against the reference on terrain_read_samples(); more
    edits through terrain_update; the same rays again see the new surface."""
    import volumetricterrain_amd as vt
    rng = np.random.default_rng(21)
    u = np.linspace(-1, 1, 64, dtype=np.float32)[:, None]
    v = np.linspace(-1, 1, 64, dtype=np.float32)[None, :]
    hm = (14.0 * np.exp(-2.5 * (u * u + v * v)) + 2.0 * np.sin(5 * u) * np.cos(4 * v) + 4.0).astype(np.float32)
    cave_xz = rng.uniform(40, 216, (6, 2))
    caves = [vt.SphereModifier((float(x), 16.0, float(z)), 7.0, False) for x, z in cave_xz]
    first = [vt.PlaneModifier(20.5, (-1, -1), (300, 300), True), vt.IslandModifier(hm, 256.0, 256.0, 30.0, True)] + \
        _demo_world_edits(rng, 24) + caves
    # camera rays looking down onto the world, rays from inside the caves, grazing rays
    k = 1024
    cam = np.stack([rng.uniform(-40, 296, k), rng.uniform(60, 140, k), rng.uniform(-40, 296, k)], 1)
    tgt = np.stack([rng.uniform(0, 256, k), rng.uniform(0, 40, k), rng.uniform(0, 256, k)], 1)
    cam[:128] = np.array([[x, 16.0, z] for x, z in cave_xz])[rng.integers(0, 6, 128)] + rng.uniform(-2, 2, (128, 3))
    tgt[:128] = cam[:128] + rng.normal(size=(128, 3))
    cam[128:192, 1] = rng.uniform(18, 30, 64)
    tgt[128:192, 1] = cam[128:192, 1] + rng.uniform(-3, 3, 64)
    O, D = cam.astype(np.float32), (tgt - cam).astype(np.float32)
    with vt.Extractor(0) as ex:
        ex.terrain_init(256, 72, 256, 1.0, (0.0, 0.0, 0.0), 1)
        for mods in (first, _demo_world_edits(rng, 16) + [vt.SphereModifier((128.0, 30.0, 128.0), 20.0, False)]):
            ex.terrain_update(mods)
            hits = ex.terrain_raycast(O, D)
            surf = Surface.of_grid(oracle_mod, ex.terrain_read_samples())
            ref = reference(surf, O, D)
            n_amb = compare(hits, ref, 1.0, "demo world")
            report("demo world", k, n_amb, check_tight(hits, ref, surf, "demo world"))
            assert n_amb < 0.01 * k, n_amb
            assert (hits["triangle"] >= 0).sum() > k // 2
            if mods is first:
                before = hits.copy()
        assert not np.array_equal(before["distance"], hits["distance"])   # the second queue moved the surface under some rays


@pytest.mark.gpu
def test_edge_cases(oracle_mod):
    """Zero rays, degenerate rays, max_distance, a ray that misses the box, argument errors, and a field with NaN samples: no NaN
    in any hit, and rays that touch no NaN cell answer exactly as on the NaN-free field, whose hits pass the tight check (0 of the
    2048 rays ambiguous, measured with the reference alone)."""
    import torch
    import volumetricterrain_amd as vt
    n = (32, 32, 32)
    g = fields.sphere(n, (16.3, 15.7, 16.1), 9.5)        # x fastest
    dim = 34
    d_g = _device(g.transpose(2, 1, 0).ravel())
    st = (1, dim, dim * dim)
    with vt.Extractor(0) as ex:
        L, h = ex._L, ex._h
        # n_rays = 0: OK, nothing written
        d_h = torch.full((RAY_HIT_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
        org = (ctypes.c_float * 3)(0, 0, 0)
        assert L.vtmc_raycast_device(h, d_g.data_ptr(), 32, 32, 32, *st, ctypes.byref(org), 1.0, None, None, 0, 1.0, 0, None, None) == 0
        assert L.vtmc_raycast_device(h, d_g.data_ptr(), 32, 32, 32, *st, ctypes.byref(org), 1.0, d_g.data_ptr(), d_g.data_ptr(), 0,
                                     1.0, 0, d_h.data_ptr(), None) == 0
        assert ex.copy_to_host(d_h.data_ptr(), RAY_HIT_BYTES).tolist() == [0xAB] * RAY_HIT_BYTES
        # argument errors
        args = lambda n_rays, md, flags, nx=32: (h, d_g.data_ptr(), nx, 32, 32, *st, ctypes.byref(org), 1.0, d_g.data_ptr(),
                                                  d_g.data_ptr(), n_rays, md, flags, d_h.data_ptr(), None)
        assert L.vtmc_raycast_device(*args(-1, 1.0, 0)) == vt._lib.ERR_INVALID_ARG
        assert L.vtmc_raycast_device(*args(1, float("nan"), 0)) == vt._lib.ERR_INVALID_ARG
        assert L.vtmc_raycast_device(*args(1, 0.0, 0)) == vt._lib.ERR_INVALID_ARG
        assert L.vtmc_raycast_device(*args(1, -2.0, 0)) == vt._lib.ERR_INVALID_ARG
        assert L.vtmc_raycast_device(*args(1, 1.0, 4)) == vt._lib.ERR_INVALID_ARG
        assert L.vtmc_raycast_device(*args(1, 1.0, 0, nx=30)) == vt._lib.ERR_DIMS
        assert L.vtmc_raycast_device(h, None, 32, 32, 32, *st, ctypes.byref(org), 1.0, None, None, 1, 1.0, 0, None, None) == vt._lib.ERR_INVALID_ARG
        with pytest.raises(vt.VtmcError) as e:
            ex.terrain_raycast(np.zeros((1, 3)), np.ones((1, 3)))
        assert e.value.code == vt._lib.ERR_NO_RESULT
        nan, inf = float("nan"), float("inf")
        c = np.array([16.3, 15.7, 16.1], np.float32)
        O = np.array([[16.3, 40, 16.1], [16.3, 40, 16.1], [16.3, 40, 16.1], [0, 0, 0], [nan, 1, 1], [1, inf, 1],
                      [-10, -10, -10], [-10, 50, 16], [16.3, 40, 16.1], [16.3, 40, 16.1]], np.float32)
        D = np.array([[0, -1, 0], [0, 0, 0], [nan, -1, 0], [0, 1, 0], [0, 1, 0], [0, -1, 0],
                      [-1, -1, -1], [1, 0, 0], [0, -1e-30, 0], [0, -1e30, 0]], np.float32)
        want = 40 - 15.7 - 9.5
        hits = _cast(ex, d_g.data_ptr(), n, st, (0, 0, 0), 1.0, O, D)
        assert abs(hits["distance"][0] - want) < 0.05 and hits["triangle"][0] >= 0
        assert np.allclose(hits["normal"][0], [0, 1, 0], atol=0.05)
        assert list(hits["triangle"][1:8]) == [-1] * 7 and list(hits["distance"][1:8]) == [-1.0] * 7   # zero / NaN dir, NaN / inf origin, misses
        assert hits["triangle"][8] >= 0 and hits["triangle"][9] >= 0                   # |d| need not be 1
        assert abs(hits["distance"][8] - hits["distance"][0]) < 1e-5 and abs(hits["distance"][9] - hits["distance"][0]) < 1e-5
        d0 = float(hits["distance"][0])
        for md, hit in ((0.5 * d0, False), (d0 * 1.001, True), (inf, True)):
            hh = _cast(ex, d_g.data_ptr(), n, st, (0, 0, 0), 1.0, O[:1], D[:1], max_distance=md)
            assert (hh["triangle"][0] >= 0) == hit, md
        # NaN samples in a box of the field
        rng = np.random.default_rng(8)
        O = rng.uniform(-10, 42, (2048, 3)).astype(np.float32)
        D = (rng.uniform(2, 30, (2048, 3)) - O).astype(np.float32)
        base = _cast(ex, d_g.data_ptr(), n, st, (0, 0, 0), 1.0, O, D)
        surf = Surface.of_grid(oracle_mod, g)
        ref = reference(surf, O, D)
        n_amb = compare(base, ref, 1.0, "sphere")
        report("sphere", len(O), n_amb, check_tight(base, ref, surf, "sphere"))
        assert n_amb < 0.01 * len(O), n_amb
        gn = g.copy()
        gn[10:15, 18:24, 12:17] = np.nan
        gn[20, 5, 9] = np.nan
        d_gn = _device(gn.transpose(2, 1, 0).ravel())
        hn = _cast(ex, d_gn.data_ptr(), n, st, (0, 0, 0), 1.0, O, D)
        for f in ("distance", "point", "normal", "barycentric"):
            assert np.isfinite(hn[f]).all(), f
        # cells next to a NaN sample: [9, 15) x [17, 24) x [11, 17) and [19, 21) x [4, 6) x [8, 10); rays that miss both boxes
        def misses(lo, hi):
            lo, hi = np.array(lo, float) - 1e-3, np.array(hi, float) + 1e-3
            dd = D.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (lo - O) / dd, (hi - O) / dd
                tn = np.nanmax(np.where(dd != 0, np.minimum(t0, t1), -np.inf), axis=1)
                tf = np.nanmin(np.where(dd != 0, np.maximum(t0, t1), np.inf), axis=1)
            inside = np.all((dd != 0) | ((O >= lo) & (O <= hi)), axis=1)
            return ~(inside & (tn <= tf) & (tf >= 0))
        clean = misses((9, 17, 11), (15, 24, 17)) & misses((19, 4, 8), (21, 6, 10))
        assert 500 < clean.sum() < len(O)
        assert hn[clean].tobytes() == base[clean].tobytes()


@pytest.mark.gpu
def test_long_rays_on_a_1024_grid(oracle_mod):
    """256 rays along and near the main diagonals of a 1024^3-cell perlin3d grid (about 3 000 cells each: every lane of the
    workgroup walks its own sub-interval; sample offsets beyond 2^31).  The reference extracts exactly the blocks each clipped segment
    crosses, padded by one block."""
    import torch
    import volumetricterrain_amd as vt
    n, dim = 1024, 1026
    O, D = _long_rays(n, 256, 17)
    with vt.Extractor(0) as ex:
        g = torch.empty(dim ** 3, dtype=torch.float32, device="cuda")
        ex.density_fill_device(vt.density_params("perlin3d", n), [[0, 0, 0]], (dim, dim, dim), (1, dim, dim * dim), 0, g.data_ptr())
        hits = _cast(ex, g.data_ptr(), (n, n, n), (1, dim, dim * dim), (0, 0, 0), 1.0, O, D)
        off = torch.tensor((np.arange(10)[None, None, :] + dim * np.arange(10)[None, :, None] + dim * dim * np.arange(10)[:, None, None]).ravel(),
                           dtype=torch.int64, device="cuda")   # tile[ix + 10 iy + 100 iz]
        n_amb, tight = 0, [0, 0]
        for grp in range(4):
            sel = np.arange(grp, len(O), 4)
            blocks = set()
            for o, d in zip(O[sel].astype(np.float64), D[sel].astype(np.float64)):
                d = d / np.linalg.norm(d)
                ts = np.arange(0.0, 2.0 * n, 0.25)
                p = o + ts[:, None] * d
                p = p[np.all((p >= 0) & (p <= n), axis=1)]
                b = np.unique(np.clip(np.floor(p / 8).astype(np.int64), 0, n // 8 - 1), axis=0)
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dz in (-1, 0, 1):
                            q = b + (dx, dy, dz)
                            q = q[np.all((q >= 0) & (q < n // 8), axis=1)]
                            blocks.update(map(tuple, q.tolist()))
            blocks = np.array(sorted(blocks, key=lambda t: (t[2], t[1], t[0])), np.int64)
            base = torch.from_numpy(8 * (blocks[:, 0] + dim * blocks[:, 1] + dim * dim * blocks[:, 2])).cuda()
            tiles = g[(base[:, None] + off[None, :]).ravel()].reshape(len(blocks), 1000).cpu().numpy()
            tris, _, cases = oracle_mod.extract_tiles(tiles)
            surf = Surface(oracle_mod, tris, blocks, cases)
            ref = reference(surf, O[sel], D[sel])
            n_amb += compare(hits[sel], ref, 1.0, "1024^3 group %d" % grp)
            tight = [a + b for a, b in zip(tight, check_tight(hits[sel], ref, surf, "1024^3 group %d" % grp))]
            del tiles
        report("1024^3 long rays", len(O), n_amb, tight)
        assert n_amb < 0.01 * len(O), n_amb
        assert (hits["triangle"] >= 0).sum() > 128
