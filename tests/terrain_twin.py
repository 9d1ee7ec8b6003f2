"""What the terrain edit tests share (test_terrain_history.py, test_terrain_brushes.py): a modifier spec ("kind", args) as the device's
modifier and as the oracle twin's, and the bit-for-bit / 1e-5 comparisons of the device's grid and triangles against the twin's."""
import numpy as np

import volumetricterrain_amd as vt


def gpu_mod(spec):
    kind, args = spec
    return {"plane": vt.PlaneModifier, "sphere": vt.SphereModifier, "cylinder": vt.CylinderModifier, "island": vt.IslandModifier,
            "smooth": vt.SmoothModifier, "flatten": vt.FlattenModifier}[kind](*args)


def oracle_mod_of(oracle_mod, spec):
    """The reference's kinds only: the oracle has no brushes (test_terrain_brushes.py mirrors them in numpy)."""
    kind, args = spec
    return {"plane": oracle_mod.plane_modifier, "sphere": oracle_mod.sphere_modifier,
            "cylinder": oracle_mod.cylinder_modifier, "island": oracle_mod.heightmap_modifier}[kind](*args)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_grid(ex, want):
    assert np.array_equal(bits(ex.terrain_read_samples()), bits(want))


def assert_triangles(ex, oracle_mod, grid, dirty, T):
    want, want_offs, _ = oracle_mod.extract_grid(np.ascontiguousarray(grid), dirty, threads=8)
    assert T == len(want)
    if T:
        got, offs = ex.read_triangles()
        assert np.array_equal(offs, want_offs) and np.array_equal(got["block"], want["block"])
        for f in ("p0", "p1", "p2", "n0", "n1", "n2"):
            assert np.abs(got[f] - want[f]).max() <= 1e-5
