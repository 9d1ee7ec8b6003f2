"""What the extraction tests share (test_gpu_parity.py, test_indexed.py, test_random_shapes.py, test_tuning_matrix.py,
test_memory_orders.py): the comparisons of soup and indexed output against the oracle, a torch view of a raw device pointer, and the
plane-wave fields of the random-shape tests."""
import numpy as np

import fields

ATOL = 1e-5  # north_star tolerance for positions / normals
FLOATS = ("p0", "p1", "p2", "n0", "n1", "n2")


def assert_tris_match(got, want, atol=ATOL):
    assert len(got) == len(want)
    assert np.array_equal(got["block"], want["block"])
    worst = 0.0
    for f in ("p0", "p1", "p2", "n0", "n1", "n2"):
        g, w = got[f], want[f]
        nan_g, nan_w = np.isnan(g), np.isnan(w)
        assert np.array_equal(nan_g, nan_w), "NaN pattern differs in " + f
        d = np.abs(np.where(nan_w, 0, g) - np.where(nan_w, 0, w))
        worst = max(worst, float(d.max()) if d.size else 0.0)
    assert worst <= atol, "max abs deviation %g > %g" % (worst, atol)
    return worst


def check_against_oracle(ex, oracle_mod, g, blocks=None, exact_floats=False):
    want_v, want_i, want_vo, want_to = oracle_mod.extract_grid_indexed(g, blocks)
    soup, _, _ = oracle_mod.extract_grid(g, blocks, threads=8)
    T = ex.extract_grid(g, blocks)
    assert T == len(want_i)
    verts, idx, voffs, toffs = ex.read_indexed_mesh()
    assert np.array_equal(voffs, want_vo) and np.array_equal(toffs, want_to)
    assert np.array_equal(idx, want_i)
    for f in ("position", "normal"):
        nan_w = np.isnan(want_v[f])
        assert np.array_equal(np.isnan(verts[f]), nan_w)
        d = np.abs(np.where(nan_w, 0, verts[f]) - np.where(nan_w, 0, want_v[f]))
        worst = float(d.max()) if d.size else 0.0
        assert worst <= (0.0 if exact_floats else ATOL), (f, worst)
    back = oracle_mod.deindex(verts, idx, voffs, toffs)
    assert np.array_equal(back["block"], soup["block"])
    for f in FLOATS:
        ok = ~np.isnan(soup[f])
        assert np.abs(back[f][ok] - soup[f][ok]).max(initial=0.0) <= ATOL
    return len(verts), T


class _DeviceArray:
    """Exposes a raw device pointer to torch through __cuda_array_interface__ (no copy, no HIP binding)."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<i4", "data": (int(ptr), False), "version": 2}


def device_view_i32(ptr, count):
    import torch
    return torch.as_tensor(_DeviceArray(ptr, count), device="cuda")


def smooth_field(rng, n, order):
    """A few random plane waves: surfaces of varying density, some cells with exact zeros."""
    g = fields._idx((n[0] + 2, n[1] + 2, n[2] + 2), order)
    x, y, z = np.meshgrid(*[np.arange(d + 2, dtype=np.float32) for d in n], indexing="ij")
    acc = np.zeros(x.shape, np.float32)
    for _ in range(rng.integers(1, 5)):
        k = rng.normal(size=3).astype(np.float32) * np.float32(rng.uniform(0.05, 0.9))
        acc += np.float32(rng.uniform(0.3, 1.0)) * np.sin(k[0] * x + k[1] * y + k[2] * z + np.float32(rng.uniform(0, 6.28)))
    acc += np.float32(rng.uniform(-0.5, 0.5))
    if rng.random() < 0.3:
        acc = np.where(rng.random(acc.shape) < 0.05, np.float32(0.0), acc)
    g[...] = acc.astype(np.float32)
    return g
