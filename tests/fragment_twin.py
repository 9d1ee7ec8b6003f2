"""The twin of the fragment query and the detach modifier (vtmc_terrain_fragments / VTMC_MOD_DETACH): a numpy restatement of the FRAGMENTS
rule of include/vtmc.h.  Integers and 32-bit copies only, so everything test_terrain_fragments.py compares with it must be EQUAL.

Grids are float32 arrays indexed [x, y, z], as Extractor.terrain_read_samples returns them.  A box is (first sample, samples per axis).
The labelling is the simplest that is obviously right: every solid sample starts as its own box-linear index, then takes the smallest
label among itself and its solid neighbours along x, y, z, over and over until nothing changes; between two such sweeps every label is
replaced by its label's label (still a sample of the same component), which only speeds the sweeps up."""
import types

import numpy as np

from terrain_twin import sample_range
from volumetricterrain_amd._lib import FRAGMENT_DTYPE
from volumetricterrain_amd.terrainfile import terrain_uniform

f32 = np.float32
NONE = np.int64(2 ** 62)   # the label of a sample that is not solid, above every index


def sample_box(lower, upper, dims, scale, origin):
    """The clamped sample box of world bounds on a terrain of `dims` cells: (first, ext, low, up), ext with a 0 when empty; low / up are
    what the dirty-block rule reads (terrain_twin.dirty_ids)."""
    m = types.SimpleNamespace(lower=[f32(v) for v in lower], upper=[f32(v) for v in upper])
    low, up, first, ext = sample_range(m, tuple(d + 2 for d in dims), scale, origin)
    return tuple(first), tuple(ext), low, up


def box_indices(ext):
    """Box-linear index ix + dx * (iy + dy * iz) of every sample of a box, indexed [x, y, z]."""
    dx, dy, dz = ext
    return np.arange(dx * dy * dz, dtype=np.int64).reshape(dz, dy, dx).transpose(2, 1, 0)


def label(box):
    """Labels of a box of samples [x, y, z]: the smallest box-linear index of its component for a solid sample (s > 0: NaN and both
    zeros are not solid), -1 for the others."""
    solid = box > 0
    lab = np.where(solid, box_indices(box.shape), NONE)
    while True:
        new = lab.copy()
        for axis in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            new[hi] = np.minimum(new[hi], lab[lo])
            new[lo] = np.minimum(new[lo], lab[hi])
        new = np.where(solid, new, NONE)
        flat = new.transpose(2, 1, 0).reshape(-1)                  # flat[box-linear index]
        jumped = np.where(solid, flat[np.where(solid, new, 0)], NONE)
        if np.array_equal(jumped, lab):
            return np.where(solid, lab, -1)
        lab = jumped


def anchored_roots(lab):
    """The labels that occur on any of the six faces of the box."""
    faces = [lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1]]
    r = np.unique(np.concatenate([f.reshape(-1) for f in faces]))
    return r[r >= 0]


def fragments(grid, first, ext, max_samples=0):
    """(records, labels of the box): the records of the fragments of the box in increasing grid index of the seed, FRAGMENT_DTYPE with
    stamp_id 0; labels as label() gives them."""
    if min(ext) <= 0:
        return np.zeros(0, FRAGMENT_DTYPE), None
    (lx, ly, lz), (dx, dy, dz) = first, ext
    lab = label(grid[lx:lx + dx, ly:ly + dy, lz:lz + dz])
    roots, counts = np.unique(lab[lab >= 0], return_counts=True)
    loose = ~np.isin(roots, anchored_roots(lab))
    if max_samples > 0:
        loose &= counts <= max_samples
    recs = np.zeros(int(loose.sum()), FRAGMENT_DTYPE)
    for rec, root, n in zip(recs, roots[loose], counts[loose]):     # np.unique sorts: increasing box-linear index = increasing grid index
        where = np.argwhere(lab == root)
        rec["seed"] = (lx + root % dx, ly + root // dx % dy, lz + root // (dx * dy))
        rec["lo"] = where.min(axis=0) + first
        rec["hi"] = where.max(axis=0) + first
        rec["n_samples"] = n
    return recs, lab


def fragment_mask(lab, recs, first, ext):
    """The samples of the box that belong to a listed fragment."""
    dx, dy, _ = ext
    roots = [(r["seed"][0] - first[0]) + dx * ((r["seed"][1] - first[1]) + dy * (r["seed"][2] - first[2])) for r in recs]
    return np.isin(lab, np.array(roots, np.int64)) & (lab >= 0)


def detach(grid, first, ext, max_samples, seed, event):
    """The grid after VTMC_MOD_DETACH with that box under event number `event`: every sample of every fragment becomes the void draw
    uniform(seed, event, grid index, 2) - 2, every other sample keeps its bits.  Returns (new grid, records)."""
    out = grid.copy()
    recs, lab = fragments(grid, first, ext, max_samples)
    if len(recs):
        (lx, ly, lz), (dx, dy, dz) = first, ext
        Dx, Dy, _ = grid.shape
        gone = fragment_mask(lab, recs, first, ext)
        ix, iy, iz = np.nonzero(gone)
        index = (ix + lx).astype(np.uint64) + np.uint64(Dx) * ((iy + ly).astype(np.uint64) + np.uint64(Dy) * (iz + lz).astype(np.uint64))
        out[ix + lx, iy + ly, iz + lz] = terrain_uniform(seed, event, index, 2) - f32(2)
    return out, recs


def stamp_box(rec, first, ext):
    """(first sample, dims) of a fragment's stamp: its bounds grown by 2, cut to the query box."""
    a = [max(int(rec["lo"][k]) - 2, first[k]) for k in range(3)]
    b = [min(int(rec["hi"][k]) + 2, first[k] + ext[k] - 1) for k in range(3)]
    return tuple(a), tuple(b[k] - a[k] + 1 for k in range(3))


def stamp(grid, lab, rec, first, ext):
    """(first, dims, samples [x, y, z]) of the stamp of one fragment: the grid's bits where the sample is not solid or belongs to the
    fragment, the sign bit flipped where it is solid and belongs to something else."""
    a, n = stamp_box(rec, first, ext)
    root = (rec["seed"][0] - first[0]) + ext[0] * ((rec["seed"][1] - first[1]) + ext[1] * (rec["seed"][2] - first[2]))
    sl = tuple(slice(a[k], a[k] + n[k]) for k in range(3))
    ll = tuple(slice(a[k] - first[k], a[k] - first[k] + n[k]) for k in range(3))
    s, other = grid[sl].copy(), (lab[ll] >= 0) & (lab[ll] != root)
    s[other] = -s[other]
    return a, n, s
