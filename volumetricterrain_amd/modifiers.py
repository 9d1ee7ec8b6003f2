"""Host-side mirror of the reference's TerrainModifier classes (TerrainModifier.cs:19-152): same
names, fields and bound formulas, flattened into the vtmc_modifier struct the C ABI takes.

Only what crosses the boundary lives here -- the AABB properties (LowerBound / UpperBound, which
the reference evaluates on the host, VoxelTerrain.cs:273-279) and the parameters of QueryDensity;
the density itself is evaluated on the GPU (csrc/terrain.hip).  All arithmetic is FP32, in the
order of the C# expressions.
"""
import numpy as np

from . import _lib
from ._lib import (AO_MAX_STEPS, LOD_MAX_LEVEL, MATERIAL_CHANNELS, MESH_MAX_TRIANGLES, MOD_CYLINDER, MOD_DETACH, MOD_EROSION, MOD_FLATTEN, MOD_HEIGHTMAP, MOD_NOISE, MOD_PATH, MOD_PLANE, MOD_SMOOTH, MOD_SPHERE, MOD_STAMP,
                   PATH_MAX_SEGMENTS, STAMP_MAX_DIM, STAMP_MAX_SAMPLES, STAMP_MIN_DIM, Modifier)

_f = np.float32
FLOAT_MIN_VALUE = _f(-3.4028234663852886e38)  # C# float.MinValue


def _vec(v):
    return np.asarray(v, _f).reshape(3)


def _dot(a, b):
    """UnityEngine.Vector3.Dot: a.x*b.x + a.y*b.y + a.z*b.z, FP32, left to right."""
    return _f(_f(_f(a[0] * b[0]) + _f(a[1] * b[1])) + _f(a[2] * b[2]))


def _project_on_plane(v, n):
    """UnityEngine.Vector3.ProjectOnPlane: v - n * Dot(v, n) / Dot(n, n)."""
    return (v - n * (_dot(v, n) / _dot(n, n))).astype(_f)


class TerrainModifier:
    AddOrErode = True  # true -> add (union), false -> erode (difference): TerrainModifier.cs:31-32

    def to_struct(self):
        m = Modifier(self.kind, 1 if self.AddOrErode else 0)
        m.lower[:] = tuple(float(x) for x in self.LowerBound)
        m.upper[:] = tuple(float(x) for x in self.UpperBound)
        p = self.params()
        m.p[0:len(p)] = tuple(float(x) for x in p)
        self.attach(m)
        return m

    def attach(self, m):
        """Hook for modifiers that carry an array (the heightmap)."""


class PlaneModifier(TerrainModifier):
    """f(x,y,z) = y0 - y (TerrainModifier.cs:38-65)."""
    kind = MOD_PLANE

    def __init__(self, height, low, up, addOrErode=True):
        if low[0] > up[0] or low[1] > up[1]:
            raise ValueError("invalud aabb")  # sic, TerrainModifier.cs:52
        self._height, self._low, self._up = _f(height), np.asarray(low, _f), np.asarray(up, _f)
        self.AddOrErode = addOrErode

    @property
    def LowerBound(self):
        return np.array([self._low[0], FLOAT_MIN_VALUE, self._low[1]], _f)

    @property
    def UpperBound(self):
        return np.array([self._up[0], self._height + _f(1), self._up[1]], _f)

    def params(self):
        return [self._height]


class SphereModifier(TerrainModifier):
    """f = r - |p - c| (TerrainModifier.cs:70-91)."""
    kind = MOD_SPHERE

    def __init__(self, center, radius, addOrErode=True):
        self._center, self._radius = _vec(center), _f(radius)
        self.AddOrErode = addOrErode

    @property
    def LowerBound(self):
        return (self._center - self._radius).astype(_f)

    @property
    def UpperBound(self):
        return (self._center + self._radius).astype(_f)

    def params(self):
        return [self._center[0], self._center[1], self._center[2], self._radius]


class CylinderModifier(TerrainModifier):
    """Capped cylinder along _axisDir (TerrainModifier.cs:96-152)."""
    kind = MOD_CYLINDER

    def __init__(self, start, direction, length, radius, addOrErode=True):
        d = _vec(direction)
        self._axisStart = _vec(start)
        self._axisDir = (d / _f(np.sqrt(_dot(d, d)))).astype(_f)  # dir.normalized
        self._axisLength, self._radius = _f(length), _f(radius)
        self.AddOrErode = addOrErode

    def _bound(self, sign):
        end = (self._axisStart + self._axisDir * self._axisLength).astype(_f)
        out = np.zeros(3, _f)
        for a in range(3):
            unit = np.zeros(3, _f)
            unit[a] = sign
            shift = _project_on_plane(unit, self._axisDir) * self._radius
            # LowerBound: dir > 0 ? start : end;  UpperBound: dir < 0 ? start : end (TerrainModifier.cs:104-131)
            from_start = self._axisDir[a] > 0 if sign < 0 else self._axisDir[a] < 0
            out[a] = ((self._axisStart if from_start else end) + shift)[a]
        return out

    @property
    def LowerBound(self):
        return self._bound(-1.0)

    @property
    def UpperBound(self):
        return self._bound(1.0)

    def params(self):
        return [*self._axisStart, *self._axisDir, self._axisLength, self._radius]


class IslandModifier(TerrainModifier):
    """The heightmap modifier of the world build (IslandModifier.cs:34-92, inserted at
    TerrainEngine.cs:87): density = bilinear(_heightmap)(x, z) - y.  The reference fills _heightmap
    from Island.GetElevation (island generation: out of scope here), so this mirror takes the
    float[widthRes, heightRes] array itself plus _island.width / .height / ._maxElevation."""
    kind = MOD_HEIGHTMAP

    def __init__(self, heightmap, island_width, island_height, max_elevation, addOrErode=True):
        self._heightmap = np.ascontiguousarray(heightmap, _f)
        if self._heightmap.ndim != 2:
            raise ValueError("heightmap must be a 2-D array indexed [u, v]")
        self._width, self._height, self._maxElevation = _f(island_width), _f(island_height), _f(max_elevation)
        self.AddOrErode = addOrErode

    @property
    def LowerBound(self):
        return np.array([0, FLOAT_MIN_VALUE, 0], _f)

    @property
    def UpperBound(self):
        return np.array([self._width, self._maxElevation, self._height], _f)

    def params(self):
        return [self._width, self._height]

    def attach(self, m):
        m.data = self._heightmap.ctypes.data   # borrowed: this object outlives the call
        m.data_dims[:] = self._heightmap.shape


# -- sculpt brushes (not in the reference; include/vtmc.h VTMC_MOD_SMOOTH / VTMC_MOD_FLATTEN) ------------------------------------------
# Stencil edits with no pointwise QueryDensity: a brush blends each sample of its box towards a target by w = s * clamp01(2 (1 - d / r)).
# The box is c -/+ r; AddOrErode is ignored by the library.

def _check_brush(center, radius, strength):
    if not np.isfinite(center).all():
        raise ValueError("brush centre must be finite")
    if not np.isfinite(radius) or not radius > 0:
        raise ValueError("brush radius must be finite and > 0")
    if not np.isfinite(strength) or not 0 <= strength <= 1:
        raise ValueError("brush strength must lie in [0, 1]")


class SmoothModifier(TerrainModifier):
    """Relaxes the surface under the brush: each sample towards the 27-point mean of its neighbours as they were before the brush."""
    kind = MOD_SMOOTH

    def __init__(self, center, radius, strength=1.0):
        self._center, self._radius, self._strength = _vec(center), _f(radius), _f(strength)
        _check_brush(self._center, self._radius, self._strength)

    @property
    def LowerBound(self):
        return (self._center - self._radius).astype(_f)

    @property
    def UpperBound(self):
        return (self._center + self._radius).astype(_f)

    def params(self):
        return [*self._center, self._radius, self._strength]


class FlattenModifier(SmoothModifier):
    """Pulls the surface under the brush onto the plane through `center` with normal `normal` (solid on the side -normal points to)."""
    kind = MOD_FLATTEN

    def __init__(self, center, normal, radius, strength=1.0):
        super().__init__(center, radius, strength)
        n = _vec(normal)
        with np.errstate(over="ignore", under="ignore"):
            nn = _dot(n, n) if np.isfinite(n).all() else _f(np.nan)
        if not np.isfinite(nn) or nn == 0:
            raise ValueError("flatten normal must be finite and non-zero")
        self._normal = (n / _f(np.sqrt(nn))).astype(_f)   # normalised as CylinderModifier's axis

    def params(self):
        return [*self._center, self._radius, self._strength, *self._normal]


# -- material paint (include/vtmc.h vtmc_material_paint) -----------------------------------------------------------------------------------
class MaterialStroke:
    """One paint stroke on the material layer (Extractor.paint): every texel within `radius` of `center` (world space) is blended towards
    the one-hot of `channel` (0..3: group 1's r, g, b, a; 4..7: group 2's) by w = strength * clamp01(2 (1 - d / radius)), the sculpt
    brushes' falloff.  No TerrainModifier: paint is not queued with the density edits, not journaled and extracts nothing."""

    def __init__(self, center, radius, channel, strength=1.0):
        with np.errstate(over="ignore"):
            self._center = np.asarray(center, np.float64).astype(_f).reshape(3)
            self._radius, self._strength = _f(radius), _f(strength)
        _check_brush(self._center, self._radius, self._strength)
        if int(channel) != channel or not 0 <= channel < MATERIAL_CHANNELS:
            raise ValueError("stroke channel must be an integer in 0..%d" % (MATERIAL_CHANNELS - 1))
        self._channel = int(channel)

    def to_struct(self):
        s = _lib.MaterialStroke()
        s.center[:] = tuple(float(x) for x in self._center)
        s.radius, s.strength, s.channel = float(self._radius), float(self._strength), self._channel
        return s


class AmbientOcclusion:
    """The parameters of Extractor.vertex_ao (vtmc_ao_params): a march of `steps` samples out to `radius` (world units) along every lattice
    direction in the normal's half space, the occlusion found scaled by `strength`.  The radius may span at most AO_MAX_RADIUS_CELLS cells
    of the terrain it is used on; that limit depends on the terrain's voxel scale and is the library's to refuse."""

    def __init__(self, radius, strength=1.0, steps=4):
        with np.errstate(over="ignore"):
            self._radius, self._strength = _f(radius), _f(strength)
        if not np.isfinite(self._radius) or not self._radius > 0:
            raise ValueError("occlusion radius must be finite and > 0")
        if not np.isfinite(self._strength) or not 0 <= self._strength <= 1:
            raise ValueError("occlusion strength must be finite and in [0, 1]")
        if int(steps) != steps or not 1 <= steps <= AO_MAX_STEPS:
            raise ValueError("occlusion steps must be an integer in 1..%d" % AO_MAX_STEPS)
        self._steps = int(steps)

    def to_struct(self):
        s = _lib.AoParams()
        s.radius, s.strength, s.steps, s.flags = float(self._radius), float(self._strength), self._steps, 0
        return s


class ScatterParams:
    """The parameters of Extractor.scatter_surface (vtmc_scatter_params): `density` instances per world unit^2 of surface; a triangle is
    kept when min_up <= up <= max_up, up the y of its unit face normal (1: flat ground, 0: a wall, -1: a ceiling); an instance when
    min_y <= its world height <= max_y (infinities: no bound) and, with material_channel 0..7, with probability weight / 255 of that
    channel of the material layer (-1: no material filter).  density * voxel_scale^2 may be at most SCATTER_MAX_DENSITY_CELLS; that limit
    depends on the terrain's voxel scale and is the library's to refuse."""

    def __init__(self, density, min_up=-1.0, max_up=1.0, min_y=-np.inf, max_y=np.inf, material_channel=-1, seed=0, max_instances=1 << 24):
        with np.errstate(over="ignore"):
            self._density = _f(density)
            self._up = (_f(min_up), _f(max_up))
            self._y = (_f(min_y), _f(max_y))
        if not np.isfinite(self._density) or not self._density > 0:
            raise ValueError("scatter density must be finite and > 0")
        for name, (lo, hi) in (("up", self._up), ("y", self._y)):
            if np.isnan(lo) or np.isnan(hi) or not lo <= hi:
                raise ValueError("scatter min_%s / max_%s must not be NaN and min <= max" % (name, name))
        if int(material_channel) != material_channel or not -1 <= material_channel < MATERIAL_CHANNELS:
            raise ValueError("scatter material_channel must be an integer in -1..%d" % (MATERIAL_CHANNELS - 1))
        if int(seed) != seed or not 0 <= seed < 1 << 32:
            raise ValueError("scatter seed must be an integer in 0..2^32-1")
        if int(max_instances) != max_instances or not 0 < max_instances < 1 << 31:
            raise ValueError("scatter max_instances must be an integer in 1..2^31-1")
        self._channel, self._seed, self._max = int(material_channel), int(seed), int(max_instances)

    def to_struct(self):
        s = _lib.ScatterParams()
        s.density, s.min_up, s.max_up = float(self._density), float(self._up[0]), float(self._up[1])
        s.min_y, s.max_y = float(self._y[0]), float(self._y[1])
        s.material_channel, s.seed, s.max_instances, s.flags = self._channel, self._seed, self._max, 0
        return s


class LodParams:
    """The parameters of Extractor.terrain_extract_lod (vtmc_lod_params): the viewer in world space, the level of the octree's roots
    (0..LOD_MAX_LEVEL; a root of 8 * 2^max_level cells must divide the terrain, which is the library's to refuse), `split` >= 1 (a node
    splits when the viewer's Chebyshev distance to it, in cells, is below split times its size) and the most nodes the call may select."""

    def __init__(self, viewer, max_level, split=2.0, max_nodes=1 << 18):
        with np.errstate(over="ignore"):
            self._viewer = tuple(_f(v) for v in viewer)
            self._split = _f(split)
        if len(self._viewer) != 3 or not all(np.isfinite(v) for v in self._viewer):
            raise ValueError("viewer must be three finite coordinates")
        if not np.isfinite(self._split) or not self._split >= 1:
            raise ValueError("split must be finite and >= 1")
        if int(max_level) != max_level or not 0 <= max_level <= LOD_MAX_LEVEL:
            raise ValueError("max_level must be an integer in 0..%d" % LOD_MAX_LEVEL)
        if int(max_nodes) != max_nodes or not 0 < max_nodes < 2 ** 31:
            raise ValueError("max_nodes must be an integer in 1..2^31-1")
        self._max_level, self._max_nodes = int(max_level), int(max_nodes)

    def to_struct(self):
        s = _lib.LodParams()
        s.viewer[:] = [float(v) for v in self._viewer]
        s.split, s.max_level, s.max_nodes = float(self._split), self._max_level, self._max_nodes
        return s


class LodSkirtParams:
    """The parameters of Extractor.lod_skirts (vtmc_lodskirt_params): `depth`, how far a skirt hangs from the boundary curve of its node, in
    the node's own cells (finite, > 0, at most LODSKIRT_MAX_DEPTH); all_faces: skirts on every face with a node behind it, not only on
    faces where the level changes."""

    def __init__(self, depth=1.0, all_faces=False):
        with np.errstate(over="ignore"):
            self._depth = _f(depth)
        if not np.isfinite(self._depth) or not 0 < self._depth <= _lib.LODSKIRT_MAX_DEPTH:
            raise ValueError("skirt depth must be finite, > 0 and at most %d" % _lib.LODSKIRT_MAX_DEPTH)
        self._flags = _lib.LODSKIRT_ALL_FACES if all_faces else 0

    def to_struct(self):
        s = _lib.LodSkirtParamsStruct()
        s.depth, s.flags = float(self._depth), self._flags
        return s


# -- noise (include/vtmc.h VTMC_MOD_NOISE) -----------------------------------------------------------------------------------------------
NOISE_BASES = {"fbm": 0, "billow": 1, "ridged": 2}


class NoiseModifier(TerrainModifier):
    """Fractal noise evaluated on the device: the form RidgedMultifractalModifier (TerrainModifier.cs:158-196) takes here, plus fBm and
    billow.  density = amplitude * sum_o(gain^o * basis(noise(p * frequency * lacunarity^o))) + bias - (p.y - ramp_center) * ramp_scale.
    The noise is the library's own Perlin over the density sampler's permutation of `seed`; the reference wraps LibNoise, which it does
    not vendor, so the values are not LibNoise's.  lower / upper None: the reference class's bounds (0, 0, 0) .. (1000, 1000, 1000)
    (TerrainModifier.cs:178-191)."""
    kind = MOD_NOISE

    def __init__(self, seed, octaves, frequency, lacunarity=2.0, gain=0.5, basis="fbm", amplitude=1.0, bias=0.0, ramp_scale=0.0,
                 ramp_center=0.0, ridge_offset=1.0, lower=None, upper=None, add_or_erode=True):
        if basis not in NOISE_BASES:
            raise ValueError("noise basis must be one of %s" % ", ".join(NOISE_BASES))
        if int(octaves) != octaves or not 1 <= octaves <= 16:
            raise ValueError("noise octaves must be an integer in 1..16")
        with np.errstate(over="ignore"):
            self._p = np.array([frequency, lacunarity, gain, amplitude, bias, ramp_scale, ramp_center, ridge_offset], np.float64).astype(_f)
        if not np.isfinite(self._p).all():
            raise ValueError("noise parameters must be finite")
        if not -2 ** 31 <= int(seed) < 2 ** 32:
            raise ValueError("noise seed must fit 32 bits")
        self._seed = int(seed) - 2 ** 32 if int(seed) >= 2 ** 31 else int(seed)   # the C# int _seed
        self._octaves, self._basis = int(octaves), NOISE_BASES[basis]
        self._low = _vec((0.0, 0.0, 0.0) if lower is None else lower)
        self._up = _vec((1000.0, 1000.0, 1000.0) if upper is None else upper)
        self.AddOrErode = add_or_erode

    @property
    def LowerBound(self):
        return self._low

    @property
    def UpperBound(self):
        return self._up

    def params(self):
        return list(self._p)

    def attach(self, m):
        m.data_dims[:] = (self._seed, self._octaves | (self._basis << 8))


# -- stamps (include/vtmc.h VTMC_MOD_STAMP) ----------------------------------------------------------------------------------------------
STAMP_MODES = ("add", "erode", "replace")


def stamp_rotation(q):
    """The rotation matrix (stamp axes -> world) of include/vtmc.h's rule: the float32 quaternion (x, y, z, w) normalised in double."""
    x, y, z, w = (float(v) for v in np.asarray(q, _f))
    n = float(np.sqrt(x * x + y * y + z * z + w * w))
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


class StampModifier(TerrainModifier):
    """Pastes stamp `stamp_id` (Extractor.stamp_create / stamp_capture; `dims` = its (nx, ny, nz), Extractor.stamp_dims) with its centre at
    `position`, turned by the quaternion `rotation` (x, y, z, w; any non-zero length) and with `pitch` world units between neighbouring
    stamp samples.  mode "add" / "erode": the CSG write of the other modifiers; "replace": the stamp's values are written, which makes a
    captured stamp pasted unturned at the voxel scale an exact copy.  The bounds are the world AABB of the turned stamp box; the kernel
    tests the footprint per sample."""
    kind = MOD_STAMP

    def __init__(self, stamp_id, dims, position, rotation=(0.0, 0.0, 0.0, 1.0), pitch=1.0, mode="add"):
        if mode not in STAMP_MODES:
            raise ValueError("stamp mode must be one of %s" % ", ".join(STAMP_MODES))
        if int(stamp_id) != stamp_id or not 0 < stamp_id < 2 ** 31:
            raise ValueError("stamp id must be a positive 32-bit integer")
        dims = tuple(int(n) for n in dims)
        if len(dims) != 3 or not all(STAMP_MIN_DIM <= n <= STAMP_MAX_DIM for n in dims) or dims[0] * dims[1] * dims[2] > STAMP_MAX_SAMPLES:
            raise ValueError("stamp dims must be three numbers in %d..%d with a product of at most 2^27" % (STAMP_MIN_DIM, STAMP_MAX_DIM))
        with np.errstate(over="ignore"):
            self._position = np.asarray(position, np.float64).astype(_f).reshape(3)
            self._rotation = np.asarray(rotation, np.float64).astype(_f).reshape(4)
            self._pitch = _f(pitch)
        if not (np.isfinite(self._position).all() and np.isfinite(self._rotation).all() and np.isfinite(self._pitch)):
            raise ValueError("stamp position, rotation and pitch must be finite")
        if not (self._rotation.astype(np.float64) ** 2).sum() > 0:
            raise ValueError("stamp rotation must be a quaternion of non-zero length")
        if not self._pitch > 0:
            raise ValueError("stamp pitch must be > 0")
        self._id, self._dims, self._mode = int(stamp_id), dims, mode
        self.AddOrErode = mode != "erode"
        # ext_i = sum_j |R_ij| * h * (n_j - 1) / 2, in double
        R, h = stamp_rotation(self._rotation), float(self._pitch)
        self._ext = np.array([sum(abs(R[i][j]) * h * (dims[j] - 1) / 2 for j in range(3)) for i in range(3)], np.float64)

    @property
    def LowerBound(self):
        return (self._position.astype(np.float64) - self._ext).astype(_f)

    @property
    def UpperBound(self):
        return (self._position.astype(np.float64) + self._ext).astype(_f)

    def params(self):
        return [*self._position, *self._rotation, self._pitch]

    def attach(self, m):
        m.data_dims[:] = (self._id, 1 if self._mode == "replace" else 0)


# -- fragments (include/vtmc.h VTMC_MOD_DETACH) ------------------------------------------------------------------------------------------
def fragment_bounds(lower, upper):
    """World bounds of a fragment box as float32 triples; None: without limit on that side (the whole terrain).  NaN is refused."""
    with np.errstate(over="ignore"):
        lo = np.full(3, -np.inf, _f) if lower is None else np.asarray(lower, np.float64).astype(_f).reshape(-1)
        up = np.full(3, np.inf, _f) if upper is None else np.asarray(upper, np.float64).astype(_f).reshape(-1)
    if lo.shape != (3,) or up.shape != (3,) or np.isnan(lo).any() or np.isnan(up).any():
        raise ValueError("fragment bounds must be three numbers each, none of them NaN")
    return lo, up


def fragment_count(n, name):
    if isinstance(n, bool) or int(n) != n or not 0 <= n < 2 ** 31:
        raise ValueError("%s must be an integer in 0..2^31-1" % name)
    return int(n)


class DetachModifier(TerrainModifier):
    """Removes every floating fragment of the box lower..upper (world bounds; None: the whole terrain): the components of solid samples
    (s > 0, joined along x, y, z inside the box) that touch no face of the box.  max_samples > 0 leaves larger fragments alone.  What it
    removes is what Extractor.terrain_fragments with the same arguments lists."""
    kind = MOD_DETACH
    AddOrErode = False

    def __init__(self, lower=None, upper=None, max_samples=0):
        self._low, self._up = fragment_bounds(lower, upper)
        self._max = fragment_count(max_samples, "max_samples")

    @property
    def LowerBound(self):
        return self._low

    @property
    def UpperBound(self):
        return self._up

    def params(self):
        return []

    def attach(self, m):
        m.data_dims[:] = (self._max, 0)


# -- erosion (include/vtmc_erosion.h VTMC_MOD_EROSION) -----------------------------------------------------------------------------------
def erosion_fault(p, iterations):
    """What csrc/terrain_erosion.h's erosion_args_fault says of the eight float32 parameters (rain, evaporation, capacity, dissolve,
    deposit, dt, talus, thermal_rate) and the iteration count, in its words, or None."""
    p = np.asarray(p, _f)
    if not np.isfinite(p).all():
        return "parameter not finite"
    if (p < 0).any():
        return "parameter negative"
    if p[0] > _f(_lib.EROSION_MAX_RAIN):
        return "rain above VTMC_EROSION_MAX_RAIN"
    if p[2] > _f(_lib.EROSION_MAX_CAPACITY):
        return "capacity above VTMC_EROSION_MAX_CAPACITY"
    if p[3] > 1:
        return "dissolve outside 0..1"
    if p[4] > 1:
        return "deposit outside 0..1"
    if not p[5] > 0 or p[5] > 1:
        return "dt outside (0, 1]"
    if p[7] > _f(_lib.EROSION_MAX_THERMAL):
        return "thermal rate above VTMC_EROSION_MAX_THERMAL"
    if _f(p[1] * p[5]) > 1:
        return "evaporation * dt above 1"
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= iterations <= _lib.EROSION_MAX_ITERATIONS:
        return "iterations outside 1..VTMC_EROSION_MAX_ITERATIONS"
    return None


class ErosionModifier(TerrainModifier):
    """Hydraulic and thermal erosion of the heightfield of the box lower..upper (world bounds; None: the whole terrain), simulated on the
    device for `iterations` steps by the rule EROSION of include/vtmc_erosion.h.  Everything but the box is in GRID units.  rain: depth per
    unit time; evaporation; capacity: sediment a unit of speed and slope carries; dissolve, deposit in 0..1; dt in (0, 1]; talus: the
    largest stable height step between neighbouring columns; thermal_rate in 0..EROSION_MAX_THERMAL, 0 turns the thermal part off.  The
    checks are the library's (ValueError here, VTMC_ERR_INVALID_ARG there, the same words).  AddOrErode is ignored by the library.  The
    maps of the run are read with Extractor.erosion_info / erosion_read / device_erosion."""
    kind = MOD_EROSION

    def __init__(self, lower, upper, iterations, rain=0.01, evaporation=0.02, capacity=1.0, dissolve=0.3, deposit=0.3, dt=0.25, talus=1.0,
                 thermal_rate=0.0):
        self._low, self._up = fragment_bounds(lower, upper)
        with np.errstate(over="ignore"):
            self._p = np.array([rain, evaporation, capacity, dissolve, deposit, dt, talus, thermal_rate], np.float64).astype(_f)
        fault = erosion_fault(self._p, iterations)
        if fault:
            raise ValueError("erosion " + fault)
        self._iterations = int(iterations)

    @property
    def LowerBound(self):
        return self._low

    @property
    def UpperBound(self):
        return self._up

    def params(self):
        return list(self._p)

    def attach(self, m):
        m.data_dims[:] = (self._iterations, 0)


# -- navigation (include/vtmc_nav.h) ----------------------------------------------------------------------------------------------------
class NavParams:
    """The parameters of Extractor.terrain_nav in WORLD units: the agent's height (the headroom a floor needs) and the largest step between
    neighbour columns, and the most spans the call may make.  to_struct(voxel_scale) gives the vtmc_nav_params of a terrain of that scale:
    agent_height = ceil(height / voxel_scale) samples (1..NAV_MAX_AGENT_HEIGHT is the library's to refuse), max_step / voxel_scale grid
    units, both in float32."""

    def __init__(self, agent_height, max_step, max_spans=1 << 24):
        with np.errstate(over="ignore"):
            self._height, self._step = _f(agent_height), _f(max_step)
        if not np.isfinite(self._height) or not self._height > 0:
            raise ValueError("nav agent_height must be finite and > 0")
        if not np.isfinite(self._step) or not self._step >= 0:
            raise ValueError("nav max_step must be finite and >= 0")
        if isinstance(max_spans, bool) or int(max_spans) != max_spans or not 0 < max_spans < 2 ** 31:
            raise ValueError("nav max_spans must be an integer in 1..2^31-1")
        self._max = int(max_spans)

    def to_struct(self, voxel_scale):
        scale = _f(voxel_scale)
        with np.errstate(over="ignore"):
            samples = float(np.ceil(self._height / scale))
            step = self._step / scale
        if not samples < 2.0 ** 31 or not np.isfinite(step):
            raise ValueError("nav parameters overflow at voxel scale %r" % (voxel_scale,))
        s = _lib.NavParamsStruct()
        s.agent_height, s.max_step, s.max_spans, s.flags = int(samples), float(step), self._max, 0
        return s


class NavErodeParams:
    """The parameters of Extractor.nav_distance and Extractor.nav_erode in WORLD units: the agent's radius, and whether the faces of the
    nav box count as open (a box cut out of a larger walkable area does not erode from its own faces).  to_struct(voxel_scale) gives the
    vtmc_naverode_params of a terrain of that scale: radius = ceil(radius / voxel_scale) columns in float32, as NavParams does for the
    height (0..NAVERODE_MAX_RADIUS is the library's to refuse); radius 0 stays 0."""

    def __init__(self, radius, open_box_faces=False):
        with np.errstate(over="ignore"):
            self._radius = _f(radius)
        if not np.isfinite(self._radius) or not self._radius >= 0:
            raise ValueError("nav erode radius must be finite and >= 0")
        self._open = bool(open_box_faces)

    def to_struct(self, voxel_scale):
        scale = _f(voxel_scale)
        with np.errstate(over="ignore"):
            columns = float(np.ceil(self._radius / scale))
        if not columns < 2.0 ** 31:
            raise ValueError("nav erode radius overflows at voxel scale %r" % (voxel_scale,))
        s = _lib.NavErodeParamsStruct()
        s.radius, s.flags = int(columns), _lib.NAVERODE_OPEN_BOX_FACES if self._open else 0
        return s


class NavSightParams:
    """The parameters of Extractor.nav_trace_smooth: how many spans ahead of a waypoint are tried as the next one (1..NAVSIGHT_MAX_LOOK is
    the library's to refuse), and how much a straight stretch may cost above the field's own path between its ends, in the field's cost
    units; None: any (NAVSIGHT_ANY_COST), the smoothing is geometric only."""

    def __init__(self, max_look=64, max_extra_cost=None):
        if isinstance(max_look, bool) or int(max_look) != max_look or not -2 ** 31 <= max_look < 2 ** 31:
            raise ValueError("nav sight max_look must be an integer")
        if max_extra_cost is not None and (isinstance(max_extra_cost, bool) or int(max_extra_cost) != max_extra_cost or not 0 <= max_extra_cost < _lib.NAVSIGHT_ANY_COST):
            raise ValueError("nav sight max_extra_cost must be None or an integer in 0..2^32-2")
        self._look, self._extra = int(max_look), _lib.NAVSIGHT_ANY_COST if max_extra_cost is None else int(max_extra_cost)

    def to_struct(self):
        s = _lib.NavSightParamsStruct()
        s.max_look, s.max_extra_cost, s.flags, s.reserved = self._look, self._extra, 0, 0
        return s


class NavCrowdParams:
    """The parameters of Extractor.navcrowd_step: how much a step may cost above the cheapest one when that one is taken, in the field's
    cost units; None: any (NAVCROWD_ANY_DETOUR), an agent sidesteps to whatever neighbour lies nearer the goal.  leave_on_arrival: an agent
    that arrives leaves the crowd (GONE) and frees its span, where otherwise it stays on it (ARRIVED)."""

    def __init__(self, max_detour=None, leave_on_arrival=False):
        if max_detour is not None and (isinstance(max_detour, bool) or int(max_detour) != max_detour or not 0 <= max_detour < _lib.NAVCROWD_ANY_DETOUR):
            raise ValueError("nav crowd max_detour must be None or an integer in 0..2^32-2")
        self._detour, self._flags = _lib.NAVCROWD_ANY_DETOUR if max_detour is None else int(max_detour), _lib.NAVCROWD_LEAVE_ON_ARRIVAL if leave_on_arrival else 0

    def to_struct(self):
        s = _lib.NavCrowdParamsStruct()
        s.max_detour, s.flags, s.reserved[0], s.reserved[1] = self._detour, self._flags, 0, 0
        return s


class NavFieldParams:
    """The parameters of Extractor.nav_field: what a unit of height climbed and a unit dropped add to a step's cost, in level steps (a
    level step costs NAVFIELD_UNIT), both in [0, 1024], and the cost beyond which a span counts as unreached.  The costs are dimensionless
    per GRID unit, so to_struct needs no voxel scale."""

    def __init__(self, climb_cost, drop_cost, max_cost=0x7fffffff):
        with np.errstate(over="ignore"):
            self._climb, self._drop = _f(climb_cost), _f(drop_cost)
        for name, v in (("climb_cost", self._climb), ("drop_cost", self._drop)):
            if not np.isfinite(v) or not 0 <= v <= 1024:
                raise ValueError("navfield %s must be finite and in [0, 1024]" % name)
        if isinstance(max_cost, bool) or int(max_cost) != max_cost or not 1 <= max_cost <= 0x7fffffff:
            raise ValueError("navfield max_cost must be an integer in 1..2^31-1")
        self._max = int(max_cost)

    def to_struct(self):
        s = _lib.NavFieldParamsStruct()
        s.climb_cost, s.drop_cost, s.max_cost, s.flags = float(self._climb), float(self._drop), self._max, 0
        return s


class LightParams:
    """The parameters of Extractor.terrain_light (vtmc_light_params): the level the open sky emits (0..255; 0: no sky light) and what each
    channel loses per hop through the open samples (1..255)."""

    def __init__(self, sky_level=255, sky_falloff=16, torch_falloff=16):
        for name, v, lowest in (("sky_level", sky_level, 0), ("sky_falloff", sky_falloff, 1), ("torch_falloff", torch_falloff, 1)):
            if isinstance(v, bool) or int(v) != v or not lowest <= v <= 255:
                raise ValueError("light %s must be an integer in %d..255" % (name, lowest))
        self._sky, self._sky_falloff, self._torch_falloff = int(sky_level), int(sky_falloff), int(torch_falloff)

    def to_struct(self):
        s = _lib.LightParamsStruct()
        s.sky_level, s.sky_falloff, s.torch_falloff, s.flags = self._sky, self._sky_falloff, self._torch_falloff, 0
        return s


# -- mesh stamps (include/vtmc.h vtmc_stamp_from_mesh) ------------------------------------------------------------------------------------
MESH_MAX_COORDINATE = 2.0 ** 20


def _stamp_dims(dims):
    dims = tuple(int(n) for n in dims)
    if len(dims) != 3 or not all(STAMP_MIN_DIM <= n <= STAMP_MAX_DIM for n in dims) or dims[0] * dims[1] * dims[2] > STAMP_MAX_SAMPLES:
        raise ValueError("stamp dims must be three numbers in %d..%d with a product of at most 2^27" % (STAMP_MIN_DIM, STAMP_MAX_DIM))
    return dims


def mesh_stamp_box(vertices, pitch, margin=4):
    """The stamp box of a mesh, (first, dims, centre): the mesh's AABB grown by `margin` samples and snapped to the lattice of `pitch`
    (first = pitch * (floor(min / pitch) - margin), the last sample at pitch * (ceil(max / pitch) + margin)), and the world position
    centre = first + pitch * (dims - 1) / 2 that StampModifier(position=centre, pitch=pitch) needs to put every sample back where it was
    voxelized.  Mesh -> stamp -> a paste turned by q at twice the size:
        first, dims, centre = mesh_stamp_box(v, pitch); sid = ex.stamp_from_mesh(v, tri, first, pitch, dims)
        ex.terrain_update([StampModifier(sid, dims, where, rotation=q, pitch=2 * pitch).to_struct()])"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    h = float(_f(pitch))
    if not (len(v) and np.isfinite(v).all() and np.isfinite(h) and h > 0 and int(margin) == margin and margin >= 0):
        raise ValueError("mesh_stamp_box needs finite vertices, a finite pitch > 0 and a whole margin >= 0")
    lo = np.floor(v.min(axis=0) / h).astype(np.int64) - int(margin)
    hi = np.ceil(v.max(axis=0) / h).astype(np.int64) + int(margin)
    dims = _stamp_dims(hi - lo + 1)
    first = (lo * h).astype(_f)
    centre = (first.astype(np.float64) + h * (np.array(dims) - 1) / 2).astype(_f)
    return first, dims, centre


def mesh_stamp_args(vertices, triangles, first, pitch, dims):
    """What vtmc_stamp_from_mesh takes, checked as the library checks it (ValueError here, VTMC_ERR_INVALID_ARG there) except for the
    closed-mesh rule, which stays the library's: (positions float32 (n, 3), indices int32 (m, 3), first float32 (3,), pitch, dims)."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.ascontiguousarray(np.asarray(vertices, np.float64).astype(_f))
        f = np.asarray(first, np.float64).astype(_f).reshape(-1)
        h = _f(pitch)
    t = np.asarray(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or len(v) < 3:
        raise ValueError("mesh vertices must be an (n, 3) array with n >= 3")
    if t.ndim != 2 or t.shape[1] != 3 or not 1 <= len(t) <= MESH_MAX_TRIANGLES or t.dtype.kind not in "iu":
        raise ValueError("mesh triangles must be an (m, 3) integer array with m in 1..%d" % MESH_MAX_TRIANGLES)
    if t.min() < 0 or t.max() >= len(v):
        raise ValueError("mesh triangle index outside the %d vertices" % len(v))
    if not np.isfinite(v).all() or np.abs(v).max() > MESH_MAX_COORDINATE:
        raise ValueError("mesh positions must be finite and at most 2^20 in magnitude")
    if f.shape != (3,) or not np.isfinite(f).all():
        raise ValueError("first must be three finite numbers")
    if not (np.isfinite(h) and h > 0):
        raise ValueError("mesh stamp pitch must be finite and > 0")
    return v, np.ascontiguousarray(t, np.int32), f, h, _stamp_dims(dims)


# -- paths (include/vtmc.h VTMC_MOD_PATH) ------------------------------------------------------------------------------------------------
PATH_MAX_COORDINATE = 2.0 ** 20


class PathModifier(TerrainModifier):
    """Carves (or, with addOrErode, builds) along curves in one pass: the union of tapered capsules over `segments`, an (n, 8) float32
    array of ax, ay, az, ra, bx, by, bz, rb -- the world-space end points and the radius at each end; round ends, the radius linear in
    between.  A segment soup: polylines (from_polyline), trees such as the reference's RiverNode (from_tree) and disjoint pieces alike.
    The library's own shape, not the value of the reference's queue of one eroding CylinderModifier per river segment
    (RiverRenderer.cs:151-170).  The bounds are the AABB of all end points grown by their radii, in float32."""
    kind = MOD_PATH

    def __init__(self, segments, addOrErode=False):
        with np.errstate(over="ignore"):
            seg = np.ascontiguousarray(np.asarray(segments, np.float64).astype(_f))
        if seg.ndim != 2 or seg.shape[1] != 8 or not 1 <= seg.shape[0] <= PATH_MAX_SEGMENTS:
            raise ValueError("path segments must be an (n, 8) array with n in 1..%d" % PATH_MAX_SEGMENTS)
        if not np.isfinite(seg).all():
            raise ValueError("path segments must be finite")
        if (seg[:, [3, 7]] < 0).any():
            raise ValueError("path radii must not be negative")
        if (np.abs(seg) > PATH_MAX_COORDINATE).any():
            raise ValueError("path coordinates and radii must not exceed 2^20 in magnitude")
        self._segments = seg
        self.AddOrErode = addOrErode

    @classmethod
    def from_polyline(cls, points, radii, addOrErode=False):
        """One segment per pair of neighbouring points; radii: one number, or one per point."""
        pts = np.asarray(points, np.float64).reshape(-1, 3)
        if len(pts) < 2:
            raise ValueError("a polyline needs at least two points")
        r = np.broadcast_to(np.asarray(radii, np.float64), (len(pts),))
        return cls(np.column_stack([pts[:-1], r[:-1], pts[1:], r[1:]]), addOrErode)

    @classmethod
    def from_tree(cls, positions, radii, parent, addOrErode=False):
        """One segment per node that has a parent (parent[i] >= 0), in node order, from the parent's position to the node's with the
        radius of each end: the shape of the reference's RiverNode tree."""
        pts = np.asarray(positions, np.float64).reshape(-1, 3)
        r = np.broadcast_to(np.asarray(radii, np.float64), (len(pts),))
        par = np.asarray(parent, np.int64).reshape(-1)
        if len(par) != len(pts) or (par >= len(pts)).any():
            raise ValueError("parent must name a node, or be negative for a root, once per position")
        kids = np.nonzero(par >= 0)[0]
        if not len(kids):
            raise ValueError("a tree needs at least one node with a parent")
        up = par[kids]
        return cls(np.column_stack([pts[up], r[up], pts[kids], r[kids]]), addOrErode)

    @property
    def segments(self):
        return self._segments

    @property
    def LowerBound(self):
        s = self._segments
        return np.minimum((s[:, 0:3] - s[:, 3:4]).min(axis=0), (s[:, 4:7] - s[:, 7:8]).min(axis=0)).astype(_f)

    @property
    def UpperBound(self):
        s = self._segments
        return np.maximum((s[:, 0:3] + s[:, 3:4]).max(axis=0), (s[:, 4:7] + s[:, 7:8]).max(axis=0)).astype(_f)

    def params(self):
        return []

    def attach(self, m):
        m.data = self._segments.ctypes.data   # borrowed: the struct keeps the array alive
        m.data_dims[:] = self._segments.shape
        m._keep = self._segments
