// voxel_terrain.hpp -- C++ host-side mirror of the reference's chunk host API for the extraction
// path: PGRTerrain.Render.VoxelTerrain and the TerrainModifier interface
// (reference: Unity-Project/Assets/Scripts/VoxelTerrain.cs, TerrainModifier.cs, Utility.cs).
//
// Same names, argument meaning and error behaviour as the C# class, so a maintainer can diff them:
//   Init / InsertModifier / Update / Free          VoxelTerrain.cs:121, :251, :262, :214
//   SetControlMap, _matControlFineness             VoxelTerrain.cs:186-209, :113 (device-resident terrains: the layer of vtmc_material_*)
//   BatchUpdate (private there, public here for tests) VoxelTerrain.cs:330-477
//   _width/_elevation/_height, _voxelScale, TerrainOrigin, blockSize, maxSampleResolution
// What differs on purpose: the three ComputeShader fields and the nine ComputeBuffer bindings
// (VoxelTerrain.cs:64-66, :370-421) are replaced by ONE vtmc context (include/vtmc.h); Unity
// objects (GameObject / Mesh / MeshCollider / Material) have no equivalent here --
// a block's result is a plain BlockMesh {vertices, normals, triangles}; the control maps SetControlMap hands to the Material live in the
// context's material layer instead, and what the shaders would sample from them comes back per vertex (VertexMaterials).  No CPU extraction path
// exists: without libvtmc.so + a HIP device Init() throws.
#ifndef VTMC_HOST_VOXEL_TERRAIN_HPP
#define VTMC_HOST_VOXEL_TERRAIN_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <deque>
#include <functional>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

struct vtmc_ctx;

namespace PGRTerrain {

// UnityEngine.Vector3 stand-in (only what the path uses)
struct Vector3 {
    float x = 0, y = 0, z = 0;
    Vector3() = default;
    Vector3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    Vector3 operator+(const Vector3 &o) const { return {x + o.x, y + o.y, z + o.z}; }
    Vector3 operator-(const Vector3 &o) const { return {x - o.x, y - o.y, z - o.z}; }
    Vector3 operator*(float s) const { return {x * s, y * s, z * s}; }
    Vector3 operator/(float s) const { return {x / s, y / s, z / s}; }
    float sqrMagnitude() const { return x * x + y * y + z * z; }
    float magnitude() const;
    Vector3 normalized() const;
    static float Dot(const Vector3 &a, const Vector3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
    static Vector3 ProjectOnPlane(const Vector3 &v, const Vector3 &n);
};
struct Vector2 {
    float x = 0, y = 0;
};
// UnityEngine.Color stand-in
struct Color {
    float r = 0, g = 0, b = 0, a = 0;
};
static_assert(sizeof(Color) == 16, "a Color[] is read as rgba floats");

namespace MathHelper {
// Utility.cs:17-47 -- the block-index key
struct Int3 {
    int _x = 0, _y = 0, _z = 0;
    Int3() = default;
    Int3(int x, int y, int z) : _x(x), _y(y), _z(z) {}
    bool operator==(const Int3 &o) const { return _x == o._x && _y == o._y && _z == o._z; }
    int GetHashCode() const { return ((17 * 23 + _x) * 23 + _y) * 23 + _z; }  // Utility.cs:37-46
};
}  // namespace MathHelper

namespace Render {

// UnityException stand-in: thrown where the reference throws (VoxelTerrain.cs:123-142 ...)
class UnityException : public std::runtime_error {
public:
    using std::runtime_error::runtime_error;
};

// What the GPU needs to evaluate a modifier itself (vtmc_modifier of include/vtmc.h, redeclared so
// this header stays free of the C ABI): kind 0 plane, 1 sphere, 2 cylinder + their parameters.
struct ModifierDesc {
    int kind = -1;
    float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const float *data = nullptr;  // kind 3 (heightmap): float[dims[0]][dims[1]], owned by the modifier
    int dims[2] = {0, 0};
};

// TerrainModifier.cs:19-33
class TerrainModifier {
public:
    virtual ~TerrainModifier() = default;
    virtual Vector3 LowerBound() const = 0;
    virtual Vector3 UpperBound() const = 0;
    virtual float QueryDensity(const Vector3 &pos) const = 0;  // > 0 solid, < 0 air
    bool AddOrErode = true;                                    // true: union, false: difference
    // New: modifiers the library can evaluate on the device describe themselves; any other
    // (user-defined QueryDensity) returns false and is applied by the host loop as in the reference.
    virtual bool Describe(ModifierDesc &) const { return false; }
};

// TerrainModifier.cs:38-65  f = y0 - y
class PlaneModifier : public TerrainModifier {
public:
    float _height;
    Vector2 _low, _up;
    PlaneModifier(float height, Vector2 low, Vector2 up, bool addOrErode);
    Vector3 LowerBound() const override { return {_low.x, std::numeric_limits<float>::lowest(), _low.y}; }
    Vector3 UpperBound() const override { return {_up.x, _height + 1, _up.y}; }
    float QueryDensity(const Vector3 &pos) const override { return _height - pos.y; }
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 0;
        d.p[0] = _height;
        return true;
    }
};

// TerrainModifier.cs:70-91  f = r - |p - c|
class SphereModifier : public TerrainModifier {
public:
    Vector3 _center;
    float _radius;
    SphereModifier(Vector3 center, float radius, bool addOrErode) : _center(center), _radius(radius) { AddOrErode = addOrErode; }
    Vector3 LowerBound() const override { return {_center.x - _radius, _center.y - _radius, _center.z - _radius}; }
    Vector3 UpperBound() const override { return {_center.x + _radius, _center.y + _radius, _center.z + _radius}; }
    float QueryDensity(const Vector3 &pos) const override { return _radius - (pos - _center).magnitude(); }
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 1;
        d.p[0] = _center.x;
        d.p[1] = _center.y;
        d.p[2] = _center.z;
        d.p[3] = _radius;
        return true;
    }
};

// TerrainModifier.cs:96-152
class CylinderModifier : public TerrainModifier {
public:
    Vector3 _axisStart, _axisDir;
    float _axisLength, _radius;
    CylinderModifier(Vector3 start, Vector3 dir, float length, float radius, bool addOrErode);
    Vector3 LowerBound() const override;
    Vector3 UpperBound() const override;
    float QueryDensity(const Vector3 &pos) const override;
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 2;
        d.p[0] = _axisStart.x;
        d.p[1] = _axisStart.y;
        d.p[2] = _axisStart.z;
        d.p[3] = _axisDir.x;
        d.p[4] = _axisDir.y;
        d.p[5] = _axisDir.z;
        d.p[6] = _axisLength;
        d.p[7] = _radius;
        return true;
    }
};

// IslandModifier.cs:34-92: density = bilinear(_heightmap)(x, z) - y.  The reference fills _heightmap
// from Island.GetElevation (island generation, out of scope): this mirror is handed the array.
class IslandModifier : public TerrainModifier {
public:
    float _islandWidth, _islandHeight, _maxElevation;
    int _widthRes, _heightRes;
    std::vector<float> _heightmap;  // [u * _heightRes + v], as the C# float[widthRes, heightRes]
    IslandModifier(std::vector<float> heightmap, int widthRes, int heightRes, float islandWidth, float islandHeight,
                   float maxElevation, bool addOrErode = true);
    Vector3 LowerBound() const override { return {0, std::numeric_limits<float>::lowest(), 0}; }
    Vector3 UpperBound() const override { return {_islandWidth, _maxElevation, _islandHeight}; }
    float QueryDensity(const Vector3 &pos) const override;
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 3;
        d.p[0] = _islandWidth;
        d.p[1] = _islandHeight;
        d.data = _heightmap.data();
        d.dims[0] = _widthRes;
        d.dims[1] = _heightRes;
        return true;
    }
};

// New (not in the reference): pastes a stamp the vtmc context keeps in device memory (vtmc_stamp_create / _capture, VTMC_MOD_STAMP of
// include/vtmc.h) with its centre at _position, turned by the quaternion _rotation (x, y, z, w; any non-zero length) and with _pitch world
// units between neighbouring stamp samples.  Device-resident terrains only: the samples live on the GPU, so QueryDensity throws.
// LowerBound / UpperBound: the world AABB of the turned stamp box, t_i -/+ sum_j |R_ij| * h * (n_j - 1) / 2, in double, rounded to float.
class StampModifier : public TerrainModifier {
public:
    enum Mode { Add, Erode, Replace };
    int _stampId;
    int _dims[3];
    Vector3 _position;
    float _rotation[4];
    float _pitch;
    Mode _mode;
    StampModifier(int stampId, int nx, int ny, int nz, Vector3 position, float qx, float qy, float qz, float qw, float pitch, Mode mode)
        : _stampId(stampId), _dims{nx, ny, nz}, _position(position), _rotation{qx, qy, qz, qw}, _pitch(pitch), _mode(mode)
    {
        const double n2 = (double)qx * qx + (double)qy * qy + (double)qz * qz + (double)qw * qw;
        if (stampId <= 0 || nx < 2 || ny < 2 || nz < 2 || nx > 1026 || ny > 1026 || nz > 1026 || (long long)nx * ny * nz > (1ll << 27) ||
            !std::isfinite(position.x) || !std::isfinite(position.y) || !std::isfinite(position.z) || !std::isfinite(n2) || !(n2 > 0) ||
            !std::isfinite(pitch) || !(pitch > 0))
            throw std::invalid_argument("StampModifier: invalid stamp id, dims, position, rotation or pitch");
        AddOrErode = mode != Erode;
        double x = qx, y = qy, z = qz, w = qw;
        const double n = std::sqrt(x * x + y * y + z * z + w * w);
        x /= n, y /= n, z /= n, w /= n;
        const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                                {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                                {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
        const double h = pitch;
        for (int i = 0; i < 3; ++i) {
            _ext[i] = 0;
            for (int j = 0; j < 3; ++j) _ext[i] += std::fabs(R[i][j]) * h * (_dims[j] - 1) / 2;
        }
    }
    Vector3 LowerBound() const override { return {(float)(_position.x - _ext[0]), (float)(_position.y - _ext[1]), (float)(_position.z - _ext[2])}; }
    Vector3 UpperBound() const override { return {(float)(_position.x + _ext[0]), (float)(_position.y + _ext[1]), (float)(_position.z + _ext[2])}; }
    float QueryDensity(const Vector3 &) const override { throw std::logic_error("StampModifier has no host density: its samples live on the device"); }
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 9;
        d.p[0] = _position.x;
        d.p[1] = _position.y;
        d.p[2] = _position.z;
        for (int k = 0; k < 4; ++k) d.p[3 + k] = _rotation[k];
        d.p[7] = _pitch;
        d.dims[0] = _stampId;
        d.dims[1] = _mode == Replace ? 1 : 0;
        return true;
    }

private:
    double _ext[3];
};

// New (not in the reference, which queues one eroding CylinderModifier per river segment, RiverRenderer.cs:151-170): carves or builds
// along curves in one pass, the union of tapered capsules over _segments (VTMC_MOD_PATH of include/vtmc.h): 8 floats per segment,
// ax, ay, az, ra, bx, by, bz, rb.  Device-resident terrains only: this mirror holds the struct and the bounds, so QueryDensity throws.
// LowerBound / UpperBound: the AABB of all end points grown by their radii, in float.
class PathModifier : public TerrainModifier {
public:
    std::vector<float> _segments;
    explicit PathModifier(std::vector<float> segments, bool addOrErode = false) : _segments(std::move(segments))
    {
        const size_t n = _segments.size() / 8;
        if (n < 1 || n > 65536 || _segments.size() % 8) throw std::invalid_argument("PathModifier: 1..65536 segments of 8 floats each");
        AddOrErode = addOrErode;
        for (int k = 0; k < 3; ++k) _low[k] = std::numeric_limits<float>::infinity(), _up[k] = -std::numeric_limits<float>::infinity();
        for (size_t s = 0; s < n; ++s)
            for (int end = 0; end < 2; ++end) {
                const float *e = &_segments[8 * s + 4 * end];
                if (!std::isfinite(e[0]) || !std::isfinite(e[1]) || !std::isfinite(e[2]) || !std::isfinite(e[3]) || e[3] < 0 || std::fabs(e[3]) > 1048576.0f ||
                    std::fabs(e[0]) > 1048576.0f || std::fabs(e[1]) > 1048576.0f || std::fabs(e[2]) > 1048576.0f)
                    throw std::invalid_argument("PathModifier: end points and radii must be finite, at most 2^20 in magnitude, radii not negative");
                for (int k = 0; k < 3; ++k) _low[k] = std::min(_low[k], e[k] - e[3]), _up[k] = std::max(_up[k], e[k] + e[3]);
            }
    }
    Vector3 LowerBound() const override { return {_low[0], _low[1], _low[2]}; }
    Vector3 UpperBound() const override { return {_up[0], _up[1], _up[2]}; }
    float QueryDensity(const Vector3 &) const override { throw std::logic_error("PathModifier has no host density: it is evaluated on the device"); }
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 10;
        d.data = _segments.data();
        d.dims[0] = (int)(_segments.size() / 8);
        d.dims[1] = 8;
        return true;
    }

private:
    float _low[3], _up[3];
};

// New (not in the reference): removes every floating fragment of the box _lower.._upper (VTMC_MOD_DETACH of include/vtmc.h): the components of
// solid samples, joined along x, y and z inside the box, that touch no face of the box.  _maxSamples > 0 leaves larger fragments alone.
// Queued after a dig in the same Update, the dig and what falls off are one step.  Device-resident terrains only: QueryDensity throws.
class DetachModifier : public TerrainModifier {
public:
    Vector3 _lower, _upper;
    int _maxSamples;
    DetachModifier(Vector3 lower, Vector3 upper, int maxSamples = 0) : _lower(lower), _upper(upper), _maxSamples(maxSamples)
    {
        if (std::isnan(lower.x) || std::isnan(lower.y) || std::isnan(lower.z) || std::isnan(upper.x) || std::isnan(upper.y) || std::isnan(upper.z) ||
            maxSamples < 0)
            throw std::invalid_argument("DetachModifier: a bound is NaN or maxSamples is negative");
        AddOrErode = false;
    }
    Vector3 LowerBound() const override { return _lower; }
    Vector3 UpperBound() const override { return _upper; }
    float QueryDensity(const Vector3 &) const override { throw std::logic_error("DetachModifier has no host density: it is evaluated on the device"); }
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 11;
        d.dims[0] = _maxSamples;
        d.dims[1] = 0;
        return true;
    }
};

// New (not in the reference): hydraulic and thermal erosion of the heightfield of the box _lower.._upper (VTMC_MOD_EROSION of
// include/vtmc_erosion.h, where the rule is), simulated on the device for _iterations steps.  Everything but the box is in grid units:
// rain depth per unit time, evaporation, sediment capacity, dissolve and deposit in 0..1, dt in (0, 1], the talus (the largest stable
// height step between neighbouring columns) and the thermal rate in 0..0.125 (0: thermal erosion off).  The constructor refuses what the
// library refuses.  AddOrErode is ignored by the library.  Device-resident terrains only: QueryDensity throws.  The maps of the run are
// read with VoxelTerrain::ReadErosion.
class ErosionModifier : public TerrainModifier {
public:
    Vector3 _lower, _upper;
    int _iterations;
    float _rain, _evaporation, _capacity, _dissolve, _deposit, _dt, _talus, _thermalRate;
    ErosionModifier(Vector3 lower, Vector3 upper, int iterations, float rain = 0.01f, float evaporation = 0.02f, float capacity = 1.0f, float dissolve = 0.3f,
                    float deposit = 0.3f, float dt = 0.25f, float talus = 1.0f, float thermalRate = 0.0f)
        : _lower(lower), _upper(upper), _iterations(iterations), _rain(rain), _evaporation(evaporation), _capacity(capacity), _dissolve(dissolve),
          _deposit(deposit), _dt(dt), _talus(talus), _thermalRate(thermalRate)
    {
        const float p[8] = {rain, evaporation, capacity, dissolve, deposit, dt, talus, thermalRate};
        bool ok = iterations >= 1 && iterations <= 65536;
        for (float v : p) ok = ok && std::isfinite(v) && !(v < 0.0f);
        ok = ok && rain <= 256.0f && capacity <= 65536.0f && dissolve <= 1.0f && deposit <= 1.0f && dt > 0.0f && dt <= 1.0f && thermalRate <= 0.125f &&
             !(evaporation * dt > 1.0f);
        if (!ok || std::isnan(lower.x) || std::isnan(lower.y) || std::isnan(lower.z) || std::isnan(upper.x) || std::isnan(upper.y) || std::isnan(upper.z))
            throw std::invalid_argument("ErosionModifier: a parameter is not finite, negative or outside its range, or a bound is NaN");
    }
    Vector3 LowerBound() const override { return _lower; }
    Vector3 UpperBound() const override { return _upper; }
    float QueryDensity(const Vector3 &) const override { throw std::logic_error("ErosionModifier has no host density: it is simulated on the device"); }
    bool Describe(ModifierDesc &d) const override
    {
        d.kind = 12;
        const float p[8] = {_rain, _evaporation, _capacity, _dissolve, _deposit, _dt, _talus, _thermalRate};
        for (int k = 0; k < 8; k++) d.p[k] = p[k];
        d.dims[0] = _iterations;
        d.dims[1] = 0;
        return true;
    }
};

// New (not in the reference): the maps of the last ErosionModifier, as VoxelTerrain::ReadErosion returns them (include/vtmc_erosion.h): the
// clamped sample box, its _nx x _nz columns, and per column (x fastest) the height before and after in grid units, the water depth and the
// suspended sediment left after the last step, and whether the column took part; every map holds 0 on a column that did not.
struct ErosionResult {
    int _boxLo[3] = {0, 0, 0}, _boxHi[3] = {0, 0, 0};
    int _nx = 0, _nz = 0, _iterations = 0;
    int _active = 0, _rewritten = 0, _clamped = 0;
    std::vector<float> _heightBefore, _heightAfter, _water, _sediment;
    std::vector<unsigned char> _activeMask;
};

// New (not in the reference): one floating fragment of VoxelTerrain::Fragments (vtmc_fragment of include/vtmc.h): the sample of smallest
// grid index, the tight inclusive sample bounds, the solid sample count, and the id of the stamp it was captured into (0: none).
struct Fragment {
    MathHelper::Int3 _seed, _lo, _hi;
    int _samples;
    int _stampId;
};

// New (not in the reference): the navigation layer of a box of the terrain, as VoxelTerrain::BuildNav returns it (vtmc_nav_span of
// include/vtmc_nav.h, where the rule is): the spans ordered by column (ix + dx * iz of the box) and bottom-up inside a column, the
// dx * dz + 1 span offsets of the columns, and the box in grid samples.  A span's height is in grid units; a link is the index of a span
// in the column at -x, +x, -z, +z or -1; _region is the smallest span index of its component.
struct NavSpan {
    float _height;
    int _y, _clearance;
    int _link[4];
    int _region;
};
struct NavResult {
    std::vector<NavSpan> _spans;
    std::vector<int> _columnOffsets;
    MathHelper::Int3 _boxLo, _boxDims;
    std::vector<int> _origin;   // after VoxelTerrain::ErodeNav: per span its index in the result that was eroded; empty after BuildNav
};

// New (not in the reference): a flow field on the last BuildNav (include/vtmc_navfield.h, where the rule is).  A goal is a span and the
// cost of standing on it; a cell is a span's cheapest cost to the nearest goal (kNavFieldUnreached: none within the limit) and the span to
// step to next (-1: arrived, or unreached); NavPaths holds, for every start, a row of _maxLen spans padded with -1 and its length.
constexpr unsigned kNavFieldUnreached = 0xffffffffu;
struct NavGoal {
    int _span;
    unsigned _cost;
};
struct NavFieldCell {
    unsigned _cost;
    int _next;
};
struct NavPaths {
    std::vector<int> _paths, _lengths;
    int _maxLen = 0;
};
// New (not in the reference): one answer of VoxelTerrain::NavSight (include/vtmc_navsight.h, where the rule is): the span the straight walk
// from one span towards another ended on and the links it followed; the pair is visible iff _last is the span walked towards.
constexpr unsigned kNavSightAnyCost = 0xffffffffu;
struct NavSightHit {
    int _last;
    int _steps;
};
// New (not in the reference): a crowd stepped along the flow field (include/vtmc_navcrowd.h, where the rule is).  An agent stands on a
// span, one agent per span, earns _speed cost units per tick and saves them in _budget; CrowdResult is what ReadCrowd returns: the agents,
// per span the index of the agent on it or -1, and the counts of vtmc_navcrowd_info.
constexpr unsigned kNavCrowdAnyDetour = 0xffffffffu;
enum NavCrowdState : unsigned { kCrowdWalking = 0, kCrowdArrived = 1, kCrowdStranded = 2, kCrowdGone = 3, kCrowdUnplaced = 4 };
struct CrowdAgent {
    int _span;
    unsigned _budget, _speed, _state;
};
struct CrowdResult {
    std::vector<CrowdAgent> _agents;
    std::vector<int> _occupancy;
    int _occupying = 0, _arrived = 0, _ticks = 0, _movedLast = 0;
};

// New (not in the reference): standing water (include/vtmc_water.h, where the rule is).  A source pours at _position (world space; its
// nearest sample is the source's) up to _level; WaterResult is what Flood returns: per source its body or -1 (dry), the bodies in the
// rule's order (descending level, then ascending grid index of the seed), the box and the two volumes (x fastest, _volumeDims samples per
// axis): the body index of every sample or -1, and the density whose extraction is the water's surface.
constexpr unsigned kWaterAtFace = 1u;
struct WaterSource {
    Vector3 _position;
    float _level;
};
struct WaterBody {
    int _seed[3], _lo[3], _hi[3];
    float _level;
    int _samples, _surface;
    unsigned _flags;
    int _sources;
    unsigned _reserved[2];
};
struct WaterResult {
    std::vector<int> _sourceBody;
    std::vector<WaterBody> _bodies;
    int _boxLo[3] = {0, 0, 0}, _boxDims[3] = {0, 0, 0}, _volumeDims[3] = {0, 0, 0};
    long long _wet = 0;
    std::vector<float> _water;
    std::vector<int> _bodyVolume;
};
struct WaterProbe {
    int _body;      // -1: dry
    float _depth;   // level - y, 0 when dry
};

// New (not in the reference): voxel lighting (include/vtmc_light.h, where the rule is).  A torch sits at _position (world space; its nearest
// sample is the torch's) with _level 1..255; LightResult is what Light returns: per torch 1 (lit) or 0 (dark: outside the box or in
// solid), the box, the counts of lit samples per channel, the rounds of the relaxation, and the volume (x fastest, _boxDims samples per
// axis, no padding): two bytes per sample, sky and torch.
struct LightSource {
    Vector3 _position;
    int _level;
};
struct LightSample {
    unsigned char _sky, _torch;
};
struct LightResult {
    std::vector<unsigned char> _sourceLit;
    int _boxLo[3] = {0, 0, 0}, _boxDims[3] = {0, 0, 0};
    long long _skySamples = 0, _torchSamples = 0;
    int _rounds = 0;
    std::vector<LightSample> _volume;
};

// New (not in the reference, which can only replace a control map whole): one paint stroke on the material layer (vtmc_material_stroke
// of include/vtmc.h).  Every texel within _radius of _center (world space) is blended towards the one-hot of _channel (0..3: control map
// 1's r, g, b, a; 4..7: control map 2's) by _strength * clamp01(2 (1 - d / _radius)).
struct MaterialStroke {
    Vector3 _center;
    float _radius;
    int _channel;
    float _strength;
    MaterialStroke(Vector3 center, float radius, int channel, float strength = 1.0f)
        : _center(center), _radius(radius), _channel(channel), _strength(strength)
    {
        if (!std::isfinite(center.x) || !std::isfinite(center.y) || !std::isfinite(center.z) || !std::isfinite(radius) || !(radius > 0) ||
            !std::isfinite(strength) || !(strength >= 0 && strength <= 1) || channel < 0 || channel > 7)
            throw std::invalid_argument("MaterialStroke: invalid centre, radius, channel or strength");
    }
};

// New (not in the reference, which meshes every block at full resolution): one node of a level-of-detail extract (vtmc_lod_node of
// include/vtmc.h).  It covers the cells [_origin, _origin + 8 * 2^_level) per axis and is meshed as one block whose cells are 2^_level
// fine cells wide.
struct LodNode {
    MathHelper::Int3 _origin;
    int _level;
};

// What replaces a block's Unity Mesh (VoxelTerrain.cs:448-465): unindexed soup, indices 0..n-1.
struct BlockMesh {
    std::vector<Vector3> vertices;
    std::vector<Vector3> normals;
    std::vector<int> triangles;
    void Clear() { vertices.clear(); normals.clear(); triangles.clear(); }
};

// The 76-byte record of include/vtmc.h, redeclared so this header stays free of the C ABI.
struct CSTriangle {
    float _position0[3], _position1[3], _position2[3];
    float _normal0[3], _normal1[3], _normal2[3];
    int _block;
    static constexpr int stride = sizeof(float) * 3 * 6 + sizeof(int);  // VoxelTerrain.cs:36
};
static_assert(sizeof(CSTriangle) == 76, "CSTriangle must stay 76 bytes");

// The extraction seam of BatchUpdate (VoxelTerrain.cs:365-427), and the only seam there is: it serves terrains whose grid lives on the
// host.  The default implementation calls libvtmc.so; tests may install a recorder to check the host logic without a GPU.  Everything
// device-resident (vtmc_terrain_*, the material layer, level of detail, navigation, water) is not pluggable: VoxelTerrain calls the
// library itself, through the one context the default backend owns, so a terrain with a backend of the caller's cannot be resident.
struct ExtractBackend {
    virtual ~ExtractBackend() = default;
    // grid: float[(W+2),(E+2),(H+2)] z fastest; blocks: (x,y,z) triples.  Fills tris (canonical
    // order) and blockTriOffsets (B+1).  Throws UnityException on failure.
    virtual void Extract(const float *grid, int width, int elevation, int height, const std::vector<MathHelper::Int3> &blocks,
                         std::vector<CSTriangle> &tris, std::vector<int> &blockTriOffsets) = 0;
};

// The default backend and the owner of the vtmc context, defined in voxel_terrain.cpp so that this header stays free of the C ABI.
class VtmcContext;

class VoxelTerrain {
public:
    // x: width, y: elevation, z: height (VoxelTerrain.cs:39-40)
    int _width = 16, _elevation = 16, _height = 16;
    static constexpr int maxSampleResolution = 1025;  // VoxelTerrain.cs:44
    static constexpr int blockSize = 8;               // VoxelTerrain.cs:54
    static constexpr int maxTriNumPerCell = 5;        // VoxelTerrain.cs:480
    float _voxelScale = 1.0f;                         // VoxelTerrain.cs:107
    Vector3 TerrainOrigin;                            // _transform.position, VoxelTerrain.cs:101
    int _device = 0;                                  // HIP device of the vtmc context (new)
    // New: keep _voxelSamples in HBM and run Update's density write on the GPU (vtmc_terrain_*).
    // Queues holding a modifier the device cannot evaluate (Describe() == false) are refused.
    bool _deviceResident = false;
    uint64_t _seed = 1;                               // seed of the device-side void / full values
    int _matControlFineness = 8;                      // VoxelTerrain.cs:113: control maps of 16 * fineness texels per axis, clamped to 1..8

    VoxelTerrain();
    ~VoxelTerrain();

    // Fresh random numbers on every read, VoxelTerrain.cs:50-51
    float voidDensity() { return _uniform(_rng) * 1.0f - 2.0f; }  // Random.Range(-2, -1)
    float fullDensity() { return _uniform(_rng) * 1.0f + 1.0f; }  // Random.Range(1, 2)
    Vector3 TerrainSize() const { return Vector3((float)_width, (float)_elevation, (float)_height) * _voxelScale; }

    void Init();                                                        // VoxelTerrain.cs:121-179
    void Free();                                                        // VoxelTerrain.cs:214-245
    void InsertModifier(std::shared_ptr<TerrainModifier> modifier);     // VoxelTerrain.cs:251-254
    void Update();                                                      // VoxelTerrain.cs:262-325
    void BatchUpdate();                                                 // VoxelTerrain.cs:330-477
    // VoxelTerrain.cs:186-209, device-resident terrains: mapData = (16 * _matControlFineness)^3 Colors, x fastest; group 1 or 2 (the
    // reference's Triplanar8Tex material has two).  Throws the reference's two errors.  The layer is created on the first call after Init.
    void SetControlMap(const Color *mapData, size_t length, int group);
    void SetControlMap(const std::vector<Color> &mapData, int group) { SetControlMap(mapData.data(), mapData.size(), group); }
    void Paint(const std::vector<MaterialStroke> &strokes);             // new: vtmc_material_paint; creates the layer when there is none
    // new: the material weights of the last Update's triangles, 8 bytes per vertex in the order of its triangles (3 per triangle)
    const std::vector<uint8_t> &VertexMaterials();

    // New: level of detail (device-resident terrains).  Chooses an octree of nodes around `viewer` (world space) by the rule of
    // include/vtmc.h -- roots of level maxLevel, a node of 8 * 2^L cells splits when the viewer's Chebyshev distance to it, in cells, is
    // below split * its size -- and meshes every node as one block.  Returns the triangle count.  The block meshes of Update are left
    // alone: the nodes' meshes are kept beside them (LodMeshes), mesh i belonging at TerrainOrigin + LodNodes()[i]._origin * _voxelScale
    // with its vertices already scaled by 2^level * _voxelScale.  Seams between nodes of different levels are not stitched.
    int ExtractLod(const Vector3 &viewer, int maxLevel, float split = 2.0f, int maxNodes = 1 << 18);
    const std::vector<LodNode> &LodNodes() const { return _lodNodes; }      // the nodes of the last ExtractLod, in list order
    const std::vector<BlockMesh> &LodMeshes() const { return _lodMeshes; }  // one mesh per node
    // New: the seams of the last ExtractLod covered (include/vtmc_lodskirt.h, where the rule is): a strip of triangles in the plane of every
    // node face where the level changes (allFaces: every face with a node behind it), hung `depth` node cells from the node's boundary
    // curve towards the solid side, built on the device from the result ExtractLod left.  Returns the number of skirt triangles; mesh i of
    // LodSkirtMeshes belongs where LodMeshes()[i] does, scaled the same way, and is drawn beside it.  Any later extract drops the skirts.
    int LodSkirts(float depth = 1.0f, bool allFaces = false);
    const std::vector<BlockMesh> &LodSkirtMeshes() const { return _lodSkirtMeshes; }  // one mesh per node, most of them empty

    // New: what no longer hangs on anything (device-resident terrains).  Lists the fragments a DetachModifier with the same bounds and
    // maxSamples would remove now and changes nothing; captureMinSamples > 0 also captures every fragment of at least that many samples
    // as a stamp (Fragment::_stampId) for debris.  A dig: Update [erode]; Fragments with capture; spawn the debris; Update [detach].
    std::vector<Fragment> Fragments(const Vector3 &lower, const Vector3 &upper, int maxSamples = 0, int captureMinSamples = 0);

    // New: where something can walk, and which places are connected (device-resident terrains).  Builds the walkable spans, their links
    // and regions for the box and changes nothing; agentHeight and maxStep are in world units (ceil(agentHeight / _voxelScale) samples of
    // headroom, maxStep / _voxelScale grid units between neighbour columns).  The result is a snapshot: after an edit, build the edit's
    // box plus a margin again.  No agent radius in the build itself (ErodeNav below), no slope by normal, no stitching across boxes; the
    // path search is BuildNavField below.
    NavResult BuildNav(const Vector3 &lower, const Vector3 &upper, float agentHeight, float maxStep, int maxSpans = 1 << 24);

    // New: where THIS agent can walk (include/vtmc_naverode.h, where the rule is).  On the last BuildNav: NavDistance gives every span's
    // distance to the nearest border of the walkable area (a span with a missing link) in half columns, capped at twice the radius, and
    // leaves the result as it is; ErodeNav replaces it by the spans an agent of that radius can occupy (links remapped, regions labelled
    // again) and returns them with _origin, every kept span's index before the call.  LocateOnNav, BuildNavField and TracePaths then work
    // on the eroded spans.  radius is in world units, ceil(radius / _voxelScale) columns; with openBoxFaces the box's own faces are no
    // borders.  ErodeNav drops the field and the distances; the next BuildNav drops all of it; an edit drops nothing.
    std::vector<int> NavDistance(float radius, bool openBoxFaces = false);
    NavResult ErodeNav(float radius, bool openBoxFaces = false);

    // New: how to get there.  On the last BuildNav: LocateOnNav gives the span each world position stands on (the nearest span of its
    // column within `below` under and `above` over it, world units; -1: none); BuildNavField every span's cheapest cost to the nearest
    // goal and the span to step to next (a level step costs 1024; climbCost / dropCost, 0..1024, are added per grid unit of height
    // climbed / dropped; a span beyond maxCost is unreached); TracePaths the spans an agent visits from each start by following next, at
    // most maxLen of them.  One field serves any number of agents.  The next BuildNav drops the field; an edit does not.  No agent
    // radius of its own (ErodeNav first), no any-angle smoothing, no field across two boxes.
    std::vector<int> LocateOnNav(const std::vector<Vector3> &positions, float below, float above);
    std::vector<NavFieldCell> BuildNavField(const std::vector<NavGoal> &goals, float climbCost, float dropCost, unsigned maxCost = 0x7fffffffu);
    NavPaths TracePaths(const std::vector<int> &starts, int maxLen);

    // New: any-angle paths (include/vtmc_navsight.h, where the rule is).  NavSight walks, for every pair, the straight line between the
    // centres of the two spans' columns over the spans of the last BuildNav or ErodeNav, following links forwards: the pair is visible
    // iff the hit's _last is `to`; a pair with a -1 gives {-1, 0}.  SmoothPaths is TracePaths with the waypoints only: of the spans that
    // following next visits, those between which that walk succeeds.  maxLook (1..256) is how many spans ahead of a waypoint are tried;
    // maxExtraCost what a straight stretch may cost above the field's own path between its ends (kNavSightAnyCost: anything).  Waypoints
    // are column centres; the only clearance is ErodeNav's radius; greedy, not the globally shortest path.
    std::vector<NavSightHit> NavSight(const std::vector<int> &from, const std::vector<int> &to);
    NavPaths SmoothPaths(const std::vector<int> &starts, int maxLen, int maxLook = 64, unsigned maxExtraCost = kNavSightAnyCost);

    // New: a crowd on the last BuildNav (include/vtmc_navcrowd.h, where the rule is).  SpawnCrowd replaces the crowd: agent i asks for
    // spans[i] (or -1) and earns speeds[i] cost units per tick; of several that ask for one span the smallest index stands; returns the
    // number of placed agents.  StepCrowd moves everybody along the field of the last BuildNavField for `ticks` ticks, on the device: an
    // agent takes the cheapest neighbour nearer the goal that was empty when the tick began and costs at most maxDetour above the cheapest
    // way (kNavCrowdAnyDetour: any); with leaveOnArrival an agent that arrives frees its span.  BuildNavField keeps the crowd (the
    // re-route); BuildNav and ErodeNav drop it.  ReadCrowd copies the agents, the occupancy and the counts.
    int SpawnCrowd(const std::vector<int> &spans, const std::vector<unsigned> &speeds);
    void StepCrowd(int ticks, unsigned maxDetour = kNavCrowdAnyDetour, bool leaveOnArrival = false);
    CrowdResult ReadCrowd();

    // New: standing water (include/vtmc_water.h, where the rule is).  Flood fills the box lower..upper (world bounds) from the sources to
    // their levels, on the device, and returns the bodies and the volumes; it changes nothing in the terrain and keeps a snapshot that
    // Init drops and an edit keeps.  ProbeWater asks that snapshot what a swimmer asks: the body and the depth at a position.
    WaterResult Flood(Vector3 lower, Vector3 upper, const std::vector<WaterSource> &sources);
    std::vector<WaterProbe> ProbeWater(const std::vector<Vector3> &positions);

    // New: voxel lighting (include/vtmc_light.h, where the rule is).  Light floods sky light (skyLevel 0..255 from the top face of the box,
    // 0: none) and the torches' light through the open samples of the box lower..upper (world bounds), each channel losing its falloff
    // (1..255) per hop, on the device, and returns the volume; it changes nothing in the terrain and keeps a snapshot that Init drops and
    // an edit keeps.  ProbeLight asks that snapshot for the two bytes at a position: (0, 0) outside the box.
    LightResult Light(Vector3 lower, Vector3 upper, int skyLevel, int skyFalloff, int torchFalloff, const std::vector<LightSource> &sources);
    std::vector<LightSample> ProbeLight(const std::vector<Vector3> &positions);

    // New: the maps the last ErosionModifier of an Update left (include/vtmc_erosion.h): a snapshot that an edit keeps and Init drops.
    // What lets a host paint sand where _heightAfter - _heightBefore > 0, or pick Flood sources where water stands.
    ErosionResult ReadErosion();

    // -- inspection (tests, callers that consume the meshes) ----------------------------------
    const BlockMesh &Block(int x, int y, int z) const { return _blocks[((size_t)x * (_elevation / blockSize) + y) * (_height / blockSize) + z]; }
    float Sample(int x, int y, int z) const { return _voxelSamples[((size_t)x * (_elevation + 2) + y) * (_height + 2) + z]; }
    const std::vector<float> &Samples() const { return _voxelSamples; }
    std::vector<float> DeviceSamples() const;  // device-resident mode: the grid copied back (z fastest, like Samples())
    const std::vector<MathHelper::Int3> &LastUpdateBlocks() const { return _lastUpdateBlocks; }
    int LastTriangleCount() const { return _lastTriNum; }
    void SeedRandom(uint32_t seed) { _rng.seed(seed); }
    void SetBackend(std::shared_ptr<ExtractBackend> backend) { _backend = std::move(backend); }

private:
    void ApplyMeshes(const std::vector<CSTriangle> &csTriangles, const std::vector<int> &offsets);  // VoxelTerrain.cs:430-465
    // the one gate of everything device-resident: the context, or UnityException("<who> needs an initialised device-resident terrain")
    VtmcContext &RequireResident(const char *who) const;
    VtmcContext &EnsureMaterialLayer();
    bool _hasMaterialLayer = false;
    std::vector<uint8_t> _vertexMaterials;
    std::vector<LodNode> _lodNodes;
    std::vector<BlockMesh> _lodMeshes, _lodSkirtMeshes;
    std::vector<float> _voxelSamples;  // float[W+2, E+2, H+2], row-major, z fastest (VoxelTerrain.cs:145)
    std::vector<BlockMesh> _blocks;    // GameObject[,,] stand-in (VoxelTerrain.cs:61)
    std::vector<MathHelper::Int3> _nextUpdateblocks, _lastUpdateBlocks;
    std::deque<std::shared_ptr<TerrainModifier>> _modifierQueue;
    std::shared_ptr<ExtractBackend> _backend;
    std::shared_ptr<VtmcContext> _vtmc;  // _backend by its own type when it is the default one (set by Init), else null
    bool _initialised = false;
    int _lastTriNum = 0;
    std::mt19937 _rng{12345u};
    std::uniform_real_distribution<float> _uniform{0.0f, 1.0f};
};

// Default backend: the HIP library behind include/vtmc.h (a VtmcContext).
std::shared_ptr<ExtractBackend> MakeVtmcBackend(int device);

}  // namespace Render
}  // namespace PGRTerrain
#endif
