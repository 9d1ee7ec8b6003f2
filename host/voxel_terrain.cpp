// voxel_terrain.cpp -- see voxel_terrain.hpp.  Reference lines are cited per function
// (Unity-Project/Assets/Scripts/VoxelTerrain.cs unless stated otherwise).
#include "voxel_terrain.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_set>

#include "../include/vtmc_navfield.h"   // includes vtmc_nav.h, which includes vtmc.h
#include "../include/vtmc_naverode.h"
#include "../include/vtmc_navsight.h"
#include "../include/vtmc_navcrowd.h"
#include "../include/vtmc_water.h"
#include "../include/vtmc_light.h"
#include "../include/vtmc_erosion.h"
#include "../include/vtmc_lodskirt.h"

namespace PGRTerrain {

float Vector3::magnitude() const { return std::sqrt(x * x + y * y + z * z); }
Vector3 Vector3::normalized() const
{
    float m = magnitude();
    return m > 1e-5f ? *this / m : Vector3();  // Unity returns zero for tiny vectors
}
Vector3 Vector3::ProjectOnPlane(const Vector3 &v, const Vector3 &n)
{
    float d = Dot(n, n);
    if (d < 1e-12f) return v;
    return v - n * (Dot(v, n) / d);
}

namespace Render {

using MathHelper::Int3;

static float Clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }  // Mathf.Clamp

PlaneModifier::PlaneModifier(float height, Vector2 low, Vector2 up, bool addOrErode) : _height(height), _low(low), _up(up)
{
    if (low.x > up.x || low.y > up.y) throw UnityException("invalud aabb");  // TerrainModifier.cs:52 (sic)
    AddOrErode = addOrErode;
}

CylinderModifier::CylinderModifier(Vector3 start, Vector3 dir, float length, float radius, bool addOrErode)
    : _axisStart(start), _axisDir(dir.normalized()), _axisLength(length), _radius(radius)
{
    AddOrErode = addOrErode;
}

// TerrainModifier.cs:103-116
Vector3 CylinderModifier::LowerBound() const
{
    Vector3 leftProj = Vector3::ProjectOnPlane({-1, 0, 0}, _axisDir);
    Vector3 downProj = Vector3::ProjectOnPlane({0, -1, 0}, _axisDir);
    Vector3 backProj = Vector3::ProjectOnPlane({0, 0, -1}, _axisDir);
    Vector3 end = _axisStart + _axisDir * _axisLength;
    return {_axisDir.x > 0 ? (_axisStart + leftProj * _radius).x : (end + leftProj * _radius).x,
            _axisDir.y > 0 ? (_axisStart + downProj * _radius).y : (end + downProj * _radius).y,
            _axisDir.z > 0 ? (_axisStart + backProj * _radius).z : (end + backProj * _radius).z};
}

// TerrainModifier.cs:118-131
Vector3 CylinderModifier::UpperBound() const
{
    Vector3 rightProj = Vector3::ProjectOnPlane({1, 0, 0}, _axisDir);
    Vector3 upProj = Vector3::ProjectOnPlane({0, 1, 0}, _axisDir);
    Vector3 foreProj = Vector3::ProjectOnPlane({0, 0, 1}, _axisDir);
    Vector3 end = _axisStart + _axisDir * _axisLength;
    return {_axisDir.x < 0 ? (_axisStart + rightProj * _radius).x : (end + rightProj * _radius).x,
            _axisDir.y < 0 ? (_axisStart + upProj * _radius).y : (end + upProj * _radius).y,
            _axisDir.z < 0 ? (_axisStart + foreProj * _radius).z : (end + foreProj * _radius).z};
}

// TerrainModifier.cs:143-149
float CylinderModifier::QueryDensity(const Vector3 &pos) const
{
    Vector3 start2pos = pos - _axisStart;
    float projLength = Vector3::Dot(start2pos, _axisDir);
    return std::min({projLength, _axisLength - projLength,
                     _radius - std::sqrt(start2pos.sqrMagnitude() - projLength * projLength)});
}

IslandModifier::IslandModifier(std::vector<float> heightmap, int widthRes, int heightRes, float islandWidth, float islandHeight,
                               float maxElevation, bool addOrErode)
    : _islandWidth(islandWidth), _islandHeight(islandHeight), _maxElevation(maxElevation), _widthRes(widthRes), _heightRes(heightRes),
      _heightmap(std::move(heightmap))
{
    if (widthRes < 1 || heightRes < 1 || _heightmap.size() != (size_t)widthRes * heightRes) throw UnityException("heightmap size mismatch");
    AddOrErode = addOrErode;
}

// IslandModifier.cs:45-73
float IslandModifier::QueryDensity(const Vector3 &pos) const
{
    auto lerp = [](float a, float b, float t) { return a + (b - a) * Clamp(t, 0.0f, 1.0f); };  // Mathf.Lerp
    float u = Clamp(pos.x, 0.0f, _islandWidth);
    u = u / _islandWidth * (float)(_widthRes - 1);
    u = Clamp(u, 0.0f, (float)(_widthRes - 1));
    float v = Clamp(pos.z, 0.0f, _islandHeight);
    v = v / _islandHeight * (float)(_heightRes - 1);
    v = Clamp(v, 0.0f, (float)(_heightRes - 1));
    const int u0 = (int)std::floor(u), u1 = (int)std::ceil(u), v0 = (int)std::floor(v), v1 = (int)std::ceil(v);
    const float h00 = _heightmap[(size_t)u0 * _heightRes + v0], h10 = _heightmap[(size_t)u1 * _heightRes + v0];
    const float h01 = _heightmap[(size_t)u0 * _heightRes + v1], h11 = _heightmap[(size_t)u1 * _heightRes + v1];
    const float h0 = lerp(h00, h01, v - (float)v0), h1 = lerp(h10, h11, v - (float)v0);
    return lerp(h0, h1, u - (float)u0) - pos.y;
}

// ---------------------------------------------------------------------------------------------
// the vtmc context: the default backend of host grids, and what every device-resident method calls
// ---------------------------------------------------------------------------------------------
// One ABI call and its check: the name in the message is the call's own text up to its '('.
#define VTMC_CHECK(c, call) (c).Check((call), #call)

class VtmcContext : public ExtractBackend {
public:
    vtmc_ctx *ctx = nullptr;
    int dims[3] = {0, 0, 0};  // of the resident terrain, as Init made it

    // replaces the three table uploads of Init (VoxelTerrain.cs:151-156); ctx stays null on failure, which reads the global error text
    explicit VtmcContext(int device) { VTMC_CHECK(*this, vtmc_create(device, &ctx)); }
    ~VtmcContext() override { vtmc_destroy(ctx); }  // VoxelTerrain.cs:228-244

    void Check(int status, const char *call) const
    {
        if (status != VTMC_OK) throw UnityException(std::string(call, std::strcspn(call, "(")) + ": " + vtmc_last_error(ctx));
    }

    // the triangles of the result the context holds, sliced by the `lists` blocks or nodes they were extracted for
    void ReadTriangles(int32_t triNum, size_t lists, std::vector<CSTriangle> &tris, std::vector<int> &offsets)
    {
        tris.resize((size_t)triNum);
        offsets.assign(lists + 1, 0);
        VTMC_CHECK(*this, vtmc_read_triangles(ctx, reinterpret_cast<vtmc_triangle *>(tris.data()), triNum, offsets.data()));
    }

    void Extract(const float *grid, int w, int e, int h, const std::vector<Int3> &blocks, std::vector<CSTriangle> &tris,
                 std::vector<int> &offsets) override
    {
        std::vector<int32_t> list;
        list.reserve(blocks.size() * 3);
        for (const Int3 &b : blocks) list.insert(list.end(), {b._x, b._y, b._z});
        int32_t triNum = 0;
        // a C# float[W+2,E+2,H+2] is z fastest: strides ((E+2)(H+2), H+2, 1)
        VTMC_CHECK(*this, vtmc_extract_grid(ctx, grid, w, e, h, (int64_t)(e + 2) * (h + 2), h + 2, 1, list.data(), (int32_t)blocks.size(), &triNum));
        ReadTriangles(triNum, blocks.size(), tris, offsets);
    }
};

std::shared_ptr<ExtractBackend> MakeVtmcBackend(int device) { return std::make_shared<VtmcContext>(device); }

static_assert(sizeof(int) == sizeof(int32_t) && sizeof(unsigned) == sizeof(uint32_t), "spans, offsets and speeds are read in place");

// a Vector3 as the ABI's float[3]; returns what follows it, for arrays of them
static float *Put3(float *out, const Vector3 &v)
{
    out[0] = v.x, out[1] = v.y, out[2] = v.z;
    return out + 3;
}

static std::vector<float> Flatten(const std::vector<Vector3> &positions)
{
    std::vector<float> p(positions.size() * 3);
    float *q = p.data();
    for (const Vector3 &v : positions) q = Put3(q, v);
    return p;
}

// the rows TracePaths and SmoothPaths fill: maxLen spans per start, padded with -1
static NavPaths PathRows(size_t starts, int maxLen)
{
    NavPaths out;
    out._maxLen = maxLen;
    out._paths.assign(starts * (size_t)(maxLen > 0 ? maxLen : 0), -1);
    out._lengths.assign(starts, 0);
    return out;
}

// VoxelTerrain.cs:430-465: one mesh of the triangles [begin, end): vertices (scaled), normals, trivial indices
static void FillMesh(BlockMesh &mesh, const std::vector<CSTriangle> &csTriangles, int begin, int end, float scale)
{
    mesh.Clear();  // VoxelTerrain.cs:453
    for (int t = begin; t < end; t++) {
        const CSTriangle &vt = csTriangles[(size_t)t];
        for (const float *p : {vt._position0, vt._position1, vt._position2}) mesh.vertices.push_back(Vector3(p[0], p[1], p[2]) * scale);
        for (const float *n : {vt._normal0, vt._normal1, vt._normal2}) mesh.normals.push_back(Vector3(n[0], n[1], n[2]));
    }
    mesh.triangles.resize(mesh.vertices.size());
    for (size_t k = 0; k < mesh.triangles.size(); k++) mesh.triangles[k] = (int)k;  // Enumerable.Range, VoxelTerrain.cs:457
}

// ---------------------------------------------------------------------------------------------
VoxelTerrain::VoxelTerrain() = default;
VoxelTerrain::~VoxelTerrain() = default;

// VoxelTerrain.cs:121-179
void VoxelTerrain::Init()
{
    if (_width % blockSize != 0 || _elevation % blockSize != 0 || _height % blockSize != 0)
        throw UnityException("block size must align to terrain size");
    if (_width + 1 > maxSampleResolution || _elevation + 1 > maxSampleResolution || _height + 1 > maxSampleResolution)
        throw UnityException("too high resolution (exceeds " + std::to_string(maxSampleResolution) + ")");
    if (_width <= 0 || _elevation <= 0 || _height <= 0) throw UnityException("block size must align to terrain size");

    _blocks.assign((size_t)(_width / blockSize) * (_elevation / blockSize) * (_height / blockSize), BlockMesh());
    // augmented by one layer so normals on the positive boundary are defined (VoxelTerrain.cs:145)
    if (!_backend) _backend = MakeVtmcBackend(_device);  // throws when no HIP device: there is no CPU path
    _vtmc = std::dynamic_pointer_cast<VtmcContext>(_backend);  // null for a backend of the caller's (SetBackend)
    if (_deviceResident) {
        _voxelSamples.clear();  // the grid lives in HBM
        if (!_vtmc) throw UnityException("backend has no device-resident terrain");
        float origin[3];
        Put3(origin, TerrainOrigin);
        VTMC_CHECK(*_vtmc, vtmc_terrain_init(_vtmc->ctx, _width, _elevation, _height, _voxelScale, origin, _seed));
        _vtmc->dims[0] = _width, _vtmc->dims[1] = _elevation, _vtmc->dims[2] = _height;
    } else {
        _voxelSamples.resize((size_t)(_width + 2) * (_elevation + 2) * (_height + 2));
        for (float &s : _voxelSamples) s = voidDensity();
    }
    _nextUpdateblocks.clear();
    _modifierQueue.clear();
    _hasMaterialLayer = false;  // vtmc_terrain_init drops the layer
    _vertexMaterials.clear();
    _initialised = true;
}

VtmcContext &VoxelTerrain::RequireResident(const char *who) const
{
    if (!_initialised || !_deviceResident || !_vtmc) throw UnityException(std::string(who) + " needs an initialised device-resident terrain");
    return *_vtmc;
}

VtmcContext &VoxelTerrain::EnsureMaterialLayer()
{
    VtmcContext &c = RequireResident("the material layer");
    if (_hasMaterialLayer) return c;
    _matControlFineness = std::min(std::max(_matControlFineness, 1), 8);  // Mathf.Clamp, VoxelTerrain.cs:191
    VTMC_CHECK(c, vtmc_material_init(c.ctx, _matControlFineness));
    _hasMaterialLayer = true;
    return c;
}

// VoxelTerrain.cs:186-209
void VoxelTerrain::SetControlMap(const Color *mapData, size_t length, int group)
{
    if (group < 1 || group > 2) throw UnityException("invalid control map group");
    const size_t controlMapSize = (size_t)std::min(std::max(_matControlFineness, 1), 8) * 16;
    if (!mapData || length != controlMapSize * controlMapSize * controlMapSize) throw UnityException("invalid control map data size");
    VtmcContext &c = EnsureMaterialLayer();
    VTMC_CHECK(c, vtmc_material_set_control_map(c.ctx, reinterpret_cast<const float *>(mapData), group));
}

void VoxelTerrain::Paint(const std::vector<MaterialStroke> &strokes)
{
    VtmcContext &c = EnsureMaterialLayer();
    std::vector<vtmc_material_stroke> s(strokes.size());
    for (size_t i = 0; i < strokes.size(); i++) {
        Put3(s[i].center, strokes[i]._center);
        s[i].radius = strokes[i]._radius;
        s[i].strength = strokes[i]._strength;
        s[i].channel = strokes[i]._channel;
    }
    VTMC_CHECK(c, vtmc_material_paint(c.ctx, s.data(), (int32_t)s.size()));
}

// 8 bytes per vertex of the last Update's result: vertex 3 t + v of triangle t
const std::vector<uint8_t> &VoxelTerrain::VertexMaterials()
{
    VtmcContext &c = EnsureMaterialLayer();
    int64_t n = 0;
    VTMC_CHECK(c, vtmc_material_vertices(c.ctx, &n));
    _vertexMaterials.resize((size_t)n * VTMC_MATERIAL_CHANNELS);
    VTMC_CHECK(c, vtmc_material_read_vertices(c.ctx, _vertexMaterials.data(), n));
    return _vertexMaterials;
}

std::vector<Fragment> VoxelTerrain::Fragments(const Vector3 &lower, const Vector3 &upper, int maxSamples, int captureMinSamples)
{
    VtmcContext &c = RequireResident("Fragments");
    float lo[3], up[3];
    Put3(lo, lower), Put3(up, upper);
    int32_t n = 0;
    VTMC_CHECK(c, vtmc_terrain_fragments(c.ctx, lo, up, maxSamples, 0, nullptr, 0, &n));
    std::vector<vtmc_fragment> list((size_t)n);
    if (n > 0) VTMC_CHECK(c, vtmc_terrain_fragments(c.ctx, lo, up, maxSamples, captureMinSamples, list.data(), n, &n));
    std::vector<Fragment> out;
    for (const vtmc_fragment &f : list)
        out.push_back(Fragment{Int3(f.seed[0], f.seed[1], f.seed[2]), Int3(f.lo[0], f.lo[1], f.lo[2]), Int3(f.hi[0], f.hi[1], f.hi[2]), f.n_samples,
                               f.stamp_id});
    return out;
}

// the nav result the context holds
static NavResult ReadNav(VtmcContext &c)
{
    NavResult out;
    int32_t n = 0, first[3], dims[3];
    VTMC_CHECK(c, vtmc_nav_info(c.ctx, first, dims, &n));
    std::vector<vtmc_nav_span> list((size_t)n);
    out._columnOffsets.assign((size_t)dims[0] * (size_t)dims[2] + 1, 0);
    VTMC_CHECK(c, vtmc_nav_read(c.ctx, list.data(), n, out._columnOffsets.data()));
    out._boxLo = Int3(first[0], first[1], first[2]);
    out._boxDims = Int3(dims[0], dims[1], dims[2]);
    for (const vtmc_nav_span &s : list) out._spans.push_back(NavSpan{s.height, s.y, s.clearance, {s.link[0], s.link[1], s.link[2], s.link[3]}, s.region});
    return out;
}

NavResult VoxelTerrain::BuildNav(const Vector3 &lower, const Vector3 &upper, float agentHeight, float maxStep, int maxSpans)
{
    VtmcContext &c = RequireResident("BuildNav");
    const float samples = std::ceil(agentHeight / _voxelScale);
    if (!(samples >= 1.0f && samples <= (float)VTMC_NAV_MAX_AGENT_HEIGHT)) throw UnityException("BuildNav: agentHeight outside 1..256 samples");
    float lo[3], up[3];
    Put3(lo, lower), Put3(up, upper);
    const vtmc_nav_params p = {(int)samples, maxStep / _voxelScale, maxSpans, 0u};
    int32_t n = 0;
    VTMC_CHECK(c, vtmc_terrain_nav_build(c.ctx, lo, up, &p, &n));
    return ReadNav(c);
}

// radius in columns, as both calls of include/vtmc_naverode.h take it
static vtmc_naverode_params ErodeParams(float radius, float voxelScale, bool openBoxFaces, const char *who)
{
    const float columns = std::ceil(radius / voxelScale);
    if (!(columns >= 0.0f && columns <= (float)VTMC_NAVERODE_MAX_RADIUS)) throw UnityException(std::string(who) + ": radius outside 0..255 columns");
    return vtmc_naverode_params{(int)columns, openBoxFaces ? VTMC_NAVERODE_OPEN_BOX_FACES : 0u, {0, 0}};
}

std::vector<int> VoxelTerrain::NavDistance(float radius, bool openBoxFaces)
{
    VtmcContext &c = RequireResident("NavDistance");
    const vtmc_naverode_params p = ErodeParams(radius, _voxelScale, openBoxFaces, "NavDistance");
    int32_t n = 0;
    VTMC_CHECK(c, vtmc_nav_distance_build(c.ctx, &p, nullptr));
    VTMC_CHECK(c, vtmc_nav_distance_device_results(c.ctx, nullptr, &n));
    std::vector<int> out((size_t)n, 0);
    VTMC_CHECK(c, vtmc_nav_distance_read(c.ctx, out.data(), n));
    return out;
}

NavResult VoxelTerrain::ErodeNav(float radius, bool openBoxFaces)
{
    VtmcContext &c = RequireResident("ErodeNav");
    const vtmc_naverode_params p = ErodeParams(radius, _voxelScale, openBoxFaces, "ErodeNav");
    int32_t n = 0;
    VTMC_CHECK(c, vtmc_nav_erode(c.ctx, &p, &n));
    NavResult out = ReadNav(c);
    out._origin.assign((size_t)n, 0);
    VTMC_CHECK(c, vtmc_nav_erode_origin(c.ctx, out._origin.data(), n));
    return out;
}

std::vector<int> VoxelTerrain::LocateOnNav(const std::vector<Vector3> &positions, float below, float above)
{
    VtmcContext &c = RequireResident("LocateOnNav");
    std::vector<int> out(positions.size(), -1);
    VTMC_CHECK(c, vtmc_nav_locate(c.ctx, Flatten(positions).data(), (int32_t)positions.size(), below / _voxelScale, above / _voxelScale, out.data()));
    return out;
}

std::vector<NavFieldCell> VoxelTerrain::BuildNavField(const std::vector<NavGoal> &goals, float climbCost, float dropCost, unsigned maxCost)
{
    VtmcContext &c = RequireResident("BuildNavField");
    std::vector<vtmc_navfield_goal> g;
    for (const NavGoal &goal : goals) g.push_back(vtmc_navfield_goal{goal._span, goal._cost});
    const vtmc_navfield_params p = {climbCost, dropCost, maxCost, 0u};
    int32_t n = 0;
    VTMC_CHECK(c, vtmc_navfield_build(c.ctx, g.data(), (int32_t)g.size(), &p, nullptr));
    VTMC_CHECK(c, vtmc_navfield_info(c.ctx, &n, nullptr, nullptr));
    std::vector<vtmc_navfield_cell> cells((size_t)n);
    VTMC_CHECK(c, vtmc_navfield_read(c.ctx, cells.data(), n));
    std::vector<NavFieldCell> out;
    for (const vtmc_navfield_cell &cell : cells) out.push_back(NavFieldCell{cell.cost, cell.next});
    return out;
}

NavPaths VoxelTerrain::TracePaths(const std::vector<int> &starts, int maxLen)
{
    VtmcContext &c = RequireResident("TracePaths");
    NavPaths out = PathRows(starts.size(), maxLen);
    VTMC_CHECK(c, vtmc_navfield_trace(c.ctx, starts.data(), (int32_t)starts.size(), maxLen, out._paths.data(), out._lengths.data()));
    return out;
}

std::vector<NavSightHit> VoxelTerrain::NavSight(const std::vector<int> &from, const std::vector<int> &to)
{
    VtmcContext &c = RequireResident("NavSight");
    if (from.size() != to.size()) throw UnityException("NavSight: as many from as to spans");
    std::vector<vtmc_navsight_hit> hits(from.size());
    VTMC_CHECK(c, vtmc_nav_sight(c.ctx, from.data(), to.data(), (int32_t)from.size(), hits.data()));
    std::vector<NavSightHit> out;
    for (const vtmc_navsight_hit &h : hits) out.push_back(NavSightHit{h.last, h.steps});
    return out;
}

NavPaths VoxelTerrain::SmoothPaths(const std::vector<int> &starts, int maxLen, int maxLook, unsigned maxExtraCost)
{
    VtmcContext &c = RequireResident("SmoothPaths");
    NavPaths out = PathRows(starts.size(), maxLen);
    const vtmc_navsight_params p = {maxLook, maxExtraCost, 0u, 0u};
    VTMC_CHECK(c, vtmc_navfield_trace_smooth(c.ctx, starts.data(), (int32_t)starts.size(), maxLen, &p, out._paths.data(), out._lengths.data()));
    return out;
}

int VoxelTerrain::SpawnCrowd(const std::vector<int> &spans, const std::vector<unsigned> &speeds)
{
    VtmcContext &c = RequireResident("SpawnCrowd");
    if (spans.size() != speeds.size()) throw UnityException("SpawnCrowd: as many speeds as spans");
    int32_t placed = 0;
    VTMC_CHECK(c, vtmc_navcrowd_spawn(c.ctx, spans.data(), speeds.data(), (int32_t)spans.size(), &placed));
    return placed;
}

void VoxelTerrain::StepCrowd(int ticks, unsigned maxDetour, bool leaveOnArrival)
{
    VtmcContext &c = RequireResident("StepCrowd");
    const vtmc_navcrowd_params p = {maxDetour, leaveOnArrival ? VTMC_NAVCROWD_LEAVE_ON_ARRIVAL : 0u, {0u, 0u}};
    VTMC_CHECK(c, vtmc_navcrowd_step(c.ctx, &p, ticks));
}

CrowdResult VoxelTerrain::ReadCrowd()
{
    VtmcContext &c = RequireResident("ReadCrowd");
    CrowdResult out;
    int32_t n = 0, nSpans = 0;
    VTMC_CHECK(c, vtmc_navcrowd_info(c.ctx, &n, &out._occupying, &out._arrived, &out._ticks, &out._movedLast));
    VTMC_CHECK(c, vtmc_nav_info(c.ctx, nullptr, nullptr, &nSpans));
    std::vector<vtmc_navcrowd_agent> agents((size_t)n);
    out._occupancy.assign((size_t)nSpans, -1);
    VTMC_CHECK(c, vtmc_navcrowd_read(c.ctx, agents.data(), n, out._occupancy.data()));
    for (const vtmc_navcrowd_agent &a : agents) out._agents.push_back(CrowdAgent{a.span, a.budget, a.speed, a.state});
    return out;
}

WaterResult VoxelTerrain::Flood(Vector3 lower, Vector3 upper, const std::vector<WaterSource> &sources)
{
    VtmcContext &c = RequireResident("Flood");
    static_assert(sizeof(WaterBody) == sizeof(vtmc_water_body), "copied as they lie");
    float lo[3], up[3];
    Put3(lo, lower), Put3(up, upper);
    std::vector<vtmc_water_source> src(sources.size());
    for (size_t i = 0; i < sources.size(); i++) {
        Put3(src[i].position, sources[i]._position);
        src[i].level = sources[i]._level;
    }
    WaterResult out;
    out._sourceBody.assign(sources.size(), -1);
    int32_t n = 0;
    VTMC_CHECK(c, vtmc_terrain_flood(c.ctx, lo, up, src.data(), (int32_t)src.size(), 0u, out._sourceBody.data(), &n));
    int64_t wet = 0;
    VTMC_CHECK(c, vtmc_water_info(c.ctx, out._boxLo, out._boxDims, out._volumeDims, &n, &wet));
    out._wet = wet;
    out._bodies.resize((size_t)n);
    VTMC_CHECK(c, vtmc_water_bodies(c.ctx, reinterpret_cast<vtmc_water_body *>(out._bodies.data()), n));
    const size_t vn = (size_t)out._volumeDims[0] * out._volumeDims[1] * out._volumeDims[2];
    out._water.resize(vn), out._bodyVolume.resize(vn);
    VTMC_CHECK(c, vtmc_water_read(c.ctx, out._water.data(), out._bodyVolume.data(), (int64_t)vn));
    return out;
}

std::vector<WaterProbe> VoxelTerrain::ProbeWater(const std::vector<Vector3> &positions)
{
    VtmcContext &c = RequireResident("ProbeWater");
    std::vector<int32_t> body(positions.size(), -1);
    std::vector<float> depth(positions.size(), 0.0f);
    VTMC_CHECK(c, vtmc_water_probe(c.ctx, Flatten(positions).data(), (int32_t)positions.size(), body.data(), depth.data()));
    std::vector<WaterProbe> out;
    for (size_t i = 0; i < positions.size(); i++) out.push_back(WaterProbe{body[i], depth[i]});
    return out;
}

LightResult VoxelTerrain::Light(Vector3 lower, Vector3 upper, int skyLevel, int skyFalloff, int torchFalloff, const std::vector<LightSource> &sources)
{
    VtmcContext &c = RequireResident("Light");
    static_assert(sizeof(LightSample) == sizeof(vtmc_light_sample), "copied as they lie");
    float lo[3], up[3];
    Put3(lo, lower), Put3(up, upper);
    std::vector<vtmc_light_source> src(sources.size());
    for (size_t i = 0; i < sources.size(); i++) {
        Put3(src[i].position, sources[i]._position);
        src[i].level = sources[i]._level;
    }
    const vtmc_light_params p = {skyLevel, skyFalloff, torchFalloff, 0u};
    LightResult out;
    out._sourceLit.assign(sources.size(), 0);
    VTMC_CHECK(c, vtmc_terrain_light(c.ctx, lo, up, &p, src.data(), (int32_t)src.size(), out._sourceLit.data()));
    int64_t nSky = 0, nTorch = 0;
    int32_t rounds = 0;
    VTMC_CHECK(c, vtmc_light_info(c.ctx, out._boxLo, out._boxDims, &nSky, &nTorch, &rounds));
    out._skySamples = nSky, out._torchSamples = nTorch, out._rounds = rounds;
    const size_t n = (size_t)out._boxDims[0] * out._boxDims[1] * out._boxDims[2];
    out._volume.resize(n);
    VTMC_CHECK(c, vtmc_light_read(c.ctx, reinterpret_cast<vtmc_light_sample *>(out._volume.data()), (int64_t)n));
    return out;
}

std::vector<LightSample> VoxelTerrain::ProbeLight(const std::vector<Vector3> &positions)
{
    VtmcContext &c = RequireResident("ProbeLight");
    std::vector<uint8_t> sky(positions.size(), 0), torch(positions.size(), 0);
    VTMC_CHECK(c, vtmc_light_probe(c.ctx, Flatten(positions).data(), (int32_t)positions.size(), sky.data(), torch.data()));
    std::vector<LightSample> out;
    for (size_t i = 0; i < positions.size(); i++) out.push_back(LightSample{sky[i], torch[i]});
    return out;
}

ErosionResult VoxelTerrain::ReadErosion()
{
    VtmcContext &c = RequireResident("ReadErosion");
    vtmc_erosion_report r;
    VTMC_CHECK(c, vtmc_erosion_info(c.ctx, &r));
    ErosionResult out;
    for (int k = 0; k < 3; k++) out._boxLo[k] = r.lo[k], out._boxHi[k] = r.hi[k];
    out._nx = r.nx, out._nz = r.nz, out._iterations = r.iterations;
    out._active = r.n_active, out._rewritten = r.n_rewritten, out._clamped = r.n_clamped;
    const size_t n = (size_t)r.nx * (size_t)r.nz;
    std::vector<float> *planes[4] = {&out._heightBefore, &out._heightAfter, &out._water, &out._sediment};
    const int32_t maps[4] = {VTMC_EROSION_HEIGHT_BEFORE, VTMC_EROSION_HEIGHT_AFTER, VTMC_EROSION_WATER, VTMC_EROSION_SEDIMENT};
    for (int k = 0; k < 4; k++) {
        planes[k]->resize(n);
        VTMC_CHECK(c, vtmc_erosion_read(c.ctx, maps[k], planes[k]->data(), (int64_t)(n * sizeof(float))));
    }
    out._activeMask.resize(n);
    VTMC_CHECK(c, vtmc_erosion_read(c.ctx, VTMC_EROSION_ACTIVE, out._activeMask.data(), (int64_t)n));
    return out;
}

int VoxelTerrain::ExtractLod(const Vector3 &viewer, int maxLevel, float split, int maxNodes)
{
    VtmcContext &c = RequireResident("ExtractLod");
    vtmc_lod_params p;
    Put3(p.viewer, viewer);
    p.split = split, p.max_level = maxLevel, p.max_nodes = maxNodes;
    int32_t nNodes = 0, triNum = 0;
    VTMC_CHECK(c, vtmc_terrain_extract_lod(c.ctx, &p, &nNodes, &triNum));
    std::vector<vtmc_lod_node> list((size_t)nNodes);
    VTMC_CHECK(c, vtmc_terrain_lod_nodes(c.ctx, list.data(), nNodes, nullptr));
    _lodNodes.clear();
    for (const vtmc_lod_node &nd : list) _lodNodes.push_back(LodNode{Int3(nd.origin[0], nd.origin[1], nd.origin[2]), nd.level});
    std::vector<CSTriangle> csTriangles;  // canonical order, _block = the node's index
    std::vector<int> offsets;
    c.ReadTriangles(triNum, _lodNodes.size(), csTriangles, offsets);
    _lodMeshes.assign(_lodNodes.size(), BlockMesh());
    for (size_t i = 0; i < _lodNodes.size(); i++)  // a node's cell in world units is 2^level * _voxelScale
        FillMesh(_lodMeshes[i], csTriangles, offsets[i], offsets[i + 1], (float)(1 << _lodNodes[i]._level) * _voxelScale);
    _lodSkirtMeshes.clear();  // they belonged to the result this one replaced
    return (int)csTriangles.size();
}

int VoxelTerrain::LodSkirts(float depth, bool allFaces)
{
    VtmcContext &c = RequireResident("LodSkirts");
    const vtmc_lodskirt_params p = {depth, allFaces ? VTMC_LODSKIRT_ALL_FACES : 0u};
    int64_t n = 0;
    VTMC_CHECK(c, vtmc_lod_skirts(c.ctx, &p, &n));
    int32_t nNodes = 0;
    VTMC_CHECK(c, vtmc_lodskirt_info(c.ctx, &nNodes, nullptr, nullptr));
    std::vector<CSTriangle> csTriangles((size_t)n);
    std::vector<int> offsets((size_t)nNodes + 1, 0);
    VTMC_CHECK(c, vtmc_lodskirt_read(c.ctx, reinterpret_cast<vtmc_triangle *>(csTriangles.data()), n, offsets.data()));
    _lodSkirtMeshes.assign((size_t)nNodes, BlockMesh());
    for (size_t i = 0; i < _lodSkirtMeshes.size() && i < _lodNodes.size(); i++)
        FillMesh(_lodSkirtMeshes[i], csTriangles, offsets[i], offsets[i + 1], (float)(1 << _lodNodes[i]._level) * _voxelScale);
    return (int)n;
}

// VoxelTerrain.cs:214-245
void VoxelTerrain::Free()
{
    for (BlockMesh &b : _blocks) b.Clear();
    _blocks.clear();
    _lodNodes.clear();
    _lodMeshes.clear();
    _lodSkirtMeshes.clear();
    _backend.reset();
    _vtmc.reset();
    _initialised = false;
}

// VoxelTerrain.cs:251-254
void VoxelTerrain::InsertModifier(std::shared_ptr<TerrainModifier> modifier) { _modifierQueue.push_back(std::move(modifier)); }

// VoxelTerrain.cs:262-325
void VoxelTerrain::Update()
{
    if (!_initialised) throw UnityException("VoxelTerrain.Update before Init");
    if (_deviceResident) {
        // the whole of Update on the device: density writes, dirty set, BatchUpdate (VoxelTerrain.cs:262-325)
        VtmcContext &c = RequireResident("Update");
        std::vector<vtmc_modifier> mods;
        std::vector<std::shared_ptr<TerrainModifier>> alive;  // descriptors borrow from the modifiers (heightmap) until the call returns
        while (!_modifierQueue.empty()) {
            std::shared_ptr<TerrainModifier> modifier = _modifierQueue.front();
            _modifierQueue.pop_front();
            ModifierDesc desc;
            if (!modifier->Describe(desc)) throw UnityException("modifier cannot be evaluated on the device (Describe() returned false)");
            vtmc_modifier m;
            m.kind = desc.kind;
            m.add_or_erode = modifier->AddOrErode ? 1 : 0;
            Put3(m.lower, modifier->LowerBound());  // evaluated on the host, as VoxelTerrain.cs:273-279 does
            Put3(m.upper, modifier->UpperBound());
            std::memcpy(m.p, desc.p, sizeof m.p);
            m.data = desc.data;
            m.data_dims[0] = desc.dims[0], m.data_dims[1] = desc.dims[1];
            mods.push_back(m);
            alive.push_back(std::move(modifier));
        }
        _lastUpdateBlocks.clear();
        _lastTriNum = 0;
        if (mods.empty()) return;
        // applies the queue in order and extracts the dirty set: its blocks ordered by block id, its triangles sliced by block
        int32_t nDirty = 0, triNum = 0;
        VTMC_CHECK(c, vtmc_terrain_update(c.ctx, mods.data(), (int32_t)mods.size(), &nDirty, &triNum));
        std::vector<int32_t> list((size_t)nDirty * 3);
        VTMC_CHECK(c, vtmc_terrain_dirty_blocks(c.ctx, list.data(), nDirty, nullptr));
        _nextUpdateblocks.clear();
        for (int32_t i = 0; i < nDirty; i++) _nextUpdateblocks.emplace_back(list[3 * (size_t)i], list[3 * (size_t)i + 1], list[3 * (size_t)i + 2]);
        std::vector<CSTriangle> csTriangles;
        std::vector<int> offsets;
        if (nDirty > 0) c.ReadTriangles(triNum, (size_t)nDirty, csTriangles, offsets);
        _lastUpdateBlocks = _nextUpdateblocks;
        _lastTriNum = (int)csTriangles.size();
        if (!csTriangles.empty()) ApplyMeshes(csTriangles, offsets);
        _nextUpdateblocks.clear();
        return;
    }
    struct Hash {
        size_t operator()(const Int3 &k) const { return (size_t)(unsigned)k.GetHashCode(); }
    };
    std::unordered_set<Int3, Hash> updateBlocks;
    std::vector<Int3> ordered;  // HashSet order is arbitrary in the reference; first-insertion order here
    const int ez = _height + 2, ey = _elevation + 2;
    while (!_modifierQueue.empty()) {
        std::shared_ptr<TerrainModifier> modifier = _modifierQueue.front();
        _modifierQueue.pop_front();

        Vector3 worldLow = (modifier->LowerBound() - TerrainOrigin) / _voxelScale;
        auto floorToInt = [](float v) { return v <= -2147483648.0f ? std::numeric_limits<int>::min() : (int)std::floor(v); };
        auto ceilToInt = [](float v) { return v >= 2147483648.0f ? std::numeric_limits<int>::max() : (int)std::ceil(v); };
        Int3 low(floorToInt(worldLow.x), floorToInt(worldLow.y), floorToInt(worldLow.z));
        low._x = std::max(low._x, 0);
        low._y = std::max(low._y, 0);
        low._z = std::max(low._z, 0);
        Vector3 worldUp = (modifier->UpperBound() - TerrainOrigin) / _voxelScale;
        Int3 up(ceilToInt(worldUp.x), ceilToInt(worldUp.y), ceilToInt(worldUp.z));
        up._x = std::min(up._x, _width + 1);
        up._y = std::min(up._y, _elevation + 1);
        up._z = std::min(up._z, _height + 1);

        // resample density function (VoxelTerrain.cs:284-305)
        for (int x = low._x; x <= up._x; x++)
            for (int y = low._y; y <= up._y; y++)
                for (int z = low._z; z <= up._z; z++) {
                    Vector3 worldPos = Vector3((float)x, (float)y, (float)z) * _voxelScale + TerrainOrigin;
                    float &s = _voxelSamples[((size_t)x * ey + y) * ez + z];
                    if (modifier->AddOrErode) {
                        float md = Clamp(modifier->QueryDensity(worldPos), voidDensity(), fullDensity());
                        s = std::max(s, md);
                    } else {
                        float minus_md = -Clamp(modifier->QueryDensity(worldPos), voidDensity(), fullDensity());
                        s = Clamp(std::min(s, minus_md), voidDensity(), fullDensity());
                    }
                }

        // dirty blocks: inclusive on both ends (VoxelTerrain.cs:307-317)
        for (int x = 0; x < _width / blockSize; x++)
            for (int y = 0; y < _elevation / blockSize; y++)
                for (int z = 0; z < _height / blockSize; z++)
                    if ((up._x >= x * blockSize && low._x <= x * blockSize + blockSize) &&
                        (up._y >= y * blockSize && low._y <= y * blockSize + blockSize) &&
                        (up._z >= z * blockSize && low._z <= z * blockSize + blockSize)) {
                        Int3 key(x, y, z);
                        if (updateBlocks.insert(key).second) ordered.push_back(key);
                    }
    }
    _nextUpdateblocks = ordered;
    _lastUpdateBlocks = ordered;
    if (!_nextUpdateblocks.empty()) BatchUpdate();
    _nextUpdateblocks.clear();
}

// VoxelTerrain.cs:330-477.  Steps 1-8 of the reference (tile gather, upload, three dispatches, two
// read-backs) collapse into one Extract call; binning by _block (VoxelTerrain.cs:437-446) becomes
// slicing because the library returns triangles grouped by block in list order.
void VoxelTerrain::BatchUpdate()
{
    if (_nextUpdateblocks.empty()) return;
    std::vector<CSTriangle> csTriangles;
    std::vector<int> offsets;
    _backend->Extract(_voxelSamples.data(), _width, _elevation, _height, _nextUpdateblocks, csTriangles, offsets);
    _lastTriNum = (int)csTriangles.size();
    if (csTriangles.empty()) return;  // "no triangles, early exit" keeps the old meshes (VoxelTerrain.cs:396-405)
    ApplyMeshes(csTriangles, offsets);
}

// the grid copied back into the C# float[W+2,E+2,H+2] layout: z fastest
std::vector<float> VoxelTerrain::DeviceSamples() const
{
    VtmcContext &c = RequireResident("DeviceSamples");
    const int64_t ey = c.dims[1] + 2, ez = c.dims[2] + 2;
    std::vector<float> out((size_t)(c.dims[0] + 2) * ey * ez);
    VTMC_CHECK(c, vtmc_terrain_read_samples(c.ctx, out.data(), ey * ez, ez, 1));
    return out;
}

// VoxelTerrain.cs:430-465: the meshes of the dirty blocks, vertices scaled by _voxelScale
void VoxelTerrain::ApplyMeshes(const std::vector<CSTriangle> &csTriangles, const std::vector<int> &offsets)
{
    const int nby = _elevation / blockSize, nbz = _height / blockSize;
    for (size_t i = 0; i < _nextUpdateblocks.size(); i++) {
        const Int3 &b = _nextUpdateblocks[i];
        FillMesh(_blocks[((size_t)b._x * nby + b._y) * nbz + b._z], csTriangles, offsets[i], offsets[i + 1], _voxelScale);
    }
}

}  // namespace Render
}  // namespace PGRTerrain

