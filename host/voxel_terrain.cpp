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
// default backend: libvtmc.so
// ---------------------------------------------------------------------------------------------
namespace {
class VtmcBackend : public ExtractBackend {
public:
    explicit VtmcBackend(int device)
    {
        // replaces the three table uploads of Init (VoxelTerrain.cs:151-156)
        if (vtmc_create(device, &_ctx) != VTMC_OK) throw UnityException(std::string("vtmc_create: ") + vtmc_last_error(nullptr));
    }
    ~VtmcBackend() override { vtmc_destroy(_ctx); }  // VoxelTerrain.cs:228-244
    void Extract(const float *grid, int w, int e, int h, const std::vector<Int3> &blocks, std::vector<CSTriangle> &tris,
                 std::vector<int> &offsets) override
    {
        std::vector<int32_t> list;
        list.reserve(blocks.size() * 3);
        for (const Int3 &b : blocks) {
            list.push_back(b._x);
            list.push_back(b._y);
            list.push_back(b._z);
        }
        int32_t triNum = 0;
        // a C# float[W+2,E+2,H+2] is z fastest: strides ((E+2)(H+2), H+2, 1)
        int rc = vtmc_extract_grid(_ctx, grid, w, e, h, (int64_t)(e + 2) * (h + 2), h + 2, 1, list.data(), (int32_t)blocks.size(), &triNum);
        if (rc != VTMC_OK) throw UnityException(std::string("vtmc_extract_grid: ") + vtmc_last_error(_ctx));
        tris.resize((size_t)triNum);
        offsets.assign(blocks.size() + 1, 0);
        rc = vtmc_read_triangles(_ctx, reinterpret_cast<vtmc_triangle *>(tris.data()), triNum, offsets.data());
        if (rc != VTMC_OK) throw UnityException(std::string("vtmc_read_triangles: ") + vtmc_last_error(_ctx));
    }

    bool TerrainInit(int w, int e, int h, float scale, const Vector3 &origin, uint64_t seed) override
    {
        const float o[3] = {origin.x, origin.y, origin.z};
        if (vtmc_terrain_init(_ctx, w, e, h, scale, o, seed) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_init: ") + vtmc_last_error(_ctx));
        _dims[0] = w;
        _dims[1] = e;
        _dims[2] = h;
        return true;
    }
    void TerrainUpdate(const std::vector<QueuedModifier> &queue, std::vector<Int3> &blocks, std::vector<CSTriangle> &tris,
                       std::vector<int> &offsets) override
    {
        std::vector<vtmc_modifier> mods(queue.size());
        for (size_t i = 0; i < queue.size(); i++) {
            vtmc_modifier &m = mods[i];
            m.kind = queue[i].desc.kind;
            m.add_or_erode = queue[i].addOrErode ? 1 : 0;
            const Vector3 &lo = queue[i].lower, &up = queue[i].upper;
            m.lower[0] = lo.x, m.lower[1] = lo.y, m.lower[2] = lo.z;
            m.upper[0] = up.x, m.upper[1] = up.y, m.upper[2] = up.z;
            std::memcpy(m.p, queue[i].desc.p, sizeof m.p);
            m.data = queue[i].desc.data;
            m.data_dims[0] = queue[i].desc.dims[0];
            m.data_dims[1] = queue[i].desc.dims[1];
        }
        int32_t nDirty = 0, triNum = 0;
        if (vtmc_terrain_update(_ctx, mods.data(), (int32_t)mods.size(), &nDirty, &triNum) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_update: ") + vtmc_last_error(_ctx));
        std::vector<int32_t> list((size_t)nDirty * 3);
        if (vtmc_terrain_dirty_blocks(_ctx, list.data(), nDirty, nullptr) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_dirty_blocks: ") + vtmc_last_error(_ctx));
        blocks.clear();
        for (int32_t i = 0; i < nDirty; i++) blocks.emplace_back(list[3 * (size_t)i], list[3 * (size_t)i + 1], list[3 * (size_t)i + 2]);
        tris.resize((size_t)triNum);
        offsets.assign((size_t)nDirty + 1, 0);
        if (nDirty > 0 && vtmc_read_triangles(_ctx, reinterpret_cast<vtmc_triangle *>(tris.data()), triNum, offsets.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_read_triangles: ") + vtmc_last_error(_ctx));
    }
    void TerrainReadSamples(std::vector<float> &out) override
    {
        const int64_t ey = _dims[1] + 2, ez = _dims[2] + 2;
        out.resize((size_t)(_dims[0] + 2) * ey * ez);
        // into the C# float[W+2,E+2,H+2] layout: z fastest
        if (vtmc_terrain_read_samples(_ctx, out.data(), ey * ez, ez, 1) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_read_samples: ") + vtmc_last_error(_ctx));
    }

    void TerrainFragments(const Vector3 &lower, const Vector3 &upper, int maxSamples, int captureMinSamples, std::vector<Fragment> &out) override
    {
        const float lo[3] = {lower.x, lower.y, lower.z}, up[3] = {upper.x, upper.y, upper.z};
        int32_t n = 0;
        if (vtmc_terrain_fragments(_ctx, lo, up, maxSamples, 0, nullptr, 0, &n) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_fragments: ") + vtmc_last_error(_ctx));
        std::vector<vtmc_fragment> list((size_t)n);
        if (n > 0 && vtmc_terrain_fragments(_ctx, lo, up, maxSamples, captureMinSamples, list.data(), n, &n) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_fragments: ") + vtmc_last_error(_ctx));
        out.clear();
        for (const vtmc_fragment &f : list)
            out.push_back(Fragment{Int3(f.seed[0], f.seed[1], f.seed[2]), Int3(f.lo[0], f.lo[1], f.lo[2]), Int3(f.hi[0], f.hi[1], f.hi[2]), f.n_samples,
                                   f.stamp_id});
    }

    void TerrainNav(const Vector3 &lower, const Vector3 &upper, int agentHeight, float maxStep, int maxSpans, NavResult &out) override
    {
        const float lo[3] = {lower.x, lower.y, lower.z}, up[3] = {upper.x, upper.y, upper.z};
        vtmc_nav_params p;
        p.agent_height = agentHeight, p.max_step = maxStep, p.max_spans = maxSpans, p.flags = 0;
        int32_t n = 0;
        if (vtmc_terrain_nav_build(_ctx, lo, up, &p, &n) != VTMC_OK) throw UnityException(std::string("vtmc_terrain_nav_build: ") + vtmc_last_error(_ctx));
        ReadNav(out);
        out._origin.clear();
    }

    // the nav result the context holds
    void ReadNav(NavResult &out)
    {
        int32_t n = 0, first[3], dims[3];
        if (vtmc_nav_info(_ctx, first, dims, &n) != VTMC_OK) throw UnityException(std::string("vtmc_nav_info: ") + vtmc_last_error(_ctx));
        std::vector<vtmc_nav_span> list((size_t)n);
        out._columnOffsets.assign((size_t)dims[0] * (size_t)dims[2] + 1, 0);
        static_assert(sizeof(int) == sizeof(int32_t), "column offsets are read in place");
        if (vtmc_nav_read(_ctx, list.data(), n, out._columnOffsets.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_nav_read: ") + vtmc_last_error(_ctx));
        out._boxLo = Int3(first[0], first[1], first[2]);
        out._boxDims = Int3(dims[0], dims[1], dims[2]);
        out._spans.clear();
        for (const vtmc_nav_span &s : list) out._spans.push_back(NavSpan{s.height, s.y, s.clearance, {s.link[0], s.link[1], s.link[2], s.link[3]}, s.region});
    }

    static vtmc_naverode_params ErodeParams(int radius, bool openBoxFaces)
    {
        vtmc_naverode_params p;
        p.radius = radius, p.flags = openBoxFaces ? VTMC_NAVERODE_OPEN_BOX_FACES : 0u, p.reserved[0] = p.reserved[1] = 0;
        return p;
    }

    void NavDistance(int radius, bool openBoxFaces, std::vector<int> &out) override
    {
        const vtmc_naverode_params p = ErodeParams(radius, openBoxFaces);
        int32_t n = 0;
        if (vtmc_nav_distance_build(_ctx, &p, nullptr) != VTMC_OK || vtmc_nav_distance_device_results(_ctx, nullptr, &n) != VTMC_OK)
            throw UnityException(std::string("vtmc_nav_distance_build: ") + vtmc_last_error(_ctx));
        out.assign((size_t)n, 0);
        if (vtmc_nav_distance_read(_ctx, out.data(), n) != VTMC_OK) throw UnityException(std::string("vtmc_nav_distance_read: ") + vtmc_last_error(_ctx));
    }

    void NavErode(int radius, bool openBoxFaces, NavResult &out) override
    {
        const vtmc_naverode_params p = ErodeParams(radius, openBoxFaces);
        int32_t n = 0;
        if (vtmc_nav_erode(_ctx, &p, &n) != VTMC_OK) throw UnityException(std::string("vtmc_nav_erode: ") + vtmc_last_error(_ctx));
        ReadNav(out);
        out._origin.assign((size_t)n, 0);
        if (vtmc_nav_erode_origin(_ctx, out._origin.data(), n) != VTMC_OK) throw UnityException(std::string("vtmc_nav_erode_origin: ") + vtmc_last_error(_ctx));
    }

    void NavLocate(const std::vector<Vector3> &positions, float below, float above, std::vector<int> &out) override
    {
        std::vector<float> p;
        for (const Vector3 &v : positions) p.insert(p.end(), {v.x, v.y, v.z});
        out.assign(positions.size(), -1);
        static_assert(sizeof(int) == sizeof(int32_t), "spans are read in place");
        if (vtmc_nav_locate(_ctx, p.data(), (int32_t)positions.size(), below, above, out.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_nav_locate: ") + vtmc_last_error(_ctx));
    }
    void NavField(const std::vector<NavGoal> &goals, float climbCost, float dropCost, unsigned maxCost, std::vector<NavFieldCell> &out) override
    {
        std::vector<vtmc_navfield_goal> g;
        for (const NavGoal &goal : goals) g.push_back(vtmc_navfield_goal{goal._span, goal._cost});
        vtmc_navfield_params p;
        p.climb_cost = climbCost, p.drop_cost = dropCost, p.max_cost = maxCost, p.flags = 0;
        int32_t n = 0;
        if (vtmc_navfield_build(_ctx, g.data(), (int32_t)g.size(), &p, nullptr) != VTMC_OK || vtmc_navfield_info(_ctx, &n, nullptr, nullptr) != VTMC_OK)
            throw UnityException(std::string("vtmc_navfield_build: ") + vtmc_last_error(_ctx));
        std::vector<vtmc_navfield_cell> cells((size_t)n);
        if (vtmc_navfield_read(_ctx, cells.data(), n) != VTMC_OK) throw UnityException(std::string("vtmc_navfield_read: ") + vtmc_last_error(_ctx));
        out.clear();
        for (const vtmc_navfield_cell &c : cells) out.push_back(NavFieldCell{c.cost, c.next});
    }
    void NavTrace(const std::vector<int> &starts, int maxLen, NavPaths &out) override
    {
        out._maxLen = maxLen;
        out._paths.assign(starts.size() * (size_t)(maxLen > 0 ? maxLen : 0), -1);
        out._lengths.assign(starts.size(), 0);
        if (vtmc_navfield_trace(_ctx, starts.data(), (int32_t)starts.size(), maxLen, out._paths.data(), out._lengths.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_navfield_trace: ") + vtmc_last_error(_ctx));
    }
    void NavSight(const std::vector<int> &from, const std::vector<int> &to, std::vector<NavSightHit> &out) override
    {
        if (from.size() != to.size()) throw UnityException("NavSight: as many from as to spans");
        std::vector<vtmc_navsight_hit> hits(from.size());
        if (vtmc_nav_sight(_ctx, from.data(), to.data(), (int32_t)from.size(), hits.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_nav_sight: ") + vtmc_last_error(_ctx));
        out.clear();
        for (const vtmc_navsight_hit &h : hits) out.push_back(NavSightHit{h.last, h.steps});
    }
    void NavTraceSmooth(const std::vector<int> &starts, int maxLen, int maxLook, unsigned maxExtraCost, NavPaths &out) override
    {
        out._maxLen = maxLen;
        out._paths.assign(starts.size() * (size_t)(maxLen > 0 ? maxLen : 0), -1);
        out._lengths.assign(starts.size(), 0);
        vtmc_navsight_params p;
        p.max_look = maxLook, p.max_extra_cost = maxExtraCost, p.flags = 0, p.reserved = 0;
        if (vtmc_navfield_trace_smooth(_ctx, starts.data(), (int32_t)starts.size(), maxLen, &p, out._paths.data(), out._lengths.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_navfield_trace_smooth: ") + vtmc_last_error(_ctx));
    }
    int CrowdSpawn(const std::vector<int> &spans, const std::vector<unsigned> &speeds) override
    {
        if (spans.size() != speeds.size()) throw UnityException("SpawnCrowd: as many speeds as spans");
        static_assert(sizeof(unsigned) == sizeof(uint32_t), "speeds are read in place");
        int32_t placed = 0;
        if (vtmc_navcrowd_spawn(_ctx, spans.data(), speeds.data(), (int32_t)spans.size(), &placed) != VTMC_OK)
            throw UnityException(std::string("vtmc_navcrowd_spawn: ") + vtmc_last_error(_ctx));
        return placed;
    }
    void CrowdStep(unsigned maxDetour, bool leaveOnArrival, int ticks) override
    {
        vtmc_navcrowd_params p;
        p.max_detour = maxDetour, p.flags = leaveOnArrival ? VTMC_NAVCROWD_LEAVE_ON_ARRIVAL : 0u, p.reserved[0] = p.reserved[1] = 0u;
        if (vtmc_navcrowd_step(_ctx, &p, ticks) != VTMC_OK) throw UnityException(std::string("vtmc_navcrowd_step: ") + vtmc_last_error(_ctx));
    }
    void CrowdRead(CrowdResult &out) override
    {
        int32_t n = 0, nSpans = 0;
        if (vtmc_navcrowd_info(_ctx, &n, &out._occupying, &out._arrived, &out._ticks, &out._movedLast) != VTMC_OK || vtmc_nav_info(_ctx, nullptr, nullptr, &nSpans) != VTMC_OK)
            throw UnityException(std::string("vtmc_navcrowd_info: ") + vtmc_last_error(_ctx));
        std::vector<vtmc_navcrowd_agent> agents((size_t)n);
        out._occupancy.assign((size_t)nSpans, -1);
        if (vtmc_navcrowd_read(_ctx, agents.data(), n, out._occupancy.data()) != VTMC_OK) throw UnityException(std::string("vtmc_navcrowd_read: ") + vtmc_last_error(_ctx));
        out._agents.clear();
        for (const vtmc_navcrowd_agent &a : agents) out._agents.push_back(CrowdAgent{a.span, a.budget, a.speed, a.state});
    }
    void Flood(const float *lower, const float *upper, const std::vector<WaterSource> &sources, WaterResult &out) override
    {
        static_assert(sizeof(WaterBody) == sizeof(vtmc_water_body) && sizeof(WaterSource) == sizeof(vtmc_water_source), "copied as they lie");
        std::vector<vtmc_water_source> src(sources.size());
        for (size_t i = 0; i < sources.size(); i++) {
            src[i].position[0] = sources[i]._position.x, src[i].position[1] = sources[i]._position.y, src[i].position[2] = sources[i]._position.z;
            src[i].level = sources[i]._level;
        }
        out = WaterResult();
        out._sourceBody.assign(sources.size(), -1);
        int32_t n = 0;
        if (vtmc_terrain_flood(_ctx, lower, upper, src.data(), (int32_t)src.size(), 0u, out._sourceBody.data(), &n) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_flood: ") + vtmc_last_error(_ctx));
        int64_t wet = 0;
        if (vtmc_water_info(_ctx, out._boxLo, out._boxDims, out._volumeDims, &n, &wet) != VTMC_OK) throw UnityException(std::string("vtmc_water_info: ") + vtmc_last_error(_ctx));
        out._wet = wet;
        out._bodies.resize((size_t)n);
        if (vtmc_water_bodies(_ctx, reinterpret_cast<vtmc_water_body *>(out._bodies.data()), n) != VTMC_OK)
            throw UnityException(std::string("vtmc_water_bodies: ") + vtmc_last_error(_ctx));
        const size_t vn = (size_t)out._volumeDims[0] * out._volumeDims[1] * out._volumeDims[2];
        out._water.resize(vn), out._bodyVolume.resize(vn);
        if (vtmc_water_read(_ctx, out._water.data(), out._bodyVolume.data(), (int64_t)vn) != VTMC_OK) throw UnityException(std::string("vtmc_water_read: ") + vtmc_last_error(_ctx));
    }
    void ProbeWater(const std::vector<Vector3> &positions, std::vector<WaterProbe> &out) override
    {
        std::vector<float> p;
        for (const Vector3 &v : positions) p.push_back(v.x), p.push_back(v.y), p.push_back(v.z);
        std::vector<int32_t> body(positions.size(), -1);
        std::vector<float> depth(positions.size(), 0.0f);
        if (vtmc_water_probe(_ctx, p.data(), (int32_t)positions.size(), body.data(), depth.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_water_probe: ") + vtmc_last_error(_ctx));
        out.clear();
        for (size_t i = 0; i < positions.size(); i++) out.push_back(WaterProbe{body[i], depth[i]});
    }

    int MaterialInit(int fineness) override
    {
        if (vtmc_material_init(_ctx, fineness) != VTMC_OK) throw UnityException(std::string("vtmc_material_init: ") + vtmc_last_error(_ctx));
        return 16 * fineness;
    }
    void MaterialSetControlMap(const Color *mapData, int group) override
    {
        if (vtmc_material_set_control_map(_ctx, reinterpret_cast<const float *>(mapData), group) != VTMC_OK)
            throw UnityException(std::string("vtmc_material_set_control_map: ") + vtmc_last_error(_ctx));
    }
    void MaterialPaint(const std::vector<MaterialStroke> &strokes) override
    {
        std::vector<vtmc_material_stroke> s(strokes.size());
        for (size_t i = 0; i < strokes.size(); i++) {
            s[i].center[0] = strokes[i]._center.x, s[i].center[1] = strokes[i]._center.y, s[i].center[2] = strokes[i]._center.z;
            s[i].radius = strokes[i]._radius;
            s[i].strength = strokes[i]._strength;
            s[i].channel = strokes[i]._channel;
        }
        if (vtmc_material_paint(_ctx, s.data(), (int32_t)s.size()) != VTMC_OK)
            throw UnityException(std::string("vtmc_material_paint: ") + vtmc_last_error(_ctx));
    }
    void MaterialVertices(std::vector<uint8_t> &out) override
    {
        int64_t n = 0;
        if (vtmc_material_vertices(_ctx, &n) != VTMC_OK) throw UnityException(std::string("vtmc_material_vertices: ") + vtmc_last_error(_ctx));
        out.resize((size_t)n * VTMC_MATERIAL_CHANNELS);
        if (vtmc_material_read_vertices(_ctx, out.data(), n) != VTMC_OK)
            throw UnityException(std::string("vtmc_material_read_vertices: ") + vtmc_last_error(_ctx));
    }

    void TerrainExtractLod(const Vector3 &viewer, int maxLevel, float split, int maxNodes, std::vector<LodNode> &nodes,
                           std::vector<CSTriangle> &tris, std::vector<int> &offsets) override
    {
        vtmc_lod_params p;
        p.viewer[0] = viewer.x, p.viewer[1] = viewer.y, p.viewer[2] = viewer.z;
        p.split = split;
        p.max_level = maxLevel;
        p.max_nodes = maxNodes;
        int32_t nNodes = 0, triNum = 0;
        if (vtmc_terrain_extract_lod(_ctx, &p, &nNodes, &triNum) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_extract_lod: ") + vtmc_last_error(_ctx));
        std::vector<vtmc_lod_node> list((size_t)nNodes);
        if (vtmc_terrain_lod_nodes(_ctx, list.data(), nNodes, nullptr) != VTMC_OK)
            throw UnityException(std::string("vtmc_terrain_lod_nodes: ") + vtmc_last_error(_ctx));
        nodes.clear();
        for (const vtmc_lod_node &nd : list) nodes.push_back(LodNode{MathHelper::Int3(nd.origin[0], nd.origin[1], nd.origin[2]), nd.level});
        tris.resize((size_t)triNum);
        offsets.assign((size_t)nNodes + 1, 0);
        if (vtmc_read_triangles(_ctx, reinterpret_cast<vtmc_triangle *>(tris.data()), triNum, offsets.data()) != VTMC_OK)
            throw UnityException(std::string("vtmc_read_triangles: ") + vtmc_last_error(_ctx));
    }

private:
    vtmc_ctx *_ctx = nullptr;
    int _dims[3] = {0, 0, 0};
};
}  // namespace

std::shared_ptr<ExtractBackend> MakeVtmcBackend(int device) { return std::make_shared<VtmcBackend>(device); }

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
    if (_deviceResident) {
        _voxelSamples.clear();  // the grid lives in HBM
        if (!_backend->TerrainInit(_width, _elevation, _height, _voxelScale, TerrainOrigin, _seed))
            throw UnityException("backend has no device-resident terrain");
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

void VoxelTerrain::EnsureMaterialLayer()
{
    if (!_initialised || !_deviceResident) throw UnityException("the material layer needs an initialised device-resident terrain");
    if (_hasMaterialLayer) return;
    _matControlFineness = std::min(std::max(_matControlFineness, 1), 8);  // Mathf.Clamp, VoxelTerrain.cs:191
    _backend->MaterialInit(_matControlFineness);
    _hasMaterialLayer = true;
}

// VoxelTerrain.cs:186-209
void VoxelTerrain::SetControlMap(const Color *mapData, size_t length, int group)
{
    if (group < 1 || group > 2) throw UnityException("invalid control map group");
    const size_t controlMapSize = (size_t)std::min(std::max(_matControlFineness, 1), 8) * 16;
    if (!mapData || length != controlMapSize * controlMapSize * controlMapSize) throw UnityException("invalid control map data size");
    EnsureMaterialLayer();
    _backend->MaterialSetControlMap(mapData, group);
}

void VoxelTerrain::Paint(const std::vector<MaterialStroke> &strokes)
{
    EnsureMaterialLayer();
    _backend->MaterialPaint(strokes);
}

const std::vector<uint8_t> &VoxelTerrain::VertexMaterials()
{
    EnsureMaterialLayer();
    _backend->MaterialVertices(_vertexMaterials);
    return _vertexMaterials;
}

std::vector<Fragment> VoxelTerrain::Fragments(const Vector3 &lower, const Vector3 &upper, int maxSamples, int captureMinSamples)
{
    if (!_initialised || !_deviceResident) throw UnityException("Fragments needs an initialised device-resident terrain");
    std::vector<Fragment> out;
    _backend->TerrainFragments(lower, upper, maxSamples, captureMinSamples, out);
    return out;
}

NavResult VoxelTerrain::BuildNav(const Vector3 &lower, const Vector3 &upper, float agentHeight, float maxStep, int maxSpans)
{
    if (!_initialised || !_deviceResident) throw UnityException("BuildNav needs an initialised device-resident terrain");
    const float samples = std::ceil(agentHeight / _voxelScale);
    if (!(samples >= 1.0f && samples <= (float)VTMC_NAV_MAX_AGENT_HEIGHT)) throw UnityException("BuildNav: agentHeight outside 1..256 samples");
    NavResult out;
    _backend->TerrainNav(lower, upper, (int)samples, maxStep / _voxelScale, maxSpans, out);
    return out;
}

static int NavRadiusColumns(float radius, float voxelScale, const char *who)
{
    const float columns = std::ceil(radius / voxelScale);
    if (!(columns >= 0.0f && columns <= (float)VTMC_NAVERODE_MAX_RADIUS)) throw UnityException(std::string(who) + ": radius outside 0..255 columns");
    return (int)columns;
}

std::vector<int> VoxelTerrain::NavDistance(float radius, bool openBoxFaces)
{
    if (!_initialised || !_deviceResident) throw UnityException("NavDistance needs an initialised device-resident terrain");
    std::vector<int> out;
    _backend->NavDistance(NavRadiusColumns(radius, _voxelScale, "NavDistance"), openBoxFaces, out);
    return out;
}

NavResult VoxelTerrain::ErodeNav(float radius, bool openBoxFaces)
{
    if (!_initialised || !_deviceResident) throw UnityException("ErodeNav needs an initialised device-resident terrain");
    NavResult out;
    _backend->NavErode(NavRadiusColumns(radius, _voxelScale, "ErodeNav"), openBoxFaces, out);
    return out;
}

std::vector<int> VoxelTerrain::LocateOnNav(const std::vector<Vector3> &positions, float below, float above)
{
    if (!_initialised || !_deviceResident) throw UnityException("LocateOnNav needs an initialised device-resident terrain");
    std::vector<int> out;
    _backend->NavLocate(positions, below / _voxelScale, above / _voxelScale, out);
    return out;
}

std::vector<NavFieldCell> VoxelTerrain::BuildNavField(const std::vector<NavGoal> &goals, float climbCost, float dropCost, unsigned maxCost)
{
    if (!_initialised || !_deviceResident) throw UnityException("BuildNavField needs an initialised device-resident terrain");
    std::vector<NavFieldCell> out;
    _backend->NavField(goals, climbCost, dropCost, maxCost, out);
    return out;
}

NavPaths VoxelTerrain::TracePaths(const std::vector<int> &starts, int maxLen)
{
    if (!_initialised || !_deviceResident) throw UnityException("TracePaths needs an initialised device-resident terrain");
    NavPaths out;
    _backend->NavTrace(starts, maxLen, out);
    return out;
}

std::vector<NavSightHit> VoxelTerrain::NavSight(const std::vector<int> &from, const std::vector<int> &to)
{
    if (!_initialised || !_deviceResident) throw UnityException("NavSight needs an initialised device-resident terrain");
    std::vector<NavSightHit> out;
    _backend->NavSight(from, to, out);
    return out;
}

NavPaths VoxelTerrain::SmoothPaths(const std::vector<int> &starts, int maxLen, int maxLook, unsigned maxExtraCost)
{
    if (!_initialised || !_deviceResident) throw UnityException("SmoothPaths needs an initialised device-resident terrain");
    NavPaths out;
    _backend->NavTraceSmooth(starts, maxLen, maxLook, maxExtraCost, out);
    return out;
}

int VoxelTerrain::SpawnCrowd(const std::vector<int> &spans, const std::vector<unsigned> &speeds)
{
    if (!_initialised || !_deviceResident) throw UnityException("SpawnCrowd needs an initialised device-resident terrain");
    return _backend->CrowdSpawn(spans, speeds);
}

void VoxelTerrain::StepCrowd(int ticks, unsigned maxDetour, bool leaveOnArrival)
{
    if (!_initialised || !_deviceResident) throw UnityException("StepCrowd needs an initialised device-resident terrain");
    _backend->CrowdStep(maxDetour, leaveOnArrival, ticks);
}

CrowdResult VoxelTerrain::ReadCrowd()
{
    if (!_initialised || !_deviceResident) throw UnityException("ReadCrowd needs an initialised device-resident terrain");
    CrowdResult out;
    _backend->CrowdRead(out);
    return out;
}

WaterResult VoxelTerrain::Flood(Vector3 lower, Vector3 upper, const std::vector<WaterSource> &sources)
{
    if (!_initialised || !_deviceResident) throw UnityException("Flood needs an initialised device-resident terrain");
    const float lo[3] = {lower.x, lower.y, lower.z}, up[3] = {upper.x, upper.y, upper.z};
    WaterResult out;
    _backend->Flood(lo, up, sources, out);
    return out;
}

std::vector<WaterProbe> VoxelTerrain::ProbeWater(const std::vector<Vector3> &positions)
{
    if (!_initialised || !_deviceResident) throw UnityException("ProbeWater needs an initialised device-resident terrain");
    std::vector<WaterProbe> out;
    _backend->ProbeWater(positions, out);
    return out;
}

int VoxelTerrain::ExtractLod(const Vector3 &viewer, int maxLevel, float split, int maxNodes)
{
    if (!_initialised || !_deviceResident) throw UnityException("ExtractLod needs an initialised device-resident terrain");
    std::vector<CSTriangle> csTriangles;
    std::vector<int> offsets;
    _backend->TerrainExtractLod(viewer, maxLevel, split, maxNodes, _lodNodes, csTriangles, offsets);
    _lodMeshes.assign(_lodNodes.size(), BlockMesh());
    for (size_t i = 0; i < _lodNodes.size(); i++) {
        BlockMesh &mesh = _lodMeshes[i];
        const float cell = (float)(1 << _lodNodes[i]._level) * _voxelScale;  // a node's cell in world units
        for (int t = offsets[i]; t < offsets[i + 1]; t++) {
            const CSTriangle &vt = csTriangles[(size_t)t];
            mesh.vertices.push_back(Vector3(vt._position0[0], vt._position0[1], vt._position0[2]) * cell);
            mesh.vertices.push_back(Vector3(vt._position1[0], vt._position1[1], vt._position1[2]) * cell);
            mesh.vertices.push_back(Vector3(vt._position2[0], vt._position2[1], vt._position2[2]) * cell);
            mesh.normals.push_back(Vector3(vt._normal0[0], vt._normal0[1], vt._normal0[2]));
            mesh.normals.push_back(Vector3(vt._normal1[0], vt._normal1[1], vt._normal1[2]));
            mesh.normals.push_back(Vector3(vt._normal2[0], vt._normal2[1], vt._normal2[2]));
        }
        mesh.triangles.resize(mesh.vertices.size());
        for (size_t k = 0; k < mesh.triangles.size(); k++) mesh.triangles[k] = (int)k;
    }
    return (int)csTriangles.size();
}

// VoxelTerrain.cs:214-245
void VoxelTerrain::Free()
{
    for (BlockMesh &b : _blocks) b.Clear();
    _blocks.clear();
    _lodNodes.clear();
    _lodMeshes.clear();
    _backend.reset();
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
        std::vector<ExtractBackend::QueuedModifier> queue;
        std::vector<std::shared_ptr<TerrainModifier>> alive;  // descriptors borrow from the modifiers (heightmap) until the call returns
        while (!_modifierQueue.empty()) {
            std::shared_ptr<TerrainModifier> modifier = _modifierQueue.front();
            _modifierQueue.pop_front();
            ExtractBackend::QueuedModifier q;
            if (!modifier->Describe(q.desc)) throw UnityException("modifier cannot be evaluated on the device (Describe() returned false)");
            q.addOrErode = modifier->AddOrErode;
            q.lower = modifier->LowerBound();
            q.upper = modifier->UpperBound();
            queue.push_back(q);
            alive.push_back(std::move(modifier));
        }
        _lastUpdateBlocks.clear();
        _lastTriNum = 0;
        if (queue.empty()) return;
        std::vector<CSTriangle> csTriangles;
        std::vector<int> offsets;
        _backend->TerrainUpdate(queue, _nextUpdateblocks, csTriangles, offsets);
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

std::vector<float> VoxelTerrain::DeviceSamples() const
{
    std::vector<float> out;
    if (!_deviceResident || !_backend) throw UnityException("DeviceSamples needs an initialised device-resident terrain");
    _backend->TerrainReadSamples(out);
    return out;
}

// VoxelTerrain.cs:430-465: per dirty block, vertices (scaled by _voxelScale), normals, trivial indices
void VoxelTerrain::ApplyMeshes(const std::vector<CSTriangle> &csTriangles, const std::vector<int> &offsets)
{
    const int nby = _elevation / blockSize, nbz = _height / blockSize;
    for (size_t i = 0; i < _nextUpdateblocks.size(); i++) {
        const Int3 &b = _nextUpdateblocks[i];
        BlockMesh &mesh = _blocks[((size_t)b._x * nby + b._y) * nbz + b._z];
        mesh.Clear();  // VoxelTerrain.cs:453
        for (int t = offsets[i]; t < offsets[i + 1]; t++) {
            const CSTriangle &vt = csTriangles[(size_t)t];
            mesh.vertices.push_back(Vector3(vt._position0[0], vt._position0[1], vt._position0[2]) * _voxelScale);
            mesh.vertices.push_back(Vector3(vt._position1[0], vt._position1[1], vt._position1[2]) * _voxelScale);
            mesh.vertices.push_back(Vector3(vt._position2[0], vt._position2[1], vt._position2[2]) * _voxelScale);
            mesh.normals.push_back(Vector3(vt._normal0[0], vt._normal0[1], vt._normal0[2]));
            mesh.normals.push_back(Vector3(vt._normal1[0], vt._normal1[1], vt._normal1[2]));
            mesh.normals.push_back(Vector3(vt._normal2[0], vt._normal2[1], vt._normal2[2]));
        }
        mesh.triangles.resize(mesh.vertices.size());
        for (size_t k = 0; k < mesh.triangles.size(); k++) mesh.triangles[k] = (int)k;  // Enumerable.Range, VoxelTerrain.cs:457
    }
}

}  // namespace Render
}  // namespace PGRTerrain
