// host_selftest.cpp -- drives the C++ VoxelTerrain mirror the way TerrainEngine / SceneManager drive
// the C# class (TerrainEngine.cs:87,148,160; SceneManager.cs:121-129).
//   host_selftest <mode> [<out_dir>]
// The modes, what each does and the token it prints when all went well are the rows of kModes at the end of this file; run without
// arguments, the program prints them.  Exit status: 0 success, 1 a failed CHECK (which prints itself), 3 an exception, 64 usage.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "voxel_terrain.hpp"

using namespace PGRTerrain;
using namespace PGRTerrain::Render;
using MathHelper::Int3;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

struct Recorder : ExtractBackend {
    int calls = 0;
    std::vector<Int3> blocks;
    std::vector<float> grid;
    void Extract(const float *g, int w, int e, int h, const std::vector<Int3> &b, std::vector<CSTriangle> &tris,
                 std::vector<int> &offs) override
    {
        ++calls;
        blocks = b;
        grid.assign(g, g + (size_t)(w + 2) * (e + 2) * (h + 2));
        tris.clear();
        offs.assign(b.size() + 1, 0);
    }
};

// whether the call throws an E
template <class E = UnityException, class F>
static bool Refused(F &&call)
{
    try {
        call();
    } catch (const E &) {
        return true;
    }
    return false;
}

// the text of the UnityException the call throws, "" when it throws none
template <class F>
static std::string Message(F &&call)
{
    try {
        call();
    } catch (const UnityException &e) {
        return e.what();
    }
    return "";
}

// <out_dir>/<name>: the elements as they lie
template <class T>
static void Dump(const std::string &out, const std::string &name, const T *data, size_t count)
{
    std::ofstream(out + "/" + name, std::ios::binary).write(reinterpret_cast<const char *>(data), (std::streamsize)(count * sizeof(T)));
}
template <class T>
static void Dump(const std::string &out, const std::string &name, const std::vector<T> &v)
{
    Dump(out, name, v.data(), v.size());
}
static_assert(sizeof(Vector3) == 12, "dumped as it lies");

static int cpu_tests(const std::string &)
{
    {  // VoxelTerrain.cs:138-142
        VoxelTerrain bad;
        bad.SetBackend(std::make_shared<Recorder>());
        bad._width = 10;
        CHECK(Message([&] { bad.Init(); }) == "block size must align to terrain size");
        bad._width = 1032;
        CHECK(Message([&] { bad.Init(); }) == "too high resolution (exceeds 1025)");
    }
    {  // a backend of the caller's has no device-resident terrain
        VoxelTerrain resident;
        resident.SetBackend(std::make_shared<Recorder>());
        resident._deviceResident = true;
        CHECK(Message([&] { resident.Init(); }) == "backend has no device-resident terrain");
    }
    VoxelTerrain vt;
    auto rec = std::make_shared<Recorder>();
    vt.SetBackend(rec);
    vt._width = vt._elevation = vt._height = 64;
    vt.Init();
    for (float s : vt.Samples()) CHECK(s >= -2.0f && s <= -1.0f);  // voidDensity, VoxelTerrain.cs:145-149
    vt.Update();                                                  // empty queue: nothing happens
    CHECK(rec->calls == 0);

    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(16, 16, 16), 10.0f, true));
    vt.Update();
    CHECK(rec->calls == 1);
    // AABB [6,26] touches blocks 0..3 on each axis (inclusive test, VoxelTerrain.cs:311-313)
    CHECK(rec->blocks.size() == 64);
    for (const Int3 &b : rec->blocks) CHECK(b._x <= 3 && b._y <= 3 && b._z <= 3);
    float c = vt.Sample(16, 16, 16);
    CHECK(c >= 1.0f && c <= 2.0f);                        // clamp(10, void, full) = full in [1,2]
    float edge = vt.Sample(16, 16, 25);                   // r - 9 = 1 -> min(1, full) = 1
    CHECK(std::fabs(edge - 1.0f) < 1e-6f);
    float inside = vt.Sample(16, 16, 25 + 0) - vt.Sample(16, 16, 26);
    CHECK(inside > 0);                                    // density decreases outwards
    CHECK(vt.Sample(40, 40, 40) <= -1.0f);                // untouched samples stay void
    CHECK(std::fabs(vt.Sample(16, 22, 16) - 4.0f) > 1.9f);  // 10 - 6 = 4 is clamped into [1,2]

    // erode: S = clamp(min(S, -md)) (VoxelTerrain.cs:296-304)
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(16, 16, 16), 4.0f, false));
    vt.Update();
    CHECK(rec->calls == 2);
    CHECK(vt.Sample(16, 16, 16) <= -1.0f);                // -clamp(4,..) = -full -> void range
    CHECK(rec->blocks.size() == 8);                       // AABB [12,20]: up >= 8b && low <= 8b+8 holds for b = 1, 2 only
    for (const Int3 &b : rec->blocks) CHECK(b._x >= 1 && b._x <= 2 && b._y >= 1 && b._y <= 2 && b._z >= 1 && b._z <= 2);

    {  // SetControlMap's two errors (VoxelTerrain.cs:187-195) come before anything reaches the backend; the layer needs a resident terrain
        auto message = [&](const std::vector<Color> &map, int group) { return Message([&] { vt.SetControlMap(map, group); }); };
        vt._matControlFineness = 1;
        const std::vector<Color> map(16 * 16 * 16);
        CHECK(message(map, 0) == "invalid control map group" && message(map, 3) == "invalid control map group");
        CHECK(message(std::vector<Color>(100), 1) == "invalid control map data size");
        vt._matControlFineness = 2;
        CHECK(message(map, 2) == "invalid control map data size");
        vt._matControlFineness = 1;
        CHECK(message(map, 1).find("device-resident") != std::string::npos);   // this terrain keeps its samples on the host
        CHECK(Refused<std::invalid_argument>([] { MaterialStroke(Vector3(0, 0, 0), -1.0f, 0); }));
    }
    {  // everything device-resident refuses this terrain, which keeps its samples on the host, and says under its own name what it needs
        const Vector3 lo(0, 0, 0), up(8, 8, 8);
        const std::vector<Color> map(16 * 16 * 16);
#define NEEDS_RESIDENT(who, call) CHECK(Message([&] { call; }) == who " needs an initialised device-resident terrain")
        NEEDS_RESIDENT("BuildNav", vt.BuildNav(lo, up, 1.0f, 0.5f));
        NEEDS_RESIDENT("NavDistance", vt.NavDistance(1.0f));
        NEEDS_RESIDENT("ErodeNav", vt.ErodeNav(1.0f));
        NEEDS_RESIDENT("LocateOnNav", vt.LocateOnNav({lo}, 1.0f, 1.0f));
        NEEDS_RESIDENT("BuildNavField", vt.BuildNavField({NavGoal{0, 0u}}, 1.0f, 1.0f));
        NEEDS_RESIDENT("TracePaths", vt.TracePaths({0}, 4));
        NEEDS_RESIDENT("NavSight", vt.NavSight({0}, {0}));
        NEEDS_RESIDENT("SmoothPaths", vt.SmoothPaths({0}, 4));
        NEEDS_RESIDENT("SpawnCrowd", vt.SpawnCrowd({0}, {1u}));
        NEEDS_RESIDENT("StepCrowd", vt.StepCrowd(1));
        NEEDS_RESIDENT("ReadCrowd", vt.ReadCrowd());
        NEEDS_RESIDENT("Flood", vt.Flood(lo, up, {WaterSource{lo, 1.0f}}));
        NEEDS_RESIDENT("ProbeWater", vt.ProbeWater({lo}));
        NEEDS_RESIDENT("Light", vt.Light(lo, up, 255, 16, 16, {LightSource{lo, 1}}));
        NEEDS_RESIDENT("ProbeLight", vt.ProbeLight({lo}));
        NEEDS_RESIDENT("ReadErosion", vt.ReadErosion());
        NEEDS_RESIDENT("Fragments", vt.Fragments(lo, up));
        NEEDS_RESIDENT("ExtractLod", vt.ExtractLod(lo, 1));
        NEEDS_RESIDENT("DeviceSamples", vt.DeviceSamples());
        NEEDS_RESIDENT("the material layer", vt.SetControlMap(map, 1));
        NEEDS_RESIDENT("the material layer", vt.Paint({MaterialStroke(lo, 1.0f, 0)}));
        NEEDS_RESIDENT("the material layer", vt.VertexMaterials());
#undef NEEDS_RESIDENT
        CHECK(rec->calls == 2);   // and none of them reached the backend
        // the erosion mirror refuses what the library refuses, and describes itself as kind 12
        CHECK(Refused<std::invalid_argument>([&] { ErosionModifier(lo, up, 0); }) && Refused<std::invalid_argument>([&] { ErosionModifier(lo, up, 65537); }));
        CHECK(Refused<std::invalid_argument>([&] { ErosionModifier(lo, up, 8, NAN); }) && Refused<std::invalid_argument>([&] { ErosionModifier(lo, up, 8, -0.1f); }));
        CHECK(Refused<std::invalid_argument>([&] { ErosionModifier(lo, up, 8, 0.01f, 8.0f, 1.0f, 0.3f, 0.3f, 0.25f); }));   // evaporation * dt > 1
        CHECK(Refused<std::invalid_argument>([&] { ErosionModifier(lo, up, 8, 0.01f, 0.02f, 1.0f, 0.3f, 0.3f, 0.0f); }));   // dt = 0
        CHECK(Refused<std::invalid_argument>([&] { ErosionModifier(lo, up, 8, 0.01f, 0.02f, 1.0f, 0.3f, 0.3f, 0.25f, 1.0f, 0.2f); }));   // thermal rate
        ModifierDesc d;
        const ErosionModifier erosion(lo, up, 40, 0.02f, 0.05f, 1.0f, 0.3f, 0.25f, 0.5f, 0.75f, 0.1f);
        CHECK(erosion.Describe(d) && d.kind == 12 && d.dims[0] == 40 && d.dims[1] == 0 && d.data == nullptr);
        CHECK(d.p[0] == 0.02f && d.p[1] == 0.05f && d.p[2] == 1.0f && d.p[3] == 0.3f && d.p[4] == 0.25f && d.p[5] == 0.5f && d.p[6] == 0.75f && d.p[7] == 0.1f);
        CHECK(Refused<std::logic_error>([&] { erosion.QueryDensity(lo); }));
    }
    return 0;
}

// the scene of --gpu and --gpu-resident: 64 x 32 x 64 cells, Init, and a plane, a sphere and an eroding cylinder in the queue
static void scene_init(VoxelTerrain &vt)
{
    vt._width = 64;
    vt._elevation = 32;
    vt._height = 64;
    vt._voxelScale = 0.5f;
    vt.TerrainOrigin = Vector3(-3.0f, 1.0f, 2.0f);
    vt.Init();
    Vector2 lo, up;
    lo.x = -100; lo.y = -100; up.x = 100; up.y = 100;
    vt.InsertModifier(std::make_shared<PlaneModifier>(6.3f, lo, up, true));
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(10.0f, 8.0f, 15.0f), 5.5f, true));
    vt.InsertModifier(std::make_shared<CylinderModifier>(Vector3(2.0f, 5.0f, 6.0f), Vector3(1.0f, 0.3f, 0.5f), 20.0f, 2.2f, false));
}

// the blocks of the last Update and their meshes: <prefix>blocks.i32, counts.i32, vertices.f32, normals.f32
static int dump_meshes(const VoxelTerrain &vt, const std::string &out, const std::string &prefix)
{
    std::vector<int> blocks, counts;
    std::vector<Vector3> vertices, normals;
    for (const Int3 &b : vt.LastUpdateBlocks()) {
        blocks.insert(blocks.end(), {b._x, b._y, b._z});
        const BlockMesh &m = vt.Block(b._x, b._y, b._z);
        counts.push_back((int)m.vertices.size());
        CHECK(m.normals.size() == m.vertices.size() && m.triangles.size() == m.vertices.size());
        for (size_t i = 0; i < m.triangles.size(); i++) CHECK(m.triangles[i] == (int)i);
        vertices.insert(vertices.end(), m.vertices.begin(), m.vertices.end());
        normals.insert(normals.end(), m.normals.begin(), m.normals.end());
    }
    Dump(out, prefix + "blocks.i32", blocks);
    Dump(out, prefix + "counts.i32", counts);
    Dump(out, prefix + "vertices.f32", vertices);
    Dump(out, prefix + "normals.f32", normals);
    return 0;
}

static int gpu_run(const std::string &out)
{
    VoxelTerrain vt;
    vt.SeedRandom(7);
    scene_init(vt);
    vt.Update();
    std::printf("blocks %zu triangles %d\n", vt.LastUpdateBlocks().size(), vt.LastTriangleCount());
    Dump(out, "grid.f32", vt.Samples());
    if (int rc = dump_meshes(vt, out, "")) return rc;
    // an edit like SceneManager.Update's mouse sphere (SceneManager.cs:121-129): small dirty set
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(5.0f, 4.0f, 9.0f), 2.0f, false));
    vt.Update();
    std::printf("edit: blocks %zu triangles %d\n", vt.LastUpdateBlocks().size(), vt.LastTriangleCount());
    vt.Free();
    return 0;
}

// the same scene with the grid resident in HBM and Update's density write on the GPU
static int gpu_resident_run(const std::string &out)
{
    VoxelTerrain vt;
    vt._deviceResident = true;
    vt._seed = 4242;
    scene_init(vt);
    {   // a small island on top (IslandModifier, the world-build modifier of TerrainEngine.cs:87)
        const int res = 9;
        std::vector<float> hm((size_t)res * res);
        for (int u = 0; u < res; u++)
            for (int v = 0; v < res; v++) hm[(size_t)u * res + v] = 4.0f + 0.5f * (float)((u * 3 + v * 5) % 7);
        vt.InsertModifier(std::make_shared<IslandModifier>(hm, res, res, 20.0f, 24.0f, 9.0f, true));
    }
    vt.Update();
    std::printf("resident: blocks %zu triangles %d\n", vt.LastUpdateBlocks().size(), vt.LastTriangleCount());
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(5.0f, 4.0f, 9.0f), 2.0f, false));
    vt.Update();
    std::printf("resident edit: blocks %zu triangles %d\n", vt.LastUpdateBlocks().size(), vt.LastTriangleCount());
    Dump(out, "r_grid.f32", vt.DeviceSamples());
    if (int rc = dump_meshes(vt, out, "r_")) return rc;
    {   // the material layer: a control map, a stroke, and the weights of the edit's vertices
        vt._matControlFineness = 1;
        std::vector<Color> map(16 * 16 * 16);
        for (Color &c : map) c.g = 1.0f;                                  // all grass: channel 1
        vt.SetControlMap(map, 1);
        vt.Paint({MaterialStroke(Vector3(5.0f, 4.0f, 9.0f), 6.0f, 2)});   // rock around the dig: channel 2
        const std::vector<uint8_t> &w = vt.VertexMaterials();
        CHECK(w.size() == (size_t)vt.LastTriangleCount() * 3 * 8);
        size_t rock = 0;
        for (size_t v = 0; v < w.size(); v += 8) {
            CHECK(w[v] == 0 && w[v + 3] == 0 && w[v + 4] == 0);           // only channels 1 and 2 were ever set
            rock += w[v + 2] > w[v + 1];
        }
        std::printf("resident materials: %zu vertices, %zu mostly rock\n", w.size() / 8, rock);
        CHECK(rock != 0);
    }
    vt.Free();
    return 0;
}

// The world every mode from --gpu-lod on shares (mirror_world of tests/nav_support.py): a device-resident terrain of 64 x 32 x 32 cells at
// scale 0.5 with seed 977, a plane, a sphere that crosses the terrain's upper x face and a dug hollow.  Returns the triangle count of its
// Update, which every mode compares with LastTriangleCount() at its end: what Update left stands.
static int resident_world(VoxelTerrain &vt)
{
    vt._width = 64;
    vt._elevation = 32;
    vt._height = 32;
    vt._voxelScale = 0.5f;
    vt.TerrainOrigin = Vector3(-3.0f, 1.0f, 2.0f);
    vt._deviceResident = true;
    vt._seed = 977;
    vt.Init();
    Vector2 lo, up;
    lo.x = -100; lo.y = -100; up.x = 100; up.y = 100;
    vt.InsertModifier(std::make_shared<PlaneModifier>(6.3f, lo, up, true));
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(27.5f, 8.0f, 10.0f), 4.25f, true));
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(5.0f, 6.0f, 9.0f), 3.0f, false));
    vt.Update();
    return vt.LastTriangleCount();
}

// the nav build the --gpu-nav* modes share: an agent 0.9 world units high (2 samples) that steps 0.4 (0.8 grid units), in a box around the dig
static NavResult world_nav(VoxelTerrain &vt) { return vt.BuildNav(Vector3(-1.0f, 1.0f, 3.0f), Vector3(14.0f, 15.0f, 16.5f), 0.9f, 0.4f); }

// every span of the build as a start, and a -1
static std::vector<int> all_spans_and_none(const NavResult &nav)
{
    std::vector<int> starts(nav._spans.size());
    for (size_t i = 0; i < starts.size(); i++) starts[i] = (int)i;
    starts.push_back(-1);
    return starts;
}

static int gpu_nav_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const NavResult nav = world_nav(vt);
    std::printf("nav: spans %zu columns %zu box %d %d %d + %d %d %d\n", nav._spans.size(), nav._columnOffsets.size() - 1, nav._boxLo._x, nav._boxLo._y,
                nav._boxLo._z, nav._boxDims._x, nav._boxDims._y, nav._boxDims._z);
    CHECK(!nav._spans.empty() && nav._columnOffsets.size() == (size_t)nav._boxDims._x * nav._boxDims._z + 1);
    CHECK(nav._columnOffsets.back() == (int)nav._spans.size() && vt.LastTriangleCount() == updateTriangles);
    static_assert(sizeof(NavSpan) == 32, "dumped as it lies");
    Dump(out, "nav_spans.bin", nav._spans);
    Dump(out, "nav_offsets.i32", nav._columnOffsets);
    const int box[6] = {nav._boxLo._x, nav._boxLo._y, nav._boxLo._z, nav._boxDims._x, nav._boxDims._y, nav._boxDims._z};
    Dump(out, "nav_box.i32", box, 6);
    CHECK(Refused([&] { vt.BuildNav(Vector3(0, 0, 0), Vector3(1, 1, 1), 200.0f, 0.4f); }));   // 200 world units of headroom are 400 samples: more than the layer takes
    return 0;
}

// the distances of an agent 1.2 world units wide (3 columns), then the erosion by 0.8 (2 columns) with the box's faces open
static int gpu_naverode_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const NavResult nav = world_nav(vt);
    const std::vector<int> dist = vt.NavDistance(1.2f);
    CHECK(dist.size() == nav._spans.size() && nav._origin.empty());
    const NavResult eroded = vt.ErodeNav(0.8f, true);
    std::printf("naverode: spans %zu kept %zu\n", nav._spans.size(), eroded._spans.size());
    CHECK(!eroded._spans.empty() && eroded._spans.size() < nav._spans.size() && eroded._origin.size() == eroded._spans.size());
    CHECK(eroded._columnOffsets.size() == nav._columnOffsets.size() && eroded._columnOffsets.back() == (int)eroded._spans.size());
    CHECK(eroded._boxLo._x == nav._boxLo._x && eroded._boxDims._z == nav._boxDims._z && vt.LastTriangleCount() == updateTriangles);
    for (size_t i = 0; i < eroded._spans.size(); i++) {
        const int o = eroded._origin[i];
        CHECK(o >= 0 && o < (int)nav._spans.size() && (i == 0 || o > eroded._origin[i - 1]) && eroded._spans[i]._y == nav._spans[(size_t)o]._y);
    }
    Dump(out, "naverode_distance.i32", dist);
    Dump(out, "naverode_spans.bin", eroded._spans);
    Dump(out, "naverode_offsets.i32", eroded._columnOffsets);
    Dump(out, "naverode_origin.i32", eroded._origin);
    CHECK(Refused([&] { vt.ErodeNav(200.0f); }));   // 200 world units are 400 columns: more than the layer takes
    return 0;
}

// a field towards two goals found by position, then every span's path
static int gpu_navfield_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const NavResult nav = world_nav(vt);
    // two agents' worth of goals by position: on the plane (height 6.3) near a corner of the box, and further along it; 1 world unit either way
    const std::vector<int> at = vt.LocateOnNav({Vector3(0.0f, 6.3f, 4.0f), Vector3(12.0f, 6.3f, 15.0f), Vector3(500.0f, 6.3f, 4.0f)}, 1.0f, 1.0f);
    CHECK(at.size() == 3 && at[0] >= 0 && at[1] >= 0 && at[2] == -1);
    const std::vector<NavFieldCell> cells = vt.BuildNavField({NavGoal{at[0], 0u}, NavGoal{at[1], 3000u}}, 2.0f, 0.5f);
    CHECK(cells.size() == nav._spans.size() && cells[(size_t)at[0]]._cost == 0u && cells[(size_t)at[0]]._next == -1);
    const std::vector<int> starts = all_spans_and_none(nav);
    const NavPaths paths = vt.TracePaths(starts, 64);
    CHECK(paths._lengths.size() == starts.size() && paths._paths.size() == starts.size() * 64 && paths._lengths.back() == 0);
    CHECK(vt.LastTriangleCount() == updateTriangles);
    std::printf("navfield: spans %zu goals %d %d\n", cells.size(), at[0], at[1]);
    static_assert(sizeof(NavFieldCell) == 8, "dumped as it lies");
    Dump(out, "navfield_cells.bin", cells);
    Dump(out, "navfield_paths.i32", paths._paths);
    Dump(out, "navfield_lengths.i32", paths._lengths);
    Dump(out, "navfield_located.i32", at);
    CHECK(Refused([&] { vt.TracePaths({(int)cells.size()}, 4); }));   // a start beyond the spans refuses the whole call
    return 0;
}

// the field of --gpu-navfield; the sight of span i towards span (7 i + 3) mod n and towards each of its links, and every span's smoothed
// path under a cost bound of 0 and under none
static int gpu_navsight_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const NavResult nav = world_nav(vt);
    const std::vector<int> at = vt.LocateOnNav({Vector3(0.0f, 6.3f, 4.0f), Vector3(12.0f, 6.3f, 15.0f)}, 1.0f, 1.0f);
    CHECK(at.size() == 2 && at[0] >= 0 && at[1] >= 0);
    const int n = (int)nav._spans.size();
    std::vector<int> from, to;
    for (int i = 0; i < n; i++) {
        from.push_back(i), to.push_back((int)((7LL * i + 3) % n));
        for (int k = 0; k < 4; k++) from.push_back(i), to.push_back(nav._spans[(size_t)i]._link[k]);   // a missing link is a -1: {-1, 0}
    }
    const std::vector<NavSightHit> hits = vt.NavSight(from, to);   // needs no field
    CHECK(hits.size() == from.size());
    for (size_t i = 0; i < hits.size(); i++) {
        if (to[i] < 0) CHECK(hits[i]._last == -1 && hits[i]._steps == 0);
        else if (i % 5 != 0) CHECK(hits[i]._last == to[i] && hits[i]._steps == 1);   // a linked neighbour is visible in one step
    }
    vt.BuildNavField({NavGoal{at[0], 0u}, NavGoal{at[1], 3000u}}, 2.0f, 0.5f);
    const std::vector<int> starts = all_spans_and_none(nav);
    const NavPaths bound = vt.SmoothPaths(starts, 64, 64, 0u), any = vt.SmoothPaths(starts, 64);
    const NavPaths plain = vt.TracePaths(starts, 64);
    CHECK(bound._lengths.size() == starts.size() && bound._paths.size() == starts.size() * 64 && bound._lengths.back() == 0 && any._lengths.size() == starts.size());
    for (size_t i = 0; i < starts.size(); i++)   // waypoints are spans of the trace
        CHECK(any._lengths[i] <= plain._lengths[i] && bound._lengths[i] <= plain._lengths[i] && any._paths[i * 64] == plain._paths[i * 64]);
    CHECK(vt.LastTriangleCount() == updateTriangles);
    std::printf("navsight: spans %d pairs %zu\n", n, hits.size());
    static_assert(sizeof(NavSightHit) == 8, "dumped as it lies");
    Dump(out, "navsight_hits.bin", hits);
    Dump(out, "navsight_bound_paths.i32", bound._paths);
    Dump(out, "navsight_bound_lengths.i32", bound._lengths);
    Dump(out, "navsight_any_paths.i32", any._paths);
    Dump(out, "navsight_any_lengths.i32", any._lengths);
    CHECK(Refused([&] { vt.SmoothPaths(starts, 64, 0); }));   // a look of 0 refuses the call
    return 0;
}

// two sources in the dug hollow, the lower one joining the higher one's body, and one far outside, flooded in a box that cuts the world
static int gpu_water_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const Vector3 lower(-1.0f, 1.0f, 3.0f), upper(30.0f, 15.0f, 16.5f);
    const std::vector<WaterSource> sources = {WaterSource{Vector3(5.0f, 5.0f, 9.0f), 6.0f}, WaterSource{Vector3(5.0f, 4.5f, 9.5f), 5.5f}, WaterSource{Vector3(500.0f, 6.0f, 10.0f), 7.0f}};
    const WaterResult w = vt.Flood(lower, upper, sources);
    CHECK(w._sourceBody.size() == 3 && w._sourceBody[0] == 0 && w._sourceBody[1] == 0 && w._sourceBody[2] == -1 && w._bodies.size() == 1 && w._bodies[0]._sources == 2);
    long long wet = 0;
    for (const WaterBody &b : w._bodies) wet += b._samples;
    const size_t vn = (size_t)w._volumeDims[0] * w._volumeDims[1] * w._volumeDims[2];
    CHECK(wet == w._wet && w._water.size() == vn && w._bodyVolume.size() == vn && vn != 0);
    for (int k = 0; k < 3; k++) CHECK(w._volumeDims[k] >= w._boxDims[k] && (w._volumeDims[k] - 2) % 8 == 0);
    long long counted = 0;
    for (int v : w._bodyVolume) counted += v >= 0;
    CHECK(counted == wet);
    const std::vector<WaterProbe> probes = vt.ProbeWater({Vector3(5.0f, 4.0f, 9.0f), Vector3(27.5f, 12.0f, 10.0f), Vector3(5.0f, 5.75f, 9.0f)});
    CHECK(probes.size() == 3 && probes[0]._body == 0 && probes[0]._depth == 2.0f && probes[1]._body == -1 && probes[1]._depth == 0.0f && probes[2]._body == 0);
    std::vector<int> probeBody;
    std::vector<float> probeDepth;
    for (const WaterProbe &p : probes) {
        CHECK(p._body < (int)w._bodies.size());
        probeBody.push_back(p._body), probeDepth.push_back(p._depth);
    }
    CHECK(vt.LastTriangleCount() == updateTriangles);
    std::printf("water: bodies %zu wet %lld volume %d x %d x %d\n", w._bodies.size(), w._wet, w._volumeDims[0], w._volumeDims[1], w._volumeDims[2]);
    static_assert(sizeof(WaterBody) == 64, "dumped as it lies");
    Dump(out, "water_source_body.i32", w._sourceBody);
    Dump(out, "water_bodies.bin", w._bodies);
    Dump(out, "water_volume.f32", w._water);
    Dump(out, "water_body_volume.i32", w._bodyVolume);
    Dump(out, "water_probe_body.i32", probeBody);
    Dump(out, "water_probe_depth.f32", probeDepth);
    // a level that is not finite refuses the call and keeps the result
    CHECK(Refused([&] { vt.Flood(lower, upper, {WaterSource{Vector3(5.0f, 6.0f, 9.0f), INFINITY}}); }));
    CHECK(vt.ProbeWater({Vector3(5.0f, 4.0f, 9.0f)})[0]._body == probes[0]._body);
    return 0;
}

// Sky light and three torches -- one in the dug hollow, one in rock, one far outside -- in a box that cuts the world; dumps the volume, the
// lit flags, the info and three probes
static int gpu_light_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const Vector3 lower(-1.0f, 1.0f, 3.0f), upper(30.0f, 15.0f, 16.5f);
    const std::vector<LightSource> torches = {LightSource{Vector3(5.0f, 4.5f, 9.0f), 200}, LightSource{Vector3(5.0f, 2.0f, 9.0f), 255}, LightSource{Vector3(500.0f, 6.0f, 10.0f), 90}};
    const LightResult r = vt.Light(lower, upper, 240, 16, 12, torches);
    CHECK(r._sourceLit.size() == 3 && r._sourceLit[0] == 1 && r._sourceLit[1] == 0 && r._sourceLit[2] == 0);
    const size_t n = (size_t)r._boxDims[0] * r._boxDims[1] * r._boxDims[2];
    CHECK(n != 0 && r._volume.size() == n && r._rounds >= 1 && r._rounds <= 256);
    long long sky = 0, torch = 0;
    int brightest = 0;
    for (const LightSample &s : r._volume) sky += s._sky != 0, torch += s._torch != 0, brightest = s._torch > brightest ? s._torch : brightest;
    CHECK(sky == r._skySamples && torch == r._torchSamples && sky > 0 && torch > 0 && brightest == 200);
    const std::vector<LightSample> probes = vt.ProbeLight({Vector3(5.0f, 4.5f, 9.0f), Vector3(5.0f, 2.0f, 9.0f), Vector3(500.0f, 0.0f, 0.0f), Vector3(5.0f, 14.0f, 9.0f)});
    CHECK(probes.size() == 4 && probes[0]._torch == 200 && probes[1]._sky == 0 && probes[1]._torch == 0 && probes[2]._sky == 0 && probes[2]._torch == 0 && probes[3]._sky == 240);
    CHECK(vt.LastTriangleCount() == updateTriangles);
    std::printf("light: sky %lld torch %lld rounds %d volume %d x %d x %d\n", r._skySamples, r._torchSamples, r._rounds, r._boxDims[0], r._boxDims[1], r._boxDims[2]);
    static_assert(sizeof(LightSample) == 2, "dumped as it lies");
    const std::vector<long long> info = {r._boxLo[0], r._boxLo[1], r._boxLo[2], r._boxDims[0], r._boxDims[1], r._boxDims[2], r._skySamples, r._torchSamples};
    Dump(out, "light_volume.bin", r._volume);
    Dump(out, "light_source_lit.u8", r._sourceLit);
    Dump(out, "light_info.i64", info);
    Dump(out, "light_probes.bin", probes);
    // a level outside 1..255 refuses the call and keeps the result
    CHECK(Refused([&] { vt.Light(lower, upper, 240, 16, 12, {LightSource{Vector3(5.0f, 4.5f, 9.0f), 256}}); }));
    CHECK(Refused([&] { vt.Light(lower, upper, 240, 0, 12, {}); }));
    CHECK(vt.ProbeLight({Vector3(5.0f, 4.5f, 9.0f)})[0]._torch == probes[0]._torch);
    return 0;
}

// An erosion of a box of that terrain in one Update with a dig before it; dumps the grid before and after, the box and the five maps
static int gpu_erosion_run(const std::string &out)
{
    VoxelTerrain vt;
    resident_world(vt);
    Dump(out, "erosion_grid_before.f32", vt.DeviceSamples());
    const Vector3 lower(-1.0f, -50.0f, 3.0f), upper(25.0f, 50.0f, 16.5f);
    vt.InsertModifier(std::make_shared<ErosionModifier>(lower, upper, 24, 0.02f, 0.05f, 1.0f, 0.3f, 0.3f, 0.25f, 0.5f, 0.1f));
    vt.Update();
    const ErosionResult r = vt.ReadErosion();
    const size_t n = (size_t)r._nx * (size_t)r._nz;
    CHECK(n != 0 && r._iterations == 24 && r._nx == r._boxHi[0] - r._boxLo[0] + 1 && r._nz == r._boxHi[2] - r._boxLo[2] + 1);
    CHECK(r._heightBefore.size() == n && r._heightAfter.size() == n && r._water.size() == n && r._sediment.size() == n && r._activeMask.size() == n);
    int active = 0, rewritten = 0;
    for (size_t i = 0; i < n; i++) {
        active += r._activeMask[i] != 0;
        rewritten += r._activeMask[i] && r._heightAfter[i] != r._heightBefore[i];
        if (!r._activeMask[i]) CHECK(r._heightBefore[i] == 0.0f && r._heightAfter[i] == 0.0f && r._water[i] == 0.0f && r._sediment[i] == 0.0f);
    }
    CHECK(active == r._active && rewritten == r._rewritten && active > 0 && rewritten > 0 && r._clamped == 0);
    CHECK(!vt.LastUpdateBlocks().empty() && vt.LastTriangleCount() > 0);
    std::printf("erosion: %d x %d columns, %d active, %d rewritten\n", r._nx, r._nz, r._active, r._rewritten);
    const int box[9] = {r._boxLo[0], r._boxLo[1], r._boxLo[2], r._boxHi[0], r._boxHi[1], r._boxHi[2], r._active, r._rewritten, r._clamped};
    Dump(out, "erosion_box.i32", box, 9);
    Dump(out, "erosion_grid_after.f32", vt.DeviceSamples());
    Dump(out, "erosion_before.f32", r._heightBefore);
    Dump(out, "erosion_after.f32", r._heightAfter);
    Dump(out, "erosion_water.f32", r._water);
    Dump(out, "erosion_sediment.f32", r._sediment);
    Dump(out, "erosion_active.u8", r._activeMask);
    vt.Free();
    CHECK(Refused([&] { vt.ReadErosion(); }));
    return 0;
}

// the field of --gpu-navfield; agents on every second span (those divisible by 7 ask for -1, and span 2 is asked for three times), 24 ticks
// with any detour that leave on arrival, then a field of the second goal alone and 16 ticks within 1024
static int gpu_navcrowd_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const NavResult nav = world_nav(vt);
    const std::vector<int> at = vt.LocateOnNav({Vector3(0.0f, 6.3f, 4.0f), Vector3(12.0f, 6.3f, 15.0f)}, 1.0f, 1.0f);
    CHECK(at.size() == 2 && at[0] >= 0 && at[1] >= 0);
    vt.BuildNavField({NavGoal{at[0], 0u}, NavGoal{at[1], 3000u}}, 2.0f, 0.5f);
    const int n = (int)nav._spans.size();
    std::vector<int> starts;
    for (int s = 0; s < n; s += 2) starts.push_back(s % 7 ? s : -1);
    starts.push_back(2), starts.push_back(2);
    std::vector<unsigned> speeds;
    for (size_t i = 0; i < starts.size(); i++) speeds.push_back(400u + (unsigned)((131 * i) % 1200));
    static_assert(sizeof(CrowdAgent) == 16, "dumped as it lies");
    std::vector<int> info;   // five counts per read, in the order of the reads
    auto dump = [&](const std::string &name) {
        const CrowdResult r = vt.ReadCrowd();
        Dump(out, "navcrowd_" + name + ".bin", r._agents);
        Dump(out, "navcrowd_" + name + "_occupancy.i32", r._occupancy);
        info.insert(info.end(), {(int)r._agents.size(), r._occupying, r._arrived, r._ticks, r._movedLast});
        Dump(out, "navcrowd_info.i32", info);
        return r;
    };
    const int placed = vt.SpawnCrowd(starts, speeds);
    const CrowdResult spawned = dump("spawned");
    CHECK(spawned._agents.size() == starts.size() && (int)spawned._occupancy.size() == n && placed > 0 && placed < (int)starts.size());
    CHECK(spawned._occupying == placed && spawned._ticks == 0);
    CHECK(spawned._agents[0]._state == kCrowdUnplaced && spawned._agents[0]._span == -1);
    CHECK(spawned._agents[1]._state == kCrowdWalking && spawned._occupancy[2] == 1 && spawned._agents.back()._state == kCrowdUnplaced);   // agent 1 asked for span 2 first
    vt.StepCrowd(24, kNavCrowdAnyDetour, true);
    const CrowdResult stepped = dump("stepped");
    CHECK(stepped._ticks == 24 && stepped._arrived > 0 && stepped._occupying + stepped._arrived == placed);   // who arrived has left
    vt.BuildNavField({NavGoal{at[1], 0u}}, 2.0f, 0.5f);   // the re-route keeps the crowd
    vt.StepCrowd(16, 1024u);
    const CrowdResult rerouted = dump("rerouted");
    CHECK(rerouted._ticks == 40 && rerouted._agents.size() == starts.size());
    CHECK(vt.LastTriangleCount() == updateTriangles);
    std::printf("navcrowd: spans %d agents %zu placed %d arrived %d\n", n, starts.size(), placed, rerouted._arrived);
    CHECK(Refused([&] { vt.SpawnCrowd({0}, {0u}); }) && vt.ReadCrowd()._ticks == 40);   // a speed of 0 refuses the call and keeps the crowd
    world_nav(vt);   // a nav build drops it
    CHECK(Refused([&] { vt.ReadCrowd(); }));
    return 0;
}

// the world meshed at mixed levels of detail: the viewer at cell (-1, 3, 5), roots of level 2, split 1
static int gpu_lod_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    const size_t blocksBefore = vt.LastUpdateBlocks().size();
    const int triNum = vt.ExtractLod(Vector3(-3.5f, 2.5f, 4.5f), 2, 1.0f);
    const std::vector<LodNode> &nodes = vt.LodNodes();
    std::printf("lod: nodes %zu triangles %d (full resolution %d)\n", nodes.size(), triNum, updateTriangles);
    CHECK(!nodes.empty() && vt.LodMeshes().size() == nodes.size() && triNum > 0 && triNum < updateTriangles);
    CHECK(vt.LastTriangleCount() == updateTriangles && vt.LastUpdateBlocks().size() == blocksBefore && blocksBefore != 0);
    std::vector<int> records, counts;
    size_t vertices = 0;
    for (size_t i = 0; i < nodes.size(); i++) {
        records.insert(records.end(), {nodes[i]._origin._x, nodes[i]._origin._y, nodes[i]._origin._z, nodes[i]._level});
        const BlockMesh &m = vt.LodMeshes()[i];
        counts.push_back((int)m.vertices.size());
        vertices += m.vertices.size();
        const float size = 8.0f * (float)(1 << nodes[i]._level) * vt._voxelScale;   // a node's mesh stays inside its box
        for (const Vector3 &v : m.vertices) CHECK(v.x >= 0 && v.x <= size && v.y >= 0 && v.y <= size && v.z >= 0 && v.z <= size);
    }
    Dump(out, "lod_nodes.i32", records);
    Dump(out, "lod_counts.i32", counts);
    CHECK(vertices == (size_t)triNum * 3);
    const size_t nodesBefore = nodes.size();
    CHECK(Refused([&] { vt.ExtractLod(Vector3(0, 0, 0), 3); }) && vt.LodNodes().size() == nodesBefore);   // a root of level 3 is 64 cells: it does not divide 32
    vt.Free();
    return 0;
}

// the seams of that mixed-level mesh covered: skirts at depth 1, then on every face, and what is refused
static int gpu_lodskirt_run(const std::string &out)
{
    VoxelTerrain vt;
    const int updateTriangles = resident_world(vt);
    CHECK(Refused([&] { vt.LodSkirts(); }));   // no level-of-detail result yet
    const int triNum = vt.ExtractLod(Vector3(-3.5f, 2.5f, 4.5f), 2, 1.0f);
    const int skirts = vt.LodSkirts(1.0f);
    std::printf("lodskirt: nodes %zu triangles %d skirt triangles %d\n", vt.LodNodes().size(), triNum, skirts);
    CHECK(skirts > 0 && skirts % 2 == 0 && vt.LodSkirtMeshes().size() == vt.LodNodes().size());
    std::vector<int> counts;
    size_t vertices = 0;
    for (size_t i = 0; i < vt.LodNodes().size(); i++) {
        const BlockMesh &m = vt.LodSkirtMeshes()[i];
        counts.push_back((int)m.vertices.size());
        vertices += m.vertices.size();
        const float cell = (float)(1 << vt.LodNodes()[i]._level) * vt._voxelScale, size = 8.0f * cell;   // a skirt leaves its node's box by its depth at the most
        for (const Vector3 &v : m.vertices) CHECK(v.x >= -1.001f * cell && v.x <= size + 1.001f * cell && v.y >= -1.001f * cell && v.y <= size + 1.001f * cell && v.z >= -1.001f * cell && v.z <= size + 1.001f * cell);
    }
    Dump(out, "lodskirt_counts.i32", counts);
    CHECK(vertices == (size_t)skirts * 3);
    CHECK(Refused([&] { vt.LodSkirts(0.0f); }) && Refused([&] { vt.LodSkirts(9.0f); }) && vt.LodSkirtMeshes().size() == counts.size());
    CHECK(vt.LodSkirts(1.0f, true) > skirts);
    CHECK(vt.LastTriangleCount() == updateTriangles);
    vt.Free();
    return 0;
}

// flag, whether it takes an <out_dir>, the run, the token printed after a run that returned 0, and what the run does
static const struct Mode {
    const char *flag;
    bool takesDir;
    int (*run)(const std::string &);
    const char *ok, *what;
} kModes[] = {
    {"--cpu", false, cpu_tests, "HOST-CPU-OK", "host logic only (recording backend, no GPU needed)"},
    {"--gpu", true, gpu_run, "HOST-GPU-OK", "real libvtmc.so backend; dumps grid + meshes for the parity test"},
    {"--gpu-resident", true, gpu_resident_run, "HOST-RESIDENT-OK", "the same scene, grid in HBM, Update on the device; dumps grid + meshes, checks the material layer"},
    {"--gpu-lod", true, gpu_lod_run, "HOST-LOD-OK", "a resident terrain meshed at three levels of detail around a viewer; dumps nodes + per-node counts"},
    {"--gpu-nav", true, gpu_nav_run, "HOST-NAV-OK", "the navigation layer of a box of that terrain; dumps the spans, the column offsets and the box"},
    {"--gpu-naverode", true, gpu_naverode_run, "HOST-NAVERODE-OK", "the agent radius on that build; dumps the distances, then the eroded spans, offsets and origin"},
    {"--gpu-navfield", true, gpu_navfield_run, "HOST-NAVFIELD-OK", "a flow field on that build; dumps the cells, every span's path and the located goal spans"},
    {"--gpu-navsight", true, gpu_navsight_run, "HOST-NAVSIGHT-OK", "any-angle paths on that field; dumps the hits of a set of pairs and every span's smoothed path"},
    {"--gpu-navcrowd", true, gpu_navcrowd_run, "HOST-NAVCROWD-OK", "a crowd on that field; dumps agents, occupancy and counts after the spawn, 24 ticks and a re-route"},
    {"--gpu-water", true, gpu_water_run, "HOST-WATER-OK", "standing water on that terrain; dumps the bodies, both volumes and three probes of one flood"},
    {"--gpu-light", true, gpu_light_run, "HOST-LIGHT-OK", "sky and torch light on that terrain; dumps the volume, the lit flags, the info and four probes of one light call"},
    {"--gpu-erosion", true, gpu_erosion_run, "HOST-EROSION-OK", "an erosion of a box of that terrain; dumps the grid before and after, the box and the five maps"},
    {"--gpu-lodskirt", true, gpu_lodskirt_run, "HOST-LODSKIRT-OK", "the seams of that mixed-level mesh covered by skirts; dumps the per-node vertex counts"},
};

int main(int argc, char **argv)
{
    for (const Mode &m : kModes) {
        if (argc < (m.takesDir ? 3 : 2) || std::strcmp(argv[1], m.flag) != 0) continue;
        try {
            const int rc = m.run(m.takesDir ? argv[2] : "");
            if (rc == 0) std::printf("%s\n", m.ok);
            return rc;
        } catch (const std::exception &e) {
            std::fprintf(stderr, "exception: %s\n", e.what());
            return 3;
        }
    }
    std::fprintf(stderr, "usage: host_selftest <mode>, one of\n");
    for (const Mode &m : kModes) std::fprintf(stderr, "  %s%s  %s\n", m.flag, m.takesDir ? " <out_dir>" : "", m.what);
    return 64;
}
