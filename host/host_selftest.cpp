// host_selftest.cpp -- drives the C++ VoxelTerrain mirror the way TerrainEngine / SceneManager drive
// the C# class (TerrainEngine.cs:87,148,160; SceneManager.cs:121-129).
//   host_selftest --cpu            host logic only (recording backend, no GPU needed)
//   host_selftest --gpu <out_dir>  real libvtmc.so backend; dumps grid + meshes for the parity test
//   host_selftest --gpu-resident <out_dir>  the same scene, grid in HBM, Update on the device
//   host_selftest --gpu-lod <out_dir>  a resident terrain meshed at three levels of detail around a viewer; dumps nodes + per-node counts
//   host_selftest --gpu-nav <out_dir>  the navigation layer of a box of a resident terrain; dumps the spans, the column offsets and the box
//   host_selftest --gpu-naverode <out_dir>  the agent radius on that build: dumps the distances, then the eroded spans, offsets and origin
//   host_selftest --gpu-water <out_dir> | --gpu-navfield <out_dir>  a flow field on that build: dumps the cells, every span's path and the located goal spans
//   host_selftest --gpu-navsight <out_dir>  any-angle paths on that field: dumps the hits of a set of pairs and every span's smoothed path
//   host_selftest --gpu-water <out_dir>     standing water on that world: dumps the bodies, both volumes and three probes of one flood
//   host_selftest --gpu-navcrowd <out_dir>  a crowd on that field: dumps agents, occupancy and counts after the spawn, 24 ticks and a re-route
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

static bool throws_with(VoxelTerrain &vt, const char *needle)
{
    try {
        vt.Init();
    } catch (const UnityException &e) {
        return std::strstr(e.what(), needle) != nullptr;
    }
    return false;
}

static int cpu_tests()
{
    {  // VoxelTerrain.cs:138-142
        VoxelTerrain bad;
        bad.SetBackend(std::make_shared<Recorder>());
        bad._width = 10;
        CHECK(throws_with(bad, "block size must align to terrain size"));
        bad._width = 1032;
        CHECK(throws_with(bad, "too high resolution (exceeds 1025)"));
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
        auto message = [&](const std::vector<Color> &map, int group) -> std::string {
            try {
                vt.SetControlMap(map, group);
            } catch (const UnityException &e) {
                return e.what();
            }
            return "";
        };
        vt._matControlFineness = 1;
        const std::vector<Color> map(16 * 16 * 16);
        CHECK(message(map, 0) == "invalid control map group" && message(map, 3) == "invalid control map group");
        CHECK(message(std::vector<Color>(100), 1) == "invalid control map data size");
        vt._matControlFineness = 2;
        CHECK(message(map, 2) == "invalid control map data size");
        vt._matControlFineness = 1;
        CHECK(message(map, 1).find("device-resident") != std::string::npos);   // this terrain keeps its samples on the host
        bool refused = false;
        try {
            MaterialStroke(Vector3(0, 0, 0), -1.0f, 0);
        } catch (const std::invalid_argument &) {
            refused = true;
        }
        CHECK(refused);
    }
    return 0;
}

static int gpu_run(const std::string &out)
{
    VoxelTerrain vt;
    vt._width = 64;
    vt._elevation = 32;
    vt._height = 64;
    vt._voxelScale = 0.5f;
    vt.TerrainOrigin = Vector3(-3.0f, 1.0f, 2.0f);
    vt.SeedRandom(7);
    vt.Init();
    Vector2 lo, up;
    lo.x = -100; lo.y = -100; up.x = 100; up.y = 100;
    vt.InsertModifier(std::make_shared<PlaneModifier>(6.3f, lo, up, true));
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(10.0f, 8.0f, 15.0f), 5.5f, true));
    vt.InsertModifier(std::make_shared<CylinderModifier>(Vector3(2.0f, 5.0f, 6.0f), Vector3(1.0f, 0.3f, 0.5f), 20.0f, 2.2f, false));
    vt.Update();
    std::printf("blocks %zu triangles %d\n", vt.LastUpdateBlocks().size(), vt.LastTriangleCount());

    std::ofstream(out + "/grid.f32", std::ios::binary)
        .write(reinterpret_cast<const char *>(vt.Samples().data()), (std::streamsize)(vt.Samples().size() * sizeof(float)));
    std::ofstream fb(out + "/blocks.i32", std::ios::binary), fv(out + "/vertices.f32", std::ios::binary),
        fn(out + "/normals.f32", std::ios::binary), fc(out + "/counts.i32", std::ios::binary);
    for (const Int3 &b : vt.LastUpdateBlocks()) {
        int xyz[3] = {b._x, b._y, b._z};
        fb.write(reinterpret_cast<const char *>(xyz), sizeof xyz);
        const BlockMesh &m = vt.Block(b._x, b._y, b._z);
        int n = (int)m.vertices.size();
        fc.write(reinterpret_cast<const char *>(&n), sizeof n);
        for (int i = 0; i < n; i++) {
            if (m.triangles[(size_t)i] != i) return 2;
            fv.write(reinterpret_cast<const char *>(&m.vertices[(size_t)i]), 12);
            fn.write(reinterpret_cast<const char *>(&m.normals[(size_t)i]), 12);
        }
    }
    // an edit like SceneManager.Update's mouse sphere (SceneManager.cs:121-129): small dirty set
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(5.0f, 4.0f, 9.0f), 2.0f, false));
    vt.Update();
    std::printf("edit: blocks %zu triangles %d\n", vt.LastUpdateBlocks().size(), vt.LastTriangleCount());
    vt.Free();
    std::printf("HOST-GPU-OK\n");
    return 0;
}

// the same scene with the grid resident in HBM and Update's density write on the GPU
static int gpu_resident_run(const std::string &out)
{
    VoxelTerrain vt;
    vt._width = 64;
    vt._elevation = 32;
    vt._height = 64;
    vt._voxelScale = 0.5f;
    vt.TerrainOrigin = Vector3(-3.0f, 1.0f, 2.0f);
    vt._deviceResident = true;
    vt._seed = 4242;
    vt.Init();
    Vector2 lo, up;
    lo.x = -100; lo.y = -100; up.x = 100; up.y = 100;
    vt.InsertModifier(std::make_shared<PlaneModifier>(6.3f, lo, up, true));
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(10.0f, 8.0f, 15.0f), 5.5f, true));
    vt.InsertModifier(std::make_shared<CylinderModifier>(Vector3(2.0f, 5.0f, 6.0f), Vector3(1.0f, 0.3f, 0.5f), 20.0f, 2.2f, false));
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
    const std::vector<float> grid = vt.DeviceSamples();
    std::ofstream(out + "/r_grid.f32", std::ios::binary).write(reinterpret_cast<const char *>(grid.data()), (std::streamsize)(grid.size() * sizeof(float)));
    std::ofstream fb(out + "/r_blocks.i32", std::ios::binary), fv(out + "/r_vertices.f32", std::ios::binary),
        fn(out + "/r_normals.f32", std::ios::binary), fc(out + "/r_counts.i32", std::ios::binary);
    for (const Int3 &b : vt.LastUpdateBlocks()) {
        int xyz[3] = {b._x, b._y, b._z};
        fb.write(reinterpret_cast<const char *>(xyz), sizeof xyz);
        const BlockMesh &m = vt.Block(b._x, b._y, b._z);
        int n = (int)m.vertices.size();
        fc.write(reinterpret_cast<const char *>(&n), sizeof n);
        for (int i = 0; i < n; i++) {
            fv.write(reinterpret_cast<const char *>(&m.vertices[(size_t)i]), 12);
            fn.write(reinterpret_cast<const char *>(&m.normals[(size_t)i]), 12);
        }
    }
    {   // the material layer: a control map, a stroke, and the weights of the edit's vertices
        vt._matControlFineness = 1;
        std::vector<Color> map(16 * 16 * 16);
        for (Color &c : map) c.g = 1.0f;                                  // all grass: channel 1
        vt.SetControlMap(map, 1);
        vt.Paint({MaterialStroke(Vector3(5.0f, 4.0f, 9.0f), 6.0f, 2)});   // rock around the dig: channel 2
        const std::vector<uint8_t> &w = vt.VertexMaterials();
        if (w.size() != (size_t)vt.LastTriangleCount() * 3 * 8) return 4;
        size_t rock = 0;
        for (size_t v = 0; v < w.size(); v += 8) {
            if (w[v] != 0 || w[v + 3] != 0 || w[v + 4] != 0) return 5;    // only channels 1 and 2 were ever set
            rock += w[v + 2] > w[v + 1];
        }
        std::printf("resident materials: %zu vertices, %zu mostly rock\n", w.size() / 8, rock);
        if (rock == 0) return 6;
    }
    vt.Free();
    std::printf("HOST-RESIDENT-OK\n");
    return 0;
}

// a device-resident terrain of 64 x 32 x 32 cells meshed at mixed levels of detail: the viewer at cell (-1, 3, 5), roots of level 2, split 1
static int gpu_nav_run(const std::string &out)
{
    VoxelTerrain vt;
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
    const int updateTriangles = vt.LastTriangleCount();
    // an agent 0.9 world units high (2 samples) that steps 0.4 (0.8 grid units), in a box around the dig
    const NavResult nav = vt.BuildNav(Vector3(-1.0f, 1.0f, 3.0f), Vector3(14.0f, 15.0f, 16.5f), 0.9f, 0.4f);
    std::printf("nav: spans %zu columns %zu box %d %d %d + %d %d %d\n", nav._spans.size(), nav._columnOffsets.size() - 1, nav._boxLo._x, nav._boxLo._y,
                nav._boxLo._z, nav._boxDims._x, nav._boxDims._y, nav._boxDims._z);
    if (nav._spans.empty() || nav._columnOffsets.size() != (size_t)nav._boxDims._x * nav._boxDims._z + 1) return 7;
    if (nav._columnOffsets.back() != (int)nav._spans.size() || vt.LastTriangleCount() != updateTriangles) return 8;   // what Update left stands
    static_assert(sizeof(NavSpan) == 32, "dumped as it lies");
    std::ofstream fs(out + "/nav_spans.bin", std::ios::binary), fo(out + "/nav_offsets.i32", std::ios::binary), fb(out + "/nav_box.i32", std::ios::binary);
    fs.write(reinterpret_cast<const char *>(nav._spans.data()), (std::streamsize)(nav._spans.size() * sizeof(NavSpan)));
    fo.write(reinterpret_cast<const char *>(nav._columnOffsets.data()), (std::streamsize)(nav._columnOffsets.size() * sizeof(int)));
    const int box[6] = {nav._boxLo._x, nav._boxLo._y, nav._boxLo._z, nav._boxDims._x, nav._boxDims._y, nav._boxDims._z};
    fb.write(reinterpret_cast<const char *>(box), sizeof box);
    bool refused = false;   // 200 world units of headroom are 400 samples: more than the layer takes
    try {
        vt.BuildNav(Vector3(0, 0, 0), Vector3(1, 1, 1), 200.0f, 0.4f);
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused) return 9;
    std::printf("HOST-NAV-OK\n");
    return 0;
}

// the world of --gpu-nav and its box; the distances of an agent 1.2 world units wide (3 columns), then the erosion by 0.8 (2 columns)
// with the box's faces open
static int gpu_naverode_run(const std::string &out)
{
    VoxelTerrain vt;
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
    const int updateTriangles = vt.LastTriangleCount();
    const NavResult nav = vt.BuildNav(Vector3(-1.0f, 1.0f, 3.0f), Vector3(14.0f, 15.0f, 16.5f), 0.9f, 0.4f);
    const std::vector<int> dist = vt.NavDistance(1.2f);
    if (dist.size() != nav._spans.size() || !nav._origin.empty()) return 7;
    const NavResult eroded = vt.ErodeNav(0.8f, true);
    std::printf("naverode: spans %zu kept %zu\n", nav._spans.size(), eroded._spans.size());
    if (eroded._spans.empty() || eroded._spans.size() >= nav._spans.size() || eroded._origin.size() != eroded._spans.size()) return 8;
    if (eroded._columnOffsets.size() != nav._columnOffsets.size() || eroded._columnOffsets.back() != (int)eroded._spans.size()) return 9;
    if (eroded._boxLo._x != nav._boxLo._x || eroded._boxDims._z != nav._boxDims._z || vt.LastTriangleCount() != updateTriangles) return 10;   // what Update left stands
    for (size_t i = 0; i < eroded._spans.size(); i++) {
        const int o = eroded._origin[i];
        if (o < 0 || o >= (int)nav._spans.size() || (i > 0 && o <= eroded._origin[i - 1]) || eroded._spans[i]._y != nav._spans[(size_t)o]._y) return 11;
    }
    std::ofstream fd(out + "/naverode_distance.i32", std::ios::binary), fs(out + "/naverode_spans.bin", std::ios::binary),
        fo(out + "/naverode_offsets.i32", std::ios::binary), fg(out + "/naverode_origin.i32", std::ios::binary);
    fd.write(reinterpret_cast<const char *>(dist.data()), (std::streamsize)(dist.size() * sizeof(int)));
    fs.write(reinterpret_cast<const char *>(eroded._spans.data()), (std::streamsize)(eroded._spans.size() * sizeof(NavSpan)));
    fo.write(reinterpret_cast<const char *>(eroded._columnOffsets.data()), (std::streamsize)(eroded._columnOffsets.size() * sizeof(int)));
    fg.write(reinterpret_cast<const char *>(eroded._origin.data()), (std::streamsize)(eroded._origin.size() * sizeof(int)));
    bool refused = false;   // 200 world units are 400 columns: more than the layer takes
    try {
        vt.ErodeNav(200.0f);
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused) return 12;
    std::printf("HOST-NAVERODE-OK\n");
    return 0;
}

// the world of --gpu-nav and its box; a field towards two goals found by position, then every span's path
static int gpu_navfield_run(const std::string &out)
{
    VoxelTerrain vt;
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
    const int updateTriangles = vt.LastTriangleCount();
    const NavResult nav = vt.BuildNav(Vector3(-1.0f, 1.0f, 3.0f), Vector3(14.0f, 15.0f, 16.5f), 0.9f, 0.4f);
    // two agents' worth of goals by position: on the plane (height 6.3) near a corner of the box, and further along it; 1 world unit either way
    const std::vector<int> at = vt.LocateOnNav({Vector3(0.0f, 6.3f, 4.0f), Vector3(12.0f, 6.3f, 15.0f), Vector3(500.0f, 6.3f, 4.0f)}, 1.0f, 1.0f);
    if (at.size() != 3 || at[0] < 0 || at[1] < 0 || at[2] != -1) return 7;
    const std::vector<NavFieldCell> cells = vt.BuildNavField({NavGoal{at[0], 0u}, NavGoal{at[1], 3000u}}, 2.0f, 0.5f);
    if (cells.size() != nav._spans.size() || cells[(size_t)at[0]]._cost != 0u || cells[(size_t)at[0]]._next != -1) return 8;
    std::vector<int> starts(nav._spans.size());
    for (size_t i = 0; i < starts.size(); i++) starts[i] = (int)i;
    starts.push_back(-1);
    const NavPaths paths = vt.TracePaths(starts, 64);
    if (paths._lengths.size() != starts.size() || paths._paths.size() != starts.size() * 64 || paths._lengths.back() != 0) return 9;
    if (vt.LastTriangleCount() != updateTriangles) return 10;   // what Update left stands
    std::printf("navfield: spans %zu goals %d %d\n", cells.size(), at[0], at[1]);
    static_assert(sizeof(NavFieldCell) == 8, "dumped as it lies");
    std::ofstream fc(out + "/navfield_cells.bin", std::ios::binary), fp(out + "/navfield_paths.i32", std::ios::binary),
        fl(out + "/navfield_lengths.i32", std::ios::binary), fa(out + "/navfield_located.i32", std::ios::binary);
    fc.write(reinterpret_cast<const char *>(cells.data()), (std::streamsize)(cells.size() * sizeof(NavFieldCell)));
    fp.write(reinterpret_cast<const char *>(paths._paths.data()), (std::streamsize)(paths._paths.size() * sizeof(int)));
    fl.write(reinterpret_cast<const char *>(paths._lengths.data()), (std::streamsize)(paths._lengths.size() * sizeof(int)));
    fa.write(reinterpret_cast<const char *>(at.data()), (std::streamsize)(at.size() * sizeof(int)));
    bool refused = false;   // a start beyond the spans refuses the whole call
    try {
        vt.TracePaths({(int)cells.size()}, 4);
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused) return 11;
    std::printf("HOST-NAVFIELD-OK\n");
    return 0;
}

// the world, the box and the field of --gpu-navfield; the sight of span i towards span (7 i + 3) mod n and towards each of its links, and
// every span's smoothed path under a cost bound of 0 and under none
static int gpu_navsight_run(const std::string &out)
{
    VoxelTerrain vt;
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
    const int updateTriangles = vt.LastTriangleCount();
    const NavResult nav = vt.BuildNav(Vector3(-1.0f, 1.0f, 3.0f), Vector3(14.0f, 15.0f, 16.5f), 0.9f, 0.4f);
    const std::vector<int> at = vt.LocateOnNav({Vector3(0.0f, 6.3f, 4.0f), Vector3(12.0f, 6.3f, 15.0f)}, 1.0f, 1.0f);
    if (at.size() != 2 || at[0] < 0 || at[1] < 0) return 7;
    const int n = (int)nav._spans.size();
    std::vector<int> from, to;
    for (int i = 0; i < n; i++) {
        from.push_back(i), to.push_back((int)((7LL * i + 3) % n));
        for (int k = 0; k < 4; k++) from.push_back(i), to.push_back(nav._spans[(size_t)i]._link[k]);   // a missing link is a -1: {-1, 0}
    }
    const std::vector<NavSightHit> hits = vt.NavSight(from, to);   // needs no field
    if (hits.size() != from.size()) return 8;
    for (size_t i = 0; i < hits.size(); i++)
        if (to[i] < 0 ? hits[i]._last != -1 || hits[i]._steps != 0 : i % 5 != 0 && (hits[i]._last != to[i] || hits[i]._steps != 1)) return 9;   // a linked neighbour is visible in one step
    vt.BuildNavField({NavGoal{at[0], 0u}, NavGoal{at[1], 3000u}}, 2.0f, 0.5f);
    std::vector<int> starts(nav._spans.size());
    for (size_t i = 0; i < starts.size(); i++) starts[i] = (int)i;
    starts.push_back(-1);
    const NavPaths bound = vt.SmoothPaths(starts, 64, 64, 0u), any = vt.SmoothPaths(starts, 64);
    const NavPaths plain = vt.TracePaths(starts, 64);
    if (bound._lengths.size() != starts.size() || bound._paths.size() != starts.size() * 64 || bound._lengths.back() != 0 || any._lengths.size() != starts.size()) return 10;
    for (size_t i = 0; i < starts.size(); i++)
        if (any._lengths[i] > plain._lengths[i] || bound._lengths[i] > plain._lengths[i] || any._paths[i * 64] != plain._paths[i * 64]) return 11;   // waypoints are spans of the trace
    if (vt.LastTriangleCount() != updateTriangles) return 12;   // what Update left stands
    std::printf("navsight: spans %d pairs %zu\n", n, hits.size());
    static_assert(sizeof(NavSightHit) == 8, "dumped as it lies");
    std::ofstream fh(out + "/navsight_hits.bin", std::ios::binary), fb(out + "/navsight_bound_paths.i32", std::ios::binary),
        fbl(out + "/navsight_bound_lengths.i32", std::ios::binary), fa(out + "/navsight_any_paths.i32", std::ios::binary),
        fal(out + "/navsight_any_lengths.i32", std::ios::binary);
    fh.write(reinterpret_cast<const char *>(hits.data()), (std::streamsize)(hits.size() * sizeof(NavSightHit)));
    fb.write(reinterpret_cast<const char *>(bound._paths.data()), (std::streamsize)(bound._paths.size() * sizeof(int)));
    fbl.write(reinterpret_cast<const char *>(bound._lengths.data()), (std::streamsize)(bound._lengths.size() * sizeof(int)));
    fa.write(reinterpret_cast<const char *>(any._paths.data()), (std::streamsize)(any._paths.size() * sizeof(int)));
    fal.write(reinterpret_cast<const char *>(any._lengths.data()), (std::streamsize)(any._lengths.size() * sizeof(int)));
    bool refused = false;   // a look of 0 refuses the call
    try {
        vt.SmoothPaths(starts, 64, 0);
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused) return 13;
    std::printf("HOST-NAVSIGHT-OK\n");
    return 0;
}

// the world of --gpu-navfield; two sources in the dug hollow, the lower one joining the higher one's body, and one far outside, flooded in a
// box that cuts the world
static int gpu_water_run(const std::string &out)
{
    VoxelTerrain vt;
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
    const int updateTriangles = vt.LastTriangleCount();
    const std::vector<WaterSource> sources = {WaterSource{Vector3(5.0f, 5.0f, 9.0f), 6.0f}, WaterSource{Vector3(5.0f, 4.5f, 9.5f), 5.5f}, WaterSource{Vector3(500.0f, 6.0f, 10.0f), 7.0f}};
    const WaterResult w = vt.Flood(Vector3(-1.0f, 1.0f, 3.0f), Vector3(30.0f, 15.0f, 16.5f), sources);
    if (w._sourceBody.size() != 3 || w._sourceBody[0] != 0 || w._sourceBody[1] != 0 || w._sourceBody[2] != -1 || w._bodies.size() != 1 || w._bodies[0]._sources != 2) return 7;
    long long wet = 0;
    for (const WaterBody &b : w._bodies) wet += b._samples;
    const size_t vn = (size_t)w._volumeDims[0] * w._volumeDims[1] * w._volumeDims[2];
    if (wet != w._wet || w._water.size() != vn || w._bodyVolume.size() != vn || vn == 0) return 8;
    for (int k = 0; k < 3; k++)
        if (w._volumeDims[k] < w._boxDims[k] || (w._volumeDims[k] - 2) % 8 != 0) return 9;
    long long counted = 0;
    for (int v : w._bodyVolume) counted += v >= 0;
    if (counted != wet) return 10;
    const std::vector<WaterProbe> probes = vt.ProbeWater({Vector3(5.0f, 4.0f, 9.0f), Vector3(27.5f, 12.0f, 10.0f), Vector3(5.0f, 5.75f, 9.0f)});
    if (probes.size() != 3 || probes[0]._body != 0 || probes[0]._depth != 2.0f || probes[1]._body != -1 || probes[1]._depth != 0.0f || probes[2]._body != 0) return 11;
    for (const WaterProbe &p : probes)
        if (p._body >= (int)w._bodies.size()) return 12;
    if (vt.LastTriangleCount() != updateTriangles) return 13;   // what Update left stands
    std::printf("water: bodies %zu wet %lld volume %d x %d x %d\n", w._bodies.size(), w._wet, w._volumeDims[0], w._volumeDims[1], w._volumeDims[2]);
    static_assert(sizeof(WaterBody) == 64, "dumped as it lies");
    std::ofstream fs(out + "/water_source_body.i32", std::ios::binary), fb(out + "/water_bodies.bin", std::ios::binary), fw(out + "/water_volume.f32", std::ios::binary),
        fv(out + "/water_body_volume.i32", std::ios::binary), fpb(out + "/water_probe_body.i32", std::ios::binary), fpd(out + "/water_probe_depth.f32", std::ios::binary);
    fs.write(reinterpret_cast<const char *>(w._sourceBody.data()), (std::streamsize)(w._sourceBody.size() * sizeof(int)));
    fb.write(reinterpret_cast<const char *>(w._bodies.data()), (std::streamsize)(w._bodies.size() * sizeof(WaterBody)));
    fw.write(reinterpret_cast<const char *>(w._water.data()), (std::streamsize)(vn * sizeof(float)));
    fv.write(reinterpret_cast<const char *>(w._bodyVolume.data()), (std::streamsize)(vn * sizeof(int)));
    for (const WaterProbe &p : probes) {
        fpb.write(reinterpret_cast<const char *>(&p._body), sizeof(int));
        fpd.write(reinterpret_cast<const char *>(&p._depth), sizeof(float));
    }
    bool refused = false;   // a level that is not finite refuses the call and keeps the result
    try {
        vt.Flood(Vector3(-1.0f, 1.0f, 3.0f), Vector3(30.0f, 15.0f, 16.5f), {WaterSource{Vector3(5.0f, 6.0f, 9.0f), INFINITY}});
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused || vt.ProbeWater({Vector3(5.0f, 4.0f, 9.0f)})[0]._body != probes[0]._body) return 14;
    std::printf("HOST-WATER-OK\n");
    return 0;
}

// the world, the box and the field of --gpu-navfield; agents on every second span (those divisible by 7 ask for -1, and span 2 is asked
// for three times), 24 ticks with any detour that leave on arrival, then a field of the second goal alone and 16 ticks within 1024
static int gpu_navcrowd_run(const std::string &out)
{
    VoxelTerrain vt;
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
    const int updateTriangles = vt.LastTriangleCount();
    const NavResult nav = vt.BuildNav(Vector3(-1.0f, 1.0f, 3.0f), Vector3(14.0f, 15.0f, 16.5f), 0.9f, 0.4f);
    const std::vector<int> at = vt.LocateOnNav({Vector3(0.0f, 6.3f, 4.0f), Vector3(12.0f, 6.3f, 15.0f)}, 1.0f, 1.0f);
    if (at.size() != 2 || at[0] < 0 || at[1] < 0) return 7;
    vt.BuildNavField({NavGoal{at[0], 0u}, NavGoal{at[1], 3000u}}, 2.0f, 0.5f);
    const int n = (int)nav._spans.size();
    std::vector<int> starts;
    for (int s = 0; s < n; s += 2) starts.push_back(s % 7 ? s : -1);
    starts.push_back(2), starts.push_back(2);
    std::vector<unsigned> speeds;
    for (size_t i = 0; i < starts.size(); i++) speeds.push_back(400u + (unsigned)((131 * i) % 1200));
    static_assert(sizeof(CrowdAgent) == 16, "dumped as it lies");
    std::ofstream fi(out + "/navcrowd_info.i32", std::ios::binary);
    auto dump = [&](const char *name) {
        const CrowdResult r = vt.ReadCrowd();
        std::ofstream fa(out + "/navcrowd_" + name + ".bin", std::ios::binary), fo(out + "/navcrowd_" + name + "_occupancy.i32", std::ios::binary);
        fa.write(reinterpret_cast<const char *>(r._agents.data()), (std::streamsize)(r._agents.size() * sizeof(CrowdAgent)));
        fo.write(reinterpret_cast<const char *>(r._occupancy.data()), (std::streamsize)(r._occupancy.size() * sizeof(int)));
        const int info[5] = {(int)r._agents.size(), r._occupying, r._arrived, r._ticks, r._movedLast};
        fi.write(reinterpret_cast<const char *>(info), sizeof info);
        return r;
    };
    const int placed = vt.SpawnCrowd(starts, speeds);
    const CrowdResult spawned = dump("spawned");
    if (spawned._agents.size() != starts.size() || (int)spawned._occupancy.size() != n || placed <= 0 || placed >= (int)starts.size() || spawned._occupying != placed ||
        spawned._ticks != 0)
        return 8;
    if (spawned._agents[0]._state != kCrowdUnplaced || spawned._agents[0]._span != -1 || spawned._agents[1]._state != kCrowdWalking || spawned._occupancy[2] != 1 ||
        spawned._agents.back()._state != kCrowdUnplaced)
        return 9;   // agent 1 asked for span 2 first
    vt.StepCrowd(24, kNavCrowdAnyDetour, true);
    const CrowdResult stepped = dump("stepped");
    if (stepped._ticks != 24 || stepped._arrived <= 0 || stepped._occupying + stepped._arrived != placed) return 10;   // who arrived has left
    vt.BuildNavField({NavGoal{at[1], 0u}}, 2.0f, 0.5f);   // the re-route keeps the crowd
    vt.StepCrowd(16, 1024u);
    const CrowdResult rerouted = dump("rerouted");
    if (rerouted._ticks != 40 || rerouted._agents.size() != starts.size()) return 11;
    if (vt.LastTriangleCount() != updateTriangles) return 12;   // what Update left stands
    std::printf("navcrowd: spans %d agents %zu placed %d arrived %d\n", n, starts.size(), placed, rerouted._arrived);
    bool refused = false;   // a speed of 0 refuses the call and keeps the crowd
    try {
        vt.SpawnCrowd({0}, {0u});
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused || vt.ReadCrowd()._ticks != 40) return 13;
    vt.BuildNav(Vector3(-1.0f, 1.0f, 3.0f), Vector3(14.0f, 15.0f, 16.5f), 0.9f, 0.4f);   // a nav build drops it
    refused = false;
    try {
        vt.ReadCrowd();
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused) return 14;
    std::printf("HOST-NAVCROWD-OK\n");
    return 0;
}

static int gpu_lod_run(const std::string &out)
{
    VoxelTerrain vt;
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
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(27.5f, 8.0f, 10.0f), 4.25f, true));   // crosses the terrain's upper x face
    vt.InsertModifier(std::make_shared<SphereModifier>(Vector3(5.0f, 6.0f, 9.0f), 3.0f, false));
    vt.Update();
    const int updateTriangles = vt.LastTriangleCount();
    const size_t blocksBefore = vt.LastUpdateBlocks().size();
    const int triNum = vt.ExtractLod(Vector3(-3.5f, 2.5f, 4.5f), 2, 1.0f);
    const std::vector<LodNode> &nodes = vt.LodNodes();
    std::printf("lod: nodes %zu triangles %d (full resolution %d)\n", nodes.size(), triNum, updateTriangles);
    if (nodes.empty() || vt.LodMeshes().size() != nodes.size() || triNum <= 0 || triNum >= updateTriangles) return 7;
    const size_t updateBlocks = vt.LastUpdateBlocks().size();
    if (vt.LastTriangleCount() != updateTriangles || updateBlocks != blocksBefore || updateBlocks == 0) return 8;   // what Update left stands
    std::ofstream fnodes(out + "/lod_nodes.i32", std::ios::binary), fc(out + "/lod_counts.i32", std::ios::binary);
    size_t vertices = 0;
    for (size_t i = 0; i < nodes.size(); i++) {
        const int rec[4] = {nodes[i]._origin._x, nodes[i]._origin._y, nodes[i]._origin._z, nodes[i]._level};
        fnodes.write(reinterpret_cast<const char *>(rec), sizeof rec);
        const BlockMesh &m = vt.LodMeshes()[i];
        const int n = (int)m.vertices.size();
        fc.write(reinterpret_cast<const char *>(&n), sizeof n);
        vertices += m.vertices.size();
        const float size = 8.0f * (float)(1 << nodes[i]._level) * vt._voxelScale;   // a node's mesh stays inside its box
        for (const Vector3 &v : m.vertices)
            if (!(v.x >= 0 && v.x <= size && v.y >= 0 && v.y <= size && v.z >= 0 && v.z <= size)) return 9;
    }
    if (vertices != (size_t)triNum * 3) return 10;
    bool refused = false;   // a root of level 3 is 64 cells: it does not divide 32
    try {
        vt.ExtractLod(Vector3(0, 0, 0), 3);
    } catch (const UnityException &) {
        refused = true;
    }
    if (!refused || vt.LodNodes().size() != nodes.size()) return 11;
    vt.Free();
    std::printf("HOST-LOD-OK\n");
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc >= 2 && std::string(argv[1]) == "--cpu") {
            int rc = cpu_tests();
            if (rc == 0) std::printf("HOST-CPU-OK\n");
            return rc;
        }
        if (argc >= 3 && std::string(argv[1]) == "--gpu") return gpu_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-resident") return gpu_resident_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-lod") return gpu_lod_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-nav") return gpu_nav_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-naverode") return gpu_naverode_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-navfield") return gpu_navfield_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-navsight") return gpu_navsight_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-navcrowd") return gpu_navcrowd_run(argv[2]);
        if (argc >= 3 && std::string(argv[1]) == "--gpu-water") return gpu_water_run(argv[2]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    std::fprintf(stderr, "usage: host_selftest --cpu | --gpu <out_dir> | --gpu-resident <out_dir> | --gpu-lod <out_dir> | --gpu-nav <out_dir> | --gpu-naverode <out_dir> | --gpu-navfield <out_dir> | --gpu-navsight <out_dir> | --gpu-navcrowd <out_dir>\n");
    return 64;
}
