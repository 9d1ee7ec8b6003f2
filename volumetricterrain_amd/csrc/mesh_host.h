// mesh_host.h -- the host half of vtmc_stamp_from_mesh (stamp_mesh.hip): the closed-mesh check and the records the kernel reads
// (vertices, canonical edges, the double normal, and the bounds a workgroup prunes with).  Plain C++ with no device code and no HIP
// header, so a stand-alone program compiles it for the CPU (tools/mesh_host_check.cpp runs it under the host sanitizers).
// The arithmetic here is part of the rule of include/vtmc.h: FP32 and FP64, one IEEE operation per step (-ffp-contract=off).
#ifndef VTMC_MESH_HOST_H
#define VTMC_MESH_HOST_H
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vtmc {

constexpr int kMeshChunk = 256;  // triangles a workgroup tests at a time: one per thread

// Every undirected index pair of the triangles that repeat no index must be used by exactly two of them.  Returns true for a closed
// mesh; else `edge` names the first offending pair in (triangle, edge) order and `uses` how many triangles use it.
inline bool mesh_closed(const int32_t *idx, int32_t n_tri, int32_t edge[2], int32_t *uses)
{
    auto key = [](int32_t a, int32_t b) { return ((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b); };
    auto degenerate = [](const int32_t *t) { return t[0] == t[1] || t[1] == t[2] || t[2] == t[0]; };
    std::vector<uint64_t> keys;
    keys.reserve((size_t)3 * n_tri);
    for (int32_t t = 0; t < n_tri; ++t) {
        const int32_t *v = idx + (size_t)3 * t;
        if (degenerate(v)) continue;
        for (int e = 0; e < 3; ++e) keys.push_back(key(v[e], v[(e + 1) % 3]));
    }
    std::sort(keys.begin(), keys.end());
    for (int32_t t = 0; t < n_tri; ++t) {
        const int32_t *v = idx + (size_t)3 * t;
        if (degenerate(v)) continue;
        for (int e = 0; e < 3; ++e) {
            const auto r = std::equal_range(keys.begin(), keys.end(), key(v[e], v[(e + 1) % 3]));
            if (r.second - r.first != 2) {
                edge[0] = std::min(v[e], v[(e + 1) % 3]);
                edge[1] = std::max(v[e], v[(e + 1) % 3]);
                *uses = (int32_t)(r.second - r.first);
                return false;
            }
        }
    }
    return true;
}

// The device records of a checked mesh, each array n (or n_chunks) entries long:
//   vert   3 float4 per triangle: (v0, 0), (v1, 0), (v2, 0), its vertices in ascending order of (x, then y, then z)
//   edge   3 float4 per triangle: its edges (v0 v1), (v1 v2), (v2 v0) with the end points in canonical order, (lo.y, lo.z, hi.y, hi.z)
//   bound  2 float4 per triangle: (min.x, min.y, min.z, 0), (max.x, max.y, max.z, 0) over its vertices
//   chunk  2 float4 per chunk of kMeshChunk triangles: the union of its triangles' bounds
//   normal 3 doubles per triangle: cross(v1 - v0, v2 - v0) in double
// and `grow`, the reach of the distance part: 3h + slack.
struct MeshRecords {
    std::vector<float> f;   // vert, edge, bound, chunk back to back
    std::vector<double> n;  // normal
    float grow = 0.0f;
    int n_tri = 0, n_chunks = 0;
    size_t vert_at() const { return 0; }
    size_t edge_at() const { return (size_t)12 * n_tri; }
    size_t bound_at() const { return (size_t)24 * n_tri; }
    size_t chunk_at() const { return (size_t)32 * n_tri; }
};

// lo <= hi by (z, then y) of the coordinate values: both triangles at a shared edge order its end points alike
inline bool mesh_edge_swapped(const float *a, const float *b) { return b[2] < a[2] || (b[2] == a[2] && b[1] < a[1]); }

inline MeshRecords mesh_records(const float *pos, const int32_t *idx, int32_t n_tri, const float first[3], float h, const int32_t dims[3])
{
    MeshRecords r;
    r.n_tri = n_tri;
    r.n_chunks = (n_tri + kMeshChunk - 1) / kMeshChunk;
    r.f.assign((size_t)32 * n_tri + (size_t)8 * r.n_chunks, 0.0f);
    r.n.assign((size_t)3 * n_tri, 0.0);
    float *vert = r.f.data() + r.vert_at(), *edge = r.f.data() + r.edge_at(), *bound = r.f.data() + r.bound_at(), *chunk = r.f.data() + r.chunk_at();
    for (int c = 0; c < r.n_chunks; ++c)
        for (int k = 0; k < 3; ++k) chunk[8 * c + k] = INFINITY, chunk[8 * c + 4 + k] = -INFINITY;
    float reach = h;  // the largest |coordinate| of the stamp's corner samples and of the referenced vertices, and h
    for (int k = 0; k < 3; ++k) reach = std::max({reach, std::fabs(first[k]), std::fabs((float)(dims[k] - 1) * h + first[k])});
    for (int32_t t = 0; t < n_tri; ++t) {
        const float *v[3] = {pos + (size_t)3 * idx[3 * (size_t)t], pos + (size_t)3 * idx[3 * (size_t)t + 1], pos + (size_t)3 * idx[3 * (size_t)t + 2]};
        // v0, v1, v2 of the rule: ascending by (x, then y, then z), so the order the mesh names a triangle's vertices in changes no bit
        std::sort(v, v + 3, [](const float *a, const float *b) { return a[0] != b[0] ? a[0] < b[0] : (a[1] != b[1] ? a[1] < b[1] : a[2] < b[2]); });
        float *b = bound + (size_t)8 * t, *cb = chunk + 8 * (t / kMeshChunk);
        for (int k = 0; k < 3; ++k) {
            for (int i = 0; i < 3; ++i) vert[(size_t)12 * t + 4 * i + k] = v[i][k];
            b[k] = std::min({v[0][k], v[1][k], v[2][k]});
            b[4 + k] = std::max({v[0][k], v[1][k], v[2][k]});
            cb[k] = std::min(cb[k], b[k]);
            cb[4 + k] = std::max(cb[4 + k], b[4 + k]);
            reach = std::max({reach, std::fabs(b[k]), std::fabs(b[4 + k])});
        }
        for (int e = 0; e < 3; ++e) {
            const float *lo = v[e], *hi = v[(e + 1) % 3];
            if (mesh_edge_swapped(lo, hi)) std::swap(lo, hi);
            float *o = edge + (size_t)12 * t + 4 * e;
            o[0] = lo[1], o[1] = lo[2], o[2] = hi[1], o[3] = hi[2];
        }
        const double ux = (double)v[1][0] - (double)v[0][0], uy = (double)v[1][1] - (double)v[0][1], uz = (double)v[1][2] - (double)v[0][2];
        const double wx = (double)v[2][0] - (double)v[0][0], wy = (double)v[2][1] - (double)v[0][1], wz = (double)v[2][2] - (double)v[0][2];
        double *n = r.n.data() + (size_t)3 * t;
        n[0] = uy * wz - uz * wy;
        n[1] = uz * wx - ux * wz;
        n[2] = ux * wy - uy * wx;
    }
    r.grow = 3.0f * h + 1e-4f * reach;
    return r;
}

}  // namespace vtmc
#endif
