// mesh_host_check.cpp -- a stand-alone run of the host half of vtmc_stamp_from_mesh (csrc/mesh_host.h: the closed-mesh check and the
// kernel's records) on a few meshes, for the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off tools/mesh_host_check.cpp -o mesh_host_check && ./mesh_host_check
// Exits 0 when every answer is the expected one.
#include "../volumetricterrain_amd/csrc/mesh_host.h"
#include <cstdio>

using namespace vtmc;

static int failures = 0;
#define EXPECT(c) \
    do { \
        if (!(c)) { \
            std::printf("line %d: %s\n", __LINE__, #c); \
            ++failures; \
        } \
    } while (0)

// n tetrahedra on a circle: 4n triangles on 4n vertices, every edge used twice
static void ring(int n, std::vector<float> &pos, std::vector<int32_t> &idx)
{
    for (int i = 0; i < n; ++i) {
        const float x = std::cos(6.2831853f * i / n) * 8.0f, z = std::sin(6.2831853f * i / n) * 8.0f;
        pos.insert(pos.end(), {x, 0.0f, z, x + 0.5f, 0.0f, z, x, 0.5f, z, x, 0.0f, z + 0.5f});
        const int a = 4 * i;
        idx.insert(idx.end(), {a, a + 2, a + 1, a, a + 1, a + 3, a, a + 3, a + 2, a + 1, a + 2, a + 3});
    }
}

int main()
{
    const float box[24] = {2, 2, 2, 6, 2, 2, 2, 6, 2, 6, 6, 2, 2, 2, 6, 6, 2, 6, 2, 6, 6, 6, 6, 6};
    const int32_t tri[36] = {0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5};
    int32_t edge[2] = {-1, -1}, uses = -1;
    EXPECT(mesh_closed(tri, 12, edge, &uses));
    EXPECT(!mesh_closed(tri + 3, 11, edge, &uses) && uses == 1 && edge[0] == 0 && edge[1] == 3);
    std::vector<int32_t> more(tri, tri + 36);
    more.insert(more.end(), {0, 0, 5});  // repeats an index: dropped by the check
    EXPECT(mesh_closed(more.data(), 13, edge, &uses));
    more.insert(more.end(), {0, 2, 3});  // a third user of three edges
    EXPECT(!mesh_closed(more.data(), 14, edge, &uses) && uses == 3);
    const int32_t one[3] = {0, 1, 2};
    EXPECT(!mesh_closed(one, 1, edge, &uses) && uses == 1);

    const float first[3] = {0.37f, 0.41f, 0.29f};
    const int32_t dims[3] = {9, 9, 9};
    const MeshRecords r = mesh_records(box, tri, 12, first, 1.0f, dims);
    EXPECT(r.n_chunks == 1 && r.f.size() == 32u * 12 + 8 && r.n.size() == 36);
    const float *chunk = r.f.data() + r.chunk_at();
    for (int k = 0; k < 3; ++k) EXPECT(chunk[k] == 2.0f && chunk[4 + k] == 6.0f);
    EXPECT(r.grow > 3.0f && r.grow < 3.01f);
    for (int t = 0; t < 12; ++t) {
        const float *v = r.f.data() + r.vert_at() + 12 * t, *b = r.f.data() + r.bound_at() + 8 * t, *e = r.f.data() + r.edge_at() + 12 * t;
        EXPECT(v[0] <= v[4] && v[4] <= v[8]);                                    // ascending in x
        for (int k = 0; k < 3; ++k) EXPECT(b[k] >= 2.0f && b[4 + k] <= 6.0f && b[k] <= b[4 + k]);
        for (int k = 0; k < 3; ++k) EXPECT(e[4 * k + 1] < e[4 * k + 3] || (e[4 * k + 1] == e[4 * k + 3] && e[4 * k] <= e[4 * k + 2]));   // lo <= hi by (z, y)
        const double *n = r.n.data() + 3 * t;
        EXPECT(std::fabs(n[0]) + std::fabs(n[1]) + std::fabs(n[2]) == 16.0);    // an axis-aligned half face of a 4 x 4 square
    }

    std::vector<float> pos;
    std::vector<int32_t> idx;
    ring(300, pos, idx);  // 1 200 triangles: five chunks, the last one short
    EXPECT(mesh_closed(idx.data(), (int32_t)idx.size() / 3, edge, &uses));
    const int32_t big[3] = {70, 9, 6};
    const MeshRecords q = mesh_records(pos.data(), idx.data(), (int32_t)idx.size() / 3, first, 0.25f, big);
    EXPECT(q.n_chunks == 5 && q.f.size() == 32u * 1200 + 40);
    for (int c = 0; c < q.n_chunks; ++c) {
        const float *cb = q.f.data() + q.chunk_at() + 8 * c;
        for (int t = c * kMeshChunk; t < std::min((c + 1) * kMeshChunk, q.n_tri); ++t) {
            const float *b = q.f.data() + q.bound_at() + 8 * (size_t)t;
            for (int k = 0; k < 3; ++k) EXPECT(cb[k] <= b[k] && cb[4 + k] >= b[4 + k]);
        }
    }
    std::printf(failures ? "%d checks failed\n" : "mesh_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
