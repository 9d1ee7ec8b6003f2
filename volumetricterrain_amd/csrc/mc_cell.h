// mc_cell.h -- what the surface queries (raycast.hip, spherequery.hip) share on the device, so both see the same triangles bit for bit
// (gfx950, wave64): the description of the surface (SurfaceGrid, CornerOffsets, load_cell), one cell's marching-cubes triangles rebuilt
// from its eight samples, and the watertight ray / triangle test.
//
// The arithmetic is the exact-mode emit's (CollectTriNum.compute:41-64 case, MarchingCube.compute:119-151 vertices and winding): the
// library is built with -ffp-contract=off and `/` is correctly rounded, so a rebuilt triangle equals the extracted one.  The case table
// (DeviceTables::vert_packed, 256 words of 5 x 12 bits) is read from LDS: each kernel copies it there with load_case_table.
#ifndef VTMC_MC_CELL_H
#define VTMC_MC_CELL_H
#include <cmath>

namespace vtmc {

// cube corner c of MarchingCube.compute:46-50 ({0,0,0},{1,0,0},{1,1,0},{0,1,0},{0,0,1},{1,0,1},{1,1,1},{0,1,1}) along each axis
__device__ __forceinline__ int corner_x(int c) { return (c ^ (c >> 1)) & 1; }
__device__ __forceinline__ int corner_y(int c) { return (c >> 1) & 1; }
__device__ __forceinline__ int corner_z(int c) { return (c >> 2) & 1; }
// endpoints of cube edge e, MarchingCube.compute:40-43 ({0,1},{1,2},{2,3},{3,0},{4,5},{5,6},{6,7},{7,4},{0,4},{1,5},{2,6},{3,7})
__device__ __forceinline__ int edge_a(int e) { return e < 8 ? e : e - 8; }
__device__ __forceinline__ int edge_b(int e) { return e < 8 ? (e & 4) | ((e + 1) & 3) : e - 4; }

// s[i] for a runtime i as a tree of selects on i's bits: a runtime index into a register array (or a chain of i == q
// selects, which the compiler folds back into one) puts the array in scratch
__device__ __forceinline__ float pick8(const float (&s)[8], int i)
{
    const bool b0 = i & 1, b1 = i & 2, b2 = i & 4;
    const float s01 = b0 ? s[1] : s[0], s23 = b0 ? s[3] : s[2], s45 = b0 ? s[5] : s[4], s67 = b0 ? s[7] : s[6];
    const float s03 = b1 ? s23 : s01, s47 = b1 ? s67 : s45;
    return b2 ? s47 : s03;
}
__device__ __forceinline__ double pick3(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// Ericson §5.1.5: the point q of triangle (a, b, c) nearest to p, by Voronoi region (vertex, edge, face) from six dot products.  One IEEE
// operation per step in the order written here (a dot is (x*x' + y*y') + z*z'), in the precision of T: the surface queries call it in
// double (spherequery.hip), the mesh voxelizer in float, where include/vtmc.h states it step by step (vtmc_stamp_from_mesh).
template <class T>
__device__ __forceinline__ void closest_on_triangle(const T *p, const T *a, const T *b, const T *c, T *q)
{
    const T ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const T ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const T d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2], d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
    T wb = 0, wc = 0;  // q = a + wb ab + wc ac, except on edge bc
    const T bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const T d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2], d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
    const T cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const T d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2], d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
    const T vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0 && d2 <= 0) {
        // vertex a
    } else if (d3 >= 0 && d4 <= d3) {
        wb = 1;  // vertex b
    } else if (vc <= 0 && d1 >= 0 && d3 <= 0) {
        wb = d1 / (d1 - d3);  // edge ab
    } else if (d6 >= 0 && d5 <= d6) {
        wc = 1;  // vertex c
    } else if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        wc = d2 / (d2 - d6);  // edge ac
    } else if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
        const T w = (d4 - d3) / ((d4 - d3) + (d5 - d6));  // edge bc
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = b[k] + w * (c[k] - b[k]);
        return;
    } else {
        const T den = 1 / (va + vb + vc);  // inside the face
        wb = vb * den;
        wc = vc * den;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * wb + ac[k] * wc;
}

// Block-local position of the vertex on cube edge e of the cell with block-local corner (lx, ly, lz): MarchingCube.compute:119-133
// as the exact-mode emit and the oracle evaluate it -- t = -a / (b - a), p = u + t * (v - u), endpoints in the reference's order.
__device__ __forceinline__ void edge_vertex(const float (&s)[8], int lx, int ly, int lz, int e, float p[3])
{
    const int a = edge_a(e), b = edge_b(e);
    const float va = pick8(s, a), vb = pick8(s, b);
    const float t = (-va) / (vb - va);
    const int l[3] = {lx, ly, lz};
    const int oa[3] = {corner_x(a), corner_y(a), corner_z(a)}, ob[3] = {corner_x(b), corner_y(b), corner_z(b)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = (float)l[k] + (float)oa[k];
        const float v = (float)l[k] + (float)ob[k];
        p[k] = u + t * (v - u);
    }
}

// The surface a query runs against: the marching-cubes surface of n[0] x n[1] x n[2] cells of a density grid in any memory order.  The
// first member of both kernels' arguments (raycast.hip, spherequery.hip); filled by surface_of_grid / surface_of_terrain (surface_query.h).
struct SurfaceGrid {
    const float *grid;
    long long sx, sy, sz;                   // element strides
    int n[3];                               // cells per axis
    double origin[3];                       // world position of sample (0,0,0)
    double scale;                           // voxel_scale
    const unsigned long long *vert_packed;  // DeviceTables::vert_packed
};

// element offsets of a cell's eight corners from its first, in MarchingCube.compute order: built once per kernel, outside its walk
struct CornerOffsets {
    long long c[8];
    __device__ __forceinline__ explicit CornerOffsets(const SurfaceGrid &g) : c{0, g.sx, g.sx + g.sy, g.sy, g.sz, g.sx + g.sz, g.sx + g.sy + g.sz, g.sy + g.sz} {}
};
// the eight corner samples of cell (cx, cy, cz): one straight run of loads, nothing waits between them
__device__ __forceinline__ void load_cell(const SurfaceGrid &g, const CornerOffsets &o, int cx, int cy, int cz, float (&s)[8])
{
    const float *base = g.grid + ((long long)cx * g.sx + (long long)cy * g.sy + (long long)cz * g.sz);
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = base[o.c[q]];
}

// the case table in LDS: one word per thread of a 256-thread workgroup (the caller's next barrier publishes it)
__device__ __forceinline__ void load_case_table(unsigned long long *s_cases, const unsigned long long *vert_packed, int tid)
{
    s_cases[tid] = vert_packed[tid];
}

// CollectTriNum.compute:41-51: strict '>', NaN is outside; 0 and 255 are the two cases without triangles
__device__ __forceinline__ unsigned cell_case(const float (&s)[8])
{
    unsigned cs = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) cs |= (unsigned)(s[q] > 0.f) << q;
    return cs;
}

// Triangle i of the cell with global corner (cx, cy, cz) whose case word is w: its vertices in grid units, exact (8b + p), wound as
// the emit writes them (MarchingCube.compute:151 swaps the last two).  False when the case has fewer than i + 1 triangles.
__device__ __forceinline__ bool cell_triangle(unsigned long long w, const float (&s)[8], int cx, int cy, int cz, int i, double P0[3],
                                              double P1[3], double P2[3])
{
    const int e0 = (int)(w >> (12 * i)) & 15, e1 = (int)(w >> (12 * i + 4)) & 15, e2 = (int)(w >> (12 * i + 8)) & 15;
    if (e0 == 15) return false;  // MarchingCube.compute:141
    const int lx = cx & 7, ly = cy & 7, lz = cz & 7;
    const double bx = (double)(cx - lx), by = (double)(cy - ly), bz = (double)(cz - lz);
    float p0[3], p1[3], p2[3];
    edge_vertex(s, lx, ly, lz, e0, p0);
    edge_vertex(s, lx, ly, lz, e2, p1);  // winding swap, MarchingCube.compute:151
    edge_vertex(s, lx, ly, lz, e1, p2);
    P0[0] = bx + p0[0], P0[1] = by + p0[1], P0[2] = bz + p0[2];
    P1[0] = bx + p1[0], P1[1] = by + p1[1], P1[2] = bz + p1[2];
    P2[0] = bx + p2[0], P2[1] = by + p2[1], P2[2] = bz + p2[2];
    return true;
}

// A ray for the watertight test (Woop, Benthin & Wald 2013): origin and direction in grid units, the axis permutation and the shear.
struct Ray {
    double o[3], d[3];
    int kx, ky, kz;
    double Sx, Sy, Sz;
};

// the permutation and shear of r.d (r.d non-zero)
__device__ __forceinline__ void ray_setup(Ray &r)
{
    const double ad[3] = {fabs(r.d[0]), fabs(r.d[1]), fabs(r.d[2])};
    r.kz = ad[0] >= ad[1] && ad[0] >= ad[2] ? 0 : (ad[1] >= ad[2] ? 1 : 2);
    r.kx = r.kz == 2 ? 0 : r.kz + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    const double dkz = pick3(r.d[0], r.d[1], r.d[2], r.kz);
    if (dkz < 0.0) {
        const int x = r.kx;
        r.kx = r.ky;
        r.ky = x;
    }
    r.Sx = pick3(r.d[0], r.d[1], r.d[2], r.kx) / dkz;
    r.Sy = pick3(r.d[0], r.d[1], r.d[2], r.ky) / dkz;
    r.Sz = 1.0 / dkz;
}

// The watertight test of the ray against triangle (P0, P1, P2): false on a miss or an edge-on triangle; else t (in the units of
// r.d's parameter) and the barycentric weights V / det, W / det of P1 and P2.
__device__ __forceinline__ bool ray_triangle(const Ray &r, const double P0[3], const double P1[3], const double P2[3], double &t, double &V,
                                             double &W, double &det)
{
    const double Ax0 = P0[0] - r.o[0], Ay0 = P0[1] - r.o[1], Az0 = P0[2] - r.o[2];
    const double Bx0 = P1[0] - r.o[0], By0 = P1[1] - r.o[1], Bz0 = P1[2] - r.o[2];
    const double Cx0 = P2[0] - r.o[0], Cy0 = P2[1] - r.o[1], Cz0 = P2[2] - r.o[2];
    const double Akz = pick3(Ax0, Ay0, Az0, r.kz), Bkz = pick3(Bx0, By0, Bz0, r.kz), Ckz = pick3(Cx0, Cy0, Cz0, r.kz);
    const double Ax = pick3(Ax0, Ay0, Az0, r.kx) - r.Sx * Akz, Ay = pick3(Ax0, Ay0, Az0, r.ky) - r.Sy * Akz;
    const double Bx = pick3(Bx0, By0, Bz0, r.kx) - r.Sx * Bkz, By = pick3(Bx0, By0, Bz0, r.ky) - r.Sy * Bkz;
    const double Cx = pick3(Cx0, Cy0, Cz0, r.kx) - r.Sx * Ckz, Cy = pick3(Cx0, Cy0, Cz0, r.ky) - r.Sy * Ckz;
    const double U = Cx * By - Cy * Bx;
    V = Ax * Cy - Ay * Cx;
    W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    det = U + V + W;
    if (det == 0.0) return false;
    const double T = U * (r.Sz * Akz) + V * (r.Sz * Bkz) + W * (r.Sz * Ckz);
    t = T / det;
    return true;
}

__device__ __forceinline__ bool finite3(const float *v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

}  // namespace vtmc

#endif
