// union_find.h -- the union-find on a parent array of int32 indices that the labelling passes share (terrain_fragments.hip: the solid
// samples of a box; terrain_nav.hip: the spans of a navigation build).  Union by smaller index, so a root is the smallest index of its
// component.  The parent array may be written by other workgroups while it is read: only the value the attaching atomic returns decides
// whether a union is done (terrain_fragments.hip, VISIBILITY).  EVERY LOOP IS BOUNDED, twice: a walk up the parents must strictly decrease the index
// and a union's retry must strictly decrease its larger root, and each loop also counts against `bound`, the number of nodes.  A violation
// sets a bit of the flag word and ends the loop.  Device code only.
#ifndef VTMC_UNION_FIND_H
#define VTMC_UNION_FIND_H
#include <hip/hip_runtime.h>
#include <climits>

namespace vtmc {

template <int kScope>
__device__ __forceinline__ int uf_load(const int *P, int i) { return __hip_atomic_load(P + i, __ATOMIC_RELAXED, kScope); }

// the root above i, or -1 with the flag set; i is solid.  Every hop goes to a strictly smaller index.
template <int kScope>
__device__ __forceinline__ int uf_find(const int *P, int i, int bound, int *flag)
{
    for (int hops = 0; hops <= bound; ++hops) {
        const int p = uf_load<kScope>(P, i);
        if (p == i) return i;
        if (p > i || p < 0) break;
        i = p;
    }
    atomicOr(flag, 1);
    return -1;
}

// every node from i up to (not including) anything <= r gets r, an ancestor of it, as its parent at the least
template <int kScope>
__device__ __forceinline__ void uf_compress(int *P, int i, int r, int bound, int *flag)
{
    for (int hops = 0; i > r && hops <= bound; ++hops) {
        const int p = __hip_atomic_fetch_min(P + i, r, __ATOMIC_RELAXED, kScope);
        if (p > i || p < 0) {
            atomicOr(flag, 1);
            return;
        }
        if (p == i) return;
        i = p;
    }
}

// joins the components of the solid samples a and b: the larger root goes under the smaller
template <int kScope, bool kCompress>
__device__ __forceinline__ void uf_union(int *P, int a, int b, int bound, int *flag)
{
    int larger = INT_MAX;
    for (int tries = 0; tries <= bound; ++tries) {
        const int ra = uf_find<kScope>(P, a, bound, flag), rb = uf_find<kScope>(P, b, bound, flag);
        if (ra < 0 || rb < 0) return;
        if (kCompress) {
            uf_compress<kScope>(P, a, ra, bound, flag);
            uf_compress<kScope>(P, b, rb, bound, flag);
        }
        if (ra == rb) return;
        a = ra > rb ? ra : rb;
        b = ra > rb ? rb : ra;
        if (a >= larger) break;   // a retry's larger root lies strictly below the last one's
        larger = a;
        // Only a ROOT is ever attached: a compare-and-swap, not an atomicMin.  An atomicMin would also re-parent an a that somebody
        // attached first (when b lies below its new parent), and for as long as that edge leads out of a's tree a concurrent
        // uf_compress along it moves nodes of the OTHER tree under its own stale root and cuts them off their ancestors: a union
        // made earlier is lost (seen on an MI355X: a few per million unions, profiles/r21/nav).
        int old = a;
        if (__hip_atomic_compare_exchange_strong(P + a, &old, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kScope)) return;
        if (old > a || old < 0) break;
        a = old;                  // somebody attached a first: old and b have yet to meet
    }
    atomicOr(flag, 2);
}

}  // namespace vtmc
#endif
