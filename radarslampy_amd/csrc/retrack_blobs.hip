// retrack_blobs.hip - K4-K6 of the device-side feature (re)detection (overview: retrack.hip): candidate order and blob bookkeeping
#include "retrack_geom.h"
#include "npsort_wave.h"
#include "ssc_body.inc"

// ------------------------------------------------------------------------------------------------ K4: ordered candidates
// the candidates of a detection (at most BP_MAX_PTS are kept) sorted by (row, column, layer): keys are unique, so a key's rank is
// the number of smaller keys - every thread counts for its keys against the whole list in LDS (broadcast reads)
__global__ __launch_bounds__(256) void rt_emit_kernel(RtArgs a, int first)
{
    __shared__ uint32_t key[BP_MAX_PTS];
    __shared__ double val[BP_MAX_PTS];
    const int ls = blockIdx.x, slot = first + ls;
    if (slot >= *a.rt_n) return;
    const int t = threadIdx.x;
    const int n = min(a.cand_n[ls], BP_MAX_PTS);
    uint32_t *crc = a.cand_rc + (int64_t)ls * BP_MAX_PTS;
    double *cval = a.cand_val + (int64_t)ls * BP_MAX_PTS;
    for (int i = t; i < n; i += 256) { key[i] = crc[i]; val[i] = cval[i]; }
    __syncthreads();
    for (int i = t; i < n; i += 256) {
        const uint32_t k = key[i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += key[j] < k ? 1 : 0;
        crc[rank] = k;
        cval[rank] = val[i];
    }
}

// ------------------------------------------------------------------------------------------------ K5: blob bookkeeping
// Two capacity classes.  The tables of the FULL class (2048 candidates, 4914 pairs in the LDS set tables) take 64 KB: two workgroups - two
// detections - per CU, while a real or synthetic scan has 250-600 candidates and a few hundred to 1400 pairs.  The SMALL class (1024
// candidates, 1228 pairs: the set then never grows past 2048 entries) takes 33 KB: four detections per CU.  Every detection goes
// through the small kernel first; one that does not fit (more candidates, tree nodes or pairs) is left untouched and marked for the
// full kernel, which runs right after it and returns at once for everything else.
template <bool SMALL> struct RtBlobCap {
    static constexpr int NP = SMALL ? 1024 : BP_MAX_PTS;
    static constexpr int NNODE = SMALL ? 320 : BP_MAX_NODES;
    static constexpr int CAPA = 2048, CAPB = SMALL ? 4096 : 8192;          // set tables (entries); tabB also holds NP packed points / doubles
    static constexpr int LDS_PAIRS = SMALL ? 1228 : BP_LDS_PAIRS;          // below this count the set never outgrows the tables
    static constexpr int NPL = SMALL ? 1280 : 3328;                        // pairs kept in LDS (full: what the 64 KB of static LDS leave)
    static constexpr int NCL = CAPB / 2;                                   // overlapping pairs gathered into tabB (uint32)
};
#define RT_BLOBS_REDO (-1)                // kp_n of a detection the small kernel left to the full one
template <bool SMALL> struct RtBlobLds {
    typedef RtBlobCap<SMALL> CP;
    int16_t xy[2 * CP::NP];           // [row, col] in response order
    int16_t idx[CP::NP];              // cKDTree.indices, later the aquicksort permutation
    uint8_t lay[CP::NP];              // layer (1 | 2) in response order; 0 = pruned
    BpNode nodes[CP::NNODE];
    int st[3 * 256];
    int16_t nbox[CP::NNODE][4];       // query_pairs' tracker box of every node: the root's bounds cut by the split planes on the way down
                                      // ({min0, max0, min1, max1}; filled as the nodes are built)
    uint8_t nslid[CP::NNODE];         // bit k: bound k of nbox lies on a slid split (BP_SLID): the tracker's bound is bp_next_up(nbox[k])
    uint16_t tabA[CP::CAPA];
    alignas(8) uint16_t tabB[CP::CAPB];   // hash table of the set order; before that the packed points of the tree build (NP x 8 B)
    uint32_t ovbits[(CP::LDS_PAIRS + 31) / 32 + 1];
    uint32_t pl[CP::NPL];             // the pairs, when they fit: the sequential set-order pass reads them one by one
    int vals[8];
};

// ---- the large nodes of the k-d tree, built by the WHOLE wavefront (round 5).  bp_build_node - bounds, libstdc++'s introselect, scipy's
// partition pass - on one lane is a chain of dependent LDS reads: ~110 us for the 530-element root of a real frame, 55 for its children
// (profiles: ranking + tree build were 323 of the 640 us of a lone detection's bookkeeping).  Both partitions are two-pointer scans that swap
// the i-th misplaced element from the left with the i-th from the right until the pointers cross; elements between the pointers are never
// touched before the pointers get there, so the two ordered lists of misplaced POSITIONS can be taken from the array as it stands (ballot +
// prefix count per 64 positions), the number of swaps is the number of i with L[i] < R[i], and the swaps are independent of each other:
// the same array, element for element, as the sequential code (an element equal to the pivot sits in both lists; it stops the scan from
// whichever side reaches it first, exactly as there; checked against the sequential algorithms on 20 000 random arrays with heavy ties: tests/test_blob_book_cpu.py).  Median-of-three, the <= 3-element insertion sort and the rare heap-select
// fallback stay sequential (uniform values / lane 0).  Lp, Rp: scratch of (end - start) uint16 each.
#define RB_WAVE_MIN 100                     // nodes with more elements take this path (a level of eight 66-element nodes is faster lane by lane)
__device__ __forceinline__ int rb_key(const BpPt *pt, int i, int d) { return (int16_t)(pt[i].v >> (16 * d)); }

// unguarded Hoare partition of [first + 1, last) around piv = key(first) as std::__unguarded_partition leaves it; returns the cut
__device__ int rb_partition_hoare(BpPt *pt, int first, int last, int d, int lane, uint16_t *Lp, uint16_t *Rp)
{
    const int piv = rb_key(pt, first, d);
    const uint64_t below = (1ull << lane) - 1ull;
    int nL = 0, nR = 0;
    // one pass over [first, last): L = positions >= first + 1 with key >= piv, ascending; R = positions with key <= piv, stored ascending
    // too and read from its end (R[i] = Rp[nR - 1 - i])
    for (int c0 = first; c0 < last; c0 += 64) {
        const int pos = c0 + lane;
        const int k = pos < last ? rb_key(pt, pos, d) : 0;
        const bool ge = pos < last && pos > first && k >= piv, le = pos < last && k <= piv;
        const uint64_t bl = __ballot(ge), br = __ballot(le);
        if (ge) Lp[nL + __popcll(bl & below)] = (uint16_t)pos;
        if (le) Rp[nR + __popcll(br & below)] = (uint16_t)pos;
        nL += __popcll(bl); nR += __popcll(br);
    }
    __syncthreads();
    const int nm = min(nL, nR);
    int kk = 0;
    for (int i0 = 0; i0 < nm; i0 += 64) {
        const int i = i0 + lane;
        const uint64_t bal = __ballot(i < nm && Lp[i] < Rp[nR - 1 - i]);
        kk += __popcll(bal);
        if (__popcll(bal) < min(64, nm - i0)) break;                       // (L ascends, R descends: once crossed, crossed for good)
    }
    for (int i = lane; i < kk; i += 64) { const int x = Lp[i], y = Rp[nR - 1 - i]; const BpPt t = pt[x]; pt[x] = pt[y]; pt[y] = t; }
    // where the left pointer stops: the next position with a key >= piv in the array AS IT IS NOW - the next entry of L, or the smallest
    // position the swaps have just filled with such a key (R[kk - 1]) when the pointer runs into the swapped region first
    const int cut = min(kk < nL ? (int)Lp[kk] : last, kk > 0 ? (int)Rp[nR - kk] : last);
    __syncthreads();
    return cut;
}

// std::nth_element(first, nth, last) on pt by coordinate d, element for element
__device__ void rb_nth_element_wave(BpPt *pt, int first, int nth, int last, int d, int lane, uint16_t *Lp, uint16_t *Rp)
{
    if (first == last || nth == last) return;
    int depth = 0;
    for (int n = last - first; n > 1; n >>= 1) depth++;
    depth *= 2;
    while (last - first > 3) {
        if (depth == 0) {                                                   // introselect's fallback: sequential, as bp_nth_element has it
            if (lane == 0) bp_heap_select_nth(pt, first, nth, last, (const int16_t *)nullptr, d);
            __syncthreads();
            return;
        }
        depth--;
        const int mid = first + (last - first) / 2, ia = first + 1, ib = mid, ic = last - 1;
        const int ka = rb_key(pt, ia, d), kb = rb_key(pt, ib, d), kc = rb_key(pt, ic, d);
        int sm;                                                             // __move_median_to_first
        if (ka < kb) sm = kb < kc ? ib : (ka < kc ? ic : ia);
        else sm = ka < kc ? ia : (kb < kc ? ic : ib);
        __syncthreads();
        if (lane == 0) { const BpPt t = pt[first]; pt[first] = pt[sm]; pt[sm] = t; }
        __syncthreads();
        const int cut = rb_partition_hoare(pt, first, last, d, lane, Lp, Rp);
        if (cut <= nth) first = cut; else last = cut;
    }
    if (lane == 0)
        for (int i = first + 1; i < last; i++) {                            // __insertion_sort
            const BpPt v = pt[i];
            const int kv = (int16_t)(v.v >> (16 * d));
            if (kv < rb_key(pt, first, d)) { for (int j = i; j > first; j--) pt[j] = pt[j - 1]; pt[first] = v; }
            else { int j = i; while (kv < rb_key(pt, j - 1, d)) { pt[j] = pt[j - 1]; j--; } pt[j] = v; }
        }
    __syncthreads();
}

// rb_aquicksort_wave (np.argsort of NumPy 1.22 by one wavefront): npsort_wave.h, here on the u8 layer keys

// bp_build_node by the whole wavefront (uniform start / end); the same return value and node fields
__device__ int rb_build_node_wave(BpPt *pt, int start, int end, BpNode &nd, int lane, uint16_t *Lp, uint16_t *Rp)
{
    nd.start = (int16_t)start; nd.end = (int16_t)end; nd.less = nd.greater = -1; nd.split_dim = -1; nd.split = 0;
    if (end - start <= BP_LEAF) return -1;
    int mx0 = -32768, mn0 = 32767, mx1 = -32768, mn1 = 32767;
    for (int j = start + lane; j < end; j += 64) {
        const int v0 = rb_key(pt, j, 0), v1 = rb_key(pt, j, 1);
        mx0 = max(mx0, v0); mn0 = min(mn0, v0); mx1 = max(mx1, v1); mn1 = min(mn1, v1);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        mx0 = max(mx0, __shfl_xor(mx0, m)); mn0 = min(mn0, __shfl_xor(mn0, m));
        mx1 = max(mx1, __shfl_xor(mx1, m)); mn1 = min(mn1, __shfl_xor(mn1, m));
    }
    int d = 0, size = 0;
    if (mx0 - mn0 > size) { d = 0; size = mx0 - mn0; }
    if (mx1 - mn1 > size) { d = 1; size = mx1 - mn1; }
    if (size <= 0) return -1;
    const int half = (end - start) / 2;
    rb_nth_element_wave(pt, start, start + half, end, d, lane, Lp, Rp);
    int split = rb_key(pt, start + half, d);
    // scipy's partition pass: p advances over keys < thr, q retreats over keys >= thr, misplaced pairs are swapped: afterwards the
    // keys below thr fill [start, start + the count returned)
    const uint64_t below = (1ull << lane) - 1ull;
    auto split_pass = [&](int thr) {
        int nL = 0, nR = 0;
        for (int c0 = start; c0 < end; c0 += 64) {
            const int pos = c0 + lane;
            const int k = pos < end ? rb_key(pt, pos, d) : 0;
            const bool ge = pos < end && k >= thr, lt = pos < end && k < thr;
            const uint64_t bl = __ballot(ge), br = __ballot(lt);
            if (ge) Lp[nL + __popcll(bl & below)] = (uint16_t)pos;
            if (lt) Rp[nR + __popcll(br & below)] = (uint16_t)pos;
            nL += __popcll(bl); nR += __popcll(br);
        }
        __syncthreads();
        const int nm = min(nL, nR);
        int kk = 0;
        for (int i0 = 0; i0 < nm; i0 += 64) {
            const int i = i0 + lane;
            const uint64_t bal = __ballot(i < nm && Lp[i] < Rp[nR - 1 - i]);
            kk += __popcll(bal);
            if (__popcll(bal) < min(64, nm - i0)) break;
        }
        for (int i = lane; i < kk; i += 64) { const int x = Lp[i], y = Rp[nR - 1 - i]; const BpPt t = pt[x]; pt[x] = pt[y]; pt[y] = t; }
        __syncthreads();
        return nR;
    };
    int p = start + split_pass(split);
    if (p == start) {                           // no point below the median key: the plane slides just above the smallest key and the
        split = d ? mn1 : mn0;                  // points AT it go to less (bp_build_node; rare)
        p = start + split_pass(split + 1);
        d |= BP_SLID;
    }
    // (p == end cannot happen: the median itself is >= split)
    nd.split_dim = (int16_t)d; nd.split = split;
    return p;
}

// bp_pyset_order by the whole wavefront: the same tables, slot for slot.  What is sequential in a CPython set is the INSERTION (the slot a
// key takes depends on the slots taken before it); everything around it is not - the tuple hashes (two 64-bit multiplications each: 64
// keys at a time, one per lane), clearing a new table, listing the old table's keys in slot order at a resize, reading the final table
// out.  The insertions themselves run on wave-uniform values (hash and key by v_readlane, uniform table reads), chunk by chunk up to
// the next resize.  order doubles as the scratch list of a resize (it is the output: free until the end).
template <bool TLDS, typename ORD>
__device__ int rb_pyset_order_wave(const uint32_t *pairs, int np, uint16_t *tabA, int capA, uint16_t *tabB, int capB, ORD *order, int lane)
{
    uint16_t *tab = tabA, *other = tabB;
    int cap_other = capB, cap_cur = capA;
    uint32_t mask = 7;
    if (lane < 8) tab[lane] = 0;
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    int fill = 0;
    // src = nullptr: the pairs p0 .. p0 + cnt - 1 themselves; else the keys listed in src[0 .. cnt)
    auto insert_chunk = [&](uint16_t *t, uint32_t msk, const ORD *src, int p0, int cnt) {
        const int key1 = lane < cnt ? (src ? (int)src[p0 + lane] : p0 + lane + 1) : 0;
        const uint64_t h = key1 ? bp_tuple_hash(pairs[key1 - 1]) : 0ull;
        for (int j = 0; j < cnt; j++) {
            const uint64_t hj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(h >> 32), j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(h & 0xffffffffull), j);
            const int kj = __builtin_amdgcn_readlane(key1, j);
            uint64_t perturb = hj;
            uint32_t i = (uint32_t)hj & msk;
            for (;;) {
                const int probes = (i + 9 <= msk) ? 9 : 0;
                int e = -1;
                for (int q = 0; q <= probes; q++) if (t[i + q] == 0) { e = (int)i + q; break; }
                if (e >= 0) { if (lane == 0) t[e] = (uint16_t)kj; break; }
                perturb >>= 5;
                i = (uint32_t)(((uint64_t)i * 5 + 1 + perturb) & msk);
            }
            // the next key reads what this one wrote: a wavefront's LDS operations execute in order (tables in LDS, TLDS); a table in
            // global memory (more than 4 914 pairs) is written through before it is read again
            if (!TLDS) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    };
    for (int p = 0; p < np;) {
        // insertions until the next resize: the smallest k with (fill + k) * 5 >= mask * 3
        int room = (int)(((uint64_t)mask * 3 + 4) / 5) - fill;
        if (room < 1) room = 1;
        const int cnt = min(min(64, np - p), room);
        insert_chunk(tab, mask, (const ORD *)nullptr, p, cnt);
        p += cnt; fill += cnt;
        __syncthreads();
        if ((uint64_t)fill * 5 >= (uint64_t)mask * 3) {
            const int minused = fill > 50000 ? fill * 2 : fill * 4;
            uint32_t newsize = 8;
            while ((int)newsize <= minused) newsize <<= 1;
            if ((int)newsize > cap_other) return -1;
            for (uint32_t k = lane; k < newsize; k += 64) other[k] = 0;
            int m = 0;
            for (uint32_t k0 = 0; k0 <= mask; k0 += 64) {
                const uint32_t k = k0 + lane;
                const int key = k <= mask ? (int)tab[k] : 0;
                const uint64_t bal = __ballot(key != 0);
                if (key) order[m + __popcll(bal & below)] = (ORD)key;
                m += __popcll(bal);
            }
            __syncthreads();
            for (int q = 0; q < m; q += 64) insert_chunk(other, newsize - 1, order, q, min(64, m - q));
            __syncthreads();
            uint16_t *t = tab; tab = other; other = t;
            const int c = cap_cur; cap_cur = cap_other; cap_other = c;
            mask = newsize - 1;
        }
    }
    __syncthreads();
    int m = 0;
    for (uint32_t k0 = 0; k0 <= mask; k0 += 64) {
        const uint32_t k = k0 + lane;
        const int key = k <= mask ? (int)tab[k] : 0;
        const uint64_t bal = __ballot(key != 0);
        // (order may still hold a resize's list below m: every entry is rewritten before it is read again, and what is written at
        // position m + rank comes from slot k >= its old position - the final scan only ever overwrites entries it has passed)
        if (key) order[m + __popcll(bal & below)] = (ORD)(key - 1);
        m += __popcll(bal);
    }
    __syncthreads();
    return m;
}

#ifdef RB_EXP_PROF
__device__ unsigned long long rb_prof[16];
extern "C" int roam_debug_blob_prof(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rb_prof), sizeof(rb_prof)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rb_prof), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#define RB_P(k) { const unsigned long long tn_ = __builtin_readcyclecounter(); if (threadIdx.x == 0) rbp_[k] += tn_ - rbt_; rbt_ = tn_; }
#else
#define RB_P(k)
#endif
// the bookkeeping of one detection (one wavefront); -> 1 when the small class left it to the full one (kp_n = RT_BLOBS_REDO)
template <bool SMALL>
__device__ int rt_blobs_body(const RtArgs &a, int first, RtBlobLds<SMALL> &L, bool forced)
{
#ifdef RB_EXP_PROF
    unsigned long long rbp_[12] = {0}, rbt_ = __builtin_readcyclecounter();
#endif
    typedef RtBlobCap<SMALL> CP;
    // (L: the workgroup's LDS, the caller's)
    const int ls = a.blob_order ? a.blob_order[blockIdx.x] : (int)blockIdx.x, slot = first + ls;
    if (slot >= *a.rt_n) return 0;
    const int lane = threadIdx.x;
    const int ncand = a.cand_n[ls];
    if (!SMALL && !forced && a.kp_n[ls] != RT_BLOBS_REDO) return 0;                      // the small kernel did it
    if (SMALL && ncand > CP::NP) {
        if (lane == 0) a.kp_n[ls] = RT_BLOBS_REDO;
        return 1;
    }
    const int n = min(ncand, BP_MAX_PTS);
    const uint32_t *crc = a.cand_rc + (int64_t)ls * BP_MAX_PTS;
    const double *cval = a.cand_val + (int64_t)ls * BP_MAX_PTS;
    double *kp = a.kp + (int64_t)ls * BP_MAX_PTS * 3;
    int flags = ncand > BP_MAX_PTS ? RT_F_CAND_OVERFLOW : 0;
    // 1. response order: peak_local_max sorts by -intensity; equal responses keep the C (row, col, layer) order.  The responses are
    // staged in LDS (the set tables are free until step 5) and every lane ranks four candidates per pass against broadcast reads
    // (straight out of global memory the n^2 / 64 dependent loads were a sixth of this kernel)
    double *sval = reinterpret_cast<double *>(L.tabB);
    for (int i = lane; i < n; i += 64) sval[i] = cval[i];
    __syncthreads();
    for (int i0 = lane; i0 < n; i0 += 256) {
        double vi[4];
        int rank[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; u++) vi[u] = i0 + 64 * u < n ? sval[i0 + 64 * u] : 0.0;
        for (int j = 0; j < n; j++) {
            const double vj = sval[j];
#pragma unroll
            for (int u = 0; u < 4; u++) rank[u] += (vj > vi[u] || (vj == vi[u] && j < i0 + 64 * u)) ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + 64 * u;
            if (i < n) {
                const uint32_t p = crc[i];
                L.xy[2 * rank[u]] = (int16_t)(p >> 16); L.xy[2 * rank[u] + 1] = (int16_t)((p >> 2) & 0x3fff); L.lay[rank[u]] = (uint8_t)(p & 3);
            }
        }
    }
    __syncthreads();
    RB_P(0)
    // 2. cKDTree, level by level: every node of a level is built by its own lane (bounds, libstdc++ nth_element, scipy's
    // partition passes - sequential per node, but a level's nodes work on disjoint index ranges), so the critical path is the
    // largest node of every level (~2 n element visits) instead of all of them (~n log n: the build on lane 0 was 1.6 of this
    // kernel's 3.2 ms).  Nodes are numbered level by level; nothing downstream depends on the numbering, only on the links.
    BpPt *pt = reinterpret_cast<BpPt *>(L.tabB);          // {row, col, index} per element: keys without a dependent second read
    for (int i = lane; i < n; i += 64)
        pt[i].v = (uint64_t)(uint16_t)L.xy[2 * i] | ((uint64_t)(uint16_t)L.xy[2 * i + 1] << 16) | ((uint64_t)i << 32);
    int nn = 0;
    if (n > 0) {
        {
            int mn0 = 32767, mx0 = -32768, mn1 = 32767, mx1 = -32768;
            for (int i = lane; i < n; i += 64) {
                const int v0 = L.xy[2 * i], v1 = L.xy[2 * i + 1];
                mn0 = min(mn0, v0); mx0 = max(mx0, v0); mn1 = min(mn1, v1); mx1 = max(mx1, v1);
            }
            for (int d = 32; d >= 1; d >>= 1) {
                mn0 = min(mn0, __shfl_xor(mn0, d)); mx0 = max(mx0, __shfl_xor(mx0, d));
                mn1 = min(mn1, __shfl_xor(mn1, d)); mx1 = max(mx1, __shfl_xor(mx1, d));
            }
            if (lane == 0) { L.nbox[0][0] = (int16_t)mn0; L.nbox[0][1] = (int16_t)mx0; L.nbox[0][2] = (int16_t)mn1; L.nbox[0][3] = (int16_t)mx1; L.nslid[0] = 0; }
        }
        if (lane == 0) { L.nodes[0].start = 0; L.nodes[0].end = (int16_t)n; }
        nn = 1;
        __syncthreads();
        for (int lo = 0, hi = 1; lo < hi && nn > 0;) {
            for (int base = lo; base < hi; base += 64) {
                const int me = base + lane;
                const bool act = me < hi;
                BpNode nd;
                int p = -1, start = 0, end = 0;
                if (act) { start = L.nodes[me].start; end = L.nodes[me].end; }
                // the large nodes of the chunk one at a time by the whole wave, the others lane by lane
                uint64_t big = __ballot(act && end - start > RB_WAVE_MIN);
                const uint64_t bigs = big;
                while (big) {
                    const int j = __ffsll((long long)big) - 1;
                    big &= big - 1;
                    BpNode ndw;
                    const int pw = rb_build_node_wave(pt, __builtin_amdgcn_readlane(start, j), __builtin_amdgcn_readlane(end, j), ndw, lane,
                                                      reinterpret_cast<uint16_t *>(L.pl), reinterpret_cast<uint16_t *>(L.pl) + CP::NP);
                    if (lane == j) { p = pw; nd = ndw; }
                }
                if (act && !((bigs >> lane) & 1ull)) p = bp_build_node(L.xy, pt, start, end, nd);
                const uint64_t bal = __ballot(act && p >= 0);
                const int kids = 2 * __popcll(bal);
                if (nn + kids > CP::NNODE) { nn = -1; break; }                 // (uniform)
                if (act) {
                    if (p >= 0) {
                        const int c0 = nn + 2 * __popcll(bal & ((1ull << lane) - 1ull));
                        nd.less = (int16_t)c0; nd.greater = (int16_t)(c0 + 1);
                        L.nodes[c0].start = (int16_t)start; L.nodes[c0].end = (int16_t)p;
                        L.nodes[c0 + 1].start = (int16_t)p; L.nodes[c0 + 1].end = (int16_t)end;
                        for (int k = 0; k < 4; k++) L.nbox[c0][k] = L.nbox[c0 + 1][k] = L.nbox[me][k];
                        const int sd = nd.split_dim & 1, slid = nd.split_dim & BP_SLID ? 1 : 0, ps = L.nslid[me];
                        L.nbox[c0][2 * sd + 1] = (int16_t)nd.split;                // less: max = split
                        L.nbox[c0 + 1][2 * sd] = (int16_t)nd.split;                // greater: min = split
                        L.nslid[c0] = (uint8_t)((ps & ~(2 << (2 * sd))) | (slid << (2 * sd + 1)));
                        L.nslid[c0 + 1] = (uint8_t)((ps & ~(1 << (2 * sd))) | (slid << (2 * sd)));
                    }
                    L.nodes[me] = nd;
                }
                nn += kids;
            }
            if (nn < 0) break;
            __syncthreads();
            lo = hi; hi = nn;
        }
    }
    __syncthreads();
    if (SMALL && nn < 0) {                                                   // more tree nodes than the small class holds: the full kernel's
        if (lane == 0) a.kp_n[ls] = RT_BLOBS_REDO;
        return 1;
    }
    for (int i = lane; i < n; i += 64) L.idx[i] = (int16_t)(pt[i].v >> 32);          // cKDTree.indices
    __syncthreads();
    RB_P(1)
    // dual-tree traversal -> ordered leaf x leaf blocks.  query_pairs recurses over node pairs with a distance tracker it pushes and pops.
    // The tracker updates mind / maxd incrementally only when all of mind, maxd and the changed dimension's terms are at least its
    // inaccurate_distance_limit - which scipy sets to the ROOT pair's maxd, so that practically every push recomputes both sums from
    // the two boxes (bp_tpush); and where it does update incrementally the terms are integers on integer pixel bounds, exact either
    // way.  So the tracker's state at a node pair is a function of the two nodes' boxes alone (nbox, nslid) and the recursion needs
    // no stack.  A box bound on a slid split is nextafter(m), no integer: such node pairs take the from-scratch float64 sums in
    // bp_tfull's order below (an incremental update of them could round differently, but needs mind >= the root's maxd >= ub, a pair
    // that is pruned whatever the last bit says); all others compare exact integers.  The pairs are expanded LEVEL BY LEVEL, every item replaced in place by its
    // children in the recursion's order (a finished leaf x leaf block is its own child), so that the list stays in emission order throughout.
    // One lane per item, ballots for the offsets; two lists of BP_MAX_TASKS packed items ping-pong in the detection's pair scratch.  (On lane 0
    // the recursion was 45 % of this kernel: ~230 us of a lone detection.)  item = a | b << 10 | m << 20; m: 0 check, 1 no check, 2 / 3 block
    // with / without the distance test
    BpTask *tasks = a.tasks + (int64_t)ls * BP_MAX_TASKS;
    int nt = 0;
    double ub = 0;
    {
        bool any2l = false;
        for (int i = lane; i < n; i += 64) any2l = any2l || L.lay[i] == 2;
        const bool any2 = __ballot(any2l) != 0;
        const double r = 2 * (any2 ? a.sigma2 : a.sigma1) * 1.4142135623730951;      // _prune_blobs: distance = 2 * max sigma * sqrt(2)
        ub = r * r;
    }
    if (nn < 0) flags |= RT_F_TREE_OVERFLOW;
    else if (n > 1) {
        const int t_gt = (int)floor(ub), t_lt = (int)ceil(ub);              // integer d: d > ub <=> d > t_gt, d < ub <=> d < t_lt
        uint32_t *fa = a.pairs + (int64_t)ls * (BP_MAX_PAIRS + 1), *fb = fa + BP_MAX_TASKS;
        if (lane == 0) fa[0] = 0u;                                          // (root, root, check)
        int F = 1;
        bool over = false;
        const uint64_t below = (1ull << lane) - 1ull;
        for (;;) {
            __syncthreads();
            int total = 0;
            bool open = false;
            for (int c0 = 0; c0 < F; c0 += 64) {
                const bool act = c0 + lane < F;
                const uint32_t it = act ? fa[c0 + lane] : 0u;
                const int na = it & 1023, nb = (it >> 10) & 1023;
                int m = act ? (int)(it >> 20) : 2;
                uint32_t ch[4];
                int cnt = 0;
                if (act && m >= 2) { ch[0] = it; cnt = 1; }
                else if (act) {
                    const BpNode n1 = L.nodes[na], n2 = L.nodes[nb];
                    const bool l1 = n1.split_dim == -1, l2 = n2.split_dim == -1;
                    bool pruned = false;
                    const int sa = L.nslid[na], sb = L.nslid[nb];
                    if (m == 0 && !(sa | sb)) {
                        int mind = 0, maxd = 0;
                        for (int k = 0; k < 2; k++) {
                            const int a0 = L.nbox[na][2 * k], a1 = L.nbox[na][2 * k + 1], b0 = L.nbox[nb][2 * k], b1 = L.nbox[nb][2 * k + 1];
                            const int lo = max(max(a0 - b1, b0 - a1), 0), hi = max(a1 - b0, b1 - a0);
                            mind += lo * lo; maxd += hi * hi;
                        }
                        if (mind > t_gt) pruned = true;
                        else if (maxd < t_lt) m = 1;
                    } else if (m == 0) {
                        // a bound on a slid split is not an integer: the tracker's float64 arithmetic as it stands (bp_tdim / bp_tfull:
                        // every product and sum rounded on its own)
                        double mind = 0, maxd = 0;
                        for (int k = 0; k < 2; k++) {
                            double a0 = (double)L.nbox[na][2 * k], a1 = (double)L.nbox[na][2 * k + 1], b0 = (double)L.nbox[nb][2 * k], b1 = (double)L.nbox[nb][2 * k + 1];
                            if ((sa >> (2 * k)) & 1) a0 = bp_next_up(a0);
                            if ((sa >> (2 * k + 1)) & 1) a1 = bp_next_up(a1);
                            if ((sb >> (2 * k)) & 1) b0 = bp_next_up(b0);
                            if ((sb >> (2 * k + 1)) & 1) b1 = bp_next_up(b1);
                            double lo = a0 - b1 > b0 - a1 ? a0 - b1 : b0 - a1;
                            if (lo < 0) lo = 0;
                            const double hi = a1 - b0 > b1 - a0 ? a1 - b0 : b1 - a0;
                            mind = __dadd_rn(mind, __dmul_rn(lo, lo)); maxd = __dadd_rn(maxd, __dmul_rn(hi, hi));
                        }
                        if (mind > ub) pruned = true;
                        else if (maxd < ub) m = 1;
                    }
                    const uint32_t mm = (uint32_t)m << 20;
                    if (pruned) cnt = 0;
                    else if (l1 && l2) { ch[0] = (uint32_t)na | ((uint32_t)nb << 10) | ((m == 0 ? 2u : 3u) << 20); cnt = 1; }
                    else if (m == 1) {
                        if (l1) { ch[0] = na | ((uint32_t)n2.less << 10) | mm; ch[1] = na | ((uint32_t)n2.greater << 10) | mm; cnt = 2; }
                        else if (na == nb) {
                            ch[0] = n1.less | ((uint32_t)n2.less << 10) | mm; ch[1] = n1.less | ((uint32_t)n2.greater << 10) | mm;
                            ch[2] = n1.greater | ((uint32_t)n2.greater << 10) | mm; cnt = 3;
                        } else { ch[0] = n1.less | ((uint32_t)nb << 10) | mm; ch[1] = n1.greater | ((uint32_t)nb << 10) | mm; cnt = 2; }
                    } else {
                        if (l1) { ch[0] = na | ((uint32_t)n2.less << 10); ch[1] = na | ((uint32_t)n2.greater << 10); cnt = 2; }
                        else if (l2) { ch[0] = n1.less | ((uint32_t)nb << 10); ch[1] = n1.greater | ((uint32_t)nb << 10); cnt = 2; }
                        else {
                            ch[0] = n1.less | ((uint32_t)n2.less << 10); ch[1] = n1.less | ((uint32_t)n2.greater << 10); cnt = 2;
                            if (na != nb) ch[cnt++] = n1.greater | ((uint32_t)n2.less << 10);
                            ch[cnt++] = n1.greater | ((uint32_t)n2.greater << 10);
                        }
                    }
                }
                const uint64_t b1 = __ballot(cnt >= 1), b2 = __ballot(cnt >= 2), b3 = __ballot(cnt >= 3), b4 = __ballot(cnt >= 4);
                const int off = total + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below) + __popcll(b4 & below);
                const int sum = __popcll(b1) + __popcll(b2) + __popcll(b3) + __popcll(b4);
                if (total + sum > BP_MAX_TASKS) { over = true; break; }     // (uniform)
                for (int j = 0; j < cnt; j++) fb[off + j] = ch[j];
                open = open || (cnt > 0 && (ch[0] >> 20) < 2u);             // (a node's children are all of one kind)
                total += sum;
            }
            if (over) break;
            uint32_t *t = fa; fa = fb; fb = t;
            F = total;
            if (!__ballot(open)) break;
        }
        __syncthreads();
        if (over) flags |= RT_F_TREE_OVERFLOW;
        else {
            nt = F;
            for (int i = lane; i < nt; i += 64) {
                const uint32_t it = fa[i];
                tasks[i].a = (int16_t)(it & 1023); tasks[i].b = (int16_t)((it >> 10) & 1023); tasks[i].mode = (int32_t)(it >> 20) - 2;
            }
        }
    }
    __syncthreads();
    RB_P(2)
    // 3. the pairs of the blocks in emission order (i-major, j ascending), 64 candidates per ballot
    uint32_t *pairs = a.pairs + (int64_t)ls * (BP_MAX_PAIRS + 1);
    int np = 0;
    for (int t = 0; t < nt; t++) {
        const BpTask tk = tasks[t];
        const BpNode n1 = L.nodes[tk.a], n2 = L.nodes[tk.b];
        const int la = n1.end - n1.start, lb = n2.end - n2.start, tot = la * lb;
        const bool same = tk.a == tk.b;
        for (int base = 0; base < tot; base += 64) {
            const int k = base + lane;
            bool ok = k < tot;
            int pi = 0, pj = 0;
            if (ok) {
                const int i = n1.start + k / lb, j = n2.start + k % lb;
                if (same && j <= i) ok = false;
                else {
                    pi = L.idx[i]; pj = L.idx[j];
                    if (!tk.mode) {
                        const double d0 = (double)L.xy[2 * pi] - (double)L.xy[2 * pj], d1 = (double)L.xy[2 * pi + 1] - (double)L.xy[2 * pj + 1];
                        ok = d0 * d0 + d1 * d1 <= ub;
                    }
                }
            }
            const uint64_t bal = __ballot(ok);
            const int o = np + __popcll(bal & ((1ull << lane) - 1ull));
            if (ok && o < BP_MAX_PAIRS) { pairs[o] = bp_pack(pi, pj); if (o < CP::NPL) L.pl[o] = bp_pack(pi, pj); }
            np += __popcll(bal);
        }
    }
    if (np > BP_MAX_PAIRS) { flags |= RT_F_PAIR_OVERFLOW; np = BP_MAX_PAIRS; }
    __syncthreads();
    RB_P(3)
    // 4. which pairs overlap by more than 0.5 (original sigmas: a pair with a pruned member never changes anything)
    if (SMALL && np > CP::LDS_PAIRS) {                                       // more pairs than the small set tables order: the full kernel's
        if (lane == 0) a.kp_n[ls] = RT_BLOBS_REDO;
        return 1;
    }
    const bool lds_set = np <= CP::LDS_PAIRS, lds_pl = np <= CP::NPL;
    uint32_t *ovb = lds_set ? L.ovbits : a.ovbits + (int64_t)ls * ((BP_MAX_PAIRS + 31) / 32 + 1);
    for (int w0 = 0; w0 < np; w0 += 64) {
        const int k = w0 + lane;
        bool ov = false;
        if (k < np) {
            const uint32_t pr = lds_pl ? L.pl[k] : pairs[k];
            const int i = (int)(pr >> 16), j = (int)(pr & 0xffffu);
            ov = bp_overlaps((double)L.xy[2 * i], (double)L.xy[2 * i + 1], L.lay[i] == 2 ? a.sigma2 : a.sigma1,
                             (double)L.xy[2 * j], (double)L.xy[2 * j + 1], L.lay[j] == 2 ? a.sigma2 : a.sigma1, 0.5);
        }
        const uint64_t bal = __ballot(ov);
        if (lane == 0) { ovb[w0 >> 5] = (uint32_t)bal; ovb[(w0 >> 5) + 1] = (uint32_t)(bal >> 32); }
    }
    __syncthreads();
    RB_P(4)
    // 5. Python-set iteration order of the pairs + the sequential pruning pass, then 6. NumPy-1.22 argsort of the sigmas
    uint16_t *order = a.order + (int64_t)ls * (BP_MAX_PAIRS + 1);
    {
        int m;
        if (lds_pl) m = rb_pyset_order_wave<true>(L.pl, np, L.tabA, CP::CAPA, L.tabB, CP::CAPB, order, lane);
        else if (lds_set) m = rb_pyset_order_wave<true>(pairs, np, L.tabA, CP::CAPA, L.tabB, CP::CAPB, order, lane);
        else {
            uint16_t *big = a.bigtab + (int64_t)ls * 2 * 131072;
            m = rb_pyset_order_wave<false>(pairs, np, big, 131072, big + 131072, 131072, order, lane);
        }
        if (m != np) flags |= RT_F_PAIR_OVERFLOW;
        if (lane == 0) L.vals[2] = m < 0 ? 0 : m;
    }
    __syncthreads();
    RB_P(5)
    // the overlapping pairs in set order, gathered by the whole wave (the hash tables are free again: 4096 pairs fit in tabB);
    // the sequential pass then walks LDS only - one lane chasing order[k] -> pairs[q] through global memory was 2/3 of this kernel
    const int m = L.vals[2];
    uint32_t *cl = reinterpret_cast<uint32_t *>(L.tabB);
    int ncl = 0;
    for (int k0 = 0; k0 < m; k0 += 64) {
        const int k = k0 + lane;
        bool ov = false;
        uint32_t pr = 0;
        if (k < m) {
            const int q = order[k];
            ov = (ovb[q >> 5] >> (q & 31)) & 1u;
            if (ov) pr = lds_pl ? L.pl[q] : pairs[q];
        }
        const uint64_t bal = __ballot(ov);
        const int o = ncl + __popcll(bal & ((1ull << lane) - 1ull));
        if (ov && o < CP::NCL) cl[o] = pr;
        ncl += __popcll(bal);
    }
    __syncthreads();
    if (lane == 0) {
        if (ncl <= CP::NCL) {
            for (int k = 0; k < ncl; k++) {
                const uint32_t pr = cl[k];
                const int i = (int)(pr >> 16), j = (int)(pr & 0xffffu);
                if (L.lay[i] == 0 || L.lay[j] == 0) continue;
                if (L.lay[i] > L.lay[j]) L.lay[j] = 0; else L.lay[i] = 0;     // sigma_i > sigma_j ? prune j : prune i (ties: i)
            }
        } else {
            for (int k = 0; k < m; k++) {
                const int q = order[k];
                if (!((ovb[q >> 5] >> (q & 31)) & 1u)) continue;
                const uint32_t pr = pairs[q];
                const int i = (int)(pr >> 16), j = (int)(pr & 0xffffu);
                if (L.lay[i] == 0 || L.lay[j] == 0) continue;
                if (L.lay[i] > L.lay[j]) L.lay[j] = 0; else L.lay[i] = 0;
            }
        }
        L.vals[1] = flags;
    }
    __syncthreads();
    RB_P(6)
    // survivors in response order (reuse xy / lay in place: a chunk of 64 is read before anything of it is overwritten, and what it writes
    // lies at or below its own positions), then sorted by sigma with NumPy 1.22's tie order.  (On lane 0 this loop was ~40 us of a lone
    // detection: 530 dependent LDS round trips.)
    int mb = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int ly = i < n ? (int)L.lay[i] : 0;
        const int16_t x = i < n ? L.xy[2 * i] : (int16_t)0, y = i < n ? L.xy[2 * i + 1] : (int16_t)0;
        const uint64_t bal = __ballot(ly != 0);
        __syncthreads();
        if (ly) { const int o = mb + __popcll(bal & ((1ull << lane) - 1ull)); L.xy[2 * o] = x; L.xy[2 * o + 1] = y; L.lay[o] = (uint8_t)ly; }
        mb += __popcll(bal);
        __syncthreads();
    }
    RB_P(7)
    rb_aquicksort_wave(L.lay, mb, L.idx, lane, L.st, reinterpret_cast<uint16_t *>(L.pl), reinterpret_cast<uint16_t *>(L.pl) + CP::NP);
    RB_P(8)
    for (int q = lane; q < mb; q += 64) {
        const int i = L.idx[q];
        kp[3 * q] = (double)L.xy[2 * i]; kp[3 * q + 1] = (double)L.xy[2 * i + 1]; kp[3 * q + 2] = L.lay[i] == 2 ? a.sigma2 : a.sigma1;
    }
    if (lane == 0) { a.kp_n[ls] = mb; a.slot_flags[ls] = L.vals[1]; }
    RB_P(9)
#ifdef RB_EXP_PROF
    if (lane == 0) for (int k = 0; k < 12; k++) atomicAdd(&rb_prof[k], rbp_[k]);
    if (lane == 0) { atomicAdd(&rb_prof[12], 1ull); atomicAdd(&rb_prof[13], (unsigned long long)n); atomicAdd(&rb_prof[14], (unsigned long long)mb); }
#endif
    return 0;
}

// large batches: every detection through the small class (33 KB of LDS: four per CU), then the few it left through the full one (64 KB)
template <bool SMALL>
__global__ __launch_bounds__(64) void rt_blobs_kernel(RtArgs a, int first)
{
    __shared__ RtBlobLds<SMALL> L;
    rt_blobs_body<SMALL>(a, first, L, false);
}
// small batches (a single sequence's lone detection): K4 (candidate order), K5 (both classes) and K6 (SSC) of a detection in ONE launch,
// one wavefront - three kernels less in the chain every step enqueues whether or not a lane re-detects (a kernel that only returns costs
// 4-6 us of the device and of the enqueuing thread; a single sequence's pair is 290 us).  The full class's LDS per workgroup; the same
// code, so the same results; K4 on 64 threads instead of 256 costs a lone detection ~10 us.
__global__ __launch_bounds__(64) void rt_book_kernel(RtArgs a, int first)
{
    __shared__ union U_ {
        RtBlobLds<true> s; RtBlobLds<false> f;
        struct { uint32_t key[BP_MAX_PTS]; double val[BP_MAX_PTS]; } e;
        uint32_t bitmap[SSC_BATCH_BITMAP_BYTES / 4];
        __device__ U_() {}
    } L;
    const int ls = blockIdx.x, slot = first + ls, lane = threadIdx.x;
    if (slot >= *a.rt_n) return;
    {   // K4 (rt_emit_kernel)
        const int n = min(a.cand_n[ls], BP_MAX_PTS);
        uint32_t *crc = a.cand_rc + (int64_t)ls * BP_MAX_PTS;
        double *cval = a.cand_val + (int64_t)ls * BP_MAX_PTS;
        for (int i = lane; i < n; i += 64) { L.e.key[i] = crc[i]; L.e.val[i] = cval[i]; }
        __syncthreads();
        for (int i0 = lane; i0 < n; i0 += 256) {
            uint32_t k[4];
            int rank[4] = {0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; u++) k[u] = i0 + 64 * u < n ? L.e.key[i0 + 64 * u] : 0u;
            for (int j = 0; j < n; j++) {
                const uint32_t kj = L.e.key[j];
#pragma unroll
                for (int u = 0; u < 4; u++) rank[u] += kj < k[u] ? 1 : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (i0 + 64 * u < n) { crc[rank[u]] = k[u]; cval[rank[u]] = L.e.val[i0 + 64 * u]; }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");                   // the lists are read back (by other lanes) right below
        __syncthreads();
    }
    if (rt_blobs_body<true>(a, first, L.s, false)) {
        __syncthreads();
        rt_blobs_body<false>(a, first, L.f, true);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __syncthreads();
    // K6 (ssc_batch_kernel)
    const int nk = min(a.kp_n[ls], BP_MAX_PTS);
    if (nk <= 0) { if (lane == 0) a.sel_n[ls] = 0; return; }
    ssc_body(a.kp + (int64_t)ls * BP_MAX_PTS * 3, nk, 200, 0.1, a.W, a.W, a.ssc_work + (int64_t)ls * 4 * BP_MAX_PTS,
             a.sel + (int64_t)ls * BP_MAX_PTS, a.sel_n + ls, L.bitmap, SSC_BATCH_BITMAP_BYTES);
}

hipError_t launch_retrack_emit(hipStream_t st, const RtArgs &a, int P)
{
    hipLaunchKernelGGL(rt_emit_kernel, dim3(P), dim3(256), 0, st, a, 0);
    return hipGetLastError();
}

hipError_t launch_retrack_bookkeeping(hipStream_t st, const RtArgs &a, int B, hipEvent_t after_order)
{
    RtArgs ab = a;
    ab.blob_order = nullptr;
    if (B < 256) {
        hipLaunchKernelGGL(rt_book_kernel, dim3(B), dim3(64), 0, st, ab, 0);                 // K4 + K5 + K6 in one launch
        return hipGetLastError();
    }
    hipLaunchKernelGGL(rt_emit_kernel, dim3(B), dim3(256), 0, st, a, 0);
    // the bookkeeping is one latency-bound wavefront per detection and its time grows with the candidate list: longest lists first
    // (in the default step 2.1 -> ... ms for the kernel; the work is the same, the tail is not)
    if (B >= 512 && a.blob_order_buf) {
        if (hipError_t e = launch_order_by_count(st, a.cand_n, B, BP_MAX_PTS, a.blob_order_buf, 1); e != hipSuccess) return e;
        ab.blob_order = a.blob_order_buf;
    }
    if (hipError_t e = after_order ? hipEventRecord(after_order, st) : hipSuccess; e != hipSuccess) return e;      // (front-end kernels of later steps wait for it)
    hipLaunchKernelGGL(rt_blobs_kernel<true>, dim3(B), dim3(64), 0, st, ab, 0);
    hipLaunchKernelGGL(rt_blobs_kernel<false>, dim3(B), dim3(64), 0, st, ab, 0);
    return launch_ssc_batch(st, a.kp, (int64_t)BP_MAX_PTS * 3, a.kp_n, BP_MAX_PTS, B, 200, 0.1, a.W, a.W, a.ssc_work, a.sel, a.sel_n, a.rt_n, 0);
}
