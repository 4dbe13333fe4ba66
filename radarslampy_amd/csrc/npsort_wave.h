// npsort_wave.h - np.argsort of NumPy 1.22.3 (npy_aquicksort) by one wavefront, on any key type.  The reference pins numpy 1.22.3
// and two of its results depend on that sort's order among equal keys: getFeatures.adaptiveNMS (the two-valued sigmas, retrack_blobs.hip)
// and scipy.signal.find_peaks(distance=...) (the priority order of equal peak heights, peaks_cond.hip).  The sequential pieces are
// blobprune.h's bp_aheapsort / bp_aquicksort_range.  Include after a definition of __syncthreads / __ballot (hip_runtime).
#pragma once
#include <stdint.h>
#include "blobprune.h"

// np.argsort of NumPy 1.22 (npy_aquicksort) by the whole wavefront: tosort = the permutation bp_aquicksort leaves, element for element.
// Quicksort's segments are disjoint, so the order they are processed in does not matter - only each segment's depth budget does (a child's
// is its parent's minus one; the budget is checked on segments that come off the stack, i.e. the LARGER child of a partition and the whole
// array).  Segments of more than QS_WAVE_MIN elements are partitioned by all lanes (median of three on uniform values, then the Hoare
// loop as the two ordered lists of stop positions: L = positions in (pl, pr) whose key is not below the pivot, R = positions in [pl, pr - 1)
// whose key is not above it, read from the right; the loop swaps L[i] with R[i] while L[i] < R[i] and ends at min(L[k], R[k - 1]) -
// tests/test_parallel_partition_model.py); the smaller ones are sorted one lane per segment, all at once, by the sequential code.
// 530 two-valued sigmas on one lane were ~100 us of a lone detection's bookkeeping.  work: 3 x 256 ints, Lp / Rp: num uint16 each.
#define QS_WAVE_MIN 64
// KEY: the sort key (any type with operator<); the wave compares KV copies of it: int for integer codes (as retrack_blobs.hip has always
// done), the key itself otherwise
template <typename KEY> struct NpWaveKey { typedef KEY type; };
template <> struct NpWaveKey<uint8_t> { typedef int type; };
template <typename KEY>
__device__ void rb_aquicksort_wave(const KEY *v, int num, int16_t *ts, int lane, int *work, uint16_t *Lp, uint16_t *Rp)
{
    typedef typename NpWaveKey<KEY>::type KV;
    for (int i = lane; i < num; i += 64) ts[i] = (int16_t)i;
    __syncthreads();
    if (num < 2) return;
    int cdepth = 0;
    for (int k = num; k > 1; k >>= 1) cdepth++;
    cdepth *= 2;
    // work[3k..3k+2] = (pl, pr, cdepth << 1 | popped); big segments are taken from the top, small ones collected from the bottom of the
    // second half (at most num / 17 + 1 leaves of 17+ elements and as many pending segments: 256 entries hold 2048 keys)
    int sp = 0, nsmall = 0;
    int *small = work + 3 * 128;
    int pl = 0, pr = num - 1, cd = cdepth;
    bool popped = true;
    const uint64_t below = (1ull << lane) - 1ull;
    for (;;) {
        if (pr - pl <= QS_WAVE_MIN || nsmall + sp + 2 >= 128) {           // (the second condition cannot arise; a full list would only cost time)
            if (lane == 0) { small[3 * nsmall] = pl; small[3 * nsmall + 1] = pr; small[3 * nsmall + 2] = cd * 2 + (popped ? 1 : 0); }
            nsmall++;
        } else if (popped && cd < 0) {
            if (lane == 0) bp_aheapsort(v, ts + pl, pr - pl + 1);
            __syncthreads();
        } else {
            const int pm = pl + ((pr - pl) >> 1);
            int a = ts[pl], b = ts[pm], c = ts[pr];                        // (uniform reads)
            if (v[b] < v[a]) { const int t = a; a = b; b = t; }
            if (v[c] < v[b]) { const int t = c; c = b; b = t; }
            if (v[b] < v[a]) { const int t = a; a = b; b = t; }
            const KV vp = v[b];
            const int old = ts[pr - 1];
            __syncthreads();
            if (lane == 0) { ts[pl] = (int16_t)a; ts[pr] = (int16_t)c; ts[pm] = (int16_t)old; ts[pr - 1] = (int16_t)b; }
            if (pm == pr - 1 && lane == 0) ts[pm] = (int16_t)b;          // (never: pr - pl > 64)
            __syncthreads();
            int nL = 0, nR = 0;
            for (int c0 = pl; c0 < pr; c0 += 64) {
                const int pos = c0 + lane;
                const bool in = pos < pr;
                const KV k = in ? (KV)v[ts[pos]] : (KV)0;
                const bool ge = in && pos > pl && !(k < vp), le = in && pos < pr - 1 && !(vp < k);
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
                if (__popcll(bal) < min(64, nm - i0)) break;
            }
            for (int i = lane; i < kk; i += 64) { const int x = Lp[i], y = Rp[nR - 1 - i]; const int16_t t = ts[x]; ts[x] = ts[y]; ts[y] = t; }
            const int pi = kk == 0 ? (int)Lp[0] : min((int)Lp[kk], (int)Rp[nR - kk]);
            __syncthreads();
            if (lane == 0) { const int16_t t = ts[pi]; ts[pi] = ts[pr - 1]; ts[pr - 1] = t; }
            __syncthreads();
            cd--;
            int ql, qr;                                                   // the larger part goes to the stack, the smaller one is next
            if (pi - pl < pr - pi) { ql = pi + 1; qr = pr; pr = pi - 1; }
            else { ql = pl; qr = pi - 1; pl = pi + 1; }
            if (lane == 0) { work[3 * sp] = ql; work[3 * sp + 1] = qr; work[3 * sp + 2] = cd; }
            sp++;
            popped = false;
            continue;
        }
        if (sp == 0) break;
        sp--;
        __syncthreads();
        pl = work[3 * sp]; pr = work[3 * sp + 1]; cd = work[3 * sp + 2];
        popped = true;
    }
    __syncthreads();
    for (int k = lane; k < nsmall; k += 64) {
        const int a = small[3 * k], b = small[3 * k + 1], c = small[3 * k + 2];
        bp_aquicksort_range(v, ts, a, b, c >> 1, (c & 1) != 0);
    }
    __syncthreads();
}
