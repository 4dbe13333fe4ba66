// peaks_common.h - device helpers of the polar peak kernels (peaks.hip: the plain detection, peaks_cond.hip: the one with
// scipy.signal.find_peaks' distance / prominence conditions): the u8 power decode, block / wave scans and NumPy's float32 pairwise
// summation order, which the mean + std threshold of getPointCloud.py:37-45 depends on.
#pragma once
#include "roam_internal.h"

// (float)k / 255.f for a power code k, exactly (see tests/test_abi_cpu.py::test_u8_decode_identity)
__device__ __forceinline__ float code_to_f32_pk(uint32_t k) { return (float)__dmul_rn((double)k, 1.0 / 255.0); }

__device__ __forceinline__ int block_excl_scan(int v, int *sh, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int n = __shfl_up(inc, d);
        if (lane >= d) inc += n;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; i++) {
        int s = sh[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// NumPy pairwise_sum leaf (n <= 128), float32, round-to-nearest, no contraction
__device__ __forceinline__ float np_leaf_sum(const float *a, int n)
{
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; i++) res = __fadd_rn(res, a[i]);
        return res;
    }
    float r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    const int nn = n - (n & 7);
    for (i = 8; i < nn; i += 8) {
        r0 = __fadd_rn(r0, a[i + 0]); r1 = __fadd_rn(r1, a[i + 1]);
        r2 = __fadd_rn(r2, a[i + 2]); r3 = __fadd_rn(r3, a[i + 3]);
        r4 = __fadd_rn(r4, a[i + 4]); r5 = __fadd_rn(r5, a[i + 5]);
        r6 = __fadd_rn(r6, a[i + 6]); r7 = __fadd_rn(r7, a[i + 7]);
    }
    float res = __fadd_rn(__fadd_rn(__fadd_rn(r0, r1), __fadd_rn(r2, r3)),
                          __fadd_rn(__fadd_rn(r4, r5), __fadd_rn(r6, r7)));
    for (; i < n; i++) res = __fadd_rn(res, a[i]);
    return res;
}

// NumPy's recursion for length n: split at n2 = n/2 - (n/2)%8 while n > 128.  The recursion is
// unrolled at compile time (depth <= 6 covers n <= 8192); n is block-uniform, so the whole walk
// is scalar work that every thread repeats for itself - no LDS stack, no serial thread-0 section
// (the first version kept an explicit stack in LDS: ~12 us of dependent LDS latency per row).
template <int D>
struct PwWalk {
    // leaf number `target` of the in-order leaf sequence -> (my_lo, my_n)
    static __device__ __forceinline__ void select(int lo, int n, int target, int &cnt, int &my_lo, int &my_n)
    {
        if (n <= 128) { if (cnt == target) { my_lo = lo; my_n = n; } cnt++; return; }
        int n2 = n / 2; n2 -= n2 % 8;
        PwWalk<D - 1>::select(lo, n2, target, cnt, my_lo, my_n);
        PwWalk<D - 1>::select(lo + n2, n - n2, target, cnt, my_lo, my_n);
    }
    static __device__ __forceinline__ float combine(const float *leaf_sum, int n, int &li)
    {
        if (n <= 128) return leaf_sum[li++];
        int n2 = n / 2; n2 -= n2 % 8;
        const float a = PwWalk<D - 1>::combine(leaf_sum, n2, li);
        const float b = PwWalk<D - 1>::combine(leaf_sum, n - n2, li);
        return __fadd_rn(a, b);
    }
};
template <>
struct PwWalk<0> {
    static __device__ __forceinline__ void select(int lo, int n, int target, int &cnt, int &my_lo, int &my_n)
    {
        if (cnt == target) { my_lo = lo; my_n = n; }
        cnt++;
    }
    static __device__ __forceinline__ float combine(const float *leaf_sum, int, int &li) { return leaf_sum[li++]; }
};

// block-wide NumPy-ordered float32 sum of a[0..n) (a and leaf_sum in LDS); every thread gets the result
__device__ __forceinline__ float block_np_sum(float *leaf_sum, const float *a, int n)
{
    int cnt = 0, my_lo = 0, my_n = -1;
    PwWalk<6>::select(0, n, (int)threadIdx.x, cnt, my_lo, my_n);
    if (my_n >= 0) leaf_sum[threadIdx.x] = np_leaf_sum(a + my_lo, my_n);
    __syncthreads();
    int li = 0;
    const float r = PwWalk<6>::combine(leaf_sum, n, li);
    __syncthreads();
    return r;
}

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_excl_scan(int v, int lane, int *total)
{
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(inc, d);
        if (lane >= d) inc += n;
    }
    *total = __shfl(inc, 63);
    return inc - v;
}
