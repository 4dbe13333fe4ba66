// retrack_geom.h - what the translation units of the device-side feature (re)detection share (the units: retrack.hip); internal, the
// engine sees retrack.h.  Tile sizes, LDS layouts and launch shapes stay private to the unit that holds the kernel.
#pragma once
#include "retrack.h"
#include <algorithm>

// ---- the contract between the integral kernel and the determinant kernel: the strip geometry of rt_det_strip_kernel, from which
// retrack_build_phases (retrack_integral.hip) derives the tiles of the integral image that are ever read
#define SD_T 16                             // position rows per step
#ifndef SD_HALVES
#define SD_HALVES 1                         // 64-column groups per workgroup (8 waves each); 1: two workgroups per CU
#endif
#define SD_PC (64 * SD_HALVES)              // position columns per strip
#define SD_OUT (SD_PC - 2)
#define SD_HL 14                            // lowest / highest box offset of size 30
#define SD_HR 16
#define SD_BC (SD_PC + SD_HL + SD_HR)       // staged columns (158 | 94)
#define SD_BP ((SD_BC + 15) / 16 * 16)      // ring pitch in doubles (160 | 96)
#define SD_DT_WORDS 24                      // words per strip of the dark-step table (the layout: rt_darktab_kernel, retrack_det.hip)

// ---- device code shared by the integral kernels and the fused kernel: which way to the integral image serves a chunk, a pixel's value
__device__ __forceinline__ float rt_code_to_f32(uint32_t k) { return (float)__dmul_rn((double)k, 1.0 / 255.0); }
// (round 5: the float32-only decode of warp.hip - fma(k, head, k * tail) - in place of the table read was tried in the one-sweep kernel's
// taps, with byte reads and with 16-bit reads: 9.1 ms per 512 detections against 6.6 with the table; the table stays)
__device__ __forceinline__ bool rt_one_sweep(const RtArgs &a, int first) { return a.W <= 2048 && *a.rt_n - first >= RT_TWO_PASS_SLOTS; }
struct __attribute__((packed)) RtU16 { uint16_t v; };
struct __attribute__((packed)) RtU32 { uint32_t v; };
// one Cartesian pixel out of the polar record (the arithmetic of warp_gather_kernel's direct path = warp_pixel); lut[k] = rt_code_to_f32(k)
__device__ __forceinline__ float rt_pixel(uint32_t m, const uint8_t *__restrict__ p, int rows, int cols, int stride, const float *lut)
{
    const int ix = m & 4095, iy = (m >> 12) & 1023;
    if (ix >= cols) return 0.f;
    const float wx1 = __fmul_rn((float)((m >> 22) & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
    const float wy1 = __fmul_rn((float)(m >> 27), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
    int r0 = iy - 1, r1 = iy;
    if (r0 < 0) r0 += rows; else if (r0 >= rows) r0 -= rows;
    if (r1 >= rows) r1 -= rows;
    const uint8_t *q0 = p + r0 * stride + ix, *q1 = p + r1 * stride + ix;
    const bool i1 = ix + 1 < cols;
    // in the last column the pair is read one byte to the left and shifted, so that no load leaves the row
    const int back = i1 ? 0 : 1, sh = back * 8;
    const uint32_t w0 = reinterpret_cast<const RtU16 *>(q0 - back)->v >> sh, w1 = reinterpret_cast<const RtU16 *>(q1 - back)->v >> sh;
    const float s00 = lut[w0 & 255], s01 = i1 ? lut[w0 >> 8] : 0.f;        // lut[k] = rt_code_to_f32(k)
    const float s10 = lut[w1 & 255], s11 = i1 ? lut[w1 >> 8] : 0.f;
    float v = __fmul_rn(s00, __fmul_rn(wy0, wx0));
    v = __fadd_rn(v, __fmul_rn(s01, __fmul_rn(wy0, wx1)));
    v = __fadd_rn(v, __fmul_rn(s10, __fmul_rn(wy1, wx0)));
    v = __fadd_rn(v, __fmul_rn(s11, __fmul_rn(wy1, wx1)));
    return v;
}

// ---- entry points between the units (kept out of the library's symbol table)
#define RT_UNIT __attribute__((visibility("hidden")))
RT_UNIT hipError_t retrack_integral_init(), retrack_det_init();      // the kernels' LDS attributes (retrack_init)
// the integral images of the chunk's first P scratch slots: the one-sweep kernel if `one_sweep`, then the two-pass pair (both return at once
// when the chunk is not their regime: only the device knows the number of detections); determinants + maxima of these slots; K1-K3 fused
RT_UNIT hipError_t launch_retrack_integral(hipStream_t st, const RtArgs &a, int first, int P, bool one_sweep);
RT_UNIT hipError_t launch_det(hipStream_t st, const RtArgs &a, int first, int P);
RT_UNIT hipError_t launch_retrack_fused(hipStream_t st, const RtArgs &a, int first, int P, int dbg);
// K4-K6 over all B detections of a step: candidate order, blob bookkeeping, ANMS (after_order: see launch_retrack)
RT_UNIT hipError_t launch_retrack_bookkeeping(hipStream_t st, const RtArgs &a, int B, hipEvent_t after_order);
