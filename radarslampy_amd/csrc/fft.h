// fft.h - what the units of the Fourier family share: the mixed-radix FFT (fft.hip) and the correlation core on top of it
// (phasecorr.hip), which fmt.hip drives for the Fourier-Mellin passes; internal.  Overview: fft.hip.
#pragma once
#include "roam_internal.h"

#define FFT_MAX_N 4096
#define FFT_TRY(call) do { const int32_t rc_ = (call); if (rc_ != ROAM_OK) return rc_; } while (0)
#define FFT_UNIT __attribute__((visibility("hidden")))       // host functions that cross a unit, kept out of the library's symbol table

// ---- fft.hip.  fft_rows: the forward (or unscaled inverse) FFT of total_rows contiguous rows of length n = 2^a 3^b 5^c <= FFT_MAX_N;
// re_in or im_in may be null (zeros), re_out or im_out may be null (not stored); in and out may be the same planes.
// fft_transpose: (batch) M x N -> N x M, both planes.  fft_twiddles: the table of length n, made on first use (null: error text set)
FFT_UNIT int32_t fft_rows(roam_ctx *ctx, hipStream_t st, const double *re_in, const double *im_in, double *re_out, double *im_out, int64_t total_rows,
                          int n, bool inverse);
FFT_UNIT int32_t fft_transpose(roam_ctx *ctx, hipStream_t st, const double *re_in, const double *im_in, int batch, int M, int N, double *re_out,
                               double *im_out);
FFT_UNIT const double *fft_twiddles(roam_ctx *ctx, int n);
FFT_UNIT bool fft_smooth(int n);                             // n = 2^a 3^b 5^c <= FFT_MAX_N
FFT_UNIT int optimal_dft_size(int n);                        // cv2.getOptimalDFTSize: the smallest 2^a 3^b 5^c >= n
void roam_fft_release(roam_ctx *ctx);                        // free the context's twiddle tables

// ---- phasecorr.hip.  cv2.createHanningWindow's float64 factor per row or column of a side of n (host)
void roam_hanning_factors(int n, double *w);

// the 7 nb planes of a chunk of nb correlations, pl = nb M N doubles each: windowed image | work re, im | F1 re, im | F2 re, im
struct PcPlanes {
    double *a, *tr, *ti, *F[2][2];
};
static inline PcPlanes pc_planes(double *base, size_t pl)
{
    return {base, base + pl, base + 2 * pl, {{base + 3 * pl, base + 4 * pl}, {base + 5 * pl, base + 6 * pl}}};
}

// the grid of pc_peak_partial_kernel: indices per block, blocks per plane (at most 1024)
struct PcPeakGrid {
    int per, nblk;
};
static inline PcPeakGrid pc_peak_grid(size_t nmn)
{
    const int per = (int)((nmn + 1023) / 1024) < 1024 ? 1024 : (int)((nmn + 1023) / 1024);
    return {per, (int)((nmn + per - 1) / per)};
}

// the device workspace of a chunk of correlations: the planes' base, the peak search's partial maxima (chunk x nblk), the results
// (3 per correlation: dx, dy, response), and the bytes of each for `chunk` correlations on planes of nmn = M N doubles
struct PcWork {
    double *f, *pv;
    int *pi;
    double *out;
};
struct PcWorkBytes {
    size_t f, pv, pi, out;
};
static inline PcWorkBytes pc_work_bytes(size_t nmn, size_t chunk)
{
    const size_t nblk = (size_t)pc_peak_grid(nmn).nblk;
    return {sizeof(double) * 7 * nmn * chunk, sizeof(double) * nblk * chunk, sizeof(int) * nblk * chunk, sizeof(double) * 3 * chunk};
}

// the parts of one device slab in the order they are taken, each on a 256-byte boundary; a null base only counts (every part null),
// and so does a part of no bytes.  off = the bytes taken so far
struct Slab {
    uint8_t *base;
    size_t off = 0;
    template <class T> T *take(size_t bytes)
    {
        T *p = base && bytes ? (T *)(base + off) : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    }
};

static inline PcWork pc_work_take(Slab &s, const PcWorkBytes &b)
{
    return {s.take<double>(b.f), s.take<double>(b.pv), s.take<int>(b.pi), s.take<double>(b.out)};
}

// pairs per chunk: 2000 MiB of scratch at bytes_per_pair, at least one, at most n and cap (the grid's z extent).  env: the tests' smaller
// chunk from ROAM_FMT_BATCH_CHUNK (read per call)
FFT_UNIT size_t pc_chunk(size_t bytes_per_pair, size_t n, size_t cap, bool env);
// The correlation of nb pairs, 12 launches on st: win0 / win1 hold the nb windowed, zero-padded M x N sources / targets (planes of
// w.f: a, and F2 re - which nothing touches before its own row pass has consumed it) -> w.out[3 b] = {dx, dy, response}
FFT_UNIT int32_t pc_correlate(roam_ctx *ctx, hipStream_t st, int nb, int M, int N, const PcWork &w, const double *win0, const double *win1);
