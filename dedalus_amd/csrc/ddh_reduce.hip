// Contraction of one storage axis of coefficient data with weight vectors: the device half of the reduced analysis
// tasks (slices b(x=x0), mode-0 gathers for ave / integ along a Fourier axis).
//
//   in [outer][n][inner] (rows of one `outer` index ostride doubles apart), w [nw][n]
//   out[o][j][i] = sum_k w[j][k] * in[o][k][i]          out [outer][nw][inner], contiguous
//
// Reference: InterpolateRealFourier / IntegrateRealFourier / AverageRealFourier (core/basis.py:1227-1300) apply a
// (1 x N) matrix along the axis with apply_matrix (tools/array.py); here the matrix rows are the weight vectors.
//
// Two kernels, both with a FIXED summation order that is a function of n alone (never of the launch shape):
//
//  * line kernel  (inner == 1): one wavefront per line.  Element k belongs to lane (k / 2) % 64; a lane sums its elements
//    in increasing k with fma, then the 64 lane sums are combined by an xor butterfly (32, 16, 8, 4, 2, 1).  16-byte loads
//    where the lines are 16-byte aligned, 8-byte loads otherwise -- the same elements reach the same lane either way.
//    Weights of n <= 1024 stay in registers across the lines a wave handles; no LDS.
//
//  * strided kernel (inner > 1, and the n == 1 gather): lanes run along the flattened (outer, inner) index, so loads are
//    coalesced along inner.  k is cut into chunks of KC = 64 * ceil(n / 1024) (at most 16 chunks); a chunk is summed in
//    increasing k with fma starting from +0, and the chunk sums are added in increasing chunk order.  When outer * inner
//    is too small to fill the device the chunks of a column are spread over the waves of a workgroup and combined through
//    LDS -- in the same chunk order, so the split and the unsplit launch give the same bits.
//
// NaN: every product enters a sum (no early-outs on zero weights), so a NaN in the input reaches every output it feeds.
// Vector stores only, no atomics.
#include <algorithm>

#include "ddh_common.h"

namespace ddh {
namespace {

constexpr int WAVE = 64;
constexpr int MAX_NW = 4;
constexpr int MAX_CHUNKS = 16;
constexpr int SPLIT_WAVES = 8;                  // waves of a split-k workgroup

__host__ __device__ inline int chunk_len(int n) { return 64 * ((n + 1023) / 1024); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

// ---- inner == 1 ------------------------------------------------------------------------------------------------------
// NB > 0: n <= 128 * NB and the weights live in registers; NB == 0: any n, weights re-read (L1 / L2) per line.
template <int NW, int NB, bool VEC>
__global__ void __launch_bounds__(256) contract_line_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                            long outer, int n, long ostride, const double *__restrict__ w) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wave = (long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x / WAVE);
    const long nwaves = (long)gridDim.x * (blockDim.x / WAVE);
    constexpr int RB = NB > 0 ? NB : 1;
    double wr[NW][RB][2];
    if (NB > 0) {
#pragma unroll
        for (int j = 0; j < NW; ++j)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int k = 128 * r + 2 * lane;
                wr[j][r][0] = k < n ? w[(long)j * n + k] : 0.0;
                wr[j][r][1] = k + 1 < n ? w[(long)j * n + k + 1] : 0.0;
            }
    }
    for (long o = wave; o < outer; o += nwaves) {
        const double *line = in + o * ostride;
        double acc[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) acc[j] = 0.0;
        if (NB > 0) {
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int k = 128 * r + 2 * lane;
                if (k < n) {                                    // (n even on the VEC path: k + 1 < n too)
                    double x0, x1 = 0.0;
                    const bool two = k + 1 < n;
                    if (VEC) {
                        const double2 v = *reinterpret_cast<const double2 *>(line + k);
                        x0 = v.x, x1 = v.y;
                    } else {
                        x0 = line[k];
                        if (two) x1 = line[k + 1];
                    }
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        acc[j] = fma(wr[j][r][0], x0, acc[j]);
                        if (two) acc[j] = fma(wr[j][r][1], x1, acc[j]);
                    }
                }
            }
        } else {
            for (int k = 2 * lane; k < n; k += 128) {
                double x0, x1 = 0.0;
                const bool two = k + 1 < n;
                if (VEC) {
                    const double2 v = *reinterpret_cast<const double2 *>(line + k);
                    x0 = v.x, x1 = v.y;
                } else {
                    x0 = line[k];
                    if (two) x1 = line[k + 1];
                }
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    acc[j] = fma(w[(long)j * n + k], x0, acc[j]);
                    if (two) acc[j] = fma(w[(long)j * n + k + 1], x1, acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) acc[j] = wave_sum(acc[j]);
        if (lane < NW) {
            double v = acc[0];
#pragma unroll
            for (int j = 1; j < NW; ++j)
                if (lane == j) v = acc[j];
            out[o * NW + lane] = v;
        }
    }
}

// ---- strided ---------------------------------------------------------------------------------------------------------
// sum of chunk c of column (o, i):  +0 then fma in increasing k
template <int NW>
__device__ __forceinline__ void chunk_sum(const double *__restrict__ col, long inner, const double *__restrict__ w, int n,
                                          int k0, int k1, double (&part)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; ++j) part[j] = 0.0;
    int k = k0;
    for (; k + 8 <= k1; k += 8) {                               // eight loads in flight, summed in increasing k
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = col[(long)(k + u) * inner];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < NW; ++j) part[j] = fma(w[(long)j * n + k + u], x[u], part[j]);   // (w index is wave-uniform)
    }
    for (; k < k1; ++k) {
        const double x = col[(long)k * inner];
#pragma unroll
        for (int j = 0; j < NW; ++j) part[j] = fma(w[(long)j * n + k], x, part[j]);
    }
}

template <int NW>
__global__ void __launch_bounds__(256) contract_strided_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                               long outer, int n, long inner, long ostride,
                                                               const double *__restrict__ w) {
    const long total = outer * inner;
    const int kc = chunk_len(n);
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const long o = t / inner, i = t - o * inner;
        const double *col = in + o * ostride + i;
        double acc[NW], part[NW];
        for (int k0 = 0, c = 0; k0 < n; k0 += kc, ++c) {
            chunk_sum<NW>(col, inner, w, n, k0, min(k0 + kc, n), part);
#pragma unroll
            for (int j = 0; j < NW; ++j) acc[j] = c == 0 ? part[j] : acc[j] + part[j];
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) out[(o * NW + j) * inner + i] = acc[j];
    }
}

// split-k: a workgroup of SPLIT_WAVES waves owns 64 columns; wave s sums chunks s, s + SPLIT_WAVES, ...
template <int NW>
__global__ void __launch_bounds__(SPLIT_WAVES *WAVE) contract_split_kernel(const double *__restrict__ in,
                                                                           double *__restrict__ out, long outer, int n,
                                                                           long inner, long ostride,
                                                                           const double *__restrict__ w) {
    __shared__ double parts[MAX_CHUNKS][NW][WAVE];
    const long total = outer * inner;
    const int kc = chunk_len(n);
    const int nchunks = (n + kc - 1) / kc;
    const int lane = threadIdx.x & (WAVE - 1), s = threadIdx.x / WAVE;
    for (long base = (long)blockIdx.x * WAVE; base < total; base += (long)gridDim.x * WAVE) {     // (block-uniform)
        const long t = base + lane;
        const bool live = t < total;
        const long o = live ? t / inner : 0, i = live ? t - o * inner : 0;
        const double *col = in + o * ostride + i;
        if (live) {
            for (int c = s; c < nchunks; c += SPLIT_WAVES) {
                double part[NW];
                chunk_sum<NW>(col, inner, w, n, c * kc, min((c + 1) * kc, n), part);
#pragma unroll
                for (int j = 0; j < NW; ++j) parts[c][j][lane] = part[j];
            }
        }
        __syncthreads();
        if (live && s < NW) {                                   // wave j combines weight vector j, in chunk order
            double acc = parts[0][s][lane];
            for (int c = 1; c < nchunks; ++c) acc += parts[c][s][lane];
            out[(o * NW + s) * inner + i] = acc;
        }
        __syncthreads();
    }
}

template <int NW>
int launch(const double *in, double *out, long outer, int n, long inner, long ostride, const double *w, hipStream_t s) {
    const long total = outer * inner;
    if (inner == 1 && n > 1) {
        const bool vec = (n % 2 == 0) && (ostride % 2 == 0) && (((uintptr_t)in) & 15) == 0;
        const long blocks = std::min<long>((outer + 3) / 4, 256L * 16);
        const dim3 g((unsigned)blocks), b(256);
#define DDH_LINE(NB)                                                                                              \
    do {                                                                                                          \
        if (vec) hipLaunchKernelGGL((contract_line_kernel<NW, NB, true>), g, b, 0, s, in, out, outer, n, ostride, w); \
        else hipLaunchKernelGGL((contract_line_kernel<NW, NB, false>), g, b, 0, s, in, out, outer, n, ostride, w);    \
    } while (0)
        if (n <= 128) DDH_LINE(1);
        else if (n <= 512) DDH_LINE(4);
        else if (n <= 1024) DDH_LINE(8);
        else DDH_LINE(0);
#undef DDH_LINE
    } else {
        const int kc = chunk_len(n);
        const int nchunks = (n + kc - 1) / kc;
        // fewer columns than eight waves per SIMD of 256 CUs, and more than one chunk to share out: split k
        if (nchunks > 1 && total < 256L * 4 * 8 * WAVE) {
            const long blocks = std::min<long>((total + WAVE - 1) / WAVE, 256L * 8);
            hipLaunchKernelGGL((contract_split_kernel<NW>), dim3((unsigned)blocks), dim3(SPLIT_WAVES * WAVE), 0, s, in, out,
                               outer, n, inner, ostride, w);
        } else {
            const long blocks = std::min<long>((total + 255) / 256, 256L * 16);
            hipLaunchKernelGGL((contract_strided_kernel<NW>), dim3((unsigned)blocks), dim3(256), 0, s, in, out, outer, n,
                               inner, ostride, w);
        }
    }
    return check_hip(hipGetLastError(), "ddh_axis_contract launch");
}

// ---- per-row weights (ddh_axis_contract_rows) ---------------------------------------------------------------------------
// out[o][i] = sum_{k >= kmin[row[o]]} w[row[o]][k] * in[o][k][i]: the weight vector and the first entry that is read depend
// on the outer index (colatitude slices: one row of Y_l^{m,s}(theta0) per (spin weight, m), data from l = max(m, |s|) on).
// Same two regimes and the same chunking of ABSOLUTE k as above, so the summation order of a line is a function of
// (n, kmin) alone: entries below kmin are skipped, not multiplied by zero -- they are never loaded.
//
//  * line kernel: element k belongs to lane (k / 2) % 64 as above; a pair straddling kmin loads its upper half alone.
//  * strided kernels: chunk c covers [max(c KC, kmin), min((c + 1) KC, n)); the sum starts with chunk kmin / KC.  A thread
//    owns V = 2 adjacent columns (16-byte loads) when inner is even and both bases are 16-byte aligned, else one.
// A row index outside 0 .. nrows - 1 reads nothing and writes NaN.

__device__ __forceinline__ bool row_of(const int *__restrict__ row, const int *__restrict__ kmin, long o, int nrows, int n,
                                       int &r, int &k0) {
    r = row[o];
    const bool ok = (unsigned)r < (unsigned)nrows;
    if (!ok) r = 0;
    k0 = ok ? min(max(kmin[r], 0), n) : n;
    return ok;
}

template <bool VEC>
__global__ void __launch_bounds__(256) rows_line_kernel(const double *__restrict__ in, double *__restrict__ out, long outer,
                                                        int n, const double *__restrict__ w, const int *__restrict__ row,
                                                        const int *__restrict__ kmin, int nrows) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wave = (long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x / WAVE);
    const long nwaves = (long)gridDim.x * (blockDim.x / WAVE);
    for (long o = wave; o < outer; o += nwaves) {
        int r, k0;
        const bool ok = row_of(row, kmin, o, nrows, n, r, k0);
        const double *line = in + o * n;
        const double *wr = w + (long)r * n;
        double acc = 0.0;
        for (int k = 2 * lane; k < n; k += 128) {
            if (k + 1 < k0) continue;                           // both entries below kmin
            const bool lo = k >= k0, hi = k + 1 < n;            // (k + 1 >= kmin here)
            double x0 = 0.0, x1 = 0.0;
            if (VEC && lo) {                                    // (n even on the VEC path: hi holds)
                const double2 v = *reinterpret_cast<const double2 *>(line + k);
                x0 = v.x, x1 = v.y;
            } else {
                if (lo) x0 = line[k];
                if (hi) x1 = line[k + 1];
            }
            if (lo) acc = fma(wr[k], x0, acc);
            if (hi) acc = fma(wr[k + 1], x1, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) out[o] = ok ? acc : __builtin_nan("");
    }
}

template <int V>
__device__ __forceinline__ void load_cols(const double *__restrict__ p, double (&x)[V]) {
    if (V == 2) {
        const double2 v = *reinterpret_cast<const double2 *>(p);
        x[0] = v.x, x[V - 1] = v.y;
    } else {
        x[0] = *p;
    }
}

// sum of the entries [k0, k1) of V adjacent columns:  +0 then fma in increasing k
template <int V>
__device__ __forceinline__ void rows_chunk_sum(const double *__restrict__ col, long inner, const double *__restrict__ wr,
                                               int k0, int k1, double (&part)[V]) {
#pragma unroll
    for (int v = 0; v < V; ++v) part[v] = 0.0;
    int k = k0;
    for (; k + 8 <= k1; k += 8) {                               // eight loads in flight, summed in increasing k
        double x[8][V];
#pragma unroll
        for (int u = 0; u < 8; ++u) load_cols<V>(col + (long)(k + u) * inner, x[u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double wk = wr[k + u];
#pragma unroll
            for (int v = 0; v < V; ++v) part[v] = fma(wk, x[u][v], part[v]);
        }
    }
    for (; k < k1; ++k) {
        double x[V];
        load_cols<V>(col + (long)k * inner, x);
        const double wk = wr[k];
#pragma unroll
        for (int v = 0; v < V; ++v) part[v] = fma(wk, x[v], part[v]);
    }
}

template <int V>
__global__ void __launch_bounds__(256) rows_strided_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                           long outer, int n, long inner, const double *__restrict__ w,
                                                           const int *__restrict__ row, const int *__restrict__ kmin,
                                                           int nrows) {
    const long iv = inner / V, items = outer * iv;
    const int kc = chunk_len(n);
    const int nchunks = (n + kc - 1) / kc;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (long)gridDim.x * blockDim.x) {
        const long o = t / iv, i = (t - o * iv) * V;
        int r, k0;
        const bool ok = row_of(row, kmin, o, nrows, n, r, k0);
        const double *col = in + o * n * inner + i;
        const double *wr = w + (long)r * n;
        double acc[V], part[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
        const int c0 = k0 / kc;
        for (int c = c0; c < nchunks; ++c) {
            rows_chunk_sum<V>(col, inner, wr, max(c * kc, k0), min((c + 1) * kc, n), part);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = c == c0 ? part[v] : acc[v] + part[v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) out[o * inner + i + v] = ok ? acc[v] : __builtin_nan("");
    }
}

// split-k: a workgroup of SPLIT_WAVES waves owns 64 items; wave s sums chunks s, s + SPLIT_WAVES, ... of those at or above
// the item's first chunk, wave v < V adds the chunk sums of column v in chunk order
template <int V>
__global__ void __launch_bounds__(SPLIT_WAVES *WAVE) rows_split_kernel(const double *__restrict__ in,
                                                                       double *__restrict__ out, long outer, int n,
                                                                       long inner, const double *__restrict__ w,
                                                                       const int *__restrict__ row,
                                                                       const int *__restrict__ kmin, int nrows) {
    __shared__ double parts[MAX_CHUNKS][V][WAVE];
    const long iv = inner / V, items = outer * iv;
    const int kc = chunk_len(n);
    const int nchunks = (n + kc - 1) / kc;
    const int lane = threadIdx.x & (WAVE - 1), s = threadIdx.x / WAVE;
    for (long base = (long)blockIdx.x * WAVE; base < items; base += (long)gridDim.x * WAVE) {     // (block-uniform)
        const long t = base + lane;
        const bool live = t < items;
        const long o = live ? t / iv : 0, i = live ? (t - o * iv) * V : 0;
        int r = 0, k0 = n;
        bool ok = false;
        if (live) ok = row_of(row, kmin, o, nrows, n, r, k0);
        const int c0 = k0 / kc;
        if (live) {
            const double *col = in + o * n * inner + i;
            const double *wr = w + (long)r * n;
            for (int c = s; c < nchunks; c += SPLIT_WAVES) {
                if (c < c0) continue;
                double part[V];
                rows_chunk_sum<V>(col, inner, wr, max(c * kc, k0), min((c + 1) * kc, n), part);
#pragma unroll
                for (int v = 0; v < V; ++v) parts[c][v][lane] = part[v];
            }
        }
        __syncthreads();
        if (live && s < V) {
            double acc = 0.0;
            if (c0 < nchunks) {
                acc = parts[c0][s][lane];
                for (int c = c0 + 1; c < nchunks; ++c) acc += parts[c][s][lane];
            }
            out[o * inner + i + s] = ok ? acc : __builtin_nan("");
        }
        __syncthreads();
    }
}

template <int V>
void launch_rows_strided(const double *in, double *out, long outer, int n, long inner, const double *w, const int *row,
                         const int *kmin, int nrows, hipStream_t s) {
    const long items = outer * (inner / V);
    const int kc = chunk_len(n);
    const int nchunks = (n + kc - 1) / kc;
    // fewer items than eight waves per SIMD of 256 CUs, and more than one chunk to share out: split k
    if (nchunks > 1 && items < 256L * 4 * 8 * WAVE) {
        const long blocks = std::min<long>((items + WAVE - 1) / WAVE, 256L * 8);
        hipLaunchKernelGGL((rows_split_kernel<V>), dim3((unsigned)blocks), dim3(SPLIT_WAVES * WAVE), 0, s, in, out, outer, n,
                           inner, w, row, kmin, nrows);
    } else {
        const long blocks = std::min<long>((items + 255) / 256, 256L * 16);
        hipLaunchKernelGGL((rows_strided_kernel<V>), dim3((unsigned)blocks), dim3(256), 0, s, in, out, outer, n, inner, w,
                           row, kmin, nrows);
    }
}

int launch_rows(const double *in, double *out, long outer, int n, long inner, const double *w, const int *row,
                const int *kmin, int nrows, hipStream_t s) {
    const bool in16 = (((uintptr_t)in) & 15) == 0;
    if (inner == 1 && n > 1) {
        const long blocks = std::min<long>((outer + 3) / 4, 256L * 16);
        const dim3 g((unsigned)blocks), b(256);
        if (in16 && n % 2 == 0)
            hipLaunchKernelGGL((rows_line_kernel<true>), g, b, 0, s, in, out, outer, n, w, row, kmin, nrows);
        else
            hipLaunchKernelGGL((rows_line_kernel<false>), g, b, 0, s, in, out, outer, n, w, row, kmin, nrows);
    } else if (in16 && inner % 2 == 0) {
        launch_rows_strided<2>(in, out, outer, n, inner, w, row, kmin, nrows, s);
    } else {
        launch_rows_strided<1>(in, out, outer, n, inner, w, row, kmin, nrows, s);
    }
    return check_hip(hipGetLastError(), "ddh_axis_contract_rows launch");
}

}  // namespace
}  // namespace ddh

using namespace ddh;

extern "C" int ddh_axis_contract_rows(const double *in_d, double *out_d, long outer, int n, long inner, const double *w_d,
                                      const int *row_d, const int *kmin_d, int nrows, void *stream) {
    if (!in_d || !out_d || !w_d || !row_d || !kmin_d) return fail("ddh_axis_contract_rows: null pointer");
    if (outer < 1 || n < 1 || inner < 1) return fail("ddh_axis_contract_rows: empty shape");
    if (nrows < 1) return fail("ddh_axis_contract_rows: no weight rows");
    return launch_rows(in_d, out_d, outer, n, inner, w_d, row_d, kmin_d, nrows, as_stream(stream));
}

extern "C" int ddh_axis_contract(const double *in_d, double *out_d, long outer, int n, long inner, long ostride,
                                 const double *w_d, int nw, void *stream) {
    if (!in_d || !out_d || !w_d) return fail("ddh_axis_contract: null pointer");
    if (outer < 1 || n < 1 || inner < 1) return fail("ddh_axis_contract: empty shape");
    if (nw < 1 || nw > MAX_NW) return fail("ddh_axis_contract: 1..4 weight vectors supported");
    if (ostride < (long)n * inner) return fail("ddh_axis_contract: ostride smaller than n * inner");
    hipStream_t s = as_stream(stream);
    switch (nw) {
        case 1: return launch<1>(in_d, out_d, outer, n, inner, ostride, w_d, s);
        case 2: return launch<2>(in_d, out_d, outer, n, inner, ostride, w_d, s);
        case 3: return launch<3>(in_d, out_d, outer, n, inner, ostride, w_d, s);
        default: return launch<4>(in_d, out_d, outer, n, inner, ostride, w_d, s);
    }
}
