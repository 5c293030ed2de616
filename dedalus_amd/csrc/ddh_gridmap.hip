// Pointwise grid-space maps and broadcasts (HBM-bound), gfx950.
//  - ddh_grid_map:        out[i] = f(in[i])  for the ufuncs of UnaryGridFunction (operators.py:505-566) and the constant
//                         exponents of Power (operators.py:306-400)
//  - ddh_grid_broadcast:  a field that lacks some bases expanded to the full grid of a product (arithmetic.py:560-640:
//                         the reference broadcasts the operands of MultiplyFields with NumPy)
// The maps are one read and one write with 16-byte accesses, launched like ddh_lincomb (ddh_grid.hip): at eight resident
// waves per SIMD a plain grid-stride loop of one 16-byte word per lane already streams at the copy rate there, so the loop
// is not unrolled -- the cheap ops stay small and the transcendental ones are not inlined several times over.
#include <atomic>

#include "ddh_common.h"

namespace ddh {

static std::atomic<long> g_map_launches{0};

constexpr int MAP_POWI = DDH_MAP_POW + 1;       // internal: integer exponent by repeated multiplication
constexpr int MAP_POWI_MAX = 8;                 // |p| up to here; larger integer exponents take pow()

template <int OP>
__device__ __forceinline__ double map_op(double x, double p, int ip) {
    if constexpr (OP == DDH_MAP_ABSOLUTE) return fabs(x);
    else if constexpr (OP == DDH_MAP_SIGN) return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x));      // np.sign: -0 -> +0, NaN -> NaN
    else if constexpr (OP == DDH_MAP_EXP) return exp(x);
    else if constexpr (OP == DDH_MAP_EXP2) return exp2(x);
    else if constexpr (OP == DDH_MAP_LOG) return log(x);
    else if constexpr (OP == DDH_MAP_LOG2) return log2(x);
    else if constexpr (OP == DDH_MAP_LOG10) return log10(x);
    else if constexpr (OP == DDH_MAP_SQRT) return sqrt(x);
    else if constexpr (OP == DDH_MAP_SQUARE) return x * x;
    else if constexpr (OP == DDH_MAP_SIN) return sin(x);
    else if constexpr (OP == DDH_MAP_COS) return cos(x);
    else if constexpr (OP == DDH_MAP_TAN) return tan(x);
    else if constexpr (OP == DDH_MAP_ARCSIN) return asin(x);
    else if constexpr (OP == DDH_MAP_ARCCOS) return acos(x);
    else if constexpr (OP == DDH_MAP_ARCTAN) return atan(x);
    else if constexpr (OP == DDH_MAP_SINH) return sinh(x);
    else if constexpr (OP == DDH_MAP_COSH) return cosh(x);
    else if constexpr (OP == DDH_MAP_TANH) return tanh(x);
    else if constexpr (OP == DDH_MAP_ARCSINH) return asinh(x);
    else if constexpr (OP == DDH_MAP_ARCCOSH) return acosh(x);
    else if constexpr (OP == DDH_MAP_ARCTANH) return atanh(x);
    else if constexpr (OP == DDH_MAP_RECIP) return 1.0 / x;
    else if constexpr (OP == DDH_MAP_POW) return pow(x, p);
    else {
        // x^ip, 1 <= |ip| <= MAP_POWI_MAX: |ip| - 1 multiplications in sequence, then one division for ip < 0 --
        // relative error (|ip| - 1 + [ip < 0]) u
        const int m = ip < 0 ? -ip : ip;
        double r = x;
        for (int k = 1; k < m; ++k) r *= x;
        return ip < 0 ? 1.0 / r : r;
    }
}

// out == in is allowed (every lane reads its words before it writes them), hence no __restrict__.
template <int OP>
__global__ void __launch_bounds__(256) map_kernel(double *out, const double *in, long n, double p, int ip, int vec) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    if (vec) {
        const long n2 = n >> 1;
        for (long i = tid; i < n2; i += stride) {
            double2 v = reinterpret_cast<const double2 *>(in)[i];
            v.x = map_op<OP>(v.x, p, ip);
            v.y = map_op<OP>(v.y, p, ip);
            reinterpret_cast<double2 *>(out)[i] = v;
        }
        if ((n & 1) && tid == 0) out[n - 1] = map_op<OP>(in[n - 1], p, ip);
    } else {
        for (long i = tid; i < n; i += stride) out[i] = map_op<OP>(in[i], p, ip);
    }
}

struct BcastArgs {
    long shape[3];      // storage axis lengths of the output
    long stride[3];     // element stride of the operand along each axis, 0 where it lacks the axis
    long cstride;       // operand elements per component
};

// flat output element -> operand element; i2_out: the index along the last axis
template <typename IDX>
__device__ __forceinline__ long bcast_src(IDX e, const BcastArgs &a, IDX &i2_out) {
    const IDX s2 = (IDX)a.shape[2], s1 = (IDX)a.shape[1], s0 = (IDX)a.shape[0];
    IDX r = e / s2;
    const IDX i2 = e - r * s2;
    IDX q = r / s1;
    const IDX i1 = r - q * s1;
    r = q;
    q = r / s0;
    const IDX i0 = r - q * s0;
    i2_out = i2;
    return (long)q * a.cstride + (long)i0 * a.stride[0] + (long)i1 * a.stride[1] + (long)i2 * a.stride[2];
}

// One 16-byte word of the output per lane and round; the operand is small and comes from the caches.  IDX: 32-bit index
// arithmetic where the output has fewer than 2^32 elements (three integer divisions per word).
template <typename IDX>
__global__ void __launch_bounds__(256)
broadcast_kernel(double *__restrict__ out, const double *__restrict__ in, long n, BcastArgs a, int vec) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    IDX i2;
    if (vec) {
        const long n2 = n >> 1;
        for (long i = tid; i < n2; i += stride) {
            const IDX e = (IDX)(2 * i);
            const long s = bcast_src<IDX>(e, a, i2);
            IDX dummy;
            // the second element: the neighbour along the last axis, or the start of the next row
            const long s1 = ((long)i2 + 1 < a.shape[2]) ? s + a.stride[2] : bcast_src<IDX>(e + 1, a, dummy);
            reinterpret_cast<double2 *>(out)[i] = make_double2(in[s], in[s1]);
        }
        if ((n & 1) && tid == 0) out[n - 1] = in[bcast_src<IDX>((IDX)(n - 1), a, i2)];
    } else {
        for (long i = tid; i < n; i += stride) out[i] = in[bcast_src<IDX>((IDX)i, a, i2)];
    }
}

static unsigned map_grid(long work_items) {      // stream_grid() of ddh_grid.hip
    long blocks = (work_items + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

template <int OP>
static void launch_map(double *out, const double *in, long n, double p, int ip, hipStream_t st) {
    const int vec = ((((uintptr_t)out) | ((uintptr_t)in)) & 15) == 0;
    hipLaunchKernelGGL(map_kernel<OP>, dim3(map_grid(vec ? n / 2 : n)), dim3(256), 0, st, out, in, n, p, ip, vec);
}

}  // namespace ddh

using namespace ddh;

extern "C" {

int ddh_grid_map(double *out, const double *in, long n, int op, double param, void *stream) {
    if (op < 0 || op > DDH_MAP_POW) return fail("ddh_grid_map: unknown op " + std::to_string(op));
    if (n <= 0) return 0;
    if (!out || !in) return fail("ddh_grid_map: null pointer");
    hipStream_t st = as_stream(stream);
    int ip = 0;
    if (op == DDH_MAP_POW) {
        // exponents that are one IEEE operation, or a few multiplications, do not pay for pow()
        if (param == 0.5) op = DDH_MAP_SQRT;
        else if (param == -1.0) op = DDH_MAP_RECIP;
        else if (param != 0.0 && param >= -MAP_POWI_MAX && param <= MAP_POWI_MAX && param == (double)(int)param) {
            op = MAP_POWI;
            ip = (int)param;
        }
    }
    switch (op) {
#define DDH_MAP_CASE(OP) case OP: launch_map<OP>(out, in, n, param, ip, st); break;
        DDH_MAP_CASE(DDH_MAP_ABSOLUTE) DDH_MAP_CASE(DDH_MAP_SIGN) DDH_MAP_CASE(DDH_MAP_EXP) DDH_MAP_CASE(DDH_MAP_EXP2)
        DDH_MAP_CASE(DDH_MAP_LOG) DDH_MAP_CASE(DDH_MAP_LOG2) DDH_MAP_CASE(DDH_MAP_LOG10) DDH_MAP_CASE(DDH_MAP_SQRT)
        DDH_MAP_CASE(DDH_MAP_SQUARE) DDH_MAP_CASE(DDH_MAP_SIN) DDH_MAP_CASE(DDH_MAP_COS) DDH_MAP_CASE(DDH_MAP_TAN)
        DDH_MAP_CASE(DDH_MAP_ARCSIN) DDH_MAP_CASE(DDH_MAP_ARCCOS) DDH_MAP_CASE(DDH_MAP_ARCTAN) DDH_MAP_CASE(DDH_MAP_SINH)
        DDH_MAP_CASE(DDH_MAP_COSH) DDH_MAP_CASE(DDH_MAP_TANH) DDH_MAP_CASE(DDH_MAP_ARCSINH) DDH_MAP_CASE(DDH_MAP_ARCCOSH)
        DDH_MAP_CASE(DDH_MAP_ARCTANH) DDH_MAP_CASE(DDH_MAP_RECIP) DDH_MAP_CASE(DDH_MAP_POW) DDH_MAP_CASE(MAP_POWI)
#undef DDH_MAP_CASE
    }
    DDH_HIP(hipGetLastError());
    g_map_launches.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

int ddh_grid_broadcast(double *out, const double *in, int ncomp, const long *shape_h, const int *present_h, void *stream) {
    if (!shape_h || !present_h) return fail("ddh_grid_broadcast: null shape / present");
    if (ncomp < 1) return fail("ddh_grid_broadcast: ncomp >= 1");
    BcastArgs a;
    long npts = 1, src = 1;
    for (int k = 2; k >= 0; --k) {
        if (shape_h[k] < 0) return fail("ddh_grid_broadcast: negative axis length");
        a.shape[k] = shape_h[k];
        a.stride[k] = present_h[k] ? src : 0;
        if (present_h[k]) src *= shape_h[k];
        npts *= shape_h[k];
    }
    a.cstride = src;
    const long n = npts * ncomp;
    if (n <= 0) return 0;
    if (!out || !in) return fail("ddh_grid_broadcast: null pointer");
    const int vec = (((uintptr_t)out) & 15) == 0;
    const dim3 grid(map_grid(vec ? n / 2 : n)), block(256);
    if (n < (1L << 32))
        hipLaunchKernelGGL(broadcast_kernel<uint32_t>, grid, block, 0, as_stream(stream), out, in, n, a, vec);
    else
        hipLaunchKernelGGL(broadcast_kernel<uint64_t>, grid, block, 0, as_stream(stream), out, in, n, a, vec);
    DDH_HIP(hipGetLastError());
    g_map_launches.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

int ddh_grid_map_launches(long *count) {
    if (!count) return fail("ddh_grid_map_launches: null pointer");
    *count = g_map_launches.load(std::memory_order_relaxed);
    return 0;
}

}  // extern "C"
