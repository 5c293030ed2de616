// Per-ell component mixes of shell tensor fields (transpose, radial and angular components), gfx950.
//
// Fields are [component][2 m + part][ell][n].  A mix is the identity along n: term t maps component ci_t to co_t with one
// real scalar per slot id,
//     y[co][i1][ell][:] = sum_t q[id(i1, ell)][t] * x[ci_t][i1][ell][:],          id = slot_map[i1][ell]
// (id = ell for every slot but the few that the packed layout covers with several ell boxes).  In
// regularity components the scalars are the entries of Q_out(ell)^T P Q_in(ell), P the permutation / selection of spin
// components: SphericalTransposeComponents.subproblem_matrix (core/operators.py:2007-2022, `kron(transpose, eye)`), and on
// spin components P itself: S2RadialComponent / S2AngularComponent (core/basis.py:5892-5969).
//
// Launch shape (the edges tests/shell_tensor_cases.py lists): one workgroup = ELLM_S = 8 consecutive (m, part) slots of one
// ell (threadIdx.y); threadIdx.x runs along the line in units of 16 bytes (two radial modes) when nr is even and both
// buffers are 16-byte aligned, else of one mode: 8 / 16 / 32 threads for <= 8 / <= 16 / more units, further units in a
// loop.  A thread loads the ncomp_in values of its unit once (independent loads, all in flight together) into a private
// column of LDS -- registers cannot be indexed by the term list -- and forms ELLM_CO = 4 output components at a time from
// it, each as one sum in term order: no atomics, the same bits on every call.  Every input element is read from memory
// once, every output element written once.  The scalars of the 8 slot ids and the term table (input component per term,
// first term per output component) are brought to LDS once per workgroup.
// A slot with slot_map < 0 carries no mode: it is never read, and +0 is written to it.
#include "ddh_common.h"

namespace ddh {

constexpr int ELLM_S = 8;     // slots per workgroup
constexpr int ELLM_CO = 4;    // output components formed concurrently
constexpr int ELLM_TX = 32;   // most threads along a line

struct EllMix : HandleBase {
    int nm = 0, nl = 0, nr = 0, ncomp_out = 0, ncomp_in = 0, nterms = 0, nq = 0;
    int *d_ci = nullptr;         // [nterms] (sorted by output component)
    int *d_first = nullptr;      // [ncomp_out + 1]
    int *d_slot = nullptr;       // [2 nm][nl]: row of q, -1: no mode
    double *d_q = nullptr;       // [nq][ntp], ntp = nterms rounded up to even
    ~EllMix() override {
        (void)hipFree(d_ci);
        (void)hipFree(d_first);
        (void)hipFree(d_slot);
        (void)hipFree(d_q);
    }
};

__device__ __forceinline__ void mix_fma(double &a, double q, double x) { a += q * x; }
__device__ __forceinline__ void mix_fma(double2 &a, double q, const double2 &x) { a.x += q * x.x; a.y += q * x.y; }
__device__ __forceinline__ void mix_zero(double &a) { a = 0.0; }
__device__ __forceinline__ void mix_zero(double2 &a) { a.x = 0.0; a.y = 0.0; }

// nu: units (of type V) per line; ntp: stride of a row of q
template <typename V>
__global__ void __launch_bounds__(ELLM_S * ELLM_TX)
ell_mix_kernel(const V *__restrict__ x, V *__restrict__ y, const int *__restrict__ ci, const int *__restrict__ first,
               const int *__restrict__ slot_map, const double *__restrict__ q, int nm, int nl, int nu, int ntp,
               int ncomp_in, int ncomp_out) {
    extern __shared__ double smem[];
    double *sq = smem;                                               // [ELLM_S][ntp]
    V *sx = reinterpret_cast<V *>(smem + ELLM_S * ntp);              // [ncomp_in][threads]; ELLM_S * ntp is even
    const int l = blockIdx.y, i1 = blockIdx.x * ELLM_S + threadIdx.y;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x, nth = blockDim.x * blockDim.y;
    int *sci = reinterpret_cast<int *>(sx + (long)ncomp_in * nth);   // [ntp], then sfirst [ncomp_out + 1]
    int *sfirst = sci + ntp;
    const int id = (i1 < 2 * nm) ? slot_map[i1 * nl + l] : -1;
    double *myq = sq + threadIdx.y * ntp;
    if (id >= 0)
        for (int t = threadIdx.x; t < ntp; t += blockDim.x) myq[t] = q[(long)id * ntp + t];
    for (int t = tid; t < ntp; t += nth) sci[t] = ci[t];             // (ci is padded to ntp entries)
    for (int c = tid; c <= ncomp_out; c += nth) sfirst[c] = first[c];
    __syncthreads();
    if (i1 >= 2 * nm) return;
    const long cstride = 2L * nm * nl * nu, line = ((long)i1 * nl + l) * nu;
    V *mine = sx + tid;
    for (int u = threadIdx.x; u < nu; u += blockDim.x) {
        if (id >= 0)
            for (int c = 0; c < ncomp_in; ++c) mine[(long)c * nth] = x[c * cstride + line + u];
        for (int co0 = 0; co0 < ncomp_out; co0 += ELLM_CO) {
            V acc[ELLM_CO];
#pragma unroll
            for (int j = 0; j < ELLM_CO; ++j) {
                mix_zero(acc[j]);
                const int co = co0 + j;
                if (id >= 0 && co < ncomp_out)
                    for (int t = sfirst[co]; t < sfirst[co + 1]; ++t) mix_fma(acc[j], myq[t], mine[(long)sci[t] * nth]);
            }
#pragma unroll
            for (int j = 0; j < ELLM_CO; ++j)
                if (co0 + j < ncomp_out) y[(co0 + j) * cstride + line + u] = acc[j];
        }
    }
}

static size_t ell_mix_lds(int ntp, int ncomp_in, int ncomp_out, int threads, size_t unit) {
    return (size_t)ELLM_S * ntp * sizeof(double) + (size_t)ncomp_in * threads * unit + (size_t)(ntp + ncomp_out + 1) * sizeof(int);
}

}  // namespace ddh

using namespace ddh;

extern "C" {

int ddh_ell_mix_create(ddh_handle *h, int nm, int nl, int nr, int ncomp_out, int ncomp_in, int nterms, const int *co_h,
                       const int *ci_h, int nq, const double *q_h, const int *slot_map_h) {
    if (nm < 1 || nl < 1 || nr < 1 || ncomp_out < 1 || ncomp_in < 1 || nterms < 0 || nterms > 4096 || nq < 1)
        return fail("ell_mix_create: bad sizes");
    const int ntp = (nterms + 2) & ~1;                    // even and >= 2: the staging area behind it stays 16-byte aligned
    const size_t lds_max = ell_mix_lds(ntp, ncomp_in, ncomp_out, ELLM_S * ELLM_TX, sizeof(double2));
    if (lds_max > 160 * 1024)
        return fail("ell_mix_create: too many components or terms for the LDS staging");
    static size_t lds_opted = 64 * 1024;                      // the attribute belongs to the kernel, not the handle: only raise
    if (lds_max > lds_opted) {                                // opt in here, for the largest launch of either instance
        DDH_HIP(hipFuncSetAttribute((const void *)ell_mix_kernel<double2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        DDH_HIP(hipFuncSetAttribute((const void *)ell_mix_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        lds_opted = lds_max;
    }
    for (long i = 0; i < 2L * nm * nl; ++i)
        if (slot_map_h[i] >= nq) return fail("ell_mix_create: slot map points past the coefficient rows");
    std::vector<int> ci(ntp, 0), first;
    if (int st = term_table("ell_mix_create", nterms, co_h, ci_h, ncomp_out, ncomp_in, first)) return st;
    for (int t = 0; t < nterms; ++t) ci[t] = ci_h[t];
    std::vector<double> q((size_t)nq * ntp, 0.0);         // [nterms][nq] -> [nq][ntp]
    for (int t = 0; t < nterms; ++t)
        for (int i = 0; i < nq; ++i) q[(size_t)i * ntp + t] = q_h[(size_t)t * nq + i];
    EllMix *p = new EllMix();
    p->kind = H_ELLMIX;
    p->nm = nm; p->nl = nl; p->nr = nr; p->ncomp_out = ncomp_out; p->ncomp_in = ncomp_in; p->nterms = nterms; p->nq = nq;
    if (check_hip(hipMalloc((void **)&p->d_ci, ci.size() * sizeof(int)), "hipMalloc") ||
        check_hip(hipMalloc((void **)&p->d_first, first.size() * sizeof(int)), "hipMalloc") ||
        check_hip(hipMalloc((void **)&p->d_slot, 2L * nm * nl * sizeof(int)), "hipMalloc") ||
        check_hip(hipMalloc((void **)&p->d_q, q.size() * sizeof(double)), "hipMalloc") ||
        check_hip(hipMemcpy(p->d_ci, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") ||
        check_hip(hipMemcpy(p->d_first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") ||
        check_hip(hipMemcpy(p->d_slot, slot_map_h, 2L * nm * nl * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") ||
        check_hip(hipMemcpy(p->d_q, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy")) {
        delete p;
        return -2;
    }
    *h = register_handle(p);
    return 0;
}

int ddh_ell_mix_apply(ddh_handle h, const double *x, double *y, void *stream) {
    EllMix *p = (EllMix *)lookup_handle(h, H_ELLMIX);
    if (!p) return -1;
    if (x == y) return fail("ell_mix_apply: in-place unsupported");
    const bool vec = p->nr % 2 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const int nu = vec ? p->nr / 2 : p->nr;
    const int tx = nu <= 8 ? 8 : (nu <= 16 ? 16 : ELLM_TX);
    const int ntp = (p->nterms + 2) & ~1;
    const dim3 grid((unsigned)((2 * p->nm + ELLM_S - 1) / ELLM_S), (unsigned)p->nl), block(tx, ELLM_S);
    const size_t lds = ell_mix_lds(ntp, p->ncomp_in, p->ncomp_out, tx * ELLM_S, vec ? sizeof(double2) : sizeof(double));
    if (vec) {                                                // (more than 64 KiB of LDS: opted in at creation)
        hipLaunchKernelGGL(ell_mix_kernel<double2>, grid, block, lds, as_stream(stream), (const double2 *)x, (double2 *)y,
                           p->d_ci, p->d_first, p->d_slot, p->d_q, p->nm, p->nl, nu, ntp, p->ncomp_in, p->ncomp_out);
    } else {
        hipLaunchKernelGGL(ell_mix_kernel<double>, grid, block, lds, as_stream(stream), x, y, p->d_ci, p->d_first, p->d_slot,
                           p->d_q, p->nm, p->nl, nu, ntp, p->ncomp_in, p->ncomp_out);
    }
    DDH_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
