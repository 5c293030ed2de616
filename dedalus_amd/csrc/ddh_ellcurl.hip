// Per-ell radial term lists with imaginary terms (the curl of shell vector fields), gfx950.
//
// Fields are [component][2 m + part][ell][n], part 0 / 1 = cos / msin of the azimuthal mode m: one complex number
// z = cos + i msin per (component, m, ell, n).  A term t maps component ci to co through a REAL radial matrix A_t[id]
// (id chosen per slot as in ddh_ell_terms_create) and carries a flag rot_t:
//     rot_t = 0:  y[co][2m + p] += A x[ci][2m + p]                                           (as ddh_ell_terms_apply)
//     rot_t = 1:  the term is i A:  y[co][2m + 0] += -A x[ci][2m + 1],  y[co][2m + 1] += +A x[ci][2m + 0]
// which is (i A)(c + i s) = -A s + i A c, the real-dtype branch of SphericalCurl.operate (core/operators.py:3944-3978:
// vec_in_cos + 1j * vec_in_msin through the purely imaginary radial matrices of :3889-3901, real part to the cos rows,
// imaginary part to the msin rows).
//
// Launch shape (the edges tests/shell_vector_cases.py lists): one workgroup = ELLC_S = 8 consecutive slots (4 azimuthal
// pairs, so both parts of a pair always sit in one workgroup) of one ell; threadIdx.x runs along the output radial
// index (64, 128 or 256 threads: nr <= 64, <= 255, >= 256), threadIdx.y over ELLC_CO = 4 output components at a time.
// The input lines of all components are staged once in LDS as [component][n][slot]: a thread then reads the 8 right-hand
// sides of one n with two 32-byte LDS loads, and every matrix element fetched from L2 / HBM is used 8 times.  The
// matrices are stored transposed ([n_in][n_out]).  Differential operators are banded in n: per term, matrix and output
// row the first / one-past-last non-zero column bounds the inner loop, so the kernel streams the lines once -- the
// regime is that of ddh_ell_terms_apply's banded path, not its GEMM path.  In that regime every lane starts its loop at
// its own row's first column: at one iteration neighbouring lanes read neighbouring LDS lines (64 bytes apart: two
// lanes per bank group, not a broadcast) and matrix elements nr + 1 doubles apart (the diagonals of the transposed
// matrix); only rows that are full (dense blocks) give the broadcast / consecutive pattern.  The access pattern is the
// one ell_terms_kernel (ddh_sphere.hip) has for grad and div; profiles/shell_vector_ops.txt holds both rates.
//
// A slot with slot_map < 0 carries no mode: it is never read -- not as the rotation partner of its pair either, where it
// contributes nothing -- and exact +0 is written to it.  No atomics: every output element is summed by one thread in
// the order (term, n_in ascending), a function of the term list alone.
#include "ddh_common.h"

namespace ddh {

constexpr int ELLC_S = 8;     // slots per workgroup (even: a (cos, msin) pair never straddles two workgroups)
constexpr int ELLC_CO = 4;    // output components processed concurrently (threadIdx.y)

struct EllTermsCx : HandleBase {
    int nm = 0, nl = 0, nr = 0, ncomp_out = 0, ncomp_in = 0, nterms = 0, nmat = 0;
    int *d_meta = nullptr;       // [nterms][3]: co, ci, rot (sorted by co)
    int *d_first = nullptr;      // [ncomp_out + 1]
    int *d_slot = nullptr;       // [2 nm][nl]: matrix index of the slot, -1: no mode
    short *d_band = nullptr;     // [nterms][nmat][nr][2]: first / one-past-last non-zero column of every row
    double *d_mats = nullptr;    // [nterms][nmat][n_in][n_out]
    ~EllTermsCx() override {
        (void)hipFree(d_meta);
        (void)hipFree(d_first);
        (void)hipFree(d_slot);
        (void)hipFree(d_band);
        (void)hipFree(d_mats);
    }
};

__global__ void __launch_bounds__(1024)
ell_terms_cx_kernel(const double *__restrict__ x, double *__restrict__ y, const int *__restrict__ meta,
                    const int *__restrict__ first, const int *__restrict__ slot_map, const short *__restrict__ band,
                    const double *__restrict__ mats, int nm, int nl, int nr, int nmat, int ncomp_in, int ncomp_out) {
    extern __shared__ double sx[];                   // [ncomp_in][nr][ELLC_S]
    const int l = blockIdx.y, i0 = blockIdx.x * ELLC_S;
    const int tlin = threadIdx.y * blockDim.x + threadIdx.x, tall = blockDim.x * blockDim.y;
    const long cstride = 2L * nm * nl * nr;
    int mid[ELLC_S];
    bool same = true;
    int mid0 = -1;
#pragma unroll
    for (int s = 0; s < ELLC_S; ++s) {
        const int i1 = i0 + s;
        mid[s] = (i1 < 2 * nm) ? slot_map[i1 * nl + l] : -1;
        if (mid[s] >= 0) {
            if (mid0 < 0) mid0 = mid[s];
            else if (mid[s] != mid0) same = false;
        }
    }
    if (mid0 >= 0) {                                  // (block-uniform) stage the live input lines, +0 for the others
        for (int w = tlin; w < ncomp_in * nr; w += tall) {
            const int ci = w / nr, ni = w - ci * nr;
#pragma unroll
            for (int s = 0; s < ELLC_S; ++s)
                sx[(long)w * ELLC_S + s] = (mid[s] >= 0) ? x[ci * cstride + ((long)(i0 + s) * nl + l) * nr + ni] : 0.0;
        }
    }
    __syncthreads();
    for (int co = threadIdx.y; co < ncomp_out; co += ELLC_CO) {
        for (int no = threadIdx.x; no < nr; no += blockDim.x) {
            double acc[ELLC_S];
#pragma unroll
            for (int s = 0; s < ELLC_S; ++s) acc[s] = 0.0;
            for (int t = (mid0 >= 0 ? first[co] : first[co + 1]); t < first[co + 1]; ++t) {
                const int ci = meta[3 * t + 1], rot = meta[3 * t + 2];
                const double *xs = sx + (long)ci * nr * ELLC_S;
                if (same) {
                    const long bi = 2 * (((long)t * nmat + mid0) * nr + no);
                    const int n0 = band[bi], n1 = band[bi + 1];          // non-zero columns of this row
                    const double *A = mats + (((long)t * nmat + mid0) * nr) * nr + no;
                    if (rot) {
                        for (int ni = n0; ni < n1; ++ni) {
                            const double a = A[(long)ni * nr];
                            const double4 xv = *reinterpret_cast<const double4 *>(xs + (long)ni * ELLC_S);
                            const double4 xw = *reinterpret_cast<const double4 *>(xs + (long)ni * ELLC_S + 4);
                            acc[0] -= a * xv.y;
                            acc[1] += a * xv.x;
                            acc[2] -= a * xv.w;
                            acc[3] += a * xv.z;
                            acc[4] -= a * xw.y;
                            acc[5] += a * xw.x;
                            acc[6] -= a * xw.w;
                            acc[7] += a * xw.z;
                        }
                    } else {
                        for (int ni = n0; ni < n1; ++ni) {
                            const double a = A[(long)ni * nr];
                            const double4 xv = *reinterpret_cast<const double4 *>(xs + (long)ni * ELLC_S);
                            const double4 xw = *reinterpret_cast<const double4 *>(xs + (long)ni * ELLC_S + 4);
                            acc[0] += a * xv.x;
                            acc[1] += a * xv.y;
                            acc[2] += a * xv.z;
                            acc[3] += a * xv.w;
                            acc[4] += a * xw.x;
                            acc[5] += a * xw.y;
                            acc[6] += a * xw.z;
                            acc[7] += a * xw.w;
                        }
                    }
                } else {                              // slots of the group use different matrices (rare)
#pragma unroll
                    for (int s = 0; s < ELLC_S; ++s) {
                        if (mid[s] < 0) continue;
                        const long bi = 2 * (((long)t * nmat + mid[s]) * nr + no);
                        const int n0 = band[bi], n1 = band[bi + 1];
                        const double *A = mats + (((long)t * nmat + mid[s]) * nr) * nr + no;
                        const int sp = rot ? (s ^ 1) : s;          // the slot read: the other part of the pair for i A
                        const double sg = (rot && !(s & 1)) ? -1.0 : 1.0;
                        for (int ni = n0; ni < n1; ++ni) acc[s] += sg * (A[(long)ni * nr] * xs[(long)ni * ELLC_S + sp]);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < ELLC_S; ++s)
                if (i0 + s < 2 * nm) y[co * cstride + ((long)(i0 + s) * nl + l) * nr + no] = (mid[s] >= 0) ? acc[s] : 0.0;
        }
    }
}

}  // namespace ddh

using namespace ddh;

extern "C" {

int ddh_ell_terms_create_cx(ddh_handle *h, int nm, int nl, int nr, int ncomp_out, int ncomp_in, int nterms,
                            const int *co_h, const int *ci_h, const int *rot_h, int nmat, const double *mats_h,
                            const int *slot_map_h) {
    if (nm < 1 || nl < 1 || nr < 1 || nr > 32767 || ncomp_out < 1 || ncomp_in < 1 || nterms < 0 || nmat < 1)
        return fail("ell_terms_create_cx: bad sizes");
    if ((size_t)ncomp_in * nr * ELLC_S * sizeof(double) > 160 * 1024)         // the limit of ddh_ell_terms_apply
        return fail("ell_terms_create_cx: too many components x radial modes for the LDS staging");
    for (long i = 0; i < 2L * nm * nl; ++i)
        if (slot_map_h[i] >= nmat) return fail("ell_terms_create_cx: slot map points past the matrices");
    const size_t nt = (size_t)(nterms > 0 ? nterms : 1);
    std::vector<int> meta(3 * nt, 0), first(ncomp_out + 1, 0);
    for (int t = 0; t < nterms; ++t) {
        if (co_h[t] < 0 || co_h[t] >= ncomp_out || (t > 0 && co_h[t] < co_h[t - 1]))
            return fail("ell_terms_create_cx: terms must be sorted by output component");
        if (ci_h[t] < 0 || ci_h[t] >= ncomp_in) return fail("ell_terms_create_cx: input component out of range");
        if (rot_h[t] != 0 && rot_h[t] != 1) return fail("ell_terms_create_cx: rot must be 0 or 1");
        meta[3 * t] = co_h[t]; meta[3 * t + 1] = ci_h[t]; meta[3 * t + 2] = rot_h[t];
        first[co_h[t] + 1] = t + 1;
    }
    for (int c = 0; c < ncomp_out; ++c)
        if (first[c + 1] < first[c]) first[c + 1] = first[c];
    const size_t per = (size_t)nmat * nr * nr;
    std::vector<double> tr(nt * per, 0.0);            // every matrix transposed to [n_in][n_out]
    std::vector<short> band(2 * nt * nmat * nr, 0);
    for (size_t t = 0; t < (size_t)nterms; ++t)
        for (size_t l = 0; l < (size_t)nmat; ++l)
            for (int i = 0; i < nr; ++i) {
                int lo = 0, hi = 0;
                for (int j = 0; j < nr; ++j) {
                    const double v = mats_h[(t * nmat + l) * nr * nr + (size_t)i * nr + j];
                    tr[(t * nmat + l) * nr * nr + (size_t)j * nr + i] = v;
                    if (v != 0.0) {
                        if (hi == 0) lo = j;
                        hi = j + 1;
                    }
                }
                band[2 * ((t * nmat + l) * nr + i)] = (short)lo;
                band[2 * ((t * nmat + l) * nr + i) + 1] = (short)hi;
            }
    EllTermsCx *p = new EllTermsCx();
    p->kind = H_ELLTCX;
    p->nm = nm; p->nl = nl; p->nr = nr; p->ncomp_out = ncomp_out; p->ncomp_in = ncomp_in; p->nterms = nterms; p->nmat = nmat;
    const size_t mb = tr.size() * sizeof(double);
    if (check_hip(hipMalloc((void **)&p->d_meta, meta.size() * sizeof(int)), "hipMalloc") ||
        check_hip(hipMalloc((void **)&p->d_first, first.size() * sizeof(int)), "hipMalloc") ||
        check_hip(hipMalloc((void **)&p->d_mats, mb), "hipMalloc") ||
        check_hip(hipMalloc((void **)&p->d_slot, 2L * nm * nl * sizeof(int)), "hipMalloc") ||
        check_hip(hipMalloc((void **)&p->d_band, band.size() * sizeof(short)), "hipMalloc") ||
        check_hip(hipMemcpy(p->d_band, band.data(), band.size() * sizeof(short), hipMemcpyHostToDevice), "hipMemcpy") ||
        check_hip(hipMemcpy(p->d_slot, slot_map_h, 2L * nm * nl * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") ||
        check_hip(hipMemcpy(p->d_meta, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") ||
        check_hip(hipMemcpy(p->d_first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") ||
        check_hip(hipMemcpy(p->d_mats, tr.data(), mb, hipMemcpyHostToDevice), "hipMemcpy")) {
        delete p;
        return -2;
    }
    *h = register_handle(p);
    return 0;
}

int ddh_ell_terms_apply_cx(ddh_handle h, const double *x, double *y, void *stream) {
    EllTermsCx *p = (EllTermsCx *)lookup_handle(h, H_ELLTCX);
    if (!p) return -1;
    if (x == y) return fail("ell_terms_apply_cx: in-place unsupported");
    const int T = p->nr >= 256 ? 256 : (p->nr > 64 ? 128 : 64);
    const dim3 grid((unsigned)((2 * p->nm + ELLC_S - 1) / ELLC_S), (unsigned)p->nl), block(T, ELLC_CO);
    const size_t lds = (size_t)p->ncomp_in * p->nr * ELLC_S * sizeof(double);       // <= 160 KiB, checked at creation
    if (lds > 64 * 1024)
        DDH_HIP(hipFuncSetAttribute((const void *)ell_terms_cx_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ell_terms_cx_kernel, grid, block, lds, as_stream(stream), x, y, p->d_meta, p->d_first, p->d_slot,
                       p->d_band, p->d_mats, p->nm, p->nl, p->nr, p->nmat, p->ncomp_in, p->ncomp_out);
    DDH_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
