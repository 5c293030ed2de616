// Matrix-free modal solve of triply periodic boxes, gfx950.
//
// With three real-Fourier axes the implicit systems are not pencils: every Fourier mode (mx, my, mz) is on its own.  A
// cell holds 2 x 2 x 2 real parts per tensor component (cos / msin along x, y, z); with the combinations P, Q of
// ddh_pencil.hip taken of the cos_z and of the msin_z rows they form four complex vectors
//     W(+kx, +kz) = P_c + i P_s      W(+kx, -kz) = P_c - i P_s      W(-kx, +kz) = Q_c + i Q_s      W(-kx, -kz) = Q_c - i Q_s
// and each solves an independent Rc x Rc complex system (a M + b L)(sx kx, ky, sz kz) X = W, Rc = the number of tensor
// components of the variables (4 .. 8).  Nothing is stored: one lane assembles its system from the symbol term list
//     A[i, j] += (a or b) * coef * kx^ex ky^ey kz^ez [mx == 0]^dx [my == 0]^dy [mz == 0]^dz
// (uniform, read through scalar loads), eliminates it with partial pivoting in registers and writes two reals per
// component.  The four systems of a cell sit in four adjacent lanes: lane (sx, sz) loads the two reals (x part sx, z part
// sz; y cos and msin: one 16-byte load) and the combinations are formed with two lane exchanges each way, so every real of
// the vectors is read once and written once and a wave touches runs of 32 consecutive doubles of a storage row.
// Replaces the reference's per-subproblem sparse LU (libraries/matsolvers.py:126-149) for these problems.
#include "ddh_common.h"

#include <atomic>

namespace ddh {

constexpr int MODAL_RC_MAX = 8;
constexpr int MODAL_RHS_MAX = 8;
constexpr int MODAL_EXP_MAX = 4;

static std::atomic<long> g_modal_launches{0};

struct ModalDev {
    int rc;
    long nx, ny, nz;             // real storage extents of a row (nx, ny) and z modes per component with a z basis
    long ncx, ncy, ncz, ncells;
    long mx_offset;
    const double *kx, *ky, *kz;
    int rrow[MODAL_RC_MAX];      // first row of component k in the right-hand-side vectors
    int xrow[MODAL_RC_MAX];      // ... in the solution vector
    int axes[MODAL_RC_MAX];      // bit 0 / 1 / 2: the component has an x / y / z basis
    const int *start;            // [rc * rc + 1] terms of entry (i, j): start[i * rc + j] .. start[i * rc + j + 1]
    const double2 *coef;
    const unsigned *expo;        // ex | ey << 4 | ez << 8 | dx << 12 | dy << 13 | dz << 14 | (1: term of L, 0: of M) << 15
};

struct ModalRhs {
    int n;
    const double *v[MODAL_RHS_MAX];
    double alpha[MODAL_RHS_MAX];
};

struct Modal : HandleBase {
    ModalDev dev;
    int nrows_rhs = 0, nrows_x = 0;
    void *d_k = nullptr, *d_start = nullptr, *d_coef = nullptr, *d_expo = nullptr;
    ~Modal() override {
        (void)hipFree(d_k);
        (void)hipFree(d_start);
        (void)hipFree(d_coef);
        (void)hipFree(d_expo);
    }
};

// offset of (ix, iy) within a storage row: natural [kx][ky] or tile-major [kx / 8][ky / 8][kx % 8][ky % 8]
__device__ __forceinline__ long modal_inrow(long ix, long iy, long ny, int tiled) {
    return tiled ? (((ix >> 3) * (ny >> 3) + (iy >> 3)) << 6) + ((ix & 7) << 3) + (iy & 7) : ix * ny + iy;
}

// k^e, e = 0 .. 4 uniform: selects, no table (a table indexed by e would live in scratch)
__device__ __forceinline__ double modal_pow(double k, unsigned e) {
    const double k2 = k * k;
    return e == 0 ? 1.0 : e == 1 ? k : e == 2 ? k2 : e == 3 ? k2 * k : k2 * k2;
}

template <int RC>
__global__ __launch_bounds__(256) void modal_solve_kernel(const ModalDev d, const double a, const double b, const ModalRhs rl,
                                                          double *__restrict__ x, const int rtiled, const int xtiled) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    long cell = t >> 2;
    const bool live = cell < d.ncells;
    if (!live) cell = d.ncells - 1;             // (the lane keeps its place in the exchanges; it stores nothing)
    const int sx = (int)(t & 1), sz = (int)((t >> 1) & 1);
    const long my = cell % d.ncy;
    const long mx = (cell / d.ncy) % d.ncx;
    const long mz = cell / (d.ncy * d.ncx);
    const long gmx = mx + d.mx_offset;
    const double kxs = sx ? -d.kx[mx] : d.kx[mx];
    const double kys = d.ky[my];
    const double kzs = sz ? -d.kz[mz] : d.kz[mz];
    const long plane = d.nx * d.ny;
    const long ix = 2 * mx + sx, iy = 2 * my;
    const long r_in = modal_inrow(ix, iy, d.ny, rtiled);
    const long x_in = modal_inrow(ix, iy, d.ny, xtiled);
    const bool slot_x = !(sx && gmx == 0);      // the msin_x slot of kx = 0, the msin_z slot of kz = 0 hold no mode
    const bool slot_z = !(sz && mz == 0);
    const bool slot_y = my != 0;                // (of the msin_y real of the pair)

    bool valid[RC];
    double wr[RC], wi[RC];
#pragma unroll
    for (int k = 0; k < RC; ++k) {
        const int ax = d.axes[k];
        const bool hasz = (ax & 4) != 0;
        valid[k] = (gmx == 0 || (ax & 1)) && (my == 0 || (ax & 2)) && (mz == 0 || hasz);
        const bool mine = valid[k] && slot_x && slot_z && (hasz || !sz);
        double va = 0.0, vb = 0.0;
        if (mine) {
            const long off = (long)(d.rrow[k] + (hasz ? 2 * mz + sz : 0)) * plane + r_in;
            for (int q = 0; q < rl.n; ++q) {
                const double2 v = *reinterpret_cast<const double2 *>(rl.v[q] + off);
                va += rl.alpha[q] * v.x;
                vb += rl.alpha[q] * v.y;
            }
            if (!slot_y) vb = 0.0;
        }
        // P / Q of this z part (lanes sx = 0 / 1), then W of this sign of kz
        const double a2 = __shfl_xor(va, 1), b2 = __shfl_xor(vb, 1);
        const double tr = sx ? a2 + vb : va - b2;
        const double ti = sx ? b2 - va : vb + a2;
        const double tr2 = __shfl_xor(tr, 2), ti2 = __shfl_xor(ti, 2);
        wr[k] = sz ? tr2 + ti : tr - ti2;
        wi[k] = sz ? ti2 - tr : ti + tr2;
    }

    // ---- the system of this lane
    double Ar[RC][RC], Ai[RC][RC];
#pragma unroll
    for (int i = 0; i < RC; ++i) {
#pragma unroll
        for (int j = 0; j < RC; ++j) {
            double sr = 0.0, si = 0.0;
            const int t0 = d.start[i * RC + j], t1 = d.start[i * RC + j + 1];
            for (int q = t0; q < t1; ++q) {
                const unsigned e = d.expo[q];
                const double2 c = d.coef[q];
                bool on = true;
                if ((e & (1u << 12)) && gmx != 0) on = false;
                if ((e & (1u << 13)) && my != 0) on = false;
                if ((e & (1u << 14)) && mz != 0) on = false;
                const double w = ((e & (1u << 15)) ? b : a) * modal_pow(kxs, e & 15u) * modal_pow(kys, (e >> 4) & 15u) *
                                 modal_pow(kzs, (e >> 8) & 15u);
                sr += on ? w * c.x : 0.0;
                si += on ? w * c.y : 0.0;
            }
            const bool keep = valid[i] && valid[j];
            Ar[i][j] = keep ? sr : (i == j ? 1.0 : 0.0);
            Ai[i][j] = keep ? si : 0.0;
        }
        if (!valid[i]) { wr[i] = 0.0; wi[i] = 0.0; }
    }

    // ---- elimination with partial pivoting; every index is a compile-time constant (compare and select)
    double pr[RC], pi[RC];                      // reciprocals of the pivots
#pragma unroll
    for (int k = 0; k < RC; ++k) {
#pragma unroll
        for (int i = k + 1; i < RC; ++i) {
            const bool sw = Ar[i][k] * Ar[i][k] + Ai[i][k] * Ai[i][k] > Ar[k][k] * Ar[k][k] + Ai[k][k] * Ai[k][k];
#pragma unroll
            for (int j = k; j < RC; ++j) {
                const double ur = Ar[k][j], ui = Ai[k][j];
                Ar[k][j] = sw ? Ar[i][j] : ur;
                Ai[k][j] = sw ? Ai[i][j] : ui;
                Ar[i][j] = sw ? ur : Ar[i][j];
                Ai[i][j] = sw ? ui : Ai[i][j];
            }
            const double ur = wr[k], ui = wi[k];
            wr[k] = sw ? wr[i] : ur;
            wi[k] = sw ? wi[i] : ui;
            wr[i] = sw ? ur : wr[i];
            wi[i] = sw ? ui : wi[i];
        }
        const double den = 1.0 / (Ar[k][k] * Ar[k][k] + Ai[k][k] * Ai[k][k]);
        pr[k] = Ar[k][k] * den;
        pi[k] = -Ai[k][k] * den;
#pragma unroll
        for (int i = k + 1; i < RC; ++i) {
            const double mr = Ar[i][k] * pr[k] - Ai[i][k] * pi[k];
            const double mi = Ar[i][k] * pi[k] + Ai[i][k] * pr[k];
#pragma unroll
            for (int j = k + 1; j < RC; ++j) {
                Ar[i][j] -= mr * Ar[k][j] - mi * Ai[k][j];
                Ai[i][j] -= mr * Ai[k][j] + mi * Ar[k][j];
            }
            wr[i] -= mr * wr[k] - mi * wi[k];
            wi[i] -= mr * wi[k] + mi * wr[k];
        }
    }
#pragma unroll
    for (int k = RC - 1; k >= 0; --k) {
        double sr = wr[k], si = wi[k];
#pragma unroll
        for (int j = k + 1; j < RC; ++j) {
            sr -= Ar[k][j] * wr[j] - Ai[k][j] * wi[j];
            si -= Ar[k][j] * wi[j] + Ai[k][j] * wr[j];
        }
        wr[k] = sr * pr[k] - si * pi[k];
        wi[k] = sr * pi[k] + si * pr[k];
    }

    // ---- back to the real parts: cos_z / msin_z parts of P (Q), then the x parts; two reals per lane and component
#pragma unroll
    for (int k = 0; k < RC; ++k) {
        const double yr = __shfl_xor(wr[k], 2), yi = __shfl_xor(wi[k], 2);
        const double tr = sz ? 0.5 * (yi - wi[k]) : 0.5 * (wr[k] + yr);
        const double ti = sz ? 0.5 * (wr[k] - yr) : 0.5 * (wi[k] + yi);
        const double ur = __shfl_xor(tr, 1), ui = __shfl_xor(ti, 1);
        const bool hasz = (d.axes[k] & 4) != 0;
        const bool mine = valid[k] && slot_x && slot_z;
        double2 o;
        o.x = mine ? (sx ? 0.5 * (ui - ti) : 0.5 * (tr + ur)) : 0.0;
        o.y = (mine && slot_y) ? (sx ? 0.5 * (tr - ur) : 0.5 * (ti + ui)) : 0.0;
        if (live && (hasz || (!sz && mz == 0))) {     // (a component without a z basis has one row: the cells of mz = 0 own it)
            const long off = (long)(d.xrow[k] + (hasz ? 2 * mz + sz : 0)) * plane + x_in;
            *reinterpret_cast<double2 *>(x + off) = o;
        }
    }
}

template <int RC>
static void modal_launch(const Modal *p, double a, double b, const ModalRhs &rl, double *x, int rtiled, int xtiled,
                         hipStream_t st) {
    const long threads = 4 * p->dev.ncells;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    hipLaunchKernelGGL(modal_solve_kernel<RC>, grid, block, 0, st, p->dev, a, b, rl, x, rtiled, xtiled);
}

}  // namespace ddh

using namespace ddh;

extern "C" {

int ddh_modal_create(ddh_handle *h, int rc, long nx, long ny, long nz, const double *kx_h, const double *ky_h,
                     const double *kz_h, long mx_offset, int nrows_rhs, int nrows_x, const int *rhs_row_h,
                     const int *x_row_h, const unsigned char *axes_h, int nterms, const int *ti_h, const int *tj_h,
                     const double *coef_re_h, const double *coef_im_h, const unsigned char *ex_h,
                     const unsigned char *ey_h, const unsigned char *ez_h, const unsigned char *flags_h) {
    if (!h || !kx_h || !ky_h || !kz_h || !rhs_row_h || !x_row_h || !axes_h) return fail("ddh_modal_create: null pointer");
    if (rc < 1 || rc > MODAL_RC_MAX) return fail("ddh_modal_create: 1 <= rc <= 8 component rows");
    if (nx < 2 || ny < 2 || nz < 2 || (nx & 1) || (ny & 1) || (nz & 1))
        return fail("ddh_modal_create: nx, ny, nz must be even and >= 2");
    if (nx * ny * (nz / 2) / 4 > (long)INT_MAX / 2) return fail("ddh_modal_create: too many cells for one launch");
    if (nterms < 0 || (nterms > 0 && (!ti_h || !tj_h || !coef_re_h || !coef_im_h || !ex_h || !ey_h || !ez_h || !flags_h)))
        return fail("ddh_modal_create: null term arrays");
    if (mx_offset < 0) return fail("ddh_modal_create: negative mx_offset");
    for (int k = 0; k < rc; ++k) {
        const int len = (axes_h[k] & 4) ? (int)nz : 1;
        if (axes_h[k] > 7) return fail("ddh_modal_create: axes bits out of range");
        if (rhs_row_h[k] < 0 || rhs_row_h[k] + len > nrows_rhs || x_row_h[k] < 0 || x_row_h[k] + len > nrows_x)
            return fail("ddh_modal_create: component rows outside the vectors");
    }
    std::vector<int> start(rc * rc + 1, 0);
    for (int t = 0; t < nterms; ++t) {
        if (ti_h[t] < 0 || ti_h[t] >= rc || tj_h[t] < 0 || tj_h[t] >= rc) return fail("ddh_modal_create: term entry out of range");
        if (ex_h[t] > MODAL_EXP_MAX || ey_h[t] > MODAL_EXP_MAX || ez_h[t] > MODAL_EXP_MAX)
            return fail("ddh_modal_create: wavenumber exponents up to 4");
        if (flags_h[t] > 15) return fail("ddh_modal_create: flags out of range");
        ++start[ti_h[t] * rc + tj_h[t] + 1];
    }
    for (int e = 0; e < rc * rc; ++e) start[e + 1] += start[e];
    std::vector<double2> coef(nterms > 0 ? nterms : 1);
    std::vector<unsigned> expo(nterms > 0 ? nterms : 1);
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int t = 0; t < nterms; ++t) {          // (stable: the terms of an entry keep their order)
        const int q = fill[ti_h[t] * rc + tj_h[t]]++;
        coef[q] = make_double2(coef_re_h[t], coef_im_h[t]);
        expo[q] = (unsigned)ex_h[t] | ((unsigned)ey_h[t] << 4) | ((unsigned)ez_h[t] << 8) | ((unsigned)flags_h[t] << 12);
    }
    Modal *p = new Modal();
    p->kind = H_MODAL;
    p->nrows_rhs = nrows_rhs;
    p->nrows_x = nrows_x;
    ModalDev &d = p->dev;
    std::memset(&d, 0, sizeof(d));
    d.rc = rc;
    d.nx = nx; d.ny = ny; d.nz = nz;
    d.ncx = nx / 2; d.ncy = ny / 2; d.ncz = nz / 2;
    d.ncells = d.ncx * d.ncy * d.ncz;
    d.mx_offset = mx_offset;
    for (int k = 0; k < rc; ++k) { d.rrow[k] = rhs_row_h[k]; d.xrow[k] = x_row_h[k]; d.axes[k] = axes_h[k]; }
    std::vector<double> kall(d.ncx + d.ncy + d.ncz);
    std::copy(kx_h, kx_h + d.ncx, kall.begin());
    std::copy(ky_h, ky_h + d.ncy, kall.begin() + d.ncx);
    std::copy(kz_h, kz_h + d.ncz, kall.begin() + d.ncx + d.ncy);
    int st = 0;
    auto up = [&](void **dst, const void *src, size_t n) {
        if (st) return;
        st = check_hip(hipMalloc(dst, n), "hipMalloc");
        if (!st) st = check_hip(hipMemcpy(*dst, src, n, hipMemcpyHostToDevice), "hipMemcpy");
    };
    up(&p->d_k, kall.data(), kall.size() * sizeof(double));
    up(&p->d_start, start.data(), start.size() * sizeof(int));
    up(&p->d_coef, coef.data(), coef.size() * sizeof(double2));
    up(&p->d_expo, expo.data(), expo.size() * sizeof(unsigned));
    if (st) { delete p; return st; }
    d.kx = (const double *)p->d_k;
    d.ky = d.kx + d.ncx;
    d.kz = d.ky + d.ncy;
    d.start = (const int *)p->d_start;
    d.coef = (const double2 *)p->d_coef;
    d.expo = (const unsigned *)p->d_expo;
    *h = register_handle(p);
    return 0;
}

int ddh_pencil_solve_modal(ddh_handle h, double a, double b, int nrhs, const double *const *rhs, const double *alphas_h,
                           int rhs_tiled, double *x, int x_tiled, void *stream) {
    Modal *p = (Modal *)lookup_handle(h, H_MODAL);
    if (!p) return -1;
    if (nrhs < 1 || nrhs > MODAL_RHS_MAX) return fail("ddh_pencil_solve_modal: 1 <= nrhs <= 8 right-hand-side terms");
    if (!rhs || !alphas_h || !x) return fail("ddh_pencil_solve_modal: null pointer");
    if ((rhs_tiled || x_tiled) && ((p->dev.nx & 7) || (p->dev.ny & 7)))
        return fail("ddh_pencil_solve_modal: tile-major vectors need nx and ny to be multiples of 8");
    ModalRhs rl;
    std::memset(&rl, 0, sizeof(rl));
    rl.n = nrhs;
    for (int q = 0; q < nrhs; ++q) {
        if (!rhs[q]) return fail("ddh_pencil_solve_modal: null right-hand side");
        if (((uintptr_t)rhs[q]) & 15) return fail("ddh_pencil_solve_modal: vectors must be 16-byte aligned");
        rl.v[q] = rhs[q];
        rl.alpha[q] = alphas_h[q];
    }
    if (((uintptr_t)x) & 15) return fail("ddh_pencil_solve_modal: vectors must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const int rt = rhs_tiled ? 1 : 0, xt = x_tiled ? 1 : 0;
    switch (p->dev.rc) {
        case 1: modal_launch<1>(p, a, b, rl, x, rt, xt, st); break;
        case 2: modal_launch<2>(p, a, b, rl, x, rt, xt, st); break;
        case 3: modal_launch<3>(p, a, b, rl, x, rt, xt, st); break;
        case 4: modal_launch<4>(p, a, b, rl, x, rt, xt, st); break;
        case 5: modal_launch<5>(p, a, b, rl, x, rt, xt, st); break;
        case 6: modal_launch<6>(p, a, b, rl, x, rt, xt, st); break;
        case 7: modal_launch<7>(p, a, b, rl, x, rt, xt, st); break;
        case 8: modal_launch<8>(p, a, b, rl, x, rt, xt, st); break;
    }
    DDH_HIP(hipGetLastError());
    g_modal_launches.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

int ddh_modal_launches(long *count) {
    if (!count) return fail("ddh_modal_launches: null pointer");
    *count = g_modal_launches.load(std::memory_order_relaxed);
    return 0;
}

}  // extern "C"
