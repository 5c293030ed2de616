// Device-side building blocks shared by the transform kernels (ddh_fft.hip) and the wave-per-line
// grid stage (ddh_gridwave.hip): plan descriptor, complex helpers, in-register DFT butterflies.
#pragma once
#include "ddh_common.h"
#include "ddh_butterfly.h"

namespace ddh {


enum FftKind { K_RFFT = 0, K_CHEB = 1, K_CFFT = 2 };
enum FftMode { RFFT_FWD = 0, RFFT_BWD, CHEB_FWD, CHEB_BWD, CFFT_FWD, CFFT_BWD };

constexpr int MAX_RADIX_PASSES = 16;
constexpr int MAX_BANDS = 4;

// division by a runtime constant without the ~40-instruction software divide
struct FastDiv {
    unsigned d, m, s;
    __host__ void set(unsigned dd) {
        d = dd ? dd : 1;
        if (d == 1) { m = 0; s = 0; return; }
        s = 0;
        while ((1ull << s) < d) ++s;
        m = (unsigned)((((1ull << 32) * ((1ull << s) - d)) / d) + 1);
    }
    __device__ __forceinline__ unsigned div(unsigned n) const {
        return d == 1 ? n : (unsigned)(((unsigned long long)__umulhi(n, m) + n) >> s);
    }
    __device__ __forceinline__ void divmod(unsigned n, unsigned &q, unsigned &r) const {
        q = div(n);
        r = n - q * d;
    }
};

struct FftDev {
    FastDiv fdN, fdM, fdMh, fdK1, fdB, fd_nb[MAX_RADIX_PASSES], fd_ns[MAX_RADIX_PASSES];
    int N;       // grid size = FFT length
    int M;       // coefficient size
    int K;       // Fourier: largest retained wavenumber
    int nradix;
    int radix[MAX_RADIX_PASSES];
    const double2 *tw;     // exp(-2 pi i q / N)
    const double2 *half;   // exp(-i pi k / (2N))
    const double *fscale;  // Chebyshev forward scale per k (includes (-1)^k)
    const double *bscale;  // Chebyshev backward scale per k
    int nbands;
    int gcd_off;           // gcd of the non-zero band offsets (independent back-substitution chains)
    int boff[MAX_BANDS];
    const double *bands;   // [nbands][M]
    const double *bsub;    // [3][M] back-substitution table (1/diag, bands over diag by chain distance) or null
    int bsub_order;        // 1: only the nearest chain neighbour enters (first-order recurrence: wavefront scan), 2: two
    int B;                 // line pairs per workgroup
    double dscale;         // RFFT_BWD: != 0 differentiates along the axis while loading (2 pi / L)
    double *dst2;          // RFFT_BWD dual output: second destination (null = single output) ...
    double dscale2;        // ... transformed with this derivative scale
    const double *dvec;    // CHEB_BWD dual output: [M] superdiagonal of the derivative operator (second pass input = dvec[k] c[k+1])
    unsigned xb;                // != 0: x-blocked stage layout on the INTERMEDIATE side of a strided wave transform
    unsigned xbw0, xbwn;        // xbwn != 0: the launch covers planes xbw0 .. xbw0 + xbwn of EVERY component (a window of this
                                // rank's z planes: outer = components x xbwn), the other side holding xbwn planes per component
    unsigned xbB;               // rows per block of that layout on the coefficient side of a real-Fourier transform (0 = 64)
                                // (ddh_fft_set_stage_layout): Chebyshev plans: row length ny; real-FFT plans: z planes gz
    unsigned long cband;        // != 0 (with ctile_nseg): the tile-major coefficient rows are kx-band-major, [kx / 8][row][ky / 8][8][8]:
                                // cband = doubles between the bands of 8 storage rows (all rows of the state vector x 8 ny);
                                // the rows of a line are then 8 ny doubles apart (ddh_fft_set_coeff_tiled)
    unsigned ctile_nseg;        // != 0: the coefficient rows [nx][ny] are written tile-major, ctile_nseg = ny / 8 64-byte
                                // segments per storage row (ddh_cheb_forward_tiled; wave kernel only)
    int ld;                     // LDS leading dimension of the FFT buffer (>= N): the workgroup kernels of ddh_fft.hip only
};

struct FftPlan : HandleBase {
    FftDev dev;
    int tkind;
    void *d_tw = nullptr, *d_half = nullptr, *d_fscale = nullptr, *d_bscale = nullptr, *d_bands = nullptr;
    // ddh_rfft_bilinear_fused: the plan of the wider grid the fused stage works on when this plan's grid size has no
    // wave kernel (see there); 0 = none yet, owned by this plan
    ddh_handle fused_alt = 0;
    ~FftPlan() override {
        if (fused_alt) (void)ddh_destroy(fused_alt);
        (void)hipFree(d_tw);
        (void)hipFree(d_half);
        (void)hipFree(d_fscale);
        (void)hipFree(d_bscale);
        (void)hipFree(d_bands);
    }
};

constexpr int FUSED_NA = 3, FUSED_NC = 4, FUSED_NB = 12, FUSED_TERMS = 32;
constexpr int FUSED_LOADS = FUSED_NA + FUSED_TERMS;
constexpr int FUSED_T = 256;
constexpr int GRIDWAVE_WAVES = 4;    // lines (wavefronts) per workgroup of the wave-per-line grid stage, both generations

// largest retained wavenumber of a Fourier plan of n_grid points and n_coeff coefficients
inline int fourier_kmax(int n_grid, int n_coeff) {
    const int KN = (n_grid - 1) / 2, KM = (n_coeff - 1) / 2;
    return KN < KM ? KN : KM;
}

struct FusedArgs {
    const double *src[FUSED_LOADS];   // line arrays in load order: the `a` operands first
    double dscale[FUSED_LOADS];       // != 0: differentiate along the axis while unpacking (2 pi / L)
    double *out[FUSED_NC];
    double coef[FUSED_TERMS];
    short tbeg[FUSED_LOADS + 1];      // terms [tbeg[l], tbeg[l+1]) multiply load l
    short bbeg[FUSED_LOADS + 1];      // batch i transforms loads [bbeg[i], bbeg[i+1]) together
    signed char flush[FUSED_LOADS];   // per batch: >= 0: result `flush` is complete after it
    signed char ia[FUSED_TERMS];
    int na, nbatch;
};

// ------------------------------------------------------------------------------------------------
// Which kernel a call takes (host only).  transform_plan (ddh_fftwave.hip) and fused_plan (ddh_gridwave.hip) decide it
// once per call from the plan descriptor and the call's shape; the launchers execute the decision.  They launch nothing
// and allocate nothing.
// ------------------------------------------------------------------------------------------------

// The sizes the wave-per-four-line-pairs transforms (ddh_wavefft.h) are instantiated for; the dispatch, the plan functions
// and ddh_fft_wave_size are all generated from these two lists.
// Chebyshev X(R, NL): N = 16 R grid points, M = 16 NL modes.  3/2 dealiasing of 128 / 256 modes (the configurations' radial
// / vertical bases), no dealiasing (N = M = 64 .. 256) and factor-two padding.
#define DDH_CHEB_WAVE_SIZES(X) X(24, 16) X(12, 8) X(16, 16) X(12, 12) X(8, 8) X(4, 4) X(16, 8) X(8, 4)
// real Fourier with 3/2 dealiasing X(R): N = 48 R grid points, M = 32 R coefficients (128 .. 512 modes)
#define DDH_RFFT_WAVE_SIZES(X) X(16) X(12) X(8) X(4)

enum class TransformKernel {
    cheb_wave,          // wave_cheb_kernel<kind, R, NL>: strided axis
    rfft_wave,          // wave_rfft_kernel<kind, R>: strided axis
    cheb_contig_wave,   // wave_cheb_contig_kernel<kind, R, NL>: contiguous axis
    workgroup           // fft_axis_kernel<MODE, inner, tmax>: every size, either axis
};
struct TransformPlan {
    const char *error;            // != nullptr: the plan's layout (xb, ctile_nseg) or the shape has no kernel
    TransformKernel kernel;
    int kind;                     // wave kernels: KIND / RKIND (backward 0 plain, 1 derivative / dual, 2 conversion / dual; 3 forward)
    int R, NL;                    // wave kernels: the size's entry in the tables above (NL: Chebyshev only)
    unsigned tpw;                 // wave kernels: tiles per wave ...
    int wsync;                    // ... and one workgroup barrier per tile
    unsigned tpo, ntiles;         // wave kernels: tiles per outer index (strided) and in all
    long npairs;                  // line pairs along the paired axis
    bool inner;                   // workgroup kernel: INNER
    int B;                        // workgroup kernel: line pairs per workgroup (FftDev::B); TMAX follows block
    unsigned bpo;                 // workgroup kernel: workgroups per outer index
    unsigned grid, block;
    size_t lds;
    bool wave() const { return kernel != TransformKernel::workgroup; }
};
// second: a second output (dual entry points); deriv: derivative at load (RFFT_BWD); dvec: FftDev::dvec given;
// aliased: the source is one of the destinations
TransformPlan transform_plan(const FftDev &d, int mode, long outer, long inner, bool second, bool deriv, bool dvec,
                             bool aliased);
// the wave kernels of a plan (ddh_fftwave.hip); d carries the per-call fields (dscale, dst2, dvec)
int launch_cheb_wave(const TransformPlan &tp, const FftDev &d, const double *src, double *dst, long inner, hipStream_t st);
int launch_rfft_wave(const TransformPlan &tp, const FftDev &d, const double *src, double *dst, long inner, hipStream_t st);
int launch_cheb_contig_wave(const TransformPlan &tp, const FftDev &d, const double *src, double *dst, long outer, hipStream_t st);

enum class FusedKernel {
    gridwave2,          // gw2::gridwave2_bilinear_kernel<C, NT, 4, twreg, dma>
    gridwave,           // gw::gridwave_bilinear_kernel<C, NT, twreg>
    workgroup           // fused_rfft_bilinear_kernel<PTS, G>
};
struct FusedPlan {
    const char *error;
    int N;                        // internal grid size: the plan's own, or the wider one (ddh_rfft_bilinear_fused)
    FusedKernel kernel;
    int C, NT;                    // wave kernels: N = 128 C, 64 NT coefficient pairs loaded per line
    bool twreg, dma;              // wave kernels: twiddles in registers; second generation: operands by LDS-DMA
    int PTS, G;                   // workgroup kernel: grid points per thread; operands per FFT batch (1 for the wave kernels)
    long lpw;                     // wave kernels: lines per wave
    unsigned grid, block;
    size_t lds;
};
FusedPlan fused_plan(const FftDev &d, long nlines);
// d: the descriptor of the grid size fp.N; f built with fp.G loads per batch
int launch_gridwave(const FusedPlan &fp, const FftDev &d, const FusedArgs &f, long nlines, hipStream_t st);     // ddh_gridwave.hip
int launch_gridwave2(const FusedPlan &fp, const FftDev &d, const FusedArgs &f, long nlines, hipStream_t st);    // ddh_gridwave2.hip

// entries of the two-level twiddle table of the LDS FFT (ddh_fft.hip): W^q = hi[q >> 5] * lo[q & 31]
__host__ __device__ __forceinline__ int tw_entries(int N) { return 32 + (N >> 5) + 1; }

}  // namespace ddh
