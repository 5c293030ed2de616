// Strided-axis Chebyshev transforms, one wavefront per four line pairs (ddh_wavefft.h): kernels and launch; transform_plan,
// the one place that decides which kernel a transform call takes.
//
// A workgroup is 8 independent wavefronts that share the read-only tables in LDS (twiddles, half-angle factors,
// conversion bands / back-substitution table / derivative vector) and nothing else: no workgroup barrier after the
// table fill.  At step i the 8 waves of workgroup g work on 8 neighbouring tiles (512 contiguous bytes per row) and a
// wave requests the coefficient rows of its next tile while it transforms the current one.
// Replaces core/transforms.py:715-902 for the strided z axis (the reference: scipy DCT + scale / pad / conversion passes).
#include "ddh_fft_dev.h"
#include "ddh_wavefft.h"

#include <cstdlib>

namespace ddh {

constexpr int WV_WAVES = 8;
#ifndef DDH_WR_WAVES
#define DDH_WR_WAVES 8
#endif
constexpr int WR_WAVES = DDH_WR_WAVES;     // waves per workgroup of the real-FFT kernels

struct WaveArgs {
    const double *src;
    double *dst, *dst2;
    long inner, npairs;
    FastDiv fd_tpo;          // tiles per outer index
    unsigned ntiles, tpw;    // tiles in all, tiles per wave
    int kind;                // backward: 0 plain, 1 dual (plain + derivative pass), 2 conversion solve
    int wsync;               // 1: the waves of a workgroup start every tile together (one s_barrier per tile)
};

template <int KIND, int R, int NL, int CH>      // KIND: 0 backward plain, 1 backward dual, 2 backward conversion, 3 forward
__global__ void __launch_bounds__(64 * WV_WAVES, 2)
wave_cheb_kernel(FftDev p, WaveArgs a) {
    constexpr bool FWD = (KIND == 3);
    extern __shared__ double2 lds[];
    constexpr int N = 16 * R;
    const int M = p.M, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: tile bases live in scalar registers
    double2 *s_tw = lds, *s_half = lds + N;
    double *s_d = reinterpret_cast<double *>(lds + 2 * N);
    // doubles: forward [nbands][M] bands; backward [2][M] back-substitution table, [M] derivative vector
    const int nd = FWD ? p.nbands * M : 3 * M;
    double2 *S = reinterpret_cast<double2 *>(s_d + ((nd + 1) & ~1)) + wave * wf::ChebWaveLds<R, NL, CH>::size;
    for (int i = tid; i < N; i += 64 * WV_WAVES) {
        s_tw[i] = p.tw[i];
        s_half[i] = p.half[i];
    }
    if (FWD) {
        for (int i = tid; i < p.nbands * M; i += 64 * WV_WAVES) s_d[i] = p.bands[i];
    } else {
        for (int i = tid; i < 2 * M; i += 64 * WV_WAVES) s_d[i] = p.bsub ? p.bsub[i] : 0.0;
        for (int i = tid; i < M; i += 64 * WV_WAVES) s_d[2 * M + i] = p.dvec ? p.dvec[i] : 0.0;
    }
    __syncthreads();                    // the only workgroup barrier
    wf::ChebTabs T;
    T.tw = s_tw;
    T.half = s_half;
    T.bands = s_d;
    T.bsub = s_d;
    T.dvec = s_d + 2 * M;
    T.M = M;
    T.Mk = 16 * NL;
    T.nbands = p.nbands;
    T.gcd_off = p.gcd_off;
    { T.boff1 = p.boff[1]; T.boff2 = p.boff[2]; T.boff3 = p.boff[3]; }
    const double kSqPi = 1.7724538509055160272981674833411, kSqPi2 = 1.2533141373155002512078826424055;
    T.fs0 = kSqPi / (2.0 * (double)N);
    T.fs1 = kSqPi2 / (double)N;
    T.bs0 = 1.0 / kSqPi;
    T.bs1 = 0.5 / kSqPi2;
    const wf::Lane L = wf::make_lane(lane);
    const unsigned g = xcd_swizzle(blockIdx.x, gridDim.x);
    const long inner = a.inner;
    // bytes between coefficient rows (kx-band-major state vector: 8 ny doubles)
    const unsigned rsb = (p.ctile_nseg && p.cband) ? (unsigned)(p.ctile_nseg * 512u) : (unsigned)(inner * 8);
    // grid side (the stage array between the z and the x transforms): natural [z][kx][ky], or x-blocked
    // [kx / 64][z][kx % 64][ky] (p.xb = ny): rows 64 ny doubles apart (256 KiB at ny = 512, not one 2 MiB page per row)
    const unsigned rsg = p.xb ? (unsigned)(64u * p.xb * 8u) : rsb;
    // i-th tile of this wave
    auto tile_of = [&](unsigned i) -> unsigned { return (g * a.tpw + i) * WV_WAVES + wave; };
    auto locate = [&](unsigned tile, long &off_c, long &off_g, bool &valid) {
        unsigned o, tb;
        a.fd_tpo.divmod(tile, o, tb);
        long seg = tb;                       // 64-byte segment of the coefficient row [nx][ny] ...
        if (p.ctile_nseg) {           // ... tile-major: [kx / 8][ky / 8][kx % 8] (ddh_cheb_forward_tiled, ddh_fft_set_coeff_tiled)
            const unsigned kxrow = tb / p.ctile_nseg, sg = tb - kxrow * p.ctile_nseg;
            seg = ((long)(kxrow >> 3) * p.ctile_nseg + sg) * 8 + (kxrow & 7);
        }
        const long pair0 = 4L * tb;
        off_c = ((long)o * M) * inner + 8 * seg;
        if (p.ctile_nseg && p.cband) {       // ... kx-band-major: [kx / 8][row][ky / 8][kx % 8]
            const unsigned kxrow = tb / p.ctile_nseg, sg = tb - kxrow * p.ctile_nseg;
            off_c = ((long)o * M) * (64L * p.ctile_nseg) + (long)(kxrow >> 3) * (long)p.cband + 64L * sg + 8L * (kxrow & 7);
        }
        off_g = ((long)o * N) * inner + 2 * pair0;
        if (p.xb) {
            const unsigned nsg = p.xb >> 3, kxrow = tb / nsg, sg = tb - kxrow * nsg;
            off_g = ((long)o * N) * inner + ((long)(kxrow >> 6) * N * 64 + (kxrow & 63)) * p.xb + 8L * sg;
        }
        valid = pair0 + L.p < a.npairs;
    };
    // The 8 waves of the workgroup take 8 neighbouring tiles per step.  With wsync they enter every step together, so
    // that their row requests (8 x 64 contiguous bytes per row) reach the memory controllers at the same time.
    const unsigned step0 = g * a.tpw * WV_WAVES;
    if (step0 >= a.ntiles) return;
    if (FWD) {
        for (unsigned i = 0; i < a.tpw; ++i) {
            if (step0 + i * WV_WAVES >= a.ntiles) break;                 // workgroup-uniform
            if (a.wsync && i > 0) __syncthreads();
            const unsigned tile = tile_of(i);
            if (tile >= a.ntiles) continue;
            long oc, og;
            bool valid;
            locate(tile, oc, og, valid);
            wf::cheb_fwd_tile<R, NL, CH>(a.src + og, a.dst + oc, rsg, rsb, valid, S, T, lane);
        }
    } else {
        double2 c[NL];
        long oc = 0, og = 0;
        bool valid = false;
        const bool have0 = tile_of(0) < a.ntiles;
        if (have0) {
            locate(tile_of(0), oc, og, valid);
            wf::cheb_bwd_load<NL>(c, a.src + oc, rsb, valid, L);
        }
        for (unsigned i = 0; i < a.tpw; ++i) {
            if (step0 + i * WV_WAVES >= a.ntiles) break;                 // workgroup-uniform
            if (a.wsync && i > 0) __syncthreads();
            if (tile_of(i) >= a.ntiles) continue;                        // this wave has run out of tiles (it still syncs)
            const unsigned tn = tile_of(i + 1);
            const bool more = (i + 1 < a.tpw) && (tn < a.ntiles);
            long ocn = oc, ogn = og;
            bool validn = valid;
            if (more) locate(tn, ocn, ogn, validn);
            const unsigned rsbn = more ? rsb : 0u;
            if (KIND == 1) {
                // the plain pass keeps c for the derivative pass
                wf::cheb_bwd_pass<R, NL, CH, 0, false>(c, S, T, a.dst + og, rsg, valid, lane, a.src + oc, rsb, valid);
                wf::cheb_bwd_pass<R, NL, CH, 1, true>(c, S, T, a.dst2 + og, rsg, valid, lane, a.src + ocn, rsbn, validn);
            } else {
                wf::cheb_bwd_pass<R, NL, CH, (KIND == 2 ? 2 : 0), true>(c, S, T, a.dst + og, rsg, valid, lane, a.src + ocn, rsbn,
                                                                      validn);
            }
            oc = ocn;
            og = ogn;
            valid = validn;
        }
    }
}

template <int KIND, int R, int NL>
static int launch_wave_cheb(const TransformPlan &tp, const FftDev &d, const WaveArgs &a, hipStream_t st) {
    auto kern = wave_cheb_kernel<KIND, R, NL, wf::WaveCH<R>::ch>;
    if (tp.lds > 64 * 1024)
        DDH_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tp.lds));
    hipLaunchKernelGGL(kern, dim3(tp.grid), dim3(tp.block), tp.lds, st, d, a);
    DDH_HIP(hipGetLastError());
    return 0;
}

// ---- Chebyshev along the CONTIGUOUS axis (the shell's radial transforms: [lines][192] <-> [lines][128]) ------------------
// The same lane code on lines that are contiguous in memory: a wave takes 8 consecutive lines (4 pairs of lines 2 p, 2 p + 1).
// Its loads follow the lane map directly (sixteen lanes of a row group read 128 contiguous bytes of one line); the grid rows
// of a backward transform leave the FFT scattered over the line (row 2 n / 2 (N - 1 - n) + 1 of FFT slot n), so they are
// written into the wave's LDS region -- laid out like the global lines, NP doubles apart -- and copied out with linear
// 16-byte stores.  The staging area is the region the transform itself has just used for its exchanges: the LDS
// operations of a wave execute in program order.  Replaces core/transforms.py:715-902 for a contiguous axis (the
// workgroup-per-tile kernel of ddh_fft.hip ran these short lines at 0.19-0.27 of the HBM rate).
constexpr int WC_WAVES = 4;

struct ContigArgs {
    const double *src;
    double *dst, *dst2;
    long nlines;             // even
    unsigned ntiles, tpw;    // tiles of 8 lines, tiles per wave
    int kind;                // backward: 0 plain, 1 dual (plain + derivative pass), 2 conversion solve
};

template <int R, int NL, int CH>
struct ChebContigLds {
    static constexpr int NP = 16 * R + 2;                       // doubles between staged lines (16-byte aligned line starts)
    static constexpr int a = wf::ChebWaveLds<R, NL, CH>::size, b = 4 * NP;
    static constexpr int size = a > b ? a : b;                  // double2 per wave
};

template <int KIND, int R, int NL, int CH>      // KIND: 0 backward plain, 1 backward dual, 2 backward conversion, 3 forward
__global__ void __launch_bounds__(64 * WC_WAVES, 2)
wave_cheb_contig_kernel(FftDev p, ContigArgs a) {
    constexpr bool FWD = (KIND == 3);
    extern __shared__ double2 lds[];
    constexpr int N = 16 * R, NP = ChebContigLds<R, NL, CH>::NP;
    const int M = p.M, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2 *s_tw = lds, *s_half = lds + N;
    double *s_d = reinterpret_cast<double *>(lds + 2 * N);
    const int nd = FWD ? p.nbands * M : 3 * M;
    double2 *S = reinterpret_cast<double2 *>(s_d + ((nd + 1) & ~1)) + wave * ChebContigLds<R, NL, CH>::size;
    for (int i = tid; i < N; i += 64 * WC_WAVES) {
        s_tw[i] = p.tw[i];
        s_half[i] = p.half[i];
    }
    if (FWD) {
        for (int i = tid; i < p.nbands * M; i += 64 * WC_WAVES) s_d[i] = p.bands[i];
    } else {
        for (int i = tid; i < 2 * M; i += 64 * WC_WAVES) s_d[i] = p.bsub ? p.bsub[i] : 0.0;
        for (int i = tid; i < M; i += 64 * WC_WAVES) s_d[2 * M + i] = (KIND == 1 && p.dvec) ? p.dvec[i] : 0.0;
    }
    __syncthreads();                    // the only workgroup barrier
    wf::ChebTabs T;
    T.tw = s_tw;
    T.half = s_half;
    T.bands = s_d;
    T.bsub = s_d;
    T.dvec = s_d + 2 * M;
    T.M = M;
    T.Mk = 16 * NL;
    T.nbands = p.nbands;
    T.gcd_off = p.gcd_off;
    { T.boff1 = p.boff[1]; T.boff2 = p.boff[2]; T.boff3 = p.boff[3]; }
    const double kSqPi = 1.7724538509055160272981674833411, kSqPi2 = 1.2533141373155002512078826424055;
    T.fs0 = kSqPi / (2.0 * (double)N);
    T.fs1 = kSqPi2 / (double)N;
    T.bs0 = 1.0 / kSqPi;
    T.bs1 = 0.5 / kSqPi2;
    const wf::Lane L = wf::make_lane(lane);
    const unsigned g = xcd_swizzle(blockIdx.x, gridDim.x);
    const unsigned lsc = (unsigned)(M * 8), lsg = (unsigned)(N * 8);      // bytes between coefficient / grid lines
    auto tile_of = [&](unsigned i) -> unsigned { return (g * a.tpw + i) * WC_WAVES + wave; };
    if (FWD) {
        for (unsigned i = 0; i < a.tpw; ++i) {
            const unsigned tile = tile_of(i);
            if (tile >= a.ntiles) break;
            const long l0 = 8L * tile;
            const bool valid = l0 + 2 * L.p < a.nlines;
            wf::cheb_fwd_tile<R, NL, CH, true>(a.src + l0 * N, a.dst + l0 * M, lsg, lsc, valid, S, T, lane);
        }
    } else {
        double2 c[NL];
        if (tile_of(0) >= a.ntiles) return;
        {
            const long l0 = 8L * tile_of(0);
            wf::cheb_bwd_load_contig<NL>(c, a.src + l0 * M, lsc, l0 + 2 * L.p < a.nlines, L);
        }
        double *stage = reinterpret_cast<double *>(S);
        // staged lines -> global, 16 bytes per lane and step
        auto copy_out = [&](double *out, long l0) {
            WF_SYNC();
#pragma unroll
            for (int it = 0; it < (8 * (N / 2) + 63) / 64; ++it) {
                const int ch = it * 64 + lane;
                const int l = ch / (N / 2), j = ch - l * (N / 2);
                if (ch < 8 * (N / 2) && l0 + l < a.nlines)
                    *reinterpret_cast<double2 *>(out + (long)l * N + 2 * j) = *reinterpret_cast<const double2 *>(stage + l * NP + 2 * j);
            }
            WF_SYNC();
        };
        for (unsigned i = 0; i < a.tpw; ++i) {
            const unsigned tile = tile_of(i);
            if (tile >= a.ntiles) break;
            const long l0 = 8L * tile;
            const bool valid = l0 + 2 * L.p < a.nlines;
            const unsigned tn = tile_of(i + 1);
            const bool more = (i + 1 < a.tpw) && (tn < a.ntiles);
            const long l0n = more ? 8L * tn : l0;
            const bool validn = l0n + 2 * L.p < a.nlines;
            const unsigned lscn = more ? lsc : 0u;
            if (KIND == 1) {
                // the plain pass keeps c for the derivative pass (field and d/dz from one read of the coefficients)
                wf::cheb_bwd_pass<R, NL, CH, 0, false, true>(c, S, T, stage, (unsigned)(NP * 8), valid, lane, a.src + l0 * M, lsc, valid);
                copy_out(a.dst + l0 * N, l0);
                wf::cheb_bwd_pass<R, NL, CH, 1, true, true>(c, S, T, stage, (unsigned)(NP * 8), valid, lane, a.src + l0n * M, lscn, validn);
                copy_out(a.dst2 + l0 * N, l0);
            } else {
                if (KIND == 2)
                    wf::cheb_bwd_pass<R, NL, CH, 2, true, true>(c, S, T, stage, (unsigned)(NP * 8), valid, lane, a.src + l0n * M, lscn, validn);
                else
                    wf::cheb_bwd_pass<R, NL, CH, 0, true, true>(c, S, T, stage, (unsigned)(NP * 8), valid, lane, a.src + l0n * M, lscn, validn);
                copy_out(a.dst + l0 * N, l0);
            }
        }
    }
}

template <int KIND, int R, int NL>
static int launch_wave_cheb_contig(const TransformPlan &tp, const FftDev &d, const ContigArgs &a, hipStream_t st) {
    auto kern = wave_cheb_contig_kernel<KIND, R, NL, wf::WaveCH<R>::ch>;
    if (tp.lds > 64 * 1024)
        DDH_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tp.lds));
    hipLaunchKernelGGL(kern, dim3(tp.grid), dim3(tp.block), tp.lds, st, d, a);
    DDH_HIP(hipGetLastError());
    return 0;
}

// ---- real Fourier, 3/2 dealiasing (N = 48 R, M = 32 R): RKIND 0 backward, 1 backward differentiated, 2 backward dual
// (plain + differentiated), 3 forward
template <int RKIND, int R>
__global__ void __launch_bounds__(64 * WR_WAVES, 2)
wave_rfft_kernel(FftDev p, WaveArgs a) {
    extern __shared__ double2 lds[];
    constexpr int N = 48 * R, M = 32 * R;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double2 *s_tw = lds;
    double2 *S = lds + N + wave * wf::RfftWaveLds<R>::size;
    for (int i = tid; i < N; i += 64 * WR_WAVES) s_tw[i] = p.tw[i];
    __syncthreads();                    // the only workgroup barrier
    const unsigned g = xcd_swizzle(blockIdx.x, gridDim.x);
    const long inner = a.inner;
    const unsigned rsb = (unsigned)(inner * 8);
    const int p4 = lane & 3;
    for (unsigned i = 0; i < a.tpw; ++i) {
        if ((g * a.tpw + i) * WR_WAVES >= a.ntiles) break;               // workgroup-uniform
        if (a.wsync && i > 0) __syncthreads();
        const unsigned tile = (g * a.tpw + i) * WR_WAVES + wave;
        if (tile >= a.ntiles) continue;
        unsigned o, tb;
        a.fd_tpo.divmod(tile, o, tb);
        const long pair0 = 4L * tb;
        long oc = ((long)o * M) * inner + 2 * pair0;
        const long og = ((long)o * N) * inner + 2 * pair0;
        unsigned rsb64 = 64u * rsb;
        int bsh = 1;
        if (p.xb) {
            // coefficient side = the stage array [comp][kx / B][z][kx % B][ky], o = comp * gz + z (p.xb = gz; B = 64 on one
            // rank, nx / P in a sharded run: the layout [p][z][nx / P][ky] the exchange delivers / takes)
            const unsigned B = p.xbB ? p.xbB : 64u;
            unsigned comp, z;
            if (p.xbwn) {                                // a window of every component's planes (ddh_fft_set_stage_window)
                comp = o / p.xbwn;
                z = p.xbw0 + (o - comp * p.xbwn);
            } else {
                comp = o / p.xb;
                z = o - comp * p.xb;
            }
            oc = ((long)comp * M * p.xb + (long)B * z) * inner + 2 * pair0;
            rsb64 = (unsigned)(B * p.xb) * rsb;
            bsh = (B == 64u) ? 1 : ((B == 128u) ? 2 : 3);
        }
        const bool valid = pair0 + p4 < a.npairs;
        if (RKIND == 3) wf::rfft_fwd_tile<R>(a.src + og, a.dst + oc, rsb, rsb64, valid, S, s_tw, lane, bsh);
        else wf::rfft_bwd_tile<R, (RKIND == 3 ? 0 : RKIND)>(a.src + oc, a.dst + og, (RKIND == 2) ? a.dst2 + og : nullptr, rsb, rsb64, valid,
                                                            (RKIND == 2) ? p.dscale2 : p.dscale, S, s_tw, lane, bsh);
    }
}

template <int RKIND, int R>
static int launch_wave_rfft(const TransformPlan &tp, const FftDev &d, const WaveArgs &a, hipStream_t st) {
    auto kern = wave_rfft_kernel<RKIND, R>;
    if (tp.lds > 64 * 1024)
        DDH_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tp.lds));
    hipLaunchKernelGGL(kern, dim3(tp.grid), dim3(tp.block), tp.lds, st, d, a);
    DDH_HIP(hipGetLastError());
    return 0;
}

// ---- which kernel a transform takes -------------------------------------------------------------------------------------
// A size's entry in DDH_CHEB_WAVE_SIZES / DDH_RFFT_WAVE_SIZES and the LDS its kernels need per wave (double2)
struct WaveSize {
    int R, NL;
    size_t strided, contig;
};
static bool wave_size(int kind, int N, int M, WaveSize &ws) {
#define DDH_X(RV, NLV)                                                                             \
    if (kind == K_CHEB && N == 16 * RV && M == 16 * NLV) {                                         \
        ws = {RV, NLV, (size_t)wf::ChebWaveLds<RV, NLV, wf::WaveCH<RV>::ch>::size,                  \
              (size_t)ChebContigLds<RV, NLV, wf::WaveCH<RV>::ch>::size};                           \
        return true;                                                                               \
    }
    DDH_CHEB_WAVE_SIZES(DDH_X)
#undef DDH_X
#define DDH_X(RV)                                                                                  \
    if (kind == K_RFFT && N == 48 * RV && M == 32 * RV) {                                          \
        ws = {RV, 0, (size_t)wf::RfftWaveLds<RV>::size, 0};                                        \
        return true;                                                                               \
    }
    DDH_RFFT_WAVE_SIZES(DDH_X)
#undef DDH_X
    return false;
}

TransformPlan transform_plan(const FftDev &d, int mode, long outer, long inner, bool second, bool deriv, bool dvec,
                             bool aliased) {
    // A/B and fallback selectors (read here and nowhere else).  DDH_FFT_WAVE: bit 0 Chebyshev, bit 1 real FFT on the strided
    // wave kernels; DDH_CHEB_CONTIG_WAVE=0: contiguous Chebyshev lines on the workgroup kernel
    static const int mask = getenv("DDH_FFT_WAVE") ? atoi(getenv("DDH_FFT_WAVE")) : 3;
    static const int contig_on = getenv("DDH_CHEB_CONTIG_WAVE") ? atoi(getenv("DDH_CHEB_CONTIG_WAVE")) : 1;
    TransformPlan tp{};
    const bool cheb = (mode == CHEB_FWD || mode == CHEB_BWD), rfft = (mode == RFFT_FWD || mode == RFFT_BWD);
    const bool cfft = !cheb && !rfft, strided = inner > 1;
    const int N = d.N;
    WaveSize ws{};
    bool wave_ok = !cfft && wave_size(cheb ? K_CHEB : K_RFFT, N, d.M, ws);
    tp.R = ws.R;
    tp.NL = ws.NL;
    // the variant of the size's wave kernel; the conversion solve of the wave kernels takes first-order chains of stride 1 or 2
    const bool chain_ok = d.bsub && d.bsub_order == 1 && (d.gcd_off == 1 || d.gcd_off == 2);
    if (mode == CHEB_FWD || mode == RFFT_FWD) {
        tp.kind = 3;
    } else if (mode == CHEB_BWD && second) {
        tp.kind = 1;
        wave_ok = wave_ok && chain_ok && dvec;
    } else if (mode == CHEB_BWD && d.nbands > 0) {
        tp.kind = 2;
        wave_ok = wave_ok && chain_ok;
    } else if (mode == RFFT_BWD) {
        tp.kind = second ? 2 : (deriv ? 1 : 0);
        wave_ok = wave_ok && !(second && deriv);     // the dual entry point transforms plainly into dst
    }
    if (rfft) wave_ok = wave_ok && d.K == d.M / 2 - 1;
    // LDS of the Chebyshev wave kernels: twiddles, half-angle factors, the bands / back-substitution + derivative tables
    const size_t cheb_tabs = (size_t)2 * N * sizeof(double2) + (size_t)(((mode == CHEB_FWD ? d.nbands * d.M : 3 * d.M) + 1) & ~1) * sizeof(double);

    if (wave_ok && strided && (mask & (cheb ? 1 : 2)) && !(inner & 1)) {
        // the plan's layouts: shapes they are defined for
        bool layout_ok = true;
        if (d.xb && cheb) {
            layout_ok = !((d.xb & 7) || inner % d.xb || (inner / d.xb) % 64);
        } else if (d.xb) {
            const unsigned long B = d.xbB ? d.xbB : 64UL;
            // (outer: whole components of gz planes each, or of the xbwn planes of a window)
            layout_ok = (B == 64 || B == 128 || B == 256) && !(d.xbwn && (d.xbw0 + d.xbwn > d.xb)) &&
                        !(outer % (d.xbwn ? d.xbwn : d.xb) || d.M % B ||
                          (unsigned long)d.xb * B * (unsigned long)inner * 8UL * (unsigned long)(d.M / B) >= 0xffffffffUL);
        }
        if (d.ctile_nseg && (!cheb || inner % (8L * d.ctile_nseg) || (inner / (8L * d.ctile_nseg)) % 8)) layout_ok = false;
        const long npairs = inner / 2, tpo = (npairs + 3) / 4;
        const unsigned long ntiles = (unsigned long)tpo * (unsigned long)outer;
        const unsigned long wpg = rfft ? WR_WAVES : WV_WAVES;
        const size_t lds = rfft ? ((size_t)N + wpg * ws.strided) * sizeof(double2) : cheb_tabs + wpg * ws.strided * sizeof(double2);
        if (layout_ok && ntiles <= 0x7fffffffUL && lds <= 160 * 1024 &&
            (unsigned long)N * (unsigned long)inner * 8UL < 0xffffffffUL) {     // 32-bit row offsets inside a tile
            tp.kernel = cheb ? TransformKernel::cheb_wave : TransformKernel::rfft_wave;
            tp.npairs = npairs;
            tp.tpo = (unsigned)tpo;
            tp.ntiles = (unsigned)ntiles;
            // tiles per wave / per-tile workgroup sync: measured per kernel at 3 x 256 x 512^2 and 1152 x 512 x 512
            // (tools/bench_strided.py, profiles/archive/r3_strided_sweep.txt)
            unsigned tpw = 1;
            if (mode == CHEB_FWD) {
                tpw = 4;
                tp.wsync = 1;
            } else if (mode == CHEB_BWD && tp.kind != 1) {
                tpw = 2;
            }
            while (tpw > 1 && ntiles / (tpw * wpg) < 1024) tpw /= 2;   // several rounds of workgroups
            tp.tpw = tpw;
            tp.grid = (unsigned)((ntiles + tpw * wpg - 1) / (tpw * wpg));
            tp.block = (unsigned)(64 * wpg);
            tp.lds = lds;
            return tp;
        }
    }
    if (wave_ok && !strided && cheb && contig_on && !d.xb && !d.ctile_nseg && !(outer & 1) && outer >= 2 && !aliased) {
        const unsigned long ntiles = ((unsigned long)outer + 7) / 8;
        const size_t lds = cheb_tabs + (size_t)WC_WAVES * ws.contig * sizeof(double2);
        if (ntiles <= 0x7fffffffUL && lds <= 160 * 1024) {
            tp.kernel = TransformKernel::cheb_contig_wave;
            tp.ntiles = (unsigned)ntiles;
            unsigned long tpw = 4;
            while (tpw > 1 && ntiles / (tpw * WC_WAVES) < 2048) tpw /= 2;   // several rounds of workgroups
            tp.tpw = (unsigned)tpw;
            tp.grid = (unsigned)((ntiles + tpw * WC_WAVES - 1) / (tpw * WC_WAVES));
            tp.block = 64 * WC_WAVES;
            tp.lds = lds;
            return tp;
        }
    }

    // the workgroup-per-tile kernel of ddh_fft.hip: every size, natural layouts only
    tp.kernel = TransformKernel::workgroup;
    if (d.xb && strided) {
        tp.error = "x-blocked stage layout (ddh_fft_set_stage_layout): only the strided-axis wave kernels at their instantiated "
                   "sizes read / write it, and this transform has none";
        return tp;
    }
    if (d.ctile_nseg) {
        tp.error = "tile-major coefficient rows (ddh_cheb_forward_tiled, ddh_fft_set_coeff_tiled): only the strided-axis "
                   "Chebyshev wave kernels at their instantiated sizes read / write that layout";
        return tp;
    }
    tp.inner = strided;
    if (cfft)
        tp.npairs = strided ? inner : outer;
    else
        tp.npairs = strided ? (inner + 1) / 2 : (outer + 1) / 2;
    // lines per workgroup: 128 B of contiguous data per row when strided; bounded by LDS (<= 64 KiB so that at least two
    // workgroups share a CU) and by 12 staged values per thread.
    const size_t per_line = (size_t)d.ld * sizeof(double2);
    int B = strided ? 8 : 4;
    if (!strided) {
        // contiguous SHORT lines (the shell's radial transforms: 192 <- 128): 4 line pairs are a tile of a few KiB, the
        // workgroup's fixed costs (twiddle tables, barriers) dominate -- up to 16 pairs while a thread keeps <= 12 items
        while (B < 16 && (long)N * (2 * B) <= 12L * 256) B *= 2;
    }
    while (B > 1 && per_line * B > 64 * 1024) B /= 2;
    if ((long)B > tp.npairs) B = (int)tp.npairs;
    // the launch's whole dynamic-LDS request (lines and the two-level twiddle table) against the 160 KiB of a workgroup
    if (per_line * B + (size_t)tw_entries(N) * sizeof(double2) > 160 * 1024) {
        tp.error = "transform: axis too long for the LDS kernel";
        return tp;
    }
    int T = 256;
    while ((long)N * B > 12L * T && T < 1024) T *= 2;
    if ((long)N * B > 12L * T) {
        tp.error = "transform: axis too long for the LDS kernel (registers)";
        return tp;
    }
    tp.B = B;
    tp.bpo = (unsigned)((tp.npairs + B - 1) / B);
    const unsigned long nblocks = strided ? (unsigned long)tp.bpo * (unsigned long)outer : tp.bpo;
    if (nblocks > 0x7fffffffUL) {
        tp.error = "transform: grid too large";
        return tp;
    }
    tp.grid = (unsigned)nblocks;
    tp.block = (unsigned)T;
    tp.lds = per_line * B + (size_t)tw_entries(N) * sizeof(double2);
    return tp;
}

static WaveArgs wave_args(const TransformPlan &tp, const FftDev &d, const double *src, double *dst, long inner) {
    WaveArgs a;
    a.src = src;
    a.dst = dst;
    a.dst2 = d.dst2;
    a.inner = inner;
    a.npairs = tp.npairs;
    a.fd_tpo.set(tp.tpo);
    a.ntiles = tp.ntiles;
    a.tpw = tp.tpw;
    a.kind = tp.kind == 3 ? 0 : tp.kind;
    a.wsync = tp.wsync;
    return a;
}

// the template instance of a plan: KIND / RKIND x the size tables
#define DDH_KIND_SWITCH(FN, ...)                                       \
    switch (tp.kind) {                                                 \
        case 3: return FN<3, __VA_ARGS__>(tp, d, a, st);               \
        case 2: return FN<2, __VA_ARGS__>(tp, d, a, st);               \
        case 1: return FN<1, __VA_ARGS__>(tp, d, a, st);               \
        default: return FN<0, __VA_ARGS__>(tp, d, a, st);              \
    }

int launch_cheb_wave(const TransformPlan &tp, const FftDev &d, const double *src, double *dst, long inner, hipStream_t st) {
    const WaveArgs a = wave_args(tp, d, src, dst, inner);
#define DDH_X(RV, NLV) \
    if (tp.R == RV && tp.NL == NLV) DDH_KIND_SWITCH(launch_wave_cheb, RV, NLV)
    DDH_CHEB_WAVE_SIZES(DDH_X)
#undef DDH_X
    return fail("transform: no Chebyshev wave kernel of this size");
}

int launch_rfft_wave(const TransformPlan &tp, const FftDev &d, const double *src, double *dst, long inner, hipStream_t st) {
    const WaveArgs a = wave_args(tp, d, src, dst, inner);
#define DDH_X(RV) \
    if (tp.R == RV) DDH_KIND_SWITCH(launch_wave_rfft, RV)
    DDH_RFFT_WAVE_SIZES(DDH_X)
#undef DDH_X
    return fail("transform: no real-FFT wave kernel of this size");
}

int launch_cheb_contig_wave(const TransformPlan &tp, const FftDev &d, const double *src, double *dst, long outer, hipStream_t st) {
    ContigArgs a;
    a.src = src;
    a.dst = dst;
    a.dst2 = d.dst2;
    a.nlines = outer;
    a.ntiles = tp.ntiles;
    a.tpw = tp.tpw;
    a.kind = tp.kind == 3 ? 0 : tp.kind;
#define DDH_X(RV, NLV) \
    if (tp.R == RV && tp.NL == NLV) DDH_KIND_SWITCH(launch_wave_cheb_contig, RV, NLV)
    DDH_CHEB_WAVE_SIZES(DDH_X)
#undef DDH_X
    return fail("transform: no Chebyshev wave kernel of this size");
}
#undef DDH_KIND_SWITCH

}  // namespace ddh

using namespace ddh;

extern "C" int ddh_fft_wave_size(int kind, int n_grid, int n_coeff, int *covered) {
    if (!covered) return fail("ddh_fft_wave_size: null pointer");
    if (kind != K_RFFT && kind != K_CHEB) return fail("ddh_fft_wave_size: kind 0 (real FFT) or 1 (Chebyshev)");
    WaveSize ws;
    *covered = wave_size(kind, n_grid, n_coeff, ws) ? 1 : 0;
    return 0;
}
