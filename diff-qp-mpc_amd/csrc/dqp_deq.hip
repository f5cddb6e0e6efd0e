// dqp_deq.hip -- the LayerNorm stages of the DEQ-MPC trajectory network (policies.DEQLayer) as fused fp32 kernels
// (dqp_deq_*, include/dqp.h "network-side kernels").  One DEQLayer call is, between its three GEMMs,
//     stage A   y  = LN(relu ? max(a, 0) : a)                 the input LayerNorm (relu 0), lndeq1(reludeq1(.)) (relu 1)
//     stage B   z2 = LN3(ReLU(z1 + LN2(xi + a2)))             the residual block behind fcdeq2
// and each stage is one pass over its (nrows, hdim) operands forward and one backward; the backward recomputes every
// intermediate from the stage's inputs and the per-row statistics (mean, rstd), so nothing of size (nrows, hdim) is
// saved between the two.
//
// Layout: a row lives in the registers of one wavefront, hdim / 64 elements per lane (at hdim 32 two rows share a
// wavefront, one per 32-lane half).  A lane owns V = min(4, hdim / 64) consecutive floats per chunk of 64 V columns --
// 16-byte accesses at hdim 256 (one) and 512 (two), 8-byte at 128, 4-byte at 64 and 32.  Statistics are two-pass on the
// registers: the mean, then the (biased) variance of the centred values, rstd = 1 / sqrt(var + eps); the arithmetic in
// registers is fp64 (see "Arithmetic" below).  Row sums are DPP row rotations, one v_permlane16_swap and (64 lanes) one
// v_permlane32_swap: every lane ends with the same bits.
//
// Rows to workgroups: a unit is one row (a pair of rows at hdim 32); a wavefront owns rpw = max(2, ceil(units / 4096))
// consecutive units, a workgroup of four wavefronts 4 rpw of them -- a function of nrows and hdim alone, at most 1024
// workgroups (the forward kernels, which leave no partials, take half as many rows per wavefront).
// Parameter gradients (sums over rows): a lane adds its columns over its wavefront's rows in row order, the four
// wavefronts are added in wavefront (= row) order through LDS into partial[workgroup], and deq_finish_kernel adds the
// partials in ascending workgroup order, in fp64, and rounds once (a sequential fp32 chain over a thousand partials
// would lose two digits against the tree sums of torch's LayerNorm backward).  No atomics: bit-identical from run to
// run, on any number of CUs.
#include <hip/hip_runtime.h>

#include "dqp_common.h"

namespace dqp {
namespace deq {

constexpr int WG = 256, WAVES = WG / WAVE;
constexpr int MAX_WG = 1024;      // workgroups = partials of a backward call, at most
constexpr int MAX_WG_FWD = 2048;  // a forward call leaves no partials: enough wavefronts to fill every SIMD's eight slots
constexpr int MIN_RPW = 2;        // units per wavefront, at least
constexpr int NVEC = 4;           // vectors per partial: dgamma2 dbeta2 dgamma3 dbeta3 (stage A uses the first two)
constexpr int FIN_COLS = 64, FIN_ROWS = 128, FIN_WG = 512;   // finish: columns per workgroup, partials per LDS chunk

struct Part {
    long long units, rpw;
    int nwg;
};

static Part partition(int nrows, int hdim, int max_wg = MAX_WG)
{
    Part p;
    p.units = hdim == 32 ? ((long long)nrows + 1) / 2 : nrows;
    p.rpw = (p.units + (long long)max_wg * WAVES - 1) / ((long long)max_wg * WAVES);
    if (p.rpw < MIN_RPW) p.rpw = MIN_RPW;
    p.nwg = (int)((p.units + p.rpw * WAVES - 1) / (p.rpw * WAVES));
    return p;
}

static bool hdim_ok(int h) { return h == 32 || h == 64 || h == 128 || h == 256 || h == 512; }

template <int H> struct Cfg {
    static constexpr int LPR = H == 32 ? 32 : 64;       // lanes per row
    static constexpr int RPU = WAVE / LPR;              // rows per unit
    static constexpr int E = H / LPR;                   // elements per lane
    static constexpr int V = E < 4 ? E : 4;             // floats per access
    static constexpr int NV = E / V;                    // accesses per row and lane
    // column of element e of lane lr
    __device__ static __forceinline__ int col(int lr, int e) { return (e / V) * (LPR * V) + lr * V + (e % V); }
};

template <int V> __device__ __forceinline__ void ldv(const float *p, float *x)
{
    if constexpr (V == 1) {
        x[0] = *p;
    } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        x[0] = t.x; x[1] = t.y;
    } else {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    }
}

template <int V> __device__ __forceinline__ void stv(float *p, const float *x)
{
    if constexpr (V == 1) *p = x[0];
    else if constexpr (V == 2) *reinterpret_cast<float2 *>(p) = make_float2(x[0], x[1]);
    else *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
}

// the lane's E elements of the row (or parameter vector) at p
template <int H> __device__ __forceinline__ void load_row(const float *p, int lr, float *x)
{
    using C = Cfg<H>;
#pragma unroll
    for (int k = 0; k < C::NV; ++k) ldv<C::V>(p + k * (C::LPR * C::V) + lr * C::V, x + k * C::V);
}

template <int H> __device__ __forceinline__ void store_row(float *p, int lr, const float *x)
{
    using C = Cfg<H>;
#pragma unroll
    for (int k = 0; k < C::NV; ++k) stv<C::V>(p + k * (C::LPR * C::V) + lr * C::V, x + k * C::V);
}

template <int CTRL> __device__ __forceinline__ double dppd(double v)
{
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, true);
}

// a + b where, of two copies of v, SWAP has left a in the first and b in the second
#define DEQ_SWAP_ADD(SWAP, v)                                                                                        \
    do {                                                                                                             \
        const auto lo_ = SWAP(__double2loint(v), __double2loint(v), false, false);                                   \
        const auto hi_ = SWAP(__double2hiint(v), __double2hiint(v), false, false);                                   \
        v = __hiloint2double(hi_[0], lo_[0]) + __hiloint2double(hi_[1], lo_[1]);                                     \
    } while (0)

// sum over the LPR lanes of a row, the same bits in each of them
template <int LPR> __device__ __forceinline__ double lanes_sum(double v)
{
    v += dppd<0x128>(v); v += dppd<0x124>(v); v += dppd<0x122>(v); v += dppd<0x121>(v);      // row_ror 8 4 2 1
    DEQ_SWAP_ADD(__builtin_amdgcn_permlane16_swap, v);             // even + odd DPP row of the 32-lane half
    if constexpr (LPR == 64) DEQ_SWAP_ADD(__builtin_amdgcn_permlane32_swap, v);              // lower + upper half
    return v;
}

// Arithmetic: operands and results are fp32 in memory; in registers every value of a row is fp64 from the load to the
// one rounding at the store (or at the update of an fp32 running sum).  These kernels move 8 to 24 bytes per element and
// do 10 to 40 flops on it, so the fp64 vector rate stays under the memory time, and an output then carries its final
// rounding instead of the five to ten of an fp32 chain.  mean and rstd reach the backward as the fp32 in `stats`.

// mean and rstd of the row in x; x becomes the centred row
template <int H> __device__ __forceinline__ void centre(double *x, double eps, double &mean, double &rstd)
{
    using C = Cfg<H>;
    double s = x[0];
#pragma unroll
    for (int e = 1; e < C::E; ++e) s += x[e];
    mean = lanes_sum<C::LPR>(s) * (1.0 / H);
    double q = 0.0;
#pragma unroll
    for (int e = 0; e < C::E; ++e) {
        x[e] -= mean;
        q = fma(x[e], x[e], q);
    }
    rstd = 1.0 / sqrt(lanes_sum<C::LPR>(q) * (1.0 / H) + eps);
}

// g = cotangent times gamma, xh = the normalised row: g becomes the cotangent of the LayerNorm's input
template <int H> __device__ __forceinline__ void ln_input_grad(double *g, const double *xh, double rstd)
{
    using C = Cfg<H>;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int e = 0; e < C::E; ++e) {
        s1 += g[e];
        s2 = fma(g[e], xh[e], s2);
    }
    const double m1 = lanes_sum<C::LPR>(s1) * (1.0 / H), m2 = lanes_sum<C::LPR>(s2) * (1.0 / H);
#pragma unroll
    for (int e = 0; e < C::E; ++e) g[e] = rstd * (g[e] - m1 - xh[e] * m2);
}

// acc += t, rounded once
__device__ __forceinline__ void add_to(float &acc, double t) { acc = (float)((double)acc + t); }

template <int H> __device__ __forceinline__ void store_row(float *p, int lr, const double *x)
{
    float f[Cfg<H>::E];
#pragma unroll
    for (int e = 0; e < Cfg<H>::E; ++e) f[e] = (float)x[e];
    store_row<H>(p, lr, f);
}

struct Rows {
    int lane, lr, sub;
    long long u, u1;
};

template <int H> __device__ __forceinline__ Rows my_rows(long long units, long long rpw)
{
    Rows r;
    r.lane = threadIdx.x & (WAVE - 1);
    r.lr = r.lane & (Cfg<H>::LPR - 1);
    r.sub = r.lane / Cfg<H>::LPR;
    r.u = ((long long)blockIdx.x * WAVES + (threadIdx.x >> 6)) * rpw;
    r.u1 = r.u + rpw < units ? r.u + rpw : units;
    return r;
}

// acc[v][e]: this lane's sums of vector v over its wavefront's rows -> partial[blockIdx.x][v][H], the wavefronts added
// in order (in fp64, rounded once)
template <int H, int NV_> __device__ __forceinline__ void write_partial(float (&acc)[NV_][Cfg<H>::E], const Rows &R,
                                                                        float *part)
{
    using C = Cfg<H>;
    __shared__ float sm[WAVES * C::RPU][NV_ * H];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV_; ++v)
#pragma unroll
        for (int e = 0; e < C::E; ++e) sm[wave * C::RPU + R.sub][v * H + C::col(R.lr, e)] = acc[v][e];
    __syncthreads();
    float *o = part + (long long)blockIdx.x * (NVEC * H);
    for (int i = threadIdx.x; i < NV_ * H; i += WG) {
        double s = sm[0][i];
#pragma unroll
        for (int w = 1; w < WAVES * C::RPU; ++w) s += (double)sm[w][i];
        o[i] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------- stage A
template <int H>
__global__ __launch_bounds__(WG) void deq_ln_forward_kernel(const float *__restrict__ a, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, double eps, int relu,
                                                             float *__restrict__ y, float *__restrict__ stats, int nrows,
                                                             long long units, long long rpw)
{
    using C = Cfg<H>;
    constexpr int E = C::E;
    const Rows R = my_rows<H>(units, rpw);
    if (R.u >= R.u1) return;
    float g[E], b[E], nx[E];
    load_row<H>(gamma, R.lr, g);
    load_row<H>(beta, R.lr, b);
    auto fetch = [&](long long u) {
        long long row = C::RPU * u + R.sub;
        row = row < nrows ? row : (long long)nrows - 1;          // the odd tail of a row pair reads a valid row
        load_row<H>(a + row * H, R.lr, nx);
    };
    fetch(R.u);
    for (long long u = R.u; u < R.u1; ++u) {
        double x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = (relu && nx[e] < 0.0f) ? 0.0 : (double)nx[e];
        if (u + 1 < R.u1) fetch(u + 1);
        double mean, rstd;
        centre<H>(x, eps, mean, rstd);
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = fma(x[e] * rstd, (double)g[e], (double)b[e]);
        const long long row = C::RPU * u + R.sub;
        if (row < nrows) {
            store_row<H>(y + row * H, R.lr, x);
            if (R.lr == 0) *reinterpret_cast<float2 *>(stats + 2 * row) = make_float2((float)mean, (float)rstd);
        }
    }
}

template <int H>
__global__ __launch_bounds__(WG) void deq_ln_backward_kernel(const float *__restrict__ a, const float *__restrict__ gamma,
                                                              const float *__restrict__ stats, int relu,
                                                              const float *__restrict__ dy, float *__restrict__ da,
                                                              float *__restrict__ part, int nrows, long long units,
                                                              long long rpw)
{
    using C = Cfg<H>;
    constexpr int E = C::E;
    const Rows R = my_rows<H>(units, rpw);
    float acc[2][E];        // dgamma dbeta
#pragma unroll
    for (int e = 0; e < E; ++e) acc[0][e] = acc[1][e] = 0.0f;
    if (R.u < R.u1) {
        float g[E], na[E], nd[E];
        float2 nst;
        load_row<H>(gamma, R.lr, g);
        auto fetch = [&](long long u) {
            long long row = C::RPU * u + R.sub;
            row = row < nrows ? row : (long long)nrows - 1;
            load_row<H>(a + row * H, R.lr, na);
            load_row<H>(dy + row * H, R.lr, nd);
            nst = *reinterpret_cast<const float2 *>(stats + 2 * row);
        };
        fetch(R.u);
        for (long long u = R.u; u < R.u1; ++u) {
            double x[E], d[E], gg[E];
            const double mean = nst.x, rstd = nst.y;
            bool pos[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                pos[e] = !relu || na[e] > 0.0f;
                x[e] = (((relu && na[e] < 0.0f) ? 0.0 : (double)na[e]) - mean) * rstd;
                d[e] = nd[e];
                gg[e] = d[e] * (double)g[e];
            }
            if (u + 1 < R.u1) fetch(u + 1);
            ln_input_grad<H>(gg, x, rstd);
            const long long row = C::RPU * u + R.sub;
            if (row < nrows) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    gg[e] = pos[e] ? gg[e] : 0.0;
                    add_to(acc[0][e], d[e] * x[e]);
                    add_to(acc[1][e], d[e]);
                }
                if (da) store_row<H>(da + row * H, R.lr, gg);
            }
        }
    }
    if (part) write_partial<H, 2>(acc, R, part);
}

// ---------------------------------------------------------------------------------------------------- stage B
struct ResArgs {
    const float *xi, *a2, *z1, *gamma2, *beta2, *gamma3, *beta3, *stats_in, *dz2;
    float *z2, *stats, *ds, *dz1, *part;
    double eps2, eps3;
    int nrows;
    long long units, rpw;
};

template <int H> __global__ __launch_bounds__(WG) void deq_res_forward_kernel(ResArgs A)
{
    using C = Cfg<H>;
    constexpr int E = C::E;
    const Rows R = my_rows<H>(A.units, A.rpw);
    if (R.u >= R.u1) return;
    float g2[E], b2[E], g3[E], b3[E], nxi[E], na2[E], nz1[E];
    load_row<H>(A.gamma2, R.lr, g2);
    load_row<H>(A.beta2, R.lr, b2);
    load_row<H>(A.gamma3, R.lr, g3);
    load_row<H>(A.beta3, R.lr, b3);
    auto fetch = [&](long long u) {
        long long row = C::RPU * u + R.sub;
        row = row < A.nrows ? row : (long long)A.nrows - 1;
        load_row<H>(A.xi + row * H, R.lr, nxi);
        load_row<H>(A.a2 + row * H, R.lr, na2);
        load_row<H>(A.z1 + row * H, R.lr, nz1);
    };
    fetch(R.u);
    for (long long u = R.u; u < R.u1; ++u) {
        double s[E], z[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            s[e] = (double)nxi[e] + (double)na2[e];
            z[e] = nz1[e];
        }
        if (u + 1 < R.u1) fetch(u + 1);
        double mean2, rstd2, mean3, rstd3;
        centre<H>(s, A.eps2, mean2, rstd2);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double t = z[e] + fma(s[e] * rstd2, (double)g2[e], (double)b2[e]);
            s[e] = t < 0.0 ? 0.0 : t;
        }
        centre<H>(s, A.eps3, mean3, rstd3);
#pragma unroll
        for (int e = 0; e < E; ++e) s[e] = fma(s[e] * rstd3, (double)g3[e], (double)b3[e]);
        const long long row = C::RPU * u + R.sub;
        if (row < A.nrows) {
            store_row<H>(A.z2 + row * H, R.lr, s);
            if (R.lr == 0)
                *reinterpret_cast<float4 *>(A.stats + 4 * row) =
                    make_float4((float)mean2, (float)rstd2, (float)mean3, (float)rstd3);
        }
    }
}

template <int H> __global__ __launch_bounds__(WG) void deq_res_backward_kernel(ResArgs A)
{
    using C = Cfg<H>;
    constexpr int E = C::E;
    const Rows R = my_rows<H>(A.units, A.rpw);
    float acc[4][E];        // dgamma2 dbeta2 dgamma3 dbeta3
#pragma unroll
    for (int e = 0; e < E; ++e) acc[0][e] = acc[1][e] = acc[2][e] = acc[3][e] = 0.0f;
    if (R.u < R.u1) {
        float g2[E], b2[E], g3[E], nxi[E], na2[E], nz1[E], nd[E];
        float4 nst;
        load_row<H>(A.gamma2, R.lr, g2);
        load_row<H>(A.beta2, R.lr, b2);
        load_row<H>(A.gamma3, R.lr, g3);
        auto fetch = [&](long long u) {
            long long row = C::RPU * u + R.sub;
            row = row < A.nrows ? row : (long long)A.nrows - 1;
            load_row<H>(A.xi + row * H, R.lr, nxi);
            load_row<H>(A.a2 + row * H, R.lr, na2);
            load_row<H>(A.z1 + row * H, R.lr, nz1);
            load_row<H>(A.dz2 + row * H, R.lr, nd);
            nst = *reinterpret_cast<const float4 *>(A.stats_in + 4 * row);
        };
        fetch(R.u);
        for (long long u = R.u; u < R.u1; ++u) {
            double x2[E], x3[E], gg[E];
            float d[E];
            bool pos[E];
            const double mean2 = nst.x, rstd2 = nst.y, mean3 = nst.z, rstd3 = nst.w;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                x2[e] = (((double)nxi[e] + (double)na2[e]) - mean2) * rstd2;
                const double t = (double)nz1[e] + fma(x2[e], (double)g2[e], (double)b2[e]);
                pos[e] = t > 0.0;
                x3[e] = ((t < 0.0 ? 0.0 : t) - mean3) * rstd3;
                d[e] = nd[e];
                gg[e] = (double)d[e] * (double)g3[e];
            }
            if (u + 1 < R.u1) fetch(u + 1);
            ln_input_grad<H>(gg, x3, rstd3);               // cotangent of ReLU's output
            const long long row = C::RPU * u + R.sub;
            const bool ok = row < A.nrows;
            if (ok) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    add_to(acc[2][e], (double)d[e] * x3[e]);
                    add_to(acc[3][e], (double)d[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                gg[e] = pos[e] ? gg[e] : 0.0;              // of t = z1 + LN2(.): dz1, and LN2's output cotangent
                x3[e] = gg[e] * (double)g2[e];             // x3 is free: the cotangent through LN2's affine
            }
            if (ok) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    add_to(acc[0][e], gg[e] * x2[e]);
                    add_to(acc[1][e], gg[e]);
                }
                if (A.dz1) store_row<H>(A.dz1 + row * H, R.lr, gg);
            }
            ln_input_grad<H>(x3, x2, rstd2);               // of s = xi + a2
            if (ok && A.ds) store_row<H>(A.ds + row * H, R.lr, x3);
        }
    }
    if (A.part) write_partial<H, 4>(acc, R, A.part);
}

// ---------------------------------------------------------------------------------------------------- finish
// out[v][c] = sum over the workgroups' partials part[p][v][c], p ascending.  A workgroup owns FIN_COLS consecutive
// entries of the flattened (v, c); all its threads stage FIN_ROWS partials at a time in LDS, the first wavefront adds
// them in order into an fp64 accumulator.
struct FinArgs {
    const float *part;
    float *out[NVEC];
    int np, nvec, hdim;
};

__global__ __launch_bounds__(FIN_WG) void deq_finish_kernel(FinArgs A)
{
    __shared__ float sm[FIN_ROWS][FIN_COLS];
    const int c = threadIdx.x & (FIN_COLS - 1), r0 = threadIdx.x / FIN_COLS;
    const int fc = blockIdx.x * FIN_COLS + c, ncols = A.nvec * A.hdim;
    const long long stride = (long long)NVEC * A.hdim;
    double s = 0.0;           // fp64: the sum of up to MAX_WG partials is then the correctly rounded one for any order
    for (int p0 = 0; p0 < A.np; p0 += FIN_ROWS) {
        // clamped addresses and a select, not a branch per load: the loads of a chunk are in flight together
        constexpr int PER = FIN_ROWS * FIN_COLS / FIN_WG;
        float v[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int p = p0 + r0 + i * (FIN_WG / FIN_COLS);
            v[i] = A.part[(p < A.np ? p : A.np - 1) * stride + (fc < ncols ? fc : ncols - 1)];
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = r0 + i * (FIN_WG / FIN_COLS);
            sm[r][c] = (p0 + r < A.np && fc < ncols) ? v[i] : 0.0f;
        }
        __syncthreads();
        if (r0 == 0) {
            // the rows past np are zeros: a fixed trip count lets the LDS reads run ahead of the dependent adds
#pragma unroll 16
            for (int r = 0; r < FIN_ROWS; ++r) s += (double)sm[r][c];
        }
        __syncthreads();
    }
    if (r0 == 0 && fc < ncols) {
        float *o = A.out[fc / A.hdim];
        if (o) o[fc % A.hdim] = (float)s;
    }
}

static int finish(const float *part, int np, int nvec, int hdim, float *o0, float *o1, float *o2, float *o3, void *stream)
{
    FinArgs F;
    F.part = part; F.np = np; F.nvec = nvec; F.hdim = hdim;
    F.out[0] = o0; F.out[1] = o1; F.out[2] = o2; F.out[3] = o3;
    DQP_LAUNCH(deq_finish_kernel, dim3((nvec * hdim + FIN_COLS - 1) / FIN_COLS), dim3(FIN_WG), 0, (hipStream_t)stream, F);
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}

// DQP_ERR_BAD_ARG / DQP_ERR_TOO_LARGE / 1 (nrows == 0: nothing to do) / DQP_OK, in the header's order
static int check_dims(const dqp_deq_dims *d)
{
    if (!d || d->nrows < 0) return DQP_ERR_BAD_ARG;
    if (!hdim_ok(d->hdim)) return DQP_ERR_TOO_LARGE;
    return d->nrows == 0 ? 1 : DQP_OK;
}

static bool aligned16(std::initializer_list<const void *> ps)
{
    for (const void *p : ps)
        if ((uintptr_t)p & 15) return false;
    return true;
}

#define DEQ_DISPATCH(HDIM, CALL)                                                                                     \
    switch (HDIM) {                                                                                                  \
    case 32: { constexpr int H = 32; CALL; } break;                                                                  \
    case 64: { constexpr int H = 64; CALL; } break;                                                                  \
    case 128: { constexpr int H = 128; CALL; } break;                                                                \
    case 256: { constexpr int H = 256; CALL; } break;                                                                \
    default: { constexpr int H = 512; CALL; } break;                                                                 \
    }

}  // namespace deq
}  // namespace dqp

extern "C" {

__attribute__((visibility("default"))) int dqp_deq_supported(const dqp_deq_dims *dims)
{
    return dims && dims->nrows >= 0 && dqp::deq::hdim_ok(dims->hdim);
}

__attribute__((visibility("default"))) size_t dqp_deq_partial_bytes(const dqp_deq_dims *dims)
{
    if (!dqp_deq_supported(dims)) return 0;
    return (size_t)dqp::deq::partition(dims->nrows, dims->hdim).nwg * dqp::deq::NVEC * dims->hdim * sizeof(float);
}

__attribute__((visibility("default"))) int
dqp_deq_ln_forward(const dqp_deq_dims *dims, const float *a, const float *gamma, const float *beta, double eps,
                   int32_t relu, float *y, float *stats, void *stream)
{
    using namespace dqp::deq;
    const int rc = check_dims(dims);
    if (rc != DQP_OK) return rc < 0 ? rc : DQP_OK;
    if (!a || !gamma || !beta || !y || !stats || !aligned16({a, gamma, beta, y, stats})) return DQP_ERR_BAD_ARG;
    const Part p = partition(dims->nrows, dims->hdim, MAX_WG_FWD);
    DEQ_DISPATCH(dims->hdim, DQP_LAUNCH(deq_ln_forward_kernel<H>, dim3(p.nwg), dim3(WG), 0, (hipStream_t)stream, a, gamma,
                                        beta, eps, (int)(relu != 0), y, stats, dims->nrows, p.units, p.rpw));
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}

__attribute__((visibility("default"))) int
dqp_deq_ln_backward(const dqp_deq_dims *dims, const float *a, const float *gamma, const float *stats, int32_t relu,
                    const float *dy, float *da, float *dgamma, float *dbeta, float *partial, void *stream)
{
    using namespace dqp::deq;
    const int rc = check_dims(dims);
    if (rc != DQP_OK) return rc < 0 ? rc : DQP_OK;
    const bool sums = dgamma || dbeta;
    if (!a || !gamma || !stats || !dy || (sums && !partial) || !aligned16({a, gamma, stats, dy, da, partial}))
        return DQP_ERR_BAD_ARG;
    if (!da && !sums) return DQP_OK;
    const Part p = partition(dims->nrows, dims->hdim);
    float *part = sums ? partial : nullptr;
    DEQ_DISPATCH(dims->hdim, DQP_LAUNCH(deq_ln_backward_kernel<H>, dim3(p.nwg), dim3(WG), 0, (hipStream_t)stream, a, gamma,
                                        stats, (int)(relu != 0), dy, da, part, dims->nrows, p.units, p.rpw));
    if (hipGetLastError() != hipSuccess) return DQP_ERR_LAUNCH;
    return sums ? finish(part, p.nwg, 2, dims->hdim, dgamma, dbeta, nullptr, nullptr, stream) : DQP_OK;
}

__attribute__((visibility("default"))) int
dqp_deq_res_forward(const dqp_deq_dims *dims, const float *xi, const float *a2, const float *z1, const float *gamma2,
                    const float *beta2, const float *gamma3, const float *beta3, double eps2, double eps3, float *z2,
                    float *stats, void *stream)
{
    using namespace dqp::deq;
    const int rc = check_dims(dims);
    if (rc != DQP_OK) return rc < 0 ? rc : DQP_OK;
    if (!xi || !a2 || !z1 || !gamma2 || !beta2 || !gamma3 || !beta3 || !z2 || !stats ||
        !aligned16({xi, a2, z1, gamma2, beta2, gamma3, beta3, z2, stats}))
        return DQP_ERR_BAD_ARG;
    const Part p = partition(dims->nrows, dims->hdim, MAX_WG_FWD);
    ResArgs A = {};
    A.xi = xi; A.a2 = a2; A.z1 = z1; A.gamma2 = gamma2; A.beta2 = beta2; A.gamma3 = gamma3; A.beta3 = beta3;
    A.z2 = z2; A.stats = stats; A.eps2 = eps2; A.eps3 = eps3;
    A.nrows = dims->nrows; A.units = p.units; A.rpw = p.rpw;
    DEQ_DISPATCH(dims->hdim, DQP_LAUNCH(deq_res_forward_kernel<H>, dim3(p.nwg), dim3(WG), 0, (hipStream_t)stream, A));
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}

__attribute__((visibility("default"))) int
dqp_deq_res_backward(const dqp_deq_dims *dims, const float *xi, const float *a2, const float *z1, const float *gamma2,
                     const float *beta2, const float *gamma3, const float *stats, const float *dz2, float *ds, float *dz1,
                     float *dgamma2, float *dbeta2, float *dgamma3, float *dbeta3, float *partial, void *stream)
{
    using namespace dqp::deq;
    const int rc = check_dims(dims);
    if (rc != DQP_OK) return rc < 0 ? rc : DQP_OK;
    const bool sums = dgamma2 || dbeta2 || dgamma3 || dbeta3;
    if (!xi || !a2 || !z1 || !gamma2 || !beta2 || !gamma3 || !stats || !dz2 || (sums && !partial) ||
        !aligned16({xi, a2, z1, gamma2, beta2, gamma3, stats, dz2, ds, dz1, partial}))
        return DQP_ERR_BAD_ARG;
    if (!ds && !dz1 && !sums) return DQP_OK;
    const Part p = partition(dims->nrows, dims->hdim);
    ResArgs A = {};
    A.xi = xi; A.a2 = a2; A.z1 = z1; A.gamma2 = gamma2; A.beta2 = beta2; A.gamma3 = gamma3; A.stats_in = stats;
    A.dz2 = dz2; A.ds = ds; A.dz1 = dz1; A.part = sums ? partial : nullptr;
    A.nrows = dims->nrows; A.units = p.units; A.rpw = p.rpw;
    DEQ_DISPATCH(dims->hdim, DQP_LAUNCH(deq_res_backward_kernel<H>, dim3(p.nwg), dim3(WG), 0, (hipStream_t)stream, A));
    if (hipGetLastError() != hipSuccess) return DQP_ERR_LAUNCH;
    return sums ? finish(A.part, p.nwg, 4, dims->hdim, dgamma2, dbeta2, dgamma3, dbeta3, stream) : DQP_OK;
}

}  // extern "C"
