// dqp_al.hip -- Newton step of the augmented-Lagrangian MPC solver.
//
// Replaces, per Newton step of qpth/al_utils.py NewtonAL.forward (al_utils.py:403-427):
//   merit_hess = diag(Q) + rho * Jc^T Jc            (al_utils.py:96-102,176-178: a bmm per step)
//   U, info    = torch.linalg.cholesky_ex(merit_hess)
//   update     = -torch.cholesky_solve(grad, U)
// and, in NewtonAL.backward (al_utils.py:465-482),  inp_grad = -cholesky_solve(x_grad, U).
//
// One problem per 256-thread workgroup (4 wavefronts); the nz x nz Hessian lives in LDS
// (nz <= 128 -> <= 132 KB).  Jc^T Jc is the one real GEMM on this path (M = N = nz, K = ncon,
// e.g. 100 x 100 x 120 for cartpole T=20), so it runs on the fp64 matrix cores:
// v_mfma_f64_16x16x4_f64 tiles, lower-triangular tile pairs dealt round-robin to the 4 waves;
// a lane's A and B operands are both plain coalesced reads of one row segment of Jc.
// Jc is staged through LDS once (coalesced HBM reads); the factorisation (square-root-free,
// H = M D M^T) keeps the matrix 16-cyclic in the registers of a 16x16 thread grid and only
// passes the pivot column through LDS, one barrier per step; the two triangular solves run on
// one wavefront with the vector in registers; L = M sqrt(D) is written out (zero upper part,
// like torch) for backward.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/dqp.h"
#include "dqp_r16_prims.h"
#include "dqp_dyn_models.h"   // row_sum (DPP row reduction)
#include "dqp_al_bounds.h"
#include "dqp_al_banded.h"

#ifdef DQP_STAMPS
namespace dqp { extern unsigned long long *g_debug_stamps; }
#endif

namespace {

using namespace dqp;        // the bound families (dqp_al_bounds.h), the host layer (dqp_al_host.h)

typedef double double4_t __attribute__((ext_vector_type(4)));

struct AlP {
    const double *Jc, *Qd, *rho, *grad, *Lin, *rhs;
    double *update, *L, *out;
    int32_t *info;
    int B, nz, ncon, ld, chunk_rows, flag_off;
    unsigned long long *stamps;   // diagnostic (only read with -DDQP_STAMPS; tools/stamps_al.py)
};

#ifdef DQP_STAMPS
#define AL_STAMP(i) do { if (P.stamps && threadIdx.x == 0) P.stamps[blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define AL_STAMP(i) do { } while (0)
#endif

__device__ __forceinline__ double bcast64(double v, int src)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, src);
    hi = __builtin_amdgcn_readlane(hi, src);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double rcp_nr(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    return fma(fma(-d, r, 1.0), r, r);
}

// x <- (M D M^T)^-1 b  (UNIT: LDS holds the unit-lower M below the diagonal and sqrt(d) on it) or
// x <- (L L^T)^-1 b    (!UNIT: LDS holds the Cholesky factor), on ONE wavefront, no barriers.
// Element i of the vector lives on lane i & 63, slot i >> 6 (nz <= 128).  Columns are fetched
// eight steps ahead of the substitution chain, so a step costs one readlane pair and one FMA.
template <bool UNIT, bool FORWARD = true>
__device__ __forceinline__ void wave_solve(const double *H, int ld, int nz, int zidx, double (&b)[2], int lane)
{
    double dg[2], rdg[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = lane + 64 * s;
        dg[s] = i < nz ? H[i * ld + i] : 1.0;
        rdg[s] = 1.0 / dg[s];
    }
    // branch-free: a masked entry reads the zero word the caller keeps at H[zidx]
    constexpr int G = 8;
    double mc[G][2], mn[G][2];
    auto load_fwd = [&](double (&m)[G][2], int k0) {     // column k = k0 + u, rows i > k
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int k = k0 + u;
            m[u][0] = H[(lane > k && lane < nz) ? lane * ld + k : zidx];
            m[u][1] = H[(lane + 64 > k && lane + 64 < nz) ? (lane + 64) * ld + k : zidx];
        }
    };
    auto load_bwd = [&](double (&m)[G][2], int k0) {     // row k = k0 - u, columns i < k
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int k = k0 - u;
            m[u][0] = H[(lane < k && k < nz) ? k * ld + lane : zidx];
            m[u][1] = H[(lane + 64 < k && k < nz) ? k * ld + lane + 64 : zidx];
        }
    };
    // eight chained substitution steps on columns/rows k0 + sgn*u, pivots in slot S (k >> 6 == S)
#define DQP_AL_CHAIN(S, SGN)                                                              \
    _Pragma("unroll") for (int u = 0; u < G; ++u) {                                       \
        const int k = k0 + (SGN) * u;                                                     \
        double wk = bcast64(b[S], k & 63);                                                \
        if (!UNIT) {                                                                      \
            wk *= bcast64(rdg[S], k & 63);                                                \
            b[S] = (lane + 64 * (S) == k) ? wk : b[S];                                    \
        }                                                                                 \
        b[0] = fma(-mc[u][0], wk, b[0]);                                                  \
        b[1] = fma(-mc[u][1], wk, b[1]);                                                  \
    }
#define DQP_AL_ROTATE() _Pragma("unroll") for (int u = 0; u < G; ++u) { mc[u][0] = mn[u][0]; mc[u][1] = mn[u][1]; }
    const int nzg = ((nz + G - 1) / G) * G, lo_end = min(nzg, 64);
    if (FORWARD) {
        load_fwd(mn, 0);
        for (int k0 = 0; k0 < lo_end; k0 += G) { DQP_AL_ROTATE(); load_fwd(mn, k0 + G); DQP_AL_CHAIN(0, 1); }
        for (int k0 = 64; k0 < nzg; k0 += G) { DQP_AL_ROTATE(); load_fwd(mn, k0 + G); DQP_AL_CHAIN(1, 1); }
    }
    if (UNIT) { b[0] *= rdg[0] * rdg[0]; b[1] *= rdg[1] * rdg[1]; }   // D^-1, d = (sqrt d)^2
    load_bwd(mn, nzg - 1);
    for (int k0 = nzg - 1; k0 >= 64; k0 -= G) { DQP_AL_ROTATE(); load_bwd(mn, k0 - G); DQP_AL_CHAIN(1, -1); }
    for (int k0 = lo_end - 1; k0 >= 0; k0 -= G) { DQP_AL_ROTATE(); load_bwd(mn, k0 - G); DQP_AL_CHAIN(0, -1); }
#undef DQP_AL_CHAIN
#undef DQP_AL_ROTATE
}

#define TRI(a, b) ((a) * ((a) + 1) / 2 + (b))

// lower-triangular 16x16 tiles in row-major order: tile t -> (ti, tj), tj <= ti
__host__ __device__ constexpr int tile_row(int t) { int ti = 0; while ((ti + 1) * (ti + 2) / 2 <= t) ++ti; return ti; }
__host__ __device__ constexpr int tile_col(int t) { return t - tile_row(t) * (tile_row(t) + 1) / 2; }

// K-loop over one staged chunk for wave W: tiles W, W+4, ... accumulate in registers; the NT
// column-block operands of a 4-row K step are fetched one step ahead of the MFMAs using them.
template <int NT, int W, int NS>
__device__ __forceinline__ void mfma_chunk(const double *Hs, int rows4, int kq, int l15, double4_t (&acc)[NS])
{
    constexpr int NZP = 16 * NT, NTILES = NT * (NT + 1) / 2;
    const double *jr = Hs + kq * NZP + l15;
    double opc[NT], opn[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) opn[c] = jr[16 * c];
    for (int c0 = 0; c0 < rows4; c0 += 4) {
#pragma unroll
        for (int c = 0; c < NT; ++c) opc[c] = opn[c];
        const double *jn = jr + (c0 + 4 < rows4 ? c0 + 4 : c0) * NZP;
#pragma unroll
        for (int c = 0; c < NT; ++c) opn[c] = jn[16 * c];
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (W + 4 * s < NTILES)
                acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(opc[tile_row(W + 4 * s)], opc[tile_col(W + 4 * s)],
                                                              acc[s], 0, 0, 0);
    }
}

// C/D layout of the f64 16x16x4 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
template <int NT, int W, int NS>
__device__ __forceinline__ void store_tiles(double *H, int ld, int nz, double rho, int kq, int l15,
                                            const double4_t (&acc)[NS])
{
    constexpr int NTILES = NT * (NT + 1) / 2;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (W + 4 * s >= NTILES) continue;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int row = 16 * tile_row(W + 4 * s) + kq + 4 * rg, col = 16 * tile_col(W + 4 * s) + l15;
            if (row < nz && col <= row) H[row * ld + col] = rho * acc[s][rg];
        }
    }
}

// One problem per 256-thread workgroup; NT = ceil(nz / 16) is a template parameter so every
// register-array loop (MFMA tiles, the 16-cyclic factor) is fully unrolled at its true size.
template <int NT>
__global__ __launch_bounds__(256) void al_newton_kernel(AlP P)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int NZP = 16 * NT, NS = (NT * (NT + 1) / 2 + 3) / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;
    const int nz = P.nz, ncon = P.ncon, ld = P.ld;
    const long long prob = blockIdx.x;
    double *H = sm;                                   // nz x ld
    if (tid == 0) sm[P.flag_off + 1] = 0.0;           // the zero word masked solve loads read
    AL_STAMP(0);
    // diagonal of the cost Hessian for the 16-cyclic owner of (i, i): threads with ty == tx
    double qd[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) qd[a] = (ty == tx && ty + 16 * a < nz) ? P.Qd[prob * nz + ty + 16 * a] : 0.0;

    // ---- H = diag(Qd) + rho * Jc^T Jc ---------------------------------------------------------
    // Jc is staged through LDS (the not-yet-written H region) in zero-padded chunks of CH rows,
    // read from HBM exactly once with coalesced loads; each wave owns up to 9 lower-triangular
    // 16x16 output tiles whose fp64 MFMA accumulators stay in registers across the whole K loop.
    const double *J = P.Jc + prob * (long long)ncon * nz;
    const double rho = P.rho[prob];
    const int CH = P.chunk_rows;
    double4_t acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int l15 = lane & 15, kq = lane >> 4;
    for (int cb = 0; cb < ncon; cb += CH) {
        const int rows = min(CH, ncon - cb), rows4 = (rows + 3) & ~3;
        __syncthreads();
        // wave w stages rows w, w+4, ...; a lane covers columns lane and lane+64; 16 loads in flight
        for (int r0 = wave; r0 < rows4; r0 += 32) {
            double v[8][2];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int rr = r0 + 4 * u, cc = lane + 64 * s;
                    v[u][s] = (rr < rows && cc < nz) ? J[(long long)(cb + rr) * nz + cc] : 0.0;
                }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int rr = r0 + 4 * u, cc = lane + 64 * s;
                    if (rr < rows4 && cc < NZP) H[rr * NZP + cc] = v[u][s];
                }
        }
        __syncthreads();
        switch (wave) {
        case 0: mfma_chunk<NT, 0, NS>(H, rows4, kq, l15, acc); break;
        case 1: mfma_chunk<NT, 1, NS>(H, rows4, kq, l15, acc); break;
        case 2: mfma_chunk<NT, 2, NS>(H, rows4, kq, l15, acc); break;
        default: mfma_chunk<NT, 3, NS>(H, rows4, kq, l15, acc); break;
        }
    }
    __syncthreads();
    AL_STAMP(1);
    switch (wave) {
    case 0: store_tiles<NT, 0, NS>(H, ld, nz, rho, kq, l15, acc); break;
    case 1: store_tiles<NT, 1, NS>(H, ld, nz, rho, kq, l15, acc); break;
    case 2: store_tiles<NT, 2, NS>(H, ld, nz, rho, kq, l15, acc); break;
    default: store_tiles<NT, 3, NS>(H, ld, nz, rho, kq, l15, acc); break;
    }
    __syncthreads();
    AL_STAMP(2);

    // ---- factorisation in registers --------------------------------------------------------------
    // Thread (ty, tx) of the 16 x 16 grid owns the 16-cyclic elements H[ty + 16a][tx + 16b],
    // b <= a.  Step k: every thread picks up the pivot and its <= NT row and <= NT column
    // operands from the published column k (double-buffered in LDS, one barrier per step) and
    // applies the rank-1 update to its registers -- next pivot column first, so its owners
    // publish it before the bulk of the update (look-ahead).  Columns stay unscaled (c_ik) with
    // the pivot d_k on the diagonal: H = M D M^T, M_ik = c_ik / d_k.
    const bool fused = nz < 16 * NT;       // row nz exists in the 16-cyclic grid (nz not a multiple of 16)
    double hr[NT * (NT + 1) / 2];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            const int row = ty + 16 * a, col = tx + 16 * b;
            hr[TRI(a, b)] = (row < nz && col <= row) ? H[row * ld + col] : 0.0;
            if (a == b) hr[TRI(a, b)] += qd[a];
            // augmented row nz = rhs^T: the elimination then carries out the forward substitution
            // M w = -grad for free (row nz ends up holding w), so wave 0 only has the backward sweep
            if (fused && row == nz && col < nz) hr[TRI(a, b)] = -P.grad[prob * nz + col];
        }
    __syncthreads();
    double *colbuf = sm;                 // 2 x 128 doubles, aliases the (now unused) H region
    double dcol[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) dcol[b] = 1.0;
    int firstbad = 0;                    // torch.linalg.cholesky_ex: info = first non-positive minor
    if (tx == 0) {
#pragma unroll
        for (int a = 0; a < NT; ++a) colbuf[ty + 16 * a] = hr[TRI(a, 0)];
    }
#pragma unroll
    for (int kb = 0; kb < NT; ++kb) {
        const int kend = min(16, nz - 16 * kb);
        for (int kr = 0; kr < kend; ++kr) {
            const int k = 16 * kb + kr;
            const double *cbuf = colbuf + (k & 1) * 128;
            double *nbuf = colbuf + ((k + 1) & 1) * 128;
            __syncthreads();
            const double d = cbuf[k];
            double r[NT], c[NT];
#pragma unroll
            for (int a = kb; a < NT; ++a) { r[a] = cbuf[ty + 16 * a]; c[a] = cbuf[tx + 16 * a]; }
            firstbad = (firstbad == 0 && !(d > 0.0)) ? k + 1 : firstbad;
            const double nrd = -rcp_nr(d);
            if (tx == kr) dcol[kb] = d;
            r[kb] = ty > kr ? r[kb] : 0.0;
            c[kb] = tx > kr ? c[kb] : 0.0;
#pragma unroll
            for (int a = kb; a < NT; ++a) r[a] *= nrd;
#pragma unroll
            for (int a = kb; a < NT; ++a) hr[TRI(a, kb)] = fma(r[a], c[kb], hr[TRI(a, kb)]);
            if (kr < 15) {
                if (tx == kr + 1) {
#pragma unroll
                    for (int a = kb; a < NT; ++a) nbuf[ty + 16 * a] = hr[TRI(a, kb)];
                }
            }
            if (kb + 1 < NT) {
#pragma unroll
                for (int a = kb + 1; a < NT; ++a) hr[TRI(a, kb + 1)] = fma(r[a], c[kb + 1], hr[TRI(a, kb + 1)]);
                if (kr == 15) {
                    if (tx == 0) {
#pragma unroll
                        for (int a = kb + 1; a < NT; ++a) nbuf[ty + 16 * a] = hr[TRI(a, kb + 1)];
                    }
                }
            }
#pragma unroll
            for (int b = kb + 2; b < NT; ++b)
#pragma unroll
                for (int a = b; a < NT; ++a) hr[TRI(a, b)] = fma(r[a], c[b], hr[TRI(a, b)]);
        }
    }
    __syncthreads();
    AL_STAMP(3);
    // LDS <- unit-lower M (strictly below the diagonal) and sqrt(d) on the diagonal
    {
        double rdc[NT], sdc[NT];
#pragma unroll
        for (int b = 0; b < NT; ++b) { rdc[b] = 1.0 / dcol[b]; sdc[b] = sqrt(dcol[b]); }
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                const int row = ty + 16 * a, col = tx + 16 * b;
                if (row < nz && col <= row) H[row * ld + col] = col == row ? sdc[b] : hr[TRI(a, b)] * rdc[b];
            }
    }
    double *wvec = sm + P.flag_off + 2;    // row nz of the elimination = w (fused forward sweep)
    if (fused && ty == (nz & 15)) {
#pragma unroll
        for (int b = 0; b < NT; ++b)
            if ((nz >> 4) >= b && tx + 16 * b < nz) {
#pragma unroll
                for (int a = 0; a < NT; ++a)
                    if (a >= b && a == (nz >> 4)) wvec[tx + 16 * b] = hr[TRI(a, b)];
            }
    }
    __syncthreads();
    const int info = firstbad;
    AL_STAMP(4);

    // ---- wave 0 solves while waves 1-3 write the factor out -------------------------------------
    if (wave == 0) {
        double b[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = lane + 64 * s;
            b[s] = i < nz ? (fused ? wvec[i] : -P.grad[prob * nz + i]) : 0.0;
        }
        if (info == 0) {
            if (fused) wave_solve<true, false>(H, ld, nz, P.flag_off + 1, b, lane);
            else wave_solve<true, true>(H, ld, nz, P.flag_off + 1, b, lane);
        }
        const double nanv = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (lane + 64 * s < nz) P.update[prob * nz + lane + 64 * s] = info == 0 ? b[s] : nanv;
        if (lane == 0 && P.info) P.info[prob] = info;
        AL_STAMP(5);
    } else if (P.L) {                     // Cholesky factor L_ik = M_ik sqrt(d_k), zero upper part
        double *Lo = P.L + prob * (long long)nz * nz;
        double sd[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) sd[s] = H[min(lane + 64 * s, nz - 1) * (ld + 1)];
        for (int i = wave - 1; i < nz; i += 3)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int j = lane + 64 * s;
                if (j < nz) Lo[i * nz + j] = j < i ? H[i * ld + j] * sd[s] : (j == i ? sd[s] : 0.0);
            }
    }
}

// out = -(L L^T)^-1 rhs   (NewtonAL.backward, al_utils.py:477-480); block loads L, wave 0 solves
__global__ __launch_bounds__(256) void al_chol_solve_kernel(AlP P)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nz = P.nz, ld = P.ld;
    const long long prob = blockIdx.x;
    double *H = sm;
    const double *Li = P.Lin + prob * (long long)nz * nz;
    if (tid == 0) sm[P.flag_off + 1] = 0.0;
    for (int i = wave; i < nz; i += 4)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int j = lane + 64 * s;
            if (j <= i) H[i * ld + j] = Li[i * nz + j];
        }
    __syncthreads();
    if (tid >= 64) return;
    double b[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) b[s] = (lane + 64 * s < nz) ? -P.rhs[prob * nz + lane + 64 * s] : 0.0;
    wave_solve<false>(H, ld, nz, P.flag_off + 1, b, lane);
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if (lane + 64 * s < nz) P.out[prob * nz + lane + 64 * s] = b[s];
}

int fill(const dqp_al_dims *d, AlP &P, size_t &lds)
{
    if (!d || d->nbatch < 0 || d->nz <= 0 || d->ncon < 0) return DQP_ERR_BAD_ARG;
    if (d->nz > 128) return DQP_ERR_TOO_LARGE;
    P.B = d->nbatch; P.nz = d->nz; P.ncon = d->ncon;
#ifdef DQP_STAMPS
    P.stamps = dqp::g_debug_stamps;
#else
    P.stamps = nullptr;
#endif
    // LDS: the nz x nz factor (ld = nz | 1: 80,800 B at nz = 100, so two problems share a CU); the
    // same region first stages Jc in chunks of `chunk_rows` zero-padded rows of 16*ceil(nz/16).
    P.ld = d->nz | 1;                 // odd leading dimension: conflict-free column reads
    const int nzp = (d->nz + 15) & ~15;
    size_t hd = (size_t)d->nz * P.ld;
    if (hd < (size_t)4 * nzp) hd = (size_t)4 * nzp;
    if (hd < 256) hd = 256;           // the double-buffered pivot column of the factorisation
    P.chunk_rows = (int)((hd / nzp) & ~(size_t)3);
    P.flag_off = (int)hd;
    lds = (hd + 2 + 128) * sizeof(double);   // + zero word, + the fused forward-sweep result
    if (lds > 160 * 1024 - 64) return DQP_ERR_TOO_LARGE;
    return DQP_OK;
}

// ------------------------------------------------------------------------------------------
// Constraint Jacobian fill + J^T (lam + rho res_c)  (al_utils.py:62-102,162-318)
struct AsmP {
    const double *Jx, *Ju, *lam, *resc, *rho;
    double *Jc, *gterm;
    int B, n, m, T;
    const double *Qd, *q, *xu;       // optional: gterm += Qd * xu + q  (the full merit gradient)
};

// value of J[row][col] for one problem; act: inequality rows count only when active
__device__ __forceinline__ double jac_entry(const AsmP &P, const double *Jx, const double *Ju,
                                            const double *resc, int row, int col, bool clamp)
{
    const int n = P.n, m = P.m, T = P.T, nt = n + m, neq = AlRows{n, m, T, false}.neq();
    const int tc = col / nt, jc = col - tc * nt;
    if (row < neq) {
        const int t = row / n, r = row - t * n;
        if (t == T - 1) return (tc == 0 && jc == r) ? 1.0 : 0.0;                 // x_0 - x0
        if (tc == t) return jc < n ? -Jx[(t * n + r) * n + jc] : -Ju[(t * n + r) * m + (jc - n)];
        return (tc == t + 1 && jc == r) ? 1.0 : 0.0;                            // + x_{t+1}
    }
    const int q = row - neq, t = q / (2 * m), k = q - t * 2 * m;                 // [upper (m), lower (m)]
    if (clamp && !(resc[row] > 0.0)) return 0.0;
    if (tc != t || jc < n) return 0.0;
    const int i = jc - n;
    return k < m ? (i == k ? 1.0 : 0.0) : (i == k - m ? -1.0 : 0.0);
}

__global__ __launch_bounds__(256) void al_assemble_kernel(AsmP P)
{
    const int n = P.n, m = P.m, T = P.T, nt = n + m, nz = T * nt;
    const AlRows R = {n, m, T, false};
    const int ncon = R.ncon();
    const long long b = blockIdx.x;
    const double *Jx = P.Jx + b * (long long)(T - 1) * n * n, *Ju = P.Ju + b * (long long)(T - 1) * n * m;
    const double *resc = P.resc + b * (long long)ncon;
    if (P.Jc) {
        double *Jc = P.Jc + b * (long long)ncon * nz;
        for (int e = threadIdx.x; e < ncon * nz; e += 256) {
            const int row = e / nz, col = e - row * nz;
            Jc[e] = jac_entry(P, Jx, Ju, resc, row, col, true);
        }
    }
    if (P.gterm) {
        // column sums with mu = lam + rho res_c (for an inactive inequality res_c = 0, so the
        // clamped and the full Jacobian give the same term): only the structurally non-zero rows
        const double *lam = P.lam + b * (long long)ncon;
        const double rho = P.rho[b];
        for (int col = threadIdx.x; col < nz; col += 256) {
            const int t = col / nt, j = col - t * nt;
            auto mu = [&](int row) { return lam[row] + rho * resc[row]; };
            double acc = 0.0;
            if (t < T - 1)
                for (int r = 0; r < n; ++r) acc += jac_entry(P, Jx, Ju, resc, R.eq(t) + r, col, false) * mu(R.eq(t) + r);
            if (j < n) {
                if (t >= 1) acc += mu(R.eq(t - 1) + j);
                if (t == 0) acc += mu(R.eq(T - 1) + j);
            } else {
                const int i = j - n;
                acc += mu(R.ctrl(t) + i) - mu(R.ctrl(t) + m + i);
            }
            if (P.Qd) acc += P.Qd[b * (long long)nz + col] * P.xu[b * (long long)nz + col] + P.q[b * (long long)nz + col];
            P.gterm[b * (long long)nz + col] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------
// merit function of a batch of candidate trajectories (al_utils.py:37-59); 16 lanes per
// (candidate, problem): lane j of the group sweeps knots j, j+16, ... and the partial sums are
// combined with DPP row reductions
struct MeritP {
    const double *xu, *xn, *x0, *Qd, *q, *lam, *rho, *ul, *uu;
    double *merit;
    int B, n, m, T, ncand;
    long long bsb, bst;         // bound layout (dqp_al_bounds.h), read with SB only
    const double *xlo, *xhi;    // state box (dqp_al_merit_xbounds), read with XB only: lower / upper of (b, t, j) at
    long long xsb, xst;         // [b xsb + t xst + j]; lam then carries the state rows, knot 0's included
};

// SB: per-sample / per-knot bounds at [b bsb + t bst + i], !SB: the n_ctrl-vector; XB: + the state rows
template <bool SB, bool XB> __device__ __forceinline__ void merit_sweep(const MeritP &P)
{
    static_assert(SB || !XB, "with a state box both boxes are read through their strides");
    const int n = P.n, m = P.m, T = P.T, nt = n + m;
    const AlRows R = {n, m, T, XB};
    const long long item = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);      // (cand, problem)
    const int r = threadIdx.x & 15;
    const long long total = (long long)P.ncand * P.B;
    const long long it = item < total ? item : total - 1;
    const long long b = it % P.B;
    const double *xu = P.xu + it * (long long)T * nt, *xn = P.xn + it * (long long)(T - 1) * n;
    const double *Qd = P.Qd + b * (long long)T * nt, *q = P.q + b * (long long)T * nt;
    const double *lam = P.lam + b * (long long)R.ncon(), *x0 = P.x0 + b * (long long)n;
    const double rho = P.rho[b];
    // with a state box the sample's rows of both boxes are taken once, in front of the sweep (the form that kernel was timed in)
    const double *ul = P.ul + (XB ? b * P.bsb : 0), *uu = P.uu + (XB ? b * P.bsb : 0);
    [[maybe_unused]] const double *xlo = XB ? P.xlo + b * P.xsb : nullptr, *xhi = XB ? P.xhi + b * P.xsb : nullptr;
    double acc = 0.0;
    for (int t = r; t < T; t += 16) {
        const double *z = xu + t * nt;
        for (int j = 0; j < nt; ++j) acc += al_cost_term(Qd[t * nt + j], q[t * nt + j], z[j]);
        for (int j = 0; j < n; ++j) {                       // equality row block of knot t
            const double res = t < T - 1 ? xu[(t + 1) * nt + j] - xn[t * n + j] : xu[j] - x0[j];
            acc += al_eq_term(rho, lam[R.eq(t) + j], res);
        }
        for (int i = 0; i < m; ++i) {                       // control rows of knot t
            const int row = R.ctrl(t) + i;
            const long long o = XB ? t * P.bst + i : al_bound_at<SB>(b, t, i, P.bsb, P.bst);
            acc += al_pair_term(rho, lam[row], lam[row + m], z[n + i] - uu[o], ul[o] - z[n + i]);
        }
        if constexpr (XB) {
            for (int j = 0; j < n; ++j) {                   // state rows of knot t
                const int row = R.state(t) + j;
                acc += al_pair_term(rho, lam[row], lam[row + n], z[j] - xhi[t * P.xst + j], xlo[t * P.xst + j] - z[j]);
            }
        }
    }
    acc = dqp::r16::row_sum(acc);
    if (r == 0 && item < total) P.merit[item] = acc;
}
// the entry points, under the names a trace shows: <SB> without a state box, <true, true> with one
template <bool SB> __global__ __launch_bounds__(256) void al_merit_kernel(MeritP P) { merit_sweep<SB, false>(P); }
template <bool SB, bool XB> __global__ __launch_bounds__(256) void al_merit_kernel(MeritP P) { merit_sweep<SB, XB>(P); }

// ------------------------------------------------------------------------------------------
// NewtonAL with a registered device model: the Python glue of al_utils.NewtonAL.forward
// (qpth/al_utils.py:363-456, 503-527) as kernels, so that the four Newton steps of one AL iteration
// are 21 back-to-back launches with no host involvement.
template <class Map>
__device__ __forceinline__ void lin_knot(const double *z, double dt, double *xn, double *Jx, double *Ju)
{
    constexpr int NX = Map::NX, NU = Map::NU, K = NX + NU;
    using S = dqp::dyn::Dual<K>;
    S xa[NX], ua[NU], o[NX];
#pragma unroll
    for (int k = 0; k < NX; ++k) { xa[k] = S(z[k]); xa[k].d[k] = 1.0; }
#pragma unroll
    for (int k = 0; k < NU; ++k) { ua[k] = S(z[NX + k]); ua[k].d[NX + k] = 1.0; }
    Map::template step<S>(xa, ua, dt, o);
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        xn[r] = o[r].v;
#pragma unroll
        for (int c = 0; c < NX; ++c) Jx[r * NX + c] = o[r].d[c];
#pragma unroll
        for (int c = 0; c < NU; ++c) Ju[r * NU + c] = o[r].d[NX + c];
    }
}

struct LinP {
    const double *xu, *x0, *ul, *uu;
    double *Jx, *Ju, *resc;
    double dt;
    int B, n, m, T, dyn;
    long long bsb, bst;         // bound layout (dqp_al_bounds.h), read with SB only
};
constexpr int LIN_NX = 8, LIN_NU = 2;       // the largest knot of the dense form (newton_dense refuses beyond)

// one thread per (problem, knot): dynamics + Jacobians of the knot, its equality rows
// x_{t+1} - f(x_t, u_t) (or x_0 - x0 for the last block) and its clamped box rows
template <bool SB> __global__ __launch_bounds__(256) void al_linearize_kernel(LinP P)
{
    const int n = P.n, m = P.m, T = P.T, nt = n + m;
    const AlRows R = {n, m, T, false};
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)P.B * T) return;
    const long long b = idx / T;
    const int t = (int)(idx - b * T);
    const double *z = P.xu + (b * T + t) * nt;
    double *resc = P.resc + b * R.ncon();
    if (t < T - 1) {
        double *oJx = P.Jx + (b * (T - 1) + t) * n * n, *oJu = P.Ju + (b * (T - 1) + t) * n * m;
        dqp::dyn::visit<int>(P.dyn, 0, [&](auto model) {        // the host has checked the id and that (n, m) are its sizes
            using Map = typename decltype(model)::Map;
            if constexpr (Map::NX <= LIN_NX && Map::NU <= LIN_NU) {
                double xn[Map::NX];
                lin_knot<Map>(z, P.dt, xn, oJx, oJu);
#pragma unroll
                for (int i = 0; i < Map::NX; ++i) resc[R.eq(t) + i] = z[nt + i] - xn[i];
            }
            return 0;
        });
    } else {
        const double *z0 = P.xu + b * T * nt;
        for (int i = 0; i < n; ++i) resc[R.eq(t) + i] = z0[i] - P.x0[b * n + i];
    }
    for (int i = 0; i < m; ++i) {
        const double u = z[n + i];
        const long long o = al_bound_at<SB>(b, t, i, P.bsb, P.bst);
        resc[R.ctrl(t) + i] = fmax(u - P.uu[o], 0.0);
        resc[R.ctrl(t) + m + i] = fmax(P.ul[o] - u, 0.0);
    }
}

struct LsAP {
    const double *xu, *upd, *x0, *Qd, *q, *lam, *rho, *ul, *uu;
    double *merit;
    double dt;
    int B, n, m, T, ncand, dyn;
    // optional: selection folded into the group kernel (argmin, acceptance, update of the iterate;
    // al_utils.py:516-526) when one group sees all candidates of its problem
    double *xu_w, *merit_cur, *status;
    int32_t *fail;
    const int32_t *info;
    long long bsb, bst;         // bound layout (dqp_al_bounds.h), read by the StridedBounds<> instantiations only
    const double *xlo, *xhi;    // state box, read by the BoxBounds<> instantiations only (else NULL); lam then carries
    long long xsb, xst;         // 2 T n more rows
};
// the merit of `ncand` candidates xu + 2^-k upd into `merit` (ncand = 0: of xu itself).  The folded selection (xu_w,
// merit_cur, status, fail, info) is the caller's to set.
LsAP ls_args(const AlProblem &v, const double *xu, const double *upd, double *merit, int ncand)
{
    LsAP P = dqp::boxed_args<LsAP>(v);
    P.xu = xu; P.upd = upd; P.merit = merit; P.dt = v.dt; P.n = v.n; P.m = v.m; P.ncand = ncand; P.dyn = v.model;
    return P;
}

// merit (al_utils.py:37-59) of ncand candidates xu + 2^-k upd per problem (x_0 pinned to x0,
// al_utils.py:515), dynamics evaluated in the kernel; 16 lanes per (candidate, problem).  ncand = 0
// evaluates the current point (step 0) into merit[b].  Knots are processed 16 at a time:
//   phase A  element-wise over the entries of knots c .. c+16, lanes along the contiguous axis
//            (coalesced): z = xu + step upd -> LDS; cost and box-constraint terms of knots c .. c+15
//   phase B  one knot per lane: the model step from the knot in LDS (odd stride: conflict-free),
//            residual against the next knot in LDS, multiplier and penalty terms
template <class Map>
__global__ __launch_bounds__(256) void al_ls_kernel(LsAP P)
{
    constexpr int n = Map::NX, m = Map::NU, nt = n + m, ZS = nt | 1;
    __shared__ double ls_lds[16 * 17 * ZS];
    constexpr bool XB = box_bounds<Map>::value;
    const int T = P.T, neq = AlRows{n, m, T, XB}.neq(), ncon = AlRows{n, m, T, XB}.ncon();
    const int nc = P.ncand > 0 ? P.ncand : 1;
    const int slot = threadIdx.x >> 4, r = threadIdx.x & 15;
    const long long item = (long long)blockIdx.x * 16 + slot;
    const long long total = (long long)nc * P.B;
    const long long it = item < total ? item : total - 1;
    const long long b = it % P.B;
    const int k = (int)(it / P.B);
    const double step = P.ncand > 0 ? al_step(k) : 0.0;
    // ncand = 0: no update exists yet and what lies in its place may be NaN (0 NaN is not 0): step 0 along the iterate itself
    const double *xu = P.xu + b * (long long)T * nt, *up = P.ncand > 0 ? P.upd + b * (long long)T * nt : xu;
    const double *Qd = P.Qd + b * (long long)T * nt, *q = P.q + b * (long long)T * nt;
    const double *lam = P.lam + b * (long long)ncon, *x0 = P.x0 + b * (long long)n;
    const double rho = P.rho[b];
    constexpr bool SB = strided_bounds<Map>::value;
    double *zb = ls_lds + slot * 17 * ZS;
    double acc = 0.0;
    for (int c = 0; c < T; c += 16) {
        const int kend = (c + 17 < T ? c + 17 : T) - c;                  // knots staged this round (<= 17)
#pragma unroll 4
        for (int e = r; e < kend * nt; e += 16) {
            const int tl = e / nt, j = e - tl * nt, t = c + tl, ge = c * nt + e;
            double z = xu[ge] + step * up[ge];
            if (t == 0 && j < n) z = x0[j];
            zb[tl * ZS + j] = z;
            if (tl < 16) {
                acc += al_cost_term(Qd[ge], q[ge], z);
                if (j >= n) {
                    const int i = j - n, row = neq + t * 2 * m + i;
                    double uut, ult;
                    if constexpr (SB) { uut = P.uu[b * P.bsb + t * P.bst + i]; ult = P.ul[b * P.bsb + t * P.bst + i]; }
                    else { uut = P.uu[i]; ult = P.ul[i]; }
                    const double hi = z - uut, lo = ult - z;
                    acc += al_pair_term(rho, lam[row], lam[row + m], hi, lo);
                } else if constexpr (XB) {      // the state rows of the element, into the same accumulator
                    const int row = neq + 2 * T * m + t * 2 * n + j;
                    const double hi = z - P.xhi[b * P.xsb + t * P.xst + j], lo = P.xlo[b * P.xsb + t * P.xst + j] - z;
                    acc += al_pair_term(rho, lam[row], lam[row + n], hi, lo);
                }
            }
        }
        __syncthreads();
        const int t = c + r;
        if (t < T - 1) {
            double z[nt], xn[n];
#pragma unroll
            for (int j = 0; j < nt; ++j) z[j] = zb[r * ZS + j];
            Map::template step<double>(z, z + n, P.dt, xn);
#pragma unroll
            for (int j = 0; j < n; ++j) {
                const double res = zb[(r + 1) * ZS + j] - xn[j];
                acc += al_eq_term(rho, lam[t * n + j], res);
            }
        }
        __syncthreads();
    }
    // (the x_0 rows contribute nothing: x_0 is pinned to x0, their residual is exactly zero)
    acc = dqp::r16::row_sum(acc);
    if (r == 0 && item < total) P.merit[item] = acc;
}

// The same merits with one lane GROUP per problem that walks its candidates itself (T <= 32): the
// problem's xu, upd, Qd, q and multipliers are loaded once into registers instead of once per
// candidate, and the group is as wide as the horizon needs (TPI = 8, 16 or 32 lanes: one knot per lane in
// the model phase -- with 16 lanes per candidate a T = 5 problem used 5 of them).
// sum over a group of TPI lanes (aligned in the wavefront), in every lane of the group: DPP steps inside a 16-lane row
// (a shuffle is a ds_bpermute round trip through the LDS crossbar, ~100 cycles each on the chain of a candidate), one
// shuffle across the two rows of a 32-lane group
template <int TPI> __device__ __forceinline__ double group_sum(double v)
{
    using dqp::r16::dppd;
    if constexpr (TPI >= 16) {
        v = dqp::r16::row_sum(v);
#pragma unroll
        for (int off = 16; off < TPI; off <<= 1) v += __shfl_xor(v, off, 64);
    } else if constexpr (TPI == 8) {
        v += dppd<0x141>(v);        // row_half_mirror: l <-> 7 - l
        v += dppd<0xb1>(v);         // quad_perm [1,0,3,2]
        v += dppd<0x4e>(v);         // quad_perm [2,3,0,1]
    } else {
        static_assert(TPI == 4, "lane groups of 4, 8, 16 or 32");
        v += dppd<0xb1>(v);
        v += dppd<0x4e>(v);
    }
    return v;
}

// A lane group (TPI <= 32 lanes) never spans wavefronts and a wavefront's LDS operations execute in order:
// the group's writes to its own LDS rows only have to be issued before its reads, which a workgroup-scope fence
// (an s_waitcnt, no s_barrier) plus a scheduling barrier guarantees -- the four wavefronts of the block do not
// wait for each other twice per candidate.
__device__ __forceinline__ void group_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

template <class Map, int TPI, int TMAX>
__global__ __launch_bounds__(256, ((TMAX * (Map::NX + Map::NU) + TPI - 1) / TPI >= 12) ? 2 : 1) void al_ls_group_kernel(LsAP P)
{
    constexpr int n = Map::NX, m = Map::NU, nt = n + m, ZS = nt | 1;
    constexpr int EPL = (TMAX * nt + TPI - 1) / TPI;       // elements of the (T, nt) arrays per lane, T <= TMAX
    extern __shared__ double lsg_lds[];
    constexpr bool XB = box_bounds<Map>::value;
    const int T = P.T, nzq = T * nt;
    const AlRows R = {n, m, T, XB};
    // This kernel alone spells its rows out from neq (AlRows of dqp_al_bounds.h has the layout): the quadrotor with a state
    // box sits at 256 registers, and R.ctrl / R.state inside its loops raised its spills
    const int neq = R.neq();
    const int nc = P.ncand > 0 ? P.ncand : 1;
    const int grp = threadIdx.x / TPI, r = threadIdx.x % TPI;
    const long long pb = (long long)blockIdx.x * (256 / TPI) + grp;
    const bool live = pb < P.B;
    const long long b = live ? pb : P.B - 1;
    const double *xu = P.xu + b * (long long)nzq, *up = P.upd + b * (long long)nzq;
    const double *Qd = P.Qd + b * (long long)nzq, *q = P.q + b * (long long)nzq;
    const double *lam = P.lam + b * (long long)R.ncon(), *x0 = P.x0 + b * (long long)n;
    const double rho = P.rho[b];
    double *zb = lsg_lds + (size_t)grp * T * ZS;
    // ---- the problem, once: element e = r + TPI i of the (T, nt) arrays; the box rows (multipliers, bounds) only exist
    // for the T m control elements and are distributed over the lanes on their own (element c = r + TPI i of the (T, m)
    // array, with its own copy of the iterate and the update): eight arrays of EPL doubles per lane were 144 - 256
    // registers before the model's own, one wavefront per SIMD; four + six short ones leave room for two
    constexpr int UPL = (TMAX * m + TPI - 1) / TPI;
    // Long knots (EPL >= 12: the quadrotor's 16 elements per lane): the quadratic cost along the search direction is
    // the polynomial c0 + s c1 + s^2 c2 of the step -- three numbers per lane instead of the cost's two arrays (64
    // registers at nt = 16, which kept the kernel at one wavefront per SIMD) and two fmas per candidate instead of 2 EPL.
    constexpr bool POLY = EPL >= 12;
    double ex[EPL], eu[EPL], eq[POLY ? 1 : EPL], el[POLY ? 1 : EPL];
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    // state box: the pair and the two multipliers of the lane's state elements, loaded once with the element (short
    // knots); the long knots, whose registers are taken, read them per candidate (20 reads of lines that stay in cache)
    constexpr bool XREG = XB && !POLY;
    [[maybe_unused]] double sh[XREG ? EPL : 1], sl[XREG ? EPL : 1], smu[XREG ? EPL : 1], sml[XREG ? EPL : 1];
    [[maybe_unused]] const double *xhb = nullptr, *xlb = nullptr;
    if constexpr (XB) { xhb = P.xhi + b * P.xsb; xlb = P.xlo + b * P.xsb; }
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        const int e = r + TPI * i, ec = e < nzq ? e : 0, t = ec / nt, j = ec - t * nt;
        const bool ok = e < nzq;
        ex[i] = ok ? xu[ec] : 0.0; eu[i] = (ok && P.ncand > 0) ? up[ec] : 0.0;
        const double qd = ok ? Qd[ec] : 0.0, ql = ok ? q[ec] : 0.0;
        if (ok && t == 0 && j < n) { ex[i] = x0[j]; eu[i] = 0.0; }            // x_0 pinned to x0 (al_utils.py:515)
        if constexpr (POLY) {
            const double qx = qd * ex[i];
            c0 += (0.5 * qx + ql) * ex[i];
            c1 += (qx + ql) * eu[i];
            c2 += 0.5 * qd * eu[i] * eu[i];
        } else {
            eq[i] = qd; el[i] = ql;
        }
        if constexpr (XREG) {
            const bool xs = ok && j < n;
            const int jx = xs ? j : 0, row = neq + 2 * T * m + t * 2 * n + jx;
            sh[i] = xs ? xhb[t * P.xst + jx] : INFINITY; sl[i] = xs ? xlb[t * P.xst + jx] : -INFINITY;
            smu[i] = xs ? lam[row] : 0.0; sml[i] = xs ? lam[row + n] : 0.0;
        }
    }
    double cx[UPL], cu[UPL], lu[UPL], ll[UPL], hi[UPL], lo[UPL];
#pragma unroll
    for (int i = 0; i < UPL; ++i) {
        const int c = r + TPI * i, cc = c < T * m ? c : 0, t = cc / m, iu = cc - t * m;
        const bool ok = c < T * m;
        const int ec = t * nt + n + iu, row = neq + t * 2 * m + iu;
        cx[i] = ok ? xu[ec] : 0.0; cu[i] = (ok && P.ncand > 0) ? up[ec] : 0.0;
        lu[i] = ok ? lam[row] : 0.0; ll[i] = ok ? lam[row + m] : 0.0;
        // strided: the element's own knot, once, with its multipliers
        const long long bo = al_bound_at<strided_bounds<Map>::value>(b, t, iu, P.bsb, P.bst);
        hi[i] = ok ? P.uu[bo] : INFINITY; lo[i] = ok ? P.ul[bo] : -INFINITY;
    }
    // multipliers of the lane's dynamics rows: registers, or -- long knots -- the group's LDS rows behind its iterate
    double ly[POLY ? 1 : n];
    double *lyb = lsg_lds + (size_t)(256 / TPI) * T * ZS + ((size_t)grp * T + r) * n;
#pragma unroll
    for (int j = 0; j < n; ++j) {
        const double v = (r < T - 1) ? lam[r * n + j] : 0.0;
        if constexpr (POLY) { if (r < T) lyb[j] = v; } else ly[j] = v;
    }
    // candidates k = blockIdx.y, blockIdx.y + gridDim.y, ...: small batches are split over more wavefronts
    const bool fold = P.xu_w != nullptr && gridDim.y == 1 && P.ncand > 0;
    double best = 0.0;
    int arg = 0;
    bool isnan_ = false;
    for (int k = blockIdx.y; k < nc; k += gridDim.y) {
        const double step = P.ncand > 0 ? al_step(k) : 0.0;
        double acc = POLY ? fma(step, fma(step, c2, c1), c0) : 0.0;
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
            const int e = r + TPI * i;
            if (e < nzq) {
                const int t = e / nt, j = e - t * nt;
                const double z = fma(step, eu[i], ex[i]);
                zb[t * ZS + j] = z;
                if constexpr (!POLY) acc += al_cost_term(eq[i], el[i], z);
                if constexpr (XB) {         // the element's state rows, into the accumulator the lane already owns
                    if (j < n) {
                        double h, l, mu, ml;
                        if constexpr (XREG) { h = sh[i]; l = sl[i]; mu = smu[i]; ml = sml[i]; }
                        else {
                            const int row = neq + 2 * T * m + t * 2 * n + j;
                            h = xhb[t * P.xst + j]; l = xlb[t * P.xst + j]; mu = lam[row]; ml = lam[row + n];
                        }
                        acc += al_pair_term(rho, mu, ml, z - h, l - z);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < UPL; ++i) {
            if (r + TPI * i < T * m) {
                const double z = fma(step, cu[i], cx[i]);
                acc += al_pair_term(rho, lu[i], ll[i], z - hi[i], lo[i] - z);
            }
        }
        group_sync();
        if (r < T - 1) {
            double z[nt], xn[n];
#pragma unroll
            for (int j = 0; j < nt; ++j) z[j] = zb[r * ZS + j];
            Map::template step<double>(z, z + n, P.dt, xn);
#pragma unroll
            for (int j = 0; j < n; ++j) {
                const double res = zb[(r + 1) * ZS + j] - xn[j];
                acc += al_eq_term(rho, POLY ? lyb[j] : ly[j], res);
            }
        }
        group_sync();
        acc = group_sum<TPI>(acc);
        if (fold) {             // torch.min over the candidates: NaN wins, else the first minimum
            if (k == 0) { best = acc; arg = 0; isnan_ = acc != acc; }
            else if (!isnan_) {
                if (acc != acc) { best = acc; arg = k; isnan_ = true; }
                else if (acc < best) { best = acc; arg = k; }
            }
        } else if (r == 0 && live) {
            P.merit[(long long)k * P.B + b] = acc;
        }
    }
    if (fold) {
        const bool take = best < P.merit_cur[b];
        if (r == 0 && live) {
            P.merit_cur[b] = best;                              // new_merit regardless of acceptance
            if (P.status) P.status[b] = take ? 1.0 : 0.0;
            if (P.info && P.info[b] != 0) atomicOr(P.fail, 1);  // Cholesky failed: the caller re-runs the slow path
        }
        if (take && live) {
            const double sb = al_step(arg);
            double *xw = P.xu_w + b * (long long)nzq;
#pragma unroll
            for (int i = 0; i < EPL; ++i) {
                const int e = r + TPI * i;
                if (e < nzq) xw[e] = fma(sb, eu[i], ex[i]);
            }
        }
    }
}

template <class Map, int TPI, int TMAX = TPI> int launch_ls_group(const LsAP &P, hipStream_t st)
{
    constexpr int ZS = (Map::NX + Map::NU) | 1, G = 256 / TPI;
    constexpr bool POLY = (TMAX * (Map::NX + Map::NU) + TPI - 1) / TPI >= 12;
    const size_t lds = (size_t)G * P.T * (ZS + (POLY ? Map::NX : 0)) * sizeof(double);
    const unsigned blocks = (unsigned)((P.B + G - 1) / G);
    // at least ~2 wavefronts per SIMD where the batch alone does not give them: split the candidates
    unsigned split = 1;
    if (P.ncand > 1) while (split < 4 && (unsigned long long)blocks * 4 * split < 2048) split *= 2;
    DQP_LAUNCH((al_ls_group_kernel<Map, TPI, TMAX>), dim3(blocks, split), dim3(256), lds, st, P);
    return (P.xu_w && split == 1 && P.ncand > 0) ? 2 : DQP_OK;     // 2: the selection happened in the kernel
}

template <class Map> int launch_ls_t(const LsAP &P, hipStream_t st)
{
    // the model phase keeps T - 1 lanes of a group busy: four lanes for the shortest horizons (config 5: T = 5)
    if (P.T <= 5) return launch_ls_group<Map, 4, 5>(P, st);
    if (P.T <= 8) return launch_ls_group<Map, 8>(P, st);
    if (P.T <= 16) return launch_ls_group<Map, 16>(P, st);
    if (P.T <= 32) return launch_ls_group<Map, 32>(P, st);
    const long long items = (long long)(P.ncand > 0 ? P.ncand : 1) * P.B;
    DQP_LAUNCH(al_ls_kernel<Map>, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, st, P);
    return DQP_OK;
}

int launch_ls(const LsAP &P, hipStream_t st)
{
    return dqp::dyn::visit<int>(P.dyn, DQP_ERR_BAD_ARG, [&](auto model) {
        using Map = typename decltype(model)::Map;
        if (P.xlo) return launch_ls_t<BoxBounds<Map>>(P, st);         // a state box: both boxes strided
        return (P.bsb != 0 || P.bst != 0) ? launch_ls_t<StridedBounds<Map>>(P, st) : launch_ls_t<Map>(P, st);
    });
}

struct OutP {
    const double *xu, *x0, *lam, *rho, *Qd, *q, *ul, *uu;
    double *lam_new, *cost, *resn;
    double dt;
    int B, n, m, T, dyn;
    double *rho_next;       // optional: rho * 10 (AL_mpc.py:307), for the next AL iteration of dqp_al_mpc_solve
    long long bsb, bst;     // bound layout (dqp_al_bounds.h), read by the StridedBounds<> instantiations only
    const double *xlo, *xhi;    // state box, read by the BoxBounds<> instantiations only (else NULL); lam / lam_new then
    long long xsb, xst;         // carry 2 T n more rows
};
// lam_new <- the multiplier update of v.lam at xu; rho_next: optional
OutP out_args(const AlProblem &v, const double *xu, double *lam_new, double *cost, double *resn, double *rho_next)
{
    OutP P = dqp::boxed_args<OutP>(v);
    P.xu = xu; P.lam_new = lam_new; P.cost = cost; P.resn = resn; P.rho_next = rho_next;
    P.dt = v.dt; P.n = v.n; P.m = v.m; P.dyn = v.model;
    return P;
}

// Between two AL iterations (qpth/AL_mpc.py:296-307): res = constraint residual at the new iterate,
// lam <- lam + rho res with the inequality block clamped at 0, cost of the iterate and the norm of
// the clamped residual; 16 lanes per problem, dynamics evaluated in the kernel.
template <class Map>
__global__ __launch_bounds__(256) void al_outer_kernel(OutP P)
{
    constexpr int n = Map::NX, m = Map::NU, nt = n + m;
    constexpr bool XB = box_bounds<Map>::value;
    const int T = P.T, neq = AlRows{n, m, T, XB}.neq(), ncon = AlRows{n, m, T, XB}.ncon();
    const long long item = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int r = threadIdx.x & 15;
    const long long b = item < P.B ? item : P.B - 1;
    const bool live = item < P.B;
    const double *xu = P.xu + b * (long long)T * nt, *lam = P.lam + b * (long long)ncon;
    const double *Qd = P.Qd + b * (long long)T * nt, *q = P.q + b * (long long)T * nt;
    double *ln = P.lam_new + b * (long long)ncon;
    const double rho = P.rho[b];
    constexpr bool SB = strided_bounds<Map>::value;
    double cost = 0.0, rn2 = 0.0;
    for (int t = r; t < T; t += 16) {
        double z[nt], xn[n];
#pragma unroll
        for (int j = 0; j < nt; ++j) z[j] = xu[t * nt + j];
        for (int j = 0; j < nt; ++j) cost += al_cost_term(Qd[t * nt + j], q[t * nt + j], z[j]);
        if (t < T - 1) {
            Map::template step<double>(z, z + n, P.dt, xn);
            for (int j = 0; j < n; ++j) {
                const double res = xu[(t + 1) * nt + j] - xn[j];
                rn2 += res * res;
                if (live) ln[t * n + j] = lam[t * n + j] + rho * res;
            }
        } else {
            for (int j = 0; j < n; ++j) {
                const double res = xu[j] - P.x0[b * n + j];
                rn2 += res * res;
                if (live) ln[(T - 1) * n + j] = lam[(T - 1) * n + j] + rho * res;
            }
        }
        for (int i = 0; i < m; ++i) {
            double uut, ult;
            if constexpr (SB) { uut = P.uu[b * P.bsb + t * P.bst + i]; ult = P.ul[b * P.bsb + t * P.bst + i]; }
            else { uut = P.uu[i]; ult = P.ul[i]; }
            const double u = z[n + i], hi = u - uut, lo = ult - u;
            const int row = neq + t * 2 * m + i;
            rn2 += al_pair_sq(hi, lo);
            if (live) {
                ln[row] = fmax(lam[row] + rho * hi, 0.0);               // AL_mpc.py:300-301
                ln[row + m] = fmax(lam[row + m] + rho * lo, 0.0);
            }
        }
        if constexpr (XB) {         // the knot's state rows: multipliers clamped at 0, their share of |res_clamp|
            for (int j = 0; j < n; ++j) {
                const double hi = z[j] - P.xhi[b * P.xsb + t * P.xst + j], lo = P.xlo[b * P.xsb + t * P.xst + j] - z[j];
                const int row = neq + 2 * T * m + t * 2 * n + j;
                rn2 += al_pair_sq(hi, lo);
                if (live) {
                    ln[row] = fmax(lam[row] + rho * hi, 0.0);
                    ln[row + n] = fmax(lam[row + n] + rho * lo, 0.0);
                }
            }
        }
    }
    cost = dqp::r16::row_sum(cost);
    rn2 = dqp::r16::row_sum(rn2);
    if (live && r == 0) {
        P.cost[b] = cost; P.resn[b] = sqrt(rn2);
        if (P.rho_next) P.rho_next[b] = rho * 10.0;
    }
}

// Head of AL_mpc.MPC.al_solve (AL_mpc.py:254-283): xu = [x_init | u_init], cost_start = compute_cost(xu), the warm
// start of the multipliers / penalty from the previous call's history (al_utils.warm_start_al, al_utils.py:16-34:
// the newest stored AL iterate whose cost was already below cost_start, the newest one if none was; lam rescaled to
// that iterate's norm), and entry 0 of this call's history.  16 lanes per problem.
struct StartP {
    const double *x_init, *u_init, *Qd, *q, *lam_in, *rho_in;
    const double *hist_cost, *hist_lam, *hist_rho;      // previous call, oldest first: (K, B), (K, B, ncon), (K, B); or NULL
    double *xu, *cost0, *lam0, *rho0;
    int B, n, m, T, K;
    int32_t *fail;          // al_iter Cholesky-failure flags, cleared here
    int nfail;
};
// XB: a state box -- the multipliers and the history rows are 2 T n wider, and the norms and the scaling of the warm start
// run over all of them
template <bool XB> __device__ __forceinline__ void start_body(const StartP &P)
{
    const int n = P.n, m = P.m, nt = n + m, T = P.T, ncon = AlRows{n, m, T, XB}.ncon();
    const long long item = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int r = threadIdx.x & 15;
    const long long b = item < P.B ? item : P.B - 1;
    const bool live = item < P.B;
    if (blockIdx.x == 0 && (int)threadIdx.x < P.nfail) P.fail[threadIdx.x] = 0;
    double *xu = P.xu + b * (long long)T * nt;
    const double *Qd = P.Qd + b * (long long)T * nt, *q = P.q + b * (long long)T * nt;
    double quad = 0.0, lin = 0.0;
    for (int e = r; e < T * nt; e += 16) {
        const int t = e / nt, j = e - t * nt;
        const double v = j < n ? P.x_init[(b * T + t) * n + j] : P.u_init[(b * T + t) * m + (j - n)];
        if (live) xu[e] = v;
        quad += v * Qd[e] * v;
        lin += q[e] * v;
    }
    const double cost0 = 0.5 * dqp::r16::row_sum(quad) + dqp::r16::row_sum(lin);       // al_utils.compute_cost, diagonal cost
    const double *lam = P.lam_in + b * (long long)ncon;
    const AlWarm w = al_warm_start(P.K, P.B, b, ncon, cost0, P.hist_cost, P.hist_lam, P.hist_rho, lam, P.rho_in[b], r, 16,
                                   [](double v) { return dqp::r16::row_sum(v); });
    if (!live) return;
    double *l0 = P.lam0 + b * (long long)ncon;
    for (int e = r; e < ncon; e += 16) l0[e] = P.K > 0 ? lam[e] * w.scale : lam[e];
    if (r == 0) { P.cost0[b] = cost0; P.rho0[b] = w.rho; }
}
__global__ __launch_bounds__(256) void al_start_kernel(StartP P) { start_body<false>(P); }
__global__ __launch_bounds__(256) void al_start_xbounds_kernel(StartP P) { start_body<true>(P); }

int launch_outer(const OutP &P, hipStream_t st)
{
    const dim3 grid((unsigned)((P.B + 15) / 16)), block(256);
    return dqp::dyn::visit<int>(P.dyn, DQP_ERR_BAD_ARG, [&](auto model) {
        using Map = typename decltype(model)::Map;
        if (P.xlo) DQP_LAUNCH(al_outer_kernel<BoxBounds<Map>>, grid, block, 0, st, P);
        else if (P.bsb != 0 || P.bst != 0) DQP_LAUNCH(al_outer_kernel<StridedBounds<Map>>, grid, block, 0, st, P);
        else DQP_LAUNCH(al_outer_kernel<Map>, grid, block, 0, st, P);
        return launched();
    });
}

struct SelP {
    const double *merit, *upd, *x0;
    double *xu, *merit_cur, *status;
    int32_t *fail;
    const int32_t *info;
    int B, n, nz, ncand;
};

// argmin over the candidates, acceptance test and update of the iterate (al_utils.py:516-526):
// one 64-thread block per problem
__global__ __launch_bounds__(64) void al_select_kernel(SelP P)
{
    const long long b = blockIdx.x;
    // torch.min over the candidates (NaN wins, else the first minimum): lane k holds candidate k -- one round of
    // loads and a wavefront reduction instead of one lane walking ncand dependent loads (11 us -> launch-bound)
    const int lane = threadIdx.x;
    const bool has = lane < P.ncand;
    const AlBest best = al_wave_argmin(has ? P.merit[(long long)lane * P.B + b] : INFINITY, has);
    const bool take = best.merit < P.merit_cur[b];
    const double s_step = al_step(best.arg);
    if (lane == 0) {
        P.merit_cur[b] = best.merit;                        // new_merit regardless of acceptance
        if (P.status) P.status[b] = take ? 1.0 : 0.0;
        if (P.info && P.info[b] != 0) atomicOr(P.fail, 1);  // Cholesky failed: the caller re-runs the slow path
    }
    if (!take) return;
    double *xu = P.xu + b * (long long)P.nz;
    const double *up = P.upd + b * (long long)P.nz;
    for (int e = threadIdx.x; e < P.nz; e += 64)
        xu[e] = e < P.n ? P.x0[b * P.n + e] : xu[e] + s_step * up[e];
}

template <typename K>
int launch(K kernel, const AlP &P, size_t lds, void *stream, int threads = 256)
{
    if (P.B == 0) return DQP_OK;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return DQP_ERR_LAUNCH;
    DQP_LAUNCH(kernel, dim3(P.B), dim3(threads), lds, (hipStream_t)stream, P);
    return launched();
}

// the dense Newton step: al_newton_kernel at the number of 16-column slots nz takes
int launch_newton(const AlP &P, size_t lds, void *stream)
{
    static constexpr decltype(&al_newton_kernel<1>) kernels[8] = {
        al_newton_kernel<1>, al_newton_kernel<2>, al_newton_kernel<3>, al_newton_kernel<4>,
        al_newton_kernel<5>, al_newton_kernel<6>, al_newton_kernel<7>, al_newton_kernel<8>};
    const int slots = (P.nz + 15) / 16;         // 1 .. 8 behind fill(); anything else takes the largest, as it always did
    return launch(kernels[slots >= 1 && slots < 8 ? slots - 1 : 7], P, lds, stream);
}

// The workspace of dqp_al_newton_solve in its two forms (include/dqp.h, "Extents"), carved and sized from ONE member
// list.  The last array, info, is nbatch int32 in a slot of nbatch doubles, so every array before it starts on a multiple
// of 8 bytes and nothing lies behind it.
struct NewtonWork {
    double *Jx, *Ju, *resc, *Jc, *grad;         // the dense form only
    double *upd, *merit, *merit_cur;            // update, AL_NCAND candidate merits, current merit
    int32_t *info;
    size_t doubles;                             // of the form, per problem
};
// The arrays of a batch of B at `base`, in the order they lie; (NULL, 0): the size alone
NewtonWork newton_work(void *base, size_t B, bool banded, size_t n, size_t m, size_t T)
{
    const size_t nz = T * (n + m), ncon = AlRows{(int)n, (int)m, (int)T, false}.ncon();   // the dense form has no state box
    NewtonWork w = {};
    auto take = [&](auto *&array, size_t per_problem) {
        array = reinterpret_cast<std::remove_reference_t<decltype(array)>>((double *)base + B * w.doubles);
        w.doubles += per_problem;
    };
    if (!banded) { take(w.Jx, (T - 1) * n * n); take(w.Ju, (T - 1) * n * m); take(w.resc, ncon); take(w.Jc, ncon * nz); take(w.grad, nz); }
    take(w.upd, nz); take(w.merit, AL_NCAND); take(w.merit_cur, 1); take(w.info, 1);
    return w;
}

// What dqp_al_newton_solve takes besides the problem, in the order of its prototype
struct NewtonIo {
    int32_t n_steps;
    double *xu, *L, *status;
    int32_t *fail;
    void *workspace;
    bool clear_fail = true;     // false: the caller's own kernel zeroed the flag (dqp_al_mpc_solve: al_start_kernel clears all)
    bool keep_factor = true;    // false: nobody reads L after this call (only the last solve's last factor is used,
                                // NewtonAL.backward, al_utils.py:477-480)
};

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int
dqp_al_newton_step(const dqp_al_dims *dims, const double *Jc, const double *Qdiag, const double *rho,
                   const double *grad, double *update, double *L, int32_t *info, void *stream)
{
    AlP P = {};
    size_t lds = 0;
    int rc = fill(dims, P, lds);
    if (rc) return rc;
    if (P.B == 0) return DQP_OK;
    if ((!Jc && P.ncon > 0) || !Qdiag || !rho || !grad || !update) return DQP_ERR_BAD_ARG;
    P.Jc = Jc; P.Qd = Qdiag; P.rho = rho; P.grad = grad; P.update = update; P.L = L; P.info = info;
    return launch_newton(P, lds, stream);
}

__attribute__((visibility("default"))) int
dqp_al_chol_solve(const dqp_al_dims *dims, const double *L, const double *rhs, double *out, void *stream)
{
    AlP P = {};
    size_t lds = 0;
    int rc = fill(dims, P, lds);
    if (rc) return rc;
    if (P.B == 0) return DQP_OK;
    if (!L || !rhs || !out) return DQP_ERR_BAD_ARG;
    P.Lin = L; P.rhs = rhs; P.out = out;
    return launch(al_chol_solve_kernel, P, lds, stream);
}

__attribute__((visibility("default"))) int
dqp_al_assemble(const dqp_al_mpc_dims *d, const double *Jx, const double *Ju, const double *lam,
                const double *res_c, const double *rho, double *Jc, double *gterm, void *stream)
{
    if (!d || d->nbatch < 0 || d->n_state <= 0 || d->n_ctrl <= 0 || d->T < 2) return DQP_ERR_BAD_ARG;
    if (d->nbatch == 0) return DQP_OK;
    if (!Jx || !Ju || !res_c || (gterm && (!lam || !rho))) return DQP_ERR_BAD_ARG;
    AsmP P = {};        // no Qd, q, xu: gterm without the cost's share
    P.Jx = Jx; P.Ju = Ju; P.lam = lam; P.resc = res_c; P.rho = rho; P.Jc = Jc; P.gterm = gterm;
    P.B = d->nbatch; P.n = d->n_state; P.m = d->n_ctrl; P.T = d->T;
    DQP_LAUNCH(al_assemble_kernel, dim3(P.B), dim3(256), 0, (hipStream_t)stream, P);
    return launched();
}

// Both merit entries behind their front checks
static int merit_launch(const AlProblem &v, int32_t ncand, const double *xu, const double *x_next, double *merit)
{
    if (ncand == 0) return DQP_OK;
    if (const int r = v.ready(xu && x_next && merit); r != 1) return r;
    MeritP P = dqp::boxed_args<MeritP>(v);
    P.xu = xu; P.xn = x_next; P.merit = merit; P.n = v.n; P.m = v.m; P.ncand = ncand;
    const dim3 grid((unsigned)(((long long)ncand * v.B + 15) / 16));
    if (!v.has_x && v.strided()) DQP_LAUNCH(al_merit_kernel<true>, grid, dim3(256), 0, v.stream, P);
    else if (!v.has_x) DQP_LAUNCH(al_merit_kernel<false>, grid, dim3(256), 0, v.stream, P);
    else DQP_LAUNCH((al_merit_kernel<true, true>), grid, dim3(256), 0, v.stream, P);
    return launched();
}

__attribute__((visibility("default"))) int
dqp_al_merit_bounds(const dqp_al_mpc_dims *d, int32_t ncand, const double *xu, const double *x_next,
                    const double *x0, const double *Qdiag, const double *q, const double *lam,
                    const double *rho, const dqp_al_bounds *bounds, double *merit, void *stream)
{
    if (dqp::al_bounds_check(d, bounds) || ncand < 0) return DQP_ERR_BAD_ARG;
    return merit_launch(dqp::al_problem(d, 0, 0.0, x0, Qdiag, q, lam, rho, bounds, nullptr, stream), ncand, xu, x_next, merit);
}

// The merit with state rows (include/dqp.h): lam has dqp_al_ncon_xbounds(dims) rows per problem; any (n_state, n_ctrl)
__attribute__((visibility("default"))) int
dqp_al_merit_xbounds(const dqp_al_mpc_dims *d, int32_t ncand, const double *xu, const double *x_next,
                     const double *x0, const double *Qdiag, const double *q, const double *lam,
                     const double *rho, const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, double *merit,
                     void *stream)
{
    // no model and any (n_state, n_ctrl): the sizes and both layouts, not al_xbounds_check
    if (dqp::al_bounds_check(d, bounds) || dqp::al_box_layout(xbounds, d, d->n_state) || ncand < 0) return DQP_ERR_BAD_ARG;
    return merit_launch(dqp::al_problem(d, 0, 0.0, x0, Qdiag, q, lam, rho, bounds, xbounds, stream), ncand, xu, x_next, merit);
}

__attribute__((visibility("default"))) int
dqp_al_merit(const dqp_al_mpc_dims *d, int32_t ncand, const double *xu, const double *x_next,
             const double *x0, const double *Qdiag, const double *q, const double *lam,
             const double *rho, const double *u_lower, const double *u_upper, double *merit, void *stream)
{
    const dqp_al_bounds bd = {u_lower, u_upper, 0, 0};
    return dqp_al_merit_bounds(d, ncand, xu, x_next, x0, Qdiag, q, lam, rho, &bd, merit, stream);
}


__attribute__((visibility("default"))) size_t dqp_al_newton_solve_bytes(const dqp_al_mpc_dims *d, int32_t banded)
{
    if (!d || d->nbatch <= 0 || d->n_state <= 0 || d->n_ctrl <= 0 || d->T < 2) return 0;
    return (size_t)d->nbatch * newton_work(nullptr, 0, banded != 0, d->n_state, d->n_ctrl, d->T).doubles * sizeof(double);
}

// What the two Newton loops share: the arguments of the candidates' line search and of the selection, the failure flag
// cleared, the merit at the start
static int newton_start(const AlProblem &v, const NewtonIo &o, const NewtonWork &w, LsAP &Lc, SelP &Se)
{
    Lc = ls_args(v, o.xu, w.upd, w.merit, AL_NCAND);
    Se.merit = w.merit; Se.upd = w.upd; Se.x0 = v.x0; Se.xu = o.xu; Se.merit_cur = w.merit_cur; Se.status = o.status;
    Se.fail = o.fail; Se.info = w.info; Se.B = v.B; Se.n = v.n; Se.nz = v.nz(); Se.ncand = AL_NCAND;
    if (o.clear_fail && hipMemsetAsync(o.fail, 0, sizeof(int32_t), v.stream) != hipSuccess) return DQP_ERR_LAUNCH;
    return launch_ls(ls_args(v, o.xu, w.upd, w.merit_cur, 0), v.stream);
}

// Block-tridiagonal form (dqp_al_banded.hip): linearise + gradient + block Cholesky + solve in ONE launch per step, no
// Jacobian / Hessian in HBM; L receives the banded factor.  The only form that takes a state box.
static int newton_banded(const AlProblem &v, const NewtonIo &o)
{
    if (!v.model_ok()) return DQP_ERR_BAD_ARG;
    if (v.too_large()) return DQP_ERR_TOO_LARGE;
    if (!o.L) return DQP_ERR_BAD_ARG;
    const NewtonWork w = newton_work(o.workspace, v.B, true, v.n, v.m, v.T);
    LsAP Lc;
    SelP Se;
    int rc = newton_start(v, o, w, Lc, Se);
    if (rc) return rc;
    // the selection folded into the line search where one group sees all candidates of its problem
    Lc.xu_w = o.xu; Lc.merit_cur = w.merit_cur; Lc.status = o.status; Lc.fail = o.fail; Lc.info = w.info;
    for (int it = 0; it < o.n_steps; ++it) {
        if ((rc = al_banded_newton_step(v, o.xu, w.upd, o.L, w.info, it == o.n_steps - 1 && o.keep_factor)) != DQP_OK) return rc;
        rc = launch_ls(Lc, v.stream);
        if (rc != DQP_OK && rc != 2) return rc;
        // candidates split over several groups: select in a launch of its own
        if (rc != 2) DQP_LAUNCH(al_select_kernel, dim3(v.B), dim3(64), 0, v.stream, Se);
    }
    return launched();
}

// Dense form: Jacobians, the assembled Jc and the nz x nz factor in HBM / LDS; control bounds only
static int newton_dense(const AlProblem &v, const NewtonIo &o)
{
    if (!v.model_ok()) return DQP_ERR_BAD_ARG;
    if (v.n > LIN_NX || v.m > LIN_NU) return DQP_ERR_TOO_LARGE;
    const dqp_al_dims ad = {v.B, v.nz(), (int)v.ncon(), 0};
    AlP A = {};
    size_t lds = 0;
    int rc = fill(&ad, A, lds);
    if (rc) return rc;
    const NewtonWork w = newton_work(o.workspace, v.B, false, v.n, v.m, v.T);
    A.Jc = w.Jc; A.Qd = v.Qd; A.rho = v.rho; A.grad = w.grad; A.update = w.upd; A.L = o.L; A.info = w.info;
    LsAP Lc;
    SelP Se;
    if ((rc = newton_start(v, o, w, Lc, Se)) != DQP_OK) return rc;
    // the clamped box rows carry the bound layout; the dense assembly and factorisation read them
    LinP Li = {};
    Li.xu = o.xu; Li.x0 = v.x0; Li.ul = v.u.lower; Li.uu = v.u.upper; Li.Jx = w.Jx; Li.Ju = w.Ju; Li.resc = w.resc;
    Li.dt = v.dt; Li.B = v.B; Li.n = v.n; Li.m = v.m; Li.T = v.T; Li.dyn = v.model; Li.bsb = v.u.stride_b; Li.bst = v.u.stride_t;
    const dim3 lin_grid((unsigned)(((long long)v.B * v.T + 255) / 256));
    AsmP As = {};
    As.Jx = w.Jx; As.Ju = w.Ju; As.lam = v.lam; As.resc = w.resc; As.rho = v.rho; As.Jc = w.Jc; As.gterm = w.grad;
    As.B = v.B; As.n = v.n; As.m = v.m; As.T = v.T; As.Qd = v.Qd; As.q = v.q; As.xu = o.xu;
    for (int it = 0; it < o.n_steps; ++it) {
        if (v.strided()) DQP_LAUNCH(al_linearize_kernel<true>, lin_grid, dim3(256), 0, v.stream, Li);
        else DQP_LAUNCH(al_linearize_kernel<false>, lin_grid, dim3(256), 0, v.stream, Li);
        DQP_LAUNCH(al_assemble_kernel, dim3(v.B), dim3(256), 0, v.stream, As);
        if ((rc = launch_newton(A, lds, v.stream)) != DQP_OK) return rc;
        if ((rc = launch_ls(Lc, v.stream)) != DQP_OK) return rc;
        DQP_LAUNCH(al_select_kernel, dim3(v.B), dim3(64), 0, v.stream, Se);
    }
    return launched();
}

__attribute__((visibility("default"))) int
dqp_al_newton_solve_bounds(const dqp_al_mpc_dims *d, int dyn_id, double dt, int32_t n_steps, int32_t banded,
                           const double *x0, const double *Qdiag, const double *q, const double *lam, const double *rho,
                           const dqp_al_bounds *bounds, double *xu, double *L, double *status,
                           int32_t *fail, void *workspace, void *stream)
{
    if (dqp::al_bounds_check(d, bounds) || n_steps < 1) return DQP_ERR_BAD_ARG;
    const AlProblem v = dqp::al_problem(d, dyn_id, dt, x0, Qdiag, q, lam, rho, bounds, nullptr, stream);
    if (const int r = v.ready(xu && fail && workspace); r != 1) return r;
    return (banded ? newton_banded : newton_dense)(v, {n_steps, xu, L, status, fail, workspace});
}

__attribute__((visibility("default"))) int
dqp_al_newton_solve(const dqp_al_mpc_dims *d, int dyn_id, double dt, int32_t n_steps, int32_t banded,
                    const double *x0, const double *Qdiag, const double *q, const double *lam, const double *rho,
                    const double *u_lower, const double *u_upper, double *xu, double *L, double *status,
                    int32_t *fail, void *workspace, void *stream)
{
    const dqp_al_bounds bd = {u_lower, u_upper, 0, 0};
    return dqp_al_newton_solve_bounds(d, dyn_id, dt, n_steps, banded, x0, Qdiag, q, lam, rho, &bd, xu, L, status, fail,
                                      workspace, stream);
}


__attribute__((visibility("default"))) int
dqp_al_outer_update(const dqp_al_mpc_dims *d, int dyn_id, double dt, const double *xu, const double *x0,
                    const double *lam, const double *rho, const double *Qdiag, const double *q,
                    const double *u_lower, const double *u_upper, double *lam_new, double *cost,
                    double *res_norm, void *stream)
{
    const dqp_al_bounds bd = {u_lower, u_upper, 0, 0};
    return dqp_al_outer_update_bounds(d, dyn_id, dt, xu, x0, lam, rho, Qdiag, q, &bd, lam_new, cost, res_norm, stream);
}

// behind either front check.  The model in front of the limit, the limit in front of the buffers.
static int outer_update(const AlProblem &v, const double *xu, double *lam_new, double *cost, double *res_norm)
{
    if (v.B == 0) return DQP_OK;
    if (!v.model_ok()) return DQP_ERR_BAD_ARG;
    if (v.too_large()) return DQP_ERR_TOO_LARGE;
    if (!v.inputs_set() || !xu || !lam_new || !cost || !res_norm) return DQP_ERR_BAD_ARG;
    return launch_outer(out_args(v, xu, lam_new, cost, res_norm, nullptr), v.stream);
}

__attribute__((visibility("default"))) int
dqp_al_outer_update_bounds(const dqp_al_mpc_dims *d, int dyn_id, double dt, const double *xu, const double *x0,
                           const double *lam, const double *rho, const double *Qdiag, const double *q,
                           const dqp_al_bounds *bounds, double *lam_new, double *cost, double *res_norm, void *stream)
{
    if (dqp::al_bounds_check(d, bounds)) return DQP_ERR_BAD_ARG;
    return outer_update(dqp::al_problem(d, dyn_id, dt, x0, Qdiag, q, lam, rho, bounds, nullptr, stream), xu, lam_new, cost, res_norm);
}

__attribute__((visibility("default"))) int
dqp_al_outer_update_xbounds(const dqp_al_mpc_dims *d, int model, double dt, const double *xu, const double *x0,
                            const double *lam, const double *rho, const double *Qdiag, const double *q,
                            const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, double *lam_new, double *cost,
                            double *res_norm, void *stream)
{
    if (const int rc = al_xbounds_check(d, bounds, xbounds, d && dyn::model_matches(model, d->n_state, d->n_ctrl))) return rc;
    return outer_update(dqp::al_problem(d, model, dt, x0, Qdiag, q, lam, rho, bounds, xbounds, stream), xu, lam_new, cost, res_norm);
}

__attribute__((visibility("default"))) int32_t dqp_al_ncon_xbounds(const dqp_al_mpc_dims *d)
{
    if (!d || d->n_state <= 0 || d->n_ctrl <= 0 || d->T <= 0) return 0;
    return AlRows{d->n_state, d->n_ctrl, d->T, true}.ncon();
}

// the workspace does not depend on the rows: that of the `_bounds` twins
__attribute__((visibility("default"))) size_t dqp_al_newton_solve_xbounds_bytes(const dqp_al_mpc_dims *d)
{
    return dqp_al_newton_solve_bytes(d, 1);
}
__attribute__((visibility("default"))) size_t dqp_al_mpc_solve_xbounds_bytes(const dqp_al_mpc_dims *d)
{
    return dqp_al_newton_solve_bytes(d, 1);
}

__attribute__((visibility("default"))) int
dqp_al_newton_solve_xbounds(const dqp_al_mpc_dims *d, int model, double dt, int32_t n_steps, const double *x0,
                            const double *Qdiag, const double *q, const double *lam, const double *rho,
                            const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, double *xu, double *L,
                            double *status, int32_t *fail, void *workspace, void *stream)
{
    if (const int rc = al_xbounds_check(d, bounds, xbounds, d && dyn::model_matches(model, d->n_state, d->n_ctrl))) return rc;
    if (n_steps < 1) return DQP_ERR_BAD_ARG;
    const AlProblem v = dqp::al_problem(d, model, dt, x0, Qdiag, q, lam, rho, bounds, xbounds, stream);
    if (const int r = v.ready(xu && fail && workspace); r != 1) return r;
    return newton_banded(v, {n_steps, xu, L, status, fail, workspace});        // block-tridiagonal only
}

__attribute__((visibility("default"))) size_t dqp_al_mpc_solve_bytes(const dqp_al_mpc_dims *d)
{
    return dqp_al_newton_solve_bytes(d, 1);
}

__attribute__((visibility("default"))) int
dqp_al_mpc_solve(const dqp_al_mpc_dims *d, int dyn_id, double dt, int32_t al_iter, int32_t newton_steps,
                 const double *x_init, const double *u_init, const double *x0, const double *Qdiag, const double *q,
                 const double *u_lower, const double *u_upper, const double *lam_in, const double *rho_in,
                 const double *prev_cost, const double *prev_lam, const double *prev_rho, int32_t n_prev,
                 double *xu, double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm, double *factor,
                 double *status, int32_t *fail, void *workspace, void *stream)
{
    const dqp_al_bounds bd = {u_lower, u_upper, 0, 0};
    return dqp_al_mpc_solve_bounds(d, dyn_id, dt, al_iter, newton_steps, x_init, u_init, x0, Qdiag, q, &bd, lam_in, rho_in,
                                   prev_cost, prev_lam, prev_rho, n_prev, xu, hist_cost, hist_lam, hist_rho, res_norm, factor,
                                   status, fail, workspace, stream);
}

// Behind either front check; v.lam / v.rho: lam_in / rho_in.  The model is not checked here: the first Newton solve
// refuses an unregistered one, behind the start kernel.
static int mpc_solve(const AlProblem &v, const AlMpcIo &io)
{
    if (const int r = v.ready(io.buffers_set()); r != 1) return r;
    if (v.too_large()) return DQP_ERR_TOO_LARGE;
    StartP S = {};
    S.x_init = io.x_init; S.u_init = io.u_init; S.Qd = v.Qd; S.q = v.q; S.lam_in = v.lam; S.rho_in = v.rho;
    S.hist_cost = io.prev_cost; S.hist_lam = io.prev_lam; S.hist_rho = io.prev_rho; S.K = io.n_prev;
    S.xu = io.xu; S.cost0 = io.hist_cost; S.lam0 = io.hist_lam; S.rho0 = io.hist_rho; S.fail = io.fail; S.nfail = io.al_iter;
    S.B = v.B; S.n = v.n; S.m = v.m; S.T = v.T;
    const dim3 start_grid((unsigned)((v.B + 15) / 16));
    if (v.has_x) DQP_LAUNCH(al_start_xbounds_kernel, start_grid, dim3(256), 0, v.stream, S);
    else DQP_LAUNCH(al_start_kernel, start_grid, dim3(256), 0, v.stream, S);
    AlProblem it = v;           // AL iteration i: the multipliers and the penalty of history row i, row i + 1 written
    NewtonIo o = {io.newton_steps, io.xu, io.factor, io.status, io.fail, io.workspace};
    o.clear_fail = false;
    const long long row = v.B, lam_row = v.B * v.ncon();
    for (int i = 0; i < io.al_iter; ++i) {
        it.lam = io.hist_lam + i * lam_row; it.rho = io.hist_rho + i * row;
        o.fail = io.fail + i; o.keep_factor = i == io.al_iter - 1;
        if (const int rc = newton_banded(it, o)) return rc;
        const OutP O = out_args(it, io.xu, io.hist_lam + (i + 1) * lam_row, io.hist_cost + (i + 1) * row, io.res_norm,
                                io.hist_rho + (i + 1) * row);
        if (const int rc = launch_outer(O, v.stream)) return rc;
    }
    return launched();
}

__attribute__((visibility("default"))) int
dqp_al_mpc_solve_bounds(const dqp_al_mpc_dims *d, int dyn_id, double dt, int32_t al_iter, int32_t newton_steps,
                        const double *x_init, const double *u_init, const double *x0, const double *Qdiag, const double *q,
                        const dqp_al_bounds *bounds, const double *lam_in, const double *rho_in,
                        const double *prev_cost, const double *prev_lam, const double *prev_rho, int32_t n_prev,
                        double *xu, double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm, double *factor,
                        double *status, int32_t *fail, void *workspace, void *stream)
{
    const AlMpcIo io = {al_iter, newton_steps, x_init, u_init, prev_cost, prev_lam, prev_rho, n_prev,
                        xu, hist_cost, hist_lam, hist_rho, res_norm, factor, status, fail, workspace};
    if (dqp::al_bounds_check(d, bounds) || !io.scalars_ok()) return DQP_ERR_BAD_ARG;
    return mpc_solve(dqp::al_problem(d, dyn_id, dt, x0, Qdiag, q, lam_in, rho_in, bounds, nullptr, stream), io);
}

__attribute__((visibility("default"))) int
dqp_al_mpc_solve_xbounds(const dqp_al_mpc_dims *d, int model, double dt, int32_t al_iter, int32_t newton_steps,
                         const double *x_init, const double *u_init, const double *x0, const double *Qdiag, const double *q,
                         const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, const double *lam_in,
                         const double *rho_in, const double *prev_cost, const double *prev_lam, const double *prev_rho,
                         int32_t n_prev, double *xu, double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm,
                         double *factor, double *status, int32_t *fail, void *workspace, void *stream)
{
    const AlMpcIo io = {al_iter, newton_steps, x_init, u_init, prev_cost, prev_lam, prev_rho, n_prev,
                        xu, hist_cost, hist_lam, hist_rho, res_norm, factor, status, fail, workspace};
    if (const int rc = al_xbounds_check(d, bounds, xbounds, d && dyn::model_matches(model, d->n_state, d->n_ctrl))) return rc;
    if (!io.scalars_ok()) return DQP_ERR_BAD_ARG;
    return mpc_solve(dqp::al_problem(d, model, dt, x0, Qdiag, q, lam_in, rho_in, bounds, xbounds, stream), io);
}

}  // extern "C"
