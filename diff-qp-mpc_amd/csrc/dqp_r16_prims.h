// dqp_r16_prims.h -- DPP-row building blocks shared by the 4-QPs-per-wavefront kernels.
//
// Conventions: a QP owns one 16-lane DPP row (r = lane & 15).  "Row-distributed" matrix: row i
// on lane i % 16, slot i / 16, all columns in consecutive VGPRs (double M[S][NC]).
// "Distributed" vector: element i on lane i % 16, slot i / 16 (double v[S]).  Every loop over a
// register index is fully unrolled, so all indices are compile-time constants.
#ifndef DQP_R16_PRIMS_H_
#define DQP_R16_PRIMS_H_
#include <hip/hip_runtime.h>
#include <math.h>

#include "dqp_common.h"

namespace dqp {
namespace r16 {

// ------------------------------------------------------------------ cross-lane primitives
template <int CTRL> __device__ __forceinline__ double dppd(double v)
{
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, true);
}

// value of lane k (0..15) of each DPP row, in every lane of that row.  k folds to a constant
// after unrolling, leaving a single v_mov_b64_dpp row_newbcast:k.
__device__ __forceinline__ double rb(double v, int k)
{
    switch (k & 15) {
    case 0: return dppd<0x150>(v);   case 1: return dppd<0x151>(v);
    case 2: return dppd<0x152>(v);   case 3: return dppd<0x153>(v);
    case 4: return dppd<0x154>(v);   case 5: return dppd<0x155>(v);
    case 6: return dppd<0x156>(v);   case 7: return dppd<0x157>(v);
    case 8: return dppd<0x158>(v);   case 9: return dppd<0x159>(v);
    case 10: return dppd<0x15a>(v);  case 11: return dppd<0x15b>(v);
    case 12: return dppd<0x15c>(v);  case 13: return dppd<0x15d>(v);
    case 14: return dppd<0x15e>(v);  default: return dppd<0x15f>(v);
    }
}
#define BC(vec, k) rb((vec)[(k) >> 4], (k) & 15)   /* element k of a distributed vector */

__device__ __forceinline__ double row_sum(double v)
{
    v += dppd<0x128>(v); v += dppd<0x124>(v); v += dppd<0x122>(v); v += dppd<0x121>(v);
    return v;
}
__device__ __forceinline__ double row_min(double v)
{
    v = fmin(v, dppd<0x128>(v)); v = fmin(v, dppd<0x124>(v));
    v = fmin(v, dppd<0x122>(v)); v = fmin(v, dppd<0x121>(v));
    return v;
}

__device__ __forceinline__ double row_max(double v)
{
    v = fmax(v, dppd<0x128>(v)); v = fmax(v, dppd<0x124>(v));
    v = fmax(v, dppd<0x122>(v)); v = fmax(v, dppd<0x121>(v));
    return v;
}

// ------------------------------------------------------------------ lane groups of 16 or 32
// Cross-lane primitives over the G lanes of one problem.  G = 16: the DPP row ones.  G = 32 (two rows):
// the row's own DPP result, then v_permlane16_swap of two copies of it, which swaps the odd rows of the
// first with the even rows of the second -- the first then holds row 0's value of each half-wavefront,
// the second row 1's, in all 32 lanes of the half (the compiler places the VALU-write wait states).
__device__ __forceinline__ void half_rows(double x, double &row0, double &row1)
{
    const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(x), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(x), false, false);
    row0 = __hiloint2double(hi[0], lo[0]);
    row1 = __hiloint2double(hi[1], lo[1]);
}
// value of lane k of the problem's lanes, in all of them (k a compile-time constant after unrolling)
template <int G> __device__ __forceinline__ double bc(double v, int k)
{
    if constexpr (G == 16) return rb(v, k);
    double a, b;
    half_rows(rb(v, k & 15), a, b);
    return k < 16 ? a : b;
}
template <int G> __device__ __forceinline__ double gsum(double v)
{
    if constexpr (G == 16) return row_sum(v);
    double a, b;
    half_rows(row_sum(v), a, b);
    return a + b;
}
template <int G> __device__ __forceinline__ double gmin(double v)
{
    if constexpr (G == 16) return row_min(v);
    double a, b;
    half_rows(row_min(v), a, b);
    return fmin(a, b);
}

// Pins a value's definition where it is written: without it the compiler may sink a per-step
// `if (r == k) rd = x` select to the first use of rd, keeping all N candidates x alive (60 VGPRs
// through the next phase) -- seen in the null-space backward kernel: 5.7 KB/lane of spills.
#define PIN(x) asm volatile("" : "+v"(x))

// keep ? v : (v with its high word cleared).  The cleared value is 0 or a positive denormal
// below 2^-1042, which every FMA on normal-range data absorbs exactly -- one v_cndmask instead of
// the two a full 64-bit select costs (these kernels issue one instruction per 4 cycles, so
// predication selects were ~20 % of the PDIPM iteration).
__device__ __forceinline__ double mask_hi(double v, bool keep)
{
    return __hiloint2double(keep ? __double2hiint(v) : 0, __double2loint(v));
}

// full-precision reciprocal / reciprocal square root from the hardware estimates + 2 Newton steps
__device__ __forceinline__ double frcp(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double frsqrt(double d)
{
    double y = __builtin_amdgcn_rsq(d);
    y = y * fma(-0.5 * d * y, y, 1.5);
    y = y * fma(-0.5 * d * y, y, 1.5);
    return y;
}

// Diagnostic phase stamps: compiled in only with -DDQP_STAMPS (tools/stamps.py builds that
// variant itself).  Even a never-taken stamp branch perturbs register allocation of the
// fully unrolled kernels by 2-3x, so the shipped build contains none.
#if defined(DQP_MARKS)   /* asm comments at the phase boundaries, for reading the .s */
#define DQP_STR2(x) #x
#define DQP_STR(x) DQP_STR2(x)
#define STAMP(P, i) asm volatile("; DQPMARK " DQP_STR(i))
#elif defined(DQP_SETUP_STOP)   /* measurement builds (tools/setup_phases.py): the wavefront ends at phase boundary DQP_SETUP_STOP */
#define STAMP(P, i)                                                                  \
    do {                                                                             \
        if ((i) == DQP_SETUP_STOP) {                                                 \
            const double a__ = stop_sum<DQP_SETUP_STOP>(st);                         \
            (P).zhat[qp * 2 + (r & 1)] = a__;                                        \
            __builtin_amdgcn_endpgm();                                               \
        }                                                                            \
    } while (0)
#elif !defined(DQP_STAMPS)
#define STAMP(P, i) do { } while (0)
#else
#define STAMP(P, i)                                                                  \
    do {                                                                             \
        if ((P).stamps) {                                                            \
            __builtin_amdgcn_sched_barrier(0);                                       \
            const unsigned long long t__ = __builtin_readcyclecounter();             \
            if (threadIdx.x == 0) (P).stamps[blockIdx.x * 16 + (i)] = t__;           \
            __builtin_amdgcn_sched_barrier(0);                                       \
        }                                                                            \
    } while (0)
#endif

constexpr __host__ __device__ int slots(int n) { return (n + 15) / 16; }
constexpr __host__ __device__ int tri(int i) { return i * (i + 1) / 2; }

// ------------------------------------------------------------------ mat-vec building blocks
// y[s] (+)= sum_j M[s][j] * x_j          (M row-distributed SR x NC, x distributed length NC)
template <int SR, int NC, int SX>
__device__ __forceinline__ void mv_nat(const double (&Mx)[SR][NC], const double (&x)[SX],
                                       double (&y)[SR], bool accumulate)
{
    if (!accumulate) {
#pragma unroll
        for (int s = 0; s < SR; ++s) y[s] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const double xb = BC(x, j);
#pragma unroll
        for (int s = 0; s < SR; ++s) y[s] = fma(Mx[s][j], xb, y[s]);
    }
}

// Reduce-scatter over the 16 lanes of a DPP row: on entry every lane holds its partials v[k]
// of 16 column sums; the return value on lane k is the total of column k.  Four mirror
// butterflies (row_mirror, row_half_mirror, quad reverse, quad swap) halve the live values.
__device__ __forceinline__ double reduce_scatter16(const double (&v)[16], int r)
{
    const bool h8 = (r & 8) != 0, h4 = (r & 4) != 0, h2 = (r & 2) != 0, h1 = (r & 1) != 0;
    double a[8], b4[4], c2[2];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double keep = h8 ? v[k + 8] : v[k], send = h8 ? v[k] : v[k + 8];
        a[k] = keep + dppd<0x140>(send);                 // row_mirror: l <-> 15-l
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double keep = h4 ? a[k + 4] : a[k], send = h4 ? a[k] : a[k + 4];
        b4[k] = keep + dppd<0x141>(send);                // row_half_mirror: l <-> 7-l
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double keep = h2 ? b4[k + 2] : b4[k], send = h2 ? b4[k] : b4[k + 2];
        c2[k] = keep + dppd<0x1b>(send);                 // quad_perm [3,2,1,0]
    }
    const double keep = h1 ? c2[1] : c2[0], send = h1 ? c2[0] : c2[1];
    return keep + dppd<0xb1>(send);                      // quad_perm [1,0,3,2]
}

// y = M^T v   (M row-distributed SR x NC, v distributed over the rows; y distributed length NC)
template <int SR, int NC, int SY>
__device__ __forceinline__ void mv_tr(const double (&Mx)[SR][NC], const double (&v)[SR],
                                      double (&y)[SY], int r)
{
#pragma unroll
    for (int g = 0; g < SY; ++g) {
        double p[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = 16 * g + k;
            if (c < NC) {
                double a = Mx[0][c < NC ? c : 0] * v[0];
#pragma unroll
                for (int s = 1; s < SR; ++s) a = fma(Mx[s][c < NC ? c : 0], v[s], a);
                p[k] = a;
            } else {
                p[k] = 0.0;
            }
        }
        y[g] = reduce_scatter16(p, r);
    }
}

// ------------------------------------------------------------------ factorizations in registers
// Lower Cholesky of the row-distributed SPD matrix (in place; strict upper part zeroed).
// rd[s] = 1/L[i][i] for the lane's rows.  Returns false on a pivot that is not positive, or --
// with reltol > 0 -- that has collapsed below reltol x the largest pivot seen (a numerically
// singular matrix: duplicated / dependent equality rows give a round-off-sized positive pivot).
template <int S, int N>
__device__ __forceinline__ bool chol_rows(double (&L)[S][N], double (&rd)[S], int r, double reltol = 0.0)
{
    bool ok = true;
    double pmax = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) rd[s] = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int sk = k >> 4, lk = k & 15;
        double dk = rb(L[sk][k], lk);
        if (!(dk > reltol * pmax)) { ok = false; dk = 1.0; }
        pmax = fmax(pmax, dk);
        const double ri = frsqrt(dk);
        if (r == lk) rd[sk] = ri;
        PIN(rd[sk]);
        double col[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s + 15 < k) col[s] = 0.0;                              // rows all above k
            else if (16 * s >= k) col[s] = L[s][k] * ri;                    // rows all >= k
            else col[s] = (r >= lk) ? L[s][k] * ri : 0.0;
            L[s][k] = col[s];
        }
#pragma unroll
        for (int j = k + 1; j < N; ++j) {
            const double cj = BC(col, j);
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (16 * s + 15 >= j) L[s][j] = fma(-col[s], cj, L[s][j]);   // only rows i >= j matter
        }
    }
    return ok;
}

// The factorisation below has one form: the look-ahead pivot chain and the folded right-hand side both won their
// measurements against the plain order, with bit-identical results.  Timing a further variant needs
// no switch in this file: tools/ab_variants.py builds one from a source file kept outside the tree.

// ties the scheduling of two independent values together: whatever consumes the outputs comes after
// everything that produced either input (the look-ahead pivot chain is spread over the trailing
// column updates this way -- the scheduler would otherwise pull the chain together again)
#define PIN2(x, y) asm volatile("" : "+v"(x), "+v"(y))

// Unpivoted LU of the row-distributed matrix (in place: unit-lower multipliers below the
// diagonal, U on/above).  rdu[s] = 1/U[i][i].
//
// Look-ahead: step k updates column k+1 first and takes the next pivot's reciprocal from it --
// broadcast, v_rcp_f64 and the four refinement FMAs of frcp, one link after each of the following
// column updates -- so the chain's latency and the DPP-after-VALU wait states hide under the rest
// of the trailing update instead of standing in front of step k+1.  Same operations on the same
// values as the plain order.
//
// RHS: the L sweep of lu_solve (L y = b) rides along as one more column of the trailing update,
// with lu_solve's own expressions and masks: at step k < N-1, b[s] = fma(-L[s][k], bcast(b[k]), b[s]).
// For a right-hand side known before the factorisation this takes the sweep's N-1 dependent
// broadcast+FMA links off the critical path; lu_solve_U finishes the solve.
template <int S, int N, bool RHS>
__device__ __forceinline__ void lu_rows_impl(double (&T)[S][N], double (&rdu)[S], double (&b)[S], int r)
{
#pragma unroll
    for (int s = 0; s < S; ++s) rdu[s] = 0.0;
    double rp = frcp(rb(T[0][0], 0));
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int sk = k >> 4, lk = k & 15;
        if (r == lk) rdu[sk] = rp;
        PIN(rdu[sk]);
        double l[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s + 15 <= k) l[s] = 0.0;
            else if (16 * s > k) { l[s] = T[s][k] * rp; T[s][k] = l[s]; }
            else { const bool a = r > lk; l[s] = mask_hi(T[s][k], a) * rp; T[s][k] = a ? l[s] : T[s][k]; }
        }
        // the next pivot's chain: d (stage 0) -> rcp estimate -> e, refined -> e, refined
        double pd = 0.0, pr = 0.0, pe = 0.0;
        int stage = 0;
#pragma unroll
        for (int j = k + 1; j < N; ++j) {
            const double ub = rb(T[sk][j], lk);
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (16 * s + 15 > k) T[s][j] = fma(-l[s], ub, T[s][j]);
            if (RHS && j == k + 1) {                   // L y = b, step k (lu_solve's expressions)
                const double bk = BC(b, k);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (16 * s + 15 <= k) continue;
                    if (16 * s > k) b[s] = fma(-T[s][k], bk, b[s]);
                    else b[s] = fma(-mask_hi(T[s][k], r > lk), bk, b[s]);
                }
            }
            if (j >= k + 2 && stage < 6) {             // one link per column from k+2 on
                double &tj = T[S - 1][j];              // (a slot that every step still updates)
                if (stage == 0) { PIN2(tj, T[(k + 1) >> 4][k + 1]); pd = rb(T[(k + 1) >> 4][k + 1], (k + 1) & 15); }
                else if (stage == 1) { PIN2(tj, pd); pr = __builtin_amdgcn_rcp(pd); }
                else if (stage & 1) { PIN2(tj, pe); pr = fma(pe, pr, pr); }
                else { PIN2(tj, pr); pe = fma(-pd, pr, 1.0); }
                ++stage;
            }
        }
        if (k + 1 < N) {                               // what the remaining columns were too few for
            if (stage == 0) { pd = rb(T[(k + 1) >> 4][k + 1], (k + 1) & 15); ++stage; }
            if (stage == 1) { pr = __builtin_amdgcn_rcp(pd); ++stage; }
#pragma unroll
            for (; stage < 6; ++stage) {
                if (stage & 1) pr = fma(pe, pr, pr);
                else pe = fma(-pd, pr, 1.0);
            }
            rp = pr;
        }
    }
}

template <int S, int N>
__device__ __forceinline__ void lu_rows(double (&T)[S][N], double (&rdu)[S], int r)
{
    double none[S];            // lu_rows_impl<RHS = false> never touches b: dead after inlining
#pragma unroll
    for (int s = 0; s < S; ++s) none[s] = 0.0;
    lu_rows_impl<S, N, false>(T, rdu, none, r);
}

// b <- U^-1 y: the U sweep and the final scaling of lu_solve.  A lane keeps its own y_k unscaled (the
// pivot scaling is applied to the broadcast copy and, once, to the whole vector at the end), so the
// only per-step predication is the one-instruction triangle mask.
template <int S, int N>
__device__ __forceinline__ void lu_solve_U(const double (&T)[S][N], const double (&rdu)[S],
                                           double (&b)[S], int r)
{
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {                 // U x = y
        const int sk = k >> 4, lk = k & 15;
        const double xk = rb(b[sk] * rdu[sk], lk);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s > k) continue;
            if (16 * s + 15 < k) b[s] = fma(-T[s][k], xk, b[s]);
            else b[s] = fma(-mask_hi(T[s][k], r < lk), xk, b[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) b[s] *= rdu[s];
}

// b <- T^-1 b with the LU above.
template <int S, int N>
__device__ __forceinline__ void lu_solve(const double (&T)[S][N], const double (&rdu)[S],
                                         double (&b)[S], int r)
{
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {                  // L y = b
        const int lk = k & 15;
        const double bk = BC(b, k);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s + 15 <= k) continue;
            if (16 * s > k) b[s] = fma(-T[s][k], bk, b[s]);
            else b[s] = fma(-mask_hi(T[s][k], r > lk), bk, b[s]);
        }
    }
    lu_solve_U<S, N>(T, rdu, b, r);
}

// lu_rows, and b <- L^-1 b along the way (lu_solve_U completes b <- T^-1 b)
template <int S, int N>
__device__ __forceinline__ void lu_rows_rhs(double (&T)[S][N], double (&rdu)[S], double (&b)[S], int r)
{
    lu_rows_impl<S, N, true>(T, rdu, b, r);
}

// factor + solve for a right-hand side known before the factorisation: b <- T^-1 b, the L sweep folded into
// the factorisation (the same values as the pair lu_rows + lu_solve)
template <int S, int N>
__device__ __forceinline__ void lu_factor_solve(double (&T)[S][N], double (&rdu)[S], double (&b)[S], int r)
{
    lu_rows_rhs<S, N>(T, rdu, b, r);
    lu_solve_U<S, N>(T, rdu, b, r);
}

// b <- L^-1 b, L lower triangular row-distributed in registers (rd = reciprocal diagonal)
template <int S, int N>
__device__ __forceinline__ void trsv_rows(const double (&L)[S][N], const double (&rd)[S],
                                          double (&b)[S], int r)
{
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int sk = k >> 4, lk = k & 15;
        const double yk = rb(b[sk] * rd[sk], lk);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s + 15 < k) continue;
            if (16 * s > k) b[s] = fma(-L[s][k], yk, b[s]);
            else b[s] = (r == lk) ? yk : fma(r > lk ? -L[s][k] : 0.0, yk, b[s]);
        }
    }
}

// ------------------------------------------------------------------ packed-triangle LDS helpers
// LDS holds, per QP, the packed lower triangle P[tri(i) + j], j <= i.
template <int S, int N>
__device__ __forceinline__ void tri_store(double *P, const double (&L)[S][N], int r, double *dummy)
{
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int i = r + 16 * s;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (j > 16 * s + 15) continue;
            double *dst = (i < N && j <= i) ? P + tri(i) + j : dummy;
            *dst = L[s][j];
        }
    }
}

// The LDS operand prefetch.  With one wavefront per SIMD nothing else runs while a wave sits in
// s_waitcnt lgkmcnt for an operand it asked for just in time, so outside the iteration loop the LDS operands
// of a dependent chain are fetched ahead of it: the triangular solves keep a ring of TRI_RING columns in
// flight, the reflector chains the next reflector's tail, the row solves of the setup the next 8 entries.
// The plain forms (D = 0 below; each entry read where it is used, bit-identical in their results) stay for the
// sizes whose kernels have no register to hold an operand ahead of its use: a kernel Cfg picks by size (Cfg::PF).
constexpr int TRI_RING = 4;    /* columns ahead: RING x one step's DPP chain (~18 cycles) > the LDS round trip */

// Orders a prefetch: every LDS read issued above stays above, whatever consumes x comes below (an LDS read
// is ordered against the "memory" clobber, the arithmetic through x -- a scheduling barrier alone orders
// only the reads, see dqp_r16n.hip).  No instruction.
__device__ __forceinline__ void after_reads(double &x) { asm volatile("" : "+v"(x) : : "memory"); }

// the lane's entries of column k of the packed triangle (rows >= k; slots wholly above k are not read)
template <int S, int N>
__device__ __forceinline__ void tri_col(const double *P, double (&c)[S], int k, int r)
{
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (16 * s + 15 < k) { c[s] = 0.0; continue; }
        const int i = r + 16 * s;
        const int ic = i < N ? i : N - 1;
        c[s] = P[tri(ic) + (k <= ic ? k : 0)];
    }
}

// Column k leaves the ring here: without this the selects that mask the entries (they depend on nothing else)
// are scheduled right behind the read, and the wait with them.
template <int S> __device__ __forceinline__ void ring_use(double (&c)[S], int k)
{
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (16 * s + 15 >= k) PIN(c[s]);
}

// y = L x with L the packed lower triangle in LDS (x, y distributed length N)
template <int S, int N, int D = TRI_RING>
__device__ __forceinline__ void tri_mv(const double *P, const double (&x)[S], double (&y)[S], int r)
{
#pragma unroll
    for (int s = 0; s < S; ++s) y[s] = 0.0;
    if constexpr (D == 0) {                         // the plain form: each entry read where it is used
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double xb = BC(x, j);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (16 * s + 15 < j) continue;
                const int i = r + 16 * s;
                const int ic = i < N ? i : N - 1;
                const double v = P[tri(ic) + (j <= ic ? j : 0)];
                y[s] = fma(mask_hi(v, j <= i && i < N), xb, y[s]);
            }
        }
        return;
    }
    constexpr int DR = D > 0 ? D : 1;
    double ring[DR][S];
#pragma unroll
    for (int j = 0; j < D && j < N; ++j) tri_col<S, N>(P, ring[j], j, r);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double col[S];
#pragma unroll
        for (int s = 0; s < S; ++s) col[s] = ring[j % DR][s];
        if (j + D < N) tri_col<S, N>(P, ring[j % DR], j + D, r);
        after_reads(y[S - 1]);
        ring_use<S>(col, j);
        const double xb = BC(x, j);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s + 15 < j) continue;
            const int i = r + 16 * s;
            y[s] = fma(mask_hi(col[s], j <= i && i < N), xb, y[s]);
        }
    }
}

// b <- L^-1 b with L packed in LDS (forward substitution; rd distributed reciprocal diagonal)
template <int S, int N, int D = TRI_RING>
__device__ __forceinline__ void tri_solve(const double *P, const double (&rd)[S], double (&b)[S], int r)
{
    if constexpr (D == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int sk = k >> 4, lk = k & 15;
            const double yk = rb(b[sk] * rd[sk], lk);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (16 * s + 15 < k) continue;
                const int i = r + 16 * s;
                const int ic = i < N ? i : N - 1;
                const double v = P[tri(ic) + (k <= ic ? k : 0)];
                if (16 * s > k) b[s] = fma((i < N) ? -v : 0.0, yk, b[s]);
                else b[s] = (r == lk) ? yk : fma((r > lk && i < N) ? -v : 0.0, yk, b[s]);
            }
        }
        return;
    }
    constexpr int DR = D > 0 ? D : 1;
    double ring[DR][S];
#pragma unroll
    for (int k = 0; k < D && k < N; ++k) tri_col<S, N>(P, ring[k], k, r);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int sk = k >> 4, lk = k & 15;
        double col[S];
#pragma unroll
        for (int s = 0; s < S; ++s) col[s] = ring[k % DR][s];
        if (k + D < N) tri_col<S, N>(P, ring[k % DR], k + D, r);
        after_reads(b[sk]);
        ring_use<S>(col, k);
        const double yk = rb(b[sk] * rd[sk], lk);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s + 15 < k) continue;
            const int i = r + 16 * s;
            const double v = col[s];
            if (16 * s > k) b[s] = fma((i < N) ? -v : 0.0, yk, b[s]);
            else b[s] = (r == lk) ? yk : fma((r > lk && i < N) ? -v : 0.0, yk, b[s]);
        }
    }
}

// b <- L^-T b with L packed in LDS: x_j = (b_j - sum_{i>j} L[i][j] x_i) / L[j][j]; the sum over
// rows is a row reduction (the transposed access pattern of row-distributed storage).
template <int S, int N, int D = TRI_RING>
__device__ __forceinline__ void tri_solve_T(const double *P, const double (&rd)[S], double (&b)[S], int r)
{
    if constexpr (D == 0) {
#pragma unroll
        for (int j = N - 1; j >= 0; --j) {
            const int sj = j >> 4, lj = j & 15;
            double part = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (16 * s + 15 <= j) continue;
                const int i = r + 16 * s;
                const int ic = i < N ? i : N - 1;
                const double v = P[tri(ic) + (j <= ic ? j : 0)];
                part = fma((i > j && i < N) ? v : 0.0, b[s], part);
            }
            const double tot = row_sum(part);
            if (r == lj) b[sj] = (b[sj] - tot) * rd[sj];
        }
        return;
    }
    constexpr int DR = D > 0 ? D : 1;
    double ring[DR][S];
#pragma unroll
    for (int j = N - 1; j > N - 1 - D && j >= 0; --j) tri_col<S, N>(P, ring[j % DR], j, r);
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
        const int sj = j >> 4, lj = j & 15;
        double col[S];
#pragma unroll
        for (int s = 0; s < S; ++s) col[s] = ring[j % DR][s];
        if (j - D >= 0) tri_col<S, N>(P, ring[j % DR], j - D, r);
        after_reads(b[S - 1]);
        ring_use<S>(col, j);
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (16 * s + 15 <= j) continue;
            const int i = r + 16 * s;
            part = fma((i > j && i < N) ? col[s] : 0.0, b[s], part);
        }
        const double tot = row_sum(part);
        if (r == lj) b[sj] = (b[sj] - tot) * rd[sj];
    }
}

// distributed vector <-> LDS (each lane touches only its own elements: no barrier needed)
template <int S>
__device__ __forceinline__ void vec_put(double *P, const double (&v)[S], int n, int r, double *dummy)
{
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int i = r + 16 * s;
        double *dst = i < n ? P + i : dummy;
        *dst = v[s];
    }
}
template <int S>
__device__ __forceinline__ void vec_get(const double *P, double (&v)[S], int n, int r)
{
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int i = r + 16 * s;
        const double x = P[i < n ? i : n - 1];
        v[s] = i < n ? x : 0.0;
    }
}

// Row-distributed load of an nrows x NC matrix (rows beyond nrows are zero).
template <int S, int NC>
__device__ __forceinline__ void load_rows(const double *src, int nrows, double (&dst)[S][NC], int r)
{
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int i = r + 16 * s;
        const double *row = src + (i < nrows ? i : nrows - 1) * NC;
        const double keep = i < nrows ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < NC; ++j) dst[s][j] = row[j];
        if (16 * s + 15 >= nrows) {
#pragma unroll
            for (int j = 0; j < NC; ++j) dst[s][j] *= keep;
        }
    }
}

// ------------------------------------------------------------------ Schur complement factor
// (C: a kernel Cfg with M, SM, oR, oDummy)
// T = R + diag(dinv) (full square, row-distributed) from the packed triangle in LDS (load_T), then LU.
// Each lane first rewrites its own diagonal entries of the LDS triangle with R_ii + dinv_i (only
// the owning lane ever reads them back), so the load needs no per-element diagonal select.
template <class C>
__device__ __forceinline__ void load_T(double *lds, double (&T)[C::SM][C::M],
                                       const double (&rdiag)[C::SM], const double (&dinv)[C::SM], int r)
{
    constexpr int M = C::M, SM = C::SM;
    double *Rp = lds + C::oR;
#pragma unroll
    for (int s = 0; s < SM; ++s) {
        const int i = r + 16 * s;
        double *dst = i < M ? Rp + tri(i) + i : lds + C::oDummy + r;
        *dst = rdiag[s] + dinv[s];
    }
#pragma unroll
    for (int s = 0; s < SM; ++s) {
        const int i = r + 16 * s;
        const int ic = i < M ? i : M - 1;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            int off;
            if (16 * s > j) off = tri(ic) + j;                          // all rows below column j
            else if (16 * s + 15 < j) off = tri(j) + ic;                // all rows above
            else off = (j <= ic) ? tri(ic) + j : tri(j) + ic;
            const double v = Rp[off];
            T[s][j] = (16 * s + 15 >= M) ? mask_hi(v, i < M) : v;       // pad rows: ~zero rows
        }
    }
}

template <class C>
__device__ __forceinline__ void factor_T(double *lds, double (&T)[C::SM][C::M],
                                         const double (&rdiag)[C::SM], const double (&dinv)[C::SM],
                                         double (&rdu)[C::SM], int r)
{
    load_T<C>(lds, T, rdiag, dinv, r);
    lu_rows<C::SM, C::M>(T, rdu, r);
}

// factor_T and b <- T^-1 b in one (the L sweep inside the factorisation)
template <class C>
__device__ __forceinline__ void factor_T_rhs(double *lds, double (&T)[C::SM][C::M],
                                             const double (&rdiag)[C::SM], const double (&dinv)[C::SM],
                                             double (&rdu)[C::SM], double (&b)[C::SM], int r)
{
    load_T<C>(lds, T, rdiag, dinv, r);
    lu_factor_solve<C::SM, C::M>(T, rdu, b, r);
}

}  // namespace r16
}  // namespace dqp
#endif
