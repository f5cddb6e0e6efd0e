// dqp_al_bounds.h -- what the AL kernels of dqp_al.hip, the banded kernels (dqp_al_banded_kernels.h) and dqp_al_fused.hip
// agree on: the bound layout (include/dqp.h: dqp_al_bounds), the row layout of the constraint vector (AlRows) and each
// formula of the merit function, the multiplier update, the line search and the warm start, once.
//
// A kernel template instantiated on StridedBounds<Map> reads the control bounds of sample b, knot t, control k at
// [b stride_b + t stride_t + k]; instantiated on the plain Map it reads the n_ctrl-vector: the strided addressing sits
// behind `if constexpr`, so the vector instantiations keep their names and never read the strides, which every argument
// struct carries (their registers, LDS, results and times against the structs without them).  The
// strided ones load a knot's bounds once per knot, next to the knot's multipliers -- never inside the substitution sweeps.
#ifndef DQP_AL_BOUNDS_H_
#define DQP_AL_BOUNDS_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dqp.h"

namespace dqp {

// line-search candidates xu + 2^-k upd, k = 0 .. 19 (al_utils.py:503-527)
constexpr int AL_NCAND = 20;

// The rows of the constraint vector (multipliers, residuals) of one problem:
//   [0, T n)                  equalities: knot t < T - 1 the dynamics residual x_{t+1} - f(x_t, u_t), knot T - 1 x_0 - x0
//   then per knot 2 m rows    control pairs [u - u_upper (m), u_lower - u (m)]
//   then per knot 2 n rows    state pairs [x - x_upper (n), x_lower - x (n)], with a state box only
// eq / ctrl / state give a knot's first row: element j of it is + j, the lower half of a pair + m or + n more.
// I: int in the kernels; long long where the host sizes buffers from dims it has not bounded yet (AlProblem::ncon).
template <class I> struct AlRowsT {
    I n, m, T;
    bool xbox;
    __host__ __device__ constexpr I neq() const { return T * n; }
    __host__ __device__ constexpr I ncon() const { return neq() + 2 * T * m + (xbox ? 2 * T * n : 0); }
    __host__ __device__ constexpr I eq(I t) const { return t * n; }
    __host__ __device__ constexpr I ctrl(I t) const { return neq() + t * 2 * m; }
    __host__ __device__ constexpr I state(I t) const { return neq() + 2 * T * m + t * 2 * n; }
};
using AlRows = AlRowsT<int>;

// ---- the formulas, on values: the call sites keep their loops, their registers and where they load

// cost of one element of the trajectory, diagonal Q: (Qd z / 2 + q) z
__device__ __forceinline__ double al_cost_term(double qd, double ql, double z) { return (0.5 * qd * z + ql) * z; }
// merit share of an equality row (al_utils.py:37-59): lam res + rho / 2 res^2
__device__ __forceinline__ double al_eq_term(double rho, double lam, double res) { return (0.5 * rho * res + lam) * res; }
// |res_clamp|^2 of a bound pair, hi = v - upper, lo = lower - v
__device__ __forceinline__ double al_pair_sq(double hi, double lo)
{
    return fmax(hi, 0.0) * fmax(hi, 0.0) + fmax(lo, 0.0) * fmax(lo, 0.0);
}
// merit share of a bound pair
__device__ __forceinline__ double al_pair_term(double rho, double lam_up, double lam_lo, double hi, double lo)
{
    return lam_up * hi + lam_lo * lo + 0.5 * rho * al_pair_sq(hi, lo);
}
// multiplier update of a bound pair, clamped at 0 (AL_mpc.py:300-301), with the pair's share of |res_clamp|^2
struct AlPairUpdate { double up, lo, sq; };
__device__ __forceinline__ AlPairUpdate al_pair_update(double rho, double lam_up, double lam_lo, double hi, double lo)
{
    return {fmax(lam_up + rho * hi, 0.0), fmax(lam_lo + rho * lo, 0.0), al_pair_sq(hi, lo)};
}
// where the bounds of (sample b, knot t, element i) lie in lower / upper: strided (SB) at [b sb + t st + i], else element i of
// the vector.  The index, not the value: the loads stay where the kernel placed them.
template <bool SB> __device__ __forceinline__ long long al_bound_at(long long b, int t, int i, long long sb, long long st)
{
    if constexpr (SB) return b * sb + t * st + i;
    else return i;
}
// step of candidate k: 2^-k in float, as the reference
__device__ __forceinline__ double al_step(int k) { return (double)exp2f(-(float)k); }

// torch.min over the candidates of a wavefront, lane k holding candidate k (`has`; v = INFINITY elsewhere): NaN wins,
// else the first minimum
struct AlBest { int arg; double merit; };
__device__ __forceinline__ AlBest al_wave_argmin(double v, bool has)
{
    const unsigned long long nanmask = __builtin_amdgcn_ballot_w64(has && v != v);
    double m = (v != v) ? INFINITY : v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
    const unsigned long long eq = __builtin_amdgcn_ballot_w64(has && v == m);
    const int arg = nanmask ? (int)__builtin_ctzll(nanmask) : (eq ? (int)__builtin_ctzll(eq) : 0);
    return {arg, __shfl(v, arg, 64)};
}

// Warm start of (lam, rho) from the previous call's K history rows, oldest first (al_utils.warm_start_al, al_utils.py:16-34):
// the newest stored AL iterate whose cost was already below cost0, the newest one if none was; lam is rescaled to that
// iterate's norm.  The lanes lane, lane + stride, ... share the ncon rows, `sum` adds over them (a row of 16 or a wavefront).
struct AlWarm { double scale, rho; };
template <class Sum>
__device__ __forceinline__ AlWarm al_warm_start(int K, long long B, long long b, int ncon, double cost0,
                                                const double *hist_cost, const double *hist_lam, const double *hist_rho,
                                                const double *lam, double rho_in, int lane, int stride, Sum sum)
{
    AlWarm w = {1.0, rho_in};
    if (K > 0) {
        int pick = K - 1;                                   // torch.max of an all-False column: index 0 = the newest
        for (int k = K - 1; k >= 0; --k)
            if (hist_cost[(long long)k * B + b] < cost0) { pick = k; break; }
        const double *lh = hist_lam + ((long long)pick * B + b) * ncon;
        double nh = 0.0, nl = 0.0;
        for (int e = lane; e < ncon; e += stride) { nh += lh[e] * lh[e]; nl += lam[e] * lam[e]; }
        w.scale = sqrt(sum(nh)) / sqrt(sum(nl));
        w.rho = hist_rho[(long long)pick * B + b];
    }
    return w;
}

template <class M> struct StridedBounds : M {};
template <class M> struct strided_bounds { static constexpr bool value = false; };
template <class M> struct strided_bounds<StridedBounds<M>> { static constexpr bool value = true; };

// BoxBounds<Map>: a state box is present (the `_xbounds` entry points).  The state bounds of sample b, knot t, state k sit
// at [b xsb + t xst + k] and their rows -- per knot [x - x_upper (n), x_lower - x (n)] -- behind the control rows, at
// [T n + 2 T m + t 2 n ...].  Both boxes use the strided addressing (a vector bound is strides (0, 0)): one family more,
// not two.  Everything it adds to a kernel sits behind `if constexpr (box_bounds<Map>::value)`.
template <class M> struct BoxBounds : M {};
template <class M> struct box_bounds { static constexpr bool value = false; };
template <class M> struct box_bounds<BoxBounds<M>> { static constexpr bool value = true; };
template <class M> struct strided_bounds<BoxBounds<M>> { static constexpr bool value = true; };

// DQP_OK for a layout the kernels take (include/dqp.h), else DQP_ERR_BAD_ARG.  Pointers are the caller's to check, behind
// its nbatch == 0 return.
// `width`: the number of bounds per knot -- n_ctrl for a control box, n_state for a state box.
inline int al_box_layout(const dqp_al_bounds *b, const dqp_al_mpc_dims *d, int width)
{
    if (!b || !d || width <= 0 || d->T <= 0) return DQP_ERR_BAD_ARG;
    const int64_t m = width, Tm = (int64_t)d->T * m;
    if (b->stride_t != 0 && b->stride_t != m) return DQP_ERR_BAD_ARG;
    if (b->stride_b != 0 && b->stride_b != Tm && !(b->stride_t == 0 && b->stride_b == m)) return DQP_ERR_BAD_ARG;
    return DQP_OK;
}
inline int al_bounds_layout(const dqp_al_bounds *b, const dqp_al_mpc_dims *d)
{
    return al_box_layout(b, d, d ? d->n_ctrl : 0);
}
// What every `_xbounds` entry checks in front of its nbatch == 0 return, in this order: sizes and both layouts
// (DQP_ERR_BAD_ARG), the block-tridiagonal kernels' limit (DQP_ERR_TOO_LARGE), the model (`model_ok`: a registered id
// whose sizes are the dims'; DQP_ERR_BAD_ARG).
inline int al_xbounds_check(const dqp_al_mpc_dims *d, const dqp_al_bounds *b, const dqp_al_bounds *xb, bool model_ok)
{
    if (!d || d->nbatch < 0 || d->n_state <= 0 || d->n_ctrl <= 0 || d->T < 2) return DQP_ERR_BAD_ARG;
    if (al_bounds_layout(b, d) != DQP_OK || al_box_layout(xb, d, d->n_state) != DQP_OK) return DQP_ERR_BAD_ARG;
    if (d->n_state + d->n_ctrl > 16 || d->n_state > 12) return DQP_ERR_TOO_LARGE;
    return model_ok ? DQP_OK : DQP_ERR_BAD_ARG;
}
inline bool al_bounds_strided(const dqp_al_bounds *b) { return b->stride_b != 0 || b->stride_t != 0; }

// The same for the MPC QP entry points (dqp_mpc_bounds of include/dqp.h), which take the time-major full layout too:
// (0, 0), (0, m), (m, 0), (m, B m), (T m, m).
inline int mpc_bounds_layout(const dqp_mpc_bounds *b, const dqp_mpc_dims *d)
{
    if (!b || !d || d->n_ctrl <= 0 || d->T <= 0 || d->nbatch < 0) return DQP_ERR_BAD_ARG;
    const int64_t m = d->n_ctrl, Tm = (int64_t)d->T * m, Bm = (int64_t)d->nbatch * m;
    const int64_t sb = b->stride_b, st = b->stride_t;
    const bool ok = (sb == 0 && (st == 0 || st == m)) || (sb == m && (st == 0 || st == Bm)) || (sb == Tm && st == m);
    return ok ? DQP_OK : DQP_ERR_BAD_ARG;
}

}  // namespace dqp
#endif
