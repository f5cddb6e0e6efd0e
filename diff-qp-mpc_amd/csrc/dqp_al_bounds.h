// dqp_al_bounds.h -- the bound layout of the AL kernels (include/dqp.h: dqp_al_bounds), shared by dqp_al.hip,
// the banded kernels (dqp_al_banded_kernels.h) and dqp_al_fused.hip.
//
// A kernel template instantiated on StridedBounds<Map> reads the control bounds of sample b, knot t, control k at
// [b stride_b + t stride_t + k]; instantiated on the plain Map it reads the n_ctrl-vector as it always did: the strided
// addressing sits behind `if constexpr`, so the vector instantiations keep their names and their instruction stream
// (DESIGN.md §4.7.1 has the disassembly comparison).  The strided ones load a knot's bounds once per knot, next to the
// knot's multipliers -- never inside the substitution sweeps.
#ifndef DQP_AL_BOUNDS_H_
#define DQP_AL_BOUNDS_H_
#include <stdint.h>

#include "../../include/dqp.h"

namespace dqp {

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
