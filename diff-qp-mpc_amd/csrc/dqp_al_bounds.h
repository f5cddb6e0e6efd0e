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

// DQP_OK for a layout the kernels take (include/dqp.h), else DQP_ERR_BAD_ARG.  Pointers are the caller's to check, behind
// its nbatch == 0 return.
inline int al_bounds_layout(const dqp_al_bounds *b, const dqp_al_mpc_dims *d)
{
    if (!b || !d || d->n_ctrl <= 0 || d->T <= 0) return DQP_ERR_BAD_ARG;
    const int64_t m = d->n_ctrl, Tm = (int64_t)d->T * m;
    if (b->stride_t != 0 && b->stride_t != m) return DQP_ERR_BAD_ARG;
    if (b->stride_b != 0 && b->stride_b != Tm && !(b->stride_t == 0 && b->stride_b == m)) return DQP_ERR_BAD_ARG;
    return DQP_OK;
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
