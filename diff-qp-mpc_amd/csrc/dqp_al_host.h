// dqp_al_host.h -- the host layer of the augmented-Lagrangian entry points (dqp_al.hip, dqp_al_banded.hip,
// dqp_al_fused.hip), host code only: the view of a problem that every entry builds once from its arguments, the argument
// checks in their two orders, the launch epilogue.  The kernels and their argument structs know nothing of it: each
// struct has one maker, next to the struct, that fills it by member name from the view.
#ifndef DQP_AL_HOST_H_
#define DQP_AL_HOST_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dqp.h"
#include "dqp_dyn_models.h"
#include "dqp_al_bounds.h"

namespace dqp {

// after a DQP_LAUNCH (or several): did the runtime take them
inline int launched() { return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH; }

// What every AL entry receives.  A box is a dqp_al_bounds {lower, upper, stride_b, stride_t}; the state box of an entry
// that has none is all zero (has_x false), and lam then has no state rows.  model 0: caller-linearised dynamics.
struct AlProblem {
    int B, n, m, T, model;
    double dt;
    const double *x0, *Qd, *q, *lam, *rho;
    dqp_al_bounds u, x;
    bool has_x;
    hipStream_t stream;

    int nz() const { return T * (n + m); }
    long long ncon() const { return AlRowsT<long long>{n, m, T, has_x}.ncon(); }
    bool strided() const { return al_bounds_strided(&u); }
    bool model_ok() const { return dyn::model_matches(model, n, m); }
    // beyond the block-tridiagonal kernels (and al_ls / al_outer, which share their limit)
    bool too_large() const { return n > 12 || n + m > 16; }
    bool inputs_set() const { return x0 && Qd && q && lam && rho && u.lower && u.upper && (!has_x || (x.lower && x.upper)); }
    // Behind a front check, in both orders: DQP_OK for an empty batch, DQP_ERR_BAD_ARG for a null buffer -- the problem's
    // own or one of the entry's (`rest`) --, else 1: go on
    int ready(bool rest) const { return B == 0 ? DQP_OK : (inputs_set() && rest) ? 1 : DQP_ERR_BAD_ARG; }
};

// `d` and `bounds` have passed al_bounds_check or al_xbounds_check; `xbounds` is NULL or has passed the latter
inline AlProblem al_problem(const dqp_al_mpc_dims *d, int model, double dt, const double *x0, const double *Qdiag,
                            const double *q, const double *lam, const double *rho, const dqp_al_bounds *bounds,
                            const dqp_al_bounds *xbounds, void *stream)
{
    AlProblem v = {};
    v.B = d->nbatch; v.n = d->n_state; v.m = d->n_ctrl; v.T = d->T; v.model = model; v.dt = dt;
    v.x0 = x0; v.Qd = Qdiag; v.q = q; v.lam = lam; v.rho = rho;
    v.u = *bounds; v.stream = (hipStream_t)stream;
    if (xbounds) { v.x = *xbounds; v.has_x = true; }
    return v;
}

// The members that every kernel argument with both boxes has under the same names (MeritP, LsAP, OutP, BandP): where
// such a struct's maker starts
template <class P> P boxed_args(const AlProblem &v)
{
    P p = {};
    p.B = v.B; p.T = v.T; p.x0 = v.x0; p.Qd = v.Qd; p.q = v.q; p.lam = v.lam; p.rho = v.rho;
    p.ul = v.u.lower; p.uu = v.u.upper; p.bsb = v.u.stride_b; p.bst = v.u.stride_t;
    p.xlo = v.x.lower; p.xhi = v.x.upper; p.xsb = v.x.stride_b; p.xst = v.x.stride_t;
    return p;
}

// The argument checks come in two orders, and every entry's check is one of them plus what only that entry has:
//   `_bounds` entries (and the vector entries, their (0, 0) twins)
//       al_bounds_check and the entry's scalar arguments (DQP_ERR_BAD_ARG) -- nbatch == 0 (DQP_OK) -- the model and the
//       buffers (DQP_ERR_BAD_ARG) and the kernels' limits (DQP_ERR_TOO_LARGE), in the order the entry states
//   `_xbounds` entries
//       al_xbounds_check (dqp_al_bounds.h: sizes, both layouts, DQP_ERR_TOO_LARGE, the model) and the entry's scalar
//       arguments -- nbatch == 0 -- the buffers
// Exceptions, kept: the banded step checks its model in front of nbatch == 0 (dqp_al_banded.hip); the caller-linearised
// step and the two merit entries have no model, and the former checks its pair in front of nbatch == 0.
inline int al_bounds_check(const dqp_al_mpc_dims *d, const dqp_al_bounds *bounds)
{
    if (!d || d->nbatch < 0 || d->n_state <= 0 || d->n_ctrl <= 0 || d->T < 2) return DQP_ERR_BAD_ARG;
    return al_bounds_layout(bounds, d);
}

// What dqp_al_mpc_solve{,_fused}{,_bounds,_xbounds} take besides the problem (whose lam / rho are lam_in / rho_in), in
// the order of their prototypes
struct AlMpcIo {
    int32_t al_iter, newton_steps;
    const double *x_init, *u_init;
    const double *prev_cost, *prev_lam, *prev_rho;
    int32_t n_prev;
    double *xu, *hist_cost, *hist_lam, *hist_rho, *res_norm, *factor, *status;
    int32_t *fail;
    void *workspace;

    bool scalars_ok() const { return al_iter >= 1 && al_iter <= 256 && newton_steps >= 1 && n_prev >= 0; }
    bool buffers_set() const       // status is optional
    {
        return x_init && u_init && xu && hist_cost && hist_lam && hist_rho && res_norm && factor && fail && workspace &&
               (n_prev == 0 || (prev_cost && prev_lam && prev_rho));
    }
};

}  // namespace dqp
#endif
