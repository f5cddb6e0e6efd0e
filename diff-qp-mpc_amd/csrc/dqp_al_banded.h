// dqp_al_banded.h -- what the files of the block-tridiagonal NewtonAL paths call in each other (the kernels and their
// argument block BandP: dqp_al_banded_kernels.h).
#ifndef DQP_AL_BANDED_H_
#define DQP_AL_BANDED_H_
#include <stdint.h>

#include "../../include/dqp.h"

namespace dqp {

struct BandP;

// dqp_al_banded_wide.hip: the launches of the DQP_BAND_WIDE_SIZES pairs.  DQP_ERR_TOO_LARGE: no kernel for (n, m).
int al_banded_wide_newton(int n_state, int n_ctrl, const BandP &P, void *stream);
int al_banded_wide_solve(int n_state, int n_ctrl, const BandP &P, void *stream);
// the same file's second object (-DDQP_BAND_WIDE_BOX): the wide pairs with a state box, BoxBounds<Given<n, m>> on 32 lanes
int al_banded_wide_box_newton(int n_state, int n_ctrl, const BandP &P, void *stream);

// dqp_al_banded_box.hip: BoxBounds<Given<n, m>> at the DQP_BAND_SIZES pairs (P.xlo / P.xhi set), by the launch rule of
// dqp_al_banded_launch.h.  DQP_ERR_TOO_LARGE: no kernel for (n, m).
int al_banded_box_newton(int n_state, int n_ctrl, const BandP &P, void *stream);
// dqp_al_banded.hip: a batch of B takes eight problems per wavefront where a knot fits a half row (dqp_al_lane_group)
bool al_banded_narrow(int B);

// dqp_al_banded.hip: dqp_al_banded_newton_step_bounds with `keep` = does the caller use this step's factor afterwards
// (the Newton loop of dqp_al.hip keeps the last step's only); `xbounds`: the state box of the `_xbounds` entries, or NULL
int al_banded_newton_step_keep_bounds(const dqp_al_mpc_dims *d, int dyn_id, double dt, const double *xu, const double *x0,
                                      const double *Qdiag, const double *q, const double *lam, const double *rho,
                                      const dqp_al_bounds *bounds, double *update, void *factor, int32_t *info, void *stream,
                                      int keep, const dqp_al_bounds *xbounds = nullptr);

}  // namespace dqp
#endif
