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

// dqp_al_banded.hip: dqp_al_banded_newton_step_bounds with `keep` = does the caller use this step's factor afterwards
// (the Newton loop of dqp_al.hip keeps the last step's only); `xbounds`: the state box of the `_xbounds` entries, or NULL
int al_banded_newton_step_keep_bounds(const dqp_al_mpc_dims *d, int dyn_id, double dt, const double *xu, const double *x0,
                                      const double *Qdiag, const double *q, const double *lam, const double *rho,
                                      const dqp_al_bounds *bounds, double *update, void *factor, int32_t *info, void *stream,
                                      int keep, const dqp_al_bounds *xbounds = nullptr);

}  // namespace dqp
#endif
