// dqp_al_banded.h -- what the files of the block-tridiagonal NewtonAL paths call in each other (the kernels and their
// argument block BandP: dqp_al_banded_kernels.h).
#ifndef DQP_AL_BANDED_H_
#define DQP_AL_BANDED_H_
#include <stdint.h>

#include "../../include/dqp.h"
#include "dqp_al_host.h"

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

// dqp_al_banded.hip: dqp_al_banded_newton_step{,_bounds,_xbounds} behind their front check -- the empty batch, the
// buffers, the launch for the problem's registered model; `keep` = does the caller use this step's factor afterwards (the Newton loop of
// dqp_al.hip keeps the last step's only)
int al_banded_newton_step(const AlProblem &v, const double *xu, double *update, void *factor, int32_t *info, bool keep);

}  // namespace dqp
#endif
