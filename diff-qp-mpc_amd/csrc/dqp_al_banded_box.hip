// dqp_al_banded_box.hip -- the block-tridiagonal NewtonAL step for caller-linearised dynamics WITH a state box at the
// DQP_BAND_SIZES pairs: al_banded_newton_kernel<BoxBounds<Given<n, m>>, G, LF> (dqp_al_banded_kernels.h), launched by the
// rule of dqp_al_banded_launch.h -- 16 lanes, 8 where n + m <= 8, the LDS-resident factor where 6 <= n + m <= 8.  A file of
// its own so that these instantiations compile next to those of dqp_al_banded.hip, not behind them.  The entry point
// (dqp_al_banded_newton_step_jac_xbounds) and its checks are in dqp_al_banded.hip; the wide pairs' launch is in
// dqp_al_banded_wide.hip.
#include "dqp_al_banded_launch.h"

int dqp::al_banded_box_newton(int n, int m, const BandP &P, void *stream)
{
    return visit_pair<BAND_NARROW, int>(n, m, DQP_ERR_TOO_LARGE, [&](auto given) {
        return run_newton<BoxBounds<decltype(given)>>(P, stream);
    });
}
