// dqp_al_banded_wide.hip -- the block-tridiagonal NewtonAL kernels (dqp_al_banded_kernels.h) for caller-linearised
// dynamics with knots of 17 to 32 variables (16 < n + m <= 32): the same kernels, instantiated here on DQP_BAND_WIDE_SIZES.
//
// Layout: one problem per 32-lane half-wavefront (two problems per wavefront), a knot's nt rows one per lane
// (r = lane & 31) exactly as in the 16-lane form, so the sweeps are the same source: the large-model forward sweep (state
// prefetched one knot ahead, unit_lower / trsv_unit, M^T products from the LDS tile) and trsvT_bcast backward.  What
// changes with G = 32 is the lane group (Grp<32>: a broadcast of lane k is the row's row_newbcast:(k & 15) followed by
// one v_permlane16_swap of two copies of it) and the LDS tile (TS = 34, two groups: 17 KB per workgroup).  The factor
// keeps its form: per (b, t) nt rows x (nt + 1 + n) doubles, element-major over the knot's lanes
// (dqp_al_banded_jac_factor_bytes).  No prefetch-ahead, half-row or LDS-factor variants, and no registered model is
// this wide.
//
// Compiled twice (_build.py), the objects side by side: as it is -- the vector-bound Newton kernels and the solve
// kernels -- and with -DDQP_BAND_WIDE_BOX: the Newton kernels with a state box, BoxBounds<Given<n, m>>, which read the
// control bounds through their strides too (dqp_al_banded_newton_step_jac_xbounds).
#include "dqp_al_banded_kernels.h"

#ifdef DQP_BAND_WIDE_BOX

int dqp::al_banded_wide_box_newton(int n, int m, const BandP &P, void *stream)
{
    return visit_pair<BAND_WIDE, int>(n, m, DQP_ERR_TOO_LARGE, [&](auto given) {
        DQP_LAUNCH((al_banded_newton_kernel<BoxBounds<decltype(given)>, 32>), dim3((P.B + 1) / 2), dim3(64), 0, (hipStream_t)stream, P);
        return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
    });
}

#else

int dqp::al_banded_wide_newton(int n, int m, const BandP &P, void *stream)
{
    return visit_pair<BAND_WIDE, int>(n, m, DQP_ERR_TOO_LARGE, [&](auto given) {
        DQP_LAUNCH((al_banded_newton_kernel<decltype(given), 32>), dim3((P.B + 1) / 2), dim3(64), 0, (hipStream_t)stream, P);
        return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
    });
}

int dqp::al_banded_wide_solve(int n, int m, const BandP &P, void *stream)
{
    return visit_pair<BAND_WIDE, int>(n, m, DQP_ERR_TOO_LARGE, [&](auto given) {
        DQP_LAUNCH((al_banded_solve_kernel<decltype(given), 32>), dim3((P.B + 1) / 2), dim3(64), 0, (hipStream_t)stream, P);
        return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
    });
}

#endif
