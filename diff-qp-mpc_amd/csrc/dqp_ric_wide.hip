// dqp_ric_wide.hip -- the stage-wise PDIPM of dqp_ric.hip for knots of 17 to 32 variables
// (16 < n + m <= 32): the same kernels, instantiated here on the wide pairs.
//
// Layout: one QP per 32-lane half-wavefront (two QPs per wavefront), a knot row-distributed one row per
// lane (r = lane & 31) exactly as in the 16-lane form, so the sweeps are the same source.  What changes
// with Cfg::G = 32 is the lane-group bookkeeping (Q = 2 places per wavefront) and the cross-lane
// primitives (ric::bc / gsum / gmin): a broadcast of lane k is the row's row_newbcast:(k & 15) followed by
// one v_permlane16_swap of two copies of it (four instructions per double against two), a reduction is the
// 16-lane one plus the same exchange.  Workspace per QP: ric::layout, unchanged (finish_kernel and the
// termination snapshot are shared with the 16-lane pairs); always the caller's buffer (no LDS-resident
// variant); no registered device model is this wide, so dyn_id != 0 is refused.
#define DQP_RIC_KERNELS_ONLY
#include "dqp_ric.hip"

namespace dqp {

// size table: (n_state, n_ctrl) pairs of the wide stage-wise kernels
#ifndef DQP_RICW_SIZES
#define DQP_RICW_SIZES X(13, 4) X(14, 7) X(24, 8)
#endif

bool ricw_supported(int n, int m)
{
#define X(a, b) if (n == a && m == b) return true;
    DQP_RICW_SIZES
#undef X
    return false;
}

long long ricw_workspace_doubles(int n, int m, int T)
{
    return ricw_supported(n, m) ? ric::layout(n, m, T).total : 0;
}

int ricw_forward(const KParams &P, void *stream)
{
    if (P.dynId) return 1;
#define X(a, b)                                                                                                       \
    if (P.mn == a && P.mm == b) {                                                                                     \
        using Cg = ric::Cfg<a, b>;                                                                                    \
        if (mpc_bounds_strided(P)) return ric::launch<Cg>(ric::forward_kernel<StridedBounds<Cg>, ric::RES_LINEAR>, P, P.mT, stream); \
        return ric::launch<Cg>(ric::forward_kernel<Cg, ric::RES_LINEAR>, P, P.mT, stream);                            \
    }
    DQP_RICW_SIZES
#undef X
    return 1;
}

// two slots per wavefront, STEP_STATE doubles per slot behind the workspaces (as ric_stepped_workspace_doubles)
long long ricw_stepped_workspace_doubles(int n, int m, int T, int B)
{
    if (!ricw_supported(n, m)) return 0;
    return (long long)((B + 1) / 2 * 2) * (ric::layout(n, m, T).total + ric::STEP_STATE);
}

int ricw_forward_stepped(const KParams &P, void *stream)
{
#define X(a, b)                                                                                                       \
    if (P.mn == a && P.mm == b) {                                                                                     \
        using Cg = ric::Cfg<a, b>;                                                                                    \
        if (mpc_bounds_strided(P)) return ric::launch<Cg>(ric::forward_kernel<StridedBounds<Cg>, ric::RES_CALLER>, P, P.mT, stream); \
        return ric::launch<Cg>(ric::forward_kernel<Cg, ric::RES_CALLER>, P, P.mT, stream);                            \
    }
    DQP_RICW_SIZES
#undef X
    return 1;
}

int ricw_snapshot_doubles(int n, int m, int T) { return ricw_supported(n, m) ? T * (2 * n + 5 * m) : 0; }

int ricw_backward(const KParams &P, void *stream)
{
#define X(a, b) if (P.mn == a && P.mm == b) return ric::launch<ric::Cfg<a, b>>(ric::backward_kernel<ric::Cfg<a, b>>, P, P.mT, stream);
    DQP_RICW_SIZES
#undef X
    return 1;
}

}  // namespace dqp
