// dqp_ric_host.hip -- host-only instantiations of the stage-wise PDIPM of dqp_ric.hip: the (n', m) pairs that run a
// problem (n, m), n <= n', with n' - n dummy states (dqp_mpc_dims.n_state_host, dqp_ric_pad.hip).
// Every (n, m) with 1 <= m <= 8, n + m <= 32 then has a host: these pairs fill the controls counts the native
// lists (DQP_RIC_SIZES, DQP_RICW_SIZES) leave without one.  Per pair: the linear-residual forward, the
// caller-residual forward and the backward, always on the caller's workspace (no LDS-resident variant, no device
// model).  The pairs never answer ric_supported / ricw_supported: the routes of unpadded problems stay as they are.
//
// One source, several objects: _build.py compiles it once per part of RIC_HOST_PARTS (the wide pairs take ~30 s
// each, one object per pair keeps the build parallel), with DQP_RIC_HOST_PART = the part's index and
// DQP_RIC_HOST_PART_SIZES = its pairs.
#define DQP_RIC_KERNELS_ONLY
#include "dqp_ric.hip"

#if !defined(DQP_RIC_HOST_PART) || !defined(DQP_RIC_HOST_PART_SIZES)
#error "dqp_ric_host.hip is compiled per part: -DDQP_RIC_HOST_PART=k -DDQP_RIC_HOST_PART_SIZES=\"X(n, m) ...\""
#endif

namespace dqp {

#define DQP_HOST_CAT2(a, b) a##b
#define DQP_HOST_CAT(a, b) DQP_HOST_CAT2(a, b)

int DQP_HOST_CAT(ric_host_run_, DQP_RIC_HOST_PART)(int op, const KParams &P, void *stream)
{
#define X(a, b)                                                                                               \
    if (P.mn == a && P.mm == b) {                                                                             \
        using Cg = ric::Cfg<a, b>;                                                                            \
        using Sg = StridedBounds<Cg>;                                                                         \
        if (op == RIC_HOST_FORWARD && mpc_bounds_strided(P)) return ric::launch<Cg>(ric::forward_kernel<Sg, ric::RES_LINEAR>, P, P.mT, stream); \
        if (op == RIC_HOST_STEPPED && mpc_bounds_strided(P)) return ric::launch<Cg>(ric::forward_kernel<Sg, ric::RES_CALLER>, P, P.mT, stream); \
        if (op == RIC_HOST_FORWARD) return ric::launch<Cg>(ric::forward_kernel<Cg, ric::RES_LINEAR>, P, P.mT, stream); \
        if (op == RIC_HOST_STEPPED) return ric::launch<Cg>(ric::forward_kernel<Cg, ric::RES_CALLER>, P, P.mT, stream); \
        return ric::launch<Cg>(ric::backward_kernel<Cg>, P, P.mT, stream);                                    \
    }
    DQP_RIC_HOST_PART_SIZES
#undef X
    return 1;
}

}  // namespace dqp
