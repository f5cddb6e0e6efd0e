// dqp_ric.hip -- the instantiations of the stage-wise PDIPM kernels (dqp_ric_kernels.h).
//
// One source, several objects: _build.py compiles it once per part of RIC_PARTS, with DQP_RIC_PART = the part's name,
// DQP_RIC_PART_SIZES = its (n_state, n_ctrl) pairs and DQP_RIC_PART_NATIVE = 1 for the native 16-lane part.  A part
// exports stage_run_<part>, which dqp_ric_pad.hip dispatches over; a kernel's machine code depends on which other
// pairs share its object, so the parts are the unit of every before / after comparison.
//
// Per pair, every part: the linear-residual forward, the caller-residual forward (dqp_mpc_qp_forward_stepped) and the
// backward on the caller's workspace, each forward with vector and with strided bounds.  The native 16-lane part adds
// the forward with its workspace in LDS (Cfg<n, m, true>), the true-dynamics forward of the pairs that have a
// registered model, and the finish kernel of the batch rule, which serves every part (sizes at run time).  The wide
// pairs (16 < n + m <= 32: one QP per 32-lane half-wavefront, what changes is the lane-group bookkeeping of Cfg::G and
// the cross-lane primitives bc / gsum / gmin) have no LDS-resident variant, and no registered model is that wide; the
// host-only pairs run padded problems, which have no model either.
#include "dqp_ric_kernels.h"

#if !defined(DQP_RIC_PART) || !defined(DQP_RIC_PART_SIZES) || !defined(DQP_RIC_PART_NATIVE)
#error "compiled per part: -DDQP_RIC_PART=name -DDQP_RIC_PART_NATIVE=0|1 -DDQP_RIC_PART_SIZES=\"X(n, m) ...\""
#endif

namespace dqp {

#if DQP_RIC_PART_NATIVE
namespace ric {
// Pass 2 of the batch-coupled rule (dqp_term.hip) when pass 1 kept its improving iterates: a flagged
// problem's outputs are rewritten from the snapshot of its best iteration before the stop -- a copy.
// One wavefront per problem; sizes at run time.
__global__ __launch_bounds__(64) void finish_kernel(KParams P, int T, int nx, int nu)
{
    const long long qp = blockIdx.x;
    const int istar = term_cap(P);
    if (!term_flagged(P, qp, istar)) return;
    const int cap = min(P.maxIter, istar);
    const double2 *h = reinterpret_cast<const double2 *>(P.histIn) + qp;
    double best = h[0].x;
    int arg = 0;
    for (int it = 1; it < cap; ++it) {
        const double v = h[(long long)it * P.B].x;
        if (v < best) { best = v; arg = it; }
    }
    const int nt = nx + nu, nz = T * nt, neq = T * nx, hm = T * nu;
    const double *sp = P.snap + ((long long)arg * P.B + qp) * (long long)(nz + neq + 4 * hm);
    const int lane = threadIdx.x;
    for (int i = lane; i < nz; i += 64) P.zhat[qp * nz + i] = sp[i];
    for (int i = lane; i < neq; i += 64) P.nu[qp * neq + i] = sp[nz + i];
    for (int i = lane; i < hm; i += 64) {
        P.slack[qp * 2 * hm + i] = sp[nz + neq + i];            P.slack[qp * 2 * hm + hm + i] = sp[nz + neq + hm + i];
        P.lam[qp * 2 * hm + i] = sp[nz + neq + 2 * hm + i];     P.lam[qp * 2 * hm + hm + i] = sp[nz + neq + 3 * hm + i];
    }
    if (lane == 0) {
        if (P.info) P.info[2 * qp + 1] = cap;
        if (P.best_resid) P.best_resid[qp] = best;
    }
}
}  // namespace ric

int stage_finish(const KParams &P, void *stream)
{
    DQP_LAUNCH(ric::finish_kernel, dim3(P.B), dim3(64), 0, (hipStream_t)stream, P, P.mT, P.mn, P.mm);
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}
#endif

namespace {

// the forward of one pair, RES = RES_LINEAR / RES_MODEL (fused) or RES_CALLER (stepped: always the caller's workspace,
// STEP_STATE doubles per slot behind it)
template <int NX, int NU, int RES> int forward(const KParams &P, void *stream)
{
    using Cg = ric::Cfg<NX, NU>;
    using Sg = StridedBounds<Cg>;
    const bool sbd = mpc_bounds_strided(P);
    if constexpr (DQP_RIC_PART_NATIVE && RES != ric::RES_CALLER) {
        // Workspace in LDS (Cfg<., ., true>) where four of them fit beside the stage without starving the CU
        // of wavefronts: up to 40 KB per wavefront, or up to 64 KB while the batch is at most two per CU.
        using Cl = ric::Cfg<NX, NU, true>;
        using Sl = StridedBounds<Cl>;
        const size_t lds = (ric::Stage<Cl>::res_ws(P.mT) + 4 * (size_t)ric::layout(NX, NU, P.mT).total) * sizeof(double);
        const bool wsl = !(P.flags & DQP_FLAG_RIC_GLOBAL_WS) && (lds <= 40 * 1024 || (lds <= 64 * 1024 && (P.B + 3) / 4 <= 512));
        if (wsl)
            return sbd ? ric::launch<Cl>(ric::forward_kernel<Sl, RES>, P, P.mT, stream, lds)
                       : ric::launch<Cl>(ric::forward_kernel<Cl, RES>, P, P.mT, stream, lds);
    }
    return sbd ? ric::launch<Cg>(ric::forward_kernel<Sg, RES>, P, P.mT, stream)
               : ric::launch<Cg>(ric::forward_kernel<Cg, RES>, P, P.mT, stream);
}

template <int NX, int NU> int run(int op, const KParams &P, void *stream)
{
    using Cg = ric::Cfg<NX, NU>;
    if (op == STAGE_BACKWARD) return ric::launch<Cg>(ric::backward_kernel<Cg>, P, P.mT, stream);
    if (op == STAGE_STEPPED) return forward<NX, NU, ric::RES_CALLER>(P, stream);
    // the true-dynamics residual of a registered model is its own instantiation: the model's registers
    // (an RK4 step of the quadrotor) would otherwise be spilled around on the linear path too.
    if constexpr (DQP_RIC_PART_NATIVE && ric::has_model<Cg>())
        if (P.dynId) return forward<NX, NU, ric::RES_MODEL>(P, stream);
    return P.dynId ? 1 : forward<NX, NU, ric::RES_LINEAR>(P, stream);
}

}  // namespace

#define DQP_RIC_CAT2(a, b) a##b
#define DQP_RIC_CAT(a, b) DQP_RIC_CAT2(a, b)

// 1: not a pair of this part, or a model it has no kernel for
int DQP_RIC_CAT(stage_run_, DQP_RIC_PART)(int op, const KParams &P, void *stream)
{
#define X(a, b) if (P.mn == a && P.mm == b) return run<a, b>(op, P, stream);
    DQP_RIC_PART_SIZES
#undef X
    return 1;
}

}  // namespace dqp
