// dqp_mpc_qp.hip -- the MPC-structured QP entry points of include/dqp.h (dqp_mpc_qp_*): host code only, no kernels.
//
// The dense (Q, p, G, h, A, b) of an MPC problem and their gradients are never materialised in HBM.  Two routes:
// the dense null-space kernels (dqp_r16n.hip) where the QP size has an instantiation -- small horizons, one QP in
// registers, the problem assembled there from the time-major MPC data -- else the stage-wise Riccati kernels (the
// stage_* interface of dqp_common.h: any horizon, n + m <= 32).  When the caller names a host pair
// (dqp_mpc_dims.n_state_host) the problem runs padded with dummy states on that pair's stage-wise kernels, whatever else
// could run it; the padded copies live in the caller's workspace behind the kernels' part (dqp_ric_pad.hip).
#include "dqp_common.h"
#include "dqp_al_bounds.h"
#include "dqp_dyn_models.h"

using namespace dqp;

namespace {

struct Route {
    bool stage;     // the stage-wise kernels, else the null-space ones
    bool padded;    // stage-wise on a host pair: P.mn is the host's state count
};

// the arrays of a forward call
struct Io {
    const double *C, *c, *F, *f, *x0;
    const dqp_mpc_bounds *bounds;
    double *tau, *lam, *nu, *slack;
    int32_t *info;
    double *best_resid;
    void *workspace, *termination;
    bool complete() const
    {
        return C && c && F && f && x0 && bounds->lower && bounds->upper && tau && lam && nu && slack && workspace;
    }
};

bool dims_ok(const dqp_mpc_dims *md)
{
    return md && md->T >= 2 && md->n_state >= 1 && md->n_ctrl >= 1 && md->has_bounds && md->nbatch >= 0;
}

// the stage-wise route: the pair whose kernels run the problem and its parameter block
int stage_params(const dqp_mpc_dims *md, const dqp_opts *opts, KParams &P, Route &rt)
{
    rt.stage = true;
    rt.padded = md->n_state_host != 0;
    const int np = rt.padded ? md->n_state_host : md->n_state, m = md->n_ctrl;
    if (rt.padded) {        // every registered model is native
        if (md->dyn_id || np < md->n_state || !stage_supported(np, m)) return DQP_ERR_BAD_ARG;
    } else if (!stage_native(np, m)) {
        return DQP_ERR_TOO_LARGE;
    }
    // the stage-wise kernels address a wavefront's four workspaces with 32-bit byte offsets
    if (md->T > 200000 || stage_layout_doubles(np, m, md->T) * 8 * 4 > 0x7fffffffLL) return DQP_ERR_TOO_LARGE;
    P.stamps = nullptr;
    P.B = md->nbatch; P.N = md->T * (np + m); P.M = 2 * md->T * m; P.E = md->T * np;
    fill_opts(opts, P);
    P.mn = np; P.mm = m; P.mT = md->T;
    return DQP_OK;
}

// the fused entry points: a host pair bypasses the null-space route, a registered model runs on the stage-wise kernels
int mpc_params(const dqp_mpc_dims *md, const dqp_opts *opts, KParams &P, size_t &lds, Route &rt)
{
    rt = Route{};
    if (!dims_ok(md)) return DQP_ERR_BAD_ARG;
    if (md->n_state_host) return stage_params(md, opts, P, rt);
    // true-dynamics residual: a registered model of this size
    if (md->dyn_id && !dqp::dyn::model_matches(md->dyn_id, md->n_state, md->n_ctrl)) return DQP_ERR_BAD_ARG;
    dqp_dims d = {};
    d.nbatch = md->nbatch;
    d.nz = md->T * (md->n_state + md->n_ctrl);
    d.nineq = 2 * md->T * md->n_ctrl;
    d.neq = md->T * md->n_state;
    const bool stagewise = opts && (opts->flags & DQP_FLAG_STAGEWISE);
    if (!md->dyn_id && !stagewise && r16n_workspace_doubles(d.nz, d.nineq, d.neq) > 0) {
        dqp_opts o2;
        if (opts) { o2 = *opts; o2.dyn_id = 0; }
        const int rc = fill_params(&d, opts ? &o2 : nullptr, P, lds);
        if (rc != DQP_OK) return rc;
        P.mn = md->n_state; P.mm = md->n_ctrl; P.mT = md->T;
        return DQP_OK;
    }
    const int rc = stage_params(md, opts, P, rt);
    if (rc != DQP_OK) return rc;
    P.dynId = md->dyn_id;
    P.dynDt = opts ? opts->dyn_dt : 0.0;
    return DQP_OK;
}

// the stepped entry points: the stage-wise kernels only, whatever the horizon (the null-space kernels keep their iterate
// in registers)
int stepped_params(const dqp_mpc_dims *md, const dqp_opts *opts, KParams &P, Route &rt)
{
    return dims_ok(md) ? stage_params(md, opts, P, rt) : DQP_ERR_BAD_ARG;
}

size_t workspace_doubles(const KParams &P, Route rt, bool stepped)
{
    if (!rt.stage) return (size_t)P.B * (size_t)r16n_workspace_doubles(P.N, P.M, P.E);
    return (size_t)(stage_workspace_doubles(P.mn, P.mm, P.mT, P.B, stepped) +
                    (rt.padded ? pad_region_doubles(P.mn, P.mm, P.mT, P.B) : 0));
}

int snapshot_doubles(const KParams &P, Route rt)
{
    return rt.stage ? stage_snapshot_doubles(P.mn, P.mm, P.mT) : r16n_snapshot_doubles(P.N, P.M, P.E);
}

// The forward of both entry points behind their argument checks: the whole solve (fused), or iterations
// [P.itBegin, P.itEnd) of it (stepped, which runs the batch rule with the call that ends the solve).
// Padded: the kernels read the padded copies and write tau, nu padded (lam, slack have the caller's layout; the bounds
// pass through as they are: controls are not padded).  The stepped call that starts the solve packs the problem, the
// later ones reuse that copy; every call pads ext_ry and hands the caller the compact iterate, and the compact nu with
// the final one.
int forward(const dqp_mpc_dims *md, const dqp_opts *opts, KParams &P, Route rt, bool stepped, const Io &io, void *stream)
{
    int rc;
    P.mC = io.C; P.mc = io.c; P.mF = io.F; P.mf = io.f; P.mx0 = io.x0;
    mpc_set_bounds(P, io.bounds);
    P.zhat = io.tau; P.lam = io.lam; P.nu = io.nu; P.slack = io.slack; P.info = io.info; P.best_resid = io.best_resid;
    P.workspace = (double *)io.workspace;
    const bool batch = (P.flags & DQP_FLAG_BATCH_TERMINATION) != 0;
    if (batch && (!io.termination || P.maxIter > 64)) return DQP_ERR_BAD_ARG;
    const bool first = !stepped || P.itBegin == 0, last = !stepped || P.itEnd == P.maxIter;
    PadRegion R = {};
    if (rt.padded) {
        R = pad_region(P.workspace + stage_workspace_doubles(P.mn, P.mm, P.mT, P.B, stepped), P.mn, P.mm, P.mT, P.B);
        const double *ry = P.itEnd > P.itBegin ? P.extRy : nullptr;
        rc = pad_pack(md->n_state, P.mn, P.mm, P.mT, P.B, R, first ? io.C : nullptr, first ? io.c : nullptr,
                      first ? io.F : nullptr, first ? io.f : nullptr, first ? io.x0 : nullptr, nullptr, nullptr, nullptr, ry,
                      stream);
        if (rc != DQP_OK) return rc;
        P.mC = R.C; P.mc = R.c; P.mF = R.F; P.mf = R.f; P.mx0 = R.x0; P.zhat = R.tau; P.nu = R.nu;
        P.extRy = ry ? R.ry : nullptr;
    }
    auto done = [&](int r) {
        if (r != DQP_OK || !rt.padded) return r;
        return pad_unpack(md->n_state, P.mn, P.mm, P.mT, P.B, R, io.tau, last ? io.nu : nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, stream);
    };
    if (batch) {
        P.eps = opts ? opts->eps : 1e-12;       // the batch rule uses the reference's eps itself
        term_bind_pass1(P, io.termination, snapshot_doubles(P, rt));
    }
    rc = !rt.stage ? r16n_forward(P, stream) : stepped ? stage_forward_stepped(P, stream) : stage_forward(P, stream);
    if (rc != DQP_OK) return stepped && rc == 1 ? DQP_ERR_TOO_LARGE : rc;
    if (!batch || !last || (P.flags & DQP_FLAG_HISTORY_ONLY)) return done(DQP_OK);
    if ((rc = term_decide(P, io.termination, stream)) != DQP_OK) return rc;
    term_bind_pass2(P, io.termination);
    // pass 2: the null-space kernels run again as an epilogue, the stage-wise route copies the kept iterates (padded:
    // on the padded iterate, then the unpack)
    return done(rt.stage ? stage_finish(P, stream) : r16n_forward(P, stream));
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) size_t dqp_mpc_qp_termination_bytes(const dqp_mpc_dims *md, const dqp_opts *o)
{
    KParams P = {};
    size_t lds = 0;
    Route rt;
    if (!o || !(o->flags & DQP_FLAG_BATCH_TERMINATION) || mpc_params(md, o, P, lds, rt) != DQP_OK || md->nbatch <= 0) return 0;
    return term_bytes(P.B, P.maxIter, snapshot_doubles(P, rt));
}

__attribute__((visibility("default"))) int dqp_mpc_qp_supported(const dqp_mpc_dims *md)
{
    KParams P = {};
    size_t lds = 0;
    Route rt;
    return mpc_params(md, nullptr, P, lds, rt) == DQP_OK ? 1 : 0;
}

__attribute__((visibility("default"))) size_t dqp_mpc_qp_workspace_bytes(const dqp_mpc_dims *md)
{
    KParams P = {};
    size_t lds = 0;
    Route rt;
    if (mpc_params(md, nullptr, P, lds, rt) != DQP_OK || md->nbatch <= 0) return 0;
    return workspace_doubles(P, rt, false) * sizeof(double);
}

__attribute__((visibility("default"))) int
dqp_mpc_qp_forward(const dqp_mpc_dims *md, const dqp_opts *opts, const double *C, const double *c,
                   const double *F, const double *f, const double *x0, const double *u_lower,
                   const double *u_upper, double *tau, double *lam, double *nu, double *slack,
                   int32_t *info, double *best_resid, void *workspace, void *termination, void *stream)
{
    const dqp_mpc_bounds bounds = {u_lower, u_upper, 0, 0};
    return dqp_mpc_qp_forward_bounds(md, opts, C, c, F, f, x0, &bounds, tau, lam, nu, slack, info, best_resid, workspace,
                                     termination, stream);
}

// the bounds of sample b, knot t, control k at [b stride_b + t stride_t + k] (include/dqp.h: dqp_mpc_bounds)
__attribute__((visibility("default"))) int
dqp_mpc_qp_forward_bounds(const dqp_mpc_dims *md, const dqp_opts *opts, const double *C, const double *c,
                          const double *F, const double *f, const double *x0, const dqp_mpc_bounds *bounds,
                          double *tau, double *lam, double *nu, double *slack, int32_t *info, double *best_resid,
                          void *workspace, void *termination, void *stream)
{
    KParams P = {};
    size_t lds = 0;
    Route rt;
    int rc = mpc_params(md, opts, P, lds, rt);
    if (rc != DQP_OK) return rc;
    if ((rc = mpc_bounds_layout(bounds, md)) != DQP_OK) return rc;
    if (P.B == 0) return DQP_OK;
    const Io io = {C, c, F, f, x0, bounds, tau, lam, nu, slack, info, best_resid, workspace, termination};
    if (!io.complete()) return DQP_ERR_BAD_ARG;
    if (P.dynId && !(P.dynDt > 0.0)) return DQP_ERR_BAD_ARG;        // the model's step needs dqp_opts.dyn_dt
    if (P.maxIter < 1) return DQP_ERR_BAD_ARG;
    return forward(md, opts, P, rt, false, io, stream);
}

__attribute__((visibility("default"))) size_t dqp_mpc_qp_stepped_workspace_bytes(const dqp_mpc_dims *md)
{
    KParams P = {};
    Route rt;
    if (stepped_params(md, nullptr, P, rt) != DQP_OK || md->nbatch <= 0) return 0;
    return workspace_doubles(P, rt, true) * sizeof(double);
}

__attribute__((visibility("default"))) size_t dqp_mpc_qp_stepped_termination_bytes(const dqp_mpc_dims *md, const dqp_opts *o)
{
    KParams P = {};
    Route rt;
    if (!o || !(o->flags & DQP_FLAG_BATCH_TERMINATION) || stepped_params(md, o, P, rt) != DQP_OK || md->nbatch <= 0) return 0;
    return term_bytes(P.B, P.maxIter, snapshot_doubles(P, rt));
}

__attribute__((visibility("default"))) int
dqp_mpc_qp_forward_stepped(const dqp_mpc_dims *md, const dqp_opts *opts, const double *C, const double *c,
                           const double *F, const double *f, const double *x0, const double *u_lower,
                           const double *u_upper, const double *ext_ry, int32_t it_begin, int32_t it_end,
                           double *tau, double *lam, double *nu, double *slack, int32_t *info, double *best_resid,
                           void *workspace, void *termination, void *stream)
{
    const dqp_mpc_bounds bounds = {u_lower, u_upper, 0, 0};
    return dqp_mpc_qp_forward_stepped_bounds(md, opts, C, c, F, f, x0, &bounds, ext_ry, it_begin, it_end, tau, lam, nu, slack,
                                             info, best_resid, workspace, termination, stream);
}

__attribute__((visibility("default"))) int
dqp_mpc_qp_forward_stepped_bounds(const dqp_mpc_dims *md, const dqp_opts *opts, const double *C, const double *c,
                                  const double *F, const double *f, const double *x0, const dqp_mpc_bounds *bounds,
                                  const double *ext_ry, int32_t it_begin, int32_t it_end, double *tau, double *lam,
                                  double *nu, double *slack, int32_t *info, double *best_resid, void *workspace,
                                  void *termination, void *stream)
{
    KParams P = {};
    Route rt;
    int rc = stepped_params(md, opts, P, rt);
    if (rc != DQP_OK) return rc;
    if ((rc = mpc_bounds_layout(bounds, md)) != DQP_OK) return rc;
    if (P.B == 0) return DQP_OK;
    const Io io = {C, c, F, f, x0, bounds, tau, lam, nu, slack, info, best_resid, workspace, termination};
    if (!io.complete()) return DQP_ERR_BAD_ARG;
    if (P.maxIter < 1 || it_begin < 0 || it_end < it_begin || it_end > P.maxIter || it_end - it_begin > 1) return DQP_ERR_BAD_ARG;
    if (it_end > it_begin && !ext_ry) return DQP_ERR_BAD_ARG;
    if (it_end == it_begin && it_begin != 0) return DQP_ERR_BAD_ARG;
    P.extRy = ext_ry; P.itBegin = it_begin; P.itEnd = it_end;
    return forward(md, opts, P, rt, true, io, stream);
}

__attribute__((visibility("default"))) int
dqp_mpc_qp_backward(const dqp_mpc_dims *md, const dqp_opts *opts, const double *C, const double *F,
                    const double *tau, const double *lam, const double *nu, const double *slack,
                    const double *dl_dtau, double *dC, double *dc, double *dF, double *df, double *dx0,
                    int32_t *info, void *workspace, void *stream)
{
    KParams P = {};
    size_t lds = 0;
    Route rt;
    int rc = mpc_params(md, opts, P, lds, rt);
    if (rc != DQP_OK) return rc;
    if (P.B == 0) return DQP_OK;
    if (!tau || !lam || !nu || !slack || !dl_dtau || !workspace) return DQP_ERR_BAD_ARG;
    if (!dC && !dc && !dF && !df && !dx0) return DQP_OK;
    P.zin = tau; P.lamin = lam; P.nuin = nu; P.slackin = slack; P.gin = dl_dtau;
    P.mdC = dC; P.mdc = dc; P.mdF = dF; P.mdf = df; P.mdx0 = dx0;
    P.info = info;
    P.workspace = (double *)workspace;
    if (!rt.stage) return r16n_backward(P, stream);
    if (!C || !F) return DQP_ERR_BAD_ARG;
    P.mC = C; P.mF = F;
    if (!rt.padded) return stage_backward(P, stream);
    // re-padded inputs (their dummy entries are exactly zero), padded gradients, compact copies
    const PadRegion R = pad_region(P.workspace + stage_workspace_doubles(P.mn, P.mm, P.mT, P.B, false), P.mn, P.mm, P.mT, P.B);
    rc = pad_pack(md->n_state, P.mn, P.mm, P.mT, P.B, R, C, nullptr, F, nullptr, nullptr, tau, nu, dl_dtau, nullptr, stream);
    if (rc != DQP_OK) return rc;
    P.mC = R.C; P.mF = R.F; P.zin = R.tau; P.nuin = R.nu; P.gin = R.g;
    P.mdC = dC ? R.dC : nullptr; P.mdc = dc ? R.dc : nullptr; P.mdF = dF ? R.dF : nullptr;
    P.mdf = df ? R.df : nullptr; P.mdx0 = dx0 ? R.dx0 : nullptr;
    if ((rc = stage_backward(P, stream)) != DQP_OK) return rc;
    return pad_unpack(md->n_state, P.mn, P.mm, P.mT, P.B, R, nullptr, nullptr, dC, dc, dF, df, dx0, stream);
}

// the smallest compiled stage-wise pair (n', n_ctrl), n' >= n_state, native or host-only; 0: none
__attribute__((visibility("default"))) int32_t dqp_mpc_qp_host_n_state(const dqp_mpc_dims *md)
{
    if (!md || md->n_state < 1 || md->n_ctrl < 1 || !md->has_bounds || md->dyn_id) return 0;
    for (int np = md->n_state; np + md->n_ctrl <= 32; ++np)     // ascending n': the 16-lane pairs come first
        if (stage_supported(np, md->n_ctrl)) return np;
    return 0;
}

}  // extern "C"
