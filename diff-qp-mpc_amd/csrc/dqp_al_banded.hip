// dqp_al_banded.hip -- host side of the block-tridiagonal NewtonAL kernels (dqp_al_banded_kernels.h) at knots of up to 16
// variables: the choice of the lane group (the launch rule itself: dqp_al_banded_launch.h), the launches for registered
// models and for the caller-linearised pairs of DQP_BAND_SIZES, and the C entry points (include/dqp.h).  The
// DQP_BAND_WIDE_SIZES pairs are launched by dqp_al_banded_wide.hip, the DQP_BAND_SIZES pairs with a state box by
// dqp_al_banded_box.hip.
#include <stdlib.h>

#include "dqp_al_banded_kernels.h"

// The pair lists of dqp_al_banded_kernels.h once more, in the file where the tests read them (tests/test_al_banded_cpu.py:
// BANDED_SRC; tests/test_gpu_al_given.py parametrises on them at import, so a suite that does not find them here runs
// nothing).  The header's definition is the one every file compiles; the preprocessor accepts a second definition only
// if it is the same, token for token, so a pair added in one place alone does not build.
#pragma clang diagnostic push
#pragma clang diagnostic error "-Wmacro-redefined"
#define DQP_BAND_SIZES                                                                                   \
    X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(6, 1) X(7, 1) X(8, 1) X(2, 2) X(3, 2) X(4, 2) X(5, 2) X(6, 2) X(8, 2) \
    X(10, 2) X(12, 2) X(3, 3) X(6, 3) X(9, 3) X(4, 4) X(6, 4) X(8, 4) X(10, 4) X(12, 4)
#define DQP_BAND_WIDE_SIZES X(13, 4) X(14, 7) X(24, 8)
#pragma clang diagnostic pop

namespace {

#ifdef DQP_BAND_STAMPS
// instrumented build (tools/stamps_band.py): the Newton kernel's second argument
unsigned long long *g_band_stamps = nullptr;
#define BAND_STAMP_ARG , g_band_stamps
#else
#define BAND_STAMP_ARG
#endif

}  // namespace

#include "dqp_al_banded_launch.h"

namespace {

// g_lane_group: 0 = by batch size, 8 / 16 = pinned (dqp_al_lane_group; initial value from DQP_AL_LANE_GROUP, read once)
static int g_lane_group = -1;
static int g_simds = 0;
inline bool narrow(int B)
{
    if (g_lane_group < 0) {
        const char *force = getenv("DQP_AL_LANE_GROUP");
        g_lane_group = (force && force[0] == '8') ? 8 : ((force && force[0] == '1') ? 16 : 0);
    }
    if (g_lane_group) return g_lane_group == 8;
    if (!g_simds) {         // four SIMDs per CU, one wavefront of these kernels per SIMD
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        g_simds = 4 * cus;
    }
    return (B + 3) / 4 > g_simds;
}
// the vector instantiation at (0, 0), the strided one otherwise; with a state box the BoxBounds<> one (both boxes strided)
template <class Map> int run_newton_layout(const BandP &P, void *stream)
{
    if constexpr (!is_given<Map>::value) {
        if (P.xlo) return run_newton<BoxBounds<Map>>(P, stream);
    }
    return (P.bsb != 0 || P.bst != 0) ? run_newton<StridedBounds<Map>>(P, stream) : run_newton<Map>(P, stream);
}
template <class Map> int run_solve(const BandP &P, void *stream)
{
    if constexpr (half_row<Map>()) {
        if (narrow(P.B)) {
            DQP_LAUNCH((al_banded_solve_kernel<Map, 8>), dim3((P.B + 7) / 8), dim3(64), 0, (hipStream_t)stream, P);
            return dqp::launched();
        }
    }
    DQP_LAUNCH((al_banded_solve_kernel<Map, 16>), dim3((P.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, P);
    return dqp::launched();
}

// The one maker of the Newton kernels' argument; the caller-linearised entries add xnext / Jx / Ju.  Solve-only mode
// (dqp_al_banded_solve) fills its few members itself.
BandP band_args(const dqp::AlProblem &v, const double *xu, double *update, void *factor, int32_t *info, bool keep)
{
    BandP P = dqp::boxed_args<BandP>(v);
    P.xu = xu; P.upd = update; P.fac = (double *)factor; P.info = info; P.dt = v.dt; P.keep = keep ? 1 : 0;
    return P;
}

bool given_supported(int n, int m) { return visit_pair<BAND_NARROW>(n, m, false, [](auto) { return true; }); }
bool given_wide(int n, int m) { return visit_pair<BAND_WIDE>(n, m, false, [](auto) { return true; }); }
// what a visit over the narrow pairs returns for a pair that is not one of them: the wide entry is asked then (a launch
// returns DQP_OK or a negative DQP_ERR_*)
constexpr int NOT_NARROW = 1;

int knot_doubles(int id, int n_, int m_)          // nt rows x (L row, 1/diag, M row)
{
    int32_t n = n_, m = m_;
    if (id != 0 && dqp_dyn_sizes(id, &n, &m) != DQP_OK) return 0;
    if (id == 0 && !given_supported(n, m)) return 0;
    return (n + m) * ((n + m) + 1 + n);
}

}  // namespace

using namespace dqp::dyn;

bool dqp::al_banded_narrow(int B) { return narrow(B); }

extern "C" {

#ifdef DQP_BAND_STAMPS
// instrumented build only: device buffer of 8 x uint64 per workgroup of the Newton kernel
__attribute__((visibility("default"))) void dqp_debug_band_stamps(void *dev_ptr) { g_band_stamps = (unsigned long long *)dev_ptr; }
#endif

__attribute__((visibility("default"))) size_t dqp_al_banded_factor_bytes(const dqp_al_mpc_dims *d, int dyn_id)
{
    const int kd = d ? knot_doubles(dyn_id, d->n_state, d->n_ctrl) : 0;
    if (!d || d->nbatch <= 0 || d->T < 2 || kd == 0) return 0;
    return (size_t)d->nbatch * d->T * kd * sizeof(double);
}

// the factor buffer of dqp_al_banded_newton_step_jac: the narrow pairs' size, or the same layout at a wide pair
__attribute__((visibility("default"))) size_t dqp_al_banded_jac_factor_bytes(const dqp_al_mpc_dims *d)
{
    if (!d || d->nbatch <= 0 || d->T < 2) return 0;
    const int n = d->n_state, nt = d->n_state + d->n_ctrl;
    if (!given_supported(n, d->n_ctrl) && !given_wide(n, d->n_ctrl)) return 0;
    return (size_t)d->nbatch * d->T * nt * (nt + 1 + n) * sizeof(double);
}

}  // extern "C"

int dqp::al_banded_newton_step(const AlProblem &v, const double *xu, double *update, void *factor, int32_t *info, bool keep)
{
    if (const int r = v.ready(xu && update && factor); r != 1) return r;        // info is optional
    const BandP P = band_args(v, xu, update, factor, info, keep);
    return visit<int>(v.model, DQP_ERR_BAD_ARG, [&](auto model) {
        return run_newton_layout<typename decltype(model)::Map>(P, v.stream);
    });
}

extern "C" {

__attribute__((visibility("default"))) int
dqp_al_banded_newton_step(const dqp_al_mpc_dims *d, int dyn_id, double dt, const double *xu, const double *x0,
                          const double *Qdiag, const double *q, const double *lam, const double *rho,
                          const double *u_lower, const double *u_upper, double *update, void *factor,
                          int32_t *info, void *stream)
{
    const dqp_al_bounds bd = {u_lower, u_upper, 0, 0};
    return dqp_al_banded_newton_step_bounds(d, dyn_id, dt, xu, x0, Qdiag, q, lam, rho, &bd, update, factor, info, stream);
}

__attribute__((visibility("default"))) int
dqp_al_banded_newton_step_bounds(const dqp_al_mpc_dims *d, int dyn_id, double dt, const double *xu, const double *x0,
                                 const double *Qdiag, const double *q, const double *lam, const double *rho,
                                 const dqp_al_bounds *bounds, double *update, void *factor, int32_t *info, void *stream)
{
    // unlike the other `_bounds` entries this one checks its model in front of the nbatch == 0 return (dqp_al_host.h)
    if (dqp::al_bounds_check(d, bounds) || !model_matches(dyn_id, d->n_state, d->n_ctrl)) return DQP_ERR_BAD_ARG;
    const dqp::AlProblem v = dqp::al_problem(d, dyn_id, dt, x0, Qdiag, q, lam, rho, bounds, nullptr, stream);
    return dqp::al_banded_newton_step(v, xu, update, factor, info, true);
}

// The step with a state box (include/dqp.h): lam has dqp_al_ncon_xbounds(dims) rows per problem
__attribute__((visibility("default"))) int
dqp_al_banded_newton_step_xbounds(const dqp_al_mpc_dims *d, int model, double dt, const double *xu, const double *x0,
                                  const double *Qdiag, const double *q, const double *lam, const double *rho,
                                  const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, double *update, void *factor,
                                  int32_t *info, void *stream)
{
    if (const int rc = dqp::al_xbounds_check(d, bounds, xbounds, d && model_matches(model, d->n_state, d->n_ctrl))) return rc;
    const dqp::AlProblem v = dqp::al_problem(d, model, dt, x0, Qdiag, q, lam, rho, bounds, xbounds, stream);
    return dqp::al_banded_newton_step(v, xu, update, factor, info, true);
}

__attribute__((visibility("default"))) int
dqp_al_banded_solve(const dqp_al_mpc_dims *d, int dyn_id, const void *factor, const double *rhs, double *out,
                    void *stream)
{
    if (!d || d->nbatch < 0 || d->T < 2) return DQP_ERR_BAD_ARG;
    if (dyn_id != 0 && !dqp::dyn::model_matches(dyn_id, d->n_state, d->n_ctrl)) return DQP_ERR_BAD_ARG;
    if (d->nbatch == 0) return DQP_OK;
    if (!factor || !rhs || !out) return DQP_ERR_BAD_ARG;
    BandP P = {};
    P.rhs = rhs; P.upd = out; P.fac = (double *)factor; P.B = d->nbatch; P.T = d->T;
    if (dyn_id == 0) {          // the factor of dqp_al_banded_newton_step_jac: layout by sizes
        const int rc = visit_pair<BAND_NARROW, int>(d->n_state, d->n_ctrl, NOT_NARROW, [&](auto given) {
            return run_solve<decltype(given)>(P, stream);
        });
        return rc == NOT_NARROW ? dqp::al_banded_wide_solve(d->n_state, d->n_ctrl, P, stream) : rc;
    }
    return visit<int>(dyn_id, DQP_ERR_BAD_ARG, [&](auto model) {
        return run_solve<typename decltype(model)::Map>(P, stream);
    });
}

// The two caller-linearised steps behind their front checks (the pair has a kernel): the empty batch, the buffers, the launch
// at the pair -- with a state box in the objects of dqp_al_banded_box.hip / dqp_al_banded_wide.hip
static int given_step(const dqp::AlProblem &v, const double *xu, const double *x_next, const double *Jx, const double *Ju,
                      double *update, void *factor, int32_t *info)
{
    if (const int r = v.ready(xu && x_next && Jx && Ju && update && factor); r != 1) return r;
    BandP P = band_args(v, xu, update, factor, info, true);
    P.xnext = x_next; P.Jx = Jx; P.Ju = Ju;
    if (v.has_x) return (given_wide(v.n, v.m) ? dqp::al_banded_wide_box_newton : dqp::al_banded_box_newton)(v.n, v.m, P, v.stream);
    const int rc = visit_pair<BAND_NARROW, int>(v.n, v.m, NOT_NARROW, [&](auto given) {
        return run_newton_layout<decltype(given)>(P, v.stream);
    });
    return rc == NOT_NARROW ? dqp::al_banded_wide_newton(v.n, v.m, P, v.stream) : rc;
}

/*
 * The same block-tridiagonal Newton step for a dynamics the CALLER linearised (include/dqp.h).
 */
__attribute__((visibility("default"))) int
dqp_al_banded_newton_step_jac_bounds(const dqp_al_mpc_dims *d, const double *xu, const double *x0, const double *Qdiag,
                                     const double *q, const double *lam, const double *rho, const dqp_al_bounds *bounds,
                                     const double *x_next, const double *Jx, const double *Ju, double *update,
                                     void *factor, int32_t *info, void *stream)
{
    if (dqp::al_bounds_check(d, bounds)) return DQP_ERR_BAD_ARG;
    const dqp::AlProblem v = dqp::al_problem(d, 0, 0.0, x0, Qdiag, q, lam, rho, bounds, nullptr, stream);
    // the pair in front of the nbatch == 0 return; the wide pairs have the vector instantiation only
    if (!given_supported(v.n, v.m) && (!given_wide(v.n, v.m) || v.strided())) return DQP_ERR_TOO_LARGE;
    return given_step(v, xu, x_next, Jx, Ju, update, factor, info);
}

// The step for caller-linearised dynamics with a state box (include/dqp.h): lam has dqp_al_ncon_xbounds(dims) rows per
// problem; BoxBounds<Given<n, m>> reads both boxes through their strides, at the wide pairs too
__attribute__((visibility("default"))) int
dqp_al_banded_newton_step_jac_xbounds(const dqp_al_mpc_dims *d, const double *xu, const double *x0, const double *Qdiag,
                                      const double *q, const double *lam, const double *rho, const dqp_al_bounds *bounds,
                                      const dqp_al_bounds *xbounds, const double *x_next, const double *Jx,
                                      const double *Ju, double *update, void *factor, int32_t *info, void *stream)
{
    // no model: the sizes and both layouts, then the pair (not al_xbounds_check, whose limit is the registered models')
    if (dqp::al_bounds_check(d, bounds) || dqp::al_box_layout(xbounds, d, d->n_state)) return DQP_ERR_BAD_ARG;
    const dqp::AlProblem v = dqp::al_problem(d, 0, 0.0, x0, Qdiag, q, lam, rho, bounds, xbounds, stream);
    if (!given_wide(v.n, v.m) && !given_supported(v.n, v.m)) return DQP_ERR_TOO_LARGE;
    return given_step(v, xu, x_next, Jx, Ju, update, factor, info);
}

__attribute__((visibility("default"))) int
dqp_al_banded_newton_step_jac(const dqp_al_mpc_dims *d, const double *xu, const double *x0, const double *Qdiag,
                              const double *q, const double *lam, const double *rho, const double *u_lower,
                              const double *u_upper, const double *x_next, const double *Jx, const double *Ju,
                              double *update, void *factor, int32_t *info, void *stream)
{
    const dqp_al_bounds bd = {u_lower, u_upper, 0, 0};
    return dqp_al_banded_newton_step_jac_bounds(d, xu, x0, Qdiag, q, lam, rho, &bd, x_next, Jx, Ju, update, factor, info,
                                                stream);
}

__attribute__((visibility("default"))) int dqp_al_lane_group(int width)
{
    if (width != 0 && width != 8 && width != 16) return DQP_ERR_BAD_ARG;
    g_lane_group = width;
    return DQP_OK;
}

}  // extern "C"
