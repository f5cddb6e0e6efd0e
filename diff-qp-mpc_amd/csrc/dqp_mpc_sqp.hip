// dqp_mpc_sqp.hip -- the gradient-free SQP rounds of qp_wrapper.MPC.solve_nonlin for a registered device model
// (include/dqp.h: dqp_mpc_linearize, dqp_mpc_sqp_*).
//
// Replaces, per round of qpth/qp_wrapper.py:348-414: linearize_dynamics (:481-515: dynamics, dx_jac, cat, bmv, two
// reshapes), the step du = u_qp - u, the best-trajectory bookkeeping (~10 where / clone / compare ops) and the two host
// tests of the loop.  The QP (dqp_mpc_qp_forward_bounds) and the line search (dqp_mpc_line_search) are the existing
// entries, called from here.  A round is
//
//     sqp_linearize_kernel -> [QP launches] -> sqp_step_kernel -> [line search] -> sqp_keep_kernel -> sqp_finish_kernel
//
// and nothing returns to the host in between.  state (int32[4]) = {done, rounds applied, 0, 0}: every kernel of this file
// reads state[0] and leaves at once when it is set, so a round enqueued behind the stop changes nothing (the QP and the
// line search of such a round run on the previous round's F, f and only write scratch).  Round 0 ignores the state it
// finds and its finish kernel writes all four words: the reset is part of the round, not a launch or a memset of its own.
// The batch-wide |u_new - u|^2 crosses workgroups at launch boundaries only: sqp_keep_kernel writes one partial per
// workgroup (samples in index order), sqp_finish_kernel adds the partials in index order.  No atomics: the sum, and with
// it the round at which the solve stops, is the same from run to run.
#include "dqp_common.h"
#include "dqp_al_bounds.h"
#include "dqp_dyn_models.h"

namespace dqp {
namespace sqp {
namespace {

constexpr int KEEP_BLOCK = 64;      // samples per workgroup of sqp_keep_kernel = samples per partial sum
constexpr int LS_MAXN = 12, LS_MAXM = 8;        // what dqp_mpc_line_search serves

// F (N, NX, NX+NU) = [df/dx, df/du] and f (N, NX) = step(x, u) - F [x; u] at the N = (T-1) B first knots of the
// time-major x (T, B, NX), u (T, B, NU): knot i of the kernel is knot (t, b) = (i / B, i % B) of both layouts.
// The passes of dyn::jac_kernel (KC seed directions each); pass c0 writes columns c0 .. c0+KC-1 of F and takes their
// share F[:, col] tau[col] off the accumulator, which starts at x_next: columns in ascending order, in registers.
template <class Map, int KC>
__global__ __launch_bounds__(256) void sqp_linearize_kernel(long long N, const double *x, const double *u, double dt,
                                                            double *F, double *f, const int32_t *state)
{
    constexpr int NX = Map::NX, NU = Map::NU, NS = NX + NU;
    using S = dyn::Dual<KC>;
    if (state && state[0]) return;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        double xv[NX], uv[NU], acc[NX];
#pragma unroll
        for (int k = 0; k < NX; ++k) xv[k] = x[i * NX + k];
#pragma unroll
        for (int k = 0; k < NU; ++k) uv[k] = u[i * NU + k];
#pragma unroll
        for (int c0 = 0; c0 < NS; c0 += KC) {
            // the passes are independent: kept apart, the register demand is that of one pass (dyn::jac_kernel)
#pragma unroll
            for (int k = 0; k < NX; ++k) asm volatile("" : "+v"(xv[k]) : : "memory");
            S xs[NX], us[NU], out[NX];
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                xs[k] = S(xv[k]);
                if (k >= c0 && k < c0 + KC) xs[k].d[k - c0] = 1.0;
            }
#pragma unroll
            for (int k = 0; k < NU; ++k) {
                us[k] = S(uv[k]);
                if (NX + k >= c0 && NX + k < c0 + KC) us[k].d[NX + k - c0] = 1.0;
            }
            Map::template step<S>(xs, us, dt, out);
            if (c0 == 0) {
#pragma unroll
                for (int r = 0; r < NX; ++r) acc[r] = out[r].v;
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int col = c0 + c;
                if (col < NS) {
                    const double tc = col < NX ? xv[col < NX ? col : 0] : uv[col >= NX ? col - NX : 0];
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        F[(i * NX + r) * NS + col] = out[r].d[c];
                        acc[r] -= out[r].d[c] * tc;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) f[i * NX + r] = acc[r];
    }
}

struct StepP {
    const double *tau, *u;      // tau (B, T, n+m) the QP solution, u (T, B, m)
    double *du;                 // (T, B, m)
    const int32_t *state;
    int B, n, m, T;
};

// du = u_qp - u, the step single_qp hands to the line search (qp_wrapper.py:321-324)
__global__ __launch_bounds__(256) void sqp_step_kernel(StepP P)
{
    if (P.state && P.state[0]) return;         // state == NULL: round 0
    const long long total = (long long)P.T * P.B * P.m;
    const int nt = P.n + P.m;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % P.m);
        const long long tb = i / P.m, t = tb / P.B, b = tb % P.B;
        P.du[i] = P.tau[(b * P.T + t) * nt + P.n + k] - P.u[i];
    }
}

struct KeepP {
    const double *xn, *un, *cost;       // the line search's last trial (T, B, n), (T, B, m) and its cost (B)
    double *x, *u;                      // current trajectory, in/out
    double *kx, *ku, *kcost;            // best trajectory seen, per sample
    double *partial;                    // one |u_new - u|^2 per workgroup
    const int32_t *state;
    double best_cost_eps;
    int B, n, m, T, first;
};

// One thread per sample: keep-best (qp_wrapper.py:366-380; `first`: the round that stores unconditionally), the commit
// x, u <- x_new, u_new and the sample's sum of (u_new - u)^2 over knots then controls; the workgroup's samples are added
// in index order by its first thread.
__global__ __launch_bounds__(KEEP_BLOCK) void sqp_keep_kernel(KeepP P)
{
    __shared__ double part[KEEP_BLOCK];
    if (!P.first && P.state[0]) return;     // uniform over the grid: nobody waits at the barrier below
    const long long b = (long long)blockIdx.x * KEEP_BLOCK + threadIdx.x;
    double s = 0.0;
    if (b < P.B) {
        const double cn = P.cost[b];
        const bool better = P.first || cn <= P.kcost[b] + P.best_cost_eps;
        if (better) P.kcost[b] = cn;
        for (int t = 0; t < P.T; ++t) {
            const long long k = (long long)t * P.B + b;
            for (int i = 0; i < P.n; ++i) {
                const double v = P.xn[k * P.n + i];
                P.x[k * P.n + i] = v;
                if (better) P.kx[k * P.n + i] = v;
            }
            for (int i = 0; i < P.m; ++i) {
                const double v = P.un[k * P.m + i], d = v - P.u[k * P.m + i];
                s += d * d;
                P.u[k * P.m + i] = v;
                if (better) P.ku[k * P.m + i] = v;
            }
        }
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int j = 0; j < KEEP_BLOCK; ++j) a += part[j];
        P.partial[blockIdx.x] = a;
    }
}

// One workgroup: the partials in index order, done = |u_new - u|_F < eps (qp_wrapper.py:392), one more round applied.
// first: round 0, which writes the whole state whatever it held; nparts == 0: the empty call from round 0, a reset only.
__global__ __launch_bounds__(256) void sqp_finish_kernel(const double *partial, int nparts, double eps, int32_t *state,
                                                         int first)
{
    __shared__ double part[256];
    if (nparts == 0) {
        if (threadIdx.x < 4) state[threadIdx.x] = 0;
        return;
    }
    if (!first && state[0]) return;
    double a = 0.0;
    for (int base = 0; base < nparts; base += 256) {
        part[threadIdx.x] = base + (int)threadIdx.x < nparts ? partial[base + threadIdx.x] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = nparts - base < 256 ? nparts - base : 256;
            for (int j = 0; j < cnt; ++j) a += part[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        state[1] = first ? 1 : state[1] + 1;
        state[0] = sqrt(a) < eps ? 1 : 0;
        if (first) state[2] = state[3] = 0;
    }
}

int grid_for(long long total)
{
    const long long g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

template <class Map, int KC>
int run_linearize(long long N, const double *x, const double *u, double dt, double *F, double *f, const int32_t *state,
                  hipStream_t st)
{
    DQP_LAUNCH((sqp_linearize_kernel<Map, KC>), dim3(grid_for(N)), dim3(256), 0, st, N, x, u, dt, F, f, state);
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}

// one instantiation per model, at the model's KC
int linearize(int dyn_id, long long N, double dt, const double *x, const double *u, double *F, double *f,
              const int32_t *state, hipStream_t st)
{
    return dqp::dyn::visit<int>(dyn_id, DQP_ERR_BAD_ARG, [&](auto model) {
        using M = decltype(model);
        return run_linearize<typename M::Map, M::KC>(N, x, u, dt, F, f, state, st);
    });
}

// DQP_OK: dims name a registered model of their own sizes
int model_dims(const dqp_mpc_dims *d)
{
    if (!d || d->nbatch < 0 || d->n_state <= 0 || d->n_ctrl <= 0 || d->T < 2) return DQP_ERR_BAD_ARG;
    return dqp::dyn::model_matches(d->dyn_id, d->n_state, d->n_ctrl) ? DQP_OK : DQP_ERR_BAD_ARG;
}

// the caller's workspace, in doubles (include/dqp.h: dqp_mpc_sqp_workspace_bytes)
struct Ws {
    double *F, *f, *tau, *lam, *nu, *slack, *info, *resid, *du, *xn, *un, *alpha, *cost, *partial, *qp, *term;
    size_t doubles;
};

size_t nparts(const dqp_mpc_dims *d) { return ((size_t)d->nbatch + KEEP_BLOCK - 1) / KEEP_BLOCK; }

Ws layout(const dqp_mpc_dims *d, const dqp_opts *o, double *base)
{
    const size_t B = d->nbatch, n = d->n_state, m = d->n_ctrl, T = d->T, nt = n + m;
    Ws w;
    size_t at = 0;
    // every array starts on 16 bytes, like the tensors the Python loop hands to the QP and the line search
    auto take = [&](size_t count) { double *p = base ? base + at : nullptr; at += (count + 1) & ~(size_t)1; return p; };
    w.F = take((T - 1) * B * n * nt);
    w.f = take((T - 1) * B * n);
    w.tau = take(B * T * nt);
    w.lam = take(2 * B * T * m);
    w.nu = take(B * T * n);
    w.slack = take(2 * B * T * m);
    w.info = take(B);                   // (B, 2) int32
    w.resid = take(B);
    w.du = take(T * B * m);
    w.xn = take(T * B * n);
    w.un = take(T * B * m);
    w.alpha = take(B);
    w.cost = take(B);
    w.partial = take(nparts(d));
    w.qp = take((dqp_mpc_qp_workspace_bytes(d) + 7) / 8);
    w.term = take((dqp_mpc_qp_termination_bytes(d, o) + 7) / 8);
    w.doubles = at;
    return w;
}

}  // namespace
}  // namespace sqp
}  // namespace dqp

using namespace dqp;
using namespace dqp::sqp;

extern "C" {

__attribute__((visibility("default"))) int dqp_mpc_linearize(const dqp_mpc_dims *d, double dt, const double *x,
                                                             const double *u, double *F, double *f, void *stream)
{
    const int rc = model_dims(d);
    if (rc != DQP_OK) return rc;
    if (d->nbatch == 0) return DQP_OK;
    if (!x || !u || !F || !f) return DQP_ERR_BAD_ARG;
    return linearize(d->dyn_id, (long long)(d->T - 1) * d->nbatch, dt, x, u, F, f, nullptr, (hipStream_t)stream);
}

__attribute__((visibility("default"))) int dqp_mpc_sqp_supported(const dqp_mpc_dims *d)
{
    if (model_dims(d) != DQP_OK || !d->has_bounds || d->n_state_host != 0) return 0;
    if (d->n_state > LS_MAXN || d->n_ctrl > LS_MAXM) return 0;
    return dqp_mpc_qp_supported(d) == 1 ? 1 : 0;
}

__attribute__((visibility("default"))) size_t dqp_mpc_sqp_workspace_bytes(const dqp_mpc_dims *d, const dqp_opts *o)
{
    if (!o || !dqp_mpc_sqp_supported(d) || d->nbatch <= 0) return 0;
    return layout(d, o, nullptr).doubles * sizeof(double);
}

__attribute__((visibility("default"))) int
dqp_mpc_sqp_rounds(const dqp_mpc_dims *d, const dqp_opts *opts, const double *C, const double *c, const double *x0,
                   const dqp_mpc_bounds *bounds, double decay, int32_t max_linesearch_iter, double best_cost_eps,
                   double eps, int32_t round_begin, int32_t round_end, double *x, double *u, double *keep_x,
                   double *keep_u, double *keep_cost, int32_t *state, void *workspace, void *stream)
{
    int rc = model_dims(d);
    if (rc != DQP_OK) return rc;
    if (!d->has_bounds || d->n_state_host != 0 || !opts) return DQP_ERR_BAD_ARG;
    if (!dqp_mpc_sqp_supported(d)) return DQP_ERR_TOO_LARGE;
    if ((rc = mpc_bounds_layout(bounds, d)) != DQP_OK) return rc;
    if (d->nbatch == 0) return DQP_OK;
    if (!C || !c || !x0 || !bounds->lower || !bounds->upper || !x || !u || !keep_x || !keep_u || !keep_cost || !state ||
        !workspace)
        return DQP_ERR_BAD_ARG;
    if (round_begin < 0 || round_end < round_begin || max_linesearch_iter < 1) return DQP_ERR_BAD_ARG;
    if (!(opts->dyn_dt > 0.0)) return DQP_ERR_BAD_ARG;             // the model's step
    hipStream_t st = (hipStream_t)stream;
    const Ws w = layout(d, opts, (double *)workspace);
    const int B = d->nbatch, n = d->n_state, m = d->n_ctrl, T = d->T, parts = (int)nparts(d);
    if (round_begin == 0 && round_end == 0)        // nothing to run: the reset alone
        DQP_LAUNCH(sqp_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)w.partial, 0, eps, state, 1);
    void *term = dqp_mpc_qp_termination_bytes(d, opts) ? (void *)w.term : nullptr;
    for (int r = round_begin; r < round_end; ++r) {
        const int32_t *seen = r == 0 ? nullptr : state;        // round 0 runs whatever `state` holds
        if ((rc = linearize(d->dyn_id, (long long)(T - 1) * B, opts->dyn_dt, x, u, w.F, w.f, seen, st)) != DQP_OK) return rc;
        rc = dqp_mpc_qp_forward_bounds(d, opts, C, c, w.F, w.f, x0, bounds, w.tau, w.lam, w.nu, w.slack, (int32_t *)w.info,
                                       w.resid, w.qp, term, stream);
        if (rc != DQP_OK) return rc;
        const StepP sp = {w.tau, u, w.du, seen, B, n, m, T};
        DQP_LAUNCH(sqp_step_kernel, dim3(grid_for((long long)T * B * m)), dim3(256), 0, st, sp);
        rc = dqp_mpc_line_search(d, d->dyn_id, opts->dyn_dt, nullptr, nullptr, x0, x, u, w.du, C, c, decay,
                                 max_linesearch_iter, w.xn, w.un, w.alpha, w.cost, stream);
        if (rc != DQP_OK) return rc;
        const KeepP kp = {w.xn, w.un, w.cost, x, u, keep_x, keep_u, keep_cost, w.partial, state, best_cost_eps,
                          B, n, m, T, r == 0 ? 1 : 0};
        DQP_LAUNCH(sqp_keep_kernel, dim3(parts), dim3(KEEP_BLOCK), 0, st, kp);
        DQP_LAUNCH(sqp_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)w.partial, parts, eps, state, r == 0 ? 1 : 0);
        if (hipGetLastError() != hipSuccess) return DQP_ERR_LAUNCH;
    }
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}

}  // extern "C"
