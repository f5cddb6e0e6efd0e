// dqp_al_fused.hip -- AL_mpc.MPC.al_solve for a registered device model as ONE kernel launch (dqp_al_mpc_solve_fused).
//
// dqp_al_mpc_solve (dqp_al.hip) is a train of 25 to 30 launches at al_iter = 2: al_start_kernel, then per AL iteration
// a merit launch, four x [al_banded_newton_kernel, al_ls_group_kernel (+ al_select_kernel)] and al_outer_kernel.  At
// the reference's training batch (B = 128) every one of them is a 20 - 30 us latency chain on a handful of wavefronts
// that re-reads xu, Qd, q and lam from HBM.  Everything in al_solve is independent per problem (the sticky
// cholesky_fail switch aside, which stays a flag the host looks at), so here one problem is one workgroup of ONE
// wavefront that runs the whole solve with the problem on chip:
//
//   LDS       xu, upd, y, Qd, q (T nt each), lam (ncon), the Jacobian columns / residuals of every knot, the
//             block-tridiagonal factor of the current Newton step, the 20 candidate merits
//   model     the wavefront is eight 8-lane groups (Grp<8>, a knot of nt <= 8 rows per group).  The forward-mode
//             Jacobians of a Newton step are evaluated for EIGHT knots at once: group g takes knots g, g + 8, ...,
//             lane r of it the seed e_r -- ceil((T - 1) / 8) model evaluations per step on the chain instead of T - 1
//   sweep     the block Cholesky sweep of al_banded_newton_kernel (the same primitives: chol_g, unit_lower, trsv_unit,
//             trsvT_bcast), replicated in the eight groups -- a SIMD instruction costs the same for 8 or 64 lanes, and
//             no group waits for another; group 0 writes the factor and the update to LDS
//   search    the 20 candidates xu + 2^-k upd over the groups (group g: k = g, g + 8, g + 16: three rounds instead of
//             twenty), lane r of a group the knots r, r + 8, ...; then the wavefront argmin of al_select_kernel
//   outer     one knot per lane: lam <- clamp(lam + rho res), cost, |res_clamp|, rho <- 10 rho, history row i + 1
//
// HBM sees the inputs once, then the history rows, xu, res_norm, status, fail and the ONE kept factor (the last Newton
// step of the last AL iteration), in the layout dqp_al_banded_solve reads: per (b, t) element c of lane r's row at
// [c nt + r] -- the same for every lane-group width (BandCfg), so NewtonAL.backward is unchanged.
//
// No wait on another workgroup anywhere: no cooperative launch, no grid barrier, no flag to spin on; the barriers
// below are workgroup barriers of a one-wavefront workgroup.  All stores are plain vector stores, the `fail` flag an
// ordinary atomicOr as in al_select_kernel.
//
// Scope: registered models with n_state + n_ctrl <= 8 (the two pendulums, PendulumDx, cartpole-1, cartpole-2, the integrator),
// 2 <= T <= 32, fp64.  RexQuadrotor (12 + 4) stays on the multi-launch path.
//
// State box (dqp_al_mpc_solve_fused_xbounds): the BoxBounds<Model> instantiations, one per model above.  Both boxes are
// read through their strides and staged in LDS once at the start; lam and the history rows carry the 2 T n state rows
// behind the control rows (AlRows::state).  A state pair enters the gradient and the diagonal of H_tt of its knot in
// the sweep (lanes r < nx, at the iterate), the merit of the knot's owner (knot 0 at the pinned x0) and the outer
// update of the knot's lane; the factor keeps its shape.  Everything it adds sits behind `if constexpr (XB)`.
#include "dqp_al_banded_kernels.h"

namespace {

struct FusedP {
    const double *x_init, *u_init, *x0, *Qd, *q, *ul, *uu, *lam_in, *rho_in;
    const double *prev_cost, *prev_lam, *prev_rho;      // previous call's history, oldest first, or NULL (n_prev = 0)
    double *xu, *hist_cost, *hist_lam, *hist_rho, *res_norm, *fac, *status;
    int32_t *fail;
    double dt;
    int B, T, al_iter, newton_steps, n_prev;
    long long bsb, bst;         // bound layout (dqp_al_bounds.h), read by the StridedBounds<> instantiations only
    const double *xlo, *xhi;    // state box, read by the BoxBounds<> instantiations only (else NULL): lower / upper of
    long long xsb, xst;         // (b, t, k) at [b xsb + t xst + k]; lam and the history rows then carry 2 T n more rows
};

using dqp::AlRows;
using dqp::AL_NCAND;
constexpr int FG = 8, FNG = 64 / FG;      // lanes per group, groups per wavefront

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// LDS carve of one problem, in doubles
template <class Map> struct FusedLds {
    using C = BandCfg<Map>;
    static constexpr int NX = C::NX, NU = C::NU, NT = C::NT;
    static constexpr int JBK = NX * (NT + 1);         // per knot: NX rows of [J[j][0 .. nt-1], res_j]
    // BoxBounds<>: + the 2 T nx state rows of lam and the problem's state bounds, upper (T, nx) then lower (T, nx)
    static constexpr bool XB = box_bounds<Map>::value;
    __host__ __device__ static int ncon(int T) { return AlRows{NX, NU, T, XB}.ncon(); }
    // StridedBounds<>: + the problem's own bounds, upper (T, nu) then lower (T, nu), staged once at the start
    static constexpr bool SB = strided_bounds<Map>::value;
    __host__ __device__ static size_t doubles(int T)
    {
        return (size_t)5 * T * NT + ncon(T) + (size_t)T * JBK + (size_t)T * NT * C::ROW + 32 + (SB ? (size_t)2 * T * NU : 0) +
               (XB ? (size_t)2 * T * NX : 0);
    }
};

template <class Map>
__global__ __launch_bounds__(64) void al_solve_fused_kernel(FusedP P)
{
    using C = BandCfg<Map>;
    using Gr = Grp<FG>;
    using Lds = FusedLds<Map>;
    constexpr int NX = C::NX, NU = C::NU, NT = C::NT, ROW = C::ROW, JBK = Lds::JBK;
    static_assert(NT <= FG, "a knot must fit an 8-lane group");
    const int lane = threadIdx.x, r = lane & (FG - 1), grp = lane / FG;
    const long long b = blockIdx.x;
    const int T = P.T, nz = T * NT;
    constexpr bool XB = Lds::XB;
    const AlRows R = {NX, NU, T, XB};
    const int ncon = R.ncon();
    const bool inT = r < NT;
    const int rr = inT ? r : 0, rx = r < NX ? r : 0, iu = (inT && r >= NX) ? r - NX : 0;

    extern __shared__ __attribute__((aligned(16))) double fs[];
    double *s_xu = fs, *s_upd = s_xu + nz, *s_y = s_upd + nz, *s_Qd = s_y + nz, *s_q = s_Qd + nz;
    double *s_lam = s_q + nz, *s_jb = s_lam + ncon, *s_fac = s_jb + T * JBK, *s_merit = s_fac + T * NT * ROW;
    constexpr bool SB = Lds::SB;
    [[maybe_unused]] double *s_uu = s_merit + 32, *s_ul = s_uu + T * NU;       // SB only (FusedLds::doubles)
    [[maybe_unused]] double *s_xhi = s_ul + T * NU, *s_xlo = s_xhi + T * NX;    // XB only
    // the group's tile for the transposed copies of the sweep (element (row, col) at [col TS + row])
    constexpr int TS = FG + 2, PS = FG * TS;
    __shared__ __attribute__((aligned(16))) double trs[FNG * PS];
    double *trow = trs + grp * PS + r;
    const double *tcol = trs + grp * PS + r * TS;

    double x0v[NX], uuv[NU], ulv[NU];
#pragma unroll
    for (int j = 0; j < NX; ++j) x0v[j] = P.x0[b * NX + j];
#pragma unroll
    for (int i = 0; i < NU; ++i) { uuv[i] = P.uu[i]; ulv[i] = P.ul[i]; }
    const double x0r = P.x0[b * NX + rx], uur = P.uu[iu], ulr = P.ul[iu];
    if constexpr (SB) {         // visible to every lane behind the barrier that closes the start phase
        for (int e = lane; e < T * NU; e += 64) {
            const int t = e / NU, i = e - t * NU;
            const long long o = dqp::al_bound_at<true>(b, t, i, P.bsb, P.bst);
            s_uu[e] = P.uu[o]; s_ul[e] = P.ul[o];
        }
    }
    if constexpr (XB) {
        for (int e = lane; e < T * NX; e += 64) {
            const int t = e / NX, j = e - t * NX;
            const long long o = dqp::al_bound_at<true>(b, t, j, P.xsb, P.xst);
            s_xhi[e] = P.xhi[o]; s_xlo[e] = P.xlo[o];
        }
    }
    // the bounds of control i of knot t: staged (SB) or the vector's element
    auto upper = [&](int t, int i) { if constexpr (SB) return s_uu[t * NU + i]; else return uuv[i]; };
    auto lower = [&](int t, int i) { if constexpr (SB) return s_ul[t * NU + i]; else return ulv[i]; };

    // ---- start (al_start_kernel): xu = [x_init | u_init], cost_start, warm start of (lam, rho), history row 0
    double rho;
    {
        const double *Qd = P.Qd + b * (long long)nz, *q = P.q + b * (long long)nz;
        double quad = 0.0, lin = 0.0;
        for (int e = lane; e < nz; e += 64) {
            const int t = e / NT, j = e - t * NT;
            const double v = j < NX ? P.x_init[(b * T + t) * NX + j] : P.u_init[(b * T + t) * NU + (j - NX)];
            const double qd = Qd[e], ql = q[e];
            s_xu[e] = v; s_Qd[e] = qd; s_q[e] = ql;
            quad += v * qd * v;
            lin += ql * v;
        }
        const double cost0 = 0.5 * wave_sum(quad) + wave_sum(lin);       // al_utils.compute_cost, diagonal cost
        const double *lam = P.lam_in + b * (long long)ncon;
        const dqp::AlWarm w = dqp::al_warm_start(P.n_prev, P.B, b, ncon, cost0, P.prev_cost, P.prev_lam, P.prev_rho, lam,
                                                 P.rho_in[b], lane, 64, [](double v) { return wave_sum(v); });
        rho = w.rho;
        double *l0 = P.hist_lam + b * (long long)ncon;
        for (int e = lane; e < ncon; e += 64) {
            const double v = P.n_prev > 0 ? lam[e] * w.scale : lam[e];
            s_lam[e] = v; l0[e] = v;
        }
        if (lane == 0) { P.hist_cost[b] = cost0; P.hist_rho[b] = rho; }
    }
#pragma unroll
    for (int j = NX; j < FG; ++j) trow[j * TS] = 0.0;       // columns nx .. 7 of the M^T tile stay zero
    __syncthreads();

    // merit (al_utils.py:37-59) of xu + step upd with x_0 pinned to x0 (al_utils.py:515), terms as al_ls_group_kernel:
    // lane r of a group sums the cost, box and dynamics terms of the knots r, r + 8, ...; in every lane of the group
    auto merit_at = [&](double step, bool with_upd) -> double {
        double acc = 0.0;
        for (int t = r; t < T; t += FG) {
            double z[NT], xn[NX];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const double u = with_upd ? s_upd[t * NT + j] : 0.0;
                z[j] = fma(step, u, s_xu[t * NT + j]);
                if (j < NX && t == 0) z[j] = x0v[j < NX ? j : 0];
                acc += dqp::al_cost_term(s_Qd[t * NT + j], s_q[t * NT + j], z[j]);
            }
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const int row = R.ctrl(t) + i;
                acc += dqp::al_pair_term(rho, s_lam[row], s_lam[row + NU], z[NX + i] - upper(t, i), lower(t, i) - z[NX + i]);
            }
            if constexpr (XB) {         // the knot's state pairs (knot 0 at the pinned x0), read where they are used
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    const int row = R.state(t) + j;
                    acc += dqp::al_pair_term(rho, s_lam[row], s_lam[row + NX], z[j] - s_xhi[t * NX + j], s_xlo[t * NX + j] - z[j]);
                }
            }
            if (t < T - 1) {
                Map::template step<double>(z, z + NX, P.dt, xn);
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    const double u = with_upd ? s_upd[(t + 1) * NT + j] : 0.0;
                    const double res = fma(step, u, s_xu[(t + 1) * NT + j]) - xn[j];
                    acc += dqp::al_eq_term(rho, s_lam[R.eq(t) + j], res);
                }
            }
        }
        return Gr::sum(acc);
    };

    double take_last = 0.0;
    for (int it = 0; it < P.al_iter; ++it) {
        double merit_cur = merit_at(0.0, false);           // merit at the start of this AL iteration
        int bad_any = 0;
        for (int ns = 0; ns < P.newton_steps; ++ns) {
            // ---- Jacobian column r of knots grp, grp + 8, ...: one forward-mode seed per lane
            for (int t = grp; t < T - 1; t += FNG) {
                Dual<1> xs[NX], us[NU], out[NX];
#pragma unroll
                for (int j = 0; j < NX; ++j) { xs[j] = Dual<1>(s_xu[t * NT + j]); xs[j].d[0] = (r == j) ? 1.0 : 0.0; }
#pragma unroll
                for (int j = 0; j < NU; ++j) { us[j] = Dual<1>(s_xu[t * NT + NX + j]); us[j].d[0] = (r == NX + j) ? 1.0 : 0.0; }
                Map::template step<Dual<1>>(xs, us, P.dt, out);
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    if (inT) s_jb[t * JBK + j * (NT + 1) + r] = out[j].d[0];
                    if (r == 0) s_jb[t * JBK + j * (NT + 1) + NT] = s_xu[(t + 1) * NT + j] - out[j].v;   // x_{t+1} - f(x_t, u_t)
                }
            }
            __syncthreads();
            // ---- forward sweep over the knots (al_banded_newton_kernel), the same in every group
            double Mprev[NX], yprev = 0.0, mu_prev[NX];
            int bad = 0;
#pragma unroll
            for (int j = 0; j < NX; ++j) { Mprev[j] = 0.0; mu_prev[j] = 0.0; }
            const double lam_first = s_lam[R.eq(T - 1) + rx];
            for (int t = 0; t < T; ++t) {
                const bool dynrow = t < T - 1;
                const int tj = dynrow ? t : 0;
                double Jc[NX], mu[NX];
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    const double col = s_jb[tj * JBK + j * (NT + 1) + rr], res = s_jb[tj * JBK + j * (NT + 1) + NT];
                    Jc[j] = (dynrow && inT) ? col : 0.0;
                    mu[j] = dynrow ? s_lam[R.eq(tj) + j] + rho * res : 0.0;
                }
                const double zr = s_xu[t * NT + rr], qdr = s_Qd[t * NT + rr], qr = s_q[t * NT + rr];
                const int row = R.ctrl(t) + iu;
                const double lup = s_lam[row], llo = s_lam[row + NU];
                // gradient element r of this knot, and the diagonal terms of H_tt
                double g = qdr * zr + qr, dg = qdr;
#pragma unroll
                for (int j = 0; j < NX; ++j) g -= Jc[j] * mu[j];
                {
                    double prev = 0.0;
#pragma unroll
                    for (int j = 0; j < NX; ++j) prev = (r == j) ? mu_prev[j] : prev;
                    const double first = lam_first + rho * (zr - x0r);
                    double rup, rlo;
                    if constexpr (SB) { rup = zr - s_uu[t * NU + iu]; rlo = s_ul[t * NU + iu] - zr; }    // once per knot
                    else { rup = zr - uur; rlo = ulr - zr; }
                    if (r < NX) {
                        g += (t > 0) ? prev : first;
                        dg += rho;
                        if constexpr (XB) {     // the knot's state pair of element r, at the iterate (knot 0 too)
                            const int xrow = R.state(t) + rx;
                            const double xup = zr - s_xhi[t * NX + rx], xlw = s_xlo[t * NX + rx] - zr;
                            g += (s_lam[xrow] + rho * fmax(xup, 0.0)) - (s_lam[xrow + NX] + rho * fmax(xlw, 0.0));
                            dg += rho * ((xup > 0.0 ? 1.0 : 0.0) + (xlw > 0.0 ? 1.0 : 0.0));
                        }
                    } else if (inT) {
                        g += (lup + rho * fmax(rup, 0.0)) - (llo + rho * fmax(rlo, 0.0));
                        dg += rho * ((rup > 0.0 ? 1.0 : 0.0) + (rlo > 0.0 ? 1.0 : 0.0));
                    }
                }
                // H_tt row r: rho J^T J + diag - Gram(M_prev) on the x-x block
                double H[1][NT], rd[1];
#pragma unroll
                for (int c = 0; c < NT; ++c) {
                    double a = 0.0;
#pragma unroll
                    for (int j = 0; j < NX; ++j) a = fma(Jc[j], Gr::rb(Jc[j], c), a);
                    H[0][c] = rho * a + ((r == c) ? dg : 0.0);
                }
                double Mt[FG];
#pragma unroll
                for (int k = 0; k < FG; ++k) Mt[k] = tcol[k];
                if (t > 0) {
#pragma unroll
                    for (int j = 0; j < NX; ++j) {
                        double a = 0.0;
#pragma unroll
                        for (int k = 0; k < NT; ++k) a = fma(Mt[k], Gr::rb(Mprev[j], k), a);
                        H[0][j] -= a;
                    }
                }
#pragma unroll
                for (int c = 0; c < NT; ++c) H[0][c] = inT ? H[0][c] : ((r == c) ? 1.0 : 0.0);
                if (!chol_g<FG, NT>(H, rd, r) && bad == 0) bad = t + 1;
                // right-hand side: y_t = L_tt^-1 (-g_t - L_{t,t-1} y_{t-1})
                double y = inT ? -g : 0.0;
                if (t > 0) {
                    double a = 0.0;
#pragma unroll
                    for (int k = 0; k < NT; ++k) a = fma(Mt[k], Gr::rb(yprev, k), a);
                    y -= a;
                }
                double *o = s_fac + t * NT * ROW + rr;
                const bool wr = grp == 0 && inT;
                if (wr) {
#pragma unroll
                    for (int c = 0; c < NT; ++c) o[c * NT] = H[0][c];
                    o[NT * NT] = rd[0];
                }
                unit_lower<FG, NT>(H, rd, r);
                const double rdm = inT ? rd[0] : 0.0, nrho_rd = -rho * rdm;
                y = trsv_unit<FG, NT>(H, y) * rdm;
                // M_t = L_tt^-1 H_{t+1,t}^T: column j of it is the distributed vector -rho J[j][:]
                double M[NX];
#pragma unroll
                for (int j = 0; j < NX; ++j) M[j] = trsv_unit<FG, NT>(H, Jc[j]) * nrho_rd;
                if (wr) {
#pragma unroll
                    for (int j = 0; j < NX; ++j) o[(NT + 1 + j) * NT] = M[j];
                    s_y[t * NT + r] = y;
                }
#pragma unroll
                for (int j = 0; j < NX; ++j) { Mprev[j] = M[j]; mu_prev[j] = mu[j]; }
                yprev = inT ? y : 0.0;
                __syncthreads();            // every lane has read M_{t-1}^T before M_t^T replaces it
#pragma unroll
                for (int j = 0; j < NX; ++j) trow[j * TS] = M[j];
                __syncthreads();
            }
            bad_any |= bad;
            // ---- backward sweep: upd_t = L_tt^-T (y_t - M_t upd_{t+1}[:NX])
            double xnext = 0.0;
            for (int t = T - 1; t >= 0; --t) {
                const double *o = s_fac + t * NT * ROW + rr;
                double L[1][NT], M[NX];
#pragma unroll
                for (int c = 0; c < NT; ++c) L[0][c] = inT ? o[c * NT] : 0.0;
                const double rdv = inT ? o[NT * NT] : 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) M[j] = inT ? o[(NT + 1 + j) * NT] : 0.0;
                double v = inT ? s_y[t * NT + rr] : 0.0;
                if (t < T - 1) {
#pragma unroll
                    for (int j = 0; j < NX; ++j) v = fma(-M[j], Gr::rb(xnext, j), v);
                }
                __syncthreads();
                v = trsvT_bcast<FG, NT, TS>(L, rdv, v, trow, tcol, r);
                if (grp == 0 && inT) s_upd[t * NT + r] = v;
                xnext = inT ? v : 0.0;
            }
            __syncthreads();
            // the backward sweep used the tile's columns nx .. 7: zero again for the next forward sweep
#pragma unroll
            for (int j = NX; j < FG; ++j) trow[j * TS] = 0.0;
            // ---- the kept factor: the last Newton step of the last AL iteration, in dqp_al_banded_solve's layout
            if (it == P.al_iter - 1 && ns == P.newton_steps - 1) {
                double *fo = P.fac + b * (long long)T * NT * ROW;
                for (int e = lane; e < T * NT * ROW; e += 64) fo[e] = s_fac[e];
            }
            // ---- line search: candidate k on group k % 8 (the surplus candidates of the last round are discarded)
            for (int k0 = 0; k0 < AL_NCAND; k0 += FNG) {
                const int k = k0 + grp;
                const double acc = merit_at(dqp::al_step(k), true);
                if (r == 0 && k < AL_NCAND) s_merit[k] = acc;
            }
            __syncthreads();
            // the best candidate (al_select_kernel), acceptance, update of the iterate
            {
                const bool has = lane < AL_NCAND;
                const dqp::AlBest best = dqp::al_wave_argmin(has ? s_merit[lane] : INFINITY, has);
                const bool take = best.merit < merit_cur;
                merit_cur = best.merit;                             // new_merit regardless of acceptance
                take_last = take ? 1.0 : 0.0;
                if (take) {
                    const double sb = dqp::al_step(best.arg);
                    for (int e = lane; e < nz; e += 64) s_xu[e] = e < NX ? P.x0[b * NX + e] : fma(sb, s_upd[e], s_xu[e]);
                }
            }
            __syncthreads();
        }
        if (lane == 0 && bad_any != 0) atomicOr(P.fail + it, 1);    // Cholesky failed: the caller re-runs the slow path
        // ---- outer update (al_outer_kernel): one knot per lane
        {
            double *ln = P.hist_lam + ((long long)(it + 1) * P.B + b) * ncon;
            double cost = 0.0, rn2 = 0.0;
            const int t = lane;
            if (t < T) {
                double z[NT], xn[NX];
#pragma unroll
                for (int j = 0; j < NT; ++j) z[j] = s_xu[t * NT + j];
#pragma unroll
                for (int j = 0; j < NT; ++j) cost += dqp::al_cost_term(s_Qd[t * NT + j], s_q[t * NT + j], z[j]);
                if (t < T - 1) {
                    Map::template step<double>(z, z + NX, P.dt, xn);
#pragma unroll
                    for (int j = 0; j < NX; ++j) {
                        const double res = s_xu[(t + 1) * NT + j] - xn[j];
                        rn2 += res * res;
                        const double v = s_lam[R.eq(t) + j] + rho * res;
                        s_lam[R.eq(t) + j] = v; ln[R.eq(t) + j] = v;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < NX; ++j) {
                        const double res = s_xu[j] - x0v[j];
                        rn2 += res * res;
                        const double v = s_lam[R.eq(t) + j] + rho * res;
                        s_lam[R.eq(t) + j] = v; ln[R.eq(t) + j] = v;
                    }
                }
#pragma unroll
                for (int i = 0; i < NU; ++i) {
                    const int row = R.ctrl(t) + i;
                    const dqp::AlPairUpdate u = dqp::al_pair_update(rho, s_lam[row], s_lam[row + NU], z[NX + i] - upper(t, i),
                                                                    lower(t, i) - z[NX + i]);
                    rn2 += u.sq;
                    s_lam[row] = u.up; ln[row] = u.up;
                    s_lam[row + NU] = u.lo; ln[row + NU] = u.lo;
                }
                if constexpr (XB) {     // the knot's state rows: multipliers clamped at 0, their share of |res_clamp|
#pragma unroll
                    for (int j = 0; j < NX; ++j) {
                        const int row = R.state(t) + j;
                        const dqp::AlPairUpdate u = dqp::al_pair_update(rho, s_lam[row], s_lam[row + NX], z[j] - s_xhi[t * NX + j],
                                                                        s_xlo[t * NX + j] - z[j]);
                        rn2 += u.sq;
                        s_lam[row] = u.up; ln[row] = u.up;
                        s_lam[row + NX] = u.lo; ln[row + NX] = u.lo;
                    }
                }
            }
            cost = wave_sum(cost);
            rn2 = wave_sum(rn2);
            if (lane == 0) {
                P.hist_cost[(long long)(it + 1) * P.B + b] = cost;
                P.res_norm[b] = sqrt(rn2);
                P.hist_rho[(long long)(it + 1) * P.B + b] = rho * 10.0;
            }
            rho = rho * 10.0;                                        // AL_mpc.py:307
        }
        __syncthreads();
    }
    double *xo = P.xu + b * (long long)nz;
    for (int e = lane; e < nz; e += 64) xo[e] = s_xu[e];
    if (lane == 0 && P.status) P.status[b] = take_last;
}

// static LDS of the kernel (the groups' tiles) next to the dynamic carve: within the 64 KB a launch gets without opt-in
constexpr size_t FUSED_STATIC_LDS = (size_t)FNG * FG * (FG + 2) * sizeof(double);
constexpr size_t FUSED_LDS_LIMIT = 64 * 1024;

// `strided`: the StridedBounds<> instantiation, whose carve also holds the problem's 2 T n_ctrl bounds; `xbox`: the
// BoxBounds<> one, which stages both boxes and holds the 2 T n_state state rows of lam
template <class Map> size_t fused_lds_bytes(int T, bool strided, bool xbox)
{
    if (xbox) return FusedLds<BoxBounds<Map>>::doubles(T) * sizeof(double);
    return (strided ? FusedLds<StridedBounds<Map>>::doubles(T) : FusedLds<Map>::doubles(T)) * sizeof(double);
}

size_t fused_lds(int dyn_id, int T, bool strided = false, bool xbox = false)
{
    return dqp::dyn::visit<size_t>(dyn_id, 0, [&](auto model) -> size_t {
        using Map = typename decltype(model)::Map;
        if constexpr (Map::NX + Map::NU <= FG) return fused_lds_bytes<Map>(T, strided, xbox);
        else return 0;          // the knot does not fit a group's tile
    });
}

bool fused_ok(const dqp_al_mpc_dims *d, int dyn_id, bool strided = false, bool xbox = false)
{
    if (!d || d->T < 2 || d->T > 32 || d->nbatch < 0) return false;
    if (!dqp::dyn::model_matches(dyn_id, d->n_state, d->n_ctrl) || d->n_state + d->n_ctrl > FG) return false;
    const size_t lds = fused_lds(dyn_id, d->T, strided, xbox);
    return lds > 0 && lds + FUSED_STATIC_LDS <= FUSED_LDS_LIMIT;
}

template <class Model> int launch_fused(const FusedP &P, size_t lds, hipStream_t st)
{
    if (P.xlo)          // a state box: both boxes strided
        DQP_LAUNCH(al_solve_fused_kernel<BoxBounds<Model>>, dim3((unsigned)P.B), dim3(64), lds, st, P);
    else if (P.bsb != 0 || P.bst != 0)
        DQP_LAUNCH(al_solve_fused_kernel<StridedBounds<Model>>, dim3((unsigned)P.B), dim3(64), lds, st, P);
    else
        DQP_LAUNCH(al_solve_fused_kernel<Model>, dim3((unsigned)P.B), dim3(64), lds, st, P);
    return dqp::launched();
}

// Behind either front check (v.lam / v.rho: lam_in / rho_in): nbatch == 0, the buffers and the model, the kernel's limits
int fused_solve(const dqp_al_mpc_dims *d, const dqp::AlProblem &v, const dqp::AlMpcIo &io)
{
    const int dyn_id = v.model;
    if (const int r = v.ready(io.buffers_set() && v.model_ok()); r != 1) return r;
    if (!fused_ok(d, dyn_id, v.strided(), v.has_x)) return DQP_ERR_TOO_LARGE;
    // the flags are OR-ed into by every workgroup: cleared in front of the launch (a memset node under capture)
    if (hipMemsetAsync(io.fail, 0, sizeof(int32_t) * (size_t)io.al_iter, v.stream) != hipSuccess) return DQP_ERR_LAUNCH;
    FusedP P = {};
    P.x_init = io.x_init; P.u_init = io.u_init; P.x0 = v.x0; P.Qd = v.Qd; P.q = v.q; P.ul = v.u.lower; P.uu = v.u.upper;
    P.lam_in = v.lam; P.rho_in = v.rho; P.prev_cost = io.prev_cost; P.prev_lam = io.prev_lam; P.prev_rho = io.prev_rho;
    P.xu = io.xu; P.hist_cost = io.hist_cost; P.hist_lam = io.hist_lam; P.hist_rho = io.hist_rho; P.res_norm = io.res_norm;
    P.fac = io.factor; P.status = io.status; P.fail = io.fail; P.bsb = v.u.stride_b; P.bst = v.u.stride_t;
    P.xlo = v.x.lower; P.xhi = v.x.upper; P.xsb = v.x.stride_b; P.xst = v.x.stride_t;     // NULL / 0 without a state box
    P.dt = v.dt; P.B = v.B; P.T = v.T; P.al_iter = io.al_iter; P.newton_steps = io.newton_steps; P.n_prev = io.n_prev;
    const size_t lds = fused_lds(dyn_id, v.T, v.strided(), v.has_x);
    return dqp::dyn::visit<int>(dyn_id, DQP_ERR_TOO_LARGE, [&](auto model) -> int {
        using Map = typename decltype(model)::Map;
        if constexpr (Map::NX + Map::NU <= FG) return launch_fused<Map>(P, lds, v.stream);
        else return DQP_ERR_TOO_LARGE;
    });
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int dqp_al_mpc_solve_fused_supported(const dqp_al_mpc_dims *d, int dyn_id)
{
    return fused_ok(d, dyn_id) ? 1 : 0;
}

// the problem lives in LDS: no workspace of its own.  The size of dqp_al_mpc_solve's is reported so that a caller that
// switches between the two entries by name can keep one buffer.
__attribute__((visibility("default"))) size_t dqp_al_mpc_solve_fused_bytes(const dqp_al_mpc_dims *d)
{
    return dqp_al_mpc_solve_bytes(d);
}

__attribute__((visibility("default"))) int
dqp_al_mpc_solve_fused_supported_bounds(const dqp_al_mpc_dims *d, int dyn_id, const dqp_al_bounds *bounds)
{
    if (dqp::al_bounds_layout(bounds, d) != DQP_OK) return 0;
    return fused_ok(d, dyn_id, dqp::al_bounds_strided(bounds)) ? 1 : 0;
}

// the staged bounds live in LDS (dqp_al_mpc_solve_fused_lds_bytes), not in the workspace: the size of the vector call
__attribute__((visibility("default"))) size_t
dqp_al_mpc_solve_fused_bytes_bounds(const dqp_al_mpc_dims *d, const dqp_al_bounds *bounds)
{
    if (dqp::al_bounds_layout(bounds, d) != DQP_OK) return 0;
    return dqp_al_mpc_solve_fused_bytes(d);
}

// LDS of one workgroup of the launch: the problem's carve (with the 2 T n_ctrl staged bounds at non-zero strides) plus
// the kernel's static tiles; 0 where dqp_al_mpc_solve_fused_supported_bounds is 0
__attribute__((visibility("default"))) size_t
dqp_al_mpc_solve_fused_lds_bytes(const dqp_al_mpc_dims *d, int dyn_id, const dqp_al_bounds *bounds)
{
    if (!dqp_al_mpc_solve_fused_supported_bounds(d, dyn_id, bounds)) return 0;
    return fused_lds(dyn_id, d->T, dqp::al_bounds_strided(bounds)) + FUSED_STATIC_LDS;
}

__attribute__((visibility("default"))) int
dqp_al_mpc_solve_fused(const dqp_al_mpc_dims *d, int dyn_id, double dt, int32_t al_iter, int32_t newton_steps,
                       const double *x_init, const double *u_init, const double *x0, const double *Qdiag, const double *q,
                       const double *u_lower, const double *u_upper, const double *lam_in, const double *rho_in,
                       const double *prev_cost, const double *prev_lam, const double *prev_rho, int32_t n_prev,
                       double *xu, double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm, double *factor,
                       double *status, int32_t *fail, void *workspace, void *stream)
{
    const dqp_al_bounds bd = {u_lower, u_upper, 0, 0};
    return dqp_al_mpc_solve_fused_bounds(d, dyn_id, dt, al_iter, newton_steps, x_init, u_init, x0, Qdiag, q, &bd, lam_in,
                                         rho_in, prev_cost, prev_lam, prev_rho, n_prev, xu, hist_cost, hist_lam, hist_rho,
                                         res_norm, factor, status, fail, workspace, stream);
}

__attribute__((visibility("default"))) int
dqp_al_mpc_solve_fused_bounds(const dqp_al_mpc_dims *d, int dyn_id, double dt, int32_t al_iter, int32_t newton_steps,
                              const double *x_init, const double *u_init, const double *x0, const double *Qdiag,
                              const double *q, const dqp_al_bounds *bounds, const double *lam_in, const double *rho_in,
                              const double *prev_cost, const double *prev_lam, const double *prev_rho, int32_t n_prev,
                              double *xu, double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm,
                              double *factor, double *status, int32_t *fail, void *workspace, void *stream)
{
    const dqp::AlMpcIo io = {al_iter, newton_steps, x_init, u_init, prev_cost, prev_lam, prev_rho, n_prev,
                             xu, hist_cost, hist_lam, hist_rho, res_norm, factor, status, fail, workspace};
    if (dqp::al_bounds_check(d, bounds) || !io.scalars_ok()) return DQP_ERR_BAD_ARG;
    return fused_solve(d, dqp::al_problem(d, dyn_id, dt, x0, Qdiag, q, lam_in, rho_in, bounds, nullptr, stream), io);
}

// State box (include/dqp.h): the BoxBounds<> instantiations, both boxes read through their strides.  `bounds` may be the
// vector form; the carve is that of the strided call plus the 4 T n_state doubles of the state rows and bounds.
__attribute__((visibility("default"))) int
dqp_al_mpc_solve_fused_supported_xbounds(const dqp_al_mpc_dims *d, int dyn_id, const dqp_al_bounds *bounds,
                                         const dqp_al_bounds *xbounds)
{
    if (!d || d->n_state <= 0 || dqp::al_bounds_layout(bounds, d) != DQP_OK) return 0;
    if (dqp::al_box_layout(xbounds, d, d->n_state) != DQP_OK) return 0;
    return fused_ok(d, dyn_id, true, true) ? 1 : 0;
}

// that of dqp_al_mpc_solve_xbounds_bytes, so that one buffer serves both entries; the kernel does not write to it
__attribute__((visibility("default"))) size_t dqp_al_mpc_solve_fused_bytes_xbounds(const dqp_al_mpc_dims *d)
{
    return dqp_al_mpc_solve_xbounds_bytes(d);
}

__attribute__((visibility("default"))) size_t
dqp_al_mpc_solve_fused_lds_bytes_xbounds(const dqp_al_mpc_dims *d, int dyn_id, const dqp_al_bounds *bounds,
                                         const dqp_al_bounds *xbounds)
{
    if (!dqp_al_mpc_solve_fused_supported_xbounds(d, dyn_id, bounds, xbounds)) return 0;
    return fused_lds(dyn_id, d->T, true, true) + FUSED_STATIC_LDS;
}

__attribute__((visibility("default"))) int
dqp_al_mpc_solve_fused_xbounds(const dqp_al_mpc_dims *d, int model, double dt, int32_t al_iter, int32_t newton_steps,
                               const double *x_init, const double *u_init, const double *x0, const double *Qdiag,
                               const double *q, const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds,
                               const double *lam_in, const double *rho_in, const double *prev_cost, const double *prev_lam,
                               const double *prev_rho, int32_t n_prev, double *xu, double *hist_cost, double *hist_lam,
                               double *hist_rho, double *res_norm, double *factor, double *status, int32_t *fail,
                               void *workspace, void *stream)
{
    const dqp::AlMpcIo io = {al_iter, newton_steps, x_init, u_init, prev_cost, prev_lam, prev_rho, n_prev,
                             xu, hist_cost, hist_lam, hist_rho, res_norm, factor, status, fail, workspace};
    if (const int rc = dqp::al_xbounds_check(d, bounds, xbounds, d && dqp::dyn::model_matches(model, d->n_state, d->n_ctrl)))
        return rc;
    if (!io.scalars_ok()) return DQP_ERR_BAD_ARG;
    return fused_solve(d, dqp::al_problem(d, model, dt, x0, Qdiag, q, lam_in, rho_in, bounds, xbounds, stream), io);
}

}  // extern "C"
