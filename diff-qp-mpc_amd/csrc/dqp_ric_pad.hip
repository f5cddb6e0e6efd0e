// dqp_ric_pad.hip -- stage-wise MPC QPs of any (n, m) with 1 <= m <= 8, n + m <= 32, on the kernels compiled for a
// pair (n', m), n' >= n (dqp_mpc_dims.n_state_host).
//
// The problem is embedded in the larger pair with d = n' - n dummy states after the real ones, knot
// tau'_t = [x_t ; x~_t ; u_t]: C'_t has I_d on the dummy diagonal, c', f', x0' are zero there, the real rows of F'_t read
// [F_x, 0, F_u] and its dummy rows are zero.  The dummy states carry no inequality rows and their equality rows are
// x~_{t+1} = 0, x~_0 = 0, so every Newton system is block-diagonal in (real, dummy): the dummy components of the
// iterates, directions and costates stay exactly zero and the residuals, mu, the step lengths and the batch rule
// are those of the (n, m) problem.  The results equal the native ones up to the association of the lane reductions.
//
// This file: the one interface to the stage-wise kernels (dqp_common.h: stage_*) -- which pairs exist, native or
// host-only, their sizes, and the dispatch over the parts of dqp_ric.hip -- then the layout of the padded copies in the
// caller's workspace and the pack / unpack copies into and out of it.  The pairs and the parts come from _build.py.
#include "dqp_ric_kernels.h"

#if !defined(DQP_RIC_NATIVE_SIZES) || !defined(DQP_RIC_HOST_SIZES) || !defined(DQP_RIC_PARTS)
#error "compile with -DDQP_RIC_NATIVE_SIZES / -DDQP_RIC_HOST_SIZES=\"X(n, m) ...\" and -DDQP_RIC_PARTS=\"PART(name) ...\""
#endif

namespace dqp {

#define X(a, b) (n == a && m == b) ||
bool stage_native(int n, int m) { return DQP_RIC_NATIVE_SIZES false; }
bool stage_supported(int n, int m) { return DQP_RIC_NATIVE_SIZES DQP_RIC_HOST_SIZES false; }
#undef X
int stage_q(int n, int m) { return n + m <= 16 ? 4 : 2; }
long long stage_layout_doubles(int n, int m, int T) { return stage_supported(n, m) ? ric::layout(n, m, T).total : 0; }
int stage_snapshot_doubles(int n, int m, int T) { return stage_supported(n, m) ? T * (2 * n + 5 * m) : 0; }

long long stage_workspace_doubles(int n, int m, int T, int B, bool stepped)
{
    const int q = stage_q(n, m);
    return (long long)((B + q - 1) / q * q) * (stage_layout_doubles(n, m, T) + (stepped ? ric::STEP_STATE : 0));
}

#define PART(name) int stage_run_##name(int op, const KParams &P, void *stream);
DQP_RIC_PARTS
#undef PART

static int stage_run(int op, const KParams &P, void *stream)
{
    int rc;
#define PART(name) if ((rc = stage_run_##name(op, P, stream)) != 1) return rc;
    DQP_RIC_PARTS
#undef PART
    return 1;
}

int stage_forward(const KParams &P, void *stream) { return stage_run(STAGE_FORWARD, P, stream); }
int stage_forward_stepped(const KParams &P, void *stream) { return stage_run(STAGE_STEPPED, P, stream); }
int stage_backward(const KParams &P, void *stream) { return stage_run(STAGE_BACKWARD, P, stream); }

// ---------------------------------------------------------------------------------------------
// Region of the padded copies (doubles, every array rounded up to an even length; include/dqp.h gives the formula):
//   C', dC' (T, B, nt', nt')   F', dF' (T-1, B, n', nt')   c', tau', g', dc' (T B nt')   nu', ry' (B, T n')
//   f', df' (T-1, B, n')       x0', dx0' (B, n')
// with nt' = n' + m; tau', g' = dl/dtau', nu', ry' batch-major like the caller's arrays, the rest time-major.
static long long ev(long long x) { return (x + 1) & ~1LL; }

long long pad_region_doubles(int np, int m, int T, int B)
{
    const long long ntp = np + m, b = B;
    return 2 * (ev(T * b * ntp * ntp) + ev((T - 1) * b * np * ntp) + 2 * ev(T * b * ntp) + ev(T * b * np) +
                ev((T - 1) * b * np) + ev(b * np));
}

PadRegion pad_region(double *base, int np, int m, int T, int B)
{
    const long long ntp = np + m, b = B;
    PadRegion R;
    double *o = base;
    auto take = [&](long long n) { double *at = o; o += ev(n); return at; };
    R.C = take(T * b * ntp * ntp);  R.dC = take(T * b * ntp * ntp);
    R.F = take((T - 1) * b * np * ntp);  R.dF = take((T - 1) * b * np * ntp);
    R.c = take(T * b * ntp);  R.tau = take(T * b * ntp);  R.g = take(T * b * ntp);  R.dc = take(T * b * ntp);
    R.nu = take(T * b * np);  R.ry = take(T * b * np);
    R.f = take((T - 1) * b * np);  R.df = take((T - 1) * b * np);
    R.x0 = take(b * np);  R.dx0 = take(b * np);
    return R;
}

// One array of R matrices, compact (ri x ci) <-> padded (ro x co): rows below rs and columns below cs keep their
// index, the next ro - ri rows / co - ci columns are the dummies, the rest move up by that much.  Pack writes every
// padded element (dummies: `diag` on the dummy diagonal, else 0), unpack every compact one.
struct PadJob {
    const double *src;
    double *dst;
    long long R;
    int ri, ci, ro, co, rs, cs;
    double diag;
};
constexpr int PAD_MAX_JOBS = 8;
struct PadJobs {
    PadJob j[PAD_MAX_JOBS];
};

// grid (x, jobs): blockIdx.y picks the array, a grid-stride loop over its elements; I: 32-bit indices where they fit
template <typename I, bool UNPACK>
__global__ __launch_bounds__(256) void pad_copy_kernel(PadJobs J)
{
    const PadJob &a = J.j[blockIdx.y];
    const I ri = a.ri, ci = a.ci, ro = a.ro, co = a.co, rs = a.rs, cs = a.cs;
    const I dr = ro - ri, dcol = co - ci;
    const I per = UNPACK ? ri * ci : ro * co;
    const I total = (I)a.R * per;
    for (I e = (I)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (I)gridDim.x * blockDim.x) {
        const I mat = e / per, k = e - mat * per;
        if constexpr (UNPACK) {
            const I i = k / ci, j = k - i * ci;
            const I ip = i < rs ? i : i + dr, jp = j < cs ? j : j + dcol;
            a.dst[e] = a.src[(mat * ro + ip) * co + jp];
        } else {
            const I ip = k / co, jp = k - ip * co;
            const bool rd = ip >= rs && ip < rs + dr, cd = jp >= cs && jp < cs + dcol;
            double v;
            if (rd || cd) {
                v = (rd && ip == jp) ? a.diag : 0.0;
            } else {
                const I i = ip < rs ? ip : ip - dr, j = jp < cs ? jp : jp - dcol;
                v = a.src[(mat * ri + i) * ci + j];
            }
            a.dst[e] = v;
        }
    }
}

static int pad_run(PadJobs &J, int nj, bool unpack, void *stream)
{
    if (nj == 0) return DQP_OK;
    long long mx = 0;
    bool small = true;
    for (int k = 0; k < nj; ++k) {
        const PadJob &a = J.j[k];
        const long long tot = a.R * (long long)(unpack ? a.ri * a.ci : a.ro * a.co);
        mx = tot > mx ? tot : mx;
        if (a.R * (long long)(a.ro * a.co) + 256LL * 8192 >= 0xffffffffLL) small = false;    // padded index + stride
    }
    const long long want = (mx + 255) / 256;
    const dim3 grid((unsigned)(want < 8192 ? (want > 0 ? want : 1) : 8192), (unsigned)nj);
    hipStream_t s = (hipStream_t)stream;
    if (small) {
        if (unpack) DQP_LAUNCH((pad_copy_kernel<unsigned, true>), grid, dim3(256), 0, s, J);
        else DQP_LAUNCH((pad_copy_kernel<unsigned, false>), grid, dim3(256), 0, s, J);
    } else {
        if (unpack) DQP_LAUNCH((pad_copy_kernel<unsigned long long, true>), grid, dim3(256), 0, s, J);
        else DQP_LAUNCH((pad_copy_kernel<unsigned long long, false>), grid, dim3(256), 0, s, J);
    }
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}

// the arrays of the MPC problem and what they pad to (vectors are 1 x len matrices)
static void add_job(PadJobs &J, int &nj, const double *src, double *dst, long long R, int ri, int ci, int ro, int co,
                    int rs, int cs, double diag)
{
    if (!src || !dst || R <= 0) return;
    J.j[nj++] = PadJob{src, dst, R, ri, ci, ro, co, rs, cs, diag};
}

int pad_pack(int n, int np, int m, int T, int B, const PadRegion &R, const double *C, const double *c, const double *F,
             const double *f, const double *x0, const double *tau, const double *nu, const double *g, const double *ry,
             void *stream)
{
    const int nt = n + m, ntp = np + m;
    const long long TB = (long long)T * B, T1B = (long long)(T - 1) * B;
    PadJobs J;
    int nj = 0;
    add_job(J, nj, C, R.C, TB, nt, nt, ntp, ntp, n, n, 1.0);       // identity cost on the dummy states
    add_job(J, nj, F, R.F, T1B, n, nt, np, ntp, n, n, 0.0);
    add_job(J, nj, c, R.c, TB, 1, nt, 1, ntp, 1, n, 0.0);
    add_job(J, nj, f, R.f, T1B, 1, n, 1, np, 1, n, 0.0);
    add_job(J, nj, x0, R.x0, B, 1, n, 1, np, 1, n, 0.0);
    if (nj + (tau != nullptr) + (nu != nullptr) + (g != nullptr) + (ry != nullptr) > PAD_MAX_JOBS) {
        const int rc = pad_run(J, nj, false, stream);
        if (rc != DQP_OK) return rc;
        nj = 0;
    }
    add_job(J, nj, tau, R.tau, TB, 1, nt, 1, ntp, 1, n, 0.0);      // (B, T, nt): one knot per row
    add_job(J, nj, g, R.g, TB, 1, nt, 1, ntp, 1, n, 0.0);
    add_job(J, nj, nu, R.nu, TB, 1, n, 1, np, 1, n, 0.0);          // (B, T n): one knot's states per row
    add_job(J, nj, ry, R.ry, TB, 1, n, 1, np, 1, n, 0.0);
    return pad_run(J, nj, false, stream);
}

int pad_unpack(int n, int np, int m, int T, int B, const PadRegion &R, double *tau, double *nu, double *dC, double *dc,
               double *dF, double *df, double *dx0, void *stream)
{
    const int nt = n + m, ntp = np + m;
    const long long TB = (long long)T * B, T1B = (long long)(T - 1) * B;
    PadJobs J;
    int nj = 0;
    add_job(J, nj, R.tau, tau, TB, 1, nt, 1, ntp, 1, n, 0.0);
    add_job(J, nj, R.nu, nu, TB, 1, n, 1, np, 1, n, 0.0);
    add_job(J, nj, R.dC, dC, TB, nt, nt, ntp, ntp, n, n, 0.0);
    add_job(J, nj, R.dc, dc, TB, 1, nt, 1, ntp, 1, n, 0.0);
    add_job(J, nj, R.dF, dF, T1B, n, nt, np, ntp, n, n, 0.0);
    add_job(J, nj, R.df, df, T1B, 1, n, 1, np, 1, n, 0.0);
    add_job(J, nj, R.dx0, dx0, B, 1, n, 1, np, 1, n, 0.0);
    return pad_run(J, nj, true, stream);
}

}  // namespace dqp
