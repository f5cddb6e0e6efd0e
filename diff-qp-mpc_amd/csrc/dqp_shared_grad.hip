// dqp_shared_grad.hip -- gradients of parameters that are SHARED by the batch (dqp_dims stride 0), written as one
// tensor summed over the batch instead of per sample (dqp_qp_backward_shared, include/dqp.h).
//
// Every matrix gradient of the dense QP is a rank-2 outer product of vectors the backward kernels produce
// (qp.py:158-181):
//     dQ_b = 1/2 (dx_b z_b^T + z_b dx_b^T)    dG_b = dlam_b z_b^T + lam_b dx_b^T    dA_b = dnu_b z_b^T + nu_b dx_b^T
// so the sum over the batch is a GEMM with the batch as the contraction axis and a small output:
//     sum_b dG_b = DLAM^T Z + LAM^T DX     with DLAM, LAM (B, nineq) and Z, DX (B, nz)
// and the shared vector gradients (dp = dx, dh = -dlam, db = -dnu) are column sums of the same vectors, i.e. the
// same product with a row of ones on the left.
//
// Three stages on the caller's stream, no atomics, no host synchronisation:
//   1. vector pass: the backward kernel of whichever family serves the size (dqp_qp_backward, unchanged), with NULL
//      matrix outputs for the shared matrices and dp / dh / db routed to `reduce_ws` where the caller does not want
//      them per sample.  z, lam and nu are the caller's forward outputs: the per-sample kernels multiply by exactly
//      those (the 1e-8 clamps of qp.py:149 enter only d = lam / slack), in both backward modes.
//   2. shared_grad_gemm_kernel: split-K.  Grid (output tiles, ceil(B / KC)); one wavefront owns one 16 x 16 output
//      tile of one gradient and accumulates KC consecutive samples on the fp64 matrix cores
//      (v_mfma_f64_16x16x4_f64: A[i][k] = X[b0 + k][i0 + i], B[k][j] = Y[b0 + k][j0 + j], so a lane group reads 16
//      contiguous doubles of one sample row).  Both products of a rank-2 gradient go into the same accumulator:
//      sample by sample (one k-group live per instruction) from a zero accumulator, so that each sample's tile carries
//      exactly the rounding of the per-sample kernels, then added in ascending sample order.  The vector sums use
//      all four k-groups per instruction (their products with 1 are exact).
//      Edge tiles and the ragged last chunk are zero-filled operands (clamped address + select), not branches.
//      The partial tile goes to reduce_ws[chunk][tile][16][16].
//   3. shared_grad_finish_kernel: one thread per output element adds its partials in ascending chunk order,
//      applies the 1/2 of dQ and stores.
// The result depends only on the inputs and B: bit-identical from run to run and on any number of CUs.
//
// Order inside a sample: the product the per-sample kernels round on its own (lam dx^T, z dx^T) comes first, the one
// they fuse (dlam z^T, dx z^T) second, so that every term of the sum is the per-sample gradient itself.
#include <hip/hip_runtime.h>

#include "dqp_common.h"

namespace dqp {
namespace shared {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int KC = 64;        // samples per split-K chunk (16 MFMA steps of 4)
constexpr int TILE = 16;
constexpr int MAXJOB = 6;     // dQ dp dG dh dA db

// one reduced gradient: out (rows, cols) = scale * sum_b (x1_b y1_b^T + sx2 * x2_b y2_b^T); x1 == NULL: the column
// sums of y1 (rows == 1, a one in row 0 on the left)
struct Job {
    const double *x1, *y1, *x2, *y2;
    double *out;
    double sx2, scale;
    int rows, cols;
    int tileBase, tilesC;     // first tile of this job in the grid, tiles per output row of tiles
};

struct Params {
    Job job[MAXJOB];
    double *part;             // [chunk][tile][16][16]
    int njob, tiles, B, nchunks;
};

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

template <bool ONES>
__device__ __forceinline__ double4_t accumulate(const Job &J, int B, long long b0, int l15, int kq, int ri, int cj)
{
    const bool rin = ri < J.rows, cin = cj < J.cols;
    const int ric = rin ? ri : J.rows - 1, cjc = cin ? cj : J.cols - 1;      // clamped: every load is in bounds
    double4_t acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
        long long b = b0 + 4 * ks + kq;
        const bool bin = b < B;
        b = bin ? b : (long long)B - 1;
        if (ONES) {
            const double a = (bin && ri == 0) ? 1.0 : 0.0;
            const double y = J.y1[b * J.cols + cjc];
            acc[ks & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (bin && cin) ? y : 0.0, acc[ks & 1], 0, 0, 0);
        } else {
            const double a1 = J.x1[b * J.rows + ric], y1 = J.y1[b * J.cols + cjc];
            const double a2 = J.x2[b * J.rows + ric], y2 = J.y2[b * J.cols + cjc];
            const bool am = bin && rin, ym = bin && cin;
            // One sample per instruction (k-group q supplies its sample, the other three supply zeros): the tile of
            // sample b is formed from a zero accumulator exactly as the per-sample kernels form it,
            // fma(x2, y2, fl(x1 y1)), and then added.  The reduction is then a sum of the SAME B terms as
            // per-sample gradients + sum(0), in ascending sample order -- it differs from that path only by the order
            // of the additions, never by the rounding of a product against a running sum.
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool aq = am && kq == q, yq = ym && kq == q;
                double4_t t = {0.0, 0.0, 0.0, 0.0};
                t = __builtin_amdgcn_mfma_f64_16x16x4f64(aq ? a1 : 0.0, yq ? y1 : 0.0, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f64_16x16x4f64(aq ? J.sx2 * a2 : 0.0, yq ? y2 : 0.0, t, 0, 0, 0);
                acc[0] += t;
            }
        }
    }
    return acc[0] + acc[1];
}

__global__ __launch_bounds__(WAVE) void shared_grad_gemm_kernel(Params G)
{
    const int lane = threadIdx.x, l15 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x;
    int j = 0;
    while (j + 1 < G.njob && t >= G.job[j + 1].tileBase) ++j;       // wavefront-uniform
    const Job &J = G.job[j];
    const int lt = t - J.tileBase, ti = lt / J.tilesC, tj = lt - ti * J.tilesC;
    const long long b0 = (long long)blockIdx.y * KC;
    const int ri = TILE * ti + l15, cj = TILE * tj + l15;
    const double4_t acc = J.x1 ? accumulate<false>(J, G.B, b0, l15, kq, ri, cj)
                               : accumulate<true>(J, G.B, b0, l15, kq, ri, cj);
    // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 * register
    double *o = G.part + ((long long)blockIdx.y * G.tiles + t) * (TILE * TILE);
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) o[(kq + 4 * rg) * TILE + l15] = acc[rg];
}

__global__ __launch_bounds__(256) void shared_grad_finish_kernel(Params G)
{
    const Job &J = G.job[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= J.rows * J.cols) return;
    const int r = idx / J.cols, c = idx - r * J.cols;
    const long long tile = J.tileBase + (r >> 4) * J.tilesC + (c >> 4);
    const long long step = (long long)G.tiles * (TILE * TILE);
    const double *p = G.part + tile * (TILE * TILE) + (r & 15) * TILE + (c & 15);
    double s = p[0];
    for (int ch = 1; ch < G.nchunks; ++ch) s += p[ch * step];        // ascending chunk order
    J.out[idx] = s * J.scale;
}

struct Shared {
    bool Q, p, G, h, A, b;
    bool any() const { return Q || p || G || h || A || b; }
};

static Shared shared_of(const dqp_dims *d)
{
    Shared s;
    s.Q = d->stride_Q == 0; s.p = d->stride_p == 0; s.G = d->stride_G == 0; s.h = d->stride_h == 0;
    s.A = d->neq > 0 && d->stride_A == 0; s.b = d->neq > 0 && d->stride_b == 0;
    return s;
}

static bool dims_ok(const dqp_dims *d) { return d->nbatch >= 0 && d->nz > 0 && d->nineq > 0 && d->neq >= 0; }

// tiles of all shared outputs
static long long tiles_of(const dqp_dims *d, const Shared &s)
{
    const long long tn = cdiv(d->nz, TILE), tm = cdiv(d->nineq, TILE), te = cdiv(d->neq, TILE);
    return (s.Q ? tn * tn : 0) + (s.p ? tn : 0) + (s.G ? tm * tn : 0) + (s.h ? tm : 0) + (s.A ? te * tn : 0) +
           (s.b ? te : 0);
}

// reduce_ws: DX (B, nz) | DH (B, nineq) | DB (B, neq) | partial tiles [chunk][tile][256]
static long long vec_doubles(const dqp_dims *d) { return (long long)d->nbatch * ((long long)d->nz + d->nineq + d->neq); }

}  // namespace shared
}  // namespace dqp

extern "C" {

__attribute__((visibility("default"))) size_t dqp_qp_backward_shared_bytes(const dqp_dims *d)
{
    using namespace dqp::shared;
    if (!d || !dims_ok(d) || d->nbatch == 0) return 0;
    const Shared s = shared_of(d);
    if (!s.any()) return 0;
    const long long n = vec_doubles(d) + (long long)cdiv(d->nbatch, KC) * tiles_of(d, s) * (TILE * TILE);
    return (size_t)n * sizeof(double);
}

__attribute__((visibility("default"))) int
dqp_qp_backward_shared(const dqp_dims *dims, const dqp_opts *opts, const double *Q, const double *G,
                       const double *A, const double *zhat, const double *lam, const double *nu,
                       const double *slack, const double *dl_dzhat, double *dQ, double *dp, double *dG,
                       double *dh, double *dA, double *db, int32_t *info, void *workspace, void *reduce_ws,
                       void *stream)
{
    using namespace dqp::shared;
    if (!dims) return DQP_ERR_BAD_ARG;
    const Shared s = shared_of(dims);
    if (!s.any())
        return dqp_qp_backward(dims, opts, Q, G, A, zhat, lam, nu, slack, dl_dzhat, dQ, dp, dG, dh, dA, db, info,
                               workspace, stream);
    if (!dims_ok(dims)) return DQP_ERR_BAD_ARG;
    if (dims->nbatch == 0) return DQP_OK;
    if (!reduce_ws) return DQP_ERR_BAD_ARG;
    const int B = dims->nbatch, N = dims->nz, M = dims->nineq, E = dims->neq;
    const int nchunks = cdiv(B, KC);
    if (nchunks > 65535) return DQP_ERR_TOO_LARGE;

    double *ws = (double *)reduce_ws;
    double *wsDX = ws, *wsDH = wsDX + (long long)B * N, *wsDB = wsDH + (long long)B * M;
    const bool wQ = s.Q && dQ, wp = s.p && dp, wG = s.G && dG, wh = s.h && dh, wA = s.A && dA, wb = s.b && db;
    const bool needDX = wQ || wG || wA || wp, needDH = wG || wh, needDB = wA || wb;
    // per-sample vectors: the caller's buffer where it is a per-sample output, else the scratch (if anything reads it)
    double *vDX = (!s.p && dp) ? dp : (needDX ? wsDX : nullptr);
    double *vDH = (!s.h && dh) ? dh : (needDH ? wsDH : nullptr);
    double *vDB = (E > 0 && !s.b && db) ? db : (needDB ? wsDB : nullptr);
    int rc = dqp_qp_backward(dims, opts, Q, G, A, zhat, lam, nu, slack, dl_dzhat, s.Q ? nullptr : dQ, vDX,
                             s.G ? nullptr : dG, vDH, s.A ? nullptr : dA, vDB, info, workspace, stream);
    if (rc != DQP_OK) return rc;

    Params P = {};
    P.part = ws + vec_doubles(dims);
    P.B = B; P.nchunks = nchunks;
    int maxElems = 0;
    auto add = [&](const double *x1, const double *y1, const double *x2, const double *y2, double sx2, double scale,
                   double *out, int rows, int cols) {
        Job &J = P.job[P.njob++];
        J.x1 = x1; J.y1 = y1; J.x2 = x2; J.y2 = y2; J.sx2 = sx2; J.scale = scale; J.out = out;
        J.rows = rows; J.cols = cols; J.tileBase = P.tiles; J.tilesC = cdiv(cols, TILE);
        P.tiles += cdiv(rows, TILE) * J.tilesC;
        if (rows * cols > maxElems) maxElems = rows * cols;
    };
    // vDH = -dlam and vDB = -dnu: the sign goes onto the operand (exact)
    if (wQ) add(zhat, vDX, vDX, zhat, 1.0, 0.5, dQ, N, N);
    if (wp) add(nullptr, vDX, nullptr, nullptr, 0.0, 1.0, dp, 1, N);
    if (wG) add(lam, vDX, vDH, zhat, -1.0, 1.0, dG, M, N);
    if (wh) add(nullptr, vDH, nullptr, nullptr, 0.0, 1.0, dh, 1, M);
    if (wA) add(nu, vDX, vDB, zhat, -1.0, 1.0, dA, E, N);
    if (wb) add(nullptr, vDB, nullptr, nullptr, 0.0, 1.0, db, 1, E);
    if (P.njob == 0) return DQP_OK;
    DQP_LAUNCH(dqp::shared::shared_grad_gemm_kernel, dim3(P.tiles, nchunks), dim3(dqp::WAVE), 0, (hipStream_t)stream, P);
    if (hipGetLastError() != hipSuccess) return DQP_ERR_LAUNCH;
    DQP_LAUNCH(dqp::shared::shared_grad_finish_kernel, dim3(cdiv(maxElems, 256), P.njob), dim3(256), 0,
               (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? DQP_OK : DQP_ERR_LAUNCH;
}

}  // extern "C"
