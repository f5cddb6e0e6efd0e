// dqp_common.h -- kernel parameter block shared by the HIP translation units of libdqp_hip.so
#ifndef DQP_COMMON_H_
#define DQP_COMMON_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dqp.h"
#include "dqp_trace.h"

namespace dqp {

constexpr int WAVE = 64;

struct KParams {
    const double *Q, *p, *G, *h, *A, *b;
    long long sQ, sp, sG, sh, sA, sb;
    // forward outputs
    double *zhat, *lam, *nu, *slack, *best_resid;
    // backward inputs / outputs
    const double *zin, *lamin, *nuin, *slackin, *gin;
    double *dQ, *dp, *dG, *dh, *dA, *db;
    int32_t *info;
    double *workspace;            // caller-provided scratch (dqp_workspace_bytes), may be NULL
    unsigned long long *stamps;   // diagnostic: s_memtime at phase boundaries (16 per workgroup) or NULL
    int B, N, M, E;
    int ldz, ldm, lde, ldt;
    double eps, stallTol;
    int maxIter, notImprovedLim;
    unsigned flags;
    // batch-coupled termination (DQP_FLAG_BATCH_TERMINATION, dqp_term.hip)
    double *hist;          // pass 1: (B, histIters, 2) = (resid, mu) per iteration, or NULL
    const int32_t *cap;    // pass 2: cap[0] = iteration cap I*, cap[TERM_HDR + qp] = iteration of this QP's best iterate
    int histIters;
    // true-dynamics equality residual (dqp_opts.dyn_*): registered model evaluated per iteration
    int dynId, dynT, dynN, dynM;
    double dynDt;
    const double *dynX0;
    // MPC-structured I/O (dqp_mpc_qp_forward / _backward, null-space kernels only): the dense
    // (Q,p,G,h,A,b) and their gradients are never materialised in HBM.  mC != NULL selects it.
    const double *mC, *mc, *mF, *mf, *mx0, *mul, *muu;     // time-major inputs (qp_wrapper layout)
    double *mdC, *mdc, *mdF, *mdf, *mdx0;                  // backward outputs
    int mn, mm, mT;
    // batch rule, null-space kernels: improving iterates of pass 1 ([it][B][snapDim]) and the history
    // as the finish pass reads it
    double *snap;
    const double *histIn;
    // caller-driven iterations (dqp_mpc_qp_forward_stepped, stage-wise kernels): iterations itBegin .. itEnd-1 of
    // maxIter, the equality residual of iteration itBegin read from extRy (B, T n) in the closure's ordering
    const double *extRy;
    int itBegin, itEnd;
};

// Layout of the control bounds of an MPC-structured call (include/dqp.h: dqp_mpc_bounds): the pair of sample b, knot t,
// control k is at mul / muu [b stride_b + t stride_t + k].  The two strides travel in sG and sh, the dense strides that an
// MPC-structured call never reads (its G and h are built in registers), so the parameter block -- and with it the
// hidden-argument offsets of every kernel that takes one -- stays as it was.  (0, 0) is the n_ctrl-vector.
__host__ __device__ inline long long mpc_bound_stride_b(const KParams &P) { return P.sG; }
__host__ __device__ inline long long mpc_bound_stride_t(const KParams &P) { return P.sh; }
inline bool mpc_bounds_strided(const KParams &P) { return P.sG != 0 || P.sh != 0; }
inline void mpc_set_bounds(KParams &P, const dqp_al_bounds *b)
{
    P.mul = b->lower; P.muu = b->upper; P.sG = b->stride_b; P.sh = b->stride_t;
}

constexpr int TERM_HDR = 8;   // int32 header words in front of the per-problem best-iteration list

// Termination buffer (dqp_termination_bytes), see dqp_term.hip: hist [histIters][B] x (resid, mu),
// then TERM_ACC_BYTES of accumulators + header, then the redo list.
constexpr int TERM_MAXIT = 64;
constexpr int TERM_ACC_BYTES = 3 * 8 + TERM_HDR * 4;

// Record one iteration of a problem's residual history (one lane per problem calls this);
// iteration-major so that the batch reduction reads it coalesced.
__device__ __forceinline__ void hist_put(const KParams &P, long long qp, int it, double resid, double mu)
{
    double2 *h = reinterpret_cast<double2 *>(P.hist) + (long long)it * P.B + qp;
    *h = make_double2(resid, mu);
}
// The problem left the loop after `iters` iterations: the rest of its history is NaN (what the
// reference's iterate is from there on: a non-finite residual never recovers, batch.py:119-131).
__device__ __forceinline__ void hist_fill(const KParams &P, long long qp, int iters)
{
    const double nan = __builtin_nan("");
    for (int it = iters; it < P.histIters; ++it)
        reinterpret_cast<double2 *>(P.hist)[(long long)it * P.B + qp] = make_double2(nan, nan);
}
// Pass 1 clears the batch reduction's accumulators itself (the reduction runs after this kernel
// on the same stream): saves a memset launch per forward call.
__device__ __forceinline__ void term_zero_acc(const KParams &P)
{
    if (P.hist && blockIdx.x == 0) {
        unsigned *a = reinterpret_cast<unsigned *>(P.hist + (long long)P.B * P.histIters * 2);
        for (int i = threadIdx.x; i < TERM_ACC_BYTES / 4; i += blockDim.x) a[i] = 0u;
    }
}

// the reference's rule on the batch-wide masks (dqp_term.hip) -> the iteration count it stops at
__device__ __forceinline__ int rule_stop(unsigned long long ai, unsigned long long anb, unsigned long long ana, int maxIter,
                                         int notImprovedLim)
{
    int nNot = 0;
    for (int it = 0; it < maxIter; ++it) {
        if (it == 0 || ((ai >> it) & 1ull)) nNot = 0;
        else nNot += 1;
        if (nNot == notImprovedLim || !((anb >> it) & 1ull) || !((ana >> it) & 1ull)) return it + 1;
    }
    return maxIter;
}

// a wave-uniform 64-bit value as scalar registers, whichever kind of load produced it
__device__ __forceinline__ unsigned long long term_uniform(unsigned long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// pass 2: the batch's stop I*.  A positive header was written by term_decide_kernel (multi-device form: the masks of
// every shard combined).  0 -- pass 1 cleared it (term_zero_acc) and I* >= 1 -- means the scan left only the masks, which
// sit in front of the header: the rule is replayed here, by every wavefront that needs I* (wave-uniform address and
// result, the mask loads travel with the header's: the kernel boundary in front of pass 2 gives the visibility the
// scan kernel used to buy with two device-wide fences).  The first lane of the grid leaves I* in the header for the caller.
// Read it once per kernel: term_flagged and the iteration clamp take the value.
// SCALAR (the null-space kernels, whose finish pass is on the path of every call): masks and rule in scalar registers.
// Otherwise (the kernels that solve again in pass 2) the rule runs on vector registers: those kernels sit at the
// register limit and pay for scalar pressure at their head with scratch (r16::forward_kernel at (30,30,15): 116 B in
// front of this change, 176 B with the scalar form, 120 B with this one).
template <bool SCALAR = false> __device__ __forceinline__ int term_cap(const KParams &P)
{
    const unsigned long long *m =
        reinterpret_cast<const unsigned long long *>(reinterpret_cast<const char *>(P.cap) - (TERM_ACC_BYTES - TERM_HDR * 4));
    const int c = P.cap[0];
    // one memory round trip: left alone, the mask loads sink into the branch below and leave only after c has arrived
    unsigned long long ai = m[0], anb = m[1], ana = m[2];
    if (SCALAR) {
        ai = term_uniform(ai); anb = term_uniform(anb); ana = term_uniform(ana);
        asm volatile("" : "+s"(ai), "+s"(anb), "+s"(ana));
    } else {
        asm volatile("" : "+v"(ai), "+v"(anb), "+v"(ana));
    }
    if (c > 0) return c;
    const int istar = rule_stop(ai, anb, ana, P.maxIter, P.notImprovedLim);
    if (blockIdx.x == 0 && threadIdx.x == 0) const_cast<int32_t *>(P.cap)[0] = istar;
    return istar;
}

// pass 2: a problem is taken back iff its best iterate of pass 1 came at an iteration the reference never ran
__device__ __forceinline__ int term_best(const KParams &P, long long qp) { return P.cap[TERM_HDR + qp]; }
__device__ __forceinline__ bool term_flagged(const KParams &P, long long qp, int cap) { return term_best(P, qp) >= cap; }

// batch rule replay (dqp_term.hip); 0 on success
size_t term_bytes(int B, int maxIter, int snapDim);
int term_decide(const KParams &P, void *term, void *stream);
int term_local_masks(const KParams &P, void *term, unsigned long long *masks, void *stream);
int term_decide_global(const KParams &P, void *term, const unsigned long long *masks, void *stream);
void term_bind_pass1(KParams &P, void *term, int snapDim);
void term_bind_pass2(KParams &P, void *term);


// DPP-row kernels (dqp_r16.hip): 4 QPs per wavefront for compile-time sizes <= 32.
// Return DQP_OK / error, or 1 when no instantiation matches (caller falls back to the
// generic kernels of dqp_pdipm.hip).
#ifdef DQP_STAMPS
extern unsigned long long *g_debug_stamps;
#endif
int r16_forward(const KParams &P, void *stream);
int r16_backward(const KParams &P, void *stream);
// null-space form of the forward kernel (dqp_r16n.hip); same return convention.  It parks
// r16n_workspace_doubles(N, M, E) doubles per QP in P.workspace (0: no instantiation).
int r16n_forward(const KParams &P, void *stream);
long long r16n_workspace_doubles(int N, int M, int E);
int r16n_snapshot_doubles(int N, int M, int E);
// stage-wise (Riccati) PDIPM for MPC-structured QPs of any horizon (kernels: dqp_ric_kernels.h), one interface for every
// compiled (n_state, n_ctrl) pair (dqp_ric_pad.hip).  The pairs are _build.py's: native (a problem of that size runs on
// them as it is) or host-only (they only run padded problems, dqp_mpc_dims.n_state_host); the per-QP workspace layout and
// the snapshot of the batch rule's finish pass are the same in all of them.
bool stage_supported(int n_state, int n_ctrl);
bool stage_native(int n_state, int n_ctrl);
int stage_q(int n_state, int n_ctrl);                           // problems per wavefront: 4 (n + m <= 16) or 2
long long stage_layout_doubles(int n_state, int n_ctrl, int T); // per QP; 0: no kernel for (n, m)
int stage_snapshot_doubles(int n_state, int n_ctrl, int T);
// B rounded up to whole wavefronts (padding rows own a slot too) times the layout; stepped: plus the loop state per slot
long long stage_workspace_doubles(int n_state, int n_ctrl, int T, int B, bool stepped);
// 1: no kernel for this (n, m), or for P.dynId on it (only native 16-lane pairs have registered models)
int stage_forward(const KParams &P, void *stream);
int stage_forward_stepped(const KParams &P, void *stream);      // iterations [P.itBegin, P.itEnd), residual from P.extRy
int stage_backward(const KParams &P, void *stream);
int stage_finish(const KParams &P, void *stream);               // dqp_ric.hip, the native part
enum { STAGE_FORWARD = 0, STAGE_STEPPED = 1, STAGE_BACKWARD = 2 };   // op of a part's stage_run_<part>(op, P, stream)
// Padded problems: a problem (n, m) on the kernels of (n', m), n' >= n, with n' - n dummy states after the real ones
// (identity cost, zero dynamics rows, zero start).  Region of the caller's workspace behind the kernels' part
// (stage_workspace_doubles of the host pair):
struct PadRegion {
    double *C, *F, *c, *tau, *g, *dc, *f, *df, *nu, *ry, *x0, *dx0, *dC, *dF;
};
long long pad_region_doubles(int n_host, int n_ctrl, int T, int B);
PadRegion pad_region(double *base, int n_host, int n_ctrl, int T, int B);
// the copies (element-wise, coalesced, no host synchronisation); NULL arrays are skipped
int pad_pack(int n, int n_host, int m, int T, int B, const PadRegion &R, const double *C, const double *c, const double *F,
             const double *f, const double *x0, const double *tau, const double *nu, const double *g, const double *ry,
             void *stream);
int pad_unpack(int n, int n_host, int m, int T, int B, const PadRegion &R, double *tau, double *nu, double *dC, double *dc,
               double *dF, double *df, double *dx0, void *stream);
// dense QPs above DQP_MAX_DIM (dqp_big.hip): one QP per workgroup, matrices in the workspace, MFMA tiles
long long big_workspace_doubles(int N, int M, int E);
bool big_fits(int N, int M, int E);         // the solver's vectors fit the LDS of a CU
int big_forward(const KParams &P, void *stream);
int big_backward(const KParams &P, void *stream);

// backward restarted from the context r16n_forward left in P.workspace (DQP_FLAG_BACKWARD_CTX)
int r16n_backward(const KParams &P, void *stream);

// dqp_pdipm.hip: the parameter block of a dense QP call (sizes, strides, options; lds_bytes: what the generic kernels need)
void fill_opts(const dqp_opts *o, KParams &P);
int fill_params(const dqp_dims *d, const dqp_opts *o, KParams &P, size_t &lds_bytes);

}  // namespace dqp
#endif
