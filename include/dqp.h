/*
 * dqp.h -- C ABI of the MI355X-native differentiable batched QP solver (libdqp_hip.so).
 *
 * This is the drop-in boundary for the hot path of swami1995/diff-qp-mpc.  The reference
 * has no C/FFI layer on this path (its boundary is a Python torch.autograd.Function built by
 * a factory closure); each entry point below names the reference interface it replaces, and
 * INTEGRATION.md shows the ~100-line Python binding a maintainer of the reference would add.
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HIP), fp64, row-major, contiguous inside one batch
 *     element.  The caller owns every buffer; the library allocates nothing and keeps no state.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue
 *     work; they never synchronise, allocate or copy, so they are hipGraph-capturable.
 *   - A batch stride of 0 means "this parameter is shared by all batch elements" (the
 *     reference's expandParam rule, qpth/util.py:36-43).
 *   - Return value: DQP_OK or a negative DQP_ERR_* for argument errors detected on the host.
 *     Per-problem numerical status is written to `info` on the device (see below).
 *   - Sizes: this build solves QPs with nz, nineq, neq <= DQP_MAX_DIM on the fused
 *     one-wavefront-per-QP kernels; larger problems return DQP_ERR_TOO_LARGE.
 */
#ifndef DQP_H_
#define DQP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQP_VERSION 303 /* (additive at 303, no bump: dqp_qp_backward_shared_bytes / dqp_qp_backward_shared -- gradients of
                           shared parameters summed over the batch on the device; dqp_al_mpc_solve_fused_supported /
                           dqp_al_mpc_solve_fused_bytes / dqp_al_mpc_solve_fused -- dqp_al_mpc_solve as one launch;
                           dqp_mpc_linearize, dqp_mpc_sqp_supported / _workspace_bytes / _rounds -- the SQP rounds of
                           qp_wrapper.MPC for a registered model, enqueued by one call;
                           dqp_deq_supported / _partial_bytes / _ln_forward / _ln_backward / _res_forward / _res_backward --
                           the LayerNorm stages of the DEQ-MPC network as fused fp32 kernels;
                           dqp_al_ncon_xbounds, dqp_al_banded_newton_step_xbounds, dqp_al_newton_solve_xbounds (+ _bytes),
                           dqp_al_outer_update_xbounds, dqp_al_mpc_solve_xbounds (+ _bytes) -- state bounds on the
                           block-tridiagonal AL paths;
                           dqp_al_banded_newton_step_jac_xbounds, dqp_al_merit_xbounds -- state bounds on the
                           caller-linearised block-tridiagonal step and in the merit kernel;
                           dqp_al_mpc_solve_fused_supported_xbounds / _bytes_xbounds / _lds_bytes_xbounds,
                           dqp_al_mpc_solve_fused_xbounds -- state bounds on the single-launch solve;)
                           0.3.3: dqp_al_banded_newton_step_jac / dqp_al_banded_solve(dims, 0, ...) at 16 < n_state + n_ctrl <= 32
                           (compiled pairs), dqp_al_banded_jac_factor_bytes;
                           0.3.2: dqp_mpc_dims.n_state_host (padded stage-wise problems), dqp_mpc_qp_host_n_state;
                           0.3.1: stage-wise MPC kernels for 16 < n_state + n_ctrl <= 32 (compiled pairs), same entry points;
                           0.3.0: DQP_FLAG_STRICT_GET_STEP, dqp_mpc_qp_forward_stepped (caller-supplied equality
                           residual, one PDIPM iteration range per call), dqp_trace_begin / dqp_trace_end, DQP_MAX_DIM_LARGE
                           (blocked dense kernels above DQP_MAX_DIM);
                           0.2.1x: dqp_mpc_qp_backward takes C and F, dqp_mpc_dims.dyn_id, dqp_mpc_qp_termination_bytes,
                           dqp_term_local_masks + dqp_qp_forward_finish,
                           dqp_al_newton_solve_bytes(dims, banded); 212: DQP_FLAG_RIC_GLOBAL_WS, smaller
                           dqp_mpc_qp_workspace_bytes of the stage-wise kernels */
#define DQP_MAX_DIM 64
#define DQP_MAX_DIM_LARGE 512 /* dqp_qp_forward / dqp_qp_backward above DQP_MAX_DIM: one QP per workgroup, matrices
                                 blocked through LDS (csrc/dqp_big.hip); the reference's prof-linear.py sizes
                                 (nz = nineq up to 500, prof-linear.py:38-46) */

enum {
    DQP_OK = 0,
    DQP_ERR_BAD_ARG = -1,    /* null pointer, negative size, nineq == 0 ...              */
    DQP_ERR_TOO_LARGE = -2,  /* a dimension exceeds DQP_MAX_DIM or LDS capacity           */
    DQP_ERR_LAUNCH = -3,     /* hipLaunchKernel / hipFuncSetAttribute reported an error   */
    DQP_ERR_NO_DEVICE = -4
};

/* per-problem status written to info[2*i + 0] */
enum {
    DQP_STATUS_OK = 0,
    DQP_STATUS_Q_NOT_PD = 1,    /* reference: RuntimeError('Q is not SPD.') qp.py:86 /
                                   LU(Q) failure batch.py:381-388                          */
    DQP_STATUS_A_RANK_DEF = 2   /* A Q^-1 A^T not positive definite (A rank deficient)    */
};

/* flags */
#define DQP_FLAG_DENSE_BACKWARD 1u /* backward of DenseQPFunction (qp.py:239-270): d = lam/slack
                                      without the 1e-8 clamps of QPFunction (qp.py:149)   */

#define DQP_FLAG_GENERIC_ONLY 2u   /* testing: skip the size-specialised DPP-row kernels     */
#define DQP_FLAG_BACKWARD_CTX 8u   /* dqp_qp_backward: `workspace` is the buffer dqp_qp_forward filled
                                      for the SAME Q, G, A (it holds the factorisations, like the
                                      reference's ctx.Q_LU / S_LU / R, qp.py:93-95): skip the
                                      refactorisation.  Ignored where no such kernel exists.   */
#define DQP_FLAG_BATCH_TERMINATION 16u /* forward: the reference's batch-coupled stopping rule
                                      (batch.py:119-144), exactly: every problem is iterated to
                                      max_iter while its (resid, mu) history is recorded in
                                      `termination`, a reduction over the batch replays the
                                      reference's rule (no sample improved for not_improved_lim
                                      iterations | best_resids.max() < eps | mu.min() > 1e32) to
                                      find the iteration the reference stops at, and the problems
                                      whose best iterate came later are taken back to there: the
                                      null-space kernels keep every improving iterate of pass 1 in
                                      `termination` and finish from the right one (an epilogue, no
                                      second solve); the other kernels re-solve up to there.  Needs
                                      the `termination` buffer (dqp_termination_bytes).  Without the
                                      flag a problem stops on its own (see dqp_qp_forward).        */
#define DQP_FLAG_HISTORY_ONLY 32u   /* with DQP_FLAG_BATCH_TERMINATION: stop after pass 1 (every problem
                                      iterated to max_iter, (resid, mu) history recorded in
                                      `termination` as (max_iter, nbatch, 2) doubles, best iterate over
                                      all max_iter iterations returned): diagnostics and profiling of
                                      the dominant launch on its own                                */
#define DQP_FLAG_NO_NULLSPACE 4u   /* forward: keep the equality rows in the iteration even when a
                                      workspace is given (the kernel used without one)       */
#define DQP_FLAG_RIC_GLOBAL_WS 64u  /* testing: dqp_mpc_qp_forward's stage-wise kernels keep their iterates
                                      and factors in the caller's workspace even where they would
                                      fit in LDS (the path long horizons take)                  */

#define DQP_FLAG_STRICT_GET_STEP 128u /* forward: batch.py:211-214 literally.  The reference's QPFunction solver computes the
                                      step ratios as -v/dv with no guard: a step component that is exactly 0.0 gives
                                      -inf, alpha = -inf, the iterate turns NaN and the problem keeps the best iterate
                                      it had (its history is NaN from there on).  Its DenseQPFunction solver guards
                                      the division (batch_LU.py:203-214), and so do these kernels by default.  With
                                      this flag a problem whose affine or combined step has an exactly-zero slack or
                                      multiplier component is frozen the way the reference's NaN freezes it.  Which
                                      problems meet an exact zero depends on the arithmetic order, so this reproduces
                                      the reference's behaviour class, not its bit pattern.       */

#define DQP_FLAG_STAGEWISE 256u /* dqp_mpc_qp_forward / _backward: take the stage-wise (Riccati) kernels even where a
                                      null-space instantiation exists for the shape (testing; and the backward of a
                                      dqp_mpc_qp_forward_stepped solve, whose workspace is the stage-wise one)        */

typedef struct dqp_dims {
    int32_t nbatch;
    int32_t nz;
    int32_t nineq;
    int32_t neq;       /* 0 = no equality constraints (A, b may be NULL)                   */
    /* batch strides in ELEMENTS (doubles); 0 = shared across the batch                    */
    int64_t stride_Q, stride_p, stride_G, stride_h, stride_A, stride_b;
} dqp_dims;

typedef struct dqp_opts {
    double eps;               /* qp.py:19  eps=1e-12                                       */
    double stall_tol;         /* per-problem early exit needs best_resid < stall_tol (1e-10) */
    int32_t max_iter;         /* qp.py:20  maxIter=20                                      */
    int32_t not_improved_lim; /* qp.py:19  notImprovedLim=3                                */
    uint32_t flags;
    int32_t reserved;
    /* True-dynamics equality residual (qp_wrapper.py:309,316,326-345 -> batch_LU.py:97 / batch.py:102):
     * with dyn_id != 0 the PDIPM evaluates ry = dyn_res(z) = [f(x_t,u_t) - x_{t+1}]_{t<T-1}, x_0 - x0
     * with f the registered device model (DQP_DYN_*, below) instead of A z - b, every iteration, as
     * the reference does with its Python closure; z is per knot [x_t (n_state), u_t (n_ctrl)], so
     * nz = dyn_T (n_state + n_ctrl) and neq = dyn_T n_state (+ n_state rows x_{T-1} = 0 of
     * add_goal_constraint, qp_wrapper.py:339-341).  A and b (the linearisation) still
     * define the Newton systems and the starting point.  dyn_x0: device pointer (nbatch, n_state).
     * Runs on the generic one-QP-per-wavefront kernels.  dyn_id == 0: ry = A z - b.                 */
    int32_t dyn_id;
    int32_t dyn_T;
    double dyn_dt;
    const double *dyn_x0;
} dqp_opts;

int dqp_version(void);
const char *dqp_error_string(int code);

/*
 * Extents.  What holds for every entry point of this header that takes device pointers:
 *   - an array argument is read and written only inside the extent its documented shape declares, from its first
 *     byte to its last, and a workspace / termination / factor / scratch buffer only inside the bytes its size function
 *     (the `*_bytes` functions: dqp_workspace_bytes, dqp_termination_bytes, dqp_qp_backward_shared_bytes,
 *     dqp_mpc_qp_workspace_bytes, dqp_mpc_qp_termination_bytes, dqp_mpc_qp_stepped_workspace_bytes,
 *     dqp_mpc_qp_stepped_termination_bytes, dqp_mpc_sqp_workspace_bytes, dqp_al_newton_solve_bytes,
 *     dqp_al_mpc_solve_bytes, dqp_al_mpc_solve_fused_bytes[_bounds], dqp_al_banded_factor_bytes,
 *     dqp_al_banded_jac_factor_bytes, dqp_deq_partial_bytes, and their `_xbounds` twins) returns for the same `dims`
 *     and `opts`: exactly that many bytes suffice, no slack has to be added, and 8-byte alignment is enough unless the
 *     entry says otherwise;
 *   - the kernels pack 2, 4 or 8 problems (or rows) into a wavefront; in a batch that is no multiple of that, the idle
 *     lanes neither load nor store outside these extents;
 *   - no result depends on a byte outside them (nor on what a workspace held before the call).
 * tests/test_gpu_guardband.py runs every family between guard bands at exactly these sizes; DESIGN.md ("Extents and
 * size functions") lists each size function beside the launcher that carves its buffer.
 */

/* Bytes of caller-provided device workspace for dqp_qp_forward (8-byte aligned).  Optional:
 * with workspace == NULL, or a size for which this returns 0, every solver state lives in
 * LDS/registers.  With it, the size-specialised forward kernels eliminate the equality
 * constraints once (null-space form), park the elimination's reflectors there between setup and
 * the final back-transformation -- ~1.4x faster at the metric size, same iterates in exact
 * arithmetic -- and leave the factorisation context (Lq, reflectors, [Gz | W], U, and the particular
 * solution of the equality rows; ~16 KB per QP at the metric size) for dqp_qp_backward and for the
 * finish pass of the batch rule: pass the same buffer with DQP_FLAG_BACKWARD_CTX to skip
 * the refactorisation (2x faster backward).  Without that flag backward needs no workspace. */
size_t dqp_workspace_bytes(const dqp_dims *dims);

/* Bytes of the device buffer DQP_FLAG_BATCH_TERMINATION needs (per-iteration residual history,
 * the batch reduction's accumulators, each problem's best-iteration index and -- sizes served by the null-space kernels --
 * max_iter iterate snapshots of (nz - neq) + 2 nineq + 2 doubles per problem: 12 KB per QP at the
 * metric size); 0 without the flag.  max_iter <= 64. */
size_t dqp_termination_bytes(const dqp_dims *dims, const dqp_opts *opts);

/*
 * The batch-coupled rule over a batch that is SHARDED across devices (the reference's rule couples every
 * sample of the batch it is given, batch.py:119-144; shards of one logical batch can reproduce the stop of
 * the whole batch with one 24-byte exchange):
 *   1. dqp_qp_forward(flags | DQP_FLAG_BATCH_TERMINATION | DQP_FLAG_HISTORY_ONLY) on every shard;
 *   2. dqp_term_local_masks -> masks[3] (device memory): bit `it` of masks[0] = some problem of the shard
 *      improved at iteration it, of masks[1] = some problem has not best_resid < eps, of masks[2] = some problem
 *      has not mu > 1e32;
 *   3. the caller ORs the masks over the shards (e.g. all_reduce(op=BOR) on an int64 tensor);
 *   4. dqp_qp_forward_finish with the combined masks: the rule, then pass 2 of this shard.
 * With the masks of a single shard step 2-4 equal what dqp_qp_forward does in one call.
 */
int dqp_term_local_masks(const dqp_dims *dims, const dqp_opts *opts, void *termination, uint64_t *masks,
                         void *stream);
int dqp_qp_forward_finish(const dqp_dims *dims, const dqp_opts *opts, const double *Q, const double *p,
                          const double *G, const double *h, const double *A, const double *b, double *zhat,
                          double *lam, double *nu, double *slack, int32_t *info, double *best_resid,
                          void *workspace, void *termination, const uint64_t *masks, void *stream);

/*
 * Replaces: qpth.qp.QPFunction(...).forward  (qpth/qp.py:24-126) =
 *           pdipm_b.pre_factor_kkt + pdipm_b.forward (qpth/solvers/pdipm/batch.py:377-428,
 *           46-208), with dyn_res(x) = A x - b and cost_grad(x) = Q x + p; and the forward of
 *           qpth.qp.DenseQPFunction (qpth/qp.py:219-237 + batch_LU.py:29-201), which solves the
 *           same Newton systems through a regularised full-KKT LU.
 * Outputs: zhat (B,nz); lam (B,nineq), nu (B,neq), slack (B,nineq) -- what the reference
 *          stashes on ctx for backward (qp.py:95,125); info (B,2) int32 = {status, PDIPM
 *          iterations run}; best_resid (B) or NULL.
 * Termination: with DQP_FLAG_BATCH_TERMINATION the reference's batch-coupled rule is reproduced
 * exactly (what the Python mirrors use by default).  Without it, termination is per problem
 * (faster in batches larger than the GPU holds at once, float-tolerance parity): the reference's rule is batch-coupled (batch.py:127-144: stop
 * when NO sample improved for not_improved_lim consecutive iterations, so in a large batch
 * every sample effectively runs max_iter iterations).  Here a problem stops when (a) it has
 * not improved for not_improved_lim consecutive iterations AND its best residual is already
 * below stall_tol (converged, stagnating at round-off), (b) its best residual < eps / 10 (one
 * Newton step past the reference's threshold: in the reference every problem of a large batch
 * keeps iterating past eps, and the extra decade is what keeps the duals of weakly active
 * constraints -- and the gradients that depend on lam/slack -- within tolerance of it), (c) its
 * residual is no longer finite (the iterate can never recover; the reference keeps spinning
 * on NaNs), (d) mu > 1e32, or (e) after max_iter iterations.  The best-residual iterate is
 * returned, as in batch.py:119-140,208.
 */
int dqp_qp_forward(const dqp_dims *dims, const dqp_opts *opts,
                   const double *Q, const double *p, const double *G, const double *h,
                   const double *A, const double *b,
                   double *zhat, double *lam, double *nu, double *slack,
                   int32_t *info, double *best_resid,
                   void *workspace, void *termination, void *stream);

/*
 * Replaces: QPFunctionFn.backward (qpth/qp.py:128-183) = factor_kkt + solve_kkt
 *           (batch.py:434-469, 351-374) with rhs (dl_dzhat, 0, 0, 0) and the outer-product
 *           gradient formulas; with DQP_FLAG_DENSE_BACKWARD, DenseQPFunction's Solver.backward
 *           (qp.py:239-270).
 * Writes PER-SAMPLE gradients dQ (B,nz,nz) dp (B,nz) dG (B,nineq,nz) dh (B,nineq)
 * dA (B,neq,nz) db (B,neq); the caller applies .mean(0) for parameters that were shared
 * (qp.py:160-178), or calls dqp_qp_backward_shared (below), which sums them on the device.
 * Any gradient pointer may be NULL to skip it.
 */
int dqp_qp_backward(const dqp_dims *dims, const dqp_opts *opts,
                    const double *Q, const double *G, const double *A,
                    const double *zhat, const double *lam, const double *nu,
                    const double *slack, const double *dl_dzhat,
                    double *dQ, double *dp, double *dG, double *dh, double *dA, double *db,
                    int32_t *info, void *workspace, void *stream);

/*
 * dqp_qp_backward for parameters that are SHARED by the batch (stride 0 in `dims`): the gradient pointer of every
 * such parameter receives ONE unbatched tensor, the SUM over the batch of the per-sample gradients --
 * dQ (nz,nz) dp (nz) dG (nineq,nz) dh (nineq) dA (neq,nz) db (neq) -- and no per-sample copy of it is ever written.
 * The caller divides by nbatch for the reference's .mean(0) (qp.py:160-178); a sum is what an all-reduce over the
 * shards of a larger batch consumes.  Parameters with a non-zero stride get per-sample gradients exactly as from
 * dqp_qp_backward (the same kernel writes them); any gradient pointer may be NULL; the flags mean what they mean there.
 *
 * How: the per-sample kernel of the size's family runs with NULL outputs for the shared matrices and leaves
 * dx, -dlam, -dnu (B, .) in the caller's buffers or in `reduce_ws`; the sums sum_b dG_b = DLAM^T Z + LAM^T DX etc. are
 * split-K GEMMs over the batch on the fp64 matrix cores (64 samples per chunk, one 16 x 16 tile per wavefront, every
 * sample's term rounded as the per-sample kernels round it, partial tiles in `reduce_ws`), finished by a kernel that
 * adds the partials in ascending chunk order.  No atomics: the
 * result depends only on the inputs and nbatch and is bit-identical from run to run.  Three enqueues, no
 * synchronisation, no allocation.
 *
 * reduce_ws: dqp_qp_backward_shared_bytes(dims) bytes of device scratch (8-byte aligned) =
 *   8 * (nbatch (nz + nineq + neq) + ceil(nbatch / 64) * T * 256),  T = 16 x 16 tiles of the shared parameters' gradients;
 * 0 when no parameter is shared (the call is then dqp_qp_backward and reduce_ws may be NULL).  A host function: it
 * needs no device.  With a shared parameter and reduce_ws == NULL: DQP_ERR_BAD_ARG.  nbatch == 0: DQP_OK, nothing
 * is written.  nbatch <= 64 * 65535.
 */
size_t dqp_qp_backward_shared_bytes(const dqp_dims *dims);
int dqp_qp_backward_shared(const dqp_dims *dims, const dqp_opts *opts,
                           const double *Q, const double *G, const double *A,
                           const double *zhat, const double *lam, const double *nu,
                           const double *slack, const double *dl_dzhat,
                           double *dQ, double *dp, double *dG, double *dh, double *dA, double *db,
                           int32_t *info, void *workspace, void *reduce_ws, void *stream);

/* ------------------------------------------------------------------ MPC-structured QPs */

typedef struct dqp_mpc_dims {
    int32_t nbatch;
    int32_t n_state;
    int32_t n_ctrl;
    int32_t T;            /* horizon; nz = T (n_state+n_ctrl), neq = T n_state                */
    int32_t has_bounds;   /* 1: nineq = 2 T n_ctrl (box on u); 0: nineq = n_ctrl placeholder  */
    int32_t dyn_id;       /* dqp_mpc_qp_*: 0, or a registered model (DQP_DYN_*) whose true step replaces
                             F tau + f in the equality residual of the PDIPM iterations -- the
                             reference's dyn_res closure (qp_wrapper.py:309,316); step = dqp_opts.dyn_dt.
                             Served by the stage-wise kernels.  Ignored by dqp_mpc_assemble etc.       */
    int32_t n_state_host; /* dqp_mpc_qp_*: 0 (the routes below), or n' >= n_state with a compiled stage-wise pair
                             (n', n_ctrl) (dqp_mpc_qp_host_n_state): the problem runs on that pair's kernels
                             with n' - n_state dummy states, exactly (see "Padded problems" below).  Needs
                             dyn_id == 0.  Ignored by dqp_mpc_assemble, _line_search, _rollout_backward.      */
} dqp_mpc_dims;

/*
 * Replaces: qp_wrapper.MPC.compute_Qq_dense / compute_Ab_dense / compute_Gh_dense
 *           (qpth/qp_wrapper.py:638-679) as called from single_qp (qp_wrapper.py:311-313).
 * Inputs are the reference's time-major tensors C (T,B,nt,nt) c (T,B,nt) F (T-1,B,n,nt)
 * f (T-1,B,n) x0 (B,n) and the control bounds u_lower/u_upper (n_ctrl,) (ignored without
 * bounds).  Outputs are the dense batch-major QP (Q,p,G,h,A,b) that dqp_qp_forward consumes.
 * Bounds that differ per sample or per knot: dqp_mpc_assemble_bounds ("Per-sample, per-knot control bounds of the MPC
 * QP" below); this entry point is that twin at strides (0, 0).
 */
int dqp_mpc_assemble(const dqp_mpc_dims *dims, const double *C, const double *c, const double *F,
                     const double *f, const double *x0, const double *u_lower,
                     const double *u_upper, double *Q, double *p, double *G, double *h,
                     double *A, double *b, void *stream);

/*
 * Adjoint of dqp_mpc_assemble (what autograd derives from the index scatters of
 * qp_wrapper.py:644-679): gathers dC,dc,dF,df,dx0 from dQ,dp,dA,db.  Any pointer may be NULL
 * (missing inputs read as zero, missing outputs are skipped).
 */
int dqp_mpc_assemble_backward(const dqp_mpc_dims *dims, const double *dQ, const double *dp,
                              const double *dA, const double *db, double *dC, double *dc,
                              double *dF, double *df, double *dx0, void *stream);

/*
 * The MPC QP end to end without the dense detour: what qp_wrapper.MPC.single_qp does between
 * linearize_dynamics and the line search (qp_wrapper.py:311-319: compute_Qq/Ab/Gh_dense +
 * qp.DenseQPFunction()) in ONE solve launch -- the kernel builds the rows of (Q,p,G,h,A,b) in
 * registers from (C,c,F,f,x0,bounds) and solves; backward scatters straight into
 * (dC,dc,dF,df,dx0) (the adjoint of the assembly applied on chip).  HBM traffic per QP at
 * n=3 m=3 T=5: 0.7 k doubles in instead of 2.3 k, 0.3 k gradient doubles out instead of 2.3 k.
 * Needs control bounds, a supported shape (dqp_mpc_qp_supported) and the workspace
 * (dqp_mpc_qp_workspace_bytes).  Two kernel families serve it:
 *   - QP sizes with a null-space kernel (small horizons, nz <= 48): the whole QP lives in registers, the
 *     workspace carries the factorisation context from forward to backward (C, F unused by backward);
 *   - any other horizon with a compiled (n_state, n_ctrl) pair, n_state + n_ctrl <= 32 -- e.g.
 *     BASELINE config 4: n 12, m 4, T 30, nz 480 --: stage-wise PDIPM, every KKT solve a Riccati
 *     recursion over the knots (O(T (n+m)^3)); iterates and per-knot factors stream through the
 *     workspace; backward refactors at the returned iterate and needs C and F again.  Pairs with
 *     n + m <= 16 run four QPs per wavefront (one 16-lane DPP row each), the wide pairs (13, 4), (14, 7)
 *     and (24, 8) two (one 32-lane half-wavefront each).
 * Workspace of the stage-wise kernels, bytes: 8 * Bp * W with Bp = B rounded up to a multiple of 4
 * (n + m <= 16) or of 2 (wide pairs), nt = n + m, ev(x) = x rounded up to even, and
 *     W = ev(ev(ev(T (3 nt + 4 n + 14 m)) + T n^2) + T nt m + T (n + m))
 * (dqp_mpc_qp_stepped_workspace_bytes: 8 * Bp * (W + 8)).
 * Padded problems (n_state_host = n' != 0): the kernels of the pair (n', m) -- native, or one of the host-only pairs
 * (15,1) (14,2) (13,3) (11,5) (10,6) (9,7) (8,8) (31,1) (30,2) (29,3) (28,4) (27,5) (26,6) (25,7) -- solve the problem
 * with d = n' - n dummy states after the real ones in every knot: identity cost and zero linear cost on them, zero
 * dynamics rows, zero start.  Every Newton system is then block-diagonal in (real, dummy), so the iterates, stop
 * iteration and gradients are those of the (n, m) problem up to round-off; the null-space route is never taken.
 * Caller arrays keep the compact (n, m) shapes.  Workspace bytes: 8 * (Bp' * W' + R) with W' = W at (n', m), Bp' = B
 * rounded up as for that pair (stepped: Bp' * (W' + 8)), nt' = n' + m, and the padded copies
 *     R = 2 (ev(T B nt'^2) + ev((T-1) B n' nt') + 2 ev(T B nt') + ev(T B n') + ev((T-1) B n') + ev(B n')).
 * Bad arguments: n' < n, (n', m) not compiled, dyn_id != 0.  The stepped call with it_begin == 0 copies C, c, F, f, x0
 * into the workspace; the later calls of the solve read that copy.
 * tau (B, T, n_state+n_ctrl) = the QP solution per knot [x_t, u_t]; lam/nu/slack/info/best_resid and
 * the termination modes as in dqp_qp_forward; backward = DenseQPFunction's (un-clamped d).
 * u_lower/u_upper (n_ctrl,) hold for every sample and knot; dqp_mpc_qp_forward_bounds takes them per sample and per knot
 * (dqp_mpc_qp_forward is that twin at strides (0, 0)).  The backward reads no bounds.
 */
int dqp_mpc_qp_supported(const dqp_mpc_dims *dims);
size_t dqp_mpc_qp_workspace_bytes(const dqp_mpc_dims *dims);
/* the smallest n' >= n_state with a compiled stage-wise pair (n', n_ctrl), native or host-only (ascending n': the 16-lane
 * pairs before the wide ones), or 0 if there is none (n_ctrl > 8, n_state + n_ctrl > 32); needs has_bounds and
 * dyn_id == 0, ignores n_state_host, T and nbatch */
int32_t dqp_mpc_qp_host_n_state(const dqp_mpc_dims *dims);
/* the `termination` buffer of dqp_mpc_qp_forward under DQP_FLAG_BATCH_TERMINATION (history, best-iteration list and the
 * improving iterates of pass 1, from which pass 2 finishes without solving again); 0 without the flag */
size_t dqp_mpc_qp_termination_bytes(const dqp_mpc_dims *dims, const dqp_opts *opts);
int dqp_mpc_qp_forward(const dqp_mpc_dims *dims, const dqp_opts *opts, const double *C, const double *c,
                       const double *F, const double *f, const double *x0, const double *u_lower,
                       const double *u_upper, double *tau, double *lam, double *nu, double *slack,
                       int32_t *info, double *best_resid, void *workspace, void *termination,
                       void *stream);
int dqp_mpc_qp_backward(const dqp_mpc_dims *dims, const dqp_opts *opts, const double *C, const double *F,
                        const double *tau, const double *lam, const double *nu, const double *slack,
                        const double *dl_dtau, double *dC, double *dc, double *dF, double *df,
                        double *dx0, int32_t *info, void *workspace, void *stream);

/*
 * dqp_mpc_qp_forward for a dynamics model the library cannot evaluate (a caller's torch module):
 * the reference passes its PDIPM a Python closure for the equality residual and calls it once per iteration on
 * the current iterate (qp_wrapper.py:309,316 -> batch_LU.py:97: ry = dyn_res(x)).  Here the caller drives the
 * iterations: a call runs ONE PDIPM iteration (it_end == it_begin + 1) of the stage-wise kernels with
 * `ext_ry` (B, T n_state) as the equality residual of the current iterate, in the closure's ordering
 * [f(x_t,u_t) - x_{t+1} (t < T-1) ; x_0 - x0] (qp_wrapper.py:326-345; the last n_state entries are recomputed on
 * chip).  The call it_begin == it_end == 0 only computes the starting point (batch_LU.py:60-86); it_begin == 0,
 * it_end == 1 computes it and runs iteration 0 on ext_ry -- for callers that know the starting iterate.  After every call `tau`
 * holds the CURRENT iterate (B, T, n_state+n_ctrl), on which the caller evaluates its model for the next call; the
 * call with it_end == opts->max_iter finishes as dqp_mpc_qp_forward does (batch rule included) and leaves the
 * returned best iterate and its multipliers in tau, lam, nu, slack.  All solver state between calls lives in
 * `workspace` (dqp_mpc_qp_stepped_workspace_bytes: always the caller's buffer) and `termination`.
 * Shapes: the stage-wise pairs of dqp_mpc_qp_forward (compiled (n_state, n_ctrl), n_state + n_ctrl <= 32).
 * Bounds per sample and per knot: dqp_mpc_qp_forward_stepped_bounds (this entry point is that twin at strides (0, 0));
 * every call of one solve passes the same bounds.
 */
size_t dqp_mpc_qp_stepped_workspace_bytes(const dqp_mpc_dims *dims);
size_t dqp_mpc_qp_stepped_termination_bytes(const dqp_mpc_dims *dims, const dqp_opts *opts);
int dqp_mpc_qp_forward_stepped(const dqp_mpc_dims *dims, const dqp_opts *opts, const double *C, const double *c,
                               const double *F, const double *f, const double *x0, const double *u_lower,
                               const double *u_upper, const double *ext_ry, int32_t it_begin, int32_t it_end,
                               double *tau, double *lam, double *nu, double *slack, int32_t *info,
                               double *best_resid, void *workspace, void *termination, void *stream);

/*
 * Replaces: qp_wrapper.MPC.line_search with its rollouts and cost evaluations
 * (qpth/qp_wrapper.py:417-436, 598-611, 690-692; ~60 torch ops and one host sync per round): backtracking
 * on the TRUE rollout cost, alpha in {1, decay, decay^2, ...}, per trajectory, in one launch.
 * Dynamics: dyn_id == 0 -> LinDx (F (T-1,B,n,nt), f (T-1,B,n)), else a registered device model
 * (DQP_DYN_*, step dt).  x (T,B,n), u (T,B,m): current trajectory; delta_u (T,B,m): the QP step; C, c
 * the quadratic cost.  Outputs: the last trial x_new, u_new, its cost, and alpha (B) with the
 * reference's convention (a trajectory that never improved carries one extra decay).
 * With C == NULL (then x, delta_u, c may be NULL) the call is the plain rollout of u from x0
 * (qp_wrapper.py:598-611): x_new = states, u_new = u.
 */
int dqp_mpc_line_search(const dqp_mpc_dims *dims, int dyn_id, double dt, const double *F, const double *f,
                        const double *x0, const double *x, const double *u, const double *delta_u,
                        const double *C, const double *c, double decay, int32_t max_iter,
                        double *x_new, double *u_new, double *alpha, double *cost_new, void *stream);

/*
 * Adjoint of the rollout x_{t+1} = f(x_t, u_t) (what autograd derives from qp_wrapper.py:598-611):
 * x (T,B,n) the rolled-out states, u (T,B,m), g_x (T,B,n) the cotangent of the states; outputs
 * d_x0 (B,n), d_u (T,B,m), and for LinDx (dyn_id == 0) d_F (T-1,B,n,nt), d_f (T-1,B,n).  Any output
 * may be NULL.  Registered models differentiate through the same forward-mode templates as
 * dqp_dyn_jacobian.
 */
int dqp_mpc_rollout_backward(const dqp_mpc_dims *dims, int dyn_id, double dt, const double *F,
                             const double *x, const double *u, const double *g_x, double *d_x0,
                             double *d_u, double *d_F, double *d_f, void *stream);

/* ------------------------------------------------------------ augmented-Lagrangian Newton */

typedef struct dqp_al_dims {
    int32_t nbatch;
    int32_t nz;        /* T (n_state + n_ctrl) <= 128                                      */
    int32_t ncon;      /* rows of the (clamped) constraint Jacobian: neq + nineq           */
    int32_t reserved;
} dqp_al_dims;

/*
 * Replaces, inside NewtonAL.forward (qpth/al_utils.py:403-427):
 *   merit_hess = diag(Q) + rho * Jc^T Jc                  (al_utils.py:96-102, 176-178)
 *   U, info = torch.linalg.cholesky_ex(merit_hess);  update = -cholesky_solve(grad, U)
 * Jc (B,ncon,nz) is the clamped constraint Jacobian, Qdiag (B,nz), rho (B), grad (B,nz).
 * Outputs: update (B,nz) (NaN when the factorisation fails, as the reference's NaN test at
 * al_utils.py:419 expects), L (B,nz,nz) lower Cholesky factor with a zero upper part (or NULL),
 * info (B) = 0 or the order of the first non-positive leading minor (cholesky_ex's info).
 */
int dqp_al_newton_step(const dqp_al_dims *dims, const double *Jc, const double *Qdiag,
                       const double *rho, const double *grad, double *update, double *L,
                       int32_t *info, void *stream);

/* Replaces NewtonAL.backward's  -torch.cholesky_solve(x_grad, U)  (al_utils.py:477-480):
 * out = -(L L^T)^-1 rhs. */
int dqp_al_chol_solve(const dqp_al_dims *dims, const double *L, const double *rhs, double *out,
                      void *stream);

/*
 * Replaces the Jacobian fill of al_utils.constraint_res_jac2 / dyn_res_eq_jac / dyn_res_ineq_jac
 * (qpth/al_utils.py:162-318: vmap(block_diag), zero-fills, index scatters, the active-set mask)
 * and the two bmm's J^T lam + rho Jc^T res_c of merit_grad_hessian (al_utils.py:62-102).
 * Inputs: the per-knot dynamics Jacobians Jx (B,T-1,n,n) = df/dx_t and Ju (B,T-1,n,m) = df/du_t,
 * lam (B,ncon), res_c (B,ncon) = the residual with inactive inequalities clamped to 0, rho (B).
 * Row order: (T-1) n dynamics rows x_{t+1} - f(x_t,u_t) knot-major, n rows x_0 - x0, then per
 * knot [u - u_upper (m), u_lower - u (m)]; columns per knot [x_t (n), u_t (m)];
 * ncon = T n + 2 T m, nz = T (n + m).
 * Outputs: Jc (B,ncon,nz) with the rows of inactive inequalities (res_c <= 0) zeroed (every
 * element written exactly once), gterm (B,nz) = J^T lam + rho Jc^T res_c.  Either may be NULL.
 */
typedef struct dqp_al_mpc_dims {
    int32_t nbatch;
    int32_t n_state;
    int32_t n_ctrl;
    int32_t T;
} dqp_al_mpc_dims;

int dqp_al_assemble(const dqp_al_mpc_dims *dims, const double *Jx, const double *Ju,
                    const double *lam, const double *res_c, const double *rho, double *Jc,
                    double *gterm, void *stream);

/*
 * Replaces al_utils.merit_function (qpth/al_utils.py:37-59) after the dynamics have been
 * evaluated:  merit = sum (1/2 Q xu^2 + q xu) + rho/2 |res_c|^2 + lam . res  with res the
 * residual vector in dqp_al_assemble's row order (x_{t+1} - x_next_t, x_0 - x0, u - u_upper,
 * u_lower - u) and res_c its clamped form.  ncand candidate trajectories per problem (the
 * 20-way line search of line_search_newton, al_utils.py:503-527, evaluates them as one batch)
 * share the problem's x0, Qdiag, q, lam, rho: xu (ncand,B,T,n+m), x_next (ncand,B,T-1,n) =
 * f(x_t,u_t) for the first T-1 knots, x0 (B,n), Qdiag/q (B,T,n+m), lam (B,ncon), rho (B),
 * u_lower/u_upper (m).  Output merit (ncand,B).
 */
int dqp_al_merit(const dqp_al_mpc_dims *dims, int32_t ncand, const double *xu, const double *x_next,
                 const double *x0, const double *Qdiag, const double *q, const double *lam,
                 const double *rho, const double *u_lower, const double *u_upper, double *merit,
                 void *stream);

/*
 * NewtonAL.forward for a registered device model (qpth/al_utils.py:363-456 with
 * merit_grad_hessian :62-102, constraint_res_jac2 :162-318 and line_search_newton :503-527):
 * n_steps Newton steps on the augmented Lagrangian, each = linearise the dynamics along xu
 * (forward-mode Jacobians) -> clamped constraint Jacobian + merit gradient -> Hessian (fp64 MFMA) +
 * Cholesky + solve -> merit of the 20 candidate steps 2^-k (dynamics evaluated in the kernel) ->
 * argmin / acceptance / update.  5 launches per step, nothing returns to the host in between.
 * xu (B,T,n+m) in/out; x0 (B,n); Qdiag, q (B,T,n+m); lam (B,ncon), rho (B); u_lower/u_upper (m).
 * Outputs: L (B,nz,nz) the Cholesky factor of the LAST step's Hessian (what NewtonAL.backward
 * needs, al_utils.py:458,477-480), status (B) 1.0 where the last line search accepted its step,
 * fail (one int32) != 0 when a Cholesky factorisation broke down (the reference then switches the
 * whole batch to an LU solve, al_utils.py:419-427: the caller re-runs its general path).
 * Dense form (banded == 0): n_state <= 8, n_ctrl <= 2, nz <= 128, L is (B,nz,nz).
 * Banded form (banded != 0): n_state <= 12, n_state + n_ctrl <= 16, any T (BASELINE config 4:
 * n 12, m 4, T 30, nz 480); L is the buffer of dqp_al_banded_factor_bytes (see below).
 * The workspace size depends on the form: banded, 8 * nbatch * (T (n_state + n_ctrl) + 22) bytes -- per problem the
 * update, the 20 candidate merits, the current merit and one double's room for the int32 pivot flag; dense, 8 * nbatch *
 * ((T-1) n^2 + (T-1) n m + ncon + ncon nz + 2 nz + 22) with n = n_state, m = n_ctrl, nz = T (n + m), ncon = T n + 2 T m
 * (the Jacobians, the residual, the constraint Jacobian, gradient and update before the same tail).  That is the whole
 * carve: earlier versions reported 16 bytes more, which no launch touched.
 */
size_t dqp_al_newton_solve_bytes(const dqp_al_mpc_dims *dims, int32_t banded);
int dqp_al_newton_solve(const dqp_al_mpc_dims *dims, int dyn_id, double dt, int32_t n_steps, int32_t banded,
                        const double *x0, const double *Qdiag, const double *q, const double *lam,
                        const double *rho, const double *u_lower, const double *u_upper, double *xu, double *L,
                        double *status, int32_t *fail, void *workspace, void *stream);

/*
 * Between two augmented-Lagrangian iterations (qpth/AL_mpc.py:296-307) for a registered device model:
 * lam_new = lam + rho res with the inequality block clamped at 0, cost (B) of the iterate
 * (diagonal cost), res_norm (B) = |clamped residual|; res in the row order of dqp_al_assemble.
 */
int dqp_al_outer_update(const dqp_al_mpc_dims *dims, int dyn_id, double dt, const double *xu, const double *x0,
                        const double *lam, const double *rho, const double *Qdiag, const double *q,
                        const double *u_lower, const double *u_upper, double *lam_new, double *cost,
                        double *res_norm, void *stream);

/*
 * Replaces: AL_mpc.MPC.al_solve for a registered device model (qpth/AL_mpc.py:254-321) as ONE call with no host
 * involvement: xu = [x_init | u_init]; cost_start; the warm start of (lam, rho) from the previous call's history
 * (al_utils.warm_start_al, al_utils.py:16-34; n_prev = 0 after reinitialize()); then al_iter times
 * [dqp_al_newton_solve (block-tridiagonal, newton_steps Newton steps with the 20-candidate line search) ->
 * lam <- clamp(lam + rho res), cost, |res_clamp|, rho <- 10 rho (AL_mpc.py:296-307)].
 * History layout, oldest first as the reference keeps it: hist_cost (al_iter+1, B), hist_lam (al_iter+1, B, ncon),
 * hist_rho (al_iter+1, B), entry 0 = the (warm-started) start, entry i+1 = after AL iteration i; the final
 * multipliers / penalty are the last entry (what the reference stores in lamda_prev / rho_prev).  prev_* = the
 * hist_* arrays of the previous call (n_prev entries).  xu (B, T, n+m) out; res_norm (B) = |res_clamp| of the last
 * iterate; factor (dqp_al_banded_factor_bytes) = the block-tridiagonal factor of the LAST Newton step, for
 * dqp_al_banded_solve (NewtonAL.backward); fail (al_iter int32): set where a Cholesky pivot was not positive in
 * that AL iteration (the reference then solves by LU: redo the call on the general path); workspace:
 * dqp_al_mpc_solve_bytes.  ncon = T n_state + 2 T n_ctrl.  n_state + n_ctrl <= 16, n_state <= 12.
 */
size_t dqp_al_mpc_solve_bytes(const dqp_al_mpc_dims *dims);
int dqp_al_mpc_solve(const dqp_al_mpc_dims *dims, int dyn_id, double dt, int32_t al_iter, int32_t newton_steps,
                     const double *x_init, const double *u_init, const double *x0, const double *Qdiag, const double *q,
                     const double *u_lower, const double *u_upper, const double *lam_in, const double *rho_in,
                     const double *prev_cost, const double *prev_lam, const double *prev_rho, int32_t n_prev,
                     double *xu, double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm, double *factor,
                     double *status, int32_t *fail, void *workspace, void *stream);

/*
 * dqp_al_mpc_solve as ONE kernel launch, for small batches (csrc/dqp_al_fused.hip): the same arguments, outputs and
 * arithmetic (up to summation order), so a caller switches by name.  One problem per one-wavefront workgroup; the
 * iterate, the cost, the multipliers, the update and the factor of the current Newton step stay in LDS for the whole
 * solve, the forward-mode Jacobians of eight knots are evaluated at once and the 20 line-search candidates are split
 * over the wavefront's eight lane groups.  No workgroup waits for another one (no cooperative launch, no grid barrier).
 * `factor` receives the factor of the last Newton step of the last AL iteration in the layout dqp_al_banded_solve
 * reads (it does not depend on dqp_al_lane_group).  `fail` is cleared by a memset enqueued in front of the launch.
 * Only enqueues on `stream` (capturable): no synchronisation, no allocation.
 *
 * dqp_al_mpc_solve_fused_supported: 1 for a registered model with n_state + n_ctrl <= 8 (DQP_DYN_PENDULUM1L,
 * CARTPOLE1L, CARTPOLE2L, PENDULUM_EULER, PENDULUM_DX, INTEGRATOR) at 2 <= T <= 32, else 0 (DQP_DYN_REXQUADROTOR, longer horizons:
 * dqp_al_mpc_solve serves them).  Needs no device.  dqp_al_mpc_solve_fused returns DQP_ERR_BAD_ARG / DQP_ERR_TOO_LARGE
 * by the rules of dqp_al_mpc_solve, DQP_ERR_TOO_LARGE wherever _supported is 0 at valid arguments, and DQP_OK at
 * nbatch == 0 (nothing is touched).  dqp_al_mpc_solve_fused_bytes: the workspace size a caller passes -- that of
 * dqp_al_mpc_solve_bytes, so that one buffer serves both entries; the fused kernel itself does not write to it.
 */
int dqp_al_mpc_solve_fused_supported(const dqp_al_mpc_dims *dims, int dyn_id);
size_t dqp_al_mpc_solve_fused_bytes(const dqp_al_mpc_dims *dims);
int dqp_al_mpc_solve_fused(const dqp_al_mpc_dims *dims, int dyn_id, double dt, int32_t al_iter, int32_t newton_steps,
                           const double *x_init, const double *u_init, const double *x0, const double *Qdiag,
                           const double *q, const double *u_lower, const double *u_upper, const double *lam_in,
                           const double *rho_in, const double *prev_cost, const double *prev_lam, const double *prev_rho,
                           int32_t n_prev, double *xu, double *hist_cost, double *hist_lam, double *hist_rho,
                           double *res_norm, double *factor, double *status, int32_t *fail, void *workspace,
                           void *stream);

/*
 * The same Newton step with the MPC structure exploited (`banded` != 0 above uses it): the Hessian
 * diag(Q) + rho Jc^T Jc is block tridiagonal in the knots, so linearisation, gradient, block Cholesky
 * and the solve run as ONE launch with every knot in registers (4 problems per wavefront), O(T (n+m)^3)
 * work, no Jacobian or Hessian in HBM.  `factor` (dqp_al_banded_factor_bytes) receives the banded
 * Cholesky factor -- per knot L_tt, 1/diag(L_tt) and L_{t+1,t}^T, in a layout private to the library (element-major
 * over the knot's lanes) -- which dqp_al_banded_solve applies for NewtonAL.backward (out = -(L L^T)^-1 rhs,
 * al_utils.py:477-480).  dqp_al_newton_solve / dqp_al_mpc_solve leave the factor of their LAST Newton step in it.
 * info (B): 0, or 1 + the knot at which a pivot was not positive.
 */
size_t dqp_al_banded_factor_bytes(const dqp_al_mpc_dims *dims, int dyn_id);
int dqp_al_banded_newton_step(const dqp_al_mpc_dims *dims, int dyn_id, double dt, const double *xu,
                              const double *x0, const double *Qdiag, const double *q, const double *lam,
                              const double *rho, const double *u_lower, const double *u_upper,
                              double *update, void *factor, int32_t *info, void *stream);
int dqp_al_banded_solve(const dqp_al_mpc_dims *dims, int dyn_id, const void *factor, const double *rhs,
                        double *out, void *stream);
/*
 * The same step for a dynamics the CALLER linearised -- a torch module with its own Jacobians such as
 * deqmpc/envs.py:50-82 or RexQuadrotor_dynamics_jac (rex_quadrotor.py:131-146) -- at any horizon:
 * x_next (B,T-1,n) = f(x_t,u_t), Jx (B,T-1,n,n) = df/dx, Ju (B,T-1,n,m) = df/du instead of a registered
 * model.  Lifts the nz <= 128 limit of dqp_al_newton_step for user dynamics (config 4 with the reference's
 * own quadrotor module: nz = 480).  Compiled (n_state, n_ctrl) pairs: DQP_BAND_SIZES (n_state + n_ctrl <= 16: one
 * problem per 8 or 16 lanes) and DQP_BAND_WIDE_SIZES (16 < n_state + n_ctrl <= 32: one problem per 32-lane
 * half-wavefront, csrc/dqp_al_banded_wide.hip) in csrc/dqp_al_banded_kernels.h; others return DQP_ERR_TOO_LARGE.
 * `factor` has dqp_al_banded_jac_factor_bytes(dims) bytes and is applied by dqp_al_banded_solve(dims, 0, ...).
 *
 * dqp_al_banded_jac_factor_bytes: the factor buffer size of this call at every pair it accepts -- at the
 * DQP_BAND_SIZES pairs the value of dqp_al_banded_factor_bytes(dims, 0), at the DQP_BAND_WIDE_SIZES pairs
 * 8 B T nt (nt + 1 + n_state) with nt = n_state + n_ctrl (the same per-knot layout); 0 for T < 2, nbatch <= 0, a null
 * `dims` or a pair that is not compiled.  dqp_al_banded_factor_bytes(dims, 0) itself stays 0 at the wide pairs
 * (callers read a zero there as "no 8- / 16-lane kernel").
 */
size_t dqp_al_banded_jac_factor_bytes(const dqp_al_mpc_dims *dims);
int dqp_al_banded_newton_step_jac(const dqp_al_mpc_dims *dims, const double *xu, const double *x0,
                                  const double *Qdiag, const double *q, const double *lam, const double *rho,
                                  const double *u_lower, const double *u_upper, const double *x_next,
                                  const double *Jx, const double *Ju, double *update, void *factor,
                                  int32_t *info, void *stream);

/* Testing / A-B runs: pins how many lanes a problem of the block-tridiagonal kernels occupies (8: two problems per
 * 16-lane DPP row where n_state + n_ctrl <= 8; 16: one per row; 0: chosen from the batch size and the device's CU
 * count, the default).  The environment variable DQP_AL_LANE_GROUP=8|16 sets the initial value (read once).  The
 * DQP_BAND_WIDE_SIZES pairs always take a 32-lane half-wavefront and ignore it. */
int dqp_al_lane_group(int width);

/*
 * Per-sample, per-knot control bounds (additive at 303).  Every entry point above that takes `u_lower` / `u_upper`
 * reads a vector of n_ctrl doubles shared by the batch and the horizon.  Its `_bounds` twin below takes the bounds as a
 * dqp_al_bounds instead -- in the position of the (u_lower, u_upper) pair, every other argument unchanged -- and reads
 *
 *     lower[b * stride_b + t * stride_t + k],   upper[the same index]
 *
 * for sample b, knot t, control k (element strides).  stride_b is 0 or T * n_ctrl, stride_t is 0 or n_ctrl:
 *
 *     (0, 0)                 n_ctrl doubles            the vector form -- the twin then launches exactly the kernels
 *                                                      of the old entry point, which is itself the twin at (0, 0)
 *     (0, n_ctrl)            (T, n_ctrl)               the same limits for every sample, varying along the horizon
 *     (n_ctrl, 0)            (B, 1, n_ctrl)            per sample, constant along the horizon: B n_ctrl doubles, packed
 *     (T n_ctrl, 0)          (B, T, n_ctrl)            the same, read from knot 0 of a full array
 *     (T n_ctrl, n_ctrl)     (B, T, n_ctrl)            per sample and per knot
 *
 * i.e. stride_t is 0 or n_ctrl and stride_b is 0, T n_ctrl or -- only at stride_t == 0 -- n_ctrl, the packed per-sample
 * form, so that no caller has to expand its bounds along the horizon.  The largest index read is
 * (nbatch - 1) stride_b + (T - 1) stride_t + n_ctrl - 1.  Any other stride, a null struct or a null lower / upper pointer
 * returns DQP_ERR_BAD_ARG (struct and strides are checked in front of the nbatch == 0 return, the pointers behind it, as
 * every other buffer).  Rows of a knot are [u - upper (m), lower - u (m)] as before; lower == upper at a knot freezes
 * that control there.
 *
 * Kernels: the block-tridiagonal Newton step (registered models and the DQP_BAND_SIZES pairs), the line-search / merit,
 * outer-update and single-launch kernels have a strided instantiation next to the vector one.  The DQP_BAND_WIDE_SIZES
 * pairs have none without a state box: dqp_al_banded_newton_step_jac_bounds returns DQP_ERR_TOO_LARGE for them at
 * non-zero strides.  With a state box (dqp_al_banded_newton_step_jac_xbounds below) they take every layout of the table,
 * because that kernel reads both boxes through their strides.
 * dqp_al_banded_solve (NewtonAL.backward) does not read the bounds -- the factor already carries the active set -- and
 * has no twin.  The single-launch solve stages the 2 T n_ctrl bounds of its problem in LDS next to the problem;
 * dqp_al_mpc_solve_fused_lds_bytes reports the launch's LDS (0 where _supported_bounds is 0).
 */
typedef struct dqp_al_bounds {
    const double *lower, *upper;
    int64_t stride_b, stride_t;
} dqp_al_bounds;

int dqp_al_merit_bounds(const dqp_al_mpc_dims *dims, int32_t ncand, const double *xu, const double *x_next,
                        const double *x0, const double *Qdiag, const double *q, const double *lam,
                        const double *rho, const dqp_al_bounds *bounds, double *merit, void *stream);
int dqp_al_newton_solve_bounds(const dqp_al_mpc_dims *dims, int dyn_id, double dt, int32_t n_steps, int32_t banded,
                               const double *x0, const double *Qdiag, const double *q, const double *lam,
                               const double *rho, const dqp_al_bounds *bounds, double *xu, double *L,
                               double *status, int32_t *fail, void *workspace, void *stream);
int dqp_al_outer_update_bounds(const dqp_al_mpc_dims *dims, int dyn_id, double dt, const double *xu, const double *x0,
                               const double *lam, const double *rho, const double *Qdiag, const double *q,
                               const dqp_al_bounds *bounds, double *lam_new, double *cost, double *res_norm,
                               void *stream);
int dqp_al_mpc_solve_bounds(const dqp_al_mpc_dims *dims, int dyn_id, double dt, int32_t al_iter, int32_t newton_steps,
                            const double *x_init, const double *u_init, const double *x0, const double *Qdiag,
                            const double *q, const dqp_al_bounds *bounds, const double *lam_in, const double *rho_in,
                            const double *prev_cost, const double *prev_lam, const double *prev_rho, int32_t n_prev,
                            double *xu, double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm,
                            double *factor, double *status, int32_t *fail, void *workspace, void *stream);
int dqp_al_mpc_solve_fused_supported_bounds(const dqp_al_mpc_dims *dims, int dyn_id, const dqp_al_bounds *bounds);
size_t dqp_al_mpc_solve_fused_bytes_bounds(const dqp_al_mpc_dims *dims, const dqp_al_bounds *bounds);
size_t dqp_al_mpc_solve_fused_lds_bytes(const dqp_al_mpc_dims *dims, int dyn_id, const dqp_al_bounds *bounds);
int dqp_al_mpc_solve_fused_bounds(const dqp_al_mpc_dims *dims, int dyn_id, double dt, int32_t al_iter,
                                  int32_t newton_steps, const double *x_init, const double *u_init, const double *x0,
                                  const double *Qdiag, const double *q, const dqp_al_bounds *bounds,
                                  const double *lam_in, const double *rho_in, const double *prev_cost,
                                  const double *prev_lam, const double *prev_rho, int32_t n_prev, double *xu,
                                  double *hist_cost, double *hist_lam, double *hist_rho, double *res_norm,
                                  double *factor, double *status, int32_t *fail, void *workspace, void *stream);
int dqp_al_banded_newton_step_bounds(const dqp_al_mpc_dims *dims, int dyn_id, double dt, const double *xu,
                                     const double *x0, const double *Qdiag, const double *q, const double *lam,
                                     const double *rho, const dqp_al_bounds *bounds, double *update, void *factor,
                                     int32_t *info, void *stream);
int dqp_al_banded_newton_step_jac_bounds(const dqp_al_mpc_dims *dims, const double *xu, const double *x0,
                                         const double *Qdiag, const double *q, const double *lam, const double *rho,
                                         const dqp_al_bounds *bounds, const double *x_next, const double *Jx,
                                         const double *Ju, double *update, void *factor, int32_t *info, void *stream);

/*
 * State bounds x_lower <= x_t <= x_upper on the block-tridiagonal AL paths of a registered model (additive at 303; for
 * caller-linearised dynamics see dqp_al_banded_newton_step_jac_xbounds below).
 * Each `_xbounds` entry below is its `_bounds` twin plus one `const dqp_al_bounds *xbounds` behind `bounds`, every other
 * argument unchanged (dqp_al_newton_solve_xbounds is the block-tridiagonal form only and has no `banded`).  The state box
 * is a second dqp_al_bounds with n_state in place of n_ctrl in the stride rules above: lower / upper of sample b, knot t,
 * state k at [b * stride_b + t * stride_t + k], layouts (0, 0), (0, n_state), (n_state, 0), (T n_state, 0),
 * (T n_state, n_state).  Bounds must be finite (a row of an infinite bound would make 0 * inf in lam . res): use a large
 * finite number for "no bound".
 *
 * Rows: res = [ equality rows (T n) | control rows (2 T m) | state rows (2 T n) ], the first two blocks where they were;
 * the state block is knot-major, per knot [x_t - x_upper (n), x_lower - x_t (n)], all knots 0 .. T-1 (knot 0's rows are
 * constant along a line search: x_0 is pinned to x0), clamped at 0 for the penalty term and their multipliers clamped at
 * 0 by the outer update, like the control rows.  lam, lam_new, lam_in, prev_lam and hist_lam have
 * dqp_al_ncon_xbounds(dims) = T n + 2 T m + 2 T n columns.  A state row adds to the diagonal of H_tt and to the gradient
 * of its knot only, so the factor keeps its shape: dqp_al_banded_factor_bytes and dqp_al_banded_solve (the backward) serve
 * these entries as they are.  The `_bytes` queries are those of the twins.
 *
 * Return codes, in front of the nbatch == 0 return and in this order: DQP_ERR_BAD_ARG for a null dims, nbatch < 0,
 * n_state / n_ctrl <= 0, T < 2, a null `bounds` / `xbounds` or one with strides outside its table;
 * DQP_ERR_TOO_LARGE for n_state + n_ctrl > 16 or n_state > 12; DQP_ERR_BAD_ARG for a `model` that is not registered or
 * whose sizes are not the dims'.  Then nbatch == 0 is DQP_OK with nothing enqueued; behind it null buffers (the lower /
 * upper of either box included) and the twins' other argument errors are DQP_ERR_BAD_ARG.  Kernels: the BoxBounds<>
 * instantiations of the Newton, line-search and outer-update kernels (csrc/dqp_al_bounds.h), which read both boxes
 * through their strides.  Only enqueue on `stream`.
 */
int32_t dqp_al_ncon_xbounds(const dqp_al_mpc_dims *dims);
int dqp_al_banded_newton_step_xbounds(const dqp_al_mpc_dims *dims, int model, double dt, const double *xu,
                                      const double *x0, const double *Qdiag, const double *q, const double *lam,
                                      const double *rho, const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds,
                                      double *update, void *factor, int32_t *info, void *stream);
size_t dqp_al_newton_solve_xbounds_bytes(const dqp_al_mpc_dims *dims);
int dqp_al_newton_solve_xbounds(const dqp_al_mpc_dims *dims, int model, double dt, int32_t n_steps, const double *x0,
                                const double *Qdiag, const double *q, const double *lam, const double *rho,
                                const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, double *xu, double *L,
                                double *status, int32_t *fail, void *workspace, void *stream);
int dqp_al_outer_update_xbounds(const dqp_al_mpc_dims *dims, int model, double dt, const double *xu, const double *x0,
                                const double *lam, const double *rho, const double *Qdiag, const double *q,
                                const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, double *lam_new, double *cost,
                                double *res_norm, void *stream);
size_t dqp_al_mpc_solve_xbounds_bytes(const dqp_al_mpc_dims *dims);
int dqp_al_mpc_solve_xbounds(const dqp_al_mpc_dims *dims, int model, double dt, int32_t al_iter, int32_t newton_steps,
                             const double *x_init, const double *u_init, const double *x0, const double *Qdiag,
                             const double *q, const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds,
                             const double *lam_in, const double *rho_in, const double *prev_cost, const double *prev_lam,
                             const double *prev_rho, int32_t n_prev, double *xu, double *hist_cost, double *hist_lam,
                             double *hist_rho, double *res_norm, double *factor, double *status, int32_t *fail,
                             void *workspace, void *stream);

/*
 * dqp_al_mpc_solve_xbounds as ONE kernel launch (additive at 303; csrc/dqp_al_fused.hip): the argument list, the rows, the
 * outputs and the kept factor of dqp_al_mpc_solve_xbounds, up to summation order, for the models and horizons of
 * dqp_al_mpc_solve_fused (n_state + n_ctrl <= 8, 2 <= T <= 32).  Kernels: al_solve_fused_kernel<BoxBounds<Model>>, which
 * reads both boxes through their strides (`bounds` may be the vector form) and stages them in LDS next to the problem.
 * dqp_al_mpc_solve_fused_supported_xbounds: 1 where the entry exists and both layouts are in their tables, else 0; needs
 * no device.  dqp_al_mpc_solve_fused_lds_bytes_xbounds: the launch's LDS -- that of dqp_al_mpc_solve_fused_lds_bytes at a
 * strided `bounds` plus 4 T n_state doubles (the state rows of lam and the staged state bounds) --, 0 where
 * _supported_xbounds is 0; at most 64 KB.  dqp_al_mpc_solve_fused_bytes_xbounds: the workspace size a caller passes, that
 * of dqp_al_mpc_solve_xbounds_bytes, so that one buffer serves both entries.
 * Return codes of dqp_al_mpc_solve_fused_xbounds: those of the `_xbounds` entries above in their order, then
 * DQP_ERR_BAD_ARG for al_iter outside 1 .. 256, newton_steps < 1 or n_prev < 0, DQP_OK with nothing touched for
 * nbatch == 0, DQP_ERR_BAD_ARG for a null buffer, and DQP_ERR_TOO_LARGE where _supported_xbounds is 0 (RexQuadrotor,
 * T > 32: dqp_al_mpc_solve_xbounds serves them).  `fail` is cleared by a memset in front of the launch (a memset node
 * under stream capture).  Only enqueues on `stream`.
 */
int dqp_al_mpc_solve_fused_supported_xbounds(const dqp_al_mpc_dims *dims, int model, const dqp_al_bounds *bounds,
                                             const dqp_al_bounds *xbounds);
size_t dqp_al_mpc_solve_fused_bytes_xbounds(const dqp_al_mpc_dims *dims);
size_t dqp_al_mpc_solve_fused_lds_bytes_xbounds(const dqp_al_mpc_dims *dims, int model, const dqp_al_bounds *bounds,
                                                const dqp_al_bounds *xbounds);
int dqp_al_mpc_solve_fused_xbounds(const dqp_al_mpc_dims *dims, int model, double dt, int32_t al_iter,
                                   int32_t newton_steps, const double *x_init, const double *u_init, const double *x0,
                                   const double *Qdiag, const double *q, const dqp_al_bounds *bounds,
                                   const dqp_al_bounds *xbounds, const double *lam_in, const double *rho_in,
                                   const double *prev_cost, const double *prev_lam, const double *prev_rho,
                                   int32_t n_prev, double *xu, double *hist_cost, double *hist_lam, double *hist_rho,
                                   double *res_norm, double *factor, double *status, int32_t *fail, void *workspace,
                                   void *stream);

/*
 * State bounds for a dynamics the CALLER linearised (additive at 303): dqp_al_banded_newton_step_jac_bounds plus
 * `xbounds` behind `bounds`, with the state box, the row order and lam's dqp_al_ncon_xbounds(dims) columns of the
 * `_xbounds` entries above.  Kernels: al_banded_newton_kernel<BoxBounds<Given<n, m>>, G, LF> at every pair of
 * DQP_BAND_SIZES (16 lanes; 8 where n_state + n_ctrl <= 8, by batch size or dqp_al_lane_group; the LDS-resident factor by
 * the rule of the twin) and of DQP_BAND_WIDE_SIZES (32 lanes).  `bounds` takes every layout of its table at the wide
 * pairs too.  `factor` has dqp_al_banded_jac_factor_bytes(dims) bytes and is applied by dqp_al_banded_solve(dims, 0, ...).
 * Return codes, in this order: DQP_ERR_BAD_ARG for a null dims, nbatch < 0, n_state / n_ctrl < 1, T < 2, a null `bounds` /
 * `xbounds` or one with strides outside its table; DQP_ERR_TOO_LARGE for a pair in neither list; DQP_OK with nothing
 * enqueued for nbatch == 0; DQP_ERR_BAD_ARG for a null buffer, the lower / upper of either box included (`info` may be
 * null).
 *
 * dqp_al_merit_xbounds: dqp_al_merit_bounds with the state rows -- the lane that sweeps knot t adds, for j < n_state,
 * lam[row] up + lam[row + n] lo + rho / 2 (max(up, 0)^2 + max(lo, 0)^2), up = x - x_upper, lo = x_lower - x,
 * row = T n + 2 T m + t 2 n + j, knot 0's rows included -- at any (n_state, n_ctrl): the sizes are run-time values of
 * that kernel.  The checks of dqp_al_merit_bounds plus the state box's layout (in front of the nbatch == 0 / ncand == 0
 * return) and its pointers (behind it).
 */
int dqp_al_banded_newton_step_jac_xbounds(const dqp_al_mpc_dims *dims, const double *xu, const double *x0,
                                          const double *Qdiag, const double *q, const double *lam, const double *rho,
                                          const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds,
                                          const double *x_next, const double *Jx, const double *Ju, double *update,
                                          void *factor, int32_t *info, void *stream);
int dqp_al_merit_xbounds(const dqp_al_mpc_dims *dims, int32_t ncand, const double *xu, const double *x_next,
                         const double *x0, const double *Qdiag, const double *q, const double *lam,
                         const double *rho, const dqp_al_bounds *bounds, const dqp_al_bounds *xbounds, double *merit,
                         void *stream);

/*
 * Per-sample, per-knot control bounds of the MPC QP (additive at 303).  dqp_mpc_assemble, dqp_mpc_qp_forward and
 * dqp_mpc_qp_forward_stepped read one vector of n_ctrl bounds for the whole batch and horizon.  Their `_bounds` twins take
 * a dqp_mpc_bounds -- the struct of the AL twins above -- in the position of the (u_lower, u_upper) pair, every other
 * argument unchanged, and read lower / upper [b * stride_b + t * stride_t + k] for sample b, knot t, control k.  With
 * m = n_ctrl, B = nbatch the accepted (stride_b, stride_t) are
 *
 *     (0, 0)        m doubles        the vector form: the twin launches exactly the kernels of the old entry point,
 *                                    which is itself the twin at (0, 0)
 *     (0, m)        (T, m)           per knot, the same for every sample
 *     (m, 0)        (B, m)           per sample, constant along the horizon
 *     (m, B m)      (T, B, m)        per sample and knot, time-major like C, c, F, f
 *     (T m, m)      (B, T, m)        per sample and knot, batch-major: the full layout of the AL twins, so one buffer
 *                                    serves both solver families
 *
 * Anything else, a null struct, or (at nbatch > 0) a null lower / upper is DQP_ERR_BAD_ARG; struct and strides are checked
 * in front of the nbatch == 0 return.  lower < upper is required of every pair and not checked: the interior-point
 * iteration has no interior at lower == upper.  Inequality rows keep their order [u - upper (T m, knot-major) ;
 * lower - u (T m)].  dqp_mpc_qp_supported, _workspace_bytes, _termination_bytes, _host_n_state and the stepped sizes do
 * not depend on the layout (the kernels read the bounds from the caller's arrays, nothing is staged), and
 * dqp_mpc_qp_backward reads no bounds: none of them has a twin.
 *
 * Kernels: the stage-wise forward kernels (16-lane, wide and host-only pairs; LDS-resident and streamed; linear,
 * registered-model and caller residual) have a strided instantiation next to the vector one, taken at non-zero strides
 * only; it loads a knot's pair with the knot's other vectors.  The null-space kernels and the assembly read the layout
 * in their one set-up pass over h.
 */
typedef dqp_al_bounds dqp_mpc_bounds;

int dqp_mpc_assemble_bounds(const dqp_mpc_dims *dims, const double *C, const double *c, const double *F,
                            const double *f, const double *x0, const dqp_mpc_bounds *bounds, double *Q, double *p,
                            double *G, double *h, double *A, double *b, void *stream);
int dqp_mpc_qp_forward_bounds(const dqp_mpc_dims *dims, const dqp_opts *opts, const double *C, const double *c,
                              const double *F, const double *f, const double *x0, const dqp_mpc_bounds *bounds,
                              double *tau, double *lam, double *nu, double *slack, int32_t *info, double *best_resid,
                              void *workspace, void *termination, void *stream);
int dqp_mpc_qp_forward_stepped_bounds(const dqp_mpc_dims *dims, const dqp_opts *opts, const double *C, const double *c,
                                      const double *F, const double *f, const double *x0, const dqp_mpc_bounds *bounds,
                                      const double *ext_ry, int32_t it_begin, int32_t it_end, double *tau, double *lam,
                                      double *nu, double *slack, int32_t *info, double *best_resid, void *workspace,
                                      void *termination, void *stream);

/*
 * The gradient-free SQP rounds of qp_wrapper.MPC.solve_nonlin for a registered device model (additive at 303;
 * csrc/dqp_mpc_sqp.hip).  Replaces, per round of qpth/qp_wrapper.py:348-414: linearize_dynamics (:481-515), single_qp,
 * line_search, the best-trajectory bookkeeping and the loop's two host tests.  The differentiable last step stays with
 * the caller.
 *
 * dqp_mpc_linearize: F_t = [df/dx, df/du](x_t, u_t), f_t = step(x_t, u_t) - F_t [x_t; u_t], t < T-1, of the model
 * dims->dyn_id (sizes as in dims, else DQP_ERR_BAD_ARG), in the layouts dqp_mpc_qp_forward reads: x (T,B,n), u (T,B,m) ->
 * F (T-1,B,n,nt), f (T-1,B,n).  One launch; forward-mode duals of the registry's templates, as dqp_dyn_jacobian.  Reads
 * neither has_bounds nor n_state_host.
 *
 * dqp_mpc_sqp_rounds enqueues rounds round_begin .. round_end-1 of the loop.  dims->dyn_id names the model, `opts` is what
 * dqp_mpc_qp_forward takes with dyn_dt the model's step (> 0); C (T,B,nt,nt), c (T,B,nt), x0 (B,n) and the bounds as for
 * dqp_mpc_qp_forward_bounds; decay, max_linesearch_iter as for dqp_mpc_line_search.  All state between calls lives in the
 * caller's buffers: x (T,B,n), u (T,B,m) the current trajectory (in/out), keep_x, keep_u, keep_cost (B) the best
 * trajectory seen per sample, and state, int32[4] = {done, rounds applied, 0, 0}.  A call with round_begin == 0 resets
 * `state` on the device (round 0 ignores what it finds there and leaves {done, 1, 0, 0}; an empty range from 0 leaves
 * zeros), and round 0 stores keep_* unconditionally.  One round:
 *   1. F, f <- the linearisation at (x, u);
 *   2. tau <- dqp_mpc_qp_forward_bounds (the model's true step in the equality residual);
 *   3. du = tau_u - u;
 *   4. x_new, u_new, cost_new <- dqp_mpc_line_search from x0;
 *   5. per sample: cost_new <= keep_cost + best_cost_eps (or round 0) -> keep_x, keep_u, keep_cost <- the new ones;
 *   6. x, u <- x_new, u_new;
 *   7. done |= |u_new - u|_F < eps over the whole batch (qp_wrapper.py:392); rounds applied += 1.
 * A round that starts with `done` set changes nothing in x, u, keep_* or state (its QP and line search run on the
 * previous round's F, f and write only the workspace): enqueueing every round in one call equals the reference's `break`.
 * The batch-wide sum of step 7 crosses workgroups at launch boundaries only and is added in index order (64 samples per
 * partial, then the partials): no atomics, the same bits from run to run.  Four launches per round on top of the QP's and
 * the line search's.  Only enqueues: no synchronisation, no allocation, no copy to the host (capturable).
 *
 * dqp_mpc_sqp_supported: 1 iff dims->dyn_id is a registered model of the sizes in dims, has_bounds is set,
 * n_state_host == 0, dqp_mpc_qp_supported(dims) == 1 and the line search serves the size (n_state <= 12, n_ctrl <= 8).
 * Needs no device.
 *
 * dqp_mpc_sqp_workspace_bytes, with B = nbatch, n = n_state, m = n_ctrl, nt = n + m and ev(x) = x rounded up to even --
 * every array starts on 16 bytes of a 16-byte aligned workspace -- (0 when unsupported, nbatch <= 0 or opts == NULL):
 *     8 * (ev((T-1) B n nt) + ev((T-1) B n)            F, f
 *          + ev(B T nt) + 4 B T m + ev(B T n)          tau, lam, slack, nu
 *          + 2 ev(B)                                   info (B,2) int32, best_resid
 *          + 2 ev(T B m) + ev(T B n)                   du, u_new, x_new
 *          + 2 ev(B) + ev(ceil(B / 64)))               alpha, cost_new, the partial sums
 *     + 16 * ceil(dqp_mpc_qp_workspace_bytes(dims) / 16) + 16 * ceil(dqp_mpc_qp_termination_bytes(dims, opts) / 16)
 *
 * Return codes: DQP_ERR_BAD_ARG for a null dims / opts / bounds, an unknown model or one whose sizes differ from dims,
 * has_bounds == 0, n_state_host != 0 and a bounds layout dqp_mpc_qp_forward_bounds refuses; DQP_ERR_TOO_LARGE where
 * dqp_mpc_sqp_supported is 0 otherwise; then nbatch == 0 returns DQP_OK with nothing enqueued; then DQP_ERR_BAD_ARG for a
 * null array, round_begin < 0, round_end < round_begin, max_linesearch_iter < 1 or dyn_dt <= 0.
 */
int dqp_mpc_linearize(const dqp_mpc_dims *dims, double dt, const double *x, const double *u,
                      double *F, double *f, void *stream);

int    dqp_mpc_sqp_supported(const dqp_mpc_dims *dims);
size_t dqp_mpc_sqp_workspace_bytes(const dqp_mpc_dims *dims, const dqp_opts *opts);
int    dqp_mpc_sqp_rounds(const dqp_mpc_dims *dims, const dqp_opts *opts, const double *C, const double *c,
                          const double *x0, const dqp_mpc_bounds *bounds, double decay,
                          int32_t max_linesearch_iter, double best_cost_eps, double eps,
                          int32_t round_begin, int32_t round_end, double *x, double *u,
                          double *keep_x, double *keep_u, double *keep_cost, int32_t *state,
                          void *workspace, void *stream);

/* ----------------------------------------------------------------- device dynamics registry */

/*
 * Robots and pendulum models the reference evaluates through per-robot torch extensions or Python
 * modules, available to callers (and inlined by the MPC / AL kernels) as device code:
 *   DQP_DYN_PENDULUM1L / CARTPOLE1L / CARTPOLE2L  deqmpc/my_envs/{pendulum1l,cartpole1l,cartpole2l}
 *       (CasADi RK4 step of the rigid-body model; state x = [q, qdot], n_state = 2 nq = 2 / 4 / 6,
 *       the control drives joint 0: deqmpc/my_envs/dynamics.py:26-63)
 *   DQP_DYN_PENDULUM_EULER   deqmpc/envs.py:5-47 PendulumDynamics (n_state 2, semi-implicit Euler)
 *   DQP_DYN_PENDULUM_DX      qpth/env_dx/pendulum.py:18-83 PendulumDx, simple=True, default
 *       parameters (n_state 3: cos th, sin th, thdot; control clamped to +-2)
 *   DQP_DYN_REXQUADROTOR     deqmpc/rex_quadrotor.py:7-129 RexQuadrotor_dynamics, default parameters
 *       (BASELINE config 4: n_state 12 = position, MRP attitude, body velocity, body rate;
 *       n_ctrl 4 motor commands; RK4)
 *   DQP_DYN_INTEGRATOR       deqmpc/envs.py:182-233 IntegratorDynamics, nx = 2, nu = 1 (the env of deqmpc/run.sh:
 *       n_state 2 = position, velocity; the control is the acceleration; semi-implicit Euler, default dt 0.1;
 *       the one linear model: df/dx = [[1, dt], [0, 1]], df/du = [[dt^2], [dt]])
 */
enum {
    DQP_DYN_PENDULUM1L = 1,
    DQP_DYN_CARTPOLE1L = 2,
    DQP_DYN_CARTPOLE2L = 3,
    DQP_DYN_PENDULUM_EULER = 4,
    DQP_DYN_PENDULUM_DX = 5,
    DQP_DYN_REXQUADROTOR = 6,
    DQP_DYN_INTEGRATOR = 7
};

/* n_state / n_ctrl of a registered model; DQP_ERR_BAD_ARG for an unknown id. */
int dqp_dyn_sizes(int id, int32_t *n_state, int32_t *n_ctrl);

/*
 * x_next = f(x, u) for n samples: x (n,n_state), u (n,n_ctrl), step dt.
 * Replaces: Dynamics.forward (deqmpc/my_envs/dynamics.py:26-63), PendulumDynamics.forward
 *           (deqmpc/envs.py:16-31), PendulumDx.forward (qpth/env_dx/pendulum.py:49-83), IntegratorDynamics.forward
 *           (deqmpc/envs.py:193-213).
 */
int dqp_dyn_step(int id, int32_t n, const double *x, const double *u, double dt, double *x_next,
                 void *stream);

/*
 * x_next and the Jacobians Jx (n,n_state,n_state) = d x_next_i / d x_j, Ju (n,n_state,n_ctrl).
 * Any output may be NULL.  Replaces: Dynamics.dynamics_derivatives / derivatives
 * (deqmpc/my_envs/dynamics.py:66-112,253-263), PendulumDynamics_jac (deqmpc/envs.py:68-82) -- the
 * `dx_jac(x, u) -> (x_next, (Jx, Ju))` closure the MPC layers call (qp_wrapper.py:497,
 * al_utils.py:212-262).
 */
int dqp_dyn_jacobian(int id, int32_t n, const double *x, const double *u, double dt, double *x_next,
                     double *Jx, double *Ju, void *stream);

/*
 * The reference extension's own interface (deqmpc/my_envs/cartpole1l/src/dynamics_cpu.cpp:8-56,
 * dynamics_gpu.cu kernels): q, qdot, tau (n,nq), per-sample step h (n); the six Jacobian blocks
 * are (n,nq,nq) with block[in i][out j], i.e. the raw CasADi buffers the reference's wrapper
 * concatenates and transposes (dynamics.py:99-112).  Robots 1-3 only.  Any block may be NULL.
 */
int dqp_dyn_forward_dynamics(int id, int32_t n, const double *q, const double *qdot, const double *tau,
                             const double *h, double *q_out, double *qdot_out, void *stream);
int dqp_dyn_forward_derivatives(int id, int32_t n, const double *q, const double *qdot,
                                const double *tau, const double *h, double *q_jac_q,
                                double *q_jac_qdot, double *q_jac_tau, double *qdot_jac_q,
                                double *qdot_jac_qdot, double *qdot_jac_tau, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-launch timing of the library's own kernels (bench.py's roofline figures, tools/).  Between
 * dqp_trace_begin and dqp_trace_end every kernel launch of this library is bracketed by a pair of HIP
 * events recorded on the launch stream; dqp_trace_end waits for them and returns one record per
 * launch, in launch order.  The one place the library owns anything: the event pool lives from begin to
 * end.  Not for use under stream capture.  Single host thread.
 */
typedef struct dqp_trace_record {
    char kernel[248];   /* demangled kernel name, truncated */
    float ms;           /* hipEventElapsedTime between the two events of this launch */
    int32_t reserved;
} dqp_trace_record;
int dqp_trace_begin(int32_t max_launches);      /* launches beyond max_launches are not recorded */
int dqp_trace_end(dqp_trace_record *out, int32_t capacity, int32_t *count);  /* out: HOST memory */

/* ------------------------------------------------------------------ network-side kernels (fp32)
 * The one exception to "all pointers fp64": the trajectory network of DEQ-MPC runs in single precision
 * (deqmpc/policies.py:191-430, DEQLayer), and so do these entries -- every `float *` below is a DEVICE pointer to
 * fp32, row-major, contiguous and 16-byte aligned (a misaligned pointer is DQP_ERR_BAD_ARG).  Scalars stay double /
 * int32_t.  They replace, between the three GEMMs of one DEQLayer iteration (policies.py:277-283), the LayerNorm, ReLU
 * and residual-add kernels, forward and backward, with one pass per stage (csrc/dqp_deq.hip):
 *
 *   stage A   y  = LN(relu ? max(a, 0) : a; gamma, beta, eps)        relu 0: inp_layer[1]; relu 1: lndeq1(reludeq1(.))
 *   stage B   z2 = LN(max(z1 + LN(xi + a2; gamma2, beta2, eps2), 0); gamma3, beta3, eps3)
 *                                                                    lndeq3(reludeq2(z1 + lndeq2(xi + fcdeq2(z1))))
 *
 * with LN of torch.nn.LayerNorm over the last axis: biased variance, rstd = 1 / sqrt(var + eps), two-pass statistics.
 * a, y, xi, a2, z1, z2 and their cotangents are (nrows, hdim); gamma*, beta* (hdim).  hdim is 32, 64, 128, 256 or 512
 * (hdim / 64 elements per lane, a row per wavefront; two rows per wavefront at 32).
 * stats: (nrows, 2) = mean, rstd of stage A; (nrows, 4) = mean2, rstd2, mean3, rstd3 of stage B -- written by the
 * forward, read by the backward, which recomputes everything else from the stage's inputs (nothing of size
 * (nrows, hdim) is kept).  The ReLU derivative is (input > 0).
 * Backward outputs: stage A da; stage B ds (the cotangent of xi AND of a2, one tensor) and dz1 (through the residual
 * only: a2's dependence on z1 is the caller's GEMM); dgamma*, dbeta* (hdim) are sums over the rows.  Any of them may be
 * NULL to skip it.
 * The row sums use no atomics: a workgroup owns a fixed set of consecutive rows, adds them in row order and leaves one
 * partial per workgroup in `partial`; a second kernel adds the partials in ascending order (fp64 accumulator, rounded
 * once).  The result depends only on
 * the inputs, nrows and hdim: bit-identical from run to run.  partial: dqp_deq_partial_bytes(dims) bytes of device
 * scratch =
 *     16 * hdim * ceil(U / (4 * max(2, ceil(U / 4096)))),     U = nrows (hdim >= 64) or ceil(nrows / 2) (hdim 32)
 * (at most 1024 partials of four hdim-vectors); needed when a dgamma / dbeta is asked for, else it may be NULL.
 * dqp_deq_supported: 1 for nrows >= 0 and one of the five hdim, else (and for NULL) 0; _partial_bytes is 0 there.
 * Both are host functions and need no device.
 * Return codes, decided on the host in front of any launch, in this order: DQP_ERR_BAD_ARG for a null `dims` or
 * nrows < 0; DQP_ERR_TOO_LARGE for another hdim; DQP_OK with nothing touched at nrows == 0; DQP_ERR_BAD_ARG for a null
 * (or misaligned) array.  Calls only enqueue on `stream` (one launch forward; backward one, plus the finish kernel
 * when a parameter gradient is asked for): no allocation, no synchronisation, hipGraph-capturable.
 */
typedef struct dqp_deq_dims {
    int32_t nrows;
    int32_t hdim;
} dqp_deq_dims;

int dqp_deq_supported(const dqp_deq_dims *dims);
size_t dqp_deq_partial_bytes(const dqp_deq_dims *dims);
int dqp_deq_ln_forward(const dqp_deq_dims *dims, const float *a, const float *gamma, const float *beta, double eps,
                       int32_t relu, float *y, float *stats, void *stream);
int dqp_deq_ln_backward(const dqp_deq_dims *dims, const float *a, const float *gamma, const float *stats, int32_t relu,
                        const float *dy, float *da, float *dgamma, float *dbeta, float *partial, void *stream);
int dqp_deq_res_forward(const dqp_deq_dims *dims, const float *xi, const float *a2, const float *z1,
                        const float *gamma2, const float *beta2, const float *gamma3, const float *beta3, double eps2,
                        double eps3, float *z2, float *stats, void *stream);
int dqp_deq_res_backward(const dqp_deq_dims *dims, const float *xi, const float *a2, const float *z1,
                         const float *gamma2, const float *beta2, const float *gamma3, const float *stats,
                         const float *dz2, float *ds, float *dz1, float *dgamma2, float *dbeta2, float *dgamma3,
                         float *dbeta3, float *partial, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DQP_H_ */
