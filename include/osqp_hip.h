/*
 * osqp_hip.h -- C ABI of libosqp_hip.so, the MI355X-native OSQP ADMM engine.
 *
 * Drop-in boundary: these are the entry points the reference's pybind11 layer
 * binds from the un-vendored osqp C core ("osqp_api_functions.h" / "osqp_api_types.h",
 * /root/reference/src/bindings.cpp.in:9-10).  Each declaration cites the call site it replaces.
 * The struct members are the ones the reference reads or writes through its bindings
 * (bindings.cpp.in:405-447 settings, :473-492 info, :64-105 solution, :41-48 CSC matrix).
 *
 * Plain pointers and sizes only: no torch / pybind / HIP types cross this boundary.
 * All functions return an osqp_error_type value (0 = OSQP_NO_ERROR) unless stated otherwise.
 * A solver handle is not thread-safe; distinct handles may be used from distinct threads
 * (bindings.cpp.in:196-201 releases the GIL around osqp_solve; multithread_test.py:38-53).
 */
#ifndef OSQP_HIP_H
#define OSQP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef int    OSQPInt;    /* OSQP_USE_LONG OFF  (reference CMakeLists.txt:9, interface.py:153) */
typedef double OSQPFloat;  /* OSQP_USE_FLOAT OFF (interface.py:152)                              */

#define OSQP_INFTY ((OSQPFloat)1e30)   /* bindings.cpp.in:340 */

/* bindings.cpp.in:343-346 */
enum osqp_linsys_solver_type { OSQP_UNKNOWN_SOLVER = 0, OSQP_DIRECT_SOLVER, OSQP_INDIRECT_SOLVER };

/* bindings.cpp.in:349-361 (same member order) */
enum osqp_status_type {
  OSQP_SOLVED = 1, OSQP_SOLVED_INACCURATE, OSQP_PRIMAL_INFEASIBLE, OSQP_PRIMAL_INFEASIBLE_INACCURATE,
  OSQP_DUAL_INFEASIBLE, OSQP_DUAL_INFEASIBLE_INACCURATE, OSQP_MAX_ITER_REACHED, OSQP_TIME_LIMIT_REACHED,
  OSQP_NON_CVX, OSQP_SIGINT, OSQP_UNSOLVED
};

/* bindings.cpp.in:364-375 (same member order) */
enum osqp_error_type {
  OSQP_NO_ERROR = 0, OSQP_DATA_VALIDATION_ERROR, OSQP_SETTINGS_VALIDATION_ERROR, OSQP_LINSYS_SOLVER_INIT_ERROR,
  OSQP_NONCVX_ERROR, OSQP_MEM_ALLOC_ERROR, OSQP_WORKSPACE_NOT_INIT_ERROR, OSQP_ALGEBRA_LOAD_ERROR,
  OSQP_CODEGEN_DEFINES_ERROR, OSQP_DATA_NOT_INITIALIZED, OSQP_FUNC_NOT_IMPLEMENTED
};

/* bindings.cpp.in:378-381 */
enum osqp_precond_type { OSQP_NO_PRECONDITIONER = 0, OSQP_DIAGONAL_PRECONDITIONER };

/* bindings.cpp.in:395-400 */
enum osqp_capabilities_type {
  OSQP_CAPABILITY_DIRECT_SOLVER = 0x01, OSQP_CAPABILITY_INDIRECT_SOLVER = 0x02, OSQP_CAPABILITY_CODEGEN = 0x04,
  OSQP_CAPABILITY_UPDATE_MATRICES = 0x08, OSQP_CAPABILITY_DERIVATIVES = 0x10
};

/* Compressed-sparse-column matrix, borrowed zero-copy from the caller (bindings.cpp.in:41-48). */
typedef struct {
  OSQPInt    m;      /* rows */
  OSQPInt    n;      /* columns */
  OSQPInt   *p;      /* column pointers (n+1) */
  OSQPInt   *i;      /* row indices (nzmax), sorted within a column (interface.py:232-235) */
  OSQPFloat *x;      /* values (nzmax) */
  OSQPInt    nzmax;  /* number of stored entries */
  OSQPInt    nz;     /* -1 for CSC (bindings.cpp.in:48) */
} OSQPCscMatrix;

/* The 29 fields bound at bindings.cpp.in:409-447, in that order. */
typedef struct {
  OSQPInt device;                         /* HIP device ordinal */
  enum osqp_linsys_solver_type linsys_solver;   /* only OSQP_INDIRECT_SOLVER is implemented */
  OSQPInt verbose;
  OSQPInt warm_starting;
  OSQPInt scaling;                        /* Ruiz iterations, 0 = off */
  OSQPInt polishing;                      /* polish by re-running the ADMM on the guessed active set (engine.cpp Engine::polish) */
  OSQPFloat rho;
  OSQPInt   rho_is_vec;
  OSQPFloat sigma;
  OSQPFloat alpha;
  OSQPInt   cg_max_iter;                  /* cap on PCG iterations per ADMM iteration (default 50) */
  OSQPInt   cg_tol_reduction;             /* first-chunk PCG tolerance = ||rhs||_inf / cg_tol_reduction */
  OSQPFloat cg_tol_fraction;              /* PCG tolerance = fraction * (scaled ADMM dual residual), non-increasing */
  enum osqp_precond_type cg_precond;
  OSQPInt   adaptive_rho;
  OSQPInt   adaptive_rho_interval;        /* 0 = automatic (2 * check_termination, or 50) */
  OSQPFloat adaptive_rho_fraction;        /* IGNORED (validated > 0 for API parity): the automatic interval (adaptive_rho_interval = 0) is 2 * check_termination, not a fraction of the setup time */
  OSQPFloat adaptive_rho_tolerance;
  OSQPInt   max_iter;
  OSQPFloat eps_abs;
  OSQPFloat eps_rel;
  OSQPFloat eps_prim_inf;
  OSQPFloat eps_dual_inf;
  OSQPInt   scaled_termination;
  OSQPInt   check_termination;            /* interval; 0 = only at max_iter */
  OSQPInt   check_dualgap;                /* termination additionally requires |duality gap| < eps_abs + eps_rel max(|obj|, |dual obj|); honoured by osqp_solve (small QPs
                                             then take the host-driven loop, not the one-launch kernel) and by every batch entry point, per problem on the
                                             device (record field duality_gap; the adjoint entries have no termination test and do not read it) */
  OSQPFloat time_limit;
  OSQPFloat delta;
  OSQPInt   polish_refine_iter;
} OSQPSettings;

/* bindings.cpp.in:473-492 */
typedef struct {
  char      status[32];
  OSQPInt   status_val;
  OSQPInt   status_polish;
  OSQPFloat obj_val;
  OSQPFloat dual_obj_val;
  OSQPFloat prim_res;
  OSQPFloat dual_res;
  OSQPFloat duality_gap;
  OSQPInt   iter;
  OSQPInt   rho_updates;
  OSQPFloat rho_estimate;
  OSQPFloat setup_time;
  OSQPFloat solve_time;
  OSQPFloat update_time;
  OSQPFloat polish_time;
  OSQPFloat run_time;
  OSQPFloat primdual_int;
  OSQPFloat rel_kkt_error;
} OSQPInfo;

/* bindings.cpp.in:64-105: host arrays owned by the solver, refreshed by osqp_solve */
typedef struct {
  OSQPFloat *x;               /* n */
  OSQPFloat *y;               /* m */
  OSQPFloat *prim_inf_cert;   /* m */
  OSQPFloat *dual_inf_cert;   /* n */
} OSQPSolution;

typedef struct OSQPWorkspace_ OSQPWorkspace;   /* opaque */

/* bindings.cpp.in:163-176 dereferences solver->settings / ->solution / ->info */
typedef struct {
  OSQPSettings  *settings;
  OSQPSolution  *solution;
  OSQPInfo      *info;
  OSQPWorkspace *work;
} OSQPSolver;

/* bindings.cpp.in:452-463 (codegen is out of scope: the struct exists so the binding compiles) */
typedef struct {
  OSQPInt embedded_mode, float_type, printing_enable, profiling_enable, interrupt_enable, derivatives_enable;
} OSQPCodegenDefines;

/* ---- core API ---- */
OSQPInt osqp_capabilities(void);                                        /* bindings.cpp.in:402 */
void    osqp_set_default_settings(OSQPSettings *settings);              /* bindings.cpp.in:449 */
const char *osqp_version(void);

/* bindings.cpp.in:153.  P: upper-triangular CSC (interface.py:221-222); A: CSC; l/u clamped to
   +-OSQP_INFTY by the caller (interface.py:237-238).  Inputs are copied; nothing is retained. */
OSQPInt osqp_setup(OSQPSolver **solverp, const OSQPCscMatrix *P, const OSQPFloat *q, const OSQPCscMatrix *A,
                   const OSQPFloat *l, const OSQPFloat *u, OSQPInt m, OSQPInt n, const OSQPSettings *settings);
OSQPInt osqp_solve(OSQPSolver *solver);                                 /* bindings.cpp.in:198 */
OSQPInt osqp_cleanup(OSQPSolver *solver);                               /* bindings.cpp.in:160 */
OSQPInt osqp_warm_start(OSQPSolver *solver, const OSQPFloat *x, const OSQPFloat *y);   /* :193, NULL-able */
OSQPInt osqp_cold_start(OSQPSolver *solver);
OSQPInt osqp_update_data_vec(OSQPSolver *solver, const OSQPFloat *q_new, const OSQPFloat *l_new,
                             const OSQPFloat *u_new);                   /* bindings.cpp.in:237, NULL-able */
/* bindings.cpp.in:280: *_new_idx == NULL means "all entries, in CSC order"; Px refers to the upper triangle */
OSQPInt osqp_update_data_mat(OSQPSolver *solver, const OSQPFloat *Px_new, const OSQPInt *Px_new_idx, OSQPInt P_new_n,
                             const OSQPFloat *Ax_new, const OSQPInt *Ax_new_idx, OSQPInt A_new_n);
OSQPInt osqp_update_settings(OSQPSolver *solver, const OSQPSettings *new_settings);    /* bindings.cpp.in:204 */
OSQPInt osqp_update_rho(OSQPSolver *solver, OSQPFloat rho_new);         /* bindings.cpp.in:213 */
void    osqp_get_dimensions(OSQPSolver *solver, OSQPInt *m, OSQPInt *n);   /* codegen/pywrapper/bindings.cpp.jinja:21 */

/* Adjoint derivatives of the last solution (bindings.cpp.in:283-319): by the batch kernel for a problem that fits its direct variant (see
   osqp_hip_batch_adjoint below), by the PCG route for every other handle (see osqp_hip_adjoint_last_record below for its contract and for the one
   kind of handle that returns OSQP_FUNC_NOT_IMPLEMENTED).  compute: needs a previous osqp_solve that ended OSQP_SOLVED on the
   current data (OSQP_DATA_NOT_INITIALIZED otherwise: every data update resets the status); dx (n) = dL/dx, dy (m) = dL/dy, either may be NULL (zero).
   It keeps the result in the handle.  get_mat: fills the x arrays of the
   caller's CSC structs, which carry the patterns of P's upper triangle and of A as given at setup (interface.py:558-564); get_vec: dq (n), dl, du (m).
   Both return OSQP_DATA_NOT_INITIALIZED before a successful compute.  An argument may be NULL (skipped).
   Codegen is out of scope: present so the reference binding links; returns OSQP_FUNC_NOT_IMPLEMENTED. */
OSQPInt osqp_adjoint_derivative_compute(OSQPSolver *solver, OSQPFloat *dx, OSQPFloat *dy);            /* :302 */
OSQPInt osqp_adjoint_derivative_get_mat(OSQPSolver *solver, OSQPCscMatrix *dP, OSQPCscMatrix *dA);    /* :310 */
OSQPInt osqp_adjoint_derivative_get_vec(OSQPSolver *solver, OSQPFloat *dq, OSQPFloat *dl, OSQPFloat *du);   /* :318 */
OSQPInt osqp_codegen(OSQPSolver *solver, const char *output_dir, const char *prefix, OSQPCodegenDefines *defines);   /* :322 */
void    osqp_set_default_codegen_defines(OSQPCodegenDefines *defines);  /* bindings.cpp.in:463 */

/* ---- extensions of this engine (no reference analogue) ---- */

/* Engine statistics of the last osqp_solve. */
typedef struct {
  double pcg_iters_total;     /* PCG iterations summed over all ADMM iterations           */
  double pcg_iters_max;       /* largest per-ADMM-iteration PCG count                     */
  double pcg_unconverged;     /* ADMM iterations whose PCG hit the budget                 */
  double kernel_launches;     /* kernels enqueued (graph nodes included)                  */
  double graph_launches;      /* hipGraphLaunch calls                                     */
  double gpu_solve_ms;        /* hipEvent time around the ADMM loop                       */
  double nnzA, nnzB;          /* stored entries of A (CSR) and B = [P+sigma I | A'] (CSR) */
  double pcg_fused;           /* 2: ONE launch per PCG iteration (k_slot1, the F1 form: banded A); 3: ONE launch per PCG iteration on the explicit reduced matrix
                                 (k_slotk, the K form: any sparsity of moderate fill); 1: two kernels (k_k2f, k_k1f); 0: three (k_k1, k_k2, k_kv) */
  double batch_direct_bw;     /* half bandwidth of the reduced KKT matrix under the engine's RCM ordering (batch / small-QP direct
                                 solve); -1 before the first batch or small solve, -2 if the pattern is too dense to analyse */
  double cg_cap_escalations;  /* times the last solve doubled its PCG iteration cap because most solves of a chunk stagnated at it */
  double windowed_blocks;     /* row blocks of A and B whose input-vector window is staged in LDS (16-bit local column indices) */
  double row_blocks;          /* row blocks of A and B in total */
  double slot_topups;         /* last solve: chunks whose string of slot launches ended before the chunk did (more launches followed) */
  double f1_replicas;         /* F1 form: replica vectors of the partial A' t (0: the form does not apply to this problem) */
  double woodbury_rows;       /* dense rows of A treated exactly in the preconditioner (0: plain Jacobi) */
  double woodbury_direct;     /* 1: that preconditioner is K^-1 for the current rho (the linear solves run without PCG iterations); 2: ... and the ADMM
                                 iteration runs as two launches (OSQPHipPolicy::woodbury_fused) */
  double preconditioner;      /* OSQP_HIP_PRECOND_*: what the PCG is preconditioned with right now (below) */
  double woodbury_factorisations, woodbury_factor_ms;   /* last solve: re-factorisations of the Woodbury system at rho updates, and their wall time */
  double reordered;           /* 1: the engine works on a permuted copy of the problem (OSQPHipPolicy::reorder) */
  double reorder_ms;          /* time setup spent looking for the permutation (0: not attempted) */
  double woodbury_cache_hits; /* last solve: rho updates served by an inverse this handle had computed for the same rho_bar before (validated by the
                                 numerical probe against the current matrices) -- woodbury_factorisations counts the others; woodbury_factor_ms covers both */
  double f1_far_columns;      /* F1 form with per-block mixing: far columns (spill slots) over all row blocks of A (0: every block fits its window) */
  double woodbury_dual_cols;  /* device-factorised Woodbury form in column space (OSQPHipPolicy::woodbury_dual): order of its dense system = dense columns (0: row space) */
  double woodbury_fused_iteration; /* 1: the column-space direct mode runs its ADMM iteration fused -- seven launches, the dense block of A streamed twice instead of four times (no KB / KA launch);
                                 2: ... with the block held dense (eight launches: the two passes are dense kernels without an index stream);
                                 3: ... and the short rows / columns by one thread each (k_wbf_rb, k_wbf_s2: seven launches) */
  double woodbury_one_launch; /* 1: the Woodbury direct mode of a few dense rows runs ONE launch per ADMM iteration (k_wbz; woodbury_direct = 2 and OSQPHipPolicy::woodbury_fused = 1) */
  double kform_nnz;           /* K form: stored entries of the explicit reduced matrix K = P + sigma I + A' diag(rho) A (0: the form is not in use) */
  double batch_wave_split;    /* last batch solve, as launched: -1 = workgroup-per-problem kernels only; >= 0 = the wave-per-problem kernel ran, with this
                                 many of the longest-expected problems on the workgroup kernel beside it (0: the wave kernel took them all -- no launch
                                 order yet, or a batch or device too small to split) */
} OSQPHipStats;
/* OSQPHipStats::preconditioner.  `cg_precond = OSQP_DIAGONAL_PRECONDITIONER` (bindings.cpp.in:426, the reference's only preconditioner) selects the
   Jacobi family: plain Jacobi M = diag(K), and -- this engine's addition, on by default, OSQPHipPolicy::woodbury / woodbury_large = 0 switch it
   off -- the same diagonal with the rows of A that hold more than 128 entries treated exactly through the Woodbury identity (1..128 such rows:
   r x r system inverted on the host; up to 16384 rows carrying most of A: formed and inverted on the device by this engine's own fp64
   matrix-core kernels, dense_hip.hip).  Which one a handle runs is reported here, never implied. */
enum { OSQP_HIP_PRECOND_NONE = 0, OSQP_HIP_PRECOND_JACOBI = 1, OSQP_HIP_PRECOND_JACOBI_WOODBURY = 2, OSQP_HIP_PRECOND_JACOBI_WOODBURY_DENSE = 3 };
OSQPInt osqp_hip_get_stats(OSQPSolver *solver, OSQPHipStats *out);

/* Re-launch one hot-path kernel `reps` times on the solver's stream with the solver's current device state and
   return its mean duration in milliseconds (hipEvent pair on that stream).  which: 0 = SpMV A (K1),
   1 = SpMV B (K2), 2 = PCG vector update (Kv), 3 = rhs kernel (KB), 4 = A x~ + z,y,x update (KA),
   5 = one whole PCG iteration (K1, K2, Kv in sequence; time per sequence) without the reductions of partials,
   6 = the same with them (what a solve executes); 7 / 8 / 9 = sequence 6 without K2 / K1 / Kv, so that (6) - (7) is
   K2's time INSIDE the sequence, i.e. with the caches in the state a solve leaves them (a same-kernel repeat keeps the
   matrix L2-resident and flatters the kernel).  10 = one FUSED PCG iteration (k_k2f, k_k1f: the default form), 11 / 12 = each
   of the two alone, 13 = the pair with the converged flag set (eager-launch cost of an early-exit pair).
   F1 form (one launch per PCG iteration; each of these times TWO consecutive launches, 0 when the form does not apply to the problem):
   14 = the F-only probe kernel without the scalar fold at the head of the launch, 15 = with it (fixed alpha, beta, no stopping test),
   16 = F launches of the slot kernel itself (phase record, scalars from the fold, a stopping test that never fires, record hand-over):
   what a launch costs inside a solve; 17 = KA of the F1 form (z~ = A x~, z / y / x update, slices of r_0 and rhs), 18 = the first launch of a chunk
   (those slices from the vectors in memory).
   Woodbury direct mode (0 when it is not on): 20 = one ADMM iteration of the two-launch form (k_wbx_y + k_wbx_x; `reps` iterations as one chunk, time per
   iteration), 21 = the kernels of M^-1 = K^-1 of the unfused form (k_wb_p1, k_wb_p2 / k_wb_gemv, k_wb_p3; column space: the five k_wbd_* launches),
   23 = one ADMM iteration of the fused column-space direct mode (seven launches: k_wbf_r, k_wbf_beta, k_wbf_g, k_wbd_gemv, k_wbf_t, k_wbf_x, k_wbf_s).
   Dense KKT mode (osqp_hip_dense_kkt; OSQP_FUNC_NOT_IMPLEMENTED unless the handle's record shows state 1): 24 = its hot path alone (k_dk_apply:
   u = K^-1 r_0, x~ = x_g + u), 25 = one ADMM iteration of the mode (KB, k_dk_apply, KA) as a solve runs it -- a captured chunk of `reps` (at most 1024)
   iterations replayed between the event pair, time per iteration; 25 moves the handle's iterates on.
   Otherwise the kernels run in a side-effect-free "probe" mode or on saved-and-restored state; solver state is unchanged. */
OSQPInt osqp_hip_time_kernel(OSQPSolver *solver, OSQPInt which, OSQPInt reps, double *mean_ms);

/* Batched solve of `nbatch` QPs that share this solver's P, A, scaling and settings and differ in q / l / u (BASELINE
   configs[4]; semantics of the reference's update-style batching, src/osqp/nn/torch.py:128-164, as ONE kernel launch:
   one workgroup per problem, iterates in LDS).  q: nbatch x n, l/u: nbatch x m, row-major, NULL = the solver's current
   vector for every problem.  x: nbatch x n, y: nbatch x m (in: warm start if warm != 0; out: solution, or the
   infeasibility certificate).  rec: nbatch x OSQP_HIP_BATCH_REC doubles {status_val, iter, obj_val, prim_res, dual_res, rho, rho_updates,
   pcg_iters, status_polish, polish_time, rho_estimate, duality_gap}.  duality_gap is 0 unless settings.check_dualgap is set: then a problem ends
   SOLVED (SOLVED_INACCURATE at max_iter) only if, besides the residual tests, |gap| < eps_abs + eps_rel max(|obj_val|, |dual_obj_val|) (x 10 on the
   approximate pass), with osqp_solve's definitions on the problem's own scaled data -- dual_obj_val = (-1/2 x'Px - sum_i support(l_i, u_i, y_i)) / c over
   the finite sides the sign of y_i selects, gap = obj_val - dual_obj_val --, and the field is the gap of the point the record describes (the ADMM
   point; the polished one where polish was accepted; NaN where x or y is a certificate or not finite): dual_obj_val = obj_val - duality_gap.  A
   batch with the setting does not take the wave-per-problem kernel (OSQPHipStats::batch_wave_split = -1), as with polishing.  With the `polishing` setting, every SOLVED problem of a directly-solved batch is polished inside
   the kernel (reduced KKT system of the guessed active set, regularised by `delta`, factorised in LDS, `polish_refine_iter` refinement
   steps: /root/reference/src/osqppurepy/_osqp.py:1710-1828); the PCG variants do not polish (status_polish = 0).  The linear system of each ADMM iteration is solved DIRECTLY (banded LDL' of the reduced KKT matrix in LDS under a
   bandwidth-reducing ordering; pcg_iters = 0, equality weight 1e3 as in the reference) when that band fits next to the iterates
   (<= 144 KB, permuted half bandwidth <= 56, <= 4096 stored entries per matrix), by PCG otherwise.  Returns OSQP_FUNC_NOT_IMPLEMENTED when a problem does not fit
   one workgroup's LDS at all (10n + 8m doubles > 64 KB): callers then loop osqp_update_data_vec + osqp_solve.  A repeated batch of the
   same size is launched in the order of the previous call's iteration counts, longest first (scheduling only; results do not depend on it). */
#define OSQP_HIP_BATCH_REC 12
OSQPInt osqp_hip_batch_solve(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *q, const OSQPFloat *l, const OSQPFloat *u,
                             OSQPFloat *x, OSQPFloat *y, OSQPFloat *rec, OSQPInt warm);
/* The same solve with EVERY array in device memory of this solver's device (e.g. torch ROCm tensors through data_ptr(); SURVEY 8f
 * rank 2: no PCIe round trip).  Asynchronous: the kernel is enqueued on `stream` (a hipStream_t; inputs must be ready on it and
 * the outputs are valid once it has drained -- the solver handle must not be used again before that); stream == NULL uses the
 * solver's own stream and waits for it.  l <= u is NOT validated on this path.  nbatch == 0 launches nothing and only answers whether the
 * problem fits the batch kernel (OSQP_NO_ERROR / OSQP_FUNC_NOT_IMPLEMENTED): ranks with an empty share of a sharded batch ask this way. */
OSQPInt osqp_hip_batch_solve_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *q_dev, const OSQPFloat *l_dev, const OSQPFloat *u_dev,
                                    OSQPFloat *x_dev, OSQPFloat *y_dev, OSQPFloat *rec_dev, OSQPInt warm_start, void *stream);

/* The same batch with PER-PROBLEM MATRIX VALUES: the reference's forward accepts a P_val / A_val per batch element and solves the elements concurrently, one
 * solver object each (/root/reference/src/osqp/nn/torch.py:128-157, 184-217).  Px: nbatch x nnz(P) (the upper triangle in the CSC order given at setup --
 * what osqp_update_data_mat takes as Px with Px_idx = NULL, bindings.cpp.in:240-281), Ax: nbatch x nnz(A) (CSC order); NULL = this solver's own values
 * for every problem.  Still ONE solve launch, one workgroup per problem: a launch in front of it assembles and equilibrates every problem's own matrices
 * (the Ruiz scaling of /root/reference/src/osqppurepy/_osqp.py:389-497 with the problem's own P, q, A -- an element is scaled exactly as a solver set up
 * with its data alone), the solve kernel then reads its problem's values; exact linear solves by the banded LDL' of the problem's own K (iteration
 * counts equal the oracle's per element).  The sparsity pattern, the settings and the launch-order history are the handle's.  _device: every array in
 * device memory, asynchronous on `stream` exactly like osqp_hip_batch_solve_device. */
OSQPInt osqp_hip_batch_solve_mat(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px, const OSQPFloat *Ax, const OSQPFloat *q, const OSQPFloat *l,
                                 const OSQPFloat *u, OSQPFloat *x, OSQPFloat *y, OSQPFloat *rec, OSQPInt warm);
OSQPInt osqp_hip_batch_solve_mat_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px_dev, const OSQPFloat *Ax_dev, const OSQPFloat *q_dev,
                                        const OSQPFloat *l_dev, const OSQPFloat *u_dev, OSQPFloat *x_dev, OSQPFloat *y_dev, OSQPFloat *rec_dev,
                                        OSQPInt warm_start, void *stream);

/* LOCKSTEP: the same batch -- QPs that share this handle's P, A, scaling and settings and differ in q / l / u -- at ANY size a handle can be set up for
 * (lockstep_hip.hip).  osqp_hip_batch_solve keeps one problem in one workgroup's LDS and declines above 10n + 8m doubles = 64 KB; here the ADMM / PCG
 * iteration of its PCG variants runs on block vectors, OSQP_HIP_LOCKSTEP_WIDTH problems at a time (a batch is processed in chunks of that width, the
 * last one ragged): lanes are problems, one pass over the matrix serves the whole chunk, every per-problem reduction is a lane-local sum.  Same
 * arguments, same conventions (NULL = the handle's own vector, warm != 0: x / y hold the unscaled warm start on entry, rec: nbatch x
 * OSQP_HIP_BATCH_REC) and the same per-problem rules as the PCG variants of osqp_hip_batch_solve: Jacobi-preconditioned CG on K_b = P + sigma I +
 * A' diag(rho_b) A stopped per problem at cg_tol_fraction x the scaled dual residual (non-increasing; relative before the first residual), equality
 * weight and adaptive rho per problem, termination / approximate statuses at max_iter / infeasibility certificates in x, y / OSQP_NON_CVX on
 * non-finite residuals decided per problem on the device every check_termination / adaptive_rho_interval iterations; time_limit ends a chunk with
 * OSQP_TIME_LIMIT_REACHED for its unfinished problems.  check_dualgap is honoured per problem (the record's duality_gap, as on osqp_hip_batch_solve: one more launch, k_ls_supp, in front of
 * every termination check, none without the setting; after an accepted polish the field is the polished point's gap); per-problem matrices: osqp_hip_batch_solve_lockstep_mat below.
 * POLISH: with settings.polishing every problem of a chunk that ends OSQP_SOLVED is polished before the chunk is written out, all of them at once, by the
 * recurrence osqp_solve's polish runs on the PCG path: the active rows guessed from the ADMM (z, y) (equality rows always), the reduced KKT system solved
 * by steps of this route's own iteration with alpha = 1 and rho = 1 / max(delta, OSQP_HIP_POLISH_DELTA_FLOOR) on the active rows, the others free, the
 * inner systems to OSQP_HIP_POLISH_PCG_TOL -- at least 1 + polish_refine_iter steps, at most 30, until a problem's reduced residuals stop halving --,
 * then z = A x and the normal-cone projection against the problem's own bounds.  A problem keeps the polished point if it improves the ADMM point's
 * residuals by the reference's rule: record fields obj / prim_res / dual_res are then the polished point's and status_polish = 1; otherwise its ADMM x, y
 * come back bit for bit and status_polish = -1.  Field polish seconds is the chunk's polish wall time for every problem that was attempted.  Status,
 * iter, rho, rho_updates, pcg_iters and rho_estimate stay the ADMM's (polish's PCG iterations are not added).  A problem that did not end OSQP_SOLVED
 * keeps status_polish = 0 and its x, y / certificate untouched, and so does every problem of a chunk whose time_limit had passed when its ADMM loop ended.
 * With polishing = 0 (the default) the route issues exactly the launches it issues without this paragraph.  INDEPENDENCE below covers the polish.
 * INDEPENDENCE: no quantity of one problem enters another problem's arithmetic and no summation order depends on a chunk's fill -- a problem's x, y
 * and record are bit-identical whatever else is in the batch and wherever in it the problem sits.
 * A handle that works on a permuted copy (OSQPHipStats::reordered) is served: the arrays keep the caller's numbering.  The handle's own iterates,
 * solution, info and launch history are not touched: an osqp_solve after the call gives the bits it would have given without it.
 * Returns OSQP_FUNC_NOT_IMPLEMENTED for a handle whose PCG runs a Woodbury-corrected preconditioner (OSQPHipStats::woodbury_rows > 0) and in the host
 * simulator.  l <= u is validated on the host-pointer path only.
 * _device: every array in device memory of this solver's device; the work goes on `stream` (NULL: the solver's own) after the solver's own stream has
 * been waited for.  Unlike osqp_hip_batch_solve_device the call RETURNS WHEN THE RESULTS ARE THERE: the host reads a few status words from `stream`
 * at every termination check.  nbatch == 0 launches nothing and answers whether the route applies.
 * osqp_hip_lockstep_last_record: what the last lockstep call of the handle did, OSQP_HIP_LOCKSTEP_LAST_REC doubles {chunks, chunk width, ADMM
 * iterations of the slowest problem, PCG iterations summed over the problems, kernel launches, GPU ms, workspace bytes, reserved}; all zero before
 * the first call: the ADMM part only.
 * osqp_hip_lockstep_polish_last_record: the polish part of the same call, OSQP_HIP_LOCKSTEP_POLISH_LAST_REC doubles {problems attempted, accepted,
 * rejected, recurrence steps of the slowest problem, PCG iterations summed over the problems, kernel launches, GPU ms, polish workspace bytes}; all
 * zero before the first call and after a call with polishing = 0. */
#define OSQP_HIP_LOCKSTEP_WIDTH 64
#define OSQP_HIP_LOCKSTEP_LAST_REC 8
#define OSQP_HIP_LOCKSTEP_POLISH_LAST_REC 8
OSQPInt osqp_hip_batch_solve_lockstep(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *q, const OSQPFloat *l, const OSQPFloat *u,
                                      OSQPFloat *x, OSQPFloat *y, OSQPFloat *rec, OSQPInt warm);
OSQPInt osqp_hip_batch_solve_lockstep_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *q_dev, const OSQPFloat *l_dev, const OSQPFloat *u_dev,
                                             OSQPFloat *x_dev, OSQPFloat *y_dev, OSQPFloat *rec_dev, OSQPInt warm_start, void *stream);
OSQPInt osqp_hip_lockstep_last_record(OSQPSolver *solver, OSQPFloat *rec);
OSQPInt osqp_hip_lockstep_polish_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* LOCKSTEP WITH PER-PROBLEM MATRICES: the lockstep route for a batch in which every problem has its own values of P and A on the handle's sparsity pattern
 * (the reference's forward with a P_val / A_val per batch element), at any size -- what osqp_hip_batch_solve_mat serves only while a problem fits one
 * workgroup's LDS.  Px is nbatch x nnz(triu P), Ax nbatch x nnz(A), both in the CSC order given at setup (the layout of osqp_hip_batch_solve_mat); either
 * may be NULL: the handle's own raw values for every problem.  Everything else -- q / l / u / x / y / rec / warm, the nbatch == 0 query, the stream
 * semantics, the OSQP_HIP_BATCH_REC record, per-problem termination, statuses, certificates, time_limit -- is osqp_hip_batch_solve_lockstep[_device]'s.
 * SCALING: every problem is assembled and equilibrated with its own P_b, q_b, A_b exactly as a solver set up with that data alone: settings.scaling
 * iterations of the reference's Ruiz rule with its scaling limits, sigma added after the equilibration.  The problem's values travel problem-minor in a
 * matrix block of 64 x (nnz(A) + nnz([P | A']) + 2n + 2m) doubles, allocated by the first call and freed with the handle; a chunk's assembly and
 * equilibration are 5 + 4 x settings.scaling launches in front of its transposes in.
 * INDEPENDENCE as above, a problem's matrices being part of the problem.  A reordered handle is served.  The handle's own matrices, scaling, iterates,
 * graphs and history are not touched.
 * POLISH as above: with settings.polishing every problem of a chunk that ends OSQP_SOLVED is polished on its OWN P_b, A_b under its own D_b, E_b, c_b --
 * the active rows are guessed in the problem's own scaled space, the recurrence runs on the chunk's matrix block, the accept test uses the problem's own
 * cost scale: what osqp_solve's polish does on a handle set up with that problem alone.  Record fields 8 and 9, the rejection rule, the time_limit rule
 * and osqp_hip_lockstep_polish_last_record (filled by these calls too, the polish work block's bytes included) are the shared entry's.  With
 * polishing = 0 record fields 8 and 9 stay 0 and the call issues exactly the launches it issues without this paragraph.
 * Returns OSQP_FUNC_NOT_IMPLEMENTED for whatever osqp_hip_batch_solve_lockstep declines, for a handle without device-side assembly, and for a handle whose
 * stored upper triangle of P holds a repeated (j, j) entry (the single-handle assembly sums those; this route has one writer per entry).
 * OUT OF SCOPE: the direct (Woodbury) route, multi-rank sharding of this entry, repeated diagonal entries of P.  (The backward pass with per-problem
 * matrices: osqp_hip_batch_adjoint_lockstep_mat below; it does not polish.)
 * osqp_hip_lockstep_mat_last_record: OSQP_HIP_LOCKSTEP_MAT_LAST_REC doubles {chunks, chunk width, ADMM iterations of the slowest problem, PCG iterations
 * summed, kernel launches and GPU ms of the call -- assembly and equilibration included, polish apart (its launches, PCG iterations and GPU ms are
 * osqp_hip_lockstep_polish_last_record's) --, bytes of the matrix block, GPU ms spent in assembly + equilibration}; all zero before the first call.
 * osqp_hip_lockstep_last_record is written as by any lockstep call.
 * osqp_hip_lockstep_mat_scaling: D (n), E (m) and c of problem b of the LAST chunk the last such call processed, numbered as osqp_hip_get_scaling numbers
 * the handle's -- so that the per-problem equilibration can be checked directly.  OSQP_DATA_NOT_INITIALIZED before the first call or for b outside
 * that chunk -- and after a call of osqp_hip_batch_adjoint_lockstep_mat[_device], which overwrites the matrix block, until the next forward call. */
#define OSQP_HIP_LOCKSTEP_MAT_LAST_REC 8
OSQPInt osqp_hip_batch_solve_lockstep_mat(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px, const OSQPFloat *Ax, const OSQPFloat *q, const OSQPFloat *l,
                                          const OSQPFloat *u, OSQPFloat *x, OSQPFloat *y, OSQPFloat *rec, OSQPInt warm);
OSQPInt osqp_hip_batch_solve_lockstep_mat_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px_dev, const OSQPFloat *Ax_dev, const OSQPFloat *q_dev,
                                                 const OSQPFloat *l_dev, const OSQPFloat *u_dev, OSQPFloat *x_dev, OSQPFloat *y_dev, OSQPFloat *rec_dev,
                                                 OSQPInt warm_start, void *stream);
OSQPInt osqp_hip_lockstep_mat_last_record(OSQPSolver *solver, OSQPFloat *rec);
OSQPInt osqp_hip_lockstep_mat_scaling(OSQPSolver *solver, OSQPInt b, OSQPFloat *D, OSQPFloat *E, OSQPFloat *c);
/* LOCKSTEP DIRECT: the lockstep route for the handles it declines -- a Woodbury-corrected handle (OSQPHipStats::woodbury_rows = r > 0) in the small mode
 * (r <= 128) whose K0 = P + sigma I + A_S' rho A_S setup found structurally DIAGONAL: P diagonal, every row of A either long (one of the r dense rows A_L)
 * or with at most one entry, no long row storing a (row, column) twice -- the factor-model portfolio QP.  Then K_b = D0_b + A_L' rho_L,b A_L and the
 * Woodbury formula is the linear solve itself, per problem and without PCG: S_b = diag(1 / rho_L,b) + A_L D0_b^-1 A_L' (r x r, SPD) is formed and
 * inverted on the device at the start and again for exactly the problems whose rho_bar has changed; an ADMM iteration is a fixed sequence of five
 * launches, the host enqueues check_termination iterations back to back and reads the decision words once per check.  Arguments, checks, the nbatch ==
 * 0 query, stream semantics, the OSQP_HIP_BATCH_REC record (pcg_iters = 0), per-problem termination / statuses / certificates / time_limit and the
 * INDEPENDENCE guarantee are those of osqp_hip_batch_solve_lockstep[_device]; a pivot of S_b that is not positive ends that problem with OSQP_NON_CVX.
 * ADAPTIVE RHO is per problem too, but NOT by the batch family's rule (the reference's factor test against adaptive_rho_tolerance): this route applies the
 * rule of osqp_solve on this handle -- the tolerance on the policy's square-root scale (OSQPHipPolicy::rho_tol_exp / OSQP_HIP_RHO_TOL_EXP; the literal
 * value for an LP) and the persistence test (rho_persist / OSQP_HIP_RHO_PERSIST) -- so an element takes the iterations, status and iterate that
 * osqp_update_data_vec + osqp_solve give from the same settings.rho (a loop over one handle starts each solve from the rho the previous one left).  The
 * duality-gap test of check_dualgap as on the PCG route; per-problem matrices: osqp_hip_batch_solve_lockstep_direct_mat below.  The decision is the structural one taken at setup, whatever became of the single handle's direct
 * mode since.
 * POLISH as on osqp_hip_batch_solve_lockstep (settings.polishing, delta, polish_refine_iter): every problem of a chunk that ends OSQP_SOLVED is polished
 * between the ADMM loop and the transposes out by the same recurrence, with the Woodbury solve in place of the PCG -- rho_bar = 1 / delta on the
 * guessed-active rows, RHO_MIN on the others (inactive dense rows included), so S_b is formed and inverted once more per attempted problem and at no
 * step; these inversions are not counted in the direct record.  Record fields 8 and 9, the rejection rule (a rejected problem keeps its ADMM x, y and
 * fields bit for bit), the time_limit rule (tested against the host's clock when the chunk's ADMM loop ends) and the polish work block are the shared
 * paragraph's; osqp_hip_lockstep_polish_last_record is filled by a polishing direct call too, with 0 for the PCG iterations.  With polishing = 0 record
 * fields 8 and 9 stay 0, the call issues exactly the launches it issues without this paragraph and leaves the polish record as it was -- except that
 * the first such call after a polishing direct call zeroes it (the record is the last call's that could polish).  A polished point's dual residual is
 * bounded by the recurrence's y step, which multiplies a rounding error by rho_bar = 1 / delta: about 1e-9 relative at delta = 1e-6.
 * Returns OSQP_FUNC_NOT_IMPLEMENTED for every other handle: no Woodbury correction, the large mode (r > 128: the lasso), a K0 that is not
 * diagonal, the host simulator -- and a handle that works on a permuted copy (OSQPHipStats::reordered): this route DECLINES it rather than gather
 * through the permutations.  The handle's own iterates, solution, info and launch history are not touched.
 * osqp_hip_lockstep_direct_last_record: OSQP_HIP_LOCKSTEP_DIRECT_LAST_REC doubles {chunks, chunk width, ADMM iterations of the slowest problem,
 * inversions of S summed over the problems, kernel launches, GPU ms, workspace bytes, seconds of the call's chunks}; all zero before the first call.
 * The inversions, launches and GPU ms are the ADMM part's: polish's are osqp_hip_lockstep_polish_last_record's. */
#define OSQP_HIP_LOCKSTEP_DIRECT_LAST_REC 8
OSQPInt osqp_hip_batch_solve_lockstep_direct(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *q, const OSQPFloat *l, const OSQPFloat *u,
                                             OSQPFloat *x, OSQPFloat *y, OSQPFloat *rec, OSQPInt warm);
OSQPInt osqp_hip_batch_solve_lockstep_direct_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *q_dev, const OSQPFloat *l_dev, const OSQPFloat *u_dev,
                                                    OSQPFloat *x_dev, OSQPFloat *y_dev, OSQPFloat *rec_dev, OSQPInt warm_start, void *stream);
OSQPInt osqp_hip_lockstep_direct_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* LOCKSTEP DIRECT WITH PER-PROBLEM MATRICES -- osqp_hip_batch_solve_lockstep_direct for a batch whose elements have their own values of P and A on the handle's
 * sparsity pattern (a factor model per day or per sample: the reference's 2-D P_val / A_val).  Px ([nbatch][nnz of the upper triangle of P]) and Ax
 * ([nbatch][nnz(A)]) are in the CSC order given at setup, as osqp_hip_batch_solve_lockstep_mat takes them; either may be NULL: that side takes the handle's
 * CURRENT values (osqp_update_data_mat included) for every problem.  Problem b is solved as a handle set up with (P_b, q_b, A_b, l_b, u_b) alone would solve
 * it under this handle's settings: its own Ruiz equilibration D_b, E_b, c_b (settings.scaling iterations, on the device, per lane), its own D0_b, S_b and
 * S_b^-1, the direct route's rho rule with this handle's tolerance.  The other arguments, the nbatch == 0 query, stream semantics, the record per problem,
 * statuses / certificates (in the problem's own units) / time_limit and the INDEPENDENCE guarantee are those of osqp_hip_batch_solve_lockstep_direct[_device].
 * POLISH as on osqp_hip_batch_solve_lockstep_direct, each problem on its OWN P_b, A_b, dense rows and S_b under its own D_b, E_b, c_b (what osqp_solve's
 * polish does on a handle set up with that problem alone).  The backward pass with per-problem matrices is osqp_hip_batch_adjoint_lockstep_direct_mat below.  The handle is only read: its matrices, scaling, dense rows, S, iterates, settings and
 * launch history are not touched.  Returns OSQP_FUNC_NOT_IMPLEMENTED unless osqp_hip_batch_solve_lockstep_direct serves the handle AND the chunk's
 * assembly does (device assembly, no repeated (j, j) entry in the stored triangle of P); in the host simulator always.
 * Device memory: 512 (nnz(A) + nnz(B) + 2 n + 2 m + n r + nnz of the view) bytes for one chunk, allocated by the first such call (22 MB of dense rows at
 * n = 2020, r = 21; 139 MB at n = 2127, r = 128).
 * osqp_hip_lockstep_direct_mat_last_record: OSQP_HIP_LOCKSTEP_DIRECT_MAT_LAST_REC doubles {chunks, chunk width, ADMM iterations of the slowest problem,
 * inversions of S summed over the problems, kernel launches, GPU ms, bytes of that block, GPU ms of the assembly + equilibration + the fill of the dense
 * rows (part of the GPU ms)}; all zero before the first such call.  Such a call also updates osqp_hip_lockstep_direct_last_record. */
#define OSQP_HIP_LOCKSTEP_DIRECT_MAT_LAST_REC 8
OSQPInt osqp_hip_batch_solve_lockstep_direct_mat(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px, const OSQPFloat *Ax, const OSQPFloat *q, const OSQPFloat *l,
                                                 const OSQPFloat *u, OSQPFloat *x, OSQPFloat *y, OSQPFloat *rec, OSQPInt warm);
OSQPInt osqp_hip_batch_solve_lockstep_direct_mat_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px_dev, const OSQPFloat *Ax_dev, const OSQPFloat *q_dev,
                                                        const OSQPFloat *l_dev, const OSQPFloat *u_dev, OSQPFloat *x_dev, OSQPFloat *y_dev, OSQPFloat *rec_dev,
                                                        OSQPInt warm_start, void *stream);
OSQPInt osqp_hip_lockstep_direct_mat_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* ADJOINT DERIVATIVES ON THE LOCKSTEP ROUTE -- the backward pass of osqp_hip_batch_solve_lockstep: the quantities osqp_hip_batch_adjoint (below) defines,
 * for a batch that shares this handle's P and A, at any size, OSQP_HIP_LOCKSTEP_WIDTH problems at a time on block vectors.  Per problem: the rows are
 * classified by the rule given there (caller's units, z = A x on the x passed in; bounds clamped to +-OSQP_INFTY), and the adjoint system is solved by
 * the recurrence the single-handle PCG route runs (osqp_adjoint_derivative_compute below): the route's own ADMM iteration with alpha = 1, a fixed
 * rho = 1 / delta_eff on the active rows (delta_eff = max(delta, OSQPHipPolicy::polish_delta_floor)), the other rows free, from a zero start, the PCG
 * driven to polish_pcg_tol; a problem ends after at least 1 + polish_refine_iter steps when its error is below 1e-13 or two steps in a row gained
 * less than 10 %, at 60 steps at the latest, and is frozen from then on.  The result is unscaled and its residual max |g - K_a r| / max |g| is taken
 * on the UNREGULARISED system in the caller's units.  x, dx: nbatch x n; y, dy: nbatch x m (dy NULL = 0); l, u: nbatch x m, NULL = the handle's own.
 * Outputs as for osqp_hip_batch_adjoint, any of them NULL (skipped); dP / dA in the caller's CSC order (dP: the stored upper triangle).
 * arec: nbatch x OSQP_HIP_ADJOINT_REC doubles {status, active rows, residual, recurrence steps}; status 0: residual < OSQP_HIP_ADJOINT_TOL; 2: more active
 * rows than variables (nothing is iterated: steps = 0, residual = inf, outputs zero); 3: residual at or above the threshold (dependent active rows).
 * The outputs of a problem with a nonzero status are written and hold its last iterate; the other problems are untouched by it.  INDEPENDENCE as on
 * the forward route: a problem's outputs and record are bit-identical whatever else is in the batch and wherever in it the problem sits.
 * A reordered handle is served in the caller's numbering.  The handle's iterates, rho, info, solution, launch graphs and history are not touched, nor
 * are the forward route's workspace and record: the work block is this route's own (allocated by the first call, freed with the handle).
 * Per-problem matrices: osqp_hip_batch_adjoint_lockstep_mat below.  Returns OSQP_FUNC_NOT_IMPLEMENTED on a handle with a Woodbury-corrected preconditioner and in the host simulator.
 * _device: stream semantics of osqp_hip_batch_solve_lockstep_device -- the call returns when the results are there; nbatch == 0 answers applicability.
 * osqp_hip_lockstep_adjoint_last_record: OSQP_HIP_LOCKSTEP_ADJOINT_LAST_REC doubles {chunks, chunk width, recurrence steps of the slowest problem, PCG
 * iterations summed over the problems, kernel launches, GPU ms, workspace bytes, reserved}; all zero before the first call. */
#define OSQP_HIP_LOCKSTEP_ADJOINT_LAST_REC 8
OSQPInt osqp_hip_batch_adjoint_lockstep(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *l, const OSQPFloat *u, const OSQPFloat *x, const OSQPFloat *y,
                                        const OSQPFloat *dx, const OSQPFloat *dy, OSQPFloat *dP, OSQPFloat *dq, OSQPFloat *dA, OSQPFloat *dl, OSQPFloat *du,
                                        OSQPFloat *arec);
OSQPInt osqp_hip_batch_adjoint_lockstep_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *l_dev, const OSQPFloat *u_dev, const OSQPFloat *x_dev,
                                               const OSQPFloat *y_dev, const OSQPFloat *dx_dev, const OSQPFloat *dy_dev, OSQPFloat *dP_dev, OSQPFloat *dq_dev,
                                               OSQPFloat *dA_dev, OSQPFloat *dl_dev, OSQPFloat *du_dev, OSQPFloat *arec_dev, void *stream);
OSQPInt osqp_hip_lockstep_adjoint_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* ADJOINT DERIVATIVES ON THE LOCKSTEP ROUTE WITH PER-PROBLEM MATRICES -- the backward pass of osqp_hip_batch_solve_lockstep_mat: problem b's adjoint system
 * is solved on its own P_b, A_b, scaled by its own D_b, E_b, c_b.  Px is nbatch x nnz(triu P), Ax nbatch x nnz(A), in the CSC order given at setup; either
 * may be NULL: the handle's own raw values for every problem (as on the forward entry).  Every other argument, the OSQP_HIP_ADJOINT_REC record, the
 * statuses 0 / 2 / 3, the nbatch == 0 query, the stream semantics and INDEPENDENCE (a problem's matrices being part of the problem) are
 * osqp_hip_batch_adjoint_lockstep[_device]'s; dP / dA are per problem in the caller's CSC order.  A chunk's matrices are assembled and equilibrated as
 * on the forward entry (5 + 4 x settings.scaling launches in front of its transposes in), with the handle's q for every problem: the adjoint does not
 * depend on the cost scale c in exact arithmetic.  A reordered handle is served.
 * MATRIX BLOCK: the forward entry's, allocated by whichever of the two entries is called first.  A call here overwrites it, so
 * osqp_hip_lockstep_mat_scaling answers OSQP_DATA_NOT_INITIALIZED from then until the next forward call; the forward entry's results do not depend on
 * calls made here in between.  The handle's own matrices, scaling, iterates, graphs and history are not touched.
 * Returns OSQP_FUNC_NOT_IMPLEMENTED unless both osqp_hip_batch_adjoint_lockstep and osqp_hip_batch_solve_lockstep_mat serve the handle: a Woodbury
 * handle, the host simulator, a handle without device-side assembly, a repeated (j, j) entry in the stored upper triangle of P.
 * OUT OF SCOPE: multi-rank sharding of this entry.  (The direct (Woodbury) route: osqp_hip_batch_adjoint_lockstep_direct_mat below.)
 * osqp_hip_lockstep_mat_adjoint_last_record: OSQP_HIP_LOCKSTEP_MAT_ADJOINT_LAST_REC doubles {chunks, chunk width, recurrence steps of the slowest
 * problem, PCG iterations summed over the problems, kernel launches of the whole call, GPU ms of the whole call, bytes of the matrix block, GPU ms spent
 * in assembly + equilibration}; all zero before the first call.  osqp_hip_lockstep_adjoint_last_record is written as by any lockstep adjoint call. */
#define OSQP_HIP_LOCKSTEP_MAT_ADJOINT_LAST_REC 8
OSQPInt osqp_hip_batch_adjoint_lockstep_mat(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px, const OSQPFloat *Ax, const OSQPFloat *l, const OSQPFloat *u,
                                            const OSQPFloat *x, const OSQPFloat *y, const OSQPFloat *dx, const OSQPFloat *dy, OSQPFloat *dP, OSQPFloat *dq,
                                            OSQPFloat *dA, OSQPFloat *dl, OSQPFloat *du, OSQPFloat *arec);
OSQPInt osqp_hip_batch_adjoint_lockstep_mat_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px_dev, const OSQPFloat *Ax_dev, const OSQPFloat *l_dev,
                                                   const OSQPFloat *u_dev, const OSQPFloat *x_dev, const OSQPFloat *y_dev, const OSQPFloat *dx_dev,
                                                   const OSQPFloat *dy_dev, OSQPFloat *dP_dev, OSQPFloat *dq_dev, OSQPFloat *dA_dev, OSQPFloat *dl_dev,
                                                   OSQPFloat *du_dev, OSQPFloat *arec_dev, void *stream);
OSQPInt osqp_hip_lockstep_mat_adjoint_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* ADJOINT DERIVATIVES ON THE DIRECT LOCKSTEP ROUTE -- the backward pass of osqp_hip_batch_solve_lockstep_direct, on exactly the handles that call accepts
 * (OSQP_FUNC_NOT_IMPLEMENTED for every other one: no Woodbury correction, r > 128, a K0 that is not diagonal, a reordered handle, the host simulator).
 * Arguments, the classification, the recurrence and its ending rule, the unscaling, the residual of the unregularised system, the outputs (dA at every
 * stored entry, the dense rows' included), arec, the statuses 0 / 2 / 3, INDEPENDENCE, the stream semantics and the nbatch == 0 query are those of
 * osqp_hip_batch_adjoint_lockstep[_device] above.  What differs is the linear solve inside a step: the Woodbury formula of the forward route per problem
 * instead of a PCG.  rho is fixed throughout the recurrence, so S_b is formed and inverted ONCE per problem (an inactive dense row has rho_min, i.e.
 * 1e6 on S_b's diagonal); a step is a fixed sequence of launches followed by one read of the decision words.  A pivot of S_b that is not positive and
 * finite leaves that problem's iterates NaN: it ends with status 3 and no other problem reads it.  The work block and the host entry's scratch are
 * this route's own (allocated by the first call, freed with the handle); the handle's solve state, the forward route's workspace and record are not written.
 * osqp_hip_lockstep_direct_adjoint_last_record: OSQP_HIP_LOCKSTEP_DIRECT_ADJOINT_LAST_REC doubles {chunks, chunk width, recurrence steps of the slowest
 * problem, inversions of S summed over the problems, kernel launches, GPU ms, workspace bytes, reserved}; all zero before the first call. */
#define OSQP_HIP_LOCKSTEP_DIRECT_ADJOINT_LAST_REC 8
OSQPInt osqp_hip_batch_adjoint_lockstep_direct(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *l, const OSQPFloat *u, const OSQPFloat *x, const OSQPFloat *y,
                                               const OSQPFloat *dx, const OSQPFloat *dy, OSQPFloat *dP, OSQPFloat *dq, OSQPFloat *dA, OSQPFloat *dl, OSQPFloat *du,
                                               OSQPFloat *arec);
OSQPInt osqp_hip_batch_adjoint_lockstep_direct_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *l_dev, const OSQPFloat *u_dev, const OSQPFloat *x_dev,
                                                      const OSQPFloat *y_dev, const OSQPFloat *dx_dev, const OSQPFloat *dy_dev, OSQPFloat *dP_dev, OSQPFloat *dq_dev,
                                                      OSQPFloat *dA_dev, OSQPFloat *dl_dev, OSQPFloat *du_dev, OSQPFloat *arec_dev, void *stream);
OSQPInt osqp_hip_lockstep_direct_adjoint_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* ... WITH PER-PROBLEM MATRICES -- the backward pass of osqp_hip_batch_solve_lockstep_direct_mat: osqp_hip_batch_adjoint_lockstep_direct's semantics on the
 * element's OWN matrices.  Problem b's adjoint system is solved on its own P_b, A_b (the dense rows' values included: one factor model per problem), scaled
 * by its own D_b, E_b, c_b, with the Woodbury formula per problem: D0_b, S_b and S_b^-1 are the problem's own, S_b is inverted once.  Px is nbatch x
 * nnz(triu P), Ax nbatch x nnz(A), in the CSC order given at setup, as osqp_hip_batch_solve_lockstep_direct_mat takes them; either may be NULL: the handle's
 * own raw values for every problem.  Every other argument, the OSQP_HIP_ADJOINT_REC record, the statuses 0 / 2 / 3, the stream semantics and INDEPENDENCE
 * (a problem's matrices being part of the problem) are osqp_hip_batch_adjoint_lockstep_direct[_device]'s; dP / dA are per problem at every stored entry, the
 * dense rows' included.  nbatch == 0 on the device entry answers applicability and does nothing else.  A chunk's matrices are prepared as on the forward
 * entry (assembly, equilibration, the chunk's own dense rows and view values: 7 + 4 x settings.scaling launches in front of its transposes in), with the
 * handle's q for every problem: the adjoint does not depend on the cost scale c in exact arithmetic.
 * MATRIX BLOCK: the forward entry's, allocated by whichever of the two entries is called first.  A call here overwrites it; the forward entry prepares it
 * anew in every call, so its results do not depend on calls made here in between.  The handle's own matrices, scaling, iterates, graphs and history, the
 * forward route's workspace and its records are not touched.
 * Returns OSQP_FUNC_NOT_IMPLEMENTED for everything either parent entry declines: what osqp_hip_batch_adjoint_lockstep_direct declines (no Woodbury
 * correction, r > 128, a K0 that is not diagonal, a reordered handle, the host simulator) and what osqp_hip_batch_solve_lockstep_direct_mat declines (a handle
 * without device-side assembly, a repeated (j, j) entry in the stored upper triangle of P).  It does not polish.
 * osqp_hip_lockstep_direct_mat_adjoint_last_record: OSQP_HIP_LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_REC doubles {chunks, chunk width, recurrence steps of the
 * slowest problem, inversions of S summed over the problems, kernel launches of the whole call, GPU ms of the whole call, bytes of the matrix block, GPU
 * ms spent in the preparation}; all zero before the first call.  osqp_hip_lockstep_direct_adjoint_last_record is written as by any direct adjoint call. */
#define OSQP_HIP_LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_REC 8
OSQPInt osqp_hip_batch_adjoint_lockstep_direct_mat(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px, const OSQPFloat *Ax, const OSQPFloat *l, const OSQPFloat *u,
                                                   const OSQPFloat *x, const OSQPFloat *y, const OSQPFloat *dx, const OSQPFloat *dy, OSQPFloat *dP, OSQPFloat *dq,
                                                   OSQPFloat *dA, OSQPFloat *dl, OSQPFloat *du, OSQPFloat *arec);
OSQPInt osqp_hip_batch_adjoint_lockstep_direct_mat_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px_dev, const OSQPFloat *Ax_dev, const OSQPFloat *l_dev,
                                                          const OSQPFloat *u_dev, const OSQPFloat *x_dev, const OSQPFloat *y_dev, const OSQPFloat *dx_dev,
                                                          const OSQPFloat *dy_dev, OSQPFloat *dP_dev, OSQPFloat *dq_dev, OSQPFloat *dA_dev, OSQPFloat *dl_dev,
                                                          OSQPFloat *du_dev, OSQPFloat *arec_dev, void *stream);
OSQPInt osqp_hip_lockstep_direct_mat_adjoint_last_record(OSQPSolver *solver, OSQPFloat *rec);

/* ADJOINT DERIVATIVES of a batch of solved QPs -- the backward pass of osqp_hip_batch_solve[_mat]: ONE launch, one workgroup per problem
 * (batch_hip.hip k_batch_adjoint).  For problem b with solution x (n), y (m) and incoming gradients dx = dL/dx (n), dy = dL/dy (m; NULL = 0):
 *   active rows by polish's rule on z = A x (lower-active: z_i - l_i < -y_i; else upper-active: u_i - z_i < y_i; l_i == u_i: always active, lower if y_i < 0),
 *   [P, A_a'; A_a, 0] [r_x; r_a] = -[dx; dy_a]  (A_a: the active rows), r_y = r_a on active rows and 0 elsewhere,
 *   dq = r_x;  dl_i = -r_y,i on lower-active rows, du_i = -r_y,i on upper-active rows, 0 elsewhere;
 *   dP_ij = (r_x,i x_j + r_x,j x_i) / 2 at every stored entry of P (upper triangle, the CSC order given at setup; the diagonal is r_x,i x_i);
 *   dA_ij = y_i r_x,j + r_y,i x_j at every stored entry of A (CSC order).
 * The system is solved as polish solves its own: the banded LDL' of P + delta I + A_a' A_a / delta in LDS (`delta` setting, in the caller's unscaled
 * units: the kernel works on the unscaled matrices), the first solve and `polish_refine_iter` refinement steps against the unregularised residual.
 * Px / Ax: nbatch x nnz per-problem values as for osqp_hip_batch_solve_mat, l / u: nbatch x m; NULL = this solver's own values for every problem.
 * x, dx: nbatch x n; y, dy: nbatch x m.  Outputs dP: nbatch x nnz(P), dq: nbatch x n, dA: nbatch x nnz(A), dl, du: nbatch x m, arec: nbatch x
 * OSQP_HIP_ADJOINT_REC doubles {status, active rows, final residual max |g - K r| / max |g| of the unregularised system, reserved}; any output may be
 * NULL (skipped).  status 0: residual < OSQP_HIP_ADJOINT_TOL; 1: a pivot of the factorisation was not positive; 2: more active rows than variables
 * (the system is singular); 3: the refinement stalled above the threshold (dependent active rows).  The outputs of an element with a nonzero status are
 * still written: they are the regularised solution.  (q does not enter the derivative.)
 * Returns OSQP_FUNC_NOT_IMPLEMENTED unless the banded factor exists for the problem (permuted half bandwidth <= 56, as for the forward's direct variant) and
 * the kernel's own LDS fits (both matrices' values + 7n + 6m doubles + the band <= 144 KB), for a problem the batch path takes at all (10n + 8m doubles
 * <= 64 KB, a handle that does not work on a reordered copy: the conditions of osqp_hip_batch_solve).  The forward's limit of 4096 stored entries per matrix does not
 * apply: a problem may be differentiated here whose forward ran on another variant.
 * _device: every array in device memory, asynchronous on `stream` with the semantics of osqp_hip_batch_solve_device (like that call it first waits, on the
 * host, for the solver's OWN stream -- pending data updates of the handle -- never for `stream`); nbatch == 0 only answers whether the problem fits. */
#define OSQP_HIP_ADJOINT_REC 4
#define OSQP_HIP_ADJOINT_TOL 1e-6
OSQPInt osqp_hip_batch_adjoint(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px, const OSQPFloat *Ax, const OSQPFloat *l, const OSQPFloat *u,
                               const OSQPFloat *x, const OSQPFloat *y, const OSQPFloat *dx, const OSQPFloat *dy, OSQPFloat *dP, OSQPFloat *dq,
                               OSQPFloat *dA, OSQPFloat *dl, OSQPFloat *du, OSQPFloat *arec);
OSQPInt osqp_hip_batch_adjoint_device(OSQPSolver *solver, OSQPInt nbatch, const OSQPFloat *Px_dev, const OSQPFloat *Ax_dev, const OSQPFloat *l_dev,
                                      const OSQPFloat *u_dev, const OSQPFloat *x_dev, const OSQPFloat *y_dev, const OSQPFloat *dx_dev,
                                      const OSQPFloat *dy_dev, OSQPFloat *dP_dev, OSQPFloat *dq_dev, OSQPFloat *dA_dev, OSQPFloat *dl_dev,
                                      OSQPFloat *du_dev, OSQPFloat *arec_dev, void *stream);
/* ADJOINT DERIVATIVES OF ONE HANDLE ON THE PCG PATH.  osqp_adjoint_derivative_compute / _get_mat / _get_vec run the batch kernel above (a batch of one)
 * where it holds the problem.  Every other handle -- the large QPs this engine exists for, reordered handles (OSQPHipStats::reordered) included --
 * takes the PCG route (adjoint_hip.hip): the rows are classified on the device by the rule above, in the caller's units, on the stored solution;
 * the adjoint system, which is polish's reduced KKT matrix with the right-hand side -[dx; dy_a], is solved by the recurrence polish runs (the
 * proximal method of multipliers at delta_eff = max(delta, OSQPHipPolicy::polish_delta_floor) with the engine's PCG kernels, from a zero start, at
 * least 1 + polish_refine_iter steps, until the residuals stall); the result is unscaled, its residual max |g - K_a r| / max |g| is evaluated on the
 * UNREGULARISED system in the caller's units, and dP / dA are written one thread per stored entry in the caller's CSC order.  The call leaves no trace
 * on the handle: q, the bounds, the iterates and warm-start vectors, rho, info, solution and the launch history are restored exactly, and an
 * osqp_solve after it gives the bits it would have given without it.
 * Return value of osqp_adjoint_derivative_compute on this route: OSQP_NO_ERROR with residual < OSQP_HIP_ADJOINT_TOL; OSQP_LINSYS_SOLVER_INIT_ERROR
 * when the recurrence stalled at or above it (status 3: dependent active rows -- the derivative is not defined, or was not reached) or when there are
 * more active rows than variables (status 2); _get_mat / _get_vec then answer OSQP_DATA_NOT_INITIALIZED.
 * A handle whose PCG runs a Woodbury-corrected preconditioner (OSQPHipStats::woodbury_rows > 0; the portfolio one-launch form is one of its modes)
 * answers OSQP_FUNC_NOT_IMPLEMENTED by default and takes this route with OSQPHipPolicy::adjoint_woodbury = 1 (OSQP_HIP_ADJOINT_WOODBURY): the
 * correction is re-formed from the adjoint's classes and rho vector (a direct mode whose check or probe fails there runs as the PCG's preconditioner),
 * the large form's inverse goes to a buffer of the call's own so that the solve's cached inverses stay alive, and everything of the correction a solve
 * reads -- the direct-mode flag, the slot flag, rho_bar's key, the inverse in use and the cache table, the factorisation counters -- is put back; a
 * Woodbury system that is not positive definite at the adjoint's rho ends the call with status 3 and the correction still on.  The host simulator
 * answers OSQP_FUNC_NOT_IMPLEMENTED whatever the field says.  osqp_hip_batch_adjoint[_device] keep their own eligibility.
 * osqp_hip_adjoint_last_record: what the last osqp_adjoint_derivative_compute of the handle found, OSQP_HIP_ADJOINT_LAST_REC doubles
 *   {status (0 / 2 / 3 as above; the batch kernel's own codes on its route), active rows, residual, recurrence steps (0 on the batch route),
 *    seconds in the recurrence, seconds in the gradient kernels, seconds of the whole call, PCG iterations of the recurrence's linear solves (one per
 *    step where a Woodbury direct mode is the solve; 0 on the batch route)};  all zero before the first call. */
#define OSQP_HIP_ADJOINT_LAST_REC 8
/* osqp_hip_adjoint_compute_at: osqp_adjoint_derivative_compute (either route) at a solution the CALLER holds -- x (n), y (m) of an earlier solve with the
 * data now on the handle.  The derivative depends on (P, A, l, u, x, y) only, so no OSQP_SOLVED solve on the current data is asked for; x = y = NULL
 * means the handle's own last solution, with that requirement.  Results through osqp_adjoint_derivative_get_mat / _get_vec as usual. */
OSQPInt osqp_hip_adjoint_compute_at(OSQPSolver *solver, const OSQPFloat *x, const OSQPFloat *y, const OSQPFloat *dx, const OSQPFloat *dy);
OSQPInt osqp_hip_adjoint_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* osqp_capabilities() reports what the reference's binding asks about and stays as it is; this adds OSQP_CAPABILITY_DERIVATIVES (the adjoint above). */
OSQPInt osqp_hip_capabilities(void);

/* Parametric re-solve with the new data ALREADY ON THE GPU (the reference's update(q, l, u) + solve() loop,
 * src/osqp/nn/torch.py:136-140, /root/reference/src/osqppurepy/_osqp.py:1312-1367 and :1493-1545 restated as kernels):
 * q_dev / l_dev / u_dev / x_dev / y_dev are UNSCALED float64 arrays in device memory of this solver's device, NULL = unchanged.
 * The solver's stream first waits for everything queued on `stream` so far (NULL: the arrays are ready), copies the vectors
 * device-to-device and rescales / re-classifies them with kernels -- no host round trip except the 4-byte l <= u verdict of
 * osqp_hip_update_data_vec_device (OSQP_DATA_VALIDATION_ERROR, nothing changed).  The host-pointer entry points
 * osqp_update_data_vec / osqp_warm_start run the same kernels behind one H2D copy per vector. */
OSQPInt osqp_hip_update_data_vec_device(OSQPSolver *solver, const OSQPFloat *q_dev, const OSQPFloat *l_dev, const OSQPFloat *u_dev, void *stream);
OSQPInt osqp_hip_warm_start_device(OSQPSolver *solver, const OSQPFloat *x_dev, const OSQPFloat *y_dev, void *stream);


/* ---- LinSysSolver slot (north_star's second boundary) -------------------------------------------------------
 * The reference's C core reaches its KKT solver through a table of function pointers created by an init_linsys_solver_*()
 * call; that header is not in the reference tree (the core is fetched at configure time, CMakeLists.txt:31-37), so the
 * member list below follows SURVEY 8b's reconstruction [UPSTREAM-UNVERIFIED]: type, name, solve, update_settings,
 * warm_start, adjoint_derivative, free, update_matrices, update_rho_vec, nthreads.  What is pinned by the reference is the
 * MEANING of solve (purepy's linsys_solver.solve, _osqp.py:307-311, and update_xz_tilde, :644-658):
 *     b = [rhs_x (n); rhs_z (m)]   ->   b = [x~ ; z~],   [[P + sigma I, A'], [A, -diag(1/rho)]] [x~; nu] = b,  z~ = rhs_z + nu / rho
 * which this (indirect) solver computes on the device as  (P + sigma I + A' diag(rho) A) x~ = rhs_x + A'(rho .* rhs_z)  by PCG
 * (warm-started from the previous x~) and  z~ = A x~.  P (upper triangle) and A arrive ALREADY SCALED, rho_vec is given per
 * constraint; the object owns device copies.  b is a host buffer of n + m doubles. */
typedef struct OSQPHipLinSysSolver_ OSQPHipLinSysSolver;
struct OSQPHipLinSysSolver_ {
  enum osqp_linsys_solver_type type;                                              /* OSQP_INDIRECT_SOLVER */
  const char *(*name)(OSQPHipLinSysSolver *self);
  OSQPInt (*solve)(OSQPHipLinSysSolver *self, OSQPFloat *b, OSQPInt admm_iter);    /* 0, or an osqp_error_type */
  void (*update_settings)(OSQPHipLinSysSolver *self, const OSQPSettings *settings);/* cg_max_iter, cg_tol_*, cg_precond */
  void (*warm_start)(OSQPHipLinSysSolver *self, const OSQPFloat *x);               /* start vector of the next PCG (n) */
  OSQPInt (*adjoint_derivative)(OSQPHipLinSysSolver *self);                        /* OSQP_FUNC_NOT_IMPLEMENTED */
  void (*free)(OSQPHipLinSysSolver *self);
  OSQPInt (*update_matrices)(OSQPHipLinSysSolver *self, const OSQPCscMatrix *P, const OSQPInt *Px_new_idx, OSQPInt P_new_n,
                             const OSQPCscMatrix *A, const OSQPInt *Ax_new_idx, OSQPInt A_new_n);   /* same pattern, new values */
  OSQPInt (*update_rho_vec)(OSQPHipLinSysSolver *self, const OSQPFloat *rho_vec, OSQPFloat rho_sc);
  OSQPInt nthreads;                                                                /* 1 host thread drives the device */
  OSQPInt pcg_iters;                                                               /* PCG iterations of the last solve */
  void *impl;
};
/* scaled_prim_res / scaled_dual_res: optional pointers to the caller's CURRENT scaled ADMM residuals; when given, a solve stops
 * at ||r||_inf <= cg_tol_fraction * (*scaled_dual_res) (this engine's rule, DESIGN.md "PCG tolerance"), otherwise (and while
 * that value is not positive) at a relative reduction of 1e-7.  polishing != 0: always the tight relative rule. */
OSQPInt osqp_hip_linsys_init(OSQPHipLinSysSolver **self, const OSQPCscMatrix *P, const OSQPCscMatrix *A, const OSQPFloat *rho_vec,
                             const OSQPSettings *settings, const OSQPFloat *scaled_prim_res, const OSQPFloat *scaled_dual_res,
                             OSQPInt polishing);

/* ---- engine policy (no reference analogue) ----------------------------------------------------------------------------------
 * Everything this engine decides beyond OSQPSettings, PER SOLVER HANDLE: which kernel forms it may use, the rules it adds to the
 * reference's ADMM loop on the indirect path (DESIGN.md sections 2, 2.1, 2.2) and how it schedules its launches.  Defaults =
 * osqp_hip_default_policy(); a new handle starts from the defaults overridden by OSQP_HIP_* environment variables (experiments and
 * A/B runs; read in ONE place, Engine's policy_from_env(), when the handle is created and -- the run-time fields -- at every solve
 * until osqp_hip_set_policy() has been called on it).  osqp_hip_set_policy() changes a handle's policy; fields marked [setup] only
 * matter to handles created afterwards through osqp_hip_set_default_policy() (process-wide default for the NEXT osqp_setup calls of
 * the calling thread), because they choose data structures built at setup. */
typedef struct {
  /* kernel forms */
  OSQPInt graph;              /* replay captured launch strings (hipGraph) instead of enqueuing them one by one                 [setup] */
  OSQPInt slots;              /* device-side scheduling of the ADMM / PCG phases ("slot" kernels)                               [setup] */
  OSQPInt pcg_fused;          /* 1: vector update fused into the SpMV kernels; 0: the three-kernel PCG iteration                [setup] */
  OSQPInt f1;                 /* one launch per PCG iteration where the matrices allow it (banded A; 1: a block's few columns outside its
                                 window are taken as far columns -- band + long-range couplings; 2: strict windows only;
                                 3: diagnostic -- the mixing kernels also on a matrix without far columns)                          [setup] */
  OSQPInt window;             /* windowed row blocks (16-bit local column indices, input window in LDS)                         [setup] */
  OSQPInt woodbury;           /* a few dense rows of A (1..128 rows with > 128 entries) are treated exactly in the preconditioner   [setup] */
  OSQPInt woodbury_direct;    /* ... and when the rest of K is diagonal, that preconditioner IS K^-1: the linear solve without PCG iterations [setup] */
  OSQPInt woodbury_large;     /* up to 16384 dense rows carrying most of A: the same correction with the r x r system formed and inverted on the device
                                 by this engine's own fp64 matrix-core kernels (dense_hip.hip; no vendor library)                  [setup] */
  OSQPInt device_driven;      /* chunk boundaries (termination test, adaptive rho, PCG tolerance / budget) decided on the device; 2: also for the Woodbury
                                 direct mode in two launches (there the host-synchronous loop is the faster one and the default) */
  OSQPInt small_direct;       /* small QPs: the whole solve as ONE launch of the batch kernel's direct (banded LDL') variant */
  OSQPInt batch_reorder;      /* batch solves: launch the problems in the order of the previous call's iteration counts */
  OSQPInt batch_variant;      /* 0 automatic; 1 direct (one wave), 2 direct256, 3 w64 (PCG), 4 w256 (PCG), 5 generic -- if applicable */
  /* rules on top of the reference's loop */
  OSQPFloat extrap;           /* PCG start = x~ + extrap * (x~ - x~_prev)  (0: the previous x~)                                  [setup] */
  OSQPFloat rho_eq_factor;    /* equality-row weight on problems with inequality rows; 0 = automatic (10, or 1e3 for n <= 256)   [setup] */
  OSQPInt rho_window;         /* ADMM iterations before an adaptation point that run with a tighter PCG tolerance (0: none) */
  OSQPFloat rho_window_tol;   /* ... tolerance factor of that window */
  OSQPInt rho_persist;        /* apply a rho estimate that stays on one side of rho at two consecutive adaptation points */
  OSQPFloat rho_tol_exp;      /* adaptive_rho_tolerance is spent as tolerance^rho_tol_exp on QPs (1 = the setting's literal value) */
  OSQPFloat budget_tolerate, budget_sigma; OSQPInt budget_slack, budget_full;   /* PCG limit per solve: mean + sigma * std of the last chunk (+ slack); full: never below cg_max_iter */
  OSQPInt cg_escalate;        /* double cg_max_iter while the inner solver stagnates; checkpointed first chunk */
  OSQPInt stall;              /* drop the PCG tolerance while the iterates run away (unbounded problems) */
  OSQPFloat polish_delta_floor; /* polish on the PCG path: the refinement recurrence runs with delta_eff = max(settings.delta, this) (Engine::polish) */
  OSQPFloat polish_pcg_tol;   /* ... relative residual its inner systems are solved to */
  /* scheduling of the launch strings (results never depend on these) */
  OSQPInt slot_poll; OSQPInt poll_low; OSQPFloat poll_first, poll_frac, poll_wait;      /* host-synchronous chunks: top-ups from polled progress */
  OSQPInt finish_pairs; OSQPInt poll_sleep_us;      /* device-driven chunks: a boundary group goes out when at most finish_pairs slot pairs are missing; pause between polls */
  /* diagnostics */
  OSQPInt slot_log, setup_timing, batch_timing, woodbury_log;
  OSQPFloat woodbury_direct_tol; /* device-factorised form: the direct mode (no confirming PCG iteration) is taken while the probe  max |M^-1 K v - v| / max |v|
                                 measured after every factorisation stays below this (default 1e-6: every linear solve then reduces its residual a
                                 millionfold -- orders beyond any tolerance the PCG would have been asked for; r03 demanded 1e-9, which the Woodbury
                                 identity misses at 5k x 10k by a factor 4-40)                                                        [setup] */
  OSQPInt woodbury_fused;     /* 1 (default): the Woodbury direct mode in its fused forms where they apply -- a few dense rows (P diagonal, one-entry short rows,
                                 n <= 16384; wbdirect_hip.hip): ONE launch per ADMM iteration (round 6; rounds 3-5: two); many dense rows in column space: seven
                                 launches that stream the dense block twice (woodbury_hip.hip wbf_iteration).  2: the two-launch form of rounds 3-5 (A/B runs);
                                 0: KB, the kernels of M^-1, KA                                                                                    [setup] */
  OSQPInt debug_fail_refactor; /* TEST HOOK: that many of the next device-side inversions of the Woodbury system report "inaccurate" (exercises the
                                 hand-over of a device-driven direct-mode solve to the host); 0 in production */
  OSQPInt reorder;            /* 1 (default): when the one-launch PCG form does not apply to the matrices as numbered by the caller, look for a
                                 bandwidth-reducing permutation of variables and constraints under which it does, and work on the permuted problem
                                 (every vector crossing this API keeps the caller's numbering); 0: never; 2: always permute (tests)      [setup] */
  OSQPInt woodbury_cache;     /* 1 (default): the device-factorised Woodbury form keeps the last four inverses by rho_bar; a rho the handle has seen before is a
                                 look-up + the numerical probe instead of an r^3 factorisation (OSQPHipStats::woodbury_cache_hits); 0: always factorise   [setup] */
  OSQPInt kform;              /* 1: where the one-launch form on A alone (f1) does not apply and no Woodbury mode is on, hold the reduced matrix
                                 K = P + sigma I + A' diag(rho) A explicitly when its fill is moderate (sum of squared row lengths of A <= 8 nnz(A)) and run
                                 ONE launch per PCG iteration on it (any sparsity pattern; k + 3 launches per ADMM iteration instead of 2 k + 4).
                                 0 (default): the two-kernel form -- measured faster on MI355X: K needs nnz(K) random gathers per product (41 per row at
                                 configs[1] sizes with unstructured columns: 4.1 M against the 2.2 M of the A / B pair), and a random 8..32-byte gather costs a
                                 whole 128-byte line of L2 -> L1 traffic: 18-24 us per 4.2 M gathers alone (profiles/r06a_kform_gather_bench.txt)        [setup] */
  OSQPInt woodbury_dual;      /* 1 (default): the device-factorised Woodbury form works in COLUMN space where that is the smaller system -- the columns the dense rows touch
                                 split into dense columns (two or more entries) and singletons (one: the lasso's -y_i); with fewer dense columns than 3/4 of the dense
                                 rows, the cd x cd system  T = D0_C + A_d' diag(w) A_d  on the dense columns replaces the r x r system S (lasso 5k x 10k: 5 000 against
                                 10 000: an eighth of the factorisation, a quarter of the inverse); 0: always the row-space form                                [setup] */
  OSQPInt woodbury_vendor;    /* RETIRED: accepted and ignored.  It selected rocBLAS / rocSOLVER for the dense system of the device-factorised Woodbury form (the route of
                                 rounds 3-5, then an A/B switch); that route is gone, this engine's own kernels (dense_hip.hip: a strided MFMA GEMM + block Gauss-Jordan
                                 inversion) are the only one.  The field keeps its place: the struct is append-only                                           */
  OSQPInt batch_wave;         /* batch solves in the spectral form: one WAVE per problem, eight problems in flight per CU, the longest-expected problems on the
                                 workgroup kernel beside it (batch_hip.hip k_batch_wave).  0 (default): for batches of at least 2048 problems, or 1280 with a
                                 launch order from a previous call (measured, MPC batch, with a launch order: 4096 QPs 2.8 ms against 5.7, 2048 1.8 against
                                 3.0, 1280 1.7 against 1.9, 1024 1.7 against 1.6; without: 2048 3.5 against 3.6, 1536 3.5 against 3.1 -- below that a
                                 problem's own latency on one wave decides); 1: at every batch size; -1: never */
  OSQPInt adjoint_woodbury;   /* 0 (default): a handle whose PCG runs a Woodbury-corrected preconditioner (OSQPHipStats::woodbury_rows > 0) answers
                                 OSQP_FUNC_NOT_IMPLEMENTED to osqp_adjoint_derivative_compute / osqp_hip_adjoint_compute_at; 1: it takes the PCG route, with the
                                 correction following the adjoint's constraint classes and its state saved and put back (Engine::adjoint_compute_pcg).  May be
                                 set on a live handle; OSQP_HIP_ADJOINT_WOODBURY, anything but 0 = on */
} OSQPHipPolicy;
void    osqp_hip_default_policy(OSQPHipPolicy *policy);
OSQPInt osqp_hip_set_policy(OSQPSolver *solver, const OSQPHipPolicy *policy);
OSQPInt osqp_hip_get_policy(OSQPSolver *solver, OSQPHipPolicy *policy);
void    osqp_hip_set_default_policy(const OSQPHipPolicy *policy);      /* NULL: back to osqp_hip_default_policy() + environment */

/* Diagnostic builds only (make TRACE=1: kernels stamp the wall clock per workgroup and phase, 16 slots per workgroup):
 * copies the stamps of the most recent launches.  The product library returns OSQP_FUNC_NOT_IMPLEMENTED. */
OSQPInt osqp_hip_trace_read(OSQPSolver *solver, unsigned long long *out, OSQPInt count);
/* Test hook (used by tests/ only): which = 0: out = A in (n -> m); 1: out = B [in_n; in_m] (n + m -> n), with the scaled device matrices. */
OSQPInt osqp_hip_test_spmv(OSQPSolver *solver, OSQPInt which, const OSQPFloat *in, OSQPFloat *out);
/* Test hook (used by tests/ only): one routine of the dense fp64 kernels (dense_hip.hip) on the CALLER's data.  The three host buffers are copied to the
   solver's device, the routine runs on the solver's stream, and C comes back whole (c_len doubles: a test sees every cell the routine wrote).  Element
   (i, k) of A is A[a_off + i as_i + k as_k], (k, j) of B is B[b_off + k bs_k + j bs_j], (i, j) of C is C[c_off + i cs_i + j cs_j]; an operand that does
   not fit its buffer is OSQP_DATA_VALIDATION_ERROR, an operand without a unit stride the routine's own error (OSQP_ALGEBRA_LOAD_ERROR).
     op 0  dense_gemm:         C (M x N) = beta C + alpha A B, inner dimension K
     op 1  dense_gemm_sym:     C (N x N, row-major, leading dimension cs_i) = alpha A B for a symmetric product; M, beta, cs_j unused
     op 2  dense_spd_inverse:  C (N x N, row-major, leading dimension cs_i) <- C^-1 in place; minpiv = the smallest pivot met (<= 0 or NaN: not positive
                               definite); A, B, M, K, alpha, beta unused */
typedef struct {
  OSQPInt op, M, N, K;
  OSQPFloat alpha, beta;
  long long as_i, as_k, bs_k, bs_j, cs_i, cs_j;
  long long a_off, b_off, c_off;
  long long a_len, b_len, c_len;
  const OSQPFloat *A, *B;
  OSQPFloat *C;
  OSQPFloat minpiv;                /* out (op 2) */
} OSQPHipDenseTest;
OSQPInt osqp_hip_test_dense(OSQPSolver *solver, OSQPHipDenseTest *t);
/* Test hook (used by tests/ only): the padded band of the batch path's direct solve (csrc/band_ldl.h) on the CALLER's matrix, in ONE workgroup of
   `threads` threads (64 or 256; guard = 1, the adjoint's pivot rule with pivot_floor, exists with 256 only -- the three forms the product runs):
   band_clear, the caller's entries scattered at band_slot(), band_factor, band_solve once per right-hand side, on the solver's stream, synchronous.
     band   [n (bw + 1)]  band[c (bw + 1) + k] = K[c + k][c], lower triangle; entries with c + k >= n are never read
     perm   [n]           position in the band's order -> variable (a permutation of 0 .. n-1)
     rhs    [nrhs n]      right-hand sides in the caller's variable order, 0 <= nrhs <= 8
     x      [nrhs n + 16] in/out: copied to the device first and back whole, so a cell the kernel did not write keeps the caller's value
     image  [band_doubles(n, bw) = 8 + roundup8(n) (bw + 8) + 64]  out: the band's whole LDS allocation from its first double (front padding, columns,
                          slack) as it stands after the last substitution: unit-lower L^ at the slots, zeros everywhere else
     dinv   [n]           out: 1 / D
     bad                  out: band_factor's result (guard = 1: a pivot was replaced)
   Everything is checked before anything is launched -- n >= 1, 0 <= bw <= min(56, n - 1), threads / guard / nrhs as above, perm a permutation, every
   length exactly as listed, band + two vectors within the product's 144 KB of LDS: anything else is OSQP_DATA_VALIDATION_ERROR. */
typedef struct {
  OSQPInt n, bw, threads, guard, nrhs;
  OSQPFloat pivot_floor;
  long long band_len, perm_len, rhs_len, x_len, image_len, dinv_len;
  const OSQPFloat *band;
  const OSQPInt *perm;
  const OSQPFloat *rhs;
  OSQPFloat *x, *image, *dinv;
  OSQPInt bad;                     /* out */
} OSQPHipBandTest;
OSQPInt osqp_hip_test_band(OSQPSolver *solver, OSQPHipBandTest *t);
/* Test hook (used by tests/ only): the Woodbury correction M^-1 (csrc/woodbury_hip.hip) of a set-up handle whose correction is on,
   at the handle's CURRENT matrices and rho vector, through the product's own functions: with refactor != 0 wb_factor (D0, then S / S^-1 of the small
   form, the device-factorised row-space form, or T / T^-1 of the column-space form, with their checks), then the caller's r is copied to the PCG's
   residual vector, the `converged` flag is cleared and wb_apply(parity, direct) runs -- with direct != 0 the caller's x0 is loaded to x~ first and the
   last kernel adds u to it.  Synchronous.  Vectors are in the caller's numbering; everything is in the SCALED problem (osqp_hip_get_scaling).
     r      [n]                right-hand side                          x0  [n with direct, else 0]  x~ before the call
     u      [n + 16]           M^-1 r                                   xs  [n + 16]                 x~ after the call (x0 + u with direct)
     dinv0  [n + 16]           1 / D0                                   rho [m + 16]                 the rho vector
     S, Sinv [order^2 + 16]    the dense system and its inverse, row-major: S (order = long rows, in the order of idx) in the small and the row-space
                               form, T (order = dense columns, in the order of idx) in the column-space form
     idx    [order + 16]       the long rows (forms 0, 1) / the dense columns (form 2) in the order S / T lists them
   Of every output exactly the listed count is written: the 16 cells behind it keep the caller's values.  form: 0 small, 1 row space, 2 column space;
   rows: long rows; exact: the direct mode's verdict (DevWb::exact) after the call; info: the two status words of the factorisation; done / iters: the
   PCG's `converged` flag and iteration count after the call; gamma = <r, u> and rnorm = max |r|: the partial results the last kernel left for the
   PCG (slots of the given parity), one per workgroup, folded here on the host in index order (sum, maximum) -- the PCG folds the same values in
   another order.  Everything the call overwrites -- residual, u, x~, the flags, those partial slots -- is restored before it returns, and a
   re-factorisation recomputes what the handle already holds: a solve after the call is the solve without it.
   OSQP_FUNC_NOT_IMPLEMENTED: the backend has no Woodbury correction, or this handle's is off.  Every length and flag is checked before anything is
   launched (anything else than listed: OSQP_DATA_VALIDATION_ERROR). */
typedef struct {
  OSQPInt refactor, parity, direct;
  long long r_len, x0_len, u_len, xs_len, dinv0_len, s_len, sinv_len, rho_len, idx_len;
  const OSQPFloat *r, *x0;
  OSQPFloat *u, *xs, *dinv0, *S, *Sinv, *rho;
  OSQPInt *idx;
  OSQPInt form, order, rows, exact, info[2], done, iters;   /* out */
  OSQPFloat gamma, rnorm;                                    /* out */
} OSQPHipWoodburyTest;
OSQPInt osqp_hip_test_woodbury(OSQPSolver *solver, OSQPHipWoodburyTest *t);
/* Test hook (used by tests/ only): single launches of the lockstep block-vector kernels (csrc/lockstep_hip.hip) on a work block the
   caller fills -- POKE, RUN, PEEK.  The entry builds the kernel arguments exactly as a lockstep solve of this handle does (settings, matrices, scalings,
   permutations, value maps, the route's resident work block and, with mat, its resident matrix block, allocated as a first solve would), uploads the
   caller's whole blocks into them, launches the listed ops in order on the solver's stream -- each op is ONE kernel launch, with the arguments and the grid
   the drivers use (one text serves both) --, synchronises, and downloads the whole blocks and x / y / rec.  No host loop of a solve runs.
     route    0: the PCG route.  1: the direct route of a Woodbury handle with a diagonal K0 (osqp_hip_batch_solve_lockstep_direct): the blocks are then that
              route's -- dws_need / dmat_need doubles (lockstep_direct_ws_doubles(n, m, r), lockstep_direct_mat_ws_doubles) -- and the ops are the kernels that route
              launches: LOAD_N LOAD_M INIT STORE_N STORE_M INITZ RHS UPD RESM RESN SETRHO (INITZ and RESM read A through the view, UPD runs over n + r rows), with
              mat the matrices of a chunk, and the ops from D0 on (VALS and WT: with mat only).  On route 0 the ops from D0 on do not belong
     mat      0: the handle's matrices (k_ls_*);  1: per-problem matrices (k_lsm_*), mat_ws is then the chunk's matrix block
     count    1 .. 64 problems;  warm: as the solve entries'
     ops      [nops], 1 <= nops <= 64, each an OSQPHipLockstepOp that belongs to (route, mat) and to this handle: the ops from BEGIN on need mat = 1, ASM_A /
              ASM_P need stored entries, and the ops a solve never launches with m = 0 (LOAD_M, STORE_M, INITZ, T, RESM, SETRHO, SUPP) need m > 0
     q l u    [count][n] / [count][m] in the caller's numbering, each optional (NULL with length 0: the handle's own vector)
     x y rec  [count][n], [count][m], [count][OSQP_HIP_BATCH_REC]: in (warm start) and out; always uploaded whole and downloaded whole
     Px Ax    with mat: [count][nnz(triu P)] / [count][nnz(A)] in the CSC order given at setup, each optional (NULL with length 0: the handle's values)
     ws       the chunk's WHOLE work block, in and out: ws_need doubles (csrc/lockstep_layout.h lockstep_ws_doubles(n, m), the engine's numbering)
     mat_ws   with mat: the WHOLE matrix block, in and out: mat_need doubles (lockstep_mat_ws_doubles); without: NULL with length 0
   What the references need of the handle, each group optional (length 0 and NULL pointers: not wanted; else every pointer of the group and the exact length),
   in the ENGINE's numbering (osqp_hip_get_reordering):
     A_rowptr [m + 1], A_col / A_val [nnzA], B_rowptr [n + 1], B_col / B_val [nnzB]    the scaled CSR of A and of B = [P + sigma I | A']
     D Dinv [n], E Einv [m]; c                                                          the handle's scaling
     Pm1 Pm2 pvmap Praw [nzP], AmA AmB avmap Araw [nzA], Bdiag [n]                      the assembly maps (Pm2 = -1: a diagonal entry), the value maps of a
                                                                                        reordered handle (the identity otherwise), the raw values
   and, with route 1, the direct route's view (each group as above):
     Av_rowptr [m + 1], Av_col Av_val vsrc [nv]                                         the view of A: a long row is the single entry 1.0 at column n + a; where a
                                                                                        view entry sits in A_val (-1: a long row's 1.0)
     WT wtpos [n r], rows [r], islong [m]                                               the dense rows (entry (column j, long row a) at j r + a), where each sits in
                                                                                        A_val (-1: none), the long rows' indices, the row flags (0 / 1)
   r, GC, cb, nv (the long rows, the column blocks of the products and their width, the view's entries) and dws_need / dmat_need are written with the sizes
   where the direct route takes the handle (0 otherwise).
   Whenever the handle is ready and t is not NULL the sizes n, m, nnzA, nnzB, nzP, nzA, G (lockstep_grid), ws_need, mat_need are written first, whatever the
   call then answers: a caller learns the lengths from a call it expects to be rejected.  Everything else is checked BEFORE anything is allocated, uploaded
   or launched: a NULL struct, a length other than listed, a NULL pointer where a length is given, an op that does not belong, count or nops outside
   1 .. 64, route or mat outside {0, 1} give OSQP_DATA_VALIDATION_ERROR and nothing runs; a handle the route declines (the solve entry's own predicate)
   gives OSQP_FUNC_NOT_IMPLEMENTED -- with route 1 in front of the op and length checks, because that route's lengths exist only where it takes the handle.  The contents of the blocks are NOT checked and need not be: the kernels take every index from the handle's arrays and
   the carve; the blocks hold values, 0/1 flags and counters only.  The resident blocks are a solve's scratch -- every solve rewrites what it reads -- so a
   solve after the call is the solve without it. */
typedef enum {
  OSQP_HIP_LS_LOAD_N = 0, OSQP_HIP_LS_LOAD_M, OSQP_HIP_LS_INIT, OSQP_HIP_LS_STORE_N, OSQP_HIP_LS_STORE_M,                       /* transposes and state */
  OSQP_HIP_LS_MINV, OSQP_HIP_LS_INITZ, OSQP_HIP_LS_RHS, OSQP_HIP_LS_T, OSQP_HIP_LS_KP, OSQP_HIP_LS_UPD, OSQP_HIP_LS_RESM, OSQP_HIP_LS_RESN,   /* row passes */
  OSQP_HIP_LS_SETRHO, OSQP_HIP_LS_CGUPD, OSQP_HIP_LS_CGP,                                                                       /* elementwise */
  OSQP_HIP_LS_CGINIT, OSQP_HIP_LS_CGALPHA, OSQP_HIP_LS_CGBETA,                                                                  /* folds */
  OSQP_HIP_LS_BEGIN, OSQP_HIP_LS_ASM_A, OSQP_HIP_LS_ASM_P, OSQP_HIP_LS_NORMS, OSQP_HIP_LS_SCALE, OSQP_HIP_LS_COST, OSQP_HIP_LS_COST_APPLY, OSQP_HIP_LS_FINISH,   /* matrices of a chunk */
  OSQP_HIP_LS_D0, OSQP_HIP_LS_S, OSQP_HIP_LS_INV,                                                                               /* direct route: the factor */
  OSQP_HIP_LS_PROD_X, OSQP_HIP_LS_PROD_XS, OSQP_HIP_LS_PROD_P, OSQP_HIP_LS_PROD2,       /* the products with the long rows: x -> pg, x~ -> pg2, p -> pg; both of the first two in one pass */
  OSQP_HIP_LS_SETL0, OSQP_HIP_LS_SETL1, OSQP_HIP_LS_H, OSQP_HIP_LS_X,                   /* k_lw_setl with start 0 / 1, k_lw_h, k_lw_x */
  OSQP_HIP_LS_VALS, OSQP_HIP_LS_WT,                                                     /* the chunk's own view values and dense rows (mat) */
  OSQP_HIP_LS_SUPP,                                                                     /* k_ls_supp (check_dualgap): both routes, with and without mat; needs m > 0 */
  OSQP_HIP_LS_OP_COUNT
} OSQPHipLockstepOp;
typedef struct {
  OSQPInt route, mat, count, warm, nops;
  const OSQPInt *ops;
  long long q_len, l_len, u_len, x_len, y_len, rec_len, px_len, ax_len, ws_len, mat_len;
  long long arp_len, anz_len, brp_len, bnz_len, n_len, m_len, pmap_len, amap_len, bdiag_len;
  long long avrp_len, av_len, wt_len, rows_len, islong_len;
  const OSQPFloat *q, *l, *u;
  OSQPFloat *x, *y, *rec;
  const OSQPFloat *Px, *Ax;
  OSQPFloat *ws, *mat_ws;
  OSQPInt *A_rowptr, *A_col, *B_rowptr, *B_col;
  OSQPFloat *A_val, *B_val, *D, *Dinv, *E, *Einv;
  OSQPInt *Pm1, *Pm2, *pvmap, *AmA, *AmB, *avmap, *Bdiag;
  OSQPFloat *Praw, *Araw;
  OSQPInt *Av_rowptr, *Av_col, *vsrc, *wtpos, *rows, *islong;
  OSQPFloat *Av_val, *WT;
  OSQPInt n, m, nnzA, nnzB, nzP, nzA, G;          /* out */
  long long ws_need, mat_need;                    /* out */
  OSQPFloat c;                                    /* out (with the n_len group) */
  OSQPInt r, GC, cb, nv;                          /* out: the direct route */
  long long dws_need, dmat_need;                  /* out: the direct route */
} OSQPHipLockstepTest;
OSQPInt osqp_hip_test_lockstep(OSQPSolver *solver, OSQPHipLockstepTest *t);
/* Test hook (used by tests/ only): osqp_hip_test_lockstep for the kernels csrc/lockstep_hip.hip adds for the BACKWARD PASS and for POLISH -- POKE, RUN, PEEK,
   each op ONE kernel launch with the kernel (shared or own-matrix twin), the arguments and the grid the drivers use (ls_adj_go / ls_pol_go: one text serves
   the drivers and this entry).  No host loop, no recurrence.
     mode     0: ADJOINT.  The arguments are LockstepAdjointParams as osqp_hip_batch_adjoint_lockstep* builds them (recurrence settings, scalings, the entry
              maps of the gradients); ws is the WHOLE adjoint work block, in and out: adj_need doubles (lockstep_adjoint_ws_doubles(n, m); route 1: dadj_need,
              lockstep_direct_adjoint_ws_doubles(n, m, r)) -- the forward's block followed by ax gdx rx | ay gdy ry | code (packed ints).
              1: POLISH.  The arguments are LockstepParams as a polishing osqp_hip_batch_solve_lockstep* builds them (pol_rho, pol_min_steps, check_dualgap,
              the epsilons) whatever settings.polishing says; ws is the forward block (ws_need / dws_need) and pol_ws the WHOLE polish block, in and out:
              pol_need doubles (lockstep_polish_ws_doubles(n, m): x | y z l u).
     route, mat, count   as osqp_hip_test_lockstep's; mat = 1 picks the k_lsm_* twin where one exists, mat_ws is then the matrix block (mat_need / dmat_need)
     ops      [nops], 1 <= nops <= 64, each an OSQPHipLockstepBackOp of this mode.  ADJ_*: mode 0 (on route 1 LOAD_N writes x~ = Dinv x to the block vector
              x~, CLASS and RESM read A through the view, as the direct backward pass launches them); GRAD_P / GRAD_A: k_ls_adj_grad<true / false>.
              LWA_SETL_X / LWA_SETL_XS (k_lwa_setl into x / x~) and LWA_ZERO: route 1, either mode.  POL_*: mode 1; POL_END takes `secs`.
              ADJ_LOAD_M, ADJ_CLASS, ADJ_RESM, ADJ_OUT_M and POL_CONE need m > 0; GRAD_P / GRAD_A need stored entries; an op that stores to a caller's
              array needs it: ADJ_OUT_N dq, ADJ_OUT_M dl or du, GRAD_P dP, GRAD_A dA.
     mode 0 arrays, [count][...] in the caller's numbering (dP / dA: the CSC order given at setup):
       in     sx gx [count][n], sy [count][m]: required.  gy l u [count][m]: each optional (NULL with length 0: zero / the handle's own bounds)
       out    dq [count][n], dl du [count][m], dP [count][nnz(triu P)], dA [count][nnz(A)], arec [count][OSQP_HIP_ADJOINT_REC]: each optional; uploaded whole and
              downloaded whole, so that what an op does not write comes back as it went in
     mode 1 arrays: x y rec as osqp_hip_test_lockstep's (no polish kernel stores to them: they come back as they went in)
   The arrays of the other mode must be absent.  Out: the sizes n, m, nzP, nzA, G, r and ws_need, dws_need, adj_need, dadj_need, mat_need, dmat_need,
   pol_need are written first whenever the handle is ready and t is not NULL (the direct route's where it takes the handle, 0 otherwise); after a call that
   ran, the scalars the references need and do not restate: gain, min_steps, max_steps, rho0 (the adjoint recurrence: as built in mode 0, the struct's defaults
   in mode 1), pol_rho, pol_min_steps (as built in mode 1, the defaults in mode 0), pol_max_steps, adjoint_tol (OSQP_HIP_ADJOINT_TOL), check_dualgap.
   Everything is checked BEFORE anything is allocated, uploaded or launched (OSQP_DATA_VALIDATION_ERROR, nothing runs): a length other than listed, a NULL
   pointer where a length is given, an array of the other mode, an op outside the enum, of the other mode, of the other route, an m-side op with m = 0, a
   gradient without stored entries, an output op without its array, mat = 1 without the matrix block.  A handle the route declines (the solve / adjoint
   entry's own predicate): OSQP_FUNC_NOT_IMPLEMENTED.  The resident blocks are scratch: a solve or backward pass after the call is the one without it. */
typedef enum {
  OSQP_HIP_LSB_ADJ_LOAD_N = 0, OSQP_HIP_LSB_ADJ_LOAD_M, OSQP_HIP_LSB_ADJ_CLASS, OSQP_HIP_LSB_ADJ_INIT, OSQP_HIP_LSB_ADJ_DECIDE, OSQP_HIP_LSB_ADJ_UNSCALE,
  OSQP_HIP_LSB_ADJ_RESM, OSQP_HIP_LSB_ADJ_RESN, OSQP_HIP_LSB_ADJ_FINAL, OSQP_HIP_LSB_ADJ_OUT_N, OSQP_HIP_LSB_ADJ_OUT_M, OSQP_HIP_LSB_ADJ_GRAD_P, OSQP_HIP_LSB_ADJ_GRAD_A,
  OSQP_HIP_LSB_LWA_SETL_X, OSQP_HIP_LSB_LWA_SETL_XS, OSQP_HIP_LSB_LWA_ZERO,
  OSQP_HIP_LSB_POL_BEGIN, OSQP_HIP_LSB_POL_CLASS, OSQP_HIP_LSB_POL_DECIDE, OSQP_HIP_LSB_POL_CONE, OSQP_HIP_LSB_POL_ACCEPT, OSQP_HIP_LSB_POL_END,
  OSQP_HIP_LSB_OP_COUNT
} OSQPHipLockstepBackOp;
typedef struct {
  OSQPInt mode, route, mat, count, nops;
  const OSQPInt *ops;
  OSQPFloat secs;
  long long sx_len, sy_len, gx_len, gy_len, l_len, u_len, dq_len, dl_len, du_len, dp_len, da_len, arec_len, x_len, y_len, rec_len, ws_len, mat_len, pol_len;
  const OSQPFloat *sx, *sy, *gx, *gy, *l, *u;
  OSQPFloat *dq, *dl, *du, *dP, *dA, *arec, *x, *y, *rec, *ws, *mat_ws, *pol_ws;
  OSQPInt n, m, nzP, nzA, G, r;                                                           /* out */
  long long ws_need, dws_need, adj_need, dadj_need, mat_need, dmat_need, pol_need;        /* out */
  OSQPInt min_steps, max_steps, pol_min_steps, pol_max_steps, check_dualgap;              /* out */
  OSQPFloat gain, rho0, pol_rho, adjoint_tol;                                             /* out */
} OSQPHipLockstepBackTest;
OSQPInt osqp_hip_test_lockstep_back(OSQPSolver *solver, OSQPHipLockstepBackTest *t);
/* Test hook (used by tests/ only): a few ADMM iterations of the PCG path (csrc/pcg_hip.hip; DESIGN.md sections 2, 4.2, 4.3) from iterates the caller
   gives, through the handle's OWN launch path, with everything the kernels left behind read back -- POKE, RUN, PEEK on a set-up handle.
     POKE   x [n], z [m], y [m], xt [n] (x~): SCALED iterates (osqp_hip_get_scaling) in the caller's numbering.  They are uploaded; then the entry does
            what the driver does after a warm start or a rho change: z~ = A x~, t0 = rho z~, v = rho z - y, and the PCG start without history
            (x_g = x~_prev = x~).
     RUN    `iters` ADMM iterations (1 .. 8), every PCG capped at `cap` iterations (0 .. 16) and stopped by ||r_i||_inf <= max(tol_rel ||rhs||_inf, tol_abs),
            tested before iteration i: with tol_rel = tol_abs = 0 every PCG with a nonzero residual runs exactly `cap` iterations.  A handle without slots
            enqueues the chunk as a solve does (captured once per (iters, cap) when the handle replays graphs); a handle with slots begins a chunk of `iters`
            iterations and enqueues the slot pairs `iters` iterations of `cap` PCG iterations need plus one spare pair, then synchronises ONCE.  No boundary
            group, no termination test, no rho adaptation, no top-up: a chunk the slots did not finish is OSQP_ALGEBRA_LOAD_ERROR.
     PEEK   x, z, y, xt, zt (z~), dx, dy, v, t0, xg (the next PCG's start), rho [m] and Minv [n] as they stand on the device -- each read where the
            form keeps it --, the chunk's PCG statistics, the last PCG's tolerance and start residual, and hist [3 cap] = gamma[0 .. cap), alpha[0 .. cap),
            beta[0 .. cap) of the LAST PCG as far as the form records them (beta: the fused pair only; entries the PCG did not reach are stale).
            form: 0 three-kernel, 1 fused pair enqueued by the host, 2 slot two-kernel, 3 F1 (f1_D replicas, f1_mix), 4 K form; launches: kernel launches enqueued.
   Every length is exact (n_len = n, m_len = m, hist_len = 3 cap; a NULL pointer only where the length is 0) and everything is checked before anything is
   uploaded or launched: anything else is OSQP_DATA_VALIDATION_ERROR.  A handle whose Woodbury correction is on answers OSQP_FUNC_NOT_IMPLEMENTED
   (osqp_hip_test_woodbury is its tier).  The handle's iterates STAY as the run left them, like after a warm start: a later osqp_solve with
   warm_starting = 0 cold-starts and is the solve of a fresh handle bit for bit; with warm_starting = 1 it continues from them. */
typedef struct {
  OSQPInt iters, cap;
  OSQPFloat tol_rel, tol_abs;
  long long n_len, m_len, hist_len;
  const OSQPFloat *x_in, *z_in, *y_in, *xt_in;
  OSQPFloat *x, *z, *y, *xt, *zt, *dx, *dy, *v, *t0, *xg, *rho, *Minv, *hist;          /* out */
  OSQPInt form, f1_D, f1_mix, launches;                                                /* out */
  OSQPInt stat_sum, stat_max, stat_unconv, stat_n, pcg_iters, pcg_done;                /* out: F_STAT_SUM / MAX / UNCONV / N of the chunk, F_ITERS / F_DONE of the last PCG */
  OSQPFloat tol_now, rn0;                                                              /* out: S_TOL_NOW, S_RN0 of the last PCG */
} OSQPHipAdmmTest;
OSQPInt osqp_hip_test_admm(OSQPSolver *solver, OSQPHipAdmmTest *t);
/* Test hook (used by tests/ only): the CHUNK BOUNDARY of a single-QP solve on vectors the caller gives -- the residual kernels and their two-level fold,
   the second stage of the infeasibility tests, the kernels that follow a rho change, and the device-driven boundary group with the rules of csrc/policy.h
   between them (DESIGN.md sections 2, 2.1) -- POKE, RUN, PEEK on a set-up handle.
     POKE   x, dx, xt (x~) [n] and z, y, dy, zt (z~) [m]: SCALED vectors (osqp_hip_get_scaling) in the caller's numbering.  They are uploaded into the
            handle's own arrays and NO refresh kernel runs: the kernels under test read exactly what was given.
     RUN    mode 0 (any handle; the host simulator too): the residual pass, then for the bits of `need` (1: primal, 2: dual) the second-stage kernels of
            the infeasibility tests -- the dual one with the caller's threshold `thr` and `unscaled` --, then the fetch of the residual block.
            mode 1: the device-driven boundary group.  The state block is built as a solve builds it (settings snapshot, PCG tolerance from a residual pass
            of the poked vectors, the first chunk), then the caller's `iter` (the iteration count the finished chunk ends at), `at_check`, `chunk_done`
            and `status_in` are set, rho_flag and stage2 cleared, the block uploaded, the residual block and the chunk's PCG statistics zeroed -- a kernel
            that should idle leaves zeros -- and the group enqueued `groups` times (1 or 2) as a solve enqueues it (replayed from a captured graph where
            the handle replays graphs); then the block is read back.
     PEEK   res [OSQP_HIP_RES_COUNT] as it stands on the device (osqp_hip_res_name gives the order); rho, rho_inv, v, t0, ztg [m]; xg, xsp, Minv [n];
            tol_rel / tol_abs: the PCG tolerance scalars on the device; launches: kernel launches enqueued; form as osqp_hip_test_admm reports it.  In
            mode 1 `dev` holds the fields of the state block a boundary writes, as the device left them, and `host` the same fields of the HOST's twin: the
            host's compilation of the same rules applied `groups` times to a copy of the uploaded block, with the residual block the device produced.
   Afterwards, with keep = 0, the handle's own rho is applied again (rho vector, v, t0, preconditioner, explicit K): a later osqp_solve with
   warm_starting = 0 is a fresh handle's solve bit for bit.  With keep = 1 a rho the group changed STAYS and the handle adopts it as a device-driven solve
   does (settings.rho): the next osqp_hip_test_admm runs at the new rho.
   Every length is exact (n_len = n, m_len = m, res_len = OSQP_HIP_RES_COUNT; a NULL pointer only where the length is 0) and everything is checked before
   anything is uploaded or launched: mode, unscaled, keep, at_check, chunk_done outside {0, 1}, need outside 0 .. 3, groups outside {1, 2}, status_in
   outside 0 .. 2, iter < 0, thr negative or not finite give OSQP_DATA_VALIDATION_ERROR.  Mode 1 answers OSQP_FUNC_NOT_IMPLEMENTED on a handle without the
   slot form or without a device state block (the host simulator), and on one whose Woodbury correction is on (osqp_hip_test_woodbury is its tier). */
#define OSQP_HIP_RES_COUNT 28
typedef struct {
  OSQPInt status, osqp_status, need, stage2, rho_flag, rho_updates, iter, boundaries;
  OSQPInt ch_next, ch_at_check, ch_kind, ch_tight, budget[2];
  OSQPFloat rho_bar, rho_estimate, tol_rel, tol_abs;
  OSQPFloat obj_val, prim_res, dual_res, dual_obj_val, duality_gap, rel_kkt_error;
  OSQPFloat inf_nd_p, inf_nd_d, inf_thr_d;
  OSQPInt inf_unscaled;
} OSQPHipBoundaryCtl;
typedef struct {
  OSQPInt mode, need, unscaled, groups, keep;
  OSQPInt iter, at_check, chunk_done, status_in;                                       /* mode 1 */
  OSQPFloat thr;
  long long n_len, m_len, res_len;
  const OSQPFloat *x_in, *dx_in, *xt_in, *z_in, *y_in, *dy_in, *zt_in;
  OSQPFloat *res, *rho, *rho_inv, *v, *t0, *ztg, *xg, *xsp, *Minv;                     /* out */
  OSQPFloat tol_rel, tol_abs;                                                          /* out */
  OSQPInt launches, form;                                                              /* out */
  OSQPHipBoundaryCtl dev, host;                                                        /* out (mode 1) */
} OSQPHipBoundaryTest;
OSQPInt osqp_hip_test_boundary(OSQPSolver *solver, OSQPHipBoundaryTest *t);
/* name of entry q of the residual block ("R_PRI_U", ...), NULL outside 0 .. OSQP_HIP_RES_COUNT - 1 */
const char *osqp_hip_res_name(OSQPInt q);
/* Weight of equality rows relative to inequality rows, rho_eq = factor * rho, used when equality and inequality rows are
   mixed (default 10; the reference's 1e3 is kept when every active row is an equality).  See engine.cpp (Engine::classify_constraints)
   classify_constraints() for the rationale.  Takes effect immediately (rho vector + preconditioner are rebuilt). */
OSQPInt osqp_hip_set_rho_eq_factor(OSQPSolver *solver, OSQPFloat factor);
/* copy out internal scaling D (n), E (m), c */
OSQPInt osqp_hip_get_scaling(OSQPSolver *solver, OSQPFloat *D, OSQPFloat *E, OSQPFloat *c);
/* the permutation this handle works under (OSQPHipPolicy::reorder): perm_cols[k] (n) / perm_rows[k] (m) = the caller's index of the engine's
   k-th variable / constraint; the identity when the problem was not reordered (OSQPHipStats::reordered = 0).  Diagnostic: nothing at this
   API is expressed in the engine's numbering. */
OSQPInt osqp_hip_get_reordering(OSQPSolver *solver, OSQPInt *perm_cols, OSQPInt *perm_rows);
/* Where `verbose` output goes.  The reference's C core prints through c_print, which its Python binding maps to PySys_WriteStdout under the GIL
   (/root/reference/cmake/printing.h:2-7) while solve() runs with the GIL released (bindings.cpp.in:197-199).  Here: every line of text a handle
   prints is handed to ITS print function, or to stdout (fputs) when none is set.  osqp_hip_set_default_print installs the function handles
   created AFTERWARDS start with (osqp_setup prints the problem header before the caller holds the handle) -- the Python layer installs one that
   writes to sys.stdout (a ctypes callback takes the GIL itself); osqp_hip_set_print changes one handle's.  fn == NULL restores stdout. */
typedef void (*osqp_hip_print_fn)(const char *text, void *user);
void    osqp_hip_set_default_print(osqp_hip_print_fn fn, void *user);
OSQPInt osqp_hip_set_print(OSQPSolver *solver, osqp_hip_print_fn fn, void *user);
/* name of the compute backend compiled into this library: "hip-gfx950" for the product */
const char *osqp_hip_backend(void);

/* DENSE KKT MODE (csrc/densekkt_hip.hip): exact linear solves for a single QP of a few hundred to a few thousand variables.
   The handle holds K^-1 = (P + sigma I + A' diag(rho) A)^-1 as a dense n x n matrix on the device (8 n^2 bytes, plus 8 m n bytes of work space); an ADMM
   iteration is then three launches with an exact solve instead of a PCG.  Opt-in per handle, off by default.
     on = 1   allocates, forms and inverts K for the handle's current rho and checks the inverse (max |K^-1 K v - v| <= 1e-6 max |v| on a probe vector).
              Synchronous: the inverse is in place when the call returns.  Every later change of rho (adaptive updates inside osqp_solve, osqp_update_rho),
              of the matrix values (osqp_update_data_mat) or of the bounds (osqp_update_data_vec with l / u: the constraint classes decide rho_i)
              factorises again.  Polish and the adjoint derivatives run on the PCG path as without the mode; the inverse is re-formed behind them.
              OSQP_FUNC_NOT_IMPLEMENTED -- the handle is left untouched, nothing is allocated -- on a backend without the mode, on a handle with a
              Woodbury correction (it has its own direct modes), without device-side assembly, with m = 0, with n > OSQP_HIP_DENSE_KKT_MAX_N or with
              m n > 2^25 (the work matrix).  OSQP_MEM_ALLOC_ERROR when the device has no room.  A reordered handle (OSQPHipPolicy::reorder) is served.
     on = 0   frees everything; from the next solve on the handle computes what a handle computes on which the mode was never enabled.
   The batch and lockstep entry points do not consult the mode.  osqp_hip_dense_kkt_last_record copies OSQP_HIP_DENSE_KKT_REC doubles:
     0 state      0 off; 1 K^-1 accepted: the solves run direct (OSQPHipStats::pcg_iters_total = 0); 2 enabled, but the inverse for the current rho was
                  refused (a pivot <= 0, or the probe above 1e-6): the handle runs its ordinary PCG path until a later factorisation is accepted
     1 order      n (0 while off)
     2, 3         factorisations during the last osqp_solve, their wall-clock milliseconds
     4, 5         probe value and smallest pivot of the last inversion
     6            device bytes the mode holds
     7            factorisations since the mode was enabled */
#define OSQP_HIP_DENSE_KKT_MAX_N 1000    /* the largest size of the sweep in DESIGN.md section 6 at which the mode is slower on neither family (it began at 4096) */
#define OSQP_HIP_DENSE_KKT_REC 8
OSQPInt osqp_hip_dense_kkt(OSQPSolver *solver, OSQPInt on);
OSQPInt osqp_hip_dense_kkt_last_record(OSQPSolver *solver, OSQPFloat *rec);
/* Test hook (used by tests/ only): the mode's kernels on a handle with the mode ON (else OSQP_FUNC_NOT_IMPLEMENTED).  Everything is in the SCALED problem
   (osqp_hip_get_scaling) and in the ENGINE's numbering (osqp_hip_get_reordering).  Synchronous.
     op OSQP_HIP_DK_FORM    factorises as a rho update does and copies out  K [n^2 + 16]  row-major AS FORMED, before the inversion, and  rho [m + 16], the
                            vector it was formed with.  Not counted in the record's factorisations.
     op OSQP_HIP_DK_APPLY   the hot path on the caller's  r [n]  (r_0) and  xg [n]  (x_g):  xs [n + 16] = x~ = x_g + K^-1 r_0,  u [n + 16] = K^-1 r_0,  done /
                            iters: the PCG's flags as the launch leaves them.  Needs state 1.
     op OSQP_HIP_DK_PROBE   the probe alone against the inverse in place: probe.
   Of an output exactly the listed count is written (the 16 cells behind it keep the caller's values); a field an op does not list has length 0.  Every
   vector of the handle the call overwrites is restored before it returns: a solve after the call is the solve without it.  Every length and pointer
   is checked before anything is launched (anything else than listed: OSQP_DATA_VALIDATION_ERROR). */
enum { OSQP_HIP_DK_FORM = 0, OSQP_HIP_DK_APPLY = 1, OSQP_HIP_DK_PROBE = 2 };
typedef struct {
  OSQPInt op;
  long long r_len, xg_len, k_len, rho_len, xs_len, u_len;
  const OSQPFloat *r, *xg;
  OSQPFloat *K, *rho, *xs, *u;
  OSQPInt state, order, done, iters;   /* out */
  OSQPFloat probe, minpiv;             /* out */
} OSQPHipDenseKktTest;
OSQPInt osqp_hip_test_dense_kkt(OSQPSolver *solver, OSQPHipDenseKktTest *t);

#ifdef __cplusplus
}
#endif
#endif /* OSQP_HIP_H */
