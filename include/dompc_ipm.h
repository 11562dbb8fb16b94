/*
 * dompc_ipm.h - C ABI of the MI355X-native structured interior-point backend that replaces
 * the `nlpsol('ipopt', ...)` call on do-mpc's MPC.make_step() path.
 *
 * Reference interfaces replaced (paths relative to the do-mpc source tree):
 *   do_mpc/controller/_mpc.py:1326-1328   self.S = castools.nlpsol('S', 'ipopt', nlp, opts)   -> dompc_create
 *   do_mpc/optimizer.py:754-770           r = self.S(x0=, lbx=, ubx=, lbg=, ubg=, p=, ...)    -> dompc_solve
 *   do_mpc/optimizer.py:772-778           r['x'], r['g'], r['lam_g'], r['lam_x'], S.stats()   -> outputs + dompc_stats
 *   do_mpc/sampling/_sampler.py:198-228   one make_step per sample, fanned out by processes   -> dompc_solve_batch*
 * The NLP itself is *not* passed as a symbolic graph: the model functions were lowered to a
 * gfx950 code object at setup() (do_mpc_amd/lowering.py) and the multi-stage structure
 * (do_mpc/optimizer.py:998-1048, do_mpc/controller/_mpc.py:1126-1245) is described by the
 * integer tables below.
 *
 * Conventions
 *   - all vectors are contiguous float64 in the reference's canonical order (opt_x, opt_p, g);
 *   - multipliers follow CasADi's sign convention  L = f + lam_g'g + lam_x'x;
 *   - return code 0 = ok, != 0 = infrastructure error (HIP, allocation, bad argument); the text is
 *     available from dompc_last_error().  Solver non-convergence is NOT an error: it is reported
 *     in dompc_stats.success / return_status, results are still written (matches optimizer.py:770-778);
 *   - the caller owns every buffer it passes; the library owns device memory, streams and the loaded
 *     code object inside the handle; a handle is not thread-safe, distinct handles are independent;
 *   - create the handle after fork(): no HIP state is touched before dompc_create().
 */
#ifndef DOMPC_IPM_H
#define DOMPC_IPM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dompc_handle dompc_handle;

/* IPOPT-named algorithm options (defaults = IPOPT 3.14 defaults, see dompc_default_options). */
typedef struct dompc_options {
  double tol;                /* ipopt.tol                      1e-8  */
  double dual_inf_tol;       /* ipopt.dual_inf_tol             1.0   */
  double constr_viol_tol;    /* ipopt.constr_viol_tol          1e-4  */
  double compl_inf_tol;      /* ipopt.compl_inf_tol            1e-4  */
  double acceptable_tol;     /* ipopt.acceptable_tol           1e-6  */
  double mu_init;            /* ipopt.mu_init                  0.1   */
  double kappa_mu;           /* mu_linear_decrease_factor      0.2   */
  double theta_mu;           /* mu_superlinear_decrease_power  1.5   */
  double kappa_eps;          /* barrier_tol_factor             10    */
  double tau_min;            /* ipopt.tau_min                  0.99  */
  double bound_push;         /* ipopt.bound_push               0.01  */
  double bound_frac;         /* ipopt.bound_frac               0.01  */
  double bound_relax_factor; /* ipopt.bound_relax_factor       1e-8  */
  double nlp_scaling_max_gradient; /*                          100   */
  double delta_w_0;          /* first_hessian_perturbation     1e-4  */
  double delta_w_min;        /* min_hessian_perturbation       1e-20 */
  double delta_w_max;        /* max_hessian_perturbation       1e20  */
  double kappa_w_minus;      /* perturb_dec_fact               1/3   */
  double kappa_w_plus;       /* perturb_inc_fact               8     */
  double kappa_w_plus_bar;   /* perturb_inc_fact_first         100   */
  int32_t max_iter;          /* ipopt.max_iter                 3000  */
  int32_t acceptable_iter;   /* ipopt.acceptable_iter          15    */
  int32_t obj_scaling;       /* gradient-based objective scaling on/off (1) */
  int32_t max_soc;           /* ipopt.max_soc: second-order correction attempts per iteration   4 (0 = off) */
  double constr_mult_init_max; /* ipopt.constr_mult_init_max: least-squares multiplier estimate at the starting point,
                                  discarded if its max-norm is above this value   1000 (0 = start from lambda = 0);
                                  models with nl_cons rows always start from lambda = 0 */
  int32_t watchdog_shortened_iter_trigger; /* ipopt.watchdog_shortened_iter_trigger: consecutive iterations with a shortened step
                                              after which the watchdog procedure starts   10 (0 = off) */
  int32_t watchdog_trial_iter_max;         /* ipopt.watchdog_trial_iter_max: full steps it may take without the filter   3 */
} dompc_options;

/* Description of one multi-stage problem class (fixed at MPC.setup()). All pointers are host
 * pointers and are copied by dompc_create(). */
typedef struct dompc_problem_desc {
  int32_t nx, nu, np, ntvp, ne, ns;     /* model dims; ne = nl_cons rows/edge, ns = slacks/(stage,scenario) */
  int32_t deg, ni, M;                   /* collocation; M = ni*(deg+1) stored slots, 0 = discrete model     */
  int32_t N;                            /* horizon                                                         */
  int32_t n_opt_x, n_opt_p, n_g;        /* canonical vector sizes                                          */
  int32_t n_nodes, n_edges, n_dummy;
  int32_t p_off_tvp, p_off_p, p_off_uprev; /* offsets inside opt_p (= [_x0 ; _tvp ; _p ; _u_prev])       */
  const int32_t* level_node_start;      /* [N+2]  nodes are ordered by (stage k, scenario s)               */
  const int32_t* node_level;            /* [n_nodes]                                                       */
  const int32_t* node_x_off;            /* [n_nodes] offset of _x[k,s,-1] in opt_x                          */
  const int32_t* node_u_off;            /* [n_nodes] offset of _u[k,s]   (-1 at stage N)                    */
  const int32_t* node_eps_off;          /* [n_nodes] offset of _eps[k,s] (-1 if none)                       */
  const int32_t* node_child_start;      /* [n_nodes] first outgoing edge                                   */
  const int32_t* node_child_count;      /* [n_nodes]                                                       */
  const int32_t* node_parent;           /* [n_nodes] parent node (-1 root)                                 */
  const int32_t* node_in_edge;          /* [n_nodes] incoming edge (-1 root)                                */
  const int32_t* edge_parent;           /* [n_edges]                                                       */
  const int32_t* edge_child;            /* [n_edges]                                                       */
  const int32_t* edge_pidx;             /* [n_edges] row of opt_p['_p'] used on this edge                   */
  const int32_t* edge_w_off;            /* [n_edges] offset of _x[k+1,c,0] (collocation slots of the edge)  */
  const int32_t* edge_row0;             /* [n_edges] first constraint row of the edge in g                  */
  const int32_t* edge_level;            /* [n_edges] stage k of the parent                                  */
  const double*  edge_omega;            /* [n_edges] scenario weight 1/n_scenarios[k+1]                     */
  const int32_t* dummy_idx;             /* [n_dummy] opt_x entries used by no constraint/cost               */
  const char*    code_object_path;      /* gfx950 code object built from the lowered model                  */
  const char*    model_hash;            /* must equal the hash embedded in the code object                  */
  int32_t device;                       /* HIP device ordinal                                              */
  int32_t max_batch;                    /* largest batch that will be passed to *_batch calls               */
  int32_t n_slots;                      /* concurrent problem slots (workgroups); 0 = what the device keeps resident */
  int32_t block_threads;                /* threads per problem in batch mode: 64, 128 or 256; 0 = choose from max_batch */
  dompc_options opts;
} dompc_problem_desc;

typedef struct dompc_stats {
  int32_t success;          /* 1 = converged to tol (or acceptable level)                                  */
  int32_t status;           /* 0 Solve_Succeeded, 1 Solved_To_Acceptable_Level, 2 Maximum_Iterations_Exceeded,
                               3 Error_In_Step_Computation, 4 Invalid_Number_Detected, 5 Internal_Error (a peer
                               workgroup / rank never arrived), 6 User_Requested_Stop (dompc_abort / watchdog)  */
  int32_t iter_count;
  int32_t n_reg;            /* iterations that needed Hessian regularisation                               */
  int32_t n_ls_fail;        /* line searches that hit alpha_min (no restoration phase)                     */
  int32_t n_sweeps;         /* derivative sweeps executed (model evaluation + condensing of every edge)        */
  int32_t n_trials;         /* function-only trial sweeps of the line search                                 */
  int32_t n_soc;            /* second-order correction solves (each one more sweep + Riccati pass)            */
  int32_t n_watchdog;       /* watchdog procedures started (IPOPT: watchdog_shortened_iter_trigger)            */
  int32_t reserved0;
  double  mu;
  double  obj;              /* unscaled objective                                                          */
  double  inf_pr, inf_du, inf_compl; /* scaled errors at exit                                                  */
  double  obj_scaling;
  double  t_wall_total;     /* filled by the host side: wall time of the call / batch                      */
} dompc_stats;

void dompc_default_options(dompc_options* opts);

int  dompc_create(const dompc_problem_desc* desc, dompc_handle** out);
void dompc_destroy(dompc_handle* h);
const char* dompc_last_error(const dompc_handle* h);   /* h may be NULL: error of the last failed create */
const char* dompc_status_string(int32_t status);

/* One solve, host buffers (what Optimizer.solve does). lam_x0/lam_g0 may be NULL (they are ignored,
 * like IPOPT with warm_start_init_point=no). Any output pointer may be NULL. */
int dompc_solve(dompc_handle* h,
                const double* x0, const double* lbx, const double* ubx,
                const double* lbg, const double* ubg, const double* p,
                const double* lam_x0, const double* lam_g0,
                double* x, double* g, double* lam_x, double* lam_g, double* f,
                dompc_stats* stats);

/* B independent solves, host buffers.  x0 and p are [B][n]; bounds are shared by the batch. */
int dompc_solve_batch(dompc_handle* h, int32_t B,
                      const double* x0, const double* lbx, const double* ubx,
                      const double* lbg, const double* ubg, const double* p,
                      double* x, double* g, double* lam_x, double* lam_g, double* f,
                      dompc_stats* stats);

/* Same with DEVICE buffers (inputs already resident in HBM), asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = default stream).  stats is a device pointer [B]. */
int dompc_solve_batch_device(dompc_handle* h, int32_t B,
                             const double* x0, const double* lbx, const double* ubx,
                             const double* lbg, const double* ubg, const double* p,
                             double* x, double* g, double* lam_x, double* lam_g, double* f,
                             dompc_stats* stats, void* stream);

/* Model-evaluation sweep only (the "Jacobian sweep" of the IPM iteration): for B iterates evaluate
 * g(x), and per edge the linearised dynamics [A|B], c and the condensed Lagrangian-Hessian block.
 * DEVICE buffers: x [B][n_opt_x], lam [B][n_g], p [B][n_opt_p]; outputs g [B][n_g],
 * blocks [B][n_edges][dompc_sweep_block_doubles()] (may be NULL: the sweep runs, only g is copied out - the
 * sweep-only roofline of bench.py).  Launched in the shape of dompc_solve_batch_device for the same B.
 * Used for roofline measurement and parity. */
int dompc_sweep_batch_device(dompc_handle* h, int32_t B,
                             const double* x, const double* lam, const double* p,
                             double* g, double* blocks, void* stream);
int64_t dompc_sweep_block_doubles(const dompc_handle* h);

/* Debug/parity entry: one Newton direction at (x, lam_g, z_l, z_u, mu) exactly as given (no push,
 * no scaling).  Host buffers.  dx [n_opt_x], dlam [n_g].  delta_w = primal regularisation to apply. */
int dompc_debug_newton_step(dompc_handle* h,
                            const double* x, const double* lam_g, const double* zl, const double* zu,
                            const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                            const double* p, double mu, double delta_w,
                            double* dx, double* dlam, double* rd, double* c);

/* Newton direction of the primal-dual system at a CONVERGED point of the barrier problem (x, lam_g, z_l, z_u at barrier
 * parameter mu; bounds as the solver relaxed them): like dompc_debug_newton_step, but the slack variables of the nl_cons
 * rows take their values at the point (s = d(x), multipliers mu / distance to the relaxed row bounds) instead of the pushed
 * starting values.  The building block of the parametric sensitivities (do_mpc/differentiator/_nlpdifferentiator.py:
 * 792-841 solves the same system densely): dv/dp_j = [d(p + h e_j) - d(p)] / h.  Host buffers. */
int dompc_newton_step_at_solution(dompc_handle* h,
                                  const double* x, const double* lam_g, const double* zl, const double* zu,
                                  const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                  const double* p, double mu, double* dx, double* dlam);

/* The same for B parameter vectors p (row-major B x n_opt_p) at ONE point: one workgroup per vector, B directions in one launch
 * (dx: B x n_opt_x, dlam: B x n_g) - all columns of a sensitivity matrix at once (do_mpc_amd/differentiator.py; the reference
 * factorises the dense KKT matrix once and solves for all right-hand sides, _nlpdifferentiator.py:792-841). */
int dompc_newton_steps_at_solution(dompc_handle* h, int32_t B,
                                   const double* x, const double* lam_g, const double* zl, const double* zu,
                                   const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                   const double* p, double mu, double* dx, double* dlam);

/* Iteration trace of problem 0 of the last solve: rows of 8 doubles (it, mu, E0, inf_pr, inf_du,
 * +-alpha (negative: line search failed), delta_w, obj). */
int dompc_debug_get_trace(dompc_handle* h, double* out, int32_t max_rows);

/* The launch shape of a solve as a function of plain values: the decision dompc_solve_batch_device makes for a batch of B problems
 * (do_mpc_amd/csrc/dompc_shape.h), without a handle and without a device - what tests/test_launch_shape.py pins.
 * facts: what a handle knows after dompc_create; overrides: what DOMPC_WIDE / DOMPC_WIDE_SPREAD / DOMPC_WIDE_BLOCK ask for.
 * Returns 1 on a null pointer or B < 1. */
typedef struct dompc_shape_facts {
  int32_t n_edges, n_leaves;     /* edges of the scenario tree, nodes of its last stage                                  */
  int32_t edges_per_wave;        /* dompc_edges_per_wavefront                                                            */
  int64_t el_size;               /* doubles of LDS per wavefront (one edge working set)                                  */
  int32_t slots64, slots256;     /* resident workgroups of the solver kernel at 64 / at (up to) 256 threads              */
  int32_t n_slots;               /* workspace slots of the handle                                                        */
  int32_t block, block_auto;     /* threads per problem of a batch; 1 = chosen per call from the batch size instead      */
  int32_t sharded;               /* 1 = tree sharding is on (dompc_set_sharding)                                         */
} dompc_shape_facts;
typedef struct dompc_shape_overrides {
  int32_t wide;                  /* workgroups per problem, -1 = not set                                                 */
  int32_t wide_spread;           /* 0 / 1, -1 = not set                                                                  */
  int32_t wide_block;            /* threads per workgroup of the wide mode (64/128/256/512), 0 = not set                 */
} dompc_shape_overrides;
typedef struct dompc_shape {
  int32_t block, grid;           /* threads per workgroup, workgroups                                                    */
  int32_t wide, wide_spread;     /* workgroups per problem (1 = one each) and whether they are spread over the XCDs      */
} dompc_shape;
int dompc_launch_shape(const dompc_shape_facts* facts, const dompc_shape_overrides* overrides, int32_t B, dompc_shape* out);

/* Stop request: running and queued solves of this handle leave their IPM loop at the next iteration and report
 * status 6 (User_Requested_Stop, success = 0); may be called from another thread while a solve is in flight.
 * stop = 0 re-arms the handle.  The blocking entry points (dompc_solve, dompc_solve_batch, the service loop of a
 * sharded solve) raise it themselves when the device has not finished within the watchdog time (environment
 * variable DOMPC_WATCHDOG_S, default 600 s) and return an error if the kernel does not react. */
int dompc_abort(dompc_handle* h, int32_t stop);

int64_t dompc_workspace_bytes(const dompc_handle* h);
int32_t dompc_num_slots(const dompc_handle* h);

/* ---- tree sharding of ONE problem over several ranks / GPUs --------------------
 * Replaces nothing in the reference (IPOPT/MUMPS is single-process); it is the multi-GPU path the
 * north star asks for: the sub-trees below `cut_level` of the scenario tree built by
 * do_mpc/optimizer.py:998-1048 (_setup_scenario_tree) go to the ranks in contiguous blocks, the stages
 * above are replicated, and the ranks exchange (a) the condensed contributions of the cut edges to
 * their parent nodes in the Riccati recursion and (b) the scalar reductions of the IPM (norms, step
 * sizes, filter quantities) - all as element-wise SUMs over a small exchange buffer.
 * The collective itself is supplied by the caller (RCCL all-reduce through torch.distributed in
 * do_mpc_amd/solver.py): `allreduce(ctx, buf, count)` must return when buf[0..count) holds the sum
 * over all ranks.  While a sharded solve runs the library serves the kernel's exchange requests from
 * the calling thread, so dompc_solve* returns only when the solve is finished.
 * Masks (host arrays, copied): 0 = another rank's, 1 = mine, 2 = replicated on every rank. */
typedef void (*dompc_allreduce_fn)(void* ctx, double* buf, int32_t count);
typedef struct dompc_shard_desc {
  int32_t rank, world, cut_level, n_cut;
  const int8_t* x_mask;      /* n_opt_x */
  const int8_t* g_mask;      /* n_g */
  const int8_t* edge_mask;   /* n_edges */
  const int8_t* node_mask;   /* n_nodes */
  const int32_t* node_cut;   /* n_nodes: index of a cut parent among the cut parents, else -1 */
  double* xbuf;              /* exchange buffer, DEVICE memory owned by the caller */
  int64_t xbuf_doubles;      /* its length; must be >= dompc_exchange_doubles(h, world, n_cut) */
  dompc_allreduce_fn allreduce;
  void* ctx;
} dompc_shard_desc;
/* Native collective: with allreduce == NULL in dompc_shard_desc the runtime calls RCCL itself
 * (ncclAllReduce, double, sum, on its own communicator and stream) from the service loop - no Python in the
 * exchange path.  The library is opened with dlopen (pass the path of the librccl already loaded in the process,
 * e.g. torch/lib/librccl.so, so that one copy is used).  Rank 0 creates the 128-byte unique id, the caller
 * distributes it (any transport), every rank joins with dompc_rccl_init before dompc_set_sharding. */
int dompc_rccl_unique_id(dompc_handle* h, const char* librccl_path, uint8_t id[128]);
int dompc_rccl_init(dompc_handle* h, const char* librccl_path, const uint8_t id[128], int32_t rank, int32_t world);

/* doubles the exchange buffer needs for (world, n_cut) */
int64_t dompc_exchange_doubles(const dompc_handle* h, int32_t world, int32_t n_cut);
/* desc == NULL switches sharding off again */
int dompc_set_sharding(dompc_handle* h, const dompc_shard_desc* desc);
/* exchanges (element-wise SUMs over the exchange buffer) the last sharded solve asked for; divided by its iteration count:
 * the collectives per interior-point iteration */
int64_t dompc_last_exchange_count(const dompc_handle* h);
/* the launch-shape-specific sibling code object `<name>_batch.hsaco` of the handle: 0 = none next to the general object, 1 = loaded and
 * launched for batches of one wavefront per problem, 2 = found but built from other sources or for another model - not used */
int dompc_batch_object_state(const dompc_handle* h);
/* edges a wavefront handles at a time in the derivative sweep of this model class: 4 = the quad sweep (csrc/dompc_quad.h: single finite
 * element, no nl_cons rows, at most 14 stage variables), 1 = the wavefront-per-edge paths */
int dompc_edges_per_wavefront(const dompc_handle* h);
/* backward Riccati pass of this model class as the code object reports it: 1 = the matrix-core recursion on one 16x16 tile per node
 * (csrc/dompc_riccati16.h: at most 16 node variables, 4 decision variables and 4 nl_cons rows per node), 0 = the generic recursion */
int dompc_riccati_kind(const dompc_handle* h);

/* ---- batched plant integration ---------------------------------------------------------
 * Replaces the integrator object of do_mpc.simulator.Simulator (do_mpc/simulator.py:381-416:
 * casadi.integrator('simulator', 'cvodes', dae, t0, t_step, {abstol, reltol}); discrete models: the `simulator`
 * Function of simulator.py:363-378) and its call in Simulator.make_step (simulator.py:757-850): x, u, tvp, p, w in,
 * x_next and y = meas(x_next, u, tvp, p) + v out, in physical units - for B samples at once, one GPU thread per sample,
 * so that an x0 batch stays resident in HBM between the controller's make_step calls.  The model's right-hand side and
 * measurement function come from a per-model gfx950 code object (do_mpc_amd/lowering.py:lower_plant).
 * Methods (dompc_plant_set_method): explicit Dormand-Prince 5(4) and the implicit SDIRK 4(3) of Hairer & Wanner, both with
 * per-sample step-size control (local error at 1/100 of abstol / reltol); default 0 = explicit, a sample that needs more than
 * `explicit_limit` explicit steps (stiff) repeats its interval with the implicit method - CVODES / IDAS of the reference are
 * implicit.  Algebraic states (semi-explicit index-1 DAE): solved for by Newton's method inside every right-hand-side
 * evaluation, per-sample start values carried from call to call (seed: dompc_plant_set_z0, the reference's
 * simulator.set_initial_guess / sim_z_num, simulator.py:603-620).  status[b]: bit 0 = step limit reached, NaN right-hand
 * side or a failed algebraic / stage solve (x_next is the state reached so far), bit 1 = the implicit method produced the
 * result, steps taken = status[b] >> 8.
 * shared_mask: bit 0/1/2/3/4 set = u/tvp/p/w/v is ONE row shared by all samples instead of [B][n]. */
typedef struct dompc_plant dompc_plant;
typedef struct dompc_plant_desc {
  int32_t nx, nu, np, ntvp, nw, nv, ny;
  int32_t discrete;                  /* 1: x_next = rhs(x, u, tvp, p, w) (no integration)                     */
  const char* code_object_path;      /* gfx950 code object built from the lowered plant                       */
  const char* model_hash;            /* must equal the hash embedded in the code object (NULL = no check)      */
  int32_t device;
  int32_t max_steps;                 /* per sample and call; 0 = 200000                                        */
  double t_step, reltol, abstol;     /* settings.t_step / reltol / abstol of the reference's SimulatorSettings */
} dompc_plant_desc;
int  dompc_plant_create(const dompc_plant_desc* desc, dompc_plant** out);
void dompc_plant_destroy(dompc_plant* h);
/* method: 0 explicit with implicit repeat for stiff samples (default), 1 explicit only, 2 implicit only;
 * explicit_limit: explicit steps per interval after which a sample counts as stiff (0 = keep, default 4000) */
int  dompc_plant_set_method(dompc_plant* h, int32_t method, int32_t explicit_limit);
/* algebraic states: their number, and the Newton start for every sample (host array of that many values, NULL = zeros).
 * Carry-over: ROW b of a call continues from the values row b found at the end of the previous call - meaningful only when the rows of
 * consecutive calls are the same trajectories.  dompc_plant_step_batch_device (resident closed loops) always carries; the host entry
 * dompc_plant_step_batch starts every call from z0 unless dompc_plant_set_z_carry(h, 1) says its rows correspond across calls
 * (Simulator.make_step: one trajectory).  A batch larger than any before starts all rows from z0. */
int32_t dompc_plant_num_alg_states(const dompc_plant* h);
int  dompc_plant_set_z0(dompc_plant* h, const double* z0);
int  dompc_plant_set_z_carry(dompc_plant* h, int32_t on);
const char* dompc_plant_last_error(const dompc_plant* h);     /* h may be NULL: error of the last failed create */
/* host buffers; w, v, y, status may be NULL */
int dompc_plant_step_batch(dompc_plant* h, int32_t B, const double* x, const double* u, const double* tvp, const double* p,
                           const double* w, const double* v, int32_t shared_mask, double* x_next, double* y, int32_t* status);
/* DEVICE buffers, asynchronous on `stream` (hipStream_t as void*) */
int dompc_plant_step_batch_device(dompc_plant* h, int32_t B, const double* x, const double* u, const double* tvp,
                                  const double* p, const double* w, const double* v, int32_t shared_mask, double* x_next,
                                  double* y, int32_t* status, void* stream);

/* ---- batched extended Kalman filter (do_mpc.estimator.EKF) ----------------------------------------------------------
 * One filter step - prediction and measurement update - for B independent filters per launch, in physical units:
 *   A_k, C_k at the prior estimate;  discrete models x- = rhs(x, u), P- = A P A' + Q;  continuous models [x; P] integrated over
 *   t_step with dP/dt = A(x) P + P A(x)' + Q (explicit Dormand-Prince 5(4), step-size control per filter, no implicit method);
 *   S = C P- C' + R, L = P- C' S^-1, x = x- + L (y - meas(x-, u)), P = (I - L C) P-.
 * The model functions come from a per-model gfx950 code object (do_mpc_amd/lowering.py:lower_ekf); at most 16 states and 16
 * measurements.  Layout: x [B][nx], P [B][nx][nx] row-major, y [B][ny]; u / tvp / p / Q (nx*nx) / R (ny*ny)
 * are [B][n] or, with their bit of shared_mask set (bit 0/1/2/3/4 = u/tvp/p/Q/R), ONE row shared by all filters.
 * status[b]: bit 0 = the integration did not reach t_step (step limit, NaN right-hand side); bit 1 = S singular or not finite - the
 * a-priori x-, P- are returned, never NaN; integration steps taken = status[b] >> 8.
 * Models with algebraic states (nz > 0, at most 16; x' = f(x, u, z), 0 = g(x, u, z), y = h(x, u, z)): the same filter on the reduced
 * system z = zeta(x, u), through the entries dompc_ekf_step_dae_batch[_device].  Before every evaluation of the model Newton solves
 * g = 0 for z (until max |g| <= z_tol, at most z_max_iter updates per solve, warm-started from the previous solve and first from the
 * guess z [B][nz]); A = f_x - f_z g_z^-1 g_x and C = h_x - h_z g_z^-1 g_x take the place of A and C.  z_out: the algebraic states
 * consistent with the a-priori state x- (the last solve of the step: the warm start of the next call); newton[b]: Newton updates
 * of filter b.  status bit 2 = a Newton iteration did not converge, or g_z was singular or not finite (with bit 0 when this happens
 * during the integration): that filter hands back its prior x, P and its guess z unchanged.  The two entries without z run such a
 * handle from the guess 0 and hand no z back. */
typedef struct dompc_ekf dompc_ekf;
typedef struct dompc_ekf_desc {
  int32_t nx, nu, np, ntvp, ny;
  int32_t discrete;                  /* 1: x- = rhs(x, u, tvp, p) (no integration)                             */
  const char* code_object_path;      /* gfx950 code object built from the lowered filter                       */
  const char* model_hash;            /* must equal the hash embedded in the code object (NULL = no check)      */
  int32_t device;
  int32_t max_steps;                 /* integration steps per filter and call; 0 = 200000                      */
  double t_step, reltol, abstol;
  int32_t nz;                        /* algebraic states of the model (0: an ODE model)                       */
  int32_t z_max_iter;                /* Newton updates per solve of g = 0; 0 = 20                              */
  double z_tol;                      /* Newton stops at max |g| <= z_tol; 0 = 1e-10                            */
} dompc_ekf_desc;
int  dompc_ekf_create(const dompc_ekf_desc* desc, dompc_ekf** out);
void dompc_ekf_destroy(dompc_ekf* h);
const char* dompc_ekf_last_error(const dompc_ekf* h);         /* h may be NULL: error of the last failed create */
/* host buffers; status may be NULL.  x_out / P_out may alias x / P. */
int dompc_ekf_step_batch(dompc_ekf* h, int32_t B, const double* x, const double* P, const double* y, const double* u,
                         const double* tvp, const double* p, const double* Q, const double* R, int32_t shared_mask,
                         double* x_out, double* P_out, int32_t* status);
/* DEVICE buffers, x and P updated IN PLACE, asynchronous on `stream` (hipStream_t as void*) */
int dompc_ekf_step_batch_device(dompc_ekf* h, int32_t B, double* x, double* P, const double* y, const double* u,
                                const double* tvp, const double* p, const double* Q, const double* R, int32_t shared_mask,
                                int32_t* status, void* stream);
/* ... for a model with algebraic states: z [B][nz] the guess (NULL = 0); z_out (may alias z) and newton may be NULL.  z_out is written
 * only when z is given: without a guess nothing is handed back (as on the device, where z is both) */
int dompc_ekf_step_dae_batch(dompc_ekf* h, int32_t B, const double* x, const double* P, const double* y, const double* u,
                             const double* z, const double* tvp, const double* p, const double* Q, const double* R,
                             int32_t shared_mask, double* x_out, double* P_out, double* z_out, int32_t* newton, int32_t* status);
/* DEVICE buffers; z is updated IN PLACE like x and P (NULL: guess 0, nothing handed back) */
int dompc_ekf_step_dae_batch_device(dompc_ekf* h, int32_t B, double* x, double* P, const double* y, const double* u, double* z,
                                    const double* tvp, const double* p, const double* Q, const double* R, int32_t shared_mask,
                                    int32_t* newton, int32_t* status, void* stream);

/* ---- batched LQR design (csrc/dompc_lqr.hip): what do_mpc.controller.LQR.setup computes - the discrete Riccati solution and the gain
 * K = -(B'PB + R)^-1 B'PA - for B designs per launch, on an infinite horizon (structure-preserving doubling iteration) or over
 * n_horizon passes of the backward recursion (the K of the LAST pass, like the reference).  A code object WITHOUT a model reads the
 * discrete pairs A [B][nx][nx], B [B][nx][nu]; one WITH a model linearises the model at (x, u, tvp, p), discretises a continuous one
 * by zero-order hold over t_step and writes the discrete pairs.  rate != 0: inputRatePenalization mode, design size n = nx + nu with
 * A~ = [[A, B], [0, I]], B~ = [[B], [I]]; otherwise n = nx.  n <= 16, nu <= 16.  Q [n][n], R [nu][nu], Pf [n][n] (terminal weight, finite
 * horizon only) are in DESIGN size, per design or - with their bit of shared_mask set (bit 0/1/2/3/4 = Q/R/Pf/tvp/p) - ONE shared.
 * status[b]: bit 0 = the doubling did not converge within max_iter; bit 1 = a singular or non-finite block, K = 0 and P = Q are
 * returned, never NaN; iterations / passes = status[b] >> 8. */
typedef struct dompc_lqr dompc_lqr;
typedef struct dompc_lqr_desc {
  int32_t nx, nu, n, rate, has_model, discrete, np, ntvp;
  const char* code_object_path;      /* gfx950 code object built from the lowered design                        */
  const char* model_hash;            /* LQR_MODEL_HASH of the header the code object was built from            */
  int32_t device;
  int32_t n_horizon;                 /* 0: infinite horizon                                                     */
  int32_t max_iter;                  /* doubling steps; 0 = 50                                                  */
  double t_step, tol;                /* tol: relative change of H that ends the doubling; 0 = 1e-13             */
  int32_t nz;                        /* algebraic states of the model (0: none; at most 16)                    */
  int32_t z_max_iter;                /* Newton updates on g = 0; 0 = 20, at most 127                            */
  double z_tol;                      /* Newton stops at max |g| <= z_tol; 0 = 1e-10                             */
} dompc_lqr_desc;
int  dompc_lqr_create(const dompc_lqr_desc* desc, dompc_lqr** out);
void dompc_lqr_destroy(dompc_lqr* h);
const char* dompc_lqr_last_error(const dompc_lqr* h);         /* h may be NULL: error of the last failed create */
/* host buffers; arrays the design does not read and outputs that are not wanted (A_out, B_out, status) may be NULL */
int dompc_lqr_design_batch(dompc_lqr* h, int32_t B, const double* A, const double* Bm, const double* x, const double* u,
                           const double* tvp, const double* p, const double* Q, const double* R, const double* Pf,
                           int32_t shared_mask, double* K_out, double* P_out, double* A_out, double* B_out, int32_t* status);
/* DEVICE buffers, asynchronous on `stream` (hipStream_t as void*); with a model A / Bm are outputs and may be NULL */
int dompc_lqr_design_batch_device(dompc_lqr* h, int32_t B, double* A, double* Bm, const double* x, const double* u,
                                  const double* tvp, const double* p, const double* Q, const double* R, const double* Pf,
                                  int32_t shared_mask, double* K, double* P, int32_t* status, void* stream);
/* ... for a model with algebraic states (desc.nz > 0; x' = f(x, u, z), 0 = g(x, u, z)): the design of the reduced system
 * x' = f(x, u, zeta(x, u)) in the same launch - Newton on g = 0 from the guess z [B][nz], g_z [Z_x Z_u] = [g_x g_u],
 * A = f_x - f_z Z_x, B = f_u - f_z Z_u, then as above.  z_out / Z_out [B][nz] (may be NULL) receive the consistent algebraic states.
 * status bit 2 = Newton did not converge, or g_z singular or not finite at the last iterate (K = 0, P = Q, A = B = 0); iterations
 * = (status >> 8) & 0xFFFF, Newton updates = status >> 24. */
int dompc_lqr_design_dae_batch(dompc_lqr* h, int32_t B, const double* x, const double* u, const double* z, const double* tvp,
                               const double* p, const double* Q, const double* R, const double* Pf, int32_t shared_mask,
                               double* K_out, double* P_out, double* A_out, double* B_out, double* Z_out, int32_t* status);
int dompc_lqr_design_dae_batch_device(dompc_lqr* h, int32_t B, double* A, double* Bm, const double* x, const double* u,
                                      const double* z, const double* tvp, const double* p, const double* Q, const double* R,
                                      const double* Pf, int32_t shared_mask, double* K, double* P, double* z_out, int32_t* status,
                                      void* stream);
/* ... time-varying LQR along B trajectories of K steps (dompc_lqr_pairs_kernel, dompc_lqr_tv_kernel): one backward recursion
 * K_k = -(B_k'PB_k + R)^-1 B_k'PA_k, P <- Q + A_k'P(A_k + B_k K_k) from P = Pf over k = K-1 .. 0, a pair and a gain per step.  The
 * horizon is K: desc.n_horizon is not read.  All trajectory arrays are STEP-MAJOR: x_traj [K][B][nx], u_traj [K][B][nu], z0 / z_out
 * [K][B][nz], A_traj [K][B][nx][nx], B_traj [K][B][nx][nu], K_traj [K][B][nu][n], P_traj [K+1][B][n][n] (entry K is Pf), P0 [B][n][n].
 * pairs: needs a code object WITH a model; the pair of knot (k, b) is what dompc_lqr_design_batch forms at that point (Jacobians
 * frozen at the knot, zero-order hold over t_step for a continuous model, reduction of algebraic states).  tvp is [K][ntvp] with bit 3
 * of shared_mask set, else [K][B][ntvp]; p is [np] with bit 4 set, else [B][np].  pair status [K][B]: bit 1 = the exponential failed,
 * bit 2 = Newton or the reduction failed (the pair is zero either way); Newton updates = status >> 24.
 * tv: reads model-size pairs whatever the code object; Q, R, Pf in design size with bits 0/1/2 of shared_mask as above (no per-step
 * weights); pair_status (may be NULL) marks failed pairs.  K_traj and / or law_M (standard mode only) receive the gains, law_M in the
 * layout of the plant rollout's law record, [K][nu][nx][ld] with the trajectory index fastest and ld >= B; P_traj may be NULL; P0 is
 * always written.  status[b]: bit 1 = singular or non-finite block, bit 2 = failed or non-finite pair, met at step (status >> 8) &
 * 0xFFFF: K_j = 0 for j <= that step (the law replays u* there), the gains of the steps behind it are kept, P0 = Q, never NaN.
 * B <= 0 launches nothing; K <= 0 launches nothing when every output is NULL and is refused otherwise. */
int dompc_lqr_pairs_device(dompc_lqr* h, int32_t B, int32_t K, const double* x_traj, const double* u_traj, const double* z0,
                           const double* tvp, const double* p, int32_t shared_mask, double* A_traj, double* B_traj, double* z_out,
                           int32_t* status, void* stream);
int dompc_lqr_tv_device(dompc_lqr* h, int32_t B, int32_t K, const double* A_traj, const double* B_traj, const int32_t* pair_status,
                        const double* Q, const double* R, const double* Pf, int32_t shared_mask, double* K_traj, double* law_M,
                        int32_t ld, double* P_traj, double* P0, int32_t* status, void* stream);
/* host buffers: with a model the knots -> pairs -> recursion (A_traj / B_traj are not read; z0 NULL = 0), without one the pairs
 * themselves; P_out, A_out, B_out, Z_out, pair_status, status may be NULL */
int dompc_lqr_tv(dompc_lqr* h, int32_t B, int32_t K, const double* A_traj, const double* B_traj, const double* x_traj,
                 const double* u_traj, const double* z0, const double* tvp, const double* p, const double* Q, const double* R,
                 const double* Pf, int32_t shared_mask, double* K_out, double* P0_out, double* P_out, double* A_out, double* B_out,
                 double* Z_out, int32_t* pair_status, int32_t* status);

/* ---- batched approximate MPC (csrc/dompc_ampc.hip): what do_mpc.approximateMPC.ApproxMPC.make_step computes - scale the input
 * [x; u_prev] by its bounds box, evaluate a feed-forward network in float32, rescale the output to [lbu, ubu] and clip - for B
 * samples per launch.  The code object is built for the network's SHAPE (n_in <= 64, n_out <= 32, n_hidden_layers <= 8 of
 * n_neurons <= 128, activations: 0 relu, 1 tanh, 2 leaky_relu, 3 sigmoid, 4 linear (output only), scaling on or off); weights,
 * biases and bounds are data of the handle and may be replaced at any time (dompc_ampc_set_weights), e.g. after every optimiser
 * step.  x: [B][nx]; u_prev: [B][n_in - nx], NULL when n_in == nx; u: [B][n_out]; all float64. */
typedef struct dompc_ampc dompc_ampc;
typedef struct dompc_ampc_desc {
  int32_t n_in, n_out, n_hidden_layers, n_neurons, act, out_act, scaling;
  int32_t nx;                        /* leading entries of the network input that come from x; the others from u_prev */
  const char* code_object_path;      /* gfx950 code object built from the lowered network shape                  */
  const char* model_hash;            /* AMPC_MODEL_HASH of the header the code object was built from             */
  int32_t device;
} dompc_ampc_desc;
int  dompc_ampc_create(const dompc_ampc_desc* desc, dompc_ampc** out);
void dompc_ampc_destroy(dompc_ampc* h);
const char* dompc_ampc_last_error(const dompc_ampc* h);       /* h may be NULL: error of the last failed create */
int64_t dompc_ampc_packed_size(const dompc_ampc* h);          /* floats of the packed weights the code object reads */
/* packed_f32: n floats in the operand order of the kernel (do_mpc_amd/ampc.py:pack_weights); lb_in / ub_in [n_in]:
 * the box of the network input (shift = lb_in, range = ub_in - lb_in); lbu / ubu [n_out].  Host pointers; returns when the copy is done. */
int dompc_ampc_set_weights(dompc_ampc* h, const float* packed_f32, int64_t n, const double* lb_in, const double* ub_in,
                           const double* lbu, const double* ubu);
/* the handle's DEVICE arrays of the last dompc_ampc_set_weights: the packed weights and shift, range, lbu, ubu, ubu - lbu - what
 * dompc_plant_ampc_loop_device takes as w and par.  Valid until the handle is destroyed; their content follows dompc_ampc_set_weights. */
int dompc_ampc_device_weights(dompc_ampc* h, const float** w, const double** par);
/* host buffers */
int dompc_ampc_step_batch(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u_out, int32_t clip_to_bounds);
/* DEVICE buffers, asynchronous on `stream` (hipStream_t as void*) */
int dompc_ampc_step_batch_device(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u, int32_t clip_to_bounds,
                                 void* stream);
/* The network's own Jacobian beside the step, ONE launch (dompc_ampc_jac_kernel of the same code object, forward mode in float32):
 * u [B][n_out] exactly as the step writes it; du_dx [B][n_out][nx] and du_du_prev [B][n_out][n_in - nx] (NULL when n_in == nx), the
 * derivative of the unclipped u with respect to x and u_prev in physical units; with clip_to_bounds the row of an output that lay
 * beyond a bound is zero.  The weights are those of the last dompc_ampc_set_weights. */
int dompc_ampc_jacobian_batch(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u_out, double* du_dx,
                              double* du_du_prev, int32_t clip_to_bounds);
/* DEVICE buffers, asynchronous on `stream`; nothing behind row B of any output is written */
int dompc_ampc_jacobian_batch_device(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u, double* du_dx,
                                     double* du_du_prev, int32_t clip_to_bounds, void* stream);

/* ---- affine state feedback  u = sat(u_ref + M (x - x_ref))  for B loops (csrc/dompc_affine.h) --------------------------------
 * The law record.  Every pointer is a DEVICE address; arrays are laid out with the loops innermost, so that one thread per loop reads
 * them coalesced over the batch: x_ref [nx][ld], u_ref [nu][ld], M [nu][nx][ld] (entry of loop b at ... * ld + b), flags [ld] (NULL:
 * all zero), lb / ub [nu] in physical units (may be infinite; read only with clip != 0), x_scale [nx].  Status bits of a step: 0 and 1
 * copied from flags, 2 = an input was clipped, 3 = max_k |x_k - x_ref_k| / x_scale_k > max_dx (bit 4 is not written by a step: the
 * event-triggered loop of do_mpc_amd marks with it, in its records, the loops it re-solved at that step).  The arithmetic is fixed - u_i =
 * fma(M[i][k], x_k - x_ref_k, u_i) for k ascending from u_ref_i, the clip as two comparisons (a NaN stays a NaN) - and the same in
 * dompc_asmpc_step_batch_device and dompc_plant_rollout_affine_device: the two give equal bits.  An LQR gain schedule is such a law
 * (x_ref = xss, u_ref = uss, M = K). */
typedef struct dompc_affine_law {
  const double *x_ref, *u_ref, *M;
  const int32_t* flags;
  const double *lb, *ub, *x_scale;
  int64_t ld;
  double max_dx;
  int32_t clip, pad;
} dompc_affine_law;

/* K control steps law -> plant in ONE launch (dompc_plant_rollout_kernel), one thread per loop: for k = 0 .. K-1 the input of the law
 * at X_traj[k] goes to U_traj[k], the plant step (the step of dompc_plant_step_batch_device, unchanged) from X_traj[k] with U_traj[k]
 * to X_traj[k+1].  X_traj [K+1][B][nx] with row 0 filled by the caller, U_traj [K][B][nu], plant_status [K][B] (as status of
 * dompc_plant_step_batch_device) and law_status [K][B] (bits above; either may be NULL); tvp_rows [K][ntvp] / p_rows [K][np]: the
 * plant's parameters of step k, shared by the batch.  No process or measurement noise, no measurement.  A loop whose plant step fails
 * goes on from the state it reached.  Plants with algebraic states are refused: dompc_plant_step_batch_device serves them.
 * DEVICE buffers, asynchronous on `stream`. */
int dompc_plant_rollout_affine_device(dompc_plant* h, int32_t B, int32_t K, const dompc_affine_law* law, double* X_traj, double* U_traj,
                                      const double* tvp_rows, const double* p_rows, int32_t* plant_status, int32_t* law_status,
                                      void* stream);

/* The general rollout (dompc_plant_loop_kernel), for every plant, those with algebraic states included: K control steps of B loops in
 * ONE launch, one thread per loop.  Every pointer of the description is a DEVICE address, except `law`, a host pointer to a record of
 * device addresses (NULL: open loop).  Per loop b and step k = 0 .. K-1:
 *   input   with a law: u = sat(u_ref + M (x - x_ref) + G (u_prev - up_ref)) at x = X_traj[k] goes to U_traj[k], its status bits to
 *           law_status[k]; G [nu][nu][ld] and up_ref [nu][ld] are laid out like the law's arrays (up_ref may be the law's u_ref); u_prev
 *           is U_prev0 [B][nu] at k = 0 and the input applied at k - 1 - the clipped one - afterwards.  G = NULL: the law of
 *           dompc_plant_rollout_affine_device, with its bits.  Without a law U_traj[k] is read, and nothing is written there.
 *   plant   the step of dompc_plant_step_batch_device, unchanged, from X_traj[k] to X_traj[k+1] with tvp_rows[k] [K][ntvp] (shared by
 *           the batch) and EITHER p_rows[k] [K][np] (shared by the batch) OR p_loops [B][np] (one row per loop, constant over the K
 *           steps); process noise W_traj [K][B][nw] and measurement noise V_traj [K][B][nv] (NULL: zero); the measurement at X_traj[k+1]
 *           to Y_traj [K][B][ny] (NULL: none); status to plant_status[k].
 *   z       the per-loop Newton starts of the algebraic states are the handle's, as in dompc_plant_step_batch_device: carried from step
 *           to step and from call to call; reseed_z != 0 seeds them with z0 (dompc_plant_set_z0) first.  Z_traj [K][B][nz] (NULL: none)
 *           receives the algebraic states at X_traj[k+1].
 * X_traj [K+1][B][nx] with row 0 filled by the caller.  A loop whose plant step fails goes on from the state it reached.  Refused, with
 * the reason in dompc_plant_last_error: null X_traj / U_traj, parameters without p_rows or p_loops (or with both), _tvp without
 * tvp_rows, a law on a plant without inputs, an incomplete law record, G without a law, up_ref or U_prev0, Z_traj on a plant without
 * algebraic states.  B <= 0 or K <= 0: nothing is launched.  Asynchronous on `stream`. */
typedef struct dompc_plant_rollout_desc {
  const dompc_affine_law* law;
  const double *G, *up_ref, *U_prev0;
  double *X_traj, *U_traj;
  const double *W_traj, *V_traj;
  double *Y_traj, *Z_traj;
  const double *tvp_rows, *p_rows, *p_loops;
  int32_t *plant_status, *law_status;
  int32_t reseed_z, pad;
  int64_t law_step;                  /* 0: one law record for the K steps.  s > 0: the record of step k is `law` with x_ref, u_ref, M, flags
                                        advanced by k nx s, k nu s, k nu nx s, k s elements ([K][nx][ld], ... with s = ld); lb, ub, x_scale,
                                        clip, max_dx are shared by the steps.  Refused with G / up_ref, without a law, and with s < B */
} dompc_plant_rollout_desc;
int dompc_plant_rollout_device(dompc_plant* h, int32_t B, int32_t K, const dompc_plant_rollout_desc* r, void* stream);

/* The fused approximate-MPC loop (csrc/dompc_ampc_loop.hip: dompc_ampc_loop_kernel): K control steps network -> plant of B loops in
 * ONE launch, one wavefront per 64 loops.  The plant handle is created on the code object of a PAIR - one plant model and one network
 * shape; it holds every plant kernel too, so the handle serves every other dompc_plant_* call as well.  Every pointer of the
 * description is a DEVICE address.  Per loop b and step k = 0 .. K-1:
 *   network the step of dompc_ampc_step_batch_device, unchanged, at x = X_traj[k] with u_prev = U_prev0 [B][nu] at k = 0 and the input
 *           applied at k - 1 - the clipped one - afterwards (n_in = nx + nu; with n_in = nx there is no u_prev and U_prev0 is not read);
 *           the input goes to U_traj[k].  w and par are the network handle's device arrays (dompc_ampc_device_weights), the shape
 *           fields its description's; clip as clip_to_bounds there.
 *   plant   the step of dompc_plant_step_batch_device, unchanged, with the parameters, noise, records and status of
 *           dompc_plant_rollout_device.
 *   z       the per-loop Newton starts of the algebraic states: z_guess [B][nz], e.g. those of the handle that runs the same loops step
 *           by step (dompc_plant_z_guess_device) - the two paths then carry ONE set of starts; NULL: this handle's own, reseed_z != 0
 *           seeds them with z0 first.
 * Refused, with the reason in dompc_plant_last_error: null X_traj / U_traj, parameters without p_rows or p_loops (or with both), _tvp
 * without tvp_rows, Z_traj on a plant without algebraic states, n_out != nu, n_in neither nx nor nx + nu, n_in = nx + nu without
 * U_prev0, null w / par, a handle whose code object has no loop kernel or was built for another network shape.  B <= 0 or K <= 0:
 * nothing is launched.  Asynchronous on `stream`. */
typedef struct dompc_plant_ampc_loop_desc {
  const float* w;
  const double* par;
  int32_t n_in, n_out, n_hidden_layers, n_neurons, act, out_act, scaling, clip;
  const double* U_prev0;
  double *X_traj, *U_traj;
  const double *W_traj, *V_traj;
  double *Y_traj, *Z_traj;
  const double *tvp_rows, *p_rows, *p_loops;
  int32_t* plant_status;
  double* z_guess;
  int32_t reseed_z, pad;
} dompc_plant_ampc_loop_desc;
int dompc_plant_ampc_loop_device(dompc_plant* h, int32_t B, int32_t K, const dompc_plant_ampc_loop_desc* d, void* stream);
/* The handle's per-loop Newton starts for B loops, a DEVICE array [B][nz] (NULL for a plant without algebraic states): allocated and
 * seeded as the next step of B samples would (reseed != 0: with z0).  Valid until the handle's buffer grows or the handle is destroyed. */
int dompc_plant_z_guess_device(dompc_plant* h, int32_t B, int32_t reseed, double** z_guess);

/* ---- sensitivity-based MPC between two solves (csrc/dompc_asmpc.hip): the class ASMPC of the reference's
 * examples/batch_reactor_differentiator, u = (I - G)^-1 (u0 + J (x - x_prev) - G u0) with J = du0/dx0, G = du0/du_prev - the affine law
 * u = u0 + M (x - x_prev), M = (I - G)^-1 J - for B loops.  The code object is built for the sizes (nx <= 64, nu <= 16); the law
 * record, the bounds and the scaling are data of the handle.
 * dompc_asmpc_prepare_device forms M for every loop and writes the law record (x_ref = x_prev, u_ref = u0): entry (r, c) of loop b's J
 * at J + b * batch_J + r * row_J + c, G alike - so both may be views into the [B][nu][nx + nu] result of dompc_sens_batch_device;
 * ok [B] (NULL: all 1).  flags bit 0: ok = 0 or J / G not finite, bit 1: I - G singular or a non-finite pivot; either gives M = 0, the
 * law then holds u0.  dompc_asmpc_set_law: the same from contiguous HOST arrays J [B][nu][nx], G [B][nu][nu]; returns when the law is
 * there.  dompc_asmpc_get_law copies the record to host arrays x_ref [B][nx], u_ref [B][nu], M [B][nu][nx], flags [B] (any may be
 * NULL).  dompc_asmpc_law fills `out` with the record for dompc_plant_rollout_affine_device; it is valid until the next preparation.
 * dompc_asmpc_set_options: bounds of the inputs in physical units (infinite allowed), x_scale [nx], clip on / off, max_dx (INFINITY:
 * never flagged); host pointers.  Defaults: no bounds, x_scale = 1, clip on, max_dx = INFINITY. */
typedef struct dompc_asmpc dompc_asmpc;
typedef struct dompc_asmpc_desc {
  int32_t nx, nu;
  const char* code_object_path;      /* gfx950 code object built for the sizes                                   */
  const char* model_hash;            /* ASMPC_MODEL_HASH of the header the code object was built from            */
  int32_t device;
} dompc_asmpc_desc;
int  dompc_asmpc_create(const dompc_asmpc_desc* desc, dompc_asmpc** out);
void dompc_asmpc_destroy(dompc_asmpc* h);
const char* dompc_asmpc_last_error(const dompc_asmpc* h);     /* h may be NULL: error of the last failed create */
int dompc_asmpc_set_options(dompc_asmpc* h, const double* lbu, const double* ubu, const double* x_scale, int32_t clip, double max_dx);
int dompc_asmpc_prepare_device(dompc_asmpc* h, int32_t B, const double* x_prev, const double* u0, const double* J, int64_t row_J,
                               int64_t batch_J, const double* G, int64_t row_G, int64_t batch_G, const int32_t* ok, void* stream);
int dompc_asmpc_set_law(dompc_asmpc* h, int32_t B, const double* x_prev, const double* u0, const double* J, const double* G,
                        const int32_t* ok);
int dompc_asmpc_get_law(dompc_asmpc* h, double* x_ref, double* u_ref, double* M, int32_t* flags);
int32_t dompc_asmpc_law_batch(const dompc_asmpc* h);          /* loops of the current law record, 0 = none */
int dompc_asmpc_law(dompc_asmpc* h, dompc_affine_law* out);
/* one step U = sat(u_ref + M (X - x_ref)) for the B loops of the law; status [B] may be NULL.  Host buffers: */
int dompc_asmpc_step_batch(dompc_asmpc* h, int32_t B, const double* x, double* u_out, int32_t* status);
/* DEVICE buffers, asynchronous on `stream` (hipStream_t as void*) */
int dompc_asmpc_step_batch_device(dompc_asmpc* h, int32_t B, const double* x, double* u, int32_t* status, void* stream);
/* ... the same step on a law record of the caller's (device addresses; e.g. the record of one step of a time-varying law written by
 * dompc_lqr_tv_device): the handle's own law, options and batch are not read.  Refused: an incomplete record, ld < B. */
int dompc_asmpc_step_law_device(dompc_asmpc* h, const dompc_affine_law* law, int32_t B, const double* x, double* u, int32_t* status,
                                void* stream);
/* Event-triggered re-solves of some loops of the law.
 * dompc_asmpc_select_device: idx[0 .. count[0]) = the loops b with status[b] & mask != 0 in ascending order of b (status [B]: what a
 * step wrote; idx [B], count [1]; entries of idx beyond count are not written).  An ordered compaction: list and count do not depend
 * on the launch shape or on timing.  DEVICE buffers, asynchronous on `stream`.
 * dompc_asmpc_update_device: dompc_asmpc_prepare_device for n compact entries, entry j written into column slot[j] of the EXISTING
 * law record (slot [n], device; distinct values).  The other columns are not touched, the record keeps its size; a slot outside the
 * record stores nothing.  0 <= n <= dompc_asmpc_law_batch; n = 0 launches nothing.  Asynchronous on `stream`.
 * dompc_asmpc_update_law: the same from contiguous HOST arrays (slot included), as dompc_asmpc_set_law; returns when it is done. */
int dompc_asmpc_select_device(dompc_asmpc* h, int32_t B, const int32_t* status, int32_t mask, int32_t* idx, int32_t* count, void* stream);
int dompc_asmpc_update_device(dompc_asmpc* h, int32_t n, const int32_t* slot, const double* x_prev, const double* u0, const double* J,
                              int64_t row_J, int64_t batch_J, const double* G, int64_t row_G, int64_t batch_G, const int32_t* ok,
                              void* stream);
int dompc_asmpc_update_law(dompc_asmpc* h, int32_t n, const int32_t* slot, const double* x_prev, const double* u0, const double* J,
                           const double* G, const int32_t* ok);

/* ---- batched parametric sensitivities of the MPC solution (mode 3 of csrc/dompc_device.hip, sens_newton in csrc/dompc_driver.h):
 * d x*[sel] / d p[cols] at B solutions of one problem class, from Newton directions of the solver's own structured KKT factorisation.
 * The points are what dompc_solve_batch(_device) returned: x [B][n_opt_x], lam_g [B][n_g], mu [B] = stats.mu / stats.obj_scaling (a
 * value that is not a positive finite number marks a member to skip, e.g. one whose solve did not succeed), p [B][n_opt_p] the
 * parameters it was solved with; lbx / ubx / lbg / ubg one shared copy.  The bound multipliers are rebuilt as mu / distance to the
 * bounds the solver relaxed.  flags bit 0: active-set reduction with active_set_tol (inactive bounds and nl_cons rows leave the
 * system, active ones are held like equalities).
 * sel [n_sel]: indices into opt_x of the wanted rows.  row_plan [n_rows][2] = (j, kind): the parameter rows a point is solved for -
 * kind 0 the base row (must be row 0), 1: p_j + h with h = max(1, |p_j|) (a parameter that enters the optimality conditions
 * linearly), 2 / -2: p_j + h / p_j - h with h = fd_step max(1, |p_j|).  col_plan [n_cols][3] = (j, ip, im): column c of the result is
 * (D[ip] - D[0]) / h for im < 0 and (D[ip] - D[im]) / 2h otherwise, D[r] the direction of row r.
 * Results: S [B][n_sel][n_cols] in the solver's scaled variables, residual_step [B] = max |dx| of the base row over the variables that
 * appear in the problem, ok [B] = 1 when every direction of the point was computed; a point that is not strictly inside its relaxed
 * bounds or a KKT matrix with the wrong inertia gives ok = 0 and NaN in S and residual_step.  Nothing of size n_opt_x leaves the GPU.
 * All pointers of dompc_sens_batch_device are DEVICE addresses, the call is asynchronous on `stream`; dompc_sens_batch takes host
 * pointers and returns when the results are there.  Not available on a sharded handle. */
int dompc_sens_batch_device(dompc_handle* h, int32_t B, const double* x, const double* lam_g, const double* mu, const double* p,
                            const double* lbx, const double* ubx, const double* lbg, const double* ubg, const int32_t* sel,
                            int32_t n_sel, const int32_t* row_plan, int32_t n_rows, const int32_t* col_plan, int32_t n_cols,
                            double fd_step, int32_t flags, double active_set_tol, double* S, double* residual_step, int32_t* ok,
                            void* stream);
int dompc_sens_batch(dompc_handle* h, int32_t B, const double* x, const double* lam_g, const double* mu, const double* p,
                     const double* lbx, const double* ubx, const double* lbg, const double* ubg, const int32_t* sel,
                     int32_t n_sel, const int32_t* row_plan, int32_t n_rows, const int32_t* col_plan, int32_t n_cols,
                     double fd_step, int32_t flags, double active_set_tol, double* S, double* residual_step, int32_t* ok);

#ifdef __cplusplus
}
#endif
#endif /* DOMPC_IPM_H */
