/*
 * mi_ilqr.h — C ABI of libmi_ilqr.so: the MI355X-native batched iLQR/DDP hot path.
 *
 * This is the drop-in boundary for the path BASELINE.json:north_star names: the
 * body of IterativeLinearQuadraticRegulator.Solve() in the reference
 * (/root/reference/ilqr.py:669-710) and the stages it calls, for a BATCH of B
 * independent problems that share model, horizon and cost matrices.  Each entry
 * point cites the reference interface it replaces.  Plain pointers and sizes
 * only; all `double*` arguments are HOST memory unless the name says `device`;
 * the library copies in/out and never keeps or frees caller memory.
 *
 * Array layout is the reference's, per problem (time on the LAST
 * axis, C order), with a leading batch axis:
 *     x_bar (B,n,N)   u_bar (B,m,N-1)   K (B,m,n,N-1)   kappa (B,m,N-1)
 *     fx (B,n,n,N-1)  fu (B,n,m,N-1)    dV_coeff (B,N-1)
 *
 * Threading: a handle is not thread-safe (the reference class is not either:
 * it mutates self.context, ilqr.py:223-229); distinct handles are independent.
 * One handle = one GPU = one HIP stream.  Multi-GPU = one process per GPU, each
 * with its own handle over its shard of the batch (no data-path collective).
 *
 * There is NO CPU fallback: every compute entry returns MI_ILQR_E_NO_DEVICE when
 * no gfx950 device is usable.
 */
#ifndef MI_ILQR_H
#define MI_ILQR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ILQR_ABI_VERSION 10  /* 10: mi_ilqr_set_control_limits (box control limits of the m <= 2 kernel families);
                                   9: mi_ilqr_comm_count; partial reads of MI_F_HIST / MI_F_ITER_CYCLES; MI_I64_CLUSTER_WORDS reads as zeros where no cluster ran;
                                   7: mi_ilqr_desc.on_indefinite, mi_ilqr_model_plugin.m_user, 256 plugin slots;
                                   8: MI_STATUS_FLAG_INDEFINITE, on_indefinite = 1 inverts with partial pivoting, asymmetric costs for n <= 32,
                                      the diagnostic field MI_I64_CLUSTER_WORDS */
#define MI_ILQR_MAX_PARAMS 16
#define MI_FIT_MAX_FREE 8        /* free parameters of one MI_F_FIT_RUN ("Parameter identification" below) */
#define MI_ILQR_CLUSTER_WORDS 40 /* 64-bit words per problem of the diagnostic field MI_I64_CLUSTER_WORDS */

/* Error codes (0 = OK).  The Python wrapper maps them onto the exception types
 * the reference raises (SURVEY.md §8b "Error convention"). */
enum {
  MI_ILQR_OK = 0,
  MI_ILQR_E_BAD_SHAPE = -1,      /* reference: assert on shapes, ilqr.py:130-131,145,155 */
  MI_ILQR_E_BAD_METHOD = -2,     /* reference: Exception('unknown interpolation method'), ilqr.py:404 */
  MI_ILQR_E_LINESEARCH = -3,     /* reference: RuntimeError("linesearch failed ..."), ilqr.py:337 */
  MI_ILQR_E_HIP = -4,
  MI_ILQR_E_NO_DEVICE = -5,
  MI_ILQR_E_BAD_ARG = -6,
  MI_ILQR_E_UNSUPPORTED = -7,    /* model / size / cost-matrix combination no kernel covers */
  MI_ILQR_E_RCCL = -8            /* librccl missing, or a collective / communicator call failed */
};

/* Device dynamics models (the `system` argument of ilqr.py:21 becomes a model
 * descriptor; Drake systems cannot run on the GPU — SURVEY.md §8b).  Parameter
 * vectors are documented in drake_ddp_amd/csrc/models.hpp. */
enum {
  MI_MODEL_PENDULUM = 0,       /* n=2  m=1  */
  MI_MODEL_ACROBOT = 1,        /* n=4  m=1  */
  MI_MODEL_CARTPOLE = 2,       /* n=4  m=1  */
  MI_MODEL_CARTPOLE_WALL = 3,  /* n=4  m=1  */
  MI_MODEL_SYNTH36 = 4,        /* n=36 m=12 */
  MI_MODEL_PLANAR_QUAD = 5,    /* n=36 m=12: planar floating-base quadruped (articulated-body algorithm, ground
                                  contact); can declare a step INFEASIBLE - such a line-search trial costs +inf, as
                                  when Drake's update throws (ilqr.py:315-323) */
  MI_MODEL_QUAD3D = 6,         /* n=37 m=12: 3-D floating-base quadruped with mini_cheetah.py:41-52's state layout
                                  (unit quaternion | position | 12 joints | 18 velocities), feet contact; can declare a
                                  step infeasible like the planar one */
  MI_MODEL_ARM27 = 7,          /* n=27 m=7: 7-joint arm pushing a free ball - the state kinova_gen3.py:52-70 / panda_fr3.py
                                  stack (7 joint angles | the ball's unit quaternion, position | 13 velocities); served by
                                  the mid-size workgroup-per-problem kernels */
  MI_MODEL_ARM27C = 8          /* n=27 m=7: the same arm, ball and contacts with COUPLED rigid-body joint dynamics - the joint-space
                                  mass matrix of three point masses + rotor inertias, centripetal / Coriolis and gravity terms,
                                  M(q) qdd = tau - ... solved per step (L D L^T); 16 parameters (Arm27's + m_wrist) */
};

/* utils_derivs_interpolation.derivs_interpolation.keypoint_method
 * (/root/reference/utils_derivs_interpolation.py:4-9; strings at ilqr.py:396-400). */
enum { MI_KP_SET_INTERVAL = 0, MI_KP_ADAPTIVE_JERK = 1, MI_KP_ITERATIVE_ERROR = 2 };

/* How fx/fu are obtained (replaces _calc_dynamics_partials, ilqr.py:233-272). */
enum { MI_JAC_FD_CENTRAL = 0, MI_JAC_AUTODIFF = 1 };

/* Which kernel family serves a small-state model (mi_ilqr_desc.kernel_mode):
 *   LATENCY    wave-per-problem, state in LDS: minimal time-to-solution, up to ~2k problems/GPU in flight;
 *   THROUGHPUT lane-per-problem, batch-minor state streamed through HBM: for tens of thousands of
 *              problems (every key-point method - a key-point list per lane; stage-level entries are not
 *              available; built-in models and family-0 plugins with n <= 6);
 *   AUTO       THROUGHPUT when B >= 8192 and the configuration allows it - except n = 2 models with
 *              N <= 257, whose LATENCY kernel (rollout and Riccati sweep parallel in time) is the faster one
 *              at every batch size - else LATENCY. */
enum { MI_KERNEL_AUTO = 0, MI_KERNEL_LATENCY = 1, MI_KERNEL_THROUGHPUT = 2 };

/* Per-problem status written by solve/forward. */
enum { MI_STATUS_CONVERGED = 0, MI_STATUS_MAX_ITERS = 1, MI_STATUS_LINESEARCH_FAILED = 2,
       MI_STATUS_INTERNAL = 3, /* a helper workgroup of the problem's cluster stopped answering (never seen) */
       /* 4: unused */
       MI_STATUS_NOT_PD = 5,   /* workgroup-per-problem kernels (n >= 5 models with m > 2), mi_ilqr_desc.on_indefinite = 0: a backward
                                  pass met a Quu that is not positive definite (a pivot of its unpivoted elimination <= 0 or not
                                  finite) - an indefinite cost expansion or one ruined by round-off - and the problem STOPPED there:
                                  its gains are NOT to be used.  The reference inverts such a Quu all the same (np.linalg.inv,
                                  ilqr.py:655) and carries on: that is on_indefinite = 1 */
       MI_STATUS_FLAG_INDEFINITE = 16 /* OR-ed onto the outcome above (ABI 8), on_indefinite = 1: a backward pass of this solve (of this
                                  mpc_run) met such a Quu, inverted it with partial pivoting like the reference and carried on;
                                  `status & ~MI_STATUS_FLAG_INDEFINITE` is the solve's outcome.  Counted in stats.n_not_pd too */ };

/* Per-problem outcome of a parameter fit (MI_F_FIT_RESULT's status column; "Parameter identification" below). */
enum { MI_FIT_CONVERGED = 0, MI_FIT_MAX_ITERS = 1, MI_FIT_STALLED = 2, MI_FIT_BAD_DATA = 3 };

/* Selector for mi_ilqr_get / mi_ilqr_set / mi_ilqr_device_ptr. */
enum {
  MI_F_X_BAR = 0, MI_F_U_BAR = 1, MI_F_K = 2, MI_F_KAPPA = 3, MI_F_DV = 4, MI_F_FX = 5, MI_F_FU = 6,
  MI_F_COST = 7,        /* (B,)   total cost L of x_bar/u_bar                          */
  MI_F_X0 = 8,          /* (B,n)                                                        */
  MI_F_HIST = 9,        /* (B,hist_cap,4) rows (L, eps, ls_trials, percentage_derivs)   */
  MI_F_X_TRIAL = 10,    /* (B,n,N)   last mi_ilqr_rollout trajectory                    */
  MI_F_U_TRIAL = 11,    /* (B,m,N-1)                                                    */
  MI_F_TRIAL_COST = 12, /* (B,2) (L, expected_improvement) of the last rollout          */
  MI_F_ITER_CYCLES = 13,/* (B,hist_cap,4) per-iteration stopwatches of the last solve, shader-clock cycles: line search,
                           linearization (0 when the rollout linearized on its way), backward pass, whole iteration - the
                           reference's time_fp / time_getDerivs / time_backwardsPass / iter time (ilqr.py:364-372,696-702);
                           wave- and workgroup-per-problem kernels */
  MI_F_X_NOM = 14,      /* (B,n) per-problem targets x_nom_b (mi_ilqr_set_cost, "Per-problem targets" below)              */
  MI_F_TARGET_STEP = 15,/* (B,n) per-problem target_step_b of mi_ilqr_mpc_run                                             */
  MI_F_MODEL_PARAMS = 16,/* (B,n_params) per-problem model parameters: problem b's plant ("Per-problem model parameters" below) */
  MI_F_COST_MATRICES = 17,/* (B,2*n*n+m*m) per-problem cost matrices, row b = Q_b | R_b | Qf_b ("Per-problem cost matrices" below) */
  MI_F_POLICY_KERNEL_MS = 18,/* (1,) read-only: milliseconds of the rollout kernel of the last policy rollout, from its own HIP events (mi_ilqr_policy_rollout) */
  MI_F_POLICY_NOISE = 19,    /* (B,n+m) per-problem standard deviations sigma_x | sigma_u of the policy rollouts' disturbances ("Process and actuation noise" below) */
  MI_F_POLICY_STREAM = 20,   /* (3,) seed | first_sample | common of the disturbances' random stream, integers held in doubles (the same) */
  MI_F_PLANT_STATE = 21,     /* (B,n) the plants' states: set, the handle holds a plant and mi_ilqr_mpc_run is the CLOSED loop ("Closed-loop MPC" below) */
  MI_F_PLANT_PARAMS = 22,    /* (B,n_params) the plants' own model parameters (default: problem b's model row) */
  MI_F_PLANT_NOISE = 23,     /* (B,n+m) per-problem standard deviations sigma_x | sigma_u of the plants' disturbances */
  MI_F_PLANT_STREAM = 24,    /* (4,) seed | clock | common | feedback of the plants, integers held in doubles */
  MI_F_PLANT_LOG = 25,       /* (B,num_resolves*replan_steps,n+m+1) read-only: rows x_k | u_k | l_k of the last closed-loop mi_ilqr_mpc_run */
  MI_F_PLANT_KERNEL_MS = 26, /* (1,) read-only: milliseconds of the plant kernels of the last closed-loop mi_ilqr_mpc_run, summed, from their own HIP events */
  MI_F_X_REF = 27,           /* (B,T,n) reference trajectories: time-varying targets, T from the byte count ("Reference trajectories" below) */
  MI_F_REF_CLOCK = 28,       /* (1,) the row of the reference a solve's window starts at, an integer held in a double */
  MI_F_POLICY_MC_DIST = 29,  /* (B,3n+2n_params) sampler rows x0_mean | x0_spread | goal | p_mean | p_spread ("Monte-Carlo on the device" below) */
  MI_F_POLICY_MC_RUN = 30,   /* (5,) write-only COMMAND: S | x0_dist | p_dist | sample_params | samples - mi_ilqr_set RUNS the evaluation */
  MI_F_POLICY_MC_STATS = 31, /* (B,10) read-only: S | counted | success | mean | M2 | min | max | argmin | argmax | steps_total of the last run */
  MI_F_POLICY_MC_SAMPLES = 32,/* (B,S,n+n_params+2) read-only: rows x0 | params | cost | steps of the last run, when it was asked for them */
  MI_F_POLICY_MC_BOX = 33,   /* (B,2n) safety box rows lo | hi, +-inf = unbounded ("Envelopes and a safety box" below) */
  MI_F_POLICY_MC_OBSERVE = 34,/* (1,) what a run observes beside the cost: bit 0 state envelopes, bit 1 control envelopes, an integer held in a double */
  MI_F_POLICY_MC_ENVELOPE = 35,/* (B,N,n,8) read-only: count | K | s1 | s2 | min | max | argmin | argmax of every state row of the last run */
  MI_F_POLICY_MC_ENVELOPE_U = 36,/* (B,N-1,m,8) read-only: the same of every control row, m the device's control dimension */
  MI_F_POLICY_MC_SAFETY = 37,/* (B,3+N) read-only: ran | safe | safe_success | exits[0 .. N-1] of the last run, integers held in doubles */
  MI_F_SEEDS_SIGMA = 38,     /* (B,m) sigma_u rows of the multi-start perturbation, m the device's control dimension ("Multi-start" below) */
  MI_F_SEEDS_RUN = 39,       /* (6,) write-only COMMAND: K | op | seed | round | hold | reserved = 0 - mi_ilqr_set RUNS perturb / select / reseed / gather; (8,): the long form, "Multi-start in the receding-horizon loop"; (10,): the sampling form, "Sampling-based MPC" */
  MI_F_SEEDS_BEST = 40,      /* (G,3) read-only: winner | cost | eligible of every group of the last select, integers held in doubles; (R+1,G,3) after a long-form run; (I,B,3) after a sampling-form run */
  MI_F_SEEDS_X_BAR = 41,     /* (G,n,N) read-only: the winners' x_bar of the last gather */
  MI_F_SEEDS_U_BAR = 42,     /* (G,m,N-1) read-only: the winners' u_bar of the last gather, m the device's control dimension; (B,m,N-1) after a sampling-form run */
  MI_F_SEEDS_COST = 43,      /* (G,) read-only: the winners' cost of the last gather; (I+1,B,2) after a sampling-form run */
  MI_F_SEEDS_KERNEL_MS = 44, /* (1,) read-only: milliseconds of the kernel of the last MI_F_SEEDS_RUN, from its own HIP events */
  /* parameter identification, values 45 .. 52: counted on from the selector before them */
  MI_F_FIT_DATA = MI_F_SEEDS_KERNEL_MS + 1, /* (B,T,2n+m) logged transitions, rows x | u | x_next, T from the byte count ("Parameter identification" below) */
  MI_F_FIT_WEIGHTS = MI_F_SEEDS_KERNEL_MS + 2, /* (B,n+1) w | count: the diagonal of the residual norm and the rows of MI_F_FIT_DATA problem b uses */
  MI_F_FIT_START = MI_F_SEEDS_KERNEL_MS + 3, /* (B,n_params+1) theta0 | mu0: the parameter rows the fit starts from and its first damping */
  MI_F_FIT_BOUNDS = MI_F_SEEDS_KERNEL_MS + 4, /* (2,n_params) lower | upper bounds of the parameters, +-inf = unbounded */
  MI_F_FIT_RUN = MI_F_SEEDS_KERNEL_MS + 5, /* (6+P,) write-only COMMAND: iterations | ftol | fd_rel | fd_floor | apply | P | free[0..P-1] - mi_ilqr_set RUNS the fit */
  MI_F_FIT_RESULT = MI_F_SEEDS_KERNEL_MS + 6, /* (B,n_params+7) read-only: theta | cost0 | cost | mu | iterations | accepted | status | count of the last run */
  MI_F_FIT_NORMAL = MI_F_SEEDS_KERNEL_MS + 7, /* (B,P+P*P) read-only: g | H (P x P, row-major, symmetric) at the returned theta */
  MI_F_FIT_KERNEL_MS = MI_F_SEEDS_KERNEL_MS + 8, /* (1,) read-only: milliseconds of the last run's kernels, first to last, from its own HIP events */
  /* int32 fields (mi_ilqr_get_int) */
  MI_I_ITERS = 100,     /* (B,) iterations of the last solve                            */
  MI_I_STATUS = 101,    /* (B,)                                                         */
  MI_I_LS_TRIALS = 102, /* (B,) reference-equivalent line-search trials, summed         */
  MI_I_KP_COUNT = 103,  /* (B,) key-points used by the last linearization               */
  MI_I_KP_LIST = 104,   /* (B,N-1) the key-point indices, first KP_COUNT valid          */
  MI_I_POLICY_MC_PASSES = 105, /* (1,) read-only (mi_ilqr_get_int): the passes over windows of sample groups the last MI_F_POLICY_MC_RUN took */
  MI_I64_STAGE_CYCLES = 200, /* (B,4) int64: what mi_ilqr_get_cycles returns - here so that mi_ilqr_get_async can queue it behind a solve */
  MI_I64_CLUSTER_WORDS = 201 /* (B,MI_ILQR_CLUSTER_WORDS) uint64 (mi_ilqr_get_int; diagnostic): the handshake words of the last solve / MPC launch
                                when it shared its linearizations among clusters of workgroups (workgroup-per-problem kernels) - zeros when it
                                did not, and for handles of the other kernel families - [1] helper shares
                                finished, [2] & 0xffff helpers that took part, [2] >> (16 + 6 x) & 63 how many of them ran on XCD x,
                                [3] >> 32 rounds (regular + early), [3] >> 8 & 0xffffff rounds that found every helper on the leader's
                                own XCD (one L2: no cache-wide invalidate), [4] progress word of the last early round, [5] >> 32 early
                                rounds opened (the helpers linearize the line search's first trial while it is being rolled out),
                                [5] & 0xffffffff early rounds whose trial was accepted, [7] candidate-group rounds (mid-size kernels: the
                                helpers roll out the line-search candidates 4 .. beside the leader's four), [8 ..] the costs of those */
};

typedef struct mi_ilqr mi_ilqr_t;

/* Everything IterativeLinearQuadraticRegulator.__init__ takes (ilqr.py:21-22,
 * 51-58, 97-100), plus the batch size and the model descriptor. */
typedef struct {
  int32_t n, m;            /* must equal the model's dimensions (ilqr.py:57-58) */
  int32_t N;               /* num_timesteps (ilqr.py:51) */
  int32_t B;               /* problems in this handle's shard */
  int32_t model_id;
  int32_t n_params;
  double model_params[MI_ILQR_MAX_PARAMS];
  double dt;
  double delta, beta, gamma;                 /* ilqr.py:52-54 */
  int32_t keypoint_method, minN, maxN;       /* derivs_interpolation fields; minN >= 1, and maxN >= 1 with MI_KP_ADAPTIVE_JERK
                                                (else MI_ILQR_E_BAD_ARG).  The reference accepts adaptiveJerk with maxN < 1, and its
                                                list can then take two entries per step and grow past N - 1 (ilqr.py:452-463);
                                                no key-point buffer here holds more than N - 1. */
  double jerk_threshold, iterative_error_threshold;
  int32_t jacobian_mode;
  double fd_step;                            /* absolute central-difference step */
  int32_t max_iters;                         /* safety cap (reference has none); <=0 -> 1000 */
  int32_t hist_cap;                          /* per-problem iteration rows kept; <=0 -> 64 */
  int32_t device_id;                         /* HIP device ordinal */
  int32_t kernel_mode;                       /* MI_KERNEL_AUTO / _LATENCY / _THROUGHPUT */
  int32_t on_indefinite;                     /* workgroup-per-problem kernels, a Quu that is not positive definite in a backward pass:
                                                0 = stop that problem with MI_STATUS_NOT_PD (default of this struct); 1 = what the reference
                                                does (np.linalg.inv, ilqr.py:655): invert it all the same - with partial pivoting, a cold
                                                path no positive definite Quu ever enters - carry on, and flag the problem's status with
                                                MI_STATUS_FLAG_INDEFINITE.  (The wave- and lane-per-problem kernels always behave like 1,
                                                without the flag: their m <= 2 inverses are closed forms.) */
} mi_ilqr_desc;

typedef struct {
  int64_t total_iters;        /* sum_b iterations */
  int64_t total_ls_trials;    /* sum_b sum_i ls_{b,i} (reference-equivalent trials) */
  int32_t n_converged, n_max_iters, n_ls_failed;
  int32_t max_iters_seen;
  double best_cost;           /* min_b L_b over converged problems */
  int32_t best_index;
  float kernel_ms;            /* HIP-event time of the solve kernel(s) on the handle's stream; 0 for a launch
                                 * that mi_ilqr_set_timing left without events */
  double algorithmic_bytes;   /* sum_b sum_i bytes_iter(ls_{b,i}) — SURVEY.md §8d formula */
  int32_t n_internal;         /* problems aborted with MI_STATUS_INTERNAL (a lost cluster helper; counted apart from
                               * n_ls_failed since ABI 5: their x_bar / u_bar are NOT a solution) */
  int32_t n_not_pd;           /* problems stopped with MI_STATUS_NOT_PD (ABI 6; the field was reserved before) */
} mi_ilqr_stats;

int mi_ilqr_abi_version(void);
/* sizeof(mi_ilqr_desc), sizeof(mi_ilqr_stats), sizeof(mi_ilqr_model_plugin) as the LIBRARY was compiled: a binding that restates the
 * structs in its own language (ctypes, cgo, JNI) compares them with its own at load time - a field added on one side only
 * would otherwise shift every later field silently.  Any pointer may be NULL. */
void mi_ilqr_struct_sizes(int32_t* desc_bytes, int32_t* stats_bytes, int32_t* plugin_bytes);
const char* mi_ilqr_strerror(int code);

/* Model registry: dimensions and default parameters of a model id. */
int mi_ilqr_model_info(int model_id, int32_t* n, int32_t* m, int32_t* n_params, double* default_params);

/* OPEN MODEL INTERFACE.  The reference takes any discrete System (ilqr.py:21,37-58); here a model is a C++ struct with
 * `template <class T> static void step(const T* x, const T* u, T* xn, const double* params, double dt)` (T = double, or
 * the forward-mode dual types of csrc/dual.hpp) compiled against the kernel headers of drake_ddp_amd/csrc into a PLUGIN
 * shared library - one translation unit, ~25 s of hipcc, nothing of libmi_ilqr.so is rebuilt
 * (drake_ddp_amd/plugin.py writes and builds that unit; INTEGRATION.md section 5 shows it by hand).  The plugin hands the
 * library this record; the returned id (>= MI_MODEL_PLUGIN_BASE) is used as mi_ilqr_desc.model_id like a built-in one.
 *   family 0: wave-per-problem kernels (state in LDS; any n, m <= 2 - n = 2 takes the time-parallel passes, n = 3..4 the
 *             matrix-core backward step, other n the scalar recursion);
 *   family 1: workgroup-per-problem kernels - n <= 32 with ANY m <= 16 (one or two 16-row tiles: the shapes of a quadrotor
 *             (12, 4), a 7-joint arm (14, 7), kinova_gen3.py's arm + free body (27, 7)), or 32 < n <= 40 with m <= 16,
 *             m % 4 == 0, 2 m <= n; dynamics as `step` per Jacobian column and a one-lane step in the rollout unless the
 *             model provides the cooperative hooks of csrc/models.hpp.  A model with 32 < n <= 40 and another number of
 *             controls declares m as the next multiple of 4 and ignores the extra ones; with any positive cost on them
 *             (R block-diagonal) and a zero initial guess their gains, feed-forward terms and values stay EXACT zeros
 *             (zero columns of fu, zero rows of Qux) and every other result is what the unpadded problem gives.  The
 *             Python mirror does this by itself (drake_ddp_amd/plugin.py pads, drake_ddp_amd/ilqr.py hides it).
 * Family-0 plugins with n <= 6 also carry the lane-per-problem THROUGHPUT kernels (kernel_mode, batches >= 8192 and
 * horizons beyond LDS under AUTO, like the built-in small models); other plugins are served by their family only. */
enum { MI_MODEL_PLUGIN_BASE = 100, MI_ILQR_MAX_PLUGINS = 256 };
typedef struct {
  int32_t abi_version;              /* MI_ILQR_ABI_VERSION of the headers the plugin was compiled against ... */
  int32_t kernel_args_bytes;        /* ... their sizeof(mi::KArgs) ... */
  int32_t handle_bytes;             /* ... and their sizeof(struct mi_ilqr) (the plugin's launch code reads the handle's stream,
                                       events and LDS size): a plugin built from other headers is refused (ABI 6) */
  int32_t m_user;                   /* 0, or the number of controls the model's step READS when that is fewer than m: controls
                                       m_user .. m-1 are padding (see family 1 above); informational - hosts size their arrays with m */
  int32_t n, m, n_params, family;
  double default_params[MI_ILQR_MAX_PARAMS];
  int (*launch)(mi_ilqr_t* h, int mode, const void* kernel_args);   /* instantiates and launches the model's kernels */
  size_t (*lds_bytes)(int32_t N, int32_t n_store);                  /* dynamic LDS of one problem (family 1: n_store < 0 asks for the
                                                                       size with the horizon's cost gradients kept in HBM) */
} mi_ilqr_model_plugin;
int mi_ilqr_register_model(const mi_ilqr_model_plugin* plugin, int32_t* model_id_out);

/* ilqr.py:21-100 — allocate the solver state on the device, zeroed (ilqr.py:70-83). */
int mi_ilqr_create(const mi_ilqr_desc* desc, mi_ilqr_t** out);
void mi_ilqr_destroy(mi_ilqr_t* h);

/* SetRunningCost / SetTerminalCost / SetTargetState (ilqr.py:111-146): Q (n,n), R (m,m),
 * Qf (n,n), x_nom (n), shared by the batch.  Any pointer may be NULL = keep.  ANY finite matrices are accepted, like the
 * reference (lxx = 2Q, luu = 2R, lx = 2Qx - 2 x_nom^T Q, never symmetrized - ilqr.py:180-184), by every kernel family:
 * wave- and lane-per-problem kernels - symmetric positive semi-definite Q, Qf and positive definite R take the
 * time-parallel / matrix-core backward passes, anything else the reference's recursion verbatim;  mid-size
 * workgroup-per-problem kernels (m > 2 or n > 6, n <= 32: Arm27, plugin family 1) - the matrix-core pass itself uses no
 * symmetry when a matrix is not symmetric (ABI 8);  the n = 33..40 kernels (n = 36 / 37 models, plugin family 1 above 32
 * states) - their matrix-core chain mirrors tiles of the symmetric products, so matrices that are not symmetric take a
 * plain-arithmetic form of the pass (ABI 9: large_backward_asym, about four times the cycles per step; MI_ILQR_E_UNSUPPORTED
 * before), and asymmetries of up to 8 ulp of the largest entry - round-off of an A^T A - are averaged away so that such
 * matrices keep the fast pass.  Definiteness is required of none - it is
 * checked where it matters: mi_ilqr_desc.on_indefinite says what a backward pass does with a Quu that is not positive
 * definite. */
int mi_ilqr_set_cost(mi_ilqr_t* h, const double* Q, const double* R, const double* Qf, const double* x_nom);

/* Per-problem targets (the reference's SetTargetState, ilqr.py:111-118, called on each problem's own object; mini_cheetah.py:151-156
 * moves it every re-solve).  Q, R, Qf stay shared by the batch.
 *   mi_ilqr_set(MI_F_X_NOM, (B,n))       gives every problem its own x_nom and switches the handle to PER-PROBLEM TARGETS;
 *   mi_ilqr_set(MI_F_TARGET_STEP, (B,n)) gives every problem its own target_step of mi_ilqr_mpc_run; set in shared mode it also
 *                                        switches: the targets start as the shared x_nom broadcast, the steps as zeros until set.
 *   mi_ilqr_get returns the targets (B,n) in both modes (shared mode: the shared x_nom broadcast) and the steps (zeros in shared mode);
 *   mi_ilqr_device_ptr returns the (B,n) device copies in per-problem mode (MI_ILQR_E_BAD_ARG in shared mode).
 *   Per-problem mode: mi_ilqr_mpc_run's target_step must be NULL (else MI_ILQR_E_BAD_ARG); before each re-solve every problem's target
 *   moves by its own row; after the call MI_F_X_NOM holds, for EVERY problem (failed ones included), x_nom_b with step_b added
 *   num_resolves times - fp64 repeated addition, the kernels' arithmetic - so the single-launch and host-loop forms agree bitwise.
 *   mi_ilqr_set_cost with a non-NULL x_nom returns the handle to shared mode and drops both fields: it is then bitwise a
 *   never-per-problem one.  Targets are problem data: they survive mi_ilqr_reset.  Wrong `bytes` is MI_ILQR_E_BAD_SHAPE, a NaN
 *   MI_ILQR_E_BAD_ARG (the handle keeps what it had).  Every kernel family, solve, mpc_run and the stage entries. */

/* Reference trajectories (time-varying targets: a path to TRACK inside the horizon; no counterpart in the reference, whose target
 * stands still).  A handle may hold a reference x_ref, (B,T,n) with T >= 1, and an integer clock c >= 0.  While it does, every place
 * a solve uses x_nom at time index t = 0 .. N-1 (the terminal term included) uses r_t = x_ref[b, min(c + t, T-1), :] instead: past
 * its end the reference holds its last row.  Q, R, Qf stay what they are (shared or per problem, symmetric or not); MI_F_X_NOM and
 * the shared x_nom are kept but ignored while a reference is held.
 *   mi_ilqr_set(MI_F_X_REF, rows, B*T*n*8)  sets the reference; T follows from `bytes` (not a whole multiple >= 1 of B*n*8:
 *                                           MI_ILQR_E_BAD_SHAPE).  The clock stays what it was.  (NULL, 0) clears the reference and
 *                                           sets the clock to 0: the handle is then bitwise one that never held a reference.
 *   mi_ilqr_set(MI_F_REF_CLOCK, &c, 8)      the clock, an integer in [0, 2^30) held in a double (else MI_ILQR_E_BAD_ARG).
 *   mi_ilqr_get reads both back (MI_F_X_REF: `bytes` = B*T*n*8, without a reference MI_ILQR_E_BAD_ARG).
 *   mi_ilqr_solve, the resident and stage entries use the window at the current clock.  mi_ilqr_mpc_run: re-solve k = 1 .. num_resolves
 *   uses the window at c + k replan_steps - the reference moves the target, so target_step must be NULL (else MI_ILQR_E_BAD_ARG) -
 *   and leaves the clock at c + num_resolves replan_steps (a run that returns an error leaves the clock where it was); the
 *   single-launch and host-loop forms agree.  A reference of ONE row is bitwise the constant target MI_F_X_NOM with that row.
 *   mi_ilqr_mpc_run(R, r) is bitwise R calls of mi_ilqr_mpc_run(1, r) on the n = 33..40 kernels.  On the mid-size ones (n <= 32:
 *   Arm27, Arm27C, family-1 plugins) it is NOT under the default candidate policy, with a reference as with a constant target: that
 *   policy rolls four line-search candidates out once a problem has backtracked in the CURRENT launch, and which search ran decides
 *   how the cost gradients are rounded.  The forms then agree to round-off (bitwise under MI_ILQR_SPEC=2, which knows no launch).
 *   With the first reference the handle allocates a (B, N-1, n) device scratch the kernels fill with 2 r_t^T Q of the window.
 * Workgroup-per-problem kernels only (n > 8 models): handles of the wave- and lane-per-problem families return MI_ILQR_E_UNSUPPORTED.
 * A handle that holds a reference refuses MI_F_PLANT_STATE and mi_ilqr_policy_rollout, a handle that holds a plant refuses a
 * reference (MI_ILQR_E_UNSUPPORTED both ways: the plant and policy kernels know constant targets only).  Problem data: survives
 * mi_ilqr_reset.  A NaN or an infinity is MI_ILQR_E_BAD_ARG; a refused call changes nothing. */

/* Per-problem model parameters (the reference builds one solver object per System: B objects may be B plants of one structure -
 * domain-randomised MPC, parameter sweeps, picking the plant whose plan matches a measurement).  The model, dt and the costs stay
 * shared by the batch; the parameters are mi_ilqr_desc.model_params until
 *   mi_ilqr_set(MI_F_MODEL_PARAMS, rows, B*n_params*8)  gives problem b row b of the (B,n_params) array (n_params:
 *                                        mi_ilqr_model_info) and switches the handle to PER-PROBLEM PARAMETERS;
 *   mi_ilqr_set(MI_F_MODEL_PARAMS, NULL, 0)  returns it to the descriptor's parameters: it is then bitwise a handle that never left them;
 *   mi_ilqr_get returns the (B,n_params) rows in both modes (shared mode: the descriptor's row repeated);
 *   mi_ilqr_device_ptr returns the (B,n_params) device rows in per-problem mode (MI_ILQR_E_BAD_ARG in shared mode); whoever writes
 *   them on the device must leave them alone while a solve runs (the lane-per-problem kernels read a copy of their own, made by
 *   mi_ilqr_set: write through mi_ilqr_set there).
 * The rows are problem data: they survive mi_ilqr_reset.  Errors: wrong `bytes` MI_ILQR_E_BAD_SHAPE; a NaN or an infinity
 * MI_ILQR_E_BAD_ARG; a model without parameters (n_params == 0) MI_ILQR_E_UNSUPPORTED; a refused call changes nothing.  Every
 * kernel family (cluster helpers and helper wavefronts read the row of the problem they serve), control-limited handles, solve,
 * mpc_run in both forms and the stage entries; it combines with per-problem targets and per-problem control limits. */

/* PER-PROBLEM COST MATRICES (the reference's SetRunningCost / SetTerminalCost are per solver object: B objects may carry B weight
 * sets - sweeps and random searches over Q / R / Qf, inverse optimal control, a different effort penalty per robot of a fleet).
 * The matrices are the shared ones of mi_ilqr_set_cost until
 *   mi_ilqr_set(MI_F_COST_MATRICES, rows, B*(2*n*n+m*m)*8)  gives problem b row b of the (B,2*n*n+m*m) array, Q_b | R_b | Qf_b each
 *                                        row-major - the order of mi_ilqr_set_cost's matrices, without x_nom, which stays with the
 *                                        targets - and switches the handle to PER-PROBLEM COST MATRICES;
 *   mi_ilqr_set(MI_F_COST_MATRICES, NULL, 0)  returns it to SHARED mode: to whatever mi_ilqr_set_cost last set;
 *   mi_ilqr_set_cost with any of Q, R, Qf non-NULL returns it to shared mode as well (x_nom alone does not);
 *   a handle back in shared mode is bitwise a handle that never left it;
 *   mi_ilqr_get returns the (B,2*n*n+m*m) rows in both modes (shared mode: the shared matrices repeated);
 *   mi_ilqr_device_ptr returns the device rows in per-problem mode (MI_ILQR_E_BAD_ARG in shared mode); the lane-per-problem kernels
 *   read a copy of their own, made by mi_ilqr_set: write through mi_ilqr_set there.
 * Every row is classified like mi_ilqr_set_cost classifies its matrices (symmetric positive semi-definite / any other / not
 * symmetric; n >= 33: asymmetries of round-off size are averaged away first, row by row, and mi_ilqr_get returns the rows so
 * averaged), and the handle runs the most general kernel form any of its rows needs - for all rows.  Rows that all equal the
 * shared matrices give the shared handle's results bit for bit.  The rows are problem data: they survive mi_ilqr_reset.  Errors:
 * wrong `bytes` MI_ILQR_E_BAD_SHAPE; a NaN or an infinity MI_ILQR_E_BAD_ARG; a refused call changes nothing.  Every kernel family
 * (cluster helpers read the row of the problem they serve), control-limited handles, solve, mpc_run in both forms and the stage
 * entries; it combines with per-problem targets and per-problem model parameters. */

/* SetInitialState / SetInitialGuess (ilqr.py:102-109,148-156): x0 (B,n), u_guess (B,m,N-1).
 * u_guess becomes u_bar (the reference aliases it, ilqr.py:156).  NULL = keep.
 * Ordering against mi_ilqr_solve_async: the new inputs are those of the NEXT solve.  Handles of more than four problems copy them
 * on the handle's stream (the call returns at once, behind a solve that is still running); wave-per-problem handles of up to four
 * problems keep x0 / u_guess in mapped host memory that the kernels read directly (no copy engine in front of a single-problem
 * solve), so there the call WAITS for a solve still in flight before it overwrites them - a caller that pipelines
 * solve_async / set_initial / collect on such a handle serializes at set_initial.
 * Handles whose pipelined cold solves share the device (mi_ilqr_solve_async, "Solve slots") hold TWO device copies of x0 and of
 * u_guess: the write goes to the copy the next solve will read, on that solve's stream, so it waits - on the device, never the
 * host - only for solves that still read that copy, and a solve_async -> set_initial -> solve_async -> ... pipeline overlaps
 * like one that re-arms resident inputs.  A solve that follows without a set_initial reads what was written last.  x0 alone or
 * u_guess alone is fine: each input has its own copies. */
int mi_ilqr_set_initial(mi_ilqr_t* h, const double* x0, const double* u_guess);

/* The same with ONE control sequence u_guess_one (m,N-1) for every problem of the batch - the argument the
 * reference's SetInitialGuess takes (ilqr.py:148-156): m(N-1) doubles cross the bus instead of B*m*(N-1), the
 * device writes the batch's copies. */
int mi_ilqr_set_initial_shared(mi_ilqr_t* h, const double* x0, const double* u_guess_one);

/* Page-locked host memory for the buffers a caller hands to mi_ilqr_set / _get / _set_initial: the copies then
 * run as direct DMA (~55 GB/s over PCIe 5 x16) instead of through the runtime's staging of pageable memory.
 * Needs a usable device; independent of any handle. */
int mi_ilqr_host_alloc(size_t bytes, void** out);
int mi_ilqr_host_free(void* p);

/* Zero the persistent solver state (x_bar,u_bar,K,kappa,dV,fx,fu) = a freshly constructed
 * reference object (ilqr.py:70-83): a solve after it without mi_ilqr_set_initial(u_guess) /
 * mi_ilqr_rearm_initial_guess starts from u_bar = 0.  Without it the state persists across solves (F10). */
int mi_ilqr_reset(mi_ilqr_t* h);

/* Box control limits u_min <= u <= u_max (the reference's SetControlLimits, ilqr.py:158-159, which is a no-op there): u_min, u_max
 * are (m,) shared by the batch, or (B,m) when `per_problem` is non-zero; +-inf is allowed, u_min == u_max fixes an input;
 * u_min > u_max or a NaN is MI_ILQR_E_BAD_ARG.  NULL, NULL clears them: the handle is then bitwise a never-limited one again.
 * Problem data like mi_ilqr_set_cost - they survive mi_ilqr_reset and apply to solve, mpc_run (every re-solve) and the stage
 * entries.  Semantics (the convention u = u_bar - eps kappa - K (x - x_bar) kept):
 *   rollout  every trial applies u_t = clip(u_bar_t - eps kappa_t - K_t (x_t - x_bar_t), u_min, u_max), the first solve's
 *            included: an initial guess outside the box is projected, every returned u_bar lies inside it exactly;
 *   backward per step the box QP  du* = argmin 1/2 du^T Quu du + Qu^T du,  u_min - u_bar_t <= du <= u_max - u_bar_t,
 *            kappa_t = -du*; rows of K of the components du* put on a bound are 0, the free rows Quu_ff^-1 Qux_f; the value
 *            update takes its general form; MI_F_DV holds kappa_t^T Qu (the reference's Qu^T Quu^-1 Qu when nothing is
 *            clamped) and a trial's expected improvement is -(eps sum dV - eps^2/2 sum_t kappa_t^T Quu_t kappa_t);
 *            a Quu that is not positive definite stops the problem with MI_STATUS_NOT_PD (counted in stats.n_not_pd).
 * Limited handles take sequential rollouts and backward passes (the time-parallel forms carry no active set).  Wave- and
 * lane-per-problem kernels (m <= 2) and the mid-size workgroup family (n <= 32, m <= 16: MI_MODEL_ARM27, MI_MODEL_ARM27C, family-1
 * plugins built with limits; there the box QP is projected Newton and the free rows of K come from a Cholesky factor of Quu_ff);
 * on any other workgroup-per-problem handle (n > 32, or a plugin built without them) MI_ILQR_E_UNSUPPORTED, the handle stays usable. */
int mi_ilqr_set_control_limits(mi_ilqr_t* h, const double* u_min, const double* u_max, int32_t per_problem);

/* Benchmark/MPC helper: make the resident u_guess (last mi_ilqr_set_initial or
 * mi_ilqr_mpc_shift) the initial guess of the next solve again, without host traffic. */
int mi_ilqr_rearm_initial_guess(mi_ilqr_t* h);

/* Solve (ilqr.py:669-710) for every problem of the batch, on the device, to convergence.
 * Blocking, like the reference call; `stats` may be NULL.  _solve_async only enqueues the
 * kernel on the handle's stream - ONE dispatch: every solve leaves its per-problem cost / iterations / status /
 * line-search trials in its own slot of a 32-deep ring, and _collect_stats(_n) reduces all slots still owed
 * their batch statistics in one launch, synchronizes and returns them (more than 32 uncollected solves:
 * the oldest are overwritten).
 * Solve slots.  A handle of the wave-per-problem family with 4 < B <= 16 x (compute units) owns two solve slots: two sets of the
 * arrays a solve writes (x_bar, u_bar, K, kappa, dV, fx, fu, the iteration log and its cycles, the stopwatches, the key-point
 * list and counts, S2 of a limited handle), each with a stream.  A COLD _solve_async (after mi_ilqr_reset) reads no solver state,
 * so with a solve already in flight it takes the other slot and the two launches share the device: the second one's wavefronts
 * land on the SIMDs the first one's finished problems have left (one launch is one wave per SIMD and lasts as long as its slowest
 * problem).  The second slot is allocated by the first solve that can use it; a handle that never pipelines cold solves never
 * pays for it.  Results are bit for bit those of one solve at a time.  Every other launch - a warm solve, a handle with a result
 * sink, the other kernel families, mpc_run, the stage entries - and every entry point that reads or writes solver state or hands
 * out a pointer or the stream first JOINS: the current slot's stream (that of the solve enqueued last) waits on the device for the
 * other one's, then the call works on the current slot as if there were one.  A warm solve continues from the solve enqueued last.
 * MI_ILQR_SOLVE_SLOTS=1 in the environment (read once per process) gives every handle one slot: one solve at a time. */
int mi_ilqr_solve(mi_ilqr_t* h, mi_ilqr_stats* stats);
int mi_ilqr_solve_async(mi_ilqr_t* h);
int mi_ilqr_collect_stats(mi_ilqr_t* h, mi_ilqr_stats* stats);
/* Up to 32 solves may be enqueued with _solve_async before collecting (each keeps its own kernel
 * events and statistics record): the statistics of the last `count` of them, oldest first. */
int mi_ilqr_collect_stats_n(mi_ilqr_t* h, int32_t count, mi_ilqr_stats* stats);

/* Stage-level entries (parity tests).
 * rollout : one line-search trial per problem with the given eps (ilqr.py:306-327)
 *           -> MI_F_X_TRIAL / MI_F_U_TRIAL / MI_F_TRIAL_COST.
 * forward : _forward_pass (ilqr.py:339-378): line search against L_last (B,; +inf allowed),
 *           linearization at the accepted trajectory, commit to x_bar/u_bar -> MI_F_COST,
 *           HIST row 0 holds (L, eps, ls, pct).
 * linearize: _get_derivatives (ilqr.py:380-415) at the current x_bar/u_bar.
 * backward: _backward_pass (ilqr.py:623-667). */
int mi_ilqr_rollout(mi_ilqr_t* h, const double* eps);
int mi_ilqr_forward(mi_ilqr_t* h, const double* L_last);
int mi_ilqr_linearize(mi_ilqr_t* h);
int mi_ilqr_backward(mi_ilqr_t* h);

/* MPC warm start on the device (acrobot.py:147-152, mini_cheetah.py:193-198):
 * x0 <- x_bar[:, replan_steps]; u_bar <- [u_bar[:, replan_steps:], repeat(u_bar[:, -1])]. */
int mi_ilqr_mpc_shift(mi_ilqr_t* h, int32_t replan_steps);

/* The whole receding-horizon loop of acrobot.py:145-155 / mini_cheetah.py:190-201 on the device:
 * `num_resolves` times { mpc_shift(replan_steps); x_nom += target_step (may be NULL); Solve }.
 * For the wave-per-problem kernels this is ONE launch and the solver state stays in LDS between
 * re-solves; the workgroup-per-problem kernel (n = 36) runs the loop in one launch as well.  Per
 * re-solve the log keeps (x0 (n), cost, iterations) for every problem:
 * mi_ilqr_get_mpc_log -> (B, num_resolves, n+2).  stats aggregate the whole loop; the per-problem status
 * is that of the LAST re-solve (a loop that hits a line-search failure stops there).
 * Limits of the single-launch form: wave-per-problem kernels N <= 512 (the in-kernel shift holds eight
 * controls per lane), workgroup-per-problem kernel m*(N-1) <= 2048.  Beyond them, and for the
 * lane-per-problem "throughput" kernels, the same loop runs as shift + solve launches from the host:
 * same results, same log (filled after each re-solve).
 * A problem whose re-solve r FAILS (line search, MI_STATUS_NOT_PD, internal) gets row r of the log and none after it:
 * the log is zero-filled at every call and both forms stop logging the problem there (rows r+1.. read as zeros).  The
 * single-launch forms also stop RE-SOLVING it (its status is that of re-solve r); the host-loop form's batched launches
 * cannot leave a problem out - it is shifted and solved on, and its final status is the last re-solve's.
 * Per-problem targets (MI_F_X_NOM / MI_F_TARGET_STEP, after mi_ilqr_set_cost): target_step must be NULL (else MI_ILQR_E_BAD_ARG),
 * each problem's target moves by its own (B,n) row before each re-solve, and MI_F_X_NOM holds x_nom_b + step_b added num_resolves
 * times afterwards, in both forms. */
int mi_ilqr_mpc_run(mi_ilqr_t* h, int32_t num_resolves, int32_t replan_steps, const double* target_step, mi_ilqr_stats* stats);
int mi_ilqr_get_mpc_log(mi_ilqr_t* h, double* dst, size_t bytes);

/* Copy a field out / in (host memory; `bytes` must equal the field size - except that the per-iteration records MI_F_HIST and
 * MI_F_ITER_CYCLES may be read in part: `bytes` = any whole number of 32-byte rows < the field size returns the LEADING rows of
 * the first problem, also through mi_ilqr_get_async and mi_ilqr_solve_into; the drop-in class keeps a 4096-row log and copies 64
 * rows with the solve, the rest only after a solve that took more iterations - the reference's table has every row, ilqr.py:704). */
int mi_ilqr_get(mi_ilqr_t* h, int which, double* dst, size_t bytes);
int mi_ilqr_get_int(mi_ilqr_t* h, int which, int32_t* dst, size_t bytes);
int mi_ilqr_set(mi_ilqr_t* h, int which, const double* src, size_t bytes);

/* Enqueue the copy-out of a field (double or int32) on the handle's stream and return: `dst` is defined after
 * the next mi_ilqr_synchronize / _collect_stats.  Meant for page-locked destinations (mi_ilqr_host_alloc): several
 * results of a solve then cost one synchronization instead of one each.  Fields that need a layout conversion
 * (the n = 36 and lane-per-problem kernels' trajectory arrays) are copied before the call returns, like mi_ilqr_get. */
int mi_ilqr_get_async(mi_ilqr_t* h, int which, void* dst, size_t bytes);

/* Result sink (wave-per-problem kernels; MI_ILQR_E_UNSUPPORTED for the n = 36/37 and lane-per-problem layouts): three
 * host arrays from mi_ilqr_host_alloc - x_bar (B,n,N), u_bar (B,m,N-1), cost (B,), the boundary's layouts - that every
 * later solve / mpc_run kernel ALSO writes its results into, problem by problem as each finishes, over the host link:
 * after mi_ilqr_collect_stats / mi_ilqr_synchronize they hold what mi_ilqr_get would return, and the copy-out of the
 * batch has overlapped the launch's slowest problems instead of following it (Solve() through the class surface:
 * 0.32 -> 0.2x ms at B = 1024).  The arrays must stay allocated while the sink is set; three NULLs clear it.
 * The persistent state in HBM is written as always (warm starts, mi_ilqr_get). */
int mi_ilqr_set_result_sink(mi_ilqr_t* h, double* x_bar_host, double* u_bar_host, double* cost_host);

/* One blocking solve whose results land in caller memory, ONE host synchronization, one call across the boundary (the
 * single-problem Solve() of the drop-in class: C1's latency is host overhead as much as kernel time): x_bar (B,n,N), u_bar
 * (B,m,N-1), cost (B,) - written by the kernel itself as each problem finishes when `page_locked` is non-zero, the three come
 * from mi_ilqr_host_alloc and the kernel family has a result sink (set for THIS solve only), copied out behind the solve
 * otherwise - plus `n_extra` further fields (double or int selectors: which[i] -> dst[i], bytes[i] as for mi_ilqr_get_async)
 * queued behind it.  stats and sink_used (1: the kernel wrote the three arrays itself) may be NULL. */
int mi_ilqr_solve_into(mi_ilqr_t* h, double* x_bar, double* u_bar, double* cost, int32_t page_locked, int32_t n_extra,
                       const int32_t* which, void* const* dst, const size_t* bytes, mi_ilqr_stats* stats, int32_t* sink_used);

/* Raw device pointer of a double field (for zero-copy consumers, e.g. a torch tensor
 * view feeding the RCCL best-cost reduction), and the handle's stream.  The per-problem result scalars
 * (MI_F_COST, MI_I_ITERS, MI_I_STATUS, MI_I_LS_TRIALS) rotate through a ring, one slot per
 * mi_ilqr_solve / mi_ilqr_solve_async: ask for their pointer again after each solve.  The same holds for the state fields
 * (MI_F_X_BAR .. MI_F_FU, MI_F_HIST, MI_F_ITER_CYCLES, the key-point fields, MI_I64_STAGE_CYCLES) and MI_F_X0 of a handle with two
 * solve slots (mi_ilqr_solve_async): the pointer is that of the solve enqueued last - ask again after each solve.
 * mi_ilqr_get_stream: the stream of the solve enqueued last, made to wait (on the device) for the other slot's stream first - work
 * a caller enqueues on it runs behind every solve enqueued so far, and a later solve of the handle behind that work.  Ask again
 * after each solve here as well. */
int mi_ilqr_device_ptr(mi_ilqr_t* h, int which, void** ptr, size_t* bytes);
int mi_ilqr_get_stream(mi_ilqr_t* h, void** hip_stream);
int mi_ilqr_synchronize(mi_ilqr_t* h);

/* ---- multi-GPU: the path's one collective -------------------------------------------
 * Problems are independent: every rank (one process per GPU) owns a handle over its contiguous shard of
 * the batch and no kernel ever exchanges data.  The only cross-rank step is the reduction of the best
 * total cost at the end of a batched solve: ONE RCCL all-reduce(min) of a few doubles over xGMI, here so
 * that a C caller needs nothing but this header.  librccl is loaded on first use (dlopen); without it
 * these entries return MI_ILQR_E_RCCL and everything else keeps working.
 *   rank 0:  mi_ilqr_comm_unique_id(id)  ->  ship the MI_ILQR_COMM_ID_BYTES bytes to every rank over the
 *            launcher's own channel (MPI_Bcast, a file, a TCP store)
 *   all:     mi_ilqr_comm_create(id, rank, world, device_id, &comm)          (collective call)
 *   all:     mi_ilqr_allreduce_min(comm, values, count)                      (blocking; in place)
 *        or  mi_ilqr_allreduce_min_start / _wait: the reduction runs on the communicator's own stream and
 *            overlaps the next solve; at most one in flight per communicator; count <= 64. */
#define MI_ILQR_COMM_ID_BYTES 128
#define MI_ILQR_COMM_MAX_COUNT 64
typedef struct mi_ilqr_comm mi_ilqr_comm_t;
int mi_ilqr_comm_unique_id(void* id_bytes);
int mi_ilqr_comm_create(const void* id_bytes, int32_t rank, int32_t world, int32_t device_id, mi_ilqr_comm_t** out);
void mi_ilqr_comm_destroy(mi_ilqr_comm_t* c);
/* The communicator's own answer (ncclCommCount, ncclCommUserRank): how many ranks it spans and which one this is - what a
 * multi-GPU bench line reports so that a scaling record can be checked from the line alone (ABI 9).  `rank` may be NULL. */
int mi_ilqr_comm_count(mi_ilqr_comm_t* c, int32_t* ranks, int32_t* rank);
int mi_ilqr_allreduce_min(mi_ilqr_comm_t* c, double* values, int32_t count);
int mi_ilqr_allreduce_min_start(mi_ilqr_comm_t* c, const double* values, int32_t count);
int mi_ilqr_allreduce_min_wait(mi_ilqr_comm_t* c, double* values, int32_t count);

/* Per-problem in-kernel stopwatches of the last solve, shader-clock cycles, (B,4):
 * line search, linearization, backward pass, whole Solve loop — the device counterpart
 * of the reference's time_fp / time_getDerivs / time_backwardsPass (ilqr.py:364-372,696-699). */
int mi_ilqr_get_cycles(mi_ilqr_t* h, int64_t* dst, size_t bytes);

/* HIP-event duration of the most recent kernel launch of the handle (0 if that launch was not timed).  For a pipelined cold solve
 * that shared the device with its neighbours (mi_ilqr_solve_async, "Solve slots") this is the span of that dispatch WHILE it
 * shares the device, not the time it would take alone. */
int mi_ilqr_last_kernel_ms(mi_ilqr_t* h, float* ms);

/* Which launches carry their start/stop events: every one (every = 1, the default), the first of every `every`
 * solves, or none (every = 0).  The events ride on the solve kernel's own dispatch packet, but a profiled dispatch
 * still serializes a pipelined stream by ~5 us; a caller that enqueues solves back to back (mi_ilqr_solve_async)
 * and wants kernel_ms only as a sample asks for one in k.  Untimed launches report kernel_ms = 0.  Timed launches overlap like
 * the others on a handle with two solve slots; kernel_ms of an overlapped launch is its span while it shares the device (the
 * exclusive kernel time is what MI_ILQR_SOLVE_SLOTS=1 measures). */
int mi_ilqr_set_timing(mi_ilqr_t* h, int32_t every);

/* Algorithmic bytes of one iteration of one problem with `ls` line-search trials. */
double mi_ilqr_bytes_per_iteration(int32_t n, int32_t m, int32_t N, int32_t ls);

/* LDS bytes one problem occupies in the wave-per-problem kernels (0 if unsupported). */
size_t mi_ilqr_lds_bytes(const mi_ilqr_desc* desc);

/* Monte-Carlo rollouts of the feedback policy the handle holds (x_bar, u_bar, K - after a solve, mpc_run or mi_ilqr_set; the reference
 * stores K for exactly this, ilqr.py:712-733): S samples per problem, one GPU lane per sample, in ONE call.  For problem b, sample s,
 * x_0 = x0[b,s], t = 0 .. N-2:
 *     u_t = u_bar[b,:,t] - K[b,:,:,t] (x_t - x_bar[b,:,t])      (ilqr.py:313 with eps = 0; clamped to problem b's box on a handle
 *                                                                 with control limits set)
 *     x_{t+1} = f(x_t, u_t; params[b,s], dt)
 *     L += (x_t - x_nom_b)' Q_b (x_t - x_nom_b) + u_t' R_b u_t  (ilqr.py:325),   L += the Qf_b term at x_{N-1}  (ilqr.py:327)
 * with the handle's cost matrices and targets (per-problem where set).  All pointers are HOST arrays:
 *   x0      (B,S,n)       in   initial states
 *   params  (B,S,n_params) in  or NULL: every sample of problem b runs on problem b's own parameters (MI_F_MODEL_PARAMS row, else
 *                              the descriptor's)
 *   cost    (B,S)         out  +inf for a sample that ended early
 *   x_final (B,S,n)       out  or NULL: the last state the sample held
 *   steps   (B,S) int32   out  or NULL: steps completed, N-1 for a full rollout
 *   X       (B,S,n,N)     out  or NULL;   U (B,S,m,N-1) out or NULL: the trajectories, NaN in the columns a sample did not reach
 * A sample ENDS at a step the model declares infeasible (MI_MODEL_PLANAR_QUAD, MI_MODEL_QUAD3D: ilqr.py:315-323) or whose result is
 * not finite, and before its first step when its x0 is not finite - that is data, not an error: steps then says how far it came
 * (X holds steps + 1 columns, U steps), x_final is the state it stopped in, and the other samples are unaffected.
 * The handle is only READ: solver state, x0, warm start, statistics, events and MI_F_* results stay what they were, a solve after
 * the call is bitwise the solve without it.  Runs on the handle's stream with one synchronization; staging memory is the handle's
 * grow-only scratch.  Errors: S < 1, NULL x0 or cost MI_ILQR_E_BAD_ARG; params for a model with n_params == 0
 * MI_ILQR_E_UNSUPPORTED; a NaN or an infinity in params MI_ILQR_E_BAD_ARG.  Every model and kernel family (additive in ABI 10). */
int mi_ilqr_policy_rollout(mi_ilqr_t* h, int32_t S, const double* x0, const double* params, double* cost, double* x_final,
                           int32_t* steps, double* X, double* U);

/* Process and actuation noise of the policy rollouts (additive in ABI 10: two selectors of mi_ilqr_set / mi_ilqr_get, no new entry
 * point).  On a handle that holds a MI_F_POLICY_NOISE array every step of mi_ilqr_policy_rollout is disturbed:
 *     u_t     = u_bar_t - K_t (x_t - x_bar_t)                       clamped on a limited handle, as above: the COMMANDED control
 *     x_{t+1} = f(x_t, u_t + sigma_u o xi^u_t) + sigma_x o xi^x_t    xi: independent standard normals, o: component by component
 *     L      += (x_t - x_nom)' Q (x_t - x_nom) + u_t' R u_t          with the commanded u_t
 * U holds the commanded controls, X the noisy states.  The disturbance on u is added after the clamp and is not clamped again (an
 * external disturbance, not a command).  The finite and infeasible checks look at the noisy x_{t+1}; ended samples, steps, x_final
 * and the NaN columns are as above.  x0 gets no noise; padding controls get none and stay exact zeros.
 *   mi_ilqr_set(MI_F_POLICY_NOISE, rows, B*(n+m)*8)  row b = sigma_x (n) | sigma_u (m, the DEVICE's number of controls) of problem b:
 *                                            standard deviations, zero where a component is to get no noise.  Survives mi_ilqr_reset.
 *   mi_ilqr_set(MI_F_POLICY_NOISE, NULL, 0)  clears it: the next rollout runs the noise-free kernel again, bitwise as before it was set.
 *   mi_ilqr_set(MI_F_POLICY_STREAM, v, 24)   v = seed | first_sample | common, each an integer value: seed in [0, 2^53), first_sample
 *                                            in [0, 2^32), common 0 or 1.  Default 0 | 0 | 0.
 *   mi_ilqr_get reads both back; MI_F_POLICY_NOISE reads as zeros while it is not set.
 * Errors: a negative, NaN or infinite sigma, a non-zero sigma on a padding control, a stream value that is not such an integer:
 * MI_ILQR_E_BAD_ARG; wrong `bytes`: MI_ILQR_E_BAD_SHAPE; a refused call changes nothing.  A rollout with noise set and
 * first_sample + S > 2^32: MI_ILQR_E_BAD_ARG.
 * The generator is counter-based: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with
 *     key     = (seed mod 2^32, seed div 2^32)
 *     counter = (first_sample + s, t, common ? 0 : b, j)     j = i / 4 for state component i, j = 256 + k / 4 for control component k
 * and the normal of a component is made from word (i mod 4) of block j by Box-Muller: words (w0, w1) give u_a = (w0 + 1/2) 2^-32,
 * u_b = (w1 + 1/2) 2^-32, z0 = r cos(2 pi u_b), z1 = r sin(2 pi u_b) with r = sqrt(-2 ln u_a); words (w2, w3) give z2, z3 the same
 * way (|z| <= 6.77).  So a normal depends on (seed, b, s, t, component) only - not on S, not on the model, not on how the samples
 * are spread over calls: S samples from first_sample = k are samples k .. k + S - 1 of one long call, and common = 1 gives every
 * problem the same disturbances (common random numbers).  The handle stays read-only for solves: a solve after a noisy rollout is
 * bitwise the solve without it. */

/* Closed-loop MPC: a plant of its own inside mi_ilqr_mpc_run (additive in ABI 10: six selectors of mi_ilqr_set / mi_ilqr_get, no new
 * entry point).  mi_ilqr_mpc_run starts every re-solve from its own prediction, x0 <- x_bar[:, replan_steps]: the controller never
 * meets a plant that differs from its model.  A handle that HOLDS A PLANT - one state per problem, optionally parameters and
 * disturbances of its own - runs each of the num_resolves rounds of mi_ilqr_mpc_run(h, num_resolves, replan_steps, ..) as
 *   1. the plants advance replan_steps steps under the policy the handle holds from the previous solve; for j = 0 .. replan_steps-1,
 *      k = the plant clock + j:
 *          u_k     = u_bar[:, j] - K[:, :, j] (x_k - x_bar[:, j])        clamped to the problem's box on a handle with control limits;
 *                                                                        u_bar[:, j] (clamped likewise) with feedback off
 *          x_{k+1} = f(x_k, u_k + sigma_u o xi^u_k; plant parameters of b, dt) + sigma_x o xi^x_k
 *          l_k     = (x_k - x_nom_b)' Q_b (x_k - x_nom_b) + u_k' R_b u_k   the matrices and the target the executed plan was solved for
 *      padding controls stay exact zeros; the disturbance on u comes after the clamp and is not clamped again; the log keeps the
 *      row x_k | u_k (commanded) | l_k;
 *   2. mi_ilqr_mpc_shift(replan_steps) as ever - the warm start - and then x0 <- the plant's state, a copy on the device;
 *   3. the targets move (target_step / MI_F_TARGET_STEP), the solve runs, row r of the MPC log is written (its x0 IS the plant's state);
 *   4. the clock advances by replan_steps.
 * Such a run always takes the host-loop form of mi_ilqr_mpc_run (shift + solve launches, every kernel family; the plant is a kernel
 * of its own between them, one GPU lane per problem).  A plant whose step is infeasible (MI_MODEL_PLANAR_QUAD, MI_MODEL_QUAD3D) or
 * not finite ENDS there - the rule of mi_ilqr_policy_rollout, applied to the noisy x_{k+1}; that is data, not an error: it keeps its
 * last state, its log row of that step is x_k | NaN | NaN and its later rows are NaN, the MPC log has no row for it from that round
 * on (they read as zeros, like the rows after a failed re-solve), and - the host loop cannot leave a problem out - it is solved on
 * from that last state; no non-finite x0 ever reaches a solve and the other problems are untouched.  It runs again once
 * MI_F_PLANT_STATE is set again.  Without a plant mi_ilqr_mpc_run takes exactly the paths it took before, bit for bit.
 *   mi_ilqr_set(MI_F_PLANT_STATE, x, B*n*8)   the handle holds a plant from now on (every plant running); a NaN or an infinity:
 *                                             MI_ILQR_E_BAD_ARG.  (NULL, 0) clears it.  mi_ilqr_get: the plants' current states
 *                                             (MI_ILQR_E_BAD_ARG without a plant).  Survives mi_ilqr_reset, like the other five.
 *   mi_ilqr_set(MI_F_PLANT_PARAMS, rows, B*n_params*8)   the plants' own parameters, the rules of MI_F_MODEL_PARAMS (MI_ILQR_E_UNSUPPORTED
 *                                             for a model without parameters); (NULL, 0) or never set: problem b's model row
 *                                             (MI_F_MODEL_PARAMS, else the descriptor's), which is also what mi_ilqr_get returns then.
 *   mi_ilqr_set(MI_F_PLANT_NOISE, rows, B*(n+m)*8)   sigma_x | sigma_u with the rules and errors of MI_F_POLICY_NOISE; (NULL, 0) clears it
 *                                             and the noise-free plant kernel runs again.  Independent of MI_F_POLICY_NOISE.
 *   mi_ilqr_set(MI_F_PLANT_STREAM, v, 32)     v = seed | clock | common | feedback, integer values: seed in [0, 2^53), clock in [0, 2^32),
 *                                             common and feedback 0 or 1.  Default 0 | 0 | 0 | 1.  mi_ilqr_mpc_run writes the advanced
 *                                             clock back; a run whose clock would pass 2^32 (clock + num_resolves * replan_steps > 2^32)
 *                                             returns MI_ILQR_E_BAD_ARG before anything is launched.
 *   mi_ilqr_get(MI_F_PLANT_LOG, dst, B*num_resolves*replan_steps*(n+m+1)*8)   the rows of the last closed-loop run; wrong `bytes`
 *                                             MI_ILQR_E_BAD_SHAPE, before any such run MI_ILQR_E_BAD_ARG (MI_F_PLANT_KERNEL_MS likewise).
 * m is the DEVICE's number of controls throughout.  A refused call changes nothing.  The normals are those of the policy rollouts:
 * Philox4x32-10 under the key (seed mod 2^32, seed div 2^32) with
 *     counter = (0, k, common ? 0 : b, j)     j = i / 4 for state component i, j = 256 + c / 4 for control component c
 * and the same Box-Muller - so the plant of problem b at clock k gets the normals that SAMPLE 0 of a policy rollout
 * (first_sample = 0) gets at step t = k: from clock 0, with the same seed and sigmas, the first segment of a closed-loop run is the
 * first replan_steps steps of that rollout. */

/* Monte-Carlo on the device (additive in ABI 10: four selectors of mi_ilqr_set / mi_ilqr_get, no new entry point).
 * mi_ilqr_policy_rollout takes every sample's x0 from the host and returns every sample's result to it.  Here the samples are DRAWN
 * where they are used and their costs are REDUCED on the device: per problem ten numbers come back, and nothing of size S crosses
 * the bus unless the caller asks for the samples.  For problem b and the global sample number g = first_sample + s, s = 0 .. S-1:
 *   start state   x0[i] = x0_mean[b,i] + x0_spread[b,i] d_i
 *   parameters    p[j]  = p_mean[b,j] + p_spread[b,j] d_j            with sample_params = 1 (models with n_params > 0); else every sample
 *                                                                    runs on problem b's own row, as mi_ilqr_policy_rollout with params = NULL
 *   d, normal  (dist = 0): the Box-Muller normal (as above) of word pair (i mod 4) of the Philox block 512 + i / 4 (parameters: 768 + j / 4)
 *   d, uniform (dist = 1): d = (w + 1/2) 2^-31 - 1 with w word i mod 4 of that block: exact in fp64, inside (-1, 1), so the draw lies
 *                          in mean +- spread
 *   counter = (g, 0, common ? 0 : b, block) under the key of MI_F_POLICY_STREAM's seed - the key of the disturbances, which use the
 *   blocks 0 .. 9 and 256 .. 259 only: draws and noise are independent under one seed.  A draw depends on (seed, b, g, component) only,
 *   not on S, the launch geometry or the model; common = 1 gives every problem the same d.  A spread of zero returns the mean's bits.
 * The rollout is mi_ilqr_policy_rollout's, with MI_F_POLICY_NOISE's disturbances when they are set: the policy, the clamp, the rule by
 * which a sample ends, the commanded-control cost, per-problem Q / R / Qf / x_nom, limits and padding controls are unchanged.  The two
 * kernels run the same arithmetic on a sample; what the compiler may do differently in them is which multiply it fuses into which
 * add (FMA contraction), so a sample's cost agrees with what mi_ilqr_policy_rollout returns for the same x0, parameters and stream
 * up to the last bits, and its steps agree unless a state lies within that of a feasibility bound.  BIT FOR BIT equality is what
 * this build was measured to give, and what its tests hold it to, for the models listed under "Monte-Carlo on the device" in
 * DESIGN.md (4.2h) - not a property of the interface.
 * A sample is COUNTED iff it ran all N-1 steps and its cost is finite.  The result of problem b, ten doubles:
 *     S | counted | success | mean | M2 | min | max | argmin | argmax | steps_total
 * mean, M2 (the sum of squared deviations from the mean), min and max run over the counted samples; argmin / argmax are global sample
 * numbers g, ties go to the lower g; steps_total is the sum of the steps of ALL S samples; success counts the counted samples with
 * |x_final_i - x_nom_b,i| <= goal[b,i] for every i (a goal of +inf ignores the component).  counted = 0: mean = M2 = NaN, min = +inf,
 * max = -inf, argmin = argmax = -1.
 * The REDUCTION ORDER is fixed and part of the contract: the samples form groups of 64 by s / 64; a group's statistic is the butterfly
 * over lane distance 1, 2, 4, 8, 16, 32 of Chan's merge of (count, mean, M2) -
 *     n = nA + nB,  delta = meanB - meanA,  mean = meanA + delta (nB / n),  M2 = (M2A + M2B) + (delta delta) ((nA nB) / n)
 * with A always the operand from the lower lane, and a merge with a count-0 operand returning the other operand's bits; the groups
 * of a problem are then folded left to right in group order.  Lanes past a ragged tail and uncounted samples enter with count 0.
 * The host runs the groups in windows (about 64 MB of the grow-only scratch per pass; the environment variable
 * MI_ILQR_MC_PASS_GROUPS=k, read once, forces windows of k groups): the result does not depend on the window, bit for bit, and S is
 * bounded by 2^32 - first_sample, not by memory.
 *   mi_ilqr_set(MI_F_POLICY_MC_DIST, rows, B*(3n+2n_params)*8)   row b = x0_mean | x0_spread | goal | p_mean | p_spread.  (NULL, 0)
 *                                            clears the rows.  Survives mi_ilqr_reset.  mi_ilqr_get reads them back (zeros while not set).
 *                                            Refusals: a NaN anywhere, a mean or spread that is not finite, a negative spread or goal:
 *                                            MI_ILQR_E_BAD_ARG; wrong `bytes`: MI_ILQR_E_BAD_SHAPE.  A refused call changes nothing.
 *   mi_ilqr_set(MI_F_POLICY_MC_RUN, v, 40)   v = S | x0_dist | p_dist | sample_params | samples, integers held in doubles: RUNS the
 *                                            evaluation on the handle's stream and synchronizes once (a run of more than 32 passes: once every 32).  Seed, first_sample and common are
 *                                            MI_F_POLICY_STREAM's, the noise MI_F_POLICY_NOISE's.  Refusals: no MI_F_POLICY_MC_DIST rows,
 *                                            S < 1, first_sample + S > 2^32, a value that is no such integer: MI_ILQR_E_BAD_ARG;
 *                                            sample_params = 1 on a model without parameters, and a handle that holds a reference
 *                                            trajectory (like mi_ilqr_policy_rollout): MI_ILQR_E_UNSUPPORTED; wrong `bytes`:
 *                                            MI_ILQR_E_BAD_SHAPE.  A refused run leaves the rows and the last results in place.
 *                                            Write-only: mi_ilqr_get refuses it.  The handle's solver state is only READ: a solve after
 *                                            the run is bitwise the solve without it.
 *   mi_ilqr_get(MI_F_POLICY_MC_STATS, dst, B*10*8)   the last run's result; before any run MI_ILQR_E_BAD_ARG.
 *   mi_ilqr_get(MI_F_POLICY_MC_SAMPLES, dst, B*S*(n+n_params+2)*8)   rows x0 | params | cost | steps (a double) of every sample of the last
 *                                            run, when that run had samples = 1 - otherwise MI_ILQR_E_BAD_ARG.  params: the drawn
 *                                            parameters, or problem b's row when they were not drawn.
 *   MI_F_POLICY_KERNEL_MS after a run: the rollout kernels of that run, summed over its passes.  The fold kernels are NOT included.
 *   mi_ilqr_get_int(MI_I_POLICY_MC_PASSES, &k, 4): the passes that run took (before any run MI_ILQR_E_BAD_ARG). */

/* ---- Envelopes and a safety box (ABI 10; selectors of mi_ilqr_set / mi_ilqr_get, no new entry point) ----
 * What a MI_F_POLICY_MC_RUN observes BESIDE the cost, reduced on the device: per-step statistics of the states and of the controls over
 * the samples, and the samples that stay inside a box.  The values reduced are the trajectories mi_ilqr_policy_rollout returns for the
 * same samples (X, U: NaN from the step at which a sample ended); nothing of size S crosses the bus.  A run that observes nothing
 * is the run it was: its ten numbers, its samples, MI_F_POLICY_KERNEL_MS and its pass count do not change.
 *   mi_ilqr_set(MI_F_POLICY_MC_OBSERVE, &v, 8)   v = 0 .. 3, an integer held in a double: bit 0 state envelopes, bit 1 control
 *                                            envelopes.  Persists on the handle.  Any other value: MI_ILQR_E_BAD_ARG.
 *   mi_ilqr_set(MI_F_POLICY_MC_BOX, rows, B*2n*8)   row b = lo | hi, +inf / -inf = unbounded.  A NaN or lo > hi: MI_ILQR_E_BAD_ARG.
 *                                            (NULL, 0) clears the box.  While the handle holds a box, runs observe it.  mi_ilqr_get
 *                                            reads the rows back (zeros while not set).  Survives mi_ilqr_reset.
 * THE FOLD.  A row is one (t, i) of one problem: the S values x_t[i] (u_t[k]) of its samples.  Per row eight doubles,
 *     count | K | s1 | s2 | min | max | argmin | argmax
 * are a LEFT FOLD in global sample order g = first_sample + s, s ascending: a non-finite v is skipped; the first finite v sets K = v;
 * then d = v - K, s1 += d, s2 += d d (a rounded product, then a rounded sum: no FMA), count += 1; min and max use strict comparisons, so
 * a tie keeps the lower sample number; argmin / argmax are global sample numbers.  An empty row: count = 0, K = s1 = s2 = 0,
 * min = +inf, max = -inf, argmin = argmax = -1.  The caller finalises:
 *     mean = K + s1 / count,   M2 = max(0, s2 - s1 s1 / count)
 * (the shifted-data one-pass variance; M2 the sum of squared deviations from the mean).  The order is fixed and nothing is contracted:
 * the eight doubles do not depend on the window (MI_ILQR_MC_PASS_GROUPS), bit for bit.
 * THE BOX.  Per sample: ran - all N states are finite; the state x_t is OUTSIDE if x_t[i] < lo[i] or x_t[i] > hi[i] for some i
 * (comparisons: a NaN is never outside, a value on a bound is inside); exit - the first t at which the sample is outside, t = 0
 * included; safe = ran and never outside; safe_success = safe and |x_{N-1}[i] - x_nom_b[i]| <= goal[b,i] for every i (the success
 * criterion above, on the run's target and goal rows).  The box only observes: a sample goes on after leaving it.  Per problem
 *     ran | safe | safe_success | exits[0 .. N-1]
 * with exits[t] the number of samples whose first outside state is x_t; integers, added as integers.
 *   mi_ilqr_get(MI_F_POLICY_MC_ENVELOPE, dst, B*N*n*8*8)        the state rows of the last run, when bit 0 was set for it
 *   mi_ilqr_get(MI_F_POLICY_MC_ENVELOPE_U, dst, B*(N-1)*m*8*8)  the control rows (the COMMANDED controls, m the device's: padding
 *                                            controls read as exact zeros), when bit 1 was set
 *   mi_ilqr_get(MI_F_POLICY_MC_SAFETY, dst, B*(3+N)*8)          the counters, when the handle held a box
 *                                            When the last run did not produce them: MI_ILQR_E_BAD_ARG.  Setting one of the three:
 *                                            MI_ILQR_E_BAD_ARG (read-only).  Wrong `bytes` anywhere: MI_ILQR_E_BAD_SHAPE.  A refused
 *                                            call changes nothing.
 * The trajectories of a window of samples stay in the handle's grow-only scratch (about 1 GiB per pass at most, never less than one
 * group of 64 samples per problem); when that memory cannot be had the run is refused with MI_ILQR_E_UNSUPPORTED and the last results
 * stay in place. */

/* ---- Multi-start (ABI 10; selectors of mi_ilqr_set / mi_ilqr_get, no new entry point) ----
 * iLQR is a local method: the answer depends on the initial guess.  A handle of B problems is read as G = B / K SEED GROUPS of K
 * consecutive problems: group g holds problems g K .. g K + K - 1, meant to be the same problem (x0, target, costs, parameters - not
 * checked) under K different guesses.  Four operations work on the handle's resident state, one kernel each (one workgroup per
 * group); nothing of size B m (N-1) crosses the bus.
 * PERTURB (op 0).  u_guess[b,j,t] = base[b,j,t] + sigma_u[b,j] z(seed, round, b, t div hold, j) for every member k >= 1 of every
 * group; member 0, the ELITE slot, gets base unchanged, so best-of-K is never worse than the single start.  base is what the next
 * solve would have started from: the pending guess, else u_bar, else zeros (a fresh or reset handle).  z is a standard normal:
 * Philox4x32-10 under the key (seed mod 2^32, seed div 2^32) at counter = (round, t div hold, b, 768 + j / 4), Box-Muller normal
 * j mod 4 of the block (words (0, 1) -> normals 0, 1; words (2, 3) -> normals 2, 3, as under "Process and actuation noise").  A normal
 * depends on (seed, round, b, t div hold, j) and nothing else: not on K, not on the launch, not on the layout.  hold >= 1 keeps the
 * disturbance constant over `hold` steps.  sigma z is a rounded product, the sum a rounded sum (no FMA); where sigma = 0, and on
 * padding controls, the element is base bit for bit.  The result is not clamped on a handle with control limits: the rollouts clamp.
 * Afterwards the handle is where mi_ilqr_reset followed by mi_ilqr_set_initial(u_guess) would leave it: cold, the guess pending.
 * SELECT (op 1).  A member is ELIGIBLE iff its status with MI_STATUS_FLAG_INDEFINITE masked off is MI_STATUS_CONVERGED or
 * MI_STATUS_MAX_ITERS and its cost is finite.  The winner is the eligible member of least cost, ties go to the lowest index.  Per
 * group three doubles: winner (the member index k) | its cost | the number of eligible members; no eligible member: -1 | +inf | 0.
 * RESEED (op 2).  Select, then rebuild the guesses: the winner's slot gets its own u_bar unperturbed, every other member the winner's
 * u_bar plus the noise of PERTURB at this round.  A group without a winner falls back to PERTURB with each member's own u_bar as
 * base, non-finite entries read as 0.  The handle ends as after PERTURB.
 * GATHER (op 3).  Select, then the winners' x_bar (G,n,N), u_bar (G,m,N-1) and cost (G,); a group without a winner: NaN rows, +inf.
 * SELECT and GATHER change nothing in the solver's state: a solve after them is bitwise the solve without them.
 *   mi_ilqr_set(MI_F_SEEDS_SIGMA, rows, B*m*8)   row b = sigma_u of problem b, m the device's control dimension: finite, non-negative,
 *                                            zero on padding controls - else MI_ILQR_E_BAD_ARG; wrong `bytes`: MI_ILQR_E_BAD_SHAPE.
 *                                            (NULL, 0) clears the rows (zeros).  Survives mi_ilqr_reset; mi_ilqr_get reads them back.
 *   mi_ilqr_set(MI_F_SEEDS_RUN, v, 48)       v = K | op | seed | round | hold | reserved = 0, integers held in doubles: RUNS the
 *                                            operation on the handle's stream and synchronizes once.  Refusals: K < 1, K not dividing
 *                                            B, an unknown op, hold < 1, a seed outside [0, 2^53), a round outside [0, 2^32), a value
 *                                            that is no such integer, reserved != 0: MI_ILQR_E_BAD_ARG; a handle whose inputs live in
 *                                            host memory (B <= 4 on the wave-per-problem kernels): MI_ILQR_E_UNSUPPORTED; wrong `bytes`:
 *                                            MI_ILQR_E_BAD_SHAPE.  A refused command changes nothing.  Write-only.
 *   mi_ilqr_get(MI_F_SEEDS_BEST, dst, G*3*8) the rows of the last SELECT, RESEED or GATHER; before any: MI_ILQR_E_BAD_ARG.
 *   mi_ilqr_get(MI_F_SEEDS_X_BAR, dst, G*n*N*8), (MI_F_SEEDS_U_BAR, dst, G*m*(N-1)*8), (MI_F_SEEDS_COST, dst, G*8)   the winners'
 *                                            rows, when the last command that selected was a GATHER - else MI_ILQR_E_BAD_ARG.
 *   mi_ilqr_get(MI_F_SEEDS_KERNEL_MS, &ms, 8)   the kernel of the last command, from its own HIP events; before any: MI_ILQR_E_BAD_ARG.
 *                                            Setting one of the five read-only selectors: MI_ILQR_E_BAD_ARG. */

/* ---- Multi-start in the receding-horizon loop (ABI 10; the LONG FORM of MI_F_SEEDS_RUN, no new selector, no new entry point) ----
 * The receding-horizon loop is where a local minimum hurts most: every re-solve starts from the shifted previous plan, and one bad
 * warm start is carried from re-solve to re-solve.  The long form joins the seeds of every group BETWEEN the re-solves of the
 * host-loop form of mi_ilqr_mpc_run, one fused kernel per re-solve (one workgroup per group), nothing of size B m (N-1) crossing the bus:
 *   mi_ilqr_set(MI_F_SEEDS_RUN, v, 64)       v = K | op | seed | round | hold | reserved = 0 | num_resolves | replan_steps, integers
 *                                            held in doubles, checked as the six of the short form are.  op must be RESEED (2),
 *                                            num_resolves >= 1 (below 2^31), 1 <= replan_steps < N - 1, round + num_resolves <= 2^32 -
 *                                            else MI_ILQR_E_BAD_ARG.  The 48-byte form is what it was; every other `bytes`:
 *                                            MI_ILQR_E_BAD_SHAPE.
 * The handle must hold a solve: a cold one (fresh, reset, or left with a pending guess by PERTURB / RESEED) is MI_ILQR_E_BAD_ARG.  A
 * handle whose inputs live in host memory is MI_ILQR_E_UNSUPPORTED, as in the short form.  A refused command changes
 * nothing.  With R = num_resolves and r = replan_steps, for i = 0 .. R - 1:
 *   1. SELECT on the cost and status the handle holds (the rule of the short form) -> row i of the selection log.
 *   2. JOIN.  For a group g with winner w every member k receives
 *        x0[gK+k]           <- x_bar[gK+w][:, r]
 *        u_guess[gK+k][j,t] <- u_bar[gK+w][j, min(t + r, N-2)]  (+ sigma_u[gK+k,j] z(seed, round + i, gK+k, t div hold, j) for k != w)
 *      - mi_ilqr_mpc_shift's shift and RESEED's reseed, applied in that order.  The winner's own slot, every element with sigma = 0
 *      and every padding control get the shifted value bit for bit; sigma z is a rounded product, the sum a rounded sum (no FMA); z is
 *      the normal of PERTURB at round + i.  A group WITHOUT a winner gets what mi_ilqr_mpc_shift followed by RESEED's fallback gives
 *      it: each member's own shifted plan with non-finite entries read as 0, member 0 unperturbed, each member's own x_bar[:, r].  A
 *      pending guess (mi_ilqr_set_initial, mi_ilqr_mpc_shift on a solved handle) is taken as the plan.  The members of a group with a
 *      winner log again: a seed whose re-solve failed is replaced, its `dead` flag of the MPC log is cleared.
 *      CLOSED LOOP (a handle that holds a plant, MI_F_PLANT_STATE): ONE PLANT PER GROUP, member 0's - its state row, plant parameters,
 *      noise sigmas, cost matrices, target and bounds.  Between SELECT and JOIN the group's plant advances r steps under the WINNER's
 *      policy (member 0's where the group has no winner), by the plant kernel of mi_ilqr_mpc_run on G lanes: lane g draws the normals
 *      of problem index g, so a K = 1 run is bitwise the closed loop of mi_ilqr_mpc_run.  The join then gives the plant's state to
 *      every member as x0 - in the place of the prediction, winner or not - and to all K rows of MI_F_PLANT_STATE.  MI_F_PLANT_LOG and
 *      the plants' flags keep their (B, ..) shapes: every member reports its group's plant.  The plant clock, MI_F_PLANT_KERNEL_MS
 *      and the 32-bit clock check behave as in mi_ilqr_mpc_run.  The members of a group whose plant has ended stop logging and are
 *      solved on from the plant's last finite state, as there.  (A reference trajectory and a plant exclude each other, as there.)
 *   3. The targets move as in the host loop of mi_ilqr_mpc_run: MI_F_TARGET_STEP rows once per re-solve, a reference trajectory's
 *      clock by r.  The long form carries no shared target_step; a caller turns one into MI_F_TARGET_STEP rows.
 *   4. mi_ilqr_solve, then row i of the MPC log of every member (x0 | cost | iterations, mi_ilqr_get_mpc_log).  For K > 1 the re-solve
 *      is COLD from the guess, as after RESEED - a member's own gains belong to a plan it no longer follows; for K = 1 every member
 *      continues its own plan and the loop is bitwise mi_ilqr_mpc_shift + mi_ilqr_solve, the host loop of mi_ilqr_mpc_run.
 * After the loop one more SELECT gives row R.  mi_ilqr_get(MI_F_SEEDS_BEST, dst, (R+1)*G*3*8) returns the log (the byte count
 * decides, as MI_F_X_REF takes T from its byte count); MI_F_SEEDS_X_BAR / _U_BAR / _COST answer MI_ILQR_E_BAD_ARG (the run was no
 * GATHER); mi_ilqr_collect_stats gives the last re-solve's statistics; MI_F_SEEDS_KERNEL_MS the join kernels' own events, summed over
 * the run.  A run that fails part-way leaves the reference's clock where it was.  mi_ilqr_mpc_run itself, in both forms, is untouched.
 * Splitting a run is exact: one call of R re-solves is bitwise R calls of one with `round` advanced by hand (each call starts a new
 * MPC log). */

/* ---- Sampling-based MPC (ABI 10; the SAMPLING FORM of MI_F_SEEDS_RUN, 10 doubles, no new selector, no new entry point) ----
 * MPPI / predictive sampling, the derivative-free counterpart of a solve: every problem b improves its own nominal plan u (m, N-1)
 * from its own x0 under its own Q, R, Qf, target, model parameters and box, by `iterations` rounds of { perturb the plan S times; roll
 * the S plans out; weight them by exp(-cost / temperature); average them }.  The loop never leaves the device.
 *   mi_ilqr_set(MI_F_SEEDS_RUN, v, 80)       v = S | op | seed | first_sample | hold | reserved = 0 | iterations | shift | temperature |
 *                                            reserved = 0, integers held in doubles.  op must be RESEED (2), as in the long form; sigma_u
 *                                            comes from MI_F_SEEDS_SIGMA (not set: zeros).  S is an integer in [1, 2^31 - 64] (whole waves of
 *                                            64 samples are counted in 32 bits), iterations and hold are integers in [1, 2^31), seed in [0, 2^53), first_sample in [0, 2^32) with first_sample + iterations S
 *                                            <= 2^32 (the sample counter is 32 bits), shift in [0, N - 2], temperature >= 0 and no NaN
 *                                            - else MI_ILQR_E_BAD_ARG.  A handle that holds a reference trajectory (MI_F_X_REF):
 *                                            MI_ILQR_E_UNSUPPORTED, as mi_ilqr_policy_rollout refuses it; a handle whose inputs live in
 *                                            host memory: MI_ILQR_E_UNSUPPORTED, as in the short form.  The 48-byte and the 64-byte
 *                                            form are what they were; 88 bytes and more stay MI_ILQR_E_BAD_SHAPE.  A refused command
 *                                            changes nothing.
 * THE NOMINAL starts as what the next solve would start from: the pending guess, else u_bar, else zeros.  With I = iterations, for
 * i = 0 .. I - 1:
 *   ROLLOUT.  Sample s = 0 .. S - 1 of problem b applies v_s[k,t] = clip(u[k,t] + sigma_u[b,k] z, box_b): the clip on a control-limited
 *   handle only and by comparisons; sigma z is a rounded product, the sum a rounded sum (no FMA).  z is a standard normal of
 *   (seed, g, t div hold, b, k) alone, g = first_sample + i S + s the GLOBAL SAMPLE NUMBER: Philox4x32-10 under the key
 *   (seed mod 2^32, seed div 2^32) at counter = (g, t div hold, b, 1024 + k / 4), Box-Muller normal k mod 4 of the block, as under
 *   "Multi-start" (blocks 1024.. are the samples'; 0.. / 256.. / 512.. / 768.. stay the states', the controls', the Monte-Carlo draws'
 *   and the seed perturbations').  z does not depend on S, on B, on the launch or on the layout.  SAMPLE 0 IS THE ELITE SLOT: it draws
 *   nothing and applies clip(u); so do a zero sigma and the padding controls, bit for bit.  Each sample is rolled out open loop - no
 *   feedback gains - and costs what mi_ilqr_policy_rollout's stage and terminal expressions give on the APPLIED control v.  A sample
 *   that meets an infeasible step (models that can fail), a non-finite state or a non-finite cost has cost +inf.
 *   UPDATE.  L_min is the least finite cost, ties to the lowest s; a_s = -(L_s - L_min) / temperature, w_s = exp(a_s) / sum exp(a_s)
 *   over the finite samples only; temperature = 0 is the indicator of the argmin (predictive sampling).  u_new[k,t] = sum_s w_s v_s[k,t]:
 *   the first finite sample's rounded product starts the sum, each later term is a rounded product added by a rounded sum; samples
 *   without a finite cost are skipped, not multiplied by zero.  Both sums - sum exp(a_s) and the blend - run SEQUENTIALLY IN s = 0, 1, ..
 *   S - 1, an order that is a function of S alone.  The result is clipped again on a limited handle.  A problem without a finite
 *   sample keeps u.
 *   LOG.  Row i: argmin sample | its cost | finite samples (no finite sample: -1 | +inf | 0), and nominal cost (sample 0's) | ESS =
 *   1 / sum w_s^2 (NaN without a finite sample).
 * A closing rollout of the final nominal alone (S = 1) gives row I of the nominal cost (its ESS: NaN).  The final nominal, shifted by
 * `shift` steps as mi_ilqr_mpc_shift shifts - u_guess[t] = u[min(t + shift, N-2)] - becomes the handle's pending guess and the handle
 * is cold, as after mi_ilqr_reset followed by mi_ilqr_set_initial(u_guess): mi_ilqr_solve polishes the plan, and a new x0 followed by
 * the command again is the receding-horizon loop.
 *   mi_ilqr_get(MI_F_SEEDS_BEST, dst, I*B*3*8)        argmin sample | its cost | finite samples, per iteration and problem
 *   mi_ilqr_get(MI_F_SEEDS_COST, dst, (I+1)*B*2*8)    nominal cost | ESS (NaN in the closing row)
 *   mi_ilqr_get(MI_F_SEEDS_U_BAR, dst, B*m*(N-1)*8)   the final nominal, unshifted, time last, m the device's control dimension
 *   mi_ilqr_get(MI_F_SEEDS_X_BAR, ..)                 MI_ILQR_E_BAD_ARG (cleared: the run keeps no states)
 *   mi_ilqr_get(MI_F_SEEDS_KERNEL_MS, &ms, 8)         the run's kernels, first to last, from one pair of HIP events
 * Consequences: one call of I iterations is bitwise I calls of one iteration with first_sample advanced by S each; under temperature =
 * 0 the nominal cost of row i + 1 is the best cost of row i bitwise, so the cost never rises; nothing of size S leaves the device and
 * nothing of size S (N-1) is ever stored - the update regenerates every sample's applied controls from the counters. */

/* ---- Parameter identification (ABI 10; selectors MI_F_FIT_* of mi_ilqr_set / mi_ilqr_get, no new entry point) ----
 * From logged transitions (x_j, u_j, x_next_j) to the parameter rows MI_F_MODEL_PARAMS takes: every problem b fits the FREE entries
 * of its own parameter row theta to its own rows by Levenberg-Marquardt on the one-step prediction error, on the device.  A model
 * without parameters answers MI_ILQR_E_UNSUPPORTED to every selector below.  A refused call changes nothing.
 *   mi_ilqr_set(MI_F_FIT_DATA, rows, B*T*(2n+m)*8)    row j of problem b = x_j | u_j | x_next_j, m the device's control dimension
 *                                            (padding controls: zeros).  T >= 1 from the byte count, T < 2^24.  Rows need not be
 *                                            consecutive in time.  Every entry finite (rows past a problem's count too: zeros will do)
 *                                            - else MI_ILQR_E_BAD_ARG.  Setting the data drops MI_F_FIT_WEIGHTS (its counts refer to T).
 *   mi_ilqr_set(MI_F_FIT_WEIGHTS, rows, B*(n+1)*8)    row b = w (n) | count: w finite and >= 0, the diagonal W of the residual norm;
 *                                            count an integer in [0, T]: problem b uses its first count rows.  Not set (NULL, 0 bytes):
 *                                            ones | T.  Needs the data: before it, MI_ILQR_E_BAD_ARG.
 *   mi_ilqr_set(MI_F_FIT_START, rows, B*(n_params+1)*8)   row b = theta0 | mu0: finite, mu0 > 0.  Not set (NULL, 0 bytes): the rows
 *                                            MI_F_MODEL_PARAMS returns | 1e-3.
 *   mi_ilqr_set(MI_F_FIT_BOUNDS, rows, 2*n_params*8)  lower | upper, no NaN, lower <= upper.  Not set (NULL, 0 bytes): -inf | +inf.
 *   mi_ilqr_set(MI_F_FIT_RUN, v, (6+P)*8)    v = iterations | ftol | fd_rel | fd_floor | apply | P | free[0] .. free[P-1], integers held
 *                                            in doubles: iterations in [0, 2^20], ftol >= 0, fd_rel > 0, fd_floor > 0, apply 0 or 1,
 *                                            P in [1, MI_FIT_MAX_FREE], free strictly increasing indices below n_params - else
 *                                            MI_ILQR_E_BAD_ARG; a byte count that is not (6+P)*8 for the P it holds: MI_ILQR_E_BAD_SHAPE.
 *                                            No data: MI_ILQR_E_BAD_ARG.
 * THE ALGORITHM, independently per problem.  With theta the problem's row and f the model's step:
 *   r_j = x_next_j - f(x_j, u_j; theta);  J_j[:, i] = (f(.; theta + h_k e_k) - f(.; theta - h_k e_k)) / (2 h_k), k = free[i],
 *   h_k = fd_rel max(|theta_k|, fd_floor) at the point being evaluated;
 *   c = sum_j r_j' W r_j, g = sum_j J_j' W r_j, H = sum_j J_j' W J_j over the first count rows: the NORMAL EQUATIONS at theta.
 *   A TRIAL: (H + mu D) delta = g by Cholesky, D_ii = H_ii where H_ii > 0, else 1; theta' = clip(theta + delta) on the free entries,
 *   by comparisons.  A factorisation that meets a pivot that is not positive or not finite is a rejected trial.  ACCEPTED when
 *   c(theta') is finite and c(theta') < c(theta): theta <- theta', the normal equations become those of theta', mu <- max(mu / 10,
 *   1e-12).  Else mu <- min(10 mu, 1e12) and the next trial is solved from the kept H, g.  `iterations` counts trials.
 *   enum { MI_FIT_CONVERGED = 0,   an accepted trial with c - c' <= ftol c, or c' == 0
 *          MI_FIT_MAX_ITERS = 1,   `iterations` trials without either end
 *          MI_FIT_STALLED = 2,     a rejected trial with mu already at 1e12
 *          MI_FIT_BAD_DATA = 3 }   count == 0 (cost +inf), or c(theta0) not finite (cost as computed): theta is theta0, untouched
 *   A finished problem is frozen while the rest of the batch goes on.  A prediction that is not finite makes that evaluation's cost
 *   non-finite; the models' feasibility bounds are not consulted (one-step prediction, not a rollout).
 * ON THE DEVICE.  fit_normal_kernel<M> (one per model, plugins included): one lane per (transition, slot), slot 0 the evaluation at
 * theta, slot i the pair theta +- h e_free[i-1]; G = P + 1 rounded up to a power of two slots per transition, 64 / G transitions per
 * wave, grid B x ceil(T / (64 / G)); every wave leaves one row c | g | upper(H), summed over its transitions by a butterfly of fixed
 * order.  fit_update_kernel (no model), one wave per problem: folds the rows left to right in wave order - an order that is a
 * function of T and P alone -, decides, moves mu and solves the next trial.  A run of I iterations is normal(theta0), I x {update,
 * normal(trial)} and the closing update: I + 1 launches of each on the handle's stream, ordered behind every solve in flight, no
 * host synchronisation between them.  Nothing of a problem's result depends on B, on the other problems or on the handle's layout.
 * apply = 1 makes the fitted rows the handle's per-problem parameter rows, exactly what mi_ilqr_set(MI_F_MODEL_PARAMS, theta) would
 * leave; apply = 0 reads and writes nothing a solve uses.
 *   mi_ilqr_get(MI_F_FIT_RESULT, dst, B*(n_params+7)*8)   row b = theta | cost0 | cost | mu | iterations | accepted | status | count:
 *                                            cost0 = c(theta0), cost = c(theta); mu: the damping to carry into a following run
 *   mi_ilqr_get(MI_F_FIT_NORMAL, dst, B*(P+P*P)*8)        row b = g | H at the returned theta (BAD_DATA by count == 0: zeros)
 *   mi_ilqr_get(MI_F_FIT_KERNEL_MS, &ms, 8)               the run's kernels, first to last, from one pair of HIP events
 *   Before any run the three answer MI_ILQR_E_BAD_ARG; mi_ilqr_set on them and mi_ilqr_get(MI_F_FIT_RUN) too.
 * With these a caller forms inv(H) cost / (count n - P) as the covariance of the fitted entries. */

#ifdef __cplusplus
}
#endif
#endif /* MI_ILQR_H */
