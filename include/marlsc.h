/*
 * marlsc.h -- C ABI of the MI355X-native vectorised supply-chain environment (libmarlsc.so).
 *
 * Drop-in boundary for the reference's env hot path. One `msc_env` handle owns E independent
 * copies of the reference's `InventoryEnvironment` (src/environment/envs/multi_env.py:38)
 * resident in HBM and steps them in lockstep on one GPU. Entry points and the reference
 * interface each one replaces:
 *
 *   msc_env_create   <- InventoryEnvironment.__init__(env_config, seed, env_meta)   multi_env.py:58-190
 *                       + per-env seeds of the RLlib env factory
 *                         SeedManager.derive_env_seed(base, worker_index, env_index)  seed_manager.py:165-186
 *                         (called from src/algorithms/base.py:413-419)
 *   msc_env_reset    <- InventoryEnvironment.reset(seed=None, options=None)          multi_env.py:192-251
 *                       (SeedManager.advance_episode / update_root_seed, seed_manager.py:100-136)
 *   msc_env_step     <- InventoryEnvironment.step(actions)                            multi_env.py:253-366
 *                       (the five components: demand_sampler.py:105-163 / :214-261,
 *                        demand_allocator.py:118-217, lead_time_sampler.py:97-108 / :169-197,
 *                        lost_sales_handler.py:71-210, reward_calculator.py:96-190)
 *                       plus RLlib's reset-after-truncation of the EnvRunner loop.
 *   msc_env_obs_flat <- the flat per-agent observation  local_i || concat_j local_j   multi_env.py:548-575
 *   msc_gae          <- RLlib 2.52.1 GAE + advantage standardisation (external to the reference;
 *                       enabled at src/algorithms/mappo.py:154-156)
 *
 * Conventions
 *   - Return value 0 = OK, negative = error; msc_last_error() gives a thread-local message.
 *   - All array arguments of msc_env_step / msc_env_reset / msc_gae are DEVICE pointers
 *     (e.g. torch data_ptr()) unless the parameter name ends in `_host`.
 *   - Every call is stream-ordered on the given hipStream_t (pass 0 for the null stream); no call
 *     synchronises the device except msc_env_create / msc_env_destroy / msc_env_read_state /
 *     msc_env_save_state / msc_env_load_state / msc_env_check / msc_env_set_timing /
 *     msc_env_read_timing.
 *   - The library owns the env state buffers; callers own every I/O buffer.
 *   - One handle per stream / host thread; a handle is not thread-safe (like the reference object).
 *   - Layouts are row-major: actions [E][W][K] f32, obs [E][W][L] f32, rewards [E][W].
 */
#ifndef MARLSC_H
#define MARLSC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msc_env msc_env;
typedef struct ihipStream_t* msc_stream_t; /* == hipStream_t */

#define MSC_ABI_VERSION 2
#define MSC_MAX_W 32   /* warehouses (agents) per env (step kernels loop warehouses over <= 16 waves above 16) */
#define MSC_MAX_K 16   /* SKUs (above 8: the sequential demand sampler and the group allocator) */
#define MSC_MAX_R 4096 /* demand regions */
#define MSC_HISTORY 5  /* rolling window, multi_env.py:147 */
#define MSC_ORDER_CAP_MAX (1 << 24) /* Poisson order records per env and step: sum(lambda_orders) + 12 sqrt(.) + 64 */

/* Component `type` strings of the reference's registries (src/environment/registry.py:300-308). */
enum msc_demand_type   { MSC_DEMAND_POISSON = 0, MSC_DEMAND_EMPIRICAL = 1 };
enum msc_action_type   { MSC_ACTION_DIRECT = 0, MSC_ACTION_DEMAND_CENTERED = 1, MSC_ACTION_BASE_STOCK = 2 };
enum msc_init_type     { MSC_INIT_UNIFORM = 0, MSC_INIT_CUSTOM = 1, MSC_INIT_ZERO = 2 };
enum msc_lead_type     { MSC_LEAD_FIXED = 0, MSC_LEAD_STOCHASTIC = 1 };
enum msc_lost_type     { MSC_LOST_CLOSEST = 0, MSC_LOST_SHIPMENT = 1, MSC_LOST_COST = 2 };
enum msc_scope         { MSC_SCOPE_AGENT = 0, MSC_SCOPE_TEAM = 1 };
enum msc_obs_norm      { MSC_OBS_OFF = 0, MSC_OBS_RATIO = 1, MSC_OBS_MEANSTD = 2 };

/* Feature toggles (FeatureConfig, src/config/schema.py:595-639); order = block order of
 * _build_local_obs (multi_env.py:620-695). */
enum msc_feature_bits {
  MSC_F_INVENTORY = 1u << 0,            MSC_F_INVENTORY_AGG = 1u << 1,
  MSC_F_PIPELINE = 1u << 2,             MSC_F_PIPELINE_AGG = 1u << 3,
  MSC_F_INCOMING_HOME = 1u << 4,        MSC_F_INCOMING_HOME_AGG = 1u << 5,
  MSC_F_SHIPPED_HOME = 1u << 6,
  MSC_F_SHIPPED_AWAY = 1u << 7,         MSC_F_SHIPPED_AWAY_AGG = 1u << 8,
  MSC_F_STOCKOUT = 1u << 9,
  MSC_F_ROLLING_MEAN = 1u << 10,        MSC_F_ROLLING_MEAN_AGG = 1u << 11,
  MSC_F_FORECAST = 1u << 12,            MSC_F_FORECAST_AGG = 1u << 13,
  MSC_F_DAYS_OF_SUPPLY = 1u << 14,
  MSC_F_NET_POSITION = 1u << 15,
  MSC_F_DEMAND_VARIABILITY = 1u << 16,
  MSC_F_DEMAND_HISTORY = 1u << 17
};

/* Environment descriptor: the reference's EnvironmentConfig + env_meta flattened to plain
 * host arrays (all HOST pointers; copied by msc_env_create). Shapes use W = n_warehouses,
 * K = n_skus, R = n_regions. */
typedef struct msc_env_desc {
  int32_t abi_version;                 /* = MSC_ABI_VERSION */
  int32_t n_warehouses, n_skus, n_regions, episode_length;

  int32_t action_type;                 /* msc_action_type */
  const double* action_param;          /* [K]: max_order_quantities | max_quantity_adjustment | max_stock_level */

  int32_t init_type;                   /* msc_init_type */
  int32_t init_min, init_max;          /* uniform: integers(min, max+1, (W,K)) (multi_env.py:522-525) */
  const int32_t* init_values;          /* custom: [W*K] */

  int32_t holding_per_sku;             /* 1: holding_cost is [K]; 0: scalar x sku_weights */
  const double* holding_cost;
  int32_t penalty_per_sku;
  const double* penalty_cost;
  const double* sku_weights;           /* [K] */
  const double* distances;             /* [W*R] */
  const double* outbound_fixed;        /* [W*R] */
  const double* outbound_variable;     /* [W*R] */
  const double* inbound_fixed;         /* [W*K] */
  const double* inbound_variable;      /* [W*K] */

  int32_t demand_type;                 /* msc_demand_type */
  const double* lambda_orders;         /* poisson: [R] (scalar mode: broadcast by the caller) */
  const double* probability_skus;      /* [R] */
  const double* lambda_quantity;       /* [R*K] */
  /* empirical trace, CSR over the sorted available timesteps (demand_sampler.py:199-261):
   * orders of trace row i are [trace_offsets[i], trace_offsets[i+1]), each with a region and
   * K quantities, already grouped/sorted by (region_id, order_id). */
  int32_t trace_n_rows;
  const int64_t* trace_offsets;        /* [trace_n_rows + 1] */
  const int32_t* trace_regions;        /* [n_trace_orders] */
  const int32_t* trace_quantities;     /* [n_trace_orders * K] */

  int32_t max_splits;                  /* greedy allocator ("default" -> W-1) */

  int32_t lead_type;                   /* msc_lead_type */
  const int32_t* expected_lead_times;  /* [W*K] */
  int32_t max_dev_per_sku;             /* 1: max_deviation is [K] (SKU-major draws); 0: scalar */
  const int32_t* max_deviation;

  int32_t lost_type;                   /* msc_lost_type */
  double lost_alpha;                   /* softmax temperature for MSC_LOST_COST */

  int32_t reward_scope;                /* msc_scope */
  double reward_scale;

  uint32_t feature_flags;              /* msc_feature_bits */
  int32_t include_warehouse_id;        /* one-hot prefix (parameter sharing) */
  int32_t obs_norm;                    /* msc_obs_norm */
  const float* obs_mean;               /* [n_features] for MSC_OBS_MEANSTD */
  const float* obs_std;
  int32_t num_eval_episodes;           /* <= 0: no eval cycling (multi_env.py:164-168, 220-224) */
  /* Episode-ahead Poisson demand (no reference counterpart: a scheduling choice, results are
   * identical either way): -1 automatic (on for <= 8,192 envs), 0 off (short-lived envs, e.g. the
   * evaluation envs), n > 0 at most n slots (future episodes per env). Its buffers take at most
   * ea_mem_fraction (<= 0: 0.25) of the device memory free at create time; fewer slots, or none,
   * when the budget binds (msc_env_dims reports the slots chosen). */
  int32_t episode_ahead;
  double ea_mem_fraction;
} msc_env_desc;

/* Optional per-step diagnostics = the reference's collect_step_info dict (multi_env.py:330-361).
 * DEVICE pointers, any may be NULL. */
typedef struct msc_step_info {
  int32_t* inventory_before;           /* [E][W][K] */
  int32_t* pending_total;              /* [E][W][K] */
  int32_t* order_quantities;           /* [E][W][K] */
  int32_t* demand_per_region;          /* [E][R][K] */
  int32_t* fulfilled_per_warehouse;    /* [E][W][K] */
  int32_t* unfulfilled_demands;        /* [E][R][K] */
  int32_t* shipment_counts;            /* [E][W][R] */
  int32_t* shipment_quantities;        /* [E][W][R] */
  int32_t* shipment_quantities_by_sku; /* [E][W][R][K] */
  int32_t* lost_order_counts;          /* [E][R] */
  int32_t* n_orders;                   /* [E] */
  double* lost_sales;                  /* [E][W][K] */
  double* costs;                       /* [E][4][W]: holding, penalty, outbound, inbound */
} msc_step_info;

/* Create E = n_envs environments on `device`. Env i gets root seed
 *   env_seeds_host[i]                                    if env_seeds_host != NULL, else
 *   SeedSequence([base_seed, worker_index, env_index_offset + i]).generate_state(1)[0].
 * Nothing is reset yet: call msc_env_reset before the first step. */
int msc_env_create(const msc_env_desc* desc, int device, int64_t n_envs, uint32_t base_seed,
                   uint32_t worker_index, int64_t env_index_offset, const uint32_t* env_seeds_host,
                   msc_env** out);
void msc_env_destroy(msc_env* env);

/* Sizes of the I/O tensors, and the episode-ahead slots per env chosen at create time (0: off). */
int msc_env_dims(const msc_env* env, int64_t* n_envs, int32_t* n_agents, int32_t* n_skus,
                 int32_t* n_regions, int32_t* local_obs_dim, int32_t* n_features,
                 int32_t* max_expected_lead_time, int32_t* ea_slots);

/* Diagnostic (no reference counterpart: the reference has one code path): the kernels this handle
 * runs, chosen at create time from its shape and the MSC_* knobs. Writes up to n of
 * {alloc (0 lane, 1 group, 2 scan), envs sorted by order count, phase A fused, phase C fused,
 *  group kernel cost tables in LDS, lane-group width, episode-ahead slots, demand (0 unit parser,
 *  9 demand_v3 where it applies), equal sampler parameters (UNI)}; returns the count written. */
int msc_env_kernel_choice(const msc_env* env, int32_t* out, int32_t n);

/* The same choice without a handle and without touching a GPU: what msc_env_create would pick for
 * this descriptor and env count under the current MSC_* knobs, on a device with n_cus compute units
 * (< 1: 256) and free_bytes of free memory (< 0: the episode-ahead memory fit is not applied).
 * Validates like msc_env_create (same codes and texts). Writes up to n of: the nine values of
 * msc_env_kernel_choice in its order, then
 *  {obs_stage (as the handle starts: its episode-ahead value where that is on), obs_ring_reg, alloc_lpe,
 *   sort_shift, scan_defer, sc_tab, sc_form, al_psplit, demand_ptrs, order_cap, RING, ea_cap,
 *   ea_batch, ea_chunk, pipeline, arena bytes / 256, bytes of one order buffer / 256}
 * (both buffers are 256-byte granular; msc_env_state_bytes = header + arena + one order buffer).
 * Returns the count written (26 at most), or < 0. */
int msc_env_plan(const msc_env_desc* desc, int64_t n_envs, int32_t n_cus, int64_t free_bytes, int32_t* out,
                 int32_t n);

/* Kernel-form options of a handle that change no result (diagnostic / tuning; no reference
 * counterpart). MSC_OPT_STEP_C_FORM: the waves per SIMD the observation kernel is compiled for, 5
 * (default: beside the pipelined demand kernel) or 4 (no register spills; the rollout collector's
 * choice, with policy kernels between steps). MSC_OPT_ALLOC_PRIO_SPLIT: the share, in 16ths of its
 * busiest env's orders, that each one-env-per-lane allocation wave runs above the pipelined demand
 * kernel's parser (s_setprio 3) before it drops below it (1 .. 16; default 14; 16: the whole kernel,
 * the rollout collector's choice). Returns 0, or < 0 for an unknown key / value. */
#define MSC_OPT_STEP_C_FORM 1
#define MSC_OPT_ALLOC_PRIO_SPLIT 2
int msc_env_set_option(msc_env* env, int32_t key, int32_t value);
/* MSC_OPT_ALLOC_TAIL (msc_env_set_option): 1 (default) lets a one-env-per-lane allocation wave whose
 * envs have all sold out (or run out of orders) finish its remaining orders in a short loop that
 * only counts them as lost; 0 keeps every order on the general path. Results are bit-identical. */
#define MSC_OPT_ALLOC_TAIL 3
/* The order index at which each block (64 consecutive envs) of the one-env-per-lane allocation
 * kernel entered that loop in the last step, -1 where it did not (the option off, another allocator,
 * or some env kept stock up to the last order of the block's busiest env). Synchronizes the device;
 * copies min(n, ceil(n_envs / 64)) values to the host array `out`. Returns 0, or < 0 on error. */
int msc_env_alloc_tail_entry(const msc_env* env, int32_t* out, int64_t n);

#define MSC_RESET_EVAL_RESTART 1  /* reset(seed=...) of a construction-seeded eval env: counter -> 0 */

/* Reset envs with mask[i] != 0 (mask == NULL: all). new_root_seeds == NULL follows the
 * construction-seeded path (advance_episode, with eval cycling); otherwise
 * update_root_seed(new_root_seeds[i]) (reset(seed=X) of an env created without a seed).
 * Writes the reset observation of every reset env into obs [E][W][L] (may be NULL). */
int msc_env_reset(msc_env* env, const uint8_t* mask, const uint32_t* new_root_seeds, int32_t flags,
                  float* obs, msc_stream_t stream);

/* One step of every env. actions [E][W][K] in [-1, 1]: they must be finite; values outside
 * [-1, 1] are rescaled like the reference's (direct clamps to [0, max_order_quantities], the other
 * two action types only at 0). The pending total of a warehouse, over all its SKUs and arrival
 * slots, must stay below 2^24: the totals are integer sums here and float32 sums in the reference
 * (order by order per SKU, numpy's pairwise sum for the observation's total), which agree while
 * every partial sum is exact in float32, that is up to 2^24 - 1.
 * Outputs obs [E][W][L] (local obs of
 * every agent), rewards [E][W] (f32, and optionally f64), truncated [E]. An env whose episode
 * ends is reset in the same call (RLlib's EnvRunner semantics): its terminal observation goes
 * to final_obs (if non-NULL) and obs receives the first observation of the next episode. */
int msc_env_step(msc_env* env, const float* actions, float* obs, float* rewards,
                 double* rewards_f64, uint8_t* truncated, float* final_obs,
                 const msc_step_info* info, msc_stream_t stream);

/* Optional split of msc_env_step: run the demand sampler of the NEXT step now (it depends only
 * on each env's own RNG stream, not on actions), e.g. on a side stream while the policy forward
 * runs. The following msc_env_step consumes these orders instead of generating them.
 * No-op for the empirical sampler. */
int msc_env_generate_demand(msc_env* env, msc_stream_t stream);

/* Automatic demand pipelining (default on for the Poisson sampler): msc_env_step also launches the
 * NEXT step's demand generation on a library-owned side stream, concurrent with the current step
 * kernel (skipped across episode boundaries and after masked resets). Results are identical either
 * way; 0 disables it (every step then runs demand + step back to back on the caller's stream). */
int msc_env_set_pipelining(msc_env* env, int32_t enabled);

/* Episode-ahead demand on / off at run time (no reference counterpart; results are identical either
 * way): 0 switches a handle whose EA buffers exist to per-step pipelined demand from the current step
 * on (e.g. a rollout whose policy kernels lose more to the background generation than the step
 * gains), != 0 lets it restart at the next common episode start. No-op without EA buffers.
 * Synchronises the device. */
int msc_env_set_episode_ahead(msc_env* env, int32_t enabled);

/* Wave priority of the step chain (no reference counterpart: a scheduling hint). With enabled != 0
 * the phase-A and phase-C kernels of msc_env_step run at s_setprio 3, like the allocation kernel,
 * ahead of the pipelined demand kernel of the next step. For callers that run their own work between
 * steps (a rollout's policy forward): the env step is then their critical path and the next step's
 * demand has slack. Default 0 (env-only stepping: the demand kernel is the critical path).
 * Synchronises the device. Results are identical either way. */
int msc_env_set_chain_priority(msc_env* env, int32_t enabled);

/* Per-launch device durations of the production path (for roofline accounting): with max_steps > 0
 * the next max_steps calls of msc_env_step bracket their demand launch and their step launch (the
 * step kernels of that call) with HIP events on the stream each runs on -- the caller's stream, or
 * the side stream for pipelined demand. 0 disables and frees the events. No reference
 * counterpart (instrumentation only). */
int msc_env_set_timing(msc_env* env, int32_t max_steps);
/* Mean device duration in ms of the recorded demand / step launches and their counts (waits for
 * the recorded events). */
int msc_env_read_timing(msc_env* env, double* demand_ms, double* step_ms, int64_t* n_demand,
                        int64_t* n_step);
/* Episode-ahead demand (few envs per GPU: E <= 8192 by default, MSC_EA=0|1 forces it): while
 * every env sits at the same timestep, the Poisson orders of whole future episodes are drawn on a
 * library-owned stream (an episode's demand depends only on its SeedSequence([root, counter]) seed,
 * src/utils/seed_manager.py:100-120, never on actions); each env step then reads its episode's
 * slot. Results are identical with and without it. Mean device duration of the episode generation
 * launches timed since msc_env_set_timing (one launch = one episode of every env in steady state),
 * their count, the slots per env (0: EA off), whether the current episode reads a slot, and the mean
 * env-steps of demand one timed launch generated (slots x steps x envs; for roofline accounting). */
int msc_env_read_timing_ea(msc_env* env, double* ea_ms, int64_t* n_ea, int32_t* slots, int32_t* active,
                           double* env_steps_per_launch);

/* Demand work issued by the handle since create (monotonic; differences bracket a timed window):
 * episode-ahead generation launches (chunks) and the env-steps of demand they drew, per-step demand
 * launches (E env-steps each), and msc_env_step calls. Everything issued before a device-wide
 * synchronize has finished after it. */
int msc_env_work_counters(const msc_env* env, int64_t* ea_launches, double* ea_env_steps, int64_t* demand_launches,
                          int64_t* steps);

/* Episode-ahead memory of the handle: the budget computed at create time (bytes; 0 when EA was not
 * requested) and the bytes allocated for the slots (0: EA off). */
int msc_env_ea_memory(const msc_env* env, int64_t* budget_bytes, int64_t* allocated_bytes);

/* Flat per-agent observation of the reference [E][W][L*(1+W)] = local_w || local_0..local_{W-1},
 * from the compact obs [E][W][L]. */
int msc_env_obs_flat(const msc_env* env, const float* obs, float* flat, msc_stream_t stream);

/* Host copies of the parity-relevant state (synchronous). Any pointer may be NULL.
 *   inventory [E][W][K] i32, timestep [E], episode_counter [E],
 *   rng [E][2][6] u64: {demand, lead_time} x {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger} */
int msc_env_read_state(const msc_env* env, int32_t* inventory_host, int32_t* timestep_host,
                       int32_t* episode_counter_host, uint64_t* rng_host);

/* Opaque checkpoint of the whole device state (synchronous): size query, save, restore. */
int64_t msc_env_state_bytes(const msc_env* env);
int msc_env_save_state(const msc_env* env, void* buf_host);
int msc_env_load_state(msc_env* env, const void* buf_host);

/* Set SeedManager._episode_counter of every env (counters_host [E], host, >= 0; synchronous).
 * Replaces the caller-side write `seed_manager._episode_counter = 0` (src/algorithms/base.py:81):
 * the next construction-seeded reset of env i derives its episode root from
 * SeedSequence([root_i, counters_host[i]]) (seed_manager.py:100-120), so E eval envs created with
 * the same root and counters 0..E-1 replay the reference eval env's episodes 0..E-1, which it runs
 * one after another with eval cycling (multi_env.py:220-224). */
int msc_env_set_episode_counters(msc_env* env, const int32_t* counters_host);

/* Synchronise and report device-side errors (order-buffer overflow, ...). */
int msc_env_check(msc_env* env);

/* Advantage estimation over T steps x N sequences (layout [T][N], time-major):
 *   delta_t = r_t + gamma * V_{t+1} * (1 - term_t) - V_t
 *   A_t     = delta_t + gamma * lam * (1 - term_t) * (1 - trunc_t) * A_{t+1}
 * where V_{t+1} = next_values[t] if trunc_t (bootstrap from the terminal obs) else values[t+1];
 * values[T] (row T of `values`, [T+1][N]) bootstraps the last row. targets = A + V.
 * All of it is float32, one rounding per operation and no fused multiply-add: gamma * lam is formed
 * once in float32, delta_t = (r_t + gamma * V_{t+1}) - V_t, A_t = delta_t + (gamma * lam) * A_{t+1};
 * a terminated step bootstraps 0 even when it is also truncated; next_values == NULL bootstraps 0 on
 * truncated steps; terminated / truncated == NULL mean no flag set.
 * stats_out (device f64[3]) receives {sum A, sum A^2, count} (accumulated, caller zeroes it)
 * for the cross-rank advantage standardisation. */
int msc_gae(const float* rewards, const float* values, const float* next_values,
            const uint8_t* terminated, const uint8_t* truncated, int64_t n_seq, int32_t T,
            float gamma, float lam, float* advantages, float* targets, double* stats_out,
            msc_stream_t stream);

/* In-place (A - mean) / max(1e-4, std) using stats {sum, sumsq, count} (device f64[3]). */
int msc_adv_normalize(float* advantages, int64_t n, const double* stats, msc_stream_t stream);

/* Per-module variants (RLlib's GAE connector standardises the advantages of every module of a
 * multi-agent batch on its own; with one policy per agent that is one group per agent):
 * sequence n belongs to group n % n_groups (the rollout's sequences are env * W + agent, so
 * n_groups = W gives one group per agent); n_groups in [1, 64] must divide n_seq.
 * stats_out is device f64 [n_groups][3] {sum A, sum A^2, count} (accumulated, caller zeroes it);
 * msc_adv_normalize_grouped standardises element i of the [T][n_seq] advantages with the
 * statistics of group i % n_groups. n_groups = 1 is msc_gae / msc_adv_normalize. */
int msc_gae_grouped(const float* rewards, const float* values, const float* next_values,
                    const uint8_t* terminated, const uint8_t* truncated, int64_t n_seq, int32_t T,
                    float gamma, float lam, float* advantages, float* targets, int32_t n_groups,
                    double* stats_out, msc_stream_t stream);
int msc_adv_normalize_grouped(float* advantages, int64_t n, int32_t n_groups, const double* stats,
                              msc_stream_t stream);

/* The PPO minibatch loss, its statistics and its gradients with respect to the network outputs in one
 * launch: RLlib 2.52.1 PPOTorchLearner.compute_loss_for_module with the reference's hysteretic
 * advantage weighting (src/algorithms/learners/hysteretic_learner.py:35-42: negative advantages
 * scaled by hysteretic_beta). Output row i of n_rows uses batch row b = idx[i] (idx device int64
 * [n_rows]; NULL: b = i), so the caller passes the whole batch's columns and the kernel gathers the
 * minibatch. Repeated indices are legal. Every idx[i] must lie in [0, B), B the rows of the batch
 * columns: that is the caller's contract, as with array indexing, and is not checked.
 *   mean [n_rows][k], values [n_rows]; log_std [n_rows][k] (log_std_rows = 0: a mu/sigma head) or one
 *   shared row [k] (log_std_rows = 1: the free parameter, already clamped at its floor by the caller);
 *   actions [B][k], logp_old / advantages / value_targets [B], and with use_kl mean_old / log_std_old
 *   [B][k] (NULL without). All float32 device buffers. Per row, with a the action:
 *     logp = sum_k -(a - mean)^2 / (2 exp(log_std)^2) - log_std - log(2 pi) / 2
 *     r    = exp(logp - logp_old),  A' = A if A >= 0 else hysteretic_beta A  (hysteretic_beta 1: off)
 *     surr = min(A' r, A' clamp(r, 1 - clip_param, 1 + clip_param))
 *     vfc  = clamp((values - value_targets)^2, 0, vf_clip_param),  ent = sum_k log_std + log(2 pi e) / 2
 *     kl   = sum_k log_std - log_std_old + (exp(2 log_std_old) + (mean_old - mean)^2) / (2 exp(2 log_std)) - 1/2
 *   total = mean_i(-surr + vf_loss_coeff vfc - entropy_coeff ent) + kl_coeff mean_i(kl)   (kl: use_kl only)
 * Outputs: total (device f32[1]); stats (device f64[5]) = {total_loss, policy_loss = mean(-surr),
 * vf_loss = mean(vfc), entropy = mean(ent), mean_kl = mean(kl)}, stored, or with accumulate_stats
 * added to what the buffer holds (a learner sums over steps on the device and reads once);
 * grad_mean [n_rows][k], grad_values [n_rows] and grad_log_std ([n_rows][k], or the row-summed [k] for
 * the shared row) = d total / d (mean, values, log_std as given: a clamp of the free parameter stays
 * with the caller). The gradients are torch autograd's, conventions at the kinks included:
 * torch.minimum splits the gradient at a tie and torch.clamp passes it at its bounds, inclusive, so
 *   - inside the clip range (A' r equals A' clamp(r)) the two halves add to the full A' r term, and a
 *     ratio exactly at 1 -+ clip_param still gets it;
 *   - (values - value_targets)^2 exactly equal to vf_clip_param still gets 2 (values - value_targets);
 *   - a row with a clipped surrogate (and no KL term) or a zero advantage has grad_mean exactly 0, a
 *     row with a clipped value error has grad_values exactly 0.
 * The clip bounds are 1 -+ clip_param formed in float64 and rounded to float32, as torch forms them.
 * Arithmetic: float32 per row, one rounding per operation, nothing contracted; the sums over rows
 * (the statistics, the shared row's gradient) are float64 in a fixed order with no atomics, so equal
 * calls give equal bits. workspace: msc_ppo_loss_workspace(n_rows, k) bytes of device memory
 * (per-block partials; 8-byte aligned; -1 for a bad shape), which the call neither allocates nor
 * keeps; it launches two kernels on `stream` and synchronises nothing.
 * Errors (msc_last_error, nothing launched): n_rows <= 0, k outside [1, 128], a null desc or required
 * pointer (idx may be null; mean_old / log_std_old only without use_kl). */
typedef struct msc_ppo_loss_desc {
  double clip_param;
  double vf_clip_param;
  double vf_loss_coeff;
  double entropy_coeff;
  double kl_coeff;
  double hysteretic_beta;   /* in (0, 1]; 1 = off */
  int32_t use_kl;
  int32_t log_std_rows;     /* 1 = one shared row [k], 0 = per row [n_rows][k] */
  int32_t accumulate_stats;
} msc_ppo_loss_desc;
int64_t msc_ppo_loss_workspace(int64_t n_rows, int32_t k);
int msc_ppo_loss(const msc_ppo_loss_desc* desc, const float* mean, const float* log_std, const float* values,
                 const int64_t* idx, const float* actions, const float* logp_old, const float* advantages,
                 const float* value_targets, const float* mean_old, const float* log_std_old, int64_t n_rows,
                 int32_t k, float* grad_mean, float* grad_log_std, float* grad_values, float* total, double* stats,
                 void* workspace, msc_stream_t stream);

/* msc_ppo_loss for n_policies policies (per-agent modules) in one call: two launches instead of two per
 * policy. Per policy bit for bit msc_ppo_loss: policy p's totals[p], stats[p], and its slices of the three
 * gradients are the bits the single call gives for (n_rows, k) on policy p's contiguous slices with
 * kl_coeff = kl_coeffs[p] (the same per-row arithmetic, row-to-block mapping and float64 summation order).
 * Every policy has n_rows rows. Layouts (float32 device buffers unless said):
 *   mean / grad_mean [n_rows][n_policies][k], values / grad_values [n_rows][n_policies];
 *   log_std [n_policies][k] (log_std_rows = 1: one shared row per policy, clamped by the caller;
 *   grad_log_std the row-summed [n_policies][k]) or [n_rows][n_policies][k] (log_std_rows = 0, grad_log_std
 *   the same shape);
 *   idx device int64 [n_rows][n_policies]: idx[i][p] is the batch row of policy p's i-th sample, in [0, B),
 *   repeats and rows shared between policies allowed, not checked. idx NULL: b = i n_policies + p, the
 *   batch interleaved like the outputs;
 *   actions [B][k], logp_old / advantages / value_targets [B], mean_old / log_std_old [B][k]: the flat batch
 *   columns msc_ppo_loss reads, one set for all policies.
 * kl_coeffs: HOST double[n_policies], one coefficient per policy (a learner adapts one per module), read
 * during the call and not kept; NULL without use_kl. desc->kl_coeff is ignored; every other field of desc
 * holds for all policies. Outputs: totals device f32[n_policies]; stats device f64[n_policies][5], stored or
 * with accumulate_stats added to, per policy as msc_ppo_loss does.
 * workspace: msc_ppo_loss_multi_workspace(n_rows, n_policies, k) = n_policies x msc_ppo_loss_workspace(n_rows,
 * k) bytes (-1 for a bad shape). The call launches two kernels on `stream`, synchronises nothing, and
 * neither allocates nor keeps memory. No atomics: equal calls give equal bits.
 * Errors (msc_last_error, nothing launched): n_rows <= 0, n_policies outside [1, 64], k outside [1, 128], a
 * null desc or required pointer (idx may be null), use_kl with null kl_coeffs, mean_old or log_std_old. */
int64_t msc_ppo_loss_multi_workspace(int64_t n_rows, int32_t n_policies, int32_t k);
int msc_ppo_loss_multi(const msc_ppo_loss_desc* desc, const double* kl_coeffs, const float* mean,
                       const float* log_std, const float* values, const int64_t* idx, const float* actions,
                       const float* logp_old, const float* advantages, const float* value_targets,
                       const float* mean_old, const float* log_std_old, int64_t n_rows, int32_t n_policies,
                       int32_t k, float* grad_mean, float* grad_log_std, float* grad_values, float* totals,
                       double* stats, void* workspace, msc_stream_t stream);

/* The learner's gradient clip and Adam step in one call: torch.nn.utils.clip_grad_norm_ per group (a group
 * is one policy: RLlib's learner clips each module's gradients by its own global norm) followed by
 * torch.optim.Adam.step (no weight decay, no amsgrad) over every tensor of every group, up to rounding order.
 *   tensors: a HOST array of n_tensors entries {p, g, m, v: float32 device buffers of n elements (the
 *   parameter, its gradient, exp_avg, exp_avg_sq), group in [0, n_groups)}. The call reads the table while
 *   it runs and keeps nothing of it: neither the table nor the pointers in it need to stay the same between
 *   calls. Entries with n = 0 are skipped. The buffers of different entries must not overlap.
 * Arithmetic. Per group, over the elements of its tensors:
 *     S = sum (double)g (double)g   in float64, in a fixed order, no atomics;   norm = sqrt(S)
 *     c = (float)min(1, max_norm / (norm + 1e-6))   in float64, rounded once;   c = 1 when max_norm <= 0
 * and with b2 = (float)beta2, a1 = (float)(1 - beta1), a2 = (float)(1 - beta2), e = (float)eps,
 * step_size = (float)(lr / (1 - beta1^step)) and r2 = (float)sqrt(1 - beta2^step), each formed on the host in
 * float64 and rounded once, per element in float32, one rounding per operation, nothing contracted, sqrt
 * and / correctly rounded:
 *     g' = g c
 *     m' = m + a1 (g' - m)
 *     v' = b2 v + (a2 g') g'
 *     p' = p - step_size (m' / (sqrt(v') / r2 + e))
 * p, m and v are updated in place; write_clipped_grads = 1 also stores g' over g (as the torch clip does),
 * 0 leaves g untouched. step is the step count after its increment (the first step is 1). Non-finite
 * gradients propagate as they do in torch; nothing is guaranteed about them.
 *   norms_out (device f64[n_groups], or NULL): every group's norm, 0 for a group without elements.
 *   workspace: msc_adam_clip_workspace(n_tensors, total_elems) bytes of device memory, total_elems the sum
 *   of the n (8-byte aligned; -1 for n_tensors <= 0 or total_elems < 0), which the call neither allocates
 *   nor keeps.
 * The table travels in the kernels' arguments, msc_adam_clip_geometry's table_capacity entries per launch:
 * one launch per that many tensors for the norms (none with max_norm <= 0 and norms_out NULL), then one per
 * that many for the update, each block over `chunk` consecutive elements of one tensor. No device
 * allocation, no synchronisation, no copy from host memory. Pointers need 4-byte alignment only: a tensor
 * whose four buffers are 16-byte aligned takes 16-byte accesses, any other 4-byte ones, with equal results.
 * Equal calls give equal bits.
 * Errors (msc_last_error, nothing launched): a null desc, table, workspace or p / g / m / v of an entry with
 * n > 0; n_tensors <= 0; n_groups <= 0; a group outside [0, n_groups); step < 1; n < 0. */
typedef struct msc_opt_tensor {
  float* p;
  float* g;
  float* m;
  float* v;
  int64_t n;
  int32_t group;
} msc_opt_tensor;
typedef struct msc_adam_clip_desc {
  double lr;
  double beta1;
  double beta2;
  double eps;
  double max_norm;              /* <= 0: no clip */
  int64_t step;                 /* after the increment, >= 1 */
  int32_t write_clipped_grads;
} msc_adam_clip_desc;
int64_t msc_adam_clip_workspace(int32_t n_tensors, int64_t total_elems);
int msc_adam_clip_geometry(int32_t* chunk, int32_t* table_capacity);
int msc_adam_clip_step(const msc_adam_clip_desc* desc, const msc_opt_tensor* tensors, int32_t n_tensors,
                       int32_t n_groups, double* norms_out, void* workspace, msc_stream_t stream);

/* Rollout action sampling (RLlib TorchDiagGaussian, rlmodules/base.py:480-557) over N rows of K:
 *   std = exp(max(log_std[n % log_std_rows][k], logstd_floor)) (one shared row, or one per agent
 *   with rows n = env * W + agent), actions = mean + std * eps (eps: standard normal draws),
 *   logp[n] = sum_k -(a - mean)^2 / (2 std^2) - log(std) - log(sqrt(2 pi)),
 *   clipped = clip(actions, -1, 1) (what the env receives; the reference's EnvRunner clips too).
 * All f32 device buffers: mean / eps / actions / clipped [N][K], log_std [log_std_rows][K], logp [N]. */
int msc_gaussian_sample(const float* mean, const float* log_std, int32_t log_std_rows, float logstd_floor,
                        const float* eps, int64_t n_rows, int32_t k, float* actions, float* logp,
                        float* clipped, msc_stream_t stream);

/* Standard-normal rollout noise keyed by global env id (no reference counterpart: RLlib draws it from
 * torch's global generator per env runner). out [n_steps][n_rows][row_len] f32: element (s, row, j)
 * depends only on (seed, row0 + row, step0 + s, j) -- Philox4x32-10, Box-Muller -- so the noise of a
 * global env is the same whichever rank owns it and however the envs are sharded.
 * Counter {j / 2, low word of row0 + row, its high word, (step0 + s) mod 2^32}, key {low word of
 * seed, high word}; output words 0 and 1 give u1 = (w0 + 0.5) 2^-32 and u2 = w1 2^-32, elements
 * 2 (j / 2) and 2 (j / 2) + 1 are sqrt(-2 log u1) times cos and sin of 2 pi u2. */
int msc_normal_keyed(float* out, int32_t n_steps, int64_t n_rows, int32_t row_len, int64_t row0, uint64_t seed,
                     uint64_t step0, msc_stream_t stream);

/* RLlib's MeanStdFilter env-to-module connector (obs_normalization "meanstd", the reference's
 * src/algorithms/mappo.py:170-171 / ippo.py:173-175; evaluation applies it with update=False,
 * base.py:131-140, :176-177), one RunningStat per column (agent x feature) of obs [n_rows][n_cols]:
 *   update != 0: every row (in row order; only rows with mask[row] != 0 when mask is given) is
 *   pushed (n += 1; M += (x - M) / n; S += (x - M_old)^2 (n - 1) / n) and normalised with the
 *   statistics that include it; update == 0: normalised with the current statistics only.
 *   out = clip((x - M) / (sqrt(var) + eps), -clip, clip) with var = S / (n - 1) (M^2 while n <= 1);
 *   clip = 0 disables clipping. out may alias obs.
 * state (device f64 [4 + 4 n_cols]): {n, buffer n, 0, 0, M[n_cols], S[n_cols], buffer M[n_cols],
 * buffer S[n_cols]}; the buffer collects the pushes since the caller last cleared it (RLlib's filter
 * buffer, merged across env runners by RunningStat.update). scratch: device f64
 * [msc_meanstd_scratch_doubles(n_rows, n_cols)] (only with update; may be null without), with
 * P = ceil(n_rows / G) segments of G = ceil(n_rows / min(n_rows, 64)) rows: 3 P n_cols segment
 * statistics, 3 n_cols final statistics and the buffer count before the call, 3 (P + 1) n_cols + 1.
 * The plan: each segment's rows are pushed sequentially from zero; a row of segment p is pushed into,
 * and normalised with, the state merged with segments 0 .. p-1 in that order (RunningStat.update,
 * m = (n1 m1 + n2 m2) / n, s = s1 + s2 + (delta^2 / n) n1 n2) and then the rows of p before it; the
 * buffer absorbs segments 0 .. P-1. A segment without a pushed row is skipped, so a call that
 * pushes nothing (an all-zero mask) leaves state as it is, bit for bit. Every operation is a float64
 * + - * / or sqrt, none contracted: out and state equal the sequential float64 evaluation of this
 * plan bit for bit (tests/meanstd_emulation.py), and a strictly sequential update to rounding. A
 * call that fails an argument check writes nothing. */
int64_t msc_meanstd_scratch_doubles(int64_t n_rows, int32_t n_cols);
int msc_meanstd_filter(const float* obs, float* out, int64_t n_rows, int32_t n_cols, const uint8_t* mask,
                       int32_t update, double* state, double* scratch, double clip, double eps,
                       msc_stream_t stream);

/* Rollout policy inference (replaces the actor's torch layer sequence in the EnvRunner's
 * _forward_inference, rlmodules/base.py:480-557, for MLPArchitecture.build networks,
 * architectures/mlp.py:14-60): out = W3 relu(W2 relu(W1 x + b1) + b2) + b3 for n_rows rows of
 * in_dim floats, in one kernel on the f32 MFMA (hidden activations stay in registers).
 * hidden1, hidden2 in {64, 128, 256, 512} (equal or not); out_dim <= 32. Weights are passed in the packed fragment
 * order the kernel streams (marlsc/mlp.py:pack_mlp3 builds them from the torch [out, in] matrices):
 *   w1p [hidden1/32][ceil(ceil(in_dim/2)/4)][64][4], w2p [hidden2/32][hidden1/8][64][4], and w3p either
 *   [hidden2/8][64][4] (MFMA output layer) or [hidden2/2][2][8] (VALU output layer, out_dim <= 8):
 *   msc_mlp3_w3_layout(out_dim) says which (0 / 1; -1 for an unsupported out_dim);
 * biases b1 [hidden1], b2 [hidden2], b3 [out_dim] as in torch. x [n_rows][in_dim], out [n_rows][out_dim]:
 * f32 device buffers; stream-ordered. pre1 (optional, [n_rows / pre1_group][hidden1]) is added to
 * the first layer's pre-activation of every row n as pre1[n / pre1_group]: the MAPPO critic's
 * first layer over local_w || global (multi_env.py:566-573) is W_local x_w + (W_global g_env + b1),
 * with the global block computed once per env (pre1_group = agents). A partial last group is legal:
 * pre1 then has ceil(n_rows / pre1_group) rows.
 *
 * Exactness. Every product (f32 MFMA, and the fma of the VALU output layer) is exact and every
 * accumulation is float32, in an order that depends on the kernel form. So when x, the weights, the
 * biases and pre1 hold integers and |b| (+ |pre1|) + sum_k |w_k| |h_k| < 2^24 at every layer, every
 * partial sum is exact and the outputs equal the integer evaluation bit for bit, for every hidden-size
 * branch, output-layer form (msc_mlp3_w3_layout) and MSC_MLP_P8 pass form; tests/test_gpu_mlp_exact.py
 * holds all of them to that. For general inputs the result is one float32 rounding order among many
 * (its error against float64 was measured at 0.5 to 0.9 of a CPU float32 evaluation's).
 * Rows are independent: a row's outputs depend on its own in_dim inputs (and its pre1 row) only, and
 * do not change with its position in the batch.
 * Non-finite inputs. A row of x that holds NaN or +-Inf leaves every other row's outputs bit-identical.
 * What that row itself returns is unspecified: the ReLU is fmaxf(h, 0), which maps a NaN hidden unit to
 * 0 where torch's relu returns NaN, so the row may come back finite. The same holds for
 * msc_mlp2_relu_forward, the _sampled entry points and msc_mlp{2,3}_relu_musigma below. */
int msc_mlp3_w3_layout(int32_t out_dim);
int msc_mlp3_relu_forward(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                          int32_t out_dim, const float* w1p, const float* b1, const float* w2p, const float* b2,
                          const float* w3p, const float* b3, float* out, const float* pre1, int32_t pre1_group,
                          msc_stream_t stream);

/* The one-hidden-layer form out = W3 relu(W1 x + b1) + b3 (MLPArchitecture.build with
 * hidden_sizes [H]: the reference IPPO actor / critic [256], config_files/algorithms/ippo.yaml:46,52,
 * and the test configs' [128] / [1024] heads), hidden a multiple of 32 up to 1024, out_dim <= 32:
 * the hidden layer is produced 256 units at a time and folded into the outputs in registers.
 * w1p as msc_mlp3_relu_forward's (hidden1 = hidden), w3p as its output layer with hidden2 = hidden
 * (layout by msc_mlp3_w3_layout(out_dim)); pre1 / pre1_group as there. */
int msc_mlp2_relu_forward(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t out_dim,
                          const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                          const float* pre1, int32_t pre1_group, msc_stream_t stream);

/* The actor forward and the rollout's action sampling in one launch: msc_mlp3_relu_forward /
 * msc_mlp2_relu_forward followed, while the out_dim means of each row are still in registers, by
 * msc_gaussian_sample's arithmetic (bit-identical to the separate call) into sample->actions /
 * logp / clipped. out (the means) may be NULL. Needs the VALU output layer (out_dim <= 8,
 * msc_mlp3_w3_layout(out_dim) == 1). Replaces the EnvRunner's _forward_inference -> TorchDiagGaussian
 * sample pair (rlmodules/base.py:480-557). */
typedef struct msc_gaussian_epilogue {
  const float* log_std;   /* [log_std_rows][out_dim]: row n % log_std_rows applies to row n */
  int32_t log_std_rows;
  float logstd_floor;
  const float* eps;       /* [n_rows][out_dim] standard-normal draws */
  float* actions;         /* [n_rows][out_dim] */
  float* logp;            /* [n_rows] */
  float* clipped;         /* [n_rows][out_dim] */
} msc_gaussian_epilogue;
int msc_mlp3_relu_forward_sampled(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                                  int32_t out_dim, const float* w1p, const float* b1, const float* w2p,
                                  const float* b2, const float* w3p, const float* b3, float* out,
                                  const float* pre1, int32_t pre1_group, const msc_gaussian_epilogue* sample,
                                  msc_stream_t stream);
int msc_mlp2_relu_forward_sampled(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t out_dim,
                                  const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                                  const float* pre1, int32_t pre1_group, const msc_gaussian_epilogue* sample,
                                  msc_stream_t stream);

/* Per-agent policies in one launch: with parameter_sharing: false (the reference schema's default) every
 * warehouse has its own RLModule (the policy mapping of ippo.py:106 / mappo.py:103), and the EnvRunner's
 * _forward_inference (rlmodules/base.py:480-557) runs once per module. These entry points evaluate
 * n_policies same-shaped MLPs with n_policies weight sets over rows laid out [n_rows / n_policies][n_policies]:
 * row n belongs to policy n % n_policies. n_rows must be a multiple of n_policies, 1 <= n_policies <= 64.
 * w1p / w2p / w3p are n_policies consecutive single-policy packs, each exactly as msc_mlp3_relu_forward
 * (msc_mlp2_relu_forward) takes it, b1 / b2 / b3 n_policies consecutive bias vectors. x [n_rows][in_dim];
 * pre1 (optional) [n_rows][hidden1], one row per row. sample may be NULL (means only, out required);
 * with it out may be NULL, out_dim <= 8 (msc_mlp3_w3_layout(out_dim) == 1) as for the _sampled entry
 * points, and log_std_rows must be 1 or n_policies (row p applies to policy p). Shape limits are the
 * single-policy entry points'; a call that violates any condition returns an error and writes nothing.
 * Nothing is read or written past n_rows rows.
 *
 * Contract. For every policy p, the outputs of rows p, p + n_policies, ... equal, bit for bit, what
 * msc_mlp{3,2}_relu_forward[_sampled] returns for policy p's rows (x, pre1, eps) gathered contiguously,
 * with policy p's pack and biases, pre1_group = 1 and log_std row p (the kernels are the same templates,
 * with rows addressed at stride n_policies). So msc_mlp3_relu_forward's exactness and non-finite
 * paragraphs hold per policy: integer data under the 2^24 headroom condition gives the integer
 * evaluation bit for bit, and a row holding NaN or +-Inf changes no other row, of its own policy or of
 * another. The result does not depend on the block order (MSC_MULTI_ORDER = 0 policy-major, 1
 * policy-minor, the default; read at each launch) or on where blocks are placed. */
int msc_mlp3_relu_multi(const float* x, int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1,
                        int32_t hidden2, int32_t out_dim, const float* w1p, const float* b1, const float* w2p,
                        const float* b2, const float* w3p, const float* b3, float* out, const float* pre1,
                        const msc_gaussian_epilogue* sample, msc_stream_t stream);
int msc_mlp2_relu_multi(const float* x, int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden,
                        int32_t out_dim, const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                        const float* pre1, const msc_gaussian_epilogue* sample, msc_stream_t stream);

/* Wide-output policy inference: the centralised (CPPO) actor maps the global observation to the joint
 * action, n_warehouses * L -> hidden -> n_warehouses * n_skus (the reference's src/algorithms/cppo.py
 * builds it with MLPArchitecture.build, architectures/mlp.py:14-60; 40 outputs at C3, 80 at C5).
 * Replaces, for 1 <= out_dim <= 128, the actor's torch layer sequence in _forward_inference and, with
 * `sample`, the TorchDiagGaussian sample after it (rlmodules/base.py:480-557): the same networks,
 * in_dim, pre1 / pre1_group and exactness / row-independence / non-finite-row statements as
 * msc_mlp3_relu_forward and msc_mlp2_relu_forward, with the output layer on ceil(out_dim / 32) <= 4
 * MFMA tiles. w1p / w2p as there; w3p [ceil(out_dim/32)][hidden_last/8][64][4]: the layout-0 (MFMA)
 * fragment order of msc_mlp3_relu_forward once per 32-row slice of W3, slices concatenated, rows past
 * out_dim zero (marlsc/mlp.py:pack_wide).
 * sample may be NULL (means only, out required); with it, out may be NULL. actions and clipped are
 * msc_gaussian_sample's, operation for operation, and logp adds the row's out_dim terms sequentially
 * in k from 0.0f as that kernel does, so all three are bit-identical to msc_gaussian_sample run on
 * the means. Nothing is read or written past n_rows rows or out_dim columns; n_rows = 0 launches nothing.
 * msc_mlp_wide_supported(hidden1, hidden2 (0: one hidden layer), out_dim): 1 when a wide kernel
 * exists (hidden sizes as the narrow kernels', 1 <= out_dim <= 128), else 0; the entry points return
 * an error, without a launch, for anything else. */
int msc_mlp_wide_supported(int32_t hidden1, int32_t hidden2, int32_t out_dim);
int msc_mlp3_relu_wide(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                       int32_t out_dim, const float* w1p, const float* b1, const float* w2p, const float* b2,
                       const float* w3p, const float* b3, float* out, const float* pre1, int32_t pre1_group,
                       const msc_gaussian_epilogue* sample, msc_stream_t stream);
int msc_mlp2_relu_wide(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t out_dim,
                       const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                       const float* pre1, int32_t pre1_group, const msc_gaussian_epilogue* sample,
                       msc_stream_t stream);

/* Team reward of the centralised view: replaces the reference wrapper's sum(rewards.values())
 * (src/environment/envs/single_env.py:156). rewards [n_envs][n_agents] f64 (device); per env the
 * agent-order sum ((r0 + r1) + r2) ... in f64 to out64 [n_envs] and, rounded once, to out32 [n_envs]
 * (either may be NULL, not both). One launch. */
int msc_reward_team_sum(const double* rewards, int64_t n_envs, int32_t n_agents, float* out32, double* out64,
                        msc_stream_t stream);

/* Rollout inference of a mu / sigma-head actor (use_mu_sigma_head): replaces the torch layer sequence
 * backbone -> MuSigmaHead.forward (architectures/mu_sigma_head.py:52-82, wired in
 * rlmodules/base.py:434-435) and, with the sampling buffers, the EnvRunner's TorchDiagGaussian
 * sample (rlmodules/base.py:480-557), by one launch. The backbone is MLPArchitecture.build with
 * output_dim = hidden[-1] and no output activation; its last Linear is followed by the two Linear
 * heads with no nonlinearity in between, so the caller folds them (marlsc/mlp.py:fold_head, in f64,
 * rounded once): W_eff = [W_mu; W_sigma] W_out ([2k][hidden]), b_eff = [W_mu; W_sigma] b_out +
 * [b_mu; b_sigma]. Per row: o = W_eff relu(.. hidden layers ..) + b_eff,
 *   mu = act_mu(o[0..k)), log_std = clamp(act_sigma(o[k..2k)), log_std_min, log_std_max)
 * (the mean is not clamped); dist_out [n_rows][2k] = [mu || log_std] when non-NULL; when eps is
 * non-NULL, actions / logp / clipped as msc_gaussian_sample(mu, log_std with one row per row, floor
 * log_std_min) computes them, operation for operation (bit-identical to that two-launch sequence).
 * k <= 8 (9..16: msc_mlp{2,3}_relu_forward on W_eff with out_dim = 2k, then msc_gaussian_sample).
 * w1p / w2p / b1 / b2 / pre1 / pre1_group as msc_mlp3_relu_forward's; bh = b_eff [2k];
 * whp [hidden/2][2][stride] floats, the dual-head VALU layout msc_mlp_musigma_layout reports:
 *   whp[s][h][c] = W_eff[c < stride/2 ? c : k + c - stride/2][32 (s / 16) + rho(s % 16, h)],
 *   rho(r, h) = (r & 3) + 8 (r >> 2) + 4 h, zero where the head's column (c mod stride/2) >= k.
 * msc_mlp_musigma_layout(hidden1, hidden2 (0: one hidden layer), k, &width, &stride): 0 and the
 * per-head register width / stride, or an error when there is no dual-head kernel: k outside 1..8,
 * unsupported hidden sizes (one hidden layer: up to 1024 units for k <= 4, 512 above), the MFMA
 * output layer forced (MSC_MLP_V3=0), or a [256, 256] A/B form without a head variant
 * (MSC_MLP_P8 = 4 / 2).
 * Exactness. The pre-activations o are sums of exact products accumulated in float32, as
 * msc_mlp3_relu_forward's: with integer x, weights, biases and pre1 under its headroom condition
 * they are the integer evaluation, and so are they, as num / 2^s, when rows of W_eff and b_eff are
 * such integers scaled by powers of two. On an exact o:
 *   MSC_ACT_NONE and MSC_ACT_RELU are exact; MSC_ACT_ELU (alpha = 1) returns o itself for o > 0;
 *   tanh, ELU's negative branch, GELU and sigmoid stay within 4 max(e32, 1) units of the float64
 *   value, one unit being 2^-24 |f(o)| (for GELU 2^-24 max(|f(o)|, |o| / 2): it is computed as
 *   0.5 o (1 + erf(o / sqrt 2)), whose last factor carries an absolute error), and e32 the error of
 *   a float32 evaluation of the same formula operation by operation (1.4 to 2.7 units). Measured:
 *   at most 0.32 of that bound ("Mu/sigma head"). The sigmoid 1 / (1 + expf(-o)) is 0
 *   for o < -88.7, where the true value is a float32 denormal: no relative bound is claimed there;
 *   the clamp is exact: a log_std whose activation lies past a limit by more than the bound above is
 *   that limit's float32 value, and mu is never clamped.
 * Only columns < k are stored or sampled: whp's padded columns and what lies past bh[2k) and past
 * eps[n_rows * k) are not read into any result, and nothing is written past n_rows rows of the four
 * outputs (n_rows = 0 launches nothing). An activation code outside MSC_ACT_* is an error, not NONE.
 * tests/test_gpu_musigma_exact.py holds every hidden-size branch, pass form and one-layer form to
 * this for k = 1..8. */
#define MSC_ACT_NONE 0
#define MSC_ACT_RELU 1
#define MSC_ACT_TANH 2
#define MSC_ACT_ELU 3
#define MSC_ACT_GELU 4 /* erf form */
#define MSC_ACT_SIGMOID 5
typedef struct msc_musigma_epilogue {
  int32_t act_mu, act_sigma;       /* MSC_ACT_* */
  float log_std_min, log_std_max;  /* MuSigmaHead.LOG_STD_MIN / LOG_STD_MAX: -4.6, 4.6 */
  const float* eps;                /* [n_rows][k] standard-normal draws; NULL: no sampling */
  float* actions;                  /* [n_rows][k]  (all three non-NULL exactly when eps is) */
  float* logp;                     /* [n_rows] */
  float* clipped;                  /* [n_rows][k] */
  float* dist_out;                 /* [n_rows][2k] = [mu || log_std], or NULL */
} msc_musigma_epilogue;
int msc_mlp_musigma_layout(int32_t hidden1, int32_t hidden2, int32_t k, int32_t* width, int32_t* stride);
int msc_mlp3_relu_musigma(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2, int32_t k,
                          const float* w1p, const float* b1, const float* w2p, const float* b2, const float* whp,
                          const float* bh, const float* pre1, int32_t pre1_group, const msc_musigma_epilogue* head,
                          msc_stream_t stream);
int msc_mlp2_relu_musigma(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t k, const float* w1p,
                          const float* b1, const float* whp, const float* bh, const float* pre1, int32_t pre1_group,
                          const msc_musigma_epilogue* head, msc_stream_t stream);

/* Diagnostic (no reference counterpart), without touching a GPU: the kernel instantiation and launch
 * geometry the fused-MLP entry points of a family would pick under the current MSC_MLP_* knobs, for
 * hidden sizes [hidden1, hidden2] (hidden2 = 0: one hidden layer), out_dim outputs (MSC_MLP_MUSIGMA: k
 * actions) and n_rows rows (MSC_MLP_MULTI: of n_policies policies, which must divide n_rows; ignored by
 * the other families). All forms of a family return the same bits, so this is what shows which one runs.
 * Writes up to n of
 *  {supported (0: the entry point would refuse these sizes, and every other value is 0),
 *   NT1, NT2 (hidden tiles of 32 units; NT2 = 0 with one hidden layer), P (layer-2 tiles per pass),
 *   waves per SIMD, IL (output layer interleaved into the next pass), output-layer width (VALU outputs of
 *   the plain families, 0 = the MFMA output layer; per-head width of the mu/sigma head; output tiles of
 *   the wide family), TB (hidden tiles per group with one hidden layer, else 0), dynamic LDS bytes,
 *   grid blocks (of 256 threads)};
 * returns the count written (MSC_MLP_PLAN_N at most), or < 0 for an unknown family or bad row /
 * policy counts. */
#define MSC_MLP_RELU 0    /* msc_mlp{3,2}_relu_forward[_sampled] */
#define MSC_MLP_MULTI 1   /* msc_mlp{3,2}_relu_multi */
#define MSC_MLP_MUSIGMA 2 /* msc_mlp{3,2}_relu_musigma */
#define MSC_MLP_WIDE 3    /* msc_mlp{3,2}_relu_wide */
#define MSC_MLP_PLAN_N 10
int msc_mlp_plan(int32_t family, int32_t hidden1, int32_t hidden2, int32_t out_dim, int64_t n_rows, int32_t n_policies,
                 int32_t* out, int32_t n);

/* The parameter gradients of a plain ReLU MLP in place of torch autograd through the module
 * MLPArchitecture.build returns (architectures/mlp.py:14-60) inside PPOTorchLearner.compute_gradients:
 * for y = W3 relu(W2 relu(W1 x + b1) + b2) + b3 (hidden2 = 0: y = W3 relu(W1 x + b1) + b3) and an upstream
 * gradient d_out [n_rows][out_dim] (msc_ppo_loss's grad_mean / grad_values, or autograd's),
 *   g_w3 = scale d_out^T h_last, g_b3 = scale sum_rows d_out, d_last = (z_last > 0) . W3^T d_out, and so on down
 * to g_w1 = scale d1^T x. No input gradient is computed (the observations are leaves).
 * The supported set is msc_mlp{3,2}_relu_forward's: hidden1, hidden2 in {64, 128, 256, 512}, or hidden2 = 0 and
 * hidden1 a multiple of 32 up to 1024; in_dim <= 1024, out_dim <= 32.
 * Inputs (f32 device buffers, stream-ordered): x [n_rows][in_dim]; w1p, b1, w2p, b2 exactly as the forward
 * entry points take them (w3 is staged in LDS by each block when out_dim x hidden_last floats fit 64 KiB, which
 * they always do with two hidden layers); w2tp the pack of W2^T (the w2p index map applied to the transposed matrix:
 * w2tp[t1][s4][lane][i] = W2[32 t2 + rho(r, h)][32 t1 + c], 4 s4 + i = 16 t2 + r; marlsc/mlp.py:pack_w2t; NULL with
 * one hidden layer, as are w2p, b2, g_w2, g_b2); w3 [out_dim][hidden_last] in torch's own layout (not the
 * forward's w3p: the layout does not depend on out_dim here). b1, b2, the packs, w3 and the workspace must be
 * 16-byte aligned.
 * Outputs in torch's layouts, ready to be .grad: g_w1 [hidden1][in_dim], g_b1 [hidden1], g_w2 [hidden2][hidden1],
 * g_b2 [hidden2], g_w3 [out_dim][hidden_last], g_b3 [out_dim]. scale multiplies every gradient; accumulate = 1
 * adds to what the buffers hold, 0 overwrites (prior contents, NaN included, are ignored). n_rows = 0 writes
 * zeros (accumulate = 0) or nothing (accumulate = 1) and launches nothing that reads x.
 * Nothing is saved by the forward: the hidden pre-activations are recomputed from x with the forward kernels'
 * packs in the forward kernels' accumulation order, so the ReLU masks are those of msc_mlp{3,2}_relu_forward
 * bit for bit. The mask is z > 0: zero gradient at z == 0, as torch.
 * Deterministic: no atomics; the reduction over rows runs in tiles of 32, split-K slices and rounds that are
 * functions of the shape arguments alone, added in a fixed order, so two calls on the same inputs give the
 * same bits. Exactness: products are exact in f32 and every sum is accumulated in f32, except the bias gradients'
 * sums over rows, which are accumulated in f64 and rounded to f32 once per slice; with integer x, weights,
 * biases and d_out whose absolute-value evaluation stays below 2^24 at every partial sum (and a power-of-two
 * scale), all six gradients equal the int64 evaluation bit for bit, whatever the reduction order. With real
 * data the order differs from torch's GEMMs: compare at f32 GEMM tolerance. No non-finite-row guarantee: a NaN
 * row reaches the sums.
 * workspace: msc_mlp_relu_backward_workspace(...) bytes of device memory (-1 for an unsupported shape), owned by
 * the caller and free again once the stream has passed the call. The bytes are monotone in n_rows and capped:
 * rows are processed in rounds of at most 16,384 (hidden1 + hidden2 <= 512) or 8,192 rows inside the call,
 * each accumulated onto the outputs, so the workspace never exceeds 64 MiB of operands (2 (hidden1 + hidden2)
 * floats per row of a round) plus 8 slices of partials (one padded copy of the six gradients each).
 * An unsupported shape or a NULL required pointer returns an error and writes nothing. */
int64_t msc_mlp_relu_backward_workspace(int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2, int32_t out_dim);
int msc_mlp_relu_backward(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2, int32_t out_dim,
                          const float* w1p, const float* b1, const float* w2p, const float* b2, const float* w2tp,
                          const float* w3, const float* d_out, float scale, int32_t accumulate, float* g_w1, float* g_b1,
                          float* g_w2, float* g_b2, float* g_w3, float* g_b3, void* workspace, msc_stream_t stream);

/* The same gradients for the n_policies same-shaped networks of per-agent policies (parameter_sharing: false) in
 * one call: three launches per round for a whole group of policies instead of three per policy.
 * Layout, msc_mlp{3,2}_relu_multi's: x [n_rows][in_dim] and d_out [n_rows][out_dim] hold the rows ordered
 * [n_rows / n_policies][n_policies], row r belongs to policy r % n_policies and is read where it lies, at stride
 * n_policies (never gathered). w1p, b1, w2p, b2, w2tp are n_policies consecutive single-policy packs / vectors,
 * each exactly as msc_mlp_relu_backward takes one; w3 is [n_policies][out_dim][hidden_last]. The six outputs are
 * the stacked torch layouts g_w1 [n_policies][hidden1][in_dim], g_b1 [n_policies][hidden1], ...,
 * g_b3 [n_policies][out_dim]. 1 <= n_policies <= 64 and n_policies divides n_rows; the shape set, the alignment
 * rules and the NULL rules are msc_mlp_relu_backward's. A violated condition returns an error (msc_last_error)
 * and writes nothing. n_rows = 0: zeros over all the stacked outputs (accumulate = 0) or nothing (accumulate = 1);
 * x is not read.
 * Contract: for every policy p, the six gradients equal, bit for bit, what msc_mlp_relu_backward returns for policy
 * p's n_rows / n_policies rows gathered contiguously, with policy p's packs and the same scale and accumulate.
 * Every policy keeps that call's geometry (row tiles of 32, slices, rounds, partials) in a workspace section of its
 * own, the policy index comes from the grid, and there are no atomics; so the determinism, the integer exactness
 * (2^24 headroom) and the mask (z > 0, the forward kernels' masks) paragraphs above hold per policy, and the result
 * depends neither on the block order nor on the grouping below. Nothing is read or written past n_rows rows, and
 * nothing is written past the stacked outputs or past the workspace bytes the query returned.
 * workspace: msc_mlp_relu_backward_multi_workspace(...) bytes (-1 exactly where the single query is, or for a bad
 * n_policies / n_rows pair) = G x msc_mlp_relu_backward_workspace(n_rows / n_policies, ...): the policies run in
 * groups of G per set of launches, G the largest count (at least 1, at most n_policies) for which G workspaces at
 * the single call's cap fit 1 GiB. G depends on in_dim, the hidden sizes and out_dim alone, so the bytes are
 * monotone in n_rows and capped.
 * msc_mlp_relu_backward_multi_plan touches no GPU: it writes up to n of
 *  {supported (0: the call would refuse these sizes, and every other value is 0), policies per group G,
 *   groups = ceil(n_policies / G), rounds per policy, slices per round, row tiles of a full round (of the only
 *   round when there is one), workspace bytes}
 * and returns the count written (MSC_MLP_BWD_MULTI_PLAN_N at most), or < 0 for a NULL out. */
#define MSC_MLP_BWD_MULTI_PLAN_N 7
int64_t msc_mlp_relu_backward_multi_workspace(int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1,
                                              int32_t hidden2, int32_t out_dim);
int msc_mlp_relu_backward_multi_plan(int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                                     int32_t out_dim, int64_t* out, int32_t n);
int msc_mlp_relu_backward_multi(const float* x, int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1,
                                int32_t hidden2, int32_t out_dim, const float* w1p, const float* b1, const float* w2p,
                                const float* b2, const float* w2tp, const float* w3, const float* d_out, float scale,
                                int32_t accumulate, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_w3,
                                float* g_b3, void* workspace, msc_stream_t stream);

/* One time step of a GRU network for n_rows rows in one launch: replaces the module
 * GRUArchitecture.build returns (architectures/gru.py:14-85: nn.GRU(batch_first) -> output_proj =
 * [act,] Linear [, act]) as BaseRLModule._forward_gru steps it on a [B, obs_dim] input
 * (rlmodules/base.py:99-141), the state laid out as get_initial_state gives it ([B, layers, hidden],
 * base.py:351-388). Per layer, PyTorch's gate order and formula:
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
 *   n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h
 * layer 2 reads layer 1's h'; y = act_out(W_o act_pre(h'_last) + b_o) (MSC_ACT_* codes).
 * x [n_rows][in_dim], h_in / h_out [n_rows][layers][hidden], y [n_rows][out_dim]: f32 device buffers,
 * stream-ordered. h_out NULL: the new state is not stored (V(final_obs) bootstrap); h_out == h_in is an
 * error (ping-pong two buffers). reset (optional, u8 [n_rows / reset_group]): rows whose group's flag
 * is non-zero read h_in as zero (the env's truncation row of the previous step, reset_group = agents).
 * The fused set (msc_gru_supported: 1 / 0): hidden in {64, 128, 256}, layers 1 or 2, in_dim <= 1024,
 * out_dim <= 32 or a multiple of 32 up to 256. Packed weights (marlsc/gru.py:pack_gru), with
 * rho(r, h) = (r & 3) + 8 (r >> 2) + 4 h, c = lane & 31, h = lane >> 5, NT = hidden / 32, gate rows in
 * torch's order (tile T = gate NT + t covers rows 32 T .. 32 T + 31 of the [3 hidden][.] matrices):
 *   wi[0] [3 NT][M4][64][4]: W_ih_l0[32 T + c][h KS + 4 m4 + i], KS = ceil(in_dim / 2), M4 = ceil(KS / 4),
 *                            zero where 4 m4 + i >= KS or the column is past in_dim;
 *   wi[1], wh[l] [3 NT][4 NT][64][4]: W[32 T + c][32 (s / 16) + rho(s % 16, h)], s = 4 s4 + i;
 *   b[l] [4 hidden] = [b_ir + b_hr | b_iz + b_hz | b_in | b_hn];
 *   wo [ceil(out_dim / 32)][4 NT][64][4]: W_o[32 q + c][32 (s / 16) + rho(s % 16, h)], zero for rows
 *   past out_dim; bo [out_dim]. */
typedef struct msc_gru_weights {
  const float* wi[2];
  const float* wh[2];
  const float* b[2];
  const float* wo;
  const float* bo;
} msc_gru_weights;
int msc_gru_supported(int32_t in_dim, int32_t hidden, int32_t layers, int32_t out_dim);
int msc_gru_step(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t layers, int32_t out_dim,
                 const float* h_in, const msc_gru_weights* w, int32_t act_pre, int32_t act_out, const uint8_t* reset,
                 int32_t reset_group, float* y, float* h_out, msc_stream_t stream);

/* Heuristic baseline policies on the device state of a handle: replaces the action functions of the
 * reference's src/experiments/run_baselines.py, which read the env object between two steps --
 *   MSC_POLICY_BASE_STOCK <- make_bs_newsvendor_action_fn / make_bs_optimized_action_fn  run_baselines.py:133-207, :296-337
 *   MSC_POLICY_ADAPTIVE   <- make_adaptive_bs_action_fn                                   run_baselines.py:209-294
 *   MSC_POLICY_RANDOM     <- make_random_action_fn                                        run_baselines.py:73-94
 * (the constant-order policy, :96-131, is a fixed action tensor of the caller). msc_policy_act writes
 * the actions [E][W][K] of every env in one launch on `stream`, from the env's on-hand inventory, its
 * pending orders (env._compute_pending_matrix), last step's home demand (env._incoming_demand_home)
 * and timestep as they stand between two msc_env_step calls (after an in-step auto-reset: the new
 * episode's). With q(x) = min(max(x, 0), maxq[k]) and act(x) = (float)(2 q(x) / maxq[k] - 1), all
 * float64 with one rounding to float32 (maxq = the `direct` action space's max_order_quantities):
 *   base-stock: act(S[cand[e]][w, k] - inventory - pending);
 *   adaptive:   at timestep 0 the env's demand window is cleared and every action is -1; otherwise
 *               last step's home demand is appended and, over the window's last n = min(count,
 *               H[cand[e]]) entries, oldest first: mean = float32 sequential sum / (float)n; var = mean
 *               when n == 1, else the float32 sequential sum of (x - mean) * (x - mean) / (float)n
 *               (numpy's axis-0 mean / var of a float32 stack); S = L mean + z[cand[e]] sqrt(L var) in
 *               float64 with L the expected lead time; act(S - inventory - pending);
 *   random:     W * K draws of numpy's Generator.random() in (agent, SKU) order from the env's own
 *               PCG64 state, (float)(-1.0 + 2.0 u) (Generator.uniform(-1, 1) cast to float32).
 * Every env carries a candidate index cand[e] < n_candidates into the tables S [n_candidates][W*K]
 * f64, z [n_candidates] f64, H [n_candidates] i32, so one handle sweeps many parameter sets at once.
 * msc_policy_create (synchronous) takes HOST arrays: S_host (base-stock), z_host and H_host (adaptive;
 * 1 <= H <= h_max, h_max <= 0: the largest H given), cand_host [E] (NULL: all 0), rng_state_host
 * [E][4] u64 {state_hi, state_lo, inc_hi, inc_lo} (random); arrays a kind does not use may be NULL.
 * The env's action space must be `direct` (the reference's baselines assume it too). The demand
 * window [h_max][W*K][E], its count and the RNG states belong to the policy, not to the env: they are
 * not part of msc_env_save_state. msc_policy_set_tables (synchronous) replaces S / z / H / cand (NULL:
 * kept) for the same n_candidates without reallocating. An argument error returns < 0 with a message
 * and launches nothing. */
typedef struct msc_policy msc_policy;
enum msc_policy_kind { MSC_POLICY_BASE_STOCK = 0, MSC_POLICY_ADAPTIVE = 1, MSC_POLICY_RANDOM = 2 };
int msc_policy_create(const msc_env* env, int32_t kind, int32_t n_candidates, int32_t h_max, const double* S_host,
                      const double* z_host, const int32_t* H_host, const int32_t* cand_host,
                      const uint64_t* rng_state_host, msc_policy** out);
int msc_policy_act(msc_policy* policy, const msc_env* env, float* actions, msc_stream_t stream);
int msc_policy_set_tables(msc_policy* policy, int32_t n_candidates, const double* S_host, const double* z_host,
                          const int32_t* H_host, const int32_t* cand_host);
void msc_policy_destroy(msc_policy* policy);

/* Utility: numpy's Generator.poisson on the device (synchronous; the env's own sampler, exposed for
 * known-answer tests): n draws with the rates lam_host[i % n_lam] (random_poisson: multiplication
 * method below 10, PTRS at or above, numpy/random/src/distributions/distributions.c) from the PCG64
 * state_host[6] {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger} (the layout of
 * msc_env_read_state's rng); draws -> out_host [n], the final state -> state_out_host (may be NULL). */
int msc_poisson_draws(const uint64_t* state_host, const double* lam_host, int64_t n_lam, int64_t n,
                      int64_t* out_host, uint64_t* state_out_host);

/* Utility: the demand generators' draw on the device (synchronous; exposed for known-answer tests).
 * One 64-lane block: lane l starts from the 128-bit PCG64 state state_host[2l], state_host[2l + 1]
 * ({high, low} halves) and n times writes numpy's random() of its state (the double's bit pattern,
 * out_host[l * n + i]) and advances the state to state * M^stride + inc (mod 2^128), M the PCG64
 * multiplier and inc the lane's stride increment inc_host[2l], inc_host[2l + 1] (any value);
 * stride is 1, 2, 3, 5 or 7. The final states -> state_out_host [64][2]. */
int msc_gen_draws(const uint64_t* state_host, const uint64_t* inc_host, int32_t stride, int64_t n, uint64_t* out_host,
                  uint64_t* state_out_host);

/* Utility: SeedSequence(words).generate_state(1, uint32)[0] (numpy-compatible), on the host. */
uint32_t msc_seedseq_u32(const uint32_t* words, int32_t n_words);

const char* msc_last_error(void);
int msc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MARLSC_H */
