// capi.hip -- the extern "C" boundary of libmarlsc.so (include/marlsc.h).
//
// Host responsibilities only: validate the descriptor (the reference's EnvironmentConfig shape
// rules, src/config/schema.py:664-890), precompute the read-only tables (home regions
// multi_env.py:144, closest warehouses lost_sales_handler.py:36, exp(-lambda) with the host libm
// exactly as numpy's random_poisson does, transposed outbound costs), derive per-env root seeds
// (SeedManager.derive_env_seed, seed_manager.py:165-186), own the HBM arenas and launch the
// kernels of env_kernels.hip / gae.hip on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/marlsc.h"
#include "env.hpp"
#include "env_plan.hpp"
#include "mlp_backward.hpp"
#include "mlp_dispatch.hpp"
#include "rng.hpp"

using namespace msc;

static thread_local char g_err[512] = "";

static int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
#define HIP_TRY(x)                                                                   \
  do {                                                                               \
    hipError_t _e = (x);                                                             \
    if (_e != hipSuccess) return set_err(-2, "%s: %s", #x, hipGetErrorString(_e));   \
  } while (0)

struct msc_env {
  EnvConst c;
  EnvState s;
  int device;
  void* tables = nullptr;   // device copy of every static table
  void* arena = nullptr;    // persistent per-env state (checkpointed by save/load_state)
  size_t arena_bytes = 0;
  void* scratch = nullptr;    // two per-step order buffers (double-buffered for pipelining)
  size_t order_bytes = 0;     // bytes of one order buffer (records + counts)
  DevEnv* dev = nullptr;      // device copies of {c, s}: dev[b] points at order buffer b
  void* al_tail = nullptr;    // s.al_tail: one int32 per 64 envs (msc_env_alloc_tail_entry)
  // Demand pipelining: the Poisson demand of step tau+1 depends only on each env's own demand
  // stream, so it is generated on a side stream while the step kernel of tau runs (their waves
  // co-reside on the CUs), unless step tau ends an episode (the in-kernel reset re-seeds the
  // demand stream) or the envs' timesteps are out of sync after a masked reset.
  hipStream_t side = nullptr;
  hipEvent_t ev_dem[2] = {nullptr, nullptr}, ev_step[2] = {nullptr, nullptr}, ev_reset = nullptr;
  // the stream each ev_dem was last recorded on (a wait from that same stream is already ordered),
  // and whether the side stream has waited on the latest ev_reset (a reset is recorded once)
  hipStream_t ev_dem_on[2] = {nullptr, nullptr};
  bool side_saw_reset = false;
  bool ev_elide = true;  // MSC_EV_ELIDE=0: every wait is issued (A/B)
  int64_t tau = 0;                // steps issued
  int t_sync = -1;                 // common timestep of every env, -1 if unknown
  bool ready[2] = {false, false};  // order buffer b holds the demand of the next step using it
  bool pipeline = true;
  // msc_env_set_timing: event pairs around demand / step launches (2 per launch)
  std::vector<hipEvent_t> tev_dem, tev_step;
  int t_cap = 0, n_tdem = 0, n_tstep = 0;
  // Episode-ahead demand (EA; few envs per GPU). A Poisson episode's orders
  // depend only on its seed (SeedSequence([root, counter]), seed_manager.py:100-120), not on
  // actions, so whole future episodes are generated on side streams while earlier ones step: slot
  // n % S holds episode n (counted from the snapshot taken when EA started, episode 0 = the one
  // running then, which keeps the per-step path). At the end of episode n its slot is refilled
  // with episode n + S. Any desynchronising event (masked reset, load_state, disabling) stops it;
  // it restarts at the next common episode start.
  int64_t ea_budget = 0, ea_bytes = 0;  // episode-ahead memory budget and bytes allocated (create time)
  bool ea_enabled = false;  // configured: Poisson demand, few envs (or MSC_EA=1), buffers allocated
  bool ea_paused = false;   // msc_env_set_episode_ahead(0): per-step demand until re-enabled
  // step_c staging / chain priority of the per-step path and with EA on, both pairs fixed at create
  int32_t obs_stage_pe = 0, chain_prio_pe = 0, obs_stage_ea = 0, chain_prio_ea = 0;
  bool ea_running = false;
  int64_t ea_n = 0;         // episode (relative to the snapshot) the envs are in
  int ea_cur = -1;          // slot of the current episode, -1: per-step demand
  void* ea_mem = nullptr;
  // One launch is a chain of T per-step parses (~60 ms at 8 x 64 x 5) whatever its lane count,
  // while the envs consume an episode in T steps: freed slots are refilled ea_batch at a time, in
  // one launch of ea_batch x E lanes on one stream (separate streams would share the process's few
  // hardware queues and serialise anyway).
  hipStream_t ea_stream = nullptr;
  int ea_batch = 1;         // slots per refill launch
  int ea_freed = 0;         // consumed slots not yet refilled
  // A generation runs as chunks of ea_chunk steps, each launched once the previous one has finished
  // (polled at every step call; flushed when a step needs the slot), so that the EA work queued on
  // the device at any time -- what a device-wide synchronize waits for -- is one short chunk.
  int ea_chunk = 50;
  struct EaItem { EaLaunch l; int wait_cons; };  // wait_cons: slot whose ev_cons precedes chunk 0 (-1: none)
  std::vector<EaItem> ea_q;  // generations not yet fully launched (head: the one in progress)
  bool ea_chunk_out = false; // a chunk of the head item is in flight (ev_chunk)
  hipEvent_t ev_chunk = nullptr;
  bool gen_pending[MSC_EA_MAX_S] = {};  // slot's generation not fully launched (ev_gen stale)
  hipEvent_t ev_gen[MSC_EA_MAX_S] = {}, ev_cons[MSC_EA_MAX_S] = {}, ev_snap = nullptr;
  std::vector<hipEvent_t> tev_ea;  // timing of EA launches (msc_env_set_timing)
  std::vector<double> tea_work;    // env-steps generated by each timed EA launch
  // demand work issued since create (msc_env_work_counters): episode-ahead generation launches
  // (chunks) and the env-steps of demand they draw; per-step demand launches (E env-steps each); steps
  int64_t cnt_ea_launch = 0, cnt_dem_launch = 0, cnt_steps = 0;
  double cnt_ea_work = 0.0;
  int n_tea = 0;
};

static void timing_free(msc_env* env) {
  for (hipEvent_t e : env->tev_dem) (void)hipEventDestroy(e);
  for (hipEvent_t e : env->tev_step) (void)hipEventDestroy(e);
  for (hipEvent_t e : env->tev_ea) (void)hipEventDestroy(e);
  env->tev_dem.clear();
  env->tev_step.clear();
  env->tev_ea.clear();
  env->t_cap = env->n_tdem = env->n_tstep = env->n_tea = 0;
}
// Everything a handle owns; msc_env_destroy and a failing msc_env_create both end here (members a
// partial create has not reached yet are null).
static void env_release(msc_env* env) {
  for (void* m : {env->tables, env->arena, env->scratch, (void*)env->dev, env->ea_mem, env->al_tail})
    if (m) (void)hipFree(m);
  for (hipEvent_t e : {env->ev_dem[0], env->ev_dem[1], env->ev_step[0], env->ev_step[1], env->ev_reset, env->ev_snap,
                       env->ev_chunk})
    if (e) (void)hipEventDestroy(e);
  for (int j = 0; j < MSC_EA_MAX_S; j++) {
    if (env->ev_gen[j]) (void)hipEventDestroy(env->ev_gen[j]);
    if (env->ev_cons[j]) (void)hipEventDestroy(env->ev_cons[j]);
  }
  timing_free(env);
  if (env->side) (void)hipStreamDestroy(env->side);
  if (env->ea_stream) (void)hipStreamDestroy(env->ea_stream);
  delete env;
}
// record event `i` (0 = before, 1 = after) of launch n of `v` on `st`, if timing is on
static hipError_t tmark(const msc_env* env, const std::vector<hipEvent_t>& v, int n, int i, hipStream_t st) {
  return n < env->t_cap ? hipEventRecord(v[2 * n + i], st) : hipSuccess;
}

// ---- episode-ahead demand (see msc_env) ----------------------------------------------------
// the EA stream waits for the work queued on `st` so far
static int ea_stream_wait(msc_env* env, hipStream_t st) {
  HIP_TRY(hipEventRecord(env->ev_snap, st));
  HIP_TRY(hipStreamWaitEvent(env->ea_stream, env->ev_snap, 0));
  return 0;
}
// `st` waits for the EA stream's work so far
static int wait_ea_stream(msc_env* env, hipStream_t st) {
  HIP_TRY(hipEventRecord(env->ev_snap, env->ea_stream));
  HIP_TRY(hipStreamWaitEvent(st, env->ev_snap, 0));
  return 0;
}
// one chunk [l.t0, l.t1) of a generation on the EA stream; after the last chunk the slots' ev_gen
static hipError_t ea_launch_chunk(msc_env* env, const EaLaunch& l) {
  hipStream_t es = env->ea_stream;
  const bool tm = env->n_tea < env->t_cap;
  if (tm) {
    (void)hipEventRecord(env->tev_ea[2 * env->n_tea], es);
    if ((int)env->tea_work.size() <= env->n_tea) env->tea_work.resize(env->n_tea + 1);
    env->tea_work[env->n_tea] = (double)l.nslots * (double)(l.t1 - l.t0) * (double)env->c.E;
  }
  hipError_t e = launch_demand_ea(env->c, env->dev, l, es);
  if (e != hipSuccess) return e;
  env->cnt_ea_launch++;
  env->cnt_ea_work += (double)l.nslots * (double)(l.t1 - l.t0) * (double)env->c.E;
  if (tm) (void)hipEventRecord(env->tev_ea[2 * env->n_tea++ + 1], es);
  if (l.t1 >= env->c.T) {
    for (int k = 0; k < l.nslots; k++) {
      const int slot = (l.slot0 + k) % env->c.ea_S;
      e = hipEventRecord(env->ev_gen[slot], es);
      if (e != hipSuccess) return e;
      env->gen_pending[slot] = false;
    }
  }
  return hipEventRecord(env->ev_chunk, es);
}
// launch the next chunk of the head generation if none is in flight (block: even if one is)
static hipError_t ea_pump(msc_env* env, bool block) {
  if (env->ea_q.empty()) return hipSuccess;
  if (env->ea_chunk_out && !block) {
    const hipError_t q = hipEventQuery(env->ev_chunk);
    if (q == hipErrorNotReady) return hipSuccess;
    if (q != hipSuccess) return q;
  }
  msc_env::EaItem& it = env->ea_q.front();
  EaLaunch& l = it.l;
  if (it.wait_cons >= 0) {  // a refill: after the step that read the slots' previous episodes
    const hipError_t w = hipStreamWaitEvent(env->ea_stream, env->ev_cons[it.wait_cons], 0);
    if (w != hipSuccess) return w;
    it.wait_cons = -1;
  }
  EaLaunch cl = l;
  cl.t1 = l.t0 + env->ea_chunk < env->c.T ? l.t0 + env->ea_chunk : env->c.T;
  const hipError_t e = ea_launch_chunk(env, cl);
  if (e != hipSuccess) return e;
  env->ea_chunk_out = true;
  l.t0 = cl.t1;
  if (l.t0 >= env->c.T) env->ea_q.erase(env->ea_q.begin());
  return hipSuccess;
}
// queue a generation (slots slot0 .. slot0 + nslots - 1, see EaLaunch)
static hipError_t ea_enqueue(msc_env* env, int slot0, int nslots, int from_slot, int iters0, int iters_step,
                             int wait_cons = -1) {
  env->ea_q.push_back({EaLaunch{slot0, nslots, from_slot, iters0, iters_step, 0, env->c.T}, wait_cons});
  for (int k = 0; k < nslots; k++) env->gen_pending[(slot0 + k) % env->c.ea_S] = true;
  return ea_pump(env, false);
}
// every chunk up to the generation of `slot` launched (its ev_gen is then current)
static hipError_t ea_flush_to(msc_env* env, int slot) {
  while (env->gen_pending[slot]) {
    if (env->ea_q.empty()) return hipErrorInvalidValue;  // (unreachable: pending slots are queued)
    const hipError_t e = ea_pump(env, true);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// Snapshot at a common episode start (t_sync == 0, after the reset): the SeedManager counter of
// the current episode -> slot 0's counter; episodes 1 .. S-1 follow from it, 1 .. B first (the
// envs need episode 1 when the per-step episode 0 ends), then B+1 .. S-1.
static int ea_start(msc_env* env, hipStream_t st) {
  const int S = env->c.ea_S, B = env->ea_batch;
  if (const int rc = wait_ea_stream(env, st)) return rc;  // EA work of an earlier run still reads ea_cnt
  HIP_TRY(hipMemcpyAsync(env->s.ea_cnt, env->s.counter, sizeof(int32_t) * env->c.E, hipMemcpyDeviceToDevice, st));
  if (const int rc = ea_stream_wait(env, st)) return rc;
  const int first = B < S - 1 ? B : S - 1;
  env->ea_q.clear();
  env->ea_chunk_out = false;
  for (int j = 0; j < S; j++) env->gen_pending[j] = false;
  HIP_TRY(ea_enqueue(env, 1, first, 0, 1, 1));
  if (first < S - 1) HIP_TRY(ea_enqueue(env, 1 + first, S - 1 - first, 0, 1 + first, 1));
  env->ea_freed = 0;
  env->ea_running = true;
  env->ea_n = 0;
  env->ea_cur = -1;
  return 0;
}
// The demand stream of the current EA episode into s.rng[0] (what the per-step path and
// read_state / save_state use), stream-ordered on st.
static int ea_materialize(const msc_env* env, hipStream_t st) {
  if (env->ea_running && env->ea_cur >= 0 && env->t_sync > 0)
    HIP_TRY(launch_ea_materialize(env->c, env->dev, env->ea_cur, env->t_sync, st));
  return 0;
}
static int ea_stop(msc_env* env, hipStream_t st, bool materialize) {
  if (!env->ea_running) return 0;
  if (materialize) {
    const int rc = ea_materialize(env, st);
    if (rc) return rc;
  }
  env->ea_running = false;
  env->ea_cur = -1;
  env->ea_q.clear();  // generations not launched yet are dropped (chunks in flight finish on the EA stream)
  for (int j = 0; j < MSC_EA_MAX_S; j++) env->gen_pending[j] = false;
  return 0;
}

extern "C" {

const char* msc_last_error(void) { return g_err; }
int msc_abi_version(void) { return MSC_ABI_VERSION; }

uint32_t msc_seedseq_u32(const uint32_t* words, int32_t n) { return ss_u32(words, n); }

// the one reader of the create-time MSC_* variables (parsed by env_plan.hpp)
static EnvKnobs read_env_knobs() {
  return read_env_knobs(+[](const char* name) -> const char* { return getenv(name); });
}

// Builds the handle that plan_env (env_plan.hpp) describes:
// knobs -> plan -> tables -> arena -> order buffers -> EA buffers -> descriptors -> streams and events.
int msc_env_create(const msc_env_desc* d, int device, int64_t n_envs, uint32_t base_seed, uint32_t worker_index,
                   int64_t env_index_offset, const uint32_t* env_seeds_host, msc_env** out) {
  if (!d || !out) return set_err(-1, "null argument");
  *out = nullptr;
  const EnvKnobs knobs = read_env_knobs();
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ncu = 0;
  EnvPlan p;
  if (const int rc = plan_env(d, n_envs, ncu, knobs, p)) return set_err(rc, "%s", p.err);
  EnvConst& c = p.c;
  const int64_t E = n_envs;
  const int nv = p.nv;

  HIP_TRY(hipSetDevice(device));
  msc_env* env = new msc_env();
  env->device = device;
  auto fail = [&](int rc) {
    env_release(env);
    return rc;
  };
  Packer tp(16);
  table_layout(d, p, tp);
  if (hipMalloc(&env->tables, tp.host.size()) != hipSuccess) return fail(set_err(-2, "hipMalloc(tables) failed"));
  if (hipMemcpy(env->tables, tp.host.data(), tp.host.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(set_err(-2, "copy tables failed"));
  tp.resolve(env->tables);

  EnvState s{};
  Packer ap(256);
  arena_layout(c, s, ap);
  env->arena_bytes = ap.padded();
  if (hipMalloc(&env->arena, env->arena_bytes) != hipSuccess)
    return fail(set_err(-2, "hipMalloc(state arena, %zu B) failed", env->arena_bytes));
  if (hipMemset(env->arena, 0, env->arena_bytes) != hipSuccess) return fail(set_err(-2, "memset arena failed"));
  ap.resolve(env->arena);
  if (c.demand_type == MSC_DEMAND_POISSON) {  // two per-step order buffers (s: the first; s2 below: the second)
    env->order_bytes = order_buffer_bytes(c, nv);
    if (hipMalloc(&env->scratch, 2 * env->order_bytes) != hipSuccess)
      return fail(set_err(-2, "hipMalloc(order buffers, %zu B) failed", 2 * env->order_bytes));
    s.orders = (uint4*)env->scratch;
    s.n_orders = (int32_t*)((char*)env->scratch + order_record_bytes(c, nv));
  }
  if (c.ea_S > 0) {  // the slots that fit the memory free now
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      free_b = 0;
    }
    const EaFit fit = ea_fit_slots(c, nv, p.ea_frac, (int64_t)free_b);
    c.ea_S = fit.slots;
    env->ea_budget = fit.budget;
  }
  if (c.ea_S > 0) {  // episode-ahead buffers; without the memory EA stays off
    Packer ep(256);
    ea_layout(c, nv, s, ep);
    if (hipMalloc(&env->ea_mem, ep.padded()) == hipSuccess) {
      ep.resolve(env->ea_mem);
      env->ea_bytes = (int64_t)ep.padded();
      env->ea_enabled = true;
    } else {
      (void)hipGetLastError();
      env->ea_mem = nullptr;
      c.ea_S = 0;
    }
  }
  {  // alloc_lane's tail entries, -1 until a step writes them
    const size_t bytes = sizeof(int32_t) * (size_t)((E + BS - 1) / BS);
    if (hipMalloc(&env->al_tail, bytes) != hipSuccess || hipMemset(env->al_tail, 0xff, bytes) != hipSuccess)
      return fail(set_err(-2, "hipMalloc(tail entries) failed"));
    s.al_tail = (int32_t*)env->al_tail;
  }
  EnvState s2 = s;
  if (s.orders) {
    s2.orders = (uint4*)((char*)s.orders + env->order_bytes);
    s2.n_orders = (int32_t*)((char*)s.n_orders + env->order_bytes);
  }
  // the per-step and the EA values of step_c's staging and the chain priority, both fixed here
  // (msc_env_set_episode_ahead swaps between them); a handle with EA starts with the EA pair
  const EaRun run = ea_run_settings(c, knobs);
  env->obs_stage_pe = c.obs_stage;
  env->chain_prio_pe = c.chain_prio;
  c.obs_stage = env->obs_stage_ea = run.obs_stage;
  c.chain_prio = env->chain_prio_ea = run.chain_prio;
  env->ea_batch = run.batch;
  env->ea_chunk = run.chunk;
  // root seeds: explicit, or SeedSequence([base_seed, worker_index, env_index])
  std::vector<uint32_t> roots(E);
  std::vector<int32_t> minus1(E, -1);
  for (int64_t i = 0; i < E; i++) {
    if (env_seeds_host) roots[i] = env_seeds_host[i];
    else {
      const uint64_t idx = (uint64_t)(env_index_offset + i);
      uint32_t words[4] = {base_seed, worker_index, (uint32_t)idx, (uint32_t)(idx >> 32)};
      roots[i] = ss_u32(words, (idx >> 32) ? 4 : 3);
    }
  }
  if (hipMemcpy(s.orig_root, roots.data(), sizeof(uint32_t) * E, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(s.root, roots.data(), sizeof(uint32_t) * E, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(s.emp_start, minus1.data(), sizeof(int32_t) * E, hipMemcpyHostToDevice) != hipSuccess)
    return fail(set_err(-2, "seed upload failed"));
  env->c = c;
  env->s = s;
  {
    DevEnv hd[2] = {{c, s}, {c, s2}};
    if (hipMalloc(&env->dev, 2 * sizeof(DevEnv)) != hipSuccess ||
        hipMemcpy(env->dev, hd, 2 * sizeof(DevEnv), hipMemcpyHostToDevice) != hipSuccess)
      return fail(set_err(-2, "device descriptor upload failed"));
  }
  env->pipeline = p.pipeline;
  env->ev_elide = p.ev_elide;
  if (hipStreamCreateWithFlags(&env->side, hipStreamNonBlocking) != hipSuccess)
    return fail(set_err(-2, "side stream creation failed"));
  const unsigned evf = hipEventDisableTiming | (p.ev_scope == EnvKnobs::EvScope::device   ? hipEventReleaseToDevice
                                                : p.ev_scope == EnvKnobs::EvScope::system ? 0u
                                                                                          : hipEventDisableSystemFence);
  for (int b = 0; b < 2; b++)
    if (hipEventCreateWithFlags(&env->ev_dem[b], evf) != hipSuccess ||
        hipEventCreateWithFlags(&env->ev_step[b], evf) != hipSuccess)
      return fail(set_err(-2, "event creation failed"));
  if (hipEventCreateWithFlags(&env->ev_reset, evf) != hipSuccess)
    return fail(set_err(-2, "event creation failed"));
  for (int b = 0; b < 2; b++) {  // recorded once so that every later wait is well-defined
    (void)hipEventRecord(env->ev_dem[b], env->side);
    env->ev_dem_on[b] = env->side;
    (void)hipEventRecord(env->ev_step[b], env->side);
  }
  (void)hipEventRecord(env->ev_reset, env->side);
  env->side_saw_reset = true;
  if (env->ea_enabled) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    const int ea_prio = p.ea_prio == EnvKnobs::EaPrio::low ? lo : p.ea_prio == EnvKnobs::EaPrio::high ? hi : 0;
    if (hipStreamCreateWithPriority(&env->ea_stream, hipStreamNonBlocking, ea_prio) != hipSuccess)
      return fail(set_err(-2, "EA stream creation failed"));
    for (int j = 0; j < MSC_EA_MAX_S; j++)
      if (hipEventCreateWithFlags(&env->ev_gen[j], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&env->ev_cons[j], hipEventDisableTiming) != hipSuccess)
        return fail(set_err(-2, "event creation failed"));
    if (hipEventCreateWithFlags(&env->ev_snap, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&env->ev_chunk, hipEventDisableTiming) != hipSuccess)
      return fail(set_err(-2, "event creation failed"));
    for (int j = 0; j < MSC_EA_MAX_S; j++) {
      (void)hipEventRecord(env->ev_gen[j], env->ea_stream);
      (void)hipEventRecord(env->ev_cons[j], env->ea_stream);
    }
  }
  *out = env;
  return 0;
}

void msc_env_destroy(msc_env* env) {
  if (!env) return;
  (void)hipSetDevice(env->device);
  (void)hipDeviceSynchronize();
  env_release(env);
}

int msc_env_plan(const msc_env_desc* d, int64_t n_envs, int32_t n_cus, int64_t free_bytes, int32_t* out, int32_t n) {
  if (!d || (!out && n > 0)) return set_err(-1, "null argument");
  const EnvKnobs knobs = read_env_knobs();
  EnvPlan p;
  if (const int rc = plan_env(d, n_envs, n_cus, knobs, p)) return set_err(rc, "%s", p.err);
  EnvConst& c = p.c;
  if (c.ea_S > 0 && free_bytes >= 0) c.ea_S = ea_fit_slots(c, p.nv, p.ea_frac, free_bytes).slots;
  const EaRun run = ea_run_settings(c, knobs);
  c.obs_stage = run.obs_stage;
  EnvState s{};
  Packer ap(256);
  arena_layout(c, s, ap);
  int32_t v[PLAN_N];
  plan_values(c, run, p.pipeline, ap.padded(), order_buffer_bytes(c, p.nv), v);
  const int m = n < PLAN_N ? n : PLAN_N;
  for (int i = 0; i < m; i++) out[i] = v[i];
  return m;
}

int msc_env_ea_memory(const msc_env* env, int64_t* budget_bytes, int64_t* allocated_bytes) {
  if (!env) return set_err(-1, "null env");
  if (budget_bytes) *budget_bytes = env->ea_budget;
  if (allocated_bytes) *allocated_bytes = env->ea_enabled ? env->ea_bytes : 0;
  return 0;
}

int msc_env_dims(const msc_env* env, int64_t* n_envs, int32_t* n_agents, int32_t* n_skus, int32_t* n_regions,
                 int32_t* local_obs_dim, int32_t* n_features, int32_t* max_lead, int32_t* ea_slots) {
  if (!env) return set_err(-1, "null env");
  if (n_envs) *n_envs = env->c.E;
  if (n_agents) *n_agents = env->c.W;
  if (n_skus) *n_skus = env->c.K;
  if (n_regions) *n_regions = env->c.R;
  if (local_obs_dim) *local_obs_dim = env->c.L;
  if (n_features) *n_features = env->c.F;
  if (max_lead) *max_lead = env->c.Lmax;
  if (ea_slots) *ea_slots = env->ea_enabled ? env->c.ea_S : 0;
  return 0;
}

int msc_env_kernel_choice(const msc_env* env, int32_t* out, int32_t n) {
  if (!env || (!out && n > 0)) return set_err(-1, "null argument");
  int32_t v[PLAN_N];  // the first nine of msc_env_plan's list (c.ea_S is 0 unless the EA buffers exist)
  plan_values(env->c, EaRun{env->ea_batch, env->ea_chunk, 0, 0}, env->pipeline, env->arena_bytes, env->order_bytes, v);
  const int m = n < 9 ? n : 9;
  for (int i = 0; i < m; i++) out[i] = v[i];
  return m;
}

int msc_env_reset(msc_env* env, const uint8_t* mask, const uint32_t* new_root_seeds, int32_t flags, float* obs,
                  msc_stream_t stream) {
  if (!env) return set_err(-1, "null env");
  hipStream_t st = (hipStream_t)stream;
  // episode-ahead demand stops (it restarts at the next common episode start); envs outside a
  // mask keep their episode, so their demand stream is materialised first
  if (const int rc = ea_stop(env, st, mask != nullptr)) return rc;
  // a reset re-seeds the demand streams: drop any demand generated ahead, order after the
  // side stream's last use of the state
  HIP_TRY(hipStreamWaitEvent(st, env->ev_dem[0], 0));
  HIP_TRY(hipStreamWaitEvent(st, env->ev_dem[1], 0));
  if (env->ready[0] || env->ready[1]) {
    // envs outside the mask keep their episode: rewind their demand stream to before the
    // dropped generation (rng[0][4][E] / rbuf[0][2][E] lead the arena's RNG slots)
    const int64_t E = env->c.E;
    HIP_TRY(hipMemcpyAsync(env->s.rng, env->s.rng_pre, sizeof(uint64_t) * 4 * E, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(env->s.rbuf, env->s.rbuf_pre, sizeof(uint32_t) * 2 * E, hipMemcpyDeviceToDevice, st));
  }
  env->ready[0] = env->ready[1] = false;
  env->t_sync = mask ? -1 : 0;
  HIP_TRY(launch_reset(env->c, env->dev, mask, new_root_seeds, flags, obs, st));
  HIP_TRY(hipEventRecord(env->ev_reset, st));
  env->side_saw_reset = false;
  return 0;
}

int msc_env_step(msc_env* env, const float* actions, float* obs, float* rewards, double* rewards_f64,
                 uint8_t* truncated, float* final_obs, const msc_step_info* info, msc_stream_t stream) {
  if (!env || !actions || !obs || !rewards || !truncated) return set_err(-1, "null argument");
  const EnvConst& c = env->c;
  hipStream_t st = (hipStream_t)stream;
  StepIO io{};
  io.actions = actions;
  io.obs = obs;
  io.rew = rewards;
  io.rew64 = rewards_f64;
  io.trunc = truncated;
  io.final_obs = final_obs;
  if (info) {
    io.info = *info;
    io.has_info = 1;
    const int64_t E = c.E, W = c.W, K = c.K, R = c.R;
    struct { void* p; size_t n; } z[] = {
        {info->fulfilled_per_warehouse, sizeof(int32_t) * E * W * K},
        {info->demand_per_region, sizeof(int32_t) * E * R * K},
        {info->unfulfilled_demands, sizeof(int32_t) * E * R * K},
        {info->shipment_counts, sizeof(int32_t) * E * W * R},
        {info->shipment_quantities, sizeof(int32_t) * E * W * R},
        {info->shipment_quantities_by_sku, sizeof(int32_t) * E * W * R * K},
        {info->lost_order_counts, sizeof(int32_t) * E * R},
        {info->lost_sales, sizeof(double) * E * W * K},
    };
    for (auto& q : z)
      if (q.p) HIP_TRY(hipMemsetAsync(q.p, 0, q.n, st));
  }
  const bool poisson = c.demand_type == MSC_DEMAND_POISSON;
  const int b = (int)(env->tau & 1);
  // episode-ahead demand: start at a common episode start; an episode n >= 1 reads its slot
  if (env->ea_enabled && !env->ea_paused && env->pipeline && !env->ea_running && env->t_sync == 0)
    if (const int rc = ea_start(env, st)) return rc;
  if (env->ea_running) HIP_TRY(ea_pump(env, false));
  if (env->ea_running && env->t_sync == 0) {
    env->ea_cur = env->ea_n >= 1 ? (int)(env->ea_n % c.ea_S) : -1;
    if (env->ea_cur >= 0) {
      HIP_TRY(ea_flush_to(env, env->ea_cur));
      HIP_TRY(hipStreamWaitEvent(st, env->ev_gen[env->ea_cur], 0));
    }
  }
  io.ea_slot = env->ea_running ? env->ea_cur : -1;
  io.ea_t = env->t_sync;
  const bool ea_step = io.ea_slot >= 0;
  if (poisson && !ea_step) {
    if (env->ready[b]) {
      HIP_TRY(hipStreamWaitEvent(st, env->ev_dem[b], 0));
    } else {
      HIP_TRY(tmark(env, env->tev_dem, env->n_tdem, 0, st));
      HIP_TRY(launch_demand(c, env->dev + b, st));
      env->cnt_dem_launch++;
      HIP_TRY(tmark(env, env->tev_dem, env->n_tdem++, 1, st));
      HIP_TRY(hipEventRecord(env->ev_dem[b], st));
      env->ev_dem_on[b] = st;
    }
  }
  HIP_TRY(tmark(env, env->tev_step, env->n_tstep, 0, st));
  HIP_TRY(launch_step(c, env->dev + b, io, false, st));
  env->cnt_steps++;
  HIP_TRY(tmark(env, env->tev_step, env->n_tstep++, 1, st));
  HIP_TRY(hipEventRecord(env->ev_step[b], st));
  env->ready[b] = false;
  const bool boundary = env->t_sync < 0 || env->t_sync + 1 >= c.T;
  if (env->ea_running && env->t_sync + 1 >= c.T) {
    // episode ea_n ends with this step: its slot is to be refilled with episode ea_n + S once the
    // step has read it; every ea_batch freed slots (consecutive mod S) go in one launch
    const int slot = (int)(env->ea_n % c.ea_S);
    HIP_TRY(hipEventRecord(env->ev_cons[slot], st));
    if (++env->ea_freed == env->ea_batch) {
      const int B = env->ea_batch;
      HIP_TRY(ea_enqueue(env, (slot - B + 1 + c.ea_S) % c.ea_S, B, -1, c.ea_S, 0, slot));
      env->ea_freed = 0;
    }
    env->ea_n++;
  }
  if (env->pipeline && !boundary && !ea_step) {
    // demand of step tau+1 into the other buffer, concurrently with this step kernel; that buffer
    // was last read by step tau-1, and the demand stream was last advanced by demand(tau)
    const int nb = b ^ 1;
    // (a wait already ordered by the side stream itself is not issued: each costs a barrier packet
    // the command processor retires between the demand launches, which bound a pipelined step)
    HIP_TRY(hipStreamWaitEvent(env->side, env->ev_step[nb], 0));
    if (!env->ev_elide || env->ev_dem_on[b] != env->side)
      HIP_TRY(hipStreamWaitEvent(env->side, env->ev_dem[b], 0));
    if (!env->ev_elide || !env->side_saw_reset) {
      HIP_TRY(hipStreamWaitEvent(env->side, env->ev_reset, 0));
      env->side_saw_reset = true;
    }
    HIP_TRY(tmark(env, env->tev_dem, env->n_tdem, 0, env->side));
    HIP_TRY(launch_demand(c, env->dev + nb, env->side));
    env->cnt_dem_launch++;
    HIP_TRY(tmark(env, env->tev_dem, env->n_tdem++, 1, env->side));
    HIP_TRY(hipEventRecord(env->ev_dem[nb], env->side));
    env->ev_dem_on[nb] = env->side;
    env->ready[nb] = true;
  }
  env->t_sync = env->t_sync < 0 ? -1 : (env->t_sync + 1 >= c.T ? 0 : env->t_sync + 1);
  env->tau++;
  return 0;
}

int msc_env_set_pipelining(msc_env* env, int32_t enabled) {
  if (!env) return set_err(-1, "null env");
  env->pipeline = enabled != 0 && env->c.demand_type == MSC_DEMAND_POISSON;
  if (!env->pipeline && env->ea_running) {  // back to per-step demand from the current step on
    HIP_TRY(hipSetDevice(env->device));
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = ea_stop(env, nullptr, true)) return rc;
    HIP_TRY(hipDeviceSynchronize());
  }
  return 0;
}

int msc_env_set_episode_ahead(msc_env* env, int32_t enabled) {
  if (!env) return set_err(-1, "null env");
  if (!env->ea_enabled) return 0;  // not configured at create (or no memory): nothing to switch
  const bool pause = enabled == 0;
  if (pause == env->ea_paused) return 0;
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  if (pause && env->ea_running)  // per-step demand from the current step on
    if (const int rc = ea_stop(env, nullptr, true)) return rc;
  env->ea_paused = pause;
  // the per-step path's step_c staging and chain priority (EA runs without staging, chain above the
  // generation waves); patched into both device descriptors
  env->c.obs_stage = pause ? env->obs_stage_pe : env->obs_stage_ea;
  env->c.chain_prio = pause ? env->chain_prio_pe : env->chain_prio_ea;
  for (int b = 0; b < 2; b++) {
    HIP_TRY(hipMemcpy(&env->dev[b].c.obs_stage, &env->c.obs_stage, sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(&env->dev[b].c.chain_prio, &env->c.chain_prio, sizeof(int32_t), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

int msc_env_set_chain_priority(msc_env* env, int32_t enabled) {
  if (!env) return set_err(-1, "null env");
  const int32_t v = enabled != 0 ? 1 : 0;
  env->c.chain_prio = v;
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());  // no launch in flight reads the descriptors being patched
  for (int b = 0; b < 2; b++)
    HIP_TRY(hipMemcpy(&env->dev[b].c.chain_prio, &v, sizeof v, hipMemcpyHostToDevice));
  return 0;
}

int msc_env_set_option(msc_env* env, int32_t key, int32_t value) {
  if (!env) return set_err(-1, "null env");
  if (key == MSC_OPT_STEP_C_FORM) {
    if (value != 4 && value != 5) return set_err(-1, "MSC_OPT_STEP_C_FORM must be 4 or 5");
    env->c.sc_form = value;  // (host-side launch choice: the device descriptor does not carry it)
    return 0;
  }
  if (key == MSC_OPT_ALLOC_PRIO_SPLIT) {
    if (value < 1 || value > 16) return set_err(-1, "MSC_OPT_ALLOC_PRIO_SPLIT must be in 1 .. 16");
    if (env->c.al_psplit == value) return 0;
    env->c.al_psplit = value;
    HIP_TRY(hipSetDevice(env->device));
    HIP_TRY(hipDeviceSynchronize());  // no launch in flight reads the descriptors being patched
    for (int b = 0; b < 2; b++)
      HIP_TRY(hipMemcpy(&env->dev[b].c.al_psplit, &value, sizeof value, hipMemcpyHostToDevice));
    return 0;
  }
  if (key == MSC_OPT_ALLOC_TAIL) {
    if (value != 0 && value != 1) return set_err(-1, "MSC_OPT_ALLOC_TAIL must be 0 or 1");
    if (env->c.al_tail == value) return 0;
    env->c.al_tail = value;
    HIP_TRY(hipSetDevice(env->device));
    HIP_TRY(hipDeviceSynchronize());  // no launch in flight reads the descriptors being patched
    for (int b = 0; b < 2; b++)
      HIP_TRY(hipMemcpy(&env->dev[b].c.al_tail, &value, sizeof value, hipMemcpyHostToDevice));
    return 0;
  }
  return set_err(-1, "unknown option %d", key);
}

int msc_env_alloc_tail_entry(const msc_env* env, int32_t* out, int64_t n) {
  if (!env || (!out && n > 0)) return set_err(-1, "null argument");
  const int64_t blocks = (env->c.E + BS - 1) / BS;
  const int64_t m = n < blocks ? n : blocks;
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  if (m > 0) HIP_TRY(hipMemcpy(out, env->al_tail, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
  return 0;
}

int msc_env_set_timing(msc_env* env, int32_t max_steps) {
  if (!env) return set_err(-1, "null env");
  if (max_steps < 0) return set_err(-1, "max_steps < 0");
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  timing_free(env);
  for (int i = 0; i < 2 * max_steps; i++) {
    hipEvent_t a, b, x;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventCreate(&x));
    env->tev_dem.push_back(a);
    env->tev_step.push_back(b);
    env->tev_ea.push_back(x);
  }
  env->t_cap = max_steps;
  return 0;
}

int msc_env_read_timing(msc_env* env, double* demand_ms, double* step_ms, int64_t* n_demand, int64_t* n_step) {
  if (!env) return set_err(-1, "null env");
  auto mean = [&](const std::vector<hipEvent_t>& v, int n, double* out) -> hipError_t {
    n = n < env->t_cap ? n : env->t_cap;
    double sum = 0.0;
    for (int i = 0; i < n; i++) {
      hipError_t e = hipEventSynchronize(v[2 * i + 1]);
      if (e != hipSuccess) return e;
      float ms = 0.f;
      e = hipEventElapsedTime(&ms, v[2 * i], v[2 * i + 1]);
      if (e != hipSuccess) return e;
      sum += ms;
    }
    if (out) *out = n ? sum / n : 0.0;
    return hipSuccess;
  };
  HIP_TRY(mean(env->tev_dem, env->n_tdem, demand_ms));
  HIP_TRY(mean(env->tev_step, env->n_tstep, step_ms));
  if (n_demand) *n_demand = env->n_tdem < env->t_cap ? env->n_tdem : env->t_cap;
  if (n_step) *n_step = env->n_tstep < env->t_cap ? env->n_tstep : env->t_cap;
  return 0;
}

int msc_env_read_timing_ea(msc_env* env, double* ea_ms, int64_t* n_ea, int32_t* slots, int32_t* active,
                           double* env_steps_per_launch) {
  if (!env) return set_err(-1, "null env");
  const int n = env->n_tea < env->t_cap ? env->n_tea : env->t_cap;
  double sum = 0.0, work = 0.0;
  for (int i = 0; i < n; i++) {
    HIP_TRY(hipEventSynchronize(env->tev_ea[2 * i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, env->tev_ea[2 * i], env->tev_ea[2 * i + 1]));
    sum += ms;
    work += i < (int)env->tea_work.size() ? env->tea_work[i] : 0.0;
  }
  if (ea_ms) *ea_ms = n ? sum / n : 0.0;
  if (env_steps_per_launch) *env_steps_per_launch = n ? work / n : 0.0;
  if (n_ea) *n_ea = n;
  if (slots) *slots = env->c.ea_S;
  if (active) *active = env->ea_running && env->ea_cur >= 0 ? 1 : 0;
  return 0;
}

int msc_env_work_counters(const msc_env* env, int64_t* ea_launches, double* ea_env_steps, int64_t* demand_launches,
                          int64_t* steps) {
  if (!env) return set_err(-1, "null env");
  if (ea_launches) *ea_launches = env->cnt_ea_launch;
  if (ea_env_steps) *ea_env_steps = env->cnt_ea_work;
  if (demand_launches) *demand_launches = env->cnt_dem_launch;
  if (steps) *steps = env->cnt_steps;
  return 0;
}

int msc_env_generate_demand(msc_env* env, msc_stream_t stream) {
  if (!env) return set_err(-1, "null env");
  if (env->c.demand_type != MSC_DEMAND_POISSON) return 0;
  // the next step reads an episode-ahead slot: nothing to generate
  if (env->ea_running && (env->t_sync == 0 ? env->ea_n >= 1 : env->ea_cur >= 0)) return 0;
  const int b = (int)(env->tau & 1);
  if (env->ready[b]) return 0;  // already generated ahead
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipStreamWaitEvent(st, env->ev_step[b], 0));     // last reader of buffer b
  HIP_TRY(hipStreamWaitEvent(st, env->ev_dem[b ^ 1], 0));  // last advance of the demand streams
  HIP_TRY(hipStreamWaitEvent(st, env->ev_reset, 0));
  HIP_TRY(launch_demand(env->c, env->dev + b, st));
  env->cnt_dem_launch++;
  HIP_TRY(hipEventRecord(env->ev_dem[b], st));
  env->ev_dem_on[b] = st;
  env->ready[b] = true;
  return 0;
}

int msc_env_obs_flat(const msc_env* env, const float* obs, float* flat, msc_stream_t stream) {
  if (!env || !obs || !flat) return set_err(-1, "null argument");
  HIP_TRY(launch_obs_flat(env->c, obs, flat, (hipStream_t)stream));
  return 0;
}

int msc_env_read_state(const msc_env* env, int32_t* inv, int32_t* ts, int32_t* ep, uint64_t* rng) {
  if (!env) return set_err(-1, "null env");
  const int64_t E = env->c.E, WK = (int64_t)env->c.W * env->c.K;
  HIP_TRY(hipDeviceSynchronize());
  if (rng && env->ea_running && env->ea_cur >= 0 && env->t_sync > 0) {
    if (const int rc = ea_materialize(env, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
  }
  if (inv) {
    std::vector<int32_t> soa(WK * E);
    HIP_TRY(hipMemcpy(soa.data(), env->s.inv, sizeof(int32_t) * WK * E, hipMemcpyDeviceToHost));
    for (int64_t e = 0; e < E; e++)
      for (int64_t i = 0; i < WK; i++) inv[e * WK + i] = soa[i * E + e];
  }
  if (ts) HIP_TRY(hipMemcpy(ts, env->s.t, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
  if (ep) HIP_TRY(hipMemcpy(ep, env->s.counter, sizeof(int32_t) * E, hipMemcpyDeviceToHost));
  if (rng) {
    std::vector<uint64_t> r(8 * E);
    std::vector<uint32_t> b(4 * E);
    HIP_TRY(hipMemcpy(r.data(), env->s.rng, sizeof(uint64_t) * 8 * E, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b.data(), env->s.rbuf, sizeof(uint32_t) * 4 * E, hipMemcpyDeviceToHost));
    if (env->ready[env->tau & 1]) {
      // the next step's demand is already generated: report the demand stream as of before it
      HIP_TRY(hipMemcpy(r.data(), env->s.rng_pre, sizeof(uint64_t) * 4 * E, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(b.data(), env->s.rbuf_pre, sizeof(uint32_t) * 2 * E, hipMemcpyDeviceToHost));
    }
    for (int64_t e = 0; e < E; e++)
      for (int k = 0; k < 2; k++) {
        for (int j = 0; j < 4; j++) rng[(e * 2 + k) * 6 + j] = r[(k * 4 + j) * E + e];
        rng[(e * 2 + k) * 6 + 4] = b[(k * 2 + 0) * E + e];
        rng[(e * 2 + k) * 6 + 5] = b[(k * 2 + 1) * E + e];
      }
  }
  return 0;
}

// Checkpoint blob: {magic, pending, t_sync, reserved} | state arena | [order buffer of the next
// step when its demand was already generated ahead (its RNG draws are then already consumed)].
struct StateHeader {
  uint32_t magic, pending;
  int32_t t_sync, reserved;
};
constexpr uint32_t STATE_MAGIC = 0x4d534331u;  // "MSC1"

int64_t msc_env_state_bytes(const msc_env* env) {
  return env ? (int64_t)(sizeof(StateHeader) + env->arena_bytes + env->order_bytes) : -1;
}

int msc_env_save_state(const msc_env* env, void* buf) {
  if (!env || !buf) return set_err(-1, "null argument");
  HIP_TRY(hipDeviceSynchronize());
  if (env->ea_running && env->ea_cur >= 0 && env->t_sync > 0) {  // the blob carries the demand stream
    if (const int rc = ea_materialize(env, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
  }
  const int b = (int)(env->tau & 1);
  StateHeader h{STATE_MAGIC, env->ready[b] ? 1u : 0u, env->t_sync, 0};
  memcpy(buf, &h, sizeof h);
  char* p = (char*)buf + sizeof h;
  HIP_TRY(hipMemcpy(p, env->arena, env->arena_bytes, hipMemcpyDeviceToHost));
  if (h.pending)
    HIP_TRY(hipMemcpy(p + env->arena_bytes, (char*)env->scratch + b * env->order_bytes, env->order_bytes,
                      hipMemcpyDeviceToHost));
  return 0;
}

int msc_env_load_state(msc_env* env, const void* buf) {
  if (!env || !buf) return set_err(-1, "null argument");
  StateHeader h;
  memcpy(&h, buf, sizeof h);
  if (h.magic != STATE_MAGIC) return set_err(-1, "not a libmarlsc state blob");
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = ea_stop(env, nullptr, false)) return rc;  // restarts at the next episode start
  const char* p = (const char*)buf + sizeof h;
  HIP_TRY(hipMemcpy(env->arena, p, env->arena_bytes, hipMemcpyHostToDevice));
  const int b = (int)(env->tau & 1);
  env->ready[0] = env->ready[1] = false;
  if (h.pending) {
    HIP_TRY(hipMemcpy((char*)env->scratch + b * env->order_bytes, p + env->arena_bytes, env->order_bytes,
                      hipMemcpyHostToDevice));
    env->ready[b] = true;
    HIP_TRY(hipEventRecord(env->ev_dem[b], env->side));
    env->ev_dem_on[b] = env->side;
  }
  env->t_sync = h.t_sync;
  return 0;
}

int msc_env_check(msc_env* env) {
  if (!env) return set_err(-1, "null env");
  HIP_TRY(hipDeviceSynchronize());
  uint32_t err = 0;
  HIP_TRY(hipMemcpy(&err, env->s.err, sizeof err, hipMemcpyDeviceToHost));
  if (err & ERR_ORDER_OVERFLOW) return set_err(-3, "per-step order buffer overflow (capacity %d)", env->c.order_cap);
  return 0;
}

int msc_gae_grouped(const float* rewards, const float* values, const float* next_values, const uint8_t* terminated,
                    const uint8_t* truncated, int64_t n_seq, int32_t T, float gamma, float lam, float* advantages,
                    float* targets, int32_t n_groups, double* stats_out, msc_stream_t stream) {
  if (!rewards || !values || !advantages || n_seq < 0 || T < 0) return set_err(-1, "bad argument");
  if (n_groups < 1 || n_groups > 64 || n_seq % n_groups != 0)
    return set_err(-1, "n_groups %d must be in [1, 64] and divide n_seq %lld", n_groups, (long long)n_seq);
  HIP_TRY(launch_gae(rewards, values, next_values, terminated, truncated, n_seq, T, gamma, lam, advantages, targets,
                     n_groups, stats_out, (hipStream_t)stream));
  return 0;
}

int msc_gae(const float* rewards, const float* values, const float* next_values, const uint8_t* terminated,
            const uint8_t* truncated, int64_t n_seq, int32_t T, float gamma, float lam, float* advantages,
            float* targets, double* stats_out, msc_stream_t stream) {
  return msc_gae_grouped(rewards, values, next_values, terminated, truncated, n_seq, T, gamma, lam, advantages,
                         targets, 1, stats_out, stream);
}

int64_t msc_ppo_loss_workspace(int64_t n_rows, int32_t k) {
  return n_rows >= 1 && k >= 1 && k <= 128 ? ppo_loss_workspace_bytes(n_rows, k) : -1;
}

int msc_ppo_loss(const msc_ppo_loss_desc* desc, const float* mean, const float* log_std, const float* values,
                 const int64_t* idx, const float* actions, const float* logp_old, const float* advantages,
                 const float* value_targets, const float* mean_old, const float* log_std_old, int64_t n_rows,
                 int32_t k, float* grad_mean, float* grad_log_std, float* grad_values, float* total, double* stats,
                 void* workspace, msc_stream_t stream) {
  if (!desc) return set_err(-1, "msc_ppo_loss: null desc");
  if (n_rows <= 0 || k < 1 || k > 128)
    return set_err(-1, "msc_ppo_loss: bad shape (n_rows %lld must be >= 1, k %d in [1, 128])", (long long)n_rows, k);
  if (!mean || !log_std || !values || !actions || !logp_old || !advantages || !value_targets || !grad_mean ||
      !grad_log_std || !grad_values || !total || !stats || !workspace)
    return set_err(-1, "msc_ppo_loss: null argument");
  if (desc->use_kl && (!mean_old || !log_std_old))
    return set_err(-1, "msc_ppo_loss: use_kl needs mean_old and log_std_old");
  if (desc->log_std_rows != 0 && desc->log_std_rows != 1)
    return set_err(-1, "msc_ppo_loss: log_std_rows %d must be 1 (shared row) or 0 (per row)", desc->log_std_rows);
  PpoLossArgs a;
  a.mean = mean, a.log_std = log_std, a.values = values, a.idx = idx;
  a.actions = actions, a.logp_old = logp_old, a.advantages = advantages, a.value_targets = value_targets;
  a.mean_old = mean_old, a.log_std_old = log_std_old;
  a.grad_mean = grad_mean, a.grad_log_std = grad_log_std, a.grad_values = grad_values;
  a.n = n_rows, a.K = k, a.use_kl = desc->use_kl ? 1 : 0, a.shared = desc->log_std_rows;
  a.lo = (float)(1.0 - desc->clip_param), a.hi = (float)(1.0 + desc->clip_param);
  a.vf_clip = (float)desc->vf_clip_param, a.c_v = (float)desc->vf_loss_coeff, a.c_e = (float)desc->entropy_coeff;
  a.kl_coeff = desc->use_kl ? (float)desc->kl_coeff : 0.0f;
  a.beta = (float)desc->hysteretic_beta;
  a.inv_n = 1.0f / (float)n_rows;
  HIP_TRY(launch_ppo_loss(a, desc->accumulate_stats ? 1 : 0, total, stats, workspace, (hipStream_t)stream));
  return 0;
}

int64_t msc_ppo_loss_multi_workspace(int64_t n_rows, int32_t n_policies, int32_t k) {
  return n_rows >= 1 && n_policies >= 1 && n_policies <= PL_MAX_POLICIES && k >= 1 && k <= 128
             ? n_policies * ppo_loss_workspace_bytes(n_rows, k)
             : -1;
}

int msc_ppo_loss_multi(const msc_ppo_loss_desc* desc, const double* kl_coeffs, const float* mean, const float* log_std,
                       const float* values, const int64_t* idx, const float* actions, const float* logp_old,
                       const float* advantages, const float* value_targets, const float* mean_old,
                       const float* log_std_old, int64_t n_rows, int32_t n_policies, int32_t k, float* grad_mean,
                       float* grad_log_std, float* grad_values, float* totals, double* stats, void* workspace,
                       msc_stream_t stream) {
  if (!desc) return set_err(-1, "msc_ppo_loss_multi: null desc");
  if (n_rows <= 0 || n_policies < 1 || n_policies > PL_MAX_POLICIES || k < 1 || k > 128)
    return set_err(-1, "msc_ppo_loss_multi: bad shape (n_rows %lld must be >= 1, n_policies %d in [1, %d], k %d in [1, 128])",
                   (long long)n_rows, n_policies, PL_MAX_POLICIES, k);
  if (!mean || !log_std || !values || !actions || !logp_old || !advantages || !value_targets || !grad_mean ||
      !grad_log_std || !grad_values || !totals || !stats || !workspace)
    return set_err(-1, "msc_ppo_loss_multi: null argument");
  if (desc->use_kl && (!kl_coeffs || !mean_old || !log_std_old))
    return set_err(-1, "msc_ppo_loss_multi: use_kl needs kl_coeffs, mean_old and log_std_old");
  if (desc->log_std_rows != 0 && desc->log_std_rows != 1)
    return set_err(-1, "msc_ppo_loss_multi: log_std_rows %d must be 1 (one shared row per policy) or 0 (per row)",
                   desc->log_std_rows);
  PpoLossMultiArgs m;
  PpoLossArgs& a = m.a;
  a.mean = mean, a.log_std = log_std, a.values = values, a.idx = idx;
  a.actions = actions, a.logp_old = logp_old, a.advantages = advantages, a.value_targets = value_targets;
  a.mean_old = mean_old, a.log_std_old = log_std_old;
  a.grad_mean = grad_mean, a.grad_log_std = grad_log_std, a.grad_values = grad_values;
  a.n = n_rows, a.K = k, a.use_kl = desc->use_kl ? 1 : 0, a.shared = desc->log_std_rows;
  a.lo = (float)(1.0 - desc->clip_param), a.hi = (float)(1.0 + desc->clip_param);
  a.vf_clip = (float)desc->vf_clip_param, a.c_v = (float)desc->vf_loss_coeff, a.c_e = (float)desc->entropy_coeff;
  a.kl_coeff = 0.0f;
  a.beta = (float)desc->hysteretic_beta;
  a.inv_n = 1.0f / (float)n_rows;
  m.P = n_policies;
  for (int p = 0; p < PL_MAX_POLICIES; p++)
    m.kl_coeff[p] = desc->use_kl && p < n_policies ? (float)kl_coeffs[p] : 0.0f;
  HIP_TRY(launch_ppo_loss_multi(m, desc->accumulate_stats ? 1 : 0, totals, stats, workspace, (hipStream_t)stream));
  return 0;
}

int64_t msc_adam_clip_workspace(int32_t n_tensors, int64_t total_elems) {
  return n_tensors >= 1 && total_elems >= 0 ? adam_clip_workspace_bytes(n_tensors, total_elems) : -1;
}

int msc_adam_clip_geometry(int32_t* chunk, int32_t* table_capacity) {
  if (!chunk || !table_capacity) return set_err(-1, "msc_adam_clip_geometry: null argument");
  *chunk = adam_clip_chunk(), *table_capacity = adam_clip_table_capacity();
  return 0;
}

int msc_adam_clip_step(const msc_adam_clip_desc* desc, const msc_opt_tensor* tensors, int32_t n_tensors,
                       int32_t n_groups, double* norms_out, void* workspace, msc_stream_t stream) {
  if (!desc) return set_err(-1, "msc_adam_clip_step: null desc");
  if (!tensors || !workspace) return set_err(-1, "msc_adam_clip_step: null argument");
  if (n_tensors <= 0 || n_groups <= 0)
    return set_err(-1, "msc_adam_clip_step: n_tensors %d and n_groups %d must be >= 1", n_tensors, n_groups);
  if (desc->step < 1) return set_err(-1, "msc_adam_clip_step: step %lld must be >= 1", (long long)desc->step);
  for (int32_t i = 0; i < n_tensors; i++) {
    const msc_opt_tensor& t = tensors[i];
    if (t.n < 0) return set_err(-1, "msc_adam_clip_step: tensor %d has n = %lld", i, (long long)t.n);
    if (t.group < 0 || t.group >= n_groups)
      return set_err(-1, "msc_adam_clip_step: tensor %d: group %d outside [0, %d)", i, t.group, n_groups);
    if (t.n > 0 && (!t.p || !t.g || !t.m || !t.v))
      return set_err(-1, "msc_adam_clip_step: tensor %d: null p, g, m or v", i);
  }
  HIP_TRY(launch_adam_clip(*desc, tensors, n_tensors, n_groups, norms_out, workspace, (hipStream_t)stream));
  return 0;
}

int msc_gaussian_sample(const float* mean, const float* log_std, int32_t log_std_rows, float logstd_floor,
                        const float* eps, int64_t n_rows, int32_t k, float* actions, float* logp, float* clipped,
                        msc_stream_t stream) {
  if (!mean || !log_std || !eps || !actions || !logp || !clipped) return set_err(-1, "null argument");
  if (n_rows < 0 || k < 1 || log_std_rows < 1)
    return set_err(-1, "bad shape (n_rows %lld, k %d, log_std_rows %d)", (long long)n_rows, k, log_std_rows);
  HIP_TRY(launch_gauss_sample(mean, log_std, log_std_rows, logstd_floor, eps, n_rows, k, actions, logp, clipped,
                              (hipStream_t)stream));
  return 0;
}

int msc_poisson_draws(const uint64_t* state_host, const double* lam_host, int64_t n_lam, int64_t n,
                      int64_t* out_host, uint64_t* state_out_host) {
  if (!state_host || !lam_host || !out_host) return set_err(-1, "null argument");
  if (n_lam < 1 || n_lam > 4096 || n < 0) return set_err(-1, "bad shape (n_lam %lld, n %lld)", (long long)n_lam, (long long)n);
  std::vector<PtrsConst> pc(n_lam);
  std::vector<double> enlam(n_lam);
  for (int64_t i = 0; i < n_lam; i++) {
    if (!(lam_host[i] > 0.0 && lam_host[i] < 1e6)) return set_err(-1, "lam[%lld]=%g: must be in (0, 1e6)", (long long)i, lam_host[i]);
    pc[i] = ptrs_const_host(lam_host[i]);
    enlam[i] = exp(-lam_host[i]);
  }
  void* mem = nullptr;
  const size_t b_st = 6 * sizeof(uint64_t), b_pc = sizeof(PtrsConst) * n_lam, b_el = sizeof(double) * n_lam,
               b_out = sizeof(int64_t) * (n > 0 ? n : 1);
  if (hipMalloc(&mem, b_st + b_pc + b_el + b_out) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(-2, "hipMalloc failed");
  }
  char* m = (char*)mem;
  int rc = 0;
  if (hipMemcpy(m, state_host, b_st, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m + b_st, pc.data(), b_pc, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m + b_st + b_pc, enlam.data(), b_el, hipMemcpyHostToDevice) != hipSuccess ||
      launch_poisson_draws((uint64_t*)m, (const PtrsConst*)(m + b_st), (const double*)(m + b_st + b_pc), n_lam, n,
                           (int64_t*)(m + b_st + b_pc + b_el), 0) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess ||
      (n > 0 && hipMemcpy(out_host, m + b_st + b_pc + b_el, sizeof(int64_t) * n, hipMemcpyDeviceToHost) != hipSuccess) ||
      (state_out_host && hipMemcpy(state_out_host, m, b_st, hipMemcpyDeviceToHost) != hipSuccess))
    rc = set_err(-2, "poisson draws: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(mem);
  return rc;
}

int msc_gen_draws(const uint64_t* state_host, const uint64_t* inc_host, int32_t stride, int64_t n, uint64_t* out_host,
                  uint64_t* state_out_host) {
  if (!state_host || !inc_host || !out_host || !state_out_host) return set_err(-1, "null argument");
  if (stride != 1 && stride != 2 && stride != 3 && stride != 5 && stride != 7)
    return set_err(-1, "stride %d: must be 1, 2, 3, 5 or 7", stride);
  if (n < 0 || n > (1 << 20)) return set_err(-1, "bad draw count %lld", (long long)n);
  void* mem = nullptr;
  const size_t b_st = 2 * 64 * sizeof(uint64_t), b_out = sizeof(uint64_t) * 64 * (size_t)(n > 0 ? n : 1);
  if (hipMalloc(&mem, 3 * b_st + b_out) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(-2, "hipMalloc failed");
  }
  char* m = (char*)mem;  // state [64][2], increment [64][2], final state [64][2], draws [64][n]
  int rc = 0;
  if (hipMemcpy(m, state_host, b_st, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m + b_st, inc_host, b_st, hipMemcpyHostToDevice) != hipSuccess ||
      launch_gen_draws(stride, (const uint64_t*)m, (const uint64_t*)(m + b_st), n, (uint64_t*)(m + 3 * b_st),
                       (uint64_t*)(m + 2 * b_st), 0) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess ||
      (n > 0 && hipMemcpy(out_host, m + 3 * b_st, sizeof(uint64_t) * 64 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) ||
      hipMemcpy(state_out_host, m + 2 * b_st, b_st, hipMemcpyDeviceToHost) != hipSuccess)
    rc = set_err(-2, "generator draws: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(mem);
  return rc;
}

int msc_normal_keyed(float* out, int32_t n_steps, int64_t n_rows, int32_t row_len, int64_t row0, uint64_t seed,
                     uint64_t step0, msc_stream_t stream) {
  if (!out) return set_err(-1, "null argument");
  if (n_steps < 0 || n_rows < 0 || row_len < 1 || row0 < 0)
    return set_err(-1, "bad shape (n_steps %d, n_rows %lld, row_len %d)", n_steps, (long long)n_rows, row_len);
  HIP_TRY(launch_normal_keyed(out, n_steps, n_rows, row_len, row0, seed, step0, (hipStream_t)stream));
  return 0;
}

int64_t msc_meanstd_scratch_doubles(int64_t n_rows, int32_t n_cols) {
  return n_rows >= 1 && n_cols >= 1 ? meanstd_scratch_doubles(n_rows, n_cols) : -1;
}

int msc_meanstd_filter(const float* obs, float* out, int64_t n_rows, int32_t n_cols, const uint8_t* mask,
                       int32_t update, double* state, double* scratch, double clip, double eps,
                       msc_stream_t stream) {
  if (!obs || !out || !state || (update && !scratch)) return set_err(-1, "null argument");
  if (n_rows < 1 || n_cols < 1) return set_err(-1, "bad shape (n_rows %lld, n_cols %d)", (long long)n_rows, n_cols);
  if (!(eps >= 0.0) || !(clip >= 0.0)) return set_err(-1, "eps and clip must be >= 0");
  HIP_TRY(launch_meanstd_filter(obs, out, n_rows, n_cols, mask, update ? 1 : 0, state, scratch, clip, eps,
                                (hipStream_t)stream));
  return 0;
}

int msc_mlp3_w3_layout(int32_t out_dim) { return out_dim >= 1 && out_dim <= 32 ? (mlp3_valu_outputs(out_dim) > 0 ? 1 : 0) : -1; }

// what an MLP entry point is, for the one argument check and the one body of the ten
struct MlpEntry {
  const char* word;       // the family in the hidden-size texts ("fused" / "wide"); nullptr: the mu/sigma head's own check
  const char* one_layer;  // the entry point a call with hidden2 = 0 is sent to (nullptr: hidden2 = 0 is this one's form)
  bool b2;                // the alignment text names b2 (every signature with a second hidden layer, and its sibling's)
  int max_out;            // bound on out_dim (0: no out_dim; k is checked with the head)
  bool multi;             // group is n_policies, not pre1_group
};
static const MlpEntry MLP3{"fused", nullptr, true, 32, false}, MLP2{"fused", nullptr, false, 32, false},
    MLP_MULTI3{"fused", "msc_mlp2_relu_multi", true, 32, true}, MLP_MULTI2{"fused", nullptr, true, 32, true},
    MLP_WIDE3{"wide", "msc_mlp2_relu_wide", true, 128, false}, MLP_WIDE2{"wide", nullptr, true, 128, false},
    MLP_HEAD3{nullptr, "msc_mlp2_relu_musigma", true, 0, false}, MLP_HEAD2{nullptr, nullptr, false, 0, false};
// and what it was called with (w3p / b3: the head's whp / bh; absent arguments 0)
struct MlpCall {
  const float* x;
  int64_t n_rows;
  int32_t in_dim, hidden1, hidden2, out_dim;
  const float *w1p, *b1, *w2p, *b2, *w3p, *b3;
  float* out;
  const float* pre1;
  int32_t group;  // pre1_group, or n_policies
};

// two: a second hidden layer is expected (w2p / b2, hidden sizes of the 64..512 set); sink: where the result goes (out,
// or the epilogue that makes out optional)
static int mlp_check(const MlpEntry& e, bool two, const MlpCall& a, const void* sink) {
  if (!e.multi && a.pre1 && a.group < 1) return set_err(-1, "pre1_group %d must be >= 1", a.group);
  // the kernel reads b1 / b2 / pre1 rows as float4
  if (((uintptr_t)a.b1 | (uintptr_t)a.b2 | (uintptr_t)a.pre1 | (uintptr_t)a.w1p | (uintptr_t)a.w2p | (uintptr_t)a.w3p) & 15)
    return set_err(-1, "b1, %spre1 and the packed weights must be 16-byte aligned", e.b2 ? "b2, " : "");
  if (!a.x || !a.w1p || !a.b1 || (two && (!a.w2p || !a.b2)) || !a.w3p || !a.b3 || !sink) return set_err(-1, "null argument");
  if (e.multi) {
    if (a.group < 1 || a.group > 64) return set_err(-1, "n_policies %d must be in 1..64", a.group);
    if (a.n_rows < 0 || a.n_rows % a.group != 0)
      return set_err(-1, "n_rows %lld must be a non-negative multiple of n_policies %d", (long long)a.n_rows, a.group);
    if (mlp_blocks(a.n_rows / a.group, a.group) > 0x7fffffff)
      return set_err(-1, "n_rows %lld: too many rows for one launch", (long long)a.n_rows);
  }
  const bool rows_in = a.n_rows >= 0 && a.in_dim >= 1 && a.in_dim <= 1024;
  if (e.max_out == 0 && !rows_in) return set_err(-1, "bad shape (n_rows %lld, in_dim %d)", (long long)a.n_rows, a.in_dim);
  if (e.max_out != 0 && !(rows_in && a.out_dim >= 1 && a.out_dim <= e.max_out))
    return set_err(-1, "bad shape (n_rows %lld, in_dim %d, out_dim %d)", (long long)a.n_rows, a.in_dim, a.out_dim);
  if (e.one_layer && a.hidden2 == 0) return set_err(-1, "hidden2 must be one of {64, 128, 256, 512} (one hidden layer: %s)", e.one_layer);
  if (e.word && two && !(mlp_hidden_ok(a.hidden1) && mlp_hidden_ok(a.hidden2)))
    return set_err(-1, "hidden sizes %d, %d: the %s MLP supports [H1, H2] with H1, H2 in {64, 128, 256, 512}", a.hidden1, a.hidden2, e.word);
  if (e.word && !two && !mlp2_supported(a.hidden1))
    return set_err(-1, "hidden size %d: the %s MLP supports multiples of 32 up to 1024", a.hidden1, e.word);
  return 0;
}

// need_valu: the family samples only on the VALU output layer; n_policies > 0: one log_std row, or one per policy
static int mlp_sample_args(const msc_gaussian_epilogue* g, int out_dim, bool need_valu, int n_policies, MlpSample* sm) {
  if (!g) return 0;
  if (!g->log_std || !g->eps || !g->actions || !g->logp || !g->clipped) return set_err(-1, "null sampling buffer");
  if (g->log_std_rows < 1) return set_err(-1, "log_std_rows %d must be >= 1", g->log_std_rows);
  if (need_valu && mlp3_valu_outputs(out_dim) == 0)
    return set_err(-1, "sampling epilogue needs the VALU output layer (out_dim %d <= 8)", out_dim);
  if (n_policies > 0 && g->log_std_rows != 1 && g->log_std_rows != n_policies)
    return set_err(-1, "log_std_rows %d must be 1 or n_policies %d", g->log_std_rows, n_policies);
  *sm = MlpSample{g->log_std, g->log_std_rows, g->logstd_floor, g->eps, g->actions, g->logp, g->clipped};
  return 0;
}

// the plain, per-agent (mlp_multi.hip) and wide-output (mlp_wide.hip: the centralised actor, cppo.py, multi-tile MFMA
// output layer with an LDS-staged sampling epilogue) entry points: check, sampling epilogue, launch
static int mlp_impl(const MlpEntry& e, bool two, const MlpCall& a, const msc_gaussian_epilogue* sample, const void* sink,
                    msc_stream_t stream) {
  const bool wide = e.max_out > 32;
  if (const int r = mlp_check(e, two, a, sink)) return r;
  MlpSample sm{};
  if (const int r = mlp_sample_args(sample, a.out_dim, !wide, e.multi ? a.group : 0, &sm)) return r;
  const MlpSample* smp = sample ? &sm : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  const int grp = a.pre1 ? a.group : 1;
  if (e.multi && two)
    HIP_TRY(launch_mlp3_relu_multi(a.x, a.n_rows / a.group, a.group, a.in_dim, a.hidden1, a.hidden2, a.out_dim, a.w1p, a.b1,
                                   a.w2p, a.b2, a.w3p, a.b3, a.out, a.pre1, st, smp));
  else if (e.multi)
    HIP_TRY(launch_mlp2_relu_multi(a.x, a.n_rows / a.group, a.group, a.in_dim, a.hidden1, a.out_dim, a.w1p, a.b1, a.w3p,
                                   a.b3, a.out, a.pre1, st, smp));
  else if (wide && two)
    HIP_TRY(launch_mlp3_wide(a.x, a.n_rows, a.in_dim, a.hidden1, a.hidden2, a.out_dim, a.w1p, a.b1, a.w2p, a.b2, a.w3p, a.b3,
                             a.out, a.pre1, grp, st, smp));
  else if (wide)
    HIP_TRY(launch_mlp2_wide(a.x, a.n_rows, a.in_dim, a.hidden1, a.out_dim, a.w1p, a.b1, a.w3p, a.b3, a.out, a.pre1, grp, st, smp));
  else if (two)
    HIP_TRY(launch_mlp3_relu(a.x, a.n_rows, a.in_dim, a.hidden1, a.hidden2, a.out_dim, a.w1p, a.b1, a.w2p, a.b2, a.w3p, a.b3,
                             a.out, a.pre1, grp, st, smp));
  else
    HIP_TRY(launch_mlp2_relu(a.x, a.n_rows, a.in_dim, a.hidden1, a.out_dim, a.w1p, a.b1, a.w3p, a.b3, a.out, a.pre1, grp, st, smp));
  return 0;
}

int msc_mlp3_relu_forward(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                          int32_t out_dim, const float* w1p, const float* b1, const float* w2p, const float* b2,
                          const float* w3p, const float* b3, float* out, const float* pre1, int32_t pre1_group,
                          msc_stream_t stream) {
  return mlp_impl(MLP3, true, {x, n_rows, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w3p, b3, out, pre1, pre1_group},
                  nullptr, out, stream);
}

int msc_mlp3_relu_forward_sampled(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                                  int32_t out_dim, const float* w1p, const float* b1, const float* w2p,
                                  const float* b2, const float* w3p, const float* b3, float* out,
                                  const float* pre1, int32_t pre1_group, const msc_gaussian_epilogue* sample,
                                  msc_stream_t stream) {
  return mlp_impl(MLP3, true, {x, n_rows, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w3p, b3, out, pre1, pre1_group},
                  sample, sample, stream);
}

int msc_mlp2_relu_forward(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t out_dim,
                          const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                          const float* pre1, int32_t pre1_group, msc_stream_t stream) {
  return mlp_impl(MLP2, false, {x, n_rows, in_dim, hidden, 0, out_dim, w1p, b1, nullptr, nullptr, w3p, b3, out, pre1, pre1_group},
                  nullptr, out, stream);
}

int msc_mlp2_relu_forward_sampled(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t out_dim,
                                  const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                                  const float* pre1, int32_t pre1_group, const msc_gaussian_epilogue* sample,
                                  msc_stream_t stream) {
  return mlp_impl(MLP2, false, {x, n_rows, in_dim, hidden, 0, out_dim, w1p, b1, nullptr, nullptr, w3p, b3, out, pre1, pre1_group},
                  sample, sample, stream);
}

// hidden2 = 0 is the one-hidden-layer form, reached through the msc_mlp2_* entry point
int msc_mlp3_relu_multi(const float* x, int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1,
                        int32_t hidden2, int32_t out_dim, const float* w1p, const float* b1, const float* w2p,
                        const float* b2, const float* w3p, const float* b3, float* out, const float* pre1,
                        const msc_gaussian_epilogue* sample, msc_stream_t stream) {
  return mlp_impl(MLP_MULTI3, hidden2 != 0,
                  {x, n_rows, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w3p, b3, out, pre1, n_policies}, sample,
                  out ? (const void*)out : sample, stream);
}

int msc_mlp2_relu_multi(const float* x, int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden,
                        int32_t out_dim, const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                        const float* pre1, const msc_gaussian_epilogue* sample, msc_stream_t stream) {
  return mlp_impl(MLP_MULTI2, false,
                  {x, n_rows, in_dim, hidden, 0, out_dim, w1p, b1, nullptr, nullptr, w3p, b3, out, pre1, n_policies}, sample,
                  out ? (const void*)out : sample, stream);
}

int msc_mlp_wide_supported(int32_t hidden1, int32_t hidden2, int32_t out_dim) {
  return mlp_wide_supported(hidden1, hidden2, out_dim) ? 1 : 0;
}

int msc_mlp3_relu_wide(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                       int32_t out_dim, const float* w1p, const float* b1, const float* w2p, const float* b2,
                       const float* w3p, const float* b3, float* out, const float* pre1, int32_t pre1_group,
                       const msc_gaussian_epilogue* sample, msc_stream_t stream) {
  return mlp_impl(MLP_WIDE3, hidden2 != 0,
                  {x, n_rows, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w3p, b3, out, pre1, pre1_group}, sample,
                  out ? (const void*)out : sample, stream);
}

int msc_mlp2_relu_wide(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t out_dim,
                       const float* w1p, const float* b1, const float* w3p, const float* b3, float* out,
                       const float* pre1, int32_t pre1_group, const msc_gaussian_epilogue* sample,
                       msc_stream_t stream) {
  return mlp_impl(MLP_WIDE2, false,
                  {x, n_rows, in_dim, hidden, 0, out_dim, w1p, b1, nullptr, nullptr, w3p, b3, out, pre1, pre1_group}, sample,
                  out ? (const void*)out : sample, stream);
}

// replaces the centralised wrapper's sum(rewards.values()) (src/environment/envs/single_env.py:156)
int msc_reward_team_sum(const double* rewards, int64_t n_envs, int32_t n_agents, float* out32, double* out64,
                        msc_stream_t stream) {
  if (!rewards || (!out32 && !out64)) return set_err(-1, "null argument");
  if (n_envs < 0 || n_agents < 1) return set_err(-1, "bad shape (n_envs %lld, n_agents %d)", (long long)n_envs, n_agents);
  HIP_TRY(launch_reward_team_sum(rewards, n_envs, n_agents, out32, out64, (hipStream_t)stream));
  return 0;
}

// mu / sigma-head actors (replaces backbone -> MuSigmaHead.forward, mu_sigma_head.py:52-82, wired in
// rlmodules/base.py:434-435, and the sampling of rlmodules/base.py:480-557)
int msc_mlp_musigma_layout(int32_t hidden1, int32_t hidden2, int32_t k, int32_t* width, int32_t* stride) {
  if (!width || !stride) return set_err(-1, "null argument");
  if (k < 1 || k > 8) return set_err(-1, "k %d: the fused mu/sigma head supports 1..8 actions", k);
  const int vk = mlp_head_width(k);
  if (vk == 0) return set_err(-1, "the fused mu/sigma head needs the VALU output layer (MFMA layout forced: it cannot sample)");
  if (hidden2 == 0) {
    if (!mlp2_head_supported(hidden1, vk))
      return set_err(-1, "hidden size %d: the fused mu/sigma head supports multiples of 32 up to %d for k = %d", hidden1,
                     vk <= 4 ? 1024 : 512, k);
  } else if (!mlp3_head_supported(hidden1, hidden2)) {
    return set_err(-1, "hidden sizes %d, %d: no fused mu/sigma head (H1, H2 in {64, 128, 256, 512}; not the "
                   "MSC_MLP_P8 = 4 / 2 forms of [256, 256])", hidden1, hidden2);
  }
  *width = vk;
  *stride = mlp_head_stride(vk);
  return 0;
}

static int musigma_args(const msc_musigma_epilogue* g, int32_t hidden1, int32_t hidden2, int32_t k, MlpMuSigma* ep) {
  if (!g) return set_err(-1, "null argument");
  int32_t vk, stride;
  if (const int r = msc_mlp_musigma_layout(hidden1, hidden2, k, &vk, &stride)) return r;
  auto act_ok = [](int a) { return a >= MSC_ACT_NONE && a <= MSC_ACT_SIGMOID; };
  if (!act_ok(g->act_mu) || !act_ok(g->act_sigma))
    return set_err(-1, "activation codes %d, %d: must be MSC_ACT_* (0..5)", g->act_mu, g->act_sigma);
  if (!(g->log_std_min <= g->log_std_max)) return set_err(-1, "log_std_min must be <= log_std_max");
  const bool any_out = g->actions || g->logp || g->clipped;
  if (!g->eps && any_out) return set_err(-1, "sampling outputs given without eps");
  if (g->eps && !(g->actions && g->logp && g->clipped)) return set_err(-1, "null sampling buffer");
  if (!g->eps && !g->dist_out) return set_err(-1, "nothing to write: neither dist_out nor sampling buffers");
  *ep = MlpMuSigma{g->act_mu, g->act_sigma, g->log_std_min, g->log_std_max, g->eps, g->actions, g->logp, g->clipped,
                   g->dist_out};
  return 0;
}

int msc_mlp3_relu_musigma(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2, int32_t k,
                          const float* w1p, const float* b1, const float* w2p, const float* b2, const float* whp,
                          const float* bh, const float* pre1, int32_t pre1_group, const msc_musigma_epilogue* head,
                          msc_stream_t stream) {
  if (const int r = mlp_check(MLP_HEAD3, true, {x, n_rows, in_dim, hidden1, hidden2, 0, w1p, b1, w2p, b2, whp, bh, nullptr,
                                                pre1, pre1_group}, head))
    return r;
  MlpMuSigma ep{};
  if (const int r = musigma_args(head, hidden1, hidden2, k, &ep)) return r;
  HIP_TRY(launch_mlp3_musigma(x, n_rows, in_dim, hidden1, hidden2, k, w1p, b1, w2p, b2, whp, bh, pre1,
                              pre1 ? pre1_group : 1, (hipStream_t)stream, ep));
  return 0;
}

int msc_mlp2_relu_musigma(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t k, const float* w1p,
                          const float* b1, const float* whp, const float* bh, const float* pre1, int32_t pre1_group,
                          const msc_musigma_epilogue* head, msc_stream_t stream) {
  if (const int r = mlp_check(MLP_HEAD2, false, {x, n_rows, in_dim, hidden, 0, 0, w1p, b1, nullptr, nullptr, whp, bh, nullptr,
                                                 pre1, pre1_group}, head))
    return r;
  MlpMuSigma ep{};
  if (const int r = musigma_args(head, hidden, 0, k, &ep)) return r;
  HIP_TRY(launch_mlp2_musigma(x, n_rows, in_dim, hidden, k, w1p, b1, whp, bh, pre1, pre1 ? pre1_group : 1,
                              (hipStream_t)stream, ep));
  return 0;
}

// what the launchers would pick, through their own dispatch with a recording callable (mlp_dispatch.hpp)
int msc_mlp_plan(int32_t family, int32_t hidden1, int32_t hidden2, int32_t out_dim, int64_t n_rows, int32_t n_policies,
                 int32_t* out, int32_t n) {
  if (!out && n > 0) return set_err(-1, "null argument");
  if (family < MSC_MLP_RELU || family > MSC_MLP_WIDE) return set_err(-1, "family %d: must be MSC_MLP_* (0..3)", family);
  const int np = family == MSC_MLP_MULTI ? n_policies : 1;
  if (np < 1 || np > 64) return set_err(-1, "n_policies %d must be in 1..64", np);
  if (n_rows < 0 || n_rows % np != 0)
    return set_err(-1, "n_rows %lld must be a non-negative multiple of n_policies %d", (long long)n_rows, np);
  MlpPlan p{};
  const bool ok = family == MSC_MLP_MUSIGMA ? mlp_musigma_plan(hidden1, hidden2, out_dim, n_rows, &p)
                  : family == MSC_MLP_WIDE  ? mlp_wide_plan(hidden1, hidden2, out_dim, n_rows, &p)
                                            : mlp_relu_plan(hidden1, hidden2, out_dim, n_rows / np,
                                                            family == MSC_MLP_MULTI ? np : 0, &p);
  if (!ok) p = MlpPlan{};
  const int32_t v[MSC_MLP_PLAN_N] = {ok, p.nt1, p.nt2, p.p, p.wpe, p.il, p.width, p.tb, (int32_t)p.lds, (int32_t)p.grid};
  const int m = n < MSC_MLP_PLAN_N ? n : MSC_MLP_PLAN_N;
  for (int i = 0; i < m; i++) out[i] = v[i];
  return m;
}

// the parameter gradients of the plain fused MLPs (mlp_backward.hip; replaces torch autograd through
// MLPArchitecture.build's module inside PPOTorchLearner.compute_gradients). The shape rules are the forward entry
// points', through their argument check: w3 stands where they take w3p and d_out where they take b3.
static const MlpEntry MLP_BWD{"fused", nullptr, true, 32, false};

int64_t msc_mlp_relu_backward_workspace(int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2, int32_t out_dim) {
  const bool hidden = hidden2 != 0 ? mlp_hidden_ok(hidden1) && mlp_hidden_ok(hidden2) : mlp2_supported(hidden1);
  if (n_rows < 0 || in_dim < 1 || in_dim > 1024 || out_dim < 1 || out_dim > 32 || !hidden) return -1;
  return mlp_backward_workspace_bytes(n_rows, in_dim, hidden1, hidden2, out_dim);
}

int msc_mlp_relu_backward(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden1, int32_t hidden2, int32_t out_dim,
                          const float* w1p, const float* b1, const float* w2p, const float* b2, const float* w2tp,
                          const float* w3, const float* d_out, float scale, int32_t accumulate, float* g_w1, float* g_b1,
                          float* g_w2, float* g_b2, float* g_w3, float* g_b3, void* workspace, msc_stream_t stream) {
  const bool two = hidden2 != 0;
  if (const int r = mlp_check(MLP_BWD, two, {x, n_rows, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w3, d_out,
                                             nullptr, nullptr, 1}, g_w1))
    return r;
  if (!g_b1 || !g_w3 || !g_b3 || (two && (!w2tp || !g_w2 || !g_b2)) || (n_rows > 0 && !workspace))
    return set_err(-1, "null argument");
  if (((uintptr_t)w2tp | (uintptr_t)workspace) & 15) return set_err(-1, "w2tp and the workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int HL = two ? hidden2 : hidden1;
  if (n_rows == 0) {  // the sum over no rows: zeros, or nothing to add; x is not read
    if (accumulate) return 0;
    HIP_TRY(hipMemsetAsync(g_w1, 0, sizeof(float) * hidden1 * in_dim, st));
    HIP_TRY(hipMemsetAsync(g_b1, 0, sizeof(float) * hidden1, st));
    if (two) {
      HIP_TRY(hipMemsetAsync(g_w2, 0, sizeof(float) * hidden2 * hidden1, st));
      HIP_TRY(hipMemsetAsync(g_b2, 0, sizeof(float) * hidden2, st));
    }
    HIP_TRY(hipMemsetAsync(g_w3, 0, sizeof(float) * out_dim * HL, st));
    HIP_TRY(hipMemsetAsync(g_b3, 0, sizeof(float) * out_dim, st));
    return 0;
  }
  const MlpBwdArgs a{x, n_rows, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w2tp, w3, d_out, scale,
                     accumulate ? 1 : 0, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3};
  HIP_TRY(launch_mlp_backward(a, workspace, st));
  return 0;
}

// the same for the P same-shaped networks of per-agent policies in one call (rows [n_rows / P][P], stacked packs
// and outputs): per policy, bit for bit what msc_mlp_relu_backward gives for its gathered rows
static const MlpEntry MLP_BWD_MULTI{"fused", nullptr, true, 32, true};

static bool mlp_bwd_multi_shape(int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                                int32_t out_dim) {
  return n_policies >= 1 && n_policies <= 64 && n_rows >= 0 && n_rows % n_policies == 0 &&
         msc_mlp_relu_backward_workspace(n_rows / n_policies, in_dim, hidden1, hidden2, out_dim) >= 0;
}

int64_t msc_mlp_relu_backward_multi_workspace(int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1,
                                              int32_t hidden2, int32_t out_dim) {
  if (!mlp_bwd_multi_shape(n_rows, n_policies, in_dim, hidden1, hidden2, out_dim)) return -1;
  const MlpBwdMultiPlan p = mlp_backward_multi_plan(n_rows / n_policies, n_policies, in_dim, hidden1, hidden2, out_dim);
  return p.G * p.policy_bytes;
}

int msc_mlp_relu_backward_multi_plan(int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1, int32_t hidden2,
                                     int32_t out_dim, int64_t* out, int32_t n) {
  if (!out && n > 0) return set_err(-1, "null argument");
  int64_t v[MSC_MLP_BWD_MULTI_PLAN_N] = {0, 0, 0, 0, 0, 0, 0};
  if (mlp_bwd_multi_shape(n_rows, n_policies, in_dim, hidden1, hidden2, out_dim)) {
    const MlpBwdMultiPlan p = mlp_backward_multi_plan(n_rows / n_policies, n_policies, in_dim, hidden1, hidden2, out_dim);
    const int64_t w[MSC_MLP_BWD_MULTI_PLAN_N] = {1, p.G, p.groups, p.rounds, p.nslice, p.tiles, p.G * p.policy_bytes};
    for (int i = 0; i < MSC_MLP_BWD_MULTI_PLAN_N; i++) v[i] = w[i];
  }
  const int m = n < MSC_MLP_BWD_MULTI_PLAN_N ? (n < 0 ? 0 : n) : MSC_MLP_BWD_MULTI_PLAN_N;
  for (int i = 0; i < m; i++) out[i] = v[i];
  return m;
}

int msc_mlp_relu_backward_multi(const float* x, int64_t n_rows, int32_t n_policies, int32_t in_dim, int32_t hidden1,
                                int32_t hidden2, int32_t out_dim, const float* w1p, const float* b1, const float* w2p,
                                const float* b2, const float* w2tp, const float* w3, const float* d_out, float scale,
                                int32_t accumulate, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_w3,
                                float* g_b3, void* workspace, msc_stream_t stream) {
  const bool two = hidden2 != 0;
  if (const int r = mlp_check(MLP_BWD_MULTI, two, {x, n_rows, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w3, d_out,
                                                   nullptr, nullptr, n_policies}, g_w1))
    return r;
  if (!g_b1 || !g_w3 || !g_b3 || (two && (!w2tp || !g_w2 || !g_b2)) || (n_rows > 0 && !workspace))
    return set_err(-1, "null argument");
  if (((uintptr_t)w2tp | (uintptr_t)workspace) & 15) return set_err(-1, "w2tp and the workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t P = n_policies, HL = two ? hidden2 : hidden1;
  if (n_rows == 0) {  // as the single call, over the P stacked outputs
    if (accumulate) return 0;
    HIP_TRY(hipMemsetAsync(g_w1, 0, sizeof(float) * P * hidden1 * in_dim, st));
    HIP_TRY(hipMemsetAsync(g_b1, 0, sizeof(float) * P * hidden1, st));
    if (two) {
      HIP_TRY(hipMemsetAsync(g_w2, 0, sizeof(float) * P * hidden2 * hidden1, st));
      HIP_TRY(hipMemsetAsync(g_b2, 0, sizeof(float) * P * hidden2, st));
    }
    HIP_TRY(hipMemsetAsync(g_w3, 0, sizeof(float) * P * out_dim * HL, st));
    HIP_TRY(hipMemsetAsync(g_b3, 0, sizeof(float) * P * out_dim, st));
    return 0;
  }
  const MlpBwdArgs a{x, n_rows / P, in_dim, hidden1, hidden2, out_dim, w1p, b1, w2p, b2, w2tp, w3, d_out, scale,
                     accumulate ? 1 : 0, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3};
  HIP_TRY(launch_mlp_backward_multi(a, n_policies, workspace, st));
  return 0;
}

// GRU networks (replaces GRUArchitecture's gru -> output_proj as BaseRLModule._forward_gru steps it,
// architectures/gru.py:14-85, rlmodules/base.py:99-141)
int msc_gru_supported(int32_t in_dim, int32_t hidden, int32_t layers, int32_t out_dim) {
  return gru_supported(in_dim, hidden, layers, out_dim) ? 1 : 0;
}

int msc_gru_step(const float* x, int64_t n_rows, int32_t in_dim, int32_t hidden, int32_t layers, int32_t out_dim,
                 const float* h_in, const msc_gru_weights* w, int32_t act_pre, int32_t act_out, const uint8_t* reset,
                 int32_t reset_group, float* y, float* h_out, msc_stream_t stream) {
  if (!x || !h_in || !w || !y) return set_err(-1, "null argument");
  if (n_rows < 0) return set_err(-1, "n_rows %lld < 0", (long long)n_rows);
  if (!gru_supported(in_dim, hidden, layers, out_dim))
    return set_err(-1, "no fused GRU step for in_dim %d, hidden %d, layers %d, out_dim %d (hidden in {64, 128, 256}, "
                   "1 or 2 layers, in_dim <= 1024, out_dim <= 32 or a multiple of 32 up to 256)", in_dim, hidden, layers,
                   out_dim);
  if (h_out == h_in) return set_err(-1, "h_out must not be h_in (ping-pong two buffers)");
  auto act_ok = [](int a) { return a >= MSC_ACT_NONE && a <= MSC_ACT_SIGMOID; };
  if (!act_ok(act_pre) || !act_ok(act_out)) return set_err(-1, "activation codes %d, %d: must be MSC_ACT_* (0..5)", act_pre, act_out);
  if (reset && (reset_group < 1 || n_rows % reset_group != 0))
    return set_err(-1, "reset_group %d must be >= 1 and divide n_rows %lld", reset_group, (long long)n_rows);
  GruWeights gw{};
  uintptr_t al = (uintptr_t)h_in | (uintptr_t)h_out | (uintptr_t)w->wo;
  for (int l = 0; l < layers; l++) {
    if (!w->wi[l] || !w->wh[l] || !w->b[l]) return set_err(-1, "null weight buffer of layer %d", l);
    gw.wi[l] = w->wi[l], gw.wh[l] = w->wh[l], gw.b[l] = w->b[l];
    al |= (uintptr_t)w->wi[l] | (uintptr_t)w->wh[l] | (uintptr_t)w->b[l];
  }
  if (!w->wo || !w->bo) return set_err(-1, "null output-projection buffer");
  if (out_dim % 4 == 0) al |= (uintptr_t)y;  // (stored as float4)
  // the kernel reads the state, the biases and the packed weights as float4, and stores the state so
  if (al & 15) return set_err(-1, "h_in, h_out, y (out_dim a multiple of 4), the biases and the packed weights must be 16-byte aligned");
  gw.wo = w->wo, gw.bo = w->bo;
  HIP_TRY(launch_gru_step(x, n_rows, in_dim, hidden, layers, out_dim, h_in, gw, act_pre, act_out, reset,
                          reset ? reset_group : 1, y, h_out, (hipStream_t)stream));
  return 0;
}

int msc_adv_normalize_grouped(float* adv, int64_t n, int32_t n_groups, const double* stats, msc_stream_t stream) {
  if (!adv || !stats || n < 0) return set_err(-1, "bad argument");
  if (n_groups < 1 || n_groups > 64 || n % n_groups != 0)
    return set_err(-1, "n_groups %d must be in [1, 64] and divide n %lld", n_groups, (long long)n);
  HIP_TRY(launch_adv_normalize(adv, n, n_groups, stats, (hipStream_t)stream));
  return 0;
}

int msc_adv_normalize(float* adv, int64_t n, const double* stats, msc_stream_t stream) {
  return msc_adv_normalize_grouped(adv, n, 1, stats, stream);
}

int msc_env_set_episode_counters(msc_env* env, const int32_t* counters_host) {
  if (!env || !counters_host) return set_err(-1, "null argument");
  const int64_t E = env->c.E;
  for (int64_t i = 0; i < E; i++)
    if (counters_host[i] < 0) return set_err(-1, "episode counter %d of env %lld is negative", counters_host[i], (long long)i);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  // episodes generated ahead assumed the old counters: stop (restarts at the next episode start)
  if (const int rc = ea_stop(env, nullptr, true)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(env->s.counter, counters_host, sizeof(int32_t) * E, hipMemcpyHostToDevice));
  return 0;
}

}  // extern "C"

// ---- baseline policies (policy.hip) ---------------------------------------------------------
struct msc_policy {
  PolicyDev p = {};
  int device = 0;
  int64_t E = 0;
  int32_t WK = 0;
  void* mem = nullptr;  // one allocation: tables, candidate map, then the kind's own state
};

// validate the host tables of a policy of `kind` for n_cand candidates and E envs (h_max > 0: the bound on H)
static int policy_check_tables(int kind, int n_cand, int64_t E, int WK, int h_max, const double* S, const double* z,
                               const int32_t* H, const int32_t* cand) {
  if (kind == MSC_POLICY_BASE_STOCK && S)
    for (int64_t i = 0; i < (int64_t)n_cand * WK; i++)
      if (!(S[i] == S[i]) || fabs(S[i]) > 1e300) return set_err(-1, "base-stock level %lld is not finite", (long long)i);
  if (kind == MSC_POLICY_ADAPTIVE) {
    for (int i = 0; z && i < n_cand; i++)
      if (!(z[i] == z[i]) || fabs(z[i]) > 1e300) return set_err(-1, "safety factor z[%d] is not finite", i);
    for (int i = 0; H && i < n_cand; i++) {
      if (H[i] < 1) return set_err(-1, "window H[%d] = %d must be >= 1", i, H[i]);
      if (h_max > 0 && H[i] > h_max) return set_err(-1, "window H[%d] = %d exceeds h_max %d", i, H[i], h_max);
    }
  }
  for (int64_t e = 0; cand && e < E; e++)
    if (cand[e] < 0 || cand[e] >= n_cand)
      return set_err(-1, "candidate index %d of env %lld is outside [0, %d)", cand[e], (long long)e, n_cand);
  return 0;
}

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" {

int msc_policy_create(const msc_env* env, int32_t kind, int32_t n_cand, int32_t h_max, const double* S_host,
                      const double* z_host, const int32_t* H_host, const int32_t* cand_host,
                      const uint64_t* rng_state_host, msc_policy** out) {
  if (!env || !out) return set_err(-1, "null argument");
  if (kind != MSC_POLICY_BASE_STOCK && kind != MSC_POLICY_ADAPTIVE && kind != MSC_POLICY_RANDOM)
    return set_err(-1, "unknown policy kind %d", kind);
  if (env->c.action_type != MSC_ACTION_DIRECT)
    return set_err(-1, "baseline policies need the `direct` action space (action_type %d)", env->c.action_type);
  if (n_cand < 1) return set_err(-1, "n_candidates %d must be >= 1", n_cand);
  const int64_t E = env->c.E;
  const int WK = env->c.W * env->c.K;
  if (kind == MSC_POLICY_BASE_STOCK && !S_host) return set_err(-1, "base-stock policy needs S_host");
  if (kind == MSC_POLICY_ADAPTIVE && (!z_host || !H_host)) return set_err(-1, "adaptive policy needs z_host and H_host");
  if (kind == MSC_POLICY_RANDOM && !rng_state_host) return set_err(-1, "random policy needs rng_state_host");
  if (const int rc = policy_check_tables(kind, n_cand, E, WK, h_max > 0 ? h_max : 0, S_host, z_host, H_host, cand_host))
    return rc;
  int hm = 0;
  if (kind == MSC_POLICY_ADAPTIVE) {
    hm = h_max;
    if (hm <= 0)
      for (int i = 0; i < n_cand; i++) hm = H_host[i] > hm ? H_host[i] : hm;
    if ((double)hm * WK * (double)E * 4.0 > 64e9) return set_err(-1, "demand window of h_max %d is too large", hm);
  }
  const size_t oS = 0, oz = oS + up256(sizeof(double) * (size_t)n_cand * WK), oH = oz + up256(sizeof(double) * n_cand),
               oc = oH + up256(sizeof(int32_t) * n_cand), ocnt = oc + up256(sizeof(int32_t) * E),
               orng = ocnt + up256(sizeof(int32_t) * E), ohist = orng + up256(sizeof(uint64_t) * 4 * E),
               total = ohist + up256(sizeof(int32_t) * (size_t)hm * WK * E);
  HIP_TRY(hipSetDevice(env->device));
  void* mem = nullptr;
  HIP_TRY(hipMalloc(&mem, total));
  msc_policy* pol = new msc_policy();
  pol->mem = mem;
  pol->device = env->device;
  pol->E = E;
  pol->WK = WK;
  char* b = (char*)mem;
  pol->p.kind = kind;
  pol->p.n_cand = n_cand;
  pol->p.h_max = hm;
  pol->p.S = (double*)(b + oS);
  pol->p.z = (double*)(b + oz);
  pol->p.H = (int32_t*)(b + oH);
  pol->p.cand = (int32_t*)(b + oc);
  pol->p.count = (int32_t*)(b + ocnt);
  pol->p.rng = (uint64_t*)(b + orng);
  pol->p.hist = (int32_t*)(b + ohist);
  hipError_t err = hipMemset(mem, 0, total);
  if (err == hipSuccess && kind == MSC_POLICY_RANDOM) {
    std::vector<uint64_t> tr((size_t)4 * E);  // [E][4] -> [4][E]
    for (int64_t e = 0; e < E; e++)
      for (int j = 0; j < 4; j++) tr[(size_t)j * E + e] = rng_state_host[e * 4 + j];
    err = hipMemcpy(pol->p.rng, tr.data(), sizeof(uint64_t) * 4 * E, hipMemcpyHostToDevice);
  }
  if (err != hipSuccess) {
    (void)hipFree(mem);
    delete pol;
    return set_err(-2, "policy state upload: %s", hipGetErrorString(err));
  }
  if (const int rc = msc_policy_set_tables(pol, n_cand, S_host, z_host, H_host, cand_host)) {
    msc_policy_destroy(pol);
    return rc;
  }
  *out = pol;
  return 0;
}

int msc_policy_set_tables(msc_policy* pol, int32_t n_cand, const double* S_host, const double* z_host,
                          const int32_t* H_host, const int32_t* cand_host) {
  if (!pol) return set_err(-1, "null policy");
  if (n_cand != pol->p.n_cand)
    return set_err(-1, "n_candidates %d differs from the %d the policy was created with", n_cand, pol->p.n_cand);
  const int kind = pol->p.kind;
  if (const int rc = policy_check_tables(kind, n_cand, pol->E, pol->WK, pol->p.h_max, S_host, z_host, H_host, cand_host))
    return rc;
  HIP_TRY(hipSetDevice(pol->device));
  HIP_TRY(hipDeviceSynchronize());  // launches that read the old tables have finished
  if (kind == MSC_POLICY_BASE_STOCK && S_host)
    HIP_TRY(hipMemcpy((void*)pol->p.S, S_host, sizeof(double) * (size_t)n_cand * pol->WK, hipMemcpyHostToDevice));
  if (kind == MSC_POLICY_ADAPTIVE && z_host)
    HIP_TRY(hipMemcpy((void*)pol->p.z, z_host, sizeof(double) * n_cand, hipMemcpyHostToDevice));
  if (kind == MSC_POLICY_ADAPTIVE && H_host)
    HIP_TRY(hipMemcpy((void*)pol->p.H, H_host, sizeof(int32_t) * n_cand, hipMemcpyHostToDevice));
  if (cand_host) HIP_TRY(hipMemcpy((void*)pol->p.cand, cand_host, sizeof(int32_t) * pol->E, hipMemcpyHostToDevice));
  return 0;
}

int msc_policy_act(msc_policy* pol, const msc_env* env, float* actions, msc_stream_t stream) {
  if (!pol || !env || !actions) return set_err(-1, "null argument");
  if (env->c.E != pol->E || env->c.W * env->c.K != pol->WK || env->device != pol->device)
    return set_err(-1, "policy was created for another env shape or device");
  if (env->c.action_type != MSC_ACTION_DIRECT) return set_err(-1, "baseline policies need the `direct` action space");
  HIP_TRY(launch_policy_act(env->c, env->dev, pol->p, actions, (hipStream_t)stream));
  return 0;
}

void msc_policy_destroy(msc_policy* pol) {
  if (!pol) return;
  (void)hipSetDevice(pol->device);
  (void)hipDeviceSynchronize();
  if (pol->mem) (void)hipFree(pol->mem);
  delete pol;
}

}  // extern "C"
