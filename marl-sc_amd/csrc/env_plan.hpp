// env_plan.hpp -- which kernels, forms and buffers a handle gets, as pure host code: no HIP runtime
// call and no environment read happens here, so the whole choice can be read top to bottom and driven
// on a machine without a GPU (msc_env_plan). msc_env_create (capi.hip) is the builder that executes it.
//
// Decision order (each value is computed once, after everything it depends on):
//   validation -> static tables -> demand form -> allocator -> fusion -> tables in LDS -> staging -> EA
// Results are identical under every choice; the measurement notes beside each rule are the record of
// why its default is what it is.
#pragma once
#include "env.hpp"

namespace msc {

// ---- rules the launchers share with the plan ------------------------------------------------------
// uint4 words of one order record: the region and K quantities as 16-bit fields
inline int order_record_vec4(int K) { return (1 + K + 7) / 8; }
// the scan allocator: <= 8 warehouses with <= 6 SKUs (one slot per lane), 9-16 warehouses with <= 6
// SKUs (two slots above 4 SKUs)
inline bool alloc_scan_supported(int W, int K) { return W <= 16 && K <= 6; }
// phase C fused into the scan allocator: one slot per lane (<= 8 warehouses), pending rings of at
// most SC_FC_RING slots
constexpr int SC_FC_RING = 4;  // pending-ring slots staged (lead times <= 3)
inline bool alloc_scan_fuse_supported(int W, int K, int RING) { return W <= 8 && K <= 6 && RING <= SC_FC_RING; }
// step_b_kernel's lane-group width: the power of two that holds the warehouses, or the wider sb_gw
// (the validated MSC_SB_GW: wider lane groups, fewer envs per wave)
inline int step_b_group_width(int W, int sb_gw) {
  const int gw = W <= 2 ? 2 : W <= 4 ? 4 : W <= 8 ? 8 : W <= 16 ? 16 : 32;
  return sb_gw > gw ? sb_gw : gw;
}

}  // namespace msc

#if !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <optional>
#include <string>
#include <utility>
#include <vector>

namespace msc {

// ---- the create-time environment variables, each parsed once (empty: unset) -----------------------
struct EnvKnobs {
  using Int = std::optional<int>;
  enum class Alloc { unset, lane, group, scan, other };
  enum class EvScope { nofence, device, system };
  enum class EaPrio { normal, low, high };
  std::optional<std::string> demand_impl;  // MSC_DEMAND_IMPL (kept verbatim: a bad value is quoted in the error)
  Alloc alloc_impl = Alloc::unset;         // MSC_ALLOC_IMPL=lane|group|scan (other: set to something else)
  Int demand_uni, obs_stage, obs_ring_reg, alloc_lpe, alloc_sort, fuse_c, fuse_a, step_c_form, al_prio_split, sc_tab,
      sb_gw, sb_tab, scan_defer, ea, ea_slots, ea_batch, ea_chunk, chain_prio;  // MSC_<NAME>, atoi
  std::optional<double> ea_mem_frac;       // MSC_EA_MEM_FRAC, atof
  bool pipeline = true;                    // MSC_PIPELINE=0 turns it off
  bool ev_elide = true;                    // MSC_EV_ELIDE=0: every wait is issued (A/B)
  EvScope ev_scope = EvScope::nofence;     // MSC_EV_SCOPE=system|device
  EaPrio ea_prio = EaPrio::normal;         // MSC_EA_PRIO=low|high
};

// The one reader of the create-time variables; `lookup` is the process environment (capi.hip's
// read_env_knobs()) or, in a test, any table of names.
inline EnvKnobs read_env_knobs(const char* (*lookup)(const char*)) {
  EnvKnobs k;
  auto num = [&](const char* name) { const char* v = lookup(name); return v ? EnvKnobs::Int(atoi(v)) : EnvKnobs::Int(); };
  auto is = [](const char* v, const char* want) { return v && strcmp(v, want) == 0; };
  if (const char* v = lookup("MSC_DEMAND_IMPL")) k.demand_impl = v;
  if (const char* v = lookup("MSC_ALLOC_IMPL"))
    k.alloc_impl = is(v, "group") ? EnvKnobs::Alloc::group : is(v, "lane") ? EnvKnobs::Alloc::lane
                 : is(v, "scan") ? EnvKnobs::Alloc::scan : EnvKnobs::Alloc::other;
  k.demand_uni = num("MSC_DEMAND_UNI");
  k.obs_stage = num("MSC_OBS_STAGE");
  k.obs_ring_reg = num("MSC_OBS_RING_REG");
  k.alloc_lpe = num("MSC_ALLOC_LPE");
  k.alloc_sort = num("MSC_ALLOC_SORT");
  k.fuse_c = num("MSC_FUSE_C");
  k.fuse_a = num("MSC_FUSE_A");
  k.step_c_form = num("MSC_STEP_C_FORM");
  k.al_prio_split = num("MSC_AL_PRIO_SPLIT");
  k.sc_tab = num("MSC_SC_TAB");
  k.sb_gw = num("MSC_SB_GW");
  k.sb_tab = num("MSC_SB_TAB");
  k.scan_defer = num("MSC_SCAN_DEFER");
  k.ea = num("MSC_EA");
  k.ea_slots = num("MSC_EA_SLOTS");
  k.ea_batch = num("MSC_EA_BATCH");
  k.ea_chunk = num("MSC_EA_CHUNK");
  k.chain_prio = num("MSC_CHAIN_PRIO");
  if (const char* v = lookup("MSC_EA_MEM_FRAC")) k.ea_mem_frac = atof(v);
  k.pipeline = !is(lookup("MSC_PIPELINE"), "0");
  k.ev_elide = !is(lookup("MSC_EV_ELIDE"), "0");
  const char* es = lookup("MSC_EV_SCOPE");
  k.ev_scope = is(es, "device") ? EnvKnobs::EvScope::device : is(es, "system") ? EnvKnobs::EvScope::system : EnvKnobs::EvScope::nofence;
  const char* ep = lookup("MSC_EA_PRIO");
  k.ea_prio = is(ep, "low") ? EnvKnobs::EaPrio::low : is(ep, "high") ? EnvKnobs::EaPrio::high : EnvKnobs::EaPrio::normal;
  return k;
}

// ---- the plan -----------------------------------------------------------------------------------
struct EnvPlan {
  EnvConst c{};  // every scalar of the handle's descriptor; the builder patches the table pointers
  int nv = 1;    // uint4 words per order record
  // host images of the static tables that the descriptor does not hold verbatim
  std::vector<double> hold, pen, ofT, ovT, enlam_o, p_sku, p_skip, enlam_q;
  std::vector<PtrsConst> ptrs_o, ptrs_q;
  std::vector<uint32_t> home_mask;
  std::vector<int32_t> closest, home_of, zeros_wk;
  std::vector<float> zeros_f, ones_f;
  std::vector<int64_t> toff;
  std::vector<uint4> trec;
  // host-side choices
  bool pipeline = true;  // the next step's demand on a side stream (Poisson demand, MSC_PIPELINE)
  bool ev_elide = true;
  EnvKnobs::EvScope ev_scope = EnvKnobs::EvScope::nofence;
  EnvKnobs::EaPrio ea_prio = EnvKnobs::EaPrio::normal;
  double ea_frac = 0.25;  // share of the free device memory the EA slots may take
  char err[512] = "";
  __attribute__((format(printf, 2, 3))) int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof err, fmt, ap);
    va_end(ap);
    return -1;
  }
};

inline int feature_dim(const msc_env_desc* d, int Lmax) {
  const uint32_t f = d->feature_flags;
  const int K = d->n_skus;
  int n = 0;
  if (f & MSC_F_INVENTORY) n += K + ((f & MSC_F_INVENTORY_AGG) ? 1 : 0);
  if (f & MSC_F_PIPELINE) n += Lmax * K + ((f & MSC_F_PIPELINE_AGG) ? 1 : 0);
  if (f & MSC_F_INCOMING_HOME) n += K + ((f & MSC_F_INCOMING_HOME_AGG) ? 1 : 0);
  if (f & MSC_F_SHIPPED_HOME) n += K;
  if (f & MSC_F_SHIPPED_AWAY) n += K + ((f & MSC_F_SHIPPED_AWAY_AGG) ? 1 : 0);
  if (f & MSC_F_STOCKOUT) n += K;
  if (f & MSC_F_ROLLING_MEAN) n += K + ((f & MSC_F_ROLLING_MEAN_AGG) ? 1 : 0);
  if (f & MSC_F_FORECAST) n += K + ((f & MSC_F_FORECAST_AGG) ? 1 : 0);
  if (f & MSC_F_DAYS_OF_SUPPLY) n += K;
  if (f & MSC_F_NET_POSITION) n += K;
  if (f & MSC_F_DEMAND_VARIABILITY) n += K;
  if (f & MSC_F_DEMAND_HISTORY) n += MSC_HISTORY * K;
  return n;
}

// Validates the descriptor (the reference's EnvironmentConfig shape rules, src/config/schema.py:664-890),
// derives the static tables and chooses every kernel form. n_cus < 1: 256. Returns 0, or -1 with p.err.
inline int plan_env(const msc_env_desc* d, int64_t n_envs, int n_cus, const EnvKnobs& k, EnvPlan& p) {
  if (!d) return p.fail("null argument");
  if (d->abi_version != MSC_ABI_VERSION) return p.fail("abi_version %d != %d", d->abi_version, MSC_ABI_VERSION);
  const int W = d->n_warehouses, K = d->n_skus, R = d->n_regions;
  if (W < 1 || W > MSC_MAX_W) return p.fail("n_warehouses must be in [1, %d]", MSC_MAX_W);
  if (K < 1 || K > MSC_MAX_K) return p.fail("n_skus must be in [1, %d]", MSC_MAX_K);
  if (R < 1 || R > MSC_MAX_R) return p.fail("n_regions must be in [1, %d]", MSC_MAX_R);
  if (d->episode_length < 1) return p.fail("episode_length must be positive");
  if (n_envs < 1) return p.fail("n_envs must be positive");
  if (d->max_splits < 0 || d->max_splits >= W) return p.fail("max_splits must be < n_warehouses=%d", W);
  const int WK = W * K;
  const bool poisson = d->demand_type == MSC_DEMAND_POISSON, empirical = d->demand_type == MSC_DEMAND_EMPIRICAL;

  // lead times -> pipeline horizon and pending ring size
  int Lmax = 0, lact_max = 0;
  for (int i = 0; i < WK; i++) {
    const int elt = d->expected_lead_times[i];
    if (elt < 1) return p.fail("expected_lead_times must be positive");
    int dev = 0;
    if (d->lead_type == MSC_LEAD_STOCHASTIC) dev = d->max_dev_per_sku ? d->max_deviation[i % K] : d->max_deviation[0];
    if (dev < 0) return p.fail("max_deviation must be non-negative");
    Lmax = elt > Lmax ? elt : Lmax;
    lact_max = elt + dev > lact_max ? elt + dev : lact_max;
  }
  const int RING = lact_max + 1;
  if (RING > MAX_RING) return p.fail("max actual lead time %d exceeds %d", lact_max, MAX_RING - 1);

  EnvConst& c = p.c;
  c = EnvConst{};
  c.W = W; c.K = K; c.R = R; c.T = d->episode_length; c.Lmax = Lmax; c.RING = RING;
  c.F = feature_dim(d, Lmax);
  c.L = c.F + (d->include_warehouse_id ? W : 0);
  c.action_type = d->action_type; c.lead_type = d->lead_type; c.dev_per_sku = d->max_dev_per_sku;
  c.lost_type = d->lost_type; c.scope = d->reward_scope; c.norm = d->obs_norm; c.wid = d->include_warehouse_id;
  c.num_eval = d->num_eval_episodes; c.max_wh = d->max_splits + 1; c.demand_type = d->demand_type;
  c.init_type = d->init_type; c.init_min = d->init_min; c.init_max = d->init_max;
  c.hold_per_sku = d->holding_per_sku; c.pen_per_sku = d->penalty_per_sku;
  c.flags = d->feature_flags; c.E = n_envs; c.scale = d->reward_scale; c.alpha = d->lost_alpha;
  c.hold_scalar = d->holding_per_sku ? 0.0 : d->holding_cost[0];
  c.pen_scalar = d->penalty_per_sku ? 0.0 : d->penalty_cost[0];
  if (c.lost_type == MSC_LOST_COST && !(c.alpha > 0)) return p.fail("cost lost-sales alpha must be > 0");
  if (c.norm == MSC_OBS_MEANSTD && (!d->obs_mean || !d->obs_std)) return p.fail("meanstd needs obs_mean/obs_std");
  if (d->init_type == MSC_INIT_UNIFORM && (d->init_min < 0 || d->init_min > d->init_max))
    return p.fail("uniform initial inventory needs 0 <= min <= max");

  // ---- static tables ---------------------------------------------------------------------
  p.hold.assign(K, 0.0), p.pen.assign(K, 0.0);
  for (int s = 0; s < K; s++) {
    p.hold[s] = d->holding_per_sku ? d->holding_cost[s] : 0.0;
    p.pen[s] = d->penalty_per_sku ? d->penalty_cost[s] : 0.0;
  }
  p.ofT.assign((size_t)R * W, 0.0), p.ovT.assign((size_t)R * W, 0.0);
  for (int w = 0; w < W; w++)
    for (int r = 0; r < R; r++) {
      p.ofT[(size_t)r * W + w] = d->outbound_fixed[(size_t)w * R + r];
      p.ovT[(size_t)r * W + w] = d->outbound_variable[(size_t)w * R + r];
    }
  p.home_mask.assign(R, 0u), p.closest.assign(R, 0), p.home_of.assign(W, 0);
  for (int w = 0; w < W; w++) {  // argmin over regions (first minimum), multi_env.py:144
    int b = 0;
    for (int r = 1; r < R; r++)
      if (d->distances[(size_t)w * R + r] < d->distances[(size_t)w * R + b]) b = r;
    p.home_mask[b] |= 1u << w;
    p.home_of[w] = b;
  }
  c.shared_home = 0;
  for (int r = 0; r < R; r++) c.shared_home |= __builtin_popcount(p.home_mask[r]) > 1 ? 1 : 0;
  for (int r = 0; r < R; r++) {  // argmin over warehouses, lost_sales_handler.py:36
    int b = 0;
    for (int w = 1; w < W; w++)
      if (d->distances[(size_t)w * R + r] < d->distances[(size_t)b * R + r]) b = w;
    p.closest[r] = b;
  }
  p.zeros_wk.assign(WK, 0), p.zeros_f.assign(c.F > 0 ? c.F : 1, 0.0f), p.ones_f.assign(c.F > 0 ? c.F : 1, 1.0f);
  p.enlam_o.assign(R, 1.0), p.p_sku.assign(R, 0.0), p.p_skip.assign(R, 0.0), p.enlam_q.assign((size_t)R * K, 1.0);
  p.ptrs_o.assign(R, PtrsConst{}), p.ptrs_q.assign((size_t)R * K, PtrsConst{});
  p.toff.clear(), p.trec.clear();
  const int nv = p.nv = order_record_vec4(K);
  int order_cap = 1;
  int64_t max_count = 1;  // the most orders one env can have in a step (sort buckets below)
  if (poisson) {
    double lam_sum = 0.0;
    for (int r = 0; r < R; r++) {
      const double lo = d->lambda_orders[r];
      // PositiveFloat in the reference schema (schema.py:191); >= 10 is numpy's PTRS branch
      if (!(lo > 0.0 && lo < 1e6)) return p.fail("lambda_orders[%d]=%g: must be in (0, 1e6)", r, lo);
      p.enlam_o[r] = exp(-lo);
      p.ptrs_o[r] = ptrs_const_host(lo);
      if (lo >= 10.0) c.demand_ptrs = 1;
      if (lo > 0.0 && lo < 10.0 && p.enlam_o[r] >= 1.0) return p.fail("lambda_orders[%d] too small", r);
      p.p_sku[r] = d->probability_skus[r];
      // random() draws are multiples of 2^-53: U < p <=> U < ceil53(p) <=> !(U > ceil53(p) - 2^-53)
      p.p_skip[r] = ldexp(ceil(ldexp(p.p_sku[r], 53)), -53) - 0x1p-53;
      lam_sum += lo;
      for (int s = 0; s < K; s++) {
        const double lq = d->lambda_quantity[(size_t)r * K + s];
        // quantities are stored as 16-bit record fields: rates far below 2^16
        if (!(lq > 0.0 && lq < 20000.0)) return p.fail("lambda_quantity[%d,%d]=%g: must be in (0, 20000)", r, s, lq);
        p.enlam_q[(size_t)r * K + s] = exp(-lq);
        p.ptrs_q[(size_t)r * K + s] = ptrs_const_host(lq);
        if (lq >= 10.0) c.demand_ptrs = 1;
      }
    }
    // record capacity per env and step in int64 first: the kernels index records with int32, so a
    // configuration whose per-step capacity does not fit is rejected here (rates up to 1e6 x 4,096
    // regions would otherwise wrap the cast)
    const double cap_d = ceil(lam_sum + 12.0 * sqrt(lam_sum + 1.0) + 64.0);
    if (!(cap_d <= (double)MSC_ORDER_CAP_MAX))
      return p.fail("sum of lambda_orders %g: per-step order capacity %.0f exceeds %d records per env", lam_sum, cap_d,
                    MSC_ORDER_CAP_MAX);
    max_count = order_cap = (int)cap_d;
  } else if (empirical) {
    const int rows = d->trace_n_rows;
    if (rows < d->episode_length) return p.fail("trace has %d timesteps < episode_length %d", rows, d->episode_length);
    const int64_t n_ord = d->trace_offsets[rows];
    p.toff.assign(d->trace_offsets, d->trace_offsets + rows + 1);
    p.trec.assign((size_t)(n_ord > 0 ? n_ord : 1) * nv, make_uint4(0, 0, 0, 0));
    for (int64_t j = 0; j < n_ord; j++) {
      uint16_t* h = reinterpret_cast<uint16_t*>(&p.trec[(size_t)j * nv]);
      const int reg = d->trace_regions[j];
      if (reg < 0 || reg >= R) return p.fail("trace region %d out of range", reg);
      h[0] = (uint16_t)reg;
      for (int s = 0; s < K; s++) {
        const int q = d->trace_quantities[j * K + s];
        if (q < 0 || q > 65535) return p.fail("trace quantity %d out of range", q);
        h[1 + s] = (uint16_t)q;
      }
    }
    c.tr_rows = rows;
    max_count = 0;
    for (int i = 0; i < rows; i++) max_count = std::max<int64_t>(max_count, p.toff[i + 1] - p.toff[i]);
  } else {
    return p.fail("unknown demand_type %d", d->demand_type);
  }
  c.order_cap = order_cap;

  // ---- kernel forms: A/B knobs change timing only, results are identical --------------------
  // -- demand form
  if (poisson) {
    // equal parameters in every region (and SKU): the demand parser's constant-threshold variant
    // (MSC_DEMAND_UNI=0 turns it off)
    c.demand_uni = 1;
    for (int r = 0; r < R; r++) {
      c.demand_uni &= p.enlam_o[r] == p.enlam_o[0] && p.p_skip[r] == p.p_skip[0] ? 1 : 0;
      for (int s = 0; s < K; s++) c.demand_uni &= p.enlam_q[(size_t)r * K + s] == p.enlam_q[0] ? 1 : 0;
    }
    if (k.demand_uni) c.demand_uni &= *k.demand_uni != 0 ? 1 : 0;
    c.uni_thr_o = p.enlam_o[0];
    c.uni_thr_m = p.p_skip[0];
    c.uni_thr_q = p.enlam_q[0];
  }
  // MSC_DEMAND_IMPL: "v3" (9, the default) is the short-round unit parser (demand_v3.hip) where the
  // sampler's parameters are equal in every region and SKU and the unit parser otherwise; "unit" (0)
  // forces the unit parser (C3 demand 0.787 -> 0.758 ms, C2 205 -> 208.7 M with v3,
  // profiles/r06/ab_demand_v3.txt). The forms that lost their A/Bs are gone.
  if (k.demand_impl && *k.demand_impl != "v3" && *k.demand_impl != "unit")
    return p.fail("MSC_DEMAND_IMPL=%s: accepted values are v3 (the default) and unit", k.demand_impl->c_str());
  c.demand_impl = k.demand_impl && *k.demand_impl == "unit" ? 0 : 9;

  // -- allocator (phase B); MSC_ALLOC_IMPL=lane|group|scan forces one where it is compiled
  // One env per lane (alloc_lane_kernel) when there are enough env chains to fill the chip and the
  // Poisson demand kernel of the next step runs beside it (it then needs the issue slots the lane
  // kernel leaves free: C3, 32768 envs: 0.80 vs 0.86 ms/step); otherwise the group-per-env kernel,
  // whose 8-16x more waves shorten each chain (C5, 8192 envs x 16 warehouses, empirical demand: 1.08
  // vs 1.71 ms/step). The lane allocator's instantiations stop at 16 x 8.
  using Alloc = EnvKnobs::Alloc;
  const bool lane = W <= 16 && K <= 8 &&
                    (k.alloc_impl == Alloc::lane || (k.alloc_impl != Alloc::group && poisson && n_envs >= 16384));
  // Few envs (BASELINE configs[1]: 4,096): the scan allocator (one env per wave, no data-dependent
  // loop per order) takes over from the group kernel at <= 8 warehouses and <= 6 SKUs. It also runs
  // 9-16 warehouses (MSC_ALLOC_IMPL=scan, which also overrides the lane default) but loses there: at
  // C5 (16 x 256, 8,192 envs, ~2.5 orders per region, so about one order per batch) 1.78 against 0.89
  // ms per step for the group kernel (profiles/r04/ab_c5_scan.txt). Any other explicit MSC_ALLOC_IMPL
  // keeps the group kernel, and so does MSC_ALLOC_IMPL=scan at a shape the scan allocator lacks.
  const bool scan = k.alloc_impl == Alloc::scan ? alloc_scan_supported(W, K)
                                                : !lane && k.alloc_impl == Alloc::unset && W <= 8 && alloc_scan_supported(W, K);
  c.alloc_impl = scan ? 2 : lane && k.alloc_impl != Alloc::scan ? 0 : 1;
  c.alloc_lpe = k.alloc_lpe.value_or(0);
  // Group kernel over empirical demand: a wave runs as many order iterations as its busiest env,
  // and trace order counts spread widely (C5: 200-1,000 per step), so the envs are visited in
  // descending order of this step's count (one counting-sort launch; results do not depend on
  // the order, every env is independent). MSC_ALLOC_SORT=0|1 forces it off / on. The flag follows
  // the lane-or-group choice, so it stays set where the scan allocator then takes the handle over
  // (it does not read the order).
  c.alloc_sort = !lane && (k.alloc_sort ? *k.alloc_sort != 0 : empirical) ? 1 : 0;
  c.sort_shift = 0;
  while ((max_count >> c.sort_shift) >= SORT_BUCKETS) c.sort_shift++;
  // alloc_lane's waves run above the parser of the next step's demand kernel for the first 12/16
  // of their orders, then below it: the pipelined C3 step is demand-bound with the allocation at
  // full priority (0.755 ms demand beside 0.64 ms of step kernels) and chain-bound below it (0.61
  // beside 0.86); 12/16 balanced them (341 -> 349 M agent-steps/s, profiles/r06/ab_alloc_prio.txt), and
  // 14/16 does with the shorter generator draw (361 -> 368 M, profiles/gen_draw/ab_alloc_prio.txt)
  c.al_psplit = k.al_prio_split && *k.al_prio_split >= 1 && *k.al_prio_split <= 16 ? *k.al_prio_split : 14;
  // alloc_lane's sold-out tail: on; per handle msc_env_set_option(MSC_OPT_ALLOC_TAIL, 0 | 1) (results identical)
  c.al_tail = 1;

  // -- fusion
  // Phase C inside the scan allocator (one env per wave: its obs, rewards and state updates from the
  // allocation's registers; no step_c launch) or the group allocator (step_b_phase_c). MSC_FUSE_C=0
  // keeps the step_c kernel.
  c.fuse_c = c.alloc_impl == 2 ? (alloc_scan_fuse_supported(W, K, RING) ? 1 : 0)
           : c.alloc_impl == 1 ? (K <= 8 && RING <= 4 ? 1 : 0)
                               : 0;
  if (k.fuse_c) c.fuse_c = c.fuse_c && *k.fuse_c != 0 ? 1 : 0;
  // phase A too when it has no per-env RNG work (fixed lead times; Poisson demand: the empirical
  // sampler draws its window start in phase A). MSC_FUSE_A=0 keeps the step_a kernel.
  c.fuse_a = c.alloc_impl == 2 && c.fuse_c && d->lead_type != MSC_LEAD_STOCHASTIC && poisson ? 1 : 0;
  if (k.fuse_a) c.fuse_a = c.fuse_a && *k.fuse_a != 0 ? 1 : 0;
  // scan allocator: lost-sales shares deferred to a post-pass (MSC_SCAN_DEFER=0: inline)
  c.scan_defer = k.scan_defer ? (*k.scan_defer != 0 ? 1 : 0) : 1;

  // -- cost tables in LDS
  c.sc_tab = k.sc_tab ? (*k.sc_tab != 0 ? 1 : 0) : 1;
  c.sb_gw = k.sb_gw && (*k.sb_gw == 4 || *k.sb_gw == 8 || *k.sb_gw == 16 || *k.sb_gw == 32) ? *k.sb_gw : 0;
  {
    // step_b's block tables ({of, ov} rows [2][R][W] f64 + closest [R] i32) in LDS: when small
    // (16 KB, room for the blocks of the pipelined demand kernel beside the step), or, with
    // empirical demand (no demand kernel beside the step), when the step_b blocks one CU holds at
    // this env count fit its 160 KB with them (C5, 8,192 envs x 16 warehouses: one 8-wave block per
    // CU, 32 KB of record windows + 66.5 KB of tables); otherwise each region change reads its cost
    // row from L2, and its wait also drains the record windows' LDS-DMA and the stores in flight
    const int ncu = n_cus < 1 ? 256 : n_cus;
    const int gw = step_b_group_width(W, c.sb_gw);
    // (blocks of 8 waves for 16- and 32-lane groups with the tables, else 4: step_b_waves)
    const int bw = gw >= 16 ? 8 : 4;
    const int64_t blocks = (n_envs * gw + 64 * bw - 1) / (64 * bw), per_cu = (blocks + ncu - 1) / ncu;
    const size_t tab = (size_t)2 * R * W * sizeof(double) + (size_t)R * sizeof(int32_t);
    const size_t blk = (size_t)bw * 2 * 128 * 16 + tab;  // waves x 2 windows x SB_REC records + tables
    c.sb_tab = tab <= 16 * 1024 ? 1 : (empirical && blk <= 160 * 1024 && (int64_t)blk * per_cu <= 160 * 1024) ? 1 : 0;
    if (k.sb_tab) c.sb_tab = *k.sb_tab != 0 && blk <= 160 * 1024 ? 1 : 0;
  }

  // -- step_c's observation staging and forms
  // Staged when the whole block's stage fits 80 KB of LDS (C3: 8 x 64 x 35 floats = 70 KiB), then
  // in two phases of ceil(W / 2) agents: half the LDS, so two step_c blocks fit beside the
  // pipelined demand kernel's (C3 MAPPO rollout 1.19 -> 1.14 ms per step; profiles/r03/ab_stage_phases.txt).
  // MSC_OBS_STAGE=0 | 1 | P where it fits: off / whole block / in P <= W phases of ceil(W / P) agents
  // (a P-th of the LDS). This is the per-step value; ea_run_settings() gives the one used with EA.
  c.obs_stage = (size_t)BS * ((c.W * c.L) | 1) * sizeof(float) <= 80 * 1024 ? (c.W >= 2 ? 2 : 1) : 0;
  if (k.obs_stage) c.obs_stage = c.obs_stage && *k.obs_stage > 0 ? *k.obs_stage : 0;
  if (c.obs_stage > c.W) c.obs_stage = c.W;
  // step_c with the pending ring in registers (8-wave blocks, up to 256 VGPRs): C2 (4,096 envs)
  // 152.7 -> 157.4 M agent-steps/s; at 32,768 envs the env line is unchanged and the MAPPO rollout
  // 1.165 -> 1.188 ms per step (fewer step_c blocks fit beside the demand kernel), so only below
  // the lane allocator's env count (profiles/r03/ab_ringreg.txt). MSC_OBS_RING_REG=0|1 forces it.
  c.obs_ring_reg = k.obs_ring_reg ? *k.obs_ring_reg != 0 : n_envs < 16384 ? 1 : 0;
  c.sc_form = k.step_c_form && *k.step_c_form == 4 ? 4 : 5;

  // -- episode-ahead (EA) Poisson demand, when the envs are too few to fill the chip with per-step
  // demand chains (MSC_EA=0|1 forces it off / on): the slots and capacity wanted before the free
  // memory is known (ea_fit_slots)
  c.ea_S = 0;
  if (poisson) {
    // (automatic below 8,193 envs; at 32,768 envs it wins only in steady state -- 0.81 -> 0.72 ms
    // per step once the generation pipeline is full, profiles/r04/ab_ea_c3.txt -- while the first
    // episodes pay for the bulk generation, so larger handles ask for it explicitly)
    bool want = d->episode_ahead < 0 ? n_envs <= 8192 : d->episode_ahead > 0;
    if (k.ea) want = *k.ea != 0;
    // 16 slots: the generation runs further ahead of the step (C2 over 48 episodes: 175.5 M
    // agent-steps/s at 12 slots, 180-183 M at 16; profiles/r03/ab_ea_slots.txt); 29 GB at 4,096 envs
    // (the memory budget may lower it)
    int S = 16;
    if (d->episode_ahead > 0 && d->episode_ahead < S) S = d->episode_ahead;
    if (k.ea_slots) S = *k.ea_slots;
    S = S < 2 ? 2 : (S > MSC_EA_MAX_S ? MSC_EA_MAX_S : S);
    if (want) {
      double lam_sum = 0.0, draws = 0.0;
      // expected uniforms per Poisson draw: lambda + 1 for the multiplication method, a few per
      // PTRS trial (two uniforms, acceptance > 0.5) at lambda >= 10
      auto per_draw = [](double lam) { return lam < 10.0 ? lam + 1.0 : 8.0; };
      for (int r = 0; r < R; r++) {
        const double lo = d->lambda_orders[r];
        lam_sum += lo;
        double per_order = K;  // the SKU mask's Bernoulli draws
        for (int s = 0; s < K; s++) per_order += d->probability_skus[r] * per_draw(d->lambda_quantity[(size_t)r * K + s]);
        draws += per_draw(lo) + lo * per_order;
      }
      const double m = lam_sum * d->episode_length;
      draws *= d->episode_length;
      const double cap_d = ceil(m + 12.0 * sqrt(m + 1.0) + 64.0);
      // slot record indices are int32 in the kernels and stream positions uint32: an episode whose
      // records or draws (with a 12-sigma margin) do not fit keeps per-step demand
      if (cap_d * nv <= (double)INT32_MAX && draws + 12.0 * sqrt(draws + 1.0) < 4294967295.0) {
        c.ea_S = S;
        c.ea_cap = (int64_t)cap_d;
      }
    }
  }
  p.ea_frac = k.ea_mem_frac ? *k.ea_mem_frac : d->ea_mem_fraction > 0.0 ? d->ea_mem_fraction : 0.25;

  // -- host-side choices
  p.pipeline = k.pipeline && poisson;
  p.ev_elide = k.ev_elide;
  // the pipelining events only order work between two streams of this device (no host waits on
  // them), so their records skip the system-scope fence: ~2 us less per record (tools/ev_gap.hip),
  // C2 224 -> 227 M, C3 +0.3 % (profiles/r06/ab_ev_nofence.txt). MSC_EV_SCOPE=system restores it,
  // =device records them with a device-scope release (A/B)
  p.ev_scope = k.ev_scope;
  // MSC_EA_PRIO=low|high: queue priority of the generation stream (A/B; default: normal)
  p.ea_prio = k.ea_prio;
  return 0;
}

// ---- episode-ahead steps that depend on the device ------------------------------------------------
// EA memory budget: at most ea_frac (default 0.25, MSC_EA_MEM_FRAC) of the memory free now, so the
// rollout / learner allocations that follow keep the rest; the slot count shrinks to what fits, and
// below 2 slots EA stays off. Returns the slots (<= c.ea_S) and the budget in bytes.
struct EaFit {
  int slots;
  int64_t budget;
};
inline EaFit ea_fit_slots(const EnvConst& c, int nv, double ea_frac, int64_t free_bytes) {
  const size_t T = c.T, E = c.E;
  const size_t slot_bytes = sizeof(uint4) * (size_t)nv * c.ea_cap * E + sizeof(int32_t) * (T + 1) * E +
                            sizeof(uint32_t) * T * E + sizeof(int32_t) * E;
  const double budget = ea_frac * (double)(size_t)free_bytes;
  const int64_t fit = (int64_t)(budget / (double)(slot_bytes + 1024 /* alignment slack */));
  return {fit < c.ea_S ? (fit < 2 ? 0 : (int)fit) : c.ea_S, (int64_t)budget};
}

// What a handle runs with once its buffers exist (c.ea_S final): the refill batch and chunk, and the
// values of obs_stage / chain_prio while EA is on (msc_env_set_episode_ahead swaps between these and
// the per-step values in c). Without EA: the per-step values, one slot per launch, 50-step chunks.
struct EaRun {
  int batch = 1, chunk = 50;
  int32_t obs_stage = 0, chain_prio = 0;
};
inline EaRun ea_run_settings(const EnvConst& c, const EnvKnobs& k) {
  EaRun r;
  r.obs_stage = c.obs_stage;
  r.chain_prio = c.chain_prio;
  if (c.ea_S <= 0) return r;
  const int S = c.ea_S;
  // refill batch: a batch freed by episodes n-B+1 .. n is needed S-B episodes later. A generation
  // chunk's duration is one lane's parse chain whatever the slots per launch, so the slots per
  // launch set the generation rate: at 4,096 envs 4 per launch (16,384 lanes) could not keep up
  // with the step (C2 sustained 173 M agent-steps/s over 96 episodes), 8 per launch can (207 M,
  // profiles/r05/ab_ea_batch.txt); at 32,768 envs a single slot per launch already fills the chip
  int B = c.E <= 8192 ? S / 2 : S / 4;
  B = B > 1 ? B : 1;
  if (k.ea_batch) B = *k.ea_batch;
  r.batch = B < 1 ? 1 : (B > S - 1 ? S - 1 : B);
  // step_c's observation staging (up to 80 KB of LDS per block) stalls behind a generation
  // chunk's pending blocks for the chunk's whole run (measured: 5.5 ms step_c launches right
  // after a chunk starts, none without staging): off with EA unless MSC_OBS_STAGE is set non-zero
  if (!(k.obs_stage && *k.obs_stage != 0)) r.obs_stage = 0;
  // the generation waves (parser 2, generators 1) are background work: the whole step chain
  // runs above them (the allocation kernels are at 3 already; MSC_CHAIN_PRIO=0 leaves step_a /
  // step_c at 0)
  r.chain_prio = (k.chain_prio && *k.chain_prio == 0) ? 0 : 1;
  // chunk A/B at C2 (scripts/gpu_ab_eachunk.sh, steps per launch -> M agent-steps/s): 5 -> 149.6,
  // 10 -> 152.9, 20 -> 157.8, 34 -> 165.3, 50 -> 170.1, 100 -> 171.4 (fewer launch ramps and
  // tails beside the step kernels); 50 keeps the work a synchronize may wait for at half an episode
  // at 32,768 envs whole-episode launches: 0.72 ms per step against 0.78 with 50-step chunks
  // (profiles/r04/ab_ea_c3.txt)
  int ch = c.E > 8192 ? c.T : 50;
  if (k.ea_chunk) ch = *k.ea_chunk;
  r.chunk = ch < 1 ? 1 : ch;
  return r;
}

// ---- buffer layouts -------------------------------------------------------------------------------
// Many fields in one allocation: add() reserves the next aligned range (with a source: also copies it
// into the host image) and notes the pointer that is to point there; resolve() patches every noted
// pointer once the allocation exists.
struct Packer {
  size_t align;
  size_t end = 0;          // end of the last field
  std::vector<char> host;  // host image of the fields added with a source
  std::vector<std::pair<void*, size_t>> fix;  // (address of the pointer field, offset)
  explicit Packer(size_t a) : align(a) {}
  template <class P>
  void add(P*& field, size_t bytes, const void* src = nullptr) {
    const size_t off = (end + align - 1) & ~(align - 1);
    end = off + bytes;
    if (src) {
      host.resize(end);
      memcpy(host.data() + off, src, bytes);
    }
    fix.emplace_back((void*)&field, off);
  }
  size_t padded() const { return (end + align - 1) & ~(align - 1); }
  void resolve(void* base) const {
    for (const auto& f : fix) {
      char* ptr = static_cast<char*>(base) + f.second;
      memcpy(f.first, &ptr, sizeof ptr);
    }
  }
};

// the static tables (read-only, shared by every env), 16-byte aligned
inline void table_layout(const msc_env_desc* d, EnvPlan& p, Packer& t) {
  EnvConst& c = p.c;
  const int K = c.K, R = c.R, W = c.W, WK = W * K;
  const bool stoch = d->lead_type == MSC_LEAD_STOCHASTIC, meanstd = c.norm == MSC_OBS_MEANSTD;
  t.add(c.act_param, sizeof(double) * K, d->action_param);
  t.add(c.init_vals, sizeof(int32_t) * WK, d->init_values ? d->init_values : p.zeros_wk.data());
  t.add(c.hold, sizeof(double) * K, p.hold.data());
  t.add(c.pen, sizeof(double) * K, p.pen.data());
  t.add(c.skw, sizeof(double) * K, d->sku_weights);
  t.add(c.ofT, sizeof(double) * p.ofT.size(), p.ofT.data());
  t.add(c.ovT, sizeof(double) * p.ovT.size(), p.ovT.data());
  t.add(c.inF, sizeof(double) * WK, d->inbound_fixed);
  t.add(c.inV, sizeof(double) * WK, d->inbound_variable);
  t.add(c.enlam_o, sizeof(double) * R, p.enlam_o.data());
  t.add(c.p_sku, sizeof(double) * R, p.p_sku.data());
  t.add(c.p_skip, sizeof(double) * R, p.p_skip.data());
  t.add(c.enlam_q, sizeof(double) * p.enlam_q.size(), p.enlam_q.data());
  t.add(c.ptrs_o, sizeof(PtrsConst) * p.ptrs_o.size(), p.ptrs_o.data());
  t.add(c.ptrs_q, sizeof(PtrsConst) * p.ptrs_q.size(), p.ptrs_q.data());
  t.add(c.elt, sizeof(int32_t) * WK, d->expected_lead_times);
  t.add(c.maxdev, sizeof(int32_t) * (stoch && d->max_dev_per_sku ? K : 1), stoch ? d->max_deviation : p.zeros_wk.data());
  t.add(c.home_mask, sizeof(uint32_t) * R, p.home_mask.data());
  t.add(c.closest, sizeof(int32_t) * R, p.closest.data());
  t.add(c.home_of, sizeof(int32_t) * W, p.home_of.data());
  t.add(c.obs_mean, sizeof(float) * p.zeros_f.size(), meanstd ? d->obs_mean : p.zeros_f.data());
  t.add(c.obs_std, sizeof(float) * p.ones_f.size(), meanstd ? d->obs_std : p.ones_f.data());
  if (c.demand_type == MSC_DEMAND_EMPIRICAL) {
    t.add(c.tr_off, sizeof(int64_t) * p.toff.size(), p.toff.data());
    t.add(c.tr_rec, sizeof(uint4) * p.trec.size(), p.trec.data());
  }
}

// The persistent state arena (SoA, env fastest), every field 256-byte aligned. msc_env_save_state /
// msc_env_load_state copy the arena raw, so this list -- its order, sizes and alignment -- IS the
// checkpoint format: changing it invalidates every saved state.
inline void arena_layout(const EnvConst& c, EnvState& s, Packer& a) {
  const size_t E = c.E, W = c.W, WK = (size_t)c.W * c.K, RING = c.RING;
  a.add(s.inv, sizeof(int32_t) * WK * E);
  a.add(s.ring_q, sizeof(int32_t) * WK * RING * E);
  a.add(s.ring_l, c.lead_type == MSC_LEAD_STOCHASTIC ? WK * RING * E : 1);
  a.add(s.hist, sizeof(int32_t) * MSC_HISTORY * WK * E);
  a.add(s.inc, sizeof(int32_t) * WK * E);
  a.add(s.fc, sizeof(float) * WK * E);
  a.add(s.rng, sizeof(uint64_t) * 8 * E);
  a.add(s.rbuf, sizeof(uint32_t) * 4 * E);
  a.add(s.rng_pre, sizeof(uint64_t) * 4 * E);
  a.add(s.rbuf_pre, sizeof(uint32_t) * 2 * E);
  a.add(s.t, sizeof(int32_t) * E);
  a.add(s.counter, sizeof(int32_t) * E);
  a.add(s.orig_root, sizeof(uint32_t) * E);
  a.add(s.root, sizeof(uint32_t) * E);
  a.add(s.emp_start, sizeof(int32_t) * E);
  a.add(s.perm, sizeof(int32_t) * E);
  a.add(s.err, sizeof(uint32_t) * 4);
  a.add(s.sc_sht, sizeof(int32_t) * WK * E);
  a.add(s.sc_shh, sizeof(int32_t) * WK * E);
  a.add(s.sc_pen, sizeof(double) * W * E);
  a.add(s.sc_out, sizeof(double) * W * E);
  a.add(s.sc_inb, sizeof(double) * W * E);
}

// the episode-ahead slots (c.ea_S final), every field 256-byte aligned
inline void ea_layout(const EnvConst& c, int nv, EnvState& s, Packer& a) {
  const size_t S = c.ea_S, T = c.T, E = c.E;
  a.add(s.ea_rec, sizeof(uint4) * (size_t)nv * c.ea_cap * S * E);
  a.add(s.ea_off, sizeof(int32_t) * S * (T + 1) * E);
  a.add(s.ea_pos, sizeof(uint32_t) * S * T * E);
  a.add(s.ea_cnt, sizeof(int32_t) * S * E);
}

// one per-step order buffer (Poisson demand; there are two): the records, then the counts
inline size_t order_record_bytes(const EnvConst& c, int nv) {
  return c.demand_type == MSC_DEMAND_POISSON ? sizeof(uint4) * (size_t)nv * c.order_cap * c.E : 0;
}
inline size_t order_buffer_bytes(const EnvConst& c, int nv) {
  return c.demand_type == MSC_DEMAND_POISSON ? (order_record_bytes(c, nv) + sizeof(int32_t) * c.E + 255) & ~size_t(255) : 0;
}

// ---- the plan as integers (msc_env_plan; msc_env_kernel_choice reports the first nine) --------------
constexpr int PLAN_N = 26;
inline void plan_values(const EnvConst& c, const EaRun& r, bool pipeline, size_t arena_bytes, size_t order_bytes,
                        int32_t v[PLAN_N]) {
  auto units = [](size_t bytes) { return (int32_t)std::min<size_t>(bytes / 256, INT32_MAX); };  // (saturating)
  const int32_t vals[PLAN_N] = {
      c.alloc_impl, c.alloc_sort, c.fuse_a, c.fuse_c, c.sb_tab, c.alloc_impl == 1 ? step_b_group_width(c.W, c.sb_gw) : 0,
      c.ea_S, c.demand_impl, c.demand_uni,
      c.obs_stage, c.obs_ring_reg, c.alloc_lpe, c.sort_shift, c.scan_defer, c.sc_tab, c.sc_form, c.al_psplit,
      c.demand_ptrs, c.order_cap, c.RING, (int32_t)c.ea_cap, r.batch, r.chunk, pipeline ? 1 : 0,
      units(arena_bytes), units(order_bytes)};
  for (int i = 0; i < PLAN_N; i++) v[i] = vals[i];
}

}  // namespace msc
#endif  // !__HIP_DEVICE_COMPILE__
