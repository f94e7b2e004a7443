// The simulation entry points of the C ABI.  Included by muavta_kernels.hip.
namespace {

ScoredDev scored_dev(const MuavtaScored& sp) {
  return {sp.edge_scores, sp.task_pri, (const unsigned long long*)sp.reserved, sp.selected, sp.replanned, sp.kind, sp.max_tasks, sp.max_agents, sp.gate, sp.flags};
}

// The token output pointers of one call, as the caller handed them over: muavta_tokens_device's arguments, the next-token fields of
// MuavtaRlStep, the park_ fields of MuavtaRlRun, the token rings of MuavtaRecord.
struct TokOut {
  float* task_feats; uint8_t* task_mask; int32_t* task_ids; float* agent_feats; uint8_t* agent_mask; int32_t* agent_ids; float* edge_valid;
  int32_t* n_urgent; float* expert_mask; int32_t* replanned;  // optional, each on its own
  bool complete() const { return task_feats && task_mask && task_ids && agent_feats && agent_mask && agent_ids && edge_valid; }
  bool all_or_none() const { return !task_feats || complete(); }  // (task_feats null: the kernels write no tokens)
  template <class TL>
  typename Sim<TL>::TokPtrs ptrs(int kind, int max_tasks, int max_agents) const {
    return {task_feats, task_mask, task_ids, agent_feats, agent_mask, agent_ids, edge_valid, n_urgent, expert_mask, replanned, kind, max_tasks, max_agents};
  }
};
TokOut next_tokens(const MuavtaRlStep& rs) {
  return {rs.task_feats, rs.task_mask, rs.task_ids, rs.agent_feats, rs.agent_mask, rs.agent_ids, rs.edge_valid, rs.n_urgent, nullptr, nullptr};
}
TokOut park_tokens(const MuavtaRlRun& rr) {
  return {rr.park_task_feats, rr.park_task_mask, rr.park_task_ids, rr.park_agent_feats, rr.park_agent_mask, rr.park_agent_ids, rr.park_edge_valid, rr.park_n_urgent, nullptr, nullptr};
}
TokOut record_tokens(const MuavtaRecord& r) {
  return {r.task_feats, r.task_mask, r.task_ids, r.agent_feats, r.agent_mask, r.agent_ids, r.edge_valid, r.n_urgent, r.expert_mask, r.replanned};
}

// The instantiation of a kernel family that the lane's allocator runs (one signature per family; with_allocator picks the tag) and the
// dynamic LDS it is launched with; launch_attr names every one of them.  (allocate_kernel is a plain function in front of its caller:
// where a kernel template is first named decides the order in which the compiler emits the kernels, and that order is kept.)
typedef void (*AllocateFn)(const DevCtx*, int, int, int, int32_t*, int32_t*, int, int);
struct AllocateKernel { AllocateFn fn; size_t lds; };
template <class TL>
using RolloutFn = void (*)(const DevCtx*, const uint64_t*, int, int, int, int, int, double*, const uint32_t*, const RecordPtrs<TL>*, int, int);

template <class TL>
static void launch_tokens(MuavtaEnv* e, const TokOut& out, int kind, int max_tasks, int max_agents) {
  hipLaunchKernelGGL(k_tokens<TL>, dim3(e->n_envs), dim3(WG), Lds<TL>::bytes(), e->stream, (const DevCtx*)e->d_ctx, out.ptrs<TL>(kind, max_tasks, max_agents));
}

template <class TL>
static void launch_rl_step(MuavtaEnv* e, const Target& t, const MuavtaRlStep& rs) {
  const MuavtaScored& p = rs.plan;
  hipLaunchKernelGGL(k_rl_step<TL>, dim3(t.count), dim3(WG), 0, t.stream, (const DevCtx*)e->d_ctx, scored_dev(p),
                     next_tokens(rs).ptrs<TL>(p.kind, p.max_tasks, p.max_agents), p.replan_interval, p.use_visibility, rs.write_obs, rs.s_wps, rs.done, e->n_envs, t.first);
}

// k_run for muavta_rl_run_device (src RUN_SRC_SCORED: `plan` with the caller's scores `sc`, next / park tokens) and for muavta_step_run (action rows
// da / di of `cap` entries, or the staged plan; of `plan` only gate and interval count, no scores, no tokens)
template <class TL>
static void launch_run(MuavtaEnv* e, const Target& t, int src, const MuavtaScored& plan, const ScoredDev& sc, const TokOut& next, const TokOut& park, const RunOut& R,
                       int write_obs, int max_steps, const int32_t* da, const int32_t* di, int cap) {
  RunArgs<TL> G;
  memset(&G, 0, sizeof(G));
  G.sc = sc; G.R = R;
  G.K = next.ptrs<TL>(plan.kind, plan.max_tasks, plan.max_agents);
  G.KP = park.ptrs<TL>(plan.kind, plan.max_tasks, plan.max_agents);
  hipLaunchKernelGGL(k_run<TL>, dim3(t.count), dim3(WG), 0, t.stream, G, (const DevCtx*)e->d_ctx, src, plan.gate, plan.replan_interval, plan.use_visibility, write_obs,
                     max_steps, da, di, cap, e->n_envs, t.first);
}

template <class TL>
static void launch_rollout(MuavtaEnv* e, const Target& t, const uint64_t* ds, int n_steps, int interval, int use_vis, int write_obs, const uint32_t* sb, size_t extra_lds,
                           const MuavtaRecord* rec) {
  const int epoch = (int)(e->pace_epoch++ % 65535u) + 1;  // 1..65535: the zero-filled table matches no launch
  char* slot = (char*)e->d_rec.p;  // slot 0, all zero: nothing to record
  if (rec && rec->rl) {  // the RL rings (rollout_record_rl has checked them): slot 2, and the recording instantiation of the installed policy's kind
    const MuavtaRlRings& r = *rec->rl;
    RlRingsDev R;
    memset(&R, 0, sizeof(R));
    R.tok = {r.task_feats, r.task_mask, r.agent_feats, r.agent_mask, r.edge_valid, r.context};
    R.next = {r.next_task_feats, r.next_task_mask, r.next_agent_feats, r.next_agent_mask, r.next_edge_valid, r.next_context};
    R.logits = r.logits; R.scores = r.scores; R.noise = r.noise; R.selected = r.selected;
    R.s_wps_before = r.s_wps_before; R.s_wps_after = r.s_wps_after; R.done = r.done; R.step = r.step; R.n_gates = r.n_gates;
    R.n_slots = r.n_slots; R.n_envs = e->n_envs;
    RecBlob blob;
    memset(&blob, 0, sizeof(blob));
    memcpy(&blob, &R, sizeof(R));
    slot += 2 * MuavtaEnv::REC_SLOT;
    hipLaunchKernelGGL(k_store_rec, dim3(1), dim3(64), 0, t.stream, blob, (uint32_t*)slot);  // (by value, stream-ordered: see below)
    const RolloutFn<TL> rl_fn = e->pol_kind == POL_CONTEXT_PAIR ? &k_rollout<TL, false, AllocLearnedRl<PolContextPair>> : &k_rollout<TL, false, AllocLearnedRl<PolPair>>;
    hipLaunchKernelGGL(rl_fn, dim3(t.count), dim3(WG), extra_lds, t.stream, (const DevCtx*)e->d_ctx, ds, n_steps, interval, use_vis, e->alloc_mode, write_obs,
                       (double*)e->d_metrics, sb, (const RecordPtrs<TL>*)slot, epoch, t.first);
    return;
  }
  if (rec) {
    RecordPtrs<TL> R;
    memset(&R, 0, sizeof(R));
    if (rec->kind >= 0) { R.K = record_tokens(*rec).ptrs<TL>(rec->kind, rec->max_tasks, rec->max_agents); R.s_wps = rec->s_wps; }
    if (rec->obs_tasks) {
      R.O.tasks = rec->obs_tasks; R.O.legal = (unsigned long long*)rec->obs_legal; R.O.pad = rec->obs_pad; R.O.agents = rec->obs_agents;
      R.O.flags = rec->obs_flags; R.O.reward = rec->obs_reward; R.O.done = rec->obs_done;
    }
    R.n_envs = e->n_envs;
    static_assert(sizeof(RecordPtrs<TL>) <= MuavtaEnv::REC_SLOT, "record-pointer slot too small");
    // The slot is filled by a one-lane kernel that takes the struct BY VALUE (kernel arguments are captured when the launch is queued)
    // — stream-ordered behind the previous launch that read the slot.  NOT hipMemcpyAsync from this stack frame: for pageable memory the
    // runtime may pin the pages and copy after the call has returned, by when the frame is gone (first r4 build: wild ring pointers).
    RecBlob blob;
    memset(&blob, 0, sizeof(blob));
    memcpy(&blob, &R, sizeof(R));
    slot += MuavtaEnv::REC_SLOT;  // slot 1: the RecordPtrs of this launch
    hipLaunchKernelGGL(k_store_rec, dim3(1), dim3(64), 0, t.stream, blob, (uint32_t*)slot);
  }
  RolloutFn<TL> rec_fn = &k_rollout<TL, true, AllocHungarian>;  // (muavta_rollout_record refuses the modes past the Hungarian family)
  if constexpr (runs_on<TL, AllocUrgencyWide>()) { if (e->alloc_mode == MUAVTA_ALLOC_URGENCY_PAIR && wide_pads(e)) rec_fn = &k_rollout<TL, true, AllocUrgencyWide>; }
  const RolloutFn<TL> fn = rec ? rec_fn
                               : with_allocator(e, [](auto al) -> RolloutFn<TL> {
                                   if constexpr (runs_on<TL, decltype(al)>()) return &k_rollout<TL, false, decltype(al)>; else return nullptr;  // (wide pads are refused on the 16-agent tiles)
                                 });
  hipLaunchKernelGGL(fn, dim3(t.count), dim3(WG), extra_lds, t.stream, (const DevCtx*)e->d_ctx, ds, n_steps, interval, use_vis, e->alloc_mode, write_obs,
                     (double*)e->d_metrics, sb, (const RecordPtrs<TL>*)slot, epoch, t.first);
}

}  // namespace

extern "C" {

int muavta_reset(MuavtaEnv* e, const uint64_t* seeds) {
  if (!e || !seeds) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  const uint64_t* ds = nullptr;
  const uint32_t* sb = nullptr;
  int slot = 0;
  { int rc = enqueue_seeding(e, seeds, &ds, &sb, &slot); if (rc) return rc; }
  DISPATCH(e, hipLaunchKernelGGL(k_reset<TL>, dim3(e->n_envs), dim3(WG), Lds<TL>::bytes(), e->stream, (const DevCtx*)e->d_ctx, ds, sb));
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipEventRecord(e->ev_consumed[slot], e->stream));
  e->last_seeded = true;  // muavta_last_seed_ms reports this reset's k_seed
  e->did_reset = true;
  e->host_valid = false;
  return MUAVTA_OK;
}

// agent ids index the per-agent arrays of the env blob on the device: reject anything outside [0, n_agents) up front
// (the reference's actions dict is keyed by agent name: an unknown name is a KeyError there, DroneEnv.py:813-816).
// `rows` rows of `cap` entries, the first of them env `first_env`; -1 ends a row.
static int check_agent_ids(MuavtaEnv* e, const int32_t* act_agent, int first_env, int rows, int cap, const char* who) {
  for (int n = 0; n < rows; n++)
    for (int k = 0; k < cap; k++) {
      const int a = act_agent[(size_t)n * cap + k];
      if (a < 0) break;
      if (a >= e->P.n_agents) {
        e->err = std::string(who) + ": env " + std::to_string(first_env + n) + " names agent id " + std::to_string(a) + ", valid ids are 0.." + std::to_string(e->P.n_agents - 1);
        return MUAVTA_E_ARG;
      }
    }
  return MUAVTA_OK;
}
// The release log is written by the whole-batch muavta_step / _step_staged only: every other stepping entry point refuses while it is on.
static int refuse_release_log(MuavtaEnv* e, const char* who) {
  if (!e->d_rel) return MUAVTA_OK;
  e->err = std::string(who) + ": the release log must be off (muavta_set_release_log)";
  return MUAVTA_E_STATE;
}
// The action rows staged for the target's envs, to the host; waits for the target's stream.
static int fetch_actions(MuavtaEnv* e, const Target& t, int32_t* act_agent, int32_t* act_index) {
  const size_t off = (size_t)t.first * e->A, bytes = (size_t)t.count * e->A * sizeof(int32_t);
  HIPCHK(e, hipMemcpyAsync(act_agent, t.act_agent + off, bytes, hipMemcpyDeviceToHost, t.stream));
  HIPCHK(e, hipMemcpyAsync(act_index, t.act_index + off, bytes, hipMemcpyDeviceToHost, t.stream));
  HIPCHK(e, hipStreamSynchronize(t.stream));
  return MUAVTA_OK;
}

// One env step of the whole batch or of a part.  aa / ai: the target's rows of `cap` entries (null: the plan staged in the env records).
// Rows longer than the tile (muavta_step_lists) and the release log exist for the whole batch only: a part's rows are the tile's, and
// muavta_step_part refuses while the log is on.
static int step_on(MuavtaEnv* e, const int32_t* part, const char* who, const int32_t* aa, const int32_t* ai, int cap) {
  if (int rc = check_target(e, part, who)) return rc;
  DeviceScope scope_(e->device);
  Target t;
  if (int rc = open_target(e, part, &t)) return rc;
  const int32_t *da = nullptr, *di = nullptr;
  if (aa) {
    int32_t *ba = t.act_agent, *bi = t.act_index;
    if (cap > e->A) {  // rows longer than the handle's action buffers
      if (cap > e->list_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        e->list_cap = 0;
        HIPCHK(e, e->d_list_agent.alloc((size_t)e->n_envs * cap * sizeof(int32_t)));
        HIPCHK(e, e->d_list_index.alloc((size_t)e->n_envs * cap * sizeof(int32_t)));
        e->list_cap = cap;
      }
      ba = e->d_list_agent; bi = e->d_list_index;
    }
    const size_t off = (size_t)t.first * cap, bytes = (size_t)t.count * cap * sizeof(int32_t);
    HIPCHK(e, hipMemcpyAsync(ba + off, aa, bytes, hipMemcpyHostToDevice, t.stream));
    HIPCHK(e, hipMemcpyAsync(bi + off, ai, bytes, hipMemcpyHostToDevice, t.stream));
    da = ba; di = bi;
  }
  if (e->d_rel) HIPCHK(e, hipMemsetAsync(e->d_rel, 0, (size_t)e->n_envs * (1 + MUAVTA_REL_ROW * e->T) * sizeof(double), t.stream));
  DISPATCH(e, hipLaunchKernelGGL(k_step<TL>, dim3(t.count), dim3(WG), 0, t.stream, (const DevCtx*)e->d_ctx, da, di, cap, (double*)e->d_rel, t.first));  // (static LDS)
  HIPCHK(e, hipGetLastError());
  e->host_valid = false;
  return MUAVTA_OK;
}

int muavta_step_lists(MuavtaEnv* e, const int32_t* act_agent, const int32_t* act_index, int32_t list_cap) {
  if (!e || !act_agent || !act_index) return MUAVTA_E_ARG;
  if (list_cap < 1 || list_cap > 32767) { e->err = "muavta_step_lists: list_cap must be in 1..32767"; return MUAVTA_E_ARG; }
  if (int rc = check_agent_ids(e, act_agent, 0, e->n_envs, list_cap, "muavta_step")) return rc;
  return step_on(e, nullptr, "step", act_agent, act_index, list_cap);
}
int muavta_step(MuavtaEnv* e, const int32_t* act_agent, const int32_t* act_index) {
  if (!e) return MUAVTA_E_ARG;
  return muavta_step_lists(e, act_agent, act_index, e->A);
}
int muavta_step_staged(MuavtaEnv* e) {
  if (!e) return MUAVTA_E_ARG;
  return step_on(e, nullptr, "step", nullptr, nullptr, e->A);
}
int muavta_step_part(MuavtaEnv* e, int32_t part, const int32_t* act_agent, const int32_t* act_index) {
  const char* who = "muavta_step_part";
  if (int rc = check_target(e, &part, who)) return rc;  // (here already: the checks below need the part's range)
  if (int rc = refuse_release_log(e, who)) return rc;
  if (act_agent && act_index) {  // NULL: the actions muavta_allocate_part staged in the env records
    int first, count;
    part_range(e, part, &first, &count);
    if (int rc = check_agent_ids(e, act_agent, first, count, e->A, who)) return rc;
  } else if (act_agent || act_index) return MUAVTA_E_ARG;
  return step_on(e, &part, who, act_agent, act_index, e->A);
}

static AllocateKernel allocate_kernel(MuavtaEnv* e) {
  return with_allocator(e, [e](auto al) {
    AllocateKernel k{};
    DISPATCH(e, if constexpr ((runs_on<TL, decltype(al)>())) (k = AllocateKernel{&k_allocate<TL, decltype(al)>, Lds<TL>::bytes() + al.EXTRA_LDS}));
    return k;
  });
}
// The planner of the handle's allocator mode for the whole batch or a part: the plan is staged in the env records and, as action rows, in
// the target's staging pair; act_* (both or neither) receive the target's rows and make the call wait.
static int allocate_on(MuavtaEnv* e, const int32_t* part, const char* who, int interval, int use_vis, int32_t* act_agent, int32_t* act_index) {
  if (int rc = check_target(e, part, who)) return rc;
  DeviceScope scope_(e->device);
  Target t;
  if (int rc = open_target(e, part, &t)) return rc;
  const AllocateKernel k = allocate_kernel(e);
  hipLaunchKernelGGL(k.fn, dim3(t.count), dim3(WG), k.lds, t.stream, (const DevCtx*)e->d_ctx, interval, use_vis, e->alloc_mode, t.act_agent, t.act_index, e->A, t.first);
  HIPCHK(e, hipGetLastError());
  e->host_valid = false;
  if (act_agent && act_index) return fetch_actions(e, t, act_agent, act_index);
  return MUAVTA_OK;
}
int muavta_allocate(MuavtaEnv* e, int32_t interval, int32_t use_vis, int32_t* act_agent, int32_t* act_index) {
  return allocate_on(e, nullptr, "allocate", interval, use_vis, act_agent, act_index);
}
int muavta_allocate_part(MuavtaEnv* e, int32_t part, int32_t interval, int32_t use_vis, int32_t* act_agent, int32_t* act_index) {
  return allocate_on(e, &part, "muavta_allocate_part", interval, use_vis, act_agent, act_index);
}

static int token_dims(int kind, int* dt, int* da);

// ---- HungarianAllocator.allocate_tasks with the caller's edge scores / priorities / reserved agents ------------------------------
static int scored_check(MuavtaEnv* e, const MuavtaScored* sp) {
  int dt, da;
  if (!e) return MUAVTA_E_ARG;
  if (!sp || token_dims(sp->kind, &dt, &da) || sp->max_tasks < 1 || sp->max_tasks > 128 || sp->max_agents < 1 || sp->max_agents > 64 ||
      sp->gate < MUAVTA_GATE_FORCE || sp->gate > MUAVTA_GATE_ALLOCATOR || (sp->flags & ~7) ||
      (sp->kind == MUAVTA_TOK_ESCORT && (sp->flags & MUAVTA_SC_FULL_TASK_LIST))) {
    e->err = "muavta_allocate_scored: bad spec (kind 0..2, max_tasks 1..128, max_agents 1..64, gate 0..3, flags 0..7; build_escort_tokens has no untruncated list)";
    return MUAVTA_E_ARG;
  }
  if (!e->did_reset) { e->err = "allocate before reset"; return MUAVTA_E_STATE; }
  return MUAVTA_OK;
}
int muavta_allocate_scored_device(MuavtaEnv* e, const MuavtaScored* sp) {
  if (int rc = scored_check(e, sp)) return rc;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  DISPATCH(e, hipLaunchKernelGGL(k_allocate_scored<TL>, dim3(e->n_envs), dim3(WG), Lds<TL>::bytes() + SCORED_EXTRA_LDS, e->stream, (const DevCtx*)e->d_ctx, scored_dev(*sp),
                                 sp->replan_interval, sp->use_visibility, (int32_t*)e->d_act_agent, (int32_t*)e->d_act_index, e->A, 0));
  HIPCHK(e, hipGetLastError());
  e->host_valid = false;
  return MUAVTA_OK;
}
int muavta_allocate_scored(MuavtaEnv* e, const MuavtaScored* sp, int32_t* act_agent, int32_t* act_index) {
  if (int rc = scored_check(e, sp)) return rc;
  DeviceScope scope_(e->device);
  const size_t N = (size_t)e->n_envs, MT = (size_t)sp->max_tasks, MA = (size_t)sp->max_agents;
  const size_t sz[5] = {N * MA * MT * 4, N * MT * 8, N * 8, N * MA * MT * 4, N * 4};  // scores, pri, reserved | selected, replanned
  size_t off[6] = {0};
  for (int i = 0; i < 5; i++) off[i + 1] = off[i] + ((sz[i] + 255) & ~(size_t)255);
  if (int rc = grow_staging(e, off[5])) return rc;
  char* b = (char*)e->d_tok.p;
  const void* in[3] = {sp->edge_scores, sp->task_pri, sp->reserved};
  for (int i = 0; i < 3; i++)
    if (in[i]) HIPCHK(e, hipMemcpyAsync(b + off[i], in[i], sz[i], hipMemcpyHostToDevice, e->stream));
  MuavtaScored d = *sp;
  d.edge_scores = sp->edge_scores ? (const float*)(b + off[0]) : nullptr;
  d.task_pri = sp->task_pri ? (const double*)(b + off[1]) : nullptr;
  d.reserved = sp->reserved ? (const uint64_t*)(b + off[2]) : nullptr;
  d.selected = sp->selected ? (float*)(b + off[3]) : nullptr;
  d.replanned = sp->replanned ? (int32_t*)(b + off[4]) : nullptr;
  if (int rc = muavta_allocate_scored_device(e, &d)) return rc;
  if (sp->selected) HIPCHK(e, hipMemcpyAsync(sp->selected, b + off[3], sz[3], hipMemcpyDeviceToHost, e->stream));
  if (sp->replanned) HIPCHK(e, hipMemcpyAsync(sp->replanned, b + off[4], sz[4], hipMemcpyDeviceToHost, e->stream));
  if (act_agent && act_index) {
    Target t;
    if (int rc = open_target(e, nullptr, &t)) return rc;
    return fetch_actions(e, t, act_agent, act_index);  // (waits for the stream: the copies above included)
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}
int muavta_rl_step_device(MuavtaEnv* e, const MuavtaRlStep* rs) {
  if (!e || !rs) return MUAVTA_E_ARG;
  if (int rc = scored_check(e, &rs->plan)) return rc;
  if (!next_tokens(*rs).all_or_none()) {
    e->err = "muavta_rl_step_device: the next-token outputs come all together or not at all (n_urgent alone is optional)"; return MUAVTA_E_ARG;
  }
  DeviceScope scope_(e->device);
  if (int rc = refuse_release_log(e, "muavta_rl_step_device")) return rc;
  // one sub-batch on its own stream (muavta_set_parts): the tensors are the whole batch's, the launch touches the part's rows
  const int32_t p = rs->part - 1, *part = rs->part > 0 ? &p : nullptr;
  Target t;
  if (int rc = check_target(e, part, "muavta_rl_step_device")) return rc;
  if (int rc = open_target(e, part, &t)) return rc;
  DISPATCH(e, launch_rl_step<TL>(e, t, *rs));
  HIPCHK(e, hipGetLastError());
  e->host_valid = false;
  return MUAVTA_OK;
}
// Run to the next replan gate (k_run; include/muavta.h): the policy in the loop, consulted only where an env's gate fired
int muavta_rl_run_device(MuavtaEnv* e, const MuavtaRlRun* rr) {
  if (!e || !rr) return MUAVTA_E_ARG;
  const MuavtaRlStep* rs = &rr->first;
  if (int rc = scored_check(e, &rs->plan)) return rc;
  if (!next_tokens(*rs).all_or_none() || !park_tokens(*rr).all_or_none()) {
    e->err = "muavta_rl_run_device: the token outputs (next / park) come all together or not at all (n_urgent alone is optional)"; return MUAVTA_E_ARG;
  }
  if (rr->max_steps < 0) { e->err = "muavta_rl_run_device: max_steps >= 0 (0: until the gate fires or the episode ends)"; return MUAVTA_E_ARG; }
  DeviceScope scope_(e->device);
  if (int rc = refuse_release_log(e, "muavta_rl_run_device")) return rc;
  const int32_t p = rs->part - 1, *part = rs->part > 0 ? &p : nullptr;
  Target t;
  if (int rc = check_target(e, part, "muavta_rl_run_device")) return rc;
  if (int rc = open_target(e, part, &t)) return rc;
  const RunOut R{rs->s_wps, rs->done, rr->n_stepped, rr->park, rr->reward_sum};
  DISPATCH(e, launch_run<TL>(e, t, RUN_SRC_SCORED, rs->plan, scored_dev(rs->plan), next_tokens(*rs), park_tokens(*rr), R, rs->write_obs, rr->max_steps, nullptr, nullptr, 0));
  HIPCHK(e, hipGetLastError());
  e->host_valid = false;
  return MUAVTA_OK;
}
int muavta_step_run(MuavtaEnv* e, const int32_t* act_agent, const int32_t* act_index, int32_t gate, int32_t interval, int32_t max_steps, int32_t write_obs,
                    int32_t* n_stepped, uint8_t* park, double* reward_sum) {
  if (!e) return MUAVTA_E_ARG;
  if (!e->did_reset) { e->err = "muavta_step_run before reset"; return MUAVTA_E_STATE; }
  if ((act_agent == nullptr) != (act_index == nullptr) || gate < MUAVTA_GATE_FORCE || gate > MUAVTA_GATE_ALLOCATOR || max_steps < 0) {
    e->err = "muavta_step_run: action rows come as a pair (or both NULL: the staged plan), gate 0..3, max_steps >= 0"; return MUAVTA_E_ARG;
  }
  if (act_agent)
    if (int rc = check_agent_ids(e, act_agent, 0, e->n_envs, e->A, "muavta_step_run")) return rc;
  DeviceScope scope_(e->device);
  if (int rc = refuse_release_log(e, "muavta_step_run")) return rc;
  Target t;
  if (int rc = open_target(e, nullptr, &t)) return rc;
  const size_t N = (size_t)e->n_envs;
  if (!e->d_run) HIPCHK(e, e->d_run.alloc(N * 16));
  double* d_rsum = (double*)e->d_run.p; int32_t* d_n = (int32_t*)(d_rsum + N); uint8_t* d_park = (uint8_t*)(d_n + N);
  const int32_t *da = nullptr, *di = nullptr;
  if (act_agent) {
    const size_t bytes = N * e->A * sizeof(int32_t);
    HIPCHK(e, hipMemcpyAsync(t.act_agent, act_agent, bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(t.act_index, act_index, bytes, hipMemcpyHostToDevice, e->stream));
    da = t.act_agent; di = t.act_index;
  }
  MuavtaScored plan{};  // (no scores, no tokens: the gate and its interval only)
  plan.gate = gate; plan.replan_interval = interval;
  const RunOut R{nullptr, nullptr, d_n, d_park, d_rsum};
  DISPATCH(e, launch_run<TL>(e, t, act_agent ? RUN_SRC_ROWS : RUN_SRC_STAGED, plan, ScoredDev{}, TokOut{}, TokOut{}, R, write_obs, max_steps, da, di, e->A));
  HIPCHK(e, hipGetLastError());
  e->host_valid = false;
  if (n_stepped) HIPCHK(e, hipMemcpyAsync(n_stepped, d_n, N * 4, hipMemcpyDeviceToHost, e->stream));
  if (park) HIPCHK(e, hipMemcpyAsync(park, d_park, N, hipMemcpyDeviceToHost, e->stream));
  if (reward_sum) HIPCHK(e, hipMemcpyAsync(reward_sum, d_rsum, N * 8, hipMemcpyDeviceToHost, e->stream));
  if (n_stepped || park || reward_sum) HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}
static int rollout_impl(MuavtaEnv* e, const uint64_t* seeds, int32_t n_steps, int32_t interval, int32_t use_vis, int32_t write_obs, const MuavtaRecord* rec) {
  if (!e || n_steps < 0) return MUAVTA_E_ARG;
  if (!seeds && !e->did_reset) { e->err = "rollout without seeds before reset"; return MUAVTA_E_STATE; }
  DeviceScope scope_(e->device);
  if (seeds && e->hl.lanes_mode != 1) {
    // a fresh episode batch while this lane's last rollout is still running (or always, in mode 2): it goes to the other lane
    bool want = e->hl.lanes_mode == 2;
    if (!want && e->n_rollouts) { want = hipEventQuery(e->ev1[(e->n_rollouts - 1) % MuavtaEnv::EV_RING]) == hipErrorNotReady; (void)hipGetLastError(); }
    if (want && ensure_twin(e) == MUAVTA_OK) flip_lanes(e);
  }
  Target t;
  if (int rc = open_target(e, nullptr, &t)) return rc;
  const uint64_t* ds = nullptr;
  const uint32_t* sb = nullptr;
  int slot = -1;
  if (seeds) { int rc = enqueue_seeding(e, seeds, &ds, &sb, &slot); if (rc) return rc; }
  e->last_seeded = ds != nullptr;
  // muavta_rollout_record's obs_done pre-fill: on the stream of the lane that runs the kernel, so only after the lane decision above
  if (rec && rec->obs_done && n_steps > 0)
    HIPCHK(e, hipMemsetAsync(rec->obs_done, MUAVTA_OBS_UNWRITTEN, (size_t)n_steps * (size_t)e->n_envs, e->stream));
  if (rec && rec->rl) {  // the RL rings' pre-fill, likewise: step = -1 in every slot (not written), no gate counted yet
    HIPCHK(e, hipMemsetAsync(rec->rl->step, 0xFF, (size_t)rec->rl->n_slots * (size_t)e->n_envs * sizeof(int32_t), e->stream));
    HIPCHK(e, hipMemsetAsync(rec->rl->n_gates, 0, (size_t)e->n_envs * sizeof(int32_t), e->stream));
  }
  const int evi = (int)(e->n_rollouts % MuavtaEnv::EV_RING);
  HIPCHK(e, hipEventRecord(e->ev0[evi], e->stream));
  static const size_t extra_lds = getenv("MUAVTA_EXTRA_LDS") ? (size_t)atoi(getenv("MUAVTA_EXTRA_LDS")) : 0;  // occupancy experiments only
  DISPATCH(e, launch_rollout<TL>(e, t, ds, n_steps, interval, use_vis, write_obs, sb, extra_lds, rec));
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipEventRecord(e->ev1[evi], e->stream));
  e->hl.ring_lane[e->hl.n_launches % MuavtaEnv::HandleLevel::RING] = (unsigned char)e->lane_id;
  e->hl.ring_no[e->hl.n_launches % MuavtaEnv::HandleLevel::RING] = e->n_rollouts;
  e->hl.n_launches++;
  e->n_rollouts++;
  e->timing_stale = false;
  if (slot >= 0) HIPCHK(e, hipEventRecord(e->ev_consumed[slot], e->stream));
  e->did_reset = true;
  e->host_valid = false;
  return MUAVTA_OK;
}
int muavta_rollout(MuavtaEnv* e, const uint64_t* seeds, int32_t n_steps, int32_t interval, int32_t use_vis, int32_t write_obs) {
  return rollout_impl(e, seeds, n_steps, interval, use_vis, write_obs, nullptr);
}
// muavta_rollout_record with rec->rl: everything that is not the one accepted combination is refused here, with its reason
static int rollout_record_rl(MuavtaEnv* e, const uint64_t* seeds, int32_t n_steps, int32_t interval, int32_t use_vis, int32_t write_obs, const MuavtaRecord* rec) {
  const MuavtaRlRings& r = *rec->rl;
  const char* why = nullptr;
  if (rec->kind >= 0 || rec->obs_tasks || rec->obs_legal || rec->obs_pad || rec->obs_agents || rec->obs_flags || rec->obs_reward || rec->obs_done)
    why = "the RL rings come alone (kind < 0, no observation rings)";
  else if (e->alloc_mode != MUAVTA_ALLOC_MLP_PAIR) why = "the RL rings need the MUAVTA_ALLOC_MLP_PAIR allocator (muavta_set_allocator)";
  else if (e->pol_kind != POL_PAIR && e->pol_kind != POL_CONTEXT_PAIR) why = "the RL rings are recorded for an MLP-Pair or MLP-ContextPair policy, not for an MLP-Coalition";
  else if (wide_pads(e)) why = "the RL rings are recorded at the (32, 16) token pads only (muavta_set TOKEN_PADS)";
  else if (r.n_slots < 1 || r.n_slots > MUAVTA_RL_MAX_SLOTS) why = "the RL rings need 1 <= n_slots <= 4096";
  else if (!(r.task_feats && r.task_mask && r.agent_feats && r.agent_mask && r.edge_valid && r.logits && r.scores && r.selected && r.s_wps_before && r.s_wps_after &&
             r.next_task_feats && r.next_task_mask && r.next_agent_feats && r.next_agent_mask && r.next_edge_valid && r.done && r.step && r.n_gates))
    why = "an RL ring is NULL (only noise may be; context / next_context follow the policy's kind)";
  else if (e->pol_kind == POL_CONTEXT_PAIR && !(r.context && r.next_context)) why = "an MLP-ContextPair policy needs the context and next_context rings";
  else if (e->pol_kind == POL_PAIR && (r.context || r.next_context)) why = "an MLP-Pair policy has no context: context and next_context must be NULL";
  if (why) { e->err = std::string("muavta_rollout_record: ") + why; return MUAVTA_E_ARG; }
  return rollout_impl(e, seeds, n_steps, interval, use_vis, write_obs, rec);  // (pre-fills step and n_gates once the lane is chosen)
}
int muavta_rollout_record(MuavtaEnv* e, const uint64_t* seeds, int32_t n_steps, int32_t interval, int32_t use_vis, int32_t write_obs, const MuavtaRecord* rec) {
  int dt, da;
  if (e && rec && rec->rl) return rollout_record_rl(e, seeds, n_steps, interval, use_vis, write_obs, rec);
  bool bad = !e || !rec;
  if (!bad && rec->kind >= 0)
    bad = token_dims(rec->kind, &dt, &da) || rec->max_tasks < 1 || rec->max_agents < 1 || rec->max_tasks > 4096 || rec->max_agents > 4096 ||
          !record_tokens(*rec).complete() || !rec->s_wps;
  const bool any_obs = !bad && (rec->obs_tasks || rec->obs_legal || rec->obs_pad || rec->obs_agents || rec->obs_flags || rec->obs_reward || rec->obs_done);
  if (any_obs)  // all seven or none, and only with per-step observations switched on
    bad = !(rec->obs_tasks && rec->obs_legal && rec->obs_pad && rec->obs_agents && rec->obs_flags && rec->obs_reward && rec->obs_done) || !write_obs;
  if (!bad && rec->kind < 0 && !any_obs) bad = true;  // nothing to record
  if (bad) {
    if (e) e->err = "muavta_rollout_record: bad argument";
    return MUAVTA_E_ARG;
  }
  if (e->alloc_mode >= MUAVTA_ALLOC_CAP_GREEDY) {  // the recording kernels carry the Hungarian-family planners only
    e->err = e->alloc_mode == MUAVTA_ALLOC_MLP_PAIR
                 ? "muavta_rollout_record: not available with the MLP-Pair allocator (set_allocator back to a Hungarian mode)"
                 : "muavta_rollout_record: not available with the Cap-Greedy / PI allocators (set_allocator back to a Hungarian mode)";
    return MUAVTA_E_ARG;
  }
  return rollout_impl(e, seeds, n_steps, interval, use_vis, write_obs, rec);  // (pre-fills obs_done once the lane is chosen)
}

int muavta_rollout_part(MuavtaEnv* e, int32_t part, int32_t n_steps, int32_t interval, int32_t use_vis, int32_t write_obs) {
  if (int rc = check_target(e, &part, "muavta_rollout_part")) return rc;
  if (n_steps < 0) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  Target t;
  if (int rc = open_target(e, &part, &t)) return rc;
  DISPATCH(e, launch_rollout<TL>(e, t, nullptr, n_steps, interval, use_vis, write_obs, nullptr, 0, nullptr));
  HIPCHK(e, hipGetLastError());
  e->timing_stale = true;  // (part launches carry no event pair: muavta_last_kernel_ms / _history refuse until the next whole-batch rollout)
  e->host_valid = false;
  return MUAVTA_OK;
}

int muavta_set_allocator(MuavtaEnv* e, int32_t mode) {
  if (!e || (mode < MUAVTA_ALLOC_HUNGARIAN || mode > MUAVTA_ALLOC_MLP_PAIR)) { if (e) e->err = "unknown allocator mode"; return MUAVTA_E_ARG; }
  if (mode == MUAVTA_ALLOC_MLP_PAIR && !e->hl.pol_set) {
    e->err = "muavta_set_allocator: MUAVTA_ALLOC_MLP_PAIR needs a policy (muavta_set_pair_policy first)";  // (or muavta_set_context_pair_policy)
    return MUAVTA_E_STATE;
  }
  e->alloc_mode = mode;
  if (e->hl.twin) e->hl.twin->alloc_mode = mode;
  return MUAVTA_OK;
}

int muavta_set_release_log(MuavtaEnv* e, int32_t enable) {
  if (!e) return MUAVTA_E_ARG;
  if (e->hl.twin) { int rc = muavta_set_release_log(e->hl.twin, enable); if (rc) { e->err = e->hl.twin->err; return rc; } }
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (enable && !e->d_rel) {
    const size_t bytes = (size_t)e->n_envs * (1 + MUAVTA_REL_ROW * e->T) * sizeof(double);
    HIPCHK(e, e->d_rel.alloc(bytes));
    HIPCHK(e, hipMemset(e->d_rel, 0, bytes));
  } else if (!enable && e->d_rel) {
    e->d_rel.reset();
  }
  return MUAVTA_OK;
}

int muavta_last_kernel_ms(MuavtaEnv* e, float* ms) {
  if (!e || !ms) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  if (!e->n_rollouts) { e->err = "no rollout launched yet"; return MUAVTA_E_STATE; }
  if (e->timing_stale) { e->err = "muavta_last_kernel_ms: the last rollout was a muavta_rollout_part launch, which records no event pair"; return MUAVTA_E_STATE; }
  const int evi = (int)((e->n_rollouts - 1) % MuavtaEnv::EV_RING);
  HIPCHK(e, hipEventSynchronize(e->ev1[evi]));
  HIPCHK(e, hipEventElapsedTime(ms, e->ev0[evi], e->ev1[evi]));
  return MUAVTA_OK;
}

// The event pair of the handle's rollout launch number h: the lane it ran on and that lane's ring slot.  False: the pair has been reused since.
struct LaunchEvents { MuavtaEnv* lane; hipEvent_t start, end; };
static bool launch_events(MuavtaEnv* e, unsigned long long h, LaunchEvents* out) {
  MuavtaEnv* L = lane_by_id(e, e->hl.ring_lane[h % MuavtaEnv::HandleLevel::RING]);
  const unsigned long long no = e->hl.ring_no[h % MuavtaEnv::HandleLevel::RING];
  if (!L || L->n_rollouts - no > (unsigned long long)MuavtaEnv::EV_RING) return false;
  *out = {L, L->ev0[no % MuavtaEnv::EV_RING], L->ev1[no % MuavtaEnv::EV_RING]};
  return true;
}

int muavta_kernel_ms_history(MuavtaEnv* e, float* ms, int32_t n) {  // durations of the last n rollout launches, oldest first
  if (!e || !ms || n < 1 || n > MuavtaEnv::EV_RING) { if (e) e->err = "muavta_kernel_ms_history: 1 <= n <= 64"; return MUAVTA_E_ARG; }
  if ((unsigned long long)n > e->hl.n_launches) { e->err = "fewer rollouts launched than asked for"; return MUAVTA_E_STATE; }
  if (e->timing_stale) { e->err = "muavta_kernel_ms_history: the last rollout was a muavta_rollout_part launch, which records no event pair"; return MUAVTA_E_STATE; }
  DeviceScope scope_(e->device);
  for (int k = 0; k < n; k++) {  // (with two state lanes consecutive launches alternate between the lanes' event rings and may overlap on the device)
    LaunchEvents ev;
    if (!launch_events(e, e->hl.n_launches - (unsigned long long)n + (unsigned long long)k, &ev)) {
      e->err = "muavta_kernel_ms_history: that launch's event pair has been reused"; return MUAVTA_E_STATE;
    }
    HIPCHK(e, hipEventSynchronize(ev.end));
    HIPCHK(e, hipEventElapsedTime(&ms[k], ev.start, ev.end));
  }
  return MUAVTA_OK;
}

int muavta_launch_gaps_ms(MuavtaEnv* e, float* ms, int32_t n) {  // idle time of the handle's stream between the last n rollout launches: n - 1 gaps, oldest first
  if (!e || !ms || n < 2 || n > MuavtaEnv::EV_RING) { if (e) e->err = "muavta_launch_gaps_ms: 2 <= n <= 64"; return MUAVTA_E_ARG; }
  if ((unsigned long long)n > e->hl.n_launches) { e->err = "fewer rollouts launched than asked for"; return MUAVTA_E_STATE; }
  if (e->timing_stale) { e->err = "muavta_launch_gaps_ms: the last rollout was a muavta_rollout_part launch, which records no event pair"; return MUAVTA_E_STATE; }
  DeviceScope scope_(e->device);
  for (int k = 0; k + 1 < n; k++) {  // end of launch i .. start of launch i + 1 (NEGATIVE when they ran on different lanes and overlapped)
    const unsigned long long h = e->hl.n_launches - (unsigned long long)n + (unsigned long long)k;
    LaunchEvents a, b;
    if (!launch_events(e, h, &a) || !launch_events(e, h + 1, &b)) { e->err = "muavta_launch_gaps_ms: an event pair has been reused"; return MUAVTA_E_STATE; }
    HIPCHK(e, hipEventSynchronize(b.start));
    HIPCHK(e, hipEventSynchronize(a.end));
    if (a.lane == b.lane) HIPCHK(e, hipEventElapsedTime(&ms[k], a.end, b.start));
    else {  // events of two streams: elapsed time in either direction, signed
      float fwd = 0.f;
      hipError_t r = hipEventElapsedTime(&fwd, a.end, b.start);
      if (r != hipSuccess) { e->err = std::string("hipEventElapsedTime: ") + hipGetErrorString(r); return MUAVTA_E_HIP; }
      ms[k] = fwd;
    }
  }
  return MUAVTA_OK;
}

int muavta_last_seed_ms(MuavtaEnv* e, float* ms) {  // the RNG seeding kernel that preceded the last muavta_rollout (0 without seeds)
  if (!e || !ms) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  *ms = 0.f;
  if (!e->last_seeded) return MUAVTA_OK;
  HIPCHK(e, hipEventSynchronize(e->ev_seeded[e->last_seed_slot]));
  HIPCHK(e, hipEventElapsedTime(ms, e->ev_seed0[e->last_seed_slot], e->ev_seeded[e->last_seed_slot]));
  return MUAVTA_OK;
}

}  // extern "C"
