// The handle behind the C ABI.  Included by muavta_kernels.hip: one translation unit, the launch sites must see the kernel templates.
namespace {

thread_local std::string g_create_error;

#define HIPCHK(env, expr)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      (env)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                             \
      return MUAVTA_E_HIP;                                                                        \
    }                                                                                             \
  } while (0)

enum TileKind { TK16 = 0, TK24 = 1, TK64 = 2 };

// An ABI call runs on its handle's device and leaves the calling thread's current device as it found it (a caller that
// mixes this library with torch on another device must not have its current device changed under it).
struct DeviceScope {
  int prev = -1, want;
  explicit DeviceScope(int d) : want(d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != want) (void)hipSetDevice(want);
  }
  ~DeviceScope() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
};

// HIPCHK for code that has no handle to report through (muavta_create, the stand-alone probes): the message goes to the thread's create
// error, and `cleanup` runs before the return.
#define HIPCHK_G(expr, cleanup) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { g_create_error = std::string(#expr) + ": " + hipGetErrorString(e_); cleanup; return MUAVTA_E_HIP; } } while (0)

// One device allocation and its owner: released when the owner goes or allocates again.  Move-only: flip_lanes swaps whole handles, so the
// device pointer travels with its lane, and nothing may keep a pointer INTO a handle across a flip.  Reads as the raw pointer.
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }
  hipError_t alloc(size_t bytes) { reset(); return hipMalloc((void**)&p, bytes); }
  operator T*() const { return p; }
};

}  // namespace

struct MuavtaEnv {
  DevParams P;
  MuavtaParams params;
  int tile = TK16;
  int alloc_mode = 0;  // MUAVTA_ALLOC_*
  DevBuf<void> d_tok;  // muavta_tokens staging (host-buffer variant)
  DevBuf<double> d_rel;  // release log [N, 1 + MUAVTA_REL_ROW*T] (muavta_set_release_log)
  // Seeding pipeline: seeds upload + k_seed run on their own stream into one of two slots, so that the seeding of launch
  // i+1 overlaps launch i (k_seed uses no LDS and few registers: its waves run next to the rollout's where a SIMD has room).
  DevBuf<uint32_t> d_seedbuf[2];  // [N][4][624] init_by_array states (k_seed)
  DevBuf<uint32_t> d_seedtmp;             // k_seed's lane-interleaved scratch
  uint64_t* h_seeds[2] = {nullptr, nullptr};    // pinned staging of the caller's seeds
  hipStream_t seed_stream = nullptr;
  hipEvent_t ev_seed0[2] = {nullptr, nullptr}, ev_seeded[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
  bool seed_used[2] = {false, false};
  unsigned seed_seq = 0;
  int last_seed_slot = 0;
  size_t tok_bytes = 0;
  int n_envs = 0, device = 0;
  int A = 0, T = 0, H = 0, E = 0, R = 0, Q = 0;
  size_t state_bytes = 0, cold_bytes = 0, lds_bytes = 0;  // per env: LDS image (EnvState), HBM-only part (EnvCold)
  DevBuf<void> blobs, cold;
  DevBuf<uint32_t> tapes;
  DevBuf<DevCtx> d_ctx;  // device copy of {P, O, tapes}
  DevBuf<uint32_t> d_pace;
  uint32_t pace_epoch = 0;
  enum { REC_SLOT = 256 };
  DevBuf<void> d_rec;  // [2][REC_SLOT]: slot 0 all zero (plain rollouts), slot 1 the RecordPtrs of the muavta_rollout_record launch in flight
  DevBuf<uint64_t> d_seeds[2];
  DevBuf<int32_t> d_act_agent, d_act_index, d_call_out;
  DevBuf<int32_t> d_list_agent, d_list_index;  // muavta_step_lists rows [N][list_cap] (grown on demand)
  DevBuf<void> d_run;  // muavta_step_run's outputs: [N] f64 reward sums | [N] i32 steps taken | [N] u8 park flags
  int list_cap = 0;
  ncclComm_t comm = nullptr;  // muavta_comm_init
  int comm_rank = 0, comm_ranks = 0;
  DevBuf<void> d_comm;    // [64 f64 send | 64 x n_ranks f64 recv | 64 i64 send | 64 i64 recv]
  DevBuf<double> d_metrics;
  DevBuf<float> d_pol_w, d_pol_scratch;  // muavta_set_pair_policy: this lane's copy of the packed weights, its per-env token / score scratch
  int pol_kind = POL_PAIR;               // ... and which network they hold (push_policy): selects the kernel instantiation of MUAVTA_ALLOC_MLP_PAIR on this lane
  ObsPtrs O{};  // the observation buffers as the kernels see them: views of obs_mem
  DevBuf<void> obs_mem[7];
  hipStream_t stream = nullptr;
  // sub-batches (muavta_set_parts): contiguous env ranges, each stepped on its own stream so that the host can decide for one part
  // while the device steps another, and so that one part's slowest env does not hold up the others' launches
  enum { MAX_PARTS = 8 };
  int n_parts = 0;
  hipStream_t part_stream[MAX_PARTS] = {};
  hipEvent_t part_ev[MAX_PARTS] = {};
  hipEvent_t ev_fork = nullptr;
  bool part_busy[MAX_PARTS] = {};         // the part's stream holds work the main stream has not been ordered after yet
  bool part_fork_needed[MAX_PARTS] = {};  // the main stream got work since the part's stream last waited for it
  DevBuf<int32_t> d_part_agent, d_part_index;  // action staging of the parts (one [N, A] pair, each part its rows)
  enum { EV_RING = 64 };
  hipEvent_t ev0[EV_RING] = {}, ev1[EV_RING] = {};  // ev0[i] .. ev1[i]: the k_rollout launch number i (mod EV_RING)
  unsigned long long n_rollouts = 0;
  bool timing_stale = false;  // a *_part rollout ran since the last whole-batch one: the event ring describes an older launch
  bool last_seeded = false;
  bool did_reset = false;
  std::vector<unsigned char> host_blobs, host_cold;  // cache for muavta_get
  bool host_valid = false;
  std::string err;
  // ---- state lanes (muavta_set_lanes) -----------------------------------------------------------------------------------------------
  // Everything above is ONE lane: the env records, tapes, observation buffers, metrics, streams, seeding slots and event rings of a batch.
  // A handle may own a second one (`hl.twin`, a complete MuavtaEnv of the same configuration that no caller ever sees): a seeded rollout
  // issued while the previous one is still running goes to the other lane — launch i + 1's workgroups start in the wave slots launch i's
  // early finishers free instead of waiting for its slowest env.  A flip SWAPS the two objects' contents (everything but `hl` and the
  // communicator), so every entry point keeps working on `*e` = the lane of the latest seeded rollout, without routing.
  int lane_id = 0;  // travels with the lane's contents
  struct HandleLevel {
    MuavtaEnv* twin = nullptr;
    int lanes_mode = 0;  // 0 auto (second lane on demand), 1 one lane only, 2 always alternate
    bool twin_failed = false;
    enum { RING = 64 };
    unsigned char ring_lane[RING] = {};         // rollout launch k (mod RING) of the HANDLE ran on this lane ...
    unsigned long long ring_no[RING] = {};      // ... as that lane's launch number
    unsigned long long n_launches = 0;
    std::vector<hipEvent_t> pending_waits;  // muavta_wait_stream events recorded while there was no second lane: one created later waits on them
    // muavta_set_pair_policy / muavta_set_context_pair_policy: the ONE installed policy — its packed weights (PW_* / PC_* layout by pol_kind) as the
    // caller last set them; a second lane created later gets its copy from here
    std::vector<float> pol_w;
    int pol_kind = POL_PAIR;
    int pol_raw = 0;
    float pol_clamp = 0.f;
    bool pol_set = false;
  } hl;
};
static int join_parts(MuavtaEnv* e);  // (sub-batches: defined with the other part helpers in front of the C ABI)
extern "C" int muavta_set_parts(MuavtaEnv* e, int32_t n_parts);
extern "C" int muavta_set_release_log(MuavtaEnv* e, int32_t enable);
extern "C" int muavta_create(const MuavtaParams* params, int32_t n_envs, int32_t device, MuavtaEnv** out);
extern "C" int muavta_destroy(MuavtaEnv* e);
extern "C" int muavta_set_slot_cap(MuavtaEnv* e, int32_t cap);
static int push_policy(MuavtaEnv* lane, const MuavtaEnv::HandleLevel& hl);

namespace {

template <class TL>
int launch_attr(MuavtaEnv* e) {
  size_t lds = Lds<TL>::bytes();
  e->lds_bytes = lds;
  if (lds > 48 * 1024) {
    const void* ks[] = {reinterpret_cast<const void*>(&k_reset<TL>), reinterpret_cast<const void*>(&k_step<TL>), reinterpret_cast<const void*>(&k_allocate<TL>),
                        reinterpret_cast<const void*>(&k_rollout<TL, false>), reinterpret_cast<const void*>(&k_rollout<TL, true>), reinterpret_cast<const void*>(&k_metrics<TL>), reinterpret_cast<const void*>(&k_observe<TL>),
                        reinterpret_cast<const void*>(&k_tokens<TL>), reinterpret_cast<const void*>(&k_call<TL>), reinterpret_cast<const void*>(&k_context<TL>),
                        reinterpret_cast<const void*>(&k_allocate<TL, true>), reinterpret_cast<const void*>(&k_rollout<TL, false, true>),
                        reinterpret_cast<const void*>(&k_pair_scores<TL>), reinterpret_cast<const void*>(&k_rollout<TL, false, false, true>),
                        reinterpret_cast<const void*>(&k_pair_scores<TL, true>), reinterpret_cast<const void*>(&k_rollout<TL, false, false, true, true>)};
    for (const void* k : ks) HIPCHK(e, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_allocate<TL, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds + SCORED_EXTRA_LDS));
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_allocate<TL, false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds + SCORED_EXTRA_LDS));
    HIPCHK(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_allocate_scored<TL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds + SCORED_EXTRA_LDS));
  }
  return MUAVTA_OK;
}

#define DISPATCH(e, CALL)                    \
  switch ((e)->tile) {                       \
    case TK16: { typedef Tile16 TL; CALL; } break; \
    case TK24: { typedef Tile24 TL; CALL; } break; \
    default:   { typedef Tile64 TL; CALL; } break; \
  }

int fill_dev_params(const MuavtaParams* p, DevParams* d, std::string* err) {
  memset(d, 0, sizeof(*d));
  if (p->abi_version != MUAVTA_ABI_VERSION) { *err = "abi_version mismatch"; return MUAVTA_E_ARG; }
  if (p->n_agent_groups < 1 || p->n_agent_groups > MUAVTA_MAX_GROUPS || p->n_task_groups < 0 || p->n_task_groups > MUAVTA_MAX_GROUPS ||
      p->n_threat_groups < 0 || p->n_threat_groups > MUAVTA_MAX_GROUPS) { *err = "group counts out of range"; return MUAVTA_E_ARG; }
  d->n_agent_groups = p->n_agent_groups; d->n_task_groups = p->n_task_groups; d->n_threat_groups = p->n_threat_groups;
  int nA = 0, nT = 0, nH = 0;
  double possible = 0;  // DroneEnv.py:670-675: summed over the static tasks only (Det tasks are created later, :685)
  for (int g = 0; g < p->n_agent_groups; g++) {
    if (p->agent_type[g] < 0 || p->agent_type[g] > MUAVTA_F2 || p->agent_count[g] < 0) { *err = "bad agent group"; return MUAVTA_E_ARG; }
    d->agent_type[g] = p->agent_type[g]; d->agent_count[g] = p->agent_count[g]; nA += p->agent_count[g];
  }
  for (int g = 0; g < p->n_task_groups; g++) {
    int ty = p->task_type[g];
    if (ty != MUAVTA_HOLD && ty != MUAVTA_REC && ty != MUAVTA_ATT) { *err = "static task types are Hold/Rec/Att"; return MUAVTA_E_ARG; }
    d->task_type[g] = ty; d->task_count[g] = p->task_count[g]; nT += p->task_count[g];
    for (int i = 0; i < p->task_count[g]; i++) possible += 1.0;
  }
  for (int g = 0; g < p->n_threat_groups; g++) {
    int ty = p->threat_type[g];
    if (ty != MUAVTA_T1 && ty != MUAVTA_T2) { *err = "threat types are T1/T2"; return MUAVTA_E_ARG; }
    d->threat_type[g] = ty; d->threat_count[g] = p->threat_count[g]; nH += p->threat_count[g];
  }
  if (nA < 1) { *err = "no agents"; return MUAVTA_E_ARG; }
  if (p->num_obstacles < 0 || p->num_obstacles > 8) { *err = "num_obstacles must be in 0..8"; return MUAVTA_E_ARG; }
  if (p->max_time_steps < 1) { *err = "max_time_steps must be >= 1"; return MUAVTA_E_ARG; }
  // (agent speeds = MAX_SPEED / frame_rate * 0.02 are divisors of the kernels' range-restricted division, see fdiv)
  if (!(p->simulation_frame_rate >= 1e-9 && p->simulation_frame_rate <= 1e9)) { *err = "simulation_frame_rate must be in [1e-9, 1e9]"; return MUAVTA_E_ARG; }
  // time steps, deadlines (t + window_length), reveal times (t + threat_delay), commit locks (t + commit_horizon) and task
  // ids (a few per step) are stored in 16 bits on the device
  if (p->max_time_steps > 20000 || p->window_length > 10000 || p->threat_delay > 10000 || p->commit_horizon > 10000 || p->window_length < -10000 ||
      p->threat_delay < -10000 || p->commit_horizon < -10000) { *err = "max_time_steps <= 20000 and window_length / threat_delay / commit_horizon within +-10000"; return MUAVTA_E_ARG; }
  d->n_agents = nA; d->n_tasks = nT + 1; d->max_tasks = d->n_tasks + 28; d->n_threats = nH;
  d->max_time_steps = p->max_time_steps; d->multiple_tasks_per_agent = p->multiple_tasks_per_agent;
  d->early_terminate = p->early_terminate; d->capability_mask = p->capability_mask; d->saturate_mask = p->saturate_mask;
  d->include_time_windows = p->include_time_windows; d->threat_delay = p->threat_delay; d->hard_windows = p->hard_windows;
  d->window_length = p->window_length; d->burst_mode = p->burst_mode; d->burst_size = p->burst_size;
  d->dual_region_bursts = p->dual_region_bursts; d->share_knowledge = p->share_knowledge; d->escort_enabled = p->escort_enabled;
  d->num_obstacles = p->num_obstacles; d->random_init_pos = p->random_init_pos;
  int need = (int)std::ceil(p->escort_requirement);
  d->escort_required_agents = need > 2 ? need : 2;
  d->escort_mask = p->escort_agent_type_mask;
  d->commit_horizon = p->commit_horizon;
  static const double MAX_SPEED[7] = {5.0, 8.0, 5.0, 20.0, 15.0, 14.0, 12.0};  // MultiDroneEnvData.py:32-38
  for (int t = 0; t < 7; t++) d->speed[t] = MAX_SPEED[t] / p->simulation_frame_rate * 0.02;
  d->threat_prob = 0.7 / p->simulation_frame_rate * 0.02;
  d->reward_norm_factor = (possible * 1 + possible) / 1000;
  // sqrt is correctly rounded and monotone, so `sqrt(v) <= r` is a threshold test on v; find the threshold
  auto sq_bound = [](double r) {
    double v = r * r;
    if (r > 0) {
      while (std::sqrt(v) > r) v = std::nextafter(v, 0.0);
      while (std::sqrt(std::nextafter(v, INFINITY)) <= r) v = std::nextafter(v, INFINITY);
    }
    return v;
  };
  d->sense_sq_bound = sq_bound(p->sense_radius);
  d->escort_sq_bound = sq_bound(p->escort_radius);
  d->fail_rate = p->fail_rate; d->arrival_rate = p->arrival_rate; d->dynamic_idle_penalty = p->dynamic_idle_penalty;
  d->sense_radius = p->sense_radius; d->miss_penalty = p->miss_penalty; d->on_time_bonus = p->on_time_bonus;
  d->reassign_penalty = p->reassign_penalty; d->escort_radius = p->escort_radius; d->escort_requirement = p->escort_requirement;
  d->escort_intercept_radius = p->escort_intercept_radius; d->mutual_support_radius = p->mutual_support_radius;
  for (int i = 0; i < 8; i++) d->rw[i] = p->reward_weights[i];
  d->rw_plain = d->reward_norm_factor > 0 ? 1 : 0;
  for (int i = 0; i < 8; i++) if (!(p->reward_weights[i] >= 0 && std::isfinite(p->reward_weights[i]))) d->rw_plain = 0;
  d->inv_mts = 1.0 / (double)(d->max_time_steps > 1 ? d->max_time_steps : 1);
  d->inv_max_tasks = 1.0 / (double)(d->max_tasks > 1 ? d->max_tasks : 1);
  return MUAVTA_OK;
}

}  // namespace

// ---- state lanes ----------------------------------------------------------------------------------------------------------------------
static void flip_lanes(MuavtaEnv* e) {  // the other lane's contents move into *e (and this one's into the twin)
  MuavtaEnv* t = e->hl.twin;
  std::swap(*e, *t);
  std::swap(e->hl, t->hl);  // (handle-level state and the RCCL communicator stay with the handle the caller holds)
  std::swap(e->comm, t->comm); std::swap(e->comm_rank, t->comm_rank); std::swap(e->comm_ranks, t->comm_ranks); std::swap(e->d_comm, t->d_comm);
}
static MuavtaEnv* lane_by_id(MuavtaEnv* e, int id) { return e->lane_id == id ? e : e->hl.twin; }
static int ensure_twin(MuavtaEnv* e) {  // create the second lane (same configuration, allocator, sub-batches, release log)
  if (e->hl.twin) return MUAVTA_OK;
  if (e->hl.twin_failed) return MUAVTA_E_HIP;
  MuavtaEnv* t = nullptr;
  int rc = muavta_create(&e->params, e->n_envs, e->device, &t);
  if (rc == MUAVTA_OK && e->n_parts) rc = muavta_set_parts(t, e->n_parts);
  if (rc == MUAVTA_OK && e->d_rel) rc = muavta_set_release_log(t, 1);
  if (rc == MUAVTA_OK) t->alloc_mode = e->alloc_mode;
  if (rc == MUAVTA_OK && e->hl.pol_set && push_policy(t, e->hl) != MUAVTA_OK) { e->err = t->err; rc = MUAVTA_E_HIP; }
  if (rc == MUAVTA_OK && e->P.slot_cap && muavta_set_slot_cap(t, e->P.slot_cap) != MUAVTA_OK) rc = MUAVTA_E_HIP;
  // the waits the caller queued before this lane existed hold for it too (its part streams fork from its main stream at their first launch)
  for (hipEvent_t ev : e->hl.pending_waits)
    if (rc == MUAVTA_OK && hipStreamWaitEvent(t->stream, ev, 0) != hipSuccess) rc = MUAVTA_E_HIP;
  if (rc != MUAVTA_OK) {  // the one failure exit: no half-made lane stays, and the handle does not try again
    if (t) muavta_destroy(t);
    e->hl.twin_failed = true;
    return rc;
  }
  for (hipEvent_t ev : e->hl.pending_waits) hipEventDestroy(ev);
  e->hl.pending_waits.clear();
  t->lane_id = e->lane_id ^ 1;
  t->hl.lanes_mode = 1;  // (a twin never grows a twin)
  e->hl.twin = t;
  return MUAVTA_OK;
}

// ---- sub-batches on their own streams (muavta_set_parts) ------------------------------------------------------------------
// Ordering between the handle's main stream and the part streams: an entry point that works on the main stream first makes it
// wait for whatever the part streams still hold (join_parts) and flags every part to wait for the main stream before its next
// launch (fork_part).  Both are event waits on the device: the host never blocks.
static int join_parts(MuavtaEnv* e) {
  for (int p = 0; p < e->n_parts; p++) {
    if (e->part_busy[p]) {
      HIPCHK(e, hipEventRecord(e->part_ev[p], e->part_stream[p]));
      HIPCHK(e, hipStreamWaitEvent(e->stream, e->part_ev[p], 0));
      e->part_busy[p] = false;
    }
    e->part_fork_needed[p] = true;
  }
  return MUAVTA_OK;
}
#define MAIN_OP(e) do { if ((e)->n_parts) { int rc_ = join_parts(e); if (rc_) return rc_; } } while (0)
static int fork_part(MuavtaEnv* e, int p) {
  if (e->part_fork_needed[p]) {
    HIPCHK(e, hipEventRecord(e->ev_fork, e->stream));
    HIPCHK(e, hipStreamWaitEvent(e->part_stream[p], e->ev_fork, 0));
    e->part_fork_needed[p] = false;
  }
  e->part_busy[p] = true;
  return MUAVTA_OK;
}
static void part_range(const MuavtaEnv* e, int p, int* first, int* count) {
  const long long N = e->n_envs, k = e->n_parts > 0 ? e->n_parts : 1;
  const int lo = (int)(N * p / k), hi = (int)(N * (p + 1) / k);
  *first = lo; *count = hi - lo;
}

// ---- where a call runs ---------------------------------------------------------------------------------------------------------------------
// The whole batch on the main stream (`part` null) or sub-batch *part on that part's stream.  An entry point validates (check_target; `who`
// names it in the message), enters the device scope and then opens the target, in this order.
struct Target {
  hipStream_t stream;
  int first, count;                // env range
  int32_t *act_agent, *act_index;  // action staging [N, A]: the handle's pair, or the parts' pair (each part its rows; env n is row n in either)
};
static int check_target(MuavtaEnv* e, const int32_t* part, const char* who) {
  if (!e) return MUAVTA_E_ARG;
  if (part && (e->n_parts < 1 || *part < 0 || *part >= e->n_parts)) { e->err = std::string(who) + ": no such part (muavta_set_parts first)"; return MUAVTA_E_ARG; }
  if (!e->did_reset) { e->err = std::string(who) + " before reset"; return MUAVTA_E_STATE; }
  return MUAVTA_OK;
}
// Orders the stream the call runs on — the main stream behind what the parts hold (MAIN_OP), or the part's stream behind the main stream
// (fork_part) — and says where that is.
static int open_target(MuavtaEnv* e, const int32_t* part, Target* t) {
  if (!part) {
    MAIN_OP(e);
    *t = {e->stream, 0, e->n_envs, e->d_act_agent, e->d_act_index};
    return MUAVTA_OK;
  }
  if (int rc = fork_part(e, *part)) return rc;
  *t = {e->part_stream[*part], 0, 0, e->d_part_agent, e->d_part_index};
  part_range(e, *part, &t->first, &t->count);
  return MUAVTA_OK;
}

// The staging buffer the host variants share (muavta_tokens, muavta_allocate_scored, muavta_pair_scores, muavta_context): at least `bytes`.
// Growing waits for the stream first: a launch still in flight may be reading the old buffer.
static int grow_staging(MuavtaEnv* e, size_t bytes) {
  if (bytes <= e->tok_bytes) return MUAVTA_OK;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->tok_bytes = 0;
  HIPCHK(e, e->d_tok.alloc(bytes));
  e->tok_bytes = bytes;
  return MUAVTA_OK;
}

// ====================================================================================================
// C ABI
// ====================================================================================================
extern "C" {

// sizeof() of the ABI structs, so a binding can verify its own layout: out[0] = MuavtaParams, out[1] = MuavtaDims
int muavta_abi_sizes(int32_t* out) {
  if (!out) return MUAVTA_E_ARG;
  out[0] = (int32_t)sizeof(MuavtaParams);
  out[1] = (int32_t)sizeof(MuavtaDims);
  out[2] = MUAVTA_ABI_VERSION;
  return MUAVTA_OK;
}

const char* muavta_last_error(const MuavtaEnv* env) { return env ? env->err.c_str() : g_create_error.c_str(); }

int muavta_create(const MuavtaParams* params, int32_t n_envs, int32_t device, MuavtaEnv** out) {
  if (!params || !out || n_envs < 1) { g_create_error = "muavta_create: bad arguments"; return MUAVTA_E_ARG; }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    g_create_error = "muavta_create: no HIP device visible; this library is the MI355X path and has no CPU fallback";
    return MUAVTA_E_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_create_error = "muavta_create: device index out of range"; return MUAVTA_E_ARG; }
  MuavtaEnv* e = new (std::nothrow) MuavtaEnv();
  if (!e) { g_create_error = "out of memory"; return MUAVTA_E_ARG; }
  int rc = fill_dev_params(params, &e->P, &g_create_error);
  if (rc) { delete e; return rc; }
  e->params = *params;
  e->n_envs = n_envs;
  e->device = device;
  int ta = params->tile_agents > e->P.n_agents ? params->tile_agents : e->P.n_agents;
  int tt = params->tile_tasks > 0 ? params->tile_tasks : 0;
  int th = params->tile_threats > e->P.n_threats ? params->tile_threats : e->P.n_threats;
  if (ta <= Tile16::A && tt <= Tile16::T && th <= Tile16::H) e->tile = TK16;
  else if (ta <= Tile24::A && tt <= Tile24::T && th <= Tile24::H) e->tile = TK24;
  else if (ta <= Tile64::A && tt <= Tile64::T && th <= Tile64::H) e->tile = TK64;
  else { g_create_error = "muavta_create: requested tile exceeds 64 agents x 128 task slots x 48 threats"; delete e; return MUAVTA_E_ARG; }
  e->P.slot_cap = 0;  // (live slots an env may use: the tile's; muavta_set_slot_cap lowers it for capacity tests)
  DISPATCH(e, { e->A = TL::A; e->T = TL::T; e->H = TL::H; e->E = TL::E; e->R = TL::R; e->Q = TL::Q; e->state_bytes = sizeof(EnvState<TL>);
                e->cold_bytes = sizeof(EnvCold<TL>); });
#define CK(expr) HIPCHK_G(expr, muavta_destroy(e))
  DeviceScope scope_(device);
  CK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  for (int i = 0; i < MuavtaEnv::EV_RING; i++) { CK(hipEventCreate(&e->ev0[i])); CK(hipEventCreate(&e->ev1[i])); }
  CK(hipStreamCreateWithFlags(&e->seed_stream, hipStreamNonBlocking));
  for (int b = 0; b < 2; b++) {
    CK(hipEventCreate(&e->ev_seed0[b])); CK(hipEventCreate(&e->ev_seeded[b])); CK(hipEventCreateWithFlags(&e->ev_consumed[b], hipEventDisableTiming));
  }
  // The sub-batch streams (muavta_set_parts) are created HERE, right behind the main and the seeding stream, and touched once:
  // HIP binds a stream to one of its few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) when the stream first gets work,
  // taking the least-loaded queue, and two streams on one queue execute in order.  Created lazily in the middle of a process'
  // life (after the framework's own streams, copy engines ...) two part streams could land on ONE queue: measured r3, two
  // sub-batches ran at 46 M env-steps/s inside bench.py against 70 M in a fresh process, with identical kernels.
  // (r4) Opt-in: MUAVTA_EAGER_PART_STREAMS=n (0..8, default 0) creates n of them here; the rest are created by muavta_set_parts when
  // they are first asked for.  A handle that never uses sub-batches owns two streams, not ten.
  {
    const char* ev = getenv("MUAVTA_EAGER_PART_STREAMS");
    int eager = ev ? atoi(ev) : 0;
    eager = eager < 0 ? 0 : eager > MuavtaEnv::MAX_PARTS ? MuavtaEnv::MAX_PARTS : eager;
    for (int p = 0; p < eager; p++) {
      CK(hipStreamCreateWithFlags(&e->part_stream[p], hipStreamNonBlocking));
      CK(hipEventCreateWithFlags(&e->part_ev[p], hipEventDisableTiming));
      CK(hipEventRecord(e->part_ev[p], e->part_stream[p]));
    }
  }
  CK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  const size_t N = (size_t)n_envs, mt = (size_t)e->P.max_tasks, nA = (size_t)e->P.n_agents;
  CK(e->blobs.alloc(N * e->state_bytes));
  CK(hipMemsetAsync(e->blobs, 0, N * e->state_bytes, e->stream));
  CK(e->cold.alloc(N * e->cold_bytes));
  CK(hipMemsetAsync(e->cold, 0, N * e->cold_bytes, e->stream));
  CK(e->tapes.alloc(N * MUAVTA_RNG_STREAMS * MUAVTA_RNG_WORDS * sizeof(uint32_t)));
  // zeroed like the blobs: without obstacles the obs stream is never seeded, yet every step prefetches its next eight words into
  // rng_win — whatever the allocation held would end up in get_state / get_rng, different from one handle to the next
  CK(hipMemsetAsync(e->tapes, 0, N * MUAVTA_RNG_STREAMS * MUAVTA_RNG_WORDS * sizeof(uint32_t), e->stream));
  for (int b = 0; b < 2; b++) {
    CK(e->d_seeds[b].alloc(N * sizeof(uint64_t)));
    CK(hipHostMalloc((void**)&e->h_seeds[b], N * sizeof(uint64_t), hipHostMallocDefault));
  }
  CK(e->d_act_agent.alloc(N * e->A * sizeof(int32_t)));
  CK(e->d_act_index.alloc(N * e->A * sizeof(int32_t)));
  CK(e->d_metrics.alloc(N * MUAVTA_N_METRICS * sizeof(double)));
  const size_t obs_bytes[7] = {N * mt * 21 * sizeof(float), N * nA * ((mt + 63) / 64) * sizeof(unsigned long long), N * mt, N * nA * 9 * sizeof(float),
                               N * 5 * sizeof(float), N * sizeof(double), N};  // tasks, legal, pad, agents, flags, reward, done
  for (int i = 0; i < 7; i++) CK(e->obs_mem[i].alloc(obs_bytes[i]));
  e->O.tasks = (float*)e->obs_mem[0].p; e->O.legal = (unsigned long long*)e->obs_mem[1].p; e->O.pad = (uint8_t*)e->obs_mem[2].p;
  e->O.agents = (float*)e->obs_mem[3].p; e->O.flags = (float*)e->obs_mem[4].p; e->O.reward = (double*)e->obs_mem[5].p; e->O.done = (uint8_t*)e->obs_mem[6].p;
  {
    DevCtx h;
    memset(&h, 0, sizeof(h));
    CK(e->d_pace.alloc((size_t)PACE_KEYS * 16 * sizeof(uint32_t)));
    CK(hipMemsetAsync(e->d_pace, 0, (size_t)PACE_KEYS * 16 * sizeof(uint32_t), e->stream));  // epoch 0 is never issued
    h.P = e->P; h.O = e->O; h.tapes = e->tapes; h.blobs = e->blobs; h.cold = e->cold; h.pace = e->d_pace;
    CK(e->d_rec.alloc(2 * MuavtaEnv::REC_SLOT));
    CK(hipMemsetAsync(e->d_rec, 0, 2 * MuavtaEnv::REC_SLOT, e->stream));
    CK(e->d_ctx.alloc(sizeof(DevCtx)));
    CK(hipMemcpyAsync(e->d_ctx, &h, sizeof(DevCtx), hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));  // `h` is a stack object
  }
#undef CK
  int arc = MUAVTA_OK;
  DISPATCH(e, arc = launch_attr<TL>(e));
  if (arc) { g_create_error = e->err; muavta_destroy(e); return arc; }
  *out = e;
  return MUAVTA_OK;
}

int muavta_destroy(MuavtaEnv* e) {
  if (!e) return MUAVTA_OK;
  muavta_comm_destroy(e);
  if (e->hl.twin) { muavta_destroy(e->hl.twin); e->hl.twin = nullptr; }
  DeviceScope scope_(e->device);
  for (hipEvent_t ev : e->hl.pending_waits) hipEventDestroy(ev);
  e->hl.pending_waits.clear();
  // whatever the handle's streams still hold completes before anything it uses is released
  if (e->seed_stream) hipStreamSynchronize(e->seed_stream);
  for (hipStream_t s : e->part_stream) if (s) hipStreamSynchronize(s);
  if (e->stream) hipStreamSynchronize(e->stream);
  for (int p = 0; p < MuavtaEnv::MAX_PARTS; p++) {
    if (e->part_stream[p]) hipStreamDestroy(e->part_stream[p]);
    if (e->part_ev[p]) hipEventDestroy(e->part_ev[p]);
  }
  if (e->ev_fork) hipEventDestroy(e->ev_fork);
  for (int i = 0; i < MuavtaEnv::EV_RING; i++) { if (e->ev0[i]) hipEventDestroy(e->ev0[i]); if (e->ev1[i]) hipEventDestroy(e->ev1[i]); }
  for (int b = 0; b < 2; b++) {
    if (e->ev_seed0[b]) hipEventDestroy(e->ev_seed0[b]);
    if (e->ev_seeded[b]) hipEventDestroy(e->ev_seeded[b]);
    if (e->ev_consumed[b]) hipEventDestroy(e->ev_consumed[b]);
    if (e->h_seeds[b]) hipHostFree(e->h_seeds[b]);
  }
  if (e->seed_stream) hipStreamDestroy(e->seed_stream);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;  // the device buffers go with their owners (DevBuf members), still inside the device scope
  return MUAVTA_OK;
}

int muavta_dims(const MuavtaEnv* e, MuavtaDims* d) {
  if (!e || !d) return MUAVTA_E_ARG;
  d->n_envs = e->n_envs; d->n_agents = e->P.n_agents; d->tile_agents = e->A; d->tile_tasks = e->T; d->tile_threats = e->H;
  d->max_tasks = e->P.max_tasks; d->obs_task_width = 21; d->obs_agent_width = 9; d->queue_cap = e->Q; d->event_cap = e->E;
  d->action_cap = e->A; d->state_bytes = (int64_t)(e->state_bytes + e->cold_bytes);
  d->n_threats = e->P.n_threats; d->known_words = (e->T + 31) / 32; d->lds_bytes = (int32_t)e->lds_bytes; d->legal_words = (e->P.max_tasks + 63) / 64;
  return MUAVTA_OK;
}

// Upload `seeds` and run the seeding kernel on the seed stream into the next slot; the handle's stream waits for it.
// The caller launches the consumer on e->stream and then records ev_consumed[slot] on it.
static int enqueue_seeding(MuavtaEnv* e, const uint64_t* seeds, const uint64_t** ds, const uint32_t** sb, int* slot) {
  const size_t N = (size_t)e->n_envs;
  const int b = (int)(e->seed_seq & 1u);  // (the slot sequence only advances once the kernel is queued: a failed call leaves it alone)
  if (e->seed_used[b]) {
    HIPCHK(e, hipEventSynchronize(e->ev_seeded[b]));                        // the staging copy of two calls ago has left h_seeds[b]
    HIPCHK(e, hipStreamWaitEvent(e->seed_stream, e->ev_consumed[b], 0));    // ... and its consumer has read d_seeds / d_seedbuf[b]
  }
  memcpy(e->h_seeds[b], seeds, N * sizeof(uint64_t));
  HIPCHK(e, hipMemcpyAsync(e->d_seeds[b], e->h_seeds[b], N * sizeof(uint64_t), hipMemcpyHostToDevice, e->seed_stream));
  const size_t seed_bytes = ((N + 15) / 16) * WG * 624 * sizeof(uint32_t);  // whole waves of 16 envs x 4 streams
  if (!e->d_seedbuf[b]) HIPCHK(e, e->d_seedbuf[b].alloc(seed_bytes));
  if (!e->d_seedtmp) HIPCHK(e, e->d_seedtmp.alloc(seed_bytes));  // k_seed's scratch (one: its launches are serialised on the seed stream)
  HIPCHK(e, hipEventRecord(e->ev_seed0[b], e->seed_stream));
  hipLaunchKernelGGL(k_seed, dim3((unsigned)((N + 15) / 16)), dim3(WG), 0, e->seed_stream, (const uint64_t*)e->d_seeds[b], (int)N,
                     (int)(e->P.num_obstacles > 0), e->d_seedbuf[b], e->d_seedtmp);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipEventRecord(e->ev_seeded[b], e->seed_stream));
  HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_seeded[b], 0));
  e->seed_used[b] = true;
  e->seed_seq++;
  e->last_seed_slot = b;
  *ds = e->d_seeds[b]; *sb = e->d_seedbuf[b]; *slot = b;
  return MUAVTA_OK;
}

// ---- sub-batches ---------------------------------------------------------------------------------------------------------
int muavta_set_parts(MuavtaEnv* e, int32_t n_parts) {
  if (!e || n_parts < 0 || n_parts > MuavtaEnv::MAX_PARTS || n_parts > e->n_envs) { if (e) e->err = "muavta_set_parts: 0 .. 8 parts, at most one per env"; return MUAVTA_E_ARG; }
  DeviceScope scope_(e->device);
  MAIN_OP(e);  // whatever the old parts hold is ordered in front of the main stream
  if (n_parts == 1) n_parts = 0;
  for (int p = 0; p < n_parts; p++) {
    if (!e->part_stream[p]) {  // (not among the MUAVTA_EAGER_PART_STREAMS created by muavta_create)
      HIPCHK(e, hipStreamCreateWithFlags(&e->part_stream[p], hipStreamNonBlocking));
      HIPCHK(e, hipEventCreateWithFlags(&e->part_ev[p], hipEventDisableTiming));
      HIPCHK(e, hipEventRecord(e->part_ev[p], e->part_stream[p]));
    }
    e->part_busy[p] = false; e->part_fork_needed[p] = true;
  }
  if (n_parts && !e->d_part_agent) {
    HIPCHK(e, e->d_part_agent.alloc((size_t)e->n_envs * e->A * sizeof(int32_t)));
    HIPCHK(e, e->d_part_index.alloc((size_t)e->n_envs * e->A * sizeof(int32_t)));
  }
  e->n_parts = n_parts;
  if (e->hl.twin) return muavta_set_parts(e->hl.twin, n_parts);
  return MUAVTA_OK;
}
int muavta_part_range(const MuavtaEnv* e, int32_t part, int32_t* first, int32_t* count) {
  if (!e || !first || !count || part < 0 || part >= (e->n_parts > 0 ? e->n_parts : 1)) return MUAVTA_E_ARG;
  int f, c;
  part_range(e, part, &f, &c);
  *first = f; *count = c;
  return MUAVTA_OK;
}
int muavta_wait_part(MuavtaEnv* e, int32_t part) {  // part < 0: every part
  if (!e || part >= e->n_parts) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  for (int p = 0; p < e->n_parts; p++)
    if (part < 0 || p == part) HIPCHK(e, hipStreamSynchronize(e->part_stream[p]));
  return MUAVTA_OK;
}

#ifdef MUAVTA_DIAG_TIMES
int muavta_diag_times(MuavtaEnv* e, uint32_t* out, int32_t n) {  // diagnostic build only: [3][n] start, end (10 ns units), hw ids
  DeviceScope scope_(e->device);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (int k = 0; k < 3; k++)
    HIPCHK(e, hipMemcpy(out + (size_t)k * n, e->d_pace + (1u << 19) + 65536u * k, (size_t)n * 4, hipMemcpyDeviceToHost));
  return MUAVTA_OK;
}
#endif
#ifdef MUAVTA_PROF
int muavta_prof_target(int env) { return hipMemcpyToSymbol(HIP_SYMBOL(g_prof_target), &env, sizeof(env)) == hipSuccess ? MUAVTA_OK : MUAVTA_E_HIP; }  // diagnostic build only
int muavta_prof_read(unsigned long long* out, int reset) {  // diagnostic build only
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), PROF_N * sizeof(unsigned long long)) != hipSuccess) return MUAVTA_E_HIP;
  if (reset) { unsigned long long z[PROF_N] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof(z)) != hipSuccess) return MUAVTA_E_HIP; }
  return MUAVTA_OK;
}
#endif

int muavta_sync(MuavtaEnv* e) {
  if (!e) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  if (e->hl.twin) { int rc = muavta_sync(e->hl.twin); if (rc) { e->err = e->hl.twin->err; return rc; } }  // everything queued on the handle: both lanes
  MAIN_OP(e);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

int muavta_wait_stream(MuavtaEnv* e, void* other_stream) {  // work queued on the handle from now on starts after what `other_stream` holds now
  if (!e) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  hipEvent_t ev = nullptr;
  HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t r = hipEventRecord(ev, (hipStream_t)other_stream);
  for (MuavtaEnv* L : {e, e->hl.twin}) {  // both lanes
    if (!L || r != hipSuccess) continue;
    r = hipStreamWaitEvent(L->stream, ev, 0);
    // sub-batches: a part's stream is ordered after the main stream's work at its next launch (fork_part), so the wait carries over
    for (int p = 0; p < L->n_parts; p++) L->part_fork_needed[p] = true;
  }
  if (r == hipSuccess && !e->hl.twin) {
    // no second lane yet: ensure_twin makes one created later wait on the event too.  Events whose work has completed order
    // nothing any more and are dropped here, so a caller that never gets a second lane keeps only the waits still in flight.
    auto& pw = e->hl.pending_waits;
    size_t k = 0;
    for (hipEvent_t w : pw) { if (hipEventQuery(w) == hipSuccess) hipEventDestroy(w); else pw[k++] = w; }
    (void)hipGetLastError();
    pw.resize(k);
    pw.push_back(ev);
    ev = nullptr;
  }
  if (ev) hipEventDestroy(ev);  // (destruction is deferred by the runtime until the event has completed)
  if (r != hipSuccess) { e->err = std::string("muavta_wait_stream: ") + hipGetErrorString(r); return MUAVTA_E_HIP; }
  return MUAVTA_OK;
}

int muavta_set_slot_cap(MuavtaEnv* e, int32_t cap) {  // test hook: an env may use at most `cap` of its tile's task slots (0: all of them)
  if (!e || cap < 0 || cap > e->T) { if (e) e->err = "muavta_set_slot_cap: 0 .. the tile's slot count"; return MUAVTA_E_ARG; }
  DeviceScope scope_(e->device);
  if (e->hl.twin) { int rc = muavta_set_slot_cap(e->hl.twin, cap); if (rc) { e->err = e->hl.twin->err; return rc; } }
  MAIN_OP(e);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->P.slot_cap = (cap > 0 && cap < e->T) ? cap : 0;
  HIPCHK(e, hipMemcpy((char*)e->d_ctx.p + offsetof(DevCtx, P) + offsetof(DevParams, slot_cap), &e->P.slot_cap, sizeof(int32_t), hipMemcpyHostToDevice));
  return MUAVTA_OK;
}
int muavta_set_lanes(MuavtaEnv* e, int32_t lanes) {
  if (!e || lanes < 0 || lanes > 2) { if (e) e->err = "muavta_set_lanes: 0 (second lane on demand), 1 (one lane) or 2 (always alternate)"; return MUAVTA_E_ARG; }
  DeviceScope scope_(e->device);
  if (lanes == 2) { int rc = ensure_twin(e); if (rc) { e->err = "muavta_set_lanes: the second lane could not be created: " + g_create_error; return rc; } }
  if (lanes == 1 && e->hl.twin) {  // back to one lane: the second lane's batch completes and its memory is released
    muavta_destroy(e->hl.twin);
    e->hl.twin = nullptr;
  }
  e->hl.lanes_mode = lanes;
  return MUAVTA_OK;
}
int muavta_lanes(const MuavtaEnv* e, int32_t* mode, int32_t* allocated) {
  if (!e) return MUAVTA_E_ARG;
  if (mode) *mode = e->hl.lanes_mode;
  if (allocated) *allocated = e->hl.twin ? 2 : 1;
  return MUAVTA_OK;
}

}  // extern "C"
