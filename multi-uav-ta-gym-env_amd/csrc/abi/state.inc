// State access through the C ABI.  Included by muavta_kernels.hip.
namespace {

int sync_host(MuavtaEnv* e) {
  if (e->host_valid) return MUAVTA_OK;
  if (e->n_parts) { int rc_ = join_parts(e); if (rc_) return rc_; }
  e->host_blobs.resize((size_t)e->n_envs * e->state_bytes);
  e->host_cold.resize((size_t)e->n_envs * e->cold_bytes);
  HIPCHK(e, hipMemcpyAsync(e->host_blobs.data(), e->blobs, e->host_blobs.size(), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->host_cold.data(), e->cold, e->host_cold.size(), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->host_valid = true;
  return MUAVTA_OK;
}

// Gather one field out of the host copy of the blobs.
template <class TL>
int gather(MuavtaEnv* e, MuavtaField f, void* dst, size_t bytes, bool scatter) {
  typedef EnvState<TL> St;
  const int N = e->n_envs, A = e->P.n_agents, T = TL::T, H = e->P.n_threats, Q = TL::Q, E = TL::E, KW = TL::KW;
  St* blobs = reinterpret_cast<St*>(e->host_blobs.data());
  EnvCold<TL>* cold = reinterpret_cast<EnvCold<TL>*>(e->host_cold.data());
  size_t need = 0;
  auto chk = [&](size_t n) { need = n; return bytes == n; };
  double* D = (double*)dst;
  int32_t* I = (int32_t*)dst;
  uint32_t* U = (uint32_t*)dst;
  auto QS = [&](int n) -> QueueSide<TL::A, TL::T, true>& {  // where this tile keeps next_free_* / orgReqs / doneReqs
    if constexpr (TL::SLIM) return static_cast<QueueSide<TL::A, TL::T, true>&>(cold[n]); else return static_cast<QueueSide<TL::A, TL::T, true>&>(blobs[n]);
  };
  auto TT = [&](int n) -> TaskTimes<TL::T, true>& {  // where this tile keeps initTime / doneTime
    if constexpr (TL::TIMES_LDS) return static_cast<TaskTimes<TL::T, true>&>(blobs[n]); else return static_cast<TaskTimes<TL::T, true>&>(cold[n]);
  };
#define BAD() do { e->err = "muavta_get/set: buffer size mismatch, need " + std::to_string(need) + " bytes"; return MUAVTA_E_ARG; } while (0)
#define RW(dstv, srcv) do { if (scatter) (srcv) = (dstv); else (dstv) = (srcv); } while (0)
  switch (f) {
    case MUAVTA_F_AGENT_POS:
      if (!chk((size_t)N * A * 2 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) { RW(D[((size_t)n * A + a) * 2], blobs[n].a_px[a]); RW(D[((size_t)n * A + a) * 2 + 1], blobs[n].a_py[a]); }
      break;
    case MUAVTA_F_AGENT_NFP:
      if (!chk((size_t)N * A * 2 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) { RW(D[((size_t)n * A + a) * 2], QS(n).a_nfx[a]); RW(D[((size_t)n * A + a) * 2 + 1], QS(n).a_nfy[a]); }
      break;
    case MUAVTA_F_AGENT_NFT:
      if (!chk((size_t)N * A * 8)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) RW(D[(size_t)n * A + a], QS(n).a_nft[a]);
      break;
    case MUAVTA_F_AGENT_DIST:
      if (!chk((size_t)N * A * 8)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) RW(D[(size_t)n * A + a], blobs[n].a_dist[a]);
      break;
    case MUAVTA_F_AGENT_CAPS:
      if (!chk((size_t)N * A * 6 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) for (int c = 0; c < 6; c++) RW(D[((size_t)n * A + a) * 6 + c], blobs[n].a_caps[c][a]);
      break;
    case MUAVTA_F_AGENT_STATE:
      if (!chk((size_t)N * A * 4)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) RW(I[(size_t)n * A + a], blobs[n].a_state[a]);
      break;
    case MUAVTA_F_AGENT_HEAD:
      if (!chk((size_t)N * A * 4)) BAD();
      if (scatter) { e->err = "AGENT_HEAD is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) I[(size_t)n * A + a] = blobs[n].a_qlen[a] > 0 ? blobs[n].a_qid[a][0] : 0;
      break;
    case MUAVTA_F_AGENT_QUEUE:
      if (!chk((size_t)N * A * Q * 4)) BAD();
      if (scatter) { e->err = "AGENT_QUEUE is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) for (int k = 0; k < Q; k++)
        I[((size_t)n * A + a) * Q + k] = k < blobs[n].a_qlen[a] ? blobs[n].a_qid[a][k] : (k == 0 ? 0 : -1);
      break;
    case MUAVTA_F_AGENT_ATTACK_CAP:
      if (!chk((size_t)N * A * 4)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) RW(I[(size_t)n * A + a], blobs[n].a_acap[a]);
      break;
    case MUAVTA_F_AGENT_TYPE:
      if (!chk((size_t)N * A * 4)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) RW(I[(size_t)n * A + a], blobs[n].a_type[a]);
      break;
    case MUAVTA_F_AGENT_NAME_IDX:
      if (!chk((size_t)N * A * 4)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) RW(I[(size_t)n * A + a], blobs[n].a_name[a]);
      break;
    case MUAVTA_F_AGENT_MISC:
      if (!chk((size_t)N * A * 6 * 4)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) {
        int32_t* r = I + ((size_t)n * A + a) * 6;
        RW(r[0], blobs[n].a_task_start[a]); RW(r[1], blobs[n].a_fail[a]); RW(r[2], blobs[n].a_reeval[a]);
        RW(r[3], blobs[n].a_last_id[a]); RW(r[4], blobs[n].a_commit[a]);
        if (!scatter) r[5] = blobs[n].a_qlen[a];
      }
      break;
    case MUAVTA_F_TASK_ID:
      if (!chk((size_t)N * T * 4)) BAD();
      if (scatter) { e->err = "TASK_ID is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) I[(size_t)n * T + s] = blobs[n].t_id[s];
      break;
    case MUAVTA_F_TASK_STATUS:
      if (!chk((size_t)N * T * 4)) BAD();
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) RW(I[(size_t)n * T + s], blobs[n].t_status[s]);
      break;
    case MUAVTA_F_TASK_POS:
      if (!chk((size_t)N * T * 2 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) { RW(D[((size_t)n * T + s) * 2], blobs[n].t_px[s]); RW(D[((size_t)n * T + s) * 2 + 1], blobs[n].t_py[s]); }
      break;
    case MUAVTA_F_TASK_CUR:
      if (!chk((size_t)N * T * 6 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) for (int c = 0; c < 6; c++) RW(D[((size_t)n * T + s) * 6 + c], cold[n].t_cur[c][s]);
      break;
    case MUAVTA_F_TASK_ALLOC:
      if (!chk((size_t)N * T * 6 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) for (int c = 0; c < 6; c++) RW(D[((size_t)n * T + s) * 6 + c], cold[n].t_alloc[c][s]);
      break;
    case MUAVTA_F_TASK_ORG_DONE:
      if (!chk((size_t)N * T * 2 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) { RW(D[((size_t)n * T + s) * 2], QS(n).t_org[s]); RW(D[((size_t)n * T + s) * 2 + 1], QS(n).t_done[s]); }
      break;
    case MUAVTA_F_TASK_TIMES:
      if (!chk((size_t)N * T * 2 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) { RW(D[((size_t)n * T + s) * 2], TT(n).t_init[s]); RW(D[((size_t)n * T + s) * 2 + 1], TT(n).t_dtime[s]); }
      break;
    case MUAVTA_F_TASK_META:
      if (!chk((size_t)N * T * 8 * 4)) BAD();
      for (int n = 0; n < N; n++) for (int s = 0; s < T; s++) {
        int32_t* r = I + ((size_t)n * T + s) * 8;
        St& b = blobs[n];
        if (scatter) { b.t_required[s] = r[3]; continue; }  // required_agents is the only field callers write (test_escort.py:107)
        r[0] = b.t_type[s]; r[1] = (b.t_flags[s] & TF_DEADLINE) ? b.t_deadline[s] : -1; r[2] = b.t_created[s]; r[3] = b.t_required[s];
        r[4] = (b.t_flags[s] & TF_ESCORT) ? 1 : 0; r[5] = b.t_ndet[s]; r[6] = b.t_prot_agent[s];
        r[7] = (b.t_flags[s] & TF_ELIGIBLE) ? (int32_t)b.t_elig[s] : -1;
      }
      break;
    case MUAVTA_F_KNOWN:
      if (!chk((size_t)N * A * KW * 4)) BAD();
      for (int n = 0; n < N; n++) for (int a = 0; a < A; a++) for (int w = 0; w < KW; w++) RW(U[((size_t)n * A + a) * KW + w], blobs[n].known[a][w]);
      if (scatter) for (int n = 0; n < N; n++) for (int sl = 0; sl < T; sl++) blobs[n].t_flags[sl] &= ~TF_KNOWN_ALL;  // caller-written masks: sense again
      break;
    case MUAVTA_F_THREAT_POS:
      if (!chk((size_t)N * H * 2 * 8)) BAD();
      for (int n = 0; n < N; n++) for (int h = 0; h < H; h++) { RW(D[((size_t)n * H + h) * 2], blobs[n].h_px[h]); RW(D[((size_t)n * H + h) * 2 + 1], blobs[n].h_py[h]); }
      break;
    case MUAVTA_F_THREAT_META:
      if (!chk((size_t)N * H * 8 * 4)) BAD();
      if (scatter) { e->err = "THREAT_META is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int h = 0; h < H; h++) {
        int32_t* r = I + ((size_t)n * H + h) * 8;
        St& b = blobs[n];
        r[0] = b.h_status[h]; r[1] = b.h_target[h]; r[2] = b.h_mission[h]; r[3] = b.h_acap[h]; r[4] = b.h_task_id[h]; r[5] = b.h_type[h];
        r[6] = b.h_group[h]; r[7] = b.h_intercept[h];
      }
      break;
    case MUAVTA_F_SCALARS:
      if (!chk((size_t)N * MUAVTA_N_SCALARS * 8)) BAD();
      if (scatter) { e->err = "SCALARS is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) {
        St& b = blobs[n];
        double* s = D + (size_t)n * MUAVTA_N_SCALARS;
        s[0] = b.time_steps; s[1] = b.last_reward; s[2] = b.F_Reward; s[3] = b.total_distance; s[4] = b.n_on_time;
        s[5] = b.n_missed_windows; s[6] = b.n_windowed_tasks; s[7] = b.n_task_switches; s[8] = b.n_reallocations;
        s[9] = b.n_arrivals; s[10] = b.idle_reserve_steps; s[11] = b.conclusion_time; s[12] = b.escort_requests;
        s[13] = b.escort_completed; s[14] = b.escort_failed; s[15] = b.escort_required_steps; s[16] = b.escort_covered_steps;
        s[17] = b.protection_breaches; s[18] = b.threats_intercepted; s[19] = b.recon_losses; s[20] = b.escort_losses;
        s[21] = b.mutual_support_engagements; s[22] = b.protected_rec_completed; s[23] = b.n_replans;
        s[24] = b.pending_reset; s[25] = b.n_reached; s[26] = b.n_pending; s[27] = b.next_task_id - 1;
      }
      break;
    case MUAVTA_F_OPEN_IDS:
      if (!chk((size_t)N * T * 4)) BAD();
      if (scatter) { e->err = "OPEN_IDS is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int k = 0; k < T; k++) I[(size_t)n * T + k] = k < blobs[n].n_open ? blobs[n].t_id[blobs[n].open_slot[k]] : -1;
      break;
    case MUAVTA_F_EVENTS:
      if (!chk((size_t)N * E * 2 * 4)) BAD();
      if (scatter) { e->err = "EVENTS is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int k = 0; k < E; k++) {
        I[((size_t)n * E + k) * 2] = k < blobs[n].n_dev ? blobs[n].dev_tag[k] : -1;
        I[((size_t)n * E + k) * 2 + 1] = k < blobs[n].n_dev ? blobs[n].dev_arg[k] : 0;
      }
      break;
    case MUAVTA_F_EVENT_LIST:
      if (!chk((size_t)N * E * 2 * 4)) BAD();
      if (scatter) { e->err = "EVENT_LIST is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int k = 0; k < E; k++) {
        I[((size_t)n * E + k) * 2] = k < blobs[n].n_events ? blobs[n].ev_tag[k] : -1;
        I[((size_t)n * E + k) * 2 + 1] = k < blobs[n].n_events ? blobs[n].ev_arg[k] : 0;
      }
      break;
    case MUAVTA_F_STAGED_ACTIONS:
      if (!chk((size_t)N * TL::A * 3 * 4)) BAD();
      if (scatter) { e->err = "STAGED_ACTIONS is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int k = 0; k < TL::A; k++) {
        St& b = blobs[n];
        int32_t* r = I + ((size_t)n * TL::A + k) * 3;
        bool v = k < b.n_act;
        r[0] = v ? b.act_agent[k] : -1; r[1] = v && b.act_slot[k] >= 0 ? b.t_id[b.act_slot[k]] : -1; r[2] = v ? b.act_index[k] : -1;
      }
      break;
    case MUAVTA_F_ERROR:
      if (!chk((size_t)N * 4)) BAD();
      if (scatter) { e->err = "ERROR is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) I[n] = blobs[n].error;
      break;
    case MUAVTA_F_ESCORTS:
      if (!chk((size_t)N * TL::A * 2 * 4)) BAD();
      if (scatter) { e->err = "ESCORTS is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++) for (int k = 0; k < TL::A; k++) {
        const bool v = k < blobs[n].n_escorts;
        I[((size_t)n * TL::A + k) * 2] = v ? blobs[n].esc_agent[k] : -1;
        I[((size_t)n * TL::A + k) * 2 + 1] = v ? blobs[n].esc_id[k] : -1;
      }
      break;
    case MUAVTA_F_KNOWN_COUNT:
      if (!chk((size_t)N * A * 4)) BAD();
      if (scatter) { e->err = "KNOWN_COUNT is read-only"; return MUAVTA_E_ARG; }
      for (int n = 0; n < N; n++)
        for (int a = 0; a < A; a++) {
          int c = blobs[n].a_gone[a];
          for (int w = 0; w < TL::KW; w++) c += __builtin_popcount(blobs[n].known[a][w]);
          I[(size_t)n * A + a] = c;
        }
      break;
    default:
      e->err = "unknown field";
      return MUAVTA_E_ARG;
  }
#undef BAD
#undef RW
  return MUAVTA_OK;
}

template <class TL>
void forget_obs_rows(MuavtaEnv* e) {  // the host rewrote the blobs: what the observation buffer holds no longer follows from them
  EnvState<TL>* blobs = reinterpret_cast<EnvState<TL>*>(e->host_blobs.data());
  for (int n = 0; n < e->n_envs; n++) blobs[n].obs_rows = -1;
}

template <class TL>
int check_errors(MuavtaEnv* e) {  // scan the per-env error words after a synchronising call
  typedef EnvState<TL> St;
  St* blobs = reinterpret_cast<St*>(e->host_blobs.data());
  for (int n = 0; n < e->n_envs; n++)
    if (blobs[n].error) {
      e->err = "env " + std::to_string(n) + " overflowed a tile (code " + std::to_string(blobs[n].error) +
               ": 1=task slots 2=agent queue 3=events 4=pending reveals 5=random_position 6=escorts 7=lsap)";
      return MUAVTA_E_CAPACITY;
    }
  return MUAVTA_OK;
}

}  // namespace

// muavta_set_pair_policy / muavta_set_context_pair_policy on ONE lane: the lane's copy of the weights, its scratch and the `pol` words of its
// context, on the lane's stream behind whatever it (and its part streams) still runs; synchronised, so the host vector may change afterwards.
// Both buffers are sized for the larger kind once, so a change of kind never frees memory that a queued launch may still read.
static int push_policy(MuavtaEnv* l, const MuavtaEnv::HandleLevel& hl) {
  DeviceScope scope_(l->device);
  MAIN_OP(l);
  PairPolicyDev pd;
  memset(&pd, 0, sizeof(pd));
  // the lane's weight buffer holds the largest kind; MLP-Pair and MLP-ContextPair share the scratch buffer of the larger block
  const size_t w_floats = PolCoalition::W::FLOATS, s_floats = PolContextPair::FLOATS, se_floats = PolCoalition::FLOATS;
  static_assert(PolCoalition::W::FLOATS >= PolContextPair::W::FLOATS && PolCoalition::W::FLOATS >= PolPair::W::FLOATS && PolContextPair::FLOATS >= PolPair::FLOATS,
                "buffer sizes");
  if (hl.pol_set) {
    if (!l->d_pol_w) HIPCHK(l, l->d_pol_w.alloc(w_floats * sizeof(float)));
    if (!l->d_pol_scratch) {
      HIPCHK(l, l->d_pol_scratch.alloc((size_t)l->n_envs * s_floats * sizeof(float)));
      HIPCHK(l, hipMemsetAsync(l->d_pol_scratch, 0, (size_t)l->n_envs * s_floats * sizeof(float), l->stream));
    }
    if (hl.pol_kind == POL_COALITION && !l->d_pol_scratch_e) {  // the escort-token block: only lanes that run this kind pay for it
      HIPCHK(l, l->d_pol_scratch_e.alloc((size_t)l->n_envs * se_floats * sizeof(float)));
      HIPCHK(l, hipMemsetAsync(l->d_pol_scratch_e, 0, (size_t)l->n_envs * se_floats * sizeof(float), l->stream));
    }
    const bool wide = hl.pol_kind != POL_COALITION && wide_pads(l);
    if (wide && !l->d_pol_scratch_w) {  // the 48 x 64 block: only lanes on which wide pads meet an MLP-Pair / MLP-ContextPair pay for it
      const size_t sw_floats = PolContextPairWide::FLOATS;
      static_assert(PolContextPairWide::FLOATS >= PolPairWide::FLOATS, "buffer sizes");
      HIPCHK(l, l->d_pol_scratch_w.alloc((size_t)l->n_envs * sw_floats * sizeof(float)));
      HIPCHK(l, hipMemsetAsync(l->d_pol_scratch_w, 0, (size_t)l->n_envs * sw_floats * sizeof(float), l->stream));
    }
    if (hl.pol_w.size() > w_floats) { l->err = "push_policy: packed weights larger than the lane's buffer"; return MUAVTA_E_ARG; }
    HIPCHK(l, hipMemcpyAsync(l->d_pol_w, hl.pol_w.data(), hl.pol_w.size() * sizeof(float), hipMemcpyHostToDevice, l->stream));
    pd.w = l->d_pol_w; pd.scratch = hl.pol_kind == POL_COALITION ? l->d_pol_scratch_e : wide ? l->d_pol_scratch_w : l->d_pol_scratch; pd.raw = hl.pol_raw; pd.clamp = hl.pol_clamp; pd.kind = hl.pol_kind;
  }
  HIPCHK(l, hipMemcpyAsync((char*)l->d_ctx.p + offsetof(DevCtx, pol), &pd, sizeof(pd), hipMemcpyHostToDevice, l->stream));
  HIPCHK(l, hipStreamSynchronize(l->stream));  // `pd` is a stack object
  l->pol_kind = hl.pol_set ? hl.pol_kind : POL_PAIR;
  return MUAVTA_OK;
}

// The two setters' common part.  `who`: the entry point's name; `packed` (non-empty: install): the weights in the kind's device layout.
// The handle holds ONE policy: either setter replaces whatever is installed, of either kind.
static int install_policy(MuavtaEnv* e, const char* who, bool clear, int kind, int raw, float clamp, std::vector<float>& packed) {
  // what the handle holds now: put back if the new policy does not reach BOTH lanes (the handle-level record must never say "set"
  // while a lane's context holds no, or another, policy)
  std::vector<float> old_w = e->hl.pol_w;
  const int old_raw = e->hl.pol_raw, old_kind = e->hl.pol_kind;
  const float old_clamp = e->hl.pol_clamp;
  const bool old_set = e->hl.pol_set;
  if (clear) {
    if (e->alloc_mode == MUAVTA_ALLOC_MLP_PAIR) {
      e->err = std::string(who) + ": the MLP-Pair allocator is selected; muavta_set_allocator to another mode before clearing its policy";
      return MUAVTA_E_STATE;
    }
    e->hl.pol_set = false;
    e->hl.pol_w.clear();
  } else {
    e->hl.pol_w.swap(packed);
    e->hl.pol_kind = kind; e->hl.pol_raw = raw; e->hl.pol_clamp = clamp; e->hl.pol_set = true;
  }
  int rc = push_policy(e, e->hl);
  if (rc == MUAVTA_OK && e->hl.twin) { rc = push_policy(e->hl.twin, e->hl); if (rc) e->err = e->hl.twin->err; }
  if (rc == MUAVTA_OK) return MUAVTA_OK;
  const std::string why = e->err;
  e->hl.pol_w.swap(old_w); e->hl.pol_raw = old_raw; e->hl.pol_kind = old_kind; e->hl.pol_clamp = old_clamp; e->hl.pol_set = old_set;
  int back = push_policy(e, e->hl);
  if (back == MUAVTA_OK && e->hl.twin) back = push_policy(e->hl.twin, e->hl);
  if (back != MUAVTA_OK) {  // not even the previous policy could be put back: no policy, and no mode that needs one
    e->hl.pol_set = false;
    e->hl.pol_w.clear();
    if (e->alloc_mode == MUAVTA_ALLOC_MLP_PAIR) { e->alloc_mode = MUAVTA_ALLOC_HUNGARIAN; if (e->hl.twin) e->hl.twin->alloc_mode = MUAVTA_ALLOC_HUNGARIAN; }
    e->err = std::string(who) + " failed (" + why + ") and the previous policy could not be restored: the handle has no policy now and runs the Hungarian allocator";
    return rc;
  }
  e->err = std::string(who) + " failed, the previous policy is kept: " + why;
  return rc;
}

// state_dict layout -> the device's (POL::W): layer 1 k-major with device row k taken from column col0(k); layer 2 in groups of four interleaved outputs
template <class POL, class Col0>
static std::vector<float> pack_policy(bool raw, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2, Col0 col0) {
  typedef typename POL::W LY;
  const int H = LY::HID, k0 = POL::np(raw) + POL::da(raw) + POL::dt(raw);
  std::vector<float> w(LY::FLOATS, 0.f);
  for (int n = 0; n < H; n++)
    for (int k = 0; k < k0; k++) w[LY::W0 + (size_t)k * H + n] = w0[(size_t)n * k0 + col0(k)];  // k-major on the device
  memcpy(&w[LY::B0], b0, H * sizeof(float));
  for (int n = 0; n < H; n++)
    for (int k = 0; k < H; k++) w[LY::W1 + ((size_t)(n / 4) * H + k) * 4 + n % 4] = w1[(size_t)n * H + k];  // four outputs interleaved
  memcpy(&w[LY::B1], b1, H * sizeof(float));
  memcpy(&w[LY::W2], w2, H * sizeof(float));
  w[LY::B2] = b2[0];
  return w;
}

extern "C" {

// ---- the learned MLP-Pair hybrid (sim/policy.inc) ---------------------------------------------------------------------------------
int muavta_set_pair_policy(MuavtaEnv* e, const MuavtaPairMlp* spec) {
  if (!e) return MUAVTA_E_ARG;
  std::vector<float> w;
  if (spec) {
    // raw_features is the MUAVTA_TOK_* kind the network consumes: 0 / 1 an MLP-Pair (hidden 128), MUAVTA_TOK_ESCORT an MLP-Coalition (hidden 256)
    const bool esc = spec->raw_features == MUAVTA_TOK_ESCORT;
    if (spec->hidden != (esc ? PolCoalition::W::HID : PolPair::W::HID) || (spec->raw_features != 0 && spec->raw_features != 1 && !esc) || !spec->w0 || !spec->b0 || !spec->w1 || !spec->b1 ||
        !spec->w2 || !spec->b2 || !(spec->score_clamp == spec->score_clamp)) {
      e->err = "muavta_set_pair_policy: bad spec (hidden must be 128, raw_features 0 or 1, six non-null arrays, score_clamp a number; "
               "or raw_features 2 = MUAVTA_TOK_ESCORT, an MLP-Coalition, with hidden 256)";
      return MUAVTA_E_ARG;
    }
    if (esc) w = pack_policy<PolCoalition>(false, spec->w0, spec->b0, spec->w1, spec->b1, spec->w2, spec->b2, [](int k) { return k; });
    else w = pack_policy<PolPair>(spec->raw_features != 0, spec->w0, spec->b0, spec->w1, spec->b1, spec->w2, spec->b2, [](int k) { return k; });
  }
  const bool esc = spec && spec->raw_features == MUAVTA_TOK_ESCORT;
  return install_policy(e, "muavta_set_pair_policy", !spec, esc ? POL_COALITION : POL_PAIR, spec && !esc ? spec->raw_features : 0, spec ? spec->score_clamp : 0.f, w);
}
// MLP-ContextPair: the same, with MLPContextPairNet.pair_mlp.  The state_dict's columns are the reference's cat — agent, task, a_pool,
// t_pool, context; the device's chain takes the env-uniform ones first (a_pool, t_pool, context, agent, task).
int muavta_set_context_pair_policy(MuavtaEnv* e, const MuavtaContextPairMlp* spec) {
  if (!e) return MUAVTA_E_ARG;
  std::vector<float> w;
  if (spec) {
    if (spec->hidden != PolContextPair::W::HID || (spec->raw_features != 0 && spec->raw_features != 1) || !spec->w0 || !spec->b0 || !spec->w1 || !spec->b1 || !spec->w2 ||
        !spec->b2 || !(spec->score_clamp == spec->score_clamp)) {
      e->err = "muavta_set_context_pair_policy: bad spec (hidden must be 192, raw_features 0 or 1, six non-null arrays, score_clamp a number)";
      return MUAVTA_E_ARG;
    }
    const bool raw = spec->raw_features != 0;
    const int pairw = PolContextPair::da(raw) + PolContextPair::dt(raw), np = PolContextPair::np(raw);  // agent + task columns; a_pool + t_pool + context columns
    w = pack_policy<PolContextPair>(raw, spec->w0, spec->b0, spec->w1, spec->b1, spec->w2, spec->b2, [=](int k) { return k < np ? k + pairw : k - np; });
  }
  return install_policy(e, "muavta_set_context_pair_policy", !spec, POL_CONTEXT_PAIR, spec ? spec->raw_features : 0, spec ? spec->score_clamp : 0.f, w);
}
int muavta_pair_scores_device(MuavtaEnv* e, float* scores, float* logits) {
  if (!e) return MUAVTA_E_ARG;
  if (!e->hl.pol_set) { e->err = "muavta_pair_scores: no policy (muavta_set_pair_policy first)"; return MUAVTA_E_STATE; }
  if (!e->did_reset) { e->err = "muavta_pair_scores before reset"; return MUAVTA_E_STATE; }
  if (!scores && !logits) return MUAVTA_OK;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  with_policy(e->pol_kind, wide_pads(e), [&](auto pol) {
    DISPATCH(e, if constexpr ((runs_on<TL, decltype(pol)>()))
                    hipLaunchKernelGGL((k_pair_scores<TL, decltype(pol)>), dim3(e->n_envs), dim3(WG), Lds<TL>::bytes(), e->stream, (const DevCtx*)e->d_ctx, scores, logits));
  });
  HIPCHK(e, hipGetLastError());
  return MUAVTA_OK;
}
int muavta_pair_scores(MuavtaEnv* e, float* scores, float* logits) {
  if (!e) return MUAVTA_E_ARG;
  if (!e->hl.pol_set) { e->err = "muavta_pair_scores: no policy (muavta_set_pair_policy first)"; return MUAVTA_E_STATE; }
  if (!e->did_reset) { e->err = "muavta_pair_scores before reset"; return MUAVTA_E_STATE; }
  DeviceScope scope_(e->device);
  const size_t one = with_policy(e->pol_kind, wide_pads(e), [e](auto pol) { typedef typename decltype(pol)::Blk B; return (size_t)e->n_envs * B::MA * B::MT * sizeof(float); });  // [N, 16, 32] (wide pads: [N, 48, 64]), MLP-Coalition: [N, 16, 48]
  if (int rc = grow_staging(e, 2 * one)) return rc;  // (shares the staging buffer of muavta_tokens' host variant)
  float* ds = (float*)e->d_tok.p;
  float* dl = (float*)((char*)e->d_tok.p + one);
  if (int rc = muavta_pair_scores_device(e, scores ? ds : nullptr, logits ? dl : nullptr)) return rc;
  if (scores) HIPCHK(e, hipMemcpyAsync(scores, ds, one, hipMemcpyDeviceToHost, e->stream));
  if (logits) HIPCHK(e, hipMemcpyAsync(logits, dl, one, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

// The observation of the last step, for the whole batch or a part's rows; waits for the target's stream.
static int observe_on(MuavtaEnv* e, const int32_t* part, const char* who, float* tasks, uint64_t* legal, uint8_t* pad, float* agents, float* flags, double* reward, uint8_t* done) {
  if (int rc = check_target(e, part, who)) return rc;
  DeviceScope scope_(e->device);
  Target t;
  if (int rc = open_target(e, part, &t)) return rc;
  hipStream_t st = t.stream;
  const size_t F = (size_t)t.first, C = (size_t)t.count, mt = (size_t)e->P.max_tasks, nA = (size_t)e->P.n_agents, kw = (mt + 63) / 64;
  if (tasks) HIPCHK(e, hipMemcpyAsync(tasks, e->O.tasks + F * mt * 21, C * mt * 21 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (legal) HIPCHK(e, hipMemcpyAsync(legal, e->O.legal + F * nA * kw, C * nA * kw * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (pad) HIPCHK(e, hipMemcpyAsync(pad, e->O.pad + F * mt, C * mt, hipMemcpyDeviceToHost, st));
  if (agents) HIPCHK(e, hipMemcpyAsync(agents, e->O.agents + F * nA * 9, C * nA * 9 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (flags) HIPCHK(e, hipMemcpyAsync(flags, e->O.flags + F * 5, C * 5 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (reward) HIPCHK(e, hipMemcpyAsync(reward, e->O.reward + F, C * sizeof(double), hipMemcpyDeviceToHost, st));
  if (done) HIPCHK(e, hipMemcpyAsync(done, e->O.done + F, C, hipMemcpyDeviceToHost, st));
  HIPCHK(e, hipStreamSynchronize(st));
  return MUAVTA_OK;
}
int muavta_observe(MuavtaEnv* e, float* tasks, uint64_t* legal, uint8_t* pad, float* agents, float* flags) {
  return observe_on(e, nullptr, "observe", tasks, legal, pad, agents, flags, nullptr, nullptr);
}
int muavta_observe_part(MuavtaEnv* e, int32_t part, float* tasks, uint64_t* legal, uint8_t* pad, float* agents, float* flags, double* reward, uint8_t* done) {
  return observe_on(e, &part, "muavta_observe_part", tasks, legal, pad, agents, flags, reward, done);
}

// ---- token builders (SURVEY §8f rank 2) --------------------------------------------------------------------------
static int token_dims(int kind, int* dt, int* da) {
  if (kind == MUAVTA_TOK_PAIR) { *dt = 13; *da = 12; }
  else if (kind == MUAVTA_TOK_PAIR_RAW) { *dt = 9; *da = 11; }
  else if (kind == MUAVTA_TOK_ESCORT) { *dt = 22; *da = 16; }
  else return MUAVTA_E_ARG;
  return MUAVTA_OK;
}
int muavta_tokens_device(MuavtaEnv* e, int32_t kind, int32_t max_tasks, int32_t max_agents, float* task_feats, uint8_t* task_mask,
                         int32_t* task_ids, float* agent_feats, uint8_t* agent_mask, int32_t* agent_ids, float* edge_valid, int32_t* n_urgent,
                         float* expert_mask, int32_t* replanned) {
  int dt, da;
  const TokOut out{task_feats, task_mask, task_ids, agent_feats, agent_mask, agent_ids, edge_valid, n_urgent, expert_mask, replanned};
  if (!e || token_dims(kind, &dt, &da) || max_tasks < 1 || max_agents < 1 || max_tasks > 4096 || max_agents > 4096 || !out.complete()) {
    if (e) e->err = "muavta_tokens: bad argument"; return MUAVTA_E_ARG;
  }
  if (!e->did_reset) { e->err = "tokens before reset"; return MUAVTA_E_STATE; }
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  DISPATCH(e, launch_tokens<TL>(e, out, kind, max_tasks, max_agents));
  HIPCHK(e, hipGetLastError());
  return MUAVTA_OK;
}
int muavta_tokens(MuavtaEnv* e, int32_t kind, int32_t max_tasks, int32_t max_agents, float* task_feats, uint8_t* task_mask,
                  int32_t* task_ids, float* agent_feats, uint8_t* agent_mask, int32_t* agent_ids, float* edge_valid, int32_t* n_urgent,
                  float* expert_mask, int32_t* replanned) {
  int dt, da;
  if (!e || token_dims(kind, &dt, &da) || max_tasks < 1 || max_agents < 1) { if (e) e->err = "muavta_tokens: bad argument"; return MUAVTA_E_ARG; }
  DeviceScope scope_(e->device);
  const size_t N = (size_t)e->n_envs, MT = (size_t)max_tasks, MA = (size_t)max_agents;
  const size_t sz[10] = {N * MT * dt * 4, N * MT, N * MT * 4, N * MA * da * 4, N * MA, N * MA * 4, N * MA * MT * 4, N * 4, N * MA * MT * 4, N * 4};
  size_t off[11] = {0};
  for (int i = 0; i < 10; i++) off[i + 1] = off[i] + ((sz[i] + 255) & ~(size_t)255);
  if (int rc = grow_staging(e, off[10])) return rc;
  char* b = (char*)e->d_tok.p;
  int rc = muavta_tokens_device(e, kind, max_tasks, max_agents, (float*)(b + off[0]), (uint8_t*)(b + off[1]), (int32_t*)(b + off[2]),
                                (float*)(b + off[3]), (uint8_t*)(b + off[4]), (int32_t*)(b + off[5]), (float*)(b + off[6]), (int32_t*)(b + off[7]),
                                expert_mask ? (float*)(b + off[8]) : nullptr, replanned ? (int32_t*)(b + off[9]) : nullptr);
  if (rc) return rc;
  void* host[10] = {task_feats, task_mask, task_ids, agent_feats, agent_mask, agent_ids, edge_valid, n_urgent, expert_mask, replanned};
  for (int i = 0; i < 10; i++)
    if (host[i]) HIPCHK(e, hipMemcpyAsync(host[i], b + off[i], sz[i], hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

int muavta_context_device(MuavtaEnv* e, int32_t kind, int32_t max_tasks, float* context) {
  if (!e || !context || (kind != MUAVTA_TOK_PAIR && kind != MUAVTA_TOK_PAIR_RAW) || max_tasks < 1 || max_tasks > 4096) {
    if (e) e->err = "muavta_context: kind MUAVTA_TOK_PAIR (8 floats per env) or MUAVTA_TOK_PAIR_RAW (1), max_tasks >= 1"; return MUAVTA_E_ARG;
  }
  if (!e->did_reset) { e->err = "context before reset"; return MUAVTA_E_STATE; }
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  DISPATCH(e, hipLaunchKernelGGL(k_context<TL>, dim3(e->n_envs), dim3(WG), Lds<TL>::bytes(), e->stream, (const DevCtx*)e->d_ctx, (int)(kind == MUAVTA_TOK_PAIR_RAW), max_tasks, context));
  HIPCHK(e, hipGetLastError());
  return MUAVTA_OK;
}
int muavta_context(MuavtaEnv* e, int32_t kind, int32_t max_tasks, float* context) {
  if (!e || !context) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  const size_t bytes = (size_t)e->n_envs * (kind == MUAVTA_TOK_PAIR_RAW ? 1 : 8) * sizeof(float);
  if (int rc = grow_staging(e, bytes)) return rc;  // (shares the staging buffer of muavta_tokens' host variant)
  if (int rc = muavta_context_device(e, kind, max_tasks, (float*)e->d_tok.p)) return rc;
  HIPCHK(e, hipMemcpyAsync(context, e->d_tok, bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

int muavta_call(MuavtaEnv* e, int32_t env_index, int32_t op, const int32_t* iargs, double darg, int32_t* out) {
  if (!e || !out || op < 0 || op >= MUAVTA_OP_COUNT_ || env_index < 0 || env_index >= e->n_envs) { if (e) e->err = "muavta_call: bad argument"; return MUAVTA_E_ARG; }
  if (!e->did_reset) { e->err = "muavta_call before reset"; return MUAVTA_E_STATE; }
  CallArgs a;
  memset(&a, 0, sizeof(a));
  a.op = op; a.env = env_index; a.d = darg;
  if (iargs) memcpy(a.i, iargs, sizeof(a.i));
  const bool has_agent = op != MUAVTA_OP_SYNC_ESCORTS && op != MUAVTA_OP_RETIRE_ESCORT;
  if (has_agent && (a.i[0] < 0 || a.i[0] >= e->P.n_agents)) { e->err = "muavta_call: agent id out of range"; return MUAVTA_E_ARG; }
  if (op == MUAVTA_OP_SET_QUEUE && (a.i[1] < 0 || a.i[1] > 6)) { e->err = "muavta_call(SET_QUEUE): at most 6 tasks"; return MUAVTA_E_ARG; }
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  if (!e->d_call_out) HIPCHK(e, e->d_call_out.alloc(MUAVTA_CALL_OUT * sizeof(int32_t)));
  DISPATCH(e, hipLaunchKernelGGL(k_call<TL>, dim3(1), dim3(WG), Lds<TL>::bytes(), e->stream, (const DevCtx*)e->d_ctx, a, e->d_call_out));
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(out, e->d_call_out, MUAVTA_CALL_OUT * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->host_valid = false;
  return MUAVTA_OK;
}

int muavta_refresh_observation(MuavtaEnv* e) {  // rebuild the obs tensors from the current state (after muavta_set)
  if (!e) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  DISPATCH(e, hipLaunchKernelGGL(k_observe<TL>, dim3(e->n_envs), dim3(WG), Lds<TL>::bytes(), e->stream, (const DevCtx*)e->d_ctx));
  HIPCHK(e, hipGetLastError());
  e->host_valid = false;  // (the kernel refreshes the derived initTime / doneTime rows of the HBM record)
  return MUAVTA_OK;
}

int muavta_step_result(MuavtaEnv* e, double* reward, uint8_t* done) {
  if (!e) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  if (reward) HIPCHK(e, hipMemcpyAsync(reward, e->O.reward, (size_t)e->n_envs * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (done) HIPCHK(e, hipMemcpyAsync(done, e->O.done, (size_t)e->n_envs, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

int muavta_metrics(MuavtaEnv* e, double* out) {
  if (!e || !out) return MUAVTA_E_ARG;
  if (!e->did_reset) { e->err = "metrics before reset"; return MUAVTA_E_STATE; }
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  DISPATCH(e, hipLaunchKernelGGL(k_metrics<TL>, dim3(e->n_envs), dim3(WG), Lds<TL>::bytes(), e->stream, (const DevCtx*)e->d_ctx, e->d_metrics));
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(out, e->d_metrics, (size_t)e->n_envs * MUAVTA_N_METRICS * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  int rc = sync_host(e);
  if (rc) return rc;
  DISPATCH(e, rc = check_errors<TL>(e));
  return rc;
}

int muavta_get(MuavtaEnv* e, MuavtaField field, void* dst, size_t bytes) {
  if (!e || !dst) return MUAVTA_E_ARG;
  if (field == MUAVTA_F_TOKEN_PADS) {  // a setting of the handle: no env record is read
    if (bytes != 2 * sizeof(int32_t)) { e->err = "muavta_get(TOKEN_PADS): i32 [2], 8 bytes"; return MUAVTA_E_ARG; }
    const int32_t pads[2] = {e->pad_t, e->pad_a};
    memcpy(dst, pads, sizeof(pads));
    return MUAVTA_OK;
  }
  DeviceScope scope_(e->device);
  if (field == MUAVTA_F_RELEASE_LOG) {
    const size_t want = (size_t)e->n_envs * (1 + MUAVTA_REL_ROW * e->T) * sizeof(double);
    if (!e->d_rel) { e->err = "release log is off (muavta_set_release_log)"; return MUAVTA_E_STATE; }
    if (bytes != want) { e->err = "muavta_get(RELEASE_LOG): wrong size"; return MUAVTA_E_ARG; }
    MAIN_OP(e);
    HIPCHK(e, hipMemcpyAsync(dst, e->d_rel, want, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MUAVTA_OK;
  }
  int rc = sync_host(e);
  if (rc) return rc;
  DISPATCH(e, rc = gather<TL>(e, field, dst, bytes, false));
  return rc;
}

int muavta_set(MuavtaEnv* e, MuavtaField field, const void* src, size_t bytes) {
  if (!e || !src) return MUAVTA_E_ARG;
  if (field == MUAVTA_F_TOKEN_PADS) {  // a setting of the handle: no env record is written
    if (bytes != 2 * sizeof(int32_t)) { e->err = "muavta_set(TOKEN_PADS): i32 [2], 8 bytes"; return MUAVTA_E_ARG; }
    int32_t pads[2];
    memcpy(pads, src, sizeof(pads));
    return set_token_pads(e, pads[0], pads[1]);
  }
  DeviceScope scope_(e->device);
  int rc = sync_host(e);
  if (rc) return rc;
  DISPATCH(e, rc = gather<TL>(e, field, const_cast<void*>(src), bytes, true));
  if (rc) return rc;
  DISPATCH(e, forget_obs_rows<TL>(e));
  HIPCHK(e, hipMemcpyAsync(e->blobs, e->host_blobs.data(), e->host_blobs.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->cold, e->host_cold.data(), e->host_cold.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

int muavta_get_state(MuavtaEnv* e, void* dst, size_t bytes) {  // [N x EnvState | N x EnvCold]
  if (!e || !dst || bytes != (size_t)e->n_envs * (e->state_bytes + e->cold_bytes)) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  HIPCHK(e, hipMemcpyAsync(dst, e->blobs, (size_t)e->n_envs * e->state_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync((char*)dst + (size_t)e->n_envs * e->state_bytes, e->cold, (size_t)e->n_envs * e->cold_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}
int muavta_set_state(MuavtaEnv* e, const void* src, size_t bytes) {
  if (!e || !src || bytes != (size_t)e->n_envs * (e->state_bytes + e->cold_bytes)) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  e->host_blobs.assign((const unsigned char*)src, (const unsigned char*)src + (size_t)e->n_envs * e->state_bytes);
  DISPATCH(e, forget_obs_rows<TL>(e));  // (the observation buffer belongs to another moment than the restored state)
  HIPCHK(e, hipMemcpyAsync(e->blobs, e->host_blobs.data(), (size_t)e->n_envs * e->state_bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->cold, (const char*)src + (size_t)e->n_envs * e->state_bytes, (size_t)e->n_envs * e->cold_bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->host_valid = false;
  e->did_reset = true;
  return MUAVTA_OK;
}
int muavta_get_rng(MuavtaEnv* e, void* dst, size_t bytes) {  // raw MT tapes, for checkpoint/resume next to get_state
  size_t need = e ? (size_t)e->n_envs * MUAVTA_RNG_STREAMS * MUAVTA_RNG_WORDS * 4 : 0;
  if (!e || !dst || bytes != need) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  HIPCHK(e, hipMemcpyAsync(dst, e->tapes, bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}
int muavta_set_rng(MuavtaEnv* e, const void* src, size_t bytes) {
  size_t need = e ? (size_t)e->n_envs * MUAVTA_RNG_STREAMS * MUAVTA_RNG_WORDS * 4 : 0;
  if (!e || !src || bytes != need) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  HIPCHK(e, hipMemcpyAsync(e->tapes, src, bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

int muavta_device_ptrs(MuavtaEnv* e, void** state, void** obs_tasks, void** obs_legal, void** obs_agents, void** metrics, void** stream) {
  if (!e) return MUAVTA_E_ARG;
  if (state) *state = e->blobs;
  if (obs_tasks) *obs_tasks = e->O.tasks;
  if (obs_legal) *obs_legal = e->O.legal;
  if (obs_agents) *obs_agents = e->O.agents;
  if (metrics) *metrics = e->d_metrics;
  if (stream) *stream = (void*)e->stream;
  return MUAVTA_OK;
}

int muavta_rollout_metrics(MuavtaEnv* e, double* out) {  // metrics written by the last muavta_rollout (no extra kernel)
  if (!e || !out) return MUAVTA_E_ARG;
  DeviceScope scope_(e->device);
  MAIN_OP(e);
  HIPCHK(e, hipMemcpyAsync(out, e->d_metrics, (size_t)e->n_envs * MUAVTA_N_METRICS * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return MUAVTA_OK;
}

// the lane that holds the rollout launched just before the latest one, if that launch ran on the OTHER lane (else nullptr: overwritten)
static MuavtaEnv* prev_batch_lane(MuavtaEnv* e) {
  if (!e->hl.twin || e->hl.n_launches < 2) return nullptr;
  const int R = MuavtaEnv::HandleLevel::RING;
  const int last = e->hl.ring_lane[(e->hl.n_launches - 1) % R], prev = e->hl.ring_lane[(e->hl.n_launches - 2) % R];
  if (last == prev) return nullptr;
  MuavtaEnv* t = lane_by_id(e, prev);
  return (t && t != e && t->n_rollouts == e->hl.ring_no[(e->hl.n_launches - 2) % R] + 1) ? t : nullptr;  // (and nothing else was launched on that lane since)
}
int muavta_rollout_metrics_back(MuavtaEnv* e, int32_t back, double* out) {  // back 0: the last seeded batch (= muavta_rollout_metrics); 1: the one before it, on the other lane
  if (!e || !out || back < 0 || back > 1) return MUAVTA_E_ARG;
  if (back == 0) return muavta_rollout_metrics(e, out);
  MuavtaEnv* t = prev_batch_lane(e);
  if (!t) { e->err = "muavta_rollout_metrics_back: the batch before the latest one is gone — it ran on the same lane (the latest rollout found it finished, or there is one lane only); muavta_set_lanes(h, 2) makes seeded rollouts always alternate"; return MUAVTA_E_STATE; }
  int rc = muavta_rollout_metrics(t, out);
  if (rc) e->err = t->err;
  return rc;
}
int muavta_error_flags_back(MuavtaEnv* e, int32_t back, int32_t* out) {  // MUAVTA_F_ERROR of the batch `back` launches ago (0 or 1)
  if (!e || !out || back < 0 || back > 1) return MUAVTA_E_ARG;
  MuavtaEnv* L = back == 0 ? e : prev_batch_lane(e);
  if (!L) { e->err = "muavta_error_flags_back: the batch before the latest one is gone (it ran on the same lane)"; return MUAVTA_E_STATE; }
  int rc = muavta_get(L, MUAVTA_F_ERROR, out, (size_t)L->n_envs * sizeof(int32_t));
  if (rc && L != e) e->err = L->err;
  return rc;
}

}  // extern "C"
