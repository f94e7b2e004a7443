// sim/entities.inc — member functions of Sim<TL> (muavta_device.h includes this file INSIDE the struct body): entity bookkeeping: task references and agent queues, task creation / release, events, the escort subsystem, releaseAllTasks, geometry helpers.
  // ---------------------------------------------------------------- references & queues (lane 0)
  DEV bool ref_valid(int id, int slot) const { return slot >= 0 && S.t_id[slot] == id; }
  DEV bool ref_retired(int id, int slot) const { return !ref_valid(id, slot) || S.t_status[slot] == 2; }
  DEV int head_id(int a) const { return S.a_qlen[a] > 0 ? S.a_qid[a][0] : 0; }
  DEV int queue_find(int a, int id) const {
    // every entry of the row is read at once (entries beyond the queue's length are stale but in bounds) and the first
    // match picked from a bit mask: one LDS round trip instead of one per entry
    const int n = S.a_qlen[a];
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < Q; k++) m |= (unsigned)(S.a_qid[a][k] == id) << k;
    m &= (1u << n) - 1u;
    return m ? __ffs((int)m) - 1 : -1;
  }
  DEV void queue_erase(int a, int k) {
    const int n = S.a_qlen[a];
    for (int i = k; i + 1 < n; i++) {
      S.a_qid[a][i] = S.a_qid[a][i + 1];
      S.a_qslot[a][i] = S.a_qslot[a][i + 1];
    }
    // the travel times live in the HBM record: up to four entries per pass with all the loads in front of the stores — a
    // load-then-store per entry is one memory round trip (~1 us) per entry on this serial path
    for (int i = k; i + 1 < n; i += 4) {
      const int r = n - 1 - i;
      double t0 = 0, t1 = 0, t2 = 0, t3 = 0;
      if (r >= 1) t0 = C.a_qtime[a][i + 1];
      if (r >= 2) t1 = C.a_qtime[a][i + 2];
      if (r >= 3) t2 = C.a_qtime[a][i + 3];
      if (r >= 4) t3 = C.a_qtime[a][i + 4];
      if (r >= 1) C.a_qtime[a][i] = t0;
      if (r >= 2) C.a_qtime[a][i + 1] = t1;
      if (r >= 3) C.a_qtime[a][i + 2] = t2;
      if (r >= 4) C.a_qtime[a][i + 3] = t3;
    }
    S.a_qlen[a] = n - 1;
  }
  DEV bool escort_type(int t) const { return (P.escort_mask >> t) & 1u; }

  // Task.removeAgentCap (DroneEnvComponents.py:280-301).  The agent's own queue entry must already be gone.
  // initTime / doneTime are NOT maintained incrementally: the reference's upkeep keeps the invariants
  // initTime == min(details times), doneTime == max(details times) + duration (or -1, -1 when empty), and
  // details == the agents' queue entries, so refresh_task_times() rebuilds them per step in one parallel pass.
  DEV void remove_agent_cap(int s, int a) {
    if (S.t_status[s] == 2) return;
    for (int c = 0; c < 6; c++) C.t_alloc[c][s] -= S.a_caps[c][a];
    S.t_ndet[s] -= 1;
    S.times_dirty = 1; obs_static_clear();
  }
  // UAV.desAllocate (DroneEnvComponents.py:97-113) for a task id that IS in the queue at position k.
  DEV void des_allocate_at(int a, int k) {
    int id = S.a_qid[a][k], slot = S.a_qslot[a][k];
    queue_erase(a, k);
    qs().a_nft[a] = (double)tnow;
    qs().a_nfx[a] = S.a_px[a];
    qs().a_nfy[a] = S.a_py[a];
    S.a_commit[a] = 0;
    if (ref_valid(id, slot)) remove_agent_cap(slot, a);
  }
  DEV bool des_allocate(int a, int id) {
    int k = queue_find(a, id);
    if (k < 0 || id == 0) return false;
    des_allocate_at(a, k);
    return true;
  }
  // `for task in self.tasks: self.desAllocate(task)` over the list being mutated
  // (DroneEnvComponents.py:115-119,122-127): every other queued task survives.
  DEV void iterate_desallocate(int a) {
    int i = 0;
    while (i < S.a_qlen[a]) {
      des_allocate_at(a, i);
      if (S.a_qlen[a] == 0) break;  // python rebinds tasks=[idle]; the running iterator sees an empty list
      i++;
    }
  }
  DEV void desallocate_all(int a) { iterate_desallocate(a); S.a_commit[a] = 0; }
  DEV void out_of_service(int a) { S.a_state[a] = -1; S.a_commit[a] = 0; iterate_desallocate(a); }

  // UAV.taskDone (DroneEnvComponents.py:143-179)
  DEV bool task_done(int a, int id, int type) {
    if (S.a_qlen[a] == 0 || S.a_qid[a][0] != id) return false;
    queue_erase(a, 0);
    S.a_task_start[a] = -1;
    if (type == MUAVTA_ATT) {
      S.a_acap[a] -= 1;
      if (S.a_acap[a] <= 0) S.a_caps[MUAVTA_ATT][a] = 0;
    }
    while (S.a_qlen[a] > 0 && ref_retired(S.a_qid[a][0], S.a_qslot[a][0])) queue_erase(a, 0);
    if (S.a_qlen[a] == 0) {
      if (S.a_reeval[a]) { S.a_last_id[a] = -1; S.a_last_slot[a] = -1; S.a_reeval[a] = 0; }
      qs().a_nft[a] = 0;
      qs().a_nfx[a] = S.a_px[a];
      qs().a_nfy[a] = S.a_py[a];
      S.a_state[a] = 0;
    } else {
      S.a_state[a] = 1;
    }
    return true;
  }
  // UAV.allocate (DroneEnvComponents.py:55-95) for a real task (id != 0) in slot s
  DEV bool uav_allocate(int a, int s, double pre_time = -1.0) {
    int id = S.t_id[s];
    if (queue_find(a, id) >= 0 || S.t_status[s] == 2) return false;
    S.a_reeval[a] = 0;
    S.a_last_id[a] = -1;
    S.a_last_slot[a] = -1;
    double time_to_task = pre_time >= 0 ? pre_time : fdiv(norm2(qs().a_nfx[a] - S.t_px[s], qs().a_nfy[a] - S.t_py[s]), speed_of(S.a_type[a]));
    double start_time = (qs().a_nft[a] - (double)tnow) > 0 ? qs().a_nft[a] : (double)tnow;
    double dur = (double)task_duration(S.t_type[s]);
    double end_time = start_time + time_to_task + dur;
    int n = S.a_qlen[a];
    if (n == 0) {
      S.a_task_start[a] = -1;
      S.a_state[a] = 1;
    }
    if (n >= Q) { fail(MUAVTA_ERR_QUEUE); return false; }
    S.a_qid[a][n] = id;
    S.a_qslot[a][n] = s;
    C.a_qtime[a][n] = time_to_task;
    S.a_qlen[a] = n + 1;
    qs().a_nft[a] = end_time;
    qs().a_nfx[a] = S.t_px[s];
    qs().a_nfy[a] = S.t_py[s];
    // Task.addAgentCap (DroneEnvComponents.py:306-326); status != 2 checked above
    S.t_ndet[s] += 1;
    S.times_dirty = 1; obs_static_clear();
    for (int c = 0; c < 6; c++) C.t_alloc[c][s] += S.a_caps[c][a];
    S.t_status[s] = 1;
    return true;
  }

  // ---------------------------------------------------------------- tasks / events (lane 0)
  DEV void push_event(int tag, int arg) {
    int n = S.n_events;
    if (n >= E) { fail(MUAVTA_ERR_EVENTS); return; }
    S.ev_tag[n] = tag;
    S.ev_arg[n] = arg;
    S.n_events = n + 1;
  }
  // A retired slot may be recycled once no LIVE agent queues it (its type/position are still read by
  // the switch penalty and the expected-distance term, :852-861,:1219-1220).
  DEV bool slot_unreferenced(int id) const {
    for (int a = 0; a < P.n_agents; a++) {
      if (S.a_state[a] == -1) continue;
      for (int k = 0; k < S.a_qlen[a]; k++) if (S.a_qid[a][k] == id) return false;
    }
    return true;
  }
  // Everything a released slot leaves behind except its column of known bits: the caller clears those (serially
  // below, or one agent per lane in the end-of-step GC) AFTER this has read them.  agent_known_tasks keeps the ids
  // of retired tasks and the token builders read len(known_ids): a reveal that is still pending for the id gets the
  // knower set (_wps_process_reveals adds the id to every set).
  DEV void release_slot_record(int s) {
    int h = S.t_threat[s];
    if (h >= 0) { S.h_tflags[h] = S.t_flags[s] & (TF_DEADLINE | TF_COUNTED); S.h_tdeadline[h] = S.t_deadline[s]; }
    if (S.t_bucket[s] == 0) atomicAdd(&S.n_retired_empty_buckets, 1);
    const int id = S.t_id[s];
    S.t_id[s] = -1;
    // a reveal can only be pending while t < created_at + threat_delay (registered at creation, :1491-1501)
    const bool pending = P.share_knowledge && tnow <= S.t_created[s] + (P.threat_delay > 0 ? P.threat_delay : 0) + 1;
    if (!pending && !rel_log) return;
    unsigned long long knowers = 0;
    for (int a = 0; a < P.n_agents; a++) knowers |= (unsigned long long)((S.known[a][s >> 5] >> (s & 31)) & 1u) << a;
    if (pending)
      for (int k = 0; k < S.n_pending; k++)
        if (S.pend_slot[k] == s && S.pend_id[k] == id) S.pend_know[k] = (typename KnowMask<A>::type)knowers;
    if (rel_log) {  // facade only: the task's final record and who knew the id when it left the device
      const int k = atomicAdd(reinterpret_cast<int*>(rel_log), 1);
      if (k < T) {
        double* r = rel_log + 1 + (size_t)k * MUAVTA_REL_ROW;
        const int ty = S.t_type[s];
        r[0] = id; r[1] = (double)(uint32_t)knowers; r[2] = (double)(uint32_t)(knowers >> 32); r[3] = ty;
        r[4] = (S.t_flags[s] & TF_DEADLINE) ? S.t_deadline[s] : -1; r[5] = S.t_created[s]; r[6] = S.t_required[s];
        r[7] = (S.t_flags[s] & TF_ESCORT) ? 1 : 0; r[8] = S.t_ndet[s]; r[9] = S.t_prot_agent[s];
        r[10] = (S.t_flags[s] & TF_ELIGIBLE) ? (double)S.t_elig[s] : -1.0; r[11] = S.t_px[s]; r[12] = S.t_py[s];
        r[13] = qs().t_org[s]; r[14] = qs().t_done[s]; r[15] = times().t_init[s]; r[16] = times().t_dtime[s];
        for (int c = 0; c < 6; c++) { r[17 + c] = C.t_cur[c][s]; r[23 + c] = C.t_alloc[c][s]; }
      }
    }
  }
  DEV void release_slot(int s) {  // serial form (lane 0, on-demand reclaim)
    release_slot_record(s);
    // leave the slot clean for its next tenant: nobody knows it, it is on the free list
    const uint32_t bit = 1u << (s & 31);
    for (int a = 0; a < P.n_agents; a++) {
      const uint32_t old = S.known[a][s >> 5];
      if (old & bit) { S.known[a][s >> 5] = old & ~bit; S.a_gone[a] += 1; }
    }
    S.free_slots[s >> 5] |= bit;
  }
  // One list item -> S.act_*[n] (lane 0; index -> slot through the open list the previous observation returned, which no phase
  // before the end of the step rewrites).  Agent ids beyond the fleet are skipped (the host entry points reject them).
  DEV bool stage_item(int n, int a, int idx) {
    if (a >= P.n_agents) return false;
    if (idx < 0) idx += S.n_open;  // python negative indexing into last_tasks_info
    S.act_agent[n] = (i8)a;
    S.act_slot[n] = (idx >= 0 && idx < S.n_open) ? (i8)S.open_slot[idx] : (i8)-1;
    S.act_index[n] = (i16)(idx < -32768 ? -32768 : idx > 32767 ? 32767 : idx);
    return true;
  }
  // the next up-to-A items of a long list (wave-uniform result: how many were staged)
  DEV int stage_more() {
    lds_sync();
    if (lane == 0) {
      int n = 0;
      while (more_pos < more_cap && n < A) {
        const int a = more_agent[more_pos];
        if (a < 0) { more_pos = more_cap; break; }
        if (stage_item(n, a, more_index[more_pos])) n++;
        more_pos++;
      }
      S.n_act = n;
    }
    lds_sync();
    return S.n_act;
  }
  DEV bool pending_item_names_slot(int s) const {  // (lane 0) an item not staged yet names slot s
    if (!more_agent) return false;
    for (int k = more_pos; k < more_cap; k++) {
      if (more_agent[k] < 0) break;
      int idx = more_index[k];
      if (idx < 0) idx += S.n_open;
      if (idx >= 0 && idx < S.n_open && S.open_slot[idx] == s) return true;
    }
    return false;
  }
  DEV int reclaim_slot_serial() {
    for (int k = 0; k < S.n_order; k++) {
      int s = S.t_order[k];
      if (S.t_status[s] != 2 || !slot_unreferenced(S.t_id[s])) continue;
      // Outside a step (muavta_call: _create_escort_for / _sync_escorts on a full tile) a slot that last_tasks_info still lists is not
      // recycled: nothing rebuilds that list before the next step applies action indices through it, and its row would name the new
      // tenant.  Inside a step the list is only read before the first creation and rebuilt at the end.  No slot left: capacity flag.
      if (!in_step) { const int r = S.t_row[s]; if (r < S.n_open && (int)S.open_slot[r] == s) continue; }
      bool staged = false;  // actions still to be applied this step may name it (-> invalid-action penalty)
      for (int j = 0; j < S.n_act; j++) staged |= (S.act_slot[j] == s);
      if (staged || pending_item_names_slot(s)) continue;
      release_slot(s);
      for (int i = k; i + 1 < S.n_order; i++) S.t_order[i] = S.t_order[i + 1];
      S.n_order--;
      return s;
    }
    return -1;
  }
  // Task.__init__ (DroneEnvComponents.py:224-263) into a free slot; returns the slot or -1
  DEV int new_task(double x, double y, int type, double req) {
    int id = S.next_task_id++;  // _alloc_task_id (:325-328)
    if (id > 32000) { fail(MUAVTA_ERR_TASK_SLOTS); return -1; }  // ids are stored in 16 bits
    int s = -1;
    for (int w = 0; w < KW; w++) if (S.free_slots[w]) { s = (w << 5) + __ffs((int)S.free_slots[w]) - 1; break; }
    if (s >= T) s = -1;
    if (s < 0) s = reclaim_slot_serial();  // tile full mid-step: recycle a retired slot before the end-of-step GC
    if (s < 0) { fail(MUAVTA_ERR_TASK_SLOTS); return -1; }
    S.free_slots[s >> 5] &= ~(1u << (s & 31));
    S.t_id[s] = id;
    S.t_px[s] = x; S.t_py[s] = y;
    for (int c = 0; c < 6; c++) { C.t_cur[c][s] = 0; C.t_alloc[c][s] = 0; }
    C.t_cur[type][s] = req;
    obs_static_clear();
    qs().t_org[s] = req; qs().t_done[s] = 0;
    times().t_init[s] = -1; times().t_dtime[s] = -1;
    S.t_status[s] = 0; S.t_type[s] = type; S.t_created[s] = 0; S.t_deadline[s] = -1; S.t_required[s] = 0;
    S.t_flags[s] = 0; S.t_elig[s] = 0; S.t_threat[s] = -1;
    S.t_prot_agent[s] = -1; S.t_prot_id[s] = -1; S.t_prot_slot[s] = -1;
    S.t_ndet[s] = 0; S.t_bucket[s] = 0;
    S.t_order[S.n_order++] = s;
    return s;
  }
  DEV void know_all(int s) { for (int a = 0; a < P.n_agents; a++) S.known[a][s >> 5] |= 1u << (s & 31); S.t_flags[s] |= TF_KNOWN_ALL; }

  // _register_dynamic_task (:1491-1504)
  DEV void register_dynamic(int s) {
    if (P.hard_windows && !(S.t_flags[s] & TF_DEADLINE)) {
      S.t_flags[s] |= TF_DEADLINE;
      S.t_deadline[s] = tnow + P.window_length;
      S.n_windowed_tasks++;
    }
    if (P.threat_delay > 0 || P.sense_radius > 0) {
      int n = S.n_pending;
      if (n >= R) { fail(MUAVTA_ERR_PENDING); return; }
      S.pend_time[n] = tnow + (P.threat_delay > 0 ? P.threat_delay : 0);
      S.pend_id[n] = S.t_id[s];
      S.pend_slot[n] = (uint8_t)s;
      S.pend_know[n] = 0;
      S.n_pending = n + 1;
    } else {
      know_all(s);
    }
  }
  // _wps_mark_window_outcome (:1543-1555) on explicit (flags, deadline) storage
  DEV void mark_outcome(u8& flags, int deadline, bool success) {
    if (!(flags & TF_DEADLINE)) return;
    if (flags & TF_COUNTED) return;
    flags |= TF_COUNTED;
    if (success && tnow <= deadline) { S.n_on_time++; S.F_Reward += P.on_time_bonus; }
    else { S.n_missed_windows++; S.F_Reward -= P.miss_penalty; }
  }
  DEV void mark_outcome_slot(int s, bool success) { mark_outcome(S.t_flags[s], S.t_deadline[s], success); }

  DEV bool counts_for_mission_done(int s) const {  // :1878-1886
    if (S.t_flags[s] & TF_ESCORT) return true;
    int ty = S.t_type[s];
    if (ty == MUAVTA_DET || ty == MUAVTA_HOLD) return true;
    return S.t_status[s] == 2;
  }
  DEV bool all_mission_done() const {  // freed slots are retired tasks, which always count as done
    for (int k = 0; k < S.n_order; k++) if (!counts_for_mission_done(S.t_order[k])) return false;
    return true;
  }
  DEV bool action_valid(int a, int s) const {  // _is_task_action_valid (:341-363)
    if (S.t_status[s] == 2) return false;
    if (S.a_qlen[a] > 0 && S.a_qid[a][0] == S.t_id[s]) return true;
    if ((S.t_flags[s] & TF_ELIGIBLE) && !((S.t_elig[s] >> S.a_type[a]) & 1u)) return false;
    int ty = S.t_type[s];
    if (P.capability_mask && S.a_caps[ty][a] <= 0) return false;
    if (P.saturate_mask && C.t_alloc[ty][s] >= qs().t_org[s]) return false;
    return true;
  }

  // ---------------------------------------------------------------- escorts (lane 0)
  DEV bool has_escort(int recon) const { return (S.esc_mask >> recon) & 1ull; }  // recon in _escort_by_recon, in one LDS read
  DEV int escort_lookup(int recon) const {
    for (int k = 0; k < S.n_escorts; k++) if (S.esc_agent[k] == recon) return k;
    return -1;
  }
  DEV void create_escort_for(int recon, int rec_slot) {  // _create_escort_for (:1888-1917)
    if (!P.escort_enabled) return;
    if (has_escort(recon)) return;
    int s = new_task(S.a_px[recon], S.a_py[recon], MUAVTA_DEF, P.escort_requirement);
    if (s < 0) return;
    S.t_flags[s] |= TF_ESCORT | TF_ELIGIBLE;
    S.t_elig[s] = P.escort_mask;
    S.t_prot_agent[s] = recon;
    S.t_prot_id[s] = rec_slot >= 0 ? (int)S.t_id[rec_slot] : -1;  // rec_slot < 0: protected_task = None (out-of-step callers only)
    S.t_prot_slot[s] = rec_slot;
    S.t_required[s] = P.escort_required_agents;
    S.t_created[s] = tnow;
    register_dynamic(s);
    int n = S.n_escorts;
    if (n >= A) { fail(MUAVTA_ERR_ESCORTS); return; }
    S.esc_mask |= 1ull << recon;
    S.esc_agent[n] = recon; S.esc_id[n] = S.t_id[s]; S.esc_slot[n] = s;
    S.esc_pid[n] = S.t_prot_id[s]; S.esc_pslot[n] = rec_slot;
    S.n_escorts = n + 1;
    S.escort_requests++;
    push_event(MUAVTA_EV_ESCORT_CREATED, S.t_id[s]);
    push_event(MUAVTA_EV_RESET_ALLOCATION, MUAVTA_DEF);
    S.pending_reset = 1;
  }
  // `holders`: superset of the agents that queue the escort task (callers that ran a wave-wide queue scan pass the
  // exact set; the default visits every agent, as the reference does)
  DEV void retire_escort_entry(int k, bool failed, unsigned long long holders = ~0ull) {  // _retire_escort (:1938-1950) for map entry k
    int s = S.esc_slot[k], id = S.esc_id[k];
    // an escort that expired by its hard window keeps its map entry forever (status == 2 -> early return)
    if (ref_retired(id, s)) return;
    // _release_escort_agents (:1919-1936): agent.desAllocate(escort) for every holder, in agents_obj order.  Every holder's
    // Task.removeAgentCap works on the SAME task: allocatedReqs is fetched once, the holders' capabilities are subtracted in order
    // in registers, and the result is stored once (a read-modify-write per holder is a memory round trip per holder).
    double al[6] = {0, 0, 0, 0, 0, 0};
    bool loaded = false;
    int nd = 0;
    for (int a = 0; a < P.n_agents; a++) {
      if (!((holders >> a) & 1ull)) continue;
      if (S.a_state[a] == -1 || S.a_qlen[a] == 0) continue;
      const int kq = queue_find(a, id);
      if (kq < 0 || id == 0) continue;
      {  // des_allocate_at(a, kq) with the task side deferred
        const int slot = S.a_qslot[a][kq];
        queue_erase(a, kq);
        qs().a_nft[a] = (double)tnow;
        qs().a_nfx[a] = S.a_px[a];
        qs().a_nfy[a] = S.a_py[a];
        S.a_commit[a] = 0;
        if (ref_valid(id, slot) && S.t_status[slot] != 2) {  // (slot == s: the one slot that holds this id)
          if (!loaded) {
#pragma unroll
            for (int c = 0; c < 6; c++) al[c] = C.t_alloc[c][s];
            loaded = true;
          }
#pragma unroll
          for (int c = 0; c < 6; c++) al[c] -= S.a_caps[c][a];
          nd++;
        }
      }
      if (S.a_qlen[a] == 0) {
        S.a_state[a] = 0;
        S.a_commit[a] = 0;
        qs().a_nft[a] = (double)tnow;
        qs().a_nfx[a] = S.a_px[a];
        qs().a_nfy[a] = S.a_py[a];
      }
    }
    if (loaded) {
#pragma unroll
      for (int c = 0; c < 6; c++) C.t_alloc[c][s] = al[c];
      S.t_ndet[s] -= nd;
      S.times_dirty = 1; obs_static_clear();
    }
    S.t_status[s] = 2;
    int recon = S.t_prot_agent[s];
    int kk = escort_lookup(recon);
    if (kk >= 0) {
      S.esc_mask &= ~(1ull << recon);
      for (int i = kk; i + 1 < S.n_escorts; i++) {
        S.esc_agent[i] = S.esc_agent[i + 1]; S.esc_id[i] = S.esc_id[i + 1]; S.esc_slot[i] = S.esc_slot[i + 1];
        S.esc_pid[i] = S.esc_pid[i + 1]; S.esc_pslot[i] = S.esc_pslot[i + 1];
      }
      S.n_escorts--;
    }
    if (failed) S.escort_failed++; else S.escort_completed++;
    push_event(MUAVTA_EV_ESCORT_RETIRED, id);
  }
  // _retire_escort (:1938-1950) of the escort that protects `recon`, with the whole wave (all lanes call it, uniform arguments):
  // every holder erases ITS OWN queue entry (lane = agent: agent.desAllocate touches the agent's own fields), Task.removeAgentCap
  // of the holders runs on one lane in agents_obj order (one fetch of allocatedReqs, one store), and the map entries behind the
  // retired one move up one lane each.  On lane 0 the same work is a chain of dependent LDS round trips: the map look-up, a pass
  // over the fleet, a five-array shift of the map (12-17 thousand cycles per retirement on the 24-agent tile).
  DEV void retire_escort_coop(int recon, bool failed) {
    cold_sync();  // the holders' lanes read queue-time rows other lanes wrote in earlier phases
    const int ne = __builtin_amdgcn_readfirstlane(S.n_escorts), nA = P.n_agents;
    const unsigned long long emk = __builtin_amdgcn_ballot_w64(lane < ne && S.esc_agent[lane < ne ? lane : 0] == recon);  // escort_lookup(recon)
    if (emk == 0ull) return;
    const int kk = __ffsll((long long)emk) - 1;
    const int s = S.esc_slot[kk], id = S.esc_id[kk];
    // an escort that expired by its hard window keeps its map entry forever (status == 2 -> early return)
    if (ref_retired(id, s)) return;
    // _release_escort_agents (:1919-1936)
    bool capped = false;
    if (lane < nA && S.a_state[lane] != -1 && S.a_qlen[lane] > 0) {
      const int a = lane;
      const int kq = queue_find(a, id);
      if (kq >= 0) {
        const int slot = S.a_qslot[a][kq];
        queue_erase(a, kq);
        qs().a_nft[a] = (double)tnow;
        qs().a_nfx[a] = S.a_px[a];
        qs().a_nfy[a] = S.a_py[a];
        S.a_commit[a] = 0;
        capped = ref_valid(id, slot) && S.t_status[slot] != 2;
        if (S.a_qlen[a] == 0) S.a_state[a] = 0;  // (commit_until / next_free_* were just set to the same values)
      }
    }
    const unsigned long long cm = __builtin_amdgcn_ballot_w64(capped);
    // the map entries behind kk, one per lane, before anybody rewrites them
    const int me = lane < ne ? lane : 0;
    const int m_agent = S.esc_agent[me], m_id = S.esc_id[me], m_slot = S.esc_slot[me], m_pid = S.esc_pid[me], m_pslot = S.esc_pslot[me];
    lds_sync();
    if (lane == 0) {
      if (cm) {  // Task.removeAgentCap of every holder, agents ascending
        double al[6];
#pragma unroll
        for (int c = 0; c < 6; c++) al[c] = C.t_alloc[c][s];
        for (unsigned long long m = cm; m; m &= m - 1ull) {
          const int a = __ffsll((long long)m) - 1;
#pragma unroll
          for (int c = 0; c < 6; c++) al[c] -= S.a_caps[c][a];
        }
#pragma unroll
        for (int c = 0; c < 6; c++) C.t_alloc[c][s] = al[c];
        S.t_ndet[s] -= __popcll(cm);
        S.times_dirty = 1; obs_static_clear();
      }
      S.t_status[s] = 2;
      S.esc_mask &= ~(1ull << recon);  // (== S.t_prot_agent[s]: the map is keyed by the protected UAV)
      S.n_escorts = ne - 1;
      if (failed) S.escort_failed++; else S.escort_completed++;
      push_event(MUAVTA_EV_ESCORT_RETIRED, id);
    }
    if (lane > kk && lane < ne) {
      S.esc_agent[lane - 1] = m_agent; S.esc_id[lane - 1] = m_id; S.esc_slot[lane - 1] = m_slot;
      S.esc_pid[lane - 1] = m_pid; S.esc_pslot[lane - 1] = m_pslot;
    }
    cold_sync();
  }
  DEV void retire_escort_for(int recon, bool failed) {  // :1952-1957
    int k = escort_lookup(recon);
    if (k >= 0) retire_escort_entry(k, failed);
  }
  // _escort_fighters_near (:1746-1764): nearest-first list into out[], returns count.
  // Stable insertion sort == python's sort(key=dist) on (dist, agent) pairs built in id order.
  template <class Out>
  DEV int escort_fighters_near(int prot, double radius, Out* out, double* outd) {
    int k = escort_lookup(prot);
    if (k < 0 || ref_retired(S.esc_id[k], S.esc_slot[k])) return 0;
    int eid = S.esc_id[k];
    int n = 0;
    for (int a = 0; a < P.n_agents; a++) {
      if (S.a_state[a] == -1 || !escort_type(S.a_type[a])) continue;
      if (S.a_qlen[a] == 0 || S.a_qid[a][0] != eid) continue;
      double d = norm2(S.a_px[a] - S.a_px[prot], S.a_py[a] - S.a_py[prot]);
      if (d <= radius) {
        int i = n;
        while (i > 0 && outd[i - 1] > d) { outd[i] = outd[i - 1]; out[i] = out[i - 1]; i--; }
        outd[i] = d; out[i] = (Out)a;
        n++;
      }
    }
    return n;
  }
  // closest_escort() for ONE PROTECTED UAV PER LANE (`need` / `prot` vary by lane; all lanes call it).  The serial form walks the
  // escort map and then the whole fleet per call — per threat lane that was n_agents LDS round trips and a square root whenever
  // any lane's filter passed.  Here lane k holds map entry k and lane a holds agent a; both are broadcast with v_readlane in
  // uniform loops, and the distance is only evaluated for an agent that heads some needed escort task.  Same arithmetic, same
  // order (agents ascending: the FIRST at the minimal distance wins).
  DEV void closest_escort_lanes(bool need, int prot, double radius, int& best, int& count) {
    best = -1; count = 0;
    if (__builtin_amdgcn_ballot_w64(need) == 0ull) return;
    const int ne = __builtin_amdgcn_readfirstlane(S.n_escorts), nA = P.n_agents;
    int eid = -1;  // the live escort task of this lane's protected UAV (escort_lookup + ref_retired)
    {
      const int ke = lane < ne ? lane : 0;
      const int ea = lane < ne ? (int)S.esc_agent[ke] : -1, ei = S.esc_id[ke], es = S.esc_slot[ke];
      const int elive = (lane < ne && !ref_retired(ei, es)) ? ei : -1;
      bool found = false;
      for (int k = 0; k < ne; k++) {
        const int ak = __builtin_amdgcn_readlane(ea, k), ik = __builtin_amdgcn_readlane(elive, k);
        if (need && !found && prot == ak) { eid = ik; found = true; }
      }
    }
    const bool want = need && eid >= 0;
    if (__builtin_amdgcn_ballot_w64(want) == 0ull) return;
    const int fa = lane < nA ? lane : 0;
    const bool fok = lane < nA && S.a_state[fa] != -1 && escort_type(S.a_type[fa]) && S.a_qlen[fa] > 0;
    const int fhead = fok ? (int)S.a_qid[fa][0] : -1;
    const double fx = S.a_px[fa], fy = S.a_py[fa];
    const double px = S.a_px[prot], py = S.a_py[prot];
    double bd = 0;
    for (int a = 0; a < nA; a++) {
      const int ha = __builtin_amdgcn_readlane(fhead, a);
      if (ha < 0) continue;
      const bool mt = want && eid == ha;
      if (__builtin_amdgcn_ballot_w64(mt) == 0ull) continue;
      const double d = norm2(readlane_f64(fx, a) - px, readlane_f64(fy, a) - py);
      if (mt && d <= radius) {
        if (count == 0 || d < bd) { bd = d; best = a; }
        count++;
      }
    }
  }
  DEV int closest_escort(int prot, double radius, int* count) {  // first element + count of the list above
    int k = escort_lookup(prot);
    *count = 0;
    if (k < 0 || ref_retired(S.esc_id[k], S.esc_slot[k])) return -1;
    int eid = S.esc_id[k];
    int best = -1, n = 0;
    double bd = 0;
    for (int a = 0; a < P.n_agents; a++) {
      if (S.a_state[a] == -1 || !escort_type(S.a_type[a])) continue;
      if (S.a_qlen[a] == 0 || S.a_qid[a][0] != eid) continue;
      double d = norm2(S.a_px[a] - S.a_px[prot], S.a_py[a] - S.a_py[prot]);
      if (d <= radius) { if (n == 0 || d < bd) { bd = d; best = a; } n++; }
    }
    *count = n;
    return best;
  }

  // ---------------------------------------------------------------- releaseAllTasks (:1442-1480)
  DEV void release_all_tasks(int for_type) {
    int ft = for_type < 0 ? for_type + 6 : for_type;  // python negative index -> caps[-1] == Det
    uint32_t avail = 0;
    for (int a = 0; a < P.n_agents; a++) {
      if (S.a_caps[ft][a] > 0 && S.a_state[a] != -1) {
        S.a_reeval[a] = 1;  // len(agent.tasks) > 0 always holds in python ([task_idle] counts)
        if (S.a_qlen[a] > 0) { S.a_last_id[a] = S.a_qid[a][0]; S.a_last_slot[a] = S.a_qslot[a][0]; }
        else { S.a_last_id[a] = 0; S.a_last_slot[a] = -1; }
        desallocate_all(a);
        avail |= 1u << S.a_type[a];
      }
    }
    for (int k = 0; k < S.n_order; k++) {
      int s = S.t_order[k];
      if (S.t_status[s] != 2 && S.t_type[s] == for_type) {
        double cum = 0;
        for (int ty = 0; ty < 7; ty++) if ((avail >> ty) & 1u) cum += CAP_TABLE[ty][for_type];
        if (cum == 0) {
          S.t_status[s] = 2;
          if (!(S.t_flags[s] & TF_REACHED)) {
            S.t_flags[s] |= TF_REACHED;
            S.n_reached++;
            if (S.n_reached == P.n_tasks) S.conclusion_time = tnow;
          }
        } else {
          S.t_status[s] = 0;
          S.t_bucket[s] = 0;
        }
      }
    }
  }

  // releaseAllTasks with the whole wave: per-agent flags by the agent's lane, queue teardown (shared f64
  // accumulators on the tasks -> agents_obj order) by lane 0 for the agents that actually queue something,
  // then one task per lane for the status/bucket reset.  All lanes must call it.
  // returns whether the call changed any state: a repeat of the same event right after a call that changed nothing
  // is a no-op (f(S) == S), which the drain loop uses to skip the tail of a burst's identical Reset_Allocation events
  DEV bool release_all_tasks_coop(int for_type) {
    PROF_COUNT(53, 1000);
    const int ft = for_type < 0 ? for_type + 6 : for_type;  // python negative index -> caps[-1] == Det
    const int a = lane;
    bool match = false, busy = false, chg = false;
    if (a < P.n_agents && S.a_caps[ft][a] > 0 && S.a_state[a] != -1) {
      match = true;
      chg = S.a_reeval[a] != 1;
      S.a_reeval[a] = 1;  // len(agent.tasks) > 0 always holds in python ([task_idle] counts)
      if (S.a_qlen[a] > 0) { S.a_last_id[a] = S.a_qid[a][0]; S.a_last_slot[a] = S.a_qslot[a][0]; busy = true; chg = true; }
      else {  // desallocateAll on [task_idle]
        chg |= S.a_last_id[a] != 0 || S.a_last_slot[a] != -1 || S.a_commit[a] != 0;
        S.a_last_id[a] = 0; S.a_last_slot[a] = -1; S.a_commit[a] = 0;
      }
    }
    unsigned long long bm = __ballot(busy);
    if (bm) cold_sync();  // the queue teardown below reads / rewrites EnvCold rows other lanes wrote in earlier phases
    uint32_t avail = 0;
    {  // available_agents: set of type indices of the matched agents
      const int ty = a < P.n_agents ? S.a_type[a] : 0;
      // (ballots straight from a compare: the ballot of a combined predicate costs a v_cndmask + v_cmp to materialise it)
      const int tym = match ? ty : -1;
#pragma unroll
      for (int t = 0; t <= MUAVTA_F2; t++) if (__builtin_amdgcn_ballot_w64(tym == t) != 0ull) avail |= 1u << t;
    }
    lds_sync();
    if (Q <= 16) {
      constexpr int HQ = (Q + 1) / 2;
      // desallocateAll of every busy agent at once.  `for task in self.tasks: self.desAllocate(task)` over the list
      // being mutated drops the queue entries at even positions and keeps the odd ones (iterate_desallocate).
      // Agent side (lane = agent): own queue compaction + next-free fields.  Task side (lane = slot): Task.removeAgentCap
      // of the dropped entries in the reference's order (agents ascending), so allocatedReqs sees the same f64 sequence.
      int rid[HQ], rsl[HQ];
#pragma unroll
      for (int i = 0; i < HQ; i++) { rid[i] = -1; rsl[i] = -1; }  // dropped (task id, slot) of this lane's agent
      if (busy) {
        const int n = S.a_qlen[a];
#pragma unroll
        for (int i = 0; i < HQ; i++) if (2 * i < n) { rid[i] = S.a_qid[a][2 * i]; rsl[i] = S.a_qslot[a][2 * i]; }
        int kid[HQ], ksl[HQ]; double ktm[HQ];
#pragma unroll
        for (int i = 0; i < HQ; i++) if (2 * i + 1 < n) { kid[i] = S.a_qid[a][2 * i + 1]; ksl[i] = S.a_qslot[a][2 * i + 1]; ktm[i] = C.a_qtime[a][2 * i + 1]; }
#pragma unroll
        for (int i = 0; i < HQ; i++) if (2 * i + 1 < n) { S.a_qid[a][i] = kid[i]; S.a_qslot[a][i] = ksl[i]; C.a_qtime[a][i] = ktm[i]; }
        S.a_qlen[a] = n >> 1;
        qs().a_nft[a] = (double)tnow; qs().a_nfx[a] = S.a_px[a]; qs().a_nfy[a] = S.a_py[a];
        S.a_commit[a] = 0;
      }
      // Task side: who dropped which slot travels through per-slot agent masks in the scratch tile (LDS atomics), and a slot
      // lane walks only the agents that dropped IT, in ascending order — not every busy agent's HQ dropped entries (r2: 2 x HQ
      // v_readlane + compares per busy agent and pass, ~600 VALU per call on the 24-agent tile).
      typedef typename BucketMask<A>::type DropMask;
      DropMask* dropm = reinterpret_cast<DropMask*>(X.cost);
      static_assert(sizeof(DropMask) * T <= sizeof(double) * Scratch<TL>::COSTN, "drop masks overflow the scratch cost tile");
      for (int sl = lane; sl < T; sl += WG) dropm[sl] = 0;
      lds_sync();
#pragma unroll
      for (int i = 0; i < HQ; i++)
        if (rsl[i] >= 0 && S.t_id[rsl[i]] == rid[i]) atomicOr(&dropm[rsl[i]], (DropMask)1 << a);  // (a live reference: the slot still holds that id)
      lds_sync();
      for (int base = 0; base < T; base += WG) {
        const int sl = base + lane;
        DropMask m = sl < T ? dropm[sl] : (DropMask)0;
        if (m != 0 && S.t_status[sl] == 2) m = 0;  // removeAgentCap ignores concluded tasks
        if (m != 0) {
          double al[6];
#pragma unroll
          for (int c = 0; c < 6; c++) al[c] = C.t_alloc[c][sl];
          int nd = 0;
          for (; m != 0; m &= m - 1) {
            const int b = (sizeof(DropMask) > 4 ? __ffsll((long long)m) : __ffs((int)m)) - 1;
#pragma unroll
            for (int c = 0; c < 6; c++) al[c] -= S.a_caps[c][b];
            nd++;
          }
#pragma unroll
          for (int c = 0; c < 6; c++) C.t_alloc[c][sl] = al[c];
          S.t_ndet[sl] -= nd;
          S.times_dirty = 1; obs_static_clear();
        }
      }
    } else if (lane == 0) {
      while (bm) {
        const int b = __ffsll((long long)bm) - 1;
        bm &= bm - 1ull;
        desallocate_all(b);
      }
    }
    cold_sync();
    if (for_type < 0) return __ballot(chg) != 0ull;  // no task has typeIdx -1
    double cum = 0;
    for (int ty = 0; ty < 7; ty++) if ((avail >> ty) & 1u) cum += CAP_TABLE[ty][for_type];
    bool dead_end = false;
    for (int k = lane; k < S.n_order; k += WG) {
      const int s = S.t_order[k];
      if (S.t_status[s] != 2 && S.t_type[s] == for_type) {
        if (cum == 0) dead_end = true;
        else { chg |= S.t_status[s] != 0 || S.t_bucket[s] != 0; S.t_status[s] = 0; S.t_bucket[s] = 0; }
      }
    }
    chg |= dead_end;
    if (__ballot(dead_end) != 0ull) {  // nobody left who can do this type: retire the tasks, in id order (:1466-1476)
      lds_sync();
      if (lane == 0) {
        for (int k = 0; k < S.n_order; k++) {
          const int s = S.t_order[k];
          if (S.t_status[s] != 2 && S.t_type[s] == for_type) {
            S.t_status[s] = 2;
            if (!(S.t_flags[s] & TF_REACHED)) {
              S.t_flags[s] |= TF_REACHED;
              S.n_reached++;
              if (S.n_reached == P.n_tasks) S.conclusion_time = tnow;
            }
          }
        }
      }
    }
    lds_sync();
    return __ballot(chg) != 0ull;
  }

  // ---------------------------------------------------------------- geometry helpers
  DEV void norm_vector(double& x, double& y) {  // EnvUtils.norm_vector (MultiDroneEnvUtils.py:168-177)
    double m = norm2(x, y);
    if (m == 0) { x = 0; y = 0; return; }
    const double r = frcp_nr(m);  // (m > 0: a norm of finite coordinates)
    x = fdiv_r(x, m, r); y = fdiv_r(y, m, r);
  }
  // core_sim SimCore::avoid_obstacles (core_sim/src/sim_core.rs:25-59); Rust `%` == fmod
  DEV void avoid_obstacles(double px, double py, double mx, double my, double& ax, double& ay) {
    ax = 0.0; ay = 0.0;
    const double PI = 3.14159265358979323846;
    for (int o = 0; o < P.num_obstacles; o++) {
      double dx = C.obst[o][0] - px, dy = C.obst[o][1] - py;
      double d_zone = sqrt(dx * dx + dy * dy) - C.obst[o][2];
      if (d_zone < 40.0) {
        double nx = dx / d_zone, ny = dy / d_zone;
        double force = libm_log(fmax(1.05, d_zone));  // f64::ln of the reference = the host libm's log, bit for bit (libm_log above)
        force = 0.5 / (1.0 - force);
        // the SIGN of the wrapped angle picks the side: an agent steered onto the line through the obstacle's centre holds two angles an ulp
        // apart, so both must be the host libm's atan2 to the last bit (muavta_atan2.h)
        double ang = libm_atan2(my, mx) - libm_atan2(dy, dx);
        ang = fmod(ang + PI, 2.0 * PI) - PI;
        double rx, ry;
        if (ang > 0.0) { rx = ny; ry = -nx; } else { rx = -ny; ry = nx; }
        ax += rx * force;
        ay += ry * force;
      }
    }
  }
  // random_position (:1371-1410)
  DEV void random_position(int st, double min_distance, double own_range, bool contact_line, int area, bool check_obs,
                           double& ox, double& oy) {
    double limit_line = contact_line ? CONTACT_LINE : 0;
    for (int tries = 0; tries < 100; tries++) {
      double x, y;
      if (area >= 0) {
        double tlx = qs().area[area][0], tly = qs().area[area][1], w = qs().area[area][2];
        x = uniform(st, tlx, tlx + w);
        y = uniform(st, tly, tly + w);
      } else {
        x = uniform(st, own_range + min_distance, AREA_W - own_range - min_distance);
        y = uniform(st, own_range + min_distance,
                    AREA_H - own_range - min_distance - ((limit_line != 0) ? (AREA_H - limit_line) : 0));
      }
      bool valid = true;
      if (check_obs) {
        for (int o = 0; o < P.num_obstacles && o < 8; o++) {
          if (C.obst[o][2] < 0) break;  // not created yet
          double d = norm2(x - C.obst[o][0], y - C.obst[o][1]) - own_range;
          if (d < C.obst[o][2] + min_distance) { valid = false; break; }
        }
      }
      if (valid) { ox = x; oy = y; return; }
    }
    fail(MUAVTA_ERR_POSITION);
    ox = 0; oy = 0;
  }
  // get_closest_agent with one agent per lane (all lanes call it): the serial scan takes `d < min` strictly, i.e. the FIRST agent
  // at the minimal distance — here the lowest lane among those equal to the wave-wide minimum.  On lane 0 the scan is a chain of
  // n_agents LDS round trips and square roots (16,000 cycles per failed engagement on the 64-agent tile).
  DEV int closest_agent_coop(double x, double y) {
    const double INF = __builtin_huge_val();
    const int a = lane < P.n_agents ? lane : 0;
    const int st = S.a_state[a], ty = S.a_type[a];
    const bool valid = lane < P.n_agents && st != -1 && st != 4;
    const double d = norm2(S.a_px[a] - x, S.a_py[a] - y);
    const bool fighter = is_fighter(ty);
    const double dW = (valid && !fighter) ? d : INF;
    const double mW = wave_min_first(dW, A);  // (A: compile-time — agent lanes only)
    if (__double2hiint(mW) != 0x7ff00000) return __ffsll((long long)__builtin_amdgcn_ballot_w64(dW == mW)) - 1;
    const double dF = (valid && fighter) ? d : INF;
    const double mF = wave_min_first(dF, A);
    if (__double2hiint(mF) != 0x7ff00000) return __ffsll((long long)__builtin_amdgcn_ballot_w64(dF == mF)) - 1;
    return -1;
  }
  // the retarget an engagement replayed on lane 0 asked for (handle_threat_engagement): all lanes, uniform
  DEV void resolve_retarget() {
    const int h = __builtin_amdgcn_readfirstlane(X.retarget_h);
    if (h < 0) return;
    const int tgt = closest_agent_coop(S.h_px[h], S.h_py[h]);
    if (lane == 0) { S.h_target[h] = tgt; S.h_mission[h] = tgt; X.retarget_h = -1; }
    lds_sync();
  }
  DEV int closest_agent(double x, double y) const {  // get_closest_agent (:1691-1723)
    double minF = __builtin_huge_val(), minW = __builtin_huge_val();
    int cF = -1, cW = -1;
    for (int a = 0; a < P.n_agents; a++) {
      int st = S.a_state[a];
      if (st != -1 && st != 4) {
        double d = norm2(S.a_px[a] - x, S.a_py[a] - y);
        if (is_fighter(S.a_type[a])) { if (d < minF) { minF = d; cF = a; } }
        else { if (d < minW) { minW = d; cW = a; } }
      }
    }
    return cW >= 0 ? cW : cF;
  }

