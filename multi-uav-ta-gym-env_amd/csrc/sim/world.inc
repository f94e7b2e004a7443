// sim/world.inc — member functions of Sim<TL> (muavta_device.h includes this file INSIDE the struct body): world dynamics of a step: threats, arrivals, escort sync, sensing, reveals / windows, reward assembly, end-of-step slot GC.
  // get_closest_agent (:1691-1723) for every threat that can spawn this step, one (threat, agent) pair per lane, so
  // that lane 0's generate_threat only looks the answer up.  Spawn positions are fixed at reset unless
  // dual_region_bursts redraws x (then generate_threat searches itself).  Result: X.roundT[threat id].
  DEV bool threat_spawn_step() const { return tnow > 40 && tnow % 10 == 0; }
  DEV void precompute_threat_targets() {
    if (!threat_spawn_step() || P.dual_region_bursts) return;  // uniform
    const int nA = P.n_agents;
    for (int g = 0; g < P.n_threat_groups; g++) {
      const int start = S.g_next[g], left = S.g_end[g] - start;
      int cnt = P.burst_mode ? (P.burst_size < left ? P.burst_size : left) : (left > 0 ? 1 : 0);
      if (cnt <= 0) continue;
      const int chunk = Scratch<TL>::COSTN / nA;  // threats per pass of the distance scratch (>= 1: COSTN >= 4 * A)
      for (int c0 = 0; c0 < cnt; c0 += chunk) {
        const int cn = cnt - c0 < chunk ? cnt - c0 : chunk;
        for (int p = lane; p < cn * nA; p += WG) {
          const int c = p / nA, a = p - c * nA, h = start + c0 + c;
          const int st = S.a_state[a];
          X.cost[p] = (h < H && st != -1 && st != 4) ? norm2(S.a_px[a] - S.h_px[h], S.a_py[a] - S.h_py[h]) : __builtin_huge_val();
        }
        lds_sync();
        for (int c = lane; c < cn; c += WG) {
          double minF = __builtin_huge_val(), minW = __builtin_huge_val();
          int cF = -1, cW = -1;
          for (int a = 0; a < nA; a++) {
            const double d = X.cost[c * nA + a];
            const int st = S.a_state[a];
            if (st != -1 && st != 4) {
              if (is_fighter(S.a_type[a])) { if (d < minF) { minF = d; cF = a; } }
              else { if (d < minW) { minW = d; cW = a; } }
            }
          }
          if (start + c0 + c < H) X.roundT[start + c0 + c] = cW >= 0 ? cW : cF;
        }
        lds_sync();
      }
    }
  }
  DEV void generate_threat() {  // :1601-1643
    if (!threat_spawn_step()) return;  // (the per-group test below needs it anyway: nine steps in ten end here)
    for (int g = 0; g < P.n_threat_groups; g++) {
      int left = S.g_end[g] - S.g_next[g];
      if (left > 0 && threat_spawn_step()) {
        if (rnd(ST_AGENT) < P.threat_prob) {
          int n_spawn = 1;
          if (P.burst_mode) n_spawn = P.burst_size < left ? P.burst_size : left;
          for (int bi = 0; bi < n_spawn; bi++) {
            if (S.g_next[g] >= S.g_end[g]) break;
            int h = S.g_next[g]++;
            if (h >= H) { fail(MUAVTA_ERR_TASK_SLOTS); break; }
            if (P.dual_region_bursts) {
              double mid = AREA_W * 0.5;
              double wide = fmax(AREA_W / 10, 40.0);
              double x;
              if ((S.burst_region_toggle + bi) % 2 == 0) x = uniform(ST_AGENT, wide, mid - wide);
              else x = uniform(ST_AGENT, mid + wide, AREA_W - wide);
              S.h_px[h] = x;
            }
            const int tgt = P.dual_region_bursts ? closest_agent(S.h_px[h], S.h_py[h]) : X.roundT[h];
            S.h_target[h] = tgt;
            S.h_mission[h] = tgt;
            // TaskFromThreat (:1861-1876)
            int ty = S.h_type[h];
            double attack = threat_attack(ty), defence = threat_defence(ty);
            int s = new_task(S.h_px[h], S.h_py[h], MUAVTA_INT, 2.0);
            if (s >= 0) {
              C.t_cur[MUAVTA_ATT][s] = defence * 2;
              C.t_cur[MUAVTA_DEF][s] = attack * 2;
              obs_static_clear();
              S.t_threat[s] = h;
              S.t_created[s] = tnow;
              if (ty == MUAVTA_T1) { S.t_required[s] = 2; S.t_flags[s] |= TF_ELIGIBLE; S.t_elig[s] = P.escort_mask; }
              S.h_task_id[h] = S.t_id[s];
              S.h_task_slot[h] = s;
            }
            S.h_status[h] = 1;
            S.h_order[S.n_active_threats++] = h;
            C.t_cur[5][S.h_det_slot[h]] -= 1.0;
            if (s >= 0) {
              register_dynamic(s);
              push_event(MUAVTA_EV_NEW_THREAT, S.t_id[s]);
            }
            push_event(MUAVTA_EV_RESET_ALLOCATION, MUAVTA_INT);
            S.pending_reset = 1;
          }
          if (P.dual_region_bursts && n_spawn > 0) S.burst_region_toggle = (S.burst_region_toggle + 1) % 2;
        }
      }
    }
  }

  // the threat's Int task: live slot, or the (flags, deadline) copy kept on the threat once freed
  DEV void threat_task_retire(int h, bool success) {
    int s = S.h_task_slot[h];
    if (ref_valid(S.h_task_id[h], s)) { S.t_status[s] = 2; mark_outcome_slot(s, success); }
    else mark_outcome(S.h_tflags[h], S.h_tdeadline[h], success);
  }

  DEV void handle_threat_engagement(int h) {  // :1781-1858
    int primary = S.h_target[h];
    int mission = S.h_mission[h] >= 0 ? S.h_mission[h] : primary;
    int n_def = 0;
    int16_t* defs = X.remaining;   // scratch lists (T >= A)
    double* defd = X.v;
    if (P.escort_enabled && mission >= 0 && is_recon(S.a_type[mission])) {
      n_def = escort_fighters_near(mission, P.mutual_support_radius, defs, defd);
      if (n_def > 0) {
        primary = defs[0];
        S.h_target[h] = primary;
        S.h_intercept[h] = primary;
      }
    }
    if (primary < 0) return;
    const int hty = S.h_type[h];
    const double t_att = threat_attack(hty), t_def = threat_defence(hty), t_rng = engage_range(hty);
    double attDiff, defDiff, engageDiff;
    if (n_def >= 2) {
      S.mutual_support_engagements++;
      double att_sum = 0, def_sum = 0, eng_sum = 0;
      for (int k = 0; k < n_def; k++) att_sum += S.a_caps[2][defs[k]];
      for (int k = 0; k < n_def; k++) def_sum += S.a_caps[3][defs[k]];
      for (int k = 0; k < n_def; k++) eng_sum += engage_range(S.a_type[defs[k]]);
      eng_sum = eng_sum / (double)n_def;
      attDiff = att_sum / fmax(t_att, 1e-6);
      defDiff = def_sum / fmax(t_def, 1e-6);
      engageDiff = eng_sum / fmax(t_rng, 1e-6);
    } else {
      attDiff = S.a_caps[2][primary] / fmax(t_att, 1e-6);
      defDiff = S.a_caps[3][primary] / fmax(t_def, 1e-6);
      engageDiff = engage_range(S.a_type[primary]) / fmax(t_rng, 1e-6);
    }
    double avg_diff = (attDiff + defDiff + engageDiff) / 3;
    double prob = avg_diff / (avg_diff + 1);
    double r = rnd(ST_AGENT);
    if (r < prob) {
      S.h_status[h] = 2;
      threat_task_retire(h, true);
      S.threats_intercepted++;
      S.a_acap[primary] -= 1;
      if (S.a_acap[primary] <= 0) S.a_caps[3][primary] = 0;
      if (S.a_qlen[primary] > 0 && S.a_qid[primary][0] == S.h_task_id[h]) task_done(primary, S.h_task_id[h], MUAVTA_INT);
      S.step_reward += 1.0;
    } else {
      S.h_acap[h] -= 1;
      S.a_acap[primary] -= 1;
      if (S.a_acap[primary] <= 0) {
        S.a_caps[3][primary] = 0;
        bool was_recon = is_recon(S.a_type[primary]);
        bool was_escort = escort_type(S.a_type[primary]);
        out_of_service(primary);
        if (was_recon) { S.recon_losses++; S.protection_breaches++; retire_escort_for(primary, true); }
        else if (was_escort) S.escort_losses++;
        S.step_reward -= 1.0;
      }
      if (S.h_acap[h] <= 0) {
        S.h_status[h] = 0;
        threat_task_retire(h, false);
      } else {
        X.retarget_h = h;  // threat.target = threat.mission_target = get_closest_agent(position): left to the whole wave (resolve_retarget),
                           // nothing reads either field before the caller gets there
      }
    }
  }

  // update_threats (:1725-1744), one active threat per lane.  A threat's turn touches only its own record
  // (position, target, its Int task's position) unless it ENGAGES (shared RNG stream, kills) or leaves the
  // area with an uncounted window (shared counters): those are events.  Threats before the first event
  // (env.threats order) commit their lane's result; lane 0 replays the reference loop from the event on.
  // Returns (first serial index, snapshot mask of threats with status != 2).
  // lanes [start, n): the threats behind the last serially replayed one; `livemask` is taken once, at start == 0
  // all_at_once (no escorts): every non-event threat commits and the mask of event threats is returned instead of the first one
  DEV unsigned long long update_threats_parallel(int start, unsigned long long& livemask, bool all_at_once) {
    static_assert(H <= 64, "one threat per lane");
    const int n = S.n_active_threats;
    const int k = lane;
    // operands in three LDS round trips (spawn-order slot -> the threat's record -> its target's position and its Int
    // task's slot), whatever branch the lane takes afterwards
    const int h = k < n ? (int)S.h_order[k] : 0;
    const int hst = S.h_status[h], hty = S.h_type[h], slot = S.h_task_slot[h], task_id = S.h_task_id[h], htf = S.h_tflags[h];
    int tgt = S.h_target[h], icpt = S.h_intercept[h];
    const int hmis = S.h_mission[h];
    const double px = S.h_px[h], py = S.h_py[h];
    bool active = k < n && hst != 2;
    if (start == 0) livemask = __ballot(active);  // python snapshots [t for t in self.threats if t.status != 2] before the loop
    active = k >= start && k < n && ((livemask >> k) & 1ull);
    const int sli = slot >= 0 ? slot : 0;
    const int t_id_at = S.t_id[sli], t_stat = S.t_status[sli], t_fl = S.t_flags[sli];
    bool evt = false;
    double npx = 0, npy = 0;
    bool live_task = false;
    if (P.escort_enabled) {  // _retarget_threat_via_escort (:1766-1779): reads agents only.  One protected UAV per threat lane,
                             // the escort map and the fleet walked in uniform loops (closest_escort_lanes)
      const int mission = hmis >= 0 ? hmis : tgt;
      const int mi = mission >= 0 ? mission : 0;
      const bool need = active && !(hst == 0 || tgt < 0) && mission >= 0 && S.a_state[mi] != -1 && is_recon(S.a_type[mi]);
      int e0, cnt;
      closest_escort_lanes(need, mi, P.escort_intercept_radius, e0, cnt);
      if (need) {
        if (cnt == 0) { tgt = mission; icpt = -1; }
        else { tgt = e0; icpt = e0; }
      }
    }
    if (active) {
      const double speed = speed_of(hty);
      if (hst == 0 || tgt < 0) {
        npx = px + speed * 0.0;
        npy = py + speed * -1.0;
      } else {
        const double ax = S.a_px[tgt], ay = S.a_py[tgt];
        double dx = ax - px, dy = ay - py;
        norm_vector(dx, dy);
        npx = px + speed * dx;
        npy = py + speed * dy;
        if (norm2(ax - npx, ay - npy) < engage_range(hty)) evt = true;
      }
      live_task = slot >= 0 && t_id_at == task_id;  // ref_valid(S.h_task_id[h], slot)
      if (npy <= 0) {  // leaving the area: an event only if the retirement would still change something
        if (live_task) evt |= (t_stat != 2) || ((t_fl & TF_DEADLINE) && !(t_fl & TF_COUNTED));
        else evt |= (htf & TF_DEADLINE) && !(htf & TF_COUNTED);
      }
    }
    const unsigned long long em = __ballot(evt);
    const int first = em ? __ffsll((long long)em) - 1 : n;
    if (active && (all_at_once ? !evt : k < first)) {
      S.h_px[h] = npx; S.h_py[h] = npy;
      S.h_target[h] = tgt; S.h_intercept[h] = icpt;
      if (live_task) { S.t_px[slot] = npx; S.t_py[slot] = npy; }
    }
    return all_at_once ? em : (unsigned long long)first;
  }
  DEV void update_threats_serial(int first, unsigned long long livemask) {  // the reference's loop body for ONE threat
    const int n = first + 1 < S.n_active_threats ? first + 1 : S.n_active_threats;
    for (int k = first; k < n; k++) {
      if (!((livemask >> k) & 1ull)) continue;
      int h = S.h_order[k];
      const double speed = speed_of(S.h_type[h]);
      if (S.h_status[h] == 0 || S.h_target[h] < 0) {
        S.h_px[h] = S.h_px[h] + speed * 0.0;
        S.h_py[h] = S.h_py[h] + speed * -1.0;
      } else {
        if (P.escort_enabled) {  // _retarget_threat_via_escort (:1766-1779)
          int mission = S.h_mission[h] >= 0 ? S.h_mission[h] : S.h_target[h];
          if (mission >= 0 && S.a_state[mission] != -1 && is_recon(S.a_type[mission])) {
            int cnt;
            int e0 = closest_escort(mission, P.escort_intercept_radius, &cnt);
            if (cnt == 0) { S.h_target[h] = mission; S.h_intercept[h] = -1; }
            else { S.h_target[h] = e0; S.h_intercept[h] = e0; }
          }
        }
        int tg = S.h_target[h];
        double dx = S.a_px[tg] - S.h_px[h], dy = S.a_py[tg] - S.h_py[h];
        norm_vector(dx, dy);
        S.h_px[h] = S.h_px[h] + speed * dx;
        S.h_py[h] = S.h_py[h] + speed * dy;
        if (norm2(S.a_px[tg] - S.h_px[h], S.a_py[tg] - S.h_py[h]) < engage_range(S.h_type[h])) handle_threat_engagement(h);
      }
      int s = S.h_task_slot[h];
      bool live = ref_valid(S.h_task_id[h], s);
      if (live) { S.t_px[s] = S.h_px[h]; S.t_py[s] = S.h_py[h]; }
      if (S.h_py[h] <= 0) threat_task_retire(h, false);
    }
  }

  DEV void inject_dynamic_arrivals() {  // :1646-1689
    if (P.arrival_rate <= 0 || tnow < 5) return;
    if (rnd(ST_TGT) >= P.arrival_rate) return;
    if (S.next_task_id - 1 >= P.max_tasks - 1) return;  // len(self.tasks) >= max_tasks - 1
    int ty = randbelow(ST_TGT, 2) == 0 ? MUAVTA_ATT : MUAVTA_REC;
    // the reference allocates the id before drawing the mission area; ids are only consumed here
    int sel = (int)randbelow(ST_MISSION, 3);
    double x, y;
    if (P.dual_region_bursts) {
      double mid = AREA_W * 0.5, wide = 40.0;
      if (rnd(ST_TGT) < 0.5) x = uniform(ST_TGT, wide, mid - wide);
      else x = uniform(ST_TGT, mid + wide, AREA_W - wide);
      y = uniform(ST_TGT, AREA_H * 0.2, AREA_H * 0.8);
    } else {
      random_position(ST_TGT, 20, 3, true, sel, true, x, y);
    }
    int s = new_task(x, y, ty, 1.0);
    S.n_arrivals++;
    if (s >= 0) {
      S.t_created[s] = tnow;
      register_dynamic(s);
      push_event(MUAVTA_EV_NEW_THREAT, S.t_id[s]);
    }
    push_event(MUAVTA_EV_RESET_ALLOCATION, ty);
    S.pending_reset = 1;
  }

  DEV void sync_escorts() {  // :1964-2000
    for (int a = 0; a < P.n_agents; a++) {
      if (S.a_state[a] == -1 || !is_recon(S.a_type[a])) continue;
      if (S.a_qlen[a] == 0) continue;
      int cid = S.a_qid[a][0], cs = S.a_qslot[a][0];
      if (ref_retired(cid, cs)) continue;
      if (S.t_type[cs] == MUAVTA_REC && !has_escort(a)) create_escort_for(a, cs);
    }
    // iterate a snapshot of the map (retiring pops entries)
    int n = S.n_escorts;
    int16_t* snap = X.row4col;  // T >= A
    for (int k = 0; k < n; k++) snap[k] = S.esc_agent[k];
    for (int k = 0; k < n; k++) {
      int recon = snap[k];
      int kk = escort_lookup(recon);
      if (kk < 0) continue;
      int es = S.esc_slot[kk];
      int rid = S.esc_pid[kk], rs = S.esc_pslot[kk];
      bool dead = S.a_state[recon] == -1;
      bool idle = S.a_qlen[recon] == 0 || S.a_state[recon] == 0 || S.a_state[recon] == 3;
      bool rec_done = ref_retired(rid, rs);
      bool wrong_task = S.a_qlen[recon] > 0 && S.a_qid[recon][0] != rid;
      if (dead || idle || rec_done || wrong_task) { retire_escort_entry(kk, dead); continue; }
      if (ref_valid(S.esc_id[kk], es)) { S.t_px[es] = S.a_px[recon]; S.t_py[es] = S.a_py[recon]; }
      S.escort_required_steps++;
      int cnt;
      closest_escort(recon, P.escort_radius, &cnt);
      if (cnt > 0) S.escort_covered_steps++;
    }
  }

  // _sync_escorts (:1964-2000) with the whole wave: the per-agent / per-escort predicates are evaluated one per
  // lane (ballots), creations and retirements (shared state, id allocation order) stay on lane 0 in the
  // reference's order, and the coverage test "any escort fighter within radius" is a ballot over agents.
  DEV void sync_escorts_coop() {
    {  // recon UAVs already on a Rec task without an escort (:1967-1974)
      const int a = lane;
      bool need = false;
      int cs = -1;
      if (a < P.n_agents && S.a_state[a] != -1 && is_recon(S.a_type[a]) && S.a_qlen[a] > 0) {
        const int cid = S.a_qid[a][0];
        cs = S.a_qslot[a][0];
        need = !ref_retired(cid, cs) && S.t_type[cs] == MUAVTA_REC && !has_escort(a);
      }
      unsigned long long nm = __ballot(need);
      if (nm) {
        if (lane == 0) {
          while (nm) {
            const int b = __ffsll((long long)nm) - 1;
            nm &= nm - 1ull;
            create_escort_for(b, S.a_qslot[b][0]);
          }
        }
        lds_sync();
      }
    }
    // Snapshot of the map, one entry per lane (retiring pops entries).  Whether an entry retires depends only on its
    // recon UAV and Rec task, which no other entry's retirement touches, so that is decided up front; coverage of
    // the entries BETWEEN two retirements is then evaluated in one pass (fighters' queues only change at a
    // retirement), one fighter per lane, instead of one map entry at a time.
    PROF(59);
    const int n = S.n_escorts;
    if (n == 0) return;
    int recon = -1, es = -1, eid = -1, rid = -1, rs = -1;
    bool retire = false, dead = false, esc_live = false, esc_here = false;
    auto decide = [&]() {  // :1978-1990 for the lane's entry, on the state as it is now
      if (lane < n) {
        dead = S.a_state[recon] == -1;
        const bool idle = S.a_qlen[recon] == 0 || S.a_state[recon] == 0 || S.a_state[recon] == 3;
        const bool rec_done = ref_retired(rid, rs);
        const bool wrong_task = S.a_qlen[recon] > 0 && S.a_qid[recon][0] != rid;
        retire = dead || idle || rec_done || wrong_task;
      }
    };
    if (lane < n) {
      recon = S.esc_agent[lane]; es = S.esc_slot[lane]; eid = S.esc_id[lane];
      rid = S.esc_pid[lane]; rs = S.esc_pslot[lane];
      esc_here = ref_valid(eid, es);  // an escort that expired by its hard window keeps its map entry (status 2, never popped) ...
      esc_live = esc_here && S.t_status[es] != 2;
    }
    decide();
    // With a RECON type among escort_agent_types a protected UAV can itself hold another UAV's escort task: retiring that escort
    // rewrites its queue (head, idle state), i.e. the verdict of ITS OWN entry further down the map.  Then the entries behind a
    // retirement are decided again on the new state, as the reference's loop sees them (found by tests/fuzz_device.py, config 7178).
    const bool recon_escorts = (P.escort_mask & ((1u << MUAVTA_R1) | (1u << MUAVTA_R2))) != 0u;
    const unsigned long long all = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    unsigned long long rm = __ballot(retire), todo = all;
    PROF_COUNT(56, 1000); PROF_COUNT(57, 1000 * n);
    while (todo) {
      PROF_COUNT(58, 1000);
      const unsigned long long low = todo & (0ull - todo);                 // lowest pending entry
      const unsigned long long nextr = rm & todo;                         // pending retirements
      const unsigned long long seg = nextr ? (todo & ((nextr & (0ull - nextr)) - 1ull)) : todo;  // entries before the next one
      if (seg) {
        // _escort_fighters_near(recon, escort_radius) non-empty? (:1746-1764) for every entry of the segment.  A fighter heads
        // for ONE task, so it can only cover the entry whose escort task that is: each fighter lane finds its entry, runs one
        // distance test (`norm <= radius` on the squared form against the host-side threshold, as in the sensing pass),
        // and the entries collect their fighters' verdicts by ballot.
        const bool fighter = lane < P.n_agents && S.a_state[lane] != -1 && escort_type(S.a_type[lane]) && S.a_qlen[lane] > 0;
        const int head = fighter ? S.a_qid[lane][0] : -1;
        const unsigned long long live_m = __ballot(esc_live);
        int myk = -1, my_recon = 0;
        for (unsigned long long m = seg & live_m; m; m &= m - 1ull) {
          const int k = __ffsll((long long)m) - 1;
          const int ek = __builtin_amdgcn_readlane(eid, k), rk = __builtin_amdgcn_readlane(recon, k);
          if (head == ek) { myk = k; my_recon = rk; }
        }
        bool near = false;
        if (fighter && myk >= 0) {
          const double dx = S.a_px[lane] - S.a_px[my_recon], dy = S.a_py[lane] - S.a_py[my_recon];
          near = fma(dy, dy, dx * dx) <= P.escort_sq_bound;
        }
        unsigned long long cov = 0ull;
        const int neark = near ? myk : -2;
        if (__ballot(near) != 0ull)
          for (unsigned long long m = seg & live_m; m; m &= m - 1ull) {
            const int k = __ffsll((long long)m) - 1;
            if (__builtin_amdgcn_ballot_w64(neark == k) != 0ull) cov |= 1ull << k;
          }
        if ((seg >> lane) & 1ull) {
          if (esc_here) { S.t_px[es] = S.a_px[recon]; S.t_py[es] = S.a_py[recon]; }  // ... and follows the protected UAV (:1995); only coverage asks for status != 2 (:1751)
        }
        if (lane == 0) { S.escort_required_steps += __popcll(seg); S.escort_covered_steps += __popcll(cov); }
        todo &= ~seg;
        lds_sync();
        PROF(60);
      } else {
        const int k = __ffsll((long long)low) - 1;
        const int rk = __builtin_amdgcn_readlane(recon, k), ek = __builtin_amdgcn_readlane(eid, k);
        const bool dk = (__ballot(dead) >> k) & 1ull;
        retire_escort_coop(rk, dk);
        (void)ek;
        todo &= ~low;
        if (recon_escorts && todo) {
          lds_sync();
          decide();
          rm = __ballot(retire);
        }
        PROF(61);
      }
    }
  }

  // The ONE pass over the live task slots of a step (TL::SCAN_ONCE).  step() used to walk S.t_order three times — the sensing candidates
  // (sense_parallel), the pre-checks `expiring` / `blocking` with the pending-reveal test beside them (scan_slots), and the fast-path test
  // of finish_step_parallel — each its own chain "t_order[k] -> that slot's fields -> ballot".  Nothing between the three creates,
  // retires, moves or re-flags a task, except a window expiry in process_lists_coop (see step()), so one walk answers all of them.
  // Two LDS round trips: (1) the list lengths, the lane's t_order / open_slot entry, its pending reveal's time and its agent's state and
  // queue length; (2) the five fields of its slot.  Every index is clamped into its array instead of guarded, so that the loads of a
  // trip do not wait for the lengths; what a lane beyond a list read is masked out of the predicates.
  // Only wave-uniform values leave the pass (SGPRs): nothing per lane stays live across process_lists_coop / step_serial_c.
  struct SlotScan {
    int nc = 0;                 // sensing candidates compacted into X.roundT, in list order (first pass only)
    int n_idle = 0;             // live agents with an empty queue
    bool any_due = false;       // a pending reveal is due (first pass only)
    bool any_expiring = false;  // a hard window ran out on a task that is not retired
    bool any_blocking = false;  // a live task still counts against mission completion
    bool responding = false;    // a live agent has a queue
    bool any_ret = false;       // a listed slot is retired: finish_step_parallel has slots to collect
    bool any_diff = false;      // t_order and open_slot (last_tasks_info) are not the same list
  };
  // first: with the sensing candidates and the pending-reveal test; the pass after an expiry needs neither (sensing comes before
  // reveals and windows, and the reveals of this step are done)
  DEV void slot_pass(SlotScan& sc, bool first, bool sense) {
    const int nO = S.n_order, no = S.n_open, np = S.n_pending;
    const int ai = lane < A ? lane : A - 1;
    const int ast = S.a_state[ai], aql = S.a_qlen[ai];
    bool due = false;
    if (first) {
      if constexpr (R <= WG) { due = lane < np && tnow >= S.pend_time[lane < R ? lane : R - 1]; }
      else for (int k = lane; k < np; k += WG) due |= tnow >= S.pend_time[k];
    }
    const bool want_cand = first && sense && P.sense_radius > 0;
    int16_t* cand = X.roundT;  // T entries
    int nc = 0;
    bool expiring = false, blocking = false, ret = false, diff = false;
#pragma unroll
    for (int base = 0; base < T; base += WG) {
      if (base > 0 && base >= nO) break;  // (uniform)
      const int k = base + lane, ki = k < T ? k : T - 1;
      const bool in = k < nO;
      const int s_ = S.t_order[ki], os = S.open_slot[ki];
      const int s = s_ < T ? s_ : T - 1;  // (an entry beyond the list is whatever the row last held)
      const int fl = S.t_flags[s], st = S.t_status[s], dl = S.t_deadline[s], ty = S.t_type[s], cr = S.t_created[s];
      expiring |= in && (fl & TF_DEADLINE) && st != 2 && tnow > dl;
      blocking |= in && !((fl & TF_ESCORT) || ty == MUAVTA_DET || ty == MUAVTA_HOLD || st == 2);  // !counts_for_mission_done(s)
      ret |= in && st == 2;
      diff |= in && (k >= no || os != s);
      if (want_cand) {  // (uniform) sense_parallel's predicate and compaction
        const bool c = in && st != 2 && !(fl & TF_KNOWN_ALL) && (cr > 0 || (fl & TF_DEADLINE));
        const unsigned long long m = __ballot(c);
        if (c) cand[nc + prefix_count(m)] = s;
        nc += __popcll(m);
      }
    }
    const bool live = lane < P.n_agents && ast != -1;
    if (first) { sc.nc = nc; sc.any_due = __ballot(due) != 0ull; }
    sc.any_expiring = __ballot(expiring) != 0ull;
    sc.any_blocking = __ballot(blocking) != 0ull;
    sc.any_ret = __ballot(ret) != 0ull;
    sc.any_diff = no != nO || __ballot(diff) != 0ull;
    sc.n_idle = __popcll(__ballot(live && aql == 0));
    sc.responding = __ballot(live && aql != 0) != 0ull;
  }

  // _wps_update_sensing (:1506-1523).  First the wave compacts the slots that can be sensed at all (dynamic,
  // open) by ballot; then lane = (agent a, candidate sub-row) with the agent's position in registers.  The
  // test `norm(d) <= sense_radius` is done on the squared form: sqrt is monotone and correctly rounded, so
  // it equals `fma(dy,dy,dx*dx) <= bound` with the bound precomputed on the host (no sqrt per pair).
  // nc_scan (TL::SCAN_ONCE): slot_pass has compacted the candidates already, that many
  DEV void sense_parallel(int nc_scan = 0) {
    if (P.sense_radius <= 0) return;
    const int nA = P.n_agents, nO = S.n_order;
    int16_t* cand = X.roundT;  // T entries
    int nc = 0;
    if constexpr (TL::SCAN_ONCE) nc = nc_scan; else
    for (int base = 0; base < nO; base += WG) {
      const int k = base + lane;
      int s = -1;
      bool c = false;
      if (k < nO) {
        s = S.t_order[k];
        const int fl = S.t_flags[s];
        c = S.t_status[s] != 2 && !(fl & TF_KNOWN_ALL) && (S.t_created[s] > 0 || (fl & TF_DEADLINE));
      }
      const unsigned long long m = __ballot(c);
      if (c) cand[nc + prefix_count(m)] = s;
      nc += __popcll(m);
    }
    if (nc == 0) return;
    lds_sync();
    int aw = 1;
    while (aw < nA) aw <<= 1;               // 16 / 32 / 64
    const int a = lane & (aw - 1), sub = lane / aw, stride = WG / aw;
    if (!(a < nA && S.a_state[a] != -1)) return;
    const double ax = S.a_px[a], ay = S.a_py[a];
    for (int k = sub; k < nc; k += stride) {
      const int s = cand[k];
      if ((S.known[a][s >> 5] >> (s & 31)) & 1u) continue;
      const double dx = ax - S.t_px[s], dy = ay - S.t_py[s];
      if (fma(dy, dy, dx * dx) <= P.sense_sq_bound) atomicOr(&S.known[a][s >> 5], 1u << (s & 31));
    }
  }


  // _wps_process_reveals (:1525-1541) and _wps_expire_windows (:1557-1573), wave-cooperative: due reveals and expired
  // windows are found by ballot and handled in list order; a reveal sets one known bit per agent lane, an expiry
  // frees the agents heading the task (found by ballot, desallocateAll on lane 0 in agent order — the f64 order of
  // removeAgentCap and the list-mutation quirk stay the reference's).
  DEV void process_lists_coop(bool any_due, bool any_exp) {
    const unsigned long long below = (1ull << lane) - 1ull;
    if (any_due) {
      const int n = S.n_pending;
      int w = 0;
      for (int base = 0; base < n; base += WG) {
        const int k = base + lane;
        int pt = 0, pid = -1, psl = 0;
        typename KnowMask<A>::type pk = 0;
        if (k < n) { pt = S.pend_time[k]; pid = S.pend_id[k]; psl = S.pend_slot[k]; pk = S.pend_know[k]; }
        const bool due = k < n && tnow >= pt;
        const unsigned long long dm = __ballot(due), km = __ballot(k < n && !due);
        if (P.share_knowledge) {
          for (unsigned long long m = dm; m; m &= m - 1ull) {
            const int b = __ffsll((long long)m) - 1;
            const int id = __builtin_amdgcn_readlane(pid, b), sl = __builtin_amdgcn_readlane(psl, b);
            if (ref_valid(id, sl)) {
              if (lane < P.n_agents) S.known[lane][sl >> 5] |= 1u << (sl & 31);
              if (lane == 0) S.t_flags[sl] |= TF_KNOWN_ALL;
            } else if (lane < P.n_agents) {  // released before the reveal: the id still joins the set of everyone who had not sensed it
              const unsigned long long kn = (unsigned long long)S.pend_know[base + b];
              S.a_gone[lane] += !((kn >> lane) & 1ull);
            }
          }
        }
        lds_sync();  // every lane holds its entry before the survivors are packed to the front
        if (k < n && !due) {
          const int d = w + prefix_count(km);
          S.pend_time[d] = pt; S.pend_id[d] = pid; S.pend_slot[d] = (uint8_t)psl; S.pend_know[d] = pk;
        }
        w += __popcll(km);
      }
      if (lane == 0) S.n_pending = w;
      lds_sync();
    }
    if (any_exp) {
      const int n = S.n_order;
      for (int base = 0; base < n; base += WG) {
        const int k = base + lane;
        int sl = -1;
        bool ex = false;
        if (k < n) {
          sl = S.t_order[k];
          ex = (S.t_flags[sl] & TF_DEADLINE) && S.t_status[sl] != 2 && tnow > S.t_deadline[sl];
        }
        for (unsigned long long m = __ballot(ex); m; m &= m - 1ull) {
          const int b = __ffsll((long long)m) - 1;
          const int s_ = __builtin_amdgcn_readlane(sl, b);
          const int id = S.t_id[s_];
          const unsigned long long hm = __ballot(lane < P.n_agents && S.a_qlen[lane] > 0 && S.a_qid[lane][0] == id);
          if (lane == 0) {
            S.t_status[s_] = 2;
            mark_outcome_slot(s_, false);
            if (!(S.t_flags[s_] & TF_REACHED)) { S.t_flags[s_] |= TF_REACHED; S.n_reached++; }
            for (unsigned long long h = hm; h; h &= h - 1ull) desallocate_all(__ffsll((long long)h) - 1);
          }
          lds_sync();  // the next expiry looks at the queues this one just changed
        }
      }
    }
  }
  // reserve tracking (:1575-1580), pending-reset latch (:1156-1160), shared reward (:1162-1178), done flags
  DEV void step_serial_c(double action_reward, double distance_reward, double quality_reward, double S_quality_reward,
                         int idle, bool responding, bool all_done_tasks) {
    // every LDS operand first (one wait), then arithmetic, then the stores
    const int irs = S.idle_reserve_steps, pr = S.pending_reset, ntid = S.next_task_id, ct = S.conclusion_time;
    const double time_penaulty = S.r_time_penalty, alloc_reward = S.r_alloc, step_reward = S.step_reward, FR = S.F_Reward;
    PROF(36);
    // Most steps add nothing to any reward term (no action applied, no task concluded): with finite weights >= 0 every product is then
    // +0.0, their sum is +0.0 and so is the quotient — the 15 dependent multiply-adds and two divisions on lane 0's chain are skipped.
    // (bit patterns, not values: a -0.0 term would make the reference's sum depend on the order of the signed zeros)
    const unsigned long long any_bits = (unsigned long long)__double_as_longlong(action_reward) | (unsigned long long)__double_as_longlong(distance_reward) |
                                        (unsigned long long)__double_as_longlong(quality_reward) | (unsigned long long)__double_as_longlong(S_quality_reward) |
                                        (unsigned long long)__double_as_longlong(alloc_reward) | (unsigned long long)__double_as_longlong(time_penaulty) |
                                        (unsigned long long)__double_as_longlong(step_reward);
    const bool quiet_reward = P.rw_plain && any_bits == 0ull;
    double total = 0.0;
    if (!quiet_reward)
    total = P.rw[0] * action_reward + P.rw[1] * distance_reward + P.rw[2] * quality_reward + P.rw[3] * S_quality_reward +
                   P.rw[4] * (double)P.n_tasks * 0.0 + P.rw[5] * alloc_reward + P.rw[6] * time_penaulty + P.rw[7] * step_reward;
    PROF(37);
    // two divisions on lane 0's chain in EVERY step: the range-restricted sequence (8 VALU each, bit-identical to IEEE inside its
    // domain: `total` is 0 or a sum of reward terms of ordinary magnitude, the divisors are a positive constant >= 0.002 and a step
    // count) instead of the compiler's ~35-instruction expansion.  A configuration without static tasks has reward_norm_factor == 0
    // (the reference raises ZeroDivisionError in its first step): that one keeps the plain division.
    const double shared = quiet_reward ? 0.0
                          : P.reward_norm_factor != 0 ? fdiv(fdiv(total, P.reward_norm_factor), (double)P.max_time_steps)
                                                      : total / P.reward_norm_factor / (double)P.max_time_steps;
    PROF(38);
    const bool all_done = (ntid > 1) && all_done_tasks;
    const bool timed_out = (tnow >= P.max_time_steps) && (P.max_time_steps > 0);
    const bool done = timed_out || (P.early_terminate && all_done);
    S.idle_reserve_steps = irs + idle;
    if (pr && responding) S.pending_reset = 0;
    if (all_done && ct > P.max_time_steps) S.conclusion_time = tnow;
    S.terminated = P.early_terminate && all_done && !timed_out;
    S.truncated = timed_out;
    S.last_reward = done ? FR : shared;  // :1202
  }

  // ---------------------------------------------------------------- end of step: slot GC + open list
  // Retired slots are recycled unless a LIVE agent still queues them (their type/position is read by
  // the switch penalty and expected-distance terms, :852-861,:1219-1220).  Parallel over slots.
  // sc (TL::SCAN_ONCE): step()'s slot pass holds the fast-path test already — on the steps that take it (most: no task created or retired) the
  // lists are not walked again.  (The other steps walk them below as before: they are about to rewrite both lists anyway.)
  DEV void finish_step_parallel(bool gc, const SlotScan* sc = nullptr) {
    if constexpr (TL::SCAN_ONCE) {
      if (gc && sc && !sc->any_ret && !sc->any_diff) {  // the fast path below
        if (lane == 0) { S.n_act = 0; S.list_stale = 0; }
        lds_sync();
        return;
      }
    }
    if (gc) {
      // fast path: no live slot is retired and every live slot is already listed as open (no task was created
      // or retired since the lists were built) -> t_order / last_tasks_info are unchanged
      // (... and the two lists really are the same list: with the tile FULL, a task concluded in this step can have had its slot
      // recycled on demand for a task created in the same step — no retired slot is left and the counts agree, but that slot now
      // sits at the END of t_order and still at its old row of last_tasks_info.  Found by tests/fuzz_device.py, config 1000488.)
      const int n = S.n_order, no = S.n_open;
      bool ret = false, diff = false;
      for (int k = lane; k < n; k += WG) {
        const int s = S.t_order[k];
        ret |= S.t_status[s] == 2;
        diff |= k >= no || (int)S.open_slot[k] != s;
      }
      const bool any_ret = __ballot(ret) != 0ull;
      if (!any_ret && no == n && __ballot(diff) == 0ull) {
        if (lane == 0) { S.n_act = 0; S.list_stale = 0; }  // (the two lists are identical: nothing is newer than last_tasks_info, whatever an out-of-step call flagged)
        lds_sync();
        return;
      }
#ifdef MUAVTA_PROF
      PROF_COUNT(30, 1000); if (any_ret) PROF_COUNT(31, 1000);
#endif
      if (any_ret) {
        if (rel_log) cold_sync();
        // slots still queued by a live agent (one agent per lane marks its queue entries), then the retired and
        // unreferenced ones are released (one slot per lane), then every agent lane drops the released columns
        // from its known mask and counts them into a_gone
        uint32_t* refmask = reinterpret_cast<uint32_t*>(X.path);
        uint32_t* relmask = refmask + KW;
        if (lane < 2 * KW) refmask[lane] = 0;
        lds_sync();
        if (lane < P.n_agents && S.a_state[lane] != -1) {
          const int ql = S.a_qlen[lane];
          for (int k = 0; k < ql; k++) {
            const int qs = S.a_qslot[lane][k];
            if (ref_valid(S.a_qid[lane][k], qs)) atomicOr(&refmask[qs >> 5], 1u << (qs & 31));
          }
        }
        lds_sync();
        for (int k = lane; k < n; k += WG) {
          const int s = S.t_order[k];
          if (S.t_status[s] == 2 && !((refmask[s >> 5] >> (s & 31)) & 1u)) {
            release_slot_record(s);
            atomicOr(&relmask[s >> 5], 1u << (s & 31));
          }
        }
        lds_sync();
        if (lane < P.n_agents) {
          int gone = 0;
          for (int w = 0; w < KW; w++) {
            const uint32_t m = relmask[w];
            if (m) { const uint32_t old = S.known[lane][w]; gone += __popc(old & m); S.known[lane][w] = old & ~m; }
          }
          if (gone) S.a_gone[lane] += gone;
        }
        if (lane < KW) S.free_slots[lane] |= relmask[lane];
        lds_sync();
      }
      PROF(35);
    }
    {  // compact t_order (drop freed slots) and rebuild last_tasks_info (:492) with ballot + popcount
      const int n = S.n_order, no_old = S.n_open;
      int w = 0, no = 0;
      bool moved = false;  // some row of last_tasks_info holds another task than before (the observation rows' static columns follow the list)
      for (int base = 0; base < n; base += WG) {
        const int k = base + lane;
        int s = -1;
        bool alive = false, open = false;
        if (k < n) {
          s = S.t_order[k];
          alive = S.t_id[s] >= 0;
          open = alive && S.t_status[s] != 2;
        }
        const unsigned long long am = __ballot(alive), om = __ballot(open);
        const unsigned long long below = (1ull << lane) - 1ull;
        lds_sync();  // every lane has read its t_order entry before any is overwritten
        if (alive) S.t_order[w + prefix_count(am)] = s;
        if (open) {
          const int row = no + prefix_count(om);
          moved |= row >= no_old || (int)S.open_slot[row] != s;  // (a row is only ever rewritten by the lane that holds its new content: rows ascend with k)
          S.open_slot[row] = s; S.t_row[s] = (uint8_t)row;
        }
        w += __popcll(am);
        no += __popcll(om);
      }
      const bool list_changed = __ballot(moved) != 0ull || no != no_old;
      if (lane == 0) { S.n_order = w; S.n_open = no; S.n_act = 0; S.list_stale = 0; if (list_changed) obs_static_clear(); }
    }
    lds_sync();
  }

