// sim/step.inc — member functions of Sim<TL> (muavta_device.h includes this file INSIDE the struct body): MultiUAVEnv.step: the phase sequence and the movement state machine.
  // ====================================================================================================
  // step (:774-1206).  n_act staged actions in S.act_agent / S.act_slot (slot < 0: invalid index).
  // ====================================================================================================
  // np.sum of n <= 128 doubles with numpy's pairwise order: 8 strided accumulators r[k] (one per lane),
  // combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 tail added in order; plain loop for n < 8.
  DEV double np_sum_wave(const double* d, int n) {
    double res;
    if (n < 8) {
      res = 0.;
      for (int i = 0; i < n; i++) res += d[i];
      return res;
    }
    const int body = n - (n % 8);
    double r = 0.;
    if (lane < 8) {
      r = d[lane];
      for (int i = 8 + lane; i < body; i += 8) r += d[i];
    }
    r = r + dpp_xchg(r, 0);   // lanes 2m, 2m+1: r[2m] + r[2m+1]
    r = r + dpp_xchg(r, 1);   // quads: (r0+r1)+(r2+r3) | (r4+r5)+(r6+r7)
    r = r + dpp_xchg(r, 2);   // row_half_mirror pairs the two quads of lanes 0..7
    res = readlane_f64(r, 0);
    for (int i = body; i < n; i++) res += d[i];
    return res;
  }

  // The same sum for up to 16 elements held one per lane (lane i: element i): the second eight join the first through a row
  // shift, the tail comes through v_readlane — no scratch row, no LDS round trips.  Same additions in the same order.
  DEV double np_sum_lanes16(double d, int n_) {
    const int n = __builtin_amdgcn_readfirstlane(n_);
    double res;
    if (n < 8) {
      res = 0.;
      for (int i = 0; i < n; i++) res += readlane_f64(d, i);
      return res;
    }
    const int body = n - (n % 8);
    double r = d;
    if (body == 16) {  // lanes 0..7: d[j] + d[8 + j]   (row_shl:8, lanes 8..15 read beyond the row: 0)
      const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(d), 0x108, 0xf, 0xf, true);
      const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(d), 0x108, 0xf, 0xf, true);
      r = d + __hiloint2double(hi, lo);
    }
    r = r + dpp_xchg(r, 0);
    r = r + dpp_xchg(r, 1);
    r = r + dpp_xchg(r, 2);
    res = readlane_f64(r, 0);
    for (int i = body; i < n; i++) res += readlane_f64(d, i);
    return res;
  }

  DEV void step(bool write_obs_flag) {
    PROF(0);
    in_step = true;
    uint32_t rng_words = 0;
    if (!ABL(0)) { rng_refill(); rng_words = rng_prefetch_issue(); }
    PROF(1);
    // previous positions stay in registers of the lane that owns the agent
    double prev_x = 0, prev_y = 0;
    if (lane < P.n_agents) { prev_x = S.a_px[lane]; prev_y = S.a_py[lane]; }
    lds_sync();
    double r_action = 0, r_distance = 0, r_quality = 0, r_squality = 0;
    {
      // drain the event queue (:800-805): infos['events'] := event_list, every Reset_Allocation in order
      const int nev = S.n_events;
      for (int k = lane; k < nev; k += WG) { S.dev_tag[k] = S.ev_tag[k]; S.dev_arg[k] = S.ev_arg[k]; }
      tnow += 1;
      if (lane == 0) { S.step_reward = 0; S.time_steps = tnow; S.n_dev = nev; S.n_events = 0; }  // :796
      lds_sync();
      int last_arg = -1000;
      bool last_changed = true;
      if (!ABL(1))
      for (int k = 0; k < nev; k++)
        if (S.dev_tag[k] == MUAVTA_EV_RESET_ALLOCATION) {
          const int arg = S.dev_arg[k];
          if (arg == last_arg && !last_changed) continue;  // same call on unchanged state: nothing to do
          last_changed = release_all_tasks_coop(arg);
          last_arg = arg;
        }
    }
    PROF(2);
    if (!ABL(2))
    for (;;) {
      if (S.n_act > 0 && !apply_actions_parallel(r_action, r_distance, r_squality)) {
        precompute_actions();
        lds_sync();
        PROF(33);
        if (lane == 0) step_serial_a(r_action, r_distance, r_quality, r_squality);
        cold_sync();
      }
      // a list longer than the staging arrays (muavta_step_lists) is applied A items at a time, in order: the loop of
      // DroneEnv.py:813-933 is sequential, so chunks applied one after the other are the same sequence
      if (!more_agent || stage_more() == 0) break;
    }
    PROF(3);
    // movement (:965-1129): lanes commit every agent up to the first "event" agent, lane 0 plays that one
    // agent exactly as the reference does, and the wave resumes behind it
    for (int start = ABL(3) ? P.n_agents : 0; start < P.n_agents;) {
      bool popped = false;
      const int first = move_parallel(start, popped);
      // (lanes that dropped a retired head shifted their EnvCold queue-time row: only then do the HBM stores have to be drained.  An
      // unconditional vmcnt(0) here — half a microsecond after the step issued its RNG-window loads and a few after the previous step's
      // observation stores — waited for all of those in every step)
      if (popped) cold_sync(); else lds_sync();
      PROF(26);
#ifdef MUAVTA_PROF
      PROF_COUNT(40, 1000); if (first < P.n_agents) PROF_COUNT(41, 1000);
#endif
      if (first >= P.n_agents) break;
      if (lane == 0) step_serial_move(first, first + 1, r_quality);
      cold_sync();  // (a concluded task / retired escort rewrites other agents' queue rows: the next pass reads them)
      PROF(4);
      start = first + 1;
    }
    // distances (:1131-1138): np.linalg.norm(axis=1) == sqrt(x*x + y*y), no fma
    double dist_sum = 0.0;
    if (!ABL(4)) {
      double d = 0.0;
      if (lane < P.n_agents) {
        double dx = S.a_px[lane] - prev_x, dy = S.a_py[lane] - prev_y;
        d = fsqrt(dx * dx + dy * dy);
        S.a_dist[lane] += d;
        if constexpr (A > 16) X.u[lane] = d;
      }
      if constexpr (A <= 16) dist_sum = np_sum_lanes16(d, P.n_agents);  // np.sum(dists) (:1138)
      else { lds_sync(); dist_sum = np_sum_wave(X.u, P.n_agents); }
    }
    if (!ABL(0)) rng_prefetch_commit(rng_words);
    PROF(5);
    if (!ABL(5)) {
    precompute_threat_targets();
    if (lane == 0) step_serial_b(dist_sum);
    lds_sync();
    }
    if (!ABL(5))
    {  // update_threats (:1725-1744): lanes advance every threat up to the first one that engages or leaves the area,
       // lane 0 plays that one as the reference does, and the wave resumes behind it
      unsigned long long livemask = 0ull;
      if (lane == 0) X.retarget_h = -1;  // (scratch: set before any replay of this phase can post a request, read behind an lds_sync)
      if (!P.escort_enabled) {
        // Without escorts a threat's turn reads nothing another threat's turn writes (own record, own Int task, agent POSITIONS —
        // an engagement changes agents' states and queues, which only _retarget_threat_via_escort looks at): one pass decides
        // every threat, the non-event ones commit at once, and lane 0 replays the event threats in env.threats order (the
        // shared RNG stream and the counters see them in the reference's sequence).
        const unsigned long long em = update_threats_parallel(0, livemask, true);
        lds_sync();
        PROF(23);
        PROF_COUNT(54, 1000);
        if (em) {
          PROF_COUNT(55, 1000 * __popcll(em));
          for (unsigned long long m = em; m; m &= m - 1ull) {
            if (lane == 0) update_threats_serial(__ffsll((long long)m) - 1, livemask);
            lds_sync();
            resolve_retarget();
          }
        }
      } else
      for (int start = 0;;) {
        const int first = (int)update_threats_parallel(start, livemask, false);
        lds_sync();
        PROF(23);
        PROF_COUNT(54, 1000);
        if (first >= S.n_active_threats) break;
        PROF_COUNT(55, 1000);
        if (lane == 0) update_threats_serial(first, livemask);
        lds_sync();
        resolve_retarget();
        start = first + 1;
      }
      if (lane == 0) step_serial_b2();
    }
    lds_sync();
    if constexpr (TL::SCAN_ONCE) { step_tail_one_pass(r_action, r_distance, r_quality, r_squality); return; }
    if (!ABL(6)) {
    if (P.escort_enabled) sync_escorts_coop();
    PROF(6);
    sense_parallel();  // _wps_update_sensing (:1506-1523)
    lds_sync();
    }
    PROF(7);
    if (!ABL(7))
    {
      // wave-wide pre-checks so that lane 0 only walks the lists when something is due this step.  ONE pass over the live
      // slots gives both "a window expired" and "a task still blocks mission completion"; the agents' idle / responding
      // flags are read alongside.  Only a window expiry (status changes, agents freed) invalidates them: evaluated again then.
      bool due = false, expiring = false, idle = false, resp = false, blocking = false;
      if (!ABL(12)) for (int k = lane; k < S.n_pending; k += WG) due |= tnow >= S.pend_time[k];
      auto scan_slots = [&]() {
        expiring = false; blocking = false;
        for (int k = lane; k < S.n_order; k += WG) {
          const int s = S.t_order[k];
          const int fl = S.t_flags[s], st = S.t_status[s], dl = S.t_deadline[s], ty = S.t_type[s];
          expiring |= (fl & TF_DEADLINE) && st != 2 && tnow > dl;
          blocking |= !((fl & TF_ESCORT) || ty == MUAVTA_DET || ty == MUAVTA_HOLD || st == 2);  // !counts_for_mission_done(s)
        }
        idle = false; resp = false;
        if (lane < P.n_agents && S.a_state[lane] != -1) { idle = S.a_qlen[lane] == 0; resp = !idle; }
      };
      if (!ABL(12)) scan_slots();
      const bool any_due = __ballot(due) != 0ull;
      const bool any_exp = P.hard_windows && __ballot(expiring) != 0ull;
      PROF(28);
      if (any_due || any_exp) process_lists_coop(any_due, any_exp);
      lds_sync();
      PROF(29);
      if (any_exp) scan_slots();
      const int n_idle = __popcll(__ballot(idle));
      const bool responding = __ballot(resp) != 0ull;
      const bool all_done_tasks = __ballot(blocking) == 0ull;
      PROF(32);
      if (!ABL(11) && lane == 0) step_serial_c(r_action, r_distance, r_quality, r_squality, n_idle, responding, all_done_tasks);
    }
    lds_sync();
    PROF(8);
    if (!ABL(8)) finish_step_parallel(true);
    PROF(9);
  }
  // The rest of step() behind the threat update where the tile walks its live slots once (TL::SCAN_ONCE): escort sync, sensing, reveals
  // and windows, the reward / done bookkeeping and the end-of-step GC, in the order above.  The pass sits behind the last phase that
  // can create, retire or move a task before sensing (step_serial_b2, or the escort sync where escorts are enabled).
  // What its results rest on: between the pass and finish_step_parallel only process_lists_coop touches a task, a pending reveal
  // or an agent's queue.  A due reveal sets TF_KNOWN_ALL and `known` bits, adds to a_gone and packs the pending list — nothing
  // behind sensing reads any of them in this step.  A window expiry sets status 2 and TF_REACHED and empties the queues of the
  // agents heading the task: `blocking`, `ret`, the agents' idle / responding flags change, so the pass is taken again behind it
  // (as the second scan_slots() and the walk of finish_step_parallel did).  t_order / open_slot / n_order / n_open are written
  // by neither, nor by sensing or step_serial_c.
  DEV void step_tail_one_pass(double r_action, double r_distance, double r_quality, double r_squality) {
    SlotScan sc;
    if (!ABL(6) && P.escort_enabled) sync_escorts_coop();
    PROF(6);
    slot_pass(sc, true, !ABL(6));
    if (!ABL(6)) sense_parallel(sc.nc);  // _wps_update_sensing (:1506-1523): before the reveals
    lds_sync();
    PROF(7);
    if (!ABL(7))
    {
      const bool any_due = !ABL(12) && sc.any_due;
      const bool any_exp = !ABL(12) && P.hard_windows && sc.any_expiring;
      PROF(28);
      if (any_due || any_exp) process_lists_coop(any_due, any_exp);
      lds_sync();
      PROF(29);
      if (any_exp) slot_pass(sc, false, false);
      PROF(32);
      if (!ABL(11) && lane == 0) step_serial_c(r_action, r_distance, r_quality, r_squality, sc.n_idle, sc.responding, !sc.any_blocking);
    }
    lds_sync();
    PROF(8);
    if (!ABL(8)) finish_step_parallel(true, &sc);
    PROF(9);
  }

  DEV void displacement(double px, double py, double ux, double uy, double speed, double& ddx, double& ddy) {
    double avx, avy;
    avoid_obstacles(px, py, ux, uy, avx, avy);
    double mx = ux + avx, my = uy + avy;  // :1123
    norm_vector(mx, my);
    ddx = mx * speed; ddy = my * speed;
  }
  // The movement state machine (:965-1129) with one agent per lane.  An agent's turn only touches its own
  // fields unless it (a) fails, (b) engages an Int task (rewrites the threat's target) or (c) concludes a
  // task; those are "events".  Agents in [start, first event) are independent of everything later in the
  // loop and commit their lane's result.  An agent either heads for its current task or (idle) for the
  // base, never both, so each lane runs ONE distance / unit-vector / displacement pipeline.
  // Returns the index of the first event agent >= start (n_agents if none).
  DEV int move_parallel(int start, bool& popped) {
    const int a = lane;
    const bool in_fleet = a >= start && a < P.n_agents;
    const int ai = in_fleet ? a : 0;  // (lanes outside the fleet read agent 0's fields and discard them)
    // Every operand of the lane's agent is read up front — two LDS round trips (agent fields, then the fields of the task
    // they point to) instead of one per branch of the state machine; the values of untaken branches are simply unused.
    const int st0 = S.a_state[ai], fail_at = S.a_fail[ai], ts0 = S.a_task_start[ai], qlen = S.a_qlen[ai], reeval = S.a_reeval[ai];
    const int atype = S.a_type[ai];
    const int last_id = S.a_last_id[ai], last_slot = S.a_last_slot[ai], head_id_ = S.a_qid[ai][0], head_slot = S.a_qslot[ai][0];
    double px = S.a_px[ai], py = S.a_py[ai];
    const bool live = in_fleet && st0 != -1;
    int cid = 0, cs = -1;
    if (reeval) { cid = last_id; cs = last_slot; }
    else if (qlen > 0) { cid = head_id_; cs = head_slot; }
    const int csi = cs >= 0 ? cs : 0;
    const int tid_at = S.t_id[csi], tstat = S.t_status[csi], ty = S.t_type[csi];
    const double tpx = S.t_px[csi], tpy = S.t_py[csi];
    bool evt = false, pop_head = false;
    int new_st = 0, new_ts = 0;
    double ddx = 0.0, ddy = 0.0;
    if (live) {
      if (fail_at == tnow) {
        evt = true;
      } else {
        const double speed = speed_of(atype);
        new_st = st0; new_ts = ts0;
        const bool retired = cid != 0 && (!(cs >= 0 && tid_at == cid) || tstat == 2);  // ref_retired(cid, cs)
        const bool to_task = cid != 0 && !retired;
        const bool idle_check = new_st == 0 && !reeval && qlen == 0;    // :987-993
        const bool to_base = !to_task && (idle_check || new_st == 3);
        if (retired) pop_head = true;  // :1004-1007, own queue only (the task is retired: removeAgentCap is a no-op)
        if (to_task || to_base) {
          // vector to the target, its norm, unit vector, displacement — identical arithmetic on both paths:
          // task: dir/dist with the EPS guard (:1014-1020); base: norm_vector(base - pos) (:1119) whose norm
          // equals norm(pos - base) used by the distance tests (:992,:1116)
          const double tx = to_task ? tpx : BASE_X, ty_ = to_task ? tpy : BASE_Y;
          const double dx = tx - px, dy = ty_ - py;
          const double dist = norm2(dx, dy);
          double ux = 0, uy = 0;
          const bool zero = to_task ? (fabs(dist) < 1e-12) : (dist == 0);
          if (!zero) { const double r = frcp_nr(dist); ux = fdiv_r(dx, dist, r); uy = fdiv_r(dy, dist, r); }
          double ndx, ndy;
          displacement(px, py, ux, uy, speed, ndx, ndy);
          if (to_task) {
            const double engage = engage_range(atype);
            if (new_st == 1) {
              if (ty == MUAVTA_INT) {
                if (dist < engage) evt = true;
                else { ddx = ndx; ddy = ndy; }
              } else if (dist < speed) {
                new_st = 2; new_ts = tnow;
                px = tpx; py = tpy;
              } else { ddx = ndx; ddy = ndy; }
            } else if (new_st == 2) {
              if (ty == MUAVTA_INT && dist >= engage) new_st = 1;
              if (new_ts == -1) {
                new_ts = tnow;
                px = tpx; py = tpy;
              } else if ((tnow - new_ts) >= task_duration(ty) && ty != MUAVTA_HOLD && ty != MUAVTA_DEF &&
                         ty != MUAVTA_INT && ty != MUAVTA_DET) {
                evt = true;
              }
            }
          } else {
            if (idle_check && dist > speed + 5) new_st = 3;
            if (new_st == 3) {  // :1114-1121
              if (dist < speed + 5) new_st = 0;
              else { ddx = ndx; ddy = ndy; }
            }
          }
        }
      }
    }
    const unsigned long long em = __ballot(evt);
    const int first = em ? __ffsll((long long)em) - 1 : P.n_agents;
    PROF(34);
    popped = __ballot(live && a < first && pop_head) != 0ull;  // (uniform)
    if (live && a < first) {  // commit: own fields only
      if (pop_head) {
        des_allocate(a, cid);
        S.a_reeval[a] = 0;
        S.a_last_id[a] = -1; S.a_last_slot[a] = -1;
      }
      S.a_state[a] = new_st;
      S.a_task_start[a] = new_ts;
      px = px + ddx; py = py + ddy;  // :1125-1127
      S.a_px[a] = fmin(fmax(px, 0.0), AREA_W);
      S.a_py[a] = fmin(fmax(py, 0.0), AREA_H);
    }
    return first;
  }

  // events drain, action application, movement state machine
  // Geometry of the staged actions, one action per lane (each agent appears at most once per step on the
  // allocator path; repeated agents fall back to the inline computation): distance to the current head and to
  // the new task (switch penalty :859-861), time_to_task of UAV.allocate (DroneEnvComponents.py:64) and the
  // expected-distance term (:1216-1229).  Agent / task positions do not change while actions are applied.
  DEV double* act_f(int k) { return X.cost + k * A; }   // 4 arrays of A doubles in the idle cost tile
  DEV void precompute_actions() {
    cold_sync();  // next_free_position rows: written by whichever lane ran the previous phases
    const int k = lane;
    if (k >= S.n_act) return;
    const int a = S.act_agent[k], s = S.act_slot[k];
    X.remaining[k] = -1;  // validity tag: agent id
    if (a < 0 || s < 0 || S.a_state[a] == -1) return;
    const double px = S.a_px[a], py = S.a_py[a], tx = S.t_px[s], ty = S.t_py[s];
    double d_old = 0;
    if (S.a_qlen[a] > 0) { const int hs = S.a_qslot[a][0]; d_old = norm2(px - S.t_px[hs], py - S.t_py[hs]); }
    act_f(0)[k] = d_old;
    act_f(1)[k] = norm2(px - tx, py - ty);
    act_f(2)[k] = fdiv(norm2(qs().a_nfx[a] - tx, qs().a_nfy[a] - ty), speed_of(S.a_type[a]));
    const int n = S.a_qlen[a];  // after the append the queue holds n + 1 entries; tasks[-2] is the current last one
    double total;
    if (n >= 1) { const int ps = S.a_qslot[a][n - 1]; total = norm2(tx - S.t_px[ps], ty - S.t_py[ps]); }
    else total = norm2(tx - px, ty - py);
    act_f(3)[k] = -div_coord(total);
    bool dup = false;
    // (kept rolled: unrolled 32-fold with one scalar accumulator pair per element it alone spilled 90 SGPRs)
#pragma clang loop unroll(disable) vectorize(disable)
    for (int q = 0; q < k; q++) dup |= S.act_agent[q] == a;
    if (!dup) X.remaining[k] = a;
  }

