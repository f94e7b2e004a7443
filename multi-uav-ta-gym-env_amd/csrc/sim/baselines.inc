// sim/baselines.inc — member functions of Sim<TL> (muavta_device.h includes this file INSIDE the struct body): the two classical
// baselines of the reference's tables, MUAVTA_ALLOC_CAP_GREEDY and MUAVTA_ALLOC_PI (include/muavta.h).  Compiled only into the
// baseline instantiations of k_rollout / k_allocate (AllocBaseline): the Hungarian kernels do not carry this code.
// Result: S.act_agent / S.act_slot / S.act_index, S.n_act, with the _apply_assign filter of the Hungarian path (a task that is
// not in env.last_tasks_info is dropped; experiments/wps_eval.py:55-61).
  // str(x) < str(y) for x, y >= 0: digit strings compare as the numbers padded to the same length, a prefix sorts first
  static DEV bool dec_less(int x, int y) {
    int nx = 1, ny = 1;
    for (int v = x; v >= 10; v /= 10) nx++;
    for (int v = y; v >= 10; v /= 10) ny++;
    long long px = x, py = y;
    for (int k = nx; k < ny; k++) px *= 10;
    for (int k = ny; k < nx; k++) py *= 10;
    return px < py || (px == py && nx < ny);
  }
  // slot s in env.last_tasks_info (_apply_assign keeps only those tasks)
  DEV bool in_last_list(int s) const { const int r = S.t_row[s]; return r < S.n_open && (int)S.open_slot[r] == s; }
  DEV bool queues_task(int a, int id) const {  // agent.id in task.allocationDetails (the device keeps the details in the queues)
    const int n = S.a_qlen[a];
    bool hit = false;
    for (int k = 0; k < n; k++) hit |= S.a_qid[a][k] == id;
    return hit;
  }
  DEV bool knows(int a, int s) const { return ((S.known[a][s >> 5] >> (s & 31)) & 1u) != 0; }

  // _open_tasks(env) (experiments/paper_eval.py:85-101): env.tasks order, id != 0, status != 2, residual demand > 0 (coalition
  // residual = required_agents - len(allocationDetails)) -> X.roundT[0, n); X.resid[s] = residual.  Reads the HBM requirement rows.
  DEV int baseline_open_tasks() {
    cold_sync();
    const int n = compact_to(X.roundT, S.n_order, [&](int k) {
      const int s = S.t_order[k];
      const double r = (S.t_id[s] != 0 && S.t_status[s] != 2) ? residual_demand(s) : 0.0;
      X.resid[s] = r;
      return r > 0;
    }, [&](int k) { return (int)S.t_order[k]; });
    lds_sync();
    return n;
  }

  DEV void allocate_baseline(int interval, int use_visibility, int mode) {
    PROF(10);
    if (lane == 0) { S.n_act = 0; S.n_calls++; }
    const bool envvis = !(P.sense_radius == 0 && P.threat_delay == 0);  // agent_visibility_map() is not None
    const bool vis = use_visibility && envvis;                            // use_visibility = 0: agent_known_ids=None
    if (mode == MUAVTA_ALLOC_CAP_GREEDY) cap_greedy(vis);
    else pi_plan(interval, vis);
    lds_sync();
    PROF(11);
  }

  // ---- Local-Cap-Greedy: CapabilityGreedy.allocate_tasks(get_live_agents(), _open_tasks(env)) every step, then the harness's filters
  // (TaskAllocation/BehaviourBased/CapabilityGreedy.py:14-47; experiments/wps_eval.py:160-167) ----
  DEV void cap_greedy(bool vis) {
    if (lane == 0) S.gate_step = tnow + 1;
    const int nt = baseline_open_tasks();
    const int nl = compact_to(X.freeA, P.n_agents, [&](int a) { return S.a_state[a] != -1; }, [&](int a) { return a; });
    lds_sync();
    // score = min(cap, missing) * 10.0 - dist / 1000.0 over (live agent, task with allocatedReqs < currentReqs at its type index);
    // the FIRST strict maximum in agent-major order wins: key (score desc, pair index asc), pair index = i * nt + j
    double best = -__builtin_inf();
    int bp = 0x7fffffff;
    for (int p = lane; p < nl * nt; p += WG) {
      const int i = p / nt, j = p - i * nt;
      const int a = X.freeA[i], s = X.roundT[j], ty = S.t_type[s];
      const double cur = C.t_cur[ty][s], al = C.t_alloc[ty][s];
      if (!(al < cur)) continue;
      const double cap = S.a_caps[ty][a];
      if (cap <= 1e-6) continue;
      const double missing = fmax(cur - al, 0.0);
      if (missing <= 0) continue;
      const double dist = norm2(S.a_px[a] - S.t_px[s], S.a_py[a] - S.t_py[s]);
      const double score = fmin(cap, missing) * 10.0 - div_small(dist, 1000.0, 1.0 / 1000.0);
      if (score > best) { best = score; bp = p; }  // (p ascends within a lane: ties keep the earlier pair)
    }
    for (int off = 1; off < WG; off <<= 1) {
      const double ob = __shfl_xor(best, off);
      const int op = __shfl_xor(bp, off);
      if (ob > best || (ob == best && op < bp)) { best = ob; bp = op; }
    }
    if (bp != 0x7fffffff && lane == 0) {  // (uniform)
      const int i = bp / nt, j = bp - i * nt;
      const int a = X.freeA[i], s = X.roundT[j];
      if (S.n_open > 0 && in_last_list(s) && (!vis || knows(a, s))) {  // `task in last_tasks_info`, `task.id in vis[agent]`
        S.act_agent[0] = (i8)a; S.act_slot[0] = (i8)s; S.act_index[0] = (i16)S.t_row[s]; S.n_act = 1;
      }
    }
  }

  // ---- Local-PI: PerformanceImpact.allocate_tasks(get_live_agents(), _open_tasks(env), time_step, events, agent_known_ids,
  // max_tasks_per_agent=1) (TaskAllocation/MarketBased/PerformanceImpact.py:49-223; CBBA.py:10-65; experiments/wps_eval.py:147-159,
  // escort_eval.py:162-175).  With one slot per agent every path is empty or one slot long, so for agent a and task s
  //   ipi = provisional rpi = rpi = _path_cost([s]) = start + [200 + (start - deadline) if start > deadline] - 5 * cap',
  //   start = max(next_free_time, t) + |position - task.position| / max_speed,
  // infeasible (ipi = inf) when start > hard_deadline + 1e-6; cap' = max(cap, 0.5) on coalition tasks.  The consensus / feasibility
  // pass (:168-223) is then a no-op: a stolen slot leaves its loser's path, so every slot has at most one claimant, and the
  // claimant's schedule is the one the inclusion phase found feasible at the same time step (tests/test_baselines_cpu.py replays the
  // reference's own pass on the fixture cases).
  // Slot table (winner i8 + RPI f64 per "{id}#r{k}" / "{id}#c{k}" slot, <= 4 T slots) in the LSAP tile, which this mode never uses.
  static_assert(offsetof(Scratch<TL>, resid) - offsetof(Scratch<TL>, cost) >= 4 * T * (sizeof(double) + 1),
                "the PI slot table (4 T x (f64 + i8)) must fit the LSAP tile cost / u / v / spc");
  DEV double* pi_rpi() { return reinterpret_cast<double*>(&X.cost[0]); }
  DEV int8_t* pi_win() { return reinterpret_cast<int8_t*>(&X.cost[0] + 4 * T); }
  DEV bool pi_cost(int a, int s, bool vis, double& c) const {
    if (vis && !knows(a, s)) return false;
    if ((S.t_flags[s] & TF_ELIGIBLE) && !((S.t_elig[s] >> S.a_type[a]) & 1u)) return false;
    if (queues_task(a, S.t_id[s])) return false;
    const bool coal = is_escort_task(s);
    const double cap = S.a_caps[S.t_type[s]][a];
    if (!coal && !(cap > 0)) return false;
    const double t0 = fmax(qs().a_nft[a], (double)tnow);
    const double start = t0 + fdiv(norm2(S.a_px[a] - S.t_px[s], S.a_py[a] - S.t_py[s]), speed_of(S.a_type[a]));
    const bool dl = (S.t_flags[s] & TF_DEADLINE) != 0;
    const double deadline = (double)S.t_deadline[s];
    if (dl && start > deadline + 1e-6) return false;
    double cost = 0.0 + start;
    if (dl && start > deadline) cost += 200.0 + (start - deadline);
    cost -= 5.0 * (coal ? fmax(cap, 0.5) : cap);
    c = cost;
    return true;
  }
  // candidate order of the inclusion loop: the tuple (ipi, agent.id, slot_key) — slot keys compare as Python strings: by str(task id)
  // first ('#' sorts below every digit), then by str(k) within a task
  static DEV bool pi_before(double c, int a, int id, int k, double oc, int oa, int oid, int ok) {
    if (c != oc) return c < oc;
    if (a != oa) return a < oa;
    if (id != oid) return dec_less(id, oid);
    return dec_less(k, ok);
  }
  DEV void pi_plan(int interval, bool vis) {
    if (!gate_fires(MUAVTA_GATE_ALLOCATOR, interval)) return;  // == should_replan (:49-57): every tag the env emits is in REPLAN_EVENTS
    if (lane == 0) { S.gate_step = tnow + 1; S.last_plan_step = tnow; S.n_replans++; }  // also on the two empty returns (:76-88)
    const int nt = baseline_open_tasks();
    const int nl = compact_to(X.freeA, P.n_agents, [&](int a) { return S.a_state[a] != -1; }, [&](int a) { return a; });
    lds_sync();
    if (nl == 0 || nt == 0) return;
    // expand_slot_keys (CBBA.py:47-65): task j owns slots [X.path[j], X.path[j + 1]) — ceil(rem) coalition slots, else
    // max(1, ceil(min(rem, 4))) — in _open_tasks order
    int ns = 0;
    for (int base = 0; base < nt; base += WG) {
      const int j = base + lane;
      int c = 0;
      if (j < nt) {
        const int s = X.roundT[j];
        const double rem = X.resid[s];
        c = is_escort_task(s) ? (int)ceil(rem) : (int)ceil(fmin(rem, 4.0));
        c = c > 1 ? c : 1;  // (rem > 0: a coalition task has at least one slot too)
      }
      int inc = c;
      for (int d = 1; d < WG; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
      if (j < nt) X.path[j] = (int16_t)(ns + inc - c);
      ns += __shfl(inc, WG - 1);
    }
    if (ns > 4 * T) { if (lane == 0) fail(MUAVTA_ERR_LSAP); return; }  // more residual demand than the slot table holds
    double* rpi = pi_rpi();
    int8_t* win = pi_win();
    for (int q = lane; q < ns; q += WG) { win[q] = -1; rpi[q] = -__builtin_inf(); }
    for (int i = lane; i < nl; i += WG) X.SR[X.freeA[i]] = 0;  // assigned_agents
    lds_sync();
    // inclusion (:104-166): each round takes the globally least candidate; a steal needs provisional rpi >= incumbent rpi - 1e-9,
    // and on a tie (|diff| <= 1e-9) the lower agent.id; the loser leaves assigned_agents
    const int rounds = ns * nl;
    for (int it = 0; it < rounds; it++) {
      double bc = __builtin_inf();
      int ba = 0x7fff, bid = 0, bk = 0, bq = -1, bj = 0;
      for (int p = lane; p < nl * nt; p += WG) {
        const int i = p / nt, j = p - i * nt;
        const int a = X.freeA[i];
        if (X.SR[a]) continue;
        const int s = X.roundT[j];
        double c;
        if (!pi_cost(a, s, vis, c)) continue;
        const int q0 = X.path[j], q1 = j + 1 < nt ? (int)X.path[j + 1] : ns;
        int kq = -1;
        for (int q = q0; q < q1; q++) {
          const int w = win[q];
          if (w == a) continue;
          if (w >= 0) {
            const double r = rpi[q];
            if (c < r - 1e-9) continue;
            if (fabs(c - r) <= 1e-9 && a >= w) continue;
          }
          if (kq < 0 || dec_less(q - q0, kq - q0)) kq = q;
        }
        if (kq < 0) continue;
        const int id = S.t_id[s];
        if (bq < 0 || pi_before(c, a, id, kq - q0, bc, ba, bid, bk)) { bc = c; ba = a; bid = id; bk = kq - q0; bq = kq; bj = j; }
      }
      for (int off = 1; off < WG; off <<= 1) {
        const double oc = __shfl_xor(bc, off);
        const int oa = __shfl_xor(ba, off), oid = __shfl_xor(bid, off), ok = __shfl_xor(bk, off), oq = __shfl_xor(bq, off), oj = __shfl_xor(bj, off);
        if (oq >= 0 && (bq < 0 || pi_before(oc, oa, oid, ok, bc, ba, bid, bk))) { bc = oc; ba = oa; bid = oid; bk = ok; bq = oq; bj = oj; }
      }
      if (bq < 0) break;  // (uniform after the butterfly)
      lds_sync();
      if (lane == 0) {
        const int prev = win[bq];
        if (prev >= 0 && prev != ba) X.SR[prev] = 0;
        win[bq] = (int8_t)ba; rpi[bq] = bc; X.SR[ba] = 1;
        X.col4row[ba] = (int16_t)bj;  // the agent's one slot, as its task's index in the list
      }
      lds_sync();
    }
    // actions (:225-240) in live order, one task each, then _apply_assign
    for (int base = 0; base < nl; base += WG) {
      const int i = base + lane;
      bool st = false;
      int a = 0, s = 0;
      if (i < nl) {
        a = X.freeA[i];
        if (X.SR[a]) { s = X.roundT[X.col4row[a]]; st = in_last_list(s); }
      }
      const unsigned long long m = __ballot(st);
      if (st) {
        const int n = S.n_act + prefix_count(m);
        S.act_agent[n] = (i8)a; S.act_slot[n] = (i8)s; S.act_index[n] = (i16)S.t_row[s];
      }
      lds_sync();
      if (lane == 0) S.n_act += __popcll(m);
      lds_sync();
    }
  }
