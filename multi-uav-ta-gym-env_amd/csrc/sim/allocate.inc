// sim/allocate.inc — member functions of Sim<TL> (muavta_device.h includes this file INSIDE the struct body): HungarianAllocator.allocate_tasks (+ the hybrids' scored variant).
  // ====================================================================================================
  // HungarianAllocator.allocate_tasks (TaskAllocation/OptimizationBased/HungarianAllocator.py:72-208)
  // + _open_tasks / _apply_assign glue (experiments/paper_eval.py:85-101, wps_eval.py:55-61).
  // Result: S.act_agent / S.act_slot / S.act_index, S.n_act.
  // ====================================================================================================
  DEV bool is_escort_task(int s) const { return (S.t_flags[s] & TF_ESCORT) || S.t_required[s] > 0; }
  DEV double residual_demand(int s) const {
    if (is_escort_task(s)) {
      double required = S.t_required[s] ? (double)S.t_required[s] : 1.0;
      return fmax(required - (double)S.t_ndet[s], 0.0);
    }
    int ty = S.t_type[s];
    return fmax(C.t_cur[ty][s] - C.t_alloc[ty][s], 0.0);
  }

  // mode 0 (MUAVTA_ALLOC_HUNGARIAN): Local-/Global-/Coalition-Hungarian as driven by the WPS / escort harness.
  // mode 1 (MUAVTA_ALLOC_URGENCY_PAIR): TaskAllocation/Hybrid/PairCostHybrid.py:31-86,520-550 — engineered
  //   float32 edge scores 0.5*urgency + 0.3*scarcity - 0.4*dist, clipped to +-0.35, for the first PAD_A live agents x
  //   first PAD_T underfilled tasks, subtracted from the Hungarian cost; replan gate = experiments/wps_eval.py:64-74.
  // The token pads of UrgencyPair(max_tasks, max_agents) (MUAVTA_F_TOKEN_PADS): 32 x 16, or the 64 x 48 of the reference's scaled suites
  //   (experiments/wps_eval.py:422-434): the template arguments PAD_T x PAD_A.  Compile-time on purpose: read from the handle's context at
  //   run time they cost the 64-agent tile's Hungarian rollout 0.8 % (two more VGPRs, a reordered cost pass; A/B against the parent's
  //   library, 4 alternating rounds), so the wide pads are kernel instantiations of their own (AllocUrgencyWide, muavta_kernels.hip) on the
  //   tiles with more than 16 agent rows and every other kernel keeps the literals it always had.
  DEV int16_t* pair_info() { return T > 64 ? X.pair_info_big : X.remaining; }
  // scored template path (SC = true, muavta_allocate_scored; a template flag, not an alloc_mode value): the caller's edge scores / task priorities / reserved agents, indexed in the token layout
  //   (sc.kind, sc.MT, sc.MA) — PairCostHybrid.plan, AttentionRAH.plan, AttentionCommit / AttentionEscort._plan_from_scores
  //   (HungarianAllocator.py:79-92,123-124,170-179).  sc_list: T bytes of LDS behind the scratch tile (the task list handed to
  //   allocate_tasks, as positions in last_tasks_info, in the token builder's order).  Compiled into k_allocate_scored only.
  // The replan gate of the callers' loops as a function of the env state (uniform): MUAVTA_GATE_* of include/muavta.h.  `events` are the
  // ones the last step drained (infos['events'], S.dev_*), the clock is the step about to be taken — what the reference's loops look at
  // between two env.step calls.  allocate<true> evaluates it at its entry; the run-to-the-next-gate kernels (k_run) after every step.
  DEV bool gate_fires(int gate, int interval) const {
    interval = interval < 1 ? 1 : interval;
    bool trig = false;
    for (int k = lane; k < S.n_dev; k += WG) trig |= S.dev_tag[k] <= MUAVTA_EV_AGENT_FAIL;  // Reset_Allocation, New_Threat, Agent_Fail
    if (gate == MUAVTA_GATE_TRAINER) return tnow == 0 || tnow % interval == 0 || __ballot(trig) != 0ull;   // train_pair_cost.py:33-43
    if (gate == MUAVTA_GATE_ESCORT) return tnow == 0 || tnow % interval == 0 || S.n_dev > 0;               // escort_eval.py:52-58
    if (gate == MUAVTA_GATE_ALLOCATOR) return (tnow - S.last_plan_step >= interval) || (S.n_dev > 0);      // should_replan (:27-41)
    return true;
  }
  template <bool SC = false, int PAD_T = 32, int PAD_A = 16>
  DEV void allocate(int interval, int use_visibility, int mode = 0, const ScoredDev* scp = nullptr, int env = 0, uint8_t* sc_list = nullptr) {
    PROF(10);
    interval = interval < 1 ? 1 : interval;
    if (lane == 0) S.n_act = 0;
    bool go;
    const bool envvis = !(P.sense_radius == 0 && P.threat_delay == 0);  // agent_visibility_map() is not None
    int n_sc = 0;  // SC: length of sc_list
    if constexpr (SC) {
      const ScoredDev& sc = *scp;
      go = gate_fires(sc.gate, interval);
      if ((go || sc.gate == MUAVTA_GATE_ALLOCATOR) && lane == 0) S.n_calls++;
      if (sc.replanned && lane == 0) sc.replanned[env] = go ? 1 : 0;
    } else
    if (mode == 1) {  // _should_replan(env, events, 15); plan(force=True) bypasses the allocator's own gate
      bool trig = false;
      for (int k = lane; k < S.n_dev; k += WG) trig |= S.dev_tag[k] <= MUAVTA_EV_AGENT_FAIL;  // Reset_Allocation, New_Threat, Agent_Fail
      go = tnow == 0 || tnow % 15 == 0 || __ballot(trig) != 0ull;
      if (go && lane == 0) S.n_calls++;
    } else if (mode == 3) {  // trainers' expert: force=True under _should_replan(env, events, interval) (train_pair_cost.py:33-43)
      bool trig = false;
      for (int k = lane; k < S.n_dev; k += WG) trig |= S.dev_tag[k] <= MUAVTA_EV_AGENT_FAIL;
      go = tnow == 0 || tnow % interval == 0 || __ballot(trig) != 0ull;
      if (go && lane == 0) S.n_calls++;
    } else if (mode == 2) {  // escort_eval._should_replan(env, events, interval): all five env tags are REPLAN_EVENTS
      go = tnow == 0 || tnow % interval == 0 || S.n_dev > 0;
      if (go && lane == 0) S.n_calls++;
    } else {
      if (lane == 0) S.n_calls++;
      // should_replan (:27-41): every tag the env emits is in the trigger set
      go = (tnow - S.last_plan_step >= interval) || (S.n_dev > 0);
    }
    if (go && lane == 0) S.gate_step = tnow + 1;
    const bool vis = use_visibility && envvis;  // agent_visibility_map() is None
    int nr = 0, n_live = 1;
    // The allocator's task list is env.tasks filtered at CALL time (_open_tasks, paper_eval.py:96-101): last_tasks_info as the last
    // observation left it, MINUS what was concluded since (the status tests below) PLUS what an out-of-step call created since — ids
    // are monotone, so those follow it in env.tasks order.  They become rows [n_open, n_plan) of open_slot for this plan only (beyond
    // n_open nobody else looks); a pair with such a task consumes its agent and the task's residual like any other and is then dropped,
    // as _apply_assign drops a task that is not in env.last_tasks_info (wps_eval.py:55-61).
    int n_plan = S.n_open;
    if (go && S.list_stale) {  // (uniform; only ever set by muavta_call)
      const int n0 = S.n_open;
      lds_sync();
      const int n_new = compact_to(S.open_slot + n0, S.n_order,
                                   [&](int k) { const int s = S.t_order[k]; const int r = S.t_row[s]; return S.t_status[s] != 2 && !(r < n0 && (int)S.open_slot[r] == s); },
                                   [&](int k) { return (int)S.t_order[k]; });
      lds_sync();
      for (int k = lane; k < n_new; k += WG) S.t_row[S.open_slot[n0 + k]] = (uint8_t)(n0 + k);
      n_plan = n0 + n_new;
      lds_sync();
    }
    if (go) {
      cold_sync();  // residual demand reads currentReqs / allocatedReqs
      if constexpr (SC) {
        const ScoredDev& sc = *scp;
        if (sc.kind == 2) {  // build_escort_tokens' sorted local open list -> sc_list; columns = its first MT entries
          const int n_live_raw = compact_to(X.freeA, P.n_agents, [&](int a) { return S.a_state[a] != -1; }, [&](int a) { return a; });
          const int n_all = compact_to(X.roundT, S.n_order, [&](int k) { const int s = S.t_order[k]; return S.t_status[s] != 2 && residual_demand(s) > 0; },
                                       [&](int k) { return S.t_order[k]; });
          lds_sync();
          const int n_list = escort_sorted_list(envvis, n_live_raw, n_all);
          const int n_cols = n_list < sc.MT ? n_list : sc.MT;  // columns = the first MT entries = the list handed over
          n_sc = n_cols;
          for (int k = lane; k < n_plan; k += WG) { const int s = S.open_slot[k]; pair_info()[s] = 255; X.resid[s] = 0.0; }  // (after the helper: pair_info may alias X.remaining)
          lds_sync();
          for (int j = lane; j < n_cols; j += WG) {
            const int s = X.path[j];
            pair_info()[s] = (int16_t)j; X.resid[s] = residual_demand(s); sc_list[j] = (uint8_t)S.t_row[s];
          }
          lds_sync();
        }
      }
      // live agents -> free list (get_live_agents order), residual demand per open task: one lane each
      // Urgency-Coalition holds committed agents out of the match (committed_names, AttentionCommit.py:24-30)
      unsigned long long held = 0ull;  // SC: reserved_agent_names (HungarianAllocator.py:91-92)
      if constexpr (SC) held = scp->reserved ? scp->reserved[env] : 0ull;
      nr = compact_to(X.freeA, P.n_agents,
                      [&](int a) { return S.a_state[a] != -1 && !(mode == 2 && S.a_commit[a] > tnow) &&
                                          !(SC && (((held >> a) & 1ull) || ((scp->flags & MUAVTA_SC_COMMIT) && S.a_commit[a] > tnow))); },
                      [&](int a) { return a; });
      n_live = nr > 1 ? nr : 1;
      bool any_open = false;
      int n_under = 0;
      if constexpr (SC) {
        const ScoredDev& sc = *scp;
        if (lane < P.n_agents) {  // token row of an agent: its rank among the live ones (tok["live"][:max_agents])
          const bool lv = S.a_state[lane] != -1;
          const unsigned long long lm = __ballot(lv);
          const int rk = prefix_count(lm);
          X.live_rank[lane] = (lv && rk < sc.MA) ? (uint8_t)rk : (uint8_t)255;
        }
        if (sc.kind != 2) {  // build_att_tokens' open_tasks (AttentionRAH.py:69-73): underfilled at the type index, env.tasks order
          const bool full = (sc.flags & MUAVTA_SC_FULL_TASK_LIST) != 0;
          for (int base = 0; base < n_plan; base += WG) {
            const int k = base + lane;
            bool under = false, inl = false;
            int s = 0, rank = 0;
            if (k < n_plan) {
              s = S.open_slot[k];
              const int ty = S.t_type[s];
              // (status: the open list is the one of the last observation — an out-of-step _retire_escort (muavta_call) concludes a task
              // behind it, and the harness lists are built from env.tasks with `status != 2` at call time)
              under = S.t_status[s] != 2 && C.t_alloc[ty][s] < C.t_cur[ty][s];
            }
            const unsigned long long um = __ballot(under);
            if (k < n_plan) {
              rank = n_under + prefix_count(um);
              inl = under && (full || rank < sc.MT);
              pair_info()[s] = (int16_t)(!under ? 255 : rank < sc.MT ? rank : 254);  // token column; 254: in the list, no column
              const double r = inl ? residual_demand(s) : 0.0;
              X.resid[s] = r;
              any_open |= r > 0;
            }
            const unsigned long long im = __ballot(inl);
            if (inl) sc_list[n_sc + prefix_count(im)] = (uint8_t)k;
            n_sc += __popcll(im);
            n_under += __popcll(um);
          }
        } else {
          any_open = n_sc > 0;  // every entry of the sorted list has residual demand
        }
      } else
      for (int base = 0; base < n_plan; base += WG) {
        const int k = base + lane;
        bool under = false;
        int s = 0;
        if (k < n_plan) {
          s = S.open_slot[k];
          const int ty = S.t_type[s];
          // Urgency-Pair only plans over build_att_tokens' open_tasks: underfilled at the type index (AttentionRAH.py:69-73).
          // _open_tasks (paper_eval.py:96-101) reads env.tasks when it is called: a task an out-of-step _retire_escort (muavta_call)
          // concluded since the last observation is still in `open_slot` and not in that list
          under = S.t_status[s] != 2 && (mode != 1 || C.t_alloc[ty][s] < C.t_cur[ty][s]);
        }
        const unsigned long long um = mode == 1 ? __ballot(under) : 0ull;
        if (k < n_plan) {
          // (Urgency-Pair hands the allocator the max_tasks token rows only: tok["open_tasks"] = kept, PairCostHybrid.py:36,62)
          const double r = (under && !(mode == 1 && n_under + prefix_count(um) >= PAD_T)) ? residual_demand(s) : 0.0;
          X.resid[s] = r;
          any_open |= r > 0;
        }
        if (mode == 1) {
          if (under) {
            const int rank = n_under + prefix_count(um);
            int n_know = 0;
            if (vis) for (int b = 0; b < P.n_agents; b++) n_know += (S.known[b][s >> 5] >> (s & 31)) & 1u;
            pair_info()[s] = (rank < PAD_T ? rank : 255) | (n_know << 8);
          } else if (k < n_plan) pair_info()[s] = 255;
          n_under += __popcll(um);
        }
      }
      if (mode == 1 && lane < P.n_agents) {
        const bool lv = S.a_state[lane] != -1;
        const unsigned long long lm = __ballot(lv);
        const int rk = prefix_count(lm);
        X.live_rank[lane] = (lv && rk < PAD_A) ? (uint8_t)rk : (uint8_t)255;
      }
      if (nr == 0 || __ballot(any_open) == 0ull) go = false;
    }
    lds_sync();
    PROF(11);
    if (!go) { if constexpr (SC) scored_selected(*scp, env, 0); return; }
    PROF_COUNT(52, 1000);
    int n_act = 0;
    while (true) {
      // round_tasks: open tasks (that had residual > 0 initially) with residual > 1e-9, in last_tasks_info order
      int nc;
      if constexpr (SC) nc = compact_to(X.roundT, n_sc, [&](int i) { return X.resid[S.open_slot[sc_list[i]]] > 1e-9; }, [&](int i) { return (int)sc_list[i]; });
      else nc = compact_to(X.roundT, n_plan, [&](int k) { return X.resid[S.open_slot[k]] > 1e-9; }, [&](int k) { return k; });
      lds_sync();
      if (nr == 0 || nc == 0) break;
      const bool tr = nc < nr;              // scipy transposes so that rows <= cols
      const int Rr = tr ? nc : nr, Cc = tr ? nr : nc;
      if (mode == 2) {  // _threat_stats (AttentionEscort.py:46-66): nearest live threat to the task (escort: to its recon)
        for (int j = lane; j < nc; j += WG) {
          const int s = S.open_slot[X.roundT[j]];
          const int pa = S.t_prot_agent[s];
          const double ax = pa >= 0 ? S.a_px[pa] : S.t_px[s], ay = pa >= 0 ? S.a_py[pa] : S.t_py[s];
          double best = MAX_COORD;
          for (int k = 0; k < S.n_active_threats; k++) {
            const int h = S.h_order[k];
            if (S.h_status[h] == 2) continue;
            const double d = norm2(S.h_px[h] - ax, S.h_py[h] - ay);
            if (d < best) best = d;
          }
          (TL::OTFC ? X.press : X.spc)[j] = 1.0 - fmin(div_coord(best), 1.0);  // threat pressure of round task j (a cost-tile LDS solve may clobber spc afterwards; the register solver leaves it)
        }
        lds_sync();
      }
      // ---- cost (:137-179) of agent a for the task in slot s (jr: its index among the round's tasks) ----
      auto pair_cost = [&](int a, int s, int jr) -> double {
        double c = 1e6;
        bool ok = !(vis && !((S.known[a][s >> 5] >> (s & 31)) & 1u));
        if (ok && (S.t_flags[s] & TF_ELIGIBLE) && !((S.t_elig[s] >> S.a_type[a]) & 1u)) ok = false;
        if (ok) {
          double urgency = 0.0;
          if (S.t_flags[s] & TF_DEADLINE) {
            int remaining = S.t_deadline[s] - tnow;
            remaining = remaining > 0 ? remaining : 0;
            urgency = 1.0 - fmin(div40((double)remaining), 1.0);
          }
          double delivered = is_escort_task(s) ? 1.0 : S.a_caps[S.t_type[s]][a];
          if (delivered > 0) {  // _cost (:43-70), left-to-right, priority = 0
            double dist = norm2(S.a_px[a] - S.t_px[s], S.a_py[a] - S.t_py[s]);
            double missing = fmax(X.resid[s], 1e-6);
            double pri = 0.0;
            if constexpr (SC) { const int col = pair_info()[s]; if (scp->pri && col < scp->MT) pri = scp->pri[(size_t)env * scp->MT + col]; }
            double base = div_coord(dist) - 0.5 * fmin(delivered, missing) - 0.4 * pri - 0.6 * urgency;
            double score = 0.0;
            if constexpr (SC) {  // edge_score_dict (PairCostHybrid.py:283-294 / AttentionEscort.py:472-482)
              const int col = pair_info()[s], row = X.live_rank[a];
              bool edge = col < scp->MT && row < scp->MA && scp->scores != nullptr;
              if (edge && (scp->flags & MUAVTA_SC_EDGE_VALID_ONLY)) {
                if (envvis && !((S.known[a][s >> 5] >> (s & 31)) & 1u)) edge = false;
                if (scp->kind != 2 && !(S.a_caps[S.t_type[s]][a] > 0)) edge = false;  // (eligibility already holds here)
              }
              if (edge) score = (double)scp->scores[((size_t)env * scp->MA + row) * scp->MT + col];
            }
            if (mode == 1) {  // urgency_edge_scores (PairCostHybrid.py:68-86) on the edges build_pair_tokens keeps (:42-60)
              const int info = pair_info()[s];
              if ((info & 255) < PAD_T && X.live_rank[a] < PAD_A && S.a_caps[S.t_type[s]][a] > 0) {
                double scar = 0.0;
                if (vis) scar = 1.0 - fmin((double)(info >> 8) / (double)n_live, 1.0);
                double v = 0.5 * urgency + 0.3 * scar - 0.4 * div_coord(dist);
                v = fmin(fmax(v, -0.35), 0.35);
                score = (double)(float)v;  // the scores array is float32
              }
            }
            if (mode == 2) {  // UrgencyCoalition.plan (AttentionEscort.py:729-752), left-to-right in f64
              const int ty = S.t_type[s];
              const bool esc = (S.t_flags[s] & TF_ESCORT) != 0;
              const double cap = S.a_caps[ty][a] > 0 ? S.a_caps[ty][a] : 0.0;
              double v = 0.45 * urgency + 0.35 * (TL::OTFC ? X.press : X.spc)[jr] * (0.5 + 0.5 * (esc ? 1.0 : 0.0)) + 0.3 * fmin(cap, 1.0) - 0.25 * div_coord(dist);
              const bool fighter = is_fighter(S.a_type[a]);
              if (fighter && (esc || ty == MUAVTA_INT)) v += 0.2;
              if (!fighter && ty == MUAVTA_REC) v += 0.2;
              score = fmin(fmax(v, 0.0), 1.0);
            }
            if (base < 1e5 / 2) c = base - score;
          }
        }
        return c;
      };
      static_assert(KW <= 4, "an agent's known mask is cached in four words");
      // pair_cost() split in two for the solvers that keep one column per lane: the column's side (task or agent fields) is
      // read from LDS ONCE per lane, the row's side is the same for every lane (broadcast reads, issued together).  Same arithmetic.
      struct TS { double px, py, urgency, missing, press, pri; int type, info; bool elig_on, esc_task, esc_flag; uint32_t elig; };
      // (the known mask as two 64-bit halves: a four-way select of 32-bit words by a per-lane index is turned into an indexed load
      // from a stack copy of the struct by the optimiser — scratch stores and a dependent scratch load per cost element on the
      // 64-agent tile; a two-way select and a 64-bit shift stay in registers)
      struct AS { double px, py; int type, rank; uint32_t k0, k1; unsigned long long k23; };
      auto load_ts = [&](int sl, int jr) {
        TS t;
        const int fl = S.t_flags[sl];
        t.px = S.t_px[sl]; t.py = S.t_py[sl]; t.type = S.t_type[sl]; t.elig = S.t_elig[sl];
        t.elig_on = (fl & TF_ELIGIBLE) != 0; t.esc_flag = (fl & TF_ESCORT) != 0;
        t.esc_task = t.esc_flag || S.t_required[sl] > 0;
        t.urgency = 0.0;
        if (fl & TF_DEADLINE) {
          int remaining = S.t_deadline[sl] - tnow;
          remaining = remaining > 0 ? remaining : 0;
          t.urgency = 1.0 - fmin(div40((double)remaining), 1.0);
        }
        t.missing = fmax(X.resid[sl], 1e-6);
        t.info = (SC || mode == 1) ? pair_info()[sl] : 0;
        t.press = mode == 2 ? (TL::OTFC ? X.press : X.spc)[jr] : 0.0;
        t.pri = 0.0;
        if constexpr (SC) { if (scp->pri && t.info < scp->MT) t.pri = scp->pri[(size_t)env * scp->MT + t.info]; }
        return t;
      };
      auto load_as = [&](int a) {
        AS g;
        g.px = S.a_px[a]; g.py = S.a_py[a]; g.type = S.a_type[a];
        g.k0 = S.known[a][0]; g.k1 = KW > 1 ? S.known[a][KW > 1 ? 1 : 0] : 0u;
        g.k23 = (KW > 2 ? (unsigned long long)S.known[a][KW > 2 ? 2 : 0] : 0ull) | ((KW > 3 ? (unsigned long long)S.known[a][KW > 3 ? 3 : 0] : 0ull) << 32);
        g.rank = (SC || mode == 1) ? (int)X.live_rank[a] : 0;
        return g;
      };
      // == pair_cost(a, sl, jr); capv = S.a_caps[t.type][a].  STRAIGHT-LINE per lane: every lane evaluates the whole expression and the
      // conditions only select the result.  In SIMT the arithmetic was executed anyway whenever one lane needed it; what the nested
      // `if`s added was an exec-mask region each (s_and_saveexec + branch + s_or: five per cost element), and on the lone wave that
      // ends a launch of configs 4 and 5 every taken branch is an instruction-buffer refill.  Same operations on the same operands
      // for every lane whose result is kept.
      auto pair_eval_cap = [&](const AS& g, int sl, const TS& t, double capv) -> double {
        bool known;
        if constexpr (KW <= 2) known = ((((sl >> 5) ? g.k1 : g.k0) >> (sl & 31)) & 1u) != 0;
        else { const unsigned long long w = (sl & 64) ? g.k23 : ((unsigned long long)g.k0 | ((unsigned long long)g.k1 << 32)); known = ((w >> (sl & 63)) & 1ull) != 0; }
        bool ok = !(vis & !known);
        ok = ok & !(t.elig_on & !((t.elig >> g.type) & 1u));
        const double delivered = t.esc_task ? 1.0 : capv;
        ok = ok & (delivered > 0);
        const double dist = norm2(g.px - t.px, g.py - t.py);
        const double dc = div_coord(dist);
        double base;
        if constexpr (SC) base = dc - 0.5 * fmin(delivered, t.missing) - 0.4 * t.pri - 0.6 * t.urgency;
        else base = dc - 0.5 * fmin(delivered, t.missing) - 0.4 * 0.0 - 0.6 * t.urgency;
        double score = 0.0;
        if constexpr (SC) {  // edge_score_dict: the caller's f32 score of (token row, token column), float()ed
          bool edge = (t.info < scp->MT) & (g.rank < scp->MA) & (scp->scores != nullptr);
          if (scp->flags & MUAVTA_SC_EDGE_VALID_ONLY) edge = edge & (!envvis | known) & !(t.elig_on & !((t.elig >> g.type) & 1u)) & ((scp->kind == 2) | (capv > 0));
          float sv = 0.f;
          if (edge) sv = scp->scores[((size_t)env * scp->MA + g.rank) * scp->MT + t.info];
          score = (double)sv;
        }
        if (mode == 1) {  // (uniform)
          double scar = 0.0;
          if (vis) scar = 1.0 - fmin((double)(t.info >> 8) / (double)n_live, 1.0);
          double v = 0.5 * t.urgency + 0.3 * scar - 0.4 * dc;
          v = fmin(fmax(v, -0.35), 0.35);
          const bool edge = ((t.info & 255) < PAD_T) & (g.rank < PAD_A) & (capv > 0);
          score = edge ? (double)(float)v : 0.0;
        }
        if (mode == 2) {  // (uniform)
          const double cap = capv > 0 ? capv : 0.0;
          double v = 0.45 * t.urgency + 0.35 * t.press * (0.5 + 0.5 * (t.esc_flag ? 1.0 : 0.0)) + 0.3 * fmin(cap, 1.0) - 0.25 * dc;
          const bool fighter = is_fighter(g.type);
          const double v_f = v + 0.2;
          v = (fighter & (t.esc_flag | (t.type == MUAVTA_INT))) ? v_f : v;
          const double v_r = v + 0.2;
          v = (!fighter & (t.type == MUAVTA_REC)) ? v_r : v;
          score = fmin(fmax(v, 0.0), 1.0);
        }
        ok = ok & (base < 1e5 / 2);
        const double c = base - score;
        return ok ? c : 1e6;
      };
      auto pair_eval = [&](int a, const AS& g, int sl, const TS& t) -> double { return pair_eval_cap(g, sl, t, S.a_caps[t.type][a]); };
      bool feasible = false;
      CostCol col;
      // REGC: one LSAP column per lane with its costs in registers, whenever the columns fit the wave (always on the 16- and
      // 24-agent tiles; up to 64 columns on the 64-agent tile, whose kernels are built for 256 VGPRs: four 16-row tuples)
      const bool reg_cols = TL::REGC && (T <= WG || Cc <= WG);
      if (reg_cols) {
        // lane = LSAP column (a task, or an agent when scipy transposes): its whole cost column goes straight into
        // uniformly indexed registers, one row per iteration — no A x T tile in LDS.  pair_cost() split in two: the column's
        // side (task or agent fields) is read from LDS ONCE per lane, the row's side is the same for every lane (broadcast
        // reads, issued together), so an iteration costs one LDS round trip instead of a chain of six.  Same arithmetic.
        const bool incol = lane < Cc;
        {
          // What a row costs the wave that ends a launch is its dependent chain, not its instruction count (§6 of DESIGN.md).  Lane r
          // fetches ROW r's operands up front (every row at once, one LDS round trip), and the row loop broadcasts them with
          // v_readlane: no LDS access on the loop's chain.  Same arithmetic as pair_cost().  (r3: first on the 64-agent tile only;
          // the other two tiles read the row's fields inside the loop — two dependent LDS round trips per row — until the end of r3.)
          auto pack = [](const TS& t) { return t.type | (t.elig_on ? 8 : 0) | (t.esc_task ? 16 : 0) | (t.esc_flag ? 32 : 0) | (int)(t.elig << 8); };
          if (!tr) {  // rows = free agents, lane = task column
            const int my_s = incol ? (int)S.open_slot[X.roundT[lane]] : (int)S.open_slot[X.roundT[0]];
            const TS ts = load_ts(my_s, incol ? lane : 0);
            const int ra = X.freeA[lane < Rr ? lane : 0];
            const AS gr = load_as(ra);
            const int rpk = gr.type | (gr.rank << 8);
            build_cols(col, Rr, [&](int i) -> double {
              AS g;
              const int a = __builtin_amdgcn_readlane(ra, i), pk = __builtin_amdgcn_readlane(rpk, i);
              g.px = readlane_f64(gr.px, i); g.py = readlane_f64(gr.py, i); g.type = pk & 255; g.rank = pk >> 8;
              g.k0 = __builtin_amdgcn_readlane(gr.k0, i); g.k1 = __builtin_amdgcn_readlane(gr.k1, i);
              g.k23 = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)gr.k23, i) | ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(gr.k23 >> 32), i) << 32);
              double c = 0.0;
              c = pair_eval_cap(g, my_s, ts, S.a_caps[ts.type][a]); feasible |= incol & (c < 1e5 / 2);  // (lanes beyond the columns evaluate column 0's operands; nobody reads their result)
              return c;
            });
          } else {  // rows = round tasks, lane = free-agent column
            const int my_a = incol ? X.freeA[lane] : X.freeA[0];
            const AS g = load_as(my_a);
            typedef double caps_vec __attribute__((ext_vector_type(8)));
            caps_vec mycaps;
#pragma unroll
            for (int c6 = 0; c6 < 6; c6++) mycaps[c6] = S.a_caps[c6][my_a];
            const int rj = lane < Rr ? lane : 0;
            const int rsl = S.open_slot[X.roundT[rj]];
            const TS tr_ = load_ts(rsl, rj);
            const int rpk = pack(tr_);
            build_cols(col, Rr, [&](int i) -> double {
              TS t;
              const int sl = __builtin_amdgcn_readlane(rsl, i), pk = __builtin_amdgcn_readlane(rpk, i);
              t.px = readlane_f64(tr_.px, i); t.py = readlane_f64(tr_.py, i); t.urgency = readlane_f64(tr_.urgency, i);
              t.missing = readlane_f64(tr_.missing, i); t.press = mode == 2 ? readlane_f64(tr_.press, i) : 0.0;
              t.info = (SC || mode == 1) ? __builtin_amdgcn_readlane(tr_.info, i) : 0;
              t.pri = SC ? readlane_f64(tr_.pri, i) : 0.0;
              t.type = pk & 7; t.elig_on = (pk & 8) != 0; t.esc_task = (pk & 16) != 0; t.esc_flag = (pk & 32) != 0; t.elig = (uint32_t)pk >> 8;
              double c = 0.0;
              c = pair_eval_cap(g, sl, t, mycaps[t.type]); feasible |= incol & (c < 1e5 / 2);
              return c;
            });
          }
        }
      } else {
        for (int p = lane; p < nr * nc; p += WG) {  // one (agent, task) pair per lane
          const int i = p / nc, j = p - i * nc;
          const double c = pair_cost(X.freeA[i], S.open_slot[X.roundT[j]], j);
          if constexpr (!TL::OTFC) X.cost[tr ? (j * Cc + i) : (i * Cc + j)] = c;  // OTFC: this pass only answers "any feasible pair?"
          feasible |= c < 1e5 / 2;
        }
      }
      // no pair under the acceptance threshold -> the round accepts nothing whatever the assignment is
      PROF_COUNT(62, 1000 * Rr);
      if (__ballot(feasible) == 0ull) { PROF_COUNT(63, 1000 * Rr); break; }
      lds_sync();
      PROF(12);
      if (reg_cols) lsap_reg_solve(Rr, Cc, [&](int i) -> double { return col.get(i); });
      else if constexpr (TL::OTFC)  // beyond 64 columns: element (row i, column j) of scipy's (possibly transposed) matrix, evaluated when scanned
        lsap(Rr, Cc, [&](int i, int j) { return tr ? pair_cost(X.freeA[j], S.open_slot[X.roundT[i]], i) : pair_cost(X.freeA[i], S.open_slot[X.roundT[j]], j); });
      else if constexpr (T <= WG && A <= 32) lsap_reg(Rr, Cc);
      else lsap(Rr, Cc);
      PROF(13);
      // accept (:182-204): one free agent per lane, actions appended in ascending agent order (scipy returns
      // rows sorted); each task appears at most once per round, so the residual updates are independent
      int n_acc = 0, n_left = 0, n_staged = 0;
      for (int base = 0; base < nr; base += WG) {
        const int i = base + lane;
        bool acc = false, keep = false;
        int a = -1, oi = 0, s = 0;
        if (i < nr) {
          a = X.freeA[i];
          const int j = tr ? X.row4col[i] : X.col4row[i];
          keep = true;
          if (j >= 0) {
            double cij;
            if constexpr (TL::NO_COST_TILE) {  // same value the solver saw, through the same straight-line evaluator
              const int sl = S.open_slot[X.roundT[j]];
              cij = pair_eval_cap(load_as(a), sl, load_ts(sl, j), S.a_caps[S.t_type[sl]][a]);
            }
            else cij = X.cost[tr ? (j * Cc + i) : (i * Cc + j)];
            if (cij < 1e5 / 2) {
              acc = true; keep = false;
              oi = X.roundT[j]; s = S.open_slot[oi];
            }
          }
        }
        // (a task beyond last_tasks_info — created by an out-of-step call since the last observation — takes its agent out of the round and
        // has its residual reduced like any other, but the pair is not an action: _apply_assign only keeps tasks of env.last_tasks_info)
        const bool stage = acc && oi < S.n_open;
        const unsigned long long am = __ballot(acc), km = __ballot(keep), sm = __ballot(stage);
        const unsigned long long below = (1ull << lane) - 1ull;
        lds_sync();  // freeA fully read before it is compacted in place
        if (acc) {
          if (stage) {
            const int n = n_act + n_staged + prefix_count(sm);
            S.act_agent[n] = a; S.act_slot[n] = s; S.act_index[n] = oi;
          }
          const double delivered = is_escort_task(s) ? 1.0 : S.a_caps[S.t_type[s]][a];
          X.resid[s] = fmax(X.resid[s] - delivered, 0.0);
        }
        if (keep) X.freeA[n_left + prefix_count(km)] = a;
        n_acc += __popcll(am);
        n_staged += __popcll(sm);
        n_left += __popcll(km);
      }
      n_act += n_staged;
      nr = n_acc ? n_left : 0;  // no accept -> stop
      lds_sync();
      PROF(14);
    }
    if ((mode == 2 || (SC && (scp->flags & MUAVTA_SC_COMMIT))) && P.commit_horizon > 0 && lane < n_act) {  // apply_agent_commits (AttentionCommit.py:33-44)
      const int a = S.act_agent[lane];
      if (S.a_qlen[a] > 0) S.a_commit[a] = tnow + P.commit_horizon;  // only agents that hold a real task now
    }
    if (lane == 0) {
      S.n_act = n_act;
      S.last_plan_step = tnow;
      S.n_replans++;
    }
    lds_sync();
    if constexpr (SC) scored_selected(*scp, env, n_act);
  }
  // _selected_mask(tok, result) (PairCostHybrid.py:296-310): 1 where the plan pairs token row i with token column j
  DEV void scored_selected(const ScoredDev& sc, int env, int n_act) {
    if (!sc.selected) return;
    float* o = sc.selected + (size_t)env * sc.MA * sc.MT;
    const int cells = sc.MA * sc.MT;
    // every staged action names at most ONE cell of the mask (token row of its agent x token column of its task): lane k holds action k's
    // cell, and each lane collects the cells of its own stride from the n_act (<= A <= 64) broadcasts — no LDS traffic in the fill.
    // (r4: every cell walked every action through three LDS reads: 9 % of a policy-in-the-loop launch, profiles/r05_run_ahead_probe.txt)
    int cell = -1;
    if (lane < n_act) {
      const int i = X.live_rank[S.act_agent[lane]], j = pair_info()[S.act_slot[lane]];
      if (i < sc.MA && j >= 0 && j < sc.MT) cell = i * sc.MT + j;
    }
    if (cells <= 32 * WG) {
      uint32_t mine = 0u;  // bit r: cell lane + 64 * r is selected
      for (int k = 0; k < n_act; k++) {
        const int ck = __builtin_amdgcn_readlane(cell, k);
        if (ck >= 0 && (ck & (WG - 1)) == lane) mine |= 1u << (ck >> 6);
      }
      for (int r = 0, idx = lane; idx < cells; r++, idx += WG) o[idx] = ((mine >> r) & 1u) ? 1.f : 0.f;
    } else {
      for (int idx = lane; idx < cells; idx += WG) {
        bool hit = false;
        for (int k = 0; k < n_act; k++) hit |= __builtin_amdgcn_readlane(cell, k) == idx;
        o[idx] = hit ? 1.f : 0.f;
      }
    }
  }

