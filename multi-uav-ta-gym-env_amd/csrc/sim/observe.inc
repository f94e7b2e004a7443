// sim/observe.inc — member functions of Sim<TL> (muavta_device.h includes this file INSIDE the struct body): observation tensors.
  // ====================================================================================================
  // Observation tensors (:365-415,:468-492), written straight to HBM by all lanes.
  // ====================================================================================================
  // Observation tensors are FEATURE-MAJOR in HBM — tasks f32 [21][max_tasks], legal bit rows u64 [A][ceil(max_tasks/64)] —
  // so with one task row per lane every store instruction is a contiguous run across the wave: no LDS
  // staging, no transposition.  The "no legal action" fallback (:401-408) is a ballot.
  // Task.initTime / doneTime of every live, non-retired slot from the agents' queue entries (== the task's
  // allocationDetails): times are non-negative doubles, so u64 min/max on their bit patterns (LDS atomics)
  // order them numerically.  One queue entry per lane.
  // The caller has passed a cold_sync() (the queue-time rows other lanes wrote are visible).  Besides updating the HBM
  // rows it leaves (initTime, doneTime) of every slot in the scratch tile (obs_times()), where the observation rows of
  // this step pick them up without another trip to memory.  Returns whether it ran.
  DEV double* obs_times() { return X.cost; }  // [2][T] after refresh_task_times() returned true
  // x / c, correctly rounded, for a divisor that is a small integer times a power of two (1200, 6, max_time_steps,
  // max_tasks <= 2^15) and inv = RN(1 / c): q = RN(x * inv) is within 2 ulp of x / c; r = x - q * c is exact in the FMA (q * c
  // has <= 53 + 15 bits and cancels against x to a few units); q + r * inv then differs from x / c by < 2^-51 ulp, and x / c is
  // never that close to a rounding boundary without being on it: both are multiples of 2^g (g = exponent of half an ulp
  // of the quotient) divided by c's odd part m, so they are >= 2^g / m apart, and x / c cannot BE a midpoint because x's
  // last bit sits >= 6 binary places above g.  Three full-rate FMAs instead of the ~12-instruction IEEE division
  // sequence with its quarter-rate v_rcp_f64 (the observation writer divides ~10 times per step and the kernel is
  // VALU-issue bound).  x must be finite (div_small_any keeps inf / NaN as the true division would) and not -0.0 (the
  // result would be +0.0: callers with a negated operand negate the quotient instead, which IEEE division commutes with).
  // *(p + byte_off) for a wave-uniform p, pinned to scalar registers so that the access is emitted in the (SGPR base,
  // 32-bit VGPR offset) addressing form and not with a 64-bit VALU add per access.
  template <class V> static DEV V& at_lane(V* p, uint32_t byte_off) {
#if !MUAVTA_OBS_SADDR
    return *(V*)((char*)p + byte_off);
#endif
    typedef __attribute__((address_space(1))) char GC;
    GC* q = (GC*)p;  // stays a global (not flat) access
    asm("" : "+s"(q));
    return *(V*)(__attribute__((address_space(1))) V*)(q + byte_off);  // zext(32-bit byte offset): what the addressing form takes
  }
  static DEV double div_small(double x, double c, double inv) {
    const double q = x * inv;
    return __builtin_fma(__builtin_fma(-q, c, x), inv, q);
  }
  static DEV double div_coord(double x) { return div_small(x, MAX_COORD, 1.0 / MAX_COORD); }  // x / MAX_COORD, x finite
  static DEV double div40(double x) { return div_small(x, 40.0, 1.0 / 40.0); }  // remaining / 40.0 of the urgency terms (x: a small non-negative integer)
  static DEV double div_small_any(double x, double c, double inv) {
    const double q = x * inv;
    const double q1 = __builtin_fma(__builtin_fma(-q, c, x), inv, q);
    return __builtin_isfinite(q) ? q1 : q;
  }
  DEV bool refresh_task_times() {
    if (!S.times_dirty) return false;  // uniform: LDS word
    lds_sync();
    if (lane == 0) S.times_dirty = 0;
    unsigned long long* tmin = reinterpret_cast<unsigned long long*>(X.cost);
    unsigned long long* tmax = tmin + T;
    for (int s = lane; s < T; s += WG) { tmin[s] = ~0ull; tmax[s] = 0ull; }
    lds_sync();
    if constexpr (A > 32) {
      // 64 agents x Q entries: one AGENT per lane, as many passes as the longest queue holds entries (3-5, not Q = 12), and the
      // lane's queue-time row (HBM) is requested in one go in front of them — one memory latency instead of one per pass.
      const int a = lane < P.n_agents ? lane : 0;
      const int ql = lane < P.n_agents ? (int)S.a_qlen[a] : 0;
      double qt[Q];
#pragma unroll
      for (int k = 0; k < Q; k++) qt[k] = k < ql ? C.a_qtime[a][k] : 0.0;
#pragma unroll
      for (int k = 0; k < Q; k++) {
        if (__ballot(k < ql) == 0ull) break;
        if (k < ql) {
          const int id = S.a_qid[a][k], slot = S.a_qslot[a][k];
          if (ref_valid(id, slot) && S.t_status[slot] != 2) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(qt[k]);
            atomicMin(&tmin[slot], bits);
            atomicMax(&tmax[slot], bits);
          }
        }
      }
    } else {
      const int nE = P.n_agents * Q;
      for (int e = lane; e < nE; e += WG) {
        const int a = e / Q, k = e - a * Q;
        if (k < S.a_qlen[a]) {
          const int id = S.a_qid[a][k], slot = S.a_qslot[a][k];
          if (ref_valid(id, slot) && S.t_status[slot] != 2) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(C.a_qtime[a][k]);
            atomicMin(&tmin[slot], bits);
            atomicMax(&tmax[slot], bits);
          }
        }
      }
    }
    lds_sync();
    double* tt = obs_times();
    for (int s = lane; s < T; s += WG) {
      double ti, td;
      if (S.t_id[s] >= 0 && S.t_status[s] != 2) {
        if (tmin[s] == ~0ull) { ti = -1; td = -1; }
        else {
          ti = __longlong_as_double((long long)tmin[s]);
          td = __longlong_as_double((long long)tmax[s]) + (double)task_duration(S.t_type[s]);
        }
        times().t_init[s] = ti; times().t_dtime[s] = td;
      } else { ti = -1; td = -1; }  // retired / free slots: no observation row reads them
      tt[s] = ti; tt[T + s] = td;
    }
    lds_sync();
    return true;
  }

  // handle_buffer: the tensors are the handle's single observation buffer (overwritten in place every step), not a ring slot —
  // its pad rows are only rewritten where live rows have just disappeared (S.obs_rows)
  DEV void write_obs(float* o_tasks, unsigned long long* o_legal, uint8_t* o_pad, float* o_agents, float* o_flags, bool handle_buffer = false) {
    // (diagnostic builds only — muavta_diag.h: parts of the write left out to time them; OBS_SKIP() is `false` in the shipped library)
    if (OBS_SKIP(16)) return;
    if (OBS_SKIP(1)) o_tasks = nullptr;
    if (OBS_SKIP(2)) o_legal = nullptr;
    if (OBS_SKIP(4)) { o_agents = nullptr; o_flags = nullptr; }
    if (OBS_SKIP(8)) o_pad = nullptr;
    cold_sync();  // the rows below read the requirement vectors the serial phases of this step may have changed
    const int MT = P.max_tasks, nA = P.n_agents;
    const int n = __builtin_amdgcn_readfirstlane(S.n_open);
    const int obs_state = handle_buffer ? __builtin_amdgcn_readfirstlane(S.obs_rows) : -1;
    const int pad_known = obs_state < 0 ? -1 : (obs_state & (OBS_STATIC - 1));
    const int pad_until = pad_known < 0 ? MT : pad_known;  // pad rows below this index have to be (re)written
    // (r4) LIGHT pass: the handle's buffer already holds the static columns of every open row (OBS_STATIC: no requirement /
    // allocation vector and no open-list change since the last write) — only the columns that move every step are rewritten:
    // position (Int and escort tasks follow their threat / UAV), status, init / end time (relative to t), age.  6 stores and 2
    // HBM operands per row (none where the task times live in LDS: TL::TIMES_LDS) instead of 21 and 16.
    const bool light = o_tasks != nullptr && obs_state > 0 && (obs_state & OBS_STATIC) != 0;
    // The HBM rows of the first 64 observation rows are requested NOW, so that their latency runs under the rebuild of the
    // task times below (LDS work); (initTime, doneTime) then come from the scratch tile when they were rebuilt.
    double pc[6], pa[6], pti = 0, ptd = 0;
    const bool dirty = __builtin_amdgcn_readfirstlane(S.times_dirty) != 0;  // (uniform: a scalar branch picks LDS or HBM below, not a per-lane pointer select)
    if (MUAVTA_OBS_PREFETCH && !light) {
      const int s0 = lane < n ? (int)S.open_slot[lane] : 0;
#pragma unroll
      for (int c = 0; c < 6; c++) { pc[c] = lane < n ? C.t_cur[c][s0] : 0.0; pa[c] = lane < n ? C.t_alloc[c][s0] : 0.0; }
      if (!dirty && lane < n) { pti = times().t_init[s0]; ptd = times().t_dtime[s0]; }
    }
    refresh_task_times();
    const double mts = (double)(P.max_time_steps > 1 ? P.max_time_steps : 1), inv_mts = P.inv_mts;
    constexpr double INV_COORD = 1.0 / MAX_COORD, INV6 = 1.0 / 6.0;
    unsigned long long leg0 = 0ull, leg1 = 0ull;  // lane a: legal bits of agent a (rows 0..63, 64..127)
    PROF(15);
    // lane a keeps agent a's (state, head id, type); the agent loop broadcasts them with v_readlane
    int my_st = 0, my_hid = 0, my_ty = 0;
    if (lane < nA) { my_st = S.a_state[lane]; my_hid = head_id(lane); my_ty = S.a_type[lane]; }
    const bool capm = P.capability_mask != 0;
    // (the reference's lists are max_tasks long unless MORE tasks are open — then they grow, DroneEnv.py:410-413 — and its "no legal
    // action" fallback looks at all of them: the loop covers every open row, the stores the first max_tasks)
    const int row_lim = n > MT ? n : MT;
    for (int base = 0; base < row_lim; base += WG) {
      const int j = base + lane;
      const uint32_t ju = (uint32_t)j;  // unsigned lane offset + uniform column pointer: stores take the (SGPR base, VGPR offset) form
      const bool in_n = j < n, in_mt = j < MT;
      int ty = 0;
      uint32_t typemask = 0;  // agent types for which this row is a valid action (before the capability mask)
      if (in_n) {
        const int s = S.open_slot[j];
        const int tid = S.t_id[s];
        ty = S.t_type[s];
        typemask = (S.t_flags[s] & TF_ELIGIBLE) ? S.t_elig[s] : 0xffffffffu;
        if (light) {  // (uniform)
          // (OBS_STATIC implies the task times are not dirty.  As HBM operands these two sat on the step's chain: a build without them ran
          // 1.2 % faster, requesting them at the start of step() instead won back 0.3 % — profiles/r04_ab_obs_light_prefetch.txt.  With
          // TL::TIMES_LDS they are LDS reads and this pass has no memory operand: +1.8 % on the headline, profiles/r07_step_chain_ab.json)
          const double ti = times().t_init[s], td = times().t_dtime[s];
          if (P.saturate_mask && C.t_alloc[ty][s] >= qs().t_org[s]) typemask = 0;
          uint32_t off = ju * 4u;
          const uint32_t cstride = (uint32_t)MT * 4u;
          // (more open tasks than max_tasks: the tensor holds the first max_tasks rows; rows beyond it only feed the legal-mask ballots)
          if (in_mt) {
          if (ty == MUAVTA_INT || (S.t_flags[s] & TF_ESCORT)) {  // the tasks that move: an Int task follows its threat, an escort its UAV
            at_lane(o_tasks, off + cstride) = (float)div_small(S.t_px[s], MAX_COORD, INV_COORD);
            at_lane(o_tasks, off + 2u * cstride) = (float)div_small(S.t_py[s], MAX_COORD, INV_COORD);
          }
          at_lane(o_tasks, off + 3u * cstride) = (float)S.t_status[s];
          if (P.include_time_windows) {
            at_lane(o_tasks, off + 16u * cstride) = (float)div_small_any(ti - (double)tnow, mts, inv_mts);
            at_lane(o_tasks, off + 17u * cstride) = (float)div_small_any(td - (double)tnow, mts, inv_mts);
          }
          at_lane(o_tasks, off + 20u * cstride) = (float)fmin(div_small((double)tnow - (double)S.t_created[s], mts, inv_mts), 1.0);
          }
        } else {
        float r[21];
        r[0] = (float)tid;
        r[1] = (float)div_small(S.t_px[s], MAX_COORD, INV_COORD);
        r[2] = (float)div_small(S.t_py[s], MAX_COORD, INV_COORD);
        r[3] = (float)S.t_status[s];
        double cur[6], alc[6], ti, td;
        if (MUAVTA_OBS_PREFETCH && base == 0) {
#pragma unroll
          for (int c = 0; c < 6; c++) { cur[c] = pc[c]; alc[c] = pa[c]; }
          if (dirty) { ti = obs_times()[s]; td = obs_times()[T + s]; } else { ti = pti; td = ptd; }
        } else {
#pragma unroll
          for (int c = 0; c < 6; c++) { cur[c] = C.t_cur[c][s]; alc[c] = C.t_alloc[c][s]; }
          if (dirty) { ti = obs_times()[s]; td = obs_times()[T + s]; } else { ti = times().t_init[s]; td = times().t_dtime[s]; }
        }
#pragma unroll
        for (int c = 0; c < 6; c++) { r[4 + c] = (float)cur[c]; r[10 + c] = (float)alc[c]; }
        r[16] = r[17] = r[18] = 0.f;
        if (P.include_time_windows) {
          r[16] = (float)div_small_any(ti - (double)tnow, mts, inv_mts);
          r[17] = (float)div_small_any(td - (double)tnow, mts, inv_mts);
          r[18] = (float)div_small((double)ty, 6.0, INV6);
        }
        // the row of the task's own type: two more loads with a per-lane row index (a select chain over the six rows loaded above
        // costs ~30 VALU; a dynamically indexed local array would live in scratch memory)
        const double cur_ty = C.t_cur[ty][s], alc_ty = C.t_alloc[ty][s];
        const double org = qs().t_org[s];
        if (P.saturate_mask && alc_ty >= org) typemask = 0;
        const double unmet = fmax(cur_ty - alc_ty, 0.0);
        r[19] = (float)fdiv(unmet, fmax(org, 1e-6));  // (unmet: 0 or a difference of capability sums, org >= 1e-6: inside fdiv's domain)
        r[20] = (float)fmin(div_small((double)tnow - (double)S.t_created[s], mts, inv_mts), 1.0);
        if (o_tasks && in_mt) {
          // feature-major: column c of row j at (c * MT + j) * 4 — one base in scalar registers, the lane's byte offset stepped by
          // the column stride (one VALU add per store; a column pointer per store was five SALU instructions)
          uint32_t off = ju * 4u;
          const uint32_t cstride = (uint32_t)MT * 4u;
#pragma unroll
          for (int c = 0; c < 21; c++) { at_lane(o_tasks, off) = r[c]; off += cstride; }
        }
        }
      } else if (o_tasks && in_mt && (j < pad_until || j == 0)) {
        // pad rows are {"status": -1}; with no open task row 0 is task_idle (all zeros).  Rows the buffer already holds as pad rows
        // are left alone.
        const float st = (j == 0 && n == 0) ? 0.f : -1.f;
        uint32_t off = ju * 4u;
        const uint32_t cstride = (uint32_t)MT * 4u;
#pragma unroll
        for (int c = 0; c < 21; c++) { at_lane(o_tasks, off) = c == 3 ? st : 0.f; off += cstride; }
      }
      if (o_pad && in_mt && !light) o_pad[ju] = j < (n == 0 ? 1 : n);  // (light: the open list, and with it the pad mask, is what the buffer holds)
      PROF(16);
      if (o_legal) {
        // legal_mask without a per-agent loop: one ballot per agent TYPE gives the rows that type may take
        // (_is_task_action_valid :341-363, eligibility + saturation); lane a then picks its type's row mask.
        unsigned long long okm = 0ull;
#pragma unroll
        for (int t = 0; t <= MUAVTA_F2; t++) {
          const unsigned long long m = __builtin_amdgcn_ballot_w64((typemask & (1u << t)) != 0u);  // (typemask is 0 beyond the open rows)
          if (my_ty == t) okm = m;
        }
        if (capm) {  // capability mask: rows whose task type the agent has capability for
          const int tyx = in_n ? ty : -1;
          unsigned long long capok = 0ull;
#pragma unroll
          for (int tt = 0; tt < 6; tt++) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(tyx == tt);
            if (lane < nA && S.a_caps[tt][lane] > 0) capok |= m;
          }
          okm &= capok;
        }
        if (lane < nA) { if (base == 0) leg0 = okm; else leg1 = okm; }
      }
      PROF(18);
    }
    if (o_legal && lane < nA) {
      // the agent's current task is always selectable (:346-348); in state 2 it is the ONLY legal row (:475-479)
      unsigned long long cur0 = 0ull, cur1 = 0ull;
      int curpos = -1;
      if (n == 0) {
        curpos = my_hid == 0 ? 0 : -1;   // single task_idle row
        if (my_st != 2) { leg0 = 1ull; }
      } else if (S.a_qlen[lane] > 0) {
        const int hs = S.a_qslot[lane][0];
        if (ref_valid(my_hid, hs) && S.t_status[hs] != 2) curpos = S.t_row[hs];
      }
      if (curpos >= 0) { if (curpos < 64) cur0 = 1ull << curpos; else cur1 = 1ull << (curpos - 64); }
      if (my_st == 2) { leg0 = cur0; leg1 = cur1; }
      else if (n > 0) { leg0 |= cur0; leg1 |= cur1; }
      // "no legal action" fallback (:401-408): the current task if it is open, else row 0
      if ((leg0 | leg1) == 0ull && n > 0 && my_st != 2) leg0 = 1ull;
      if (n > MT) {  // rows beyond the tensor's width took part in the fallback above and are dropped here
        if (MT < 64) { leg0 &= (1ull << MT) - 1ull; leg1 = 0ull; }
        else if (MT < 128) leg1 &= (1ull << (MT - 64)) - 1ull;
      }
      const int KM = (MT + 63) >> 6;
      o_legal[lane * KM] = leg0;
      if (KM > 1) o_legal[lane * KM + 1] = leg1;
    }
    PROF(19);
    if (o_agents && lane < nA) {
      const int a = lane;
      float* r = o_agents + a * 9;
      r[0] = (float)div_small(S.a_px[a], MAX_COORD, INV_COORD);
      r[1] = (float)div_small(S.a_py[a], MAX_COORD, INV_COORD);
#pragma unroll
      for (int c = 0; c < 6; c++) r[2 + c] = (float)S.a_caps[c][a];
      r[8] = (float)head_id(a);
    }
    if (o_flags && lane == 0) {  // _event_flag_vector (:417-438)
      float f = 0, t = 0, r = 0;
      for (int k = 0; k < S.n_events; k++) {
        if (S.ev_tag[k] == MUAVTA_EV_AGENT_FAIL) f = 1; else if (S.ev_tag[k] == MUAVTA_EV_NEW_THREAT) t = 1;
        else if (S.ev_tag[k] == MUAVTA_EV_RESET_ALLOCATION) r = 1;
      }
      o_flags[0] = f; o_flags[1] = t; o_flags[2] = r;
      o_flags[3] = (float)div_small((double)tnow, mts, inv_mts);
      o_flags[4] = (float)div_small((double)n, (double)(P.max_tasks > 1 ? P.max_tasks : 1), P.inv_max_tasks);
    }
    if (handle_buffer && o_tasks && lane == 0) S.obs_rows = (n > 0 ? n : 1) | OBS_STATIC;  // rows from here on hold pad rows now; the open rows' static columns are current
  }

