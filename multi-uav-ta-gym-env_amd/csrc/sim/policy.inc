// sim/policy.inc — member functions of Sim<TL> (muavta_device.h includes this file INSIDE the struct body): the learned MLP-Pair hybrid.
  // ====================================================================================================
  // PairCostHybrid(use_attention=False) (TaskAllocation/Hybrid/PairCostHybrid.py:154-197,266-278,308-328):
  //   logits = pair_mlp(cat([agent_feats[i], task_feats[j]]))     Linear(25|20, 128) - ReLU - Linear(128, 128) - ReLU - Linear(128, 1)
  //   scores = tanh(logits) * score_clamp * edge_valid            -> HungarianAllocator.allocate_tasks(edge_scores=...) = allocate<true>
  // ARITHMETIC CONTRACT (DESIGN.md §7; tests/policy_mlp_py.py is its host twin).  torch leaves its summation order open, so the device
  // defines its own and keeps to it everywhere:
  //   * every Linear output is ONE k-ascending float32 fmaf chain that starts from the bias:
  //         acc = b[n];  for k = 0 .. K-1:  acc = fmaf(W[n][k], x[k], acc)
  //     layer 1's x is the reference's cat: the agent row's 12 (raw: 11) features, then the task row's 13 (raw: 9) — one chain, not an
  //     agent part plus a task part; ReLU is `acc > 0 ? acc : 0`; layer 3 runs n-ascending over layer 2's outputs;
  //   * score = tanhf(logit) * score_clamp, float32, on the pairs whose edge_valid is 1; masked pairs are not evaluated at all;
  //   * with exploration noise (the RL rings of muavta_rollout_record): score = tanhf(logit + noise) * score_clamp, the sum ONE float32 addition.
  // One PAIR per lane: the lane keeps its pair's 128 hidden activations in registers and walks the chains by itself, the weights are
  // wave-uniform scalar operands streamed through the scalar cache.  So a logit is a pure function of its 25 (20) inputs and the
  // weights — the same instruction sequence whatever the lane, the batch, the position in the valid list or the env — and no value
  // crosses lanes anywhere in the forward pass.  The valid pairs of the 16 x 32 grid (wide pads: 48 x 64) are compacted first (row-major), 64
  // per pass: a pad row or column — the 24 x 48 tile has fewer agents and slots than the wide pads — has no valid pair and costs no pass.
  // ====================================================================================================
  typedef const __attribute__((address_space(4))) float pol_cf;  // constant address space: uniform indices become scalar loads
  typedef float pol_f2 __attribute__((ext_vector_type(2)));
  static DEV float pol_relu(float v) { return v > 0.f ? v : 0.f; }
  static DEV const float* as_global_f(const float* p) { return (const float*)(const __attribute__((address_space(1))) float*)p; }
  // blk: this env's scratch block (POL::FLOATS), its token tensors ([MT, Dt], [16, Da], [16, MT]) complete and visible (cold_sync() by the
  // caller).  scores / logits: this env's [16, MT] outputs (either may be null).  fill: masked entries are written as 0 (MLP-Pair's fused mode
  // leaves them alone: allocate<true> under MUAVTA_SC_EDGE_VALID_ONLY never reads them).  Scratch: X.cost .. X.spc (the list of valid cells).
  // POL: the policy's traits (muavta_device.h) — the packed-weight offsets and the width, the feature widths and the grid, the env-uniform head of
  // layer 1's input row (PolContextPair: `pre`, written by context_prefix() below, with the 192 floats of HEAD behind it), the score function and
  // the place of the list of valid cells (PolCoalition: 1,536 B do not fit in front of Scratch::resid) — everything else is the same code.
  // tpad / apad (POL::SIGMOID): the token builder's task_mask / agent_mask (1 = pad row); a pair of a pad row is masked like one whose edge_valid is 0.
  // noise: this env's [16, MT] exploration draws of a recorded gate, or null: added to the logit of an evaluated cell under the tanhf (the logit
  // that is written stays the network's) and set to 0 in every other cell — the slot then holds noise * edge_valid (PairCostHybrid.py:266-278).
  template <bool RAW, class POL>
  DEV void pair_forward_t(const PairPolicyDev& pol, float* blk, float* scores, float* logits, bool fill, float* noise = nullptr) {
    typedef typename POL::W LY;
    typedef typename POL::Blk B;
    constexpr int Da = POL::da(RAW), Dt = POL::dt(RAW), NP = POL::np(RAW), K0 = NP + Da + Dt, HID = LY::HID;
    constexpr int MT = B::MT, CELLS = B::MA * MT;
    static_assert(K0 <= LY::W0_ROWS && HID % 64 == 0, "layer 1's weights are stored k-major, W0_ROWS rows of HID");
    // the list of valid cells: the cost tile and the LSAP's duals / spc behind it (one run of doubles, all idle between the token builder and the plan)
    static_assert(POL::LIST_IN_BLOCK || (offsetof(Scratch<TL>, resid) - offsetof(Scratch<TL>, cost) >= CELLS * sizeof(uint16_t) && offsetof(Scratch<TL>, u) > offsetof(Scratch<TL>, cost) &&
                  offsetof(Scratch<TL>, resid) > offsetof(Scratch<TL>, spc)), "the list of valid cells needs 1 KB in front of Scratch::resid");
    const float *tf = blk + B::TF, *af = blk + B::AF, *ev = blk + B::EV, *pre = nullptr;
    if constexpr (NP > 0) pre = blk + POL::PRE;
    const uint8_t *tpad = reinterpret_cast<const uint8_t*>(blk + B::TMASK), *apad = reinterpret_cast<const uint8_t*>(blk + B::AMASK);
    const uint64_t wb = (uint64_t)pol.w;
    uint32_t wlo = __builtin_amdgcn_readfirstlane((uint32_t)wb), whi = __builtin_amdgcn_readfirstlane((uint32_t)(wb >> 32));
    const float clamp = pol.clamp;
    uint16_t* list;
    if constexpr (POL::LIST_IN_BLOCK) list = reinterpret_cast<uint16_t*>(blk + POL::LIST); else list = reinterpret_cast<uint16_t*>(X.cost);
    int nv = 0;
    for (int base = 0; base < CELLS; base += WG) {
      const int c = base + lane;
      bool v = ev[c] != 0.f;
      if constexpr (POL::SIGMOID) v = v && tpad[c % MT] == 0 && apad[c / MT] == 0;  // (pad pairs are masked here too, whatever edge_valid holds)
      const unsigned long long m = __ballot(v);
      if (v) list[nv + prefix_count(m)] = (uint16_t)c;
      else if (fill) {
        if (scores) scores[c] = 0.f;
        if (logits) logits[c] = 0.f;
      }
      if (noise && !v) noise[c] = 0.f;
      nv += __popcll(m);
    }
    // NP > 0: the first NP inputs of layer 1 (a_pool, t_pool, context) are the same for every pair of the env, so the chains' values after them
    // are computed ONCE per plan — output n on lane n % 64, the same fmaf steps in the same order, hence the same bits — and parked in the
    // env's scratch block (POL::HEAD); every pair's chain continues from there.  Written and read back with vector accesses: not through
    // the scalar cache, which may still hold the line of the previous plan.
    float* head = nullptr;
    if constexpr (NP > 0) {
      head = blk + POL::HEAD;
      if (nv > 0) {  // (uniform)
        const float* wg = as_global_f(pol.w);
        for (int n = lane; n < HID; n += WG) {
          float acc = wg[LY::B0 + n];
#pragma unroll 1
          for (int k = 0; k < NP; k++) acc = __builtin_fmaf(wg[LY::W0 + k * HID + n], pre[k], acc);
          head[n] = acc;
        }
      }
      cold_sync();  // every lane's outputs are in memory before any lane reads another's
    }
    if constexpr (POL::LIST_IN_BLOCK) cold_sync();  // the list is in global memory: every lane's entries are there before any lane reads another's
    lds_sync();
    for (int b0 = 0; b0 < nv; b0 += WG) {  // (uniform)
      // (the weights' base is made opaque once per pass: otherwise layer 1's 128 biases — pass-invariant scalar loads — are hoisted in
      // front of the loop and held, i.e. spilled, across it)
      asm volatile("" : "+s"(wlo), "+s"(whi));
      pol_cf* w = (pol_cf*)(((uint64_t)whi << 32) | (uint64_t)wlo);
      const bool act = b0 + lane < nv;
      const int c = list[act ? b0 + lane : b0];  // lanes beyond the list redo the pass's first pair; their result is dropped
      const int i = c / MT, j = c - i * MT;
      const float* xa = af + i * Da;
      const float* xt = tf + j * Dt;
      // The arithmetic is written two chains wide (v_pk_fma_f32: two independent IEEE fmas per instruction, each chain's own
      // order untouched): outputs n and n + 1 share an instruction, the input value is broadcast to both halves.
      // Layer 1, 64 outputs at a time: k is the outer loop, so one pass over the pair's inputs feeds 64 chains that each still take
      // their products in ascending k.  (Rolled loops with a bounded body on purpose: fully unrolled, every weight of the layer is a
      // scalar load the scheduler issues up front — thousands of live SGPRs, all spilled.)
      pol_f2 h1[HID / 2];
#pragma unroll
      for (int nc = 0; nc < HID / 2; nc += 32) {
#pragma unroll
        for (int t = 0; t < 32; t++) {
          if constexpr (NP > 0) h1[nc + t] = pol_f2{head[2 * (nc + t)], head[2 * (nc + t) + 1]};
          else h1[nc + t] = pol_f2{w[LY::B0 + 2 * (nc + t)], w[LY::B0 + 2 * (nc + t) + 1]};
        }
#pragma unroll 1
        for (int k = NP; k < K0; k++) {
          const float xk = *(k < NP + Da ? xa + (k - NP) : xt + (k - NP - Da));
          pol_cf* r = w + LY::W0 + k * HID + 2 * nc;
#pragma unroll
          for (int t = 0; t < 32; t++) h1[nc + t] = __builtin_elementwise_fma(pol_f2{r[2 * t], r[2 * t + 1]}, pol_f2{xk, xk}, h1[nc + t]);
        }
#pragma unroll
        for (int t = 0; t < 32; t++) h1[nc + t] = pol_f2{pol_relu(h1[nc + t].x), pol_relu(h1[nc + t].y)};
        if constexpr (HID > 192) {  // (the upper half is made opaque as soon as it is complete, as layer 2 does below: see there)
          if (nc >= 64) {
#pragma unroll
            for (int t = 0; t < 32; t++) asm volatile("" : "+v"(h1[nc + t]));
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // Layers 2 and 3 together: four of layer 2's chains side by side (outputs n .. n + 3, their weights interleaved in memory so
      // that the four of one k are neighbours: LY::W1), eight k at a time, and layer 3's chain takes their outputs in ascending n
      // as they complete.  The weights of the NEXT eight k are requested right after the first products of a chunk have consumed
      // the current ones (scalar loads return out of order, so the wait in front of those products must find nothing else in
      // flight), and arrive while the chunk's other products issue.
      float logit = w[LY::B2];
#pragma unroll 1
      for (int n = 0; n < HID; n += 4) {
        pol_cf* r = w + LY::W1 + n * HID;  // [k][4]
        // (no instruction: the activations become new values in every iteration, so the (h, h) operand pairs below are formed where
        // they are used — as the packed FMA's operand select — instead of once in front of the loop in 128 more register pairs)
        // (256 wide: the kernel is built for one wave per SIMD, so the 256 activations live in the unified 512-entry register file — the
        // allocator places them (about 480 registers in all, nothing spilled) and moves what it keeps in the accumulator half where the
        // products need it.  Pinning the upper half there by hand ("a" constraints) measured 2 - 8 % slower and left scratch reloads in
        // this loop; the upper half in LDS 32 % slower: DESIGN.md §7.1.)
#pragma unroll
        for (int q = 0; q < HID / 2; q++) asm volatile("" : "+v"(h1[q]));
        pol_f2 a01 = pol_f2{w[LY::B1 + n], w[LY::B1 + n + 1]}, a23 = pol_f2{w[LY::B1 + n + 2], w[LY::B1 + n + 3]};
        float cw[32];
#pragma unroll
        for (int q = 0; q < 32; q++) cw[q] = r[q];
#pragma unroll
        for (int kc = 0; kc < HID; kc += 8) {
          pol_f2 hh[4];
#pragma unroll
          for (int p = 0; p < 4; p++) {
            hh[p] = h1[kc / 2 + p];
            if (HID > 192 && kc >= 128) asm volatile("" : "+v"(hh[p]));  // (256 wide: the upper half's copy is made here, in its chunk, not at the top of the loop)
          }
          {
            const float h = hh[0].x;
            a01 = __builtin_elementwise_fma(pol_f2{cw[0], cw[1]}, pol_f2{h, h}, a01);
            a23 = __builtin_elementwise_fma(pol_f2{cw[2], cw[3]}, pol_f2{h, h}, a23);
          }
          __builtin_amdgcn_sched_barrier(0);
          float dw[32];
          if (kc + 8 < HID) {
#pragma unroll
            for (int q = 0; q < 32; q++) dw[q] = r[(kc + 8) * 4 + q];
          }
#pragma unroll
          for (int q = 1; q < 8; q++) {
            const float h = (q & 1) ? hh[q / 2].y : hh[q / 2].x;
            a01 = __builtin_elementwise_fma(pol_f2{cw[4 * q], cw[4 * q + 1]}, pol_f2{h, h}, a01);
            a23 = __builtin_elementwise_fma(pol_f2{cw[4 * q + 2], cw[4 * q + 3]}, pol_f2{h, h}, a23);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (kc + 8 < HID) {
#pragma unroll
            for (int q = 0; q < 32; q++) cw[q] = dw[q];
          }
        }
        logit = __builtin_fmaf(w[LY::W2 + n], pol_relu(a01.x), logit);
        logit = __builtin_fmaf(w[LY::W2 + n + 1], pol_relu(a01.y), logit);
        logit = __builtin_fmaf(w[LY::W2 + n + 2], pol_relu(a23.x), logit);
        logit = __builtin_fmaf(w[LY::W2 + n + 3], pol_relu(a23.y), logit);
      }
      if (act) {
        if (logits) logits[c] = logit;
        if constexpr (POL::SIGMOID) {  // AttentionEscort.act: 1 / (1 + exp(-clip(logit, -20, 20))), float32, IEEE division
          if (scores) scores[c] = 1.0f / (1.0f + expf(-fminf(fmaxf(logit, -20.0f), 20.0f)));
        } else if (scores) scores[c] = tanhf(noise ? logit + noise[c] : logit) * clamp;
      }
    }
    lds_sync();
  }
  // ---- MLP-ContextPair: ContextPairHybrid(use_attention=False) (TaskAllocation/Hybrid/ContextPairHybrid.py:154-210) --------------------
  //   pair = cat([agent_feats[i], task_feats[j], a_pool, t_pool, context]);  logits = pair_mlp(pair)   Linear(58|41, 192) - ReLU - Linear(192, 192) - ReLU - Linear(192, 1)
  // plan(), the tokens, edge_valid, the scored Hungarian and the gate are PairCostHybrid's.  CONTRACT (DESIGN.md §7.1; tests/policy_mlp_py.py):
  //   * pool[d]: s = 0.0f; s = s + x[row][d] in float32 over the rows whose mask is 0, ascending row; pool[d] = s / (float)max(count, 1), IEEE division
  //     (a_pool over the 16 agent rows, t_pool over the 32 task rows; the wide variant: 48 and 64); context = what Sim::context(raw, 32 | 64, .) writes;
  //   * layer 1: one fmaf chain per output from the bias over a_pool, t_pool, context, the agent row, the task row (each ascending) — the
  //     env-uniform inputs first, the state_dict's columns (agent, task, a_pool, t_pool, context) are permuted when the weights are packed;
  //   * ReLU, layers 2 and 3, tanhf, the masked pairs: as above.
  // context_prefix: the 25 + 8 (raw: 20 + 1) env-uniform inputs into the env's scratch block behind the MLP-Pair layout (PolContextPair::PRE).  One
  // column per lane; the forward pass reads them back with vector loads (every lane the same address) and runs the chains' env-uniform
  // head once per plan (pair_forward_t).
  template <bool RAW, class POL>
  DEV void context_prefix_t(float* base) {
    typedef typename POL::Blk B;
    constexpr int Da = POL::da(RAW), Dt = POL::dt(RAW);
    float* pre = base + POL::PRE;
    if (lane < Da + Dt) {
      const bool ag = lane < Da;
      const int d = ag ? lane : lane - Da, rows = ag ? B::MA : B::MT, D = ag ? Da : Dt;
      const float* x = base + (ag ? B::AF : B::TF);
      const uint8_t* pad = reinterpret_cast<const uint8_t*>(base + (ag ? B::AMASK : B::TMASK));
      float s = 0.0f;
      int count = 0;
      for (int r = 0; r < rows; r++)
        if (pad[r] == 0) { s = s + x[r * D + d]; count++; }
      pre[lane] = s / (float)(count > 1 ? count : 1);
    }
    context(RAW ? 1 : 0, B::MT, pre + Da + Dt);
    cold_sync();  // the columns are in memory before the forward pass reads them across lanes
  }
  template <class POL>
  DEV void context_prefix(const PairPolicyDev& pol, float* base) {
    if (pol.raw) context_prefix_t<true, POL>(base);  // (uniform)
    else context_prefix_t<false, POL>(base);
  }
  // ---- MLP-Coalition: AttentionEscort(use_attention=False) (TaskAllocation/Hybrid/AttentionEscort.py:326-367,370-524) ---------------------------
  //   logits = pair_mlp(cat([agent_feats[i], task_feats[j]]))      Linear(38, 256) - ReLU - Linear(256, 256) - ReLU - Linear(256, 1)
  //   scores = sigmoid(clip(logits, -20, 20)) * edge_valid * non-pad -> _plan_from_scores: allocate_tasks(force=True, reserved=committed_names,
  //   edge_scores = every non-pad pair) + apply_agent_commits.  CONTRACT (DESIGN.md §7.1; tests/policy_mlp_py.py): layer 1 is one chain over the
  //   agent row's 16 features, then the task row's 22; layers 2 and 3 as above; score = 1.0f / (1.0f + expf(-fminf(fmaxf(logit, -20.0f), 20.0f)));
  //   pad pairs and pairs whose edge_valid is 0 are not evaluated and score 0; score_clamp is not used.
  // The forward pass of the installed policy over the env's scratch block (a network with env-uniform inputs: after context_prefix())
  template <class POL>
  DEV void policy_forward(const PairPolicyDev& pol, float* base, float* scores, float* logits, bool fill, float* noise = nullptr) {
    if constexpr (!POL::RAW_TOKENS) pair_forward_t<false, POL>(pol, base, scores, logits, fill, noise);
    else if (pol.raw) pair_forward_t<true, POL>(pol, base, scores, logits, fill, noise);  // (uniform)
    else pair_forward_t<false, POL>(pol, base, scores, logits, fill, noise);
  }
  // POL's tokens — build_pair_tokens(env, 32, 16[, raw]) (wide: 64, 48) or build_escort_tokens(env, 48, 16) — of the current state into this env's scratch block
  template <class POL>
  DEV void policy_tokens(const PairPolicyDev& pol, float* base) {
    typedef typename POL::Blk B;
    TokPtrs K;
    K.task_feats = base + B::TF; K.agent_feats = base + B::AF; K.edge_valid = base + B::EV;
    K.task_ids = reinterpret_cast<int32_t*>(base + B::TID); K.agent_ids = reinterpret_cast<int32_t*>(base + B::AID);
    K.task_mask = reinterpret_cast<uint8_t*>(base + B::TMASK); K.agent_mask = reinterpret_cast<uint8_t*>(base + B::AMASK);
    K.n_urgent = nullptr; K.expert_mask = nullptr; K.replanned = nullptr;
    K.kind = POL::tok_kind(pol.raw); K.max_tasks = B::MT; K.max_agents = B::MA;
    cold_sync();  // the token rows read currentReqs / allocatedReqs
    tokens(K, 0);
    cold_sync();  // every lane's rows are in memory before any lane reads another's
  }
  // MUAVTA_ALLOC_MLP_PAIR: what wps_eval's loop does at a step with policy = PairCostHybrid(use_attention=False) (experiments/
  // wps_eval.py:244-254,490-492; train_pair_cost.py:73-93 with its own interval) —
  //     if _should_replan(env, events, interval):  tok = build_tokens(env); scores = score_tokens(tok); result = plan(.., scores=scores)
  // — tokens and scores only where the gate fires (uniform), then the scored Hungarian with the gate, the token pads and the flags the
  // reference's plan uses (POL::GATE, POL::FLAGS).  With a PolCoalition policy: run_escort_episode's MLP-Coalition branch (experiments/escort_eval.py:181-188) —
  //     if _should_replan(env, events, interval):  result, *_ = mlp.plan(env, hung_force, events=events, explore=False, force=True)
  // — whose plan reads every non-pad cell (no MUAVTA_SC_EDGE_VALID_ONLY), so masked cells are written as 0, the reference's score there (POL::FILL).
  // scratch: this env's POL::FLOATS block; sc_list: T bytes of LDS behind the tile (allocate<true>'s task list).
  template <class POL>
  DEV void allocate_learned(int interval, int use_visibility, const PairPolicyDev& pol, float* scratch, uint8_t* sc_list) {
    typedef typename POL::Blk B;
    if (gate_fires(POL::GATE, interval)) {
      policy_tokens<POL>(pol, scratch);
      if constexpr (POL::np(false) > 0) context_prefix<POL>(pol, scratch);
      policy_forward<POL>(pol, scratch, scratch + B::SCORES, nullptr, POL::FILL);
      cold_sync();  // the scores are in memory before the cost evaluation reads them across lanes
    }
    ScoredDev sc;
    sc.scores = scratch + B::SCORES; sc.pri = nullptr; sc.reserved = nullptr; sc.selected = nullptr; sc.replanned = nullptr;
    sc.kind = POL::tok_kind(pol.raw); sc.MT = B::MT; sc.MA = B::MA; sc.gate = POL::GATE; sc.flags = POL::FLAGS;
    allocate<true>(interval, use_visibility, 4, &sc, 0, sc_list);
  }
  // The same plan with the gate's transition recorded (the RL rings of muavta_rollout_record; muavta_kernels.hip: rl_gate_open).  at_gate():
  // called where the gate fired, between the token builder and the forward pass — it counts the gate and hands back this env's [16, MT]
  // blocks of the slot it belongs to, or nothing past the last slot: such a gate is planned from the scratch block, without noise, as above.
  // A recorded gate's scores are written to the slot itself, masked cells as 0, and the plan reads them there.
  struct RlGate { float *scores, *logits, *noise, *selected; };
  template <class POL, class F>
  DEV void allocate_learned_rl(int interval, int use_visibility, const PairPolicyDev& pol, float* scratch, uint8_t* sc_list, F at_gate) {
    typedef typename POL::Blk B;
    RlGate g{nullptr, nullptr, nullptr, nullptr};
    if (gate_fires(POL::GATE, interval)) {
      policy_tokens<POL>(pol, scratch);
      if constexpr (POL::np(false) > 0) context_prefix<POL>(pol, scratch);
      g = at_gate();
      policy_forward<POL>(pol, scratch, g.scores ? g.scores : scratch + B::SCORES, g.logits, g.scores ? true : (bool)POL::FILL, g.noise);  // (ONE call site)
      cold_sync();  // the scores are in memory before the cost evaluation reads them across lanes
    }
    ScoredDev sc;
    sc.scores = g.scores ? g.scores : scratch + B::SCORES; sc.pri = nullptr; sc.reserved = nullptr; sc.selected = g.selected; sc.replanned = nullptr;
    sc.kind = POL::tok_kind(pol.raw); sc.MT = B::MT; sc.MA = B::MA; sc.gate = POL::GATE; sc.flags = POL::FLAGS;
    allocate<true>(interval, use_visibility, 4, &sc, 0, sc_list);
  }

