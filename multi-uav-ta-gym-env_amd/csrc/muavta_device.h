// muavta_device.h — device-side simulation of ONE env instance by ONE workgroup (gfx950, wave64).
//
// Execution model: the env's state blob sits in LDS (EnvState).  A step is a sequence of phases separated
// by lds_sync().  Phases whose iterations are independent (pairwise sensing, the agent x task cost tile,
// distances, slot GC, observation rows, MT19937 regeneration) are spread over the 64 lanes.  The
// order-dependent bookkeeping of the reference is parallelised where its order can be kept exactly:
//   * "everything up to the first event, then lane 0 replays that one entity as the reference does, then the
//     wave resumes behind it" — the per-agent state machine and the threat update;
//   * "one entity per lane, order-dependent sums replayed in order" — action application (reward addends via
//     v_readlane, allocatedReqs of a shared task via a same-slot prefix), releaseAllTasks (agent lanes compact
//     their queues, slot lanes replay removeAgentCap in agent order), reveals / window expiry;
//   * the LSAP keeps scipy's scan order as per-column positions and never touches LDS inside the solve.
// What is left on lane 0 is entity creation (arrivals, threat spawns, escorts), engagements, task completion.
// Everything is f64 with -ffp-contract=off; FMAs are explicit where numpy emits them.
//
// Every routine cites the reference lines it restates (mUAV_TA/DroneEnv.py unless another file is
// named).  This file is the product path; it shares no code with oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>

#include "muavta_state.h"

#define DEV __device__ __forceinline__
#define DEVN __device__ __noinline__

// 1: the observation rows' HBM operands are requested before the task-time rebuild (latency overlap, +28 live VGPRs there)
// k_rollout's issue-priority pacing of the envs that share a SIMD: 0 off, 1..3 = that priority for the env furthest behind,
// 4 = ranked (3 for the last, one less per neighbour further behind).  Measured on the headline tile (profiles/r02_pacing.txt):
// off 164 M env-steps/s, 1 -> 177 M, 4 -> 182 M; raising priority only while an env replans: 172 M.
#ifndef MUAVTA_PACE_PRIO
#define MUAVTA_PACE_PRIO 4
#endif
#ifndef MUAVTA_PACE_HOLD  // 0 off; n: a wave more than n steps ahead of a neighbour on its SIMD sleeps until it has caught up (muavta_kernels.hip)
#define MUAVTA_PACE_HOLD 0
#endif
#ifndef MUAVTA_PACE_HOLD_WINDOW
#define MUAVTA_PACE_HOLD_WINDOW 48
#endif
#ifndef MUAVTA_PACE_HOLD_SLEEP
#define MUAVTA_PACE_HOLD_SLEEP 16
#endif
#ifndef MUAVTA_PACE_HOLD_POLLS
#define MUAVTA_PACE_HOLD_POLLS 256
#endif
#ifndef MUAVTA_OBS_SADDR
#define MUAVTA_OBS_SADDR 1
#endif
#ifndef MUAVTA_LDS_ZERO_REG  // 1: the rollout phases address the LDS block through one pinned zero register (muavta_kernels.hip: lds_zero) — measured slower
#define MUAVTA_LDS_ZERO_REG 0
#endif
#ifndef MUAVTA_OBS_PREFETCH
#define MUAVTA_OBS_PREFETCH 0
#endif


#ifdef MUAVTA_DIAGNOSTIC_BUILD
#include "muavta_diag.h"   // ABL(), OBS_SKIP(): wrong-result timing switches of diagnostic builds
#else
#if defined(MUAVTA_ABLATE) || defined(MUAVTA_OBS_SKIP)
#error "MUAVTA_ABLATE / MUAVTA_OBS_SKIP produce wrong results: they need -DMUAVTA_DIAGNOSTIC_BUILD and are never part of the shipped library"
#endif
#define ABL(bit) 0
#define OBS_SKIP(mask) false
#endif

namespace muavta {

constexpr int WG = 64;  // one wave64 per env

// Phase separator for a ONE-wave workgroup: LDS instructions of a wave are executed in issue order, so
// a later ds_read of another lane's ds_write needs no s_barrier and, unlike __syncthreads(), no
// vmcnt(0) drain of the observation / tape stores still in flight.  Global-memory hand-offs between
// lanes (MT19937 regeneration) keep the full __syncthreads().
__device__ __forceinline__ void lds_sync() {
  static_assert(WG == 64, "lds_sync() assumes the workgroup is a single wave64");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Publish point for the HBM-resident part of an env (EnvCold): placed at the entry and exit of every wave-parallel phase
// that reads or writes it, so that a lane's loads are issued only after every other lane's stores have been acknowledged
// by the memory system (one wave, one CU: the L1 is write-through and shared, no cache maintenance is needed).
__device__ __forceinline__ void cold_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

#include "muavta_math.h"

template <class TL>
struct alignas(16) Scratch {
  enum { A = TL::A, T = TL::T,
         COSTN_MIN = 4 * A > 2 * T ? 4 * A : 2 * T,  // act_f: 4 x A doubles; refresh_task_times: 2 x T u64
         COSTN = !TL::NO_COST_TILE ? A * T           // REGC / OTFC: only small staging arrays live here ...
               : (A <= 16 && COSTN_MIN < 144) ? 144 : COSTN_MIN };  // ... and the scratch still has to hold the 3 KB reset RNG window
  double cost[COSTN];  // LSAP cost tile, R x C row-major with R = min(nr, nc) (unless TL::REGC)
  double u[A], v[T], spc[T], resid[T];  // (the register-resident LSAP leaves u/v/spc to their other users)
  double press[TL::OTFC ? T : 1];       // Urgency-Coalition threat pressure per round task where the LDS solver (which owns spc) evaluates costs on the fly
  // index lists of the allocator / LSAP and scratch lists of the serial phases: agent ids, slot ids, row numbers (< 128), -1
  // markers, and Urgency-Pair's (rank | n_know << 8) — 16 bits each
  int16_t path[T], col4row[A], row4col[T], remaining[T], freeA[A], roundT[T];
  uint8_t SR[A], SC[T];
  uint8_t live_rank[A];                  // Urgency-Pair: rank of an agent among the live ones (255 = beyond the token pad)
  int32_t retarget_h;                    // threat whose get_closest_agent() the serial replay of its engagement left to the wave (-1: none)
  int16_t pair_info_big[T > 64 ? T : 1]; // Urgency-Pair per-slot (rank, n_know) when `remaining` is busy (LDS LSAP, T > 64)
};

#include "muavta_rng.h"

#ifdef MUAVTA_PROF
enum { PROF_N = 64 };  // slots 0..47: cycle accumulators, 48..63: event counters (x1000)
__device__ unsigned long long g_prof[PROF_N];
__device__ int g_prof_target = -1;  // >= 0: only this env's stamps are accumulated (tools/phase_profile.py --slowest)
// per-phase cycle accumulators of a diagnostic build: 64 + 1 (last stamp) u64 words in LDS right behind the Scratch tile
#define MUAVTA_PROF_LDS_BYTES 528
#define PROF(i) do { if (threadIdx.x == 0) { unsigned long long t_ = clock64(); prof_lds()[i] += t_ - prof_lds()[PROF_N]; prof_lds()[PROF_N] = t_; } } while (0)
#define PROF_COUNT(i, n) do { if (threadIdx.x == 0) prof_lds()[i] += (n); } while (0)
#else
#define PROF(i) do { } while (0)
#define PROF_COUNT(i, n) do { } while (0)
#endif

// muavta_allocate_scored: the caller's planner inputs in token layout (device pointers, kernel arguments), see include/muavta.h
struct ScoredDev {
  const float* scores;                  // [N, MA, MT] or null
  const double* pri;                    // [N, MT] or null
  const unsigned long long* reserved;   // [N] or null
  float* selected;                      // [N, MA, MT] or null
  int32_t* replanned;                   // [N] or null
  int32_t kind, MT, MA, gate, flags;
};

// muavta_set_pair_policy: the MLP-Pair network (PairCostHybrid.pair_mlp, use_attention=False) and the per-env token / score scratch of
// the MUAVTA_ALLOC_MLP_PAIR mode.  Weights: ONE packed f32 buffer per lane, laid out for the order the forward pass streams them through
// the scalar cache in: layer 1 k-major (W0T[k][n]: its loop runs k outside, 64 outputs inside); layer 2 in groups of four outputs with
// their weights interleaved ([n / 4][k][n % 4]: the four chains that run side by side read one k of each from neighbouring words);
// layer 3 and the biases as they are.  See sim/policy.inc.
struct PairPolicyDev {
  const float* w;    // [POL::W::FLOATS] of the installed kind, null: no policy set
  float* scratch;    // [N][POL::FLOATS] (POL_COALITION: a buffer of its own)
  int32_t raw;       // checkpoint's raw_features: tokens of kind MUAVTA_TOK_PAIR_RAW (agent 11 + task 9) instead of MUAVTA_TOK_PAIR (12 + 13)
  float clamp;       // score_clamp (unused by POL_COALITION: its score is a sigmoid)
  int32_t kind;      // POL_PAIR / POL_CONTEXT_PAIR / POL_COALITION: which network `w` holds (and which kernel instantiations run it).  Appended: nothing in front of it moves
};
enum { POL_PAIR = 0, POL_CONTEXT_PAIR = 1, POL_COALITION = 2 };
// The packed weights of a three-layer MLP of width HID whose first layer takes up to W0_ROWS inputs (k-major), in floats.
template <int HID_, int W0_ROWS_>
struct PackedMlp {
  enum { HID = HID_, W0_ROWS = W0_ROWS_,
         W0 = 0, B0 = W0 + HID * W0_ROWS, W1 = B0 + HID, B1 = W1 + HID * HID, W2 = B1 + HID, B2 = W2 + HID, FLOATS = B2 + 16 };
};
// The front of a policy's per-env scratch block, in floats: the token tensors of the plan being made — MT task rows of DT features, MA
// agent rows of DA — and its scores.  END: the first float behind the pad masks; what follows belongs to the policy's traits.
template <int MT_, int DT, int DA, int MA_ = 16>
struct TokenBlock {
  static_assert(MT_ % 4 == 0 && MA_ % 4 == 0, "the pad masks are bytes packed into whole floats");
  enum { MA = MA_, MT = MT_,
         TF = 0, AF = TF + MT * DT, EV = AF + MA * DA, SCORES = EV + MA * MT, TID = SCORES + MA * MT,
         AID = TID + MT, TMASK = AID + MA, AMASK = TMASK + MT / 4, END = AMASK + MA / 4 };
};
// One traits type per learned network: everything sim/policy.inc, the kernels and the host layer need to know about it.
//   KIND, W             the POL_* kind and the packed-weight layout
//   Blk, FLOATS         the token block and the per-env stride of the scratch buffer (grid: Blk::MA x Blk::MT)
//   tok_kind(raw)       the MUAVTA_TOK_* kind of the tokens it consumes; RAW_TOKENS: that follows from PairPolicyDev::raw
//   da / dt / np(raw)   features per agent row / per task row, and the env-uniform inputs in front of them in layer 1's chain
//   LIST_IN_BLOCK       the list of valid cells sits in the scratch block (LIST) instead of the idle LDS in front of Scratch::resid
//   SIGMOID             score = sigmoid of the logit clipped to +-20 (and pad pairs are masked) instead of tanhf(logit) * clamp
//   GATE, FLAGS, FILL   its plan's MUAVTA_GATE_* and MUAVTA_SC_* flags, and whether that plan reads masked cells (they are written as 0)
//   MAX_WAVES           waves per SIMD its rollout instantiation is built for: the hidden activations live in registers
//   WIDE                the variant over the 48 x 64 token pads (MUAVTA_F_TOKEN_PADS): instantiated for the tiles with more than 16 agent rows only
// MLP-Pair (muavta_set_pair_policy): Linear(25|20, 128) - ReLU - Linear(128, 128) - ReLU - Linear(128, 1) over build_pair_tokens(env, 32, 16).
struct PolPair {
  typedef PackedMlp<128, 25> W;
  typedef TokenBlock<32, 13, 12> Blk;
  enum { KIND = POL_PAIR, FLOATS = (Blk::END + 3) & ~3, RAW_TOKENS = 1, LIST_IN_BLOCK = 0, SIGMOID = 0,
         GATE = MUAVTA_GATE_TRAINER, FLAGS = MUAVTA_SC_EDGE_VALID_ONLY, FILL = 0, MAX_WAVES = 3, WIDE = 0 };
  static constexpr int tok_kind(int raw) { return raw ? MUAVTA_TOK_PAIR_RAW : MUAVTA_TOK_PAIR; }
  static constexpr int da(bool raw) { return raw ? 11 : 12; }
  static constexpr int dt(bool raw) { return raw ? 9 : 13; }
  static constexpr int np(bool) { return 0; }
};
// MLP-ContextPair (muavta_set_context_pair_policy): MLPContextPairNet.pair_mlp, Linear(58|41, 192) - ReLU - Linear(192, 192) - ReLU - Linear(192, 1).
// MLP-Pair's tokens, gate and plan; layer 1's columns permuted to a_pool, t_pool, context, agent, task; and a larger scratch block: the MLP-Pair
// block, then the env-uniform head of layer 1's input row — a_pool [12|11], t_pool [13|9], context [8|1], contiguous (PRE; sim/policy.inc:
// context_prefix) — and the 192 chains' values after those inputs (HEAD: computed once per plan, every pair's chain continues from them).
struct PolContextPair : PolPair {
  typedef PackedMlp<192, 58> W;
  enum { KIND = POL_CONTEXT_PAIR, PRE = PolPair::FLOATS, HEAD = PRE + 36, FLOATS = HEAD + W::HID, MAX_WAVES = 2 };
  static constexpr int np(bool raw) { return da(raw) + dt(raw) + (raw ? 1 : 8); }
};
// MLP-Coalition (muavta_set_pair_policy with raw_features == MUAVTA_TOK_ESCORT): MLPCoalitionNet.pair_mlp, Linear(38, 256) - ReLU - Linear(256, 256) -
// ReLU - Linear(256, 1) over build_escort_tokens(env, 48, 16) (agent 16 + task 22 features, 16 x 48 pairs).  Its scratch block (a buffer of its
// own, allocated when a policy of this kind is first installed) ends with the list of valid cells: 768 x u16 — more than the idle LDS in front
// of Scratch::resid holds on every tile.
struct PolCoalition {
  typedef PackedMlp<256, 38> W;
  typedef TokenBlock<48, 22, 16> Blk;
  enum { KIND = POL_COALITION, LIST = Blk::END, FLOATS = (LIST + Blk::MA * Blk::MT / 2 + 3) & ~3, RAW_TOKENS = 0, LIST_IN_BLOCK = 1, SIGMOID = 1,
         GATE = MUAVTA_GATE_ESCORT, FLAGS = MUAVTA_SC_COMMIT, FILL = 1, MAX_WAVES = 1, WIDE = 0 };
  static constexpr int tok_kind(int) { return MUAVTA_TOK_ESCORT; }
  static constexpr int da(bool) { return 16; }
  static constexpr int dt(bool) { return 22; }
  static constexpr int np(bool) { return 0; }
};
// MLP-Pair / MLP-ContextPair over build_pair_tokens(env, 64, 48[, raw]): PairCostHybrid(max_tasks=64, max_agents=48) and the matching ContextPair
// hybrid of the reference's scaled suites (experiments/wps_eval.py:422-434).  The same networks, packed weights, feature widths, gate and flags —
// an MLP's weights do not depend on the pads — over a 48 x 64 grid.  The scratch block: the token block of that grid, then the list of valid
// cells (3,072 x u16: more than the idle LDS in front of Scratch::resid holds, so it sits in the block as MLP-Coalition's does), then for
// MLP-ContextPair PRE and HEAD as in the narrow block.  A buffer of its own, allocated when wide pads first meet an installed policy.
struct PolPairWide : PolPair {
  typedef TokenBlock<64, 13, 12, 48> Blk;
  enum { LIST = Blk::END, FLOATS = (LIST + Blk::MA * Blk::MT / 2 + 3) & ~3, LIST_IN_BLOCK = 1, WIDE = 1 };
};
struct PolContextPairWide : PolPairWide {
  typedef PackedMlp<192, 58> W;
  enum { KIND = POL_CONTEXT_PAIR, PRE = PolPairWide::FLOATS, HEAD = PRE + 36, FLOATS = HEAD + W::HID, MAX_WAVES = 2 };
  static constexpr int np(bool raw) { return da(raw) + dt(raw) + (raw ? 1 : 8); }
};
static_assert(PolPairWide::Blk::SCORES == 4480 && PolPairWide::LIST == 7692 && PolPairWide::FLOATS == 9228 && PolContextPairWide::HEAD == 9264 &&
              PolContextPairWide::FLOATS == 9456, "wide MLP-Pair / MLP-ContextPair scratch block");
// (the values of the PW_* / PC_* / PWE_* and PS_* / PSC_* / PE_* enums these templates replace: neither layout may move)
static_assert(PolPair::W::FLOATS == 19984 && PolContextPair::W::FLOATS == 48592 && PolCoalition::W::FLOATS == 76048, "packed-weight layout");
static_assert(PolPair::FLOATS == 1692 && PolPair::Blk::SCORES == 1120 && PolContextPair::PRE == 1692 && PolContextPair::HEAD == 1728 &&
              PolContextPair::FLOATS == 1920, "MLP-Pair / MLP-ContextPair scratch block");
static_assert(PolCoalition::Blk::SCORES == 2080 && PolCoalition::LIST == 2928 && PolCoalition::FLOATS == 3312, "MLP-Coalition scratch block");

template <class TL>
struct Sim {
  typedef EnvState<TL> State;
#ifdef MUAVTA_PROF
  DEV unsigned long long* prof_lds() { return reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(&X) + sizeof(Scratch<TL>)); }
  DEV void prof_begin() { if (threadIdx.x < PROF_N) prof_lds()[threadIdx.x] = 0; if (threadIdx.x == 0) prof_lds()[PROF_N] = clock64(); lds_sync(); }
  DEV void prof_flush(int env) { lds_sync(); if (threadIdx.x < PROF_N && (g_prof_target < 0 || g_prof_target == env)) atomicAdd(&g_prof[threadIdx.x], prof_lds()[threadIdx.x]); }
#endif
  enum { A = TL::A, T = TL::T, H = TL::H, R = TL::R, E = TL::E, Q = TL::Q, KW = TL::KW };
  typedef EnvCold<TL> Cold;
  State& S;    // LDS
  Cold& C;     // HBM (L2-resident): requirement vectors, queue-entry times, init/done times, obstacles
  Scratch<TL>& X;
  double* rel_log = nullptr;  // optional per-env release log in HBM (muavta_set_release_log)
  // muavta_step_lists: the (agent, index) items of this env beyond the ones staged in S.act_* (which hold TL::A at a time), still
  // in the caller's rows in HBM: this env's row, its length and the next item to stage.  nullptr everywhere else.
  const int32_t* more_agent = nullptr;
  const int32_t* more_index = nullptr;
  int more_cap = 0, more_pos = 0;
  int tnow;                   // env.time_steps in a (uniform) register: it changes once per step, and every LDS read of it is ~100 cycles of latency
  const DevParams& P;
  uint32_t* tape;  // [4][1248] in HBM
  int lane;
  // LDS window of prefetched raw tape words consulted by next32(): normally the 8-word window in the state
  // blob; reset() points it at a 192-word-per-stream copy in the scratch tile (a reset draws ~100 words)
  const uint32_t* win_ptr;
  uint32_t win_len, win_stride;
  bool in_step = false;  // step() is running in this object (reclaim_slot_serial: which slots may be recycled on demand)

  __device__ Sim(State& s, Cold& c, Scratch<TL>& x, const DevParams& p, uint32_t* t)
      : S(s), C(c), X(x), P(p), tape(t), lane(opaque_lane()), win_ptr(&s.rng_win[0][0]), win_len(8), win_stride(8), tnow(s.time_steps) {}
  // The lane id, opaque to the optimiser.  A Sim built inside the 150-step loop of k_rollout would otherwise have every
  // lane-derived value (ballot prefix masks, lane & 7, lane < n ...) hoisted out of the loop, where they overflow the 128
  // VGPRs and come back as scratch (HBM) reloads at ~150 sites of the step; recomputing them is one or two VALU ops.
  static __device__ __forceinline__ int opaque_lane() {
    int l = threadIdx.x;
    asm volatile("" : "+v"(l));
    return l;
  }
  DEV void sync_clock() { tnow = S.time_steps; }
  // next_free_* / orgReqs / doneReqs / mission areas: LDS or the HBM record, by tile (QueueSide in muavta_state.h)
  DEV QueueSide<A, T, true>& qs() const {
    if constexpr (TL::SLIM) return static_cast<QueueSide<A, T, true>&>(C); else return static_cast<QueueSide<A, T, true>&>(S);
  }  // after the blob was (re)loaded or reset behind this object's back
  // initTime / doneTime of the tasks: LDS or the HBM record, by tile (TaskTimes in muavta_state.h)
  DEV TaskTimes<T, true>& times() const {
    if constexpr (TL::TIMES_LDS) return static_cast<TaskTimes<T, true>&>(S); else return static_cast<TaskTimes<T, true>&>(C);
  }

  DEV void fail(int code) { if (S.error == 0) S.error = code; }
  // S.obs_rows = (rows of the handle's task tensor from which on pad rows are known to be there) | OBS_STATIC, or -1 (unknown).
  // OBS_STATIC: the columns of rows [0, n_open) that only change with a task's requirement / allocation vectors or with the open list
  // itself (id, current_reqs, alloc_reqs, type, unmet) are up to date in the handle's buffer; the observation writer then only
  // rewrites the columns that move every step (position, status, init / end time, age).  Cleared by everything that changes
  // allocatedReqs (the times_dirty sites), currentReqs, orgReqs, or the open list.  Any lane may clear it (same value).
  enum { OBS_STATIC = 1 << 16 };
  DEV void obs_static_clear() { const int v = S.obs_rows; if (v > 0) S.obs_rows = v & (OBS_STATIC - 1); }
  DEV double speed_of(int t) const {  // P.speed[t] without a memory access for a per-lane t
    return t == 0 ? P.speed[0] : t == 1 ? P.speed[1] : t == 2 ? P.speed[2] : t == 3 ? P.speed[3] : t == 4 ? P.speed[4]
         : t == 5 ? P.speed[5] : P.speed[6];
  }


#include "sim/rng.inc"
#include "sim/entities.inc"
#include "sim/reset.inc"
#include "sim/step.inc"
#include "sim/actions.inc"
#include "sim/world.inc"
#include "sim/observe.inc"
#include "sim/allocate.inc"
#include "sim/baselines.inc"
#include "sim/tokens.inc"
#include "sim/policy.inc"
#include "sim/lsap.inc"
#include "sim/metrics.inc"
};


}  // namespace muavta

