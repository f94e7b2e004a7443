// muavta_kernels.hip — gfx950 kernels + the C ABI of include/muavta.h.
//
// One workgroup (one wave64) simulates one env instance with its state blob resident in LDS
// (see muavta_device.h).  Kernels:
//   k_reset     seeds -> initial state                              (MultiUAVEnv.reset)
//   k_step      load blob -> apply actions + step -> store blob     (MultiUAVEnv.step)
//   k_allocate  load blob -> Local-Hungarian -> staged actions      (HungarianAllocator.allocate_tasks)
//   k_rollout   [reset] + n x (allocate -> step) in ONE launch, blob never leaves LDS in between
//   k_metrics   calculate_metrics for every env
//   k_lsap / k_avoid   stand-alone solver / obstacle-avoidance entry points
//   k_lsap_tile        the stand-alone solver built from an env tile's own Sim<TL> (muavta_lsap_impl: MUAVTA_LSAP_TILE16 / 24 / 64)
// There is no CPU fallback: without a HIP device every entry point fails with MUAVTA_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is dlopen()ed by muavta_comm_*

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "muavta_device.h"

using namespace muavta;

namespace {

#define AS1 __attribute__((address_space(1)))
#define AS3 __attribute__((address_space(3)))
#define AS4 __attribute__((address_space(4)))
// A pointer loaded from memory (or received by an out-of-line function) is a generic pointer to the compiler, and accesses
// through it become FLAT instructions, which tie up the LDS counter as well as the memory counter.  A round trip through
// the global address space tells the address-space inference what it is.
template <class T> __device__ __forceinline__ T* as_global(T* p) { return (T*)(AS1 T*)p; }

struct ObsPtrs {
  float* tasks;    // [N, 21, max_tasks]  (feature-major)
  unsigned long long* legal;  // [N, A, ceil(max_tasks/64)] bit rows
  uint8_t* pad;    // [N, max_tasks]
  float* agents;   // [N, A, 9]
  float* flags;    // [N, 5]
  double* reward;  // [N]
  uint8_t* done;   // [N]
};

// Launch-invariant context in device memory (one copy per handle).  Kernels get a pointer to it and read it through the
// scalar cache as constant memory (it is written once, by muavta_create); the out-of-line step body of k_rollout gets the
// same pointer instead of ~700 B of by-value arguments.
struct DevCtx {
  DevParams P;
  ObsPtrs O;
  uint32_t* tapes;  // [N][4][1248] MT19937 tapes
  void* blobs;      // EnvState<TL>[N]: the LDS image of every env between launches
  void* cold;       // EnvCold<TL>[N]: the HBM-only part of every env
  uint32_t* pace;   // [PACE_KEYS][16] step counters of the waves resident on each SIMD (k_rollout's issue-priority pacing)
  PairPolicyDev pol;  // muavta_set_pair_policy (rewritten on the handle's stream; all zero: no policy).  Last: nothing in front of it moves
};
enum { PACE_KEYS = 1 << 16 };  // (XCC_ID[3:0], HW_ID[15:4] = se, sh, cu, pipe, simd)
// the context as uniform constant memory: scalar loads, hoistable across the phase barriers
__device__ __forceinline__ const DevCtx& ctx_ref(const DevCtx* p) {
  const uint64_t b = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return *(const DevCtx*)(const AS4 DevCtx*)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ ObsPtrs obs_ptrs(const DevCtx& c) {
  ObsPtrs o;
  o.tasks = as_global(c.O.tasks); o.legal = as_global(c.O.legal); o.pad = as_global(c.O.pad); o.agents = as_global(c.O.agents);
  o.flags = as_global(c.O.flags); o.reward = as_global(c.O.reward); o.done = as_global(c.O.done);
  return o;
}
template <class TL> __device__ __forceinline__ EnvState<TL>* blob_of(const DevCtx& c, int env) { return as_global(reinterpret_cast<EnvState<TL>*>(c.blobs)) + env; }
template <class TL> __device__ __forceinline__ EnvCold<TL>* cold_of(const DevCtx& c, int env) { return as_global(reinterpret_cast<EnvCold<TL>*>(c.cold)) + env; }
__device__ __forceinline__ uint32_t* tape_of(const DevCtx& c, int env) { return as_global(c.tapes) + (size_t)env * MUAVTA_RNG_STREAMS * MUAVTA_RNG_WORDS; }

template <class TL>
__device__ __forceinline__ void obs_for_env(Sim<TL>& sim, const DevParams& P, const ObsPtrs& O, int env, bool handle_buffer = true) {
  const size_t mt = (size_t)P.max_tasks, nA = (size_t)P.n_agents;
  sim.write_obs(O.tasks + (size_t)env * mt * 21, O.legal + (size_t)env * nA * ((mt + 63) >> 6), O.pad + (size_t)env * mt,
                O.agents + (size_t)env * nA * 9, O.flags + (size_t)env * 5, handle_buffer);
  if (threadIdx.x == 0) {
    O.reward[env] = sim.S.last_reward;
    O.done[env] = (uint8_t)((sim.S.terminated ? 1 : 0) | (sim.S.truncated ? 2 : 0));
  }
}

// 16-byte-per-lane coalesced copy between the HBM blob and LDS.
__device__ __forceinline__ void copy16(void* dst, const void* src, int bytes) {
  uint4* d = reinterpret_cast<uint4*>(dst);
  const uint4* s = reinterpret_cast<const uint4*>(src);
  for (int i = threadIdx.x; i < bytes / 16; i += WG) d[i] = s[i];
}

extern __shared__ __align__(16) unsigned char muavta_smem[];
template <class TL>
struct Lds {
  EnvState<TL>* S;
  Scratch<TL>* X;
  __device__ Lds(unsigned char* base) {
    S = reinterpret_cast<EnvState<TL>*>(base);
    X = reinterpret_cast<Scratch<TL>*>(base + ((sizeof(EnvState<TL>) + 15) & ~size_t(15)));
  }
  static constexpr size_t bytes() { return ((sizeof(EnvState<TL>) + 15) & ~size_t(15)) + sizeof(Scratch<TL>); }
};

#define smem muavta_smem
#ifdef MUAVTA_PROF
#define PROF_AT(sim, i) do { if (threadIdx.x == 0) { unsigned long long t_ = clock64(); (sim).prof_lds()[i] += t_ - (sim).prof_lds()[PROF_N]; (sim).prof_lds()[PROF_N] = t_; } } while (0)
#define PROF_EXTRA_LDS MUAVTA_PROF_LDS_BYTES
#else
#define PROF_AT(sim, i) do { } while (0)
#define PROF_EXTRA_LDS 0
#endif
// The fused kernels own a STATIC LDS block of their tile's size: its address is a compile-time constant (0), so LDS addresses
// fold into the ds_* offset fields.  With the dynamic `extern __shared__` array every address was formed as `0 + x` at run
// time (v_add_u32 v, 0, v / s_add_i32 s, 0, imm: 2 % of the kernel's VALU instructions).  They are launched with no dynamic LDS.
// Experiment (MUAVTA_LDS_ZERO_REG=1, off): a DS instruction takes its address from a VGPR, so every access at a constant address
// is preceded by its own rematerialised `v_mov_b32 v, 0` (887 in the 16-agent rollout kernel, 6 % of its static VALU
// instructions).  Addressing the block through ONE pinned zero register the compiler cannot see through removes 400 of them,
// but loads at uniform addresses then stop being uniform values: 560 scalar branches become exec-mask regions and 490 address
// adds move from the SALU to the VALU.  Measured r3: 219 M env-steps/s against 231 M (config 2), 55.0 against 57.1 M (config 4).
#if MUAVTA_LDS_ZERO_REG
static __device__ __forceinline__ uint32_t lds_zero() { uint32_t z; asm volatile("v_mov_b32 %0, 0" : "=v"(z)); return z; }
#else
static __device__ __forceinline__ uint32_t lds_zero() { return 0u; }
#endif
#define KERNEL_LDS(TL) __shared__ __align__(16) unsigned char lds_own[Lds<TL>::bytes() + PROF_EXTRA_LDS]
// Residency on a CU is bound by LDS bytes per env (160 KiB per CU, 1 KiB granule): 16 envs of the 16-agent tile
// (BASELINE configs 2 and 3: 4096 envs = 16 per CU, one round) need <= 10 KiB each.
static_assert(Lds<Tile16>::bytes() <= 10240, "Tile16 no longer fits 16 workgroups per CU");
static_assert(!MUAVTA_TILE24_SLIM || Lds<Tile24>::bytes() <= 10240, "Tile24 no longer fits 16 workgroups per CU");
static_assert(sizeof(EnvState<Tile16>) % 16 == 0 && sizeof(EnvState<Tile24>) % 16 == 0 && sizeof(EnvState<Tile64>) % 16 == 0, "blob copies move 16 B per lane");
static_assert(sizeof(EnvCold<Tile16>) % 16 == 0 && sizeof(EnvCold<Tile24>) % 16 == 0 && sizeof(EnvCold<Tile64>) % 16 == 0, "cold records are 16 B aligned");

// Minimum waves per SIMD the register allocator must leave room for in the fused rollout / step kernels: Tile::MIN_WAVES (4 =>
// at most 128 VGPRs, which is what 16 single-wave workgroups per CU need; 2 => 256 VGPRs on the 64-agent tile).
#ifdef MUAVTA_MIN_WAVES  // (experiments: one value for every tile)
#define TILE_MIN_WAVES(TL) MUAVTA_MIN_WAVES
#else
#define TILE_MIN_WAVES(TL) TL::MIN_WAVES
#endif

// ---- RNG seeding, one LANE per stream --------------------------------------------------------------------------
// CPython's init_by_array is a serial recurrence of 2 x 624 dependent steps; inside k_reset / k_rollout one lane of
// the env's wave would walk it while 63 idle (it was 65 % of a reset).  Here 16 envs x 4 streams share a wave: k_seed
// seeds every env's agent stream (Random(seed), DroneEnv.py:531-533) and draws the three stream seeds from it
// (randint(0, 2^63-1) x 3, :535-538), then the obs / tgt / mission lanes seed theirs.  The reset kernels only load
// the four 624-word states.  Layout: seedbuf [N][4][624] u32 (per-env block contiguous for the coalesced load there).
// init_genrand(19650218), the key-independent half of init_by_array: a compile-time table read through the scalar cache
struct GenrandTable {
  uint32_t v[624];
  constexpr GenrandTable() : v{} {
    uint32_t g = 19650218u;
    v[0] = g;
    for (int i = 1; i < 624; i++) { g = 1812433253u * (g ^ (g >> 30)) + (uint32_t)i; v[i] = g; }
  }
};
__constant__ GenrandTable G_TAB = GenrandTable();
// init_by_array(key[0..len)) into this lane's 624 words of seedbuf (same recurrence as mt_seed).  len is 1 or 2 (seeds below /
// from 2^32): key[j] + j alternates k0, k1 + 1 for len 2 and is k0 for len 1.  The kernel needs no LDS (r2 kept a [624][65]-word
// tile: 162 KB, a whole CU's LDS, which is why k_seed could only start once the previous rollout had drained a CU): the first
// loop's 624 words go through a scratch buffer in GLOBAL memory, 16 words (four 16-byte vectors) at a time in a lane-
// interleaved layout [vector][lane] — every store / load instruction of the wave moves 1 KB of consecutive bytes — and the
// second loop reads them back two chunks ahead of its dependent chain and writes the final state straight into the stream's
// own 624 words (per-lane 64-byte runs: stores, nobody waits for them).  mt[0] is only ever read as the running `prev` (kept
// in a register) and ends as 0x80000000; mt[1] is rewritten by the two wrap-around steps.
typedef uint32_t seed_u4 __attribute__((ext_vector_type(4)));
DEV void seed_stream(uint32_t* mt, seed_u4* tmp /* this wave's [156][64] vectors, already offset by the lane */, uint32_t k0, uint32_t k1, int len) {
  seed_u4* mt4 = reinterpret_cast<seed_u4*>(mt);
  uint32_t prev = 19650218u, m1 = 0;
  const uint32_t add_even = k0, add_odd = len == 2 ? k1 + 1u : k0;  // first loop step i uses j = (i - 1) % len
  for (int base = 0; base < 624; base += 16) {  // first loop, i = 1 .. 623
    uint32_t m[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int i = base + q;
      if (i != 0) prev = (G_TAB.v[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + (((q - 1) & 1) ? add_odd : add_even);  // (i - 1) & 1 == (q - 1) & 1
      m[q] = i != 0 ? prev : 0x80000000u;
      if (i == 1) m1 = prev;
    }
#pragma unroll
    for (int v = 0; v < 4; v++) tmp[(base / 4 + v) * WG] = seed_u4{m[4 * v], m[4 * v + 1], m[4 * v + 2], m[4 * v + 3]};
  }
  // 624th step of the first loop: i wrapped to 1 (mt[0] = mt[623]), j = 623 % len
  prev = (m1 ^ ((prev ^ (prev >> 30)) * 1664525u)) + (len == 2 ? add_odd : add_even);
  m1 = prev;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the chunks are read back below (same lane, same addresses)
  seed_u4 n0[4], n1[4];  // the next two chunks, in flight
#pragma unroll
  for (int v = 0; v < 4; v++) { n0[v] = tmp[v * WG]; n1[v] = tmp[(4 + v) * WG]; }
  for (int base = 0; base < 624; base += 16) {  // second loop, i = 2 .. 623
    uint32_t m[16];
#pragma unroll
    for (int v = 0; v < 4; v++) { m[4 * v] = n0[v].x; m[4 * v + 1] = n0[v].y; m[4 * v + 2] = n0[v].z; m[4 * v + 3] = n0[v].w; n0[v] = n1[v]; }
    if (base + 32 < 624) {
#pragma unroll
      for (int v = 0; v < 4; v++) n1[v] = tmp[((base + 32) / 4 + v) * WG];
    }
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int i = base + q;
      if (i >= 2) { prev = (m[q] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i; m[q] = prev; }
    }
#pragma unroll
    for (int v = 0; v < 4; v++) mt4[base / 4 + v] = seed_u4{m[4 * v], m[4 * v + 1], m[4 * v + 2], m[4 * v + 3]};  // (chunk 0 carries mt[0] = 0x80000000 and a stale mt[1])
  }
  // 623rd iteration of the second loop: i wrapped to 1 with mt[0] = mt[623]
  prev = (m1 ^ ((prev ^ (prev >> 30)) * 1566083941u)) - 1u;
  mt[1] = prev;  // (after the chunk store above: stores of one lane to one address land in order)
}
// i-th output word of the first block after seeding (i < 227), from this lane's state in global memory
DEV uint32_t seed_output(const uint32_t* mt, int i) {
  const uint32_t y = (mt[i] & 0x80000000u) | (mt[i + 1] & 0x7fffffffu);
  uint32_t v = mt[i + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  v ^= (v >> 11); v ^= (v << 7) & 0x9d2c5680u; v ^= (v << 15) & 0xefc60000u; v ^= (v >> 18);
  return v;
}
// One wave = 16 envs x 4 streams, one lane each.  Phase 1: the agent-stream lanes run init_by_array(seed) and draw the three
// stream seeds (Random.randint(0, 2^63-1) == _randbelow(2^63): getrandbits(64) until < 2^63, in the order obs, tgt, mission,
// DroneEnv.py:535-538); phase 2: the obs / tgt / mission lanes run theirs, the seeds handed over by a lane shuffle.  No LDS and
// ~40 VGPRs: the waves find room next to a running rollout, so the seeding of the NEXT launch overlaps all of this one.
__global__ __launch_bounds__(WG, 8) void k_seed(const uint64_t* seeds, int n, int with_obs, uint32_t* seedbuf, uint32_t* seedtmp) {
  const int lane = threadIdx.x, el = lane >> 2, st = lane & 3;
  const int e = blockIdx.x * 16 + el;
  uint32_t* mt = seedbuf + ((size_t)blockIdx.x * WG + lane) * 624;  // [N][4][624]: this lane's stream
  seed_u4* tmp = reinterpret_cast<seed_u4*>(seedtmp) + (size_t)blockIdx.x * 156 * WG + lane;  // this wave's [156][64] scratch vectors
  unsigned long long d0 = 0, d1 = 0, d2 = 0;
  if (e < n && st == ST_AGENT) {
    const uint64_t seed = seeds[e];
    seed_stream(mt, tmp, (uint32_t)seed, (uint32_t)(seed >> 32), (seed >> 32) ? 2 : 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int i = 0, j = 0;
    while (j < 3 && i <= 220) {  // (110 rejections in a row: the three seeds stay 0)
      const uint64_t lo = seed_output(mt, i), hi = seed_output(mt, i + 1);
      i += 2;
      const uint64_t r = lo | (hi << 32);
      if (r < (1ull << 63)) { if (j == 0) d0 = r; else if (j == 1) d1 = r; else d2 = r; j++; }
    }
  }
  // the agent lane of each env hands its draws to the env's other lanes
  const int src = lane & ~3;
  d0 = __shfl(d0, src); d1 = __shfl(d1, src); d2 = __shfl(d2, src);
  if (e < n && st != ST_AGENT && (st != ST_OBS || with_obs)) {
    const uint64_t sd = st == ST_OBS ? d0 : st == ST_TGT ? d1 : d2;
    seed_stream(mt, tmp, (uint32_t)sd, (uint32_t)(sd >> 32), (sd >> 32) ? 2 : 1);
  }
}

template <class TL>
__global__ __launch_bounds__(WG) void k_reset(const DevCtx* __restrict__ ctxp, const uint64_t* seeds, const uint32_t* seedbuf) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = blockIdx.x;
  Lds<TL> L(smem);
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, tape_of(ctx, env));
  sim.reset(seeds[env], seedbuf + (size_t)env * 4 * 624);
  obs_for_env(sim, ctx.P, obs_ptrs(ctx), env);
  lds_sync();
  copy16(blob_of<TL>(ctx, env), L.S, sizeof(EnvState<TL>));
}

// act_agent == nullptr: use the actions staged in the blob by k_allocate
template <class TL>
__global__ __launch_bounds__(WG, TILE_MIN_WAVES(TL)) void k_step(const DevCtx* __restrict__ ctxp, const int32_t* act_agent, const int32_t* act_index, int act_cap,
                                             double* rel_log, int env_base) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const DevParams& P = ctx.P;
  const int env = env_base + blockIdx.x;  // (env_base: the first env of a sub-batch launched on its own stream, muavta_*_part)
  KERNEL_LDS(TL);
  Lds<TL> L(lds_own + lds_zero());
  EnvState<TL>* blob = blob_of<TL>(ctx, env);
  copy16(L.S, blob, sizeof(EnvState<TL>));
  lds_sync();
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, P, tape_of(ctx, env));
  if (rel_log) sim.rel_log = rel_log + (size_t)env * (1 + MUAVTA_REL_ROW * TL::T);
  if (act_agent) {
    // the env's row of (agent, index) items: the first TL::A of them are staged here, a longer row (muavta_step_lists) is
    // consumed by the action phase A items at a time
    sim.more_agent = act_agent + (size_t)env * act_cap; sim.more_index = act_index + (size_t)env * act_cap;
    sim.more_cap = act_cap; sim.more_pos = 0;
    sim.stage_more();
    if (act_cap <= TL::A) sim.more_agent = nullptr;  // (uniform: nothing beyond the staged items)
  }
  lds_sync();
  sim.step(true);
  obs_for_env(sim, P, obs_ptrs(ctx), env);
  lds_sync();
  copy16(blob, L.S, sizeof(EnvState<TL>));
}

enum { SCORED_EXTRA_LDS = 128 };  // allocate<true>'s task list: one byte per slot, behind the tile
static_assert(Lds<Tile16>::bytes() + SCORED_EXTRA_LDS <= 10240, "k_run / k_rl_step / the learned policies' rollouts of Tile16 no longer fit 16 workgroups per CU");
// The allocator a k_allocate / k_rollout instantiation runs, as ONE tag type: the Hungarian family and the classical baselines pick their
// variant from the run-time `mode`; a learned policy is named by its traits (muavta_device.h).  A tag gives the LDS its kernels need behind
// the tile (allocate<true>'s task list) and the waves per SIMD its rollout is built for.  A fourth learned policy is a traits type next to
// the three in muavta_device.h, whatever of sim/policy.inc's forward pass its traits cannot express, and one line each in with_policy
// and for_each_policy (abi/handle.inc): every kernel instantiation, launch attribute and host-side size follows from there.
struct AllocHungarian { enum { EXTRA_LDS = 0, MAX_WAVES = 8, WIDE = 0 }; };  // MUAVTA_ALLOC_HUNGARIAN .. _HUNGARIAN_GATED (sim/allocate.inc)
// MUAVTA_ALLOC_URGENCY_PAIR at the wide token pads (MUAVTA_F_TOKEN_PADS = (64, 48)): allocate() with PAD_T x PAD_A = 64 x 48.  The tiles with more than 16 agent rows only
struct AllocUrgencyWide { enum { EXTRA_LDS = 0, MAX_WAVES = 8, WIDE = 1 }; };
struct AllocBaseline { enum { EXTRA_LDS = 0, MAX_WAVES = 8, WIDE = 0 }; };   // MUAVTA_ALLOC_CAP_GREEDY, _PI (sim/baselines.inc): the Hungarian kernels do not carry this code
template <class POL>
struct AllocLearned { typedef POL Pol; enum { EXTRA_LDS = SCORED_EXTRA_LDS, MAX_WAVES = POL::MAX_WAVES, WIDE = POL::WIDE }; };  // MUAVTA_ALLOC_MLP_PAIR (sim/policy.inc)
// ... with the transition of every replan gate recorded (MuavtaRlRings of muavta_rollout_record): k_rollout only, PolPair and PolContextPair only.
// A tag of its own, not a value of k_rollout's REC: every instantiation the library had before keeps its name.
template <class POL>
struct AllocLearnedRl : AllocLearned<POL> {};
template <class AL> struct records_rl : std::false_type {};
template <class POL> struct records_rl<AllocLearnedRl<POL>> : std::true_type {};
// The one place that turns a tag into the allocator's call.  sc_list: EXTRA_LDS bytes of LDS behind the tile.  A macro on purpose: as a
// function (free or a member of Sim, both tried) the helper is one more level for the inliner, and with it the instruction streams of 24 of
// the code object's 83 functions change (every k_rollout but the baselines', every learned k_allocate; two swapped instructions in the
// Hungarian rollouts, 10 more VGPRs in k_allocate<.., AllocLearned<PolCoalition>>): profiles/allocator_tags_kernel_identity.txt.
#define RUN_ALLOCATOR(AL, sim, ctx, env, interval, use_vis, mode, sc_list)                                                                  \
  {                                                                                                                                        \
    if constexpr (std::is_same<AL, AllocHungarian>::value) (sim).allocate(interval, use_vis, mode);                                        \
    else if constexpr (std::is_same<AL, AllocUrgencyWide>::value) (sim).template allocate<false, 64, 48>(interval, use_vis, mode);         \
    else if constexpr (std::is_same<AL, AllocBaseline>::value) (sim).allocate_baseline(interval, use_vis, mode);                           \
    else (sim).template allocate_learned<typename AL::Pol>(interval, use_vis, (ctx).pol, as_global((ctx).pol.scratch) + (size_t)(env) * AL::Pol::FLOATS, sc_list); \
  }

template <class TL, class AL>
__global__ __launch_bounds__(WG) void k_allocate(const DevCtx* __restrict__ ctxp, int interval, int use_vis, int mode,
                                                 int32_t* out_agent, int32_t* out_index, int act_cap, int env_base) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = env_base + blockIdx.x;
  Lds<TL> L(smem);
  EnvState<TL>* blob = blob_of<TL>(ctx, env);
  copy16(L.S, blob, sizeof(EnvState<TL>));
  lds_sync();
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, tape_of(ctx, env));
  RUN_ALLOCATOR(AL, sim, ctx, env, interval, use_vis, mode, smem + Lds<TL>::bytes());
  lds_sync();
  if (out_agent) {
    const EnvState<TL>& S = *L.S;
    for (int k = threadIdx.x; k < act_cap; k += WG) {
      out_agent[(size_t)env * act_cap + k] = k < S.n_act ? S.act_agent[k] : -1;
      out_index[(size_t)env * act_cap + k] = k < S.n_act ? S.act_index[k] : 0;
    }
  }
  copy16(blob, L.S, sizeof(EnvState<TL>));
}

template <class TL>
__device__ __forceinline__ typename Sim<TL>::TokPtrs global_tok_ptrs(typename Sim<TL>::TokPtrs K) {  // kernel-argument pointers as global (not FLAT) accesses
  K.task_feats = as_global(K.task_feats); K.task_mask = as_global(K.task_mask); K.task_ids = as_global(K.task_ids);
  K.agent_feats = as_global(K.agent_feats); K.agent_mask = as_global(K.agent_mask); K.agent_ids = as_global(K.agent_ids);
  K.edge_valid = as_global(K.edge_valid); K.n_urgent = as_global(K.n_urgent); K.expert_mask = as_global(K.expert_mask);
  K.replanned = as_global(K.replanned);
  return K;
}

// muavta_allocate_scored: k_allocate with the caller's edge scores / priorities / reserved agents (Sim::allocate<true>).  The
// task list handed to the allocator sits in T bytes of LDS behind the tile.
template <class TL>
__global__ __launch_bounds__(WG) void k_allocate_scored(const DevCtx* __restrict__ ctxp, ScoredDev sc, int interval, int use_vis,
                                                        int32_t* out_agent, int32_t* out_index, int act_cap, int env_base) {
  static_assert(TL::T <= SCORED_EXTRA_LDS, "the scored allocator's task list is one byte per slot");
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = env_base + blockIdx.x;
  Lds<TL> L(smem);
  EnvState<TL>* blob = blob_of<TL>(ctx, env);
  copy16(L.S, blob, sizeof(EnvState<TL>));
  lds_sync();
  sc.scores = as_global(sc.scores); sc.pri = as_global(sc.pri); sc.reserved = as_global(sc.reserved);
  sc.selected = as_global(sc.selected); sc.replanned = as_global(sc.replanned);
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, tape_of(ctx, env));
  sim.template allocate<true>(interval, use_vis, 4, &sc, env, smem + Lds<TL>::bytes());
  lds_sync();
  if (out_agent) {
    const EnvState<TL>& S = *L.S;
    for (int k = threadIdx.x; k < act_cap; k += WG) {
      out_agent[(size_t)env * act_cap + k] = k < S.n_act ? S.act_agent[k] : -1;
      out_index[(size_t)env * act_cap + k] = k < S.n_act ? S.act_index[k] : 0;
    }
  }
  copy16(blob, L.S, sizeof(EnvState<TL>));
}

// muavta_rl_step_device: one iteration of run_rl_episode's loop body (experiments/train_pair_cost.py:139-153) per env and launch —
// policy.plan with the caller's scores (allocate<true>) -> _apply_assign -> env.step -> compute_s_wps -> build_tokens (next_tok) —
// with ONE load and ONE store of the env record instead of four (k_tokens, k_allocate_scored, k_step, k_metrics).
template <class TL>
__global__ __launch_bounds__(WG, TILE_MIN_WAVES(TL)) void k_rl_step(const DevCtx* __restrict__ ctxp, ScoredDev sc, typename Sim<TL>::TokPtrs K, int interval, int use_vis,
                                                                    int write_obs, double* s_wps, uint8_t* done, int n_envs, int env_base) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const DevParams& P = ctx.P;
  const int env = env_base + blockIdx.x;
  __shared__ __align__(16) unsigned char lds_own[Lds<TL>::bytes() + SCORED_EXTRA_LDS];
  Lds<TL> L(lds_own + lds_zero());
  EnvState<TL>* blob = blob_of<TL>(ctx, env);
  copy16(L.S, blob, sizeof(EnvState<TL>));
  lds_sync();
  sc.scores = as_global(sc.scores); sc.pri = as_global(sc.pri); sc.reserved = as_global(sc.reserved);
  sc.selected = as_global(sc.selected); sc.replanned = as_global(sc.replanned);
  K = global_tok_ptrs<TL>(K);
  s_wps = as_global(s_wps); done = as_global(done);
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, P, tape_of(ctx, env));
  const double before = sim.s_wps();
  if (!(L.S->terminated || L.S->truncated)) {  // (uniform)  the reference's loop ends with the episode (:139)
    sim.template allocate<true>(interval, use_vis, 4, &sc, env, lds_own + Lds<TL>::bytes());
    lds_sync();
    sim.step(true);
    if (write_obs) obs_for_env(sim, P, obs_ptrs(ctx), env);
    lds_sync();
  } else {
    if (sc.replanned && threadIdx.x == 0) sc.replanned[env] = 0;
    if (sc.selected) for (int i = threadIdx.x; i < sc.MA * sc.MT; i += WG) sc.selected[(size_t)env * sc.MA * sc.MT + i] = 0.f;
  }
  if (threadIdx.x == 0) {
    if (s_wps) { s_wps[env] = before; s_wps[(size_t)n_envs + env] = sim.s_wps(); }
    if (done) done[env] = (uint8_t)((L.S->terminated ? 1 : 0) | (L.S->truncated ? 2 : 0));
  }
  if (K.task_feats) {
    cold_sync();
    sim.tokens(K, env);  // next_tok (:150): the tokens the policy sees at the next iteration
  }
  lds_sync();
  copy16(blob, L.S, sizeof(EnvState<TL>));
}

// muavta_rl_run_device / muavta_step_run: run to the next replan gate.  The reference's trainer and evaluation loops consult the planner
// only when their gate fires and step with EMPTY actions otherwise (experiments/train_pair_cost.py:86-89,139-145; wps_eval.py:248-254,273):
//     if _should_replan(env, events): result = policy.plan(...); actions = _apply_assign(env, result)      <- the launch's FIRST step
//     obs, reward, done, trunc, info = env.step(actions)                                                    <- quiet steps: actions = {}
// One launch per env takes the first step with its plan — src 0: allocate<true> with the caller's scores under the caller's gate (one
// iteration of run_rl_episode: S_WPS before / after, next_tok, done); src 1: the actions muavta_allocate staged; src 2: the caller's
// action rows — and then keeps stepping quietly until the env's own gate fires again, its episode ends, or max_steps steps are taken
// (0: no bound).  Where it stopped: park tokens (what the policy sees next), park flags, the number of steps taken, the summed reward.
struct RunOut {
  double* s_wps;        // [2][N] S_WPS before / after the first step (src 0)
  uint8_t* done;        // [N] done flags after the first step (src 0: ep_done of the pushed transition)
  int32_t* n_stepped;   // [N] env steps this launch took
  uint8_t* park;        // [N] bit 0 terminated, bit 1 truncated, bit 2 stopped at a gate (the next launch plans)
  double* reward_sum;   // [N] rewards of this launch's steps, added in step order
};
enum { RUN_SRC_SCORED = 0, RUN_SRC_STAGED = 1, RUN_SRC_ROWS = 2 };
// The launch's tensors (~45 pointers) are a by-value kernel argument that the body never names: it reads them from the KERNARG SEGMENT
// (constant memory, through the scalar cache) where they are used, like the context.  Named, the compiler loads every argument in the
// prologue and keeps them live across the step loop (first build: 259 SGPR spill stores and 60 spilled VGPRs on the 16-agent tile).
template <class TL> struct RunArgs { ScoredDev sc; typename Sim<TL>::TokPtrs K, KP; RunOut R; };
template <class TL>
__global__ __launch_bounds__(WG, TILE_MIN_WAVES(TL)) void k_run(RunArgs<TL> args_in_kernarg_segment, const DevCtx* __restrict__ ctxp, int src, int gate, int interval, int use_vis,
                                                                int write_obs, int max_steps, const int32_t* act_agent, const int32_t* act_index, int act_cap, int n_envs,
                                                                int env_base) {
  static_assert(alignof(RunArgs<TL>) <= 8, "first kernel argument: offset 0 of the kernarg segment");
  const uint64_t argp = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  const DevCtx& ctx0 = ctx_ref(ctxp);
  const int env = env_base + blockIdx.x;
  __shared__ __align__(16) unsigned char lds_own[Lds<TL>::bytes() + SCORED_EXTRA_LDS];
  Lds<TL> L(lds_own + lds_zero());
  EnvState<TL>* blob = blob_of<TL>(ctx0, env);
  copy16(L.S, blob, sizeof(EnvState<TL>));
  lds_sync();
  const uint32_t arg_lo = __builtin_amdgcn_readfirstlane((uint32_t)argp), arg_hi = __builtin_amdgcn_readfirstlane((uint32_t)(argp >> 32));
  int n = 0;
  bool at_gate = false;
  double rsum = 0.0;
  const bool over0 = L.S->terminated || L.S->truncated;  // (uniform)  the reference's loops end with the episode: such an env is left alone
  for (;;) {  // ONE call site each for the planner, the step and the token builder; every iteration builds its own Sim (lane-derived values
              // and launch constants must not be hoisted across the step: see k_rollout)
    uint32_t lo = arg_lo, hi = arg_hi;
    asm volatile("" : "+s"(lo), "+s"(hi));
    const RunArgs<TL>& G = *(const RunArgs<TL>*)(const AS4 RunArgs<TL>*)(((uint64_t)hi << 32) | (uint64_t)lo);
    const DevCtx& ctx = ctx_ref(ctxp);
    Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, tape_of(ctx, env));
    const bool first = n == 0;
    if (!over0) {
      if (first) {
        if (src == RUN_SRC_SCORED) {
          ScoredDev sc = G.sc;
          sc.scores = as_global(sc.scores); sc.pri = as_global(sc.pri); sc.reserved = as_global(sc.reserved);
          sc.selected = as_global(sc.selected); sc.replanned = as_global(sc.replanned);
          if (threadIdx.x == 0 && G.R.s_wps) as_global(G.R.s_wps)[env] = sim.s_wps();  // before the step
          sim.template allocate<true>(interval, use_vis, 4, &sc, env, lds_own + Lds<TL>::bytes());
          lds_sync();
        } else if (src == RUN_SRC_ROWS) {
          sim.more_agent = act_agent + (size_t)env * act_cap; sim.more_index = act_index + (size_t)env * act_cap;
          sim.more_cap = act_cap; sim.more_pos = 0;
          sim.stage_more();
          if (act_cap <= TL::A) sim.more_agent = nullptr;  // (uniform: nothing beyond the staged items)
          lds_sync();
        }
      } else {
        if (threadIdx.x == 0) L.S->n_act = 0;  // env.step({})
        lds_sync();
      }
      sim.step(true);
      n++;
      lds_sync();
      rsum += L.S->last_reward;
    } else if (src == RUN_SRC_SCORED) {
      const ScoredDev& sc = G.sc;
      if (sc.replanned && threadIdx.x == 0) as_global(sc.replanned)[env] = 0;
      if (sc.selected) for (int i = threadIdx.x; i < sc.MA * sc.MT; i += WG) as_global(sc.selected)[(size_t)env * sc.MA * sc.MT + i] = 0.f;
      if (threadIdx.x == 0 && G.R.s_wps) as_global(G.R.s_wps)[env] = sim.s_wps();
    }
    const bool over = L.S->terminated || L.S->truncated;
    if (!over) at_gate = sim.gate_fires(gate, interval);
    const bool stop = over || at_gate || (max_steps > 0 && n >= max_steps);
    const bool planned = first && src == RUN_SRC_SCORED && !over0 && L.S->gate_step == sim.tnow;  // (uniform) the gate fired at the step just taken: an RL sample
    if (first && src == RUN_SRC_SCORED && threadIdx.x == 0) {
      if (G.R.s_wps) as_global(G.R.s_wps)[(size_t)n_envs + env] = sim.s_wps();
      if (G.R.done) as_global(G.R.done)[env] = (uint8_t)((L.S->terminated ? 1 : 0) | (L.S->truncated ? 2 : 0));
    }
    // next_tok of the planned step (train_pair_cost.py:150-151) and / or the tokens of the state the env stops in
#pragma nounroll
    for (int w = 0; w < 2; w++) {
      const typename Sim<TL>::TokPtrs& Kc = w == 0 ? G.K : G.KP;
      const bool want = Kc.task_feats != nullptr && (w == 0 ? planned : stop);
      if (!want) continue;
      const typename Sim<TL>::TokPtrs cur = global_tok_ptrs<TL>(Kc);
      cold_sync();
      sim.tokens(cur, env);
      lds_sync();
    }
    if (stop) {
      if (write_obs && !over0) { obs_for_env(sim, ctx.P, obs_ptrs(ctx), env); lds_sync(); }
      if (threadIdx.x == 0) {
        if (G.R.n_stepped) as_global(G.R.n_stepped)[env] = n;
        if (G.R.park) as_global(G.R.park)[env] = (uint8_t)((L.S->terminated ? 1 : 0) | (L.S->truncated ? 2 : 0) | (at_gate ? 4 : 0));
        if (G.R.reward_sum) as_global(G.R.reward_sum)[env] = rsum;
      }
      break;
    }
  }
  lds_sync();
  copy16(blob, L.S, sizeof(EnvState<TL>));
}

// The body of the fused rollout, OUT OF LINE on purpose.  Inlined into the 150-step loop of k_rollout the compiler hoists
// loop invariants across the whole body and the kernel needs 255 VGPRs (+188 B/lane of scratch: two waves per SIMD); as a
// function of its own the body fits the 128 VGPRs of FOUR waves per SIMD — with 10 KiB of LDS per env that is 16 resident
// envs per CU, the whole 4096-env batch in one round.  The function must not name the `extern __shared__` array (every
// reference becomes a load from the dynamic-LDS offset table) nor take generic pointers (FLAT accesses): it gets the LDS
// base as a number and rebuilds typed pointers.  An iteration is  step -> observation write -> NEXT step's allocate:
// the function's return waits for all memory operations, and this way the observation stores have drained by then.
#ifndef MUAVTA_PHASE_ATTR
#define MUAVTA_PHASE_ATTR __forceinline__
#define MUAVTA_PHASE_INLINED 1  // the body sees the kernel's own `smem`: LDS addresses fold to constants + lane offsets
#else
#define MUAVTA_PHASE_INLINED 0
#endif
enum { PH_ALLOC = 1, PH_STEP = 2, PH_OBS = 4 };
// muavta_rollout_record: per-step training data of the fused rollout in caller-owned rings [n_slots][N][...] — the token
// tensors / expert labels of the plan staged for step t and S_WPS before step t (experiments/train_pair_cost.py:96-156).
template <class TL>
struct RecordPtrs {
  typename Sim<TL>::TokPtrs K;  // K.task_feats == nullptr: no token rings
  double* s_wps;   // [n_steps + 1][N]
  ObsPtrs O;       // O.tasks == nullptr: no observation rings
  int n_envs;
};
struct RecBlob { uint32_t w[64]; };  // 256 B: a RecordPtrs<TL> by value
__global__ void k_store_rec(RecBlob b, uint32_t* dst) { dst[threadIdx.x] = b.w[threadIdx.x]; }

// The RL half of muavta_rollout_record (MuavtaRlRings): per-GATE rings [n_slots][N][...] of the transitions run_rl_episode pushes
// (experiments/train_pair_cost.py:131-156).  The pointers sit in a device slot of their own (the handle's third record slot) that the
// instantiations with an AllocLearnedRl tag — and only they — are handed in place of a RecordPtrs.
struct RlTokRings { float* task_feats; uint8_t* task_mask; float* agent_feats; uint8_t* agent_mask; float* edge_valid; float* context; };
struct RlRingsDev {
  RlTokRings tok, next;  // build_tokens(env) (+ the context vector) at the gate / after the step that follows it
  float *logits, *scores, *noise, *selected;  // [n_slots][N][MA][MT]; noise: input and output, or null
  double *s_wps_before, *s_wps_after;         // [n_slots][N]
  uint8_t* done;                              // [n_slots][N]
  int32_t *step, *n_gates;                    // [n_slots][N] (pre-filled with -1), [N] (pre-filled with 0)
  int32_t n_slots, n_envs;
};
static_assert(sizeof(RlRingsDev) <= sizeof(RecBlob), "k_store_rec moves one RecBlob");
// The token block of the plan in the env's scratch (policy_tokens; with env-uniform inputs: context_prefix behind it), complete and visible,
// into row `at` = slot * N + env of a ring set.  The rows are compact in the block too: [MT][dt(raw)], [MA][da(raw)].
template <class POL>
__device__ __forceinline__ void rl_store_tokens(const RlTokRings& R, const PairPolicyDev& pol, const float* blk, size_t at) {
  typedef typename POL::Blk B;
  static_assert(B::MT <= WG && B::MA <= WG, "one pad-mask byte per lane");
  const int lane = threadIdx.x, Dt = POL::dt(pol.raw != 0), Da = POL::da(pol.raw != 0);
  float *tf = as_global(R.task_feats) + at * (size_t)(B::MT * Dt), *af = as_global(R.agent_feats) + at * (size_t)(B::MA * Da);
  float* ev = as_global(R.edge_valid) + at * (size_t)(B::MA * B::MT);
  for (int i = lane; i < B::MT * Dt; i += WG) tf[i] = blk[B::TF + i];
  for (int i = lane; i < B::MA * Da; i += WG) af[i] = blk[B::AF + i];
  for (int i = lane; i < B::MA * B::MT; i += WG) ev[i] = blk[B::EV + i];
  const uint8_t *tm = reinterpret_cast<const uint8_t*>(blk + B::TMASK), *am = reinterpret_cast<const uint8_t*>(blk + B::AMASK);
  if (lane < B::MT) as_global(R.task_mask)[at * B::MT + lane] = tm[lane];
  if (lane < B::MA) as_global(R.agent_mask)[at * B::MA + lane] = am[lane];
  if constexpr (POL::np(false) > 0) {  // the context vector: the tail of the env-uniform head of layer 1's input row
    const int nc = pol.raw ? 1 : 8;
    if (lane < nc) as_global(R.context)[at * nc + lane] = blk[POL::PRE + Da + Dt + lane];
  }
}
// A gate fired and its tokens are in the scratch block: count it, and if it still has a slot, store what is known before the forward pass
// (tokens, time step, S_WPS) and hand the slot's [MA][MT] blocks to the plan.  The count lives in n_gates[env] between the phases — no
// register is carried across the step body — and is this wave's alone.
template <class TL, class POL>
__device__ __forceinline__ typename Sim<TL>::RlGate rl_gate_open(Sim<TL>& sim, const RlRingsDev& R, const PairPolicyDev& pol, const float* blk, int env) {
  typename Sim<TL>::RlGate g{nullptr, nullptr, nullptr, nullptr};
  int32_t* ng = as_global(R.n_gates) + env;
  const int k = __builtin_amdgcn_readfirstlane(*ng);
  if (threadIdx.x == 0) *ng = k + 1;
  if (k >= R.n_slots) return g;  // (uniform)
  const size_t at = (size_t)k * R.n_envs + env, cell0 = at * (size_t)(POL::Blk::MA * POL::Blk::MT);
  rl_store_tokens<POL>(R.tok, pol, blk, at);
  if (threadIdx.x == 0) { as_global(R.step)[at] = sim.tnow; as_global(R.s_wps_before)[at] = sim.s_wps(); }
  g.scores = as_global(R.scores) + cell0; g.logits = as_global(R.logits) + cell0; g.selected = as_global(R.selected) + cell0;
  if (R.noise) g.noise = as_global(R.noise) + cell0;
  return g;
}
// The step that followed a gate is done: S_WPS and the done bits after it, and the tokens of the state it left (also of a final state, as the
// reference builds them, :150-151).  The scratch block is free for that: the next gate rebuilds it, and no plan reads it in between.
template <class TL, class POL>
__device__ __forceinline__ void rl_after_step(Sim<TL>& sim, const RlRingsDev& R, const PairPolicyDev& pol, float* blk, int env) {
  const int k = __builtin_amdgcn_readfirstlane(as_global(R.n_gates)[env]) - 1;  // the gate of the step just taken
  if (k < 0 || k >= R.n_slots) return;  // (uniform)
  const size_t at = (size_t)k * R.n_envs + env;
  if (threadIdx.x == 0) {
    as_global(R.s_wps_after)[at] = sim.s_wps();
    as_global(R.done)[at] = (uint8_t)((sim.S.terminated ? 1 : 0) | (sim.S.truncated ? 2 : 0));
  }
  sim.template policy_tokens<POL>(pol, blk);
  if constexpr (POL::np(false) > 0) sim.template context_prefix<POL>(pol, blk);
  rl_store_tokens<POL>(R.next, pol, blk, at);
}

template <class TL, bool REC, class AL>
__device__ MUAVTA_PHASE_ATTR void rollout_phase(const DevCtx* ctxp, unsigned char* lds_own, uint32_t lds_base, int env, int phases, int interval, int use_vis, int mode,
                                                const RecordPtrs<TL>& rec, int slot, int oslot) {
  const DevCtx& ctx = ctx_ref(ctxp);
#if MUAVTA_PHASE_INLINED
  Lds<TL> L(lds_own + lds_zero());
#else
  Lds<TL> L((unsigned char*)(AS3 unsigned char*)(uintptr_t)__builtin_amdgcn_readfirstlane(lds_base));
#endif
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, tape_of(ctx, env));
  if (phases & PH_STEP) sim.step(true);
  if (phases & PH_OBS) {
    ObsPtrs O = obs_ptrs(ctx);
    int at = env;
    bool handle_buffer = true;
    if constexpr (REC) {
      if (oslot >= 0) {  // slot `oslot` of the caller's observation rings instead of the handle's single buffer (a fresh buffer: every row is written)
        handle_buffer = false;
        O.tasks = as_global(rec.O.tasks); O.legal = as_global(rec.O.legal); O.pad = as_global(rec.O.pad); O.agents = as_global(rec.O.agents);
        O.flags = as_global(rec.O.flags); O.reward = as_global(rec.O.reward); O.done = as_global(rec.O.done);
        at = oslot * rec.n_envs + env;
      }
    }
    obs_for_env(sim, ctx.P, O, at, handle_buffer);
  }
  lds_sync();
  if constexpr (records_rl<AL>::value) {  // (such a launch's `rec` is the handle's RlRingsDev slot)
    if ((phases & PH_STEP) && L.S->gate_step == sim.tnow)  // (uniform) the gate fired at the step just taken: its transition is completed
      rl_after_step<TL, typename AL::Pol>(sim, reinterpret_cast<const RlRingsDev&>(rec), ctx.pol, as_global(ctx.pol.scratch) + (size_t)env * AL::Pol::FLOATS, env);
  }
  if (!ABL(9) && (phases & PH_ALLOC) && !(L.S->terminated || L.S->truncated)) {
    if constexpr (records_rl<AL>::value) {
      typedef typename AL::Pol POL;
      float* blk = as_global(ctx.pol.scratch) + (size_t)env * POL::FLOATS;
      sim.template allocate_learned_rl<POL>(interval, use_vis, ctx.pol, blk, reinterpret_cast<unsigned char*>(L.S) + Lds<TL>::bytes() + PROF_EXTRA_LDS,
                                            [&]() { return rl_gate_open<TL, POL>(sim, reinterpret_cast<const RlRingsDev&>(rec), ctx.pol, blk, env); });
    } else
    RUN_ALLOCATOR(AL, sim, ctx, env, interval, use_vis, mode, reinterpret_cast<unsigned char*>(L.S) + Lds<TL>::bytes() + PROF_EXTRA_LDS);
    if (REC && rec.K.task_feats) {  // the sample of step `slot`: tokens + labels of the plan just staged, S_WPS before the step
      const typename Sim<TL>::TokPtrs K = global_tok_ptrs<TL>(rec.K);
      cold_sync();
      sim.tokens(K, slot * rec.n_envs + env);
      if (threadIdx.x == 0) as_global(rec.s_wps)[(size_t)slot * rec.n_envs + env] = sim.s_wps();
      lds_sync();
    }
  }
  PROF_AT(sim, 20);
}

// (a learned policy's forward pass keeps a pair's hidden activations in registers, so AL caps the waves per SIMD its instantiations are
// built for — PolPair: 128 activations, ~145 VGPRs, three waves, 168 VGPRs, where the tile's other kernels are built for four; PolContextPair:
// 192, two waves, 256 VGPRs; PolCoalition: 256, one wave — about 480 of the unified 512-entry register file, the allocator's placement, no spill)
template <class TL, bool REC, class AL>
__global__ __launch_bounds__(WG, TILE_MIN_WAVES(TL) < AL::MAX_WAVES ? TILE_MIN_WAVES(TL) : AL::MAX_WAVES) void k_rollout(const DevCtx* __restrict__ ctxp, const uint64_t* seeds, int n_steps, int interval, int use_vis,
                                                int mode, int write_obs, double* metrics, const uint32_t* seedbuf, const RecordPtrs<TL>* __restrict__ recp, int epoch, int env_base) {
  const DevCtx& ctx = ctx_ref(ctxp);
  // The ring pointers of muavta_rollout_record sit in device memory (one slot per handle, written on the launch's stream just ahead of
  // it) and are read through the scalar cache where they are used, like the context: as by-value kernel arguments they were ~40
  // SGPRs that the recording variants kept alive across the whole step loop (r3: 176-181 SGPR spills, 8 spilled VGPRs + 48 B of
  // scratch on the 24-agent tile).  The plain rollout gets the handle's all-zero slot and never reads it.
  const uint32_t rec_lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)recp), rec_hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)recp >> 32));
  // (unsigned halves: v_readfirstlane returns int, and a low word with bit 31 set would sign-extend into the high word)
  const RecordPtrs<TL>& rec = *(const RecordPtrs<TL>*)(const AS4 RecordPtrs<TL>*)(((uint64_t)rec_hi << 32) | (uint64_t)rec_lo);
  const int env = env_base + blockIdx.x;
  __shared__ __align__(16) unsigned char lds_own[Lds<TL>::bytes() + PROF_EXTRA_LDS + AL::EXTRA_LDS];  // KERNEL_LDS(TL) (+ a learned policy: allocate<true>'s task list)
  Lds<TL> L(lds_own);
  EnvState<TL>* blob = blob_of<TL>(ctx, env);
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, tape_of(ctx, env));
// (r4) The pacing row is read and written with WORKGROUP-scope (plain) accesses: the waves that share a row share a SIMD, hence a CU
// and its vector L1, which is coherent for them; a slightly stale counter only delays a priority change by a step.  With AGENT scope
// (r2, r3) every step's 16-lane read went to the memory side of the fabric (~2 us on this eight-XCD part) and — VMEM loads return in
// order — the step's first `s_waitcnt vmcnt(0)` waited for it: tools/ablate_probe.py measured the whole pacing block at 0.35 ms of a
// 1.19 ms quiet launch.  Headline 240 -> 248 M on one box (profiles/r04_ab_pacing.txt); publishing every 2nd / 4th step changes nothing.
// NOTE on the memory model: the waves that share a row belong to DIFFERENT workgroups (one env per workgroup), and workgroup scope
// promises nothing across workgroups — it works because they share a CU's L1, and would stop working under tgsplit / another CU mode.
// Correctness never depends on a loaded value: the row only feeds s_setprio and (MUAVTA_PACE_HOLD builds) a sleep loop whose polls are
// bounded by MUAVTA_PACE_HOLD_POLLS; a build that holds on these values uses AGENT scope.  -DMUAVTA_PACE_SCOPE overrides.
#ifndef MUAVTA_PACE_SCOPE
#if MUAVTA_PACE_HOLD
#define MUAVTA_PACE_SCOPE __HIP_MEMORY_SCOPE_AGENT
#else
#define MUAVTA_PACE_SCOPE __HIP_MEMORY_SCOPE_WORKGROUP
#endif
#endif
static_assert(MUAVTA_PACE_HOLD_POLLS > 0 && MUAVTA_PACE_HOLD_POLLS <= (1 << 16), "the hold loop of the pacing block must be poll-bounded");
#ifndef MUAVTA_PACE_EVERY
#define MUAVTA_PACE_EVERY 1  // publish / read / re-rank every n-th step (a power of two)
#endif
#if MUAVTA_PACE_PRIO
  constexpr bool PACED = TL::A <= 32 && !ABL(10);  // the 64-agent tile has one or two waves per SIMD: nothing to pace
  // Pacing: the envs whose waves share a SIMD advance at different speeds (replans, episode length), and the launch ends on
  // the SIMD whose last env runs alone, at a quarter of the SIMD's multi-wave throughput.  Each wave publishes its step
  // counter in a row of the SIMD it runs on (hardware ids), reads its neighbours' and asks for issue priority while nobody
  // on the SIMD is further behind, so that the co-resident envs finish together.  Timing only: results do not depend on it.
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc_id = __builtin_amdgcn_s_getreg(20 | (3 << 11));
  uint32_t* pace_row = as_global(ctx.pace) + ((((xcc_id & 15u) << 12) | ((hw_id >> 4) & 0xFFFu)) << 4);
  const uint32_t pace_tag = (uint32_t)epoch << 16;
#endif
#ifdef MUAVTA_PROF
  sim.prof_begin();
#endif
#ifdef MUAVTA_DIAG_TIMES
  if (threadIdx.x == 0 && env < 65536) as_global(ctx.pace)[(1u << 19) + env] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  if (seeds) {
    sim.reset(seeds[env], seedbuf + (size_t)env * 4 * 624);
  } else {
    copy16(L.S, blob, sizeof(EnvState<TL>));
    lds_sync();
  }
  uint32_t lds_base = (uint32_t)(uintptr_t)(AS3 unsigned char*)lds_own;
#if !MUAVTA_PHASE_INLINED
  asm volatile("" : "+v"(lds_base));  // opaque: keeps constant propagation from re-introducing the symbol into the callee
#endif
  // schedule: [allocate] , n_steps x [step, observation, next allocate] , [observation if it was not written per step] —
  // driven through ONE call site so that an inlined build carries one copy of the body
  for (int k = n_steps > 0 ? 0 : n_steps + 1; k <= n_steps + 1; k++) {
    int ph;
    if (k == 0) ph = PH_ALLOC;
    else if (k <= n_steps) {
      if (L.S->terminated || L.S->truncated) {  // uniform: read from LDS after a barrier
        if constexpr (REC) {
          // the episode ended during step k - 1: the allocate of that step was skipped, so token slots k-1 .. n_steps-1 have no
          // sample.  They become all-pad rows with replanned = 0 and carry the final S_WPS forward (zero step reward), instead
          // of staying uninitialised ring memory (the observation rings mark theirs with MUAVTA_OBS_UNWRITTEN).
          if (rec.K.task_feats) {
            const typename Sim<TL>::TokPtrs K = global_tok_ptrs<TL>(rec.K);
            const double fin = sim.s_wps();
            for (int sl = k - 1; sl < n_steps; sl++) {
              sim.tokens_pad(K, sl * rec.n_envs + env);
              if (threadIdx.x == 0) as_global(rec.s_wps)[(size_t)sl * rec.n_envs + env] = fin;
            }
          }
        }
        k = n_steps;
        continue;
      }
      ph = PH_STEP | (write_obs ? PH_OBS : 0) | (k < n_steps ? PH_ALLOC : 0);
    } else ph = (write_obs && !(REC && rec.O.tasks)) ? 0 : PH_OBS;  // with observation rings the handle's buffer gets the final one
#if MUAVTA_PACE_PRIO
    uint32_t seen = 0;
    if (PACED && k >= 1 && k <= n_steps && (k & (MUAVTA_PACE_EVERY - 1)) == 0) {
      if (threadIdx.x == 0) __hip_atomic_store(pace_row + (hw_id & 15u), pace_tag | (uint32_t)k, __ATOMIC_RELAXED, MUAVTA_PACE_SCOPE);
      if (threadIdx.x < 16) seen = __hip_atomic_load(pace_row + threadIdx.x, __ATOMIC_RELAXED, MUAVTA_PACE_SCOPE);
    }
#endif
    if (ph) rollout_phase<TL, REC, AL>(ctxp, lds_own, lds_base, env, ph, interval, use_vis, mode, rec, k < n_steps ? k : n_steps,
                                   (REC && rec.O.tasks && k >= 1 && k <= n_steps) ? k - 1 : -1);
#if MUAVTA_PACE_PRIO
    if (PACED && k >= 1 && k <= n_steps && (k & (MUAVTA_PACE_EVERY - 1)) == 0) {  // consumed a step later: the load's latency stays off the env's dependent chain
      const bool behind_me = threadIdx.x < 16 && (seen >> 16) == (uint32_t)epoch && (seen & 0xFFFFu) < (uint32_t)k;
#if MUAVTA_PACE_PRIO == 4  // ranked: 3 for the last env of the SIMD, one less per neighbour that is further behind
      const int n_behind = __popcll(__ballot(behind_me));
      if (n_behind == 0) __builtin_amdgcn_s_setprio(3); else if (n_behind == 1) __builtin_amdgcn_s_setprio(2);
      else if (n_behind == 2) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
#else
      if (__ballot(behind_me) != 0ull) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(MUAVTA_PACE_PRIO);
#endif
#if MUAVTA_PACE_HOLD
      // Holding: a wave more than MUAVTA_PACE_HOLD steps AHEAD of a neighbour on its SIMD sleeps until that neighbour has caught up.
      // A wave is latency-bound (it uses about a third of the SIMD's issue slots and runs 1.33x faster alone than as one of
      // four), so an env with heavier steps falls behind whatever its priority and ends the launch running alone; the slots its
      // neighbours give up while they wait are the only thing that speeds it up.  The furthest-behind wave never waits (progress),
      // neighbours further behind than the window are ignored (a later workgroup that took over a wave slot of a multi-round
      // launch), and the polls are bounded.  Timing only.
      for (int polls = 0; polls < MUAVTA_PACE_HOLD_POLLS; polls++) {
        const uint32_t st = seen & 0xFFFFu;
        const bool wait_for = threadIdx.x < 16 && (seen >> 16) == (uint32_t)epoch && st + MUAVTA_PACE_HOLD < (uint32_t)k &&
                              st + MUAVTA_PACE_HOLD_WINDOW >= (uint32_t)k;
        if (__ballot(wait_for) == 0ull) break;
        __builtin_amdgcn_s_sleep(MUAVTA_PACE_HOLD_SLEEP);
        if (threadIdx.x < 16) seen = __hip_atomic_load(pace_row + threadIdx.x, __ATOMIC_RELAXED, MUAVTA_PACE_SCOPE);
      }
#endif
    }
#endif
  }
#if MUAVTA_PACE_PRIO
  if (PACED && threadIdx.x == 0) __hip_atomic_store(pace_row + (hw_id & 15u), pace_tag | 0xFFFFu, __ATOMIC_RELAXED, MUAVTA_PACE_SCOPE);
  __builtin_amdgcn_s_setprio(0);
#endif
  if (REC && rec.K.task_feats) {  // S_WPS after the last step closes the reward series
    if (threadIdx.x == 0) as_global(rec.s_wps)[(size_t)n_steps * rec.n_envs + env] = sim.s_wps();
  }
  sim.sync_clock();
  sim.metrics(as_global(metrics) + (size_t)env * MUAVTA_N_METRICS);
  lds_sync();
  copy16(blob, L.S, sizeof(EnvState<TL>));
#ifdef MUAVTA_PROF
  sim.prof_flush(env);
#endif
#ifdef MUAVTA_DIAG_TIMES  // tools/end_times_probe.py: when each env's wave ended and on which SIMD (rows of the pace table no SIMD key reaches)
  if (threadIdx.x == 0 && env < 65536) {
    as_global(ctx.pace)[(1u << 19) + 65536 + env] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    as_global(ctx.pace)[(1u << 19) + 131072 + env] = __builtin_amdgcn_s_getreg(4 | (31 << 11)) | (__builtin_amdgcn_s_getreg(20 | (3 << 11)) << 16);
  }
#endif
}

template <class TL>
__global__ __launch_bounds__(WG) void k_metrics(const DevCtx* __restrict__ ctxp, double* metrics) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = blockIdx.x;
  Lds<TL> L(smem);
  copy16(L.S, blob_of<TL>(ctx, env), sizeof(EnvState<TL>));
  lds_sync();
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, nullptr);
  sim.metrics(metrics + (size_t)env * MUAVTA_N_METRICS);
}

template <class TL>
__global__ __launch_bounds__(WG) void k_observe(const DevCtx* __restrict__ ctxp) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = blockIdx.x;
  Lds<TL> L(smem);
  copy16(L.S, blob_of<TL>(ctx, env), sizeof(EnvState<TL>));
  lds_sync();
  // muavta_refresh_observation is the FULL rewrite of the handle's observation buffers: pad rows included, whatever the record
  // believes they hold (a caller may have touched the zero-copy views of muavta_device_ptrs in place)
  if (threadIdx.x == 0) L.S->obs_rows = -1;
  lds_sync();
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, nullptr);
  obs_for_env(sim, ctx.P, obs_ptrs(ctx), env);
  lds_sync();
  if (threadIdx.x == 0) {  // the only fields this kernel changes in the record: which rows of the buffer hold pad rows now, and the
    EnvState<TL>* blob = blob_of<TL>(ctx, env);   // task times it rebuilt on the way (refresh_task_times)
    blob->obs_rows = L.S->obs_rows;
    blob->times_dirty = L.S->times_dirty;
  }
  if constexpr (TL::TIMES_LDS) {  // (those times are part of the record on this tile, not of the HBM part the rebuild wrote in place)
    EnvState<TL>* blob = blob_of<TL>(ctx, env);
    for (int s = threadIdx.x; s < TL::T; s += WG) { blob->t_init[s] = L.S->t_init[s]; blob->t_dtime[s] = L.S->t_dtime[s]; }
  }
}

template <class TL>
__global__ __launch_bounds__(WG) void k_tokens(const DevCtx* __restrict__ ctxp, typename Sim<TL>::TokPtrs K) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = blockIdx.x;
  Lds<TL> L(smem);
  copy16(L.S, blob_of<TL>(ctx, env), sizeof(EnvState<TL>));
  lds_sync();
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, nullptr);
  sim.tokens(K, env);
}

// muavta_pair_scores(_device): the installed policy's scores / logits of every env's CURRENT state — POL's tokens into the env's scratch
// block, then the forward pass of sim/policy.inc, the same code the MUAVTA_ALLOC_MLP_PAIR mode runs at a replan.  scores / logits:
// [N, POL::Blk::MA, POL::Blk::MT] (either may be null); entries whose edge_valid is 0 are written as 0.  The env records are not changed.
template <class TL, class POL>
__global__ __launch_bounds__(WG) void k_pair_scores(const DevCtx* __restrict__ ctxp, float* scores, float* logits) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = blockIdx.x;
  Lds<TL> L(smem);
  copy16(L.S, blob_of<TL>(ctx, env), sizeof(EnvState<TL>));
  lds_sync();
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, nullptr);
  float* scratch = as_global(ctx.pol.scratch) + (size_t)env * POL::FLOATS;
  sim.template policy_tokens<POL>(ctx.pol, scratch);
  const size_t at = (size_t)env * POL::Blk::MA * POL::Blk::MT;
  if constexpr (POL::np(false) > 0) sim.template context_prefix<POL>(ctx.pol, scratch);
  sim.template policy_forward<POL>(ctx.pol, scratch, scores ? as_global(scores) + at : nullptr, logits ? as_global(logits) + at : nullptr, true);
}

template <class TL>
__global__ __launch_bounds__(WG) void k_context(const DevCtx* __restrict__ ctxp, int raw, int max_tasks, float* out) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = blockIdx.x;
  Lds<TL> L(smem);
  copy16(L.S, blob_of<TL>(ctx, env), sizeof(EnvState<TL>));
  lds_sync();
  Sim<TL> sim(*L.S, *cold_of<TL>(ctx, env), *L.X, ctx.P, nullptr);
  sim.context(raw, max_tasks, as_global(out) + (size_t)env * (raw ? 1 : 8));
}

// muavta_call: one of the reference's out-of-step mutators on ONE env, with the device routines step() itself uses.
struct CallArgs { int32_t op, env, i[8]; double d; };
template <class TL>
__global__ __launch_bounds__(WG) void k_call(const DevCtx* __restrict__ ctxp, CallArgs a, int32_t* out) {
  const DevCtx& ctx = ctx_ref(ctxp);
  const int env = a.env, lane = threadIdx.x;
  Lds<TL> L(smem);
  EnvState<TL>& S = *L.S;
  EnvState<TL>* blob = blob_of<TL>(ctx, env);
  copy16(L.S, blob, sizeof(EnvState<TL>));
  lds_sync();
  Sim<TL> sim(S, *cold_of<TL>(ctx, env), *L.X, ctx.P, tape_of(ctx, env));
  auto slot_of = [&](int id) -> int {  // uniform: the live slot holding task `id`, or -1
    int found = -1;
    for (int base = 0; base < TL::T; base += WG) {
      const int s = base + lane;
      const unsigned long long m = __ballot(id > 0 && s < TL::T && S.t_id[s] == id);
      if (m) found = base + __ffsll((long long)m) - 1;
    }
    return found;
  };
  for (int k = lane; k < MUAVTA_CALL_OUT; k += WG) out[k] = 0;
  __syncthreads();
  const int ag = a.i[0];
  switch (a.op) {
    case MUAVTA_OP_UAV_ALLOCATE: {
      const int s = slot_of(a.i[1]);
      sim.tnow = a.i[2];
      if (lane == 0) out[0] = (s >= 0 && sim.uav_allocate(ag, s)) ? 1 : 0;
    } break;
    case MUAVTA_OP_CREATE_ESCORT: {
      const int s = slot_of(a.i[1]);
      if (lane == 0) {
        S.list_stale = 1;  // (a task may be born behind last_tasks_info: Sim::allocate extends its list)
        if (ctx.P.escort_enabled && (s >= 0 || a.i[1] == 0)) sim.create_escort_for(ag, s);  // rec_task None (id 0): protected_task = None
        const int k = sim.escort_lookup(ag);
        out[0] = (ctx.P.escort_enabled && k >= 0) ? (int)S.esc_id[k] : -1;
      }
    } break;
    case MUAVTA_OP_SYNC_ESCORTS:
      if (lane == 0) S.list_stale = 1;
      lds_sync();
      if (ctx.P.escort_enabled) sim.sync_escorts_coop();
      break;
    case MUAVTA_OP_RETIRE_ESCORT:
      if (lane == 0)
        for (int k = 0; k < S.n_escorts; k++)
          if (S.esc_id[k] == a.i[0]) { sim.retire_escort_entry(k, a.i[1] != 0); break; }
      break;
    case MUAVTA_OP_ESCORT_FIGHTERS_NEAR:
      if (lane == 0) {
        int16_t* who = L.X->remaining;
        const int n = sim.escort_fighters_near(ag, a.d < 0 ? ctx.P.escort_radius : a.d, who, L.X->v);
        out[0] = n;
        for (int k = 0; k < n && k + 1 < MUAVTA_CALL_OUT; k++) out[1 + k] = who[k];
      }
      break;
    case MUAVTA_OP_ACTION_VALID: {
      const int s = slot_of(a.i[1]);
      if (lane == 0) out[0] = (s >= 0 && sim.action_valid(ag, s)) ? 1 : 0;
    } break;
    case MUAVTA_OP_SET_QUEUE: {
      int slots[6];
      for (int k = 0; k < 6; k++) slots[k] = (k < a.i[1]) ? slot_of(a.i[2 + k]) : -1;
      if (lane == 0) {
        int n = 0;
        for (int k = 0; k < a.i[1] && k < 6 && n < TL::Q; k++) {
          if (a.i[2 + k] == 0 || slots[k] < 0) continue;  // task_idle, or a task that is no longer resident
          S.a_qid[ag][n] = (i16)a.i[2 + k]; S.a_qslot[ag][n] = (i8)slots[k]; sim.C.a_qtime[ag][n] = 0.0;
          n++;
        }
        S.a_qlen[ag] = (i8)n;
        if (a.i[7] == 1 && n == 0) {  // UAV.allocate(task_idle) (DroneEnvComponents.py:59-60,85-92): more than the list assignment
          S.a_reeval[ag] = 0; S.a_last_id[ag] = -1; S.a_last_slot[ag] = -1;
          sim.qs().a_nft[ag] = 0.0; sim.qs().a_nfx[ag] = S.a_px[ag]; sim.qs().a_nfy[ag] = S.a_py[ag];
        }
      }
    } break;
    default: break;
  }
  cold_sync();
  sim.refresh_task_times();  // initTime / doneTime follow the allocationDetails the call may have changed
  lds_sync();
  copy16(blob, L.S, sizeof(EnvState<TL>));
}

// Stand-alone LSAP: one problem per workgroup, cost tile staged in LDS (transposed when nc < nr).
// REG: the register-resident solver of the allocator path (rows <= 32, columns <= 64); else the LDS solver (64 x 128).
typedef Tile<32, 64, 16, 16, 16, 8> TileLsapReg;
typedef Tile<64, 128, 16, 16, 16, 8> TileLsapLds;  // keeps the full cost tile in LDS (the env's 64x128 tile evaluates costs on the fly)
// What a stand-alone solve reports (lane 0): the status word, and the assignment in scipy's output form — rows ascending, min(nr, nc) pairs
template <class TL>
__device__ __forceinline__ void lsap_probe_out(const Lds<TL>& L, int prob, int nr, int nc, int64_t* row, int64_t* col, int32_t* status) {
  if (threadIdx.x != 0) return;
  const bool tr = nc < nr;
  const int Rr = tr ? nc : nr;
  status[prob] = L.S->error;  // MUAVTA_ERR_LSAP: no finite assignment (scipy: "cost matrix is infeasible")
  int64_t* r = row + (size_t)prob * Rr;
  int64_t* cc = col + (size_t)prob * Rr;
  int n = 0;
  if (!tr) { for (int i = 0; i < nr; i++) { r[n] = i; cc[n] = L.X->col4row[i]; n++; } }
  else { for (int i = 0; i < nr; i++) if (L.X->row4col[i] >= 0) { r[n] = i; cc[n] = L.X->row4col[i]; n++; } }
}
template <class TL, bool REG>
__global__ __launch_bounds__(WG) void k_lsap(const double* cost, int nr, int nc, int64_t* row, int64_t* col, int32_t* status) {
  Lds<TL> L(smem);
  DevParams dummy;
  Sim<TL> sim(*L.S, *reinterpret_cast<EnvCold<TL>*>(L.S) /* never touched by the solver */, *L.X, dummy, nullptr);
  const int prob = blockIdx.x;
  const double* c = cost + (size_t)prob * nr * nc;
  const bool tr = nc < nr;
  const int Rr = tr ? nc : nr, Cc = tr ? nr : nc;
  for (int p = threadIdx.x; p < nr * nc; p += WG) {
    int i = p / nc, j = p - i * nc;
    L.X->cost[tr ? (j * Cc + i) : (i * Cc + j)] = c[p];
  }
  if (threadIdx.x == 0) L.S->error = 0;
  lds_sync();
  if constexpr (REG) sim.lsap_reg(Rr, Cc); else sim.lsap(Rr, Cc);
  lsap_probe_out(L, blockIdx.x, nr, nc, row, col, status);
}

// Stand-alone LSAP on an ENV tile (Tile16 / Tile24 / Tile64): Sim<TL> over Lds<TL> for the tile type the env kernels are built from — the
// same CostCol layout, row count and scratch array sizes — along the route Sim::allocate takes: cost columns in registers + lsap_reg_solve
// while the columns fit the wave, the on-the-fly lsap(nr, nc, cost_at) beyond that (Tile64).  These tiles hold no A x T cost tile in LDS, so
// each cost element is read from the global input (transposed index when nc < nr).  A kernel of its own: the copies of the solver inlined
// into k_rollout / k_allocate are checked by the simulation-against-oracle tests, not by this probe.
template <class TL>
__global__ __launch_bounds__(WG) void k_lsap_tile(const double* cost, int nr, int nc, int64_t* row, int64_t* col, int32_t* status) {
  Lds<TL> L(smem);
  DevParams dummy;
  Sim<TL> sim(*L.S, *reinterpret_cast<EnvCold<TL>*>(L.S) /* never touched by the solver */, *L.X, dummy, nullptr);
  const int prob = blockIdx.x;
  const double* c = cost + (size_t)prob * nr * nc;
  const bool tr = nc < nr;
  const int Rr = tr ? nc : nr, Cc = tr ? nr : nc;
  auto cost_at = [c, nc, tr](int i, int j) -> double { return tr ? c[j * nc + i] : c[i * nc + j]; };  // element (i, j) of scipy's (possibly transposed) matrix
  if (threadIdx.x == 0) L.S->error = 0;
  lds_sync();
  const bool reg_cols = TL::REGC && (TL::T <= WG || Cc <= WG);  // (Sim::allocate's condition)
  if (reg_cols) {
    const int lane = sim.lane;
    typename Sim<TL>::CostCol cc;
    sim.build_cols(cc, Rr, [&](int i) -> double { return lane < Cc ? cost_at(i, lane) : 0.0; });
    sim.lsap_reg_solve(Rr, Cc, [&](int i) -> double { return cc.get(i); });
  } else if constexpr (TL::OTFC) {
    sim.lsap(Rr, Cc, cost_at);
  }
  lsap_probe_out(L, blockIdx.x, nr, nc, row, col, status);
}

__global__ void k_domain_math(const double* x, const double* y, int n, double* out_sqrt, double* out_div, double* out_div2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out_sqrt[i] = fsqrt(x[i]);
  out_div[i] = fdiv(x[i], y[i]);
  const double r = frcp_nr(y[i]);
  out_div2[i] = fdiv_r(-x[i], y[i], r);
}

__global__ void k_libm_log(const double* x, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = libm_log(x[i]);
}

__global__ void k_libm_atan2(const double* y, const double* x, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = libm_atan2(y[i], x[i]);
}

__global__ void k_avoid(const double* pos, const double* mov, int n, const double* obst, int n_obs, double* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // same arithmetic as Sim::avoid_obstacles (core_sim/src/sim_core.rs:25-59)
  double px = pos[2 * i], py = pos[2 * i + 1], mx = mov[2 * i], my = mov[2 * i + 1];
  double ax = 0.0, ay = 0.0;
  const double PI = 3.14159265358979323846;
  for (int o = 0; o < n_obs; o++) {
    double dx = obst[3 * o] - px, dy = obst[3 * o + 1] - py;
    double d_zone = sqrt(dx * dx + dy * dy) - obst[3 * o + 2];
    if (d_zone < 40.0) {
      double nx = dx / d_zone, ny = dy / d_zone;
      double force = libm_log(fmax(1.05, d_zone));
      force = 0.5 / (1.0 - force);
      double ang = libm_atan2(my, mx) - libm_atan2(dy, dx);
      ang = fmod(ang + PI, 2.0 * PI) - PI;
      double rx, ry;
      if (ang > 0.0) { rx = ny; ry = -nx; } else { rx = -ny; ry = nx; }
      ax += rx * force;
      ay += ry * force;
    }
  }
  out[2 * i] = ax;
  out[2 * i + 1] = ay;
}

// ====================================================================================================
// Host side
// ====================================================================================================
}  // namespace

#include "abi/handle.inc"
#include "abi/sim.inc"
#include "abi/state.inc"
#include "abi/comm.inc"
#include "abi/probes.inc"
