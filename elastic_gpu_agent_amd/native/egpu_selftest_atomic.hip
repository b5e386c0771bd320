// Atomic sweep of the GPU self-test (part of libegpu_kernels.so): the
// read-modify-write atomics that split-K epilogues, MoE combines, histograms
// and tile counters run, in the two places that execute them: the atomic ALUs
// of the LDS and the atomic units behind the vector memory path.
//
//   atomic_selftest_kernel  256 threads = 4 waves per workgroup. Contention is
//                           the thing under test, so the unit of determinism is
//                           the workgroup: group = workgroup % 4, and the host
//                           replays four groups of 256 lanes whatever the grid.
//                           Per kind and round: plain stores initialise the
//                           arena, barrier, every lane issues its slots' atomics
//                           fully unrolled, barrier, every wave reads the whole
//                           arena back and folds it with what its own lanes got
//                           returned, barrier. One record {cu_id, sig[NKINDS]}
//                           per wave, pattern = 4 * group + wave.
//   atomic_cells_kernel     one workgroup, one kind, one round: the initial
//                           cells, every lane's returned words per slot and the
//                           final cells, so a test can name the wrong cell.
//
// Three arenas of 4 KiB, all generator-addressed (selftest_atomic_ref.h): the
// workgroup's dynamic LDS, the workgroup's slice of one global buffer, and one
// grid-shared slice that every lane of every workgroup adds into (g_grid; the
// host compares it with a closed form after the kernel). No address depends on
// a value read back and no loop on data: no spin, no retry, no lock. A lane
// that sits a slot out is masked by the generator. Global atomics are
// agent-scope; global cells are read back with agent-scope atomic loads after
// an agent-scope fence, because a plain load may be served from a line the
// CU's vector L1 kept from an earlier round. Vector atomics only, through the
// compiler builtins; each becomes one instruction (docs/HEALTH.md).
// inject_kind corrupts a signature, or for g_grid adds one unit to grid cell 0.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#define EGPU_ST_FN __host__ __device__ inline
#include "selftest_atomic_ref.h"

// shared with egpu_kernels.hip (egpu_last_error lives there)
extern __attribute__((visibility("hidden"))) char g_err[512];

#define EGPU_CHECK(expr)                                   \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) {                                \
      snprintf(g_err, sizeof(g_err), "%s: %s", #expr,      \
               hipGetErrorString(_e));                     \
      return (int)_e;                                      \
    }                                                      \
  } while (0)

#define EGPU_BAD_ARG(...)                        \
  do {                                           \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__); \
    return -1;                                   \
  } while (0)

#define EGPU_ATOMICTEST_VERSION 1
#define EGPU_ATOMICTEST_MAX_BLOCKS 65536
#define AT_RECORD_WORDS (1 + EGPU_AT_NKINDS)
#define AT_INJECT_NONE (-1)
#define AT_ARENA_BYTES (EGPU_AT_WORDS * sizeof(uint32_t))

extern "C" {
struct egpu_atomictest_params {
  int32_t blocks;
  int32_t rounds;
  uint32_t seed;
  int32_t inject_kind;   // -1 = none, else a kind index
  int32_t inject_block;  // workgroup whose data of that kind is corrupted
};

struct egpu_atomictest_report {
  uint32_t version;
  uint32_t waves_run;
  uint32_t cus_seen;
  uint32_t bad_waves;
  uint32_t bad_kinds;  // bit (1 << kind)
  uint32_t n_bad_cus;
  uint32_t bad_cus[64];  // physical ids (census encoding), deduplicated
  float kernel_ms;
  uint32_t grid_bad_cells;  // words of the grid slice that differ from the closed form
};
}

// ---------------------------------------------------------------- device side

namespace at = egpu_at;

using at_h2 = __attribute__((ext_vector_type(2))) _Float16;
using at_s2 = __attribute__((ext_vector_type(2))) short;
#define AT_AS(n) __attribute__((address_space(n)))

__device__ inline uint32_t at_wave_sum(uint32_t v) {
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// body(integral_constant<int, 0>) ... body(integral_constant<int, N - 1>)
template <int... I, typename F>
__device__ inline void at_each(std::integer_sequence<int, I...>, F&& body) {
  (body(std::integral_constant<int, I>{}), ...);
}

// One atomic of opcode OP on the cell at `word` of the arena. LDS: the arena
// is the workgroup's LDS and the scope the workgroup; else global memory and
// agent scope. Returns what a returning op returned.
template <int OP, bool LDS>
__device__ inline uint64_t at_issue(uint32_t* arena, int word, uint64_t a, uint64_t b) {
  constexpr int SC = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  uint32_t* p32 = arena + word;
  uint64_t* p64 = (uint64_t*)p32;
  const uint32_t a32 = (uint32_t)a;
  if constexpr (OP == at::OP_ADD32) {
    __hip_atomic_fetch_add(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_ADD64) {
    __hip_atomic_fetch_add(p64, a, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_AND) {
    __hip_atomic_fetch_and(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_OR) {
    __hip_atomic_fetch_or(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_XOR) {
    __hip_atomic_fetch_xor(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_MINI) {
    __hip_atomic_fetch_min((int*)p32, (int)a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_MAXI) {
    __hip_atomic_fetch_max((int*)p32, (int)a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_MINU) {
    __hip_atomic_fetch_min(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_MAXU) {
    __hip_atomic_fetch_max(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_FADD32) {
    __hip_atomic_fetch_add((float*)p32, __uint_as_float(a32), __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_FADD64) {
    __hip_atomic_fetch_add((double*)p64, __longlong_as_double((long long)a), __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_FMIN64) {
    __hip_atomic_fetch_min((double*)p64, __longlong_as_double((long long)a), __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_FMAX64) {
    __hip_atomic_fetch_max((double*)p64, __longlong_as_double((long long)a), __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_PKF16) {
    const at_h2 v = __builtin_bit_cast(at_h2, a32);
    if constexpr (LDS)
      __builtin_amdgcn_ds_atomic_fadd_v2f16((AT_AS(3) at_h2*)p32, v);
    else
      __builtin_amdgcn_global_atomic_fadd_v2f16((AT_AS(1) at_h2*)p32, v);
  } else if constexpr (OP == at::OP_PKBF16) {
    const at_s2 v = __builtin_bit_cast(at_s2, a32);
    if constexpr (LDS)
      __builtin_amdgcn_ds_atomic_fadd_v2bf16((AT_AS(3) at_s2*)p32, v);
    else
      __builtin_amdgcn_global_atomic_fadd_v2bf16((AT_AS(1) at_s2*)p32, v);
  } else if constexpr (OP == at::OP_ADDR32) {
    return __hip_atomic_fetch_add(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_ADDR64) {
    return __hip_atomic_fetch_add(p64, a, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_INC) {
    if constexpr (LDS) return __builtin_amdgcn_atomic_inc32(p32, a32, __ATOMIC_RELAXED, "workgroup");
    else return __builtin_amdgcn_atomic_inc32(p32, a32, __ATOMIC_RELAXED, "agent");
  } else if constexpr (OP == at::OP_DEC) {
    if constexpr (LDS) return __builtin_amdgcn_atomic_dec32(p32, a32, __ATOMIC_RELAXED, "workgroup");
    else return __builtin_amdgcn_atomic_dec32(p32, a32, __ATOMIC_RELAXED, "agent");
  } else if constexpr (OP == at::OP_SWAP) {
    return __hip_atomic_exchange(p32, a32, __ATOMIC_RELAXED, SC);
  } else if constexpr (OP == at::OP_CAS32 || OP == at::OP_CLAIM) {
    uint32_t expect = (uint32_t)b;  // left holding the value before, equal or not
    __hip_atomic_compare_exchange_strong(p32, &expect, a32, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SC);
    return expect;
  } else if constexpr (OP == at::OP_CAS64) {
    uint64_t expect = b;
    __hip_atomic_compare_exchange_strong(p64, &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SC);
    return expect;
  }
  return 0;
}

// Orders the phases of a round. Global: everything issued so far has reached
// the agent's level before the barrier, nothing after it is served early.
template <bool LDS> __device__ inline void at_phase() {
  if constexpr (!LDS) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  __syncthreads();
  if constexpr (!LDS) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
}

template <bool LDS> __device__ inline uint32_t at_read(uint32_t* arena, int word) {
  if constexpr (LDS) return arena[word];
  else return __hip_atomic_load(arena + word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int KIND> __device__ inline void at_init(uint32_t* arena, uint32_t seed, int group, int rd, int tid) {
#pragma unroll
  for (int i = 0; i < EGPU_AT_WORDS / EGPU_AT_LANES; ++i)
    arena[tid + EGPU_AT_LANES * i] = at::init_word(KIND, seed, group, rd, tid + EGPU_AT_LANES * i);
}

// The lane's atomics of one round, one per slot; ops and returned words out.
template <int KIND>
__device__ inline void at_atomics(uint32_t* arena, uint32_t seed, int group, int rd, int tid,
                                  at::op_t ops[EGPU_AT_NSLOT], uint64_t ret[EGPU_AT_NSLOT]) {
  at_each(std::make_integer_sequence<int, EGPU_AT_NSLOT>{}, [&](auto s_c) {
    constexpr int s = decltype(s_c)::value;
    constexpr int OP = at::slot_of(KIND, s).op;
    ret[s] = 0;
    if constexpr (OP != at::OP_NONE) {
      ops[s] = at::gen_op(KIND, s, seed, group, rd, tid);
      if (ops[s].op != at::OP_NONE) ret[s] = at_issue<OP, at::is_lds(KIND)>(arena, ops[s].cell, ops[s].a, ops[s].b);
    } else {
      ops[s] = at::op_t{at::OP_NONE, EGPU_AT_SLOT_WORDS * s, 0, 0, false};
    }
  });
}

// One round of one kind on the workgroup's arena; the wave's round sum.
template <int KIND>
__device__ inline uint32_t at_round(uint32_t* arena, uint32_t seed, int group, int rd, int tid) {
  constexpr bool LDS = at::is_lds(KIND);
  const int lane = tid & 63;
  at::op_t ops[EGPU_AT_NSLOT];
  uint64_t ret[EGPU_AT_NSLOT];
  at_init<KIND>(arena, seed, group, rd, tid);
  at_phase<LDS>();
  at_atomics<KIND>(arena, seed, group, rd, tid, ops, ret);
  at_phase<LDS>();
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < EGPU_AT_WORDS / 64; ++i)
    s += at::final_term(KIND, lane + 64 * i, at_read<LDS>(arena, lane + 64 * i));
#pragma unroll
  for (int k = 0; k < EGPU_AT_NSLOT; ++k)
    if (at::returns(at::slot_of(KIND, k).op))
      s += at::lane_term(ops[k], tid, ret[k], at_read<LDS>(arena, ops[k].cell));
  at_phase<LDS>();  // nobody re-initialises a cell another wave still reads
  return at_wave_sum(s);
}

template <int KIND>
__device__ inline uint32_t at_sig(uint32_t* arena, uint32_t seed, int group, int rounds, int tid) {
  uint32_t sig = 0;
  for (int rd = 0; rd < rounds; ++rd) sig = at::round_step(sig, at_round<KIND>(arena, seed, group, rd, tid));
  return sig;
}

// global: blocks slices of 4 KiB, then the grid slice.
__global__ void __launch_bounds__(256)
atomic_selftest_kernel(uint32_t* __restrict__ out, uint32_t* global, int rounds, uint32_t seed,
                       int inject_kind, int inject_block) {
  extern __shared__ __attribute__((aligned(16))) uint32_t at_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int group = blockIdx.x % EGPU_AT_GROUPS;
  uint32_t* mine = global + (size_t)blockIdx.x * EGPU_AT_WORDS;
  uint32_t* grid = global + (size_t)gridDim.x * EGPU_AT_WORDS;

  uint32_t hwid, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));

  uint32_t sig[EGPU_AT_NKINDS];
  sig[at::K_L_ADD] = at_sig<at::K_L_ADD>(at_lds, seed, group, rounds, tid);
  sig[at::K_L_LOGIC] = at_sig<at::K_L_LOGIC>(at_lds, seed, group, rounds, tid);
  sig[at::K_L_RTN] = at_sig<at::K_L_RTN>(at_lds, seed, group, rounds, tid);
  sig[at::K_L_CAS] = at_sig<at::K_L_CAS>(at_lds, seed, group, rounds, tid);
  sig[at::K_L_FADD] = at_sig<at::K_L_FADD>(at_lds, seed, group, rounds, tid);
  sig[at::K_G_ADD] = at_sig<at::K_G_ADD>(mine, seed, group, rounds, tid);
  sig[at::K_G_LOGIC] = at_sig<at::K_G_LOGIC>(mine, seed, group, rounds, tid);
  sig[at::K_G_RTN] = at_sig<at::K_G_RTN>(mine, seed, group, rounds, tid);
  sig[at::K_G_CAS] = at_sig<at::K_G_CAS>(mine, seed, group, rounds, tid);
  sig[at::K_G_FADD] = at_sig<at::K_G_FADD>(mine, seed, group, rounds, tid);
  // g_grid: no initialisation, no read-back, no signature
  sig[at::K_G_GRID] = 0;
  for (int rd = 0; rd < rounds; ++rd) {
    at::op_t ops[EGPU_AT_NSLOT];
    uint64_t ret[EGPU_AT_NSLOT];
    at_atomics<at::K_G_GRID>(grid, seed, group, rd, tid, ops, ret);
  }
  if (inject_kind == at::K_G_GRID && (int)blockIdx.x == inject_block && tid == 0)
    __hip_atomic_fetch_add(grid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  if (lane == 0) {
    uint32_t* rec = out + (size_t)(blockIdx.x * 4 + wave) * AT_RECORD_WORDS;
    // same encoding as the census: (xcc << 16) | {SE, SH, CU} bits of HW_ID
    rec[0] = (xcc << 16) | ((hwid >> 8) & 0x7F);
#pragma unroll
    for (int k = 0; k < EGPU_AT_NKINDS; ++k)
      rec[1 + k] = sig[k] ^ (((int)blockIdx.x == inject_block && k == inject_kind &&
                              k != at::K_G_GRID) ? 1u : 0u);
  }
}

// Launched with one workgroup of 256 threads and 4 KiB of dynamic LDS. global:
// one arena, zero for g_grid. init, fin: 1024 words; ret: 256 x NSLOT x 2.
template <int KIND>
__global__ void __launch_bounds__(256)
atomic_cells_kernel(int group, uint32_t seed, int round, uint32_t* global, uint32_t* __restrict__ init,
                    uint32_t* __restrict__ ret_out, uint32_t* __restrict__ fin) {
  extern __shared__ __attribute__((aligned(16))) uint32_t at_lds[];
  constexpr bool LDS = at::is_lds(KIND);
  uint32_t* arena = global;
  if constexpr (LDS) arena = at_lds;
  const int tid = threadIdx.x;
  at::op_t ops[EGPU_AT_NSLOT];
  uint64_t ret[EGPU_AT_NSLOT];
  if constexpr (KIND != at::K_G_GRID) at_init<KIND>(arena, seed, group, round, tid);
  at_phase<LDS>();
#pragma unroll
  for (int i = 0; i < EGPU_AT_WORDS / EGPU_AT_LANES; ++i)
    init[tid + EGPU_AT_LANES * i] = at_read<LDS>(arena, tid + EGPU_AT_LANES * i);
  at_phase<LDS>();
  at_atomics<KIND>(arena, seed, group, round, tid, ops, ret);
  at_phase<LDS>();
#pragma unroll
  for (int s = 0; s < EGPU_AT_NSLOT; ++s) {
    ret_out[2 * (EGPU_AT_NSLOT * tid + s)] = (uint32_t)ret[s];
    ret_out[2 * (EGPU_AT_NSLOT * tid + s) + 1] = (uint32_t)(ret[s] >> 32);
  }
#pragma unroll
  for (int i = 0; i < EGPU_AT_WORDS / EGPU_AT_LANES; ++i)
    fin[tid + EGPU_AT_LANES * i] = at_read<LDS>(arena, tid + EGPU_AT_LANES * i);
}

// ---------------------------------------------------------------- host side

namespace {

struct AtResources {
  void* dev = nullptr;     // records, or the cells kernel's outputs
  void* arenas = nullptr;  // the workgroups' slices and the grid slice
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~AtResources() {
    if (dev) (void)hipFree(dev);
    if (arenas) (void)hipFree(arenas);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int at_validate(const egpu_atomictest_params* p) {
  if (p == nullptr) EGPU_BAD_ARG("atomictest: params is null");
  if (p->blocks <= 0 || p->blocks > EGPU_ATOMICTEST_MAX_BLOCKS)
    EGPU_BAD_ARG("atomictest: blocks %d outside [1, %d]", p->blocks, EGPU_ATOMICTEST_MAX_BLOCKS);
  if (!at::rounds_ok(p->rounds))
    EGPU_BAD_ARG("atomictest: rounds %d outside [1, %d]", p->rounds, EGPU_AT_MAX_ROUNDS);
  if (!at::grid_work_ok(p->blocks, p->rounds))
    EGPU_BAD_ARG("atomictest: blocks x rounds = %lld is over %d, where a g_grid f64 cell stops being exact",
                 (long long)p->blocks * p->rounds, EGPU_AT_GRID_MAX_WORK);
  if (p->inject_kind != AT_INJECT_NONE) {
    if (!at::kind_ok(p->inject_kind)) EGPU_BAD_ARG("atomictest: unknown inject_kind %d", p->inject_kind);
    if (p->inject_block < 0 || p->inject_block >= p->blocks)
      EGPU_BAD_ARG("atomictest: inject_block %d is not a workgroup of a %d-block grid",
                   p->inject_block, p->blocks);
  }
  return 0;
}

int at_check_point(const char* who, int kind, int group, int round) {
  if (!at::kind_ok(kind)) EGPU_BAD_ARG("%s: unknown kind %d", who, kind);
  if (group < 0 || group >= EGPU_AT_GROUPS)
    EGPU_BAD_ARG("%s: group %d outside [0, %d)", who, group, EGPU_AT_GROUPS);
  if (round < 0 || round >= EGPU_AT_MAX_ROUNDS)
    EGPU_BAD_ARG("%s: round %d outside [0, %d)", who, round, EGPU_AT_MAX_ROUNDS);
  return 0;
}

// Runs atomic_selftest_kernel; recs = 4*blocks records of AT_RECORD_WORDS
// words, grid = the grid slice after the kernel.
int at_run(const egpu_atomictest_params* p, AtResources& res, std::vector<uint32_t>& recs,
           std::vector<uint32_t>& grid, float* ms) {
  const size_t words = (size_t)p->blocks * 4 * AT_RECORD_WORDS;
  const size_t arena_bytes = ((size_t)p->blocks + 1) * AT_ARENA_BYTES;
  EGPU_CHECK(hipMalloc(&res.dev, words * sizeof(uint32_t)));
  EGPU_CHECK(hipMalloc(&res.arenas, arena_bytes));
  EGPU_CHECK(hipMemset(res.dev, 0xFF, words * sizeof(uint32_t)));
  EGPU_CHECK(hipMemset(res.arenas, 0, arena_bytes));
  EGPU_CHECK(hipEventCreate(&res.ev[0]));
  EGPU_CHECK(hipEventCreate(&res.ev[1]));
  EGPU_CHECK(hipEventRecord(res.ev[0], 0));
  const bool inject = p->inject_kind != AT_INJECT_NONE;
  hipLaunchKernelGGL(atomic_selftest_kernel, dim3(p->blocks), dim3(256), AT_ARENA_BYTES, 0,
                     (uint32_t*)res.dev, (uint32_t*)res.arenas, p->rounds, p->seed,
                     inject ? p->inject_kind : -1, inject ? p->inject_block : -1);
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipEventRecord(res.ev[1], 0));
  EGPU_CHECK(hipEventSynchronize(res.ev[1]));
  EGPU_CHECK(hipEventElapsedTime(ms, res.ev[0], res.ev[1]));
  recs.resize(words);
  grid.resize(EGPU_AT_WORDS);
  EGPU_CHECK(hipMemcpy(recs.data(), res.dev, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(grid.data(), (uint32_t*)res.arenas + (size_t)p->blocks * EGPU_AT_WORDS,
                       AT_ARENA_BYTES, hipMemcpyDeviceToHost));
  return 0;
}

void at_add_unique(uint32_t* ids, uint32_t* n, uint32_t cap, uint32_t id) {
  for (uint32_t j = 0; j < *n; ++j)
    if (ids[j] == id) return;
  if (*n < cap) ids[(*n)++] = id;
}

template <int KIND>
void at_launch_cells(int group, uint32_t seed, int round, uint32_t* global, uint32_t* init, uint32_t* ret,
                     uint32_t* fin) {
  hipLaunchKernelGGL(atomic_cells_kernel<KIND>, dim3(1), dim3(256), AT_ARENA_BYTES, 0, group, seed, round,
                     global, init, ret, fin);
}

}  // namespace

// Host reference: out[NKINDS * (4 * group + wave) + kind]. No HIP call.
extern "C" int egpu_atomictest_expected(uint32_t seed, int rounds, uint32_t* out) {
  if (out == nullptr) EGPU_BAD_ARG("atomictest_expected: out is null");
  if (at::expected_all(seed, rounds, (uint32_t(*)[EGPU_AT_NKINDS])out) != 0)
    EGPU_BAD_ARG("atomictest_expected: rounds %d outside [1, %d]", rounds, EGPU_AT_MAX_ROUNDS);
  return 0;
}

// Host only, no HIP call: what the generator emits for one workgroup, kind and
// round and what the reference makes of it in lane order. ops: 256 x NSLOT x
// EGPU_AT_OP_WORDS words; init, fin: 1024; ret: 256 x NSLOT x 2.
extern "C" int egpu_atomictest_ops(int kind, int group, uint32_t seed, int round, uint32_t* ops,
                                   uint32_t* init, uint32_t* ret, uint32_t* fin) {
  if (!ops || !init || !ret || !fin) EGPU_BAD_ARG("atomictest_ops: null output");
  if (int rc = at_check_point("atomictest_ops", kind, group, round)) return rc;
  std::vector<at::workgroup> wg(1);
  at::replay(kind, seed, group, round, wg.data());
  for (int w = 0; w < EGPU_AT_WORDS; ++w) init[w] = wg[0].init[w], fin[w] = wg[0].fin[w];
  for (int tid = 0; tid < EGPU_AT_LANES; ++tid)
    for (int s = 0; s < EGPU_AT_NSLOT; ++s) {
      const at::op_t& o = wg[0].ops[tid][s];
      uint32_t* w = ops + EGPU_AT_OP_WORDS * (EGPU_AT_NSLOT * tid + s);
      w[0] = (uint32_t)o.op, w[1] = (uint32_t)o.cell;
      w[2] = (uint32_t)o.a, w[3] = (uint32_t)(o.a >> 32), w[4] = (uint32_t)o.b, w[5] = (uint32_t)(o.b >> 32);
      ret[2 * (EGPU_AT_NSLOT * tid + s)] = (uint32_t)wg[0].ret[tid][s];
      ret[2 * (EGPU_AT_NSLOT * tid + s) + 1] = (uint32_t)(wg[0].ret[tid][s] >> 32);
    }
  return 0;
}

// Arguments are validated before the first HIP call: a bad argument is an
// error code (-1) on a machine with no GPU too.
extern "C" int egpu_atomictest(int device, const egpu_atomictest_params* p, egpu_atomictest_report* rep) {
  if (rep == nullptr) EGPU_BAD_ARG("atomictest: report is null");
  if (device < 0) EGPU_BAD_ARG("atomictest: device %d is negative", device);
  if (int rc = at_validate(p)) return rc;
  *rep = egpu_atomictest_report{};
  rep->version = EGPU_ATOMICTEST_VERSION;

  std::vector<uint32_t> expected(EGPU_AT_PATTERNS * EGPU_AT_NKINDS), grid_want(EGPU_AT_WORDS);
  at::expected_all(p->seed, p->rounds, (uint32_t(*)[EGPU_AT_NKINDS])expected.data());
  at::grid_expected(p->seed, p->blocks, p->rounds, grid_want.data());

  EGPU_CHECK(hipSetDevice(device));
  AtResources res;
  std::vector<uint32_t> recs, grid;
  if (int rc = at_run(p, res, recs, grid, &rep->kernel_ms)) return rc;

  std::vector<uint32_t> cus(1024);
  uint32_t n_cus = 0;
  for (size_t wv = 0; wv < (size_t)p->blocks * 4; ++wv) {
    const uint32_t* r = &recs[wv * AT_RECORD_WORDS];
    if (r[0] == 0xFFFFFFFFu) continue;  // record never written
    rep->waves_run++;
    at_add_unique(cus.data(), &n_cus, (uint32_t)cus.size(), r[0]);
    const uint32_t* e = &expected[(wv % EGPU_AT_PATTERNS) * EGPU_AT_NKINDS];
    uint32_t kinds = 0;
    for (int k = 0; k < EGPU_AT_NKINDS; ++k)
      if (r[1 + k] != e[k]) kinds |= 1u << k;
    if (kinds) {
      rep->bad_waves++;
      rep->bad_kinds |= kinds;
      at_add_unique(rep->bad_cus, &rep->n_bad_cus, 64, r[0]);
    }
  }
  rep->cus_seen = n_cus;
  // the grid slice belongs to no wave and no CU
  for (int w = 0; w < EGPU_AT_WORDS; ++w)
    if (grid[w] != grid_want[w]) rep->grid_bad_cells++;
  if (rep->grid_bad_cells) rep->bad_kinds |= 1u << at::K_G_GRID;
  return 0;
}

// The raw records of one run, AT_RECORD_WORDS words per wave:
// {cu_id, sig[NKINDS]}. records holds 4*blocks of them.
extern "C" int egpu_atomictest_records(int device, const egpu_atomictest_params* p, uint32_t* records,
                                       int max_records) {
  if (records == nullptr) EGPU_BAD_ARG("atomictest_records: records is null");
  if (device < 0) EGPU_BAD_ARG("atomictest_records: device %d is negative", device);
  if (int rc = at_validate(p)) return rc;
  if (max_records < p->blocks * 4)
    EGPU_BAD_ARG("atomictest_records: room for %d records, need %d", max_records, p->blocks * 4);
  EGPU_CHECK(hipSetDevice(device));
  AtResources res;
  std::vector<uint32_t> recs, grid;
  float ms = 0.f;
  if (int rc = at_run(p, res, recs, grid, &ms)) return rc;
  for (size_t i = 0; i < recs.size(); ++i) records[i] = recs[i];
  return 0;
}

// One workgroup, one kind, one round on the GPU. init_out, fin_out: the 1024
// words of the arena before and after the atomics; ret_out: 256 x NSLOT x 2
// words, what each lane's atomic of each slot returned (0 where none did).
extern "C" int egpu_atomictest_cells(int device, int kind, int group, uint32_t seed, int round,
                                     uint32_t* init_out, uint32_t* ret_out, uint32_t* fin_out) {
  if (!init_out || !ret_out || !fin_out) EGPU_BAD_ARG("atomictest_cells: null output");
  if (device < 0) EGPU_BAD_ARG("atomictest_cells: device %d is negative", device);
  if (int rc = at_check_point("atomictest_cells", kind, group, round)) return rc;
  EGPU_CHECK(hipSetDevice(device));
  AtResources res;
  constexpr size_t ret_words = 2 * EGPU_AT_NSLOT * EGPU_AT_LANES;
  const size_t bytes = (2 * EGPU_AT_WORDS + ret_words) * sizeof(uint32_t);
  EGPU_CHECK(hipMalloc(&res.dev, bytes));
  EGPU_CHECK(hipMalloc(&res.arenas, AT_ARENA_BYTES));
  EGPU_CHECK(hipMemset(res.dev, 0, bytes));
  EGPU_CHECK(hipMemset(res.arenas, 0, AT_ARENA_BYTES));
  uint32_t* init = (uint32_t*)res.dev;
  uint32_t* fin = init + EGPU_AT_WORDS;
  uint32_t* ret = fin + EGPU_AT_WORDS;
  uint32_t* g = (uint32_t*)res.arenas;
  switch (kind) {
    case at::K_L_ADD: at_launch_cells<at::K_L_ADD>(group, seed, round, g, init, ret, fin); break;
    case at::K_L_LOGIC: at_launch_cells<at::K_L_LOGIC>(group, seed, round, g, init, ret, fin); break;
    case at::K_L_RTN: at_launch_cells<at::K_L_RTN>(group, seed, round, g, init, ret, fin); break;
    case at::K_L_CAS: at_launch_cells<at::K_L_CAS>(group, seed, round, g, init, ret, fin); break;
    case at::K_L_FADD: at_launch_cells<at::K_L_FADD>(group, seed, round, g, init, ret, fin); break;
    case at::K_G_ADD: at_launch_cells<at::K_G_ADD>(group, seed, round, g, init, ret, fin); break;
    case at::K_G_LOGIC: at_launch_cells<at::K_G_LOGIC>(group, seed, round, g, init, ret, fin); break;
    case at::K_G_RTN: at_launch_cells<at::K_G_RTN>(group, seed, round, g, init, ret, fin); break;
    case at::K_G_CAS: at_launch_cells<at::K_G_CAS>(group, seed, round, g, init, ret, fin); break;
    case at::K_G_FADD: at_launch_cells<at::K_G_FADD>(group, seed, round, g, init, ret, fin); break;
    default: at_launch_cells<at::K_G_GRID>(group, seed, round, g, init, ret, fin); break;
  }
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipDeviceSynchronize());
  EGPU_CHECK(hipMemcpy(init_out, init, AT_ARENA_BYTES, hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(fin_out, fin, AT_ARENA_BYTES, hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(ret_out, ret, ret_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}
