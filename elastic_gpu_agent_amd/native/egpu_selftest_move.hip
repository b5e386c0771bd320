// Move sweep of the GPU self-test (part of libegpu_kernels.so): the gfx950
// data-movement paths that feed the matrix instructions and that neither the
// LDS march (32-bit words) nor the memory check reaches.
//
//   move_selftest_kernel  256 threads = 4 waves per workgroup. LDS is four
//                         4 KiB slabs, one per wave. Per kind and round a wave
//                         fills ITS slab (or, for the direct-to-LDS kinds, has
//                         the hardware load it from the global source buffer),
//                         the workgroup meets at a barrier, and the wave reads
//                         the slab of wave (w + 1) & 3 through the instruction
//                         under test, four tiles of 64 lanes x 4 registers. What
//                         each lane received is folded with weights that differ
//                         per lane, tile and register. The lane kinds (bperm,
//                         swap, dpp) move the wave's own registers. One record
//                         {cu_id, sig[NKINDS]} per wave; inputs are a pure
//                         function of pattern = (blockIdx.x*4 + wave) % 16,
//                         seed and round.
//   move_tile_kernel      one wave, one kind, one round, tile 0: the raw
//                         registers every lane received and the source words, so
//                         a test can say which element went to the wrong lane.
//
// The device only executes the instructions; which lane must receive what is
// written down in selftest_move_ref.h and nowhere here. Every LDS address is
// slab base + a constant + lane * constant, every global address is inside
// the source buffer by g2l_offset's modulo; none depends on data. All DPP
// controls, swap flags and instruction offsets are compile-time constants.
// inject_kind corrupts a signature only, never an address.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#define EGPU_ST_FN __host__ __device__ inline
#include "selftest_move_ref.h"

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

#define EGPU_MOVETEST_VERSION 1
#define EGPU_MOVETEST_MAX_BLOCKS 65536
#define MOVE_RECORD_WORDS (1 + EGPU_MOVE_NKINDS)
#define MOVE_INJECT_NONE (-1)
#define MOVE_SLAB_BYTES (EGPU_MOVE_SLAB_WORDS * 4)
#define MOVE_TILE_BYTES (EGPU_MOVE_TILE_WORDS * 4)

extern "C" {
struct egpu_movetest_params {
  int32_t blocks;
  int32_t rounds;
  uint32_t seed;
  int32_t inject_kind;   // -1 = none, else a kind index
  int32_t inject_block;  // workgroup whose signature of that kind is corrupted
};

struct egpu_movetest_report {
  uint32_t version;
  uint32_t waves_run;
  uint32_t cus_seen;
  uint32_t bad_waves;
  uint32_t bad_kinds;  // bit (1 << kind)
  uint32_t n_bad_cus;
  uint32_t bad_cus[64];  // physical ids (census encoding), deduplicated
  float kernel_ms;
};
}

// ---------------------------------------------------------------- device side

namespace mv = egpu_mv;

#define MOVE_LDS __attribute__((address_space(3)))
#define MOVE_GLOBAL __attribute__((address_space(1)))
using mv_u4 = __attribute__((ext_vector_type(4))) uint32_t;
using mv_i2 = __attribute__((ext_vector_type(2))) int;
using mv_i3 = __attribute__((ext_vector_type(3))) int;
using mv_s4 = __attribute__((ext_vector_type(4))) short;

__device__ inline uint32_t move_wave_sum(uint32_t v) {
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// s_waitcnt vmcnt(0), the other counters left alone (gfx9 encoding)
__device__ inline void move_wait_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// The four words of 16-byte chunk `chunk` of tile TILE, as generated.
template <int KIND>
__device__ inline mv_u4 move_gen_chunk(uint32_t seed, int pattern, int round, int tile, int chunk) {
  mv_u4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    v[k] = mv::slab_word(seed, pattern, KIND, round,
                         (uint32_t)(tile * EGPU_MOVE_TILE_WORDS + 4 * chunk + k));
  return v;
}

// Fills the wave's own slab (LDS byte offset `slab`, wave-uniform) for one round.
template <int KIND>
__device__ inline void move_fill(uint32_t slab, const uint32_t* __restrict__ src, uint32_t seed,
                                 int pattern, int round, int lane) {
  if constexpr (mv::is_g2l(KIND)) {
    // The instruction offset advances the global and the LDS address alike; the
    // hardware adds lane * size to the wave-uniform LDS base in M0.
    MOVE_LDS uint32_t* dst = (MOVE_LDS uint32_t*)(uintptr_t)slab;
    const uint32_t* from = src + mv::g2l_offset(seed, pattern, KIND, round);
    if constexpr (KIND == mv::K_G2L16) {
      const MOVE_GLOBAL uint32_t* g = (const MOVE_GLOBAL uint32_t*)(uintptr_t)(from + 4 * lane);
      __builtin_amdgcn_global_load_lds(g, dst, 16, 0 * MOVE_TILE_BYTES, 0);
      __builtin_amdgcn_global_load_lds(g, dst, 16, 1 * MOVE_TILE_BYTES, 0);
      __builtin_amdgcn_global_load_lds(g, dst, 16, 2 * MOVE_TILE_BYTES, 0);
      __builtin_amdgcn_global_load_lds(g, dst, 16, 3 * MOVE_TILE_BYTES, 0);
    } else {
      const MOVE_GLOBAL uint32_t* g = (const MOVE_GLOBAL uint32_t*)(uintptr_t)(from + lane);
#define MOVE_G2L4(i) __builtin_amdgcn_global_load_lds(g, dst, 4, (i) * 256, 0)
      MOVE_G2L4(0); MOVE_G2L4(1); MOVE_G2L4(2); MOVE_G2L4(3);
      MOVE_G2L4(4); MOVE_G2L4(5); MOVE_G2L4(6); MOVE_G2L4(7);
      MOVE_G2L4(8); MOVE_G2L4(9); MOVE_G2L4(10); MOVE_G2L4(11);
      MOVE_G2L4(12); MOVE_G2L4(13); MOVE_G2L4(14); MOVE_G2L4(15);
#undef MOVE_G2L4
    }
    move_wait_vmem();
  } else {
    const int slot = KIND == mv::K_B128 ? mv::b128_swizzle(lane) : lane;
#pragma unroll
    for (int t = 0; t < EGPU_MOVE_TILES; ++t)
      *(MOVE_LDS mv_u4*)(uintptr_t)(slab + t * MOVE_TILE_BYTES + 16 * slot) =
          move_gen_chunk<KIND>(seed, pattern, round, t, lane);
  }
}

// Reads tile TILE of the slab at LDS byte offset `slab` through the instruction
// under test: the four registers the lane received (unused ones zero).
template <int KIND, int TILE>
__device__ inline mv_u4 move_read(uint32_t slab, int lane) {
  const uint32_t tile = slab + TILE * MOVE_TILE_BYTES;
  mv_u4 r = {0, 0, 0, 0};
  if constexpr (mv::is_g2l(KIND)) {
    r = *(MOVE_LDS mv_u4*)(uintptr_t)(tile + 16 * mv::g2l_read_slot(KIND, lane));
  } else if constexpr (KIND == mv::K_B128) {
    r = *(MOVE_LDS mv_u4*)(uintptr_t)(tile + 16 * lane);
  } else if constexpr (KIND == mv::K_TR6) {
    const mv_i3 v = __builtin_amdgcn_ds_read_tr6_b96_v3i32((MOVE_LDS mv_i3*)(uintptr_t)(tile + 16 * lane));
    r[0] = v[0], r[1] = v[1], r[2] = v[2];
  } else {
    mv_i2 lo, hi;
    if constexpr (KIND == mv::K_TR16) {
      lo = __builtin_bit_cast(mv_i2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                         (MOVE_LDS mv_s4*)(uintptr_t)(tile + 8 * lane)));
      hi = __builtin_bit_cast(mv_i2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                         (MOVE_LDS mv_s4*)(uintptr_t)(tile + 512 + 8 * lane)));
    } else if constexpr (KIND == mv::K_TR8) {
      lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((MOVE_LDS mv_i2*)(uintptr_t)(tile + 8 * lane));
      hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((MOVE_LDS mv_i2*)(uintptr_t)(tile + 512 + 8 * lane));
    } else {
      lo = __builtin_amdgcn_ds_read_tr4_b64_v2i32((MOVE_LDS mv_i2*)(uintptr_t)(tile + 8 * lane));
      hi = __builtin_amdgcn_ds_read_tr4_b64_v2i32((MOVE_LDS mv_i2*)(uintptr_t)(tile + 512 + 8 * lane));
    }
    r[0] = lo[0], r[1] = lo[1], r[2] = hi[0], r[3] = hi[1];
  }
  return r;
}

// The lane kinds: s[reg] is word reg * 64 + lane of the generated tile.
template <int KIND>
__device__ inline mv_u4 move_lanes(uint32_t seed, int pattern, int round, int tile, int lane) {
  int s[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
    s[reg] = (int)mv::slab_word(seed, pattern, KIND, round,
                                (uint32_t)(tile * EGPU_MOVE_TILE_WORDS + 64 * reg + lane));
  mv_u4 r;
  if constexpr (KIND == mv::K_BPERM) {
    const int to = 4 * mv::lane_perm(round, lane);  // byte address of a lane, always in [0, 252]
    r[0] = __builtin_amdgcn_ds_bpermute(to, s[0]);
    r[1] = __builtin_amdgcn_ds_bpermute(to, s[1]);
    r[2] = __builtin_amdgcn_ds_permute(to, s[2]);
    r[3] = __builtin_amdgcn_ds_permute(to, s[3]);
  } else if constexpr (KIND == mv::K_SWAP) {
    const auto a = __builtin_amdgcn_permlane16_swap(s[0], s[1], false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(s[2], s[3], false, false);
    r[0] = a[0], r[1] = a[1], r[2] = b[0], r[3] = b[1];
  } else {
    // old = the lane's own value: a lane without a source keeps it
    const int q = __builtin_amdgcn_update_dpp(s[0], s[0], 0x39, 0xF, 0xF, false);   // quad_perm:[1,2,3,0]
    r[0] = __builtin_amdgcn_update_dpp(q, q, 0x140, 0xF, 0xF, false);               // row_mirror
    const int o = __builtin_amdgcn_update_dpp(s[1], s[1], 0x123, 0xF, 0xF, false);  // row_ror:3
    r[1] = __builtin_amdgcn_update_dpp(o, o, 0x141, 0xF, 0xF, false);               // row_half_mirror
    r[2] = __builtin_amdgcn_update_dpp(s[2], s[2], 0x142, 0xF, 0xF, false);         // row_bcast:15
    r[3] = __builtin_amdgcn_update_dpp(s[3], s[3], 0x143, 0xF, 0xF, false);         // row_bcast:31
  }
  return r;
}

__device__ inline uint32_t move_fold(mv_u4 r, int lane, int tile) {
  uint32_t s = 0;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) s += r[reg] * mv::reg_weight(lane, tile, reg);
  return s;
}

// Signature of one kind. `own` and `next` are the LDS byte offsets of the
// wave's slab and of its neighbour's. Every wave of the workgroup runs the
// same number of rounds, so the barriers are met by all four.
template <int KIND>
__device__ inline uint32_t move_sig(uint32_t own, uint32_t next, const uint32_t* __restrict__ src,
                                    uint32_t seed, int pattern, int lane, int rounds) {
  uint32_t sig = 0;
  for (int rd = 0; rd < rounds; ++rd) {
    uint32_t s = 0;
    if constexpr (mv::is_lane_kind(KIND)) {
#pragma unroll
      for (int t = 0; t < EGPU_MOVE_TILES; ++t)
        s += move_fold(move_lanes<KIND>(seed, pattern, rd, t, lane), lane, t);
    } else {
      move_fill<KIND>(own, src, seed, pattern, rd, lane);
      __syncthreads();
      s += move_fold(move_read<KIND, 0>(next, lane), lane, 0);
      s += move_fold(move_read<KIND, 1>(next, lane), lane, 1);
      s += move_fold(move_read<KIND, 2>(next, lane), lane, 2);
      s += move_fold(move_read<KIND, 3>(next, lane), lane, 3);
      __syncthreads();  // the neighbour has read this wave's slab before it is refilled
    }
    sig = mv::round_step(sig, move_wave_sum(s));
  }
  return sig;
}

__global__ void __launch_bounds__(256)
move_selftest_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ src, int rounds,
                     uint32_t seed, int inject_kind, int inject_block) {
  extern __shared__ mv_u4 move_lds[];  // 4 slabs of MOVE_SLAB_BYTES
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pattern = (blockIdx.x * 4 + wave) % EGPU_MOVE_PATTERNS;
  const uint32_t base = (uint32_t)(uintptr_t)move_lds;
  const uint32_t own = base + wave * MOVE_SLAB_BYTES, next = base + ((wave + 1) & 3) * MOVE_SLAB_BYTES;

  uint32_t hwid, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));

  uint32_t sig[EGPU_MOVE_NKINDS];
  sig[mv::K_G2L16] = move_sig<mv::K_G2L16>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_G2L4] = move_sig<mv::K_G2L4>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_B128] = move_sig<mv::K_B128>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_TR16] = move_sig<mv::K_TR16>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_TR8] = move_sig<mv::K_TR8>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_TR6] = move_sig<mv::K_TR6>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_TR4] = move_sig<mv::K_TR4>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_BPERM] = move_sig<mv::K_BPERM>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_SWAP] = move_sig<mv::K_SWAP>(own, next, src, seed, pattern, lane, rounds);
  sig[mv::K_DPP] = move_sig<mv::K_DPP>(own, next, src, seed, pattern, lane, rounds);

  if (lane == 0) {
    uint32_t* rec = out + (size_t)(blockIdx.x * 4 + wave) * MOVE_RECORD_WORDS;
    // same encoding as the census: (xcc << 16) | {SE, SH, CU} bits of HW_ID
    rec[0] = (xcc << 16) | ((hwid >> 8) & 0x7F);
#pragma unroll
    for (int k = 0; k < EGPU_MOVE_NKINDS; ++k)
      rec[1 + k] = sig[k] ^ (((int)blockIdx.x == inject_block && k == inject_kind) ? 1u : 0u);
  }
}

// regs: 64 x 4 words; srcw: the 256 source words of tile 0 (for the LDS kinds
// read back from LDS with plain 32-bit reads, for the direct-to-LDS kinds read
// from the global buffer, for b128 and the lane kinds as generated).
template <int KIND>
__global__ void __launch_bounds__(64)
move_tile_kernel(const uint32_t* __restrict__ src, int pattern, uint32_t seed, int round,
                 uint32_t* __restrict__ regs, uint32_t* __restrict__ srcw) {
  extern __shared__ mv_u4 move_lds[];  // one slab
  const int lane = threadIdx.x & 63;
  const uint32_t slab = (uint32_t)(uintptr_t)move_lds;
  mv_u4 r;
  if constexpr (mv::is_lane_kind(KIND)) {
    r = move_lanes<KIND>(seed, pattern, round, 0, lane);
  } else {
    move_fill<KIND>(slab, src, seed, pattern, round, lane);
    __syncthreads();
    r = move_read<KIND, 0>(slab, lane);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    regs[4 * lane + k] = r[k];
    const int w = 64 * k + lane;
    if constexpr (mv::is_g2l(KIND))
      srcw[w] = src[mv::g2l_offset(seed, pattern, KIND, round) + w];
    else if constexpr (KIND == mv::K_B128 || mv::is_lane_kind(KIND))
      srcw[w] = mv::slab_word(seed, pattern, KIND, round, (uint32_t)w);
    else
      srcw[w] = ((const uint32_t*)move_lds)[w];
  }
}

__global__ void __launch_bounds__(256)
move_fill_kernel(uint32_t* __restrict__ src, uint32_t seed) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < EGPU_MOVE_SRC_WORDS) src[i] = mv::src_word(seed, i);
}

// ---------------------------------------------------------------- host side

namespace {

struct MoveResources {
  void* dev[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~MoveResources() {
    for (void* p : dev)
      if (p) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int move_validate(const egpu_movetest_params* p) {
  if (p == nullptr) EGPU_BAD_ARG("movetest: params is null");
  if (p->blocks <= 0 || p->blocks > EGPU_MOVETEST_MAX_BLOCKS)
    EGPU_BAD_ARG("movetest: blocks %d outside [1, %d]", p->blocks, EGPU_MOVETEST_MAX_BLOCKS);
  if (!mv::rounds_ok(p->rounds))
    EGPU_BAD_ARG("movetest: rounds %d outside [1, %d]", p->rounds, EGPU_MOVE_MAX_ROUNDS);
  if (p->inject_kind != MOVE_INJECT_NONE) {
    if (!mv::kind_ok(p->inject_kind)) EGPU_BAD_ARG("movetest: unknown inject_kind %d", p->inject_kind);
    if (p->inject_block < 0 || p->inject_block >= p->blocks)
      EGPU_BAD_ARG("movetest: inject_block %d is not a workgroup of a %d-block grid",
                   p->inject_block, p->blocks);
  }
  return 0;
}

// Allocates the global source of the direct-to-LDS kinds into res.dev[1] and
// fills it on the device.
int move_source(MoveResources& res, uint32_t seed) {
  EGPU_CHECK(hipMalloc(&res.dev[1], EGPU_MOVE_SRC_WORDS * sizeof(uint32_t)));
  hipLaunchKernelGGL(move_fill_kernel, dim3(EGPU_MOVE_SRC_WORDS / 256), dim3(256), 0, 0,
                     (uint32_t*)res.dev[1], seed);
  EGPU_CHECK(hipGetLastError());
  return 0;
}

// Runs move_selftest_kernel; recs = 4*blocks records of MOVE_RECORD_WORDS words.
int move_run(const egpu_movetest_params* p, MoveResources& res, std::vector<uint32_t>& recs,
             float* ms) {
  const size_t words = (size_t)p->blocks * 4 * MOVE_RECORD_WORDS;
  EGPU_CHECK(hipMalloc(&res.dev[0], words * sizeof(uint32_t)));
  EGPU_CHECK(hipMemset(res.dev[0], 0xFF, words * sizeof(uint32_t)));
  if (int rc = move_source(res, p->seed)) return rc;
  EGPU_CHECK(hipEventCreate(&res.ev[0]));
  EGPU_CHECK(hipEventCreate(&res.ev[1]));
  EGPU_CHECK(hipEventRecord(res.ev[0], 0));
  const bool inject = p->inject_kind != MOVE_INJECT_NONE;
  hipLaunchKernelGGL(move_selftest_kernel, dim3(p->blocks), dim3(256), 4 * MOVE_SLAB_BYTES, 0,
                     (uint32_t*)res.dev[0], (const uint32_t*)res.dev[1], p->rounds, p->seed,
                     inject ? p->inject_kind : -1, inject ? p->inject_block : -1);
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipEventRecord(res.ev[1], 0));
  EGPU_CHECK(hipEventSynchronize(res.ev[1]));
  EGPU_CHECK(hipEventElapsedTime(ms, res.ev[0], res.ev[1]));
  recs.resize(words);
  EGPU_CHECK(hipMemcpy(recs.data(), res.dev[0], words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

void move_add_unique(uint32_t* ids, uint32_t* n, uint32_t cap, uint32_t id) {
  for (uint32_t j = 0; j < *n; ++j)
    if (ids[j] == id) return;
  if (*n < cap) ids[(*n)++] = id;
}

template <int KIND>
void move_launch_tile(const uint32_t* src, int pattern, uint32_t seed, int round, uint32_t* regs,
                      uint32_t* srcw) {
  hipLaunchKernelGGL(move_tile_kernel<KIND>, dim3(1), dim3(64), MOVE_SLAB_BYTES, 0, src, pattern,
                     seed, round, regs, srcw);
}

}  // namespace

// Host reference: out[NKINDS * pattern + kind], 16 patterns. Touches no HIP
// API, so it runs on a machine without a GPU.
extern "C" int egpu_movetest_expected(uint32_t seed, int rounds, uint32_t* out) {
  if (out == nullptr) EGPU_BAD_ARG("movetest_expected: out is null");
  if (mv::expected_all(seed, rounds, out) != 0)
    EGPU_BAD_ARG("movetest_expected: rounds %d outside [1, %d]", rounds, EGPU_MOVE_MAX_ROUNDS);
  return 0;
}

// Host only. out[ELEMS * lane + j] = source element index of element j of that
// lane, ELEMS = geometry_of(kind).elems (bperm: the map of round 0). out needs
// room for 64 * EGPU_MOVE_MAX_ELEMS entries.
extern "C" int egpu_movetest_lane_map(int kind, int32_t* out) {
  if (out == nullptr) EGPU_BAD_ARG("movetest_lane_map: out is null");
  if (!mv::kind_ok(kind)) EGPU_BAD_ARG("movetest_lane_map: unknown kind %d", kind);
  const int elems = mv::geometry_of(kind).elems;
  for (int lane = 0; lane < 64; ++lane)
    for (int j = 0; j < elems; ++j) out[elems * lane + j] = mv::map_index(kind, 0, lane, j);
  return 0;
}

// Arguments are validated before the first HIP call: a bad argument is an
// error code (-1) on a machine with no GPU too.
extern "C" int egpu_movetest(int device, const egpu_movetest_params* p, egpu_movetest_report* rep) {
  if (rep == nullptr) EGPU_BAD_ARG("movetest: report is null");
  if (device < 0) EGPU_BAD_ARG("movetest: device %d is negative", device);
  if (int rc = move_validate(p)) return rc;
  *rep = egpu_movetest_report{};
  rep->version = EGPU_MOVETEST_VERSION;

  std::vector<uint32_t> expected(EGPU_MOVE_PATTERNS * EGPU_MOVE_NKINDS);
  mv::expected_all(p->seed, p->rounds, expected.data());

  EGPU_CHECK(hipSetDevice(device));
  MoveResources res;
  std::vector<uint32_t> recs;
  if (int rc = move_run(p, res, recs, &rep->kernel_ms)) return rc;

  std::vector<uint32_t> cus(1024);
  uint32_t n_cus = 0;
  for (size_t wv = 0; wv < (size_t)p->blocks * 4; ++wv) {
    const uint32_t* r = &recs[wv * MOVE_RECORD_WORDS];
    if (r[0] == 0xFFFFFFFFu) continue;  // record never written
    rep->waves_run++;
    move_add_unique(cus.data(), &n_cus, (uint32_t)cus.size(), r[0]);
    const uint32_t* e = &expected[(wv % EGPU_MOVE_PATTERNS) * EGPU_MOVE_NKINDS];
    uint32_t kinds = 0;
    for (int k = 0; k < EGPU_MOVE_NKINDS; ++k)
      if (r[1 + k] != e[k]) kinds |= 1u << k;
    if (kinds) {
      rep->bad_waves++;
      rep->bad_kinds |= kinds;
      move_add_unique(rep->bad_cus, &rep->n_bad_cus, 64, r[0]);
    }
  }
  rep->cus_seen = n_cus;
  return 0;
}

// The raw records of one run, MOVE_RECORD_WORDS words per wave:
// {cu_id, sig[NKINDS]}. records holds 4*blocks of them.
extern "C" int egpu_movetest_records(int device, const egpu_movetest_params* p, uint32_t* records,
                                     int max_records) {
  if (records == nullptr) EGPU_BAD_ARG("movetest_records: records is null");
  if (device < 0) EGPU_BAD_ARG("movetest_records: device %d is negative", device);
  if (int rc = move_validate(p)) return rc;
  if (max_records < p->blocks * 4)
    EGPU_BAD_ARG("movetest_records: room for %d records, need %d", max_records, p->blocks * 4);
  EGPU_CHECK(hipSetDevice(device));
  MoveResources res;
  std::vector<uint32_t> recs;
  float ms = 0.f;
  if (int rc = move_run(p, res, recs, &ms)) return rc;
  for (size_t i = 0; i < recs.size(); ++i) records[i] = recs[i];
  return 0;
}

// One wave, one kind, one round, tile 0. regs_out[4 * lane + reg] is what the
// lane received (unused registers zero), src_out the 256 source words.
extern "C" int egpu_movetest_tile(int device, int kind, int pattern, uint32_t seed, int round,
                                  uint32_t* regs_out, uint32_t* src_out) {
  if (regs_out == nullptr || src_out == nullptr) EGPU_BAD_ARG("movetest_tile: null output");
  if (device < 0) EGPU_BAD_ARG("movetest_tile: device %d is negative", device);
  if (!mv::kind_ok(kind)) EGPU_BAD_ARG("movetest_tile: unknown kind %d", kind);
  if (pattern < 0 || pattern >= EGPU_MOVE_PATTERNS)
    EGPU_BAD_ARG("movetest_tile: pattern %d outside [0, %d)", pattern, EGPU_MOVE_PATTERNS);
  if (round < 0 || round >= EGPU_MOVE_MAX_ROUNDS)
    EGPU_BAD_ARG("movetest_tile: round %d outside [0, %d)", round, EGPU_MOVE_MAX_ROUNDS);
  EGPU_CHECK(hipSetDevice(device));
  MoveResources res;
  const size_t bytes = EGPU_MOVE_TILE_WORDS * sizeof(uint32_t);
  if (int rc = move_source(res, seed)) return rc;
  EGPU_CHECK(hipMalloc(&res.dev[0], bytes));
  EGPU_CHECK(hipMalloc(&res.dev[2], bytes));
  EGPU_CHECK(hipMemset(res.dev[0], 0, bytes));
  EGPU_CHECK(hipMemset(res.dev[2], 0, bytes));
  const uint32_t* src = (const uint32_t*)res.dev[1];
  uint32_t *regs = (uint32_t*)res.dev[0], *srcw = (uint32_t*)res.dev[2];
  switch (kind) {
    case mv::K_G2L16: move_launch_tile<mv::K_G2L16>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_G2L4: move_launch_tile<mv::K_G2L4>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_B128: move_launch_tile<mv::K_B128>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_TR16: move_launch_tile<mv::K_TR16>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_TR8: move_launch_tile<mv::K_TR8>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_TR6: move_launch_tile<mv::K_TR6>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_TR4: move_launch_tile<mv::K_TR4>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_BPERM: move_launch_tile<mv::K_BPERM>(src, pattern, seed, round, regs, srcw); break;
    case mv::K_SWAP: move_launch_tile<mv::K_SWAP>(src, pattern, seed, round, regs, srcw); break;
    default: move_launch_tile<mv::K_DPP>(src, pattern, seed, round, regs, srcw); break;
  }
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipDeviceSynchronize());
  EGPU_CHECK(hipMemcpy(regs_out, regs, bytes, hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(src_out, srcw, bytes, hipMemcpyDeviceToHost));
  return 0;
}
