// Matrix sweep of the GPU self-test (part of libegpu_kernels.so): the MFMA
// shapes and number formats that selftest_kernel's one bf16 instruction does
// not reach.
//
//   mx_selftest_kernel  256 threads = 4 waves per workgroup, like
//                       selftest_kernel. Every wave runs every kind of
//                       selftest_mx_ref.h: `rounds` MFMAs into one accumulator,
//                       operands regenerated each round, and writes one record
//                       {cu_id, sig[NKINDS]}. Inputs are a pure function of
//                       pattern = (blockIdx.x*4 + wave) % 16, seed and rounds.
//   mx_tile_kernel      one wave, one kind: the D tile and the operands and
//                       scales the lanes meant to supply in the last round, so
//                       a test can compare against a plain matmul. A wrong lane
//                       map, packing or scale select shows as a wrong tile.
//
// All format and opsel arguments of the instructions are compile-time
// constants. inject_kind corrupts data only, never an address.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#define EGPU_ST_FN __host__ __device__ inline
#include "selftest_mx_ref.h"

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

#define EGPU_BAD_ARG(...)                       \
  do {                                          \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__); \
    return -1;                                  \
  } while (0)

#define EGPU_MXTEST_VERSION 1
#define EGPU_MXTEST_MAX_BLOCKS 65536
#define MX_RECORD_WORDS (1 + EGPU_MX_NKINDS)
#define MX_INJECT_NONE (-1)

extern "C" {
struct egpu_mxtest_params {
  int32_t blocks;
  int32_t rounds;
  uint32_t seed;
  int32_t inject_kind;   // -1 = none, else a kind index
  int32_t inject_block;  // workgroup whose signature of that kind is corrupted
};

struct egpu_mxtest_report {
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

namespace mx = egpu_mx;

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x8 = __attribute__((ext_vector_type(8))) int;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using i32x16 = __attribute__((ext_vector_type(16))) int;

__device__ inline uint32_t mx_wave_sum(uint32_t v) {
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// One MFMA of KIND on the registers lane_operands produced.
template <int KIND, typename ACC>
__device__ inline ACC mx_mfma(const mx::lane_regs& r, ACC acc) {
  const u32x4 a4 = {r.a[0], r.a[1], r.a[2], r.a[3]}, b4 = {r.b[0], r.b[1], r.b[2], r.b[3]};
  const i32x8 a8 = {(int)r.a[0], (int)r.a[1], (int)r.a[2], (int)r.a[3],
                    (int)r.a[4], (int)r.a[5], (int)r.a[6], (int)r.a[7]};
  const i32x8 b8 = {(int)r.b[0], (int)r.b[1], (int)r.b[2], (int)r.b[3],
                    (int)r.b[4], (int)r.b[5], (int)r.b[6], (int)r.b[7]};
  const long al = (long)(((uint64_t)r.a[1] << 32) | r.a[0]);
  const long bl = (long)(((uint64_t)r.b[1] << 32) | r.b[0]);
  if constexpr (KIND == mx::K_F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a4),
                                                  __builtin_bit_cast(half8, b4), acc, 0, 0, 0);
  else if constexpr (KIND == mx::K_I8)
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, a4),
                                                 __builtin_bit_cast(i32x4, b4), acc, 0, 0, 0);
  else if constexpr (KIND == mx::K_FP8)
    return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(al, bl, acc, 0, 0, 0);
  else if constexpr (KIND == mx::K_BF8)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(al, bl, acc, 0, 0, 0);
  else if constexpr (KIND == mx::K_BF16S)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a4),
                                                   __builtin_bit_cast(bf16x8, b4), acc, 0, 0, 0);
  else if constexpr (KIND == mx::K_MXFP8)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
        a8, b8, acc, 0, 0, mx::SCALE_BYTE_A, (int)r.sa, mx::SCALE_BYTE_B, (int)r.sb);
  else if constexpr (KIND == mx::K_MXFP6)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
        a8, b8, acc, 2, 2, mx::SCALE_BYTE_A, (int)r.sa, mx::SCALE_BYTE_B, (int)r.sb);
  else if constexpr (KIND == mx::K_MXFP4)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
        a8, b8, acc, 4, 4, mx::SCALE_BYTE_A, (int)r.sa, mx::SCALE_BYTE_B, (int)r.sb);
  else
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
        a8, b8, acc, 0, 4, mx::SCALE_BYTE_A, (int)r.sa, mx::SCALE_BYTE_B, (int)r.sb);
}

template <int KIND> struct mx_acc {
  using type = f32x16;
};
template <> struct mx_acc<mx::K_I8> {
  using type = i32x16;
};
template <> struct mx_acc<mx::K_BF16S> {
  using type = f32x4;
};
template <> struct mx_acc<mx::K_MXMIX> {
  using type = f32x4;
};

// `rounds` MFMAs of KIND into one accumulator. units[reg] = acc * 4 as an
// integer (i8: acc); *last = the registers of the last round.
template <int KIND>
__device__ inline void mx_chain(uint32_t seed, int pattern, int lane, int rounds,
                                int units[mx::traits<KIND>::NREG], mx::lane_regs* last) {
  using T = mx::traits<KIND>;
  typename mx_acc<KIND>::type acc;
#pragma unroll
  for (int i = 0; i < T::NREG; ++i) acc[i] = 0;
  mx::lane_regs r;
  for (int rd = 0; rd < rounds; ++rd) {
    mx::lane_operands<KIND>(seed, pattern, lane, rd, &r);
    acc = mx_mfma<KIND>(r, acc);
  }
#pragma unroll
  for (int i = 0; i < T::NREG; ++i)
    units[i] = KIND == mx::K_I8 ? (int)acc[i] : (int)((float)acc[i] * 4.0f);
  *last = r;
}

template <int KIND>
__device__ inline uint32_t mx_sig(uint32_t seed, int pattern, int lane, int rounds) {
  int units[mx::traits<KIND>::NREG];
  mx::lane_regs last;
  mx_chain<KIND>(seed, pattern, lane, rounds, units, &last);
  uint32_t h = 0;
#pragma unroll
  for (int reg = 0; reg < mx::traits<KIND>::NREG; ++reg) h = mx::acc_hash_step(h, units[reg]);
  return mx_wave_sum(h * mx::lane_weight(lane));
}

__global__ void __launch_bounds__(256)
mx_selftest_kernel(uint32_t* __restrict__ out, int rounds, uint32_t seed, int inject_kind,
                   int inject_block) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int pattern = (blockIdx.x * 4 + wave) % EGPU_MX_PATTERNS;

  uint32_t hwid, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));

  uint32_t sig[EGPU_MX_NKINDS];
  sig[mx::K_F16] = mx_sig<mx::K_F16>(seed, pattern, lane, rounds);
  sig[mx::K_I8] = mx_sig<mx::K_I8>(seed, pattern, lane, rounds);
  sig[mx::K_FP8] = mx_sig<mx::K_FP8>(seed, pattern, lane, rounds);
  sig[mx::K_BF8] = mx_sig<mx::K_BF8>(seed, pattern, lane, rounds);
  sig[mx::K_BF16S] = mx_sig<mx::K_BF16S>(seed, pattern, lane, rounds);
  sig[mx::K_MXFP8] = mx_sig<mx::K_MXFP8>(seed, pattern, lane, rounds);
  sig[mx::K_MXFP6] = mx_sig<mx::K_MXFP6>(seed, pattern, lane, rounds);
  sig[mx::K_MXFP4] = mx_sig<mx::K_MXFP4>(seed, pattern, lane, rounds);
  sig[mx::K_MXMIX] = mx_sig<mx::K_MXMIX>(seed, pattern, lane, rounds);

  if (lane == 0) {
    uint32_t* rec = out + (size_t)(blockIdx.x * 4 + wave) * MX_RECORD_WORDS;
    // same encoding as the census: (xcc << 16) | {SE, SH, CU} bits of HW_ID
    rec[0] = (xcc << 16) | ((hwid >> 8) & 0x7F);
#pragma unroll
    for (int k = 0; k < EGPU_MX_NKINDS; ++k)
      rec[1 + k] = sig[k] ^ (((int)blockIdx.x == inject_block && k == inject_kind) ? 1u : 0u);
  }
}

// d: M x M; a: M x K; b: K x M; sa: M x K/32; sb: K/32 x M (all int32,
// row-major). a and b hold four times the value the lane encoded.
template <int KIND>
__global__ void __launch_bounds__(64)
mx_tile_kernel(int pattern, uint32_t seed, int rounds, int32_t* __restrict__ d,
               int32_t* __restrict__ a, int32_t* __restrict__ b, int32_t* __restrict__ sa,
               int32_t* __restrict__ sb) {
  using T = mx::traits<KIND>;
  const int lane = threadIdx.x & 63;
  int units[T::NREG];
  mx::lane_regs last;
  mx_chain<KIND>(seed, pattern, lane, rounds, units, &last);
  const int idx = mx::ab_index(T::M, lane);
#pragma unroll
  for (int reg = 0; reg < T::NREG; ++reg) d[mx::cd_row(T::M, lane, reg) * T::M + idx] = units[reg];
#pragma unroll
  for (int j = 0; j < T::E; ++j) {
    const int ka = mx::ab_k(T::M, T::E, mx::fmt_bits(T::FA), lane, j);
    const int kb = mx::ab_k(T::M, T::E, mx::fmt_bits(T::FB), lane, j);
    a[idx * T::K + ka] = mx::elem_x4(T::FA, mx::elem_code(last.wa, j));
    b[kb * T::M + idx] = mx::elem_x4(T::FB, mx::elem_code(last.wb, j));
  }
  if (T::SCALED) {
    const int kb = lane / T::M;
    sa[idx * (T::K / 32) + kb] = (int)((last.sa >> (8 * mx::SCALE_BYTE_A)) & 0xffu) - 127;
    sb[kb * T::M + idx] = (int)((last.sb >> (8 * mx::SCALE_BYTE_B)) & 0xffu) - 127;
  }
}

// ---------------------------------------------------------------- host side

namespace {

// the largest tile operands: 32 x 64 = 16 x 128 = 2048 elements
enum { TILE_D = 1024, TILE_AB = 2048, TILE_S = 64 };

struct MxResources {
  void* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~MxResources() {
    for (void* p : dev)
      if (p) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int mx_validate(const egpu_mxtest_params* p) {
  if (p == nullptr) EGPU_BAD_ARG("mxtest: params is null");
  if (p->blocks <= 0 || p->blocks > EGPU_MXTEST_MAX_BLOCKS)
    EGPU_BAD_ARG("mxtest: blocks %d outside [1, %d]", p->blocks, EGPU_MXTEST_MAX_BLOCKS);
  if (!mx::rounds_ok(p->rounds))
    EGPU_BAD_ARG("mxtest: rounds %d outside [1, %d]", p->rounds, EGPU_MX_MAX_ROUNDS);
  if (p->inject_kind != MX_INJECT_NONE) {
    if (p->inject_kind < 0 || p->inject_kind >= EGPU_MX_NKINDS)
      EGPU_BAD_ARG("mxtest: unknown inject_kind %d", p->inject_kind);
    if (p->inject_block < 0 || p->inject_block >= p->blocks)
      EGPU_BAD_ARG("mxtest: inject_block %d is not a workgroup of a %d-block grid",
                   p->inject_block, p->blocks);
  }
  return 0;
}

// Runs mx_selftest_kernel; recs = 4*blocks records of MX_RECORD_WORDS words.
int mx_run(const egpu_mxtest_params* p, MxResources& res, std::vector<uint32_t>& recs, float* ms) {
  const size_t words = (size_t)p->blocks * 4 * MX_RECORD_WORDS;
  EGPU_CHECK(hipMalloc(&res.dev[0], words * sizeof(uint32_t)));
  EGPU_CHECK(hipMemset(res.dev[0], 0xFF, words * sizeof(uint32_t)));
  EGPU_CHECK(hipEventCreate(&res.ev[0]));
  EGPU_CHECK(hipEventCreate(&res.ev[1]));
  EGPU_CHECK(hipEventRecord(res.ev[0], 0));
  const bool inject = p->inject_kind != MX_INJECT_NONE;
  hipLaunchKernelGGL(mx_selftest_kernel, dim3(p->blocks), dim3(256), 0, 0, (uint32_t*)res.dev[0],
                     p->rounds, p->seed, inject ? p->inject_kind : -1,
                     inject ? p->inject_block : -1);
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipEventRecord(res.ev[1], 0));
  EGPU_CHECK(hipEventSynchronize(res.ev[1]));
  EGPU_CHECK(hipEventElapsedTime(ms, res.ev[0], res.ev[1]));
  recs.resize(words);
  EGPU_CHECK(hipMemcpy(recs.data(), res.dev[0], words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

void mx_add_unique(uint32_t* ids, uint32_t* n, uint32_t cap, uint32_t id) {
  for (uint32_t j = 0; j < *n; ++j)
    if (ids[j] == id) return;
  if (*n < cap) ids[(*n)++] = id;
}

struct launch_tile_fn {
  int pattern, rounds;
  uint32_t seed;
  int32_t *d, *a, *b, *sa, *sb;
  template <int KIND> void operator()() {
    hipLaunchKernelGGL(mx_tile_kernel<KIND>, dim3(1), dim3(64), 0, 0, pattern, seed, rounds, d, a,
                       b, sa, sb);
  }
};

}  // namespace

// Host reference: out[NKINDS * pattern + kind], 16 patterns. Touches no HIP
// API, so it runs on a machine without a GPU.
extern "C" int egpu_mxtest_expected(uint32_t seed, int rounds, uint32_t* out) {
  if (out == nullptr) EGPU_BAD_ARG("mxtest_expected: out is null");
  if (mx::expected_all(seed, rounds, out) != 0)
    EGPU_BAD_ARG("mxtest_expected: rounds %d outside [1, %d]", rounds, EGPU_MX_MAX_ROUNDS);
  return 0;
}

struct lane_regs_fn {
  uint32_t seed;
  int pattern, round;
  uint32_t *a, *b, *sa, *sb;
  template <int KIND> void operator()() {
    for (int l = 0; l < 64; ++l) {
      mx::lane_regs r;
      mx::lane_operands<KIND>(seed, pattern, l, round, &r);
      for (int i = 0; i < 8; ++i) {
        a[8 * l + i] = r.a[i];
        b[8 * l + i] = r.b[i];
      }
      sa[l] = r.sa;
      sb[l] = r.sb;
    }
  }
};

// The registers the 64 lanes hand to the instruction in one round, as the
// generator encodes them: a and b 8 words per lane (unused high words zero), sa
// and sb one scale word per lane (zero for unscaled kinds). Touches no HIP API;
// tests decode these bits with decoders of their own.
extern "C" int egpu_mxtest_lane_regs(int kind, int pattern, uint32_t seed, int round, uint32_t* a,
                                     uint32_t* b, uint32_t* sa, uint32_t* sb) {
  if (a == nullptr || b == nullptr || sa == nullptr || sb == nullptr)
    EGPU_BAD_ARG("mxtest_lane_regs: null output");
  if (kind < 0 || kind >= EGPU_MX_NKINDS) EGPU_BAD_ARG("mxtest_lane_regs: unknown kind %d", kind);
  if (pattern < 0 || pattern >= EGPU_MX_PATTERNS)
    EGPU_BAD_ARG("mxtest_lane_regs: pattern %d outside [0, %d)", pattern, EGPU_MX_PATTERNS);
  if (round < 0 || round >= EGPU_MX_MAX_ROUNDS)
    EGPU_BAD_ARG("mxtest_lane_regs: round %d outside [0, %d)", round, EGPU_MX_MAX_ROUNDS);
  lane_regs_fn f{seed, pattern, round, a, b, sa, sb};
  mx::for_kind(kind, f);
  return 0;
}

// Arguments are validated before the first HIP call: a bad argument is an
// error code (-1) on a machine with no GPU too.
extern "C" int egpu_mxtest(int device, const egpu_mxtest_params* p, egpu_mxtest_report* rep) {
  if (rep == nullptr) EGPU_BAD_ARG("mxtest: report is null");
  if (device < 0) EGPU_BAD_ARG("mxtest: device %d is negative", device);
  if (int rc = mx_validate(p)) return rc;
  *rep = egpu_mxtest_report{};
  rep->version = EGPU_MXTEST_VERSION;

  std::vector<uint32_t> expected(EGPU_MX_PATTERNS * EGPU_MX_NKINDS);
  mx::expected_all(p->seed, p->rounds, expected.data());

  EGPU_CHECK(hipSetDevice(device));
  MxResources res;
  std::vector<uint32_t> recs;
  if (int rc = mx_run(p, res, recs, &rep->kernel_ms)) return rc;

  std::vector<uint32_t> cus(1024);
  uint32_t n_cus = 0;
  for (size_t wv = 0; wv < (size_t)p->blocks * 4; ++wv) {
    const uint32_t* r = &recs[wv * MX_RECORD_WORDS];
    if (r[0] == 0xFFFFFFFFu) continue;  // record never written
    rep->waves_run++;
    mx_add_unique(cus.data(), &n_cus, (uint32_t)cus.size(), r[0]);
    const uint32_t* e = &expected[(wv % EGPU_MX_PATTERNS) * EGPU_MX_NKINDS];
    uint32_t kinds = 0;
    for (int k = 0; k < EGPU_MX_NKINDS; ++k)
      if (r[1 + k] != e[k]) kinds |= 1u << k;
    if (kinds) {
      rep->bad_waves++;
      rep->bad_kinds |= kinds;
      mx_add_unique(rep->bad_cus, &rep->n_bad_cus, 64, r[0]);
    }
  }
  rep->cus_seen = n_cus;
  return 0;
}

// The raw records of one run, MX_RECORD_WORDS words per wave:
// {cu_id, sig[NKINDS]}. records holds 4*blocks of them.
extern "C" int egpu_mxtest_records(int device, const egpu_mxtest_params* p, uint32_t* records,
                                   int max_records) {
  if (records == nullptr) EGPU_BAD_ARG("mxtest_records: records is null");
  if (device < 0) EGPU_BAD_ARG("mxtest_records: device %d is negative", device);
  if (int rc = mx_validate(p)) return rc;
  if (max_records < p->blocks * 4)
    EGPU_BAD_ARG("mxtest_records: room for %d records, need %d", max_records, p->blocks * 4);
  EGPU_CHECK(hipSetDevice(device));
  MxResources res;
  std::vector<uint32_t> recs;
  float ms = 0.f;
  if (int rc = mx_run(p, res, recs, &ms)) return rc;
  for (size_t i = 0; i < recs.size(); ++i) records[i] = recs[i];
  return 0;
}

// One wave of one kind. d (M*M) is the D tile after `rounds` MFMAs in hash
// units (acc*4; i8: acc); a (M*K) and b (K*M) are four times the last round's
// operand values; sa (M * K/32) and sb (K/32 * M) are that round's scale
// exponents, zero for unscaled kinds. Callers pass room for the largest kind:
// d 1024, a and b 2048, sa and sb 64 int32 each.
extern "C" int egpu_mxtest_tile(int device, int kind, int pattern, uint32_t seed, int rounds,
                                int32_t* d, int32_t* a, int32_t* b, int32_t* sa, int32_t* sb) {
  if (d == nullptr || a == nullptr || b == nullptr || sa == nullptr || sb == nullptr)
    EGPU_BAD_ARG("mxtest_tile: null output");
  if (device < 0) EGPU_BAD_ARG("mxtest_tile: device %d is negative", device);
  if (kind < 0 || kind >= EGPU_MX_NKINDS) EGPU_BAD_ARG("mxtest_tile: unknown kind %d", kind);
  if (pattern < 0 || pattern >= EGPU_MX_PATTERNS)
    EGPU_BAD_ARG("mxtest_tile: pattern %d outside [0, %d)", pattern, EGPU_MX_PATTERNS);
  if (!mx::rounds_ok(rounds))
    EGPU_BAD_ARG("mxtest_tile: rounds %d outside [1, %d]", rounds, EGPU_MX_MAX_ROUNDS);
  EGPU_CHECK(hipSetDevice(device));
  MxResources res;
  const size_t sizes[5] = {TILE_D, TILE_AB, TILE_AB, TILE_S, TILE_S};
  int32_t* host[5] = {d, a, b, sa, sb};
  for (int i = 0; i < 5; ++i) {
    EGPU_CHECK(hipMalloc(&res.dev[i], sizes[i] * sizeof(int32_t)));
    EGPU_CHECK(hipMemset(res.dev[i], 0, sizes[i] * sizeof(int32_t)));
  }
  launch_tile_fn launch{pattern, rounds, seed, (int32_t*)res.dev[0], (int32_t*)res.dev[1],
                        (int32_t*)res.dev[2], (int32_t*)res.dev[3], (int32_t*)res.dev[4]};
  mx::for_kind(kind, launch);
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipDeviceSynchronize());
  for (int i = 0; i < 5; ++i)
    EGPU_CHECK(hipMemcpy(host[i], res.dev[i], sizes[i] * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}
