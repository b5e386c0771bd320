// GPU self-test kernels (part of libegpu_kernels.so): checks RESULTS, where
// the probes in egpu_kernels.hip check placement and timing.
//
//   selftest_kernel     256 threads = 4 waves per workgroup, so every SIMD of
//                       the CU that runs the workgroup executes the checks.
//                       Each wave writes one record {cu_id, int_sig, fma_sig,
//                       mfma_sig, lds_bad}. Inputs are a pure function of
//                       pattern = (blockIdx.x*4 + wave) % 64, seed and rounds,
//                       so the host needs 64 expected records whatever the
//                       grid (selftest_ref.h).
//   hbm_pattern_kernel  grid-stride write / verify of a scratch buffer with
//                       16-byte accesses. It checks the pages the allocator
//                       hands out, and below the 256 MB Infinity Cache mostly
//                       the cache: a data-path sanity check, not a memory
//                       tester.
//   mfma_tile_kernel    one wave, returns the D tile and the last A and B so a
//                       test can compare against a plain matmul: a wrong lane
//                       map shows as a wrong tile, not as an opaque signature.
//
// inject_kind simulates a miscompare so detection is testable on a healthy
// GPU. It corrupts data only, never an address.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#define EGPU_ST_FN __host__ __device__ inline
#include "selftest_ref.h"

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

enum { INJECT_NONE = 0, INJECT_INT = 1, INJECT_FMA = 2, INJECT_MFMA = 3, INJECT_LDS = 4,
       INJECT_HBM = 5 };
enum { KIND_INT = 1, KIND_FMA = 2, KIND_MFMA = 4, KIND_LDS = 8 };
enum { HBM_OK = 0, HBM_FAILED = 1, HBM_SKIPPED = 2, HBM_OFF = 3 };

#define EGPU_SELFTEST_VERSION 1
#define EGPU_SELFTEST_MIN_LDS 1024
#define EGPU_SELFTEST_MAX_BLOCKS 65536
#define EGPU_SELFTEST_MAX_HBM (64ull << 30)
#define RECORD_WORDS 5

extern "C" {
struct egpu_selftest_params {
  int32_t blocks;
  int32_t rounds;
  uint32_t seed;
  uint32_t lds_bytes;
  uint64_t hbm_bytes;  // 0 = no memory-path check
  int32_t inject_kind;
  int32_t reserved;
  uint64_t inject_arg;  // workgroup index (int/fma/mfma/lds) or byte offset (hbm)
};

struct egpu_selftest_report {
  uint32_t version;
  uint32_t waves_run;
  uint32_t cus_seen;
  uint32_t bad_waves;
  uint32_t bad_kinds;  // KIND_* bit mask
  uint32_t n_bad_cus;
  uint32_t bad_cus[64];  // physical ids (census encoding), deduplicated
  uint32_t lds_bytes;
  int32_t hbm_status;  // HBM_*
  uint64_t hbm_bytes_checked;
  uint64_t hbm_miscompares;
  uint64_t hbm_first_bad_offset;
  float kernel_ms;
  float hbm_ms;
};
}

// ---------------------------------------------------------------- device side

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using short8 = __attribute__((ext_vector_type(8))) short;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ inline uint32_t wave_sum(uint32_t v) {
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// whole numbers in [-3, 3] are exact in bf16: the top 16 bits of the f32
__device__ inline short bf16_bits(int k) { return (short)(__float_as_uint((float)k) >> 16); }

// `rounds` MFMAs into one accumulator; A and B regenerated every round.
// Lane l holds A[l&31][8*(l>>5)+j] and B[8*(l>>5)+j][l&31], j = 0..7.
__device__ inline f32x16 mfma_chain(uint32_t s, int rounds, uint32_t* last_a, uint32_t* last_b) {
  f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  uint32_t wa = 0, wb = 0;
  for (int r = 0; r < rounds; ++r) {
    wa = egpu_st::mfma_word(s, r, 0);
    wb = egpu_st::mfma_word(s, r, 1);
    short8 a, b;
    for (int j = 0; j < 8; ++j) {
      a[j] = bf16_bits(egpu_st::mfma_elem(wa, j));
      b[j] = bf16_bits(egpu_st::mfma_elem(wb, j));
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                  __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  }
  *last_a = wa;
  *last_b = wb;
  return acc;
}

__global__ void __launch_bounds__(256)
selftest_kernel(uint32_t* __restrict__ out, int rounds, uint32_t seed, uint32_t lds_words,
                int inject_kind, int inject_block) {
  extern __shared__ uint32_t lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int pattern = (blockIdx.x * 4 + wave) & 63;
  const bool inject_here = (int)blockIdx.x == inject_block;

  uint32_t hwid, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));

  const uint32_t w = egpu_st::lane_weight(lane);
  uint32_t int_sig =
      wave_sum(egpu_st::int_chain(egpu_st::lane_seed(seed, pattern, lane, 0), rounds) * w);
  uint32_t fma_sig =
      wave_sum(egpu_st::fma_chain(egpu_st::lane_seed(seed, pattern, lane, 1), rounds) * w);

  uint32_t wa, wb;
  const f32x16 acc = mfma_chain(egpu_st::lane_seed(seed, pattern, lane, 2), rounds, &wa, &wb);
  uint32_t h = 0;
  for (int reg = 0; reg < 16; ++reg) h = egpu_st::acc_hash_step(h, (int)acc[reg]);
  uint32_t mfma_sig = wave_sum(h * w);

  // LDS march: every word is written by thread (word % 256) and verified by a
  // thread of another wave; then again with the complement.
  uint32_t bad = 0;
  const uint32_t other = (uint32_t)(tid + 67) & 255u;
  for (int pass = 0; pass < 2; ++pass) {
    const uint32_t inv = pass ? 0xffffffffu : 0u;
    for (uint32_t i = tid; i < lds_words; i += 256) lds[i] = egpu_st::lds_word(i, seed) ^ inv;
    __syncthreads();
    if (pass == 0 && inject_kind == INJECT_LDS && inject_here && tid == 0) lds[0] ^= 1u;
    __syncthreads();
    for (uint32_t i = other; i < lds_words; i += 256)
      bad += lds[i] != (egpu_st::lds_word(i, seed) ^ inv);
    __syncthreads();
  }
  // LDS belongs to the CU, not to a wave: every record of the workgroup
  // carries the workgroup's total (the march left no LDS to spare for a
  // counter, so the first four words are reused)
  bad = wave_sum(bad);
  if (lane == 0) lds[wave] = bad;
  __syncthreads();
  const uint32_t lds_bad = lds[0] + lds[1] + lds[2] + lds[3];

  if (inject_here) {
    if (inject_kind == INJECT_INT) int_sig ^= 1u;
    if (inject_kind == INJECT_FMA) fma_sig ^= 1u;
    if (inject_kind == INJECT_MFMA) mfma_sig ^= 1u;
  }
  if (lane == 0) {
    uint32_t* rec = out + (size_t)(blockIdx.x * 4 + wave) * RECORD_WORDS;
    // same encoding as the census: (xcc << 16) | {SE, SH, CU} bits of HW_ID
    rec[0] = (xcc << 16) | ((hwid >> 8) & 0x7F);
    rec[1] = int_sig;
    rec[2] = fma_sig;
    rec[3] = mfma_sig;
    rec[4] = lds_bad;
  }
}

__global__ void __launch_bounds__(64)
mfma_tile_kernel(int pattern, uint32_t seed, int rounds, int32_t* __restrict__ d,
                 int8_t* __restrict__ a, int8_t* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  uint32_t wa, wb;
  const f32x16 acc = mfma_chain(egpu_st::lane_seed(seed, pattern, lane, 2), rounds, &wa, &wb);
  for (int reg = 0; reg < 16; ++reg) {
    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    d[row * 32 + (lane & 31)] = (int)acc[reg];
  }
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * (lane >> 5) + j;
    a[(lane & 31) * 16 + k] = (int8_t)egpu_st::mfma_elem(wa, j);
    b[k * 32 + (lane & 31)] = (int8_t)egpu_st::mfma_elem(wb, j);
  }
}

__global__ void __launch_bounds__(256)
hbm_pattern_kernel(uint4* __restrict__ buf, uint64_t n16, uint32_t seed, uint32_t inv, int verify,
                   unsigned long long* __restrict__ miscompares,
                   unsigned long long* __restrict__ first_bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
    const uint32_t p[4] = {egpu_st::hbm_word(i, 0, seed) ^ inv, egpu_st::hbm_word(i, 1, seed) ^ inv,
                           egpu_st::hbm_word(i, 2, seed) ^ inv, egpu_st::hbm_word(i, 3, seed) ^ inv};
    if (!verify) {
      buf[i] = make_uint4(p[0], p[1], p[2], p[3]);
      continue;
    }
    const uint4 v = buf[i];
    const uint32_t got[4] = {v.x, v.y, v.z, v.w};
    for (int k = 0; k < 4; ++k)
      if (got[k] != p[k]) {
        atomicAdd(miscompares, 1ull);
        atomicMin(first_bad, (unsigned long long)(i * 16 + 4 * k));
      }
  }
}

// ---------------------------------------------------------------- host side

namespace {

// frees whatever was allocated, on every return path
struct Resources {
  void* dev[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~Resources() {
    for (void* p : dev)
      if (p) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int validate(const egpu_selftest_params* p) {
  if (p == nullptr) EGPU_BAD_ARG("selftest: params is null");
  if (p->blocks <= 0 || p->blocks > EGPU_SELFTEST_MAX_BLOCKS)
    EGPU_BAD_ARG("selftest: blocks %d outside [1, %d]", p->blocks, EGPU_SELFTEST_MAX_BLOCKS);
  if (!egpu_st::rounds_ok(p->rounds))
    EGPU_BAD_ARG("selftest: rounds %d outside [1, %d]", p->rounds, EGPU_SELFTEST_MAX_ROUNDS);
  if (p->lds_bytes < EGPU_SELFTEST_MIN_LDS || p->lds_bytes > EGPU_SELFTEST_MAX_LDS ||
      p->lds_bytes % 4 != 0)
    EGPU_BAD_ARG("selftest: lds_bytes %u must be a multiple of 4 in [%d, %d]", p->lds_bytes,
                 EGPU_SELFTEST_MIN_LDS, EGPU_SELFTEST_MAX_LDS);
  if (p->hbm_bytes % 16 != 0 || p->hbm_bytes > EGPU_SELFTEST_MAX_HBM)
    EGPU_BAD_ARG("selftest: hbm_bytes %llu must be a multiple of 16, at most %llu",
                 (unsigned long long)p->hbm_bytes, EGPU_SELFTEST_MAX_HBM);
  switch (p->inject_kind) {
    case INJECT_NONE:
      break;
    case INJECT_INT:
    case INJECT_FMA:
    case INJECT_MFMA:
    case INJECT_LDS:
      if (p->inject_arg >= (uint64_t)p->blocks)
        EGPU_BAD_ARG("selftest: inject_arg %llu is not a workgroup of a %d-block grid",
                     (unsigned long long)p->inject_arg, p->blocks);
      break;
    case INJECT_HBM:
      if (p->inject_arg % 4 != 0 || p->inject_arg >= p->hbm_bytes)
        EGPU_BAD_ARG("selftest: inject_arg %llu is not a word offset inside hbm_bytes",
                     (unsigned long long)p->inject_arg);
      break;
    default:
      EGPU_BAD_ARG("selftest: unknown inject_kind %d", p->inject_kind);
  }
  return 0;
}

// Runs selftest_kernel; recs = 4*blocks records of RECORD_WORDS words.
int run_compute(const egpu_selftest_params* p, Resources& res, std::vector<uint32_t>& recs,
                float* ms) {
  const size_t words = (size_t)p->blocks * 4 * RECORD_WORDS;
  EGPU_CHECK(hipMalloc(&res.dev[0], words * sizeof(uint32_t)));
  EGPU_CHECK(hipMemset(res.dev[0], 0xFF, words * sizeof(uint32_t)));
  if (p->lds_bytes > 65536)
    EGPU_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(selftest_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)p->lds_bytes));
  const bool wg_inject = p->inject_kind >= INJECT_INT && p->inject_kind <= INJECT_LDS;
  EGPU_CHECK(hipEventCreate(&res.ev[0]));
  EGPU_CHECK(hipEventCreate(&res.ev[1]));
  EGPU_CHECK(hipEventRecord(res.ev[0], 0));
  hipLaunchKernelGGL(selftest_kernel, dim3(p->blocks), dim3(256), p->lds_bytes, 0,
                     (uint32_t*)res.dev[0], p->rounds, p->seed, p->lds_bytes / 4,
                     wg_inject ? p->inject_kind : INJECT_NONE,
                     wg_inject ? (int)p->inject_arg : -1);
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipEventRecord(res.ev[1], 0));
  EGPU_CHECK(hipEventSynchronize(res.ev[1]));
  EGPU_CHECK(hipEventElapsedTime(ms, res.ev[0], res.ev[1]));
  recs.resize(words);
  EGPU_CHECK(hipMemcpy(recs.data(), res.dev[0], words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

void add_unique(uint32_t* ids, uint32_t* n, uint32_t cap, uint32_t id) {
  for (uint32_t j = 0; j < *n; ++j)
    if (ids[j] == id) return;
  if (*n < cap) ids[(*n)++] = id;
}

int run_hbm(const egpu_selftest_params* p, Resources& res, egpu_selftest_report* rep) {
  if (p->hbm_bytes == 0) {
    rep->hbm_status = HBM_OFF;
    return 0;
  }
  if (hipMalloc(&res.dev[1], p->hbm_bytes) != hipSuccess) {
    // tenants may legitimately own the memory: not a failure of the GPU
    (void)hipGetLastError();
    res.dev[1] = nullptr;
    rep->hbm_status = HBM_SKIPPED;
    return 0;
  }
  EGPU_CHECK(hipMalloc(&res.dev[2], 2 * sizeof(unsigned long long)));
  const unsigned long long init[2] = {0ull, ~0ull};
  EGPU_CHECK(hipMemcpy(res.dev[2], init, sizeof(init), hipMemcpyHostToDevice));
  uint4* buf = (uint4*)res.dev[1];
  unsigned long long* counters = (unsigned long long*)res.dev[2];
  const uint64_t n16 = p->hbm_bytes / 16;
  // about four elements per thread, so the grid-stride loop and its tail run
  // even on a small buffer; 4096 workgroups fill all 8 XCDs on a large one
  uint64_t grid = n16 / (256 * 4);
  grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);
  EGPU_CHECK(hipEventRecord(res.ev[0], 0));
  for (int pass = 0; pass < 2; ++pass) {
    const uint32_t inv = pass ? 0xffffffffu : 0u;
    hipLaunchKernelGGL(hbm_pattern_kernel, dim3((unsigned)grid), dim3(256), 0, 0, buf, n16,
                       p->seed, inv, 0, counters, counters + 1);
    EGPU_CHECK(hipGetLastError());
    if (pass == 0 && p->inject_kind == INJECT_HBM) {
      const uint64_t off = p->inject_arg;
      const uint32_t wrong = egpu_st::hbm_word(off / 16, (int)(off % 16) / 4, p->seed) ^ 1u;
      EGPU_CHECK(hipMemcpy((char*)res.dev[1] + off, &wrong, 4, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(hbm_pattern_kernel, dim3((unsigned)grid), dim3(256), 0, 0, buf, n16,
                       p->seed, inv, 1, counters, counters + 1);
    EGPU_CHECK(hipGetLastError());
  }
  EGPU_CHECK(hipEventRecord(res.ev[1], 0));
  EGPU_CHECK(hipEventSynchronize(res.ev[1]));
  EGPU_CHECK(hipEventElapsedTime(&rep->hbm_ms, res.ev[0], res.ev[1]));
  unsigned long long got[2] = {0, 0};
  EGPU_CHECK(hipMemcpy(got, res.dev[2], sizeof(got), hipMemcpyDeviceToHost));
  rep->hbm_bytes_checked = p->hbm_bytes;
  rep->hbm_miscompares = got[0];
  rep->hbm_first_bad_offset = got[0] ? got[1] : 0;
  rep->hbm_status = got[0] ? HBM_FAILED : HBM_OK;
  return 0;
}

}  // namespace

// Host reference: 64 x (int_sig, fma_sig, mfma_sig). Touches no HIP API, so
// it runs on a machine without a GPU.
extern "C" int egpu_selftest_expected(uint32_t seed, int rounds, uint32_t* out) {
  if (out == nullptr) EGPU_BAD_ARG("selftest_expected: out is null");
  if (egpu_st::expected_all(seed, rounds, out) != 0)
    EGPU_BAD_ARG("selftest_expected: rounds %d outside [1, %d]", rounds,
                 EGPU_SELFTEST_MAX_ROUNDS);
  return 0;
}

// Arguments are validated before the first HIP call: a bad argument is an
// error code (-1) on a machine with no GPU too.
extern "C" int egpu_selftest(int device, const egpu_selftest_params* p,
                             egpu_selftest_report* rep) {
  if (rep == nullptr) EGPU_BAD_ARG("selftest: report is null");
  if (device < 0) EGPU_BAD_ARG("selftest: device %d is negative", device);
  if (int rc = validate(p)) return rc;
  *rep = egpu_selftest_report{};
  rep->version = EGPU_SELFTEST_VERSION;
  rep->lds_bytes = p->lds_bytes;

  std::vector<uint32_t> expected(EGPU_SELFTEST_PATTERNS * 3);
  egpu_st::expected_all(p->seed, p->rounds, expected.data());

  EGPU_CHECK(hipSetDevice(device));
  Resources res;
  std::vector<uint32_t> recs;
  if (int rc = run_compute(p, res, recs, &rep->kernel_ms)) return rc;

  std::vector<uint32_t> cus(1024);
  uint32_t n_cus = 0;
  for (size_t wv = 0; wv < (size_t)p->blocks * 4; ++wv) {
    const uint32_t* r = &recs[wv * RECORD_WORDS];
    if (r[0] == 0xFFFFFFFFu) continue;  // record never written
    rep->waves_run++;
    add_unique(cus.data(), &n_cus, (uint32_t)cus.size(), r[0]);
    const uint32_t* e = &expected[(wv & 63) * 3];
    uint32_t kinds = 0;
    if (r[1] != e[0]) kinds |= KIND_INT;
    if (r[2] != e[1]) kinds |= KIND_FMA;
    if (r[3] != e[2]) kinds |= KIND_MFMA;
    if (r[4] != 0) kinds |= KIND_LDS;
    if (kinds) {
      rep->bad_waves++;
      rep->bad_kinds |= kinds;
      add_unique(rep->bad_cus, &rep->n_bad_cus, 64, r[0]);
    }
  }
  rep->cus_seen = n_cus;
  return run_hbm(p, res, rep);
}

// The raw records of one compute run, RECORD_WORDS words per wave:
// {cu_id, int_sig, fma_sig, mfma_sig, lds_bad}. records holds 4*blocks of them.
extern "C" int egpu_selftest_records(int device, const egpu_selftest_params* p, uint32_t* records,
                                     int max_records) {
  if (records == nullptr) EGPU_BAD_ARG("selftest_records: records is null");
  if (device < 0) EGPU_BAD_ARG("selftest_records: device %d is negative", device);
  if (int rc = validate(p)) return rc;
  if (max_records < p->blocks * 4)
    EGPU_BAD_ARG("selftest_records: room for %d records, need %d", max_records, p->blocks * 4);
  EGPU_CHECK(hipSetDevice(device));
  Resources res;
  std::vector<uint32_t> recs;
  float ms = 0.f;
  if (int rc = run_compute(p, res, recs, &ms)) return rc;
  for (size_t i = 0; i < recs.size(); ++i) records[i] = recs[i];
  return 0;
}

// One wave: D (32x32 row-major, as integers) after `rounds` MFMAs, and the
// A (32x16) and B (16x32) of the last round.
extern "C" int egpu_selftest_mfma_tile(int device, int pattern, uint32_t seed, int rounds,
                                       int32_t* d, int8_t* a, int8_t* b) {
  if (d == nullptr || a == nullptr || b == nullptr)
    EGPU_BAD_ARG("selftest_mfma_tile: null output");
  if (device < 0) EGPU_BAD_ARG("selftest_mfma_tile: device %d is negative", device);
  if (pattern < 0 || pattern >= EGPU_SELFTEST_PATTERNS)
    EGPU_BAD_ARG("selftest_mfma_tile: pattern %d outside [0, 64)", pattern);
  if (!egpu_st::rounds_ok(rounds))
    EGPU_BAD_ARG("selftest_mfma_tile: rounds %d outside [1, %d]", rounds,
                 EGPU_SELFTEST_MAX_ROUNDS);
  EGPU_CHECK(hipSetDevice(device));
  Resources res;
  EGPU_CHECK(hipMalloc(&res.dev[0], 1024 * sizeof(int32_t)));
  EGPU_CHECK(hipMalloc(&res.dev[1], 512));
  EGPU_CHECK(hipMalloc(&res.dev[2], 512));
  hipLaunchKernelGGL(mfma_tile_kernel, dim3(1), dim3(64), 0, 0, pattern, seed, rounds,
                     (int32_t*)res.dev[0], (int8_t*)res.dev[1], (int8_t*)res.dev[2]);
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipDeviceSynchronize());
  EGPU_CHECK(hipMemcpy(d, res.dev[0], 1024 * sizeof(int32_t), hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(a, res.dev[1], 512, hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(b, res.dev[2], 512, hipMemcpyDeviceToHost));
  return 0;
}
