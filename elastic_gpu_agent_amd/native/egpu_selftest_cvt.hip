// Conversion sweep of the GPU self-test (part of libegpu_kernels.so): the
// gfx950 VALU conversions that quantise to and dequantise from the OCP FP8,
// FP6 and FP4 formats, the path every low-precision kernel runs before and
// after a block-scaled MFMA and that no other sweep reaches.
//
//   cvt_selftest_kernel  256 threads = 4 waves per workgroup, so every SIMD of
//                        the CU runs every kind. Per kind and round a lane
//                        generates its source registers, its `old` words and
//                        its scale (selftest_cvt_ref.h: lane_sources), issues
//                        the kind's conversions fully unrolled (32 elements
//                        per lane) and folds the raw result registers with
//                        weights that differ per lane and register. One record
//                        {cu_id, sig[NKINDS]} per wave; inputs are a pure
//                        function of pattern = (blockIdx.x*4 + wave) % 16,
//                        seed and round.
//   cvt_tile_kernel      one wave, one kind, one round: the raw source, old,
//                        scale and result registers of every lane, so a test
//                        can name the wrong lane, register and bit.
//
// Register-only on purpose: no LDS storage (the wave sum is a cross-lane
// shuffle, as in the other sweeps), and the only global access is the store of
// the record (tile: of the registers) at an address that is a function of
// workgroup, wave and lane. The conversions under test are the only float
// instructions: sources and results cross as bit patterns. Every select
// immediate is a compile-time constant. The device only executes the
// instructions; what they must produce is written down in selftest_cvt_ref.h.
// inject_kind corrupts a signature only.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#define EGPU_ST_FN __host__ __device__ inline
#include "selftest_cvt_ref.h"

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

#define EGPU_CVTTEST_VERSION 1
#define EGPU_CVTTEST_MAX_BLOCKS 65536
#define CVT_RECORD_WORDS (1 + EGPU_CVT_NKINDS)
#define CVT_INJECT_NONE (-1)

extern "C" {
struct egpu_cvttest_params {
  int32_t blocks;
  int32_t rounds;
  uint32_t seed;
  int32_t inject_kind;   // -1 = none, else a kind index
  int32_t inject_block;  // workgroup whose signature of that kind is corrupted
};

struct egpu_cvttest_report {
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

namespace cv = egpu_cv;

using cv_s2 = __attribute__((ext_vector_type(2))) short;
using cv_h2 = __attribute__((ext_vector_type(2))) _Float16;
using cv_y2 = __attribute__((ext_vector_type(2))) __bf16;
using cv_f2 = __attribute__((ext_vector_type(2))) float;
using cv_f16 = __attribute__((ext_vector_type(16))) float;
using cv_f32 = __attribute__((ext_vector_type(32))) float;
using cv_u6 = __attribute__((ext_vector_type(6))) uint32_t;

__device__ inline uint32_t cvt_wave_sum(uint32_t v) {
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// body(integral_constant<int, 0>) ... body(integral_constant<int, N - 1>): a
// loop whose index is a constant expression, as the select immediates need.
template <int... I, typename F>
__device__ inline void cvt_each(std::integer_sequence<int, I...>, F&& body) {
  (body(std::integral_constant<int, I>{}), ...);
}
#define CVT_FOR(N, i, ...)                                             \
  cvt_each(std::make_integer_sequence<int, N>{}, [&](auto i##_c) {     \
    constexpr int i = decltype(i##_c)::value;                          \
    __VA_ARGS__                                                        \
  })

template <typename T> __device__ inline uint32_t cvt_bits(T v) { return __builtin_bit_cast(uint32_t, v); }
__device__ inline float cvt_f(uint32_t bits) { return __uint_as_float(bits); }

// Two f32 -> two 8-bit codes into half (i & 1) of old[i].
#define CVT_ENC_WORD(BUILTIN, N, src, old, res)                                              \
  CVT_FOR(N, i, res[i] = cvt_bits(BUILTIN(__builtin_bit_cast(cv_s2, old[i]), cvt_f(src[2 * i]), \
                                          cvt_f(src[2 * i + 1]), scale, (i & 1) != 0));)
// Half (i & 1) of src[i >> 1] -> two f32.
#define CVT_DEC_WORD(BUILTIN, N, src, res)                                 \
  CVT_FOR(N, i, const cv_f2 v = BUILTIN(src[i >> 1], scale, (i & 1) != 0); \
          res[2 * i] = __float_as_uint(v[0]); res[2 * i + 1] = __float_as_uint(v[1]);)

// The conversions of one kind: io's registers in, res out (unused ones zero).
template <int KIND>
__device__ inline void cvt_convert(const cv::lane_io& io, uint32_t res[EGPU_CVT_NRES]) {
  const float scale = cvt_f(io.scale);
  const uint32_t* src = io.src;
  const uint32_t* old = io.old;
#pragma unroll
  for (int i = 0; i < EGPU_CVT_NRES; ++i) res[i] = 0;
  if constexpr (KIND == cv::K_ENC_FP8) {
    CVT_ENC_WORD(__builtin_amdgcn_cvt_scalef32_pk_fp8_f32, 16, src, old, res);
  } else if constexpr (KIND == cv::K_ENC_BF8) {
    CVT_ENC_WORD(__builtin_amdgcn_cvt_scalef32_pk_bf8_f32, 16, src, old, res);
  } else if constexpr (KIND == cv::K_ENC_FP6 || KIND == cv::K_ENC_BF6) {
    cv_f16 a, b;
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = cvt_f(src[j]), b[j] = cvt_f(src[16 + j]);
    cv_u6 r;
    if constexpr (KIND == cv::K_ENC_FP6)
      r = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, scale);
    else
      r = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, scale);
#pragma unroll
    for (int j = 0; j < 6; ++j) res[j] = r[j];
  } else if constexpr (KIND == cv::K_ENC_FP4) {
    CVT_FOR(16, i, res[i] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(
                       old[i], cvt_f(src[2 * i]), cvt_f(src[2 * i + 1]), scale, i & 3););
  } else if constexpr (KIND == cv::K_DEC_FP8) {
    CVT_DEC_WORD(__builtin_amdgcn_cvt_scalef32_pk_f32_fp8, 16, src, res);
  } else if constexpr (KIND == cv::K_DEC_BF8) {
    CVT_DEC_WORD(__builtin_amdgcn_cvt_scalef32_pk_f32_bf8, 16, src, res);
  } else if constexpr (KIND == cv::K_DEC_FP6 || KIND == cv::K_DEC_BF6) {
    cv_u6 s;
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = src[j];
    cv_f32 r;
    if constexpr (KIND == cv::K_DEC_FP6)
      r = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(s, scale);
    else
      r = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(s, scale);
#pragma unroll
    for (int j = 0; j < 32; ++j) res[j] = __float_as_uint(r[j]);
  } else if constexpr (KIND == cv::K_DEC_FP4) {
    CVT_FOR(16, i, const cv_f2 v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(src[i >> 2], scale, i & 3);
            res[2 * i] = __float_as_uint(v[0]); res[2 * i + 1] = __float_as_uint(v[1]););
  } else if constexpr (KIND == cv::K_X16) {
    constexpr int s1 = cv::src_base(KIND, 1), s2 = cv::src_base(KIND, 2), s3 = cv::src_base(KIND, 3);
    constexpr int o1 = cv::old_base(KIND, 1);
    constexpr int r1 = cv::res_base(KIND, 1), r2 = cv::res_base(KIND, 2), r3 = cv::res_base(KIND, 3);
    CVT_FOR(8, i, res[i] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_fp8_f16(
                       __builtin_bit_cast(cv_s2, old[i]), __builtin_bit_cast(cv_h2, src[i]), scale,
                       (i & 1) != 0)););
    CVT_FOR(8, i, res[r1 + i] = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(
                       old[o1 + i], __builtin_bit_cast(cv_y2, src[s1 + i]), scale, i & 3););
    CVT_FOR(8, i, res[r2 + i] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(
                       src[s2 + (i >> 1)], scale, (i & 1) != 0)););
    CVT_FOR(8, i, res[r3 + i] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(
                       src[s3 + (i >> 2)], scale, i & 3)););
  } else {  // K_PLAIN: the unscaled converts
    constexpr int s1 = cv::src_base(KIND, 1), s2 = cv::src_base(KIND, 2), s3 = cv::src_base(KIND, 3),
                  s4 = cv::src_base(KIND, 4);
    constexpr int o1 = cv::old_base(KIND, 1);
    constexpr int r1 = cv::res_base(KIND, 1), r2 = cv::res_base(KIND, 2), r3 = cv::res_base(KIND, 3),
                  r4 = cv::res_base(KIND, 4);
    CVT_FOR(4, i, res[i] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(
                       cvt_f(src[2 * i]), cvt_f(src[2 * i + 1]), (int)old[i], (i & 1) != 0););
    CVT_FOR(4, i, res[r1 + i] = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(
                       cvt_f(src[s1 + 2 * i]), cvt_f(src[s1 + 2 * i + 1]), (int)old[o1 + i],
                       (i & 1) != 0););
    CVT_FOR(4, i, const cv_f2 v = __builtin_amdgcn_cvt_pk_f32_fp8((int)src[s2 + (i >> 1)], (i & 1) != 0);
            res[r2 + 2 * i] = __float_as_uint(v[0]); res[r2 + 2 * i + 1] = __float_as_uint(v[1]););
    CVT_FOR(8, i, res[r3 + i] = __float_as_uint(
                       __builtin_amdgcn_cvt_f32_fp8((int)src[s3 + (i >> 2)], i & 3)););
    CVT_FOR(8, i, res[r4 + i] = __float_as_uint(
                       __builtin_amdgcn_cvt_f32_bf8((int)src[s4 + (i >> 2)], i & 3)););
  }
}

template <int KIND>
__device__ inline uint32_t cvt_sig(uint32_t seed, int pattern, int lane, int rounds) {
  uint32_t sig = 0;
  for (int rd = 0; rd < rounds; ++rd) {
    cv::lane_io io;
    uint32_t res[EGPU_CVT_NRES];
    cv::lane_sources<KIND>(seed, pattern, lane, rd, &io);
    cvt_convert<KIND>(io, res);
    uint32_t s = 0;
#pragma unroll
    for (int reg = 0; reg < EGPU_CVT_NRES; ++reg) s += cv::fold_term(res[reg], lane, reg);
    sig = cv::round_step(sig, cvt_wave_sum(s));
  }
  return sig;
}

__global__ void __launch_bounds__(256)
cvt_selftest_kernel(uint32_t* __restrict__ out, int rounds, uint32_t seed, int inject_kind,
                    int inject_block) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pattern = (blockIdx.x * 4 + wave) % EGPU_CVT_PATTERNS;

  uint32_t hwid, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));

  uint32_t sig[EGPU_CVT_NKINDS];
  sig[cv::K_ENC_FP8] = cvt_sig<cv::K_ENC_FP8>(seed, pattern, lane, rounds);
  sig[cv::K_ENC_BF8] = cvt_sig<cv::K_ENC_BF8>(seed, pattern, lane, rounds);
  sig[cv::K_ENC_FP6] = cvt_sig<cv::K_ENC_FP6>(seed, pattern, lane, rounds);
  sig[cv::K_ENC_BF6] = cvt_sig<cv::K_ENC_BF6>(seed, pattern, lane, rounds);
  sig[cv::K_ENC_FP4] = cvt_sig<cv::K_ENC_FP4>(seed, pattern, lane, rounds);
  sig[cv::K_DEC_FP8] = cvt_sig<cv::K_DEC_FP8>(seed, pattern, lane, rounds);
  sig[cv::K_DEC_BF8] = cvt_sig<cv::K_DEC_BF8>(seed, pattern, lane, rounds);
  sig[cv::K_DEC_FP6] = cvt_sig<cv::K_DEC_FP6>(seed, pattern, lane, rounds);
  sig[cv::K_DEC_BF6] = cvt_sig<cv::K_DEC_BF6>(seed, pattern, lane, rounds);
  sig[cv::K_DEC_FP4] = cvt_sig<cv::K_DEC_FP4>(seed, pattern, lane, rounds);
  sig[cv::K_X16] = cvt_sig<cv::K_X16>(seed, pattern, lane, rounds);
  sig[cv::K_PLAIN] = cvt_sig<cv::K_PLAIN>(seed, pattern, lane, rounds);

  if (lane == 0) {
    uint32_t* rec = out + (size_t)(blockIdx.x * 4 + wave) * CVT_RECORD_WORDS;
    // same encoding as the census: (xcc << 16) | {SE, SH, CU} bits of HW_ID
    rec[0] = (xcc << 16) | ((hwid >> 8) & 0x7F);
#pragma unroll
    for (int k = 0; k < EGPU_CVT_NKINDS; ++k)
      rec[1 + k] = sig[k] ^ (((int)blockIdx.x == inject_block && k == inject_kind) ? 1u : 0u);
  }
}

// Launched with exactly 64 threads. src: 64 x NSRC words, old: 64 x NOLD,
// scale: 64, res: 64 x NRES.
template <int KIND>
__global__ void __launch_bounds__(64)
cvt_tile_kernel(int pattern, uint32_t seed, int round, uint32_t* __restrict__ src,
                uint32_t* __restrict__ old, uint32_t* __restrict__ scale,
                uint32_t* __restrict__ res) {
  const int lane = threadIdx.x & 63;
  cv::lane_io io;
  uint32_t r[EGPU_CVT_NRES];
  cv::lane_sources<KIND>(seed, pattern, lane, round, &io);
  cvt_convert<KIND>(io, r);
#pragma unroll
  for (int i = 0; i < EGPU_CVT_NSRC; ++i) src[EGPU_CVT_NSRC * lane + i] = io.src[i];
#pragma unroll
  for (int i = 0; i < EGPU_CVT_NOLD; ++i) old[EGPU_CVT_NOLD * lane + i] = io.old[i];
  scale[lane] = io.scale;
#pragma unroll
  for (int i = 0; i < EGPU_CVT_NRES; ++i) res[EGPU_CVT_NRES * lane + i] = r[i];
}

// ---------------------------------------------------------------- host side

namespace {

struct CvtResources {
  void* dev = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~CvtResources() {
    if (dev) (void)hipFree(dev);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int cvt_validate(const egpu_cvttest_params* p) {
  if (p == nullptr) EGPU_BAD_ARG("cvttest: params is null");
  if (p->blocks <= 0 || p->blocks > EGPU_CVTTEST_MAX_BLOCKS)
    EGPU_BAD_ARG("cvttest: blocks %d outside [1, %d]", p->blocks, EGPU_CVTTEST_MAX_BLOCKS);
  if (!cv::rounds_ok(p->rounds))
    EGPU_BAD_ARG("cvttest: rounds %d outside [1, %d]", p->rounds, EGPU_CVT_MAX_ROUNDS);
  if (p->inject_kind != CVT_INJECT_NONE) {
    if (!cv::kind_ok(p->inject_kind)) EGPU_BAD_ARG("cvttest: unknown inject_kind %d", p->inject_kind);
    if (p->inject_block < 0 || p->inject_block >= p->blocks)
      EGPU_BAD_ARG("cvttest: inject_block %d is not a workgroup of a %d-block grid",
                   p->inject_block, p->blocks);
  }
  return 0;
}

int cvt_check_point(const char* who, int kind, int pattern, int round) {
  if (!cv::kind_ok(kind)) EGPU_BAD_ARG("%s: unknown kind %d", who, kind);
  if (pattern < 0 || pattern >= EGPU_CVT_PATTERNS)
    EGPU_BAD_ARG("%s: pattern %d outside [0, %d)", who, pattern, EGPU_CVT_PATTERNS);
  if (round < 0 || round >= EGPU_CVT_MAX_ROUNDS)
    EGPU_BAD_ARG("%s: round %d outside [0, %d)", who, round, EGPU_CVT_MAX_ROUNDS);
  return 0;
}

// Runs cvt_selftest_kernel; recs = 4*blocks records of CVT_RECORD_WORDS words.
int cvt_run(const egpu_cvttest_params* p, CvtResources& res, std::vector<uint32_t>& recs, float* ms) {
  const size_t words = (size_t)p->blocks * 4 * CVT_RECORD_WORDS;
  EGPU_CHECK(hipMalloc(&res.dev, words * sizeof(uint32_t)));
  EGPU_CHECK(hipMemset(res.dev, 0xFF, words * sizeof(uint32_t)));
  EGPU_CHECK(hipEventCreate(&res.ev[0]));
  EGPU_CHECK(hipEventCreate(&res.ev[1]));
  EGPU_CHECK(hipEventRecord(res.ev[0], 0));
  const bool inject = p->inject_kind != CVT_INJECT_NONE;
  hipLaunchKernelGGL(cvt_selftest_kernel, dim3(p->blocks), dim3(256), 0, 0, (uint32_t*)res.dev,
                     p->rounds, p->seed, inject ? p->inject_kind : -1, inject ? p->inject_block : -1);
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipEventRecord(res.ev[1], 0));
  EGPU_CHECK(hipEventSynchronize(res.ev[1]));
  EGPU_CHECK(hipEventElapsedTime(ms, res.ev[0], res.ev[1]));
  recs.resize(words);
  EGPU_CHECK(hipMemcpy(recs.data(), res.dev, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

void cvt_add_unique(uint32_t* ids, uint32_t* n, uint32_t cap, uint32_t id) {
  for (uint32_t j = 0; j < *n; ++j)
    if (ids[j] == id) return;
  if (*n < cap) ids[(*n)++] = id;
}

struct cvt_launch_tile {
  int pattern;
  uint32_t seed;
  int round;
  uint32_t *src, *old, *scale, *res;
  template <int KIND> void operator()() {
    hipLaunchKernelGGL(cvt_tile_kernel<KIND>, dim3(1), dim3(64), 0, 0, pattern, seed, round, src, old,
                       scale, res);
  }
};

}  // namespace

// Host reference: out[NKINDS * pattern + kind], 16 patterns. Touches no HIP
// API, so it runs on a machine without a GPU.
extern "C" int egpu_cvttest_expected(uint32_t seed, int rounds, uint32_t* out) {
  if (out == nullptr) EGPU_BAD_ARG("cvttest_expected: out is null");
  if (cv::expected_all(seed, rounds, (uint32_t(*)[EGPU_CVT_NKINDS])out) != 0)
    EGPU_BAD_ARG("cvttest_expected: rounds %d outside [1, %d]", rounds, EGPU_CVT_MAX_ROUNDS);
  return 0;
}

// Host only: what the generator emits for one lane (src: NSRC words, old: NOLD,
// one scale word) and what the reference says the instructions must leave in
// the lane's NRES result registers.
extern "C" int egpu_cvttest_lane_regs(int kind, int pattern, uint32_t seed, int round, int lane,
                                      uint32_t* src, uint32_t* old, uint32_t* scale, uint32_t* res) {
  if (!src || !old || !scale || !res) EGPU_BAD_ARG("cvttest_lane_regs: null output");
  if (int rc = cvt_check_point("cvttest_lane_regs", kind, pattern, round)) return rc;
  if (lane < 0 || lane >= 64) EGPU_BAD_ARG("cvttest_lane_regs: lane %d outside [0, 64)", lane);
  cv::lane_io io;
  cv::lane_reference(kind, seed, pattern, lane, round, &io, res);
  for (int i = 0; i < EGPU_CVT_NSRC; ++i) src[i] = io.src[i];
  for (int i = 0; i < EGPU_CVT_NOLD; ++i) old[i] = io.old[i];
  *scale = io.scale;
  return 0;
}

// Arguments are validated before the first HIP call: a bad argument is an
// error code (-1) on a machine with no GPU too.
extern "C" int egpu_cvttest(int device, const egpu_cvttest_params* p, egpu_cvttest_report* rep) {
  if (rep == nullptr) EGPU_BAD_ARG("cvttest: report is null");
  if (device < 0) EGPU_BAD_ARG("cvttest: device %d is negative", device);
  if (int rc = cvt_validate(p)) return rc;
  *rep = egpu_cvttest_report{};
  rep->version = EGPU_CVTTEST_VERSION;

  std::vector<uint32_t> expected(EGPU_CVT_PATTERNS * EGPU_CVT_NKINDS);
  cv::expected_all(p->seed, p->rounds, (uint32_t(*)[EGPU_CVT_NKINDS])expected.data());

  EGPU_CHECK(hipSetDevice(device));
  CvtResources res;
  std::vector<uint32_t> recs;
  if (int rc = cvt_run(p, res, recs, &rep->kernel_ms)) return rc;

  std::vector<uint32_t> cus(1024);
  uint32_t n_cus = 0;
  for (size_t wv = 0; wv < (size_t)p->blocks * 4; ++wv) {
    const uint32_t* r = &recs[wv * CVT_RECORD_WORDS];
    if (r[0] == 0xFFFFFFFFu) continue;  // record never written
    rep->waves_run++;
    cvt_add_unique(cus.data(), &n_cus, (uint32_t)cus.size(), r[0]);
    const uint32_t* e = &expected[(wv % EGPU_CVT_PATTERNS) * EGPU_CVT_NKINDS];
    uint32_t kinds = 0;
    for (int k = 0; k < EGPU_CVT_NKINDS; ++k)
      if (r[1 + k] != e[k]) kinds |= 1u << k;
    if (kinds) {
      rep->bad_waves++;
      rep->bad_kinds |= kinds;
      cvt_add_unique(rep->bad_cus, &rep->n_bad_cus, 64, r[0]);
    }
  }
  rep->cus_seen = n_cus;
  return 0;
}

// The raw records of one run, CVT_RECORD_WORDS words per wave:
// {cu_id, sig[NKINDS]}. records holds 4*blocks of them.
extern "C" int egpu_cvttest_records(int device, const egpu_cvttest_params* p, uint32_t* records,
                                    int max_records) {
  if (records == nullptr) EGPU_BAD_ARG("cvttest_records: records is null");
  if (device < 0) EGPU_BAD_ARG("cvttest_records: device %d is negative", device);
  if (int rc = cvt_validate(p)) return rc;
  if (max_records < p->blocks * 4)
    EGPU_BAD_ARG("cvttest_records: room for %d records, need %d", max_records, p->blocks * 4);
  EGPU_CHECK(hipSetDevice(device));
  CvtResources res;
  std::vector<uint32_t> recs;
  float ms = 0.f;
  if (int rc = cvt_run(p, res, recs, &ms)) return rc;
  for (size_t i = 0; i < recs.size(); ++i) records[i] = recs[i];
  return 0;
}

// One wave, one kind, one round: the registers of every lane, lane-major.
// src_out: 64 x NSRC words, old_out: 64 x NOLD, scale_out: 64, res_out:
// 64 x NRES (unused registers zero).
extern "C" int egpu_cvttest_tile(int device, int kind, int pattern, uint32_t seed, int round,
                                 uint32_t* src_out, uint32_t* old_out, uint32_t* scale_out,
                                 uint32_t* res_out) {
  if (!src_out || !old_out || !scale_out || !res_out) EGPU_BAD_ARG("cvttest_tile: null output");
  if (device < 0) EGPU_BAD_ARG("cvttest_tile: device %d is negative", device);
  if (int rc = cvt_check_point("cvttest_tile", kind, pattern, round)) return rc;
  EGPU_CHECK(hipSetDevice(device));
  CvtResources res;
  constexpr size_t per_lane = EGPU_CVT_NSRC + EGPU_CVT_NOLD + 1 + EGPU_CVT_NRES;
  const size_t bytes = 64 * per_lane * sizeof(uint32_t);
  EGPU_CHECK(hipMalloc(&res.dev, bytes));
  EGPU_CHECK(hipMemset(res.dev, 0, bytes));
  uint32_t* src = (uint32_t*)res.dev;
  uint32_t* old = src + 64 * EGPU_CVT_NSRC;
  uint32_t* scale = old + 64 * EGPU_CVT_NOLD;
  uint32_t* out = scale + 64;
  cv::for_kind(kind, cvt_launch_tile{pattern, seed, round, src, old, scale, out});
  EGPU_CHECK(hipGetLastError());
  EGPU_CHECK(hipDeviceSynchronize());
  EGPU_CHECK(hipMemcpy(src_out, src, 64 * EGPU_CVT_NSRC * sizeof(uint32_t), hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(old_out, old, 64 * EGPU_CVT_NOLD * sizeof(uint32_t), hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(scale_out, scale, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  EGPU_CHECK(hipMemcpy(res_out, out, 64 * EGPU_CVT_NRES * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}
