// Shared host-side helpers for libndmps_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/ndmps_hip.h"

namespace ndmps {

void set_error(const char* fmt, ...);

#define NDMPS_CHECK_HIP(expr)                                                        \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      ndmps::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                       __FILE__, __LINE__);                                          \
      return NDMPS_EHIP;                                                             \
    }                                                                                \
  } while (0)

#define NDMPS_REQUIRE(cond, ...)                                                     \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      ndmps::set_error(__VA_ARGS__);                                                 \
      return NDMPS_EINVAL;                                                           \
    }                                                                                \
  } while (0)

#define NDMPS_TRY(expr)                                                              \
  do {                                                                               \
    int _r = (expr);                                                                 \
    if (_r != NDMPS_OK) return _r;                                                   \
  } while (0)

#define NDMPS_LAUNCH_CHECK() NDMPS_CHECK_HIP(hipGetLastError())

static inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
static inline int64_t ceil_div(int64_t x, int64_t a) { return (x + a - 1) / a; }

// bump allocator over a caller-provided device workspace (256-byte aligned pieces); on no memory (p == NULL) take()
// returns NULL and still advances `used`: a carve of Arena(nullptr, 0) is the size query of that carve
struct Arena {
  char* base;
  int64_t size;
  int64_t used;
  Arena(void* p, int64_t n) : base((char*)p), size(n), used(0) {}
  template <typename T>
  T* take(int64_t count) {
    int64_t off = round_up(used, 256);
    int64_t end = off + (int64_t)sizeof(T) * count;
    used = end;
    if (end > size || base == nullptr) return nullptr;
    return (T*)(base + off);
  }
  bool fits() const { return base != nullptr && used <= size; }  // every take() so far returned memory
  int64_t query_bytes() const { return round_up(used, 256) + 256; }  // what a size query answers: room to align the base
};

constexpr int kNumCU = 256;  // MI355X
// workgroups of 256 threads for a grid-stride loop over n elements: at most 8 per CU
static inline int grid1d(int64_t n) {
  const int64_t g = ceil_div(n, 256), cap = (int64_t)kNumCU * 8;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// element conversions of the storage types (fp32, bf16, fp64) to and from the fp64 side of the path
__device__ __forceinline__ double to_f64(float x) { return (double)x; }
__device__ __forceinline__ double to_f64(__bf16 x) { return (double)(float)x; }
__device__ __forceinline__ double to_f64(double x) { return x; }
template <typename T>
__device__ __forceinline__ T from_f64(double x) { return (T)(float)x; }
template <>
__device__ __forceinline__ double from_f64<double>(double x) { return x; }
// element i of an array in the storage type of `code` (0 fp32, 1 bf16, 2 fp64)
__device__ __forceinline__ double load_any(const void* p, int code, int64_t i) {
  if (code == 2) return ((const double*)p)[i];
  if (code == 1) return to_f64(((const __bf16*)p)[i]);
  return to_f64(((const float*)p)[i]);
}
// dst[0 .. n) <- src widened to fp64; src is fp32 (code 0) or bf16 (code 1), both on the device (util.hip)
int widen(const void* src, int code, int64_t n, double* dst, hipStream_t s);

// accumulator of v_mfma_f64_16x16x4_f64
typedef double f64x4 __attribute__((ext_vector_type(4)));

// four consecutive elements as fp32 (16-byte load for fp32 input, 8-byte load for bf16 input)
__device__ __forceinline__ float4 load4_as_f32(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4_as_f32(const __bf16* p) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
// read-once streams: non-temporal (the lines are not kept in the caches in front of data that is read again)
__device__ __forceinline__ float4 load4_stream_f32(const float* p) {
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float4 load4_stream_f32(const __bf16* p) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  const bf16x4 v = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(p));
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

// upper bound of the Gram workspace of a matrix of at most n columns, or of `batch` of them in one launch (gram.hip)
int64_t gram_ws_bound(int64_t n, int batch = 1);

// launch spans for bench.py's roofline (util.hip); slot ids
constexpr int kSpanTridiagColumns = 1;
constexpr int kSpanTridiagTeam = 2;
constexpr int kSpanGram = 3;       // Gram launches that take the device-side turn (a lockstep group's raw Gram); `bytes` = flops
constexpr int kSpanGramSmall = 4;  // every other batched Gram launch; `bytes` = flops
constexpr int kSpanTridiagPanel = 5;   // panel-blocked tridiagonalisation (orders from 1536 on): two launches per column
constexpr int kSpanTridiagTail = 6;    // last 128 columns in LDS + eigenvalues by multi-section (single-workgroup kernels)
constexpr int kSpanEigenVectors = 7;   // inverse iteration, orthonormalisation, back-transformation of the kept vectors
void* span_begin(hipStream_t s);
void span_end(void* begin, hipStream_t s, int slot, int64_t launches, int64_t bytes);

// turns between streams for kernels that fill the GPU alone (util.hip): begin() enqueues the acquire, end() (or the
// destructor, on an early return) the release; the submission of a whole turn is atomic per device
constexpr int kTurnTeam = 0, kTurnGram = 1;
class Turn {
 public:
  Turn(hipStream_t s, int which, unsigned weight = 1, unsigned cap = 1) : s_(s), which_(which), weight_(weight), cap_(cap) {}
  ~Turn();
  Turn(const Turn&) = delete;
  Turn& operator=(const Turn&) = delete;
  int begin();
  int end();

 private:
  hipStream_t s_;
  int which_;
  unsigned weight_, cap_;  // units asked for / units there are
  void* dev_ = nullptr;    // per-device turn state while the turn is open
};

}  // namespace ndmps
