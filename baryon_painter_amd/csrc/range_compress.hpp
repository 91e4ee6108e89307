// The six range-compression modes of utils/data_transforms.py (_MODES; the reference's data_transforms.py:72-108) on
// the device: ONE definition, shared by the paint path (paint.hip, scales.hip) and the batch assembly (pointwise.hip,
// scales.hip), so that every surface stores the same bits.
//
// A launch has one mode (a painter has one per field): the mode is a template argument, and the per-tile constants come
// from a record of four float64 the host fills (data_transforms.DeviceRangeCompress.records) -- the device evaluates no
// constant of its own, so both sides share the branch values exactly:
//
//   mode              s              k       c        b
//   RC_SHIFT_LOG      std            k       --       --
//   RC_LOG            std            k       eps      log(eps) / k
//   RC_SHIFT_LOG_2P   std            k[1]    k[0]     --
//   RC_LOG_TANH       std            k       eps      --
//   RC_X_1PX          std            k[0]    k[1]     --
//   RC_INV_X          std * mean * k k       mean     std            (mean: its square root with sqrt_of_mean)
//
// The arithmetic is that of the host lambdas for a float32 tile, Python-float k / eps and np.float64 statistics under
// NumPy 2's promotion rules.  Forward: float32 / float64 promotes, so every operation is float64 and the result is
// rounded to float32 once.  Inverse: a Python float beside a float32 array is rounded to float32 and the operation is
// float32, until the np.float64 std enters; the float32 exp / arctanh are the correctly rounded ones (evaluated in
// double and rounded), as bp_paint_store's exp has always been.  Comparisons are written as np.where takes them: a NaN
// fails `x > 0`.  No floating-point contraction: the host rounds every operation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

enum { RC_SHIFT_LOG = 0, RC_LOG = 1, RC_SHIFT_LOG_2P = 2, RC_LOG_TANH = 3, RC_X_1PX = 4, RC_INV_X = 5, RC_MODES = 6 };

struct RcRec {
  double s, k, c, b;
};

// Where a launch's records lie: `stride` doubles per tile, s and k at `is` / `ik`; c and b (records of four only) at
// 2 and 3.  The two-double {sigma, k} / {k, sigma} tables of the shift-log entry points are read through this too.
struct RcTable {
  const double* p;
  int stride, is, ik;
};

__host__ __device__ static inline RcTable rc_table4(const double* p) { return RcTable{p, 4, 0, 1}; }

__device__ __forceinline__ RcRec rc_record(const RcTable& t, int64_t n) {
  const double* r = t.p + n * t.stride;
  RcRec o{r[t.is], r[t.ik], 0.0, 0.0};
  if (t.stride == 4) { o.c = r[2]; o.b = r[3]; }
  return o;
}

// raw float32 -> transformed float32
template <int M>
__device__ __forceinline__ float rc_forward(const RcRec& r, float xf) {
#pragma clang fp contract(off)
  const double x = (double)xf;
  if (M == RC_SHIFT_LOG) return (float)(log(x / r.s + 1.0) / r.k);
  if (M == RC_LOG) return x > 0.0 ? (float)(log(x / r.s + r.c) / r.k) : (float)r.b;
  if (M == RC_SHIFT_LOG_2P) return (float)(log(x / r.s + r.c) / r.k);
  if (M == RC_LOG_TANH) return x > 0.0 ? (float)tanh(log(x / r.s + r.c) / r.k) : -1.0f;
  if (M == RC_X_1PX) return (float)(x / (x + r.s) * r.k - r.c);
  const double t = x / r.s;                                       // RC_INV_X
  return t > -1.0 ? (float)(2.0 / (t + 1.0) - 1.001) : -1.0f;
}

// The CGAN's "shift-log-cam" map into the tanh range, np.log(x / sigma + 1) / k0 - k1 with a float32 x and float64
// statistics (painter.CGANPainter.transform): evaluated in double, rounded to float32 once.  Not one of the six modes:
// ONE definition all the same, shared by the paint path (paint.hip, bp_paint_load_cam) and the CGAN's batch assembly
// (assemble_gan.hip), so that a tile a painter trains on and the same tile it later paints are the same bits.
__device__ __forceinline__ float rc_shift_log_cam(float xf, double sigma, double k0, double k1) {
#pragma clang fp contract(off)
  return (float)(log((double)xf / sigma + 1.0) / k0 - k1);
}

__device__ __forceinline__ float rc_expf(float t) { return (float)exp((double)t); }   // correctly rounded float32 exp

// float32 activation -> physical value (the float64 the host holds, rounded to float32 once)
template <int M>
__device__ __forceinline__ float rc_inverse(const RcRec& r, float y) {
#pragma clang fp contract(off)
  if (M == RC_SHIFT_LOG) {
    const float e = rc_expf(y * (float)r.k) - 1.0f;
    return (float)((double)e * r.s);
  }
  if (M == RC_LOG) {
    const float e = rc_expf(y * (float)r.k) - (float)r.c;
    return (double)y > r.b ? (float)((double)e * r.s) : 0.0f;     // (float32 > np.float64 compares in float64)
  }
  if (M == RC_SHIFT_LOG_2P) {
    const float e = rc_expf(y * (float)r.k) - (float)r.c;
    return (float)((double)e * r.s);
  }
  if (M == RC_LOG_TANH) {
    if (!(y > -1.0f)) return 0.0f;                                // (np.where(y > -1, ..., 0): a NaN gives 0)
    const float a = (float)atanh((double)y);                      // correctly rounded float32 arctanh
    const float e = rc_expf(a * (float)r.k) - (float)r.c;
    return (float)((double)e * r.s);
  }
  if (M == RC_X_1PX) {
    const float q = (float)r.k / (y + (float)r.c) - 1.0f;
    return (float)(r.s / (double)q);
  }
  const float q = 2.0f / (y + 1.001f) - 1.0f;                     // RC_INV_X: ((q * std) * mean) * k, the host's order
  return y >= -1.0f ? (float)((double)q * r.b * r.c * r.k) : 0.0f;
}

// f(std::integral_constant<int, mode>) for a valid mode; false (nothing called) otherwise
template <class F>
static inline bool rc_dispatch(int mode, F&& f) {
  switch (mode) {
    case RC_SHIFT_LOG: f(std::integral_constant<int, RC_SHIFT_LOG>{}); return true;
    case RC_LOG: f(std::integral_constant<int, RC_LOG>{}); return true;
    case RC_SHIFT_LOG_2P: f(std::integral_constant<int, RC_SHIFT_LOG_2P>{}); return true;
    case RC_LOG_TANH: f(std::integral_constant<int, RC_LOG_TANH>{}); return true;
    case RC_X_1PX: f(std::integral_constant<int, RC_X_1PX>{}); return true;
    case RC_INV_X: f(std::integral_constant<int, RC_INV_X>{}); return true;
    default: return false;
  }
}
