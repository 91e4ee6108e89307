// Compton-y map of a light cone on the device (lightcone.project_planes(on_device=True), process_SLICS.py:55-64): a
// painted float64 plane P (n x n) is added into the y map (res x res) as
//   y += scipy.ndimage.zoom(where(isnan(P), 0, P) * s, res / n, order=3, mode="mirror")
// in float64: cubic B-spline prefilter (gain 6, pole sqrt(3) - 2) under whole-sample symmetric ("mirror") boundaries
// along axis 0, then axis 1, then tensor-product sampling at i (n - 1) / (res - 1) with mirrored taps.  (bp_plane_cut's
// zoom is the half-sample "reflect" one, and a thread per line; this file is neither.)
//
// The prefilter is parallel ALONG the line as well as across lines.  The causal recursion c+[i] = x[i] + z c+[i-1]
// forgets its start as z^k, and |z|^32 = 5e-19: a piece of a line that starts WARM = 32 samples early from c+ = x is
// exact to double precision, and so is the anti-causal recursion c[i] = z (c[i+1] - c+[i]) started 32 samples late
// from its steady state z / (z - 1) c+.  The line is taken as its infinite mirrored extension (indices folded with
// period 2 (n - 1)), of which SciPy's initialisations are the closed-form sums: the line's two ends need no special
// case.  One workgroup stages LINES lines x (WARM + CHUNK + WARM) samples in LDS; a thread owns SUB = 32 consecutive
// samples of one line and runs, with a barrier between the steps,
//   A  the causal warm-up over the 32 samples before its own (input, read only, result in a register)
//   B  the causal recursion over its own samples, in place
//   C  the anti-causal warm-up over the 32 samples after its own (its neighbour's c+, read only)
//   D  the anti-causal recursion over its own samples, in place
// The threads of the last 32 samples (the tail warm-up) stop after B.  Axis 0 stages rows of LINES columns, axis 1
// rows of WARM + CHUNK + WARM columns, transposed into the same LDS layout: global loads and stores run along rows in
// both.  NaN -> 0 and the scale are applied where the first pass loads P.  Lines shorter than WARM go through a thread
// per line with SciPy's exact initialisation.  No atomics anywhere: the same inputs give the same bits.
// Compiled without floating-point contraction, like plane.hip.
#include "common.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RB = 256;
constexpr int WARM = 32;                       // warm-up samples on either side (>= 32: see above)
constexpr int SUB = 32;                        // samples per thread (== WARM: a warm-up is one neighbour's samples)
constexpr int LINES = 32;                      // lines per workgroup
constexpr int NSUB = 8;                        // sub-chunks per workgroup, the tail warm-up included
constexpr int CHUNK = (NSUB - 1) * SUB;        // samples a workgroup finishes per line (224)
constexpr int SPAN = WARM + CHUNK + WARM;      // samples it stages per line (288)
constexpr int PITCH = LINES + 1;               // LDS row pitch in doubles (the transposed fill of axis 1 strides by it)
static_assert(SUB == WARM && CHUNK + WARM == NSUB * SUB, "a thread's warm-up is its neighbour's sub-chunk");

// whole-sample symmetric boundary (SciPy's "mirror"): i mod 2 (n - 1), then 2 (n - 1) - i above n - 1  (n >= 2)
__device__ __forceinline__ int mirror_ws(int i, int n) {
  const int p = 2 * (n - 1);
  int m = i % p;
  if (m < 0) m += p;
  return m >= n ? p - m : m;
}

// One axis of the prefilter for lines of n >= WARM samples.  AXIS 0: line = column, sample = row; AXIS 1: line = row,
// sample = column.  FIRST: src is the plane itself (NaN -> 0, times `scale`), else the previous pass's output.  src
// and dst are n x n row-major and must not alias (a workgroup reads WARM samples into its neighbours' chunks).
template <int AXIS, bool FIRST>
__global__ __launch_bounds__(LINES * NSUB) void prefilter_chunk_kernel(const double* __restrict__ src,
                                                                       double* __restrict__ dst, int n, double scale) {
  __shared__ double s[SPAN * PITCH];
  const int l0 = blockIdx.x * LINES;           // first line
  const int k0 = blockIdx.y * CHUNK - WARM;    // sample index of staged sample 0
  const int tid = threadIdx.x;
  for (int e = tid; e < SPAN * LINES; e += LINES * NSUB) {
    int k, l;
    if (AXIS == 0) { l = e % LINES; k = e / LINES; } else { k = e % SPAN; l = e / SPAN; }
    double v = 0.0;
    if (l0 + l < n) {
      const int m = mirror_ws(k0 + k, n);
      v = AXIS == 0 ? src[(size_t)m * n + (l0 + l)] : src[(size_t)(l0 + l) * n + m];
      if (FIRST) {
        if (isnan(v)) v = 0.0;
        v *= scale;
      }
      v *= 6.0;                                // gain (1 - z) (1 - 1/z)
    }
    s[k * PITCH + l] = v;
  }
  __syncthreads();
  const double z = sqrt(3.0) - 2.0;
  const int l = tid % LINES, g = tid / LINES;  // sub-chunk g owns staged samples [WARM + g SUB, WARM + (g + 1) SUB)
  double* own = s + (WARM + g * SUB) * PITCH + l;
  // A: causal warm-up over the SUB samples before its own
  double prev = own[-WARM * PITCH];
#pragma unroll 8
  for (int i = -WARM + 1; i < 0; ++i) prev = own[i * PITCH] + z * prev;
  __syncthreads();
  // B: causal recursion over its own
#pragma unroll 8
  for (int i = 0; i < SUB; ++i) {
    prev = own[i * PITCH] + z * prev;
    own[i * PITCH] = prev;
  }
  __syncthreads();
  // C: anti-causal warm-up over the SUB samples after its own, from the steady state of a constant c+
  const bool tail = g == NSUB - 1;
  if (!tail) {
    prev = own[(SUB + WARM - 1) * PITCH] * (z / (z - 1.0));
#pragma unroll 8
    for (int i = SUB + WARM - 2; i >= SUB; --i) prev = z * (prev - own[i * PITCH]);
  }
  __syncthreads();
  // D: anti-causal recursion over its own
  if (!tail) {
#pragma unroll 8
    for (int i = SUB - 1; i >= 0; --i) {
      prev = z * (prev - own[i * PITCH]);
      own[i * PITCH] = prev;
    }
  }
  __syncthreads();
  for (int e = tid; e < CHUNK * LINES; e += LINES * NSUB) {
    int k, ll;
    if (AXIS == 0) { ll = e % LINES; k = e / LINES; } else { k = e % CHUNK; ll = e / CHUNK; }
    const int m = k0 + WARM + k;
    if (l0 + ll < n && m < n) {
      const double v = s[(WARM + k) * PITCH + ll];
      if (AXIS == 0) dst[(size_t)m * n + (l0 + ll)] = v; else dst[(size_t)(l0 + ll) * n + m] = v;
    }
  }
}

// Lines of 2 <= n < WARM samples: a thread per line, SciPy's closed-form initialisations.  Element i of line L is
// src[L * ls + i * es]; in place when src == dst (the second pass).
template <bool FIRST>
__global__ __launch_bounds__(WARM) void prefilter_short_kernel(const double* src, double* dst, int n, int ls, int es,
                                                               double scale) {
  const int L = threadIdx.x;
  if (L >= n) return;
  const double* x = src + (size_t)L * ls;
  double* c = dst + (size_t)L * ls;
  for (int i = 0; i < n; ++i) {
    double v = x[i * es];
    if (FIRST) {
      if (isnan(v)) v = 0.0;
      v *= scale;
    }
    c[i * es] = v * 6.0;
  }
  const double z = sqrt(3.0) - 2.0;
  const double zn = pow(z, (double)(n - 1));
  double c0 = c[0] + zn * c[(n - 1) * es], zi = z;
  for (int i = 1; i < n - 1; ++i) {
    c0 += zi * (c[i * es] + zn * c[(n - 1 - i) * es]);
    zi *= z;
  }
  double prev = c0 / (1.0 - zn * zn);
  c[0] = prev;
  for (int i = 1; i < n; ++i) {
    prev = c[i * es] + z * prev;
    c[i * es] = prev;
  }
  prev = (z * c[(n - 2) * es] + prev) * z / (z * z - 1.0);
  c[(n - 1) * es] = prev;
  for (int i = n - 2; i >= 0; --i) {
    prev = z * (prev - c[i * es]);
    c[i * es] = prev;
  }
}

// per-axis taps and weights of output coordinate k.  The coordinate is k times the rounded ratio (n_in - 1) /
// (n_out - 1), as SciPy's zoom forms it (plane.hip's spline_taps divides last: up to an ulp of the coordinate apart)
__device__ __forceinline__ void spline_taps_ws(int k, int n_in, int n_out, int (&idx)[4], double (&w)[4]) {
  const double cc = (double)k * ((double)(n_in - 1) / (double)(n_out - 1));
  const double f = floor(cc), t = cc - f, u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0;
  w[3] = t * t * t / 6.0;
  w[2] = 1.0 - w[0] - w[1] - w[3];
  const int fi = (int)f;
#pragma unroll
  for (int p = 0; p < 4; ++p) idx[p] = mirror_ws(fi - 1 + p, n_in);
}

// y[i][j] += sum_p wi[p] * (sum_q wj[q] * coef[ti[p]][tj[q]]): one thread per pixel of y, each read and written once
__global__ __launch_bounds__(RB) void project_sample_kernel(const double* __restrict__ coef, int n, int res,
                                                            unsigned total, double* __restrict__ y) {
  const unsigned o = blockIdx.x * RB + threadIdx.x;
  if (o >= total) return;
  const unsigned i = o / (unsigned)res, j = o - i * (unsigned)res;
  int ti[4], tj[4];
  double wi[4], wj[4];
  spline_taps_ws((int)i, n, res, ti, wi);
  spline_taps_ws((int)j, n, res, tj, wj);
  double v = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const double* row = coef + (size_t)ti[p] * n;
    double inner = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) inner += wj[q] * row[tj[q]];
    v += wi[p] * inner;
  }
  y[o] += v;
}

}  // namespace

extern "C" {

size_t bp_plane_project_workspace(int32_t n, int32_t res) {
  if (n < 2 || res < 2) return 0;
  return (size_t)2 * n * n * sizeof(double);
}

int bp_plane_project(const double* plane, int32_t rows, int32_t cols, double scale, double* scratch,
                     size_t scratch_bytes, double* y, int32_t res, void* stream) {
  if (!plane || !scratch || !y || rows != cols || rows < 2 || res < 2) return BP_EINVAL;
  const int n = rows;
  if ((int64_t)n * n >= ((int64_t)1 << 31) || (int64_t)res * res >= ((int64_t)1 << 31)) return BP_EUNSUPPORTED;
  if (scratch_bytes < bp_plane_project_workspace(n, res)) return BP_EWORKSPACE;
  const hipStream_t sm = bp_stream(stream);
  double* a = scratch;                          // after the axis-0 pass
  double* b = scratch + (size_t)n * n;          // after the axis-1 pass: the spline coefficients
  const double* coef;
  if (n < WARM) {
    hipLaunchKernelGGL(prefilter_short_kernel<true>, dim3(1), dim3(WARM), 0, sm, plane, a, n, 1, n, scale);
    hipLaunchKernelGGL(prefilter_short_kernel<false>, dim3(1), dim3(WARM), 0, sm, (const double*)a, a, n, n, 1, 0.0);
    coef = a;
  } else {
    const dim3 grid((n + LINES - 1) / LINES, (n + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL((prefilter_chunk_kernel<0, true>), grid, dim3(LINES * NSUB), 0, sm, plane, a, n, scale);
    hipLaunchKernelGGL((prefilter_chunk_kernel<1, false>), grid, dim3(LINES * NSUB), 0, sm, (const double*)a, b, n,
                       0.0);
    coef = b;
  }
  const int64_t total = (int64_t)res * res;
  hipLaunchKernelGGL(project_sample_kernel, dim3((unsigned)((total + RB - 1) / RB)), dim3(RB), 0, sm, coef, n, res,
                     (unsigned)total, y);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

}  // extern "C"
