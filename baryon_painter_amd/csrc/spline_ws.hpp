// SciPy's spline zoom under whole-sample symmetric ("mirror") boundaries in float64, the kernels that ymap.hip (a painted
// plane into the y map) and window.hip (a window of a mass plane into a raw tile) share: B-spline prefilter (SciPy's
// poles and gain: Spline<ORDER> below) along axis 0, then axis 1, then tensor-product sampling at i (n - 1) / (res - 1)
// with ORDER + 1 mirrored taps per axis.  What differs between the two is where the first pass reads its samples and
// where the sampler leaves its pixels: both are template parameters,
//   Load   double operator()(int r, int c) const     sample (r, c) of the n x n image a pass reads
//   Store  void operator()(unsigned o, double v) const   pixel o = i * res + j of the res x res result
// (CoefLoad below reads the previous pass's output.)
//
// The prefilter is parallel ALONG the line as well as across lines.  The causal recursion c+[i] = x[i] + z c+[i-1]
// forgets its start as z^k: a piece of a line that starts `warm` samples early from c+ = x, |z|^warm <= 1e-18, is
// exact to double precision, and so is the anti-causal recursion c[i] = z (c[i+1] - c+[i]) started `warm` samples late
// from its steady state z / (z - 1) c+.  For the cubic pole |z|^32 = 5e-19.  The line is taken as its infinite mirrored
// extension (indices folded with period 2 (n - 1)), of which SciPy's initialisations are the closed-form sums: the
// line's two ends need no special case.  One workgroup stages LINES lines x (HALO + CHUNK + HALO) samples in LDS; a
// thread owns SUB = 32 consecutive samples of one line and runs per pole, with a barrier between the steps,
//   A  the causal warm-up over the `warm` samples before its own (read only, result in a register)
//   B  the causal recursion over its own samples, in place
//   C  the anti-causal warm-up over the `warm` samples after its own (its neighbours' c+, read only)
//   D  the anti-causal recursion over its own samples, in place
// The threads of the last `warm` samples (the tail warm-up) stop after B.  Orders 4 and 5 have two poles: the second
// runs the same four steps on the first's output, where that is exact, so HALO is the sum of the two warm-ups (see
// Spline<ORDER>).  Axis 0 stages rows of LINES columns, axis 1 rows of SPAN columns, transposed into the same LDS
// layout: global loads and stores run along rows in both.  Lines shorter than SHORT go through a thread per line with
// SciPy's exact initialisation, once per pole.  No atomics anywhere: the same inputs give the same bits.  Compiled
// without floating-point contraction, like plane.hip.
#pragma once
#include "common.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RB = 256;
constexpr int SUB = 32;                        // samples per thread (a warm-up is one or two neighbours' samples)
constexpr int LINES = 32;                      // lines per workgroup
constexpr int CHUNK = 7 * SUB;                 // samples a workgroup finishes per line (224)
constexpr int SHORT = 32;                      // lines shorter than this go through the thread-per-line kernel
constexpr int PITCH = LINES + 1;               // LDS row pitch in doubles (the transposed fill of axis 1 strides by it)

// SciPy's prefilter of a B-spline of degree ORDER (ni_splines.c): POLES poles z, each a causal and an anti-causal
// first-order recursion, behind the gain prod (1 - z) (1 - 1/z).  W1, W2: the warm-up of the first and of the second
// pole in samples, the smallest multiple of SUB with |z|^W <= 1e-18, that is W >= log(1e-18) / log|z|:
//   order 2  z = -0.1716             23.5           -> 32        |z|^32 = 3e-25
//   order 3  z = -0.2679             31.5           -> 32        |z|^32 = 5e-19
//   order 4  z = -0.3613, -0.01373   40.7,  9.7     -> 64, 32    |z|^W  = 5e-29, 3e-60
//   order 5  z = -0.4306, -0.04310   49.2, 13.2     -> 64, 32    |z|^W  = 4e-24, 2e-44
// (32 samples would leave 7e-15 and 2e-12 of the first quartic and quintic pole's start.)  The second pole's warm-up
// must read the first pole's output where that is already exact: of the staged samples [0, SPAN) the first pole's
// causal output is exact on [W1, SPAN), its anti-causal output on [W1, SPAN - W1), the second pole's causal output on
// [W1 + W2, SPAN - W1) and its anti-causal output, the coefficients, on [W1 + W2, SPAN - W1 - W2): HALO = W1 + W2.
template <int ORDER> struct Spline;
template <> struct Spline<2> { static constexpr int POLES = 1, W1 = 32, W2 = 0; };
template <> struct Spline<3> { static constexpr int POLES = 1, W1 = 32, W2 = 0; };
template <> struct Spline<4> { static constexpr int POLES = 2, W1 = 64, W2 = 32; };
template <> struct Spline<5> { static constexpr int POLES = 2, W1 = 64, W2 = 32; };

template <int ORDER> struct Geo {
  using S = Spline<ORDER>;
  static constexpr int HALO = S::W1 + S::W2;             // staged samples on either side of the chunk
  static constexpr int SPAN = HALO + CHUNK + HALO;       // samples staged per line (288; 416 with two poles)
  static constexpr int NSUB = (SPAN - S::W1) / SUB;      // sub-chunks (threads) per line, the tail warm-ups included
  static constexpr int THREADS = LINES * NSUB;           // 256; 352
  static_assert(S::W1 % SUB == 0 && S::W2 % SUB == 0 && CHUNK % SUB == 0, "warm-ups are whole sub-chunks");
  static_assert(SPAN * PITCH * sizeof(double) <= 160 * 1024, "one workgroup's LDS");
};

// pole P (0, 1) of the prefilter of degree ORDER: SciPy's closed forms (get_filter_poles), evaluated in double
template <int ORDER> __device__ __forceinline__ double spline_pole(int p) {
  if (ORDER == 2) return sqrt(8.0) - 3.0;
  if (ORDER == 3) return sqrt(3.0) - 2.0;
  if (ORDER == 4)
    return p == 0 ? sqrt(664.0 - sqrt(438976.0)) + sqrt(304.0) - 19.0 : sqrt(664.0 + sqrt(438976.0)) - sqrt(304.0) - 19.0;
  return p == 0 ? sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25) - 6.5 : sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5;
}

// gain prod (1 - z) (1 - 1/z), SciPy's filter_gain.  The cubic's is 6; rounded as written it comes out an ulp or two
// below, and the order-3 kernels have always multiplied by the literal: they keep it, bit for bit.
template <int ORDER> __device__ __forceinline__ double spline_gain() {
  if (ORDER == 3) return 6.0;
  double g = 1.0;
  for (int p = 0; p < Spline<ORDER>::POLES; ++p) {
    const double z = spline_pole<ORDER>(p);
    g *= (1.0 - z) * (1.0 - 1.0 / z);
  }
  return g;
}

// whole-sample symmetric boundary (SciPy's "mirror"): i mod 2 (n - 1), then 2 (n - 1) - i above n - 1  (n >= 2)
__device__ __forceinline__ int mirror_ws(int i, int n) {
  const int p = 2 * (n - 1);
  int m = i % p;
  if (m < 0) m += p;
  return m >= n ? p - m : m;
}

// Load of the passes behind the first: the previous pass's output, n x n row-major
struct CoefLoad {
  const double* src;
  int n;
  __device__ __forceinline__ double operator()(int r, int c) const { return src[(size_t)r * n + c]; }
};

// Steps A to D of one pole on a thread's sub-chunk `own` (LDS, samples PITCH apart), W its warm-up.  `causal` /
// `anti`: the thread's samples lie where this pole's causal / anti-causal output is exact (all W samples before /
// after them are staged and exact).  Every thread of the workgroup calls it: the barriers are unconditional.
template <int W> __device__ __forceinline__ void pole_steps(double* own, double z, bool causal, bool anti) {
  double prev = 0.0;
  // A: causal warm-up over the W samples before its own
  if (causal) {
    prev = own[-W * PITCH];
#pragma unroll 8
    for (int i = -W + 1; i < 0; ++i) prev = own[i * PITCH] + z * prev;
  }
  __syncthreads();
  // B: causal recursion over its own
  if (causal) {
#pragma unroll 8
    for (int i = 0; i < SUB; ++i) {
      prev = own[i * PITCH] + z * prev;
      own[i * PITCH] = prev;
    }
  }
  __syncthreads();
  // C: anti-causal warm-up over the W samples after its own, from the steady state of a constant c+
  if (anti) {
    prev = own[(SUB + W - 1) * PITCH] * (z / (z - 1.0));
#pragma unroll 8
    for (int i = SUB + W - 2; i >= SUB; --i) prev = z * (prev - own[i * PITCH]);
  }
  __syncthreads();
  // D: anti-causal recursion over its own
  if (anti) {
#pragma unroll 8
    for (int i = SUB - 1; i >= 0; --i) {
      prev = z * (prev - own[i * PITCH]);
      own[i * PITCH] = prev;
    }
  }
  __syncthreads();
}

// One axis of the prefilter for lines of n >= SHORT samples.  AXIS 0: line = column, sample = row; AXIS 1: line = row,
// sample = column.  `load` gives the n x n image this pass reads; dst is n x n row-major and must not be what `load`
// reads (a workgroup reads HALO samples into its neighbours' chunks).
template <int ORDER, int AXIS, class Load>
__global__ __launch_bounds__(Geo<ORDER>::THREADS) void prefilter_chunk_kernel(Load load, double* __restrict__ dst,
                                                                              int n) {
  using S = Spline<ORDER>;
  constexpr int HALO = Geo<ORDER>::HALO, SPAN = Geo<ORDER>::SPAN, THREADS = Geo<ORDER>::THREADS;
  __shared__ double s[SPAN * PITCH];
  const int l0 = blockIdx.x * LINES;           // first line
  const int k0 = blockIdx.y * CHUNK - HALO;    // sample index of staged sample 0
  const int tid = threadIdx.x;
  const double gain = spline_gain<ORDER>();
  for (int e = tid; e < SPAN * LINES; e += THREADS) {
    int k, l;
    if (AXIS == 0) { l = e % LINES; k = e / LINES; } else { k = e % SPAN; l = e / SPAN; }
    double v = 0.0;
    if (l0 + l < n) {
      const int m = mirror_ws(k0 + k, n);
      v = AXIS == 0 ? load(m, l0 + l) : load(l0 + l, m);
      v *= gain;
    }
    s[k * PITCH + l] = v;
  }
  __syncthreads();
  const int l = tid % LINES, g = tid / LINES;
  const int o = S::W1 + g * SUB;               // sub-chunk g owns the staged samples [o, o + SUB)
  double* own = s + o * PITCH + l;
  // (the first pole's causal steps are every thread's: all of [W1, SPAN) has its W1 samples of raw input before it)
  pole_steps<S::W1>(own, spline_pole<ORDER>(0), true, o + SUB + S::W1 <= SPAN);
  if (S::POLES == 2) {
    const bool causal = o >= HALO && o + SUB <= SPAN - S::W1;
    pole_steps<S::W2>(own, spline_pole<ORDER>(1), causal, causal && o + SUB + S::W2 <= SPAN - S::W1);
  }
  for (int e = tid; e < CHUNK * LINES; e += THREADS) {
    int k, ll;
    if (AXIS == 0) { ll = e % LINES; k = e / LINES; } else { k = e % CHUNK; ll = e / CHUNK; }
    const int m = k0 + HALO + k;
    if (l0 + ll < n && m < n) {
      const double v = s[(HALO + k) * PITCH + ll];
      if (AXIS == 0) dst[(size_t)m * n + (l0 + ll)] = v; else dst[(size_t)(l0 + ll) * n + m] = v;
    }
  }
}

// Lines of 2 <= n < SHORT samples: a thread per line, SciPy's closed-form initialisations, pole after pole.  AXIS 0:
// line L is column L (element i at dst[i * n + L]); AXIS 1: line L is row L.  A thread reads element i of its own line
// through `load` right before it writes it, so `load` may read dst itself (the second pass, in place).
template <int ORDER, int AXIS, class Load>
__global__ __launch_bounds__(SHORT) void prefilter_short_kernel(Load load, double* dst, int n) {
  const int L = threadIdx.x;
  if (L >= n) return;
  const int ls = AXIS == 0 ? 1 : n, es = AXIS == 0 ? n : 1;
  double* c = dst + (size_t)L * ls;
  const double gain = spline_gain<ORDER>();
  for (int i = 0; i < n; ++i) {
    const double v = AXIS == 0 ? load(i, L) : load(L, i);
    c[i * es] = v * gain;
  }
  for (int p = 0; p < Spline<ORDER>::POLES; ++p) {
    const double z = spline_pole<ORDER>(p);
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
}

// per-axis taps and weights of output coordinate k.  The coordinate is k times the rounded ratio (n_in - 1) /
// (n_out - 1), as SciPy's zoom forms it (plane.hip's spline_taps divides last: up to an ulp of the coordinate apart).
// ORDER + 1 taps from floor(c) - ORDER / 2 (odd orders) or floor(c + 0.5) - ORDER / 2 (even orders); the weights are
// the centred B-spline of degree ORDER at the tap distances, t the offset from the middle knot (in [0, 1) for odd and
// [-0.5, 0.5) for even orders), the last one (the cubic's third) one minus the others.
template <int ORDER>
__device__ __forceinline__ void spline_taps_ws(int k, int n_in, int n_out, int (&idx)[ORDER + 1],
                                               double (&w)[ORDER + 1]) {
  const double cc = (double)k * ((double)(n_in - 1) / (double)(n_out - 1));
  const double f = (ORDER & 1) ? floor(cc) : floor(cc + 0.5), t = cc - f, u = 1.0 - t;
  if constexpr (ORDER == 2) {
    w[0] = 0.5 * ((0.5 - t) * (0.5 - t));
    w[1] = 0.75 - t * t;
    w[2] = 1.0 - w[0] - w[1];
  } else if constexpr (ORDER == 3) {
    w[0] = u * u * u / 6.0;
    w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0;
    w[3] = t * t * t / 6.0;
    w[2] = 1.0 - w[0] - w[1] - w[3];
  } else if constexpr (ORDER == 4) {
    const double q = t * t, h = (0.5 - t) * (0.5 - t), y = 1.0 + t;
    w[0] = h * h / 24.0;                                                                   // 1.5 <= |x| <= 2.5
    w[1] = y * (y * (y * (5.0 - y) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;              // 0.5 <= |x| <= 1.5
    w[2] = q * (q * 0.25 - 0.625) + 115.0 / 192.0;                                         // |x| <= 0.5
    w[3] = u * (u * (u * (5.0 - u) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
    w[4] = 1.0 - w[0] - w[1] - w[2] - w[3];
  } else {
    const double q = t * t, u2 = u * u, y = 1.0 + t, v = 1.0 + u;
    w[0] = u * u2 * u2 / 120.0;                                                            // 2 <= |x| <= 3
    w[1] = y * (y * (y * (y * (y / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;         // 1 <= |x| <= 2
    w[2] = q * (q * (0.25 - t / 12.0) - 0.5) + 0.55;                                       // |x| <= 1
    w[3] = u2 * (u2 * (0.25 - u / 12.0) - 0.5) + 0.55;
    w[4] = v * (v * (v * (v * (v / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
    w[5] = 1.0 - w[0] - w[1] - w[2] - w[3] - w[4];
  }
  const int fi = (int)f;
#pragma unroll
  for (int p = 0; p <= ORDER; ++p) idx[p] = mirror_ws(fi - ORDER / 2 + p, n_in);
}

// store(o, sum_p wi[p] * (sum_q wj[q] * coef[ti[p]][tj[q]])) for pixel o = i * res + j: one thread per pixel
template <int ORDER, class Store>
__global__ __launch_bounds__(RB) void project_sample_kernel(const double* __restrict__ coef, int n, int res,
                                                            unsigned total, Store store) {
  const unsigned o = blockIdx.x * RB + threadIdx.x;
  if (o >= total) return;
  const unsigned i = o / (unsigned)res, j = o - i * (unsigned)res;
  int ti[ORDER + 1], tj[ORDER + 1];
  double wi[ORDER + 1], wj[ORDER + 1];
  spline_taps_ws<ORDER>((int)i, n, res, ti, wi);
  spline_taps_ws<ORDER>((int)j, n, res, tj, wj);
  double v = 0.0;
#pragma unroll
  for (int p = 0; p <= ORDER; ++p) {
    const double* row = coef + (size_t)ti[p] * n;
    double inner = 0.0;
#pragma unroll
    for (int q = 0; q <= ORDER; ++q) inner += wj[q] * row[tj[q]];
    v += wi[p] * inner;
  }
  store(o, v);
}

// The three launches of one n x n image at one order into a res x res result (arguments checked by the caller):
// scratch holds two float64 images of n x n.  `first` is the image itself, `store` the result.
template <int ORDER, class Load, class Store>
void spline_zoom_launch(Load first, int n, double* scratch, Store store, int res, hipStream_t sm) {
  double* a = scratch;                          // after the axis-0 pass
  double* b = scratch + (size_t)n * n;          // after the axis-1 pass: the spline coefficients
  const double* coef;
  if (n < SHORT) {
    hipLaunchKernelGGL((prefilter_short_kernel<ORDER, 0, Load>), dim3(1), dim3(SHORT), 0, sm, first, a, n);
    hipLaunchKernelGGL((prefilter_short_kernel<ORDER, 1, CoefLoad>), dim3(1), dim3(SHORT), 0, sm, CoefLoad{a, n}, a, n);
    coef = a;
  } else {
    const dim3 grid((n + LINES - 1) / LINES, (n + CHUNK - 1) / CHUNK), block(Geo<ORDER>::THREADS);
    hipLaunchKernelGGL((prefilter_chunk_kernel<ORDER, 0, Load>), grid, block, 0, sm, first, a, n);
    hipLaunchKernelGGL((prefilter_chunk_kernel<ORDER, 1, CoefLoad>), grid, block, 0, sm, CoefLoad{a, n}, b, n);
    coef = b;
  }
  const int64_t total = (int64_t)res * res;
  hipLaunchKernelGGL((project_sample_kernel<ORDER, Store>), dim3((unsigned)((total + RB - 1) / RB)), dim3(RB), 0, sm,
                     coef, n, res, (unsigned)total, store);
}

}  // namespace
