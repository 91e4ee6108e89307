// Ensembles of planes and y maps (lightcone.paint_plane_ensemble / paint_light_cone_ensemble): the moments over K
// blended planes, or over K projected maps, on the device.
//   bp_plane_moments  per element i of `count`: P_k = acc[k][i] / wsum[k][i] (acc[k][i] without wsum), then the
//                     arithmetic of paint_store_moments_kernel (csrc/paint.hip) kept in float64:
//                       S = ((P_0 + P_1) + ...) + P_{K-1},  M = S / K,  Q = ((P_0 - M)^2 + (P_1 - M)^2) + ...,
//                       mean = M,  var = Q / K
//                     -- the population variance in two passes -- and optionally planes[k][i] = P_k.
// One thread owns an element and all its draws: no atomics, no workspace, the same inputs give the same bits.  Up to 16
// quotients stay in registers between the two sums; beyond that they are read and divided a second time, the same
// instructions on the same values.  The kernel streams 2 K + 2 (+ K) doubles per element from and to HBM: two elements
// a thread as 16-byte accesses where every pointer and every draw's row allow it, one otherwise, a grid of at most
// 2048 workgroups striding over the 64-bit count.
// The whole file is compiled without floating-point contraction: every product and every sum is rounded separately.
#include "common.hpp"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int RB = 256;
constexpr int DRAWS_MAX = 64;
constexpr int64_t GRID_MAX = 2048;                              // 256 CUs x 8 workgroups, the rest is strided over

template <int V>
struct Pack;
template <>
struct Pack<1> {
  double v[1];
  __device__ __forceinline__ void load(const double* p) { v[0] = *p; }
  __device__ __forceinline__ void store(double* p) const { *p = v[0]; }
};
template <>
struct Pack<2> {
  double v[2];
  __device__ __forceinline__ void load(const double* p) {
    const double2 t = *reinterpret_cast<const double2*>(p);
    v[0] = t.x;
    v[1] = t.y;
  }
  __device__ __forceinline__ void store(double* p) const { *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]); }
};

// P_k of V consecutive elements at e
template <int V>
__device__ __forceinline__ void quotient(const double* acc, const double* wsum, int64_t at, Pack<V>& p) {
  p.load(acc + at);
  if (wsum) {
    Pack<V> w;
    w.load(wsum + at);
#pragma unroll
    for (int v = 0; v < V; ++v) p.v[v] = p.v[v] / w.v[v];
  }
}

// KMAX > 0: draws <= KMAX, the quotients stay in registers; KMAX == 0: any number of draws, two passes over the inputs
template <int KMAX, int V>
__global__ __launch_bounds__(RB) void plane_moments_kernel(const double* __restrict__ acc, const double* __restrict__ wsum,
                                                           int draws, int64_t count, double* __restrict__ mean,
                                                           double* __restrict__ var, double* __restrict__ planes) {
  const double K = (double)draws;
  const int64_t units = count / V;                              // (V == 2 only where count is even)
  const int64_t step = (int64_t)gridDim.x * RB;
  for (int64_t u = (int64_t)blockIdx.x * RB + threadIdx.x; u < units; u += step) {
    const int64_t e = u * V;
    Pack<V> S, M, Q;
    if constexpr (KMAX > 0) {
      Pack<V> p[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < draws) {
          quotient<V>(acc, wsum, (int64_t)k * count + e, p[k]);
          if (planes) p[k].store(planes + (int64_t)k * count + e);
#pragma unroll
          for (int v = 0; v < V; ++v) S.v[v] = k == 0 ? p[k].v[v] : S.v[v] + p[k].v[v];
        }
      }
#pragma unroll
      for (int v = 0; v < V; ++v) M.v[v] = S.v[v] / K;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < draws) {
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const double d = p[k].v[v] - M.v[v];
            Q.v[v] = k == 0 ? d * d : Q.v[v] + d * d;
          }
        }
      }
    } else {
      Pack<V> p;
      for (int k = 0; k < draws; ++k) {
        quotient<V>(acc, wsum, (int64_t)k * count + e, p);
        if (planes) p.store(planes + (int64_t)k * count + e);
#pragma unroll
        for (int v = 0; v < V; ++v) S.v[v] = k == 0 ? p.v[v] : S.v[v] + p.v[v];
      }
#pragma unroll
      for (int v = 0; v < V; ++v) M.v[v] = S.v[v] / K;
      for (int k = 0; k < draws; ++k) {
        quotient<V>(acc, wsum, (int64_t)k * count + e, p);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const double d = p.v[v] - M.v[v];
          Q.v[v] = k == 0 ? d * d : Q.v[v] + d * d;
        }
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) Q.v[v] = Q.v[v] / K;
    M.store(mean + e);
    Q.store(var + e);
  }
}

template <int V>
void launch(int draws, unsigned blocks, hipStream_t sm, const double* acc, const double* wsum, int64_t count,
            double* mean, double* var, double* planes) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RB), 0, sm, acc, wsum, draws, count, mean, var, planes);
  };
  if (draws <= 4) go(plane_moments_kernel<4, V>);
  else if (draws <= 16) go(plane_moments_kernel<16, V>);
  else go(plane_moments_kernel<0, V>);
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int bp_plane_moments(const double* acc, const double* wsum, int32_t draws, int64_t count, double* mean, double* var,
                     double* planes, void* stream) {
  if (!acc || !mean || !var || draws < 1 || count < 1) return BP_EINVAL;
  if (draws > DRAWS_MAX) return BP_EUNSUPPORTED;
  // an even count keeps row k * count of every draw on the alignment of its base pointer
  const bool wide = count % 2 == 0 && aligned16(acc) && aligned16(mean) && aligned16(var) && (!wsum || aligned16(wsum)) &&
                    (!planes || aligned16(planes));
  const int64_t units = wide ? count / 2 : count;
  const unsigned blocks = (unsigned)std::min<int64_t>((units + RB - 1) / RB, GRID_MAX);
  const hipStream_t sm = bp_stream(stream);
  if (wide) launch<2>(draws, blocks, sm, acc, wsum, count, mean, var, planes);
  else launch<1>(draws, blocks, sm, acc, wsum, count, mean, var, planes);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

}  // extern "C"
