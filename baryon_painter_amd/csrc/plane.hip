// Light-cone planes on the device (lightcone.paint_plane(on_device=True), process_SLICS.py:198-220): the pieces that
// sit on either side of the captured paint graph when a whole periodic plane is painted, so that the plane is uploaded
// once and only the finished plane comes back.
//   bp_plane_cut     wrap-around tile cut of lightcone.get_tile straight into the graph's raw tiles; when the cut is
//                    not the network's tile size, the cubic-spline resampling of scipy.ndimage.zoom(order=3,
//                    mode="reflect") in float64 (prefilter along axis 0, then axis 1; tensor-product sampling)
//   bp_plane_blend   acc += w * p, wsum += w for a batch of painted tiles, tile by tile in tile order, each product
//                    formed in double from the float32 tile (the host loop's order: no atomics, no fused multiply-add)
//   bp_plane_blend_fields  the same for the (n, fields, tile, tile) tiles of a painter with several label fields into
//                    one accumulator plane per field, each field with its own regularisation mask: one launch over
//                    (field, pixel)
//   bp_plane_finish  acc / wsum (0 / 0 = NaN where no tile reaches, as in the reference)
//   bp_tile_outliers the blend's tile statistics and, per tile, how many pixels its regularisation mask zeroes
//   bp_tile_keep     the problematic tiles of a batch (a non-zero count in any field), raw and painted, into a capped
//                    buffer behind a device cursor that also counts the tiles the buffer has no room for
// The whole file is compiled without floating-point contraction: the host expressions these kernels restate round
// every product and every sum separately.
#include "common.hpp"
#include <math.h>

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int RB = 256;

__device__ __forceinline__ int wrap(int i, int n) {
  const int r = i % n;
  return r < 0 ? r + n : r;
}

// half-sample symmetric boundary (SciPy's "reflect"): i mod 2n, then 2n - 1 - i above n
__device__ __forceinline__ int mirror(int i, int n) {
  const int m = wrap(i, 2 * n);
  return m >= n ? 2 * n - 1 - m : m;
}

// cut == tile: a gather, (float) of the plane's value (bit-exact to get_tile + astype(float32))
template <typename T>
__global__ __launch_bounds__(RB) void cut_gather_kernel(const T* plane, int rows, int cols, const int* org, int tile,
                                                        unsigned total, float* out) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  const unsigned tt = (unsigned)tile * (unsigned)tile;
  const unsigned t = i / tt, rc = i - t * tt, r = rc / (unsigned)tile, c = rc - r * (unsigned)tile;
  const int x = wrap(wrap(org[2 * t], rows) + (int)r, rows), y = wrap(wrap(org[2 * t + 1], cols) + (int)c, cols);
  out[i] = (float)plane[(int64_t)x * cols + y];
}

// cut != tile, step 1: the cut as float64, a[t][r][c]
template <typename T>
__global__ __launch_bounds__(RB) void cut_load_kernel(const T* plane, int rows, int cols, const int* org, int cut,
                                                      unsigned total, double* a) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  const unsigned cc = (unsigned)cut * (unsigned)cut;
  const unsigned t = i / cc, rc = i - t * cc, r = rc / (unsigned)cut, c = rc - r * (unsigned)cut;
  const int x = wrap(wrap(org[2 * t], rows) + (int)r, rows), y = wrap(wrap(org[2 * t + 1], cols) + (int)c, cols);
  a[i] = (double)plane[(int64_t)x * cols + y];
}

// step 2 / 4: cubic B-spline prefilter of n_lines lines of n elements, in place.  Line L = (t, j) of a [t][k][j]
// image: element k at a[t * n * n + k * n + j], so the threads of a wave (consecutive j) load consecutive doubles.
// Called on [t][r][c] it filters along axis 0, on the transposed [t][c][r] along axis 1.
__global__ __launch_bounds__(RB) void prefilter_kernel(double* a, int n, unsigned n_lines) {
  const unsigned L = blockIdx.x * RB + threadIdx.x;
  if (L >= n_lines) return;
  const unsigned t = L / (unsigned)n, j = L - t * (unsigned)n;
  double* c = a + (size_t)t * n * n + j;
  const int s = n;
  const double z = sqrt(3.0) - 2.0;
  for (int i = 0; i < n; ++i) c[i * s] *= 6.0;                 // gain (1 - z) (1 - 1/z)
  const double zn = pow(z, (double)n);
  // causal initialisation under half-sample symmetric boundaries
  const double c0 = c[0], cl = c[(n - 1) * s];
  double sum = c0 + zn * cl, zi = z;
  for (int i = 1; i < n; ++i) {
    if (fabs(zi) < 1e-18) break;
    sum += zi * (c[i * s] + zn * c[(n - 1 - i) * s]);
    zi *= z;
  }
  double prev = sum * z / (1.0 - zn * zn) + c0;
  c[0] = prev;
  for (int i = 1; i < n; ++i) {                                // causal pass
    prev = c[i * s] + z * prev;
    c[i * s] = prev;
  }
  prev *= z / (z - 1.0);                                       // anti-causal initialisation
  c[(n - 1) * s] = prev;
  for (int i = n - 2; i >= 0; --i) {                           // anti-causal pass
    prev = z * (prev - c[i * s]);
    c[i * s] = prev;
  }
}

// step 3: b[t][c][r] = a[t][r][c] through LDS, 32 x 32 blocks (reads and writes along rows of 32 doubles)
constexpr int TB = 32;
__global__ __launch_bounds__(TB * 8) void transpose_kernel(const double* a, double* b, int n) {
  __shared__ double s[TB][TB + 1];
  const int t = blockIdx.z, r0 = blockIdx.y * TB, c0 = blockIdx.x * TB;
  const double* src = a + (size_t)t * n * n;
  double* dst = b + (size_t)t * n * n;
  const int tx = threadIdx.x % TB, ty = threadIdx.x / TB;
  for (int k = ty; k < TB; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    if (r < n && c < n) s[k][tx] = src[(size_t)r * n + c];
  }
  __syncthreads();
  for (int k = ty; k < TB; k += 8) {
    const int c = c0 + k, r = r0 + tx;
    if (r < n && c < n) dst[(size_t)c * n + r] = s[tx][k];
  }
}

// per-axis taps and weights of output coordinate k (cc = k (n_in - 1) / (n_out - 1))
__device__ __forceinline__ void spline_taps(int k, int n_in, int n_out, int (&idx)[4], double (&w)[4]) {
  const double cc = (double)k * (double)(n_in - 1) / (double)(n_out - 1);
  const double f = floor(cc), t = cc - f, u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0;
  w[3] = t * t * t / 6.0;
  w[2] = 1.0 - w[0] - w[1] - w[3];
  const int fi = (int)f;
#pragma unroll
  for (int p = 0; p < 4; ++p) idx[p] = mirror(fi - 1 + p, n_in);
}

// step 5: out[t][i][j] = sum_p wi[p] * (sum_q wj[q] * coef(row ti[p], col tj[q])), coefficients as b[t][col][row]
__global__ __launch_bounds__(RB) void zoom_sample_kernel(const double* b, int cut, int tile, unsigned total, float* out) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  const unsigned tt = (unsigned)tile * (unsigned)tile;
  const unsigned t = i / tt, rc = i - t * tt, r = rc / (unsigned)tile, c = rc - r * (unsigned)tile;
  int ti[4], tj[4];
  double wi[4], wj[4];
  spline_taps((int)r, cut, tile, ti, wi);
  spline_taps((int)c, cut, tile, tj, wj);
  const double* bt = b + (size_t)t * cut * cut;
  double v = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    double inner = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) inner += wj[q] * bt[(size_t)tj[q] * cut + ti[p]];
    v += wi[p] * inner;
  }
  out[i] = (float)v;
}

// op(p[k]) for k = threadIdx.x, threadIdx.x + RB, ... < tt in ascending order, the plain strided loop's order; the loads
// of eight strides are issued before the first of them is used (one workgroup walks a whole tile: with one load in
// flight per thread the walk waits out a memory latency per stride)
template <typename Op>
__device__ __forceinline__ void strided(const float* p, int tt, Op op) {
  constexpr int U = 8;
  int k = threadIdx.x;
  for (; k + (U - 1) * RB < tt; k += U * RB) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = p[k + u * RB];
#pragma unroll
    for (int u = 0; u < U; ++u) op(v[u]);
  }
  for (; k < tt; k += RB) op(p[k]);
}

// mean and population standard deviation of one painted tile of tt pixels in float64, by one workgroup of RB threads
// through `red`: a fixed-order reduction (strided partial sums, then a tree over the workgroup).  Every thread returns
// with the same mean and the same sum of squared deviations; the std is sqrt(that / tt).  The one reduction behind the
// blend's masks and the outlier counts
__device__ __forceinline__ void tile_moments(const float* p, int tt, double* red, double& mean, double& ssq) {
  double s = 0.0;
  strided(p, tt, [&](float v) { s += (double)v; });
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = RB / 2; h > 0; h /= 2) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  mean = red[0] / (double)tt;
  __syncthreads();
  s = 0.0;
  strided(p, tt, [&](float v) {
    const double d = (double)v - mean;
    s += d * d;
  });
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = RB / 2; h > 0; h /= 2) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  ssq = red[0];
}

// one workgroup per tile: stats[2t] = mean, stats[2t + 1] = std
__global__ __launch_bounds__(RB) void tile_stats_kernel(const float* tiles, int tt, double* stats) {
  __shared__ double red[RB];
  double mean, ssq;
  tile_moments(tiles + (size_t)blockIdx.x * tt, tt, red, mean, ssq);
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = mean;
    stats[2 * blockIdx.x + 1] = sqrt(ssq / (double)tt);
  }
}

// tile_stats_kernel, and counts[t] = the number of pixels the blend's mask would zero in tile t: the blend's own
// expression on the blend's own mean and std (a NaN anywhere compares false: count 0)
__global__ __launch_bounds__(RB) void tile_outliers_kernel(const float* tiles, int tt, double reg_std, double* stats,
                                                           int* counts) {
  __shared__ double red[RB];
  __shared__ int cnt[RB];
  const float* p = tiles + (size_t)blockIdx.x * tt;
  double mean, ssq;
  tile_moments(p, tt, red, mean, ssq);
  const double sd = sqrt(ssq / (double)tt);
  int c = 0;
  strided(p, tt, [&](float v) {
    if (fabs((double)v - mean) > sd * reg_std) ++c;
  });
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int h = RB / 2; h > 0; h /= 2) {
    if ((int)threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = mean;
    stats[2 * blockIdx.x + 1] = sd;
    counts[blockIdx.x] = cnt[0];
  }
}

// is tile t of the batch problematic: any of its `fields` counts non-zero
__device__ __forceinline__ bool tile_flagged(const int* counts, int fields, int t) {
  for (int f = 0; f < fields; ++f)
    if (counts[(size_t)t * fields + f] != 0) return true;
  return false;
}

// blockIdx.y = tile t of the batch; a problematic tile's rank among the batch's problematic tiles (those before it,
// counted by the workgroup) plus *cursor is its slot; below cap, the blocks of the tile copy its raw tile and its
// painted field tiles there, as V = float4 (16-byte) or float words: items of tt / (sizeof(V) / 4) per image
template <typename V>
__global__ __launch_bounds__(RB) void tile_keep_kernel(const float* raw, const float* painted, const int* counts, int fields,
                                                       int tt, int first_index, int cap, const int* cursor,
                                                       int* kept_index, float* kept_raw, float* kept_painted) {
  __shared__ int cnt[RB];
  const int t = blockIdx.y;
  if (!tile_flagged(counts, fields, t)) return;
  int c = 0;
  for (int u = threadIdx.x; u < t; u += RB) c += tile_flagged(counts, fields, u) ? 1 : 0;
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int h = RB / 2; h > 0; h /= 2) {
    if ((int)threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
    __syncthreads();
  }
  const int64_t slot = (int64_t)*cursor + cnt[0];
  if (slot < 0 || slot >= cap) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) kept_index[slot] = first_index + t;
  constexpr int per = (int)(sizeof(V) / sizeof(float));
  const size_t items = (size_t)tt / per;                     // per image
  const V* sr = reinterpret_cast<const V*>(raw + (size_t)t * tt);
  V* dr = reinterpret_cast<V*>(kept_raw + (size_t)slot * tt);
  const V* sp = reinterpret_cast<const V*>(painted + (size_t)t * fields * tt);
  V* dp = reinterpret_cast<V*>(kept_painted + (size_t)slot * fields * tt);
  const size_t stride = (size_t)gridDim.x * RB;
  for (size_t i = (size_t)blockIdx.x * RB + threadIdx.x; i < items; i += stride) dr[i] = sr[i];
  for (size_t i = (size_t)blockIdx.x * RB + threadIdx.x; i < items * fields; i += stride) dp[i] = sp[i];
}

// behind tile_keep_kernel on the same stream: *cursor += the batch's problematic tiles (one workgroup)
__global__ __launch_bounds__(RB) void tile_keep_advance_kernel(const int* counts, int n, int fields, int* cursor) {
  __shared__ int cnt[RB];
  int c = 0;
  for (int u = threadIdx.x; u < n; u += RB) c += tile_flagged(counts, fields, u) ? 1 : 0;
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int h = RB / 2; h > 0; h /= 2) {
    if ((int)threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *cursor += cnt[0];
}

// one thread per plane pixel of the batch's bounding box [bx0, bx1) x [by0, by1); the covering tiles in tile order
__global__ __launch_bounds__(RB) void blend_kernel(const float* tiles, int n, int tile, const int* dst, int bx0,
                                                   int by0, int bw, unsigned total, const double* weight, int reg,
                                                   double reg_std, const double* stats, double* acc, double* wsum,
                                                   int cols) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  const unsigned ry = i / (unsigned)bw;
  const int x = bx0 + (int)ry, y = by0 + (int)(i - ry * (unsigned)bw);
  const int64_t o = (int64_t)x * cols + y;
  double a = acc[o], s = wsum[o];
  const size_t tt = (size_t)tile * tile;
  for (int t = 0; t < n; ++t) {
    const int lx = x - dst[2 * t], ly = y - dst[2 * t + 1];
    if (lx < 0 || lx >= tile || ly < 0 || ly >= tile) continue;
    const int l = lx * tile + ly;
    const double p = (double)tiles[t * tt + l];
    double w = weight[l];
    if (reg && fabs(p - stats[2 * t]) > stats[2 * t + 1] * reg_std) w = 0.0;
    a += w * p;
    s += w;
  }
  acc[o] = a;
  wsum[o] = s;
}

// blend_kernel for tiles of `fields` label fields, (n, fields, tile, tile): blockIdx.y is the field, whose accumulators
// are plane blockIdx.y of acc / wsum and whose tile t is tiles[t * fields + f] with stats row t * fields + f; per field
// the loop, its order and its arithmetic are blend_kernel's
__global__ __launch_bounds__(RB) void blend_fields_kernel(const float* tiles, int n, int fields, int tile, const int* dst,
                                                          int bx0, int by0, int bw, unsigned total, const double* weight,
                                                          int reg, double reg_std, const double* stats, double* acc,
                                                          double* wsum, int rows, int cols) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  const int f = blockIdx.y;
  const unsigned ry = i / (unsigned)bw;
  const int x = bx0 + (int)ry, y = by0 + (int)(i - ry * (unsigned)bw);
  const int64_t o = (int64_t)f * rows * cols + (int64_t)x * cols + y;
  double a = acc[o], s = wsum[o];
  const size_t tt = (size_t)tile * tile;
  for (int t = 0; t < n; ++t) {
    const int lx = x - dst[2 * t], ly = y - dst[2 * t + 1];
    if (lx < 0 || lx >= tile || ly < 0 || ly >= tile) continue;
    const int l = lx * tile + ly;
    const size_t tf = (size_t)t * fields + f;
    const double p = (double)tiles[tf * tt + l];
    double w = weight[l];
    if (reg && fabs(p - stats[2 * tf]) > stats[2 * tf + 1] * reg_std) w = 0.0;
    a += w * p;
    s += w;
  }
  acc[o] = a;
  wsum[o] = s;
}

__global__ __launch_bounds__(RB) void finish_kernel(const double* acc, const double* wsum, int64_t count, double* out) {
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i < count) out[i] = acc[i] / wsum[i];
}

static inline unsigned nblocks(int64_t total) { return (unsigned)((total + RB - 1) / RB); }

template <typename T>
int plane_cut(const T* plane, int32_t rows, int32_t cols, const int32_t* origins, int32_t n, int32_t cut,
              int32_t tile, double* scratch, size_t scratch_bytes, float* out, hipStream_t sm) {
  if (cut == tile) {
    const int64_t total = (int64_t)n * tile * tile;
    hipLaunchKernelGGL(cut_gather_kernel<T>, dim3(nblocks(total)), dim3(RB), 0, sm, plane, rows, cols, origins, tile,
                       (unsigned)total, out);
    BP_CHECK_LAUNCH();
    return BP_OK;
  }
  // chunks of as many tiles as two float64 images of the cut per tile in the scratch allow
  const size_t per = (size_t)2 * cut * cut * sizeof(double);
  const int chunk = (int)std::min<size_t>(std::min<size_t>((size_t)n, 65535), scratch_bytes / per);   // (grid z)
  if (chunk < 1) return BP_EWORKSPACE;
  double* a = scratch;
  double* b = scratch + (size_t)chunk * cut * cut;
  for (int t0 = 0; t0 < n; t0 += chunk) {
    const int m = std::min(chunk, n - t0);
    const int64_t cells = (int64_t)m * cut * cut;
    hipLaunchKernelGGL(cut_load_kernel<T>, dim3(nblocks(cells)), dim3(RB), 0, sm, plane, rows, cols, origins + 2 * t0,
                       cut, (unsigned)cells, a);
    const unsigned lines = (unsigned)m * (unsigned)cut;
    hipLaunchKernelGGL(prefilter_kernel, dim3(nblocks(lines)), dim3(RB), 0, sm, a, (int)cut, lines);      // axis 0
    const dim3 tg((cut + TB - 1) / TB, (cut + TB - 1) / TB, m);
    hipLaunchKernelGGL(transpose_kernel, tg, dim3(TB * 8), 0, sm, (const double*)a, b, (int)cut);
    hipLaunchKernelGGL(prefilter_kernel, dim3(nblocks(lines)), dim3(RB), 0, sm, b, (int)cut, lines);      // axis 1
    const int64_t px = (int64_t)m * tile * tile;
    hipLaunchKernelGGL(zoom_sample_kernel, dim3(nblocks(px)), dim3(RB), 0, sm, (const double*)b, (int)cut, (int)tile,
                       (unsigned)px, out + (size_t)t0 * tile * tile);
    BP_CHECK_LAUNCH();
  }
  return BP_OK;
}

}  // namespace

extern "C" {

size_t bp_plane_cut_workspace(int32_t n, int32_t cut, int32_t tile) {
  if (n <= 0 || cut <= 0 || cut == tile) return 0;
  return (size_t)2 * n * cut * cut * sizeof(double);
}

int bp_plane_cut(const void* plane, int32_t dtype, int32_t rows, int32_t cols, const int32_t* origins, int32_t n,
                 int32_t cut, int32_t tile, double* scratch, size_t scratch_bytes, float* out, void* stream) {
  if (!plane || !origins || !out || rows <= 0 || cols <= 0 || n <= 0 || cut <= 0 || tile <= 0 ||
      (dtype != BP_F32 && dtype != BP_F64) || (cut != tile && (!scratch || cut < 2 || tile < 2)))
    return BP_EINVAL;
  if ((int64_t)rows * cols >= ((int64_t)1 << 31) || (int64_t)n * tile * tile >= ((int64_t)1 << 31) ||
      (int64_t)n * cut * cut >= ((int64_t)1 << 31))
    return BP_EUNSUPPORTED;
  const hipStream_t sm = bp_stream(stream);
  return dtype == BP_F32
             ? plane_cut(static_cast<const float*>(plane), rows, cols, origins, n, cut, tile, scratch, scratch_bytes, out, sm)
             : plane_cut(static_cast<const double*>(plane), rows, cols, origins, n, cut, tile, scratch, scratch_bytes, out, sm);
}

int bp_plane_blend(const float* tiles, int32_t n, int32_t tile, const int32_t* dst, int32_t bx0, int32_t by0,
                   int32_t bx1, int32_t by1, const double* weight, int32_t regularise, double regularise_std,
                   double* stats, double* acc, double* wsum, int32_t rows, int32_t cols, void* stream) {
  if (!tiles || !dst || !weight || !acc || !wsum || n <= 0 || tile <= 0 || rows <= 0 || cols <= 0 ||
      (regularise && !stats) || bx0 < 0 || by0 < 0 || bx1 > rows || by1 > cols || bx0 >= bx1 || by0 >= by1)
    return BP_EINVAL;
  if ((int64_t)rows * cols >= ((int64_t)1 << 31) || (int64_t)n * tile * tile >= ((int64_t)1 << 31))
    return BP_EUNSUPPORTED;
  const hipStream_t sm = bp_stream(stream);
  if (regularise) {
    hipLaunchKernelGGL(tile_stats_kernel, dim3(n), dim3(RB), 0, sm, tiles, tile * tile, stats);
    BP_CHECK_LAUNCH();
  }
  const int64_t total = (int64_t)(bx1 - bx0) * (by1 - by0);
  hipLaunchKernelGGL(blend_kernel, dim3(nblocks(total)), dim3(RB), 0, sm, tiles, n, tile, dst, bx0, by0, by1 - by0,
                     (unsigned)total, weight, regularise ? 1 : 0, regularise_std, (const double*)stats, acc, wsum,
                     cols);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_plane_blend_fields(const float* tiles, int32_t n, int32_t fields, int32_t tile, const int32_t* dst, int32_t bx0,
                          int32_t by0, int32_t bx1, int32_t by1, const double* weight, int32_t regularise,
                          double regularise_std, double* stats, double* acc, double* wsum, int32_t rows, int32_t cols,
                          void* stream) {
  if (!tiles || !dst || !weight || !acc || !wsum || n <= 0 || fields <= 0 || tile <= 0 || rows <= 0 || cols <= 0 ||
      (regularise && !stats) || bx0 < 0 || by0 < 0 || bx1 > rows || by1 > cols || bx0 >= bx1 || by0 >= by1)
    return BP_EINVAL;
  if ((int64_t)rows * cols >= ((int64_t)1 << 31) || (int64_t)n * fields * tile * tile >= ((int64_t)1 << 31) ||
      fields > 65535)                                                          // (grid y)
    return BP_EUNSUPPORTED;
  const hipStream_t sm = bp_stream(stream);
  if (regularise) {       // a field's tile is a contiguous (tile, tile) image: tile_stats_kernel's row t * fields + f
    hipLaunchKernelGGL(tile_stats_kernel, dim3(n * fields), dim3(RB), 0, sm, tiles, tile * tile, stats);
    BP_CHECK_LAUNCH();
  }
  const int64_t total = (int64_t)(bx1 - bx0) * (by1 - by0);
  hipLaunchKernelGGL(blend_fields_kernel, dim3(nblocks(total), fields), dim3(RB), 0, sm, tiles, n, fields, tile, dst, bx0,
                     by0, by1 - by0, (unsigned)total, weight, regularise ? 1 : 0, regularise_std, (const double*)stats,
                     acc, wsum, rows, cols);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_tile_outliers(const float* tiles, int32_t n_images, int32_t tile, double regularise_std, double* stats,
                     int32_t* counts, void* stream) {
  if (!tiles || !stats || !counts || n_images < 1 || tile < 1 || !(regularise_std >= 0.0) || isinf(regularise_std))
    return BP_EINVAL;
  if ((int64_t)n_images * tile * tile >= ((int64_t)1 << 31)) return BP_EUNSUPPORTED;
  hipLaunchKernelGGL(tile_outliers_kernel, dim3(n_images), dim3(RB), 0, bp_stream(stream), tiles, tile * tile,
                     regularise_std, stats, counts);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_tile_keep(const float* raw, const float* painted, const int32_t* counts, int32_t n, int32_t fields, int32_t tile,
                 int32_t first_index, int32_t cap, int32_t* cursor, int32_t* kept_index, float* kept_raw,
                 float* kept_painted, void* stream) {
  if (!raw || !painted || !counts || !cursor || n < 1 || fields < 1 || tile < 1 || first_index < 0 || cap < 0 ||
      (cap > 0 && (!kept_index || !kept_raw || !kept_painted)))
    return BP_EINVAL;
  if ((int64_t)n * fields * tile * tile >= ((int64_t)1 << 31) || n > 65535 ||                  // (grid y)
      (int64_t)first_index + n >= ((int64_t)1 << 31))
    return BP_EUNSUPPORTED;
  const hipStream_t sm = bp_stream(stream);
  const int tt = tile * tile;
  if (cap > 0) {
    const bool vec = tt % 4 == 0 && ((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(painted) |
                                      reinterpret_cast<uintptr_t>(kept_raw) | reinterpret_cast<uintptr_t>(kept_painted)) &
                                     15) == 0;
    const int64_t items = (int64_t)(vec ? tt / 4 : tt) * fields;
    const dim3 grid((unsigned)std::min<int64_t>((items + RB - 1) / RB, 64), n);
    if (vec)
      hipLaunchKernelGGL(tile_keep_kernel<float4>, grid, dim3(RB), 0, sm, raw, painted, counts, fields, tt, first_index, cap,
                         (const int*)cursor, kept_index, kept_raw, kept_painted);
    else
      hipLaunchKernelGGL(tile_keep_kernel<float>, grid, dim3(RB), 0, sm, raw, painted, counts, fields, tt, first_index, cap,
                         (const int*)cursor, kept_index, kept_raw, kept_painted);
    BP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(tile_keep_advance_kernel, dim3(1), dim3(RB), 0, sm, counts, n, fields, cursor);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_plane_finish(const double* acc, const double* wsum, int64_t count, double* out, void* stream) {
  if (!acc || !wsum || !out || count <= 0) return BP_EINVAL;
  hipLaunchKernelGGL(finish_kernel, dim3(nblocks(count)), dim3(RB), 0, bp_stream(stream), acc, wsum, count, out);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

}  // extern "C"
