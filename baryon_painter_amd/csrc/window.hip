// The low-redshift branch of a light cone on the device (lightcone.paint_small_plane(on_device=True),
// process_SLICS.py:149-176): ONE tile is cut with wrap-around from the periodic mass plane, its minimum subtracted where
// asked, resampled to the network's tile with scipy.ndimage.zoom(order=3, mode="mirror"), painted, and the central
// footprint of the painted tile cropped.  Here are the three steps around the paint graph:
//   bp_window_min   the minimum of the wrapped window, in the plane's dtype, left on the device
//   bp_window_zoom  the window (minus that minimum) through spline_ws.hpp's float64 prefilter and sampler, rounded once
//                   to float32: the first pass gathers the wrapped window from the plane as it loads (no float64 copy
//                   of the window is staged), the sampler stores the float32 tile (nothing is zeroed or accumulated)
//   bp_tile_crop    the wrapped crop of the painted float32 tile as float64
// No atomics: the same inputs give the same bits.  Compiled without floating-point contraction, like ymap.hip.
#include "spline_ws.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int MIN_BLOCKS = 256;                // partial minima of stage one (fixed: the scratch is MIN_BLOCKS values)

// i mod n, not negative (np.take(mode="wrap"))
static inline int wrap_host(int64_t i, int n) {
  int64_t m = i % n;
  return (int)(m < 0 ? m + n : m);
}

// pixel (r, c) of the window at (x0, y0) of a periodic rows x cols plane; 0 <= x0 < rows, 0 <= y0 < cols (wrapped on
// the host), r, c < 2^16: the sums fit an unsigned
template <class T> struct Window {
  const T* plane;
  unsigned rows, cols, x0, y0;
  __device__ __forceinline__ T at(int r, int c) const {
    const unsigned pr = (x0 + (unsigned)r) % rows, pc = (y0 + (unsigned)c) % cols;
    return plane[(size_t)pr * cols + pc];
  }
};

// the first pass's load: the wrapped gather, minus the minimum in the plane's dtype, widened
template <class T> struct WindowLoad {
  Window<T> w;
  const T* minimum;                            // device, or nullptr
  __device__ __forceinline__ double operator()(int r, int c) const {
    T v = w.at(r, c);
    if (minimum) v = v - minimum[0];
    return (double)v;
  }
};

// the sampler's store: one rounding to float32
struct TileStore {
  float* out;
  __device__ __forceinline__ void operator()(unsigned o, double v) const { out[o] = (float)v; }
};

// np.min's: a NaN wins
template <class T> __device__ __forceinline__ T min_nan(T a, T b) {
  if (isnan(a)) return a;
  if (isnan(b)) return b;
  return b < a ? b : a;
}

// the minimum of v over the workgroup's RB threads, in thread 0 (tree in LDS, fixed order)
template <class T> __device__ __forceinline__ T block_min(T v, T* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = RB / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] = min_nan(s[threadIdx.x], s[threadIdx.x + h]);
    __syncthreads();
  }
  return s[0];
}

// stage one: workgroup b takes pixels b * RB + t, + gridDim.x * RB, ... of the window; partial[b] its minimum
template <class T>
__global__ __launch_bounds__(RB) void window_min_partial_kernel(Window<T> w, int size, unsigned total,
                                                                T* __restrict__ partial) {
  __shared__ T s[RB];
  const unsigned step = gridDim.x * RB;
  unsigned o = blockIdx.x * RB + threadIdx.x;
  // (every workgroup has a first pixel: the grid is no larger than the window)
  T m = w.at(0, 0);
  for (; o < total; o += step) {
    const unsigned r = o / (unsigned)size;
    m = min_nan(m, w.at((int)r, (int)(o - r * (unsigned)size)));
  }
  m = block_min(m, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// stage two: one workgroup over the `count` <= RB partial minima
template <class T>
__global__ __launch_bounds__(RB) void window_min_final_kernel(const T* __restrict__ partial, int count,
                                                              T* __restrict__ out) {
  __shared__ T s[RB];
  const T m = block_min(partial[(int)threadIdx.x < count ? threadIdx.x : 0], s);
  if (threadIdx.x == 0) out[0] = m;
}

template <class T>
void window_min_launch(const void* plane, int rows, int cols, int x0, int y0, int size, void* scratch, void* out,
                       hipStream_t sm) {
  const Window<T> w{(const T*)plane, (unsigned)rows, (unsigned)cols, (unsigned)x0, (unsigned)y0};
  const int64_t total = (int64_t)size * size;
  const int64_t need = (total + RB - 1) / RB;
  const int blocks = need < MIN_BLOCKS ? (int)need : MIN_BLOCKS;
  hipLaunchKernelGGL(window_min_partial_kernel<T>, dim3(blocks), dim3(RB), 0, sm, w, size, (unsigned)total,
                     (T*)scratch);
  hipLaunchKernelGGL(window_min_final_kernel<T>, dim3(1), dim3(RB), 0, sm, (const T*)scratch, blocks, (T*)out);
}

template <class T>
void window_zoom_launch(const void* plane, int rows, int cols, int x0, int y0, int size, const void* minimum,
                        int tile, double* scratch, float* out, hipStream_t sm) {
  const Window<T> w{(const T*)plane, (unsigned)rows, (unsigned)cols, (unsigned)x0, (unsigned)y0};
  spline_zoom_launch<3>(WindowLoad<T>{w, (const T*)minimum}, size, scratch, TileStore{out}, tile, sm);
}

__global__ __launch_bounds__(RB) void tile_crop_kernel(const float* __restrict__ img, int tile, int r0, int c0, int m,
                                                       unsigned total, double* __restrict__ out) {
  const unsigned o = blockIdx.x * RB + threadIdx.x;
  if (o >= total) return;
  const unsigned i = o / (unsigned)m, j = o - i * (unsigned)m;
  const unsigned r = ((unsigned)r0 + i) % (unsigned)tile, c = ((unsigned)c0 + j) % (unsigned)tile;
  out[o] = (double)img[(size_t)r * tile + c];
}

inline bool dtype_ok(int32_t dtype) { return dtype == BP_F32 || dtype == BP_F64; }
inline bool origin_ok(int32_t v) { return v > -(1 << 30) && v < (1 << 30); }
inline bool square_ok(int32_t n) { return (int64_t)n * n < ((int64_t)1 << 31); }

}  // namespace

extern "C" {

size_t bp_window_min_workspace(void) { return (size_t)MIN_BLOCKS * sizeof(double); }

int bp_window_min(const void* plane, int32_t dtype, int32_t rows, int32_t cols, int32_t x0, int32_t y0, int32_t size,
                  void* scratch, size_t scratch_bytes, void* min_out, void* stream) {
  if (!plane || !scratch || !min_out || rows < 1 || cols < 1 || size < 1 || !dtype_ok(dtype)) return BP_EINVAL;
  if (!square_ok(size) || !origin_ok(x0) || !origin_ok(y0)) return BP_EUNSUPPORTED;
  if (scratch_bytes < bp_window_min_workspace()) return BP_EWORKSPACE;
  const hipStream_t sm = bp_stream(stream);
  const int wx = wrap_host(x0, rows), wy = wrap_host(y0, cols);
  if (dtype == BP_F32) window_min_launch<float>(plane, rows, cols, wx, wy, size, scratch, min_out, sm);
  else window_min_launch<double>(plane, rows, cols, wx, wy, size, scratch, min_out, sm);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

size_t bp_window_zoom_workspace(int32_t size, int32_t tile) {
  if (size < 2 || tile < 2 || !square_ok(size) || !square_ok(tile)) return 0;
  return (size_t)2 * size * size * sizeof(double);
}

int bp_window_zoom(const void* plane, int32_t dtype, int32_t rows, int32_t cols, int32_t x0, int32_t y0, int32_t size,
                   const void* minimum, int32_t tile, double* scratch, size_t scratch_bytes, float* out,
                   void* stream) {
  if (!plane || !scratch || !out || rows < 1 || cols < 1 || size < 2 || tile < 2 || !dtype_ok(dtype)) return BP_EINVAL;
  if (!square_ok(size) || !square_ok(tile) || !origin_ok(x0) || !origin_ok(y0)) return BP_EUNSUPPORTED;
  if (scratch_bytes < bp_window_zoom_workspace(size, tile)) return BP_EWORKSPACE;
  const hipStream_t sm = bp_stream(stream);
  const int wx = wrap_host(x0, rows), wy = wrap_host(y0, cols);
  if (dtype == BP_F32) window_zoom_launch<float>(plane, rows, cols, wx, wy, size, minimum, tile, scratch, out, sm);
  else window_zoom_launch<double>(plane, rows, cols, wx, wy, size, minimum, tile, scratch, out, sm);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_tile_crop(const float* img, int32_t tile, int32_t r0, int32_t c0, int32_t m, double* out, void* stream) {
  if (!img || !out || tile < 1 || m < 1) return BP_EINVAL;
  if (!square_ok(tile) || !square_ok(m) || !origin_ok(r0) || !origin_ok(c0)) return BP_EUNSUPPORTED;
  const int64_t total = (int64_t)m * m;
  hipLaunchKernelGGL(tile_crop_kernel, dim3((unsigned)((total + RB - 1) / RB)), dim3(RB), 0, bp_stream(stream), img,
                     tile, wrap_host(r0, tile), wrap_host(c0, tile), m, (unsigned)total, out);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

}  // extern "C"
