// Split-scale (Gaussian pyramid) transform on the device (utils/data_transforms.py: create_split_scale_transform, the
// reference's data_transforms.py:14-42), for multi-scale painters on the paint path:
//   bp_split_scale         n float32 tiles (n, h, w) -> their pyramids in `levels` channels of an NHWC view
//   bp_paint_load_scales2  bp_paint_load2 with the pyramid between the shift-log transform and the layout
//   bp_paint_store_scales  bp_paint_store for a `levels`-channel head: the inverse of the pyramid (channel 0, or the
//                          float32 sum of the channels in channel order), then the inverse shift-log
//   bp_tile_minima         per-tile minimum of a gathered training tile (the datasets' subtract_minimum)
//   bp_gather_tiles_scales bp_gather_tiles [minus the minima] with the pyramid behind the transform, stored as NCHW
//                          planes: a training batch of a multi-scale model, assembled from the stacks in HBM
//   bp_paint_load_scales2_mode / bp_paint_store_scales_mode / bp_gather_tiles_scales_mode   the same three with any of
//                          the six range-compression modes (range_compress.hpp) and records of four float64 per tile
// The pyramid: d = x; for i = n_scale-1 .. 1: g = gaussian_filter(d, sigma_i); scale i = g; d -= g; scale 0 = d; with
// include_original a leading channel holds x.  What scipy.ndimage.gaussian_filter does on a float32 tile is the
// contract, restated here:
//   * weights exp(-0.5 k^2 / sigma^2), k = -r .. r, divided by their float64 sum, r = int(truncate * sigma + 0.5):
//     computed on the host with SciPy's expression and read from device memory as float64, one radius per level;
//   * axis 0 is filtered first, then axis 1;
//   * each axis accumulates in float64 and is rounded to float32 once;
//   * boundary mode "reflect" (d c b a | a b c d), applied repeatedly when r exceeds the line: index reflection with
//     period 2n;
//   * the subtraction d -= g is a float32 subtraction.
// The float64 sums are formed tap by tap from k = -r upwards with fused multiply-adds (SciPy pairs the symmetric taps):
// they differ from SciPy's by float64 rounding, 2^-29 of a float32 ulp, which moves a float32 result only when the sum
// lies that close to a rounding boundary.
// Layout of the work: per filtered level two launches.  The axis-0 pass stages a strip of 64 columns x (64 + 2r) rows,
// the reflected halo folded while staging, in LDS and writes the float32 intermediate to the caller's scratch; the
// axis-1 pass stages whole rows of that intermediate with their reflected halo in LDS, rounds, subtracts, and writes
// the level's channel straight into the view(s) -- the last level's pass writes the residual, the original and the aux
// planes with it, so a pixel's channels are written by two launches, not by one per channel.  No atomics, no host
// synchronisation; every launch can be captured.  Except for the explicit fma of the filter sums the file is compiled
// without floating-point contraction (the host expressions round every operation).
// The training batch (bp_gather_tiles_scales) gathers inside the axis-0 pass of the coarsest level: the staged strip is
// made of gathered, transformed pixels (assemble.hpp: bp_gather_tiles' expression), so the stacks are read once and the
// transformed tile is written once, for the residual and the original, beside the axis-0 intermediate.
#include "common.hpp"
#include "assemble.hpp"
#include "range_compress.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RB = 256;
constexpr int CW = 64;          // axis-0 pass: columns per workgroup (one per lane)
constexpr int CH = 64;          // ... and output rows per workgroup
constexpr int RROWS = 4;        // axis-1 pass: rows per workgroup (one per wave)
constexpr int MAX_SCALES = 16;
constexpr size_t LDS_MAX = 65536;

// half-sample symmetric boundary (SciPy's "reflect"), any distance: i mod 2n, then 2n - 1 - i above n
__device__ __forceinline__ int fold(int i, int n) {
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m >= n ? 2 * n - 1 - m : m;
}

struct Dst {
  float* p;       // nullptr: no such destination
  int cs, co;     // NHWC view: channel stride and offset; NCHW planes: channels per sample and first channel
};

// what bp_gather_tiles reads, the optional minima, and where the transformed tile goes
struct GatherArgs {
  const TileDesc* d100;
  const TileDesc* d150;
  const SampleXform* xf;
  const float* minima;  // nullptr: nothing is subtracted
  float* v;             // (n, t, t): the transformed tile
  const double* rec;    // M >= 0: (n, 4) records of range_compress.hpp's mode M, applied in place of xf's transform
};

constexpr int XF_OWN = -1;      // the gather kernels' M: the transform the SampleXform itself names (bp_gather_tiles')

// one sample's share of GatherArgs, wave-uniform
template <int M>
struct Gathered {
  TileDesc a, b;
  SampleXform x;
  RcRec rc;
  float mn;
  bool sub;
  __device__ __forceinline__ Gathered(const GatherArgs& g, int n)
      : a(g.d100[n]), b(g.d150[n]), x(g.xf[n]), rc{}, mn(g.minima ? g.minima[n] : 0.f), sub(g.minima != nullptr) {
    if constexpr (M >= 0) rc = rc_record(rc_table4(g.rec), n);
  }
  // bp_gather_tiles' value with the float32 `d - d.min()` of datasets.py:402 in front of the transform
  __device__ __forceinline__ float at(int r, int c) const {
    float s = tile_scale(tile_sum(a, b, r, c), x);
    if (sub) s = s - mn;
    if constexpr (M >= 0) return rc_forward<M>(rc, s);
    else return tile_transform(s, x);
  }
};

// raw (n, 1, h, w) -> the float32 transformed value of bp_paint_load, e.g. (float) (log((double) x / sigma + 1) / k)
template <int M>
__global__ __launch_bounds__(RB) void transform_kernel(const float* raw, RcTable xf, unsigned hw, unsigned total,
                                                       float* v) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  v[i] = rc_forward<M>(rc_record(xf, i / hw), raw[i]);
}

// axis 0: tmp[t][y][x] = (float) sum_k wgt[k + r] * src[t][fold(y + k)][x]
__global__ __launch_bounds__(RB) void filter_axis0_kernel(const float* src, float* tmp, const double* wgt, int r, int h,
                                                          int w) {
  extern __shared__ float lds[];                         // (CH + 2r) rows of CW columns
  const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
  const int x = blockIdx.x * CW + tx, y0 = blockIdx.y * CH;
  const size_t base = (size_t)blockIdx.z * h * w;
  const int rows = min(CH, h - y0);
  const bool col_ok = x < w;
  for (int rr = ty; rr < rows + 2 * r; rr += RB / CW)
    lds[rr * CW + tx] = col_ok ? src[base + (size_t)fold(y0 - r + rr, h) * w + x] : 0.f;
  __syncthreads();
  if (!col_ok) return;
  for (int oy = ty; oy < rows; oy += RB / CW) {
    const float* p = lds + oy * CW + tx;
    double acc = 0.0;
    for (int k = 0; k <= 2 * r; ++k) acc = fma(wgt[k], (double)p[k * CW], acc);
    tmp[base + (size_t)(y0 + oy) * w + x] = (float)acc;
  }
}

// The same pass with the gather in front: the strip is staged from the stacks, and the rows a workgroup owns are
// written to g.v as well (the tile the level's residual and the original are taken from).
template <int M>
__global__ __launch_bounds__(RB) void gather_axis0_kernel(GatherArgs g, float* tmp, const double* wgt, int r, int t) {
  extern __shared__ float lds[];                         // (CH + 2r) rows of CW columns
  const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
  const int x = blockIdx.x * CW + tx, y0 = blockIdx.y * CH;
  const size_t base = (size_t)blockIdx.z * t * t;
  const int rows = min(CH, t - y0);
  const bool col_ok = x < t;
  const Gathered<M> src(g, blockIdx.z);
  for (int rr = ty; rr < rows + 2 * r; rr += RB / CW) {
    float val = 0.f;
    if (col_ok) {
      const int y = fold(y0 - r + rr, t);
      val = src.at(y, x);
      if (rr >= r && rr < r + rows) g.v[base + (size_t)y * t + x] = val;      // y = y0 + rr - r: each pixel once
    }
    lds[rr * CW + tx] = val;
  }
  __syncthreads();
  if (!col_ok) return;
  for (int oy = ty; oy < rows; oy += RB / CW) {
    const float* p = lds + oy * CW + tx;
    double acc = 0.0;
    for (int k = 0; k <= 2 * r; ++k) acc = fma(wgt[k], (double)p[k * CW], acc);
    tmp[base + (size_t)(y0 + oy) * t + x] = (float)acc;
  }
}

// n_scale = 1: the gathered tile itself, (n, 1 + inc, t, t) planes (with include_original the tile twice)
template <int M>
__global__ __launch_bounds__(RB) void gather_planes_kernel(GatherArgs g, float* out, int t, int inc, unsigned total) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  const unsigned hw = (unsigned)t * (unsigned)t, n = i / hw, yx = i % hw;
  const Gathered<M> src(g, n);
  const float val = src.at(yx / t, yx % t);
  for (int ch = 0; ch <= inc; ++ch) out[((size_t)n * (1 + inc) + ch) * hw + yx] = val;
}

// minimum of a tile as bp_gather_tiles sums and scales it, NaN if the tile holds one (np.min): one workgroup per
// tile, lanes -> waves (DPP shuffles) -> LDS, combined in wave order.  min is exact, so any order gives the same bits.
__global__ __launch_bounds__(RB) void tile_min_kernel(const TileDesc* d100, const TileDesc* d150, const SampleXform* xf,
                                                      int t, float* minima) {
  __shared__ float sm[RB / 64];
  __shared__ int sn[RB / 64];
  const int n = blockIdx.x;
  const TileDesc a = d100[n], b = d150[n];
  const SampleXform x = xf[n];
  float m = INFINITY;
  int nan = 0;
  for (int i = threadIdx.x; i < t * t; i += RB) {
    const float s = tile_scale(tile_sum(a, b, i / t, i % t), x);
    nan |= s != s;
    m = fminf(m, s);                                     // (skips a NaN: `nan` remembers it)
  }
  for (int off = 32; off > 0; off >>= 1) {
    m = fminf(m, __shfl_xor(m, off));
    nan |= __shfl_xor(nan, off);
  }
  if (threadIdx.x % 64 == 0) { sm[threadIdx.x / 64] = m; sn[threadIdx.x / 64] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < RB / 64; ++w) { m = fminf(m, sm[w]); nan |= sn[w]; }
    minima[n] = nan ? __builtin_nanf("") : m;
  }
}

struct RowArgs {
  const float* tmp;     // the axis-0 result
  const float* dsrc;    // the residual this level was filtered from
  float* dres;          // where the next residual goes (not the last level)
  const float* orig;    // x itself (last level with include_original)
  const float* aux;     // (n, caux) (last level)
  const double* wgt;
  int r, h, w, rows_total, caux;
  int ch_g;             // channel of this level's g
  int ch_res;           // channel of the residual (scale 0); < 0: not the last level
  int ch_orig;          // channel of the original; < 0: none
  int ch_aux;           // first aux channel
  Dst d0, d1;
};

// PL = false: channel ch of pixel `pixel` of an NHWC view; PL = true: plane ch of (n, d.cs, h, w) NCHW planes
template <bool PL>
__device__ __forceinline__ void put(const Dst& d, size_t pixel, size_t hw, int ch, float v) {
  if (!d.p) return;
  if (PL) d.p[(pixel / hw * d.cs + d.co + ch) * hw + pixel % hw] = v;
  else d.p[pixel * d.cs + d.co + ch] = v;
}

// what the last launch writes besides its own g: the residual, the original and the aux planes of a pixel
template <bool PL>
__device__ __forceinline__ void put_tail(const RowArgs& a, size_t pixel, int n, float res) {
  const size_t hw = (size_t)a.h * a.w;
  put<PL>(a.d0, pixel, hw, a.ch_res, res);
  put<PL>(a.d1, pixel, hw, a.ch_res, res);
  if (a.ch_orig >= 0) {
    const float o = a.orig[pixel];
    put<PL>(a.d0, pixel, hw, a.ch_orig, o);
    put<PL>(a.d1, pixel, hw, a.ch_orig, o);
  }
  for (int c = 0; c < a.caux; ++c) {
    const float v = a.aux[(size_t)n * a.caux + c];
    put<PL>(a.d0, pixel, hw, a.ch_aux + c, v);
    put<PL>(a.d1, pixel, hw, a.ch_aux + c, v);
  }
}

// axis 1: g = (float) sum_k wgt[k + r] * tmp[row][fold(x + k)]; residual = dsrc - g (float32)
template <bool PL>
__global__ __launch_bounds__(RB) void filter_axis1_kernel(RowArgs a) {
  extern __shared__ float lds[];                         // RROWS rows of w + 2r floats
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int row = blockIdx.x * RROWS + wave;             // row of the (n * h, w) image stack
  const int span = a.w + 2 * a.r;
  float* line = lds + wave * span;
  const bool row_ok = row < a.rows_total;
  if (row_ok)
    for (int j = lane; j < span; j += 64) line[j] = a.tmp[(size_t)row * a.w + fold(j - a.r, a.w)];
  __syncthreads();
  if (!row_ok) return;
  const int n = row / a.h;
  for (int x = lane; x < a.w; x += 64) {
    const float* p = line + x;
    double acc = 0.0;
    for (int k = 0; k <= 2 * a.r; ++k) acc = fma(a.wgt[k], (double)p[k], acc);
    const float g = (float)acc;
    const size_t pixel = (size_t)row * a.w + x;
    const float res = a.dsrc[pixel] - g;
    put<PL>(a.d0, pixel, (size_t)a.h * a.w, a.ch_g, g);
    put<PL>(a.d1, pixel, (size_t)a.h * a.w, a.ch_g, g);
    if (a.ch_res >= 0) put_tail<PL>(a, pixel, n, res);
    else a.dres[pixel] = res;
  }
}

// n_scale = 1: nothing is filtered, the residual is the tile
__global__ __launch_bounds__(RB) void emit_kernel(RowArgs a, unsigned total) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  put_tail<false>(a, i, (int)(i / ((unsigned)a.h * (unsigned)a.w)), a.dsrc[i]);
}

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

template <int M>
__global__ __launch_bounds__(RB) void paint_store_scales_kernel(const float* src, int src_cs, int src_co, int c, PW pw,
                                                                int softplus, int include_original, RcTable xf,
                                                                float* dst, unsigned hw, unsigned total) {
  const unsigned i = blockIdx.x * RB + threadIdx.x;      // (n, 1, H, W) destination index
  if (i >= total) return;
  const unsigned n = i / hw;
  const float* s = src + (size_t)i * src_cs + src_co;
  const int used = include_original ? 1 : c;
  float v = 0.f;
  for (int ch = 0; ch < used; ++ch) {
    float t = pw_apply(pw, ch, s[ch]);
    if (softplus) t = softplus_f(t);
    v = ch == 0 ? t : v + t;                             // ((c0 + c1) + c2) ...: NumPy's order for sum(axis=0)
  }
  // bp_paint_store's expression, e.g. (np.exp(x * k) - 1) * std: float32 product, float32 exp, float32 subtraction,
  // double product
  dst[i] = rc_inverse<M>(rc_record(xf, n), v);
}

static inline unsigned nblocks(int64_t total) { return (unsigned)((total + RB - 1) / RB); }

// BP_OK if the pyramid of (n, h, w) tiles with these radii has a launch form here
int check_levels(int32_t n, int32_t h, int32_t w, int32_t n_scale, const double* weights, const int32_t* radii,
                 int64_t channels) {
  if (n <= 0 || h <= 0 || w <= 0 || n_scale < 1) return BP_EINVAL;
  if (n_scale > 1 && (!weights || !radii)) return BP_EINVAL;
  for (int i = 1; i < n_scale; ++i)
    if (radii[i] < 0) return BP_EINVAL;
  if (n_scale > MAX_SCALES || n > 65535 || (int64_t)n * h * w * channels >= ((int64_t)1 << 31)) return BP_EUNSUPPORTED;
  for (int i = 1; i < n_scale; ++i) {
    const int64_t r = radii[i];
    if ((CH + 2 * r) * CW * sizeof(float) > LDS_MAX || (w + 2 * r) * RROWS * sizeof(float) > LDS_MAX)
      return BP_EUNSUPPORTED;
  }
  return BP_OK;
}

// f(std::integral_constant<int, M>) for the gather kernels' M: XF_OWN or a range-compression mode
template <class F>
inline bool gather_dispatch(int gmode, F&& f) {
  if (gmode == XF_OWN) { f(std::integral_constant<int, XF_OWN>{}); return true; }
  return rc_dispatch(gmode, f);
}

// x (n, h, w) float32 planar -> pyramid channels [0, levels) of d0 (and d1), aux planes behind them.  `tmp` and `d`
// are planes of n * h * w floats.  With `ga` (square tiles, n_scale > 1) x is ga->v, which the first axis-0 pass gathers
// and writes itself, and d0 / d1 are NCHW planes.
int pyramid(const float* x, int32_t n, int32_t h, int32_t w, int32_t n_scale, int inc, const double* weights,
            const int32_t* radii, float* tmp, float* d, const float* aux, int caux, Dst d0, Dst d1, hipStream_t sm,
            const GatherArgs* ga = nullptr, int gmode = XF_OWN) {
  RowArgs a{};
  a.h = h; a.w = w; a.rows_total = n * h; a.caux = caux; a.aux = aux;
  a.d0 = d0; a.d1 = d1;
  a.ch_aux = n_scale + inc;
  const int64_t total = (int64_t)n * h * w;
  if (n_scale == 1) {
    a.dsrc = x; a.orig = x; a.ch_res = inc; a.ch_orig = inc ? 0 : -1;
    hipLaunchKernelGGL(emit_kernel, dim3(nblocks(total)), dim3(RB), 0, sm, a, (unsigned)total);
    BP_CHECK_LAUNCH();
    return BP_OK;
  }
  size_t woff[MAX_SCALES + 1] = {0, 0};
  for (int i = 1; i < n_scale; ++i) woff[i + 1] = woff[i] + 2 * (size_t)radii[i] + 1;
  const float* cur = x;
  for (int i = n_scale - 1; i >= 1; --i) {
    const int r = radii[i];
    const double* wg = weights + woff[i];
    const dim3 g0((w + CW - 1) / CW, (h + CH - 1) / CH, n);
    if (ga && cur == x)
      gather_dispatch(gmode, [&](auto m) {
        gather_axis0_kernel<decltype(m)::value><<<g0, dim3(RB), (size_t)(CH + 2 * r) * CW * sizeof(float), sm>>>(
            *ga, tmp, wg, r, (int)h);
      });
    else
      hipLaunchKernelGGL(filter_axis0_kernel, g0, dim3(RB), (size_t)(CH + 2 * r) * CW * sizeof(float), sm, cur, tmp, wg,
                         r, (int)h, (int)w);
    a.tmp = tmp; a.dsrc = cur; a.wgt = wg; a.r = r; a.ch_g = inc + i;
    const bool last = i == 1;
    a.dres = last ? nullptr : d;
    a.ch_res = last ? inc : -1;
    a.ch_orig = last && inc ? 0 : -1;
    a.orig = x;
    hipLaunchKernelGGL(ga ? filter_axis1_kernel<true> : filter_axis1_kernel<false>, dim3((n * h + RROWS - 1) / RROWS),
                       dim3(RB), (size_t)(w + 2 * r) * RROWS * sizeof(float), sm, a);
    BP_CHECK_LAUNCH();
    cur = d;
  }
  return BP_OK;
}

}  // namespace

extern "C" {

size_t bp_split_scale_workspace(int32_t n, int32_t h, int32_t w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)3 * n * h * w * sizeof(float);     // axis-0 intermediate, residual, transformed tile
}

int bp_split_scale(const float* tiles, int32_t n, int32_t h, int32_t w, int32_t n_scale, int32_t include_original,
                   const double* weights, const int32_t* radii, void* scratch, size_t scratch_bytes, const bp_view* out,
                   void* stream) {
  const int inc = include_original ? 1 : 0;
  if (!tiles || !bp_view_ok_any(out) || n_scale < 1 || out->c != n_scale + inc || out->n != n || out->h != h ||
      out->w != w)
    return BP_EINVAL;
  if (out->dtype != BP_F32) return BP_EUNSUPPORTED;
  const int rc = check_levels(n, h, w, n_scale, weights, radii, out->cstride);
  if (rc != BP_OK) return rc;
  if (n_scale > 1 && (!scratch || scratch_bytes < bp_split_scale_workspace(n, h, w))) return BP_EWORKSPACE;
  float* s = static_cast<float*>(scratch);
  const size_t plane = (size_t)n * h * w;
  return pyramid(tiles, n, h, w, n_scale, inc, weights, radii, s, s ? s + plane : nullptr, nullptr, 0,
                 Dst{out->ptr, out->cstride, out->coff}, Dst{nullptr, 0, 0}, bp_stream(stream));
}

static int paint_load_scales2_any(int32_t mode, const float* raw_nchw, RcTable xf, const float* aux, int32_t caux,
                                  int32_t n_scale, int32_t include_original, const double* weights, const int32_t* radii,
                                  void* scratch, size_t scratch_bytes, const bp_view* out, const bp_view* out2,
                                  void* stream) {
  const int inc = include_original ? 1 : 0;
  if (mode < 0 || mode >= RC_MODES) return BP_EINVAL;
  if (!raw_nchw || !xf.p || !bp_view_ok_any(out) || !bp_view_ok_any(out2) || n_scale < 1 || caux < 0 ||
      out->c != n_scale + inc + caux || out2->c != out->c || out2->n != out->n || out2->h != out->h ||
      out2->w != out->w || (caux > 0 && !aux))
    return BP_EINVAL;
  if (out->dtype != BP_F32 || out2->dtype != BP_F32) return BP_EUNSUPPORTED;
  const int32_t n = out->n, h = out->h, w = out->w;
  const int rc = check_levels(n, h, w, n_scale, weights, radii, out->cstride > out2->cstride ? out->cstride : out2->cstride);
  if (rc != BP_OK) return rc;
  if (!scratch || scratch_bytes < bp_split_scale_workspace(n, h, w)) return BP_EWORKSPACE;
  float* s = static_cast<float*>(scratch);
  const size_t plane = (size_t)n * h * w;
  float* v = s + 2 * plane;
  const hipStream_t sm = bp_stream(stream);
  rc_dispatch(mode, [&](auto m) {
    transform_kernel<decltype(m)::value><<<dim3(nblocks((int64_t)plane)), dim3(RB), 0, sm>>>(
        raw_nchw, xf, (unsigned)(h * w), (unsigned)plane, v);
  });
  BP_CHECK_LAUNCH();
  return pyramid(v, n, h, w, n_scale, inc, weights, radii, s, s + plane, aux, caux,
                 Dst{out->ptr, out->cstride, out->coff}, Dst{out2->ptr, out2->cstride, out2->coff}, sm);
}

int bp_paint_load_scales2(const float* raw_nchw, const double* sigma_k, const float* aux, int32_t caux, int32_t n_scale,
                          int32_t include_original, const double* weights, const int32_t* radii, void* scratch,
                          size_t scratch_bytes, const bp_view* out, const bp_view* out2, void* stream) {
  return paint_load_scales2_any(RC_SHIFT_LOG, raw_nchw, RcTable{sigma_k, 2, 0, 1}, aux, caux, n_scale, include_original,
                                weights, radii, scratch, scratch_bytes, out, out2, stream);
}

int bp_paint_load_scales2_mode(int32_t mode, const float* raw_nchw, const double* records, const float* aux, int32_t caux,
                               int32_t n_scale, int32_t include_original, const double* weights, const int32_t* radii,
                               void* scratch, size_t scratch_bytes, const bp_view* out, const bp_view* out2,
                               void* stream) {
  return paint_load_scales2_any(mode, raw_nchw, rc_table4(records), aux, caux, n_scale, include_original, weights, radii,
                                scratch, scratch_bytes, out, out2, stream);
}

size_t bp_gather_tiles_scales_workspace(int32_t n, int32_t tile, int32_t n_scale) {
  return n_scale > 1 ? bp_split_scale_workspace(n, tile, tile) : 0;
}

int bp_tile_minima(const void* desc100, const void* desc150, const void* xform, int32_t n, int32_t tile, float* minima,
                   void* stream) {
  if (!desc100 || !desc150 || !xform || n <= 0 || tile <= 0 || !minima) return BP_EINVAL;
  if ((int64_t)tile * tile >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  hipLaunchKernelGGL(tile_min_kernel, dim3(n), dim3(RB), 0, bp_stream(stream), static_cast<const TileDesc*>(desc100),
                     static_cast<const TileDesc*>(desc150), static_cast<const SampleXform*>(xform), (int)tile, minima);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

// gmode: XF_OWN (the transform xform names) or a range-compression mode over `records`
static int gather_tiles_scales_any(int gmode, const double* records, const void* desc100, const void* desc150,
                                   const void* xform, const float* minima, int32_t n, int32_t tile, int32_t n_scale,
                                   int32_t include_original, const double* weights, const int32_t* radii, void* scratch,
                                   size_t scratch_bytes, float* out_nchw, void* stream) {
  const int inc = include_original ? 1 : 0;
  if (!desc100 || !desc150 || !xform || !out_nchw) return BP_EINVAL;
  const int rc = check_levels(n, tile, tile, n_scale, weights, radii, n_scale + inc);
  if (rc != BP_OK) return rc;
  if (n_scale > 1 && (!scratch || scratch_bytes < bp_gather_tiles_scales_workspace(n, tile, n_scale)))
    return BP_EWORKSPACE;
  const hipStream_t sm = bp_stream(stream);
  const size_t plane = (size_t)n * tile * tile;
  float* s = static_cast<float*>(scratch);
  const GatherArgs ga{static_cast<const TileDesc*>(desc100), static_cast<const TileDesc*>(desc150),
                      static_cast<const SampleXform*>(xform), minima, n_scale > 1 ? s + 2 * plane : nullptr, records};
  if (n_scale == 1) {
    gather_dispatch(gmode, [&](auto m) {
      gather_planes_kernel<decltype(m)::value><<<dim3(nblocks((int64_t)plane)), dim3(RB), 0, sm>>>(
          ga, out_nchw, (int)tile, inc, (unsigned)plane);
    });
    BP_CHECK_LAUNCH();
    return BP_OK;
  }
  return pyramid(ga.v, n, tile, tile, n_scale, inc, weights, radii, s, s + plane, nullptr, 0,
                 Dst{out_nchw, n_scale + inc, 0}, Dst{nullptr, 0, 0}, sm, &ga, gmode);
}

int bp_gather_tiles_scales(const void* desc100, const void* desc150, const void* xform, const float* minima, int32_t n,
                           int32_t tile, int32_t n_scale, int32_t include_original, const double* weights,
                           const int32_t* radii, void* scratch, size_t scratch_bytes, float* out_nchw, void* stream) {
  return gather_tiles_scales_any(XF_OWN, nullptr, desc100, desc150, xform, minima, n, tile, n_scale, include_original,
                                 weights, radii, scratch, scratch_bytes, out_nchw, stream);
}

int bp_gather_tiles_scales_mode(int32_t mode, const double* records, const void* desc100, const void* desc150,
                                const void* xform, const float* minima, int32_t n, int32_t tile, int32_t n_scale,
                                int32_t include_original, const double* weights, const int32_t* radii, void* scratch,
                                size_t scratch_bytes, float* out_nchw, void* stream) {
  if (mode < 0 || mode >= RC_MODES || !records) return BP_EINVAL;
  return gather_tiles_scales_any(mode, records, desc100, desc150, xform, minima, n, tile, n_scale, include_original,
                                 weights, radii, scratch, scratch_bytes, out_nchw, stream);
}

static int paint_store_scales_any(int32_t mode, const bp_view* src, const bp_pointwise* pw, int32_t softplus,
                                  int32_t include_original, RcTable xf, float* dst_nchw, void* stream) {
  if (mode < 0 || mode >= RC_MODES) return BP_EINVAL;
  if (!bp_view_ok_any(src) || !xf.p || !dst_nchw || (include_original && src->c < 2)) return BP_EINVAL;
  if (src->dtype != BP_F32) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)src->h * src->w, total = (int64_t)src->n * hw;
  if (total * src->cstride >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  rc_dispatch(mode, [&](auto m) {
    paint_store_scales_kernel<decltype(m)::value><<<dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream)>>>(
        src->ptr, src->cstride, src->coff, src->c, bp_pw(pw), softplus ? 1 : 0, include_original ? 1 : 0, xf, dst_nchw,
        (unsigned)hw, (unsigned)total);
  });
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_paint_store_scales(const bp_view* src, const bp_pointwise* pw, int32_t softplus, int32_t include_original,
                          const double* k_sigma, float* dst_nchw, void* stream) {
  return paint_store_scales_any(RC_SHIFT_LOG, src, pw, softplus, include_original, RcTable{k_sigma, 2, 1, 0}, dst_nchw,
                                stream);
}

int bp_paint_store_scales_mode(int32_t mode, const bp_view* src, const bp_pointwise* pw, int32_t softplus,
                               int32_t include_original, const double* records, float* dst_nchw, void* stream) {
  return paint_store_scales_any(mode, src, pw, softplus, include_original, rc_table4(records), dst_nchw, stream);
}

}  // extern "C"
