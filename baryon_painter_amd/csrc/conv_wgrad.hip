// Weight gradient on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), NHWC.
//
//   dst[cy][cx][ky][kx] = sum_{n,q} act(X)[n, q*s + k - p, cx] * act(Y)[n, q, cy]
// X is the tensor on the fine grid (Conv2d: the layer input; ConvTranspose2d: the output
// gradient), Y the one on the coarse grid (Conv2d: dy; ConvTranspose2d: the layer input); the
// result is exactly the torch weight layout in both cases.
//   GEMM view: M = 16 X-channels, N = 16 Y-channels, K = pixels (4 per MFMA).
// A workgroup owns one kernel row ky, one 16-channel X tile and 16*NTY Y channels, and walks a
// strided subset ("split") of the BH x 16 pixel tiles; its 4 waves take different pixel rows and
// are summed through LDS at the end.  Partial results per split go to a workspace and a second
// kernel adds them in a fixed order, so the gradient is bitwise reproducible (no float atomics).
#include "common.hpp"
#include "kernels.hpp"
#include <vector>

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int WG_BH = 8;    // pixel rows per tile (2 per wave)
constexpr int WG_BW = 16;   // pixel columns per tile
constexpr int KW_MAX = 9;

struct WgradArgs {
  const float* X; int xh, xw, xcs, xco, cx;
  const float* Y; int yh, yw, ycs, yco, cy;
  int n, k, stride, pad;
  PW pwx, pwy;
  float* ws;
  int ncxt, ncyg, nsplit, tiles_x, tiles_y, IW, IWq, CXP, CYP;
};

template <int NTY>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
  constexpr int CYB = 16 * NTY;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int s = a.stride;
  float* lds_x = smem;                                   // [BH][s][IWq][16]
  float* lds_y = smem + (size_t)WG_BH * s * a.IWq * 16;  // [NTY][BH][BW][16]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;

  const int cxt = blockIdx.x % a.ncxt;
  const int cyg = blockIdx.x / a.ncxt;
  const int ky = blockIdx.y;
  const int split = blockIdx.z;
  const int cx0 = cxt * 16, cy0 = cyg * CYB;

  v4f acc[KW_MAX][NTY];
#pragma unroll
  for (int t = 0; t < KW_MAX; ++t)
#pragma unroll
    for (int nt = 0; nt < NTY; ++nt) acc[t][nt] = v4f{0.f, 0.f, 0.f, 0.f};

  const int tiles_per_img = a.tiles_x * a.tiles_y;
  const int ntiles = a.n * tiles_per_img;
  for (int tile = split; tile < ntiles; tile += a.nsplit) {
    const int n = tile / tiles_per_img;
    const int ty_ = (tile % tiles_per_img) / a.tiles_x, tx_ = tile % a.tiles_x;
    const int qy0 = ty_ * WG_BH, qx0 = tx_ * WG_BW;
    __syncthreads();
    // ---- stage X rows: row r <-> iy = (qy0+r)*s + ky - p, col c <-> ix = qx0*s - p + c
    const float* Xn = a.X + (int64_t)n * a.xh * a.xw * a.xcs + a.xco;
    for (int e = tid; e < WG_BH * a.IW * 16; e += 256) {
      const int ch = e & 15;
      const int c = (e >> 4) % a.IW;
      const int r = (e >> 4) / a.IW;
      const int iy = (qy0 + r) * s + ky - a.pad, ix = qx0 * s - a.pad + c;
      float v = 0.f;
      if (iy >= 0 && iy < a.xh && ix >= 0 && ix < a.xw && (qy0 + r) < a.yh && cx0 + ch < a.cx)
        v = pw_apply(a.pwx, cx0 + ch, Xn[((int64_t)iy * a.xw + ix) * a.xcs + cx0 + ch]);
      lds_x[((r * s + c % s) * a.IWq + c / s) * 16 + ch] = v;
    }
    // ---- stage Y tile
    const float* Yn = a.Y + (int64_t)n * a.yh * a.yw * a.ycs + a.yco;
    for (int e = tid; e < WG_BH * WG_BW * CYB; e += 256) {
      const int ch = e % CYB;
      const int c = (e / CYB) % WG_BW;
      const int r = e / (CYB * WG_BW);
      const int qy = qy0 + r, qx = qx0 + c;
      float v = 0.f;
      if (qy < a.yh && qx < a.yw && cy0 + ch < a.cy)
        v = pw_apply(a.pwy, cy0 + ch, Yn[((int64_t)qy * a.yw + qx) * a.ycs + cy0 + ch]);
      lds_y[(((ch >> 4) * WG_BH + r) * WG_BW + c) * 16 + (ch & 15)] = v;
    }
    __syncthreads();
    // ---- this wave's rows: 2 rows x 4 pixel groups
#pragma unroll
    for (int rr = 0; rr < WG_BH / 4; ++rr) {
      const int r = wave * (WG_BH / 4) + rr;
#pragma unroll
      for (int g = 0; g < WG_BW / 4; ++g) {
        const int qxl = 4 * g + kq;
        float bf[NTY];
#pragma unroll
        for (int nt = 0; nt < NTY; ++nt) bf[nt] = lds_y[((nt * WG_BH + r) * WG_BW + qxl) * 16 + li];
#pragma unroll
        for (int t = 0; t < KW_MAX; ++t) {
          if (t < a.k) {
            const float af = lds_x[((r * s + t % s) * a.IWq + qxl + t / s) * 16 + li];
#pragma unroll
            for (int nt = 0; nt < NTY; ++nt)
              acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[nt], acc[t][nt], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- sum the 4 waves through LDS and write this split's partial tile
  //      D[row = 4*(lane>>4)+r : X channel][col = lane&15 : Y channel]
  float* red = smem;  // [4 waves][NTY][64 lanes][4]
#pragma unroll
  for (int t = 0; t < KW_MAX; ++t) {
    if (t < a.k) {
      __syncthreads();
#pragma unroll
      for (int nt = 0; nt < NTY; ++nt)
        *reinterpret_cast<float4*>(red + ((wave * NTY + nt) * 64 + lane) * 4) =
            make_float4(acc[t][nt][0], acc[t][nt][1], acc[t][nt][2], acc[t][nt][3]);
      __syncthreads();
      for (int e = tid; e < NTY * 256; e += 256) {
        const int nt = e / 256, l = (e % 256) / 4, r = e % 4;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += red[((w * NTY + nt) * 64 + l) * 4 + r];
        const int cx = cx0 + 4 * (l >> 4) + r, cy = cy0 + nt * 16 + (l & 15);
        a.ws[((((int64_t)split * a.k + ky) * a.k + t) * a.CYP + cy) * a.CXP + cx] = sum;
      }
    }
  }
}

struct WreduceArgs {
  const float* ws; float* dst;
  int k, cx, cy, CXP, CYP, nsplit;
  int cx_total, cx_off, cy_off;     // position of this (cx, cy) block inside the full weight tensor
};

// WR_GRP: split groups per block (threads = 64 outputs x WR_GRP): 4 for the few-way splits of the fp32 kernels, 16 for
// the 128 ... 512-way splits of the bf16 and thin-layer kernels
template <int WR_GRP>
__device__ __forceinline__ void wgrad_reduce_block(const WreduceArgs& a, int64_t block, double (*sh)[64]) {
  // 64 consecutive outputs (workspace order [ky][kx][cy][cx], cx fastest: coalesced) x WR_GRP groups of splits per
  // block: a thread adds every WR_GRP-th split (two chains, loads independent of each other), the groups are then
  // added in a fixed order -> bitwise reproducible.  (With four groups a 512-way split is 128 trips per thread:
  // latency-bound, 30 us for 25 MB; sixteen cut the chain to 32.)
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t i = block * 64 + lane;
  const int64_t total = (int64_t)a.k * a.k * a.cy * a.cx;
  double s = 0.0;
  int cx = 0, cy = 0, t = 0;
  if (i < total) {
    cx = i % a.cx;
    cy = (i / a.cx) % a.cy;
    t = i / ((int64_t)a.cx * a.cy);
    const int64_t stride = (int64_t)a.k * a.k * a.CYP * a.CXP;
    const float* p = a.ws + ((int64_t)t * a.CYP + cy) * a.CXP + cx;
    double s0 = 0.0, s1 = 0.0;
    int sp = grp;
    for (; sp + WR_GRP < a.nsplit; sp += 2 * WR_GRP) {
      s0 += (double)p[sp * stride];
      s1 += (double)p[(sp + WR_GRP) * stride];
    }
    if (sp < a.nsplit) s0 += (double)p[sp * stride];
    s = s0 + s1;
  }
  sh[grp][lane] = s;
  __syncthreads();
  if (grp == 0 && i < total) {
    double r = sh[0][lane];
#pragma unroll
    for (int g = 1; g < WR_GRP; ++g) r += sh[g][lane];
    a.dst[((int64_t)(a.cy_off + cy) * a.cx_total + a.cx_off + cx) * a.k * a.k + t] = (float)r;
  }
}

template <int WR_GRP>
__global__ __launch_bounds__(64 * WR_GRP) void wgrad_reduce_kernel(WreduceArgs a) {
  __shared__ double sh[WR_GRP][64];
  wgrad_reduce_block<WR_GRP>(a, blockIdx.x, sh);
}

// Deferred reductions (bp_wgrad_defer_begin / _flush): the reductions of many layers in one launch.  A block finds its
// job by scanning the table of first blocks (a few dozen entries, scalar loads); each job is reduced exactly as its own
// launch would reduce it, so deferring changes no bit of dW.
constexpr int WR_BATCH = 40;
struct WreduceBatch {
  int njobs;
  int first[WR_BATCH + 1];
  WreduceArgs job[WR_BATCH];
};
static_assert(sizeof(WreduceBatch) <= 4096, "kernel argument block");

template <int WR_GRP>
__global__ __launch_bounds__(64 * WR_GRP) void wgrad_reduce_batch_kernel(WreduceBatch b) {
  __shared__ double sh[WR_GRP][64];
  const int blk = blockIdx.x;
  int j = 0;
  while (j + 1 < b.njobs && blk >= b.first[j + 1]) ++j;
  wgrad_reduce_block<WR_GRP>(b.job[j], blk - b.first[j], sh);
}

}  // namespace

// Per host thread: between bp_wgrad_defer_begin() and bp_wgrad_defer_flush() the reductions of calls flagged
// BP_IMPL_DEFER are collected, not launched: the flag is the caller's promise that the call's workspace is its own
// until the flush (cvae._Plan: one per fp32 layer).
struct DeferState { bool on = false, private_ws = false; std::vector<WreduceArgs> jobs; };
static thread_local DeferState t_defer;

// (fills in the position of the (cx, cy) block inside dW: a WreduceArgs built with cx_total left at 0 wrote every
//  produced channel onto the first one's row)
static int wgrad_reduce(const float* ws, float* dst, int k, int cx, int cy, int CXP, int CYP, int nsplit,
                        hipStream_t st, int cx_total = -1, int cx_off = 0, int cy_off = 0, bool may_defer = true) {
  WreduceArgs r{};
  r.ws = ws; r.dst = dst; r.k = k; r.cx = cx; r.cy = cy; r.CXP = CXP; r.CYP = CYP; r.nsplit = nsplit;
  r.cx_total = cx_total < 0 ? cx : cx_total; r.cx_off = cx_off; r.cy_off = cy_off;
  if (t_defer.on && t_defer.private_ws && may_defer) {
    t_defer.jobs.push_back(r);
    return BP_OK;
  }
  const int64_t total = (int64_t)cy * cx * k * k;
  if (r.nsplit > 64) hipLaunchKernelGGL(wgrad_reduce_kernel<16>, dim3((unsigned)((total + 63) / 64)), dim3(1024), 0, st, r);
  else hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, r);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

template <int WR_GRP>
static int wgrad_reduce_flush_class(const std::vector<WreduceArgs>& jobs, bool wide, hipStream_t st) {
  WreduceBatch b{};
  auto launch = [&]() {
    if (b.njobs == 0) return;
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel<WR_GRP>, dim3((unsigned)b.first[b.njobs]), dim3(64 * WR_GRP), 0, st, b);
    b = WreduceBatch{};
  };
  for (const WreduceArgs& r : jobs) {
    if ((r.nsplit > 64) != wide) continue;
    const int64_t nb = ((int64_t)r.cy * r.cx * r.k * r.k + 63) / 64;
    if (b.njobs == WR_BATCH || b.first[b.njobs] + nb > 0x3fffffff) launch();
    b.job[b.njobs] = r;
    b.first[b.njobs + 1] = b.first[b.njobs] + (int)nb;
    ++b.njobs;
  }
  launch();
  BP_CHECK_LAUNCH();
  return BP_OK;
}

void bp_wgrad_private_ws(bool on) { t_defer.private_ws = on; }

int bp_wgrad_defer_begin_impl() {
  t_defer.on = true;
  t_defer.jobs.clear();
  return BP_OK;
}

int bp_wgrad_defer_flush_impl(hipStream_t st, int end) {
  int rc = BP_OK;
  // (the state is per host thread: a flush from another thread than the one that called bp_wgrad_defer_begin would find
  //  an empty list, report success and leave every deferred dW unreduced -- refuse it instead)
  if (end >= 0 && !t_defer.on) return BP_EINVAL;
  if (end < 0) t_defer.jobs.clear();          // abandon
  if (!t_defer.jobs.empty()) {
    rc = wgrad_reduce_flush_class<16>(t_defer.jobs, true, st);
    if (rc == BP_OK) rc = wgrad_reduce_flush_class<4>(t_defer.jobs, false, st);
    t_defer.jobs.clear();
  }
  if (end) t_defer.on = false;
  return rc;
}

namespace {

// The generic kernel: every layer of k <= 9 whose staged tiles fit the LDS.
int wgrad_general(const WgradCall& c, float* ws, size_t ws_bytes, WgradRow* row, hipStream_t st, bool dry) {
  const bp_conv* cv = c.cv;
  const bp_view *X = c.X, *Y = c.Y;
  if (cv->k > KW_MAX) return BP_EUNSUPPORTED;
  const int NTY = (Y->c > 16) ? 2 : 1;
  const int CYB = 16 * NTY;
  WgradArgs a{};
  a.ncxt = bp_ceil_div(X->c, 16);
  a.ncyg = bp_ceil_div(Y->c, CYB);
  a.CXP = a.ncxt * 16;
  a.CYP = a.ncyg * CYB;
  a.tiles_x = bp_ceil_div(Y->w, WG_BW);
  a.tiles_y = bp_ceil_div(Y->h, WG_BH);
  const int64_t ntiles = (int64_t)Y->n * a.tiles_x * a.tiles_y;
  const int64_t base = (int64_t)a.ncxt * a.ncyg * cv->k;
  int64_t ns = (2048 + base - 1) / base;
  if (ns > ntiles) ns = ntiles;
  if (ns < 1) ns = 1;
  if (ns > 65535) ns = 65535;
  a.nsplit = (int)ns;
  a.IW = (WG_BW - 1) * cv->stride + cv->k;
  a.IWq = bp_ceil_div(a.IW, cv->stride);
  const size_t lds_main = ((size_t)WG_BH * cv->stride * a.IWq * 16 + (size_t)NTY * WG_BH * WG_BW * 16) * 4;
  const size_t lds_red = (size_t)4 * NTY * 64 * 4 * 4;
  const size_t lds_bytes = lds_main > lds_red ? lds_main : lds_red;
  if (lds_bytes > 64 * 1024) return BP_EUNSUPPORTED;
  *row = WgradRow{BP_WG_GENERAL, a.nsplit, a.CXP, a.CYP, (size_t)a.nsplit * cv->k * cv->k * a.CYP * a.CXP * sizeof(float)};
  if (dry) return BP_OK;
  if (!ws || ws_bytes < row->bytes) return BP_EWORKSPACE;
  a.X = X->ptr; a.xh = X->h; a.xw = X->w; a.xcs = X->cstride; a.xco = X->coff; a.cx = X->c;
  a.Y = Y->ptr; a.yh = Y->h; a.yw = Y->w; a.ycs = Y->cstride; a.yco = Y->coff; a.cy = Y->c;
  a.n = X->n; a.k = cv->k; a.stride = cv->stride; a.pad = cv->pad; a.pwx = c.pwx; a.pwy = c.pwy;
  a.ws = ws;
  dim3 grid((unsigned)(a.ncxt * a.ncyg), (unsigned)cv->k, (unsigned)a.nsplit);
  if (NTY == 2)
    hipLaunchKernelGGL((wgrad_kernel<2>), grid, dim3(256), lds_bytes, st, a);
  else
    hipLaunchKernelGGL((wgrad_kernel<1>), grid, dim3(256), lds_bytes, st, a);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

const WgradFamily& wgrad_family_general() {
  static const WgradFamily f = {"general", bp_wgrad_plan_of<wgrad_general>, bp_wgrad_run_of<wgrad_general>, false, false};
  return f;
}

// One or two channels on one side and many on the other (the k9 stem / head of the CGAN generator): the tap-packed
// few-channel kernel runs once per 16-channel chunk of the wide side, each chunk reduced into its block of dW.
bool wide_side(const WgradCall& c, bool* on_x) {
  if (c.X->c > 16 && c.Y->c <= 2) *on_x = true;
  else if (c.Y->c > 16 && c.X->c <= 2) *on_x = false;
  else return false;
  return true;
}

// chunk c0 of the wide side: its views, and the pointwise operand moved to its channels
struct Chunk {
  bp_view sub;
  WgradCall call;
  Chunk(const WgradCall& c, bool on_x, int c0, int nc) : sub(on_x ? *c.X : *c.Y), call(c) {
    sub.c = nc;
    sub.coff += c0;
    PW& p = on_x ? call.pwx : call.pwy;
    if (p.scale) p = PW{p.scale + c0, p.shift + c0, p.slope + c0};
    (on_x ? call.X : call.Y) = &sub;
  }
  Chunk(const Chunk&) = delete;
};

bool chunked_plan(const WgradCall& c, WgradRow* row) {
  bool on_x = false;
  if (!wide_side(c, &on_x)) return false;
  // every chunk size that occurs needs an instantiation: the full 16 channels and the ragged tail (33 = 2 x 16 + 1 has
  // a one-channel tail without one -- such a layer is not chunked at all, rather than refused after two chunks of dW)
  const int wide = on_x ? c.X->c : c.Y->c;
  for (int nc = 16; nc > 0; nc = (nc == 16 ? wide % 16 : 0)) {
    const Chunk ch(c, on_x, 0, nc);
    WgradRow r;
    if (bp_wgrad_small(ch.call, nullptr, 0, &r, nullptr, true) != BP_OK) return false;
    if (nc == 16) *row = WgradRow{BP_WG_SMALL_CHUNKED, r.nsplit, r.cxp, r.cyp, r.bytes};
    else if (r.bytes > row->bytes) row->bytes = r.bytes;
  }
  return true;
}

int chunked_run(const WgradCall& c, const WgradRow&, float* dst, void* ws, size_t ws_bytes, hipStream_t st) {
  bool on_x = false;
  wide_side(c, &on_x);
  const int wide = on_x ? c.X->c : c.Y->c;
  for (int c0 = 0; c0 < wide; c0 += 16) {
    const Chunk ch(c, on_x, c0, wide - c0 < 16 ? wide - c0 : 16);
    WgradRow r;
    int rc = bp_wgrad_small(ch.call, reinterpret_cast<float*>(ws), ws_bytes, &r, st, false);
    if (rc == BP_OK)
      rc = wgrad_reduce(reinterpret_cast<const float*>(ws), dst, c.cv->k, ch.call.X->c, ch.call.Y->c, r.cxp, r.cyp,
                        r.nsplit, st, c.X->c, on_x ? c0 : 0, on_x ? 0 : c0, /*may_defer=*/false);      // (the chunks share one workspace)
    if (rc != BP_OK) return rc;
  }
  return BP_OK;
}

const WgradFamily& wgrad_family_chunked() {
  static const WgradFamily f = {"small_chunked", chunked_plan, chunked_run, true, false};
  return f;
}

// The two tables are the one place the priority order is written: bp_wgrad_select() walks them for the call, for the
// plan query and for the workspace query alike.  A new family: write its WgradFamily record next to its kernels, declare
// its accessor in kernels.hpp, insert it here.
//
// fp32.  stem, flat and flat_s2 are kernels of one layer each, disjoint among themselves; they come first because the
// kernels behind them take their layers too (small the stem's and the head's, tiles the stride-2 k4 layers').  chunked
// stands before tiles, which accepts its k9 layers whole; thin never sees them (its Y has one channel, its X at most
// eight).  ws_f32 stands before tiles (both take the 128 <-> 128 k3 layers), enc before small and tiles (both take the
// k8 stride-4 layer), thin before small (which has instantiations for three of thin's layers), small before tiles (which
// takes any channel count at its (k, stride)), and general, which takes every k <= 9, last.
// may_requalify: stem, flat and flat_s2 look at the pointwise operands, ws_f32 at an option.
using FamilyFn = const WgradFamily& (*)();
const FamilyFn F32_FAMILIES[] = {bp_wgrad_family_stem,  bp_wgrad_family_flat, bp_wgrad_family_flat_s2, wgrad_family_chunked,
                                 bp_wgrad_family_ws_f32, bp_wgrad_family_enc,  bp_wgrad_family_thin,    bp_wgrad_family_small,
                                 bp_wgrad_family_tiles,  wgrad_family_general};
// bf16 (operands may be fp32 or bf16).  wf, sf and wh are kernels of one layer each, disjoint among themselves; the
// tiled kernels take their layers too.  ws_bf16 stands before tiled: both take the 128 <-> 128 k3 layers.
// may_requalify: ws_bf16 looks at an option.  wf, sf and wh refuse a pointwise operand on Y and are NOT marked: the
// workspace has always been sized for them alone.  bp_conv_backward_weight cannot reach the other branch -- they accept
// plain convolutions only, whose pointwise operand lands on X -- and a caller of these tables that could would be
// answered BP_EWORKSPACE where the tiled kernel needs more.
const FamilyFn BF16_FAMILIES[] = {bp_wgrad_family_bf16_wf, bp_wgrad_family_bf16_sf, bp_wgrad_family_bf16_wh,
                                  bp_wgrad_family_ws_bf16, bp_wgrad_family_bf16_tiled};

}  // namespace

int bp_wgrad_select(bool bf16, const WgradCall& c, WgradSelection* s) {
  const FamilyFn* table = bf16 ? BF16_FAMILIES : F32_FAMILIES;
  const size_t count = bf16 ? sizeof(BF16_FAMILIES) / sizeof(FamilyFn) : sizeof(F32_FAMILIES) / sizeof(FamilyFn);
  *s = WgradSelection{};
  for (size_t i = 0; i < count; ++i) {
    const WgradFamily& f = table[i]();
    WgradRow row;
    if (!f.plan(c, &row)) continue;
    if (!s->family) { s->family = &f; s->row = row; }
    if (row.bytes > s->ws_bytes) s->ws_bytes = row.bytes;
    if (!f.may_requalify) break;      // (the families behind it: only for the size of the workspace)
  }
  return s->family ? BP_OK : BP_EUNSUPPORTED;
}

int bp_wgrad_run(const WgradSelection& s, const WgradCall& c, float* dst, void* workspace, size_t workspace_bytes,
                 hipStream_t st) {
  const int rc = s.family->run(c, s.row, dst, workspace, workspace_bytes, st);
  if (rc != BP_OK || s.family->reduces_itself) return rc;
  return wgrad_reduce(reinterpret_cast<const float*>(workspace), dst, c.cv->k, c.X->c, c.Y->c, s.row.cxp, s.row.cyp,
                      s.row.nsplit, st);
}
