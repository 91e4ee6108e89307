// Fully connected layers of the latent bottleneck (nn.Linear behind Flatten / in front of Unflatten, utils.py:132-133,
// 148-157): forward, data gradient and weight gradient of  out[n][g] = sum_f act(x[n][f]) * W[g][f] + b[g]  in exact fp32.
//
// Shape of the problem: a skinny product.  The batch is 1 ... 256 rows, the weight matrix (O, K) up to 512 x 16 384 =
// 33.5 MB, so every kernel here is bound by ONE pass over the weights (read in forward / data gradient, written in the
// weight gradient); the activations (at most 4 MB) are re-read from L2.  All batch rows of a weight tile are therefore
// handled by one workgroup:
//   forward        workgroup = (32 output features) x (one slab of K) x (up to 256 rows).  The long sum over K is split
//                  into slabs; each slab's partial products go to the workspace and a second launch adds the slabs in
//                  ascending order (+ bias) and scatters the result into the NHWC output view.  No atomics.
//   data gradient  workgroup = (32 input features) x (all of O) x (up to 256 rows): the sum over g is complete inside
//                  the workgroup, the result goes straight into the gradient view.
//   weight grad.   one wave = one 32 x 32 tile of dW, summed over the batch in ascending order; written once, in torch's
//                  (O, K) layout.  db from the same launch (the tiles of the first column).
// Batches of 32 rows and more run on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: bit-for-bit an fmaf chain in
// ascending k), smaller ones on the vector ALUs.  Every sum has a fixed order: the same call gives the same bits.
//
// Feature order: the reference flattens (c, h, w) tensors with c slowest and unflattens the same way; the slots are
// NHWC.  The permutation is applied to the ACTIVATION index (feature f of an (c, h, w) operand is channel f / (h*w) of
// pixel f % (h*w)), never to the weights: those are read and their gradient written as torch stores them.
#include "common.hpp"

namespace {

constexpr int TB = 256;        // threads of a product workgroup (4 waves)
constexpr int TILE = 32;       // features per weight tile, both ways
constexpr int LS = TILE + 1;   // LDS row stride in floats (odd: a column of 32 rows hits 32 banks)
constexpr int MAXROWS = 256;   // batch rows per workgroup
constexpr int KSLAB_MIN = 256; // shortest slab of the forward's split over K
constexpr int WG_GT = 8;       // output features per thread of the vector-ALU weight gradient

typedef float f32x16 __attribute__((ext_vector_type(16)));

// An NHWC view read as rows of c*h*w features in (c, h, w) order.
struct Geo {
  int hw, cs, co;
};
static inline Geo geo_of(const bp_view* v) { return Geo{v->h * v->w, v->cstride, v->coff}; }
__device__ __forceinline__ int64_t geo_off(const Geo& g, int n, int f, int& ch) {
  ch = f / g.hw;
  const int p = f - ch * g.hw;
  return ((int64_t)n * g.hw + p) * g.cs + g.co + ch;
}

// C[n][j] = sum_k A[n][k] * B(k, j) for one tile of 32 j, one range of k and up to 256 rows n.
//   MODE 0 (forward):        A = act(x),  k = input feature of this slab,  j = output feature,  B(k, j) = W[j][k];
//                            C = this slab's partial sums  part[slab][n][O]
//   MODE 1 (data gradient):  A = dy,      k = output feature (all of them), j = input feature,  B(k, j) = W[k][j];
//                            C = the dx view
// A weight tile is staged as read (rows = output features, columns = input features); VEC: 16-byte loads of W.
template <int MODE, bool MFMA, bool VEC>
__global__ __launch_bounds__(TB) void lin_product_kernel(const float* __restrict__ A, Geo ga, PW pw,
                                                         const float* __restrict__ W, int K, int O, int n_total,
                                                         int kslab, float* __restrict__ Cout, Geo gc) {
  extern __shared__ float smem[];
  float* Ws = smem;                    // [TILE][LS]
  float* As = smem + TILE * LS;        // [rows_pad][LS]
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * TILE;
  const int n0 = blockIdx.z * MAXROWS;
  const int nrows = min(MAXROWS, n_total - n0);
  const int rows_pad = MFMA ? ((nrows + TILE - 1) / TILE) * TILE : nrows;
  const int kb = MODE == 0 ? blockIdx.y * kslab : 0;
  const int ke = MODE == 0 ? min(K, kb + kslab) : O;
  const int J = MODE == 0 ? O : K;
  const int nchunks = (ke - kb + TILE - 1) / TILE;

  // this thread's part of a weight tile: row wr, columns wc ... wc + 3
  const int wr = tid >> 3, wc = (tid & 7) * 4;
  auto load_w = [&](int kc, float (&v)[4]) {
    const int R = MODE == 0 ? j0 + wr : kc + wr;            // output feature
    const int Cc = MODE == 0 ? kc + wc : j0 + wc;           // input feature
    const int Clim = MODE == 0 ? ke : K;
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (R >= O) return;
    const float* src = W + (size_t)R * K + Cc;
    if (VEC && Cc + 3 < Clim) {
      const float4 q = *reinterpret_cast<const float4*>(src);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (Cc + i < Clim) v[i] = src[i];
    }
  };

  f32x16 acc[2];
  float vacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  const int lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int ntiles = rows_pad / TILE;

  float wreg[4];
  if (nchunks > 0) load_w(kb, wreg);
  for (int c = 0; c < nchunks; ++c) {
    const int kc = kb + c * TILE;
    __syncthreads();                   // the previous chunk's products are done with the tiles
#pragma unroll
    for (int i = 0; i < 4; ++i) Ws[wr * LS + wc + i] = wreg[i];
    for (int idx = tid; idx < rows_pad * TILE; idx += TB) {
      const int row = idx >> 5, kk = idx & 31, k = kc + kk;
      float v = 0.f;
      if (row < nrows && k < ke) {
        int ch;
        const int64_t off = geo_off(ga, n0 + row, k, ch);
        v = A[off];
        if (MODE == 0) v = pw_apply(pw, ch, v);
      }
      As[row * LS + kk] = v;
    }
    __syncthreads();
    if (c + 1 < nchunks) load_w(kc + TILE, wreg);     // in flight during the products
    if (MFMA) {
#pragma unroll 4
      for (int kk = 0; kk < TILE; kk += 2) {
        const float b = MODE == 0 ? Ws[r * LS + kk + h] : Ws[(kk + h) * LS + r];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int tile = wv + 4 * t;
          if (tile < ntiles)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(tile * TILE + r) * LS + kk + h], b, acc[t], 0, 0, 0);
        }
      }
    } else {
      const int j = tid & 31, rq = tid >> 5;
#pragma unroll 8
      for (int kk = 0; kk < TILE; ++kk) {
        const float b = MODE == 0 ? Ws[j * LS + kk] : Ws[kk * LS + j];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = rq + 8 * q;
          if (row < nrows) vacc[q] = fmaf(As[row * LS + kk], b, vacc[q]);
        }
      }
    }
  }

  auto store = [&](int row, int col, float v) {
    const int n = n0 + row, j = j0 + col;
    if (row >= nrows || j >= J) return;
    if (MODE == 0) {
      Cout[((size_t)blockIdx.y * n_total + n) * O + j] = v;
    } else {
      int ch;
      Cout[geo_off(gc, n, j, ch)] = v;
    }
  };
  if (MFMA) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int tile = wv + 4 * t;
      if (tile >= ntiles) continue;
#pragma unroll
      for (int i = 0; i < 16; ++i) store(tile * TILE + (i & 3) + 8 * (i >> 2) + 4 * h, r, acc[t][i]);
    }
  } else {
    const int j = tid & 31, rq = tid >> 5;
#pragma unroll
    for (int q = 0; q < 4; ++q) store(rq + 8 * q, j, vacc[q]);
  }
}

// out[n][g] = ((part[0] + part[1]) + ...) + b[g], ascending slabs, into the output view.
__global__ __launch_bounds__(TB) void lin_reduce_kernel(const float* __restrict__ part, int nslab, int n_total, int O,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        Geo gy) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int64_t total = (int64_t)n_total * O;
  if (i >= total) return;
  const int n = (int)(i / O), g = (int)(i - (int64_t)n * O);
  float s = part[i];
  for (int k = 1; k < nslab; ++k) s += part[(size_t)k * total + i];
  if (bias) s += bias[g];
  int ch;
  out[geo_off(gy, n, g, ch)] = s;
}

// dW[g][f] = sum_n dy[n][g] * act(x[n][f]) for one 32 x 32 tile per wave, n ascending; db[g] = sum_n dy[n][g].
__global__ __launch_bounds__(64) void lin_wgrad_mfma_kernel(const float* __restrict__ x, Geo gx, PW pw,
                                                            const float* __restrict__ dy, Geo gd, int n_total, int K,
                                                            int O, float* __restrict__ dW, float* __restrict__ db) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int f0 = blockIdx.x * TILE, g0 = blockIdx.y * TILE;
  const int f = f0 + r, g = g0 + r;
  const bool fok = f < K, gok = g < O;
  int chf = 0, chg = 0;
  const int64_t xoff = fok ? geo_off(gx, 0, f, chf) : 0, doff = gok ? geo_off(gd, 0, g, chg) : 0;
  const int64_t xs = (int64_t)gx.hw * gx.cs, ds = (int64_t)gd.hw * gd.cs;      // floats between batch rows
  float sc = 1.f, sf = 0.f, sl = 1.f;
  const bool act = pw.scale != nullptr && fok;
  if (act) { sc = pw.scale[chf]; sf = pw.shift[chf]; sl = pw.slope[chf]; }
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 4
  for (int nn = 0; nn < n_total; nn += 2) {
    const int m = nn + h;
    float a = 0.f, b = 0.f;
    if (m < n_total) {
      if (gok) a = dy[doff + m * ds];
      if (fok) {
        b = x[xoff + m * xs];
        if (act) {
          const float t = fmaf(b, sc, sf);
          b = t > 0.f ? t : t * sl;
        }
      }
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (fok) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = g0 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (row < O) dW[(size_t)row * K + f] = acc[i];
    }
  }
  if (db != nullptr && blockIdx.x == 0 && h == 0 && gok) {
    float s = 0.f;
    for (int m = 0; m < n_total; ++m) s += dy[doff + m * ds];
    db[g] = s;
  }
}

// The same sums on the vector ALUs (batches below one matrix-core tile): a thread owns one input feature and WG_GT
// output features.
__global__ __launch_bounds__(TB) void lin_wgrad_valu_kernel(const float* __restrict__ x, Geo gx, PW pw,
                                                            const float* __restrict__ dy, Geo gd, int n_total, int K,
                                                            int O, float* __restrict__ dW, float* __restrict__ db) {
  const int f = blockIdx.x * TB + threadIdx.x, g0 = blockIdx.y * WG_GT;
  const int64_t xs = (int64_t)gx.hw * gx.cs, ds = (int64_t)gd.hw * gd.cs;
  if (db != nullptr && blockIdx.x == 0 && threadIdx.x < WG_GT && g0 + threadIdx.x < O) {
    int ch;
    const int64_t doff = geo_off(gd, 0, g0 + threadIdx.x, ch);
    float s = 0.f;
    for (int m = 0; m < n_total; ++m) s += dy[doff + m * ds];
    db[g0 + threadIdx.x] = s;
  }
  if (f >= K) return;
  int chf;
  const int64_t xoff = geo_off(gx, 0, f, chf);
  int64_t doff[WG_GT];
#pragma unroll
  for (int i = 0; i < WG_GT; ++i) {
    int ch;
    doff[i] = g0 + i < O ? geo_off(gd, 0, g0 + i, ch) : -1;
  }
  float acc[WG_GT];
#pragma unroll
  for (int i = 0; i < WG_GT; ++i) acc[i] = 0.f;
  for (int m = 0; m < n_total; ++m) {
    const float xv = pw_apply(pw, chf, x[xoff + m * xs]);
#pragma unroll
    for (int i = 0; i < WG_GT; ++i)
      if (doff[i] >= 0) acc[i] = fmaf(dy[doff[i] + m * ds], xv, acc[i]);
  }
#pragma unroll
  for (int i = 0; i < WG_GT; ++i)
    if (doff[i] >= 0) dW[(size_t)(g0 + i) * K + f] = acc[i];
}

// ---- host side
bool desc_ok(const bp_linear* d) {
  return d && d->in_features > 0 && d->out_features > 0 && d->in_c > 0 && d->in_h > 0 && d->in_w > 0 && d->out_c > 0 &&
         d->out_h > 0 && d->out_w > 0 && (int64_t)d->in_c * d->in_h * d->in_w == d->in_features &&
         (int64_t)d->out_c * d->out_h * d->out_w == d->out_features &&
         (int64_t)d->in_features * d->out_features < (int64_t)1 << 31;
}
// `v` holds n rows of the descriptor's input (side 0) or output (side 1) features
bool side_ok(const bp_linear* d, int side, const bp_view* v) {
  if (!bp_view_ok(v)) return false;
  const int c = side ? d->out_c : d->in_c, h = side ? d->out_h : d->in_h, w = side ? d->out_w : d->in_w;
  return v->c == c && v->h == h && v->w == w && (int64_t)v->n * v->h * v->w * v->cstride < (int64_t)1 << 31;
}
// split of the forward's sum over K: slab length (a multiple of the tile) and slab count.  A function of the layer
// alone, so that a row's result does not depend on the batch it is part of.
void split_k(const bp_linear* d, int* kslab, int* nslab) {
  const int K = d->in_features, otiles = bp_ceil_div(d->out_features, TILE);
  int s = 512 / otiles;                                     // about two workgroups per compute unit
  const int most = bp_ceil_div(K, KSLAB_MIN);
  if (s > most) s = most;
  if (s < 1) s = 1;
  *kslab = bp_round_up(bp_ceil_div(K, s), TILE);
  *nslab = bp_ceil_div(K, *kslab);
}
bool vec_ok(const float* w, int K) { return K % 4 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0; }

template <int MODE>
void launch_product(bool mfma, bool vec, dim3 grid, size_t lds, hipStream_t st, const float* A, Geo ga, PW pw,
                    const float* W, int K, int O, int n, int kslab, float* Cout, Geo gc) {
#define BP_LIN_GO(M, V) \
  hipLaunchKernelGGL((lin_product_kernel<MODE, M, V>), grid, dim3(TB), lds, st, A, ga, pw, W, K, O, n, kslab, Cout, gc)
  if (mfma) { if (vec) BP_LIN_GO(true, true); else BP_LIN_GO(true, false); }
  else { if (vec) BP_LIN_GO(false, true); else BP_LIN_GO(false, false); }
#undef BP_LIN_GO
}
size_t product_lds(int n) {
  const int rows = n < MAXROWS ? n : MAXROWS;
  return (size_t)(TILE + bp_round_up(rows, TILE)) * LS * sizeof(float);
}

}  // namespace

extern "C" {

size_t bp_linear_workspace(int32_t n, const bp_linear* d) {
  if (n <= 0 || !desc_ok(d)) return 0;
  int kslab, nslab;
  split_k(d, &kslab, &nslab);
  return (size_t)nslab * n * d->out_features * sizeof(float);
}

int bp_linear_forward(const bp_linear* d, const bp_view* x, const bp_pointwise* x_pw, const float* weight,
                      const float* bias, const bp_view* y, void* workspace, size_t workspace_bytes, void* stream) {
  if (!desc_ok(d) || !side_ok(d, 0, x) || !side_ok(d, 1, y) || x->n != y->n || !weight || !workspace) return BP_EINVAL;
  if ((d->has_bias != 0) != (bias != nullptr)) return BP_EINVAL;
  const int n = x->n, K = d->in_features, O = d->out_features;
  if (workspace_bytes < bp_linear_workspace(n, d)) return BP_EWORKSPACE;
  int kslab, nslab;
  split_k(d, &kslab, &nslab);
  float* part = static_cast<float*>(workspace);
  const dim3 grid(bp_ceil_div(O, TILE), nslab, bp_ceil_div(n, MAXROWS));
  launch_product<0>(n >= TILE, vec_ok(weight, K), grid, product_lds(n), bp_stream(stream), x->ptr, geo_of(x),
                    bp_pw(x_pw), weight, K, O, n, kslab, part, Geo{1, O, 0});
  BP_CHECK_LAUNCH();
  const int64_t total = (int64_t)n * O;
  hipLaunchKernelGGL(lin_reduce_kernel, dim3((unsigned)((total + TB - 1) / TB)), dim3(TB), 0, bp_stream(stream), part,
                     nslab, n, O, bias, y->ptr, geo_of(y));
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_linear_backward_data(const bp_linear* d, const bp_view* dy, const float* weight, const bp_view* dx,
                            void* stream) {
  if (!desc_ok(d) || !side_ok(d, 1, dy) || !side_ok(d, 0, dx) || dx->n != dy->n || !weight) return BP_EINVAL;
  const int n = dy->n, K = d->in_features, O = d->out_features;
  const dim3 grid(bp_ceil_div(K, TILE), 1, bp_ceil_div(n, MAXROWS));
  launch_product<1>(n >= TILE, vec_ok(weight, K), grid, product_lds(n), bp_stream(stream), dy->ptr, geo_of(dy),
                    PW{nullptr, nullptr, nullptr}, weight, K, O, n, 0, dx->ptr, geo_of(dx));
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_linear_backward_weight(const bp_linear* d, const bp_view* x, const bp_pointwise* x_pw, const bp_view* dy,
                              float* dweight, float* dbias, void* stream) {
  if (!desc_ok(d) || !side_ok(d, 0, x) || !side_ok(d, 1, dy) || x->n != dy->n || !dweight) return BP_EINVAL;
  if ((d->has_bias != 0) != (dbias != nullptr)) return BP_EINVAL;
  const int n = x->n, K = d->in_features, O = d->out_features;
  if (n >= TILE) {
    hipLaunchKernelGGL(lin_wgrad_mfma_kernel, dim3(bp_ceil_div(K, TILE), bp_ceil_div(O, TILE)), dim3(64), 0,
                       bp_stream(stream), x->ptr, geo_of(x), bp_pw(x_pw), dy->ptr, geo_of(dy), n, K, O, dweight, dbias);
  } else {
    hipLaunchKernelGGL(lin_wgrad_valu_kernel, dim3(bp_ceil_div(K, TB), bp_ceil_div(O, WG_GT)), dim3(TB), 0,
                       bp_stream(stream), x->ptr, geo_of(x), bp_pw(x_pw), dy->ptr, geo_of(dy), n, K, O, dweight, dbias);
  }
  BP_CHECK_LAUNCH();
  return BP_OK;
}

}  // extern "C"
