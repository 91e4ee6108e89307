// Scoring a CVAE painter on tiles whose truth is known (CVAE.score / CVAEPainter.score).
//   bp_loglik_samples   per-SAMPLE Gaussian log-density of the truth under the two heads, float64: the HBM-streaming
//                       kernel of the feature (x, mu and var are each read once) plus a fixed-order sum of chunk partials
//   bp_posterior_score  log p(z|y) - log q(z|x,y) of every draw, the importance weights and the five columns of the
//                       score (bound, elbo, log_likelihood, kl, ess): one wave per tile
// Everything that enters a sum is float64 and written without contraction, so the NumPy restatement in
// tests/score_ref.py differs from it by summation order alone.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int SB = 256;                    // threads of a streaming block
constexpr int CHUNK = 2048;                // pixels of a sample that one block sums: two groups of four per thread
constexpr int DRAWS_MAX = 64;              // one lane per draw in bp_posterior_score

// (paint.hip / pointwise.hip: the activation the paint paths apply to the mean head)
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

struct ViewD { const float* p; int cs, co; };
static inline ViewD vd(const bp_view* v) {
  return v ? ViewD{v->ptr, v->cstride, v->coff} : ViewD{nullptr, 0, 0};
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);       // (a + b on both partners: every lane, same bits)
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = fmax(v, __shfl_xor(v, s, 64));
  return v;
}

__device__ __forceinline__ double ll_term(float x, float mu_raw, float lv, bool softplus, bool with_var) {
  const float xm = softplus ? softplus_f(mu_raw) : mu_raw;
  const double d = (double)x - (double)xm;
  const double c0 = -0.91893853320467274178;         // -log(2 pi) / 2
  const double q = 0.5 * (d * d);
  if (!with_var) return c0 - q;
  const double l = (double)lv;
  return (c0 - 0.5 * l) - q * exp(-l);
}

struct SamplesArgs {
  const float* x;
  ViewD mu, var;
  double* partial;        // [L n][c][nchunk]
  int n, c, hw, nchunk, softplus;
};

// Block b sums pixels [k CHUNK, (k + 1) CHUNK) of sample s = b / nchunk, k = b % nchunk.  Thread t takes the pixel groups
// (it SB + t) 4 ... + 3, it = 0, 1, in that order, in BOTH paths: VEC only says how they are loaded.  The thread sums,
// the shuffle tree and the four wave sums added in order are then a function of (h, w, c) alone.
template <bool VEC, bool VAR>
__global__ __launch_bounds__(SB) void loglik_samples_kernel(SamplesArgs a) {
  __shared__ double sh[SB / 64];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x / (unsigned)a.nchunk;
  const int k = blockIdx.x % (unsigned)a.nchunk;
  const int m = (int)(s % a.n);
  const bool sp = a.softplus != 0;
  for (int ch = 0; ch < a.c; ++ch) {
    const float* xs = a.x + ((int64_t)m * a.c + ch) * a.hw;
    double acc = 0.0;
#pragma unroll
    for (int it = 0; it < CHUNK / (4 * SB); ++it) {
      const int p0 = k * CHUNK + (it * SB + t) * 4;
      if (VEC) {
        if (p0 < a.hw) {                                  // (hw % 4 == 0: the whole group is inside)
          const float4 xv = *reinterpret_cast<const float4*>(xs + p0);
          const float4 mv = *reinterpret_cast<const float4*>(a.mu.p + s * a.hw + p0);
          float4 lv = make_float4(0.f, 0.f, 0.f, 0.f);
          if (VAR) lv = *reinterpret_cast<const float4*>(a.var.p + s * a.hw + p0);
          acc += ll_term(xv.x, mv.x, lv.x, sp, VAR);
          acc += ll_term(xv.y, mv.y, lv.y, sp, VAR);
          acc += ll_term(xv.z, mv.z, lv.z, sp, VAR);
          acc += ll_term(xv.w, mv.w, lv.w, sp, VAR);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = p0 + j;
          if (p < a.hw) {
            const int64_t pix = s * a.hw + p;
            const float lv = VAR ? a.var.p[pix * a.var.cs + a.var.co + ch] : 0.f;
            acc += ll_term(xs[p], a.mu.p[pix * a.mu.cs + a.mu.co + ch], lv, sp, VAR);
          }
        }
      }
    }
    acc = wave_sum(acc);
    if (ch > 0) __syncthreads();                          // (thread 0 has read the previous channel's wave sums)
    if ((t & 63) == 0) sh[t >> 6] = acc;
    __syncthreads();
    if (t == 0) a.partial[(s * a.c + ch) * a.nchunk + k] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  }
}

// One wave per (sample, channel): lane l adds chunks l, l + 64, ... in ascending order, then the shuffle tree.
__global__ __launch_bounds__(SB) void loglik_samples_sum_kernel(const double* partial, int nchunk, int64_t rows,
                                                                double* out) {
  const int64_t row = (int64_t)blockIdx.x * (SB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  double v = 0.0;
  for (int k = lane; k < nchunk; k += 64) v += partial[row * nchunk + k];
  v = wave_sum(v);
  if (lane == 0) out[row] = v;
}

struct ScoreArgs {
  bp_latent lt;
  const float* stats4; const float* eps; const double* loglik;
  double* score; double* log_w;
  int c;
};

// One wave per tile m; lane k holds draw k.  The latent elements are walked 64 at a time: lane j evaluates the element's
// standard deviations and their logarithms once, then every draw's term is summed over the 64 lanes by the shuffle
// tree and added to r_k, groups in ascending order.
__global__ __launch_bounds__(64) void posterior_score_kernel(ScoreArgs a) {
  const int lane = threadIdx.x;
  const int m = blockIdx.x;
  const int n = a.lt.n, K = a.lt.L;
  const int64_t per = (int64_t)a.lt.zc * a.lt.zh * a.lt.zw;
  const int64_t plane = (int64_t)n * per;
  const double mzv = (double)a.lt.min_z_var;
  double r = 0.0;
  for (int64_t j0 = 0; j0 < per; j0 += 64) {
    const int64_t j = j0 + lane;
    const bool on = j < per;
    double zmu = 0.0, pmu = 0.0, sq = 1.0, spd = 1.0, dlog = 0.0;
    if (on) {
      const int64_t i = (int64_t)m * per + j;
      zmu = (double)a.stats4[i];
      pmu = (double)a.stats4[2 * plane + i];
      sq = exp(0.5 * (double)a.stats4[plane + i]) + mzv;
      spd = exp(0.5 * (double)a.stats4[3 * plane + i]) + mzv;
      dlog = log(sq) - log(spd);
    }
    for (int k = 0; k < K; ++k) {
      double term = 0.0;
      if (on) {
        const double e = (double)a.eps[((int64_t)k * n + m) * per + j];
        const double u = ((zmu + e * sq) - pmu) / spd;
        term = dlog + (0.5 * (e * e) - 0.5 * (u * u));
      }
      term = wave_sum(term);
      if (lane == k) r += term;
    }
  }
  const bool act = lane < K;
  double lls = 0.0;
  if (act) {
    const double* row = a.loglik + ((int64_t)lane * n + m) * a.c;
    lls = row[0];
    for (int ch = 1; ch < a.c; ++ch) lls += row[ch];
  }
  const double lw = lls + r;
  if (act && a.log_w) a.log_w[(int64_t)lane * n + m] = lw;
  const double ninf = -__builtin_huge_val();
  const double mx = wave_max(act ? lw : ninf);
  const double ms = (mx - mx == 0.0) ? mx : 0.0;                    // (a non-finite maximum is not subtracted)
  const double dk = (double)K;
  const double s1 = wave_sum(act ? exp(lw - ms) : 0.0);
  const double s2 = wave_sum(act ? exp(2.0 * (lw - ms)) : 0.0);
  const double e1 = wave_sum(act ? lw : 0.0);
  const double e2 = wave_sum(act ? lls : 0.0);
  const double e3 = wave_sum(act ? r : 0.0);
  if (lane == 0) {
    const double lse1 = ms + log(s1);
    const double lse2 = 2.0 * ms + log(s2);
    double* o = a.score + (int64_t)m * 5;
    o[0] = lse1 - log(dk);
    o[1] = e1 / dk;
    o[2] = e2 / dk;
    o[3] = -(e3 / dk);
    o[4] = exp(2.0 * lse1 - lse2);
  }
}

bool samples_desc_ok(const bp_loglik* ll) {
  return ll && ll->n >= 1 && ll->L >= 1 && ll->c >= 1 && ll->h >= 1 && ll->w >= 1;
}
bool samples_supported(const bp_loglik* ll) {
  return ll->L <= DRAWS_MAX && (double)ll->n * ll->L * ll->h * ll->w * ll->c < 2147483648.0;
}
int samples_chunks(const bp_loglik* ll) { return (int)(((int64_t)ll->h * ll->w + CHUNK - 1) / CHUNK); }
bool samples_view_ok(const bp_loglik* ll, const bp_view* v) {
  return bp_view_ok_any(v) && (int64_t)v->n == (int64_t)ll->n * ll->L && v->h == ll->h && v->w == ll->w && v->c == ll->c;
}

}  // namespace

extern "C" {

size_t bp_loglik_samples_workspace(const bp_loglik* ll) {
  if (!samples_desc_ok(ll) || !samples_supported(ll)) return 0;
  return (size_t)ll->n * ll->L * ll->c * samples_chunks(ll) * sizeof(double);
}

int bp_loglik_samples(const bp_loglik* ll, const float* x_nchw, const bp_view* mu_raw, const bp_view* var_raw,
                      double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!samples_desc_ok(ll) || !x_nchw || !out || !workspace || !samples_view_ok(ll, mu_raw)) return BP_EINVAL;
  if (var_raw && !samples_view_ok(ll, var_raw)) return BP_EINVAL;
  if (mu_raw->dtype != BP_F32 || (var_raw && var_raw->dtype != BP_F32) || !samples_supported(ll)) return BP_EUNSUPPORTED;
  if (workspace_bytes < bp_loglik_samples_workspace(ll)) return BP_EWORKSPACE;
  SamplesArgs a;
  a.x = x_nchw; a.mu = vd(mu_raw); a.var = vd(var_raw);
  a.partial = static_cast<double*>(workspace);
  a.n = ll->n; a.c = ll->c; a.hw = ll->h * ll->w; a.nchunk = samples_chunks(ll); a.softplus = ll->mu_softplus;
  const int64_t samples = (int64_t)ll->n * ll->L;
  const auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool vec = ll->c == 1 && mu_raw->cstride == 1 && (!var_raw || var_raw->cstride == 1) && a.hw % 4 == 0 &&
                   al16(x_nchw) && al16(mu_raw->ptr) && (!var_raw || al16(var_raw->ptr));
  const dim3 grid((unsigned)(samples * a.nchunk));          // (< 2^31: n L H W c is, and a chunk is never empty)
  hipStream_t st = bp_stream(stream);
  if (vec) {
    if (var_raw) loglik_samples_kernel<true, true><<<grid, SB, 0, st>>>(a);
    else loglik_samples_kernel<true, false><<<grid, SB, 0, st>>>(a);
  } else {
    if (var_raw) loglik_samples_kernel<false, true><<<grid, SB, 0, st>>>(a);
    else loglik_samples_kernel<false, false><<<grid, SB, 0, st>>>(a);
  }
  BP_CHECK_LAUNCH();
  const int64_t rows = samples * ll->c;
  loglik_samples_sum_kernel<<<(unsigned)((rows + SB / 64 - 1) / (SB / 64)), SB, 0, st>>>(a.partial, a.nchunk, rows, out);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_posterior_score(const bp_latent* lt, const float* stats4, const float* eps, const double* loglik, int32_t c,
                       double* score, double* log_w, void* stream) {
  if (!lt || !stats4 || !eps || !loglik || !score || lt->n < 1 || lt->L < 1 || c < 1 || lt->zc < 1 || lt->zh < 1 ||
      lt->zw < 1)
    return BP_EINVAL;
  if (lt->L > DRAWS_MAX) return BP_EUNSUPPORTED;
  ScoreArgs a;
  a.lt = *lt; a.stats4 = stats4; a.eps = eps; a.loglik = loglik; a.score = score; a.log_w = log_w; a.c = c;
  posterior_score_kernel<<<(unsigned)lt->n, 64, 0, bp_stream(stream)>>>(a);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

}  // extern "C"
