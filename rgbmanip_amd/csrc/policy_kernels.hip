// PPO policy kernels (gfx950): fused actor-critic forward, fused PPO loss + backward, gradient reduction,
// gradient-clip + adaptive-LR + Adam — the arithmetic of
//   /root/reference/algo/ppo/ppo/module.py:73-107   (ActorCritic.act / act_inference / evaluate)
//   /root/reference/algo/ppo/ppo/ppo.py:472-528     (one minibatch of PPO.update)
// for the reference's MLPs (obs -> h0 -> h1 -> h2 -> out, ELU hidden activations, 36 985 parameters for the shipped cfg).
// The problem is launch/latency bound, so the design minimises launches and host syncs: one launch for
// forward+loss+backward of a minibatch (64 rows per workgroup, activations in LDS, weight rows as wave-uniform scalar
// loads), one deterministic cross-block reduction, one single-block optimiser step that also applies the KL-adaptive
// learning-rate rule on the device (the reference syncs the host twice per minibatch for that, ppo.py:486-495,527-528).
// The Gaussian is the reference's quirky one: scale_tril = diag(exp(log_std)^2), i.e. std = exp(2*log_std).
#include "common.h"
#include "kernels.h"

namespace rgbm {

constexpr int PK_ROWS = 64;      // rows per workgroup
constexpr int PK_MAXW = 128;     // max layer width
constexpr int PK_LD = PK_MAXW + 1;
constexpr float LOG_2PI = 1.8378770664093453f;

__device__ __forceinline__ float elu(float x) { return x > 0.f ? x : expm1f(x); }

// one dense layer for the block's 64 rows: out[r][o] = act(b[o] + sum_i W[o][i] * in[r][i]); lane = row, wave = column group
__device__ __forceinline__ void dense_fwd(const float* __restrict__ W, const float* __restrict__ b, const float* in, int ldi,
                                          float* out, int ldo, int I, int O, bool act) {
  const int r = threadIdx.x & 63, g = threadIdx.x >> 6;
  for (int o = g; o < O; o += 4) {
    const float* wr = W + (long long)o * I;      // wave-uniform address -> scalar loads
    float acc = b[o];
    for (int i = 0; i < I; ++i) acc = fmaf(wr[i], in[r * ldi + i], acc);
    out[r * ldo + o] = act ? elu(acc) : acc;
  }
}

// ---------------------------------------------------------------------------------------------------------
// forward only: mode 0 = act (sample with supplied N(0,1) noise), 1 = act_inference (mean), 2 = evaluate(actions)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void policy_forward_kernel(const float* __restrict__ P, PolicyLayout L, int n, int mode,
                                                             const float* __restrict__ obs, const float* __restrict__ noise,
                                                             float* __restrict__ actions, float* __restrict__ logp,
                                                             float* __restrict__ value, float* __restrict__ mu_out) {
  __shared__ float bufA[PK_ROWS * PK_LD], bufB[PK_ROWS * PK_LD], a0[PK_ROWS * PK_LD];
  const int r = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * PK_ROWS + r;
  const bool live = row < n;
  for (int i = g; i < L.dims[0]; i += 4) a0[r * PK_LD + i] = live ? obs[row * L.dims[0] + i] : 0.f;
  __syncthreads();
  for (int net = 0; net < (mode == 1 ? 1 : 2); ++net) {
    const float* in = a0;
    float* outb = bufA;
    for (int l = 0; l < 4; ++l) {
      const int I = L.dims[l], O = (l == 3) ? (net == 0 ? L.dims[4] : 1) : L.dims[l + 1];
      dense_fwd(P + L.w[net][l], P + L.b[net][l], in, PK_LD, outb, PK_LD, I, O, l < 3);
      __syncthreads();
      in = outb;
      outb = (outb == bufA) ? bufB : bufA;
    }
    // `in` now holds the net's output
    if (net == 0) {
      const int A = L.dims[4];
      if (live && g == 0) {
        float lp = -0.5f * A * LOG_2PI;
        for (int k = 0; k < A; ++k) {
          const float m = in[r * PK_LD + k], ls = P[L.log_std + k];
          mu_out[row * A + k] = m;
          if (mode == 1) continue;
          float a;
          if (mode == 0) { a = m + expf(2.f * ls) * noise[row * A + k]; actions[row * A + k] = a; }
          else a = actions[row * A + k];
          const float d = a - m;
          lp += -(d * d) / (2.f * expf(4.f * ls)) - 2.f * ls;
        }
        if (mode != 1) logp[row] = lp;
      }
      __syncthreads();
    } else if (live && g == 0) {
      value[row] = in[r * PK_LD];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// forward + PPO loss + backward for one minibatch; partial gradients per workgroup
// ---------------------------------------------------------------------------------------------------------
// dW[o][i] += sum_r delta[r][o] * a[r][i]   (256 threads stride over the O*I elements; rows from LDS)
__device__ __forceinline__ void dense_wgrad(const float* delta, int ldd, const float* a, int lda, float* gW, float* gb, int I,
                                            int O, int nrows) {
  for (int e = threadIdx.x; e < O * I; e += 256) {
    const int o = e / I, i = e - o * I;
    float acc = 0.f;
    for (int r = 0; r < nrows; ++r) acc = fmaf(delta[r * ldd + o], a[r * lda + i], acc);
    gW[e] = acc;
  }
  for (int o = threadIdx.x; o < O; o += 256) {
    float acc = 0.f;
    for (int r = 0; r < nrows; ++r) acc += delta[r * ldd + o];
    gb[o] = acc;
  }
}
// dprev[r][i] = (sum_o W[o][i] * delta[r][o]) * elu'(a_prev)   with elu'(z) expressed through a = elu(z): a>0 ? 1 : a+1
__device__ __forceinline__ void dense_dgrad(const float* __restrict__ W, const float* delta, int ldd, const float* aprev, int lda,
                                            float* dprev, int I, int O) {
  const int r = threadIdx.x & 63, g = threadIdx.x >> 6;
  for (int i = g; i < I; i += 4) {
    float acc = 0.f;
    for (int o = 0; o < O; ++o) acc = fmaf(W[(long long)o * I + i], delta[r * ldd + o], acc);
    const float a = aprev[r * lda + i];
    dprev[r * ldd + i] = acc * (a > 0.f ? 1.f : a + 1.f);
  }
}

__global__ __launch_bounds__(256) void ppo_loss_grad_kernel(const float* __restrict__ P, PolicyLayout L, int n,
                                                            const float* __restrict__ obs, const float* __restrict__ actions,
                                                            const float* __restrict__ old_logp, const float* __restrict__ adv,
                                                            const float* __restrict__ returns, const float* __restrict__ old_values,
                                                            const float* __restrict__ old_mu, const float* __restrict__ old_sigma,
                                                            float clip, float vcoef, float ecoef, float* __restrict__ partial,
                                                            int pstride) {
  extern __shared__ float sm[];
  // activations a0 (obs), a1, a2, a3 of the current net, each [64][dims[l]+1]; two delta buffers [64][LDD]
  float* act_[4];
  int lda[4];
  int off = 0, wmax = L.dims[4];
  for (int l = 0; l < 4; ++l) { act_[l] = sm + off; lda[l] = L.dims[l] + 1; off += PK_ROWS * lda[l]; if (l > 0 && L.dims[l] > wmax) wmax = L.dims[l]; }
  const int LDD = wmax + 1;
  float* dA = sm + off;                  // delta of the layer being processed
  float* dB = dA + PK_ROWS * LDD;
  float* red = dB + PK_ROWS * LDD;       // [64][20]: row statistics (3) + log_std gradient contributions (<=16)
  const int r = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long long row0 = (long long)blockIdx.x * PK_ROWS;
  const long long row = row0 + r;
  const int nrows = (int)((n - row0) < PK_ROWS ? (n - row0) : PK_ROWS);
  const bool live = r < nrows;
  const int A = L.dims[4];
  float* gout = partial + (long long)blockIdx.x * pstride;
  const float invn = 1.0f / (float)n;

  for (int i = g; i < L.dims[0]; i += 4) act_[0][r * lda[0] + i] = live ? obs[row * L.dims[0] + i] : 0.f;
  __syncthreads();

  for (int net = 0; net < 2; ++net) {
    // ---- forward, keeping every activation ----
    for (int l = 0; l < 3; ++l) {
      dense_fwd(P + L.w[net][l], P + L.b[net][l], act_[l], lda[l], act_[l + 1], lda[l + 1], L.dims[l], L.dims[l + 1], true);
      __syncthreads();
    }
    const int O = net == 0 ? A : 1;
    dense_fwd(P + L.w[net][3], P + L.b[net][3], act_[3], lda[3], dB, LDD, L.dims[3], O, false);   // dB temporarily holds the output
    __syncthreads();
    // ---- loss gradient w.r.t. the net output -> dA ----
    if (g == 0) {
      if (net == 0) {
        float lp = -0.5f * A * LOG_2PI, kl = 0.f;
        for (int k = 0; k < A; ++k) {
          const float m = dB[r * LDD + k], ls = P[L.log_std + k];
          const float a = live ? actions[row * A + k] : m;
          const float d = a - m;
          lp += -(d * d) / (2.f * expf(4.f * ls)) - 2.f * ls;
          if (live) {
            const float os = old_sigma[row * A + k], om = old_mu[row * A + k];
            const float eo = expf(os), en = expf(ls);
            kl += ls - os + (eo * eo + (om - m) * (om - m)) / (2.f * en * en) - 0.5f;     // ppo.py:482-483
          }
        }
        float dlp = 0.f, surr = 0.f;
        if (live) {
          const float ratio = expf(lp - old_logp[row]);
          const float ad = adv[row];
          const float s1 = -ad * ratio;
          const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
          const float s2 = -ad * rc;
          surr = fmaxf(s1, s2);
          // d max(s1,s2)/d logp: s1 branch -> -ad*ratio; clipped branch contributes only inside the clip range (then s1==s2)
          const bool inside = ratio > 1.f - clip && ratio < 1.f + clip;
          dlp = (s1 > s2 || inside) ? -ad * ratio : ((s1 == s2) ? 0.5f * -ad * ratio : 0.f);
        }
        for (int k = 0; k < A; ++k) {
          const float m = dB[r * LDD + k], ls = P[L.log_std + k];
          const float a = live ? actions[row * A + k] : m;
          const float d = a - m, iv = expf(-4.f * ls);
          dA[r * LDD + k] = live ? dlp * (d * iv) * invn : 0.f;                              // dL/dmu
          red[r * 20 + 4 + k] = live ? (dlp * (2.f * d * d * iv - 2.f) * invn) : 0.f;          // dL/dlog_std via logp
        }
        red[r * 20 + 0] = surr;
        red[r * 20 + 2] = kl;
      } else {
        float vl = 0.f, dv = 0.f;
        if (live) {
          const float v = dB[r * LDD], tv = old_values[row], rt = returns[row];
          const float diff = v - tv;
          const float vc = tv + fminf(fmaxf(diff, -clip), clip);
          const float l1 = (v - rt) * (v - rt), l2 = (vc - rt) * (vc - rt);
          vl = fmaxf(l1, l2);
          const bool inside = diff > -clip && diff < clip;
          if (l1 > l2) dv = 2.f * (v - rt);
          else if (l1 < l2) dv = inside ? 2.f * (vc - rt) : 0.f;
          else dv = inside ? 2.f * (v - rt) : (v - rt);      // tie: torch.max splits the gradient evenly
          dv *= vcoef * invn;
        }
        dA[r * LDD] = dv;
        red[r * 20 + 1] = vl;
      }
    }
    __syncthreads();
    // ---- backward through the four layers ----
    float* dcur = dA;
    float* dnext = dB;
    for (int l = 3; l >= 0; --l) {
      const int I = L.dims[l], Ol = (l == 3) ? O : L.dims[l + 1];
      dense_wgrad(dcur, LDD, act_[l], lda[l], gout + L.w[net][l], gout + L.b[net][l], I, Ol, PK_ROWS);
      if (l > 0) dense_dgrad(P + L.w[net][l], dcur, LDD, act_[l], lda[l], dnext, I, Ol);
      __syncthreads();
      float* t = dcur; dcur = dnext; dnext = t;
    }
    if (net == 0) {
      // log_std gradient (+ entropy term: entropy = const + 2*sum(log_std) for every row -> -ecoef * 2)
      if (threadIdx.x < A) {
        float acc = 0.f;
        for (int rr = 0; rr < PK_ROWS; ++rr) acc += red[rr * 20 + 4 + threadIdx.x];
        gout[L.log_std + threadIdx.x] = acc - ecoef * 2.f * (float)nrows * invn;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    float acc = 0.f;
    for (int rr = 0; rr < PK_ROWS; ++rr) acc += red[rr * 20 + threadIdx.x];
    gout[L.total + threadIdx.x] = acc;
  }
  if (threadIdx.x == 3) gout[L.total + 3] = (float)nrows;
}

// grads[e] = sum over workgroups (fixed order -> deterministic); e in [0, total+4)
__global__ void ppo_reduce_kernel(const float* __restrict__ partial, int nblk, int pstride, int count, float* __restrict__ grads) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  float acc = 0.f;
  for (int b = 0; b < nblk; ++b) acc += partial[(long long)b * pstride + e];
  grads[e] = acc;
}

// single-workgroup optimiser step: average over ranks, clip by global norm, KL-adaptive LR, Adam (torch defaults)
__global__ __launch_bounds__(1024) void ppo_adam_kernel(float* __restrict__ P, const float* __restrict__ grads, float* __restrict__ m,
                                                        float* __restrict__ v, PolicyOptState* __restrict__ st, int total,
                                                        float inv_world, float max_norm, float desired_kl, float lr_min,
                                                        float lr_max, int adaptive) {
  __shared__ double red[1024];
  __shared__ float s_coef, s_lr, s_bc1, s_bc2s;
  double acc = 0.0;
  for (int i = threadIdx.x; i < total; i += 1024) { const double gval = (double)grads[i] * inv_world; acc += gval * gval; }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    float coef = max_norm / (norm + 1e-6f);
    s_coef = coef > 1.f ? 1.f : coef;
    const float rows = grads[total + 3];
    const float kl_mean = grads[total + 2] / rows;
    float lr = st->lr;
    if (adaptive) {                                   // ppo.py:486-495 (asymmetric clamps kept as shipped)
      if (kl_mean > desired_kl * 2.0f) lr = fmaxf(lr_min, lr / 1.5f);
      else if (kl_mean < desired_kl / 2.0f && kl_mean > 0.0f) lr = fminf(lr_max, lr * 1.5f);
    }
    st->lr = lr;
    st->t += 1;
    st->sum_surr += (double)(grads[total + 0] / rows);
    st->sum_vloss += (double)(grads[total + 1] / rows);
    st->last_kl = kl_mean;
    st->last_norm = norm;
    st->n_updates += 1;
    const double bc1 = 1.0 - pow(0.9, (double)st->t), bc2 = 1.0 - pow(0.999, (double)st->t);
    s_lr = lr; s_bc1 = (float)bc1; s_bc2s = (float)sqrt(bc2);
  }
  __syncthreads();
  const float coef = s_coef, lr = s_lr, bc1 = s_bc1, bc2s = s_bc2s;
  for (int i = threadIdx.x; i < total; i += 1024) {
    const float gval = grads[i] * inv_world * coef;
    const float mi = 0.9f * m[i] + 0.1f * gval;
    const float vi = 0.999f * v[i] + 0.001f * gval * gval;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2s + 1e-8f;
    P[i] -= (lr / bc1) * (mi / denom);
  }
}

static int check_layout(const PolicyLayout& L) {
  for (int l = 0; l < 5; ++l) RGBM_REQUIRE(L.dims[l] > 0 && L.dims[l] <= PK_MAXW, "policy layer width must be in 1..128");
  RGBM_REQUIRE(L.dims[4] <= 16, "policy action dim must be <= 16");
  return 0;
}

int launch_policy_forward(const float* params, const PolicyLayout& L, int n, int mode, const float* obs, const float* noise,
                          float* actions, float* logp, float* value, float* mu, hipStream_t s) {
  if (int rc = check_layout(L)) return rc;
  RGBM_REQUIRE(n > 0 && mode >= 0 && mode <= 2, "policy_forward arguments");
  hipLaunchKernelGGL(policy_forward_kernel, dim3((n + PK_ROWS - 1) / PK_ROWS), dim3(256), 0, s, params, L, n, mode, obs, noise,
                     actions, logp, value, mu);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int policy_partial_floats(const PolicyLayout& L, int n) { return ((n + PK_ROWS - 1) / PK_ROWS) * (L.total + 4); }

int launch_ppo_minibatch(const float* params, const PolicyLayout& L, int n, const float* obs, const float* actions,
                         const float* old_logp, const float* adv, const float* returns, const float* old_values,
                         const float* old_mu, const float* old_sigma, float clip, float vcoef, float ecoef, float* partial,
                         float* grads, hipStream_t s) {
  if (int rc = check_layout(L)) return rc;
  RGBM_REQUIRE(n > 0, "ppo_minibatch rows");
  const int nblk = (n + PK_ROWS - 1) / PK_ROWS, pstride = L.total + 4;
  int wmax = L.dims[4], asum = 0;
  for (int l = 0; l < 4; ++l) { asum += L.dims[l] + 1; if (l > 0 && L.dims[l] > wmax) wmax = L.dims[l]; }
  const size_t lds = (size_t)(PK_ROWS * (asum + 2 * (wmax + 1)) + PK_ROWS * 20) * sizeof(float);
  RGBM_REQUIRE(lds <= 160 * 1024, "policy too wide for the LDS-resident backward pass");
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(ppo_loss_grad_kernel), (int)lds)) return rc;
  hipLaunchKernelGGL(ppo_loss_grad_kernel, dim3(nblk), dim3(256), lds, s, params, L, n, obs, actions, old_logp, adv, returns,
                     old_values, old_mu, old_sigma, clip, vcoef, ecoef, partial, pstride);
  RGBM_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ppo_reduce_kernel, dim3((pstride + 255) / 256), dim3(256), 0, s, partial, nblk, pstride, pstride, grads);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_ppo_adam(float* params, const float* grads, float* m, float* v, PolicyOptState* st, int total, float inv_world,
                    float max_norm, float desired_kl, float lr_min, float lr_max, int adaptive, hipStream_t s) {
  hipLaunchKernelGGL(ppo_adam_kernel, dim3(1), dim3(1024), 0, s, params, grads, m, v, st, total, inv_world, max_norm, desired_kl,
                     lr_min, lr_max, adaptive);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}


// =========================================================================================================
// General actor-critic (rgbm_policy_desc): 1..6 hidden layers per net, each net with its own widths (1..512), any of the
// reference's activations (module.py:109-126), an optional second input for the critic (asymmetric), action dim 1..32,
// clipped or plain-MSE value loss.  The two kernels above stay the specialisation for the shipped shape (same three hidden
// widths <= 128 in both nets, ELU, symmetric, clipped value loss, action dim <= 16): the launchers below forward to them
// when the descriptor says so, so that shape computes what it always did.
//
// Design.  Same dataflow as above (lane = row, 64 rows per workgroup, weight rows as wave-uniform scalar loads, fp32
// FMA in the reference's summation order) with three changes that remove the LDS capacity limit and fill the chip:
//   * one workgroup per (64-row tile, net): grid.y = 2, actor and critic run side by side and write disjoint parts of
//     the tile's partial gradient;
//   * activations and the two delta buffers live in a global scratch, column-major [col][64] (coalesced for lane = row);
//     LDS holds only the operand of the layer in flight ([64][maxw+1]) plus a 32-column chunk tile for the weight
//     gradient: 149 KB at width 512, 74 KB for the 256-wide default;
//   * 16 waves per workgroup and 8 outputs per lane and LDS read (8 FMAs per ds_read_b32 instead of 1).
// The activation is a template parameter; its derivative is written from the stored output.
// =========================================================================================================
constexpr int PX_NT = 1024;     // threads per workgroup
constexpr int PX_T = 8;         // outputs per lane
constexpr int PX_CH = 32;       // columns per weight-gradient chunk
constexpr int PX_LDC = PX_CH + 1;
constexpr int PX_RED = 4 + POLICY_MAX_ACT;

template <int ACT> __device__ __forceinline__ float act_fwd(float x) {
  if (ACT == PACT_ELU) return x > 0.f ? x : expm1f(x);
  if (ACT == PACT_SELU) return 1.0507009873554804934193349852946f * (x > 0.f ? x : 1.6732632423543772848170429916717f * expm1f(x));
  if (ACT == PACT_RELU) return x > 0.f ? x : 0.f;
  if (ACT == PACT_LRELU) return x > 0.f ? x : 0.01f * x;
  if (ACT == PACT_TANH) return tanhf(x);
  return 1.f / (1.f + expf(-x));
}
// d act / d x written through a = act(x)
template <int ACT> __device__ __forceinline__ float act_dfo(float a) {
  if (ACT == PACT_ELU) return a > 0.f ? 1.f : a + 1.f;
  if (ACT == PACT_SELU)
    return a > 0.f ? 1.0507009873554804934193349852946f
                   : a + 1.0507009873554804934193349852946f * 1.6732632423543772848170429916717f;
  if (ACT == PACT_RELU) return a > 0.f ? 1.f : 0.f;
  if (ACT == PACT_LRELU) return a > 0.f ? 1.f : 0.01f;
  if (ACT == PACT_TANH) return 1.f - a * a;
  return a * (1.f - a);
}

struct NetView {          // one net of the descriptor, as the kernels walk it
  int nl;                 // linear layers = hidden + 1
  int in_dim, out_dim;
  const int* hid;
  const int* w;
  const int* b;
  __device__ __forceinline__ int in_w(int k) const { return k == 0 ? in_dim : hid[k - 1]; }
  __device__ __forceinline__ int out_w(int k) const { return k == nl - 1 ? out_dim : hid[k]; }
};
__device__ __forceinline__ NetView net_view(const PolicyDesc& D, int net) {
  NetView v;
  v.nl = D.n_hidden[net] + 1;
  v.in_dim = (net == 1 && D.asymmetric) ? D.state_dim : D.obs_dim;
  v.out_dim = net == 0 ? D.act_dim : 1;
  v.hid = D.hidden[net];
  v.w = D.w[net];
  v.b = D.b[net];
  return v;
}
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// out[r][o] = act(b[o] + sum_i W[o][i] * X[r][i]) for the tile's rows; lane = row (rr), wave = groups of PX_T columns.
// X is row-major in LDS (odd leading dimension); out is addressed as out[r * os_r + o * os_o].
template <int ACT>
__device__ __forceinline__ void dense_fwd_x(const float* __restrict__ W, const float* __restrict__ b, const float* X, int ldx,
                                            int rr, int I, int O, bool act, float* out, int os_r, int os_o, bool wr) {
  const int nw = blockDim.x >> 6;
  for (int o0 = wave_id() * PX_T; o0 < O; o0 += nw * PX_T) {
    const int nt = O - o0 < PX_T ? O - o0 : PX_T;
    float acc[PX_T];
#pragma unroll
    for (int t = 0; t < PX_T; ++t) acc[t] = t < nt ? b[o0 + t] : 0.f;
    const float* wr0 = W + (long long)o0 * I;
    if (nt == PX_T) {
#pragma unroll 4
      for (int i = 0; i < I; ++i) {
        const float x = X[rr * ldx + i];
#pragma unroll
        for (int t = 0; t < PX_T; ++t) acc[t] = fmaf(wr0[t * I + i], x, acc[t]);
      }
    } else {
      for (int i = 0; i < I; ++i) {
        const float x = X[rr * ldx + i];
#pragma unroll
        for (int t = 0; t < PX_T; ++t) if (t < nt) acc[t] = fmaf(wr0[t * I + i], x, acc[t]);
      }
    }
    if (wr) {
#pragma unroll
      for (int t = 0; t < PX_T; ++t) if (t < nt) out[rr * os_r + (o0 + t) * os_o] = act ? act_fwd<ACT>(acc[t]) : acc[t];
    }
  }
}

// log-prob / sample epilogue of the actor (module.py:73-107) for one row; `m` points at the row's means (stride 1)
__device__ __forceinline__ void policy_head(const float* __restrict__ P, int log_std, int A, int mode, const float* m, long long row,
                                            const float* __restrict__ noise, float* __restrict__ actions, float* __restrict__ logp,
                                            float* __restrict__ mu_out) {
  float lp = -0.5f * A * LOG_2PI;
  for (int k = 0; k < A; ++k) {
    const float mk = m[k], ls = P[log_std + k];
    mu_out[row * A + k] = mk;
    if (mode == 1) continue;
    float a;
    if (mode == 0) { a = mk + expf(2.f * ls) * noise[row * A + k]; actions[row * A + k] = a; }
    else a = actions[row * A + k];
    const float d = a - mk;
    lp += -(d * d) / (2.f * expf(4.f * ls)) - 2.f * ls;
  }
  if (mode != 1) logp[row] = lp;
}

// forward only; R (64 or 32) rows per workgroup so that two operand tiles fit in LDS at any width; grid.y = net
template <int ACT>
__global__ __launch_bounds__(PX_NT) void policy_forward_x_kernel(const float* __restrict__ P, PolicyDesc D, int n, int mode, int R, int ld,
                                                                 const float* __restrict__ obs, const float* __restrict__ states,
                                                                 const float* __restrict__ noise, float* __restrict__ actions,
                                                                 float* __restrict__ logp, float* __restrict__ value,
                                                                 float* __restrict__ mu_out) {
  extern __shared__ float sm[];
  const int net = blockIdx.y;
  const NetView V = net_view(D, net);
  float* X = sm;
  float* Y = sm + R * ld;
  const int lane = threadIdx.x & 63, rr = lane & (R - 1), nw = blockDim.x >> 6;
  const bool wr = lane < R;
  const long long row = (long long)blockIdx.x * R + rr;
  const bool live = wr && row < n;
  const float* in = (net == 1 && D.asymmetric) ? states : obs;
  for (int c = wave_id(); c < V.in_dim; c += nw)
    if (wr) X[rr * ld + c] = live ? in[row * V.in_dim + c] : 0.f;
  __syncthreads();
  for (int k = 0; k < V.nl; ++k) {
    dense_fwd_x<ACT>(P + V.w[k], P + V.b[k], X, ld, rr, V.in_w(k), V.out_w(k), k < V.nl - 1, Y, ld, 1, wr);
    __syncthreads();
    float* t = X; X = Y; Y = t;
  }
  if (live && threadIdx.x < 64) {
    if (net == 0) policy_head(P, D.log_std, D.act_dim, mode, X + rr * ld, row, noise, actions, logp, mu_out);
    else value[row] = X[rr * ld];
  }
}

// X[r][c] <- G[c][r] for c < C (G column-major [C][64] in global memory)
__device__ __forceinline__ void load_tile_x(float* X, int ldx, const float* G, int C) {
  const int r = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int c = wave_id(); c < C; c += nw) X[r * ldx + c] = G[c * 64 + r];
}

// forward + PPO loss + backward of one net for one 64-row tile; activations and deltas in the global scratch `ws`
template <int ACT>
__global__ __launch_bounds__(PX_NT) void ppo_loss_grad_x_kernel(const float* __restrict__ P, PolicyDesc D, int n, int ldx,
                                                                const float* __restrict__ obs, const float* __restrict__ states,
                                                                const float* __restrict__ actions, const float* __restrict__ old_logp,
                                                                const float* __restrict__ adv, const float* __restrict__ returns,
                                                                const float* __restrict__ old_values, const float* __restrict__ old_mu,
                                                                const float* __restrict__ old_sigma, float clip, float vcoef, float ecoef,
                                                                int clipped_vloss, float* __restrict__ partial, int pstride,
                                                                float* __restrict__ ws, long long region) {
  extern __shared__ float sm[];
  const int net = blockIdx.y;
  const NetView V = net_view(D, net);
  float* X = sm;                        // [64][ldx]  operand of the layer in flight (activation or delta)
  float* Cb = X + 64 * ldx;             // [64][33]   net output, later the activation chunk of the weight gradient
  float* red = Cb + 64 * PX_LDC;        // [64][36]   row statistics (3) + log_std gradient contributions
  const int r = threadIdx.x & 63, nw = blockDim.x >> 6;
  const long long row0 = (long long)blockIdx.x * 64;
  const long long row = row0 + r;
  const int nrows = (int)((n - row0) < 64 ? (n - row0) : 64);
  const bool live = r < nrows;
  const int A = D.act_dim;
  float* gout = partial + (long long)blockIdx.x * pstride;
  const float invn = 1.0f / (float)n;
  // scratch of this (tile, net): a_0 .. a_{nl-1} (inputs of every linear layer), then two delta buffers of maxd columns
  float* gA = ws + ((long long)blockIdx.x * 2 + net) * region;
  int asum = 0, maxd = V.out_dim;
  for (int k = 0; k < V.nl; ++k) { asum += V.in_w(k); if (k < V.nl - 1 && V.hid[k] > maxd) maxd = V.hid[k]; }
  float* dcur = gA + (long long)asum * 64;
  float* dnext = dcur + (long long)maxd * 64;

  const float* in = (net == 1 && D.asymmetric) ? states : obs;
  for (int c = wave_id(); c < V.in_dim; c += nw) {
    const float x = live ? in[row * V.in_dim + c] : 0.f;
    X[r * ldx + c] = x;
    gA[c * 64 + r] = x;
  }
  __syncthreads();
  // ---- forward, every activation kept in the scratch ----
  {
    float* a = gA;
    for (int k = 0; k < V.nl - 1; ++k) {
      float* an = a + (long long)V.in_w(k) * 64;
      dense_fwd_x<ACT>(P + V.w[k], P + V.b[k], X, ldx, r, V.in_w(k), V.hid[k], true, an, 1, 64, true);
      __syncthreads();
      load_tile_x(X, ldx, an, V.hid[k]);
      __syncthreads();
      a = an;
    }
    dense_fwd_x<ACT>(P + V.w[V.nl - 1], P + V.b[V.nl - 1], X, ldx, r, V.in_w(V.nl - 1), V.out_dim, false, Cb, PX_LDC, 1, true);
    __syncthreads();
  }
  // ---- loss gradient w.r.t. the net output -> dcur (same arithmetic as ppo_loss_grad_kernel) ----
  if (threadIdx.x < 64) {
    if (net == 0) {
      float lp = -0.5f * A * LOG_2PI, kl = 0.f;
      for (int k = 0; k < A; ++k) {
        const float m = Cb[r * PX_LDC + k], ls = P[D.log_std + k];
        const float a = live ? actions[row * A + k] : m;
        const float d = a - m;
        lp += -(d * d) / (2.f * expf(4.f * ls)) - 2.f * ls;
        if (live) {
          const float os = old_sigma[row * A + k], om = old_mu[row * A + k];
          const float eo = expf(os), en = expf(ls);
          kl += ls - os + (eo * eo + (om - m) * (om - m)) / (2.f * en * en) - 0.5f;     // ppo.py:482-483
        }
      }
      float dlp = 0.f, surr = 0.f;
      if (live) {
        const float ratio = expf(lp - old_logp[row]);
        const float ad = adv[row];
        const float s1 = -ad * ratio;
        const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
        const float s2 = -ad * rc;
        surr = fmaxf(s1, s2);
        const bool inside = ratio > 1.f - clip && ratio < 1.f + clip;
        dlp = (s1 > s2 || inside) ? -ad * ratio : ((s1 == s2) ? 0.5f * -ad * ratio : 0.f);
      }
      for (int k = 0; k < A; ++k) {
        const float m = Cb[r * PX_LDC + k], ls = P[D.log_std + k];
        const float a = live ? actions[row * A + k] : m;
        const float d = a - m, iv = expf(-4.f * ls);
        dcur[k * 64 + r] = live ? dlp * (d * iv) * invn : 0.f;                                   // dL/dmu
        red[r * PX_RED + 4 + k] = live ? (dlp * (2.f * d * d * iv - 2.f) * invn) : 0.f;          // dL/dlog_std via logp
      }
      red[r * PX_RED + 0] = surr;
      red[r * PX_RED + 2] = kl;
    } else {
      float vl = 0.f, dv = 0.f;
      if (live) {
        const float v = Cb[r * PX_LDC], rt = returns[row];
        if (clipped_vloss) {
          const float tv = old_values[row];
          const float diff = v - tv;
          const float vc = tv + fminf(fmaxf(diff, -clip), clip);
          const float l1 = (v - rt) * (v - rt), l2 = (vc - rt) * (vc - rt);
          vl = fmaxf(l1, l2);
          const bool inside = diff > -clip && diff < clip;
          if (l1 > l2) dv = 2.f * (v - rt);
          else if (l1 < l2) dv = inside ? 2.f * (vc - rt) : 0.f;
          else dv = inside ? 2.f * (v - rt) : (v - rt);      // tie: torch.max splits the gradient evenly
        } else {                                             // ppo.py:512: (returns - value)^2
          vl = (rt - v) * (rt - v);
          dv = 2.f * (v - rt);
        }
        dv *= vcoef * invn;
      }
      dcur[r] = dv;
      red[r * PX_RED + 1] = vl;
    }
  }
  __syncthreads();
  // ---- backward through the layers, last to first ----
  {
    const float* a = gA + (long long)(asum - V.in_w(V.nl - 1)) * 64;     // a_k: input of layer k
    for (int k = V.nl - 1; k >= 0; --k) {
      const int I = V.in_w(k), O = V.out_w(k);
      const float* W = P + V.w[k];
      float* gW = gout + V.w[k];
      float* gb = gout + V.b[k];
      load_tile_x(X, ldx, dcur, O);                                      // X = delta of layer k's output
      __syncthreads();
      if (k > 0) {
        // dprev[r][i] = (sum_o W[o][i] * delta[r][o]) * act'(a_k[r][i])
        for (int i0 = wave_id() * PX_T; i0 < I; i0 += nw * PX_T) {
          const int nt = I - i0 < PX_T ? I - i0 : PX_T;
          float acc[PX_T];
#pragma unroll
          for (int t = 0; t < PX_T; ++t) acc[t] = 0.f;
          if (nt == PX_T) {
            for (int o = 0; o < O; ++o) {
              const float d = X[r * ldx + o];
              const float* wr0 = W + (long long)o * I + i0;
#pragma unroll
              for (int t = 0; t < PX_T; ++t) acc[t] = fmaf(wr0[t], d, acc[t]);
            }
          } else {
            for (int o = 0; o < O; ++o) {
              const float d = X[r * ldx + o];
              const float* wr0 = W + (long long)o * I + i0;
#pragma unroll
              for (int t = 0; t < PX_T; ++t) if (t < nt) acc[t] = fmaf(wr0[t], d, acc[t]);
            }
          }
#pragma unroll
          for (int t = 0; t < PX_T; ++t)
            if (t < nt) dnext[(i0 + t) * 64 + r] = acc[t] * act_dfo<ACT>(a[(i0 + t) * 64 + r]);
        }
      }
      // dW[o][i] = sum_r delta[r][o] * a_k[r][i], 32 columns of a_k at a time through LDS
      for (int c0 = 0; c0 < I; c0 += PX_CH) {
        const int cw = I - c0 < PX_CH ? I - c0 : PX_CH;
        for (int c = wave_id(); c < cw; c += nw) Cb[r * PX_LDC + c] = a[(c0 + c) * 64 + r];
        __syncthreads();
        const int j = threadIdx.x & (PX_CH - 1), og = threadIdx.x / PX_CH;
        if (j < cw) {
          for (int o0 = og * PX_T; o0 < O; o0 += (PX_NT / PX_CH) * PX_T) {
            int col[PX_T];
            float acc[PX_T];
#pragma unroll
            for (int t = 0; t < PX_T; ++t) { col[t] = o0 + t < O ? o0 + t : O - 1; acc[t] = 0.f; }
            for (int rw = 0; rw < 64; ++rw) {
              const float av = Cb[rw * PX_LDC + j];
#pragma unroll
              for (int t = 0; t < PX_T; ++t) acc[t] = fmaf(X[rw * ldx + col[t]], av, acc[t]);
            }
#pragma unroll
            for (int t = 0; t < PX_T; ++t) if (o0 + t < O) gW[(long long)(o0 + t) * I + c0 + j] = acc[t];
          }
        }
        __syncthreads();
      }
      for (int o = threadIdx.x; o < O; o += PX_NT) {
        float acc = 0.f;
        for (int rw = 0; rw < 64; ++rw) acc += X[rw * ldx + o];
        gb[o] = acc;
      }
      __syncthreads();
      float* t = dcur; dcur = dnext; dnext = t;
      if (k > 0) a -= (long long)V.in_w(k - 1) * 64;
    }
  }
  if (net == 0) {
    // log_std gradient (+ entropy term: entropy = const + 2*sum(log_std) for every row -> -ecoef * 2)
    if (threadIdx.x < A) {
      float acc = 0.f;
      for (int rw = 0; rw < 64; ++rw) acc += red[rw * PX_RED + 4 + threadIdx.x];
      gout[D.log_std + threadIdx.x] = acc - ecoef * 2.f * (float)nrows * invn;
    }
    if (threadIdx.x == 64 || threadIdx.x == 66) {
      const int s = threadIdx.x - 64;
      float acc = 0.f;
      for (int rw = 0; rw < 64; ++rw) acc += red[rw * PX_RED + s];
      gout[D.total + s] = acc;
    }
    if (threadIdx.x == 67) gout[D.total + 3] = (float)nrows;
  } else if (threadIdx.x == 65) {
    float acc = 0.f;
    for (int rw = 0; rw < 64; ++rw) acc += red[rw * PX_RED + 1];
    gout[D.total + 1] = acc;
  }
}

// ---- host side ----
static int check_desc(const PolicyDesc& D) {
  RGBM_REQUIRE(D.obs_dim >= 1 && D.obs_dim <= POLICY_MAX_WIDTH, "policy desc: observation dim must be in 1..512");
  RGBM_REQUIRE(!D.asymmetric || (D.state_dim >= 1 && D.state_dim <= POLICY_MAX_WIDTH), "policy desc: state dim must be in 1..512");
  RGBM_REQUIRE(D.act_dim >= 1 && D.act_dim <= POLICY_MAX_ACT, "policy desc: action dim must be in 1..32");
  RGBM_REQUIRE(D.activation >= 0 && D.activation <= PACT_SIGMOID, "policy desc: unknown activation id");
  RGBM_REQUIRE(D.total > 0 && D.log_std >= 0 && (long long)D.log_std + D.act_dim <= D.total, "policy desc: log_std offset outside the vector");
  for (int net = 0; net < 2; ++net) {
    const int nh = D.n_hidden[net];
    RGBM_REQUIRE(nh >= 1 && nh <= POLICY_MAX_HIDDEN, "policy desc: each net needs 1..6 hidden layers");
    int in = (net == 1 && D.asymmetric) ? D.state_dim : D.obs_dim;
    for (int k = 0; k <= nh; ++k) {
      const int out = k == nh ? (net == 0 ? D.act_dim : 1) : D.hidden[net][k];
      RGBM_REQUIRE(out >= 1 && out <= POLICY_MAX_WIDTH, "policy desc: hidden width must be in 1..512");
      RGBM_REQUIRE(D.w[net][k] >= 0 && (long long)D.w[net][k] + (long long)out * in <= D.total && D.b[net][k] >= 0 &&
                       (long long)D.b[net][k] + out <= D.total, "policy desc: layer offset outside the vector");
      in = out;
    }
  }
  return 0;
}

// the shipped shape's specialisation: the descriptor as a PolicyLayout when the kernels at the top of this file cover it
static bool legacy_shape(const PolicyDesc& D, PolicyLayout* L) {
  if (D.activation != PACT_ELU || D.asymmetric || D.n_hidden[0] != 3 || D.n_hidden[1] != 3 || D.act_dim > 16) return false;
  if (D.obs_dim > PK_MAXW) return false;
  int asum = D.obs_dim + 1, wmax = D.act_dim;
  for (int k = 0; k < 3; ++k) {
    if (D.hidden[0][k] != D.hidden[1][k] || D.hidden[0][k] > PK_MAXW) return false;
    asum += D.hidden[0][k] + 1;
    if (D.hidden[0][k] > wmax) wmax = D.hidden[0][k];
  }
  if ((size_t)(PK_ROWS * (asum + 2 * (wmax + 1)) + PK_ROWS * 20) * sizeof(float) > 160 * 1024) return false;
  L->dims[0] = D.obs_dim;
  for (int k = 0; k < 3; ++k) L->dims[k + 1] = D.hidden[0][k];
  L->dims[4] = D.act_dim;
  L->log_std = D.log_std;
  for (int net = 0; net < 2; ++net)
    for (int k = 0; k < 4; ++k) { L->w[net][k] = D.w[net][k]; L->b[net][k] = D.b[net][k]; }
  L->total = D.total;
  return true;
}

// widest operand of either net (inputs, hidden layers, outputs) and the scratch floats of one (tile, net)
static void desc_extent(const PolicyDesc& D, int* maxw, long long* region) {
  int mw = 1;
  long long reg = 0;
  for (int net = 0; net < 2; ++net) {
    int in = (net == 1 && D.asymmetric) ? D.state_dim : D.obs_dim;
    int asum = in, maxd = net == 0 ? D.act_dim : 1;
    if (in > mw) mw = in;
    for (int k = 0; k < D.n_hidden[net]; ++k) {
      const int h = D.hidden[net][k];
      asum += h;
      if (h > maxd) maxd = h;
    }
    if (maxd > mw) mw = maxd;
    const long long rg = 64LL * (asum + 2 * maxd);
    if (rg > reg) reg = rg;
  }
  *maxw = mw;
  *region = reg;
}

template <int ACT>
static int launch_forward_act(const float* params, const PolicyDesc& D, int n, int mode, const float* obs, const float* states,
                              const float* noise, float* actions, float* logp, float* value, float* mu, hipStream_t s) {
  int maxw;
  long long region;
  desc_extent(D, &maxw, &region);
  const int ld = maxw + 1;
  const int R = (size_t)2 * 64 * ld * sizeof(float) <= 160 * 1024 ? 64 : 32;
  const size_t lds = (size_t)2 * R * ld * sizeof(float);
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(policy_forward_x_kernel<ACT>), (int)lds)) return rc;
  hipLaunchKernelGGL(policy_forward_x_kernel<ACT>, dim3((n + R - 1) / R, mode == 1 ? 1 : 2), dim3(PX_NT), lds, s, params, D, n, mode,
                     R, ld, obs, states, noise, actions, logp, value, mu);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_policy_forward_ex(const float* params, const PolicyDesc& D, int n, int mode, const float* obs, const float* states,
                             const float* noise, float* actions, float* logp, float* value, float* mu, hipStream_t s) {
  if (int rc = check_desc(D)) return rc;
  RGBM_REQUIRE(n > 0 && mode >= 0 && mode <= 2, "policy_forward_ex arguments");
  RGBM_REQUIRE(!D.asymmetric || mode == 1 || states, "policy_forward_ex: an asymmetric critic needs states");
  PolicyLayout L;
  if (legacy_shape(D, &L)) return launch_policy_forward(params, L, n, mode, obs, noise, actions, logp, value, mu, s);
  switch (D.activation) {
    case PACT_ELU: return launch_forward_act<PACT_ELU>(params, D, n, mode, obs, states, noise, actions, logp, value, mu, s);
    case PACT_SELU: return launch_forward_act<PACT_SELU>(params, D, n, mode, obs, states, noise, actions, logp, value, mu, s);
    case PACT_RELU: return launch_forward_act<PACT_RELU>(params, D, n, mode, obs, states, noise, actions, logp, value, mu, s);
    case PACT_LRELU: return launch_forward_act<PACT_LRELU>(params, D, n, mode, obs, states, noise, actions, logp, value, mu, s);
    case PACT_TANH: return launch_forward_act<PACT_TANH>(params, D, n, mode, obs, states, noise, actions, logp, value, mu, s);
    default: return launch_forward_act<PACT_SIGMOID>(params, D, n, mode, obs, states, noise, actions, logp, value, mu, s);
  }
}

int ppo_scratch_floats_ex(const PolicyDesc& D, int n, int clipped_vloss, size_t* count) {
  if (int rc = check_desc(D)) return rc;
  RGBM_REQUIRE(n > 0, "ppo_scratch_floats_ex rows");
  const size_t nblk = (size_t)(n + 63) / 64;
  PolicyLayout L;
  if (clipped_vloss && legacy_shape(D, &L)) { *count = (size_t)policy_partial_floats(L, n); return 0; }
  int maxw;
  long long region;
  desc_extent(D, &maxw, &region);
  *count = nblk * (size_t)(D.total + 4) + nblk * 2 * (size_t)region;
  return 0;
}

template <int ACT>
static int launch_minibatch_act(const float* params, const PolicyDesc& D, int n, const float* obs, const float* states,
                                const float* actions, const float* old_logp, const float* adv, const float* returns,
                                const float* old_values, const float* old_mu, const float* old_sigma, float clip, float vcoef,
                                float ecoef, int clipped_vloss, float* scratch, hipStream_t s) {
  int maxw;
  long long region;
  desc_extent(D, &maxw, &region);
  const int nblk = (n + 63) / 64, pstride = D.total + 4, ldx = maxw + 1;
  const size_t lds = (size_t)64 * (ldx + PX_LDC + PX_RED) * sizeof(float);
  RGBM_REQUIRE(lds <= 160 * 1024, "policy operand tile exceeds LDS");
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(ppo_loss_grad_x_kernel<ACT>), (int)lds)) return rc;
  hipLaunchKernelGGL(ppo_loss_grad_x_kernel<ACT>, dim3(nblk, 2), dim3(PX_NT), lds, s, params, D, n, ldx, obs, states, actions, old_logp,
                     adv, returns, old_values, old_mu, old_sigma, clip, vcoef, ecoef, clipped_vloss, scratch, pstride,
                     scratch + (size_t)nblk * pstride, region);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_ppo_minibatch_ex(const float* params, const PolicyDesc& D, int n, const float* obs, const float* states,
                            const float* actions, const float* old_logp, const float* adv, const float* returns,
                            const float* old_values, const float* old_mu, const float* old_sigma, float clip, float vcoef, float ecoef,
                            int clipped_vloss, float* scratch, float* grads, hipStream_t s) {
  if (int rc = check_desc(D)) return rc;
  RGBM_REQUIRE(n > 0, "ppo_minibatch_ex rows");
  RGBM_REQUIRE(!D.asymmetric || states, "ppo_minibatch_ex: an asymmetric critic needs states");
  RGBM_REQUIRE(!clipped_vloss || old_values, "ppo_minibatch_ex: the clipped value loss needs old_values");
  PolicyLayout L;
  if (clipped_vloss && legacy_shape(D, &L))
    return launch_ppo_minibatch(params, L, n, obs, actions, old_logp, adv, returns, old_values, old_mu, old_sigma, clip, vcoef, ecoef,
                                scratch, grads, s);
  int rc;
#define RGBM_PX_CASE(A)                                                                                                          \
  case A: rc = launch_minibatch_act<A>(params, D, n, obs, states, actions, old_logp, adv, returns, old_values, old_mu, old_sigma, \
                                       clip, vcoef, ecoef, clipped_vloss, scratch, s); break;
  switch (D.activation) {
    RGBM_PX_CASE(PACT_ELU)
    RGBM_PX_CASE(PACT_SELU)
    RGBM_PX_CASE(PACT_RELU)
    RGBM_PX_CASE(PACT_LRELU)
    RGBM_PX_CASE(PACT_TANH)
    default: rc = launch_minibatch_act<PACT_SIGMOID>(params, D, n, obs, states, actions, old_logp, adv, returns, old_values, old_mu,
                                                         old_sigma, clip, vcoef, ecoef, clipped_vloss, scratch, s);
  }
#undef RGBM_PX_CASE
  if (rc) return rc;
  const int nblk = (n + 63) / 64, pstride = D.total + 4;
  hipLaunchKernelGGL(ppo_reduce_kernel, dim3((pstride + 255) / 256), dim3(256), 0, s, scratch, nblk, pstride, pstride, grads);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
