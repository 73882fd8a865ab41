// lg_train.hip — gfx950 kernels of PPO.update (include/lgtrain.h) for the feed-forward ActorCritic: one optimiser step is eight launches and no
// host synchronisation.
//
//   ppo_forward_kernel      32 rows of the mini-batch through ALL layers of a network (blockIdx.y: actor / critic), the tile of mlp_tile in
//                           lg_policy.hip: same activation image in LDS, same tiled weights (the lg_mlp's own buffers), the same k-ordered MFMA chain
//                           per accumulator, bias and apply_act -- so the values are lg_mlp_forward's bit for bit.  The rows are gathered through the
//                           index vector while staging; every layer's post-activation output is also written to a workspace.
//                           ppo_wide_forward_kernel: the same body (lg_train_forward_body.h) with a split-K first layer, for observation rows wider than
//                           one activation image (lg_mlp_create_wide).
//   ppo_loss_kernel         one lane per row: log-prob, ratio, both surrogate branches, the value loss, the KL term; dL/dmu, dL/dvalue, the row's
//                           part of dL/dsigma; per-block sums in a fixed order.
//   ppo_loss_finish_kernel  the block sums in block order -> the four loss means, the gradient of std / log_std, the KL-adaptive learning rate.
//   ppo_backward_kernel     delta_l = (delta_{l+1} W_{l+1}) * act'(a_l): the same 32-row tile run down the network on a second, TRANSPOSED tiling
//                           of the weights; act' is a function of the saved output a_l.  Every delta is written out.
//   ppo_wgrad_kernel        dW_l = delta_{l+1}^T a_l and db_l (a column of ones appended to a_l): the reduction runs over the batch, split into slabs
//                           of WGRAD_SLAB rows (blockIdx.y); a wave owns a 32 x 64 tile of dW and reads both operands straight from the workspaces.
//   ppo_grad_reduce_kernel  the slab partials in slab order -> the gradient in torch's layout, and per-block sums of squares.
//   ppo_norm_finish_kernel  the global norm, the clip coefficient, the step count and Adam's bias corrections.
//   ppo_adam_kernel         clip + Adam on the fp32 masters (torch's layout); the same lane rewrites the element in the forward tiling, in the
//                           transposed tiling, and (std segment) in the device std vector the acts read.
// No atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_train_internal.h"
#include "../../include/lgtrain.h"

#define LOSS_ROWS 256         // rows per block of the loss kernel
#define LOSS_SLOTS 36         // surrogate, value, (entropy), KL, then up to 32 sigma gradients

// the networks, segments, masters and workspaces are the shared core's (lg_train_internal.h); nstd = A: std / log_std trails the flat vector
struct lg_ppo : TrainCore {
  lg_mlp* actor = nullptr; lg_mlp* critic = nullptr;
  int A = 0;
  int loss_blocks = 0;
  float* loss_part = nullptr;
};

LG_DEV float act_grad_from_output(float a, int act) {
  switch (act) {
    case LG_ACT_ELU: return a > 0.f ? 1.f : a + 1.f;
    case LG_ACT_RELU: return a > 0.f ? 1.f : 0.f;
    case LG_ACT_TANH: return 1.f - a * a;
    case LG_ACT_LRELU: return a > 0.f ? 1.f : 0.01f;
    case LG_ACT_SELU: return a > 0.f ? 1.0507009873554805f : a + 1.0507009873554805f * 1.6732632423543772f;
  }
  return 1.f;
}

// columns [k0, k0 + Kp) of rows of `src` (width K, optionally gathered through idx) -> activation image of padded width Kp
LG_DEV void stage_rows(const float* __restrict__ src, const int64_t* __restrict__ idx, int K, int Kp, int64_t row0, int64_t n, float* img, int k0 = 0) {
  const int tid = threadIdx.x;
  for (int base = 0; base < MLP_ROWS * Kp; base += 4 * MLP_THREADS) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * MLP_THREADS + tid, r = e / Kp, k = e - r * Kp;
      const int64_t row = row0 + r;
      float val = 0.f;
      if (e < MLP_ROWS * Kp && row < n && k0 + k < K) val = src[(idx ? idx[row] : row) * K + k0 + k];
      v[u] = val;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * MLP_THREADS + tid, r = e / Kp, k = e - r * Kp;
      if (e < MLP_ROWS * Kp) img[IMG(r, k)] = v[u];
    }
  }
}

// the epilogue of chunk c of layer l of the training forward: bias, activation, the next layer's image, and the saved output a[l + 1]
LG_DEV void forward_chunk_out(const float* __restrict__ fb, float* save, int nout, bool last, int act, int c, const f32x4& acc0, const f32x4& acc1, float* out,
                              int64_t row0, int64_t n) {
  const int lane = threadIdx.x & 63;
  const int col = c * 16 + (lane & 15);
  const float bias = fb[col];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = 4 * (lane >> 4) + i;
    float v0 = acc0[i] + bias, v1 = acc1[i] + bias;
    if (!last) {
      v0 = apply_act(v0, act); v1 = apply_act(v1, act);
      if (col >= nout) { v0 = 0.f; v1 = 0.f; }
      out[IMG(m, col)] = v0;
      out[IMG(m + 16, col)] = v1;
    }
    if (col < nout) {
      if (row0 + m < n) save[(row0 + m) * nout + col] = v0;
      if (row0 + m + 16 < n) save[(row0 + m + 16) * nout + col] = v1;
    }
  }
}

// the training forward (its body: lg_train_forward_body.h), and its instance for networks with more than MLP_MAXW inputs
__global__ __launch_bounds__(MLP_THREADS) void ppo_forward_kernel(TrainNet NA, TrainNet NC, const float* __restrict__ obs, const float* __restrict__ cobs,
                                                                  const int64_t* __restrict__ idx, int64_t n) {
#define PPO_FORWARD_WIDE 0
#include "lg_train_forward_body.h"
#undef PPO_FORWARD_WIDE
}

__global__ __launch_bounds__(MLP_THREADS) void ppo_wide_forward_kernel(TrainNet NA, TrainNet NC, const float* __restrict__ obs, const float* __restrict__ cobs,
                                                                       const int64_t* __restrict__ idx, int64_t n) {
#define PPO_FORWARD_WIDE 1
#include "lg_train_forward_body.h"
#undef PPO_FORWARD_WIDE
}

__global__ __launch_bounds__(MLP_THREADS) void ppo_backward_kernel(TrainNet NA, TrainNet NC, int64_t n) {
  __shared__ __attribute__((aligned(16))) float buf0[MLP_IMG];
  __shared__ __attribute__((aligned(16))) float buf1[MLP_IMG];
  const TrainNet& M = blockIdx.y == 0 ? NA : NC;
  if (M.L < 2) return;
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  stage_rows(M.d[M.L - 1], nullptr, M.dims[M.L], M.bkpad[M.L - 1], row0, n, buf0);
  lds_barrier();
  float* in = buf0; float* out = buf1;
  for (int l = M.L - 1; l >= 1; --l) {                    // layer l's weights take d[l] (width dims[l + 1]) to d[l - 1] (width dims[l])
    const int nblk = M.bkpad[l] >> 4, nch = M.bnch[l], nout = M.dims[l];
    const float4* ap = reinterpret_cast<const float4*>(in) + (lane & 15) * 4 + (lane >> 4);
    const float4* wl = reinterpret_cast<const float4*>(M.bw[l]) + lane;
    const float* __restrict__ aout = M.a[l];
    float* dst = M.d[l - 1];
    for (int c = wv; c < nch; c += MLP_THREADS / 64) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      chunk_chain(wl + (size_t)c * nblk * 64, ap, nblk, acc0, acc1);
      const int col = c * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * (lane >> 4) + i;
        float v0 = 0.f, v1 = 0.f;
        if (col < nout) {
          if (row0 + m < n) { v0 = acc0[i] * act_grad_from_output(aout[(row0 + m) * nout + col], M.act); dst[(row0 + m) * nout + col] = v0; }
          if (row0 + m + 16 < n) { v1 = acc1[i] * act_grad_from_output(aout[(row0 + m + 16) * nout + col], M.act); dst[(row0 + m + 16) * nout + col] = v1; }
        }
        if (l > 1) {                                         // the last step's image feeds nothing
          out[IMG(m, col)] = v0;
          out[IMG(m + 16, col)] = v1;
        }
      }
    }
    lds_barrier();
    float* t = in; in = out; out = t;
  }
}

// per mini-batch row i (rollout row r = idx[i]).  part[block][LOSS_SLOTS]: sums over the block's rows of surrogate, value loss, 0, KL, and the rows'
// contributions to dL/dsigma_a, each ALREADY divided by n where the loss is a mean.
__global__ __launch_bounds__(LOSS_ROWS) void ppo_loss_kernel(lg_ppo_rows R, const int64_t* __restrict__ idx, int64_t n, int A, const float* __restrict__ mu_new,
                                                             const float* __restrict__ val_new, const float* __restrict__ stdv, lg_ppo_hyper H,
                                                             float* __restrict__ dmu, float* __restrict__ dval, float* __restrict__ part) {
  __shared__ float red[LOSS_ROWS][LOSS_SLOTS + 1];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * LOSS_ROWS + tid;
  for (int s = 0; s < LOSS_SLOTS; ++s) red[tid][s] = 0.f;
  if (i < n) {
    const int64_t r = idx[i];
    const float invn = 1.f / (float)n;
    const float adv = R.advantages[r], ret = R.returns[r], oldv = R.values[r], oldlp = R.actions_log_prob[r], v = val_new[i];
    float logp = 0.f, kl = 0.f;
    for (int a = 0; a < A; ++a) {
      const float mu = mu_new[i * A + a], sd = stdv[a], dd = R.actions[r * A + a] - mu;
      logp += -(dd * dd) / (2.f * sd * sd) - logf(sd) - 0.91893853320467274178f;
      const float om = R.mu[r * A + a], os = R.sigma[r * A + a];
      kl += logf(sd / os + 1.0e-5f) + (os * os + (om - mu) * (om - mu)) / (2.f * sd * sd) - 0.5f;
    }
    const float ratio = expf(logp - oldlp), lo = 1.f - H.clip_param, hi = 1.f + H.clip_param;
    const float s1 = -adv * ratio, s2 = -adv * fminf(fmaxf(ratio, lo), hi);
    // torch.max splits a tie evenly and clamp passes the gradient inside its bounds: inside the clip both branches are the same number and the
    // two halves add up to -adv; outside, only the unclipped branch carries a gradient, and only where it is the larger one
    const bool inside = ratio >= lo && ratio <= hi;
    const float glp = ((inside || s1 > s2) ? -adv : 0.f) * ratio * invn;           // dL / dlogp_i
    for (int a = 0; a < A; ++a) {
      const float mu = mu_new[i * A + a], sd = stdv[a], dd = R.actions[r * A + a] - mu;
      dmu[i * A + a] = glp * (dd / (sd * sd));
      red[tid][4 + a] = glp * (dd * dd / (sd * sd * sd) - 1.f / sd);
    }
    float vl, gv;
    if (H.use_clipped_value_loss) {
      const float dv = v - oldv, vc = oldv + fminf(fmaxf(dv, -H.clip_param), H.clip_param);
      const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
      const float g1 = 2.f * (v - ret), g2 = (dv >= -H.clip_param && dv <= H.clip_param) ? 2.f * (vc - ret) : 0.f;
      vl = fmaxf(l1, l2);
      gv = l1 > l2 ? g1 : (l2 > l1 ? g2 : 0.5f * (g1 + g2));
    } else {
      vl = (ret - v) * (ret - v);
      gv = 2.f * (v - ret);
    }
    dval[i] = H.value_loss_coef * gv * invn;
    red[tid][0] = fmaxf(s1, s2) * invn;
    red[tid][1] = vl * invn;
    red[tid][3] = kl * invn;
  }
  __syncthreads();
  if (tid < LOSS_SLOTS) {
    float s = 0.f;
    for (int rr = 0; rr < LOSS_ROWS; ++rr) s += red[rr][tid];
    part[(size_t)blockIdx.x * LOSS_SLOTS + tid] = s;
  }
}

__global__ __launch_bounds__(64) void ppo_loss_finish_kernel(const float* __restrict__ part, int nblocks, int A, const float* __restrict__ stdv, int std_type,
                                                             lg_ppo_hyper H, float* __restrict__ gstd, TrainScalars* __restrict__ sc, int accumulate) {
  __shared__ float tot[LOSS_SLOTS];
  const int tid = threadIdx.x;
  if (tid < LOSS_SLOTS) {
    float s = 0.f;
    for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * LOSS_SLOTS + tid];
    tot[tid] = s;
  }
  __syncthreads();
  if (tid >= 4 && tid < 4 + A) {
    const float sd = stdv[tid - 4];
    float g = tot[tid] - H.entropy_coef / sd;                 // the entropy bonus: -entropy_coef * d/dsigma (0.5 + log sqrt(2 pi) + log sigma)
    if (std_type == LG_STD_LOG) g *= sd;                      // sigma = exp(log_std)
    gstd[tid - 4] = g;
  }
  if (tid == 0) {
    float ent = 0.f;
    for (int a = 0; a < A; ++a) ent += 0.5f + 0.91893853320467274178f + logf(stdv[a]);
    const float klm = tot[3];
    sc->means[0] = tot[0]; sc->means[1] = tot[1]; sc->means[2] = ent; sc->means[3] = klm;
    double lr = sc->lr;
    if (H.schedule == LG_SCHEDULE_ADAPTIVE) {                  // ppo.py:301-304
      const double kl = (double)klm, want = H.desired_kl;
      if (kl > want * 2.0) lr = fmax(1e-5, lr / 1.5);
      else if (kl < want / 2.0 && kl > 0.0) lr = fmin(1e-2, lr * 1.5);
      sc->lr = lr;
    }
    if (accumulate) { sc->acc[0] += (double)tot[1]; sc->acc[1] += (double)tot[0]; sc->acc[2] += (double)ent; sc->acc[3] += (double)klm; }
  }
}

// dW = D^T [A | 1] over the rows of one slab.  MFMA 16x16x4: A operand lane (m = lane & 15, k = lane >> 4) = D[row k][o m], B operand lane
// (k = lane >> 4, n = lane & 15) = A[row k][i n]; C[m = 4 (lane >> 4) + t][n = lane & 15].  Rows in ascending order per accumulator.
__global__ __launch_bounds__(256) void ppo_wgrad_kernel(const TrainSeg* __restrict__ segs, const float* __restrict__ obs, const float* __restrict__ cobs,
                                                        const int64_t* __restrict__ idx, int64_t n) {
  const TrainSeg S = segs[blockIdx.z];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int dO = S.dO, dI = S.dI, W = dI + 1;
  const int to = (dO + 31) / 32, ti = (W + 63) / 64;
  const int tile = blockIdx.x * 4 + wv;
  const int64_t r0 = (int64_t)blockIdx.y * WGRAD_SLAB;
  if (tile >= to * ti || r0 >= n) return;
  const int64_t r1 = r0 + WGRAD_SLAB < n ? r0 + WGRAD_SLAB : n;
  const int o0 = (tile / ti) * 32, i0 = (tile % ti) * 64;
  const float* __restrict__ Ain = S.Ain ? S.Ain : (S.net == 0 ? obs : cobs);
  const bool gather = S.Ain == nullptr;
  const int oc = o0 + (lane & 15), ic = i0 + (lane & 15);
  f32x4 acc[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[h][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t ks = r0; ks < r1; ks += 4) {
    const int64_t row = ks + (lane >> 4);
    const bool valid = row < r1;
    float av[2], bv[4];
    const int64_t src = valid ? (gather ? idx[row] : row) : 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) av[h] = (valid && oc + 16 * h < dO) ? S.D[row * dO + oc + 16 * h] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = ic + 16 * q;
      bv[q] = !valid ? 0.f : (i < dI ? Ain[src * dI + i] : (i == dI ? 1.f : 0.f));
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[h][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[h], bv[q], acc[h][q], 0, 0, 0);
  }
  float* __restrict__ P = S.partial + (size_t)blockIdx.y * dO * W;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int o = o0 + 16 * h + 4 * (lane >> 4) + t, i = ic + 16 * q;
        if (o < dO && i < W) P[(size_t)o * W + i] = acc[h][q][t];
      }
}

__global__ __launch_bounds__(256) void ppo_grad_reduce_kernel(const TrainSeg* __restrict__ segs, int nslabs, float* __restrict__ G, float* __restrict__ norm_part) {
  __shared__ float red[256];
  const TrainSeg S = segs[blockIdx.y];
  const int W = S.dI + 1;
  const int64_t count = (int64_t)S.dO * W, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float g = 0.f;
  if (e < count) {
    for (int s = 0; s < nslabs; ++s) g += S.partial[(size_t)s * count + e];
    const int o = (int)(e / W), i = (int)(e - (int64_t)o * W);
    G[i < S.dI ? S.woff + (int64_t)o * S.dI + i : S.boff + o] = g;
  }
  const float s = block_sum_256(g * g, red);
  if (threadIdx.x == 0) norm_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void ppo_norm_finish_kernel(const float* __restrict__ norm_part, int count, const float* __restrict__ gstd, int A, float max_grad_norm,
                                                              int clip_on, TrainScalars* __restrict__ sc) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < count; i += 256) s += norm_part[i];
  if ((int)threadIdx.x < A) s += gstd[threadIdx.x] * gstd[threadIdx.x];
  const float total = block_sum_256(s, red);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(total);
    sc->norm = norm;
    sc->clip = clip_on ? fminf(1.f, max_grad_norm / (norm + 1e-6f)) : 1.f;  // clip_grad_norm_; off: the gradient passes as it is
    const int64_t t = sc->step + 1;
    sc->step = t;
    sc->step_size = (float)(sc->lr / (1.0 - pow(0.9, (double)t)));         // torch.optim.Adam, defaults
    sc->bc2_sqrt = (float)sqrt(1.0 - pow(0.999, (double)t));
  }
}

// blockIdx.y < nseg: a (network, layer); == nseg: std / log_std.  retile_only: no step, the masters are written to the tilings as they are.
__global__ __launch_bounds__(256) void ppo_adam_kernel(const TrainSeg* __restrict__ segs, int nseg, int64_t std_off, int A, int std_type, float* __restrict__ std_dev,
                                                       float* __restrict__ theta, float* __restrict__ m1, float* __restrict__ m2, const float* __restrict__ G,
                                                       const TrainScalars* __restrict__ sc, int retile_only) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool is_std = (int)blockIdx.y == nseg;
  TrainSeg S;
  int o = 0, i = 0;
  int64_t flat;
  if (is_std) {
    if (e >= A) return;
    flat = std_off + e;
  } else {
    S = segs[blockIdx.y];
    const int W = S.dI + 1;
    if (e >= (int64_t)S.dO * W) return;
    o = (int)(e / W); i = (int)(e - (int64_t)o * W);
    flat = i < S.dI ? S.woff + (int64_t)o * S.dI + i : S.boff + o;
  }
  float th = theta[flat];
  if (!retile_only) {
    const float g = G[flat] * sc->clip;
    float a = m1[flat], b = m2[flat];
    a = a + (g - a) * 0.1f;                                   // exp_avg.lerp_(grad, 1 - beta1)
    b = b * 0.999f + 0.001f * g * g;                          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    m1[flat] = a; m2[flat] = b;
    th = th - sc->step_size * (a / (sqrtf(b) / sc->bc2_sqrt + 1e-8f));
    theta[flat] = th;
  }
  if (is_std) { std_dev[e] = std_type == LG_STD_LOG ? expf(th) : th; return; }
  if (i == S.dI) { if (S.fb) S.fb[o] = th; return; }
  // forward tiling: chunk o / 16, block i / 16, lane (o % 16) + 16 (i % 4), slot (i / 4) % 4 (lg_mlp_create)
  if (S.fw) S.fw[((((size_t)(o >> 4) * S.f_nb + (i >> 4)) * 64) + ((o & 15) | ((i & 3) << 4))) * 4 + ((i >> 2) & 3)] = th;
  // transposed tiling: the same with o and i exchanged
  if (S.bw) S.bw[((((size_t)(i >> 4) * S.b_nb + (o >> 4)) * 64) + ((i & 15) | ((o & 3) << 4))) * 4 + ((o >> 2) & 3)] = th;
}

// mode 0: clear the update's sums; 1: the means over `steps` steps and the learning rate -> stats
__global__ void ppo_stats_kernel(TrainScalars* __restrict__ sc, lg_ppo_stats* __restrict__ stats, int mode, int steps) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (mode == 0) { for (int k = 0; k < 4; ++k) sc->acc[k] = 0.0; return; }
  stats->value_function = sc->acc[0] / steps; stats->surrogate = sc->acc[1] / steps; stats->entropy = sc->acc[2] / steps; stats->kl = sc->acc[3] / steps;
  stats->learning_rate = sc->lr;
}

// ------------------------------------------------------------------------------------------------------------------------ host side
// ---- what the trainers share (lg_train_internal.h)
void* train_alloc(TrainCore* p, size_t bytes, bool zero) {
  void* d = nullptr;
  if (bytes == 0) bytes = 4;
  if (hipMalloc(&d, bytes) != hipSuccess) { lg_policy_fail(LG_ERR_HIP, "workspace allocation failed"); return nullptr; }
  p->allocs.push_back(d);
  if (zero && hipMemset(d, 0, bytes) != hipSuccess) { lg_policy_fail(LG_ERR_HIP, "workspace allocation failed"); return nullptr; }
  return d;
}

void train_core_free(TrainCore* c) {
  for (void* d : c->allocs) (void)hipFree(d);
  c->allocs.clear();
}

bool train_core_add_net(TrainCore* c, const lg_mlp* net, int64_t* off) {
  bool ok = true;
  auto alloc = [&](size_t floats, bool zero) -> float* { float* d = ok ? (float*)train_alloc(c, floats * sizeof(float), zero) : nullptr; if (!d) ok = false; return d; };
  const int slabs_max = (int)((c->max_rows + WGRAD_SLAB - 1) / WGRAD_SLAB);
  const int k = c->nnet++;
  const MlpDev& h = net->h;
  TrainNet& N = c->net[k];
  N.L = h.L; N.act = h.act;
  for (int l = 0; l <= h.L; ++l) N.dims[l] = h.dims[l];
  N.a[0] = nullptr;
  for (int l = 0; l < h.L; ++l) {
    const int dI = h.dims[l], dO = h.dims[l + 1];
    N.fkpad[l] = h.kpad[l]; N.fnch[l] = h.nchunks[l]; N.fw[l] = h.w[l]; N.fb[l] = h.b[l];
    N.bkpad[l] = (dO + 63) & ~63; N.bnch[l] = ((dI + 63) & ~63) / 16;
    N.bw[l] = l > 0 ? alloc((size_t)N.bnch[l] * (N.bkpad[l] / 16) * 64 * 4, true) : nullptr;
    N.a[l + 1] = alloc((size_t)c->max_rows * dO, false);
    N.d[l] = alloc((size_t)c->max_rows * dO, false);
    TrainSeg& S = c->seg[c->nseg++];
    S.net = k; S.layer = l; S.dO = dO; S.dI = dI; S.f_nb = h.kpad[l] / 16; S.b_nb = N.bkpad[l] / 16;
    S.woff = *off; *off += (int64_t)dO * dI; S.boff = *off; *off += dO;
    S.D = N.d[l]; S.Ain = l > 0 ? N.a[l] : nullptr;
    S.partial = alloc((size_t)slabs_max * dO * (dI + 1), false);
    S.fw = const_cast<float*>(h.w[l]); S.fb = const_cast<float*>(h.b[l]); S.bw = const_cast<float*>(N.bw[l]);
    const int64_t cnt = (int64_t)dO * (dI + 1);
    if (cnt > c->big) c->big = cnt;
    const int tiles = ((dO + 31) / 32) * ((dI + 1 + 63) / 64);
    if ((tiles + 3) / 4 > c->wgrad_blocks) c->wgrad_blocks = (tiles + 3) / 4;
  }
  return ok;
}

TrainSeg& train_core_add_seg(TrainCore* c, int net, int layer_id, int dO, int dI, const float* D, const float* Ain, float* fw, float* fb, int f_nb, float* bw, int b_nb,
                             bool* ok) {
  const int slabs_max = (int)((c->max_rows + WGRAD_SLAB - 1) / WGRAD_SLAB);
  TrainSeg& S = c->seg[c->nseg++];
  S.net = net; S.layer = layer_id; S.dO = dO; S.dI = dI; S.f_nb = f_nb; S.b_nb = b_nb; S.woff = 0; S.boff = 0;
  S.D = D; S.Ain = Ain; S.fw = fw; S.fb = fb; S.bw = bw;
  S.partial = *ok ? (float*)train_alloc(c, (size_t)slabs_max * dO * (dI + 1) * sizeof(float), false) : nullptr;
  if (!S.partial) *ok = false;
  const int64_t cnt = (int64_t)dO * (dI + 1);
  if (cnt > c->big) c->big = cnt;
  const int tiles = ((dO + 31) / 32) * ((dI + 1 + 63) / 64);
  if ((tiles + 3) / 4 > c->wgrad_blocks) c->wgrad_blocks = (tiles + 3) / 4;
  return S;
}

static int train_core_retile_or_step(TrainCore* p, hipStream_t st, bool step) {
  hipLaunchKernelGGL(ppo_adam_kernel, dim3((unsigned)((p->big + 255) / 256), p->nseg + (p->nstd > 0 ? 1 : 0)), dim3(256), 0, st, p->d_seg, p->nseg, p->std_off,
                     p->nstd, p->std_type, p->std_dev, p->theta, p->m, p->v, p->G, p->sc, step ? 0 : 1);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int train_core_retile(TrainCore* c, hipStream_t st) { return train_core_retile_or_step(c, st, false); }

int train_core_finish(TrainCore* c, int64_t off, const float* const* const* ws, const float* const* const* bs, const float* tail, double learning_rate) {
  bool ok = true;
  auto alloc = [&](size_t floats, bool zero) -> float* { float* d = ok ? (float*)train_alloc(c, floats * sizeof(float), zero) : nullptr; if (!d) ok = false; return d; };
  c->std_off = off; c->P = off + c->nstd;
  if (c->nstd > c->big) c->big = c->nstd;
  c->red_blocks = (int)((c->big + 255) / 256);
  c->theta = alloc(c->P, false); c->m = alloc(c->P, true); c->v = alloc(c->P, true); c->G = alloc(c->P, true);
  c->norm_part = alloc((size_t)c->red_blocks * c->nseg, true);
  c->sc = ok ? (TrainScalars*)train_alloc(c, sizeof(TrainScalars), true) : nullptr;
  c->d_seg = ok && c->sc ? (TrainSeg*)train_alloc(c, sizeof(TrainSeg) * TRAIN_MAX_SEGS, true) : nullptr;
  if (!ok || !c->sc || !c->d_seg) return LG_ERR_HIP;
  // the masters, in the flat order of the module's parameters()
  std::vector<float> flat((size_t)c->P);
  for (int s = 0; s < c->nseg; ++s) {
    const TrainSeg& S = c->seg[s];
    const float* w = ws[S.net][S.layer]; const float* b = bs[S.net][S.layer];
    for (int64_t e = 0; e < (int64_t)S.dO * S.dI; ++e) flat[S.woff + e] = w[e];
    for (int o = 0; o < S.dO; ++o) flat[S.boff + o] = b[o];
  }
  for (int a = 0; a < c->nstd; ++a) flat[c->std_off + a] = tail[a];
  TrainScalars sc0{};
  sc0.lr = learning_rate; sc0.clip = 1.f;
  if (hipMemcpy(c->theta, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_seg, c->seg, sizeof(TrainSeg) * c->nseg, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->sc, &sc0, sizeof(sc0), hipMemcpyHostToDevice) != hipSuccess)
    return lg_policy_fail(LG_ERR_HIP, "parameter upload failed");
  const int rc = train_core_retile(c, nullptr);
  if (rc != LG_OK) return rc;
  POLICY_TRY(hipDeviceSynchronize());
  return LG_OK;
}

void train_launch_forward(const TrainCore* c, const float* obs, const float* cobs, const int64_t* idx, int64_t n, hipStream_t st) {
  const unsigned tiles = (unsigned)((n + MLP_ROWS - 1) / MLP_ROWS);
  bool wide = false;
  for (int k = 0; k < c->nnet; ++k) wide |= c->net[k].fkpad[0] > MLP_MAXW;
  hipLaunchKernelGGL(wide ? ppo_wide_forward_kernel : ppo_forward_kernel, dim3(tiles, c->nnet), dim3(MLP_THREADS), 0, st, c->net[0], c->net[c->nnet - 1],
                     obs, cobs, idx, n);
}

void train_launch_backward(const TrainCore* c, int64_t n, hipStream_t st) {
  const unsigned tiles = (unsigned)((n + MLP_ROWS - 1) / MLP_ROWS);
  bool any = false;
  for (int k = 0; k < c->nnet; ++k) any |= c->net[k].L > 1;
  if (any) hipLaunchKernelGGL(ppo_backward_kernel, dim3(tiles, c->nnet), dim3(MLP_THREADS), 0, st, c->net[0], c->net[c->nnet - 1], n);
}

void train_launch_backward_net(const TrainCore* c, int k, int64_t n, hipStream_t st) {
  const unsigned tiles = (unsigned)((n + MLP_ROWS - 1) / MLP_ROWS);
  if (c->net[k].L > 1) hipLaunchKernelGGL(ppo_backward_kernel, dim3(tiles, 1), dim3(MLP_THREADS), 0, st, c->net[k], c->net[k], n);
}

int train_launch_optimise(TrainCore* c, const float* obs, const float* cobs, const int64_t* idx, int64_t n, float max_grad_norm, int clip_on, hipStream_t st) {
  const int nslabs = (int)((n + WGRAD_SLAB - 1) / WGRAD_SLAB);
  hipLaunchKernelGGL(ppo_wgrad_kernel, dim3(c->wgrad_blocks, nslabs, c->nseg), dim3(256), 0, st, (const TrainSeg*)c->d_seg, obs, cobs, idx, n);
  hipLaunchKernelGGL(ppo_grad_reduce_kernel, dim3(c->red_blocks, c->nseg), dim3(256), 0, st, (const TrainSeg*)c->d_seg, nslabs, c->G, c->norm_part);
  hipLaunchKernelGGL(ppo_norm_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)c->norm_part, c->red_blocks * c->nseg, (const float*)(c->G + c->std_off), c->nstd,
                     max_grad_norm, clip_on, c->sc);
  return train_core_retile_or_step(c, st, true);
}

// the passes of train_launch_optimise one by one, for a trainer whose segments do not all share a row count (the estimator's convolutions bring their
// own weight-gradient kernel and slab counts): segments [seg0, seg0 + count) only
void train_launch_wgrad_range(const TrainCore* c, int seg0, int count, const float* obs, const float* cobs, const int64_t* idx, int64_t n, hipStream_t st) {
  const int nslabs = (int)((n + WGRAD_SLAB - 1) / WGRAD_SLAB);
  hipLaunchKernelGGL(ppo_wgrad_kernel, dim3(c->wgrad_blocks, nslabs, count), dim3(256), 0, st, (const TrainSeg*)(c->d_seg + seg0), obs, cobs, idx, n);
}

void train_launch_reduce_range(const TrainCore* c, int seg0, int count, int nslabs, hipStream_t st) {
  hipLaunchKernelGGL(ppo_grad_reduce_kernel, dim3(c->red_blocks, count), dim3(256), 0, st, (const TrainSeg*)(c->d_seg + seg0), nslabs, c->G,
                     c->norm_part + (size_t)seg0 * c->red_blocks);
}

int train_launch_norm_adam(TrainCore* c, float max_grad_norm, int clip_on, hipStream_t st) {
  hipLaunchKernelGGL(ppo_norm_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)c->norm_part, c->red_blocks * c->nseg, (const float*)(c->G + c->std_off), c->nstd,
                     max_grad_norm, clip_on, c->sc);
  return train_core_retile_or_step(c, st, true);
}

// ---- the entry points every trainer exports under its own prefix (lg_train_internal.h)
int64_t train_api_parameter_count(TrainCore* p) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  return p->P;
}

int64_t train_api_workspace_bytes(TrainCore* p) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  DeviceScope ds_(p->device);
  int64_t total = 0;
  for (void* d : p->allocs) {
    size_t bytes = 0;
    if (hipMemPtrGetInfo(d, &bytes) == hipSuccess) total += (int64_t)bytes;
  }
  return total;
}

static int train_core_get_state(TrainCore* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, hipStream_t st) {
  POLICY_TRY(hipStreamSynchronize(st));
  const size_t bytes = (size_t)p->P * sizeof(float);
  if (params) POLICY_TRY(hipMemcpy(params, p->theta, bytes, hipMemcpyDeviceToHost));
  if (exp_avg) POLICY_TRY(hipMemcpy(exp_avg, p->m, bytes, hipMemcpyDeviceToHost));
  if (exp_avg_sq) POLICY_TRY(hipMemcpy(exp_avg_sq, p->v, bytes, hipMemcpyDeviceToHost));
  TrainScalars sc;
  POLICY_TRY(hipMemcpy(&sc, p->sc, sizeof(sc), hipMemcpyDeviceToHost));
  if (step) *step = sc.step;
  if (lr) *lr = sc.lr;
  return LG_OK;
}

static int train_core_set_state(TrainCore* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, hipStream_t st) {
  POLICY_TRY(hipStreamSynchronize(st));
  const size_t bytes = (size_t)p->P * sizeof(float);
  POLICY_TRY(hipMemcpy(p->theta, params, bytes, hipMemcpyHostToDevice));
  POLICY_TRY(hipMemcpy(p->m, exp_avg, bytes, hipMemcpyHostToDevice));
  POLICY_TRY(hipMemcpy(p->v, exp_avg_sq, bytes, hipMemcpyHostToDevice));
  TrainScalars sc;
  POLICY_TRY(hipMemcpy(&sc, p->sc, sizeof(sc), hipMemcpyDeviceToHost));
  sc.step = step; sc.lr = lr;
  POLICY_TRY(hipMemcpy(p->sc, &sc, sizeof(sc), hipMemcpyHostToDevice));
  const int rc = train_core_retile(p, st);
  if (rc != LG_OK) return rc;
  POLICY_TRY(hipStreamSynchronize(st));
  return LG_OK;
}

int train_api_get_state(TrainCore* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  DeviceScope ds_(p->device);
  return train_core_get_state(p, params, exp_avg, exp_avg_sq, step, lr, (hipStream_t)stream);
}

int train_api_get_parameters(TrainCore* p, float* params, void* stream) {
  if (!p || !params) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  return train_api_get_state(p, params, nullptr, nullptr, nullptr, nullptr, stream);
}

int train_api_set_state(TrainCore* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  if (!p || !params || !exp_avg || !exp_avg_sq) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  if (step < 0 || !(lr > 0.0)) return lg_policy_fail(LG_ERR_INVALID, "step < 0 or learning rate <= 0");
  DeviceScope ds_(p->device);
  hipStream_t st = (hipStream_t)stream;
  int rc = train_core_set_state(p, params, exp_avg, exp_avg_sq, step, lr, st);
  if (rc != LG_OK || !p->retile_own) return rc;
  if ((rc = p->retile_own(p, st)) != LG_OK) return rc;
  POLICY_TRY(hipStreamSynchronize(st));
  return LG_OK;
}

int train_api_set_learning_rate(TrainCore* p, double lr, void* stream) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!(lr > 0.0)) return lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  POLICY_TRY(hipMemcpy(&p->sc->lr, &lr, sizeof(double), hipMemcpyHostToDevice));
  return LG_OK;
}

int train_api_group_gradients(TrainCore* p, float* g, float* norm, float* losses, int64_t capacity, void* stream) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (losses && capacity < p->last_steps) return lg_policy_fail(LG_ERR_INVALID, "the last group had more steps than the buffer holds");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (g) POLICY_TRY(hipMemcpy(g, p->G, (size_t)p->P * sizeof(float), hipMemcpyDeviceToHost));
  if (norm) POLICY_TRY(hipMemcpy(norm, &p->sc->norm, sizeof(float), hipMemcpyDeviceToHost));
  if (losses && p->last_steps > 0) POLICY_TRY(hipMemcpy(losses, p->group_loss, (size_t)p->last_steps * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int train_api_step_losses(TrainCore* p, float* losses, int64_t count, void* stream) {
  if (!p || !losses) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  if (count < 0 || count > p->last_update_steps) return lg_policy_fail(LG_ERR_INVALID, "count exceeds the steps of the last update");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (count > 0) POLICY_TRY(hipMemcpy(losses, p->seq_loss, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

size_t train_ppo_loss_floats(int64_t max_rows) { return (size_t)((max_rows + LOSS_ROWS - 1) / LOSS_ROWS) * LOSS_SLOTS; }

void train_launch_ppo_loss(TrainCore* p, const lg_ppo_rows* r, const int64_t* idx, int64_t n, const lg_ppo_hyper* h, float* loss_part, int accumulate, hipStream_t st) {
  const int loss_blocks = (int)((n + LOSS_ROWS - 1) / LOSS_ROWS);
  const TrainNet &NA = p->net[0], &NC = p->net[1];
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(loss_blocks), dim3(LOSS_ROWS), 0, st, *r, idx, n, p->nstd, (const float*)NA.a[NA.L], (const float*)NC.a[NC.L],
                     (const float*)p->std_dev, *h, NA.d[NA.L - 1], NC.d[NC.L - 1], loss_part);
  hipLaunchKernelGGL(ppo_loss_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)loss_part, loss_blocks, p->nstd, (const float*)p->std_dev, p->std_type, *h,
                     p->G + p->std_off, p->sc, accumulate);
}

void train_launch_ppo_stats(TrainCore* c, lg_ppo_stats* stats, int mode, int steps, hipStream_t st) {
  hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(1), 0, st, c->sc, stats, mode, steps);
}

// ---- PPO
static int train_check_call(lg_ppo* p, const lg_ppo_rows* r, const int64_t* idx, const lg_ppo_hyper* h) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!r || !idx || !h) return lg_policy_fail(LG_ERR_INVALID, "null rows, indices or hyper-parameters");
  if (!r->observations || !r->critic_observations || !r->actions || !r->values || !r->returns || !r->advantages || !r->actions_log_prob || !r->mu || !r->sigma)
    return lg_policy_fail(LG_ERR_INVALID, "null row pointer");
  if (h->schedule != LG_SCHEDULE_FIXED && h->schedule != LG_SCHEDULE_ADAPTIVE) return lg_policy_fail(LG_ERR_INVALID, "unknown schedule (fixed | adaptive)");
  return LG_OK;
}

static int train_step(lg_ppo* p, const lg_ppo_rows* r, const int64_t* idx, int64_t n, const lg_ppo_hyper* h, hipStream_t st, int accumulate) {
  p->last_rows = n;
  const int loss_blocks = (int)((n + LOSS_ROWS - 1) / LOSS_ROWS);
  const TrainNet &NA = p->net[0], &NC = p->net[1];
  train_launch_forward(p, r->observations, r->critic_observations, idx, n, st);
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(loss_blocks), dim3(LOSS_ROWS), 0, st, *r, idx, n, p->A, (const float*)NA.a[NA.L], (const float*)NC.a[NC.L],
                     (const float*)p->std_dev, *h, NA.d[NA.L - 1], NC.d[NC.L - 1], p->loss_part);
  hipLaunchKernelGGL(ppo_loss_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)p->loss_part, loss_blocks, p->A, (const float*)p->std_dev, p->std_type, *h,
                     p->G + p->std_off, p->sc, accumulate);
  train_launch_backward(p, n, st);
  return train_launch_optimise(p, r->observations, r->critic_observations, idx, n, h->max_grad_norm, 1, st);
}

extern "C" {

int32_t lg_ppo_wgrad_slab_rows(void) { return WGRAD_SLAB; }

void lg_ppo_destroy(lg_ppo* p) {
  if (!p) return;
  DeviceScope ds_(p->device);
  (void)hipDeviceSynchronize();
  train_core_free(p);
  delete p;
}

lg_ppo* lg_ppo_create(lg_mlp* actor, lg_mlp* critic, const float* const* aw, const float* const* ab, const float* const* cw, const float* const* cb,
                      const float* std_host, int32_t noise_std_type, double learning_rate, int64_t max_rows, float* std_device) {
  POLICY_ENTRY;
  if (!actor || !critic) { lg_policy_fail(LG_ERR_INVALID, "null network"); return nullptr; }
  if (!aw || !ab || !cw || !cb || !std_host || !std_device) { lg_policy_fail(LG_ERR_INVALID, "null parameter list or std vector"); return nullptr; }
  if (noise_std_type != LG_STD_SCALAR && noise_std_type != LG_STD_LOG) { lg_policy_fail(LG_ERR_INVALID, "unknown noise_std_type (scalar | log)"); return nullptr; }
  if (max_rows < 1) { lg_policy_fail(LG_ERR_INVALID, "max_rows < 1"); return nullptr; }
  if (!(learning_rate > 0.0)) { lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0"); return nullptr; }
  if (actor->device != critic->device) { lg_policy_fail(LG_ERR_INVALID, "the actor and the critic live on different devices"); return nullptr; }
  if (actor->h.act_out || critic->h.act_out) { lg_policy_fail(LG_ERR_UNSUPPORTED, "a network with an output activation cannot be trained here"); return nullptr; }
  if (critic->h.dims[critic->h.L] != 1) { lg_policy_fail(LG_ERR_UNSUPPORTED, "the critic must end in 1 output"); return nullptr; }
  if (actor->h.dims[actor->h.L] > 32) { lg_policy_fail(LG_ERR_UNSUPPORTED, "the actor ends in more than 32 actions"); return nullptr; }
  const lg_mlp* nets[2] = {actor, critic};
  const float* const* ws[2] = {aw, cw};
  const float* const* bs[2] = {ab, cb};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < nets[k]->h.L; ++l)
      if (!ws[k][l] || !bs[k][l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  if (!lg_policy_device_ok(actor->device)) return nullptr;
  DeviceScope ds_(actor->device);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_ppo* p = new lg_ppo();
  p->actor = actor; p->critic = critic; p->device = actor->device; p->A = actor->h.dims[actor->h.L]; p->max_rows = max_rows;
  p->nstd = p->A; p->std_type = noise_std_type; p->std_dev = std_device;
  int64_t off = 0;
  bool ok = train_core_add_net(p, actor, &off) && train_core_add_net(p, critic, &off);
  p->loss_blocks = (int)((max_rows + LOSS_ROWS - 1) / LOSS_ROWS);
  p->loss_part = ok ? (float*)train_alloc(p, (size_t)p->loss_blocks * LOSS_SLOTS * sizeof(float), true) : nullptr;
  if (!ok || !p->loss_part || train_core_finish(p, off, ws, bs, std_host, learning_rate) != LG_OK) { lg_ppo_destroy(p); return nullptr; }
  return p;
}

int lg_ppo_minibatch(lg_ppo* p, const lg_ppo_rows* rows, const int64_t* indices, int64_t count, const lg_ppo_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  const int rc = train_check_call(p, rows, indices, hyper);
  if (rc != LG_OK) return rc;
  if (count <= 0) return lg_policy_fail(LG_ERR_INVALID, "count <= 0");
  if (count > p->max_rows) return lg_policy_fail(LG_ERR_INVALID, "count > max_rows of the trainer");
  DeviceScope ds_(p->device);
  return train_step(p, rows, indices, count, hyper, (hipStream_t)stream, 0);
}

int lg_ppo_update(lg_ppo* p, const lg_ppo_rows* rows, int64_t R, const int64_t* indices, int32_t num_mini_batches, int32_t num_learning_epochs,
                  const lg_ppo_hyper* hyper, lg_ppo_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = train_check_call(p, rows, indices, hyper);
  if (rc != LG_OK) return rc;
  if (num_mini_batches < 1 || num_learning_epochs < 1) return lg_policy_fail(LG_ERR_INVALID, "num_mini_batches < 1 or num_learning_epochs < 1");
  const int64_t mini = R / num_mini_batches;
  if (mini <= 0) return lg_policy_fail(LG_ERR_INVALID, "R / num_mini_batches == 0");
  if (mini > p->max_rows) return lg_policy_fail(LG_ERR_INVALID, "R / num_mini_batches > max_rows of the trainer");
  DeviceScope ds_(p->device);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(1), 0, st, p->sc, stats, 0, 1);
  for (int e = 0; e < num_learning_epochs; ++e)
    for (int i = 0; i < num_mini_batches; ++i) {
      const int r2 = train_step(p, rows, indices + (int64_t)i * mini, mini, hyper, st, 1);
      if (r2 != LG_OK) return r2;
    }
  if (stats) hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(1), 0, st, p->sc, stats, 1, num_mini_batches * num_learning_epochs);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int64_t lg_ppo_parameter_count(lg_ppo* p) {
  POLICY_ENTRY;
  return train_api_parameter_count(p);
}

int lg_ppo_gradients(lg_ppo* p, float* g, float* norm, float* means, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (g) POLICY_TRY(hipMemcpy(g, p->G, (size_t)p->P * sizeof(float), hipMemcpyDeviceToHost));
  TrainScalars sc;
  POLICY_TRY(hipMemcpy(&sc, p->sc, sizeof(sc), hipMemcpyDeviceToHost));
  if (norm) *norm = sc.norm;
  if (means) for (int k = 0; k < 4; ++k) means[k] = sc.means[k];
  return LG_OK;
}

int lg_ppo_forward_outputs(lg_ppo* p, float* mean, float* values, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (p->last_rows <= 0) return lg_policy_fail(LG_ERR_INVALID, "no mini-batch has run yet");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const TrainNet &NA = p->net[0], &NC = p->net[1];
  if (mean) POLICY_TRY(hipMemcpy(mean, NA.a[NA.L], (size_t)p->last_rows * p->A * sizeof(float), hipMemcpyDeviceToHost));
  if (values) POLICY_TRY(hipMemcpy(values, NC.a[NC.L], (size_t)p->last_rows * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int lg_ppo_get_state(lg_ppo* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  POLICY_ENTRY;
  return train_api_get_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_ppo_get_parameters(lg_ppo* p, float* params, void* stream) {
  POLICY_ENTRY;
  return train_api_get_parameters(p, params, stream);
}

int lg_ppo_set_state(lg_ppo* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_ppo_set_learning_rate(lg_ppo* p, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_learning_rate(p, lr, stream);
}

}  // extern "C"
