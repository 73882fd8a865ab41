// lg_train_symmetry.hip — gfx950 kernels of PPO.update with symmetry augmentation and the mirror loss (include/lgtrain_symmetry.h), a trainer on the
// shared core of lg_train_internal.h.  The augmentation function arrives as signed-permutation tables and is applied where rows are staged: logical
// row i of a mini-batch of B rows is block k = i / B of mini-batch row j = i - k B, and column c of it is sign_k[c] * src[idx[j]][perm_k[c]].  The
// actor runs on nA = K B rows; the critic on nC = K B rows with data augmentation and on nC = B rows without.
//
//   sym_fwd_kernel          the forward tile of lg_train.hip (same image, same tiled weights, same k-ordered MFMA chain, so block 0 gives its
//                           values bit for bit) with the table applied while staging, and a row count per network.
//   sym_loss_kernel         one lane per logical row: the clipped losses on the rows they cover (all with augmentation, block 0 without) with the
//                           transformed actions, KL over block 0, the mirror term of rows >= B against the transformed output of row j; dL/dmu,
//                           dL/dvalue; per-block sums in a fixed order (slot 2: the symmetry sum).
//   sym_loss_finish_kernel  the block sums in block order -> the five means, the gradient of std / log_std, the KL-adaptive learning rate.
//   sym_wgrad_kernel        the slab weight gradients of lg_train.hip with the table applied to the layer-0 operand and a row count per network.
//   sym_stats_kernel        clears / reports the update's sums.
// The backward data pass, the slab reduction, the norm and Adam are lg_train.hip's launches.  No atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_train_internal.h"
#include "../../include/lgtrain_symmetry.h"

#define SYM_LOSS_ROWS 256     // rows per block of the loss kernel
#define SYM_LOSS_SLOTS 36     // surrogate, value, symmetry, KL, then up to 32 sigma gradients

// (K, W) tables on the device
struct SymTable {
  const int32_t* perm;
  const float* sign;
  int W;
};

struct SymScalars {
  double acc;                        // sum over an update's steps of the symmetry loss
  float mean;                        // last mini-batch
};

struct lg_ppo_sym : TrainCore {
  lg_mlp* actor = nullptr; lg_mlp* critic = nullptr;
  int A = 0, K = 0, aug = 0, mirror = 0;
  float coeff = 0.f;
  int64_t rows_max = 0, last_actor_rows = 0, last_critic_rows = 0;    // rows_max: mini-batch rows B the workspaces were sized for
  SymTable tobs{}, tcobs{}, tact{};
  float* loss_part = nullptr;
  SymScalars* ss = nullptr;
};

// logical rows [row0, row0 + 32) of a network's input -> activation image of padded width Kp
LG_DEV void sym_stage_rows(const float* __restrict__ src, const int64_t* __restrict__ idx, SymTable T, int Kp, int row0, int B, int n, float* img) {
  const int tid = threadIdx.x, K = T.W;
  for (int base = 0; base < MLP_ROWS * Kp; base += 4 * MLP_THREADS) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * MLP_THREADS + tid, r = e / Kp, k = e - r * Kp;
      const int row = row0 + r;
      float val = 0.f;
      if (e < MLP_ROWS * Kp && row < n && k < K) {
        const int blk = row / B, j = row - blk * B, t = blk * K + k;
        val = T.sign[t] * src[idx[j] * K + T.perm[t]];
      }
      v[u] = val;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * MLP_THREADS + tid, r = e / Kp, k = e - r * Kp;
      if (e < MLP_ROWS * Kp) img[IMG(r, k)] = v[u];
    }
  }
}

__global__ __launch_bounds__(MLP_THREADS) void sym_fwd_kernel(TrainNet NA, TrainNet NC, const float* __restrict__ obs, const float* __restrict__ cobs,
                                                              const int64_t* __restrict__ idx, int B, int nA, int nC, SymTable TA, SymTable TC) {
  __shared__ __attribute__((aligned(16))) float buf0[MLP_IMG];
  __shared__ __attribute__((aligned(16))) float buf1[MLP_IMG];
  const TrainNet& M = blockIdx.y == 0 ? NA : NC;
  const int n = blockIdx.y == 0 ? nA : nC;
  const int row0 = (int)blockIdx.x * MLP_ROWS;
  if (row0 >= n) return;                                     // the critic's grid is the actor's
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  sym_stage_rows(blockIdx.y == 0 ? obs : cobs, idx, blockIdx.y == 0 ? TA : TC, M.fkpad[0], row0, B, n, buf0);
  lds_barrier();
  float* in = buf0; float* out = buf1;
  for (int l = 0; l < M.L; ++l) {
    const int nblk = M.fkpad[l] >> 4, nch = M.fnch[l], nout = M.dims[l + 1];
    const bool last = l == M.L - 1;
    const float4* ap = reinterpret_cast<const float4*>(in) + (lane & 15) * 4 + (lane >> 4);
    const float4* wl = reinterpret_cast<const float4*>(M.fw[l]) + lane;
    float* save = M.a[l + 1];
    for (int c = wv; c < nch; c += MLP_THREADS / 64) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      chunk_chain(wl + (size_t)c * nblk * 64, ap, nblk, acc0, acc1);
      const int col = c * 16 + (lane & 15);
      const float bias = M.fb[l][col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * (lane >> 4) + i;
        float v0 = acc0[i] + bias, v1 = acc1[i] + bias;
        if (!last) {
          v0 = apply_act(v0, M.act); v1 = apply_act(v1, M.act);
          if (col >= nout) { v0 = 0.f; v1 = 0.f; }
          out[IMG(m, col)] = v0;
          out[IMG(m + 16, col)] = v1;
        }
        if (col < nout) {
          if (row0 + m < n) save[(int64_t)(row0 + m) * nout + col] = v0;
          if (row0 + m + 16 < n) save[(int64_t)(row0 + m + 16) * nout + col] = v1;
        }
      }
    }
    lds_barrier();
    float* t = in; in = out; out = t;
  }
}

// per logical row i = k B + j (rollout row r = idx[j]).  part[block][SYM_LOSS_SLOTS]: sums over the block's rows of surrogate, value loss, symmetry
// loss, KL, and the rows' contributions to dL/dsigma_a, each ALREADY divided by its divisor: K B (augmentation) or B for the clipped losses, B for
// the KL, (K - 1) B A for the symmetry loss.  cm: mirror_loss_coeff, 0 when the term is only reported.
__global__ __launch_bounds__(SYM_LOSS_ROWS) void sym_loss_kernel(lg_ppo_rows R, const int64_t* __restrict__ idx, int B, int K, int aug, float cm, int A, SymTable TACT,
                                                                 const float* __restrict__ mu_new, const float* __restrict__ val_new, const float* __restrict__ stdv,
                                                                 lg_ppo_hyper H, float* __restrict__ dmu, float* __restrict__ dval, float* __restrict__ part) {
  __shared__ float red[SYM_LOSS_ROWS][SYM_LOSS_SLOTS + 1];
  const int tid = threadIdx.x;
  const int i = (int)blockIdx.x * SYM_LOSS_ROWS + tid, nA = K * B;
  for (int s = 0; s < SYM_LOSS_SLOTS; ++s) red[tid][s] = 0.f;
  if (i < nA) {
    const int k = i / B, j = i - k * B;
    const int64_t r = idx[j];
    const int32_t* __restrict__ ap = TACT.perm + k * A;
    const float* __restrict__ as = TACT.sign + k * A;
    const float* __restrict__ mu_i = mu_new + (int64_t)i * A;
    const bool ppo = aug || k == 0;                           // the clipped losses cover this row
    float glp = 0.f;
    if (ppo) {
      const float invn = 1.f / (float)(aug ? nA : B);
      const float adv = R.advantages[r], ret = R.returns[r], oldv = R.values[r], oldlp = R.actions_log_prob[r], v = val_new[i];
      float logp = 0.f, kl = 0.f;
      for (int a = 0; a < A; ++a) {
        const float mu = mu_i[a], sd = stdv[a], dd = as[a] * R.actions[r * A + ap[a]] - mu;
        logp += -(dd * dd) / (2.f * sd * sd) - logf(sd) - 0.91893853320467274178f;
        if (k == 0) {                                         // ppo.py:275-289: the KL of the original rows
          const float om = R.mu[r * A + a], os = R.sigma[r * A + a];
          kl += logf(sd / os + 1.0e-5f) + (os * os + (om - mu) * (om - mu)) / (2.f * sd * sd) - 0.5f;
        }
      }
      const float ratio = expf(logp - oldlp), lo = 1.f - H.clip_param, hi = 1.f + H.clip_param;
      const float s1 = -adv * ratio, s2 = -adv * fminf(fmaxf(ratio, lo), hi);
      const bool inside = ratio >= lo && ratio <= hi;         // the tie rule of ppo_loss_kernel
      glp = ((inside || s1 > s2) ? -adv : 0.f) * ratio * invn;
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
      red[tid][3] = kl / (float)B;
    }
    const float invm = 1.f / ((float)(K - 1) * (float)B * (float)A);
    const float* __restrict__ mu_j = mu_new + (int64_t)j * A;
    float sym = 0.f;
    for (int a = 0; a < A; ++a) {
      const float mu = mu_i[a], sd = stdv[a];
      float g = 0.f;
      if (ppo) {
        const float dd = as[a] * R.actions[r * A + ap[a]] - mu;
        g = glp * (dd / (sd * sd));
        red[tid][4 + a] = glp * (dd * dd / (sd * sd * sd) - 1.f / sd);
      }
      if (k > 0) {                                            // ppo.py:356-365: the target is the transformed mean of the original row, detached
        const float diff = mu - as[a] * mu_j[ap[a]];
        sym += diff * diff * invm;
        g += cm * 2.f * diff * invm;
      }
      dmu[(int64_t)i * A + a] = g;
    }
    red[tid][2] = sym;
  }
  __syncthreads();
  if (tid < SYM_LOSS_SLOTS) {
    float s = 0.f;
    for (int rr = 0; rr < SYM_LOSS_ROWS; ++rr) s += red[rr][tid];
    part[(size_t)blockIdx.x * SYM_LOSS_SLOTS + tid] = s;
  }
}

__global__ __launch_bounds__(64) void sym_loss_finish_kernel(const float* __restrict__ part, int nblocks, int A, const float* __restrict__ stdv, int std_type,
                                                             lg_ppo_hyper H, float* __restrict__ gstd, TrainScalars* __restrict__ sc, SymScalars* __restrict__ ss,
                                                             int accumulate) {
  __shared__ float tot[SYM_LOSS_SLOTS];
  const int tid = threadIdx.x;
  if (tid < SYM_LOSS_SLOTS) {
    float s = 0.f;
    for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * SYM_LOSS_SLOTS + tid];
    tot[tid] = s;
  }
  __syncthreads();
  if (tid >= 4 && tid < 4 + A) {
    const float sd = stdv[tid - 4];
    float g = tot[tid] - H.entropy_coef / sd;                 // the entropy of the first B rows: one row's, whatever B
    if (std_type == LG_STD_LOG) g *= sd;
    gstd[tid - 4] = g;
  }
  if (tid == 0) {
    float ent = 0.f;
    for (int a = 0; a < A; ++a) ent += 0.5f + 0.91893853320467274178f + logf(stdv[a]);
    const float klm = tot[3];
    sc->means[0] = tot[0]; sc->means[1] = tot[1]; sc->means[2] = ent; sc->means[3] = klm;
    ss->mean = tot[2];
    double lr = sc->lr;
    if (H.schedule == LG_SCHEDULE_ADAPTIVE) {                  // ppo.py:301-304
      const double kl = (double)klm, want = H.desired_kl;
      if (kl > want * 2.0) lr = fmax(1e-5, lr / 1.5);
      else if (kl < want / 2.0 && kl > 0.0) lr = fmin(1e-2, lr * 1.5);
      sc->lr = lr;
    }
    if (accumulate) {
      sc->acc[0] += (double)tot[1]; sc->acc[1] += (double)tot[0]; sc->acc[2] += (double)ent; sc->acc[3] += (double)klm;
      ss->acc += (double)tot[2];
    }
  }
}

// ppo_wgrad_kernel of lg_train.hip with the layer-0 operand read through the tables and a row count per network: same tiles, same slabs, rows in
// ascending order per accumulator.
__global__ __launch_bounds__(256) void sym_wgrad_kernel(const TrainSeg* __restrict__ segs, const float* __restrict__ obs, const float* __restrict__ cobs,
                                                        const int64_t* __restrict__ idx, int B, int nA, int nC, SymTable TA, SymTable TC) {
  const TrainSeg S = segs[blockIdx.z];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int dO = S.dO, dI = S.dI, W = dI + 1;
  const int to = (dO + 31) / 32, ti = (W + 63) / 64;
  const int tile = blockIdx.x * 4 + wv;
  const int n = S.net == 0 ? nA : nC;
  const int r0 = (int)blockIdx.y * WGRAD_SLAB;
  if (tile >= to * ti || r0 >= n) return;
  const int r1 = r0 + WGRAD_SLAB < n ? r0 + WGRAD_SLAB : n;
  const int o0 = (tile / ti) * 32, i0 = (tile % ti) * 64;
  const bool gather = S.Ain == nullptr;
  const float* __restrict__ Ain = gather ? (S.net == 0 ? obs : cobs) : S.Ain;
  const SymTable T = S.net == 0 ? TA : TC;
  const int oc = o0 + (lane & 15), ic = i0 + (lane & 15);
  f32x4 acc[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[h][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = r0; ks < r1; ks += 4) {
    const int row = ks + (lane >> 4);
    const bool valid = row < r1;
    float av[2], bv[4];
    int64_t src = valid ? row : 0;
    int tb = 0;
    if (gather && valid) { const int blk = row / B; src = idx[row - blk * B]; tb = blk * dI; }
#pragma unroll
    for (int h = 0; h < 2; ++h) av[h] = (valid && oc + 16 * h < dO) ? S.D[(int64_t)row * dO + oc + 16 * h] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = ic + 16 * q;
      float b = 0.f;
      if (valid) {
        if (i < dI) b = gather ? T.sign[tb + i] * Ain[src * dI + T.perm[tb + i]] : Ain[src * dI + i];
        else if (i == dI) b = 1.f;
      }
      bv[q] = b;
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

// mode 0: clear the update's sums; 1: the means over `steps` steps and the learning rate -> stats
__global__ void sym_stats_kernel(TrainScalars* __restrict__ sc, SymScalars* __restrict__ ss, lg_ppo_sym_stats* __restrict__ stats, int mode, int steps) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (mode == 0) { for (int k = 0; k < 4; ++k) sc->acc[k] = 0.0; ss->acc = 0.0; return; }
  stats->value_function = sc->acc[0] / steps; stats->surrogate = sc->acc[1] / steps; stats->entropy = sc->acc[2] / steps; stats->kl = sc->acc[3] / steps;
  stats->learning_rate = sc->lr;
  stats->symmetry = ss->acc / steps;
}

// ------------------------------------------------------------------------------------------------------------------------ host side
static int sym_check_call(lg_ppo_sym* p, const lg_ppo_rows* r, const int64_t* idx, const lg_ppo_hyper* h) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!r || !idx || !h) return lg_policy_fail(LG_ERR_INVALID, "null rows, indices or hyper-parameters");
  if (!r->observations || !r->critic_observations || !r->actions || !r->values || !r->returns || !r->advantages || !r->actions_log_prob || !r->mu || !r->sigma)
    return lg_policy_fail(LG_ERR_INVALID, "null row pointer");
  if (h->schedule != LG_SCHEDULE_FIXED && h->schedule != LG_SCHEDULE_ADAPTIVE) return lg_policy_fail(LG_ERR_INVALID, "unknown schedule (fixed | adaptive)");
  return LG_OK;
}

static int sym_step(lg_ppo_sym* p, const lg_ppo_rows* r, const int64_t* idx, int64_t count, const lg_ppo_hyper* h, hipStream_t st, int accumulate) {
  const int B = (int)count, nA = p->K * B, nC = p->aug ? nA : B;
  p->last_rows = count; p->last_actor_rows = nA; p->last_critic_rows = nC;
  const int loss_blocks = (nA + SYM_LOSS_ROWS - 1) / SYM_LOSS_ROWS;
  const int slabsA = (nA + WGRAD_SLAB - 1) / WGRAD_SLAB, slabsC = (nC + WGRAD_SLAB - 1) / WGRAD_SLAB;
  const TrainNet &NA = p->net[0], &NC = p->net[1];
  hipLaunchKernelGGL(sym_fwd_kernel, dim3((unsigned)((nA + MLP_ROWS - 1) / MLP_ROWS), 2), dim3(MLP_THREADS), 0, st, NA, NC, r->observations, r->critic_observations,
                     idx, B, nA, nC, p->tobs, p->tcobs);
  hipLaunchKernelGGL(sym_loss_kernel, dim3(loss_blocks), dim3(SYM_LOSS_ROWS), 0, st, *r, idx, B, p->K, p->aug, p->mirror ? p->coeff : 0.f, p->A, p->tact,
                     (const float*)NA.a[NA.L], (const float*)NC.a[NC.L], (const float*)p->std_dev, *h, NA.d[NA.L - 1], NC.d[NC.L - 1], p->loss_part);
  hipLaunchKernelGGL(sym_loss_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)p->loss_part, loss_blocks, p->A, (const float*)p->std_dev, p->std_type, *h,
                     p->G + p->std_off, p->sc, p->ss, accumulate);
  if (nA == nC) train_launch_backward(p, nA, st);
  else { train_launch_backward_net(p, 0, nA, st); train_launch_backward_net(p, 1, nC, st); }
  hipLaunchKernelGGL(sym_wgrad_kernel, dim3(p->wgrad_blocks, slabsA, p->nseg), dim3(256), 0, st, (const TrainSeg*)p->d_seg, r->observations, r->critic_observations,
                     idx, B, nA, nC, p->tobs, p->tcobs);
  train_launch_reduce_range(p, 0, NA.L, slabsA, st);
  train_launch_reduce_range(p, NA.L, NC.L, slabsC, st);
  return train_launch_norm_adam(p, h->max_grad_norm, 1, st);
}

// the K x W table of one kind, checked and uploaded; false + message on refusal
static bool sym_upload_table(lg_ppo_sym* p, const char* what, int K, int W, int want, const int32_t* perm, const float* sign, SymTable* out) {
  if (W != want) { lg_policy_fail(LG_ERR_INVALID, std::string("the ") + what + " table is " + std::to_string(W) + " wide, the network takes " + std::to_string(want)); return false; }
  if (!perm || !sign) { lg_policy_fail(LG_ERR_INVALID, std::string("null ") + what + " table"); return false; }
  for (int k = 0; k < K; ++k)
    for (int c = 0; c < W; ++c) {
      const int32_t s = perm[k * W + c];
      const float g = sign[k * W + c];
      if (s < 0 || s >= W) { lg_policy_fail(LG_ERR_INVALID, std::string("the ") + what + " table has an index out of range"); return false; }
      if (g != 1.f && g != -1.f) { lg_policy_fail(LG_ERR_INVALID, std::string("the ") + what + " table has a sign that is not +1 or -1"); return false; }
      if (k == 0 && (s != c || g != 1.f)) { lg_policy_fail(LG_ERR_INVALID, std::string("block 0 of the ") + what + " table is not the identity"); return false; }
    }
  int32_t* dp = (int32_t*)train_alloc(p, (size_t)K * W * sizeof(int32_t), false);
  float* ds = dp ? (float*)train_alloc(p, (size_t)K * W * sizeof(float), false) : nullptr;
  if (!dp || !ds) return false;
  if (hipMemcpy(dp, perm, (size_t)K * W * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ds, sign, (size_t)K * W * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { lg_policy_fail(LG_ERR_HIP, "table upload failed"); return false; }
  out->perm = dp; out->sign = ds; out->W = W;
  return true;
}

extern "C" {

void lg_ppo_sym_destroy(lg_ppo_sym* p) {
  if (!p) return;
  DeviceScope ds_(p->device);
  (void)hipDeviceSynchronize();
  train_core_free(p);
  delete p;
}

lg_ppo_sym* lg_ppo_sym_create(lg_mlp* actor, lg_mlp* critic, const float* const* aw, const float* const* ab, const float* const* cw, const float* const* cb,
                              const float* std_host, int32_t noise_std_type, double learning_rate, int64_t max_rows, float* std_device,
                              const lg_ppo_sym_tables* tables, const lg_ppo_sym_config* config) {
  POLICY_ENTRY;
  if (!actor || !critic) { lg_policy_fail(LG_ERR_INVALID, "null network"); return nullptr; }
  if (!aw || !ab || !cw || !cb || !std_host || !std_device) { lg_policy_fail(LG_ERR_INVALID, "null parameter list or std vector"); return nullptr; }
  if (!tables || !config) { lg_policy_fail(LG_ERR_INVALID, "null tables or config"); return nullptr; }
  if (noise_std_type != LG_STD_SCALAR && noise_std_type != LG_STD_LOG) { lg_policy_fail(LG_ERR_INVALID, "unknown noise_std_type (scalar | log)"); return nullptr; }
  if (max_rows < 1) { lg_policy_fail(LG_ERR_INVALID, "max_rows < 1"); return nullptr; }
  if (!(learning_rate > 0.0)) { lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0"); return nullptr; }
  const int K = tables->num_blocks;
  if (K < 2 || K > LG_PPO_SYM_MAX_BLOCKS) {
    lg_policy_fail(LG_ERR_INVALID, "num_blocks " + std::to_string(K) + " is outside [2, LG_PPO_SYM_MAX_BLOCKS = " + std::to_string(LG_PPO_SYM_MAX_BLOCKS) + "]");
    return nullptr;
  }
  if (max_rows > ((int64_t)0x7fffffff - 1024) / K) { lg_policy_fail(LG_ERR_INVALID, "num_blocks * max_rows does not fit the kernels' 32-bit row arithmetic"); return nullptr; }
  if (!isfinite(config->mirror_loss_coeff)) { lg_policy_fail(LG_ERR_INVALID, "mirror_loss_coeff is not finite"); return nullptr; }
  if (actor->device != critic->device) { lg_policy_fail(LG_ERR_INVALID, "the actor and the critic live on different devices"); return nullptr; }
  if (actor->h.act_out || critic->h.act_out) { lg_policy_fail(LG_ERR_UNSUPPORTED, "a network with an output activation cannot be trained here"); return nullptr; }
  if (critic->h.dims[critic->h.L] != 1) { lg_policy_fail(LG_ERR_UNSUPPORTED, "the critic must end in 1 output"); return nullptr; }
  if (actor->h.dims[actor->h.L] > 32) { lg_policy_fail(LG_ERR_UNSUPPORTED, "the actor ends in more than 32 actions"); return nullptr; }
  const lg_mlp* nets[2] = {actor, critic};
  for (int k = 0; k < 2; ++k)                                  // sym_fwd_kernel stages a whole mirrored row into one activation image
    if (mlp_is_wide(nets[k])) {
      lg_policy_fail(LG_ERR_UNSUPPORTED, std::string(k == 0 ? "the actor's" : "the critic's") + " first layer takes " + std::to_string(nets[k]->h.dims[0]) +
                                             " inputs: the symmetric update stages rows of at most " + std::to_string(MLP_MAXW) + " columns");
      return nullptr;
    }
  const float* const* ws[2] = {aw, cw};
  const float* const* bs[2] = {ab, cb};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < nets[k]->h.L; ++l)
      if (!ws[k][l] || !bs[k][l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  if (!lg_policy_device_ok(actor->device)) return nullptr;
  DeviceScope ds_(actor->device);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_ppo_sym* p = new lg_ppo_sym();
  p->actor = actor; p->critic = critic; p->device = actor->device; p->A = actor->h.dims[actor->h.L];
  p->K = K; p->aug = config->use_data_augmentation != 0; p->mirror = config->use_mirror_loss != 0; p->coeff = config->mirror_loss_coeff;
  p->rows_max = max_rows;
  p->nstd = p->A; p->std_type = noise_std_type; p->std_dev = std_device;
  bool ok = sym_upload_table(p, "observation", K, tables->observation_width, actor->h.dims[0], tables->observation_perm, tables->observation_sign, &p->tobs) &&
            sym_upload_table(p, "critic observation", K, tables->critic_observation_width, critic->h.dims[0], tables->critic_observation_perm,
                             tables->critic_observation_sign, &p->tcobs) &&
            sym_upload_table(p, "action", K, tables->action_width, p->A, tables->action_perm, tables->action_sign, &p->tact);
  int64_t off = 0;
  p->max_rows = K * max_rows;                                // the actor sees every block
  ok = ok && train_core_add_net(p, actor, &off);
  if (!p->aug) p->max_rows = max_rows;                       // without augmentation the critic sees the original rows only
  ok = ok && train_core_add_net(p, critic, &off);
  p->max_rows = K * max_rows;
  const int loss_blocks = (int)((K * max_rows + SYM_LOSS_ROWS - 1) / SYM_LOSS_ROWS);
  p->loss_part = ok ? (float*)train_alloc(p, (size_t)loss_blocks * SYM_LOSS_SLOTS * sizeof(float), true) : nullptr;
  p->ss = p->loss_part ? (SymScalars*)train_alloc(p, sizeof(SymScalars), true) : nullptr;
  if (!ok || !p->loss_part || !p->ss || train_core_finish(p, off, ws, bs, std_host, learning_rate) != LG_OK) { lg_ppo_sym_destroy(p); return nullptr; }
  return p;
}

int lg_ppo_sym_minibatch(lg_ppo_sym* p, const lg_ppo_rows* rows, const int64_t* indices, int64_t count, const lg_ppo_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  const int rc = sym_check_call(p, rows, indices, hyper);
  if (rc != LG_OK) return rc;
  if (count <= 0) return lg_policy_fail(LG_ERR_INVALID, "count <= 0");
  if (count > p->rows_max) return lg_policy_fail(LG_ERR_INVALID, "count > max_rows of the trainer");
  DeviceScope ds_(p->device);
  return sym_step(p, rows, indices, count, hyper, (hipStream_t)stream, 0);
}

int lg_ppo_sym_update(lg_ppo_sym* p, const lg_ppo_rows* rows, int64_t R, const int64_t* indices, int32_t num_mini_batches, int32_t num_learning_epochs,
                      const lg_ppo_hyper* hyper, lg_ppo_sym_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = sym_check_call(p, rows, indices, hyper);
  if (rc != LG_OK) return rc;
  if (num_mini_batches < 1 || num_learning_epochs < 1) return lg_policy_fail(LG_ERR_INVALID, "num_mini_batches < 1 or num_learning_epochs < 1");
  const int64_t mini = R / num_mini_batches;
  if (mini <= 0) return lg_policy_fail(LG_ERR_INVALID, "R / num_mini_batches == 0");
  if (mini > p->rows_max) return lg_policy_fail(LG_ERR_INVALID, "R / num_mini_batches > max_rows of the trainer");
  DeviceScope ds_(p->device);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sym_stats_kernel, dim3(1), dim3(1), 0, st, p->sc, p->ss, stats, 0, 1);
  for (int e = 0; e < num_learning_epochs; ++e)
    for (int i = 0; i < num_mini_batches; ++i) {
      const int r2 = sym_step(p, rows, indices + (int64_t)i * mini, mini, hyper, st, 1);
      if (r2 != LG_OK) return r2;
    }
  if (stats) hipLaunchKernelGGL(sym_stats_kernel, dim3(1), dim3(1), 0, st, p->sc, p->ss, stats, 1, num_mini_batches * num_learning_epochs);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int64_t lg_ppo_sym_parameter_count(lg_ppo_sym* p) {
  POLICY_ENTRY;
  return train_api_parameter_count(p);
}

int lg_ppo_sym_gradients(lg_ppo_sym* p, float* g, float* norm, float* means, float* symmetry, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (g) POLICY_TRY(hipMemcpy(g, p->G, (size_t)p->P * sizeof(float), hipMemcpyDeviceToHost));
  TrainScalars sc;
  SymScalars ss;
  POLICY_TRY(hipMemcpy(&sc, p->sc, sizeof(sc), hipMemcpyDeviceToHost));
  POLICY_TRY(hipMemcpy(&ss, p->ss, sizeof(ss), hipMemcpyDeviceToHost));
  if (norm) *norm = sc.norm;
  if (means) for (int k = 0; k < 4; ++k) means[k] = sc.means[k];
  if (symmetry) *symmetry = ss.mean;
  return LG_OK;
}

int lg_ppo_sym_forward_outputs(lg_ppo_sym* p, float* mean, float* values, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (p->last_rows <= 0) return lg_policy_fail(LG_ERR_INVALID, "no mini-batch has run yet");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const TrainNet &NA = p->net[0], &NC = p->net[1];
  if (mean) POLICY_TRY(hipMemcpy(mean, NA.a[NA.L], (size_t)p->last_actor_rows * p->A * sizeof(float), hipMemcpyDeviceToHost));
  if (values) POLICY_TRY(hipMemcpy(values, NC.a[NC.L], (size_t)p->last_critic_rows * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int lg_ppo_sym_get_state(lg_ppo_sym* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  POLICY_ENTRY;
  return train_api_get_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_ppo_sym_get_parameters(lg_ppo_sym* p, float* params, void* stream) {
  POLICY_ENTRY;
  return train_api_get_parameters(p, params, stream);
}

int lg_ppo_sym_set_state(lg_ppo_sym* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_ppo_sym_set_learning_rate(lg_ppo_sym* p, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_learning_rate(p, lr, stream);
}

}  // extern "C"
