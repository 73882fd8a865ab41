// lg_train_recurrent.hip — gfx950 kernels of PPO.update for the recurrent actor-critic (include/lgtrain_recurrent.h): backpropagation through
// time through the LSTM / GRU memory in front of each MLP.  Everything around the memory is lg_train.hip's (lg_train_internal.h): the MLPs' forward
// with saved activations, the clipped losses, the MLPs' backward, the slab weight-gradient pass and its fixed-order reduction, the norm, Adam.
//
//   rnn_train_forward_kernel   one step of one memory layer for 32 rows (blockIdx.y: actor's / critic's memory): rnn_tile of lg_rnn_tile.h with
//                              SAVE -- the inference tile, the same k-chain, plus the gates, the entering and the new state written out.  The
//                              entering state is the saved hidden row where a trajectory starts, else the row's own state after step t - 1.
//   rows_matmul_kernel         dL/d(input) of the MLPs' first layers: d[0] W_0 on the transposed tiling Adam keeps for it.
//   rnn_backward_kernel        one step of one layer backwards.  The gate derivative is the staging pass: D_t (rows, G H) is formed from the saved
//                              gates, dL/dh' (from above plus the carry) and the dc carry while the activation image is filled (and written out
//                              for the weight gradients); then dx = D_ih W_ih and dh_prev = D_hh W_hh on the matrix cores, 1024 columns of D per
//                              pass.  dh_prev / dc_prev are zero for rows that entered the step from a saved row.
//   rnn_retile_kernel          the masters -> the lg_rnn forward images (rnn_tile_weights' layout) and the combined bias rows.
//   rec_index_kernel           mini-batch row t * count + j -> rollout row t * N + env0 + j.
// The memory's weight gradients are TWO segments per layer of the existing slab pass over all T * count rows; the transposed tilings are written by
// the Adam kernel (its transposed formula is the one D W needs).  No atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_rnn_tile.h"
#include "lg_train_internal.h"
#include "lg_train_recurrent_internal.h"
#include "../../include/lgtrain_recurrent.h"

#define BK_PASS 1024          // columns of D per pass of the backward tile: the 128 KB image of the forward tile

// both memories' operands in ONE kernel argument, indexed by blockIdx.y: the operands of the memory that is not this workgroup's are never loaded
struct RnnTrainPair { RnnStepArgs S[2]; RnnSaveArgs V[2]; };

__global__ __launch_bounds__(MLP_THREADS) void rnn_train_forward_kernel(RnnTrainPair P, int64_t n) {
  __shared__ __attribute__((aligned(16))) float img[MLP_ROWS * RNN_KMAX];
  const RnnStepArgs& S = P.S[blockIdx.y];
  const RnnSaveArgs& V = P.V[blockIdx.y];
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  if (S.L.gru) rnn_tile<true, true>(S, V, row0, n, img); else rnn_tile<false, true>(S, V, row0, n, img);
}

// layer 0 of a wide memory (lg_rnn_create_wide): the tile with SAVE and SEED on the projection rows y of this step (rnn_wide_xproj_kernel ran over all
// T * count rows of the mini-batch before the first step: the projection does not depend on the state).  The image holds h alone: 64 KB.
__global__ __launch_bounds__(MLP_THREADS) void rnn_wide_train_forward_kernel(RnnTrainPair P, const float* __restrict__ y0, const float* __restrict__ y1, int64_t n) {
  __shared__ __attribute__((aligned(16))) float img[MLP_ROWS * RNN_XMAX];
  const RnnStepArgs& S = P.S[blockIdx.y];
  const RnnSaveArgs& V = P.V[blockIdx.y];
  const float* __restrict__ y = blockIdx.y == 0 ? y0 : y1;
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  if (S.L.gru) rnn_tile<true, true, true>(S, V, row0, n, img, y); else rnn_tile<false, true, true>(S, V, row0, n, img, y);
}

// one 16-column chunk over nblk blocks of 16 inputs: both row halves, k ascending (chunk_chain of lg_train.hip)
LG_DEV void rec_chain(const float4* __restrict__ wc, const float4* ap, int nblk, f32x4& acc0, f32x4& acc1) {
  for (int kb = 0; kb < nblk; ++kb) {
    const float4 w = wc[(size_t)kb * 64], p = ap[kb * 128], q = ap[kb * 128 + 64];
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.x, w.x, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.x, w.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.y, w.y, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.y, w.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.z, w.z, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.z, w.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.w, w.w, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.w, w.w, acc1, 0, 0, 0);
  }
}

// 32 rows of a (rows, K) matrix times a transposed tiling [chunk][nbk blocks of 16 k][lane][4] (the bw of a TrainSeg), BK_PASS columns per pass:
// stage(row, k) gives the matrix element, emit(row, col, partial sum of this pass, first pass, last pass) takes the product.
template <class Stage, class Emit>
LG_DEV void rows_times_tiled(int K, int nbk, const float* __restrict__ wt, int nch, int64_t row0, int64_t n, float* img, Stage stage, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float4* ap = reinterpret_cast<const float4*>(img) + (lane & 15) * 4 + (lane >> 4);
  for (int k0 = 0; k0 < K; k0 += BK_PASS) {
    const int kw = K - k0 < BK_PASS ? K - k0 : BK_PASS, nblk = (kw + 15) >> 4, Kp = nblk * 16;
    for (int e = tid; e < MLP_ROWS * Kp; e += MLP_THREADS) {
      const int r = e / Kp, k = e - r * Kp;
      const int64_t row = row0 + r;
      img[IMG(r, k)] = (row < n && k < kw) ? stage(row, k0 + k) : 0.f;
    }
    lds_barrier();
    const bool first = k0 == 0, last = k0 + BK_PASS >= K;
    for (int c = wv; c < nch; c += MLP_THREADS / 64) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      rec_chain(reinterpret_cast<const float4*>(wt) + ((size_t)c * nbk + (k0 >> 4)) * 64 + lane, ap, nblk, acc0, acc1);
      const int col = c * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * (lane >> 4) + i;
        if (row0 + m < n) emit(row0 + m, col, acc0[i], first, last);
        if (row0 + m + 16 < n) emit(row0 + m + 16, col, acc1[i], first, last);
      }
    }
    lds_barrier();
  }
}

__global__ __launch_bounds__(MLP_THREADS) void rows_matmul_kernel(RowsMatArgs M0, RowsMatArgs M1, int64_t n) {
  __shared__ __attribute__((aligned(16))) float img[MLP_ROWS * BK_PASS];
  const RowsMatArgs& M = blockIdx.y == 0 ? M0 : M1;
  const float* __restrict__ A = M.A;
  float* __restrict__ out = M.out;
  const int K = M.K, nout = M.nout;
  rows_times_tiled(K, M.nbk, M.wt, M.nch, (int64_t)blockIdx.x * MLP_ROWS, n, img,
                   [&](int64_t row, int k) { return A[row * K + k]; },
                   [&](int64_t row, int col, float v, bool first, bool) {
                     if (col >= nout) return;
                     if (!first) v += out[row * nout + col];
                     out[row * nout + col] = v;
                   });
}

// the derivative of the loss w.r.t. gate g's pre-activation of (row, unit u): vx as weight_ih / bias_ih see it, vh as weight_hh / bias_hh do
// (they differ in a GRU's n gate, where r multiplies the hidden side only); dcp: dL/dc_prev (LSTM)
template <bool GRU>
LG_DEV void gate_grad(const RnnBackArgs& B, int64_t row, int g, int u, float& vx, float& vh, float& dcp) {
  const int64_t e = row * B.H + u;
  const float dh = B.dup[e] + (B.dh_in ? B.dh_in[e] : 0.f);
  if (GRU) {
    const float r = B.gate[0][e], z = B.gate[1][e], ng = B.gate[2][e], hnp = B.gate[3][e];
    const float dnp = dh * (1.f - z) * (1.f - ng * ng);
    dcp = 0.f;
    if (g == 0) vx = vh = dnp * hnp * r * (1.f - r);
    else if (g == 1) vx = vh = dh * (B.hin[e] - ng) * z * (1.f - z);
    else { vx = dnp; vh = dnp * r; }
  } else {
    const float ig = B.gate[0][e], fg = B.gate[1][e], gg = B.gate[2][e], og = B.gate[3][e];
    const float tc = tanhf(B.cnew[e]);
    const float dc = dh * og * (1.f - tc * tc) + (B.dc_in ? B.dc_in[e] : 0.f);
    dcp = dc * fg;
    float v;
    if (g == 0) v = dc * gg * ig * (1.f - ig);
    else if (g == 1) v = dc * B.cin[e] * fg * (1.f - fg);
    else if (g == 2) v = dc * ig * (1.f - gg * gg);
    else v = dh * tc * og * (1.f - og);
    vx = vh = v;
  }
}

template <bool GRU>
LG_DEV void rnn_back_tile(const RnnBackArgs& B, int64_t row0, int64_t n, float* img) {
  const int H = B.H, K = B.K, I = B.I;
  const float* __restrict__ dprev = B.dprev;
  if (B.nchx > 0) {                                         // dx = D_ih W_ih
    float* __restrict__ dx = B.dx;
    rows_times_tiled(K, B.nbk, B.wtx, B.nchx, row0, n, img,
                     [&](int64_t row, int k) { const int g = k / H; float vx, vh, dcp; gate_grad<GRU>(B, row, g, k - g * H, vx, vh, dcp); return vx; },
                     [&](int64_t row, int col, float v, bool first, bool) {
                       if (col >= I) return;
                       if (!first) v += dx[row * I + col];
                       dx[row * I + col] = v;
                     });
  }
  float* __restrict__ dh_out = B.dh_out;                    // dh_prev = D_hh W_hh (+ z dh for a GRU); the staging pass writes D and dc_prev
  rows_times_tiled(K, B.nbk, B.wth, B.nchh, row0, n, img,
                   [&](int64_t row, int k) {
                     const int g = k / H, u = k - g * H;
                     float vx, vh, dcp;
                     gate_grad<GRU>(B, row, g, u, vx, vh, dcp);
                     B.Dih[row * K + k] = vx;
                     if (GRU) B.Dhh[row * K + k] = vh;
                     else if (g == 1) B.dc_out[row * H + u] = (!dprev || dprev[row] != 0.f) ? 0.f : dcp;
                     return vh;
                   },
                   [&](int64_t row, int col, float v, bool first, bool last) {
                     if (col >= H) return;
                     const int64_t e = row * H + col;
                     if (!first) v += dh_out[e];
                     if (last) {
                       if (GRU) v += (B.dup[e] + (B.dh_in ? B.dh_in[e] : 0.f)) * B.gate[1][e];
                       if (!dprev || dprev[row] != 0.f) v = 0.f;          // the row entered from a saved hidden row: nothing crosses to step t - 1
                     }
                     dh_out[e] = v;
                   });
}

struct RnnBackPair { RnnBackArgs B[2]; };

__global__ __launch_bounds__(MLP_THREADS) void rnn_backward_kernel(RnnBackPair P, int64_t n) {
  __shared__ __attribute__((aligned(16))) float img[MLP_ROWS * BK_PASS];
  const RnnBackArgs& B = P.B[blockIdx.y];
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  if (B.gru) rnn_back_tile<true>(B, row0, n, img); else rnn_back_tile<false>(B, row0, n, img);
}

// element e of the tiled weights (rnn_tile_weights_at of lg_policy.hip, the same index arithmetic), then of the bias rows.  A wide layer 0 has two
// entries: the projection image (Ip = RNN_NO_HH: no hidden part; b NULL: no bias rows) and the seeded tile's (I = Ip = 0: h alone, and the bias rows)
__global__ __launch_bounds__(256) void rnn_retile_kernel(const RnnRetile* __restrict__ tab, const float* __restrict__ theta) {
  const RnnRetile R = tab[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int Hp = 16 * R.nch, H = R.H;
  const int64_t wcount = (int64_t)R.nch * (R.nb + 1) * R.G * 256;
  if (e < wcount) {
    const int s = (int)(e & 3), ln = (int)((e >> 2) & 63);
    int64_t rest = e >> 8;
    const int g = (int)(rest % R.G); rest /= R.G;
    const int b = (int)(rest % (R.nb + 1)), c = (int)(rest / (R.nb + 1));
    const int u = c * 16 + (ln & 15), k = b * 16 + s * 4 + (ln >> 4);
    float v = 0.f;
    if (u < H) {
      if (k < R.I) v = theta[R.wih + (int64_t)(g * H + u) * R.I + k];
      else if (k >= R.Ip && k < R.Ip + H) v = theta[R.whh + (int64_t)(g * H + u) * H + (k - R.Ip)];
    }
    R.w[e] = v;
  } else if (e < wcount + 4 * Hp && R.b) {
    const int j = (int)(e - wcount), g = j / Hp, u = j - g * Hp;
    float v = 0.f;
    if (u < H) {
      if (R.G == 4) v = theta[R.bih + g * H + u] + theta[R.bhh + g * H + u];
      else if (g < 2) v = theta[R.bih + g * H + u] + theta[R.bhh + g * H + u];
      else if (g == 2) v = theta[R.bih + 2 * H + u];
      else v = theta[R.bhh + 2 * H + u];
    }
    R.b[j] = v;
  }
}

__global__ __launch_bounds__(256) void rec_index_kernel(int64_t* __restrict__ idx, int64_t rows, int64_t count, int64_t N, int64_t env0) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const int64_t t = i / count;
  idx[i] = t * N + env0 + (i - t * count);
}

// ------------------------------------------------------------------------------------------------------------------------ host side
struct RecMem {
  lg_rnn* m = nullptr;
  int G = 0, L = 0, I = 0, H = 0;
  MemLayer layer[RNN_MAX_LAYERS];
  float* y = nullptr;                // a wide memory: layer 0's projection of the mini-batch, (max_rows, G * H padded to 16)
};

struct lg_ppo_recurrent : TrainCore {
  RecMem mem[2];
  int A = 0, nretile = 0;
  int64_t retile_big = 0;
  float* loss_part = nullptr;
  int64_t* idx = nullptr;
  RnnRetile* d_retile = nullptr;
};

static int rec_retile(TrainCore* c, hipStream_t st) {
  lg_ppo_recurrent* p = static_cast<lg_ppo_recurrent*>(c);
  hipLaunchKernelGGL(rnn_retile_kernel, dim3((unsigned)((p->retile_big + 255) / 256), p->nretile), dim3(256), 0, st, (const RnnRetile*)p->d_retile, (const float*)p->theta);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

static int rec_check_call(lg_ppo_recurrent* p, const lg_ppo_rows* r, const lg_rollout_hidden* hid, const float* dones, int32_t T, int64_t N, const lg_ppo_hyper* h) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!r || !hid || !dones || !h) return lg_policy_fail(LG_ERR_INVALID, "null rows, hidden rows, dones or hyper-parameters");
  if (!r->observations || !r->critic_observations || !r->actions || !r->values || !r->returns || !r->advantages || !r->actions_log_prob || !r->mu || !r->sigma)
    return lg_policy_fail(LG_ERR_INVALID, "null row pointer");
  if (!hid->h_a || !hid->h_c || (p->mem[0].G == 4 && (!hid->c_a || !hid->c_c))) return lg_policy_fail(LG_ERR_INVALID, "null hidden-state row");
  if (T < 1 || N < 1) return lg_policy_fail(LG_ERR_INVALID, "T < 1 or N < 1");
  if (h->schedule != LG_SCHEDULE_FIXED && h->schedule != LG_SCHEDULE_ADAPTIVE) return lg_policy_fail(LG_ERR_INVALID, "unknown schedule (fixed | adaptive)");
  return LG_OK;
}

static int rec_step(lg_ppo_recurrent* p, const lg_ppo_rows* r, const lg_rollout_hidden* hid, const float* dones, int T, int64_t N, int64_t env0, int64_t mb,
                    const lg_ppo_hyper* h, hipStream_t st, int accumulate) {
  const int64_t n = (int64_t)T * mb;
  p->last_rows = n;
  const unsigned tiles = (unsigned)((mb + MLP_ROWS - 1) / MLP_ROWS);
  const int L = p->mem[0].L;
  const float* xs[2] = {r->observations, r->critic_observations};
  const float* hs[2] = {hid->h_a, hid->h_c};
  const float* cs[2] = {hid->c_a, hid->c_c};
  hipLaunchKernelGGL(rec_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->idx, n, mb, N, env0);
  // ---- a wide memory's input projection: all T * mb rows at once
  const bool wide[2] = {p->mem[0].m->wide, p->mem[1].m->wide};
  RnnXprojArgs X[2];
  for (int k = 0; k < 2; ++k) X[k] = RnnXprojArgs{p->mem[k].m->xproj, xs[k], p->idx, p->mem[k].y};
  if (wide[0] && wide[1]) rnn_launch_xproj(&X[0], &X[1], n, st);
  else for (int k = 0; k < 2; ++k) if (wide[k]) rnn_launch_xproj(&X[k], nullptr, n, st);
  // ---- forward through time
  for (int t = 0; t < T; ++t)
    for (int l = 0; l < L; ++l) {
      RnnTrainPair P;
      RnnStepArgs* S = P.S; RnnSaveArgs* V = P.V;
      for (int k = 0; k < 2; ++k) {
        const RecMem& M = p->mem[k];
        const MemLayer& Y = M.layer[l];
        const size_t at = (size_t)t * mb * M.H, before = t > 0 ? (size_t)(t - 1) * mb * M.H : 0;
        const size_t saved = (((size_t)t * L + l) * N + env0) * M.H;
        S[k].L = M.m->layer[l];
        S[k].x = l == 0 ? xs[k] + ((size_t)t * N + env0) * M.I : M.layer[l - 1].hnew + at;
        S[k].h = nullptr; S[k].c = nullptr; S[k].reset = nullptr; S[k].out = nullptr;
        V[k].hs = hs[k] + saved; V[k].cs = M.G == 4 ? cs[k] + saved : nullptr;
        V[k].hprev = t > 0 ? Y.hnew + before : nullptr; V[k].cprev = (t > 0 && M.G == 4) ? Y.cnew + before : nullptr;
        V[k].dprev = t > 0 ? dones + (size_t)(t - 1) * N + env0 : nullptr;
        for (int g = 0; g < 4; ++g) V[k].gate[g] = Y.gate[g] + at;
        V[k].hin = Y.hin + at; V[k].hnew = Y.hnew + at;
        V[k].cin = M.G == 4 ? Y.cin + at : nullptr; V[k].cnew = M.G == 4 ? Y.cnew + at : nullptr;
      }
      if (l > 0 || !(wide[0] || wide[1])) {
        hipLaunchKernelGGL(rnn_train_forward_kernel, dim3(tiles, 2), dim3(MLP_THREADS), 0, st, P, mb);
        continue;
      }
      const float* yt[2];
      for (int k = 0; k < 2; ++k) yt[k] = wide[k] ? p->mem[k].y + (size_t)t * mb * p->mem[k].G * 16 * p->mem[k].m->xproj.nch : nullptr;
      if (wide[0] && wide[1]) {
        hipLaunchKernelGGL(rnn_wide_train_forward_kernel, dim3(tiles, 2), dim3(MLP_THREADS), 0, st, P, yt[0], yt[1], mb);
      } else {                                               // a mixed pair: one memory after the other
        for (int k = 0; k < 2; ++k) {
          RnnTrainPair One{};
          One.S[0] = P.S[k]; One.V[0] = P.V[k];
          if (wide[k]) hipLaunchKernelGGL(rnn_wide_train_forward_kernel, dim3(tiles, 1), dim3(MLP_THREADS), 0, st, One, yt[k], yt[k], mb);
          else hipLaunchKernelGGL(rnn_train_forward_kernel, dim3(tiles, 1), dim3(MLP_THREADS), 0, st, One, mb);
        }
      }
    }
  // ---- the MLPs on the memories' outputs, time-major; the losses; the MLPs' backward and dL/d(their input)
  train_launch_forward(p, p->mem[0].layer[L - 1].hnew, p->mem[1].layer[L - 1].hnew, nullptr, n, st);
  train_launch_ppo_loss(p, r, p->idx, n, h, p->loss_part, accumulate, st);
  train_launch_backward(p, n, st);
  {
    RowsMatArgs M[2];
    for (int k = 0; k < 2; ++k) {
      const TrainNet& Nn = p->net[k];
      M[k].A = Nn.d[0]; M[k].K = Nn.dims[1]; M[k].nbk = Nn.bkpad[0] / 16; M[k].wt = Nn.bw[0];
      M[k].nout = p->mem[k].H; M[k].nch = (p->mem[k].H + 15) / 16; M[k].out = p->mem[k].layer[L - 1].dup;
    }
    hipLaunchKernelGGL(rows_matmul_kernel, dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS), 2), dim3(MLP_THREADS), 0, st, M[0], M[1], n);
  }
  // ---- backward through time
  for (int t = T - 1; t >= 0; --t)
    for (int l = L - 1; l >= 0; --l) {
      RnnBackPair P;
      RnnBackArgs* B = P.B;
      for (int k = 0; k < 2; ++k) {
        const RecMem& M = p->mem[k];
        const MemLayer& Y = M.layer[l];
        const size_t at = (size_t)t * mb * M.H;
        const int Il = l == 0 ? M.I : M.H;
        RnnBackArgs& b = B[k];
        b.gru = M.G == 3; b.I = Il; b.H = M.H; b.K = M.G * M.H; b.nbk = (b.K + 15) / 16;
        b.nchx = l > 0 ? (Il + 15) / 16 : 0; b.nchh = (M.H + 15) / 16;
        b.wtx = Y.wtx; b.wth = Y.wth;
        for (int g = 0; g < 4; ++g) b.gate[g] = Y.gate[g] + at;
        b.hin = Y.hin + at; b.cin = M.G == 4 ? Y.cin + at : nullptr; b.cnew = M.G == 4 ? Y.cnew + at : nullptr;
        b.dup = Y.dup + at;
        b.dh_in = t + 1 < T ? Y.dh[(t + 1) & 1] : nullptr; b.dc_in = (t + 1 < T && M.G == 4) ? Y.dc[(t + 1) & 1] : nullptr;
        b.dprev = t > 0 ? dones + (size_t)(t - 1) * N + env0 : nullptr;
        b.dh_out = Y.dh[t & 1]; b.dc_out = M.G == 4 ? Y.dc[t & 1] : nullptr;
        b.dx = l > 0 ? M.layer[l - 1].dup + at : nullptr;
        b.Dih = Y.Dih + (size_t)t * mb * b.K; b.Dhh = Y.Dhh + (size_t)t * mb * b.K;
      }
      hipLaunchKernelGGL(rnn_backward_kernel, dim3(tiles, 2), dim3(MLP_THREADS), 0, st, P, mb);
    }
  // ---- every weight gradient in one slab pass, the norm, Adam, the images
  const int rc = train_launch_optimise(p, r->observations, r->critic_observations, p->idx, n, h->max_grad_norm, 1, st);
  if (rc != LG_OK) return rc;
  return rec_retile(p, st);
}

extern "C" {

void lg_ppo_recurrent_destroy(lg_ppo_recurrent* p) {
  if (!p) return;
  DeviceScope ds_(p->device);
  (void)hipDeviceSynchronize();
  train_core_free(p);
  delete p;
}

lg_ppo_recurrent* lg_ppo_recurrent_create(lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const lg_ppo_recurrent_params* q, int32_t noise_std_type,
                                          double learning_rate, int64_t max_rows, float* std_device) {
  POLICY_ENTRY;
  if (!mem_a || !mem_c || !actor || !critic) { lg_policy_fail(LG_ERR_INVALID, "null memory or network"); return nullptr; }
  if (!q || !std_device) { lg_policy_fail(LG_ERR_INVALID, "null parameters or std vector"); return nullptr; }
  if (!q->mem_a_w_ih || !q->mem_a_w_hh || !q->mem_a_b_ih || !q->mem_a_b_hh || !q->mem_c_w_ih || !q->mem_c_w_hh || !q->mem_c_b_ih || !q->mem_c_b_hh ||
      !q->actor_weights || !q->actor_biases || !q->critic_weights || !q->critic_biases || !q->std) { lg_policy_fail(LG_ERR_INVALID, "null parameter list or std vector"); return nullptr; }
  if (noise_std_type != LG_STD_SCALAR && noise_std_type != LG_STD_LOG) { lg_policy_fail(LG_ERR_INVALID, "unknown noise_std_type (scalar | log)"); return nullptr; }
  if (max_rows < 1) { lg_policy_fail(LG_ERR_INVALID, "max_rows < 1"); return nullptr; }
  if (!(learning_rate > 0.0)) { lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0"); return nullptr; }
  if (mem_a->type != mem_c->type || mem_a->num_layers != mem_c->num_layers) { lg_policy_fail(LG_ERR_UNSUPPORTED, "the two memories differ in type or depth"); return nullptr; }
  if (q->rnn_type != mem_a->type) { lg_policy_fail(LG_ERR_INVALID, "the parameters' rnn_type is not the memory handles' (lstm against gru)"); return nullptr; }
  if (q->num_layers != mem_a->num_layers || q->input_a != mem_a->input || q->hidden_a != mem_a->hidden || q->input_c != mem_c->input || q->hidden_c != mem_c->hidden) {
    lg_policy_fail(LG_ERR_INVALID, "the parameters' depth or widths disagree with the memory handles"); return nullptr; }
  for (const lg_mlp* head : {actor, critic})
    if (mlp_is_wide(head)) {
      lg_policy_fail(LG_ERR_UNSUPPORTED, "a head's first layer takes " + std::to_string(head->h.dims[0]) + " inputs: a head reads its memory's hidden row of at most " +
                                             std::to_string(MLP_MAXW) + " columns");
      return nullptr;
    }
  if (actor->h.dims[0] != mem_a->hidden || critic->h.dims[0] != mem_c->hidden) { lg_policy_fail(LG_ERR_INVALID, "an MLP's input width is not its memory's hidden width"); return nullptr; }
  if (actor->device != critic->device || mem_a->device != actor->device || mem_c->device != actor->device) {
    lg_policy_fail(LG_ERR_INVALID, "the memories and the networks live on different devices"); return nullptr; }
  if (actor->h.act_out || critic->h.act_out) { lg_policy_fail(LG_ERR_UNSUPPORTED, "a network with an output activation cannot be trained here"); return nullptr; }
  if (critic->h.dims[critic->h.L] != 1) { lg_policy_fail(LG_ERR_UNSUPPORTED, "the critic must end in 1 output"); return nullptr; }
  if (actor->h.dims[actor->h.L] > 32) { lg_policy_fail(LG_ERR_UNSUPPORTED, "the actor ends in more than 32 actions"); return nullptr; }
  const lg_mlp* nets[2] = {actor, critic};
  lg_rnn* mems[2] = {mem_a, mem_c};
  const float* const* mlp_w[2] = {q->actor_weights, q->critic_weights};
  const float* const* mlp_b[2] = {q->actor_biases, q->critic_biases};
  const float* const* rw[2][2] = {{q->mem_a_w_ih, q->mem_a_w_hh}, {q->mem_c_w_ih, q->mem_c_w_hh}};
  const float* const* rb[2][2] = {{q->mem_a_b_ih, q->mem_a_b_hh}, {q->mem_c_b_ih, q->mem_c_b_hh}};
  // host tables in the shape train_core_finish reads: [network][layer], a memory's tensors behind the MLP's at LG_MLP_MAX_LAYERS + 2 l (+ 1: the hidden side)
  const float* wtab[2][LG_MLP_MAX_LAYERS + 2 * RNN_MAX_LAYERS] = {};
  const float* btab[2][LG_MLP_MAX_LAYERS + 2 * RNN_MAX_LAYERS] = {};
  for (int k = 0; k < 2; ++k) {
    for (int l = 0; l < nets[k]->h.L; ++l) {
      if (!mlp_w[k][l] || !mlp_b[k][l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
      wtab[k][l] = mlp_w[k][l]; btab[k][l] = mlp_b[k][l];
    }
    for (int l = 0; l < mems[k]->num_layers; ++l)
      for (int s = 0; s < 2; ++s) {
        if (!rw[k][s][l] || !rb[k][s][l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
        wtab[k][LG_MLP_MAX_LAYERS + 2 * l + s] = rw[k][s][l]; btab[k][LG_MLP_MAX_LAYERS + 2 * l + s] = rb[k][s][l];
      }
  }
  if (!lg_policy_device_ok(actor->device)) return nullptr;
  DeviceScope ds_(actor->device);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_ppo_recurrent* p = new lg_ppo_recurrent();
  p->device = actor->device; p->A = actor->h.dims[actor->h.L]; p->max_rows = max_rows; p->retile_own = rec_retile;
  p->nstd = p->A; p->std_type = noise_std_type; p->std_dev = std_device;
  bool ok = true;
  auto alloc = [&](size_t floats, bool zero) -> float* { float* d = ok ? (float*)train_alloc(p, floats * sizeof(float), zero) : nullptr; if (!d) ok = false; return d; };
  const size_t R = (size_t)max_rows;
  int64_t off = 0;
  int first_seg[2];
  for (int k = 0; k < 2 && ok; ++k) { first_seg[k] = p->nseg; ok = train_core_add_net(p, nets[k], &off); }
  std::vector<RnnRetile> retile;
  for (int k = 0; k < 2 && ok; ++k) {
    RecMem& M = p->mem[k];
    M.m = mems[k]; M.G = mems[k]->type == LG_RNN_GRU ? 3 : 4; M.L = mems[k]->num_layers; M.I = mems[k]->input; M.H = mems[k]->hidden;
    const int H = M.H, K = M.G * H, nbk = (K + 15) / 16;
    // the MLP's first layer now reads the top layer's h' (dense, time-major) and propagates into it: a transposed tiling for layer 0 too
    TrainNet& Nn = p->net[k];
    TrainSeg& S0 = p->seg[first_seg[k]];
    for (int l = 0; l < M.L; ++l) {
      MemLayer& Y = M.layer[l];
      const int I = l == 0 ? M.I : H;
      for (int g = 0; g < 4; ++g) Y.gate[g] = alloc(R * H, false);
      Y.hin = alloc(R * H, false); Y.hnew = alloc(R * H, false); Y.dup = alloc(R * H, false);
      Y.cin = M.G == 4 ? alloc(R * H, false) : nullptr; Y.cnew = M.G == 4 ? alloc(R * H, false) : nullptr;
      Y.Dih = alloc(R * K, false); Y.Dhh = M.G == 3 ? alloc(R * K, false) : Y.Dih;
      for (int s = 0; s < 2; ++s) { Y.dh[s] = alloc(R * H, true); Y.dc[s] = M.G == 4 ? alloc(R * H, true) : nullptr; }
      Y.wtx = l > 0 ? alloc((size_t)((I + 15) / 16) * nbk * 256, true) : nullptr;
      Y.wth = alloc((size_t)((H + 15) / 16) * nbk * 256, true);
      // weight_ih + bias_ih with (D_ih, x); weight_hh + bias_hh with (D_hh, h_in)
      train_core_add_seg(p, k, LG_MLP_MAX_LAYERS + 2 * l, K, I, Y.Dih, l == 0 ? nullptr : M.layer[l - 1].hnew, nullptr, nullptr, 0, Y.wtx, nbk, &ok);
      train_core_add_seg(p, k, LG_MLP_MAX_LAYERS + 2 * l + 1, K, H, Y.Dhh, Y.hin, nullptr, nullptr, 0, Y.wth, nbk, &ok);
    }
    if (mems[k]->wide) M.y = alloc(R * M.G * 16 * ((H + 15) / 16), false);
    float* bw0 = alloc((size_t)Nn.bnch[0] * (Nn.bkpad[0] / 16) * 256, true);
    Nn.bw[0] = bw0; S0.bw = bw0; S0.Ain = M.layer[M.L - 1].hnew;
  }
  // the flat order: actor, critic, then per memory and layer weight_ih, weight_hh, bias_ih, bias_hh, then std / log_std
  for (int k = 0, s = first_seg[1] + nets[1]->h.L; k < 2 && ok; ++k)
    for (int l = 0; l < p->mem[k].L; ++l, s += 2) {
      TrainSeg &Si = p->seg[s], &Sh = p->seg[s + 1];
      Si.woff = off; off += (int64_t)Si.dO * Si.dI;
      Sh.woff = off; off += (int64_t)Sh.dO * Sh.dI;
      Si.boff = off; off += Si.dO;
      Sh.boff = off; off += Sh.dO;
      const RnnLayerDev& D = p->mem[k].m->layer[l];
      RnnRetile rt;
      rt.w = const_cast<float*>(D.w); rt.b = const_cast<float*>(D.b); rt.G = p->mem[k].G; rt.I = D.I; rt.H = D.H; rt.Ip = D.Ip; rt.nb = D.nb; rt.nch = D.nch;
      rt.wih = Si.woff; rt.whh = Sh.woff; rt.bih = Si.boff; rt.bhh = Sh.boff;
      retile.push_back(rt);
      const int64_t cnt = (int64_t)D.nch * (D.nb + 1) * rt.G * 256 + 4 * 16 * D.nch;
      if (cnt > p->retile_big) p->retile_big = cnt;
      if (l == 0 && p->mem[k].m->wide) {
        const RnnLayerDev& Xd = p->mem[k].m->xproj;
        RnnRetile rx = rt;
        rx.w = const_cast<float*>(Xd.w); rx.b = nullptr; rx.I = Xd.I; rx.Ip = RNN_NO_HH; rx.nb = Xd.nbx;
        retile.push_back(rx);
        const int64_t cx = (int64_t)Xd.nch * (Xd.nbx + 1) * rx.G * 256;
        if (cx > p->retile_big) p->retile_big = cx;
      }
    }
  p->nretile = (int)retile.size();
  p->loss_part = alloc(train_ppo_loss_floats(max_rows), true);
  p->idx = ok ? (int64_t*)train_alloc(p, R * sizeof(int64_t), true) : nullptr;
  p->d_retile = ok && p->idx ? (RnnRetile*)train_alloc(p, sizeof(RnnRetile) * (retile.size() + 1), true) : nullptr;
  const float* const* ws[2] = {wtab[0], wtab[1]};
  const float* const* bs[2] = {btab[0], btab[1]};
  if (!ok || !p->idx || !p->d_retile || train_core_finish(p, off, ws, bs, q->std, learning_rate) != LG_OK ||
      hipMemcpy(p->d_retile, retile.data(), sizeof(RnnRetile) * retile.size(), hipMemcpyHostToDevice) != hipSuccess || rec_retile(p, nullptr) != LG_OK ||
      hipDeviceSynchronize() != hipSuccess) {
    lg_ppo_recurrent_destroy(p);
    return nullptr;
  }
  return p;
}

int lg_ppo_recurrent_minibatch(lg_ppo_recurrent* p, const lg_ppo_rows* rows, const lg_rollout_hidden* hidden, const float* dones, int32_t T, int64_t N, int64_t env0,
                               int64_t count, const lg_ppo_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  const int rc = rec_check_call(p, rows, hidden, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  if (count < 1 || env0 < 0 || env0 + count > N) return lg_policy_fail(LG_ERR_INVALID, "the env slice [env0, env0 + count) is empty or leaves [0, N)");
  if ((int64_t)T * count > p->max_rows) return lg_policy_fail(LG_ERR_INVALID, "T * count > max_rows of the trainer");
  DeviceScope ds_(p->device);
  const int r2 = rec_step(p, rows, hidden, dones, T, N, env0, count, hyper, (hipStream_t)stream, 0);
  if (r2 != LG_OK) return r2;
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_ppo_recurrent_update(lg_ppo_recurrent* p, const lg_ppo_rows* rows, const lg_rollout_hidden* hidden, const float* dones, int32_t T, int64_t N,
                            int32_t num_mini_batches, int32_t num_learning_epochs, const lg_ppo_hyper* hyper, lg_ppo_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = rec_check_call(p, rows, hidden, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  if (num_mini_batches < 1 || num_learning_epochs < 1) return lg_policy_fail(LG_ERR_INVALID, "num_mini_batches < 1 or num_learning_epochs < 1");
  const int64_t mb = N / num_mini_batches;
  if (mb <= 0) return lg_policy_fail(LG_ERR_INVALID, "N / num_mini_batches == 0");
  if ((int64_t)T * mb > p->max_rows) return lg_policy_fail(LG_ERR_INVALID, "T * (N / num_mini_batches) > max_rows of the trainer");
  DeviceScope ds_(p->device);
  hipStream_t st = (hipStream_t)stream;
  train_launch_ppo_stats(p, stats, 0, 1, st);
  for (int e = 0; e < num_learning_epochs; ++e)
    for (int i = 0; i < num_mini_batches; ++i) {
      const int r2 = rec_step(p, rows, hidden, dones, T, N, (int64_t)i * mb, mb, hyper, st, 1);
      if (r2 != LG_OK) return r2;
    }
  if (stats) train_launch_ppo_stats(p, stats, 1, num_mini_batches * num_learning_epochs, st);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int64_t lg_ppo_recurrent_parameter_count(lg_ppo_recurrent* p) {
  POLICY_ENTRY;
  return train_api_parameter_count(p);
}

int64_t lg_ppo_recurrent_workspace_bytes(lg_ppo_recurrent* p) {
  POLICY_ENTRY;
  return train_api_workspace_bytes(p);
}

int lg_ppo_recurrent_gradients(lg_ppo_recurrent* p, float* g, float* norm, float* means, void* stream) {
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

int lg_ppo_recurrent_forward_outputs(lg_ppo_recurrent* p, float* mean, float* values, void* stream) {
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

int lg_ppo_recurrent_get_state(lg_ppo_recurrent* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  POLICY_ENTRY;
  return train_api_get_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_ppo_recurrent_get_parameters(lg_ppo_recurrent* p, float* params, void* stream) {
  POLICY_ENTRY;
  return train_api_get_parameters(p, params, stream);
}

int lg_ppo_recurrent_set_state(lg_ppo_recurrent* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_ppo_recurrent_set_learning_rate(lg_ppo_recurrent* p, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_learning_rate(p, lr, stream);
}

int lg_ppo_recurrent_get_images(lg_ppo_recurrent* p, int32_t memory, int32_t layer, float* tiled, float* bias, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (memory < 0 || memory > 1 || layer < 0 || layer >= p->mem[0].L) return lg_policy_fail(LG_ERR_INVALID, "no such memory (0 | 1) or layer");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const RnnLayerDev& D = p->mem[memory].m->layer[layer];
  const size_t wcount = (size_t)D.nch * (D.nb + 1) * p->mem[memory].G * 256;
  if (tiled) POLICY_TRY(hipMemcpy(tiled, D.w, wcount * sizeof(float), hipMemcpyDeviceToHost));
  if (bias) POLICY_TRY(hipMemcpy(bias, D.b, (size_t)4 * 16 * D.nch * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

}  // extern "C"

// ---- ONE memory through the kernels above (lg_train_recurrent_internal.h): the launches of rec_step with grid.y = 1
void rec_launch_forward_one(const RnnStepArgs& S, const RnnSaveArgs& V, int64_t n, hipStream_t st) {
  RnnTrainPair P{};
  P.S[0] = S; P.V[0] = V;
  hipLaunchKernelGGL(rnn_train_forward_kernel, dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS), 1), dim3(MLP_THREADS), 0, st, P, n);
}

void rec_launch_backward_one(const RnnBackArgs& B, int64_t n, hipStream_t st) {
  RnnBackPair P{};
  P.B[0] = B;
  hipLaunchKernelGGL(rnn_backward_kernel, dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS), 1), dim3(MLP_THREADS), 0, st, P, n);
}

void rec_launch_rows_matmul_one(const RowsMatArgs& M, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(rows_matmul_kernel, dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS), 1), dim3(MLP_THREADS), 0, st, M, M, n);
}

void rec_launch_retile(const RnnRetile* tab, int count, int64_t big, const float* theta, hipStream_t st) {
  hipLaunchKernelGGL(rnn_retile_kernel, dim3((unsigned)((big + 255) / 256), count), dim3(256), 0, st, tab, theta);
}

// ---- one trained memory and its carried state (lg_train_recurrent_internal.h): truncated BPTT through the launches above
bool mem_alloc(TrainCore* c, TrainMem* M, lg_rnn* rnn) {
  bool ok = true;
  auto alloc = [&](size_t floats, bool zero) -> float* { float* d = ok ? (float*)train_alloc(c, floats * sizeof(float), zero) : nullptr; if (!d) ok = false; return d; };
  M->rnn = rnn; M->device = c->device; M->max_rows = c->max_rows;
  M->I = rnn->input; M->H = rnn->hidden; M->ML = rnn->num_layers; M->Gates = rnn->type == LG_RNN_GRU ? 3 : 4;
  const size_t R = (size_t)c->max_rows;
  const int H = M->H, ML = M->ML, K = M->Gates * H, nbk = (K + 15) / 16;
  const bool lstm = M->Gates == 4;
  M->zero_state = alloc(R * H, true);
  M->carry_h = alloc(ML * R * H, true); M->cur_h = alloc(ML * R * H, true);
  if (lstm) { M->carry_c = alloc(ML * R * H, true); M->cur_c = alloc(ML * R * H, true); }
  for (int l = 0; l < ML && ok; ++l) {
    MemLayer& Y = M->layer[l];
    const int I = l == 0 ? M->I : H;
    for (int g = 0; g < 4; ++g) Y.gate[g] = alloc(R * H, false);
    Y.hin = alloc(R * H, false); Y.hnew = alloc(R * H, false); Y.dup = alloc(R * H, false);
    Y.cin = lstm ? alloc(R * H, false) : nullptr; Y.cnew = lstm ? alloc(R * H, false) : nullptr;
    Y.Dih = alloc(R * K, false); Y.Dhh = lstm ? Y.Dih : alloc(R * K, false);
    for (int s = 0; s < 2; ++s) { Y.dh[s] = alloc(R * H, true); Y.dc[s] = lstm ? alloc(R * H, true) : nullptr; }
    Y.wtx = alloc((size_t)((I + 15) / 16) * nbk * 256, true);
    Y.wth = alloc((size_t)((H + 15) / 16) * nbk * 256, true);
  }
  return ok;
}

void mem_place_layer(TrainMem* M, int l, TrainSeg& Si, TrainSeg& Sh, int64_t* off) {
  Si.woff = *off; *off += (int64_t)Si.dO * Si.dI;
  Sh.woff = *off; *off += (int64_t)Sh.dO * Sh.dI;
  Si.boff = *off; *off += Si.dO;
  Sh.boff = *off; *off += Sh.dO;
  const RnnLayerDev& D = M->rnn->layer[l];
  RnnRetile& rt = M->retile[l];
  rt.w = const_cast<float*>(D.w); rt.b = const_cast<float*>(D.b); rt.G = M->Gates; rt.I = D.I; rt.H = D.H; rt.Ip = D.Ip; rt.nb = D.nb; rt.nch = D.nch;
  rt.wih = Si.woff; rt.whh = Sh.woff; rt.bih = Si.boff; rt.bhh = Sh.boff;
  const int64_t cnt = (int64_t)D.nch * (D.nb + 1) * rt.G * 256 + 4 * 16 * D.nch;
  if (cnt > M->retile_big) M->retile_big = cnt;
}

bool mem_upload_retile(TrainCore* c, TrainMem* M) {
  M->d_retile = (RnnRetile*)lg_policy_upload(M->retile, sizeof(RnnRetile) * (M->ML + 1), c->allocs);
  return M->d_retile != nullptr;
}

int mem_retile(const TrainMem* M, const float* theta, hipStream_t st) {
  rec_launch_retile(M->d_retile, M->ML, M->retile_big, theta, st);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int mem_check_rows(const TrainMem* M, int64_t N) {
  if (M->carry_n != 0 && M->carry_n != N) return lg_policy_fail(LG_ERR_INVALID, "N is not the carry's number of rows (reset the carry first)");
  return LG_OK;
}

int mem_open_carry(TrainMem* M, int64_t N, hipStream_t st) {
  if (M->carry_n == N) return LG_OK;
  const size_t bytes = (size_t)M->ML * M->max_rows * M->H * sizeof(float);
  POLICY_TRY(hipMemsetAsync(M->carry_h, 0, bytes, st));
  POLICY_TRY(hipMemsetAsync(M->cur_h, 0, bytes, st));
  if (M->carry_c) { POLICY_TRY(hipMemsetAsync(M->carry_c, 0, bytes, st)); POLICY_TRY(hipMemsetAsync(M->cur_c, 0, bytes, st)); }
  M->carry_n = N;
  return LG_OK;
}

// step s of the span reads a saved row (the carry or the running state), not the step before
static bool mem_saved_entry(const MemSpan& W, int64_t s) { return s == 0 || (W.t0 + s) % W.T == 0; }
static const float* mem_prev_dones(const TrainMem* M, const MemSpan& W, int64_t s) { return W.dones ? W.dones + ((W.t0 + s - 1) % W.T) * W.N : M->zero_state; }

void mem_forward(const TrainMem* M, const MemSpan& W, const float* x0, bool x0_by_time, hipStream_t st) {
  const int H = M->H;
  const int64_t N = W.N;
  const bool lstm = M->Gates == 4;
  const size_t lstride = (size_t)M->max_rows * H;
  for (int64_t s = 0; s < W.nsteps; ++s)
    for (int l = 0; l < M->ML; ++l) {
      const MemLayer& Y = M->layer[l];
      const size_t at = (size_t)s * N * H, before = s > 0 ? (size_t)(s - 1) * N * H : 0;
      const bool epoch = (W.t0 + s) % W.T == 0;
      RnnStepArgs S{}; RnnSaveArgs V{};
      S.L = M->rnn->layer[l];
      S.x = l == 0 ? x0 + (size_t)(x0_by_time ? (W.t0 + s) % W.T : s) * N * M->I : M->layer[l - 1].hnew + at;
      if (mem_saved_entry(W, s)) {
        V.hs = (epoch ? M->carry_h : M->cur_h) + l * lstride; V.cs = lstm ? (epoch ? M->carry_c : M->cur_c) + l * lstride : nullptr;
        V.hprev = nullptr; V.cprev = nullptr; V.dprev = nullptr;
      } else {
        V.hs = M->zero_state; V.cs = lstm ? M->zero_state : nullptr;
        V.hprev = Y.hnew + before; V.cprev = lstm ? Y.cnew + before : nullptr; V.dprev = mem_prev_dones(M, W, s);
      }
      for (int g = 0; g < 4; ++g) V.gate[g] = Y.gate[g] + at;
      V.hin = Y.hin + at; V.hnew = Y.hnew + at;
      V.cin = lstm ? Y.cin + at : nullptr; V.cnew = lstm ? Y.cnew + at : nullptr;
      rec_launch_forward_one(S, V, N, st);
    }
}

void mem_top_matmul(const TrainMem* M, const TrainNet& head, int64_t n, hipStream_t st) {
  RowsMatArgs A;
  A.A = head.d[0]; A.K = head.dims[1]; A.nbk = head.bkpad[0] / 16; A.wt = head.bw[0]; A.nout = M->H; A.nch = (M->H + 15) / 16; A.out = M->layer[M->ML - 1].dup;
  rec_launch_rows_matmul_one(A, n, st);
}

void mem_backward(const TrainMem* M, const MemSpan& W, float* dx0, hipStream_t st) {
  const int H = M->H;
  const int64_t N = W.N, nsteps = W.nsteps;
  const bool lstm = M->Gates == 4;
  for (int64_t s = nsteps - 1; s >= 0; --s)
    for (int l = M->ML - 1; l >= 0; --l) {
      const MemLayer& Y = M->layer[l];
      const size_t at = (size_t)s * N * H;
      const int Il = l == 0 ? M->I : H;
      RnnBackArgs b{};
      b.gru = lstm ? 0 : 1; b.I = Il; b.H = H; b.K = M->Gates * H; b.nbk = (b.K + 15) / 16;
      b.dx = l > 0 ? M->layer[l - 1].dup + at : (dx0 ? dx0 + (size_t)s * N * M->I : nullptr);
      b.nchx = b.dx ? (Il + 15) / 16 : 0; b.nchh = (H + 15) / 16;
      b.wtx = Y.wtx; b.wth = Y.wth;
      for (int g = 0; g < 4; ++g) b.gate[g] = Y.gate[g] + at;
      b.hin = Y.hin + at; b.cin = lstm ? Y.cin + at : nullptr; b.cnew = lstm ? Y.cnew + at : nullptr;
      b.dup = Y.dup + at;
      b.dh_in = s + 1 < nsteps ? Y.dh[(s + 1) & 1] : nullptr; b.dc_in = (s + 1 < nsteps && lstm) ? Y.dc[(s + 1) & 1] : nullptr;
      b.dprev = mem_saved_entry(W, s) ? nullptr : mem_prev_dones(M, W, s);
      b.dh_out = Y.dh[s & 1]; b.dc_out = lstm ? Y.dc[s & 1] : nullptr;
      b.Dih = Y.Dih + (size_t)s * N * b.K; b.Dhh = Y.Dhh + (size_t)s * N * b.K;
      rec_launch_backward_one(b, N, st);
    }
}

int mem_keep_running(TrainMem* M, const MemSpan& W, hipStream_t st) {
  const size_t lstride = (size_t)M->max_rows * M->H, last = (size_t)(W.nsteps - 1) * W.N * M->H, bytes = (size_t)W.N * M->H * sizeof(float);
  for (int l = 0; l < M->ML; ++l) {
    POLICY_TRY(hipMemcpyAsync(M->cur_h + l * lstride, M->layer[l].hnew + last, bytes, hipMemcpyDeviceToDevice, st));
    if (M->cur_c) POLICY_TRY(hipMemcpyAsync(M->cur_c + l * lstride, M->layer[l].cnew + last, bytes, hipMemcpyDeviceToDevice, st));
  }
  return LG_OK;
}

int mem_keep_carry(TrainMem* M, hipStream_t st) {
  const size_t bytes = (size_t)M->ML * M->max_rows * M->H * sizeof(float);
  POLICY_TRY(hipMemcpyAsync(M->carry_h, M->cur_h, bytes, hipMemcpyDeviceToDevice, st));
  if (M->carry_c) POLICY_TRY(hipMemcpyAsync(M->carry_c, M->cur_c, bytes, hipMemcpyDeviceToDevice, st));
  return LG_OK;
}

int64_t mem_get_carry(TrainMem* M, float* h, float* c, int64_t capacity_rows, int32_t running, hipMemcpyKind kind, void* stream) {
  if (!M) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  const int64_t N = M->carry_n;
  if (!h || N == 0 || capacity_rows < N) return N;
  DeviceScope ds_(M->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const size_t lstride = (size_t)M->max_rows * M->H, row = (size_t)N * M->H;
  for (int l = 0; l < M->ML; ++l) {
    POLICY_TRY(hipMemcpy(h + l * row, (running ? M->cur_h : M->carry_h) + l * lstride, row * sizeof(float), kind));
    if (c && M->carry_c) POLICY_TRY(hipMemcpy(c + l * row, (running ? M->cur_c : M->carry_c) + l * lstride, row * sizeof(float), kind));
  }
  return N;
}

int mem_set_carry(TrainMem* M, const float* h, const float* c, int64_t N, hipMemcpyKind kind, void* stream) {
  if (!M || !h) return lg_policy_fail(LG_ERR_INVALID, "null trainer or state");
  if (M->carry_c && !c) return lg_policy_fail(LG_ERR_INVALID, "an LSTM needs its cell state");
  if (N < 1 || N > M->max_rows) return lg_policy_fail(LG_ERR_INVALID, "N < 1 or N > max_rows of the trainer");
  DeviceScope ds_(M->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const size_t lstride = (size_t)M->max_rows * M->H, row = (size_t)N * M->H;
  for (int l = 0; l < M->ML; ++l) {
    POLICY_TRY(hipMemcpy(M->carry_h + l * lstride, h + l * row, row * sizeof(float), kind));
    POLICY_TRY(hipMemcpy(M->cur_h + l * lstride, h + l * row, row * sizeof(float), kind));
    if (M->carry_c) {
      POLICY_TRY(hipMemcpy(M->carry_c + l * lstride, c + l * row, row * sizeof(float), kind));
      POLICY_TRY(hipMemcpy(M->cur_c + l * lstride, c + l * row, row * sizeof(float), kind));
    }
  }
  M->carry_n = N;
  return LG_OK;
}

int mem_reset_carry(TrainMem* M) {
  if (!M) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  M->carry_n = 0;
  return LG_OK;
}
