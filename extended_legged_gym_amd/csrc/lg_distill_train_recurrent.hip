// lg_distill_train_recurrent.hip — Distillation.update (include/lgdistill_recurrent.h) for the recurrent student: a trainer over the student's memory
// (lg_rnn) and MLP (lg_mlp).  A group of G steps is one batch of G * N rows, step-major.  Reused as they are: the memory's forward with saved gates /
// backward step / rows x transposed tiling / retile (lg_train_recurrent_internal.h), the MLP's forward with saved activations, backward data pass,
// slab weight gradients and reduction (lg_train_internal.h), the row index and the behaviour loss (lg_distill_train_internal.h).  New here:
//
//   rdistill_norm_kernel       TWO norms from the reduction's block sums, in block order: over the student's segments (the one the clip uses) and over
//                              the memory's; the clip coefficient from the first alone; the step count and Adam's bias corrections.
//   rdistill_adam_kernel       ppo_adam_kernel's arithmetic, with the clip coefficient applied to the first nclip segments only (student.*): the
//                              gradients of memory_s.* enter Adam as they are.  The same lane rewrites the element in the MLP's forward tiling and in
//                              the transposed tilings; the memory's forward images are rnn_retile_kernel's.
//   rdistill_mask_rows_kernel  Memory.reset(dones): zero h (and c) in every layer for the rows whose episode ended.
//   rdistill_stats_kernel      clears the update's sums / writes the stats.
// No host synchronisation inside an update and no atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_train_internal.h"
#include "lg_train_recurrent_internal.h"
#include "lg_distill_train_internal.h"
#include "../../include/lgdistill_recurrent.h"

#define RDISTILL_MAX_STEPS 65535    // steps of one batch: blockIdx.y of the loss kernel

struct RDistillScalars {
  float memory_norm;                 // the norm over memory_s.* of the last optimiser step
};

// norm_part: [segment][block] sums of squares; the first n_student entries are student.*'s
__global__ __launch_bounds__(256) void rdistill_norm_kernel(const float* __restrict__ norm_part, int n_student, int n_all, float max_grad_norm, int clip_on,
                                                            TrainScalars* __restrict__ sc, RDistillScalars* __restrict__ rs) {
  __shared__ float red[256];
  float s = 0.f, m = 0.f;
  for (int i = threadIdx.x; i < n_student; i += 256) s += norm_part[i];
  for (int i = n_student + threadIdx.x; i < n_all; i += 256) m += norm_part[i];
  const float ts = block_sum_256(s, red);
  __syncthreads();
  const float tm = block_sum_256(m, red);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(ts);
    sc->norm = norm;
    rs->memory_norm = sqrtf(tm);
    sc->clip = clip_on ? fminf(1.f, max_grad_norm / (norm + 1e-6f)) : 1.f;  // clip_grad_norm_(policy.student.parameters(), max_grad_norm)
    const int64_t t = sc->step + 1;
    sc->step = t;
    sc->step_size = (float)(sc->lr / (1.0 - pow(0.9, (double)t)));         // torch.optim.Adam, defaults
    sc->bc2_sqrt = (float)sqrt(1.0 - pow(0.999, (double)t));
  }
}

// blockIdx.y: a segment; segments [0, nclip) take the clip coefficient, the others pass unscaled
__global__ __launch_bounds__(256) void rdistill_adam_kernel(const TrainSeg* __restrict__ segs, int nclip, float* __restrict__ theta, float* __restrict__ m1,
                                                            float* __restrict__ m2, const float* __restrict__ G, const TrainScalars* __restrict__ sc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const TrainSeg S = segs[blockIdx.y];
  const int W = S.dI + 1;
  if (e >= (int64_t)S.dO * W) return;
  const int o = (int)(e / W), i = (int)(e - (int64_t)o * W);
  const int64_t flat = i < S.dI ? S.woff + (int64_t)o * S.dI + i : S.boff + o;
  const float clip = (int)blockIdx.y < nclip ? sc->clip : 1.f;
  const float g = G[flat] * clip;
  float a = m1[flat], b = m2[flat];
  a = a + (g - a) * 0.1f;                                     // exp_avg.lerp_(grad, 1 - beta1)
  b = b * 0.999f + 0.001f * g * g;                            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  m1[flat] = a; m2[flat] = b;
  const float th = theta[flat] - sc->step_size * (a / (sqrtf(b) / sc->bc2_sqrt + 1e-8f));
  theta[flat] = th;
  if (i == S.dI) { if (S.fb) S.fb[o] = th; return; }
  // the tilings of ppo_adam_kernel (lg_train.hip): forward chunk o / 16, block i / 16, lane (o % 16) + 16 (i % 4), slot (i / 4) % 4; transposed: o and i exchanged
  if (S.fw) S.fw[((((size_t)(o >> 4) * S.f_nb + (i >> 4)) * 64) + ((o & 15) | ((i & 3) << 4))) * 4 + ((i >> 2) & 3)] = th;
  if (S.bw) S.bw[((((size_t)(i >> 4) * S.b_nb + (o >> 4)) * 64) + ((i & 15) | ((o & 3) << 4))) * 4 + ((o >> 2) & 3)] = th;
}

// h, c (layers, cap, H) (c may be NULL): rows j < N of every layer with dones[j] != 0 -> 0
__global__ __launch_bounds__(256) void rdistill_mask_rows_kernel(float* __restrict__ h, float* __restrict__ c, const float* __restrict__ dones, int64_t N, int H,
                                                                 int64_t layer_stride, int layers) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * H) return;
  if (dones[idx / H] != 0.f)
    for (int l = 0; l < layers; ++l) { h[l * layer_stride + idx] = 0.f; if (c) c[l * layer_stride + idx] = 0.f; }
}

// mode 0: clear the update's sums; 1: write the stats
__global__ void rdistill_stats_kernel(DistillScalars* __restrict__ ds, const TrainScalars* __restrict__ sc, const RDistillScalars* __restrict__ rs,
                                      lg_distill_rtrain_stats* __restrict__ stats, int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (mode == 0) { ds->acc = 0.0; ds->steps = 0; ds->optimizer_steps = 0; return; }
  stats->behavior = ds->acc / (double)ds->steps;
  stats->optimizer_steps = (double)ds->optimizer_steps;
  stats->grad_norm = (double)sc->norm;
  stats->memory_grad_norm = (double)rs->memory_norm;
}

// ------------------------------------------------------------------------------------------------------------------------ host side
struct RDistillLayer {
  float *gate[4], *hin, *cin, *cnew, *hnew, *dup, *Dih, *Dhh, *dh[2], *dc[2];
  float *wtx, *wth;
};

struct lg_distill_rtrain : TrainCore {
  lg_rnn* mem = nullptr; lg_mlp* student = nullptr;
  int S_in = 0, H = 0, Gates = 0, ML = 0, A = 0;
  int nstudent = 0;                            // segments [0, nstudent): student.*, the ones the clip covers; then weight_ih, weight_hh per memory layer
  int64_t student_floats = 0;
  RDistillLayer layer[RNN_MAX_LAYERS];
  float* zero_state = nullptr;
  float *carry_h = nullptr, *carry_c = nullptr, *cur_h = nullptr, *cur_c = nullptr;          // (ML, max_rows, H)
  int64_t carry_n = 0;
  RnnRetile* d_retile = nullptr; int64_t retile_big = 0;
  int64_t last_steps = 0, last_update_steps = 0, seq_cap = 0;
  int64_t* rows = nullptr;
  float *loss_part = nullptr, *step_tmp = nullptr, *group_loss = nullptr, *seq_loss = nullptr;
  DistillScalars* ds = nullptr;
  RDistillScalars* rs = nullptr;
};

// the masters -> the memory's forward images (the MLP's and every transposed tiling are the Adam kernel's / train_core_retile's)
static int rdistill_retile(lg_distill_rtrain* p, hipStream_t st) {
  rec_launch_retile(p->d_retile, p->ML, p->retile_big, p->theta, st);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

static int rdistill_check_call(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, const lg_distill_train_hyper* h) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!obs || !tgt || !dones || !h) return lg_policy_fail(LG_ERR_INVALID, "null observations, targets, dones or hyper-parameters");
  if (T < 1 || N < 1) return lg_policy_fail(LG_ERR_INVALID, "T < 1 or N < 1");
  if (h->loss_type != LG_LOSS_MSE && h->loss_type != LG_LOSS_HUBER) return lg_policy_fail(LG_ERR_INVALID, "unknown loss type (mse | huber)");
  if (p->carry_n != 0 && p->carry_n != N) return lg_policy_fail(LG_ERR_INVALID, "N is not the carry's number of rows (reset the carry first)");
  return LG_OK;
}

// the first call after a reset: zero carry and running state for N rows
static int rdistill_open_carry(lg_distill_rtrain* p, int64_t N, hipStream_t st) {
  if (p->carry_n == N) return LG_OK;
  const size_t bytes = (size_t)p->ML * p->max_rows * p->H * sizeof(float);
  POLICY_TRY(hipMemsetAsync(p->carry_h, 0, bytes, st));
  POLICY_TRY(hipMemsetAsync(p->cur_h, 0, bytes, st));
  if (p->carry_c) { POLICY_TRY(hipMemsetAsync(p->carry_c, 0, bytes, st)); POLICY_TRY(hipMemsetAsync(p->cur_c, 0, bytes, st)); }
  p->carry_n = N;
  return LG_OK;
}

// steps [first, first + nsteps) of the sequence as one batch; train: an optimiser step, else forward and loss only.  seq_loss: where the update keeps
// these steps' losses, or NULL (a group call: the losses go to group_loss either way).
static int rdistill_steps(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, int64_t first, int64_t nsteps,
                          const lg_distill_train_hyper* h, bool train, float* seq_loss, hipStream_t st) {
  const int64_t n = nsteps * N, t0 = first % T;
  const int H = p->H, L = p->ML;
  const bool lstm = p->Gates == 4;
  const size_t lstride = (size_t)p->max_rows * H;
  int rc = rdistill_open_carry(p, N, st);
  if (rc != LG_OK) return rc;
  p->last_rows = n;
  if (train || !seq_loss) p->last_steps = nsteps;
  // ---- the memory through time.  A step with time index 0 enters with the carry, the batch's first step otherwise with the running state, both as
  // constants (dprev NULL: every row reads the saved row); every other step with the step before's state, zero where its dones ended the episode
  auto saved_entry = [&](int64_t s) { return s == 0 || (t0 + s) % T == 0; };
  auto prev_dones = [&](int64_t s) -> const float* { return dones + ((t0 + s - 1) % T) * N; };
  for (int64_t s = 0; s < nsteps; ++s)
    for (int l = 0; l < L; ++l) {
      const RDistillLayer& Y = p->layer[l];
      const size_t at = (size_t)s * N * H, before = s > 0 ? (size_t)(s - 1) * N * H : 0;
      const bool epoch = (t0 + s) % T == 0;
      RnnStepArgs S{}; RnnSaveArgs V{};
      S.L = p->mem->layer[l];
      S.x = l == 0 ? obs + (size_t)((t0 + s) % T) * N * p->S_in : p->layer[l - 1].hnew + at;
      if (saved_entry(s)) {
        V.hs = (epoch ? p->carry_h : p->cur_h) + l * lstride; V.cs = lstm ? (epoch ? p->carry_c : p->cur_c) + l * lstride : nullptr;
        V.hprev = nullptr; V.cprev = nullptr; V.dprev = nullptr;
      } else {
        V.hs = p->zero_state; V.cs = lstm ? p->zero_state : nullptr;
        V.hprev = Y.hnew + before; V.cprev = lstm ? Y.cnew + before : nullptr; V.dprev = prev_dones(s);
      }
      for (int g = 0; g < 4; ++g) V.gate[g] = Y.gate[g] + at;
      V.hin = Y.hin + at; V.hnew = Y.hnew + at;
      V.cin = lstm ? Y.cin + at : nullptr; V.cnew = lstm ? Y.cnew + at : nullptr;
      rec_launch_forward_one(S, V, N, st);
    }
  // ---- the student on the memory's outputs, the losses
  const TrainNet& Sn = p->net[0];
  const float* top = p->layer[L - 1].hnew;
  train_launch_forward(p, top, top, nullptr, n, st);
  distill_launch_loss(Sn.a[Sn.L], tgt, N, p->A, T, t0, nsteps, h->loss_type, train ? Sn.d[Sn.L - 1] : (float*)nullptr, p->loss_part, p->step_tmp, p->group_loss,
                      seq_loss ? seq_loss : (train ? (float*)nullptr : p->group_loss), p->ds, train ? 1 : 0, st);
  if (train) {
    // ---- the student backwards and dL/d(its input)
    train_launch_backward(p, n, st);
    {
      RowsMatArgs M;
      M.A = Sn.d[0]; M.K = Sn.dims[1]; M.nbk = Sn.bkpad[0] / 16; M.wt = Sn.bw[0]; M.nout = H; M.nch = (H + 15) / 16; M.out = p->layer[L - 1].dup;
      rec_launch_rows_matmul_one(M, n, st);
    }
    // ---- backwards through time; nothing is propagated into the observations
    for (int64_t s = nsteps - 1; s >= 0; --s)
      for (int l = L - 1; l >= 0; --l) {
        const RDistillLayer& Y = p->layer[l];
        const size_t at = (size_t)s * N * H;
        const int Il = l == 0 ? p->S_in : H;
        RnnBackArgs b{};
        b.gru = lstm ? 0 : 1; b.I = Il; b.H = H; b.K = p->Gates * H; b.nbk = (b.K + 15) / 16;
        b.nchx = l > 0 ? (Il + 15) / 16 : 0; b.nchh = (H + 15) / 16;
        b.wtx = Y.wtx; b.wth = Y.wth;
        for (int g = 0; g < 4; ++g) b.gate[g] = Y.gate[g] + at;
        b.hin = Y.hin + at; b.cin = lstm ? Y.cin + at : nullptr; b.cnew = lstm ? Y.cnew + at : nullptr;
        b.dup = Y.dup + at;
        b.dh_in = s + 1 < nsteps ? Y.dh[(s + 1) & 1] : nullptr; b.dc_in = (s + 1 < nsteps && lstm) ? Y.dc[(s + 1) & 1] : nullptr;
        b.dprev = saved_entry(s) ? nullptr : prev_dones(s);
        b.dh_out = Y.dh[s & 1]; b.dc_out = lstm ? Y.dc[s & 1] : nullptr;
        b.dx = l > 0 ? p->layer[l - 1].dup + at : nullptr;
        b.Dih = Y.Dih + (size_t)s * N * b.K; b.Dhh = Y.Dhh + (size_t)s * N * b.K;
        rec_launch_backward_one(b, N, st);
      }
    // ---- every weight gradient in one slab pass (weight_ih of layer 0 gathers its observation rows), the reduction, the two norms, Adam, the images
    distill_launch_rows(p->rows, n, N, T, t0, st);
    train_launch_wgrad_range(p, 0, p->nseg, obs, obs, p->rows, n, st);
    train_launch_reduce_range(p, 0, p->nseg, (int)((n + WGRAD_SLAB - 1) / WGRAD_SLAB), st);
    hipLaunchKernelGGL(rdistill_norm_kernel, dim3(1), dim3(256), 0, st, (const float*)p->norm_part, p->red_blocks * p->nstudent, p->red_blocks * p->nseg, h->max_grad_norm,
                       h->max_grad_norm > 0.f ? 1 : 0, p->sc, p->rs);
    hipLaunchKernelGGL(rdistill_adam_kernel, dim3((unsigned)((p->big + 255) / 256), p->nseg), dim3(256), 0, st, (const TrainSeg*)p->d_seg, p->nstudent, p->theta, p->m,
                       p->v, (const float*)p->G, (const TrainScalars*)p->sc);
    if ((rc = rdistill_retile(p, st)) != LG_OK) return rc;
  }
  // ---- the running state: the memory after the last step, its dones applied
  for (int l = 0; l < L; ++l) {
    const size_t last = (size_t)(nsteps - 1) * N * H, bytes = (size_t)N * H * sizeof(float);
    POLICY_TRY(hipMemcpyAsync(p->cur_h + l * lstride, p->layer[l].hnew + last, bytes, hipMemcpyDeviceToDevice, st));
    if (lstm) POLICY_TRY(hipMemcpyAsync(p->cur_c + l * lstride, p->layer[l].cnew + last, bytes, hipMemcpyDeviceToDevice, st));
  }
  hipLaunchKernelGGL(rdistill_mask_rows_kernel, dim3((unsigned)((N * H + 255) / 256)), dim3(256), 0, st, p->cur_h, lstm ? p->cur_c : (float*)nullptr,
                     dones + ((t0 + nsteps - 1) % T) * N, N, H, (int64_t)lstride, L);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

extern "C" {

void lg_distill_rtrain_destroy(lg_distill_rtrain* p) {
  if (!p) return;
  DeviceScope ds_(p->device);
  (void)hipDeviceSynchronize();
  train_core_free(p);
  delete p;
}

lg_distill_rtrain* lg_distill_rtrain_create(lg_rnn* mem, lg_mlp* student, const lg_distill_rtrain_params* q, double learning_rate, int64_t max_rows) {
  POLICY_ENTRY;
  if (!mem || !student) { lg_policy_fail(LG_ERR_INVALID, "null memory or network"); return nullptr; }
  if (!q) { lg_policy_fail(LG_ERR_INVALID, "null parameters"); return nullptr; }
  if (!q->student_weights || !q->student_biases || !q->memory_w_ih || !q->memory_w_hh || !q->memory_b_ih || !q->memory_b_hh) {
    lg_policy_fail(LG_ERR_INVALID, "null parameter list"); return nullptr; }
  if (max_rows < 1) { lg_policy_fail(LG_ERR_INVALID, "max_rows < 1"); return nullptr; }
  if (!(learning_rate > 0.0)) { lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0"); return nullptr; }
  if (student->h.act_out) { lg_policy_fail(LG_ERR_UNSUPPORTED, "a network with an output activation cannot be trained here"); return nullptr; }
  if (student->h.dims[0] != mem->hidden) { lg_policy_fail(LG_ERR_INVALID, "the MLP's input width is not the memory's hidden width"); return nullptr; }
  if (student->device != mem->device) { lg_policy_fail(LG_ERR_INVALID, "the memory and the network live on different devices"); return nullptr; }
  const int ML = mem->num_layers, Ls = student->h.L, H = mem->hidden;
  if (ML < 1 || ML > RNN_MAX_LAYERS) { lg_policy_fail(LG_ERR_INVALID, "memory depth out of range"); return nullptr; }
  for (int l = 0; l < Ls; ++l) if (!q->student_weights[l] || !q->student_biases[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  for (int l = 0; l < ML; ++l) if (!q->memory_w_ih[l] || !q->memory_w_hh[l] || !q->memory_b_ih[l] || !q->memory_b_hh[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  if (!lg_policy_device_ok(student->device)) return nullptr;
  DeviceScope ds_(student->device);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_distill_rtrain* p = new lg_distill_rtrain();
  p->mem = mem; p->student = student; p->device = student->device; p->max_rows = max_rows;
  p->S_in = mem->input; p->H = H; p->ML = ML; p->Gates = mem->type == LG_RNN_GRU ? 3 : 4; p->A = student->h.dims[Ls];
  bool ok = true;
  auto alloc = [&](size_t floats, bool zero) -> float* { float* d = ok ? (float*)train_alloc(p, floats * sizeof(float), zero) : nullptr; if (!d) ok = false; return d; };
  const size_t R = (size_t)max_rows;
  const int slabs_max = (int)((max_rows + WGRAD_SLAB - 1) / WGRAD_SLAB);
  const int K = p->Gates * H, nbk = (K + 15) / 16;
  const bool lstm = p->Gates == 4;
  p->zero_state = alloc(R * H, true);
  p->carry_h = alloc(ML * R * H, true); p->cur_h = alloc(ML * R * H, true);
  if (lstm) { p->carry_c = alloc(ML * R * H, true); p->cur_c = alloc(ML * R * H, true); }
  // ---- segments: the student's (net 0, at the head of the flat vector), then weight_ih / weight_hh of every memory layer.  Layer ids behind the
  // student's index the host tables.
  int64_t off = 0;
  ok = ok && train_core_add_net(p, student, &off);
  p->nstudent = p->nseg; p->student_floats = off;
  enum { ID_MEM = LG_MLP_MAX_LAYERS, ID_COUNT = ID_MEM + 2 * RNN_MAX_LAYERS };
  const float* wtab[ID_COUNT] = {}; const float* btab[ID_COUNT] = {};
  for (int l = 0; l < Ls; ++l) { wtab[l] = q->student_weights[l]; btab[l] = q->student_biases[l]; }
  auto dense_seg = [&](int id, int dO, int dI, const float* Dp, const float* Ain, float* bw, int b_nb) -> TrainSeg& {
    TrainSeg& S = p->seg[p->nseg++];
    S.net = 0; S.layer = id; S.dO = dO; S.dI = dI; S.f_nb = 0; S.b_nb = b_nb; S.woff = 0; S.boff = 0;
    S.D = Dp; S.Ain = Ain; S.partial = alloc((size_t)slabs_max * dO * (dI + 1), false);
    S.fw = nullptr; S.fb = nullptr; S.bw = bw;
    const int64_t cnt = (int64_t)dO * (dI + 1);
    if (cnt > p->big) p->big = cnt;
    const int tiles = ((dO + 31) / 32) * ((dI + 1 + 63) / 64);
    if ((tiles + 3) / 4 > p->wgrad_blocks) p->wgrad_blocks = (tiles + 3) / 4;
    return S;
  };
  std::vector<RnnRetile> rret;
  for (int l = 0; l < ML && ok; ++l) {
    RDistillLayer& Y = p->layer[l];
    const int I = l == 0 ? p->S_in : H;
    for (int g = 0; g < 4; ++g) Y.gate[g] = alloc(R * H, false);
    Y.hin = alloc(R * H, false); Y.hnew = alloc(R * H, false); Y.dup = alloc(R * H, false);
    Y.cin = lstm ? alloc(R * H, false) : nullptr; Y.cnew = lstm ? alloc(R * H, false) : nullptr;
    Y.Dih = alloc(R * K, false); Y.Dhh = lstm ? Y.Dih : alloc(R * K, false);
    for (int s = 0; s < 2; ++s) { Y.dh[s] = alloc(R * H, true); Y.dc[s] = lstm ? alloc(R * H, true) : nullptr; }
    Y.wtx = alloc((size_t)((I + 15) / 16) * nbk * 256, true);
    Y.wth = alloc((size_t)((H + 15) / 16) * nbk * 256, true);
    // weight_ih of layer 0 reads the gathered observation rows (Ain NULL); the flat order of a layer is weight_ih, weight_hh, bias_ih, bias_hh
    TrainSeg& Si = dense_seg(ID_MEM + 2 * l, K, I, Y.Dih, l == 0 ? nullptr : p->layer[l - 1].hnew, Y.wtx, nbk);
    TrainSeg& Sh = dense_seg(ID_MEM + 2 * l + 1, K, H, Y.Dhh, Y.hin, Y.wth, nbk);
    wtab[ID_MEM + 2 * l] = q->memory_w_ih[l]; btab[ID_MEM + 2 * l] = q->memory_b_ih[l];
    wtab[ID_MEM + 2 * l + 1] = q->memory_w_hh[l]; btab[ID_MEM + 2 * l + 1] = q->memory_b_hh[l];
    Si.woff = off; off += (int64_t)K * I;
    Sh.woff = off; off += (int64_t)K * H;
    Si.boff = off; off += K;
    Sh.boff = off; off += K;
    const RnnLayerDev& D = mem->layer[l];
    RnnRetile rt;
    rt.w = const_cast<float*>(D.w); rt.b = const_cast<float*>(D.b); rt.G = p->Gates; rt.I = D.I; rt.H = D.H; rt.Ip = D.Ip; rt.nb = D.nb; rt.nch = D.nch;
    rt.wih = Si.woff; rt.whh = Sh.woff; rt.bih = Si.boff; rt.bhh = Sh.boff;
    rret.push_back(rt);
    const int64_t cnt = (int64_t)D.nch * (D.nb + 1) * rt.G * 256 + 4 * 16 * D.nch;
    if (cnt > p->retile_big) p->retile_big = cnt;
  }
  // the student's first layer reads the top layer's h' (dense, step-major) and propagates into it: a transposed tiling for layer 0 too
  if (ok) {
    TrainNet& Nn = p->net[0];
    float* bw0 = alloc((size_t)Nn.bnch[0] * (Nn.bkpad[0] / 16) * 256, true);
    Nn.bw[0] = bw0; p->seg[0].bw = bw0; p->seg[0].Ain = p->layer[ML - 1].hnew;
  }
  auto zalloc = [&](size_t bytes) -> void* { void* d = ok ? train_alloc(p, bytes, true) : nullptr; if (!d) ok = false; return d; };
  p->loss_part = (float*)zalloc(distill_loss_floats(max_rows, p->A) * sizeof(float));
  p->rows = (int64_t*)zalloc(R * sizeof(int64_t));
  p->step_tmp = (float*)zalloc(R * sizeof(float));
  p->group_loss = (float*)zalloc(R * sizeof(float));
  p->seq_cap = 1024;
  p->seq_loss = (float*)zalloc((size_t)p->seq_cap * sizeof(float));
  p->ds = (DistillScalars*)zalloc(sizeof(DistillScalars));
  p->rs = (RDistillScalars*)zalloc(sizeof(RDistillScalars));
  p->d_retile = (RnnRetile*)zalloc(sizeof(RnnRetile) * (rret.size() + 1));
  const float* const* ws[1] = {wtab};
  const float* const* bs[1] = {btab};
  if (!ok || train_core_finish(p, off, ws, bs, nullptr, learning_rate) != LG_OK ||
      hipMemcpy(p->d_retile, rret.data(), sizeof(RnnRetile) * rret.size(), hipMemcpyHostToDevice) != hipSuccess || rdistill_retile(p, nullptr) != LG_OK ||
      hipDeviceSynchronize() != hipSuccess) {
    lg_distill_rtrain_destroy(p);
    return nullptr;
  }
  return p;
}

int lg_distill_rtrain_group(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, int64_t first_step, int64_t num_steps,
                            int32_t train, const lg_distill_train_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  const int rc = rdistill_check_call(p, obs, tgt, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  if (num_steps < 1 || first_step < 0) return lg_policy_fail(LG_ERR_INVALID, "num_steps < 1 or first_step < 0");
  if (num_steps > RDISTILL_MAX_STEPS) return lg_policy_fail(LG_ERR_INVALID, "num_steps > 65535");
  if (N > p->max_rows || num_steps > p->max_rows / N) return lg_policy_fail(LG_ERR_INVALID, "num_steps * N > max_rows of the trainer");
  DeviceScope ds_(p->device);
  return rdistill_steps(p, obs, tgt, dones, T, N, first_step, num_steps, hyper, train != 0, nullptr, (hipStream_t)stream);
}

int lg_distill_rtrain_update(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, int32_t E, int32_t G,
                             const lg_distill_train_hyper* hyper, lg_distill_rtrain_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = rdistill_check_call(p, obs, tgt, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  if (E < 1 || G < 1) return lg_policy_fail(LG_ERR_INVALID, "num_learning_epochs < 1 or gradient_length < 1");
  if (G > RDISTILL_MAX_STEPS) return lg_policy_fail(LG_ERR_INVALID, "gradient_length > 65535");
  if (N > p->max_rows || G > p->max_rows / N) return lg_policy_fail(LG_ERR_INVALID, "gradient_length * N > max_rows of the trainer");
  DeviceScope ds_(p->device);
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)E * T;
  if (total > p->seq_cap) {                                  // (the old vector stays with the trainer: kernels in flight may still write it)
    float* grown = (float*)train_alloc(p, (size_t)total * sizeof(float), true);
    if (!grown) return LG_ERR_HIP;
    p->seq_loss = grown; p->seq_cap = total;
  }
  p->last_update_steps = total;
  hipLaunchKernelGGL(rdistill_stats_kernel, dim3(1), dim3(1), 0, st, p->ds, (const TrainScalars*)p->sc, (const RDistillScalars*)p->rs, stats, 0);
  int64_t k = 0;
  for (; total - k >= G; k += G) {
    const int r2 = rdistill_steps(p, obs, tgt, dones, T, N, k, G, hyper, true, p->seq_loss + k, st);
    if (r2 != LG_OK) return r2;
  }
  if (k < total) {
    const int r2 = rdistill_steps(p, obs, tgt, dones, T, N, k, total - k, hyper, false, p->seq_loss + k, st);
    if (r2 != LG_OK) return r2;
  }
  const size_t bytes = (size_t)p->ML * p->max_rows * p->H * sizeof(float);
  POLICY_TRY(hipMemcpyAsync(p->carry_h, p->cur_h, bytes, hipMemcpyDeviceToDevice, st));
  if (p->carry_c) POLICY_TRY(hipMemcpyAsync(p->carry_c, p->cur_c, bytes, hipMemcpyDeviceToDevice, st));
  if (stats) hipLaunchKernelGGL(rdistill_stats_kernel, dim3(1), dim3(1), 0, st, p->ds, (const TrainScalars*)p->sc, (const RDistillScalars*)p->rs, stats, 1);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int64_t lg_distill_rtrain_parameter_count(lg_distill_rtrain* p) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  return p->P;
}

int64_t lg_distill_rtrain_student_parameter_count(lg_distill_rtrain* p) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  return p->student_floats;
}

int64_t lg_distill_rtrain_workspace_bytes(lg_distill_rtrain* p) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  DeviceScope ds_(p->device);
  int64_t total = 0;
  for (void* d : p->allocs) {
    size_t bytes = 0;
    if (hipMemPtrGetInfo(d, &bytes) == hipSuccess) total += (int64_t)bytes;
  }
  return total;
}

int lg_distill_rtrain_gradients(lg_distill_rtrain* p, float* g, float* norms, float* losses, int64_t capacity, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (losses && capacity < p->last_steps) return lg_policy_fail(LG_ERR_INVALID, "the last group had more steps than the buffer holds");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (g) POLICY_TRY(hipMemcpy(g, p->G, (size_t)p->P * sizeof(float), hipMemcpyDeviceToHost));
  if (norms) {
    POLICY_TRY(hipMemcpy(norms, &p->sc->norm, sizeof(float), hipMemcpyDeviceToHost));
    POLICY_TRY(hipMemcpy(norms + 1, &p->rs->memory_norm, sizeof(float), hipMemcpyDeviceToHost));
  }
  if (losses && p->last_steps > 0) POLICY_TRY(hipMemcpy(losses, p->group_loss, (size_t)p->last_steps * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int lg_distill_rtrain_forward_outputs(lg_distill_rtrain* p, float* actions, void* stream) {
  POLICY_ENTRY;
  if (!p || !actions) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  if (p->last_rows <= 0) return lg_policy_fail(LG_ERR_INVALID, "no group has run yet");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const TrainNet& S = p->net[0];
  POLICY_TRY(hipMemcpy(actions, S.a[S.L], (size_t)p->last_rows * p->A * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int lg_distill_rtrain_step_losses(lg_distill_rtrain* p, float* losses, int64_t count, void* stream) {
  POLICY_ENTRY;
  if (!p || !losses) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  if (count < 0 || count > p->last_update_steps) return lg_policy_fail(LG_ERR_INVALID, "count exceeds the steps of the last update");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (count > 0) POLICY_TRY(hipMemcpy(losses, p->seq_loss, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int64_t lg_distill_rtrain_get_carry(lg_distill_rtrain* p, float* h, float* c, int64_t capacity_rows, int32_t running, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  const int64_t N = p->carry_n;
  if (!h || N == 0 || capacity_rows < N) return N;
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const size_t lstride = (size_t)p->max_rows * p->H, row = (size_t)N * p->H;
  for (int l = 0; l < p->ML; ++l) {
    POLICY_TRY(hipMemcpy(h + l * row, (running ? p->cur_h : p->carry_h) + l * lstride, row * sizeof(float), hipMemcpyDefault));
    if (c && p->carry_c) POLICY_TRY(hipMemcpy(c + l * row, (running ? p->cur_c : p->carry_c) + l * lstride, row * sizeof(float), hipMemcpyDefault));
  }
  return N;
}

int lg_distill_rtrain_set_carry(lg_distill_rtrain* p, const float* h, const float* c, int64_t N, void* stream) {
  POLICY_ENTRY;
  if (!p || !h) return lg_policy_fail(LG_ERR_INVALID, "null trainer or state");
  if (p->carry_c && !c) return lg_policy_fail(LG_ERR_INVALID, "an LSTM needs its cell state");
  if (N < 1 || N > p->max_rows) return lg_policy_fail(LG_ERR_INVALID, "N < 1 or N > max_rows of the trainer");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const size_t lstride = (size_t)p->max_rows * p->H, row = (size_t)N * p->H;
  for (int l = 0; l < p->ML; ++l) {
    POLICY_TRY(hipMemcpy(p->carry_h + l * lstride, h + l * row, row * sizeof(float), hipMemcpyDefault));
    POLICY_TRY(hipMemcpy(p->cur_h + l * lstride, h + l * row, row * sizeof(float), hipMemcpyDefault));
    if (p->carry_c) {
      POLICY_TRY(hipMemcpy(p->carry_c + l * lstride, c + l * row, row * sizeof(float), hipMemcpyDefault));
      POLICY_TRY(hipMemcpy(p->cur_c + l * lstride, c + l * row, row * sizeof(float), hipMemcpyDefault));
    }
  }
  p->carry_n = N;
  return LG_OK;
}

int lg_distill_rtrain_reset_carry(lg_distill_rtrain* p, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  p->carry_n = 0;
  return LG_OK;
}

int lg_distill_rtrain_get_state(lg_distill_rtrain* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  DeviceScope ds_(p->device);
  return train_core_get_state(p, params, exp_avg, exp_avg_sq, step, lr, (hipStream_t)stream);
}

int lg_distill_rtrain_get_parameters(lg_distill_rtrain* p, float* params, void* stream) {
  POLICY_ENTRY;
  if (!p || !params) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  return lg_distill_rtrain_get_state(p, params, nullptr, nullptr, nullptr, nullptr, stream);
}

int lg_distill_rtrain_set_state(lg_distill_rtrain* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  POLICY_ENTRY;
  if (!p || !params || !exp_avg || !exp_avg_sq) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  if (step < 0 || !(lr > 0.0)) return lg_policy_fail(LG_ERR_INVALID, "step < 0 or learning rate <= 0");
  DeviceScope ds_(p->device);
  int rc = train_core_set_state(p, params, exp_avg, exp_avg_sq, step, lr, (hipStream_t)stream);
  if (rc == LG_OK) rc = rdistill_retile(p, (hipStream_t)stream);
  if (rc != LG_OK) return rc;
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  return LG_OK;
}

int lg_distill_rtrain_set_learning_rate(lg_distill_rtrain* p, double lr, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!(lr > 0.0)) return lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0");
  DeviceScope ds_(p->device);
  return train_core_set_learning_rate(p, lr, (hipStream_t)stream);
}

}  // extern "C"
