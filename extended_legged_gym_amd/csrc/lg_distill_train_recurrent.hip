// lg_distill_train_recurrent.hip — Distillation.update (include/lgdistill_recurrent.h) for the recurrent student: a trainer over the student's memory
// (lg_rnn) and MLP (lg_mlp).  A group of G steps is one batch of G * N rows, step-major.  Reused as they are: the memory's forward with saved gates /
// backward step / rows x transposed tiling / retile (lg_train_recurrent_internal.h), the MLP's forward with saved activations, backward data pass,
// slab weight gradients and reduction (lg_train_internal.h), the row index, the behaviour loss, the state mask after a group (Memory.reset(dones)) and
// the update's loop (lg_train_sequence_internal.h).  New here:
//
//   rdistill_norm_kernel       TWO norms from the reduction's block sums, in block order: over the student's segments (the one the clip uses) and over
//                              the memory's; the clip coefficient from the first alone; the step count and Adam's bias corrections.
//   rdistill_adam_kernel       ppo_adam_kernel's arithmetic, with the clip coefficient applied to the first nclip segments only (student.*): the
//                              gradients of memory_s.* enter Adam as they are.  The same lane rewrites the element in the MLP's forward tiling and in
//                              the transposed tilings; the memory's forward images are rnn_retile_kernel's.
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
#include "lg_train_sequence_internal.h"
#include "../../include/lgdistill_recurrent.h"

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

// ------------------------------------------------------------------------------------------------------------------------ host side
struct lg_distill_rtrain : SeqCore {
  lg_mlp* student = nullptr;
  TrainMem tm;                                 // the student's memory, its workspaces and carried state (lg_train_recurrent_internal.h)
  int nstudent = 0;                            // segments [0, nstudent): student.*, the ones the clip covers; then weight_ih, weight_hh per memory layer
  int64_t student_floats = 0;
  RDistillScalars* rs = nullptr;
};

static TrainMem* rdistill_mem(lg_distill_rtrain* p) { return p ? &p->tm : nullptr; }

// the masters -> the memory's forward images (the MLP's and every transposed tiling are the Adam kernel's / train_core_retile's)
static int rdistill_retile(TrainCore* c, hipStream_t st) { return mem_retile(&static_cast<lg_distill_rtrain*>(c)->tm, c->theta, st); }

static int rdistill_check_call(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, const lg_distill_train_hyper* h) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!obs || !tgt || !dones || !h) return lg_policy_fail(LG_ERR_INVALID, "null observations, targets, dones or hyper-parameters");
  if (T < 1 || N < 1) return lg_policy_fail(LG_ERR_INVALID, "T < 1 or N < 1");
  if (h->loss_type != LG_LOSS_MSE && h->loss_type != LG_LOSS_HUBER) return lg_policy_fail(LG_ERR_INVALID, "unknown loss type (mse | huber)");
  return mem_check_rows(&p->tm, N);
}

// steps [first, first + nsteps) of the sequence as one batch; train: an optimiser step, else forward and loss only.  seq_loss: where the update keeps
// these steps' losses, or NULL (a group call: the losses go to group_loss either way, so last_steps counts a standalone forward-only group too; the
// update's forward-only remainder leaves both alone).
static int rdistill_steps(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, int64_t first, int64_t nsteps,
                          const lg_distill_train_hyper* h, bool train, float* seq_loss, hipStream_t st) {
  const int64_t n = nsteps * N, t0 = first % T;
  TrainMem* M = &p->tm;
  const MemSpan W{T, N, t0, nsteps, dones};
  int rc = mem_open_carry(M, N, st);
  if (rc != LG_OK) return rc;
  p->last_rows = n;
  if (train || !seq_loss) p->last_steps = nsteps;
  mem_forward(M, W, obs, true, st);
  // ---- the student on the memory's outputs, the losses
  const TrainNet& Sn = p->net[0];
  const float* top = M->layer[M->ML - 1].hnew;
  train_launch_forward(p, top, top, nullptr, n, st);
  seq_launch_loss(p, Sn.a[Sn.L], tgt, N, T, t0, nsteps, h->loss_type, train ? Sn.d[Sn.L - 1] : (float*)nullptr, train || !seq_loss ? p->group_loss : (float*)nullptr,
                  seq_loss, train ? 1 : 0, st);
  if (train) {
    // ---- the student backwards and dL/d(its input); then backwards through time: nothing is propagated into the observations
    train_launch_backward(p, n, st);
    mem_top_matmul(M, Sn, n, st);
    mem_backward(M, W, nullptr, st);
    // ---- every weight gradient in one slab pass (weight_ih of layer 0 gathers its observation rows), the reduction, the two norms, Adam, the images
    seq_launch_rows(p->rows, n, N, T, t0, st);
    train_launch_wgrad_range(p, 0, p->nseg, obs, obs, p->rows, n, st);
    train_launch_reduce_range(p, 0, p->nseg, (int)((n + WGRAD_SLAB - 1) / WGRAD_SLAB), st);
    hipLaunchKernelGGL(rdistill_norm_kernel, dim3(1), dim3(256), 0, st, (const float*)p->norm_part, p->red_blocks * p->nstudent, p->red_blocks * p->nseg, h->max_grad_norm,
                       h->max_grad_norm > 0.f ? 1 : 0, p->sc, p->rs);
    hipLaunchKernelGGL(rdistill_adam_kernel, dim3((unsigned)((p->big + 255) / 256), p->nseg), dim3(256), 0, st, (const TrainSeg*)p->d_seg, p->nstudent, p->theta, p->m,
                       p->v, (const float*)p->G, (const TrainScalars*)p->sc);
    if ((rc = mem_retile(M, p->theta, st)) != LG_OK) return rc;
  }
  // ---- the running state: the memory after the last step, its dones applied
  if ((rc = mem_keep_running(M, W, st)) != LG_OK) return rc;
  seq_launch_mask_rows(M->cur_h, M->cur_c, dones + ((t0 + nsteps - 1) % T) * N, N, M->H, M->max_rows * M->H, M->ML, st);
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
  if (mlp_is_wide(student)) {
    lg_policy_fail(LG_ERR_UNSUPPORTED, "the student's first layer takes " + std::to_string(student->h.dims[0]) + " inputs: it reads the memory's hidden row of at most " +
                                           std::to_string(MLP_MAXW) + " columns");
    return nullptr;
  }
  if (mem->wide) {
    lg_policy_fail(LG_ERR_UNSUPPORTED, "the memory is a wide one (lg_rnn_create_wide, " + std::to_string(mem->input) + " inputs): this trainer takes memories of at most " +
                                           std::to_string(RNN_XMAX) + " inputs (lg_ppo_recurrent_create trains a wide memory)");
    return nullptr;
  }
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
  p->student = student; p->device = student->device; p->max_rows = max_rows;
  p->retile_own = rdistill_retile;
  TrainMem* M = &p->tm;
  bool ok = true;
  auto alloc = [&](size_t floats, bool zero) -> float* { float* d = ok ? (float*)train_alloc(p, floats * sizeof(float), zero) : nullptr; if (!d) ok = false; return d; };
  ok = mem_alloc(p, M, mem);
  const int K = M->Gates * H, nbk = (K + 15) / 16;
  // ---- segments: the student's (net 0, at the head of the flat vector), then weight_ih / weight_hh of every memory layer.  Layer ids behind the
  // student's index the host tables.
  int64_t off = 0;
  ok = ok && train_core_add_net(p, student, &off);
  p->nstudent = p->nseg; p->student_floats = off;
  enum { ID_MEM = LG_MLP_MAX_LAYERS, ID_COUNT = ID_MEM + 2 * RNN_MAX_LAYERS };
  const float* wtab[ID_COUNT] = {}; const float* btab[ID_COUNT] = {};
  for (int l = 0; l < Ls; ++l) { wtab[l] = q->student_weights[l]; btab[l] = q->student_biases[l]; }
  for (int l = 0; l < ML && ok; ++l) {
    const MemLayer& Y = M->layer[l];
    // weight_ih of layer 0 reads the gathered observation rows (Ain NULL); the flat order of a layer is weight_ih, weight_hh, bias_ih, bias_hh
    TrainSeg& Si = train_core_add_seg(p, 0, ID_MEM + 2 * l, K, l == 0 ? M->I : H, Y.Dih, l == 0 ? nullptr : M->layer[l - 1].hnew, nullptr, nullptr, 0, Y.wtx, nbk, &ok);
    TrainSeg& Sh = train_core_add_seg(p, 0, ID_MEM + 2 * l + 1, K, H, Y.Dhh, Y.hin, nullptr, nullptr, 0, Y.wth, nbk, &ok);
    wtab[ID_MEM + 2 * l] = q->memory_w_ih[l]; btab[ID_MEM + 2 * l] = q->memory_b_ih[l];
    wtab[ID_MEM + 2 * l + 1] = q->memory_w_hh[l]; btab[ID_MEM + 2 * l + 1] = q->memory_b_hh[l];
    mem_place_layer(M, l, Si, Sh, &off);
  }
  // the student's first layer reads the top layer's h' (dense, step-major) and propagates into it: a transposed tiling for layer 0 too
  if (ok) {
    TrainNet& Nn = p->net[0];
    float* bw0 = alloc((size_t)Nn.bnch[0] * (Nn.bkpad[0] / 16) * 256, true);
    Nn.bw[0] = bw0; p->seg[0].bw = bw0; p->seg[0].Ain = M->layer[ML - 1].hnew;
  }
  ok = ok && seq_alloc(p, max_rows, student->h.dims[Ls], true);
  p->rs = (RDistillScalars*)alloc(sizeof(RDistillScalars) / sizeof(float), true);
  ok = ok && mem_upload_retile(p, M);
  const float* const* ws[1] = {wtab};
  const float* const* bs[1] = {btab};
  if (!ok || train_core_finish(p, off, ws, bs, nullptr, learning_rate) != LG_OK || rdistill_retile(p, nullptr) != LG_OK || hipDeviceSynchronize() != hipSuccess) {
    lg_distill_rtrain_destroy(p);
    return nullptr;
  }
  return p;
}

int lg_distill_rtrain_group(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, int64_t first_step, int64_t num_steps,
                            int32_t train, const lg_distill_train_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  int rc = rdistill_check_call(p, obs, tgt, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  if ((rc = seq_check_group(p, N, first_step, num_steps)) != LG_OK) return rc;
  DeviceScope ds_(p->device);
  return rdistill_steps(p, obs, tgt, dones, T, N, first_step, num_steps, hyper, train != 0, nullptr, (hipStream_t)stream);
}

int lg_distill_rtrain_update(lg_distill_rtrain* p, const float* obs, const float* tgt, const float* dones, int64_t T, int64_t N, int32_t E, int32_t G,
                             const lg_distill_train_hyper* hyper, lg_distill_rtrain_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = rdistill_check_call(p, obs, tgt, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  return seq_update(p, T, N, E, G, [&](int64_t first, int64_t nsteps, bool train, float* seq_loss, hipStream_t st) {
    return rdistill_steps(p, obs, tgt, dones, T, N, first, nsteps, hyper, train, seq_loss, st); }, &p->tm, stats, &p->rs->memory_norm, stream);
}

int64_t lg_distill_rtrain_parameter_count(lg_distill_rtrain* p) {
  POLICY_ENTRY;
  return train_api_parameter_count(p);
}

int64_t lg_distill_rtrain_student_parameter_count(lg_distill_rtrain* p) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  return p->student_floats;
}

int64_t lg_distill_rtrain_workspace_bytes(lg_distill_rtrain* p) {
  POLICY_ENTRY;
  return train_api_workspace_bytes(p);
}

int lg_distill_rtrain_gradients(lg_distill_rtrain* p, float* g, float* norms, float* losses, int64_t capacity, void* stream) {
  POLICY_ENTRY;
  const int rc = train_api_group_gradients(p, g, norms, losses, capacity, stream);
  if (rc != LG_OK || !norms) return rc;
  DeviceScope ds_(p->device);
  POLICY_TRY(hipMemcpy(norms + 1, &p->rs->memory_norm, sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int lg_distill_rtrain_forward_outputs(lg_distill_rtrain* p, float* actions, void* stream) {
  POLICY_ENTRY;
  return seq_forward_outputs(p, actions, stream);
}

int lg_distill_rtrain_step_losses(lg_distill_rtrain* p, float* losses, int64_t count, void* stream) {
  POLICY_ENTRY;
  return train_api_step_losses(p, losses, count, stream);
}

// the caller's h / c may be device tensors (hipMemcpyDefault)
int64_t lg_distill_rtrain_get_carry(lg_distill_rtrain* p, float* h, float* c, int64_t capacity_rows, int32_t running, void* stream) {
  POLICY_ENTRY;
  return mem_get_carry(rdistill_mem(p), h, c, capacity_rows, running, hipMemcpyDefault, stream);
}

int lg_distill_rtrain_set_carry(lg_distill_rtrain* p, const float* h, const float* c, int64_t N, void* stream) {
  POLICY_ENTRY;
  return mem_set_carry(rdistill_mem(p), h, c, N, hipMemcpyDefault, stream);
}

int lg_distill_rtrain_reset_carry(lg_distill_rtrain* p, void* stream) {
  POLICY_ENTRY;
  return mem_reset_carry(rdistill_mem(p));
}

int lg_distill_rtrain_get_state(lg_distill_rtrain* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  POLICY_ENTRY;
  return train_api_get_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_distill_rtrain_get_parameters(lg_distill_rtrain* p, float* params, void* stream) {
  POLICY_ENTRY;
  return train_api_get_parameters(p, params, stream);
}

int lg_distill_rtrain_set_state(lg_distill_rtrain* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_distill_rtrain_set_learning_rate(lg_distill_rtrain* p, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_learning_rate(p, lr, stream);
}

}  // extern "C"
