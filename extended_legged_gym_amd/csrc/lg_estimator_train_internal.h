// lg_estimator_train_internal.h -- what the two translation units of the estimator's trainer share: the trainer itself (lg_estimator_train.hip owns
// the fp32 path, the create body and every lg_estimator_train_* entry point) and the state of the bf16 encoder path (lg_estimator_train_bf16.hip:
// its kernels, its workspaces and the lg_estimator_bf16train_* entry points).  A trainer with b16 != NULL trains an LG_PREC_BF16 encoder: est_steps
// then runs est16_forward in place of enc_forward_saved, est16_backward in place of the fp32 pool / convolution backward, and est16_retile in place
// of est_conv_retile_kernel; everything behind the encoder is the one path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lg_device.h"
#include "lg_estimator_internal.h"
#include "lg_train_internal.h"
#include "lg_train_recurrent_internal.h"
#include "lg_train_sequence_internal.h"
#include "../../include/lgestimator_train.h"

#define EST_DENSE_EXTRA 3           // depth_encoder.10, depth_encoder.12, combination_mlp.0

// the derivative of the encoder's activation from its OUTPUT: the one formula of both translation units
LG_DEV float est_act_grad(float y, int act) {
  switch (act) {
    case LG_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case LG_ACT_TANH: return 1.f - y * y;
    default: return y > 0.f ? 1.f : y + 1.f;                // ELU
  }
}

struct DgradLayer {
  int Hin, Win, Cin, Hout, Wout, Cout, sh, pad, act;       // sh = stride - 1 (stride 1 | 2): t is a multiple of the stride iff (t & sh) == 0, t / stride = t >> sh
  int py, px, Hc, Wc;                                       // the rows of this launch: input pixels (py + (sh + 1) cy, px + (sh + 1) cx), cy < Hc, cx < Wc
  int nkb, nkb_w;                                           // this launch's K rounded up to 64, / 16; k-blocks per chunk of the weight image
  const float* wt;                                          // [16-column chunk of ci][k / 16][lane][4], k = (ky, kx, co) over ALL taps
  const int32_t* ktab;                                      // [16 nkb]: (ky << 26) | (kx << 22) | co of this launch's k, -1 beyond its K
  const int32_t* wblk;                                      // [nkb]: the k-block of the weight image that holds this launch's k-block
};

struct ConvRetile;
struct Est16;                                  // lg_estimator_train_bf16.hip

struct lg_estimator_train : SeqCore {
  lg_conv_encoder* enc = nullptr; lg_mlp* combine = nullptr; lg_mlp* decoder = nullptr;
  TrainMem tm;                                 // the memory, its workspaces and carried state (lg_train_recurrent_internal.h)
  int F = 0, P_in = 0, cat_w = 0, Fc = 0, act = 0;
  int nd = 0;                                  // dense segments [0, nd): decoder, depth_encoder.10 / .12, combination_mlp.0, the memory's; then conv 1-4
  int seg_l10 = 0;                             // the segment of depth_encoder.10; depth_encoder.12 is the next one
  int64_t map_floats[4] = {0, 0, 0, 0};
  float* map[4] = {nullptr, nullptr, nullptr, nullptr};
  float *pool = nullptr, *y5 = nullptr, *cat = nullptr, *comb = nullptr;
  float *dA = nullptr, *dB = nullptr, *dpool = nullptr, *d5 = nullptr, *d6 = nullptr, *dcomb = nullptr;
  DgradLayer dg_comb, dg_l12, dg_l10, dg_conv[4][4];       // dg_conv[l][parity class]: conv l + 1 (index 0 unused); a stride-1 layer has class 0 only (Hc == 0: no launch)
  ConvRetile* d_cretile = nullptr; int64_t cretile_big = 0;
  Est16* b16 = nullptr;                        // the bf16 encoder path's state; NULL: an fp32 trainer
  // the last group's rows, for lg_estimator_bf16train_backward_stage (set for a bf16 trainer only)
  const float* last_depth = nullptr; int64_t last_N = 0, last_T = 0, last_t0 = 0;
};

// ---- lg_estimator_train.hip
// the body of lg_estimator_train_create and lg_estimator_bf16train_create (which check the encoder's precision themselves)
lg_estimator_train* est_train_create(lg_conv_encoder* enc, lg_mlp* combine, lg_rnn* mem, lg_mlp* decoder, const lg_estimator_train_params* q, double learning_rate,
                                     int64_t max_rows, bool bf16);
void est_launch_dgrad(const DgradLayer& L, const float* D, int64_t d_estride, int64_t n, const float* ysrc, int64_t y_estride, float* out, int64_t out_estride,
                      hipStream_t st);

// ---- lg_estimator_train_bf16.hip
int32_t est16_slab_rows();
// the bf16 workspaces, images and tables of p (p->map_floats, p->seg[p->nd + l].woff / boff and p->seg_l10 stand); bw10 / bw12: the fp32 transposed
// images of the two linear layers, which est16_retile fills with R(W).  false + message on failure.
bool est16_setup(lg_estimator_train* p, float* bw10, float* bw12);
void est16_free(lg_estimator_train* p);
// stages 1-7 of the bf16 encoder on rows [at, at + n) of the group: the bf16 maps, the fp32 expansions of the pooled and linear-1 rows, the features
// into the cat rows
int est16_forward(lg_estimator_train* p, const float* depth, int64_t depth_stride, int64_t n, int64_t at, hipStream_t st);
// from dpool: the pooling and conv 4 .. conv 1 backwards; cslabs[l]: the slabs of conv l + 1's weight gradient
void est16_backward(lg_estimator_train* p, const float* depth, int64_t n, int64_t N, int64_t T, int64_t t0, int* cslabs, hipStream_t st);
void est16_retile(lg_estimator_train* p, hipStream_t st);
