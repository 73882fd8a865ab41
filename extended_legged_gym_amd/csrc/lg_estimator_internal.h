// lg_estimator_internal.h -- what the estimator's trainer (lg_estimator_train.hip) shares with lg_estimator.hip beyond the C ABI: the encoder handle
// and its layer descriptions (the trainer rewrites the device images in place), and the fp32 launch list onto maps the caller owns.  The kernels
// themselves live in lg_estimator.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "lg_policy_internal.h"

#define CONV_ROWS 64         // rows (env, pixel) per workgroup
#define CONV_COLS 64         // output channels per workgroup (grid.y walks the groups)
#define CONV_THREADS 256     // four waves, one 16-row tile each
#define CONV_KC 64           // k per staged chunk (four blocks of 16)
#define ENC_LAYERS 6         // conv 0 2 4 6, linear 10 12 of the nn.Sequential
#define ENC_MAX_HW 128
#define ENC_MAX_OUT 512

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ConvLayerDev {
  int Hin, Win, Cin, Hout, Wout, Cout, stride, pad, act;
  int nkb;                 // K rounded up to 64, / 16
  const float* w;          // tiled [chunk][k / 16][lane][4], Cout rounded up to 64
  const uint16_t* w16;     // bf16 mode instead of w: tiled [chunk][k / 32][lane][8] (lg_conv_tile_weights_bf16); nkb and ktab are then those of enc_bf16_gemm_kernel
  const float* b;          // bias, zero-padded to the same width
  const int32_t* ktab;     // [16 nkb]: (ky << 26) | (kx << 22) | offset of tap k from the patch's first pixel, -1 beyond K
};

struct lg_conv_encoder {
  int device = 0, H = 0, W = 0, out_dim = 0, act = 0, prec = LG_PREC_F32;
  ConvLayerDev layer[ENC_LAYERS];
  int Hp = 0, Wp = 0;                      // the map the pooling reads
  size_t floats_a = 0, floats_b = 0;       // per env: workspace A holds the maps of layers 0, 2 and the pooled row, B those of 1, 3 and the first linear (bf16 mode: elements of 2 bytes)
  int64_t cap = 0;                         // envs the workspaces hold
  float *ws_a = nullptr, *ws_b = nullptr;
  float *cat = nullptr, *comb = nullptr, *memo = nullptr;   // lg_estimator_step: (cap, cat_w), (cap, comb_w), (cap, mem_w)
  int64_t step_cap = 0; int cat_w = 0, comb_w = 0, mem_w = 0;
  std::vector<void*> allocs;
};

static const int kConvShape[4][5] = {{1, 32, 5, 2, 2}, {32, 64, 3, 2, 1}, {64, 128, 3, 2, 1}, {128, 64, 3, 1, 1}};   // C_in, C_out, k, stride, pad

// stage k = 1..7 (conv 1-4, pool + flatten, linear 1, linear 2) of the fp32 encoder on n images, written to maps[k - 1] with rows strides[k - 1] floats
// apart (conv maps (env, y, x, channel)); the kernels and grids of lg_conv_encoder_forward
int enc_forward_saved(lg_conv_encoder* e, const float* depth, int64_t depth_stride, int64_t n, float* const* maps, const int64_t* strides, hipStream_t st);
// the same stages of an LG_PREC_BF16 encoder: maps[0 .. 5] bf16 (strides in elements), maps[6] the fp32 features; the kernels and grids of its
// lg_conv_encoder_forward
int enc_forward_saved_bf16(lg_conv_encoder* e, const float* depth, int64_t depth_stride, int64_t n, void* const* maps, const int64_t* strides, hipStream_t st);
// columns [col0, col0 + P) of the (n, stride) rows = proprio (n, P)
void enc_launch_cat(const float* proprio, int64_t n, int P, float* dst, int stride, int col0, hipStream_t st);
