// lg_estimator.hip — gfx950 kernels of the terrain estimator (include/lgpolicy.h, section "terrain estimator"): the depth-image CNN encoder of
// rsl_rl's TerrainEstimator (modules/terrain_estimator.py:80-109) as implicit GEMMs on the fp32 matrix cores, and the estimator's single step
// (encoder -> cat with the base velocities -> Linear + act -> memory -> decoder, :162-198) on top of lg_mlp_forward / lg_rnn_step.
//
// One kernel serves the four convolutions and the two linear layers.  A layer is the product  rows x K x C_out  with
//     rows = (env, output pixel) over ALL envs of the call -- a 64-row tile spans envs, so the 28-pixel maps of conv3 / conv4 fill their
//            tiles and a weight fragment is used by every env of the tile;
//     K    = kh * kw * C_in, ordered (ky, kx, ci) with ci fastest, over activations held (env, y, x, channel): 16 successive k of one row are
//            64 contiguous bytes for C_in >= 16;
// (a linear layer is the 1 x 1 convolution of a 1 x 1 image).  Workgroup = 4 waves = 64 rows x 64 output channels; wave w owns rows 16 w .. 16 w + 15
// and four accumulators (one per 16-channel chunk).  K runs in chunks of 64: all 256 lanes gather the chunk's 64 x 64 patch values (zero outside
// the image and beyond K; the per-k offset and tap come from a table built at create time, so the loop has no division) into an LDS image
// [k / 16][row][k % 4][(k / 4) % 4] -- the one of lg_policy.hip: a lane's four successive A operands of v_mfma_f32_16x16x4_f32 are one
// ds_read_b128, 1 KB contiguous per wave -- double-buffered, one barrier per chunk, the next chunk's global loads in flight under the current
// chunk's 64 MFMAs per wave.  Weights are re-tiled once on the host (lg_conv_tile_weights): [16-channel chunk][k / 16][lane][(k / 4) % 4], one
// coalesced 16-byte load per lane and four k-steps.  Exact fp32: each output is one k-ordered fmaf chain, no atomics, no split K -- the same
// input gives the same bits.
//
// Maps go layer by layer through global memory (two ping-pong workspaces owned by the encoder): that one path serves every image size up to the
// limit (at 58 x 87 the first map alone is 163 KB per env, more than a compute unit's LDS), and the maps of a 64-row tile are small enough to stay
// in L2 between layers.  AdaptiveAvgPool2d((4, 4)) + Flatten is a kernel of its own (one lane per output, torch's windows
// [floor(i L / 4), ceil((i + 1) L / 4))), writing torch's channel-major order so the first linear layer reads its weights as torch stores them.
//
// Precision LG_PREC_BF16 (opt-in; the code below the marker "bf16 encoder") runs the same seven stages on v_mfma_f32_16x16x32_bf16: bf16 operands,
// fp32 accumulators, bias and activation in fp32, maps of stages 1-6 kept as bf16 (round to nearest even), features in fp32.  The fp32 kernels and
// their launch list are not touched by it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_estimator_internal.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgstep.h"

LG_DEV float enc_act(float x, int act) {
  switch (act) {
    case LG_ACT_RELU: return fmaxf(x, 0.f);
    case LG_ACT_TANH: return tanhf(x);
    default: return x > 0.f ? x : expm1f(x);        // nn.ELU
  }
}

__global__ __launch_bounds__(CONV_THREADS) void conv_gemm_kernel(ConvLayerDev L, const float* __restrict__ in, int64_t in_estride, int64_t n,
                                                                  float* __restrict__ out, int64_t out_estride) {
  __shared__ __attribute__((aligned(16))) float a_lds[2][CONV_KC * CONV_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = L.Hout * L.Wout;
  const int64_t M = n * HW, row0 = (int64_t)blockIdx.x * CONV_ROWS;
  // gather role: tap kk of the block, rows rb + 16 j
  const int kk = tid & 15, rb = tid >> 4;
  const float* src[4]; int iy0[4], ix0[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t m = row0 + rb + 16 * j;
    if (m < M) {
      const int64_t e = m / HW; const int pix = (int)(m - e * HW), oy = pix / L.Wout, ox = pix - oy * L.Wout;
      iy0[j] = oy * L.stride - L.pad; ix0[j] = ox * L.stride - L.pad;
      src[j] = in + e * in_estride + ((int64_t)iy0[j] * L.Win + ix0[j]) * L.Cin;
    } else { iy0[j] = -(1 << 20); ix0[j] = 0; src[j] = in; }          // every tap out of the image: zeros
  }
  float v[16];
  auto gather = [&](int kb0) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int t = L.ktab[(kb0 + b) * 16 + kk];
      const int ky = (t >> 26) & 15, kx = (t >> 22) & 15, off = t & 0x3fffff;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int iy = iy0[j] + ky, ix = ix0[j] + kx;
        const bool ok = t >= 0 && iy >= 0 && iy < L.Hin && ix >= 0 && ix < L.Win;
        v[b * 4 + j] = ok ? src[j][off] : 0.f;
      }
    }
  };
  const float4* wl = reinterpret_cast<const float4*>(L.w) + (size_t)blockIdx.y * 4 * L.nkb * 64 + lane;
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  gather(0);
  for (int kb0 = 0, it = 0; kb0 < L.nkb; kb0 += 4, ++it) {
    float* buf = a_lds[it & 1];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) buf[((b * CONV_ROWS + rb + 16 * j) * 4 + (kk & 3)) * 4 + (kk >> 2)] = v[b * 4 + j];
    __syncthreads();
    if (kb0 + 4 < L.nkb) gather(kb0 + 4);
    const float4* ap = reinterpret_cast<const float4*>(buf) + (wv * 16 + (lane & 15)) * 4 + (lane >> 4);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float4 a = ap[b * CONV_ROWS * 4];
      float4 w[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = wl[((size_t)c * L.nkb + kb0 + b) * 64];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[c].x, acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[c].y, acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[c].z, acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[c].w, acc[c], 0, 0, 0);
    }
  }
  // epilogue: accumulator entry i of a lane is C[row 4 (lane >> 4) + i][channel lane & 15]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = row0 + wv * 16 + 4 * (lane >> 4) + i;
    if (m >= M) continue;
    const int64_t e = m / HW; const int pix = (int)(m - e * HW);
    float* dst = out + e * out_estride + (int64_t)pix * L.Cout;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = blockIdx.y * CONV_COLS + c * 16 + (lane & 15);
      if (col < L.Cout) dst[col] = enc_act(acc[c][i] + L.b[col], L.act);
    }
  }
}

// AdaptiveAvgPool2d((4, 4)) + Flatten: x (n, H, W, C) -> y (n, C 16), y[e, c 16 + i 4 + j]
__global__ __launch_bounds__(256) void pool_flatten_kernel(const float* __restrict__ x, int64_t n, int H, int W, int C, float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * 16 * C) return;
  const int c = (int)(idx % C); const int64_t t = idx / C; const int ij = (int)(t & 15); const int64_t e = t >> 4;
  const int i = ij >> 2, j = ij & 3;
  const int y0 = (i * H) / 4, y1 = ((i + 1) * H + 3) / 4, x0 = (j * W) / 4, x1 = ((j + 1) * W + 3) / 4;
  float s = 0.f;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) s += x[((e * H + yy) * W + xx) * C + c];
  y[e * 16 * C + c * 16 + ij] = s / (float)((y1 - y0) * (x1 - x0));
}

// columns [col0, col0 + P) of the (n, stride) staging rows = proprio (n, P): the second half of torch.cat
__global__ __launch_bounds__(256) void cat_columns_kernel(const float* __restrict__ src, int64_t n, int P, float* __restrict__ dst, int stride, int col0) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * P) return;
  const int64_t r = idx / P; const int k = (int)(idx - r * P);
  dst[r * stride + col0 + k] = src[idx];
}

// ------------------------------------------------------------------------------------------------------------ bf16 encoder (LG_PREC_BF16)
// The same product rows x K x C_out, the same 64 x 64 workgroup tile and the same accumulator map (entry i of a lane is C[row 4 (lane >> 4) + i]
// [channel lane & 15]) on v_mfma_f32_16x16x32_bf16, whose operands are A[row lane & 15][k = 8 (lane >> 4) + j] and B[k = 8 (lane >> 4) + j]
// [channel lane & 15], j = 0..7.  K runs in steps of 32.  Behind conv 1 every C_in is a multiple of 32 and the maps are bf16 (env, y, x, channel),
// so a k-step lies inside one tap and a lane's eight A values are 16 contiguous, 16-byte aligned bytes of the map: the lane loads its operand
// straight from global memory (zero outside the image), no LDS image, no barrier; the per-step tap and offset come from a table built at create
// time (one entry per k-step, wave uniform).  conv 1 (C_in = 1, K = 25: one k-step, the cost is the gather) reads its eight taps one by one from
// the fp32 image through the per-k table of the fp32 kernel and rounds them to bf16 there.  Weights: lg_conv_tile_weights_bf16, one coalesced
// 16-byte load per lane, chunk and k-step.  The next step's operands are loaded before the current step's MFMAs.  Each output is one
// accumulator over k-steps in ascending order: no atomics, no split K, equal inputs give equal bits.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

LG_DEV void enc_store(float* p, float v) { *p = v; }
LG_DEV void enc_store(__bf16* p, float v) { *p = (__bf16)v; }          // v_cvt_pk_bf16_f32: round to nearest even

// FIRST: `in` is the fp32 image (C_in = 1, ktab per k); else a bf16 map (C_in % 32 == 0, ktab per k-step).  TOut: __bf16 maps, float features.
template <bool FIRST, typename TOut>
__global__ __launch_bounds__(CONV_THREADS) void enc_bf16_gemm_kernel(ConvLayerDev L, const void* __restrict__ in_, int64_t in_estride, int64_t n,
                                                                      TOut* __restrict__ out, int64_t out_estride) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4;
  const int HW = L.Hout * L.Wout, nks = L.nkb;
  const int64_t M = n * HW, row0 = (int64_t)blockIdx.x * CONV_ROWS + wv * 16;
  // operand role: row lane & 15 of the wave's 16, k = 8 g + j of each step
  const int64_t ma = row0 + (lane & 15);
  int iy0 = -(1 << 20), ix0 = 0; int64_t base = 0;          // a row beyond M: every tap out of the image
  if (ma < M) {
    const int64_t e = ma / HW; const int pix = (int)(ma - e * HW), oy = pix / L.Wout, ox = pix - oy * L.Wout;
    iy0 = oy * L.stride - L.pad; ix0 = ox * L.stride - L.pad;
    base = e * in_estride + ((int64_t)iy0 * L.Win + ix0) * L.Cin + (FIRST ? 0 : 8 * g);
  }
  auto load_a = [&](int s) -> bf16x8 {
    bf16x8 a;
    if (FIRST) {
      const float* in = static_cast<const float*>(in_);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = L.ktab[s * 32 + 8 * g + j];
        const int iy = iy0 + ((t >> 26) & 15), ix = ix0 + ((t >> 22) & 15);
        const bool ok = t >= 0 && iy >= 0 && iy < L.Hin && ix >= 0 && ix < L.Win;
        a[j] = (__bf16)(ok ? in[base + (t & 0x3fffff)] : 0.f);
      }
    } else {
      const int t = L.ktab[s];
      const int iy = iy0 + ((t >> 26) & 15), ix = ix0 + ((t >> 22) & 15);
      const bool ok = iy >= 0 && iy < L.Hin && ix >= 0 && ix < L.Win;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = (__bf16)0.f;
      if (ok) a = *reinterpret_cast<const bf16x8*>(static_cast<const __bf16*>(in_) + base + (t & 0x3fffff));
    }
    return a;
  };
  const int nch = min(4, (L.Cout - (int)blockIdx.y * CONV_COLS + 15) / 16);          // chunks of this column group that hold a channel (wave uniform); the rest are zero padding
  const bf16x8* wl = reinterpret_cast<const bf16x8*>(L.w16) + (size_t)blockIdx.y * 4 * nks * 64 + lane;
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 a = load_a(0), w[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) w[c] = wl[(size_t)c * nks * 64];
  for (int s = 0; s < nks; ++s) {
    bf16x8 an = a, wn[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) wn[c] = w[c];
    if (s + 1 < nks) {
      an = load_a(s + 1);
#pragma unroll
      for (int c = 0; c < 4; ++c) wn[c] = wl[((size_t)c * nks + s + 1) * 64];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nch) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w[c], acc[c], 0, 0, 0);
    a = an;
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = wn[c];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = row0 + 4 * g + i;
    if (m >= M) continue;
    const int64_t e = m / HW; const int pix = (int)(m - e * HW);
    TOut* dst = out + e * out_estride + (int64_t)pix * L.Cout;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = blockIdx.y * CONV_COLS + c * 16 + (lane & 15);
      if (col < L.Cout) enc_store(dst + col, enc_act(acc[c][i] + L.b[col], L.act));
    }
  }
}

// pool_flatten_kernel on a bf16 map: the window is averaged in fp32 and the mean rounded to bf16
__global__ __launch_bounds__(256) void enc_bf16_pool_kernel(const __bf16* __restrict__ x, int64_t n, int H, int W, int C, __bf16* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * 16 * C) return;
  const int c = (int)(idx % C); const int64_t t = idx / C; const int ij = (int)(t & 15); const int64_t e = t >> 4;
  const int i = ij >> 2, j = ij & 3;
  const int y0 = (i * H) / 4, y1 = ((i + 1) * H + 3) / 4, x0 = (j * W) / 4, x1 = ((j + 1) * W + 3) / 4;
  float s = 0.f;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) s += (float)x[((e * H + yy) * W + xx) * C + c];
  y[e * 16 * C + c * 16 + ij] = (__bf16)(s / (float)((y1 - y0) * (x1 - x0)));
}

// lg_conv_encoder_forward_stages on a bf16 encoder: the rows of a bf16 stage, expanded exactly
__global__ __launch_bounds__(256) void enc_bf16_expand_kernel(const __bf16* __restrict__ x, int64_t count, float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < count) y[idx] = (float)x[idx];
}

// fp32 -> bf16, round to nearest even (NaN stays a quiet NaN)
static uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static int64_t conv_tiled_count_bf16(int cout, int cin, int kh, int kw) {
  const int64_t K = (int64_t)cin * kh * kw, nks = (K + 31) / 32, nch = ((cout + 63) & ~63) / 16;
  return nch * nks * 64 * 8;
}

static void conv_tile_weights_bf16(int cout, int cin, int kh, int kw, const float* w, uint16_t* tiled) {
  const int K = cin * kh * kw, nks = (K + 31) / 32, nch = ((cout + 63) & ~63) / 16;
  for (int c = 0; c < nch; ++c)
    for (int s = 0; s < nks; ++s)
      for (int ln = 0; ln < 64; ++ln)
        for (int j = 0; j < 8; ++j) {
          const int col = c * 16 + (ln & 15), k = s * 32 + 8 * (ln >> 4) + j;
          uint16_t v = 0;
          if (col < cout && k < K) {
            const int ci = k % cin, tap = k / cin, ky = tap / kw, kx = tap - ky * kw;
            v = bf16_rne(w[(((size_t)col * cin + ci) * kh + ky) * kw + kx]);
          }
          tiled[(((size_t)c * nks + s) * 64 + ln) * 8 + j] = v;
        }
}

static int64_t conv_tiled_count(int cout, int cin, int kh, int kw) {
  const int64_t K = (int64_t)cin * kh * kw, nkb = ((K + 63) & ~(int64_t)63) / 16, nch = ((cout + 63) & ~63) / 16;
  return nch * nkb * 64 * 4;
}

static void conv_tile_weights(int cout, int cin, int kh, int kw, const float* w, float* tiled) {
  const int K = cin * kh * kw, nkb = ((K + 63) & ~63) / 16, nch = ((cout + 63) & ~63) / 16;
  for (int c = 0; c < nch; ++c)
    for (int b = 0; b < nkb; ++b)
      for (int ln = 0; ln < 64; ++ln)
        for (int s = 0; s < 4; ++s) {
          const int col = c * 16 + (ln & 15), k = b * 16 + s * 4 + (ln >> 4);
          float v = 0.f;
          if (col < cout && k < K) {
            const int ci = k % cin, tap = k / cin, ky = tap / kw, kx = tap - ky * kw;
            v = w[(((size_t)col * cin + ci) * kh + ky) * kw + kx];
          }
          tiled[(((size_t)c * nkb + b) * 64 + ln) * 4 + s] = v;
        }
}

static bool enc_grow(float** p, size_t floats) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  return hipMalloc((void**)p, floats * sizeof(float)) == hipSuccess;
}

extern "C" {

int64_t lg_conv_tile_weights(int32_t c_out, int32_t c_in, int32_t kh, int32_t kw, const float* weight, float* tiled) {
  POLICY_ENTRY;
  if (c_out < 1 || c_out > ENC_MAX_OUT || c_in < 1 || c_in > 1024 || kh < 1 || kh > 15 || kw < 1 || kw > 15)
    return lg_policy_fail(LG_ERR_INVALID, "c_out outside 1..512, c_in outside 1..1024 or kh / kw outside 1..15");
  if (tiled) {
    if (!weight) return lg_policy_fail(LG_ERR_INVALID, "null weight");
    conv_tile_weights(c_out, c_in, kh, kw, weight, tiled);
  }
  return conv_tiled_count(c_out, c_in, kh, kw);
}

int64_t lg_conv_tile_weights_bf16(int32_t c_out, int32_t c_in, int32_t kh, int32_t kw, const float* weight, uint16_t* tiled) {
  POLICY_ENTRY;
  if (c_out < 1 || c_out > ENC_MAX_OUT || c_in < 1 || c_in > 1024 || kh < 1 || kh > 15 || kw < 1 || kw > 15)
    return lg_policy_fail(LG_ERR_INVALID, "c_out outside 1..512, c_in outside 1..1024 or kh / kw outside 1..15");
  if (tiled) {
    if (!weight) return lg_policy_fail(LG_ERR_INVALID, "null weight");
    conv_tile_weights_bf16(c_out, c_in, kh, kw, weight, tiled);
  }
  return conv_tiled_count_bf16(c_out, c_in, kh, kw);
}

void lg_conv_encoder_destroy(lg_conv_encoder* e) {
  if (!e) return;
  DeviceScope ds_(e->device);
  for (void* p : e->allocs) (void)hipFree(p);
  for (float* p : {e->ws_a, e->ws_b, e->cat, e->comb, e->memo}) if (p) (void)hipFree(p);
  delete e;
}

lg_conv_encoder* lg_conv_encoder_create_precision(int32_t height, int32_t width, int32_t out_dim, int32_t activation, const float* const* weights,
                                                  const float* const* biases, int device_id, int32_t precision) {
  POLICY_ENTRY;
  if (precision != LG_PREC_F32 && precision != LG_PREC_BF16) { lg_policy_fail(LG_ERR_INVALID, "precision must be LG_PREC_F32 or LG_PREC_BF16"); return nullptr; }
  if (height < 8 || height > ENC_MAX_HW || width < 8 || width > ENC_MAX_HW) { lg_policy_fail(LG_ERR_INVALID, "image size out of range (8..128 per side)"); return nullptr; }
  if (out_dim < 1 || out_dim > ENC_MAX_OUT) { lg_policy_fail(LG_ERR_INVALID, "out_dim out of range (1..512)"); return nullptr; }
  if (activation != LG_ACT_ELU && activation != LG_ACT_RELU && activation != LG_ACT_TANH) { lg_policy_fail(LG_ERR_INVALID, "activation must be elu, relu or tanh"); return nullptr; }
  if (!weights || !biases) { lg_policy_fail(LG_ERR_INVALID, "null weight list"); return nullptr; }
  for (int l = 0; l < ENC_LAYERS; ++l) if (!weights[l] || !biases[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight"); return nullptr; }
  if (!lg_policy_device_ok(device_id)) return nullptr;
  DeviceScope ds_(device_id);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_conv_encoder* e = new lg_conv_encoder();
  e->device = device_id; e->H = height; e->W = width; e->out_dim = out_dim; e->act = activation; e->prec = precision;
  const bool bf16 = precision == LG_PREC_BF16;
  int h = height, w = width;
  size_t map_floats[ENC_LAYERS];
  for (int l = 0; l < ENC_LAYERS; ++l) {
    ConvLayerDev& L = e->layer[l];
    int kh = 1;
    if (l < 4) {
      const int* s = kConvShape[l];
      kh = s[2];
      L.Hin = h; L.Win = w; L.Cin = s[0]; L.Cout = s[1]; L.stride = s[3]; L.pad = s[4];
      L.Hout = (h + 2 * s[4] - s[2]) / s[3] + 1; L.Wout = (w + 2 * s[4] - s[2]) / s[3] + 1;
      h = L.Hout; w = L.Wout;
    } else {
      L.Hin = L.Win = L.Hout = L.Wout = 1; L.stride = 1; L.pad = 0;
      L.Cin = l == 4 ? 64 * 16 : 128; L.Cout = l == 4 ? 128 : out_dim;
    }
    L.act = activation;
    const int K = L.Cin * kh * kh;
    L.nkb = bf16 ? (K + 31) / 32 : ((K + 63) & ~63) / 16;          // bf16: k-steps of 32
    map_floats[l] = (size_t)L.Hout * L.Wout * L.Cout;
    // tw: the tiled weights as 4-byte words (bf16: two values per word)
    std::vector<float> tw((size_t)(bf16 ? conv_tiled_count_bf16(L.Cout, L.Cin, kh, kh) / 2 : conv_tiled_count(L.Cout, L.Cin, kh, kh))), tb((size_t)((L.Cout + 63) & ~63), 0.f);
    if (bf16) conv_tile_weights_bf16(L.Cout, L.Cin, kh, kh, weights[l], reinterpret_cast<uint16_t*>(tw.data()));
    else conv_tile_weights(L.Cout, L.Cin, kh, kh, weights[l], tw.data());
    for (int i = 0; i < L.Cout; ++i) tb[i] = biases[l][i];
    // per k (fp32, and conv 1 of bf16) or per k-step of 32 (bf16 behind conv 1: C_in % 32 == 0, a step lies inside one tap)
    const bool per_step = bf16 && l > 0;
    std::vector<int32_t> kt(per_step ? (size_t)L.nkb : bf16 ? (size_t)L.nkb * 32 : (size_t)L.nkb * 16, -1);
    for (int k = 0; k < K; k += per_step ? 32 : 1) {
      const int ci = k % L.Cin, tap = k / L.Cin, ky = tap / kh, kx = tap - ky * kh;
      kt[per_step ? k / 32 : k] = (ky << 26) | (kx << 22) | ((ky * L.Win + kx) * L.Cin + ci);         // offset < 15 * 128 * 1024 + ... < 2^22 for every supported shape
    }
    const void* dw = lg_policy_upload(tw.data(), tw.size() * 4, e->allocs);
    L.b = dw ? (const float*)lg_policy_upload(tb.data(), tb.size() * 4, e->allocs) : nullptr;
    L.ktab = L.b ? (const int32_t*)lg_policy_upload(kt.data(), kt.size() * 4, e->allocs) : nullptr;
    if (!L.ktab) { lg_conv_encoder_destroy(e); return nullptr; }
    L.w = bf16 ? nullptr : (const float*)dw; L.w16 = bf16 ? (const uint16_t*)dw : nullptr;
  }
  e->Hp = h; e->Wp = w;
  e->floats_a = std::max(std::max(map_floats[0], map_floats[2]), (size_t)1024);
  e->floats_b = std::max(std::max(map_floats[1], map_floats[3]), (size_t)128);
  return e;
}

lg_conv_encoder* lg_conv_encoder_create(int32_t height, int32_t width, int32_t out_dim, int32_t activation, const float* const* weights,
                                        const float* const* biases, int device_id) {
  POLICY_ENTRY;
  return lg_conv_encoder_create_precision(height, width, out_dim, activation, weights, biases, device_id, LG_PREC_F32);
}

int32_t lg_conv_encoder_precision(const lg_conv_encoder* e) {
  POLICY_ENTRY;
  if (!e) return lg_policy_fail(LG_ERR_INVALID, "null encoder");
  return e->prec;
}

static int enc_launch(const ConvLayerDev& L, const float* in, int64_t in_estride, int64_t n, float* out, int64_t out_estride, hipStream_t st) {
  const int64_t tiles = (n * L.Hout * L.Wout + CONV_ROWS - 1) / CONV_ROWS;
  if (tiles > 0x7fffffff) return lg_policy_fail(LG_ERR_UNSUPPORTED, "too many rows for one launch");
  hipLaunchKernelGGL(conv_gemm_kernel, dim3((unsigned)tiles, (unsigned)((L.Cout + CONV_COLS - 1) / CONV_COLS)), dim3(CONV_THREADS), 0, st, L, in, in_estride, n, out,
                     out_estride);
  return LG_OK;
}

// bf16 mode: stage k = 1 reads the fp32 image, stage 7 writes fp32 features, everything between is bf16
static int enc_launch_bf16(const ConvLayerDev& L, int k, const void* in, int64_t in_estride, int64_t n, void* out, int64_t out_estride, hipStream_t st) {
  const int64_t tiles = (n * L.Hout * L.Wout + CONV_ROWS - 1) / CONV_ROWS;
  if (tiles > 0x7fffffff) return lg_policy_fail(LG_ERR_UNSUPPORTED, "too many rows for one launch");
  const dim3 grid((unsigned)tiles, (unsigned)((L.Cout + CONV_COLS - 1) / CONV_COLS)), block(CONV_THREADS);
  if (k == 1) hipLaunchKernelGGL((enc_bf16_gemm_kernel<true, __bf16>), grid, block, 0, st, L, in, in_estride, n, (__bf16*)out, out_estride);
  else if (k == ENC_LAYERS + 1) hipLaunchKernelGGL((enc_bf16_gemm_kernel<false, float>), grid, block, 0, st, L, in, in_estride, n, (float*)out, out_estride);
  else hipLaunchKernelGGL((enc_bf16_gemm_kernel<false, __bf16>), grid, block, 0, st, L, in, in_estride, n, (__bf16*)out, out_estride);
  return LG_OK;
}

// floats of one env's output of stage k = 1..7 (conv 1-4, pool + flatten, linear 1, linear 2), and its map: (H, W, C) of a conv stage, (1, 1, width) else
static int64_t enc_stage_shape(const lg_conv_encoder* e, int k, int* h, int* w, int* c) {
  const ConvLayerDev& L = e->layer[k <= 4 ? k - 1 : k == 5 ? 3 : k - 2];
  *h = k <= 4 ? L.Hout : 1; *w = k <= 4 ? L.Wout : 1; *c = k == 5 ? 16 * L.Cout : L.Cout;
  return (int64_t)*h * *w * *c;
}

// The encoder's launch list, cut after `stages` of its seven stages: stage k reads stage k - 1's rows (the depth images for k = 1) and writes workspace
// A (k odd) or B (k even); the last one, linear 2, writes `features`, rows `feat_stride` floats apart (lg_estimator_step has them written straight into
// the first columns of its cat rows).  *last (if asked for) = where the rows of the last stage run are.
static int enc_forward(lg_conv_encoder* e, const float* depth, int64_t depth_stride, int64_t n, float* features, int64_t feat_stride, hipStream_t st,
                       int stages = ENC_LAYERS + 1, const float** last = nullptr) {
  if (n > e->cap) {          // the workspaces grow to the largest n seen; hipFree waits for the device, so a caller that alternates streams stays safe
    const size_t per = e->prec == LG_PREC_BF16 ? 2 : 1;          // bf16 maps: two elements per float
    if (!enc_grow(&e->ws_a, ((size_t)n * e->floats_a + per - 1) / per) || !enc_grow(&e->ws_b, ((size_t)n * e->floats_b + per - 1) / per)) {
      e->cap = 0; return lg_policy_fail(LG_ERR_HIP, "workspace allocation failed");
    }
    e->cap = n;
  }
  const float* in = depth; int64_t in_stride = depth_stride;
  if (e->prec == LG_PREC_BF16) {          // the same stage list; `in` / `out` hold bf16 between the image and the features
    for (int k = 1; k <= stages; ++k) {
      int h, w, c;
      float* out = k == ENC_LAYERS + 1 ? features : (k & 1) ? e->ws_a : e->ws_b;
      const int64_t out_stride = k == ENC_LAYERS + 1 ? feat_stride : enc_stage_shape(e, k, &h, &w, &c);
      if (k == 5) hipLaunchKernelGGL(enc_bf16_pool_kernel, dim3((unsigned)((n * 1024 + 255) / 256)), dim3(256), 0, st, (const __bf16*)in, n, e->Hp, e->Wp, 64, (__bf16*)out);
      else {
        const int rc = enc_launch_bf16(e->layer[k < 5 ? k - 1 : k - 2], k, in, in_stride, n, out, out_stride, st);
        if (rc != LG_OK) return rc;
      }
      in = out; in_stride = out_stride;
    }
    POLICY_TRY(hipGetLastError());
    if (last) *last = in;
    return LG_OK;
  }
  for (int k = 1; k <= stages; ++k) {
    int h, w, c;
    float* out = k == ENC_LAYERS + 1 ? features : (k & 1) ? e->ws_a : e->ws_b;
    const int64_t out_stride = k == ENC_LAYERS + 1 ? feat_stride : enc_stage_shape(e, k, &h, &w, &c);
    if (k == 5) hipLaunchKernelGGL(pool_flatten_kernel, dim3((unsigned)((n * 1024 + 255) / 256)), dim3(256), 0, st, in, n, e->Hp, e->Wp, 64, out);
    else {
      const int rc = enc_launch(e->layer[k < 5 ? k - 1 : k - 2], in, in_stride, n, out, out_stride, st);
      if (rc != LG_OK) return rc;
    }
    in = out; in_stride = out_stride;
  }
  POLICY_TRY(hipGetLastError());
  if (last) *last = in;
  return LG_OK;
}

int lg_conv_encoder_forward(lg_conv_encoder* e, const float* depth, int64_t depth_stride, int64_t n, float* features, void* stream) {
  POLICY_ENTRY;
  if (!e || !depth || !features) return lg_policy_fail(LG_ERR_INVALID, "null argument");
  if (n <= 0) return lg_policy_fail(LG_ERR_INVALID, "n must be positive");
  if (depth_stride < (int64_t)e->H * e->W) return lg_policy_fail(LG_ERR_INVALID, "depth_stride is smaller than one image");
  DeviceScope ds_(e->device);
  return enc_forward(e, depth, depth_stride, n, features, e->out_dim, (hipStream_t)stream);
}

int64_t lg_conv_encoder_stage_shape(const lg_conv_encoder* e, int32_t stage, int32_t* h, int32_t* w, int32_t* c) {
  POLICY_ENTRY;
  if (!e || stage < 1 || stage > ENC_LAYERS + 1) return lg_policy_fail(LG_ERR_INVALID, "null encoder or stage outside 1..7");
  int hh, ww, cc;
  const int64_t count = enc_stage_shape(e, stage, &hh, &ww, &cc);
  if (h) *h = hh;
  if (w) *w = ww;
  if (c) *c = cc;
  return count;
}

int lg_conv_encoder_forward_stages(lg_conv_encoder* e, const float* depth, int64_t depth_stride, int64_t n, int32_t stages, float* out, void* stream) {
  POLICY_ENTRY;
  if (!e || !depth || !out) return lg_policy_fail(LG_ERR_INVALID, "null argument");
  if (n <= 0) return lg_policy_fail(LG_ERR_INVALID, "n must be positive");
  if (depth_stride < (int64_t)e->H * e->W) return lg_policy_fail(LG_ERR_INVALID, "depth_stride is smaller than one image");
  if (stages < 1 || stages > ENC_LAYERS + 1) return lg_policy_fail(LG_ERR_INVALID, "stages must be 1..7");
  DeviceScope ds_(e->device);
  const float* last = nullptr;
  const int rc = enc_forward(e, depth, depth_stride, n, out, e->out_dim, (hipStream_t)stream, stages, &last);
  if (rc != LG_OK || last == out) return rc;
  int h, w, c;
  if (e->prec == LG_PREC_BF16) {
    const int64_t count = n * enc_stage_shape(e, stages, &h, &w, &c);
    hipLaunchKernelGGL(enc_bf16_expand_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)last, count, out);
    POLICY_TRY(hipGetLastError());
    return LG_OK;
  }
  POLICY_TRY(hipMemcpyAsync(out, last, (size_t)n * enc_stage_shape(e, stages, &h, &w, &c) * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LG_OK;
}

// a stage of lg_estimator_step failed: its name goes in front of the reason the stage left
static int stage_fail(int rc, const char* stage) {
  const std::string why = lg_mlp_last_error(nullptr);
  const size_t at = why.find(": ");
  return lg_policy_fail(rc, std::string(stage) + ": " + (at == std::string::npos ? why : why.substr(at + 2)));
}

int lg_estimator_step(lg_conv_encoder* e, lg_mlp* combine, lg_rnn* mem, lg_mlp* decoder, const float* depth, int64_t depth_stride, const float* proprio,
                      int64_t n, float* h, float* c, const float* reset, float* predictions, void* stream) {
  POLICY_ENTRY;
  if (!e || !combine || !mem || !decoder || !depth || !h || !predictions) return lg_policy_fail(LG_ERR_INVALID, "null argument");
  if (n <= 0) return lg_policy_fail(LG_ERR_INVALID, "n must be positive");
  if (depth_stride < (int64_t)e->H * e->W) return lg_policy_fail(LG_ERR_INVALID, "depth_stride is smaller than one image");
  int cl, cin, cout, cdev, rtype, rin, rhid, rdev, dl, din, dout, ddev;
  lg_mlp_widths(combine, &cl, &cin, &cout, &cdev);
  lg_rnn_widths(mem, &rtype, &rin, &rhid, &rdev);
  lg_mlp_widths(decoder, &dl, &din, &dout, &ddev);
  if (cin > MLP_MAXW) return lg_policy_fail(LG_ERR_UNSUPPORTED, "combine takes " + std::to_string(cin) + " inputs: the estimator's stages are at most " + std::to_string(MLP_MAXW) + " wide (a handle of lg_mlp_create_wide is refused)");
  if (mem->wide) return lg_policy_fail(LG_ERR_UNSUPPORTED, "the memory is a wide one (lg_rnn_create_wide, " + std::to_string(rin) + " inputs): the estimator's memory takes at most " + std::to_string(RNN_XMAX) + " inputs");
  const int P = cin - e->out_dim;
  if (cl != 1 || P < 0 || cout != rin || din != rhid)
    return lg_policy_fail(LG_ERR_INVALID, "stage widths do not chain (combine: one layer of encoder out_dim + proprio inputs; its outputs = the memory's input; decoder input = the memory's hidden width)");
  if (P > 0 && !proprio) return lg_policy_fail(LG_ERR_INVALID, "null proprio");
  if (rtype == LG_RNN_LSTM && !c) return lg_policy_fail(LG_ERR_INVALID, "an LSTM needs its cell state");
  if (cdev != e->device || rdev != e->device || ddev != e->device) return lg_policy_fail(LG_ERR_INVALID, "the stages live on different devices");
  DeviceScope ds_(e->device);
  if (n > e->step_cap || cin != e->cat_w || cout != e->comb_w || rhid != e->mem_w) {
    if (!enc_grow(&e->cat, (size_t)n * cin) || !enc_grow(&e->comb, (size_t)n * cout) || !enc_grow(&e->memo, (size_t)n * rhid)) {
      e->step_cap = 0; return lg_policy_fail(LG_ERR_HIP, "workspace allocation failed");
    }
    e->step_cap = n; e->cat_w = cin; e->comb_w = cout; e->mem_w = rhid;
  }
  hipStream_t st = (hipStream_t)stream;
  int rc = enc_forward(e, depth, depth_stride, n, e->cat, cin, st);
  if (rc != LG_OK) return rc;
  if (P > 0) hipLaunchKernelGGL(cat_columns_kernel, dim3((unsigned)((n * P + 255) / 256)), dim3(256), 0, st, proprio, n, P, e->cat, cin, e->out_dim);
  POLICY_TRY(hipGetLastError());
  if ((rc = lg_mlp_forward(combine, e->cat, n, e->comb, stream)) != LG_OK) return stage_fail(rc, "combine");
  if ((rc = lg_rnn_step(mem, e->comb, n, h, c, reset, e->memo, stream)) != LG_OK) return stage_fail(rc, "memory");
  if ((rc = lg_mlp_forward(decoder, e->memo, n, predictions, stream)) != LG_OK) return stage_fail(rc, "decoder");
  return LG_OK;
}

}  // extern "C"

// lg_estimator_internal.h: the fp32 launch list onto the caller's maps -- the same kernels, the same grids, so stage k's rows are those of
// lg_conv_encoder_forward_stages bit for bit.  maps[k - 1] / strides[k - 1]: where the rows of stage k go and how far apart they are.
int enc_forward_saved(lg_conv_encoder* e, const float* depth, int64_t depth_stride, int64_t n, float* const* maps, const int64_t* strides, hipStream_t st) {
  const float* in = depth; int64_t in_stride = depth_stride;
  for (int k = 1; k <= ENC_LAYERS + 1; ++k) {
    if (k == 5) hipLaunchKernelGGL(pool_flatten_kernel, dim3((unsigned)((n * 1024 + 255) / 256)), dim3(256), 0, st, in, n, e->Hp, e->Wp, 64, maps[k - 1]);
    else {
      const int rc = enc_launch(e->layer[k < 5 ? k - 1 : k - 2], in, in_stride, n, maps[k - 1], strides[k - 1], st);
      if (rc != LG_OK) return rc;
    }
    in = maps[k - 1]; in_stride = strides[k - 1];
  }
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

// The same for an LG_PREC_BF16 encoder: the launch list of enc_forward's bf16 branch onto the caller's maps, so the features are those of
// lg_conv_encoder_forward / lg_estimator_step bit for bit.  maps[0 .. 5] hold bf16, maps[6] the fp32 features.
int enc_forward_saved_bf16(lg_conv_encoder* e, const float* depth, int64_t depth_stride, int64_t n, void* const* maps, const int64_t* strides, hipStream_t st) {
  const void* in = depth; int64_t in_stride = depth_stride;
  for (int k = 1; k <= ENC_LAYERS + 1; ++k) {
    if (k == 5) hipLaunchKernelGGL(enc_bf16_pool_kernel, dim3((unsigned)((n * 1024 + 255) / 256)), dim3(256), 0, st, (const __bf16*)in, n, e->Hp, e->Wp, 64, (__bf16*)maps[k - 1]);
    else {
      const int rc = enc_launch_bf16(e->layer[k < 5 ? k - 1 : k - 2], k, in, in_stride, n, maps[k - 1], strides[k - 1], st);
      if (rc != LG_OK) return rc;
    }
    in = maps[k - 1]; in_stride = strides[k - 1];
  }
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

void enc_launch_cat(const float* proprio, int64_t n, int P, float* dst, int stride, int col0, hipStream_t st) {
  hipLaunchKernelGGL(cat_columns_kernel, dim3((unsigned)((n * P + 255) / 256)), dim3(256), 0, st, proprio, n, P, dst, stride, col0);
}
