// lg_estimator_train.hip — EstimatorDistillation.update (include/lgestimator_train.h) for the terrain estimator: a trainer over the four handles of
// an estimator (depth encoder, combination layer, memory, decoder).  A group of G steps is one batch of G * N rows.  Reused as they are: the
// encoder's forward kernels onto trainer-owned maps (lg_estimator_internal.h), lg_mlp_forward for the combination layer, the memory's forward with
// saved gates / backward step / retile (lg_train_recurrent_internal.h), and for every dense layer the forward with saved activations, the backward
// data pass, the slab weight gradients, the reduction, the norm and Adam of lg_train.hip (lg_train_internal.h), the loss (mse | huber | l1), the
// use_dones state mask and the update's loop (lg_train_sequence_internal.h).  New here, all fp32 on
// v_mfma_f32_16x16x4_f32, activations channel last (env, y, x, channel):
//
//   est_dgrad_kernel          the data gradient of a convolution (and, as the 1 x 1 convolution of a 1 x 1 image, of a linear layer) as an implicit
//                             GEMM: rows = (env, INPUT pixel), K = kh kw C_out ordered (ky, kx, co), columns = C_in, on a transposed tiling of the
//                             weights.  The tile, the LDS image and the k-chain are conv_gemm_kernel's; the gather takes D[e, oy, ox, co] where
//                             iy + pad - ky = stride oy (zero where the border says there is no such output pixel).  A stride-2 layer is four
//                             launches, one per parity (iy & 1, ix & 1) of the input pixel: each walks only the taps whose parity can reach an
//                             output pixel (4, 2, 2 and 1 of a 3 x 3 kernel's 9), through a table of the k-blocks of the one weight image -- the
//                             products left out are exact zeros, so the sums keep their bits and a quarter of the work remains.  The epilogue
//                             multiplies by the activation derivative of the layer BELOW, read from its saved output, so every delta that is
//                             written is one w.r.t. a pre-activation.
//   est_pool_backward_kernel  AdaptiveAvgPool2d((4, 4)) + Flatten backwards, torch's windows [floor(i L / 4), ceil((i + 1) L / 4)): one lane per map
//                             element gathers the (up to 4 x 4) windows that hold it, in (i, j) order; times the derivative of conv 4's activation.
//   est_conv_wgrad_kernel     dW[co, (ky, kx, ci)] and db of a convolution: the reduction runs over rows = (env, OUTPUT pixel), cut into slabs of
//                             EST_WGRAD_SLAB rows (blockIdx.y); a wave owns a 32 x 64 tile of [C_out][K + 1] and reads both operands from the maps
//                             (the tile of ppo_wgrad_kernel); partials in torch's (ci, ky, kx) order, reduced in slab order by ppo_grad_reduce_kernel.
//   est_act_delta_kernel      d *= act'(y) for the combination layer, whose weight gradient needs its pre-activation delta as rows.
//   est_conv_retile_kernel    the masters -> the forward images of conv 1-4 (lg_conv_tile_weights' layout, bit for bit) with their bias rows, and the
//                             transposed images of conv 2-4.
// A trainer of an LG_PREC_BF16 encoder (lg_estimator_bf16train_create) is the same object: its steps take the encoder's forward, the pooling / convolution
// backward and the retile from lg_estimator_train_bf16.hip (lg_estimator_train_internal.h) and everything else from here.
// No atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_estimator_train_internal.h"

#define EST_WGRAD_SLAB 8192         // rows (env, output pixel) per slab of a convolution's weight gradient

__global__ __launch_bounds__(CONV_THREADS) void est_dgrad_kernel(DgradLayer L, const float* __restrict__ D, int64_t d_estride, int64_t n, const float* __restrict__ ysrc,
                                                                  int64_t y_estride, float* __restrict__ out, int64_t out_estride) {
  __shared__ __attribute__((aligned(16))) float a_lds[2][CONV_KC * CONV_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = L.Hc * L.Wc;
  const int64_t M = n * HW, row0 = (int64_t)blockIdx.x * CONV_ROWS;
  const int kk = tid & 15, rb = tid >> 4;
  const float* src[4]; int iyp[4], ixp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t m = row0 + rb + 16 * j;
    if (m < M) {
      const int64_t e = m / HW; const int pix = (int)(m - e * HW), cy = pix / L.Wc, cx = pix - cy * L.Wc;
      iyp[j] = L.py + (cy << L.sh) + L.pad; ixp[j] = L.px + (cx << L.sh) + L.pad; src[j] = D + e * d_estride;
    } else { iyp[j] = -(1 << 20); ixp[j] = 0; src[j] = D; }          // no tap reaches an output pixel: zeros
  }
  float v[16];
  auto gather = [&](int kb0) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int t = L.ktab[(kb0 + b) * 16 + kk];
      const int ky = (t >> 26) & 15, kx = (t >> 22) & 15, co = t & 0x3fffff;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ty = iyp[j] - ky, tx = ixp[j] - kx, oy = ty >> L.sh, ox = tx >> L.sh;
        const bool ok = t >= 0 && ty >= 0 && tx >= 0 && ((ty | tx) & L.sh) == 0 && oy < L.Hout && ox < L.Wout;
        v[b * 4 + j] = ok ? src[j][((int64_t)oy * L.Wout + ox) * L.Cout + co] : 0.f;
      }
    }
  };
  const float4* wl = reinterpret_cast<const float4*>(L.wt) + (size_t)blockIdx.y * 4 * L.nkb_w * 64 + lane;
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
    int wb[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) wb[b] = L.wblk[kb0 + b];
    const float4* ap = reinterpret_cast<const float4*>(buf) + (wv * 16 + (lane & 15)) * 4 + (lane >> 4);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float4 a = ap[b * CONV_ROWS * 4];
      float4 w[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = wl[((size_t)c * L.nkb_w + wb[b]) * 64];
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
    const int64_t e = m / HW; const int cp = (int)(m - e * HW), cy = cp / L.Wc, cx = cp - cy * L.Wc;
    const int pix = (L.py + (cy << L.sh)) * L.Win + L.px + (cx << L.sh);
    float* dst = out + e * out_estride + (int64_t)pix * L.Cin;
    const float* ys = ysrc ? ysrc + e * y_estride + (int64_t)pix * L.Cin : nullptr;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = blockIdx.y * CONV_COLS + c * 16 + (lane & 15);
      if (col < L.Cin) dst[col] = ys ? acc[c][i] * est_act_grad(ys[col], L.act) : acc[c][i];
    }
  }
}

// dp (n, 16 C) in torch's flatten order c 16 + i 4 + j; y, d (n, H, W, C)
__global__ __launch_bounds__(256) void est_pool_backward_kernel(const float* __restrict__ dp, const float* __restrict__ y, int64_t n, int H, int W, int C, int act,
                                                                 float* __restrict__ d) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * H * W * C) return;
  const int c = (int)(idx % C); int64_t t = idx / C;
  const int xx = (int)(t % W); t /= W;
  const int yy = (int)(t % H); const int64_t e = t / H;
  float s = 0.f;
  for (int i = 0; i < 4; ++i) {
    const int y0 = (i * H) / 4, y1 = ((i + 1) * H + 3) / 4;
    if (yy < y0 || yy >= y1) continue;
    for (int j = 0; j < 4; ++j) {
      const int x0 = (j * W) / 4, x1 = ((j + 1) * W + 3) / 4;
      if (xx < x0 || xx >= x1) continue;
      s += dp[e * 16 * C + c * 16 + i * 4 + j] / (float)((y1 - y0) * (x1 - x0));
    }
  }
  d[idx] = s * est_act_grad(y[idx], act);
}

__global__ __launch_bounds__(256) void est_act_delta_kernel(float* __restrict__ d, const float* __restrict__ y, int64_t count, int act) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < count) d[idx] *= est_act_grad(y[idx], act);
}

struct WgradConv {
  int Hin, Win, Cin, Hout, Wout, Cout, stride, pad, kh, K;
  const float* D; int64_t d_estride;          // (rows, Hout, Wout, Cout)
  const float* X; int64_t x_estride;          // (rows, Hin, Win, Cin); T > 0: the (T, N, h, w) images, row r at time index (t0 + r / N) mod T
  int64_t N, T, t0;
  float* partial;                              // [slab][Cout][K + 1], column (ci kh + ky) kh + kx, the bias last
};

// MFMA 16x16x4 as ppo_wgrad_kernel: A operand lane (m = lane & 15, k = lane >> 4) = D[row k][co m], B operand lane (k = lane >> 4, n = lane & 15) =
// X[tap of row k][column n]; C[m = 4 (lane >> 4) + t][n = lane & 15].  Rows in ascending order per accumulator.  M < 2^31 (checked by the host).
__global__ __launch_bounds__(256) void est_conv_wgrad_kernel(WgradConv Wc, uint32_t M) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int dO = Wc.Cout, W = Wc.K + 1;
  const int to = (dO + 31) / 32, ti = (W + 63) / 64;
  const int tile = blockIdx.x * 4 + wv;
  const uint32_t r0 = blockIdx.y * (uint32_t)EST_WGRAD_SLAB;
  if (tile >= to * ti || r0 >= M) return;
  const uint32_t r1 = M - r0 > (uint32_t)EST_WGRAD_SLAB ? r0 + EST_WGRAD_SLAB : M;
  const int o0 = (tile / ti) * 32, i0 = (tile % ti) * 64;
  const int oc = o0 + (lane & 15);
  int ky[4], kx[4], ci[4], kind[4];            // this lane's four columns, (ky, kx, ci) with ci fastest: 16 lanes read 64 contiguous bytes of a pixel
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = i0 + 16 * q + (lane & 15);
    kind[q] = k < Wc.K ? 0 : (k == Wc.K ? 1 : 2);
    const int tap = k / Wc.Cin;
    ci[q] = k - tap * Wc.Cin; ky[q] = tap / Wc.kh; kx[q] = tap - ky[q] * Wc.kh;
  }
  const uint32_t HW = (uint32_t)(Wc.Hout * Wc.Wout);
  f32x4 acc[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[h][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (uint32_t ks = r0; ks < r1; ks += 4) {
    const uint32_t row = ks + (lane >> 4);
    const bool valid = row < r1;
    const uint32_t e = valid ? row / HW : 0, pix = valid ? row - e * HW : 0;
    const int oy = (int)(pix / (uint32_t)Wc.Wout), ox = (int)pix - oy * Wc.Wout;
    int64_t xe = e;
    if (Wc.T > 0) { const int64_t s = e / Wc.N; xe = ((Wc.t0 + s) % Wc.T) * Wc.N + (e - s * Wc.N); }
    const float* __restrict__ dr = Wc.D + (int64_t)e * Wc.d_estride + (int64_t)pix * dO;
    const float* __restrict__ xr = Wc.X + xe * Wc.x_estride;
    float av[2], bv[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) av[h] = (valid && oc + 16 * h < dO) ? dr[oc + 16 * h] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int iy = oy * Wc.stride - Wc.pad + ky[q], ix = ox * Wc.stride - Wc.pad + kx[q];
      const bool in = valid && kind[q] == 0 && iy >= 0 && iy < Wc.Hin && ix >= 0 && ix < Wc.Win;
      bv[q] = in ? xr[((int64_t)iy * Wc.Win + ix) * Wc.Cin + ci[q]] : ((valid && kind[q] == 1) ? 1.f : 0.f);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[h][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[h], bv[q], acc[h][q], 0, 0, 0);
  }
  float* __restrict__ P = Wc.partial + (size_t)blockIdx.y * dO * W;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (kind[q] == 2) continue;
      const int col = kind[q] == 1 ? Wc.K : (ci[q] * Wc.kh + ky[q]) * Wc.kh + kx[q];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int o = o0 + 16 * h + 4 * (lane >> 4) + t;
        if (o < dO) P[(size_t)o * W + col] = acc[h][q][t];
      }
    }
}

struct ConvRetile {
  float* fw; float* fb; float* bw;            // forward image, bias row (C_out padded to 64), transposed image (NULL: conv 1)
  int Cout, Cin, kh, nkb_f, nch_f, nkb_b, nch_b;
  int64_t woff, boff;
};

__global__ __launch_bounds__(256) void est_conv_retile_kernel(const ConvRetile* __restrict__ tab, const float* __restrict__ theta) {
  const ConvRetile R = tab[blockIdx.y];
  int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int taps = R.kh * R.kh, K = R.Cin * taps, Kb = R.Cout * taps;
  const int64_t fcount = (int64_t)R.nch_f * R.nkb_f * 256, bcount = R.bw ? (int64_t)R.nch_b * R.nkb_b * 256 : 0;
  if (e < fcount) {          // lg_conv_tile_weights: [chunk][k / 16][lane][4], column = chunk 16 + (lane & 15), k = block 16 + slot 4 + (lane >> 4), k = (ky, kx, ci)
    const int s = (int)(e & 3), ln = (int)((e >> 2) & 63);
    const int64_t rest = e >> 8;
    const int b = (int)(rest % R.nkb_f), c = (int)(rest / R.nkb_f);
    const int col = c * 16 + (ln & 15), k = b * 16 + s * 4 + (ln >> 4);
    float v = 0.f;
    if (col < R.Cout && k < K) {
      const int ci = k % R.Cin, tap = k / R.Cin, ky = tap / R.kh, kx = tap - ky * R.kh;
      v = theta[R.woff + (((int64_t)col * R.Cin + ci) * R.kh + ky) * R.kh + kx];
    }
    R.fw[e] = v;
    return;
  }
  e -= fcount;
  if (e < bcount) {          // the same tiling of the transposed product: column = ci, k = (ky, kx, co)
    const int s = (int)(e & 3), ln = (int)((e >> 2) & 63);
    const int64_t rest = e >> 8;
    const int b = (int)(rest % R.nkb_b), c = (int)(rest / R.nkb_b);
    const int col = c * 16 + (ln & 15), k = b * 16 + s * 4 + (ln >> 4);
    float v = 0.f;
    if (col < R.Cin && k < Kb) {
      const int co = k % R.Cout, tap = k / R.Cout, ky = tap / R.kh, kx = tap - ky * R.kh;
      v = theta[R.woff + (((int64_t)co * R.Cin + col) * R.kh + ky) * R.kh + kx];
    }
    R.bw[e] = v;
    return;
  }
  e -= bcount;
  if (e < ((R.Cout + 63) & ~63)) R.fb[e] = e < R.Cout ? theta[R.boff + e] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------------ host side
static TrainMem* est_mem(lg_estimator_train* p) { return p ? &p->tm : nullptr; }

// the masters -> the convolutions' and the memory's images (the dense layers' are the Adam kernel's / train_core_retile's)
static int est_retile(TrainCore* c, hipStream_t st) {
  lg_estimator_train* p = static_cast<lg_estimator_train*>(c);
  if (p->b16) est16_retile(p, st);
  else hipLaunchKernelGGL(est_conv_retile_kernel, dim3((unsigned)((p->cretile_big + 255) / 256), 4), dim3(256), 0, st, (const ConvRetile*)p->d_cretile, (const float*)p->theta);
  return mem_retile(&p->tm, p->theta, st);
}

void est_launch_dgrad(const DgradLayer& L, const float* D, int64_t d_estride, int64_t n, const float* ysrc, int64_t y_estride, float* out, int64_t out_estride,
                      hipStream_t st) {
  if (L.Hc < 1 || L.Wc < 1) return;
  const int64_t tiles = (n * L.Hc * L.Wc + CONV_ROWS - 1) / CONV_ROWS;
  hipLaunchKernelGGL(est_dgrad_kernel, dim3((unsigned)tiles, (unsigned)((L.Cin + CONV_COLS - 1) / CONV_COLS)), dim3(CONV_THREADS), 0, st, L, D, d_estride, n, ysrc, y_estride,
                     out, out_estride);
}

// conv l (0-based) of the encoder: D (n, Hout, Wout, Cout), X its input maps; returns the number of slabs
static int est_launch_conv_wgrad(lg_estimator_train* p, int l, const float* D, const float* X, int64_t x_estride, int64_t n, int64_t N, int64_t T, int64_t t0, hipStream_t st) {
  const ConvLayerDev& C = p->enc->layer[l];
  const TrainSeg& S = p->seg[p->nd + l];
  WgradConv W;
  W.Hin = C.Hin; W.Win = C.Win; W.Cin = C.Cin; W.Hout = C.Hout; W.Wout = C.Wout; W.Cout = C.Cout; W.stride = C.stride; W.pad = C.pad; W.kh = kConvShape[l][2];
  W.K = C.Cin * W.kh * W.kh;
  W.D = D; W.d_estride = (int64_t)C.Hout * C.Wout * C.Cout; W.X = X; W.x_estride = x_estride; W.N = N; W.T = T; W.t0 = t0; W.partial = S.partial;
  const int64_t M = n * C.Hout * C.Wout;
  const int nslabs = (int)((M + EST_WGRAD_SLAB - 1) / EST_WGRAD_SLAB);
  const int tiles = ((C.Cout + 31) / 32) * ((W.K + 1 + 63) / 64);
  hipLaunchKernelGGL(est_conv_wgrad_kernel, dim3((unsigned)((tiles + 3) / 4), (unsigned)nslabs), dim3(256), 0, st, W, (uint32_t)M);
  return nslabs;
}

// stages 1-7 of the fp32 encoder on rows [at, at + n) of the group: the saved maps, the features into the cat rows
static int est_forward_fp32(lg_estimator_train* p, const float* depth, int64_t depth_stride, int64_t n, int64_t at, hipStream_t st) {
  float* maps[7] = {p->map[0] + at * p->map_floats[0], p->map[1] + at * p->map_floats[1], p->map[2] + at * p->map_floats[2], p->map[3] + at * p->map_floats[3],
                    p->pool + at * 1024, p->y5 + at * 128, p->cat + at * p->cat_w};
  const int64_t strides[7] = {p->map_floats[0], p->map_floats[1], p->map_floats[2], p->map_floats[3], 1024, 128, p->cat_w};
  return enc_forward_saved(p->enc, depth, depth_stride, n, maps, strides, st);
}

// from dpool: the pooling and conv 4 .. conv 1 backwards, each convolution's weight gradient as soon as its delta stands (two delta buffers ping-pong);
// cslabs[l]: the slabs of conv l + 1's weight gradient.  The sibling of est16_backward.
static void est_backward_fp32(lg_estimator_train* p, const float* depth, int64_t n, int64_t N, int64_t T, int64_t t0, int* cslabs, hipStream_t st) {
  const ConvLayerDev* C = p->enc->layer;
  const int hw = p->enc->H * p->enc->W;
  hipLaunchKernelGGL(est_pool_backward_kernel, dim3((unsigned)((n * p->map_floats[3] + 255) / 256)), dim3(256), 0, st, (const float*)p->dpool, (const float*)p->map[3], n,
                     C[3].Hout, C[3].Wout, 64, p->act, p->dB);
  cslabs[3] = est_launch_conv_wgrad(p, 3, p->dB, p->map[2], p->map_floats[2], n, N, 0, 0, st);
  for (int k = 0; k < 4; ++k) est_launch_dgrad(p->dg_conv[3][k], p->dB, p->map_floats[3], n, p->map[2], p->map_floats[2], p->dA, p->map_floats[2], st);
  cslabs[2] = est_launch_conv_wgrad(p, 2, p->dA, p->map[1], p->map_floats[1], n, N, 0, 0, st);
  for (int k = 0; k < 4; ++k) est_launch_dgrad(p->dg_conv[2][k], p->dA, p->map_floats[2], n, p->map[1], p->map_floats[1], p->dB, p->map_floats[1], st);
  cslabs[1] = est_launch_conv_wgrad(p, 1, p->dB, p->map[0], p->map_floats[0], n, N, 0, 0, st);
  for (int k = 0; k < 4; ++k) est_launch_dgrad(p->dg_conv[1][k], p->dB, p->map_floats[1], n, p->map[0], p->map_floats[0], p->dA, p->map_floats[0], st);
  cslabs[0] = est_launch_conv_wgrad(p, 0, p->dA, depth, hw, n, N, T, t0, st);
}

static int est_check_call(lg_estimator_train* p, const float* depth, const float* proprio, const float* tgt, const float* dones, int64_t T, int64_t N,
                          const lg_estimator_train_hyper* h) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!depth || !tgt || !h || (p->P_in > 0 && !proprio)) return lg_policy_fail(LG_ERR_INVALID, "null depth images, proprio rows, targets or hyper-parameters");
  if (T < 1 || N < 1) return lg_policy_fail(LG_ERR_INVALID, "T < 1 or N < 1");
  if (h->loss_type != LG_EST_LOSS_MSE && h->loss_type != LG_EST_LOSS_HUBER && h->loss_type != LG_EST_LOSS_L1)
    return lg_policy_fail(LG_ERR_INVALID, "unknown loss type (mse | huber | l1)");
  if (h->use_dones && !dones) return lg_policy_fail(LG_ERR_INVALID, "use_dones without dones");
  return mem_check_rows(&p->tm, N);
}

// steps [first, first + nsteps) of the sequence as one batch; train: an optimiser step, else forward and loss only.  seq_loss: where the update keeps
// these steps' losses, or NULL.
static int est_steps(lg_estimator_train* p, const float* depth, const float* proprio, const float* tgt, const float* dones, int64_t T, int64_t N, int64_t first,
                     int64_t nsteps, const lg_estimator_train_hyper* h, bool train, float* seq_loss, hipStream_t st) {
  const int64_t n = nsteps * N, t0 = first % T;
  const int hw = p->enc->H * p->enc->W;
  const bool use_dones = h->use_dones != 0;
  TrainMem* M = &p->tm;
  const MemSpan W{T, N, t0, nsteps, use_dones ? dones : nullptr};
  int rc = mem_open_carry(M, N, st);
  if (rc != LG_OK) return rc;
  p->last_rows = n;
  if (p->b16) { p->last_depth = depth; p->last_N = N; p->last_T = T; p->last_t0 = t0; }          // lg_estimator_bf16train_backward_stage reads them
  p->last_steps = nsteps;                                    // always, and group_loss with it: after an update they are the forward-only remainder's, if there is one
  // ---- the encoder and the cat rows, one launch list per run of consecutive time indices
  for (int64_t s = 0; s < nsteps;) {
    const int64_t t = (t0 + s) % T, len = std::min(nsteps - s, T - t), at = s * N;
    if ((rc = p->b16 ? est16_forward(p, depth + t * N * hw, hw, len * N, at, st) : est_forward_fp32(p, depth + t * N * hw, hw, len * N, at, st)) != LG_OK) return rc;
    if (p->P_in > 0) enc_launch_cat(proprio + t * N * p->P_in, len * N, p->P_in, p->cat + at * p->cat_w, p->cat_w, p->F, st);
    s += len;
  }
  if ((rc = lg_mlp_forward(p->combine, p->cat, n, p->comb, st)) != LG_OK) return rc;
  mem_forward(M, W, p->comb, false, st);
  // ---- the decoder on the memory's outputs, the losses
  const TrainNet& Dn = p->net[0];
  const float* top = M->layer[M->ML - 1].hnew;
  train_launch_forward(p, top, top, nullptr, n, st);
  seq_launch_loss(p, Dn.a[Dn.L], tgt, N, T, t0, nsteps, h->loss_type, train ? Dn.d[Dn.L - 1] : (float*)nullptr, p->group_loss, seq_loss, train ? 1 : 0, st);
  if (train) {
    // ---- the decoder backwards and dL/d(its input); then backwards through time: layer 0 propagates into the combination layer's output
    train_launch_backward(p, n, st);
    mem_top_matmul(M, Dn, n, st);
    mem_backward(M, W, p->dcomb, st);
    // ---- the combination layer and the encoder backwards; each convolution's weight gradient as soon as its delta stands (two delta buffers ping-pong)
    hipLaunchKernelGGL(est_act_delta_kernel, dim3((unsigned)((n * p->Fc + 255) / 256)), dim3(256), 0, st, p->dcomb, (const float*)p->comb, n * p->Fc, p->act);
    est_launch_dgrad(p->dg_comb, p->dcomb, p->Fc, n, p->cat, p->cat_w, p->d6, p->F, st);
    est_launch_dgrad(p->dg_l12, p->d6, p->F, n, p->y5, 128, p->d5, 128, st);
    est_launch_dgrad(p->dg_l10, p->d5, 128, n, nullptr, 0, p->dpool, 1024, st);
    int cslabs[4];
    if (p->b16) est16_backward(p, depth, n, N, T, t0, cslabs, st);
    else est_backward_fp32(p, depth, n, N, T, t0, cslabs, st);
    // ---- the dense weight gradients in one slab pass, every reduction, the norm, Adam, the images
    train_launch_wgrad_range(p, 0, p->nd, nullptr, nullptr, nullptr, n, st);
    train_launch_reduce_range(p, 0, p->nd, (int)((n + WGRAD_SLAB - 1) / WGRAD_SLAB), st);
    for (int l = 0; l < 4; ++l) train_launch_reduce_range(p, p->nd + l, 1, cslabs[l], st);
    if ((rc = train_launch_norm_adam(p, h->max_grad_norm, h->max_grad_norm > 0.f ? 1 : 0, st)) != LG_OK) return rc;
    if ((rc = est_retile(p, st)) != LG_OK) return rc;
  }
  // ---- the running state: the memory after the last step
  if ((rc = mem_keep_running(M, W, st)) != LG_OK) return rc;
  if (use_dones) seq_launch_mask_rows(M->cur_h, M->cur_c, dones + ((t0 + nsteps - 1) % T) * N, N, M->H, M->max_rows * M->H, M->ML, st);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

static const int32_t* est_upload_table(lg_estimator_train* p, const std::vector<int32_t>& t) {
  int32_t* d = (int32_t*)train_alloc(p, t.size() * sizeof(int32_t), false);
  if (d && hipMemcpy(d, t.data(), t.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { lg_policy_fail(LG_ERR_HIP, "table upload failed"); return nullptr; }
  return d;
}

// The tables of one data-gradient launch: the taps (ky, kx) a pixel of parity (py, px) can reach an output pixel through (all of them for stride 1),
// each with its cout channels -- k-blocks of 16 lie inside one tap when cout is a multiple of 16, which every strided layer's is; else (the linear
// layers, one tap) the k order is the weight image's own.  false + message on failure.
static bool est_dgrad_tables(lg_estimator_train* p, DgradLayer& G, int kh, int stride) {
  std::vector<int32_t> kt, wb;
  for (int ky = 0; ky < kh; ++ky)
    for (int kx = 0; kx < kh; ++kx) {
      if (stride == 2 && ((((G.py + G.pad - ky) & 1) != 0) || (((G.px + G.pad - kx) & 1) != 0))) continue;
      for (int co = 0; co < G.Cout; ++co) {
        if ((kt.size() & 15) == 0) wb.push_back((int32_t)(((ky * kh + kx) * G.Cout + co) / 16));
        kt.push_back((ky << 26) | (kx << 22) | co);
      }
    }
  if (kt.empty()) { G.Hc = 0; return true; }              // no tap reaches these pixels (not with a 3 x 3 kernel and pad 1): nothing to launch
  G.nkb = (int)((kt.size() + 63) & ~(size_t)63) / 16;
  kt.resize((size_t)G.nkb * 16, -1);
  wb.resize((size_t)G.nkb, 0);                             // padding blocks: their A operands are zeros, any block of the image serves
  G.ktab = est_upload_table(p, kt);
  G.wblk = G.ktab ? est_upload_table(p, wb) : nullptr;
  return G.wblk != nullptr;
}

extern "C" {

int32_t lg_estimator_train_wgrad_slab_rows(void) { return EST_WGRAD_SLAB; }

void lg_estimator_train_destroy(lg_estimator_train* p) {
  if (!p) return;
  DeviceScope ds_(p->device);
  (void)hipDeviceSynchronize();
  est16_free(p);
  train_core_free(p);
  delete p;
}

lg_estimator_train* lg_estimator_train_create(lg_conv_encoder* enc, lg_mlp* combine, lg_rnn* mem, lg_mlp* decoder, const lg_estimator_train_params* q, double learning_rate,
                                              int64_t max_rows) {
  POLICY_ENTRY;
  if (enc && enc->prec != LG_PREC_F32) {
    lg_policy_fail(LG_ERR_UNSUPPORTED, "a bf16 encoder cannot be trained by this entry: lg_estimator_bf16train_create trains it, or train fp32, then build a bf16 estimator from the parameters");
    return nullptr;
  }
  return est_train_create(enc, combine, mem, decoder, q, learning_rate, max_rows, false);
}

}  // extern "C"

lg_estimator_train* est_train_create(lg_conv_encoder* enc, lg_mlp* combine, lg_rnn* mem, lg_mlp* decoder, const lg_estimator_train_params* q, double learning_rate,
                                     int64_t max_rows, bool bf16) {
  if (!enc || !combine || !mem || !decoder) { lg_policy_fail(LG_ERR_INVALID, "null encoder, combination layer, memory or decoder"); return nullptr; }
  if (!q) { lg_policy_fail(LG_ERR_INVALID, "null parameters"); return nullptr; }
  if (!q->encoder_weights || !q->encoder_biases || !q->combine_weight || !q->combine_bias || !q->memory_w_ih || !q->memory_w_hh || !q->memory_b_ih || !q->memory_b_hh ||
      !q->decoder_weights || !q->decoder_biases) { lg_policy_fail(LG_ERR_INVALID, "null parameter list"); return nullptr; }
  if (max_rows < 1) { lg_policy_fail(LG_ERR_INVALID, "max_rows < 1"); return nullptr; }
  if (!(learning_rate > 0.0)) { lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0"); return nullptr; }
  if (mem->wide) {
    lg_policy_fail(LG_ERR_UNSUPPORTED, "the memory is a wide one (lg_rnn_create_wide, " + std::to_string(mem->input) + " inputs): the estimator's memory takes at most " +
                                           std::to_string(RNN_XMAX) + " inputs");
    return nullptr;
  }
  const int F = enc->out_dim, cat_w = combine->h.dims[0], Fc = combine->h.dims[combine->h.L], H = mem->hidden, ML = mem->num_layers;
  if (combine->h.L != 1 || cat_w < F || Fc != mem->input || decoder->h.dims[0] != H) {
    lg_policy_fail(LG_ERR_INVALID, "stage widths do not chain (combine: one layer of encoder out_dim + proprio inputs; its outputs = the memory's input; decoder input = the memory's hidden width)");
    return nullptr;
  }
  if (!combine->h.act_out || decoder->h.act_out) { lg_policy_fail(LG_ERR_INVALID, "the combination layer must end in the activation and the decoder must not"); return nullptr; }
  if (combine->device != enc->device || mem->device != enc->device || decoder->device != enc->device) { lg_policy_fail(LG_ERR_INVALID, "the stages live on different devices"); return nullptr; }
  if (ML < 1 || ML > RNN_MAX_LAYERS) { lg_policy_fail(LG_ERR_INVALID, "memory depth out of range"); return nullptr; }
  for (int l = 0; l < ENC_LAYERS; ++l) if (!q->encoder_weights[l] || !q->encoder_biases[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  for (int l = 0; l < ML; ++l) if (!q->memory_w_ih[l] || !q->memory_w_hh[l] || !q->memory_b_ih[l] || !q->memory_b_hh[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  for (int l = 0; l < decoder->h.L; ++l) if (!q->decoder_weights[l] || !q->decoder_biases[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  if (max_rows * (int64_t)enc->H * enc->W > 0x7fffffff) { lg_policy_fail(LG_ERR_UNSUPPORTED, "max_rows x image pixels exceeds 2^31 - 1"); return nullptr; }
  if (!lg_policy_device_ok(enc->device)) return nullptr;
  DeviceScope ds_(enc->device);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_estimator_train* p = new lg_estimator_train();
  p->enc = enc; p->combine = combine; p->decoder = decoder; p->device = enc->device; p->max_rows = max_rows;
  p->F = F; p->cat_w = cat_w; p->P_in = cat_w - F; p->Fc = Fc; p->act = enc->act;
  p->retile_own = est_retile;
  TrainMem* M = &p->tm;
  bool ok = true;
  auto alloc = [&](size_t floats, bool zero) -> float* { float* d = ok ? (float*)train_alloc(p, floats * sizeof(float), zero) : nullptr; if (!d) ok = false; return d; };
  const size_t R = (size_t)max_rows;
  // ---- workspaces
  for (int l = 0; l < 4; ++l) { p->map_floats[l] = (int64_t)enc->layer[l].Hout * enc->layer[l].Wout * enc->layer[l].Cout; if (!bf16) p->map[l] = alloc(R * p->map_floats[l], false); }
  p->pool = alloc(R * 1024, false); p->y5 = alloc(R * 128, false); p->cat = alloc(R * cat_w, false); p->comb = alloc(R * Fc, false);
  if (!bf16) { p->dA = alloc(R * std::max(p->map_floats[0], p->map_floats[2]), false); p->dB = alloc(R * std::max(p->map_floats[1], p->map_floats[3]), false); }
  p->dpool = alloc(R * 1024, false); p->d5 = alloc(R * 128, false); p->d6 = alloc(R * F, false); p->dcomb = alloc(R * Fc, false);
  ok = ok && mem_alloc(p, M, mem);
  const int K = M->Gates * H, nbk = (K + 15) / 16;
  // ---- segments: the decoder's (net 0), then the dense ones by hand, then the convolutions.  Layer ids behind the decoder's index the host tables.
  int64_t off = 0;
  ok = ok && train_core_add_net(p, decoder, &off);
  const int dec_first = 0, Ld = decoder->h.L;
  enum { ID_L10 = LG_MLP_MAX_LAYERS, ID_L12, ID_COMB, ID_MEM, ID_CONV = ID_MEM + 2 * RNN_MAX_LAYERS, ID_COUNT = ID_CONV + 4 };
  const float* wtab[ID_COUNT] = {}; const float* btab[ID_COUNT] = {};
  for (int l = 0; l < Ld; ++l) { wtab[l] = q->decoder_weights[l]; btab[l] = q->decoder_biases[l]; }
  auto dense_seg = [&](int id, int dO, int dI, const float* Dp, const float* Ain, float* fw, float* fb, int f_nb, float* bw, int b_nb) -> TrainSeg& {
    return train_core_add_seg(p, 0, id, dO, dI, Dp, Ain, fw, fb, f_nb, bw, b_nb, &ok);
  };
  // a transposed image the data-gradient kernel reads: chunks of 16 inputs padded to 64 columns, K = dO padded to 64
  auto transposed = [&](int dO, int dI) -> float* { return alloc((size_t)(((dI + 63) & ~63) / 16) * (((dO + 63) & ~63) / 16) * 256, true); };
  const ConvLayerDev& L10 = enc->layer[4]; const ConvLayerDev& L12 = enc->layer[5];
  float* bw10 = transposed(128, 1024); float* bw12 = transposed(F, 128); float* bwc = transposed(Fc, cat_w);
  const int seg_l10 = p->seg_l10 = p->nseg;
  if (bf16) {          // Adam writes no image of the two linear layers: est16_retile rounds the masters into the bf16 forward images and the fp32 transposed ones
    dense_seg(ID_L10, 128, 1024, p->d5, p->pool, nullptr, nullptr, 0, nullptr, 0);
    dense_seg(ID_L12, F, 128, p->d6, p->y5, nullptr, nullptr, 0, nullptr, 0);
  } else {
    dense_seg(ID_L10, 128, 1024, p->d5, p->pool, const_cast<float*>(L10.w), const_cast<float*>(L10.b), L10.nkb, bw10, 128 / 16);
    dense_seg(ID_L12, F, 128, p->d6, p->y5, const_cast<float*>(L12.w), const_cast<float*>(L12.b), L12.nkb, bw12, ((F + 63) & ~63) / 16);
  }
  dense_seg(ID_COMB, Fc, cat_w, p->dcomb, p->cat, const_cast<float*>(combine->h.w[0]), const_cast<float*>(combine->h.b[0]), combine->h.kpad[0] / 16, bwc, ((Fc + 63) & ~63) / 16);
  wtab[ID_L10] = q->encoder_weights[4]; btab[ID_L10] = q->encoder_biases[4];
  wtab[ID_L12] = q->encoder_weights[5]; btab[ID_L12] = q->encoder_biases[5];
  wtab[ID_COMB] = q->combine_weight; btab[ID_COMB] = q->combine_bias;
  const int seg_mem = p->nseg;
  for (int l = 0; l < ML && ok; ++l) {
    const MemLayer& Y = M->layer[l];
    const int I = l == 0 ? Fc : H;
    dense_seg(ID_MEM + 2 * l, K, I, Y.Dih, l == 0 ? p->comb : M->layer[l - 1].hnew, nullptr, nullptr, 0, Y.wtx, nbk);
    dense_seg(ID_MEM + 2 * l + 1, K, H, Y.Dhh, Y.hin, nullptr, nullptr, 0, Y.wth, nbk);
    wtab[ID_MEM + 2 * l] = q->memory_w_ih[l]; btab[ID_MEM + 2 * l] = q->memory_b_ih[l];
    wtab[ID_MEM + 2 * l + 1] = q->memory_w_hh[l]; btab[ID_MEM + 2 * l + 1] = q->memory_b_hh[l];
  }
  p->nd = p->nseg;
  // the decoder's first layer reads the top layer's h' (dense, step-major) and propagates into it: a transposed tiling for layer 0 too
  {
    TrainNet& Nn = p->net[0];
    float* bw0 = alloc((size_t)Nn.bnch[0] * (Nn.bkpad[0] / 16) * 256, true);
    Nn.bw[0] = bw0; p->seg[dec_first].bw = bw0; p->seg[dec_first].Ain = M->layer[ML - 1].hnew;
  }
  float* conv_bw[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int l = 0; l < 4 && ok; ++l) {          // the partials are est_conv_wgrad_kernel's; Adam writes no image (fw, fb, bw NULL): est_conv_retile_kernel does
    const ConvLayerDev& C = enc->layer[l];
    const int kh = kConvShape[l][2], dI = C.Cin * kh * kh;
    const int64_t slab = bf16 ? est16_slab_rows() : EST_WGRAD_SLAB, cslabs = (max_rows * C.Hout * C.Wout + slab - 1) / slab;
    TrainSeg& S = p->seg[p->nseg++];
    S.net = 0; S.layer = ID_CONV + l; S.dO = C.Cout; S.dI = dI; S.f_nb = 0; S.b_nb = 0; S.woff = 0; S.boff = 0; S.D = nullptr; S.Ain = nullptr;
    S.partial = alloc((size_t)cslabs * C.Cout * (dI + 1), false);
    S.fw = nullptr; S.fb = nullptr; S.bw = nullptr;
    const int64_t cnt = (int64_t)C.Cout * (dI + 1);
    if (cnt > p->big) p->big = cnt;
    wtab[ID_CONV + l] = q->encoder_weights[l]; btab[ID_CONV + l] = q->encoder_biases[l];
    if (l > 0 && !bf16) conv_bw[l] = alloc((size_t)(((C.Cin + 63) & ~63) / 16) * (((kh * kh * C.Cout + 63) & ~63) / 16) * 256, true);
  }
  // ---- the flat order: the module's state_dict()
  auto place = [&](TrainSeg& S) { S.woff = off; off += (int64_t)S.dO * S.dI; S.boff = off; off += S.dO; };
  off = 0;
  for (int l = 0; l < 4; ++l) place(p->seg[p->nd + l]);
  place(p->seg[seg_l10]); place(p->seg[seg_l10 + 1]); place(p->seg[seg_l10 + 2]);
  for (int l = 0; l < ML; ++l) mem_place_layer(M, l, p->seg[seg_mem + 2 * l], p->seg[seg_mem + 2 * l + 1], &off);
  for (int l = 0; l < Ld; ++l) place(p->seg[dec_first + l]);
  std::vector<ConvRetile> cret(4);
  for (int l = 0; l < 4; ++l) {
    const ConvLayerDev& C = enc->layer[l];
    const int kh = kConvShape[l][2];
    ConvRetile& r = cret[l];
    r.fw = const_cast<float*>(C.w); r.fb = const_cast<float*>(C.b); r.bw = conv_bw[l];
    r.Cout = C.Cout; r.Cin = C.Cin; r.kh = kh; r.nkb_f = C.nkb; r.nch_f = ((C.Cout + 63) & ~63) / 16;
    r.nkb_b = ((kh * kh * C.Cout + 63) & ~63) / 16; r.nch_b = ((C.Cin + 63) & ~63) / 16;
    r.woff = p->seg[p->nd + l].woff; r.boff = p->seg[p->nd + l].boff;
    const int64_t cnt = (int64_t)r.nch_f * r.nkb_f * 256 + (r.bw ? (int64_t)r.nch_b * r.nkb_b * 256 : 0) + ((C.Cout + 63) & ~63);
    if (cnt > p->cretile_big) p->cretile_big = cnt;
  }
  // ---- the data-gradient passes
  auto dgrad = [&](DgradLayer& G, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int kh, int stride, int pad, const float* wt, int cls) {
    G.Hin = Hin; G.Win = Win; G.Cin = Cin; G.Hout = Hout; G.Wout = Wout; G.Cout = Cout; G.sh = stride - 1; G.pad = pad; G.act = p->act;
    G.py = cls >> 1; G.px = cls & 1;
    G.Hc = (Hin - G.py + stride - 1) / stride; G.Wc = (Win - G.px + stride - 1) / stride;
    G.nkb_w = ((kh * kh * Cout + 63) & ~63) / 16; G.wt = wt;
    if (ok && !est_dgrad_tables(p, G, kh, stride)) ok = false;
  };
  dgrad(p->dg_comb, 1, 1, F, 1, 1, Fc, 1, 1, 0, bwc, 0);          // only the first F inputs of the cat rows are propagated: the proprio columns are data
  dgrad(p->dg_l12, 1, 1, 128, 1, 1, F, 1, 1, 0, bw12, 0);
  dgrad(p->dg_l10, 1, 1, 1024, 1, 1, 128, 1, 1, 0, bw10, 0);
  for (int l = 1; l < 4 && !bf16; ++l) {
    const ConvLayerDev& C = enc->layer[l];
    for (int cls = 0; cls < 4; ++cls) {
      if (C.stride == 1 && cls > 0) { p->dg_conv[l][cls] = DgradLayer{}; continue; }          // Hc = 0: never launched
      dgrad(p->dg_conv[l][cls], C.Hin, C.Win, C.Cin, C.Hout, C.Wout, C.Cout, kConvShape[l][2], C.stride, C.pad, conv_bw[l], cls);
    }
  }
  // ---- losses (the row index stays out: only the first convolution's weight gradient reads rows by time index, and it computes them itself)
  ok = ok && seq_alloc(p, max_rows, decoder->h.dims[decoder->h.L], false);
  p->d_cretile = ok ? (ConvRetile*)train_alloc(p, sizeof(ConvRetile) * 4, true) : nullptr;
  ok = ok && p->d_cretile;
  ok = ok && mem_upload_retile(p, M);
  ok = ok && (!bf16 || est16_setup(p, bw10, bw12));
  const float* const* ws[1] = {wtab};
  const float* const* bs[1] = {btab};
  if (!ok || train_core_finish(p, off, ws, bs, nullptr, learning_rate) != LG_OK ||
      hipMemcpy(p->d_cretile, cret.data(), sizeof(ConvRetile) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      est_retile(p, nullptr) != LG_OK || hipDeviceSynchronize() != hipSuccess) {
    lg_estimator_train_destroy(p);
    return nullptr;
  }
  return p;
}

extern "C" {

int lg_estimator_train_group(lg_estimator_train* p, const float* depth, const float* proprio, const float* tgt, const float* dones, int64_t T, int64_t N,
                             int64_t first_step, int64_t num_steps, int32_t train, const lg_estimator_train_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  int rc = est_check_call(p, depth, proprio, tgt, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  if ((rc = seq_check_group(p, N, first_step, num_steps)) != LG_OK) return rc;
  DeviceScope ds_(p->device);
  return est_steps(p, depth, proprio, tgt, dones, T, N, first_step, num_steps, hyper, train != 0, nullptr, (hipStream_t)stream);
}

int lg_estimator_train_update(lg_estimator_train* p, const float* depth, const float* proprio, const float* tgt, const float* dones, int64_t T, int64_t N, int32_t E,
                              int32_t G, const lg_estimator_train_hyper* hyper, lg_estimator_train_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = est_check_call(p, depth, proprio, tgt, dones, T, N, hyper);
  if (rc != LG_OK) return rc;
  return seq_update(p, T, N, E, G, [&](int64_t first, int64_t nsteps, bool train, float* seq_loss, hipStream_t st) {
    return est_steps(p, depth, proprio, tgt, dones, T, N, first, nsteps, hyper, train, seq_loss, st); }, &p->tm, stats, nullptr, stream);
}

int64_t lg_estimator_train_parameter_count(lg_estimator_train* p) {
  POLICY_ENTRY;
  return train_api_parameter_count(p);
}

int64_t lg_estimator_train_workspace_bytes(lg_estimator_train* p) {
  POLICY_ENTRY;
  return train_api_workspace_bytes(p);
}

int lg_estimator_train_gradients(lg_estimator_train* p, float* g, float* norm, float* losses, int64_t capacity, void* stream) {
  POLICY_ENTRY;
  return train_api_group_gradients(p, g, norm, losses, capacity, stream);
}

int lg_estimator_train_forward_outputs(lg_estimator_train* p, float* predictions, void* stream) {
  POLICY_ENTRY;
  return seq_forward_outputs(p, predictions, stream);
}

int lg_estimator_train_step_losses(lg_estimator_train* p, float* losses, int64_t count, void* stream) {
  POLICY_ENTRY;
  return train_api_step_losses(p, losses, count, stream);
}

// the caller's h / c are HOST arrays
int64_t lg_estimator_train_get_carry(lg_estimator_train* p, float* h, float* c, int64_t capacity_rows, int32_t running, void* stream) {
  POLICY_ENTRY;
  return mem_get_carry(est_mem(p), h, c, capacity_rows, running, hipMemcpyDeviceToHost, stream);
}

int lg_estimator_train_set_carry(lg_estimator_train* p, const float* h, const float* c, int64_t N, void* stream) {
  POLICY_ENTRY;
  return mem_set_carry(est_mem(p), h, c, N, hipMemcpyHostToDevice, stream);
}

int lg_estimator_train_reset_carry(lg_estimator_train* p, void* stream) {
  POLICY_ENTRY;
  return mem_reset_carry(est_mem(p));
}

int lg_estimator_train_get_state(lg_estimator_train* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  POLICY_ENTRY;
  return train_api_get_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_estimator_train_get_parameters(lg_estimator_train* p, float* params, void* stream) {
  POLICY_ENTRY;
  return train_api_get_parameters(p, params, stream);
}

int lg_estimator_train_set_state(lg_estimator_train* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_estimator_train_set_learning_rate(lg_estimator_train* p, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_learning_rate(p, lr, stream);
}

}  // extern "C"
