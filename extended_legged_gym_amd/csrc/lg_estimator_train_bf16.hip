// lg_estimator_train_bf16.hip — the encoder side of the terrain estimator's trainer for an LG_PREC_BF16 depth encoder (include/lgestimator_train_bf16.h).
// The trainer, its create body, its steps and every lg_estimator_train_* entry point are lg_estimator_train.hip's (lg_estimator_train_internal.h); the
// forward is the bf16 inference launch list onto trainer-owned maps (enc_forward_saved_bf16).  New here, on v_mfma_f32_16x16x32_bf16 with fp32
// accumulators, maps and map-shaped deltas bf16 channel last (env, y, x, channel):
//
//   est16_dgrad_kernel          the data gradient of conv 2-4, est_dgrad_kernel's implicit GEMM: rows = (env, INPUT pixel), K = (ky, kx, co) with co
//                               fastest, columns = C_in.  Every C_out is a multiple of 32, so a k-step of 32 lies inside one tap and a lane's eight A
//                               operands are 16 contiguous bytes of the delta map, loaded straight from global memory (zero where no output pixel is
//                               reached), as enc_bf16_gemm_kernel loads its patches.  A stride-2 layer is four launches, one per parity class, each
//                               through its own table of k-steps: the products left out are exact zeros.  The epilogue multiplies by the activation
//                               derivative of the layer below, from its saved bf16 output, and rounds once to bf16.
//   est16_wgrad_kernel          dW[co, (ky, kx, ci)] and db of conv 1-4.  The MFMA's K is the row (env, OUTPUT pixel), cut into slabs of EST16_SLAB rows
//                               (blockIdx.y); blockIdx.x walks tiles of 64 columns (ky, kx, ci | bias).  Both operands are channel last, so a lane's
//                               eight consecutive k are eight different rows: a k-step's 32 rows of D (all C_out) and of the gathered X taps are
//                               staged row-major in LDS (double-buffered, one barrier per step, the next step's global loads in flight) and read back
//                               with the transposed LDS read ds_read_b64_tr_b16, every lane with an in-bounds 8-byte aligned address (tiles are padded,
//                               no lane is masked).  Wave w owns columns 16 w .. 16 w + 15 and one accumulator per 16 output channels.  Conv 1 reads the
//                               fp32 image by time index and rounds at load.  Rows beyond the slab's end are staged as zeros.  Partials are fp32 per
//                               slab in torch's (ci, ky, kx) order with the bias column last: ppo_grad_reduce_kernel reduces them in slab order.
//   est16_pool_backward_kernel  est_pool_backward_kernel on a bf16 map: fp32 window arithmetic, one rounding at the store.
//   est16_retile_kernel         the masters -> the six bf16 forward images (lg_conv_tile_weights_bf16's layout) and bias rows, the bf16 transposed
//                               images of conv 2-4 and the fp32 transposed images of the two linear layers, which hold R(W).
//   est16_expand_kernel         bf16 -> fp32, exact;  est16_round_kernel  fp32 -> bf16, nearest even (lg_estimator_bf16train_backward_stage's deltas).
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
#include "../../include/lgestimator_train_bf16.h"

#define EST16_SLAB 8192             // rows (env, output pixel) per slab of a convolution's weight gradient; a multiple of EST16_KS
#define EST16_KS 32                 // rows per k-step
#define EST16_NCOL 64               // columns (ky, kx, ci | bias) per workgroup

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

LG_DEV bf16x8 est16_zero8() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
  return z;
}

struct Dgrad16 {
  int Hin, Win, Cin, Hout, Wout, Cout, sh, pad, act;       // as DgradLayer
  int py, px, Hc, Wc;
  int nks, nks_w;                                           // this launch's k-steps of 32; k-steps per chunk of the weight image
  const uint16_t* wt;                                       // bf16 [16-column chunk of ci][k / 32][lane][8], k = (ky, kx, co) over ALL taps
  const int32_t* stab;                                      // [nks]: (ky << 26) | (kx << 22) | first co of the step
  const int32_t* wstep;                                     // [nks]: the k-step of the weight image
};

__global__ __launch_bounds__(CONV_THREADS) void est16_dgrad_kernel(Dgrad16 L, const __bf16* __restrict__ D, int64_t d_estride, int64_t n, const __bf16* __restrict__ ysrc,
                                                                    int64_t y_estride, __bf16* __restrict__ out, int64_t out_estride) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4;
  const int HW = L.Hc * L.Wc;
  const int64_t M = n * HW, row0 = (int64_t)blockIdx.x * CONV_ROWS + wv * 16;
  const int64_t ma = row0 + (lane & 15);
  int iyp = -(1 << 20), ixp = 0; int64_t base = 0;          // a row beyond M: no tap reaches an output pixel
  if (ma < M) {
    const int64_t e = ma / HW; const int pix = (int)(ma - e * HW), cy = pix / L.Wc, cx = pix - cy * L.Wc;
    iyp = L.py + (cy << L.sh) + L.pad; ixp = L.px + (cx << L.sh) + L.pad; base = e * d_estride + 8 * g;
  }
  auto load_a = [&](int s) -> bf16x8 {
    const int t = L.stab[s];
    const int ty = iyp - ((t >> 26) & 15), tx = ixp - ((t >> 22) & 15), oy = ty >> L.sh, ox = tx >> L.sh;
    const bool ok = ty >= 0 && tx >= 0 && ((ty | tx) & L.sh) == 0 && oy < L.Hout && ox < L.Wout;
    bf16x8 a = est16_zero8();
    if (ok) a = *reinterpret_cast<const bf16x8*>(D + base + ((int64_t)oy * L.Wout + ox) * L.Cout + (t & 0x3fffff));
    return a;
  };
  const int nch = min(4, (L.Cin - (int)blockIdx.y * CONV_COLS + 15) / 16);          // chunks of this column group that hold a channel (wave uniform)
  const bf16x8* wl = reinterpret_cast<const bf16x8*>(L.wt) + (size_t)blockIdx.y * 4 * L.nks_w * 64 + lane;
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 a = load_a(0), w[4];
  {
    const int ws = L.wstep[0];
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = c < nch ? wl[((size_t)c * L.nks_w + ws) * 64] : est16_zero8();
  }
  for (int s = 0; s < L.nks; ++s) {
    bf16x8 an = a, wn[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) wn[c] = w[c];
    if (s + 1 < L.nks) {
      an = load_a(s + 1);
      const int ws = L.wstep[s + 1];
#pragma unroll
      for (int c = 0; c < 4; ++c) if (c < nch) wn[c] = wl[((size_t)c * L.nks_w + ws) * 64];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nch) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w[c], acc[c], 0, 0, 0);
    a = an;
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = wn[c];
  }
  // epilogue: accumulator entry i of a lane is C[row 4 (lane >> 4) + i][channel lane & 15]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = row0 + 4 * g + i;
    if (m >= M) continue;
    const int64_t e = m / HW; const int cp = (int)(m - e * HW), cy = cp / L.Wc, cx = cp - cy * L.Wc;
    const int pix = (L.py + (cy << L.sh)) * L.Win + L.px + (cx << L.sh);
    __bf16* dst = out + e * out_estride + (int64_t)pix * L.Cin;
    const __bf16* ys = ysrc + e * y_estride + (int64_t)pix * L.Cin;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = blockIdx.y * CONV_COLS + c * 16 + (lane & 15);
      if (col < L.Cin) dst[col] = (__bf16)(acc[c][i] * est_act_grad((float)ys[col], L.act));
    }
  }
}

// dp (n, 16 C) fp32 in torch's flatten order c 16 + i 4 + j; y, d (n, H, W, C) bf16
__global__ __launch_bounds__(256) void est16_pool_backward_kernel(const float* __restrict__ dp, const __bf16* __restrict__ y, int64_t n, int H, int W, int C, int act,
                                                                   __bf16* __restrict__ d) {
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
  d[idx] = (__bf16)(s * est_act_grad((float)y[idx], act));
}

__global__ __launch_bounds__(256) void est16_expand_kernel(const __bf16* __restrict__ x, int64_t count, float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < count) y[idx] = (float)x[idx];
}

__global__ __launch_bounds__(256) void est16_round_kernel(const float* __restrict__ x, int64_t count, __bf16* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < count) y[idx] = (__bf16)x[idx];
}

struct Wgrad16 {
  int Hin, Win, Cin, Hout, Wout, Cout, stride, pad, kh, K;
  const __bf16* D; int64_t d_estride;          // (rows, Hout, Wout, Cout)
  const void* X; int64_t x_estride;            // bf16 (rows, Hin, Win, Cin); conv 1: the fp32 (T, N, h, w) images, row r at time index (t0 + r / N) mod T
  int64_t N, T, t0;
  float* partial;                              // [slab][Cout][K + 1], column (ci kh + ky) kh + kx, the bias last
};

// four rows x 16 columns of a row-major bf16 LDS tile, transposed: lane 4 q + p of a 16-lane group gives the address of row q, columns 4 p .. 4 p + 3,
// and lane i of the group receives column i of the four rows.  EXEC must be all ones: never called under a lane-dependent condition.
LG_DEV bf16x4 est16_tr_read(const __bf16* p) {
  const s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(uint32_t)(uintptr_t)p);
  return __builtin_bit_cast(bf16x4, r);
}

// MT: C_out / 16.  FIRST: conv 1 (C_in = 1: column = tap, X the fp32 image); else C_in % 8 == 0 and K % 8 == 0: a 16-byte chunk of 8 columns lies inside
// one tap (or is the bias column and seven beyond it).  M < 2^31 (checked by the host); the host launches no slab that starts beyond M.
template <int MT, bool FIRST>
__global__ __launch_bounds__(256) void est16_wgrad_kernel(Wgrad16 Wc, uint32_t M) {
  constexpr int DS = MT * 16 + 8, XS = EST16_NCOL + 8;          // row strides in elements: multiples of 8, so 16-byte stores and 8-byte reads stay aligned
  constexpr int DCH = (MT * 2 + 7) / 8;                         // 16-byte chunks of a D row per staging lane
  __shared__ __attribute__((aligned(16))) __bf16 lds[2][EST16_KS * (DS + XS)];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4;
  const uint32_t r0 = blockIdx.y * (uint32_t)EST16_SLAB;
  const uint32_t r1 = M - r0 > (uint32_t)EST16_SLAB ? r0 + EST16_SLAB : M;
  const int col0 = blockIdx.x * EST16_NCOL;
  const uint32_t HW = (uint32_t)(Wc.Hout * Wc.Wout);
  // staging role: row srow of the step, 16-byte chunk sch of the X tile and chunks sch + 8 i of the D tile
  const int srow = tid >> 3, sch = tid & 7;
  const int kc = col0 + 8 * sch;
  const int kind = kc < Wc.K ? 0 : (kc == Wc.K ? 1 : 2);        // FIRST: per column below
  int ky = 0, kx = 0, ci0 = 0;
  if (!FIRST && kind == 0) { const int tap = kc / Wc.Cin; ci0 = kc - tap * Wc.Cin; ky = tap / Wc.kh; kx = tap - ky * Wc.kh; }
  bf16x8 xv, dv[DCH];
  auto load = [&](uint32_t ks) {
    const uint32_t row = ks + srow;
    const bool valid = row < r1;
    const uint32_t e = valid ? row / HW : 0, pix = valid ? row - e * HW : 0;
    const int oy = (int)(pix / (uint32_t)Wc.Wout), ox = (int)pix - oy * Wc.Wout;
#pragma unroll
    for (int i = 0; i < DCH; ++i) {
      const int c = sch + 8 * i;
      dv[i] = est16_zero8();
      if (valid && c * 8 < Wc.Cout) dv[i] = *reinterpret_cast<const bf16x8*>(Wc.D + (int64_t)e * Wc.d_estride + (int64_t)pix * Wc.Cout + 8 * c);
    }
    xv = est16_zero8();
    if (FIRST) {
      if (valid && kc <= Wc.K) {
        const int64_t s = e / Wc.N;
        const float* img = static_cast<const float*>(Wc.X) + (((Wc.t0 + s) % Wc.T) * Wc.N + (e - s * Wc.N)) * Wc.x_estride;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kc + j, qy = k / Wc.kh, qx = k - qy * Wc.kh;
          const int iy = oy * Wc.stride - Wc.pad + qy, ix = ox * Wc.stride - Wc.pad + qx;
          float v = 0.f;
          if (k < Wc.K) { if (iy >= 0 && iy < Wc.Hin && ix >= 0 && ix < Wc.Win) v = img[iy * Wc.Win + ix]; }
          else if (k == Wc.K) v = 1.f;
          xv[j] = (__bf16)v;
        }
      }
    } else if (valid) {
      if (kind == 0) {
        const int iy = oy * Wc.stride - Wc.pad + ky, ix = ox * Wc.stride - Wc.pad + kx;
        if (iy >= 0 && iy < Wc.Hin && ix >= 0 && ix < Wc.Win)
          xv = *reinterpret_cast<const bf16x8*>(static_cast<const __bf16*>(Wc.X) + (int64_t)e * Wc.x_estride + ((int64_t)iy * Wc.Win + ix) * Wc.Cin + ci0);
      } else if (kind == 1) xv[0] = (__bf16)1.f;
    }
  };
  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  // operand role: rows 8 g + 4 r + q of the step, columns 4 p .. 4 p + 3 of the wave's 16 (X) or of output-channel tile m (D)
  const int trow = 8 * g + ((lane & 15) >> 2), tcol = 4 * (lane & 3);
  load(r0);
  for (uint32_t ks = r0, it = 0; ks < r1; ks += EST16_KS, ++it) {
    __bf16* dt = lds[it & 1];
    __bf16* xt = dt + EST16_KS * DS;
#pragma unroll
    for (int i = 0; i < DCH; ++i)
      if ((sch + 8 * i) * 8 < MT * 16) *reinterpret_cast<bf16x8*>(dt + srow * DS + 8 * (sch + 8 * i)) = dv[i];
    *reinterpret_cast<bf16x8*>(xt + srow * XS + 8 * sch) = xv;
    __syncthreads();
    if (ks + EST16_KS < r1) load(ks + EST16_KS);
    const bf16x4 b0 = est16_tr_read(xt + trow * XS + 16 * wv + tcol), b1 = est16_tr_read(xt + (trow + 4) * XS + 16 * wv + tcol);
    const bf16x8 b = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const bf16x4 a0 = est16_tr_read(dt + trow * DS + 16 * m + tcol), a1 = est16_tr_read(dt + (trow + 4) * DS + 16 * m + tcol);
      const bf16x8 a = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[m], 0, 0, 0);
    }
  }
  // accumulator entry t of a lane is C[output channel 16 m + 4 (lane >> 4) + t][column lane & 15]
  const int col = col0 + 16 * wv + (lane & 15);
  if (col > Wc.K) return;
  int tc = Wc.K;
  if (col < Wc.K) { const int tap = col / Wc.Cin, ci = col - tap * Wc.Cin, qy = tap / Wc.kh, qx = tap - qy * Wc.kh; tc = (ci * Wc.kh + qy) * Wc.kh + qx; }
  float* __restrict__ P = Wc.partial + (size_t)blockIdx.y * Wc.Cout * (Wc.K + 1);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < 4; ++t) P[(size_t)(16 * m + 4 * g + t) * (Wc.K + 1) + tc] = acc[m][t];
}

struct Retile16 {
  uint16_t* fw; float* fb; uint16_t* bw; float* bwf;       // bf16 forward image, bias row (C_out padded to 64), bf16 transposed image (conv 2-4), fp32 transposed image (linear)
  int Cout, Cin, kh, nks_f, nch_f, nks_b, nch_b, b_nb;
  int64_t woff, boff;
};

LG_DEV uint16_t est16_bits(float v) { const __bf16 b = (__bf16)v; return __builtin_bit_cast(uint16_t, b); }

__global__ __launch_bounds__(256) void est16_retile_kernel(const Retile16* __restrict__ tab, const float* __restrict__ theta) {
  const Retile16 R = tab[blockIdx.y];
  int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int taps = R.kh * R.kh, K = R.Cin * taps, Kb = R.Cout * taps;
  const int64_t fcount = (int64_t)R.nch_f * R.nks_f * 512, bcount = R.bw ? (int64_t)R.nch_b * R.nks_b * 512 : 0, lcount = R.bwf ? (int64_t)R.Cout * R.Cin : 0;
  if (e < fcount) {          // lg_conv_tile_weights_bf16: [chunk][k / 32][lane][8], column = chunk 16 + (lane & 15), k = step 32 + 8 (lane >> 4) + j, k = (ky, kx, ci)
    const int j = (int)(e & 7), ln = (int)((e >> 3) & 63);
    const int64_t rest = e >> 9;
    const int s = (int)(rest % R.nks_f), c = (int)(rest / R.nks_f);
    const int col = c * 16 + (ln & 15), k = s * 32 + 8 * (ln >> 4) + j;
    uint16_t v = 0;
    if (col < R.Cout && k < K) {
      const int ci = k % R.Cin, tap = k / R.Cin, ky = tap / R.kh, kx = tap - ky * R.kh;
      v = est16_bits(theta[R.woff + (((int64_t)col * R.Cin + ci) * R.kh + ky) * R.kh + kx]);
    }
    R.fw[e] = v;
    return;
  }
  e -= fcount;
  if (e < bcount) {          // the same tiling of the transposed product: column = ci, k = (ky, kx, co)
    const int j = (int)(e & 7), ln = (int)((e >> 3) & 63);
    const int64_t rest = e >> 9;
    const int s = (int)(rest % R.nks_b), c = (int)(rest / R.nks_b);
    const int col = c * 16 + (ln & 15), k = s * 32 + 8 * (ln >> 4) + j;
    uint16_t v = 0;
    if (col < R.Cin && k < Kb) {
      const int co = k % R.Cout, tap = k / R.Cout, ky = tap / R.kh, kx = tap - ky * R.kh;
      v = est16_bits(theta[R.woff + (((int64_t)co * R.Cin + col) * R.kh + ky) * R.kh + kx]);
    }
    R.bw[e] = v;
    return;
  }
  e -= bcount;
  if (e < lcount) {          // ppo_adam_kernel's transposed tiling of a dense layer, holding R(W)
    const int o = (int)(e / R.Cin), i = (int)(e - (int64_t)o * R.Cin);
    R.bwf[((((size_t)(i >> 4) * R.b_nb + (o >> 4)) * 64) + ((i & 15) | ((o & 3) << 4))) * 4 + ((o >> 2) & 3)] = (float)(__bf16)theta[R.woff + e];
    return;
  }
  e -= lcount;
  if (e < ((R.Cout + 63) & ~63)) R.fb[e] = e < R.Cout ? theta[R.boff + e] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------------ host side
struct Est16 {
  __bf16* map[4] = {nullptr, nullptr, nullptr, nullptr};
  __bf16 *pool = nullptr, *y5 = nullptr, *dA = nullptr, *dB = nullptr;
  uint16_t* bwt[4] = {nullptr, nullptr, nullptr, nullptr};          // the bf16 transposed images of conv 2-4 (index 0 unused)
  Dgrad16 dg[4][4];                                                 // dg[l][parity class]: conv l + 1
  Retile16* d_tab = nullptr; int64_t retile_big = 0;
};

int32_t est16_slab_rows() { return EST16_SLAB; }

static const int kWgradMT[4] = {2, 4, 8, 4};          // the weight gradient's instance of conv 1-4: est16_wgrad_kernel<C_out / 16>

void est16_free(lg_estimator_train* p) {
  if (!p || !p->b16) return;
  delete p->b16;          // the device memory is the core's (train_alloc)
  p->b16 = nullptr;
}

static const int32_t* est16_upload_table(lg_estimator_train* p, const std::vector<int32_t>& t) {
  int32_t* d = (int32_t*)train_alloc(p, t.size() * sizeof(int32_t), false);
  if (d && hipMemcpy(d, t.data(), t.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { lg_policy_fail(LG_ERR_HIP, "table upload failed"); return nullptr; }
  return d;
}

bool est16_setup(lg_estimator_train* p, float* bw10, float* bw12) {
  Est16* B = p->b16 = new Est16();
  lg_conv_encoder* enc = p->enc;
  const size_t R = (size_t)p->max_rows;
  // what the kernels assume of conv 1-4: C_out = 16 MT of the layer's weight-gradient instance; behind conv 1 a k-step of 32 output channels lies inside
  // one tap of the data gradient and a 16-byte chunk of 8 input channels inside one tap of the weight gradient
  for (int l = 0; l < 4; ++l) {
    const ConvLayerDev& C = enc->layer[l];
    if (C.Cout != 16 * kWgradMT[l] || (l == 0 ? C.Cin != 1 : (C.Cout % 32 != 0 || C.Cin % 8 != 0))) {
      lg_policy_fail(LG_ERR_UNSUPPORTED, "the encoder's convolution widths are not the ones the bf16 gradient kernels are built for");
      return false;
    }
  }
  bool ok = true;
  auto alloc16 = [&](size_t elems, bool zero) -> __bf16* { __bf16* d = ok ? (__bf16*)train_alloc(p, elems * 2, zero) : nullptr; if (!d) ok = false; return d; };
  for (int l = 0; l < 4; ++l) B->map[l] = alloc16(R * p->map_floats[l], false);
  B->pool = alloc16(R * 1024, false); B->y5 = alloc16(R * 128, false);
  B->dA = alloc16(R * std::max(p->map_floats[0], p->map_floats[2]), false); B->dB = alloc16(R * std::max(p->map_floats[1], p->map_floats[3]), false);
  std::vector<Retile16> tab(ENC_LAYERS);
  for (int l = 0; l < ENC_LAYERS && ok; ++l) {
    const ConvLayerDev& C = enc->layer[l];
    const int kh = l < 4 ? kConvShape[l][2] : 1;
    const TrainSeg& S = l < 4 ? p->seg[p->nd + l] : p->seg[p->seg_l10 + (l - 4)];
    Retile16& r = tab[l];
    r.fw = const_cast<uint16_t*>(C.w16); r.fb = const_cast<float*>(C.b); r.bw = nullptr; r.bwf = l == 4 ? bw10 : l == 5 ? bw12 : nullptr;
    r.Cout = C.Cout; r.Cin = C.Cin; r.kh = kh; r.nks_f = C.nkb; r.nch_f = ((C.Cout + 63) & ~63) / 16;
    r.nks_b = kh * kh * C.Cout / 32; r.nch_b = ((C.Cin + 63) & ~63) / 16; r.b_nb = ((C.Cout + 63) & ~63) / 16;
    r.woff = S.woff; r.boff = S.boff;
    if (l > 0 && l < 4) r.bw = B->bwt[l] = (uint16_t*)alloc16((size_t)r.nch_b * r.nks_b * 512, true);
    const int64_t cnt = (int64_t)r.nch_f * r.nks_f * 512 + (r.bw ? (int64_t)r.nch_b * r.nks_b * 512 : 0) + (r.bwf ? (int64_t)C.Cout * C.Cin : 0) + ((C.Cout + 63) & ~63);
    if (cnt > B->retile_big) B->retile_big = cnt;
  }
  B->d_tab = ok ? (Retile16*)train_alloc(p, sizeof(Retile16) * ENC_LAYERS, true) : nullptr;
  if (!B->d_tab || hipMemcpy(B->d_tab, tab.data(), sizeof(Retile16) * ENC_LAYERS, hipMemcpyHostToDevice) != hipSuccess) {
    if (B->d_tab) lg_policy_fail(LG_ERR_HIP, "table upload failed");
    return false;
  }
  // the data-gradient launches of conv 2-4: per parity class, the k-steps (ky, kx, 32 co) whose tap can reach an output pixel
  for (int l = 1; l < 4; ++l) {
    const ConvLayerDev& C = enc->layer[l];
    const int kh = kConvShape[l][2];
    for (int cls = 0; cls < 4; ++cls) {
      Dgrad16& G = B->dg[l][cls];
      G = Dgrad16{};
      if (C.stride == 1 && cls > 0) continue;          // Hc = 0: never launched
      G.Hin = C.Hin; G.Win = C.Win; G.Cin = C.Cin; G.Hout = C.Hout; G.Wout = C.Wout; G.Cout = C.Cout; G.sh = C.stride - 1; G.pad = C.pad; G.act = p->act;
      G.py = cls >> 1; G.px = cls & 1;
      G.Hc = (C.Hin - G.py + C.stride - 1) / C.stride; G.Wc = (C.Win - G.px + C.stride - 1) / C.stride;
      G.nks_w = kh * kh * C.Cout / 32; G.wt = B->bwt[l];
      std::vector<int32_t> st, ws;
      for (int ky = 0; ky < kh; ++ky)
        for (int kx = 0; kx < kh; ++kx) {
          if (C.stride == 2 && ((((G.py + G.pad - ky) & 1) != 0) || (((G.px + G.pad - kx) & 1) != 0))) continue;
          for (int co = 0; co < C.Cout; co += 32) { st.push_back((ky << 26) | (kx << 22) | co); ws.push_back(((ky * kh + kx) * C.Cout + co) / 32); }
        }
      if (st.empty()) { G.Hc = 0; continue; }
      G.nks = (int)st.size();
      G.stab = est16_upload_table(p, st);
      G.wstep = G.stab ? est16_upload_table(p, ws) : nullptr;
      if (!G.wstep) return false;
    }
  }
  return true;
}

void est16_retile(lg_estimator_train* p, hipStream_t st) {
  Est16* B = p->b16;
  hipLaunchKernelGGL(est16_retile_kernel, dim3((unsigned)((B->retile_big + 255) / 256), ENC_LAYERS), dim3(256), 0, st, (const Retile16*)B->d_tab, (const float*)p->theta);
}

static void est16_expand(const __bf16* x, int64_t count, float* y, hipStream_t st) {
  hipLaunchKernelGGL(est16_expand_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, x, count, y);
}

int est16_forward(lg_estimator_train* p, const float* depth, int64_t depth_stride, int64_t n, int64_t at, hipStream_t st) {
  Est16* B = p->b16;
  void* maps[7] = {B->map[0] + at * p->map_floats[0], B->map[1] + at * p->map_floats[1], B->map[2] + at * p->map_floats[2], B->map[3] + at * p->map_floats[3],
                   B->pool + at * 1024, B->y5 + at * 128, p->cat + at * p->cat_w};
  const int64_t strides[7] = {p->map_floats[0], p->map_floats[1], p->map_floats[2], p->map_floats[3], 1024, 128, p->cat_w};
  const int rc = enc_forward_saved_bf16(p->enc, depth, depth_stride, n, maps, strides, st);
  if (rc != LG_OK) return rc;
  // what the fp32 backward kernels of the two linear layers read
  est16_expand(B->pool + at * 1024, n * 1024, p->pool + at * 1024, st);
  est16_expand(B->y5 + at * 128, n * 128, p->y5 + at * 128, st);
  return LG_OK;
}

static void est16_launch_dgrad(const Dgrad16& L, const __bf16* D, int64_t d_estride, int64_t n, const __bf16* ysrc, int64_t y_estride, __bf16* out, int64_t out_estride,
                               hipStream_t st) {
  if (L.Hc < 1 || L.Wc < 1) return;
  const int64_t tiles = (n * L.Hc * L.Wc + CONV_ROWS - 1) / CONV_ROWS;
  hipLaunchKernelGGL(est16_dgrad_kernel, dim3((unsigned)tiles, (unsigned)((L.Cin + CONV_COLS - 1) / CONV_COLS)), dim3(CONV_THREADS), 0, st, L, D, d_estride, n, ysrc, y_estride,
                     out, out_estride);
}

// conv l (0-based): D (n, Hout, Wout, Cout) bf16, X its input maps (conv 1: the fp32 images); returns the number of slabs
static int est16_launch_wgrad(lg_estimator_train* p, int l, const __bf16* D, const void* X, int64_t x_estride, int64_t n, int64_t N, int64_t T, int64_t t0, hipStream_t st) {
  const ConvLayerDev& C = p->enc->layer[l];
  Wgrad16 W;
  W.Hin = C.Hin; W.Win = C.Win; W.Cin = C.Cin; W.Hout = C.Hout; W.Wout = C.Wout; W.Cout = C.Cout; W.stride = C.stride; W.pad = C.pad; W.kh = kConvShape[l][2];
  W.K = C.Cin * W.kh * W.kh;
  W.D = D; W.d_estride = (int64_t)C.Hout * C.Wout * C.Cout; W.X = X; W.x_estride = x_estride; W.N = N; W.T = T; W.t0 = t0; W.partial = p->seg[p->nd + l].partial;
  const int64_t M = n * C.Hout * C.Wout;
  const int nslabs = (int)((M + EST16_SLAB - 1) / EST16_SLAB);
  const dim3 grid((unsigned)((W.K + 1 + EST16_NCOL - 1) / EST16_NCOL), (unsigned)nslabs), block(256);
  if (l == 0) hipLaunchKernelGGL((est16_wgrad_kernel<2, true>), grid, block, 0, st, W, (uint32_t)M);                          // C_out = 16 MT: checked by est16_setup
  else if (kWgradMT[l] == 8) hipLaunchKernelGGL((est16_wgrad_kernel<8, false>), grid, block, 0, st, W, (uint32_t)M);
  else hipLaunchKernelGGL((est16_wgrad_kernel<4, false>), grid, block, 0, st, W, (uint32_t)M);
  return nslabs;
}

static void est16_pool_backward(lg_estimator_train* p, const float* dpool, int64_t n, hipStream_t st) {
  const ConvLayerDev& C = p->enc->layer[3];
  hipLaunchKernelGGL(est16_pool_backward_kernel, dim3((unsigned)((n * p->map_floats[3] + 255) / 256)), dim3(256), 0, st, dpool, (const __bf16*)p->b16->map[3], n, C.Hout, C.Wout,
                     64, p->act, p->b16->dB);
}

// the delta buffers ping-pong as the fp32 path's: conv 4's and conv 2's deltas in dB, conv 3's and conv 1's in dA
static void est16_dgrad_conv(lg_estimator_train* p, int l, int64_t n, hipStream_t st) {
  Est16* B = p->b16;
  const __bf16* D = (l & 1) ? B->dB : B->dA;
  __bf16* out = (l & 1) ? B->dA : B->dB;
  for (int k = 0; k < 4; ++k) est16_launch_dgrad(B->dg[l][k], D, p->map_floats[l], n, B->map[l - 1], p->map_floats[l - 1], out, p->map_floats[l - 1], st);
}

void est16_backward(lg_estimator_train* p, const float* depth, int64_t n, int64_t N, int64_t T, int64_t t0, int* cslabs, hipStream_t st) {
  Est16* B = p->b16;
  const int hw = p->enc->H * p->enc->W;
  est16_pool_backward(p, p->dpool, n, st);
  cslabs[3] = est16_launch_wgrad(p, 3, B->dB, B->map[2], p->map_floats[2], n, N, 0, 0, st);
  est16_dgrad_conv(p, 3, n, st);
  cslabs[2] = est16_launch_wgrad(p, 2, B->dA, B->map[1], p->map_floats[1], n, N, 0, 0, st);
  est16_dgrad_conv(p, 2, n, st);
  cslabs[1] = est16_launch_wgrad(p, 1, B->dB, B->map[0], p->map_floats[0], n, N, 0, 0, st);
  est16_dgrad_conv(p, 1, n, st);
  cslabs[0] = est16_launch_wgrad(p, 0, B->dA, depth, hw, n, N, T, t0, st);
}

extern "C" {

int32_t lg_estimator_bf16train_wgrad_slab_rows(void) { return EST16_SLAB; }

lg_estimator_train* lg_estimator_bf16train_create(lg_conv_encoder* enc, lg_mlp* combine, lg_rnn* mem, lg_mlp* decoder, const lg_estimator_train_params* q, double learning_rate,
                                                  int64_t max_rows) {
  POLICY_ENTRY;
  if (enc && enc->prec != LG_PREC_BF16) {
    lg_policy_fail(LG_ERR_UNSUPPORTED, "the encoder is fp32 (LG_PREC_F32): lg_estimator_train_create trains it; this entry trains an LG_PREC_BF16 encoder");
    return nullptr;
  }
  return est_train_create(enc, combine, mem, decoder, q, learning_rate, max_rows, true);
}

int lg_estimator_bf16train_saved_stage(lg_estimator_train* p, int32_t k, float* out, int64_t capacity, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!p->b16) return lg_policy_fail(LG_ERR_INVALID, "an fp32 trainer saves fp32 maps: this entry reads a trainer of lg_estimator_bf16train_create");
  if (k < 1 || k > 6) return lg_policy_fail(LG_ERR_INVALID, "stage outside 1..6");
  if (!out) return lg_policy_fail(LG_ERR_INVALID, "null output");
  if (p->last_rows < 1) return lg_policy_fail(LG_ERR_INVALID, "no group call yet");
  const int64_t per = k <= 4 ? p->map_floats[k - 1] : k == 5 ? 1024 : 128, count = p->last_rows * per;
  if (capacity < count) return lg_policy_fail(LG_ERR_INVALID, "capacity is smaller than rows x the stage's width");
  DeviceScope ds_(p->device);
  Est16* B = p->b16;
  est16_expand(k <= 4 ? B->map[k - 1] : k == 5 ? B->pool : B->y5, count, out, (hipStream_t)stream);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_estimator_bf16train_backward_stage(lg_estimator_train* p, int32_t stage, const float* delta_in, int64_t rows, float* delta_out, float* wgrad_out, void* stream) {
  POLICY_ENTRY;
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!p->b16) return lg_policy_fail(LG_ERR_INVALID, "an fp32 trainer: this entry runs the stages of a trainer of lg_estimator_bf16train_create");
  if (stage < LG_EST16_POOL_BACKWARD || stage > LG_EST16_LINEAR1) return lg_policy_fail(LG_ERR_INVALID, "unknown stage");
  if (!delta_in) return lg_policy_fail(LG_ERR_INVALID, "null delta");
  if (p->last_rows < 1 || rows != p->last_rows) return lg_policy_fail(LG_ERR_INVALID, "rows are not the last group call's");
  DeviceScope ds_(p->device);
  hipStream_t st = (hipStream_t)stream;
  Est16* B = p->b16;
  const int64_t n = rows;
  auto round_in = [&](__bf16* dst, int64_t count) { hipLaunchKernelGGL(est16_round_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, delta_in, count, dst); };
  // the reduced gradient of segment s: dW then db, torch's layout
  auto grad_out = [&](int s, int nslabs) -> int {
    train_launch_reduce_range(p, s, 1, nslabs, st);
    if (!wgrad_out) return LG_OK;
    const TrainSeg& S = p->seg[s];
    POLICY_TRY(hipMemcpyAsync(wgrad_out, p->G + S.woff, (size_t)S.dO * S.dI * sizeof(float), hipMemcpyDeviceToDevice, st));
    POLICY_TRY(hipMemcpyAsync(wgrad_out + (int64_t)S.dO * S.dI, p->G + S.boff, (size_t)S.dO * sizeof(float), hipMemcpyDeviceToDevice, st));
    return LG_OK;
  };
  int rc = LG_OK;
  if (stage == LG_EST16_POOL_BACKWARD) {
    est16_pool_backward(p, delta_in, n, st);
    if (delta_out) est16_expand(B->dB, n * p->map_floats[3], delta_out, st);
  } else if (stage <= LG_EST16_DGRAD_CONV2) {
    const int l = 4 - stage;                                   // conv l + 1: 3, 2, 1
    round_in((l & 1) ? B->dB : B->dA, n * p->map_floats[l]);
    est16_dgrad_conv(p, l, n, st);
    if (delta_out) est16_expand((l & 1) ? B->dA : B->dB, n * p->map_floats[l - 1], delta_out, st);
  } else if (stage <= LG_EST16_WGRAD_CONV1) {
    const int l = LG_EST16_WGRAD_CONV1 - stage;                // 3, 2, 1, 0
    __bf16* D = (l & 1) ? B->dB : B->dA;
    round_in(D, n * p->map_floats[l]);
    const int nslabs = l == 0 ? est16_launch_wgrad(p, 0, D, p->last_depth, (int64_t)p->enc->H * p->enc->W, n, p->last_N, p->last_T, p->last_t0, st)
                              : est16_launch_wgrad(p, l, D, B->map[l - 1], p->map_floats[l - 1], n, p->last_N, 0, 0, st);
    rc = grad_out(p->nd + l, nslabs);
  } else {
    const bool l12 = stage == LG_EST16_LINEAR2;
    const int s = p->seg_l10 + (l12 ? 1 : 0);
    float* D = l12 ? p->d6 : p->d5;                            // the segment's delta rows
    POLICY_TRY(hipMemcpyAsync(D, delta_in, (size_t)n * p->seg[s].dO * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (l12) est_launch_dgrad(p->dg_l12, p->d6, p->F, n, p->y5, 128, p->d5, 128, st);
    else est_launch_dgrad(p->dg_l10, p->d5, 128, n, nullptr, 0, p->dpool, 1024, st);
    if (delta_out) POLICY_TRY(hipMemcpyAsync(delta_out, l12 ? p->d5 : p->dpool, (size_t)n * (l12 ? 128 : 1024) * sizeof(float), hipMemcpyDeviceToDevice, st));
    train_launch_wgrad_range(p, s, 1, nullptr, nullptr, nullptr, n, st);
    rc = grad_out(s, (int)((n + WGRAD_SLAB - 1) / WGRAD_SLAB));
  }
  if (rc != LG_OK) return rc;
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

}  // extern "C"
