// lg_policy.hip — gfx950 kernels for the rollout-collection side of PPO (include/lgpolicy.h): fused MLP forward on the
// fp32 matrix cores, PPO.act (both networks + Gaussian sampling + log-prob) in one launch, GAE returns; further down the planner's
// arithmetic and the LSTM / GRU memory of the recurrent actor-critic (one launch per memory layer).
//
// MLP kernel.  Workgroup = 8 waves = 32 rows of the batch through ALL layers.  The activations of the current layer live in LDS
// in an image a lane reads with ONE ds_read_b128 per four k-steps: [k/16][row][k%4][(k/4)%4] -- the four values a lane feeds to
// four successive v_mfma_f32_16x16x4_f32 (A operand: lane = (row, k%4)) are adjacent, and the 64 lanes of a wave read 1 KB
// contiguous (conflict-free).  The next layer's image is written to a second LDS buffer by the epilogue (bias + activation on the
// accumulator fragments).  Weights are re-tiled once on the host the same way ([16-column chunk][k/16][lane][(k/4)%4]): one
// coalesced global_load_dwordx4 per wave and eight MFMAs.  Each wave owns every eighth 16-column chunk of a layer and keeps two
// independent accumulators (rows 0-15 and 16-31), which is what the 16x16x4 instruction needs to issue back to back.
// Exact fp32: the MFMA is a k-ordered fmaf chain.
//
// Why 16-byte operand loads and two waves per SIMD (tools/micro/mfma_loop.hip, measured on MI355X): data returning from a global
// load holds the matrix pipe of that SIMD for ~16 cycles per VGPR written and a ds_read for ~4-14, whatever the wave does
// meanwhile -- a two-chain MFMA loop at 36 cycles per MFMA runs at 54 with one global_load_dword + one ds_read2_b32 per MFMA pair
// (the round-1 loop: 80 us for the 235-512-256-128 pair at 4096 rows), at 46 with one dwordx4 + two b128 per eight MFMAs, and at
// 41 with a second wave on the SIMD to fill the gaps.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_rnn_tile.h"
#include "lg_switches.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgrunner.h"
#include "../../include/lgrunner_privileged.h"
#include "../../include/lgstep.h"

// ---- the one error channel and the create functions' plumbing (lg_policy_internal.h)
thread_local const char* lg_policy_entry = nullptr;
static thread_local std::string g_pol_err;

int lg_policy_device_of(const void* p) {
  hipPointerAttribute_t pa;
  return hipPointerGetAttributes(&pa, p) == hipSuccess ? pa.device : -1;
}

int lg_policy_fail(int status, const std::string& what) {
  g_pol_err = std::string(lg_policy_entry ? lg_policy_entry : "lg_policy") + ": " + what;
  return status;
}

bool lg_policy_device_ok(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { lg_policy_fail(LG_ERR_HIP, "no HIP device: these kernels have no CPU path"); return false; }
  if (device_id < 0 || device_id >= ndev) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return false; }
  return true;
}

const void* lg_policy_upload(const void* host, size_t bytes, std::vector<void*>& allocs) {
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) { lg_policy_fail(LG_ERR_HIP, "weight upload failed"); return nullptr; }
  allocs.push_back(d);
  if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) { lg_policy_fail(LG_ERR_HIP, "weight upload failed"); return nullptr; }
  return d;
}

// stage an input tile: columns [k0, k0 + Kp) of 32 rows of x (n, K0) row-major -> activation image of padded width Kp (zeros past column K0 and
// past row n).  Eight independent loads in flight per lane.
LG_DEV void mlp_stage(const float* __restrict__ x, int K0, int k0, int Kp, int64_t row0, int64_t n, float* img) {
  const int tid = threadIdx.x;
  for (int base = 0; base < MLP_ROWS * Kp; base += 8 * MLP_THREADS) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * MLP_THREADS + tid, r = idx / Kp, k = idx - r * Kp;
      const int64_t row = row0 + r;
      v[u] = (idx < MLP_ROWS * Kp && row < n && k0 + k < K0) ? x[row * K0 + k0 + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * MLP_THREADS + tid, r = idx / Kp, k = idx - r * Kp;
      if (idx < MLP_ROWS * Kp) img[IMG(r, k)] = v[u];
    }
  }
}

// volatile asm keeps the two accumulator chains interleaved as written (the compiler otherwise issues the dependent MFMAs of one
// accumulator back to back: 40-cycle dependent latency instead of the 32-cycle issue rate)
#define MFMA_IN_ORDER(ACC, A, B) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(ACC) : "v"(A), "v"(B))
// One block = 16 inputs = four k-steps = eight MFMAs on the fragments (W, A0, A1), in ascending k.  The fragments of the block
// TWO ahead (of this chunk, or of the wave's next chunk) are requested in the middle of the block: sched_barrier pins the order,
// the compiler's s_waitcnt before a block's first MFMA then only waits for loads issued sixteen MFMAs earlier.
#define MLP_BLOCK(W, A0, A1, NW, NA0, NA1, WN, AN)                                                            \
      {                                                                                                       \
        MFMA_IN_ORDER(acc0, A0.x, W.x); MFMA_IN_ORDER(acc1, A1.x, W.x);                                       \
        MFMA_IN_ORDER(acc0, A0.y, W.y); MFMA_IN_ORDER(acc1, A1.y, W.y);                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        NW = *(WN); NA0 = *(AN); NA1 = (AN)[64];                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        MFMA_IN_ORDER(acc0, A0.z, W.z); MFMA_IN_ORDER(acc1, A1.z, W.z);                                       \
        MFMA_IN_ORDER(acc0, A0.w, W.w); MFMA_IN_ORDER(acc1, A1.w, W.w);                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
      }

// Layer 0 of a network whose input row is wider than one activation image (kpad[0] > MLP_MAXW; lg_mlp_create_wide): split-K.  The row is staged
// into `img` in slabs of MLP_MAXW columns (the last one padded to 64 as any input is), and between slabs the workgroup barriers and restages.  A wave
// keeps the accumulators of ALL its chunks (at most MLP_WIDE_CHUNKS, both row halves) live across the slabs, so every output element is still ONE
// k-ascending MFMA chain from zero, the chain of the one-slab path: the result does not depend on where the slabs are cut, and columns whose weights
// are zero change no bit.  Bias and activation follow the last slab; nothing is summed through LDS or memory.  Ends as a layer of mlp_tile ends:
// the next layer's image in `out` (or the rows in `yrows` / `y_global` when the network has one layer), and a barrier.
#define MLP_WIDE_CHUNKS (MLP_MAXW / 16 / (MLP_THREADS / 64))
LG_DEV void mlp_wide_first_layer(const MlpDev& M, const float* __restrict__ x, int64_t row0, int64_t n, float* img, float* out, float* yrows,
                                 float* __restrict__ y_global) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K0 = M.dims[0], K0p = M.kpad[0], nblk0 = K0p >> 4, nch = M.nchunks[0], nout = M.dims[1];
  const bool last = M.L == 1;
  const float4* ap = reinterpret_cast<const float4*>(img) + (lane & 15) * 4 + (lane >> 4);
  const float4* wl = reinterpret_cast<const float4*>(M.w[0]) + lane;
  f32x4 acc[MLP_WIDE_CHUNKS][2];
#pragma unroll
  for (int ci = 0; ci < MLP_WIDE_CHUNKS; ++ci) { acc[ci][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[ci][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int k0 = 0; k0 < K0p; k0 += MLP_MAXW) {
    const int Kp = K0p - k0 < MLP_MAXW ? K0p - k0 : MLP_MAXW, nblk = Kp >> 4;       // a multiple of 64 columns = of 4 blocks
    if (k0) lds_barrier();                                                            // every wave has read the slab before
    mlp_stage(x, K0, k0, Kp, row0, n, img);
    lds_barrier();
    const float4* ws = wl + (size_t)(k0 >> 4) * 64;                                   // the slab's first block within a chunk
    float4 w0, w1, w2, w3, p0, p1, p2, p3, q0, q1, q2, q3;
    if (wv < nch) {
      const float4* wc = ws + (size_t)wv * nblk0 * 64;
      w0 = wc[0]; p0 = ap[0]; q0 = ap[64];
      w1 = wc[64]; p1 = ap[128]; q1 = ap[128 + 64];
    }
#pragma unroll
    for (int ci = 0; ci < MLP_WIDE_CHUNKS; ++ci) {
      const int c = wv + ci * (MLP_THREADS / 64);
      if (c < nch) {
        f32x4 acc0 = acc[ci][0], acc1 = acc[ci][1];
        const float4* wc = ws + (size_t)c * nblk0 * 64;
        const int cn = c + MLP_THREADS / 64 < nch ? c + MLP_THREADS / 64 : c;         // the wave's last chunk re-reads its own first blocks
        const float4* wnext = ws + (size_t)cn * nblk0 * 64;
        for (int kb = 0; kb < nblk; kb += 4) {
          const bool more = kb + 4 < nblk;
          MLP_BLOCK(w0, p0, q0, w2, p2, q2, wc + (size_t)(kb + 2) * 64, ap + (kb + 2) * 128)
          MLP_BLOCK(w1, p1, q1, w3, p3, q3, wc + (size_t)(kb + 3) * 64, ap + (kb + 3) * 128)
          MLP_BLOCK(w2, p2, q2, w0, p0, q0, more ? wc + (size_t)(kb + 4) * 64 : wnext, more ? ap + (kb + 4) * 128 : ap)
          MLP_BLOCK(w3, p3, q3, w1, p1, q1, more ? wc + (size_t)(kb + 5) * 64 : wnext + 64, more ? ap + (kb + 5) * 128 : ap + 128)
        }
        // as in mlp_tile: the last MFMA's result latency, before anything the compiler schedules touches the accumulators
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
        acc[ci][0] = acc0; acc[ci][1] = acc1;
      }
    }
  }
#pragma unroll
  for (int ci = 0; ci < MLP_WIDE_CHUNKS; ++ci) {
    const int c = wv + ci * (MLP_THREADS / 64);
    if (c < nch) {
      const int col = c * 16 + (lane & 15);
      const float bias = M.b[0][col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * (lane >> 4) + i;
        float v0 = acc[ci][0][i] + bias, v1 = acc[ci][1][i] + bias;
        if (!last) {
          v0 = apply_act(v0, M.act); v1 = apply_act(v1, M.act);
          if (col >= nout) { v0 = 0.f; v1 = 0.f; }
          out[IMG(m, col)] = v0;
          out[IMG(m + 16, col)] = v1;
        } else if (col < nout) {
          if (M.act_out) { v0 = apply_act(v0, M.act); v1 = apply_act(v1, M.act); }
          if (yrows) { yrows[m * 16 * nch + col] = v0; yrows[(m + 16) * 16 * nch + col] = v1; }
          if (y_global) {
            if (row0 + m < n) y_global[(row0 + m) * nout + col] = v0;
            if (row0 + m + 16 < n) y_global[(row0 + m + 16) * nout + col] = v1;
          }
        }
      }
    }
  }
  lds_barrier();
}

// 32 rows of x through the whole network; result rows (width dims[L], <= 16 * nchunks) left in `yrows` / written to `y_global`.  WIDE: the instance
// that also takes networks with more than MLP_MAXW inputs (a narrow network in the same launch runs the loop below from layer 0, as in the
// narrow instance).
template <bool WIDE>
LG_DEV void mlp_tile(const MlpDev& M, const float* __restrict__ x, int64_t row0, int64_t n, float* buf0, float* buf1, float* yrows /* [32][16*?] */,
                     float* __restrict__ y_global) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* in = buf0; float* out = buf1;
  int l0 = 0;
  if (WIDE && M.kpad[0] > MLP_MAXW) {
    mlp_wide_first_layer(M, x, row0, n, buf0, buf1, yrows, y_global);
    in = buf1; out = buf0; l0 = 1;
  } else {
    mlp_stage(x, M.dims[0], 0, M.kpad[0], row0, n, buf0);
    lds_barrier();
  }
  for (int l = l0; l < M.L; ++l) {
    const int nblk = M.kpad[l] >> 4, nch = M.nchunks[l];          // blocks of 16 inputs per chunk: a multiple of 4
    const bool last = l == M.L - 1;
    const int nout = M.dims[l + 1];
    // A fragments: lane (row = lane & 15, k%4 = lane >> 4) reads float4 (block * 32 + row) * 4 + k%4: the wave covers 64 consecutive
    // float4 of the block; rows 16-31 sit 64 float4 further
    const float4* ap = reinterpret_cast<const float4*>(in) + (lane & 15) * 4 + (lane >> 4);
    const float4* wl = reinterpret_cast<const float4*>(M.w[l]) + lane;
    float4 w0, w1, w2, w3, p0, p1, p2, p3, q0, q1, q2, q3;     // four rotating fragment sets (weights, rows 0-15, rows 16-31)
    if (wv < nch) {
      const float4* wc = wl + (size_t)wv * nblk * 64;
      w0 = wc[0]; p0 = ap[0]; q0 = ap[64];
      w1 = wc[64]; p1 = ap[128]; q1 = ap[128 + 64];
    }
    for (int c = wv; c < nch; c += MLP_THREADS / 64) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const float4* wc = wl + (size_t)c * nblk * 64;
      const int cn = c + MLP_THREADS / 64 < nch ? c + MLP_THREADS / 64 : c;           // the wave's last chunk re-reads its own first blocks
      const float4* wnext = wl + (size_t)cn * nblk * 64;
      const int col = c * 16 + (lane & 15);
      const float bias = M.b[l][col];
      for (int kb = 0; kb < nblk; kb += 4) {
        const bool more = kb + 4 < nblk;
        MLP_BLOCK(w0, p0, q0, w2, p2, q2, wc + (size_t)(kb + 2) * 64, ap + (kb + 2) * 128)
        MLP_BLOCK(w1, p1, q1, w3, p3, q3, wc + (size_t)(kb + 3) * 64, ap + (kb + 3) * 128)
        MLP_BLOCK(w2, p2, q2, w0, p0, q0, more ? wc + (size_t)(kb + 4) * 64 : wnext, more ? ap + (kb + 4) * 128 : ap)
        MLP_BLOCK(w3, p3, q3, w1, p1, q1, more ? wc + (size_t)(kb + 5) * 64 : wnext + 64, more ? ap + (kb + 5) * 128 : ap + 128)
      }
      // the MFMAs above are opaque to the compiler's hazard recogniser: give the last one its result latency before the
      // accumulators are read by the epilogue
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
      // epilogue: C[m = 4 * (lane >> 4) + i][col = lane & 15]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * (lane >> 4) + i;
        float v0 = acc0[i] + bias, v1 = acc1[i] + bias;
        if (!last) {
          v0 = apply_act(v0, M.act); v1 = apply_act(v1, M.act);
          if (col >= nout) { v0 = 0.f; v1 = 0.f; }                 // padded columns feed zeros to the next layer
          out[IMG(m, col)] = v0;
          out[IMG(m + 16, col)] = v1;
        } else if (col < nout) {
          if (M.act_out) { v0 = apply_act(v0, M.act); v1 = apply_act(v1, M.act); }
          if (yrows) { yrows[m * 16 * nch + col] = v0; yrows[(m + 16) * 16 * nch + col] = v1; }
          if (y_global) {
            if (row0 + m < n) y_global[(row0 + m) * nout + col] = v0;
            if (row0 + m + 16 < n) y_global[(row0 + m + 16) * nout + col] = v1;
          }
        }
      }
    }
    lds_barrier();
    float* t = in; in = out; out = t;
  }
#undef MLP_BLOCK
}

__global__ __launch_bounds__(MLP_THREADS) void mlp_forward_kernel(MlpDev M, const float* __restrict__ x, int64_t n, float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float buf0[MLP_IMG];
  __shared__ __attribute__((aligned(16))) float buf1[MLP_IMG];
  mlp_tile<false>(M, x, (int64_t)blockIdx.x * MLP_ROWS, n, buf0, buf1, nullptr, y);
}

// The *_wide_* kernels (this one and the two acts below) are the WIDE instances of the same bodies, for launches in which a network has more than
// MLP_MAXW inputs; the host picks them from the handles (mlp_is_wide), and every other launch takes the kernels above, unchanged.
__global__ __launch_bounds__(MLP_THREADS) void mlp_wide_forward_kernel(MlpDev M, const float* __restrict__ x, int64_t n, float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float buf0[MLP_IMG];
  __shared__ __attribute__((aligned(16))) float buf1[MLP_IMG];
  mlp_tile<true>(M, x, (int64_t)blockIdx.x * MLP_ROWS, n, buf0, buf1, nullptr, y);
}

// PPO.act: blockIdx.y = 0 actor (+ sampling, log-prob), 1 critic.  LOGP = false is Distillation.act (lg_distill_act): the second network is the teacher
// (its whole output row goes to `values`), and no log-prob is kept (distillation.py:89-96 stores none).
template <bool LOGP, bool WIDE>
LG_DEV void policy_act_body(const MlpDev& A, const MlpDev& Cr, const float* __restrict__ obs, const float* __restrict__ cobs, int64_t n,
                            const float* __restrict__ stdv, uint32_t seed_lo, uint32_t seed_hi, uint32_t call_lo, uint32_t call_hi, int deterministic,
                            float* __restrict__ actions, float* __restrict__ mean, float* __restrict__ logp, float* __restrict__ values) {
  __shared__ __attribute__((aligned(16))) float buf0[MLP_IMG];
  __shared__ __attribute__((aligned(16))) float buf1[MLP_IMG];
  __shared__ float yrows[MLP_ROWS * 16 * 2];       // output rows of the actor (<= 32 actions)
  __shared__ float lp[LOGP ? MLP_ROWS : 1][32];
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  if (blockIdx.y == 1) { mlp_tile<WIDE>(Cr, cobs, row0, n, buf0, buf1, nullptr, values); return; }
  const int na = A.dims[A.L], stride = 16 * A.nchunks[A.L - 1];
  mlp_tile<WIDE>(A, obs, row0, n, buf0, buf1, yrows, mean);
  // one lane per (row, action): z from Philox + Box-Muller, two normals per counter word pair
  const int tid = threadIdx.x;
  for (int idx = tid; idx < MLP_ROWS * 32; idx += MLP_THREADS) {
    const int r = idx >> 5, a = idx & 31;
    float term = 0.f;
    if (a < na && row0 + r < n) {
      const float mu = yrows[r * stride + a], sd = stdv[a];
      float act = mu;
      if (!deterministic) {
        uint32_t o[4];
        philox4((uint32_t)(row0 + r), (uint32_t)((uint64_t)(row0 + r) >> 32), (uint32_t)(a >> 1), call_lo ^ (call_hi * 0x9E3779B9u), seed_lo, seed_hi, o);
        const float u1 = fmaxf(u01(o[0]), 5.9604645e-8f), u2 = u01(o[1]);
        const float rad = sqrtf(-2.f * logf(u1));
        const float z = (a & 1) ? rad * sinf(6.28318530717958647692f * u2) : rad * cosf(6.28318530717958647692f * u2);
        act = mu + sd * z;
      }
      actions[(row0 + r) * na + a] = act;
      if (LOGP) {
        const float d = act - mu;
        term = -(d * d) / (2.f * sd * sd) - logf(sd) - 0.91893853320467274178f;      // Normal.log_prob
      }
    }
    if (LOGP) lp[r][a] = term;
  }
  if (!LOGP) return;
  lds_barrier();
  if (tid < MLP_ROWS && row0 + tid < n) {
    float sacc = 0.f;
    for (int a = 0; a < na; ++a) sacc += lp[tid][a];
    logp[row0 + tid] = sacc;
  }
}

__global__ __launch_bounds__(MLP_THREADS) void policy_act_kernel(MlpDev A, MlpDev Cr, const float* __restrict__ obs, const float* __restrict__ cobs,
                                                         int64_t n, const float* __restrict__ stdv, uint32_t seed_lo, uint32_t seed_hi,
                                                         uint32_t call_lo, uint32_t call_hi, int deterministic, float* __restrict__ actions,
                                                         float* __restrict__ mean, float* __restrict__ logp, float* __restrict__ values) {
  policy_act_body<true, false>(A, Cr, obs, cobs, n, stdv, seed_lo, seed_hi, call_lo, call_hi, deterministic, actions, mean, logp, values);
}

__global__ __launch_bounds__(MLP_THREADS) void distill_act_kernel(MlpDev S, MlpDev Te, const float* __restrict__ obs, const float* __restrict__ tobs,
                                                          int64_t n, const float* __restrict__ stdv, uint32_t seed_lo, uint32_t seed_hi,
                                                          uint32_t call_lo, uint32_t call_hi, int deterministic, float* __restrict__ actions,
                                                          float* __restrict__ mean, float* __restrict__ teacher_actions) {
  policy_act_body<false, false>(S, Te, obs, tobs, n, stdv, seed_lo, seed_hi, call_lo, call_hi, deterministic, actions, mean, nullptr, teacher_actions);
}

__global__ __launch_bounds__(MLP_THREADS) void policy_wide_act_kernel(MlpDev A, MlpDev Cr, const float* __restrict__ obs, const float* __restrict__ cobs,
                                                              int64_t n, const float* __restrict__ stdv, uint32_t seed_lo, uint32_t seed_hi,
                                                              uint32_t call_lo, uint32_t call_hi, int deterministic, float* __restrict__ actions,
                                                              float* __restrict__ mean, float* __restrict__ logp, float* __restrict__ values) {
  policy_act_body<true, true>(A, Cr, obs, cobs, n, stdv, seed_lo, seed_hi, call_lo, call_hi, deterministic, actions, mean, logp, values);
}

__global__ __launch_bounds__(MLP_THREADS) void distill_wide_act_kernel(MlpDev S, MlpDev Te, const float* __restrict__ obs, const float* __restrict__ tobs,
                                                               int64_t n, const float* __restrict__ stdv, uint32_t seed_lo, uint32_t seed_hi,
                                                               uint32_t call_lo, uint32_t call_hi, int deterministic, float* __restrict__ actions,
                                                               float* __restrict__ mean, float* __restrict__ teacher_actions) {
  policy_act_body<false, true>(S, Te, obs, tobs, n, stdv, seed_lo, seed_hi, call_lo, call_hi, deterministic, actions, mean, nullptr, teacher_actions);
}

// GAE (rollout_storage.py:145-160): one lane per env, the T-step recursion in registers
__global__ __launch_bounds__(256) void gae_kernel(const float* __restrict__ rew, const float* __restrict__ dones, const float* __restrict__ val,
                                                  const float* __restrict__ last, int T, int64_t n, float gamma, float lam,
                                                  float* __restrict__ ret, float* __restrict__ adv) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float a = 0.f, next = last[e];
  for (int t = T - 1; t >= 0; --t) {
    const float v = val[(size_t)t * n + e];
    const float nt = 1.f - dones[(size_t)t * n + e];
    const float delta = rew[(size_t)t * n + e] + nt * gamma * next - v;
    a = delta + nt * gamma * lam * a;
    ret[(size_t)t * n + e] = a + v;
    adv[(size_t)t * n + e] = (a + v) - v;          // self.returns - self.values, as the reference computes it
    next = v;
  }
}

// mean / unbiased std over all entries, then (x - mean) / (std + 1e-8): one workgroup, fixed-order tree (deterministic)
__global__ __launch_bounds__(1024) void normalize_kernel(float* __restrict__ adv, int64_t count) {
  __shared__ double s1[1024], s2[1024];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t i = tid; i < count; i += 1024) a += (double)adv[i];
  s1[tid] = a;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) { if (tid < off) s1[tid] += s1[tid + off]; __syncthreads(); }
  const double mean = s1[0] / (double)count;
  double q = 0.0;
  for (int64_t i = tid; i < count; i += 1024) { const double d = (double)adv[i] - mean; q += d * d; }
  s2[tid] = q;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) { if (tid < off) s2[tid] += s2[tid + off]; __syncthreads(); }
  const double sd = count > 1 ? sqrt(s2[0] / (double)(count - 1)) : 0.0;
  const float m = (float)mean, inv = 1.f / ((float)sd + 1e-8f);
  for (int64_t i = tid; i < count; i += 1024) adv[i] = (adv[i] - m) * inv;
}

extern "C" {

const char* lg_mlp_last_error(lg_mlp*) { return g_pol_err.c_str(); }

void lg_mlp_destroy(lg_mlp* m) {
  if (!m) return;
  DeviceScope ds_(m->device);
  for (void* p : m->allocs) (void)hipFree(p);
  delete m;
}

// the body of both create functions; max_input: the widest dims[0] the caller's entry point takes
static lg_mlp* mlp_create(int32_t L, const int32_t* dims, const float* const* weights, const float* const* biases, int32_t activation, int device_id,
                          int max_input) {
  if (L <= 0 || L > LG_MLP_MAX_LAYERS || !dims || !weights || !biases) { lg_policy_fail(LG_ERR_INVALID, "bad layer list"); return nullptr; }
  if (activation < LG_ACT_ELU || activation > LG_ACT_SELU) { lg_policy_fail(LG_ERR_INVALID, "unknown activation"); return nullptr; }
  // (an output wider than 32 is fine for lg_mlp_forward; lg_policy_act checks its own limit)
  if (max_input == MLP_MAXW) {
    for (int l = 0; l <= L; ++l) if (dims[l] <= 0 || dims[l] > MLP_MAXW) { lg_policy_fail(LG_ERR_INVALID, "layer width out of range (1..512)"); return nullptr; }
  } else {
    for (int l = 0; l <= L; ++l) {
      const int most = l == 0 ? max_input : MLP_MAXW;
      if (dims[l] >= 1 && dims[l] <= most) continue;
      const std::string which = std::string(l == 0 ? "input" : (l == L ? "output" : "hidden")) + " width " + std::to_string(dims[l]) + " (dims[" + std::to_string(l) + "])";
      lg_policy_fail(LG_ERR_INVALID, dims[l] < 1 ? which + " is below 1"
                                                 : which + " is over " + std::to_string(most) + (l == 0 ? "" : ": only the input row may be wider than 512"));
      return nullptr;
    }
  }
  if (!lg_policy_device_ok(device_id)) return nullptr;
  DeviceScope ds_(device_id);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_mlp* m = new lg_mlp();
  m->device = device_id; m->h.L = L; m->h.act = activation; m->h.act_out = 0;
  for (int l = 0; l <= L; ++l) m->h.dims[l] = dims[l];
  for (int l = 0; l < L; ++l) {
    const int K = dims[l], N = dims[l + 1], Kp = (K + 63) & ~63, nb = Kp / 16;
    // hidden layers produce the next layer's whole padded input (zero weights and bias -> act(0) = 0 in the padding)
    const int nch = l == L - 1 ? (N + 15) / 16 : ((N + 63) & ~63) / 16;
    m->h.kpad[l] = Kp; m->h.nchunks[l] = nch;
    // B fragment of v_mfma_f32_16x16x4_f32: lane holds B[k = lane >> 4][n = lane & 15] = W[n][k]; the fragments of the four
    // k-steps of a 16-input block sit in one float4 per lane
    std::vector<float> tw((size_t)nch * nb * 64 * 4, 0.f), tb((size_t)nch * 16, 0.f);
    for (int c = 0; c < nch; ++c)
      for (int b = 0; b < nb; ++b)
        for (int ln = 0; ln < 64; ++ln)
          for (int s = 0; s < 4; ++s) {
            const int nn = c * 16 + (ln & 15), kk = b * 16 + s * 4 + (ln >> 4);
            if (nn < N && kk < K) tw[(((size_t)c * nb + b) * 64 + ln) * 4 + s] = weights[l][(size_t)nn * K + kk];
          }
    for (int i = 0; i < N; ++i) tb[i] = biases[l][i];
    m->h.w[l] = (const float*)lg_policy_upload(tw.data(), tw.size() * 4, m->allocs);
    m->h.b[l] = m->h.w[l] ? (const float*)lg_policy_upload(tb.data(), tb.size() * 4, m->allocs) : nullptr;
    if (!m->h.b[l]) { lg_mlp_destroy(m); return nullptr; }
  }
  return m;
}

lg_mlp* lg_mlp_create(int32_t L, const int32_t* dims, const float* const* weights, const float* const* biases, int32_t activation,
                      int device_id) {
  POLICY_ENTRY;
  return mlp_create(L, dims, weights, biases, activation, device_id, MLP_MAXW);
}

lg_mlp* lg_mlp_create_wide(int32_t L, const int32_t* dims, const float* const* weights, const float* const* biases, int32_t activation,
                           int device_id) {
  POLICY_ENTRY;
  return mlp_create(L, dims, weights, biases, activation, device_id, LG_MLP_MAX_INPUT);
}

int lg_mlp_set_output_activation(lg_mlp* m, int32_t enabled) {
  POLICY_ENTRY;
  if (!m) return lg_policy_fail(LG_ERR_INVALID, "null network");
  m->h.act_out = enabled != 0;
  return LG_OK;
}

int lg_mlp_forward(lg_mlp* m, const float* x, int64_t n, float* y, void* stream) {
  POLICY_ENTRY;
  if (!m || !x || !y || n < 0) return lg_policy_fail(LG_ERR_INVALID, "null network or row, or n < 0");
  DeviceScope ds_(m->device);
  if (n == 0) return LG_OK;
  hipLaunchKernelGGL(mlp_is_wide(m) ? mlp_wide_forward_kernel : mlp_forward_kernel, dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS)), dim3(MLP_THREADS), 0,
                     (hipStream_t)stream, m->h, x, n, y);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_policy_act(lg_mlp* actor, lg_mlp* critic, const float* obs, const float* critic_obs, int64_t n, const float* std_, uint64_t seed,
                  uint64_t call, int32_t deterministic, float* actions, float* action_mean, float* logp, float* values, void* stream) {
  POLICY_ENTRY;
  if (!actor || !critic || !obs || !critic_obs || !std_ || !actions || !action_mean || !logp || !values || n < 0)
    return lg_policy_fail(LG_ERR_INVALID, "null network or row, or n < 0");
  DeviceScope ds_(actor->device);
  if (actor->h.dims[actor->h.L] > 32) return lg_policy_fail(LG_ERR_UNSUPPORTED, "the actor ends in more than 32 actions");
  if (n == 0) return LG_OK;
  hipLaunchKernelGGL(mlp_is_wide(actor) || mlp_is_wide(critic) ? policy_wide_act_kernel : policy_act_kernel,
                     dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS), 2), dim3(MLP_THREADS), 0, (hipStream_t)stream, actor->h, critic->h,
                     obs, critic_obs, n, std_, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), deterministic,
                     actions, action_mean, logp, values);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_compute_returns(const float* rewards, const float* dones, const float* values, const float* last_values, int32_t T, int64_t n,
                       float gamma, float lam, int32_t normalize, float* returns, float* advantages, void* stream) {
  POLICY_ENTRY;
  if (!rewards || !dones || !values || !last_values || !returns || !advantages || T <= 0 || n <= 0) return lg_policy_fail(LG_ERR_INVALID, "null row, T < 1 or n < 1");
  const int dev = lg_policy_device_of(rewards);          // no context in this call: run where the rows live
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "the rewards are not device memory");
  DeviceScope ds_(dev);
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rewards, dones, values, last_values, T, n,
                     gamma, lam, returns, advantages);
  if (normalize) hipLaunchKernelGGL(normalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, advantages, (int64_t)T * n);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

// the sigma rows of all T transitions (ppo.py:155: action_std broadcast over the envs): one launch for the whole rollout
__global__ __launch_bounds__(256) void fill_sigma_kernel(int64_t rows, int A, const float* __restrict__ std, float* __restrict__ sigma) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * A) return;
  sigma[i] = std[i % A];
}

}  // extern "C"


// ============================================================================================ recurrent memory (lgpolicy.h: lg_rnn_*)
// One step of one nn.LSTM / nn.GRU layer (rsl_rl networks/memory.py:27-33, inference mode) for 32 rows per workgroup; ONE launch per
// memory layer, the actor's and the critic's memory side by side on blockIdx.y when both step together (lg_policy_act_recurrent).
//
// The two products W_ih x + W_hh h are one k-chain over the concatenated row [x (padded to 16) ; h (padded to 16)], staged in LDS in the
// MLP kernel's activation image (IMG above: one ds_read_b128 feeds four k-steps).  A wave owns 16 hidden units at a time and keeps ALL
// gate accumulators of those units for both row halves (LSTM: i f g o; GRU: r z n_x n_h -- the n gate's x part and h part apart, because
// r multiplies the h part only): 8 independent 16x16 tiles, 32 MFMAs per pair of LDS reads, and the gate non-linearities + state update are
// a register epilogue with no second pass through LDS or HBM.  Weights are re-tiled on the host (rnn_tile_weights) so that a wave loads the
// fragments of one gate for a block of 16 inputs with one coalesced dwordx4; the fragments of the next block are requested before
// the MFMAs of the current one.
// LDS: 32 rows x 1024 floats = 128 KB (input 512 + hidden 512, the widest allowed), static; nothing else is staged.
// RnnLayerDev and struct lg_rnn: lg_policy_internal.h (the trainer reaches the images); the tile itself: lg_rnn_tile.h (SAVE = false here)

void lg_mlp_widths(const lg_mlp* m, int* layers, int* in, int* out, int* device) { *layers = m->h.L; *in = m->h.dims[0]; *out = m->h.dims[m->h.L]; *device = m->device; }
void lg_rnn_widths(const lg_rnn* m, int* type, int* input, int* hidden, int* device) { *type = m->type; *input = m->input; *hidden = m->hidden; *device = m->device; }

// blockIdx.y picks the memory (0: the actor's or the only one, 1: the critic's)
__global__ __launch_bounds__(MLP_THREADS) void rnn_layer_kernel(RnnStepArgs S0, RnnStepArgs S1, int64_t n) {
  __shared__ __attribute__((aligned(16))) float img[MLP_ROWS * RNN_KMAX];
  const RnnStepArgs& S = blockIdx.y == 0 ? S0 : S1;
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  const RnnSaveArgs none{};
  if (S.L.gru) rnn_tile<true, false>(S, none, row0, n, img); else rnn_tile<false, false>(S, none, row0, n, img);
}

// ---- a wide memory (lgpolicy_wide.h: lg_rnn_create_wide): layer 0 as projection + seeded step.
// The one-launch tile cannot take more than RNN_XMAX inputs: it keeps the whole row [x ; h] of 32 rows resident (128 KB at 512 + 512; 320 KB at
// 2048 + 512, a workgroup has 160), and it cannot slab x either, because a wave walks its chunks one after another under the resident row -- slabs would
// need the accumulators of ALL chunks of the wave alive at once (8 chunks x 8 tiles x 4 registers).  So the x part is cut off the chain: here the
// chunks lie on blockIdx.y, a wave owns ONE chunk of 16 hidden units and keeps its G gate accumulators of both row halves in registers while the row
// passes through LDS in slabs of RNN_XMAX columns.  Every output is one k-ascending chain from zero over blocks of 16 inputs, the chain the narrow tile
// walks before it reaches h, stored unrounded; rnn_tile<.., SEED> picks it up.  64 KB of LDS: two workgroups per CU.
template <int G>
LG_DEV void rnn_xproj_tile(const RnnXprojArgs& P, int64_t row0, int64_t n, float* img) {
  const RnnLayerDev& R = P.L;
  const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.y * (MLP_THREADS / 64) + (tid >> 6);
  const int I = R.I, Hp = 16 * R.nch;
  const float* __restrict__ x = P.x;
  const int64_t* __restrict__ gather = P.idx;
  f32x4 acc[4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g) { acc[g][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const float4* ap = reinterpret_cast<const float4*>(img) + (lane & 15) * 4 + (lane >> 4);
  for (int k0 = 0; k0 < R.Ip; k0 += RNN_XMAX) {
    const int Kp = R.Ip - k0 < RNN_XMAX ? R.Ip - k0 : RNN_XMAX;       // a multiple of 16
    if (k0) lds_barrier();                                             // every wave has read the slab before
    for (int base = 0; base < MLP_ROWS * Kp; base += 8 * MLP_THREADS) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + u * MLP_THREADS + tid, r = e / Kp, k = e - r * Kp;
        const int64_t row = row0 + r;
        float val = 0.f;
        if (e < MLP_ROWS * Kp && row < n && k0 + k < I) val = x[(gather ? gather[row] : row) * I + k0 + k];
        v[u] = val;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + u * MLP_THREADS + tid, r = e / Kp, k = e - r * Kp;
        if (e < MLP_ROWS * Kp) img[IMG(r, k)] = v[u];
      }
    }
    lds_barrier();
    if (c < R.nch) {
      const int kb0 = k0 >> 4;
      const float4* wc = reinterpret_cast<const float4*>(R.w) + ((size_t)c * (R.nbx + 1) + kb0) * G * 64 + lane;
      rnn_blocks<G, 2>(acc, wc, ap, 0, Kp >> 4, R.nbx - kb0);
    }
  }
  if (c >= R.nch) return;
  float* __restrict__ y = P.y;
  const int col = c * 16 + (lane & 15);
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + 4 * (lane >> 4) + i + 16 * hf;
        if (row < n) y[(row * G + g) * Hp + col] = acc[g][hf][i];
      }
}

// blockIdx.y: eight chunks of 16 hidden units; blockIdx.z picks the memory
__global__ __launch_bounds__(MLP_THREADS) void rnn_wide_xproj_kernel(RnnXprojArgs P0, RnnXprojArgs P1, int64_t n) {
  __shared__ __attribute__((aligned(16))) float img[MLP_ROWS * RNN_XMAX];
  const RnnXprojArgs& P = blockIdx.z == 0 ? P0 : P1;
  if ((int)blockIdx.y * (MLP_THREADS / 64) >= P.L.nch) return;        // the narrower memory of a pair: the whole workgroup leaves
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  if (P.L.gru) rnn_xproj_tile<3>(P, row0, n, img); else rnn_xproj_tile<4>(P, row0, n, img);
}

void rnn_launch_xproj(const RnnXprojArgs* a, const RnnXprojArgs* b, int64_t n, hipStream_t st) {
  const int nch = b && b->L.nch > a->L.nch ? b->L.nch : a->L.nch, per = MLP_THREADS / 64;
  hipLaunchKernelGGL(rnn_wide_xproj_kernel, dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS), (nch + per - 1) / per, b ? 2 : 1), dim3(MLP_THREADS), 0, st, *a, b ? *b : *a, n);
}

// layer 0 of a wide memory after its projection y: the tile with SEED; the image holds h alone (32 rows x 512 floats = 64 KB).  Both memories' operands
// in ONE kernel argument indexed by blockIdx.y: the operands of the memory that is not this workgroup's are never loaded
struct RnnWidePair { RnnStepArgs S[2]; const float* y[2]; };
__global__ __launch_bounds__(MLP_THREADS) void rnn_wide_layer_kernel(RnnWidePair P, int64_t n) {
  __shared__ __attribute__((aligned(16))) float img[MLP_ROWS * RNN_XMAX];
  const RnnStepArgs& S = P.S[blockIdx.y];
  const float* __restrict__ y = P.y[blockIdx.y];
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  const RnnSaveArgs none{};
  if (S.L.gru) rnn_tile<true, false, true>(S, none, row0, n, img, y); else rnn_tile<false, false, true>(S, none, row0, n, img, y);
}

// Memory.reset(dones) (memory.py:45-51): hidden_state[..., dones == 1, :] = 0 on every layer
__global__ __launch_bounds__(256) void rnn_reset_rows_kernel(float* __restrict__ h, float* __restrict__ c, const float* __restrict__ dones, int64_t n, int H, int L) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)L * n * H) return;
  const int64_t row = (idx / H) % n;
  if (dones[row] != 0.f) { h[idx] = 0.f; if (c) c[idx] = 0.f; }
}

// [x ; h] weights of one layer in MFMA B-fragment order: tiled[((c * (nb + 1) + b) * G + g) * 64 + lane][s] = Wcat[g * H + 16 c + (lane & 15)][16 b + 4 s + (lane >> 4)],
// Wcat[:, 0 .. I) = w_ih, Wcat[:, Ip .. Ip + H) = w_hh, zero elsewhere (Ip = I rounded up to 16); block nb of every chunk is all zero (what the second half
// of an odd block count multiplies).  A pure function of its arguments.
static size_t rnn_tiled_count(int G, int I, int H) {
  const int Ip = (I + 15) & ~15, nb = (Ip + ((H + 15) & ~15)) / 16, nch = (H + 15) / 16;
  return (size_t)nch * (nb + 1) * G * 64 * 4;
}
void rnn_tile_weights_at(int G, int I, int Ip, int nb, int H, const float* w_ih, const float* w_hh, float* tiled) {
  const int nch = (H + 15) / 16;
  for (int c = 0; c < nch; ++c)
    for (int b = 0; b <= nb; ++b)
      for (int g = 0; g < G; ++g)
        for (int ln = 0; ln < 64; ++ln)
          for (int s = 0; s < 4; ++s) {
            const int u = c * 16 + (ln & 15), k = b * 16 + s * 4 + (ln >> 4);
            float v = 0.f;
            if (u < H) {
              if (k < I) v = w_ih[(size_t)(g * H + u) * I + k];
              else if (k >= Ip && k < Ip + H) v = w_hh[(size_t)(g * H + u) * H + (k - Ip)];
            }
            tiled[((((size_t)c * (nb + 1) + b) * G + g) * 64 + ln) * 4 + s] = v;
          }
}
static void rnn_tile_weights(int G, int I, int H, const float* w_ih, const float* w_hh, float* tiled) {
  const int Ip = (I + 15) & ~15;
  rnn_tile_weights_at(G, I, Ip, (Ip + ((H + 15) & ~15)) / 16, H, w_ih, w_hh, tiled);
}
// the two images of a wide layer 0: the projection's (w_ih alone, nbx + 1 blocks per chunk) and the seeded tile's (w_hh alone, nch + 1 blocks)
static size_t rnn_tiled_count_x(int G, int I, int H) { return (size_t)((H + 15) / 16) * (((I + 15) >> 4) + 1) * G * 64 * 4; }
static size_t rnn_tiled_count_h(int G, int H) { return (size_t)((H + 15) / 16) * ((H + 15) / 16 + 1) * G * 64 * 4; }

static int rnn_check(const lg_rnn* m, const float* h, const float* c, int64_t n) {
  if (!m || !h || n < 0) return lg_policy_fail(LG_ERR_INVALID, "null memory or hidden state, or n < 0");
  if (m->type == LG_RNN_LSTM && !c) return lg_policy_fail(LG_ERR_INVALID, "an LSTM needs its cell state");
  return LG_OK;
}

static RnnStepArgs rnn_args(const lg_rnn* m, int l, const float* x, int64_t n, float* h, float* c, const float* reset, float* out) {
  RnnStepArgs a;
  const size_t slab = (size_t)n * m->hidden;
  a.L = m->layer[l];
  a.x = l == 0 ? x : h + (size_t)(l - 1) * slab;
  a.h = h + (size_t)l * slab;
  a.c = m->type == LG_RNN_LSTM ? c + (size_t)l * slab : nullptr;
  a.reset = reset;
  a.out = l == m->num_layers - 1 ? out : nullptr;
  return a;
}

// the projection workspace of a wide memory for n rows: allocated at the first step, regrown when n grows (the old buffer is released only after the
// stream it was last used on has drained), never shrunk
static int rnn_wide_workspace(lg_rnn* m, int64_t n, hipStream_t st) {
  if (n > m->y_rows) {
    if (m->y) { POLICY_TRY(hipStreamSynchronize(m->y_stream)); (void)hipFree(m->y); m->y = nullptr; m->y_rows = 0; }
    const int G = m->type == LG_RNN_GRU ? 3 : 4;
    POLICY_TRY(hipMalloc((void**)&m->y, (size_t)n * G * 16 * m->xproj.nch * sizeof(float)));
    m->y_rows = n;
  }
  m->y_stream = st;
  return LG_OK;
}

// layers of one memory (b null), or of two memories of equal depth side by side
static int rnn_step_pair(lg_rnn* a, const float* xa, float* ha, float* ca, float* outa, lg_rnn* b, const float* xb, float* hb, float* cb, float* outb,
                         int64_t n, const float* reset, hipStream_t st) {
  const unsigned tiles = (unsigned)((n + MLP_ROWS - 1) / MLP_ROWS);
  const bool any_wide = a->wide || (b && b->wide);
  if (any_wide) {
    // layer 0 of a wide memory: projection, then the seeded tile; two wide memories side by side, a mixed pair one memory after the other
    int rc = a->wide ? rnn_wide_workspace(a, n, st) : LG_OK;
    if (rc == LG_OK && b && b->wide) rc = rnn_wide_workspace(b, n, st);
    if (rc != LG_OK) return rc;
    const RnnStepArgs s0 = rnn_args(a, 0, xa, n, ha, ca, reset, outa);
    const RnnStepArgs s1 = b ? rnn_args(b, 0, xb, n, hb, cb, reset, outb) : s0;
    const RnnXprojArgs p0{a->xproj, xa, nullptr, a->y}, p1{b ? b->xproj : a->xproj, xb, nullptr, b ? b->y : nullptr};
    if (b && a->wide && b->wide) {
      rnn_launch_xproj(&p0, &p1, n, st);
      hipLaunchKernelGGL(rnn_wide_layer_kernel, dim3(tiles, 2), dim3(MLP_THREADS), 0, st, RnnWidePair{{s0, s1}, {a->y, b->y}}, n);
    } else {
      lg_rnn* mem[2] = {a, b};
      const RnnStepArgs* ss[2] = {&s0, &s1};
      const RnnXprojArgs* pp[2] = {&p0, &p1};
      for (int k = 0; k < (b ? 2 : 1); ++k) {
        if (mem[k]->wide) {
          rnn_launch_xproj(pp[k], nullptr, n, st);
          hipLaunchKernelGGL(rnn_wide_layer_kernel, dim3(tiles, 1), dim3(MLP_THREADS), 0, st, RnnWidePair{{*ss[k], *ss[k]}, {mem[k]->y, mem[k]->y}}, n);
        } else {
          hipLaunchKernelGGL(rnn_layer_kernel, dim3(tiles, 1), dim3(MLP_THREADS), 0, st, *ss[k], *ss[k], n);
        }
      }
    }
  }
  for (int l = any_wide ? 1 : 0; l < a->num_layers; ++l) {
    const RnnStepArgs s0 = rnn_args(a, l, xa, n, ha, ca, reset, outa);
    const RnnStepArgs s1 = b ? rnn_args(b, l, xb, n, hb, cb, reset, outb) : s0;
    hipLaunchKernelGGL(rnn_layer_kernel, dim3(tiles, b ? 2 : 1), dim3(MLP_THREADS), 0, st, s0, s1, n);
  }
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

// The memories in front of two MLP heads step -- side by side when their depths agree, else one after the other; b null: a alone -- and *top_a / *top_b
// point at the top layers' h', where the heads read it (ActorCriticRecurrent.act / evaluate: actor(memory_a(obs)), critic(memory_c(obs))).  A head
// without a memory reads its row itself: *top_b = xb.
static int rnn_step_heads(lg_rnn* a, const float* xa, float* ha, float* ca, lg_rnn* b, const float* xb, float* hb, float* cb, int64_t n, const float* reset,
                          hipStream_t st, const float** top_a, const float** top_b) {
  int rc;
  if (b && b->num_layers == a->num_layers) {
    rc = rnn_step_pair(a, xa, ha, ca, nullptr, b, xb, hb, cb, nullptr, n, reset, st);
  } else {
    rc = rnn_step_pair(a, xa, ha, ca, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, reset, st);
    if (rc == LG_OK && b) rc = rnn_step_pair(b, xb, hb, cb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, reset, st);
  }
  *top_a = ha + (size_t)(a->num_layers - 1) * n * a->hidden;
  *top_b = b ? hb + (size_t)(b->num_layers - 1) * n * b->hidden : xb;
  return rc;
}

// the env's observation rows and (n, O, A): what every collector asks the env first
static int env_shape(lg_ctx* env, const float** obs, int64_t* n, int64_t* O, int64_t* A) {
  void* p; int64_t shp[4], ashp[4]; int32_t nd, dt;
  if (lg_get_tensor(env, LG_T_OBS_BUF, &p, shp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's observation rows: ") + lg_last_error(env));
  *obs = (const float*)p; *n = shp[0]; *O = shp[1];
  if (lg_get_tensor(env, LG_T_ACTIONS, &p, ashp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's action rows: ") + lg_last_error(env));
  *A = ashp[1];
  return LG_OK;
}

extern "C" int lg_step_transition(lg_ctx* ctx, const float* actions, float* next_observations, const float* values, float gamma,
                                  float* rewards, float* dones, void* stream);

extern "C" {

int64_t lg_rnn_tile_weights(int32_t type, int32_t input, int32_t hidden, const float* w_ih, const float* w_hh, float* tiled) {
  POLICY_ENTRY;
  if ((type != LG_RNN_LSTM && type != LG_RNN_GRU) || input < 1 || input > 512 || hidden < 1 || hidden > 512)
    return lg_policy_fail(LG_ERR_INVALID, "unknown memory type, or a width out of range (1..512)");
  const int G = type == LG_RNN_GRU ? 3 : 4;
  if (tiled) {
    if (!w_ih || !w_hh) return lg_policy_fail(LG_ERR_INVALID, "null weight");
    rnn_tile_weights(G, input, hidden, w_ih, w_hh, tiled);
  }
  return (int64_t)rnn_tiled_count(G, input, hidden);
}

void lg_rnn_destroy(lg_rnn* m) {
  if (!m) return;
  DeviceScope ds_(m->device);
  for (void* p : m->allocs) (void)hipFree(p);
  if (m->y) (void)hipFree(m->y);
  delete m;
}

// the body of lg_rnn_create (max_input 512) and lg_rnn_create_wide (LG_RNN_MAX_INPUT).  wide: layer 0 takes the projection + seeded-tile path
static lg_rnn* rnn_create(int32_t type, int32_t num_layers, int32_t input, int32_t hidden, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, int device_id, int max_input, bool wide) {
  if (type != LG_RNN_LSTM && type != LG_RNN_GRU) { lg_policy_fail(LG_ERR_INVALID, "unknown memory type (lstm | gru)"); return nullptr; }
  if (num_layers < 1 || num_layers > RNN_MAX_LAYERS) { lg_policy_fail(LG_ERR_INVALID, "number of layers out of range (1..4)"); return nullptr; }
  if (input < 1 || input > max_input) { lg_policy_fail(LG_ERR_INVALID, "input width out of range (1.." + std::to_string(max_input) + ")"); return nullptr; }
  if (hidden < 1 || hidden > 512) { lg_policy_fail(LG_ERR_INVALID, "hidden width out of range (1..512)"); return nullptr; }
  if (!w_ih || !w_hh || !b_ih || !b_hh) { lg_policy_fail(LG_ERR_INVALID, "null weight list"); return nullptr; }
  for (int l = 0; l < num_layers; ++l)
    if (!w_ih[l] || !w_hh[l] || !b_ih[l] || !b_hh[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight"); return nullptr; }
  if (!lg_policy_device_ok(device_id)) return nullptr;
  DeviceScope ds_(device_id);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_rnn* m = new lg_rnn();
  m->type = type; m->num_layers = num_layers; m->input = input; m->hidden = hidden; m->device = device_id; m->wide = wide;
  const int G = type == LG_RNN_GRU ? 3 : 4, H = hidden;
  for (int l = 0; l < num_layers; ++l) {
    const int I = l == 0 ? input : hidden, Ip = (I + 15) & ~15, nch = (H + 15) / 16, Hp = 16 * nch;
    RnnLayerDev& R = m->layer[l];
    R.gru = type == LG_RNN_GRU; R.I = I; R.H = H; R.Ip = Ip; R.nbx = Ip / 16; R.nb = (Ip + Hp) / 16; R.nch = nch;
    std::vector<float> tw, tb((size_t)4 * Hp, 0.f);
    if (wide && l == 0) {
      RnnLayerDev& X = m->xproj;
      X = R; X.b = nullptr;
      std::vector<float> tx(rnn_tiled_count_x(G, I, H));
      rnn_tile_weights_at(G, I, RNN_NO_HH, X.nbx, H, w_ih[l], nullptr, tx.data());
      X.w = (const float*)lg_policy_upload(tx.data(), tx.size() * 4, m->allocs);
      if (!X.w) { lg_rnn_destroy(m); return nullptr; }
      R.I = 0; R.Ip = 0; R.nbx = 0; R.nb = nch;                 // the seeded tile's image: h alone
      tw.resize(rnn_tiled_count_h(G, H));
      rnn_tile_weights_at(G, 0, 0, nch, H, nullptr, w_hh[l], tw.data());
    } else {
      tw.resize(rnn_tiled_count(G, I, H));
      rnn_tile_weights(G, I, H, w_ih[l], w_hh[l], tw.data());
    }
    for (int u = 0; u < H; ++u) {
      if (type == LG_RNN_LSTM) {
        for (int g = 0; g < 4; ++g) tb[(size_t)g * Hp + u] = b_ih[l][g * H + u] + b_hh[l][g * H + u];
      } else {
        tb[u] = b_ih[l][u] + b_hh[l][u];
        tb[(size_t)Hp + u] = b_ih[l][H + u] + b_hh[l][H + u];
        tb[(size_t)2 * Hp + u] = b_ih[l][2 * H + u];
        tb[(size_t)3 * Hp + u] = b_hh[l][2 * H + u];
      }
    }
    R.w = (const float*)lg_policy_upload(tw.data(), tw.size() * 4, m->allocs);
    R.b = R.w ? (const float*)lg_policy_upload(tb.data(), tb.size() * 4, m->allocs) : nullptr;
    if (!R.b) { lg_rnn_destroy(m); return nullptr; }
  }
  return m;
}

lg_rnn* lg_rnn_create(int32_t type, int32_t num_layers, int32_t input, int32_t hidden, const float* const* w_ih, const float* const* w_hh,
                      const float* const* b_ih, const float* const* b_hh, int device_id) {
  POLICY_ENTRY;
  return rnn_create(type, num_layers, input, hidden, w_ih, w_hh, b_ih, b_hh, device_id, RNN_XMAX, false);
}

lg_rnn* lg_rnn_create_wide(int32_t type, int32_t num_layers, int32_t input, int32_t hidden, const float* const* w_ih, const float* const* w_hh,
                           const float* const* b_ih, const float* const* b_hh, int device_id) {
  POLICY_ENTRY;
  // diagnostic (lgpolicy_wide_memory.h, lg_switches.h): LG_RNN_FORCE_WIDE=1 sends a narrow memory through the wide kernels too, to compare their bits
  // with lg_rnn_create's
  int force = 0;
  std::string bad;
  if (!lg_switch_flag("LG_RNN_FORCE_WIDE", force, bad)) { lg_policy_fail(LG_ERR_INVALID, bad); return nullptr; }
  const bool wide = input > RNN_XMAX || force == 1;
  return rnn_create(type, num_layers, input, hidden, w_ih, w_hh, b_ih, b_hh, device_id, LG_RNN_MAX_INPUT, wide);
}

int64_t lg_rnn_tile_weights_wide(int32_t type, int32_t input, int32_t hidden, const float* w_ih, const float* w_hh, float* tiled_x, float* tiled_h,
                                 int64_t* count_h) {
  POLICY_ENTRY;
  if (type != LG_RNN_LSTM && type != LG_RNN_GRU) return lg_policy_fail(LG_ERR_INVALID, "unknown memory type (lstm | gru)");
  if (input < 1 || input > LG_RNN_MAX_INPUT) return lg_policy_fail(LG_ERR_INVALID, "input width out of range (1.." + std::to_string(LG_RNN_MAX_INPUT) + ")");
  if (hidden < 1 || hidden > 512) return lg_policy_fail(LG_ERR_INVALID, "hidden width out of range (1..512)");
  const int G = type == LG_RNN_GRU ? 3 : 4;
  if (tiled_x) {
    if (!w_ih) return lg_policy_fail(LG_ERR_INVALID, "null weight");
    rnn_tile_weights_at(G, input, RNN_NO_HH, (input + 15) >> 4, hidden, w_ih, nullptr, tiled_x);
  }
  if (tiled_h) {
    if (!w_hh) return lg_policy_fail(LG_ERR_INVALID, "null weight");
    rnn_tile_weights_at(G, 0, 0, (hidden + 15) / 16, hidden, nullptr, w_hh, tiled_h);
  }
  if (count_h) *count_h = (int64_t)rnn_tiled_count_h(G, hidden);
  return (int64_t)rnn_tiled_count_x(G, input, hidden);
}

int lg_rnn_step(lg_rnn* m, const float* x, int64_t n, float* h, float* c, const float* reset, float* out, void* stream) {
  POLICY_ENTRY;
  if (!x) return lg_policy_fail(LG_ERR_INVALID, "null input row");
  int rc = rnn_check(m, h, c, n);
  if (rc != LG_OK || n == 0) return rc;
  DeviceScope ds_(m->device);
  return rnn_step_pair(m, x, h, c, out, nullptr, nullptr, nullptr, nullptr, nullptr, n, reset, (hipStream_t)stream);
}

int lg_rnn_reset_rows(lg_rnn* m, float* h, float* c, const float* dones, int64_t n, void* stream) {
  POLICY_ENTRY;
  if (!dones) return lg_policy_fail(LG_ERR_INVALID, "null dones row");
  int rc = rnn_check(m, h, c, n);
  if (rc != LG_OK || n == 0) return rc;
  DeviceScope ds_(m->device);
  const int64_t total = (int64_t)m->num_layers * n * m->hidden;
  hipLaunchKernelGGL(rnn_reset_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h, m->type == LG_RNN_LSTM ? c : nullptr, dones, n,
                     m->hidden, m->num_layers);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_policy_act_recurrent(lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* obs, const float* critic_obs, int64_t n, const float* std_,
                            uint64_t seed, uint64_t call, int32_t deterministic, float* h_a, float* c_a, float* h_c, float* c_c, const float* reset,
                            float* actions, float* action_mean, float* actions_log_prob, float* values, void* stream) {
  POLICY_ENTRY;
  if (!mem_a || !mem_c || !actor || !critic || !obs || !critic_obs) return lg_policy_fail(LG_ERR_INVALID, "null network or row");
  int rc = rnn_check(mem_a, h_a, c_a, n);
  if (rc == LG_OK) rc = rnn_check(mem_c, h_c, c_c, n);
  if (rc != LG_OK) return rc;
  if (actor->h.dims[0] != mem_a->hidden || critic->h.dims[0] != mem_c->hidden) return lg_policy_fail(LG_ERR_INVALID, "an MLP's input width is not its memory's hidden width");
  if (n == 0) return LG_OK;
  DeviceScope ds_(mem_a->device);
  const float *top_a, *top_c;
  rc = rnn_step_heads(mem_a, obs, h_a, c_a, mem_c, critic_obs, h_c, c_c, n, reset, (hipStream_t)stream, &top_a, &top_c);
  if (rc != LG_OK) return rc;
  return lg_policy_act(actor, critic, top_a, top_c, n, std_, seed, call, deterministic, actions, action_mean, actions_log_prob, values, stream);
}

// both PPO collectors: the loop is lg_policy_collect_rollout, at the end of this file (behind the history layer it shares with the distillation collector)
int lg_collect_rollout(lg_ctx* env, lg_mlp* actor, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                       float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, void* stream) {
  POLICY_ENTRY;
  if (!env || !actor || !critic || !std || !out || T <= 0) return lg_policy_fail(LG_ERR_INVALID, "null argument or T < 1");
  return lg_policy_collect_rollout(env, nullptr, actor, nullptr, critic, std, seed, first_call, T, gamma, lam, normalize_advantage, out, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, stream);
}

int lg_collect_rollout_recurrent(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call,
                                 int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid,
                                 float* h_a, float* c_a, float* h_c, float* c_c, void* stream) {
  POLICY_ENTRY;
  if (!env || !mem_a || !mem_c || !actor || !critic || !std || !out || !hid || T <= 0) return lg_policy_fail(LG_ERR_INVALID, "null argument or T < 1");
  return lg_policy_collect_rollout(env, mem_a, actor, mem_c, critic, std, seed, first_call, T, gamma, lam, normalize_advantage, out, hid, h_a, c_a, h_c, c_c,
                                   nullptr, stream);
}

}  // extern "C"


// ============================================================================================ teacher-student distillation (lgpolicy.h)
// The observation-history layer (AnymalStudent.compute_observations, anymal.py:336-383) in one launch.  One lane owns one (row, column) and walks
// its H slots from the oldest to the newest: slot s takes what slot s - 1 held, so every location is read before the same lane overwrites it and
// the shift needs no second buffer; a row's slots are never split across lanes.  Memory-bound and tiny (4 MB at 4096 x 240): the point is one
// launch instead of five and no host work inside the collection loop.  The noise is torch's sequence of rounded fp32 operations (2 u, - 1,
// * scale, +): contraction is switched off for the kernel, so nothing fuses to an FMA.
__global__ __launch_bounds__(256) void obs_history_kernel(float* __restrict__ hist, int64_t n, int H, int W, const float* __restrict__ obs, int64_t stride,
                                                          const float* __restrict__ dones, const float* __restrict__ scale, const float* __restrict__ inject,
                                                          uint32_t seed_lo, uint32_t seed_hi, uint32_t call_lo, uint32_t call_hi, float clip,
                                                          float* __restrict__ out) {
#pragma clang fp contract(off)       // every product below is rounded before it is added, as in the torch function (the compiler's default fuses them)
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * W) return;
  const int64_t row = idx / W;
  const int j = (int)(idx - row * W);
  const float keep = (dones && dones[row] != 0.f) ? 0.f : 1.f;       // history * (~reset): a product, as in the torch function (-x * 0 = -0)
  const size_t base = (size_t)row * H * W;
  for (int s = H - 1; s >= 0; --s) {
    const int k = s * W + j;
    float v = s > 0 ? hist[base + k - W] * keep : obs[row * stride + j];
    if (scale) {
      float u;
      if (inject) {
        u = inject[base + k];
      } else {
        uint32_t o[4];
        philox4((uint32_t)row, (uint32_t)((uint64_t)row >> 32), 0x80000000u | (uint32_t)k, call_lo ^ (call_hi * 0x9E3779B9u), seed_lo, seed_hi, o);
        u = u01(o[0]);
      }
      const float t2 = 2.f * u, t1 = t2 - 1.f, ns = t1 * scale[k];
      v = v + ns;
    }
    hist[base + k] = v;
    if (out) out[base + k] = v < -clip ? -clip : (v > clip ? clip : v);           // torch.clip: a NaN stays a NaN
  }
}

// observations[0] of a collection: the clipped copy of the history as it stands
__global__ __launch_bounds__(256) void obs_clip_kernel(const float* __restrict__ src, int64_t count, float clip, float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const float v = src[i];
  dst[i] = v < -clip ? -clip : (v > clip ? clip : v);
}

static int distill_widths(lg_mlp* student, lg_mlp* teacher) {
  const int A = student->h.dims[student->h.L], At = teacher->h.dims[teacher->h.L];
  if (A != At) return lg_policy_fail(LG_ERR_INVALID, "the student and the teacher end in different action widths");
  if (A > 32) return lg_policy_fail(LG_ERR_UNSUPPORTED, "the networks end in more than 32 actions");
  return LG_OK;
}

// ---- the row a reader (the student; the actor of the two-stream PPO collection) derives from the env's raw row: the history layer's, or the
// first `width` columns.  `who` names the reader in the refusals, `wider` ends the last of them.
static int derived_row_check(const lg_obs_history* hist, int64_t width, int64_t env_width, const char* who, const char* wider) {
  if (hist) {
    if (!hist->history || hist->H < 1 || hist->W < 1 || hist->W > env_width || !(hist->clip > 0.f)) return lg_policy_fail(LG_ERR_INVALID, "bad history layer (pointer, H, W <= env row, clip > 0)");
    if ((int64_t)hist->H * hist->W != width) return lg_policy_fail(LG_ERR_INVALID, std::string("the ") + who + "'s input width is not H x W of the history layer");
  } else if (width > env_width) {
    return lg_policy_fail(LG_ERR_INVALID, std::string("without a history layer the ") + who + " reads a prefix of the env's observation row" + wider);
  }
  return LG_OK;
}

struct DerivedRow { const lg_obs_history* hist; const float* env_obs; int64_t n, env_width, width; uint64_t first_call; void* stream; };

// t >= 0: the row after step t -- the layer steps in place on the env's own raw row (dst NULL: it steps and writes no row out); t < 0: row 0 of
// a collection, the clipped history as it stands.  Without a layer both are the 2-D copy of the prefix.  One launch or one copy.
static int derived_row(const DerivedRow& r, int t, const float* dones_t, float* dst) {
  const lg_obs_history* hist = r.hist;
  hipStream_t st = (hipStream_t)r.stream;
  const size_t count = (size_t)r.n * r.width;
  if (hist && t < 0) {
    hipLaunchKernelGGL(obs_clip_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, hist->history, (int64_t)count, hist->clip, dst);
    return LG_OK;
  }
  if (hist) return lg_obs_history_step(hist->history, r.n, hist->H, hist->W, r.env_obs, r.env_width, dones_t, hist->noise_scale,
                                       hist->inject_u ? hist->inject_u + (size_t)t * count : nullptr, hist->noise_seed, r.first_call + (uint64_t)t, hist->clip, dst, r.stream);
  if (dst) POLICY_TRY(hipMemcpy2DAsync(dst, (size_t)r.width * 4, r.env_obs, (size_t)r.env_width * 4, (size_t)r.width * 4, (size_t)r.n, hipMemcpyDeviceToDevice, st));
  return LG_OK;
}

extern "C" {

int lg_obs_history_step(float* history, int64_t n, int32_t H, int32_t W, const float* obs, int64_t obs_stride, const float* dones,
                        const float* noise_scale, const float* inject_u, uint64_t seed, uint64_t call, float clip, float* obs_out, void* stream) {
  POLICY_ENTRY;
  if (H < 1 || W < 1) return lg_policy_fail(LG_ERR_INVALID, "history length H and row width W must be at least 1");
  if (obs_stride < W) return lg_policy_fail(LG_ERR_INVALID, "the observation row stride is smaller than W");
  if (!(clip > 0.f)) return lg_policy_fail(LG_ERR_INVALID, "clip must be positive (INFINITY: no clip)");
  if (!history || !obs || n < 0) return lg_policy_fail(LG_ERR_INVALID, "null history or observation pointer");
  if (n == 0) return LG_OK;
  const int dev = lg_policy_device_of(history);
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "the history is not device memory");
  DeviceScope ds_(dev);
  hipLaunchKernelGGL(obs_history_kernel, dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, (hipStream_t)stream, history, n, H, W, obs, obs_stride, dones,
                     noise_scale, inject_u, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), clip, obs_out);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_distill_act(lg_mlp* student, lg_mlp* teacher, const float* obs, const float* teacher_obs, int64_t n, const float* std_, uint64_t seed,
                   uint64_t call, int32_t deterministic, float* actions, float* action_mean, float* teacher_actions, void* stream) {
  POLICY_ENTRY;
  if (!student || !teacher || !obs || !teacher_obs || !std_ || !actions || !teacher_actions || n < 0) return lg_policy_fail(LG_ERR_INVALID, "null network or row");
  const int rc = distill_widths(student, teacher);
  if (rc != LG_OK || n == 0) return rc;
  DeviceScope ds_(student->device);
  hipLaunchKernelGGL(mlp_is_wide(student) || mlp_is_wide(teacher) ? distill_wide_act_kernel : distill_act_kernel,
                     dim3((unsigned)((n + MLP_ROWS - 1) / MLP_ROWS), 2), dim3(MLP_THREADS), 0, (hipStream_t)stream, student->h, teacher->h,
                     obs, teacher_obs, n, std_, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), deterministic,
                     actions, action_mean, teacher_actions);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_distill_act_recurrent(lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* obs, const float* teacher_obs, int64_t n,
                             const float* std_, uint64_t seed, uint64_t call, int32_t deterministic, float* h_s, float* c_s, float* h_t, float* c_t,
                             const float* reset, float* actions, float* action_mean, float* teacher_actions, void* stream) {
  POLICY_ENTRY;
  if (!mem_s || !student || !teacher || !obs || !teacher_obs) return lg_policy_fail(LG_ERR_INVALID, "null network or row");
  int rc = rnn_check(mem_s, h_s, c_s, n);
  if (rc == LG_OK && mem_t) rc = rnn_check(mem_t, h_t, c_t, n);
  if (rc != LG_OK) return rc;
  if (student->h.dims[0] != mem_s->hidden || (mem_t && teacher->h.dims[0] != mem_t->hidden))
    return lg_policy_fail(LG_ERR_INVALID, "an MLP's input width is not its memory's hidden width");
  rc = distill_widths(student, teacher);
  if (rc != LG_OK || n == 0) return rc;
  DeviceScope ds_(mem_s->device);
  const float *top_s, *top_t;
  rc = rnn_step_heads(mem_s, obs, h_s, c_s, mem_t, teacher_obs, h_t, c_t, n, reset, (hipStream_t)stream, &top_s, &top_t);
  if (rc != LG_OK) return rc;
  return lg_distill_act(student, teacher, top_s, top_t, n, std_, seed, call, deterministic, actions, action_mean, teacher_actions, stream);
}

// both collectors: the loop is lg_policy_collect_distillation, at the end of this file
int lg_collect_distillation(lg_ctx* env, lg_mlp* student, lg_mlp* teacher, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                            const lg_obs_history* history, const lg_distill_rollout* rows, void* stream) {
  POLICY_ENTRY;
  return lg_policy_collect_distillation(env, 0, nullptr, student, nullptr, teacher, std, seed, first_call, T, history, rows, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, nullptr, nullptr, stream);
}

int lg_collect_distillation_recurrent(lg_ctx* env, lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* std, uint64_t seed,
                                      uint64_t first_call, int32_t T, const lg_obs_history* history, const lg_distill_rollout* rows, float* h_s0, float* c_s0,
                                      float* h_t0, float* c_t0, float* h_s, float* c_s, float* h_t, float* c_t, void* stream) {
  POLICY_ENTRY;
  return lg_policy_collect_distillation(env, 1, mem_s, student, mem_t, teacher, std, seed, first_call, T, history, rows, h_s0, c_s0, h_t0, c_t0, h_s, c_s, h_t, c_t,
                                        nullptr, stream);
}

}  // extern "C"


// ============================================================================================ the PPO collection loop (lgpolicy.h, lgrunner.h, lgrunner_privileged.h)
int lg_policy_reward_rows(lg_ctx* env, EnvRewardRows* rows) {
  void* p; int64_t shp[4]; int32_t nd, dt;
  if (lg_get_tensor(env, LG_T_REW_BUF, &p, shp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's reward rows: ") + lg_last_error(env));
  rows->rew = (const float*)p; rows->n = shp[0];
  if (lg_get_tensor(env, LG_T_EXTRAS_EPISODE, &p, shp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's episode extras: ") + lg_last_error(env));
  rows->extras = (const float*)p; rows->K = shp[0];
  return LG_OK;
}

// The one loop of every PPO collector; mem_a NULL = the feed-forward ActorCritic (no memory state, no hidden-state rows); hooks and the two modes:
// lg_policy_internal.h.  The step itself (lg_step_transition) writes the critic's stream: the env's row, O_c wide, stored in crit_rows and
// normalised in place by norm_c.  With one stream that is out->observations and the actor reads it too; with two it is the privileged rows, and
// the actor's row (O_a wide, out->observations, norm_a) is derived after each step from the env's own raw row, never from the stored one.
// Per step: act, physics, post-physics, [the actor's row: one launch or copy], [the normaliser step: paired, three launches, for two handles].
int lg_policy_collect_rollout(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call,
                              int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a,
                              float* c_a, float* h_c, float* c_c, const CollectHooks* hooks, void* stream) {
  DeviceScope ds_(actor->device);
  if (!out->observations || !out->actions || !out->rewards || !out->dones || !out->values || !out->actions_log_prob || !out->mu ||
      !out->sigma || !out->last_values) return lg_policy_fail(LG_ERR_INVALID, "null output row");
  const bool lstm_a = mem_a && mem_a->type == LG_RNN_LSTM, lstm_c = mem_a && mem_c->type == LG_RNN_LSTM;
  if (mem_a && (!hid->h_a || !hid->h_c || (lstm_a && !hid->c_a) || (lstm_c && !hid->c_c))) return lg_policy_fail(LG_ERR_INVALID, "null hidden-state row");
  const float* env_obs; int64_t n, Oc, Aenv;
  int rc = env_shape(env, &env_obs, &n, &Oc, &Aenv);
  if (rc == LG_OK && mem_a) rc = rnn_check(mem_a, h_a, c_a, n);
  if (rc == LG_OK && mem_a) rc = rnn_check(mem_c, h_c, c_c, n);
  if (rc != LG_OK) return rc;
  const CollectHooks hk = hooks ? *hooks : CollectHooks();
  const bool two = hk.privileged_observations != nullptr;
  if (hk.sensors && two) return lg_policy_fail(LG_ERR_UNSUPPORTED, "a sensor rig together with privileged observations (two streams) is not built");
  if (hk.sensors && lg_policy_sensor_env(hk.sensors) != env) return lg_policy_fail(LG_ERR_INVALID, "the sensor rig is attached to another env context");
  const int A = actor->h.dims[actor->h.L];
  const int64_t Oa = mem_a ? mem_a->input : actor->h.dims[0];
  if ((!two && Oa != Oc) || (mem_a ? mem_c->input : critic->h.dims[0]) != Oc || critic->h.dims[critic->h.L] != 1 || A != Aenv)
    return lg_policy_fail(LG_ERR_INVALID, two ? "network widths do not match the env (the critic reads the env's observation row, one action per DOF, scalar value)"
                                              : "network widths do not match the env (obs width, one action per DOF, scalar value)");
  lg_obsnorm *norm_a = two ? hk.normalizer : nullptr, *norm_c = two ? hk.normalizer_c : hk.normalizer;
  if (two) {
    if ((rc = derived_row_check(hk.history, Oa, Oc, "actor", ": its input is wider than that row")) != LG_OK) return rc;
    if (norm_a && lg_obsnorm_width(norm_a) != Oa) return lg_policy_fail(LG_ERR_INVALID, "the actor's normaliser does not have the actor's input width");
    if (norm_c && lg_obsnorm_width(norm_c) != Oc) return lg_policy_fail(LG_ERR_INVALID, "the critic's normaliser does not have the env's observation width");
    if (norm_a && norm_a == norm_c) return lg_policy_fail(LG_ERR_INVALID, "the actor and the critic need a normaliser each");
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t sa = mem_a ? (size_t)mem_a->num_layers * n * mem_a->hidden : 0, sc = mem_a ? (size_t)mem_c->num_layers * n * mem_c->hidden : 0;
  const size_t so = (size_t)n * Oa, sp = (size_t)n * Oc;
  EnvRewardRows env_rows;
  if ((hk.raw_rewards || hk.extras) && (rc = lg_policy_reward_rows(env, &env_rows)) != LG_OK) return rc;
  // a normaliser's carried row: row 0 of this collection when it holds one, the normalised row after the last step when the loop is done
  float *carried_a = nullptr, *carried_c = nullptr; bool valid_a = false, valid_c = false;
  if (norm_a && (rc = lg_obsnorm_carried_begin(norm_a, n, Oa, &carried_a, &valid_a)) != LG_OK) return rc;
  if (norm_c && (rc = lg_obsnorm_carried_begin(norm_c, n, Oc, &carried_c, &valid_c)) != LG_OK) return rc;
  float* crit_rows = two ? hk.privileged_observations : out->observations;
  const DerivedRow actor_row{hk.history, env_obs, n, Oc, Oa, first_call, stream};
  // row 0 of each stream: the carried row where one is held, else the clipped history (the column prefix) for the actor and the env's raw row.
  // Every later row of the critic's stream is written by the step itself, as are the reward (with the time-out bootstrap) and done rows
  if (two) {
    if (valid_a) POLICY_TRY(hipMemcpyAsync(out->observations, carried_a, so * 4, hipMemcpyDeviceToDevice, st));
    else if ((rc = derived_row(actor_row, -1, nullptr, out->observations)) != LG_OK) return rc;
  }
  POLICY_TRY(hipMemcpyAsync(crit_rows, valid_c ? carried_c : env_obs, sp * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(fill_sigma_kernel, dim3((unsigned)(((int64_t)T * n * A + 255) / 256)), dim3(256), 0, st, (int64_t)T * n, A, std, out->sigma);
  for (int t = 0; t < T; ++t) {
    const float* obs_t = out->observations + t * so;
    const float* crit_t = crit_rows + t * sp;
    float* act_t = out->actions + (size_t)t * n * A;
    float* dones_t = out->dones + (size_t)t * n;
    if (mem_a) {
      // RolloutStorage._save_hidden_states (rollout_storage.py:123-140): the state BEFORE this step's act (ppo.py:148-149)
      POLICY_TRY(hipMemcpyAsync(hid->h_a + t * sa, h_a, sa * 4, hipMemcpyDeviceToDevice, st));
      if (lstm_a) POLICY_TRY(hipMemcpyAsync(hid->c_a + t * sa, c_a, sa * 4, hipMemcpyDeviceToDevice, st));
      POLICY_TRY(hipMemcpyAsync(hid->h_c + t * sc, h_c, sc * 4, hipMemcpyDeviceToDevice, st));
      if (lstm_c) POLICY_TRY(hipMemcpyAsync(hid->c_c + t * sc, c_c, sc * 4, hipMemcpyDeviceToDevice, st));
      rc = lg_policy_act_recurrent(mem_a, actor, mem_c, critic, obs_t, crit_t, n, std, seed, first_call + (uint64_t)t, 0, h_a, c_a, h_c, c_c, nullptr, act_t,
                                   out->mu + (size_t)t * n * A, out->actions_log_prob + (size_t)t * n, out->values + (size_t)t * n, stream);
    } else {
      rc = lg_policy_act(actor, critic, obs_t, crit_t, n, std, seed, first_call + (uint64_t)t, 0, act_t, out->mu + (size_t)t * n * A,
                         out->actions_log_prob + (size_t)t * n, out->values + (size_t)t * n, stream);
    }
    if (rc != LG_OK) return rc;
    const bool more = t + 1 < T;
    // the critic's next row; after the last step into its normaliser's carried row (none: the env's own row serves)
    float* next_c = more ? crit_rows + (t + 1) * sp : carried_c;
    if (hk.sensors) {
      if ((rc = lg_policy_sensor_step(hk.sensors, act_t, next_c, out->values + (size_t)t * n, gamma, out->rewards + (size_t)t * n, dones_t, stream)) != LG_OK) return rc;
    } else {
      rc = lg_step_transition(env, act_t, next_c, out->values + (size_t)t * n, gamma, out->rewards + (size_t)t * n, dones_t, stream);
      if (rc != LG_OK) return lg_policy_fail(rc, std::string("lg_step_transition failed: ") + lg_last_error(env));
    }
    // two streams: the actor's next row; after the last step the un-normalised row goes to last_observations and its normalised copy to the carried row
    float *norm_out_a = nullptr, *next_a = nullptr;
    if (two) {
      norm_out_a = more ? out->observations + (t + 1) * so : carried_a;
      next_a = more ? norm_out_a : (hk.last_observations ? hk.last_observations : carried_a);
      if ((rc = derived_row(actor_row, t, dones_t, next_a)) != LG_OK) return rc;
    }
    if (norm_a && norm_c) rc = lg_obsnorm_step_pair(norm_a, next_a, Oa, norm_out_a, norm_c, next_c, Oc, next_c, n, hk.update, stream);
    else if (norm_a) rc = lg_obsnorm_step(norm_a, next_a, n, Oa, hk.update, norm_out_a, stream);
    else if (norm_c) rc = lg_obsnorm_step(norm_c, next_c, n, Oc, hk.update, next_c, stream);          // on_policy_runner.py:425-427
    if (rc != LG_OK) return rc;
    if (hk.raw_rewards) POLICY_TRY(hipMemcpyAsync(hk.raw_rewards + (size_t)t * n, env_rows.rew, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    if (hk.extras) POLICY_TRY(hipMemcpyAsync(hk.extras + (size_t)t * env_rows.K, env_rows.extras, (size_t)env_rows.K * 4, hipMemcpyDeviceToDevice, st));
    if (mem_a) {                                       // PPO.process_env_step ends with policy.reset(dones) (ppo.py:188)
      rc = lg_rnn_reset_rows(mem_a, h_a, c_a, dones_t, n, stream);
      if (rc == LG_OK) rc = lg_rnn_reset_rows(mem_c, h_c, c_c, dones_t, n, stream);
      if (rc != LG_OK) return rc;
    }
  }
  // last_values = critic(last obs) (ppo.py:186-192); a recurrent policy.evaluate goes through Memory.forward, so the critic memory advances once more
  const float* last = norm_c ? carried_c : env_obs;
  if (mem_a) {
    rc = lg_rnn_step(mem_c, last, n, h_c, c_c, nullptr, nullptr, stream);
    if (rc != LG_OK) return rc;
    last = h_c + (size_t)(mem_c->num_layers - 1) * n * mem_c->hidden;
  }
  rc = lg_mlp_forward(critic, last, n, out->last_values, stream);
  if (rc == LG_OK && out->returns && out->advantages)
    rc = lg_compute_returns(out->rewards, out->dones, out->values, out->last_values, T, n, gamma, lam, normalize_advantage, out->returns,
                            out->advantages, stream);
  if (rc != LG_OK) return rc;
  POLICY_TRY(hipGetLastError());
  if (norm_a) lg_obsnorm_carried_commit(norm_a);
  if (norm_c) lg_obsnorm_carried_commit(norm_c);
  return LG_OK;
}


// ============================================================================================ the distillation collection loop (lgpolicy.h, lgrunner_distill.h)
// The one loop of every distillation collector; recurrent = 0: the feed-forward StudentTeacher (no memory, no state pointers); hooks:
// lg_policy_internal.h.  The step itself (lg_step_transition) writes the teacher's stream: the env's row, O_t wide, normalised in place by
// normalizer_t.  The student's row (O_s wide, normalizer_s) is derived after each step from the env's own raw row, never from the stored one.
// Per step: act, physics, post-physics, the student's row (one launch or copy), [the normaliser step: paired, three launches, for two handles].
int lg_policy_collect_distillation(lg_ctx* env, int recurrent, lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* std, uint64_t seed,
                                   uint64_t first_call, int32_t T, const lg_obs_history* hist, const lg_distill_rollout* out, float* h_s0, float* c_s0, float* h_t0,
                                   float* c_t0, float* h_s, float* c_s, float* h_t, float* c_t, const DistillHooks* hooks, void* stream) {
  if (!env || (recurrent && !mem_s) || !student || !teacher || !std || !out || T <= 0) return lg_policy_fail(LG_ERR_INVALID, "null argument or T < 1");
  const float* env_obs; int64_t n, Ot, Aenv;
  int rc = env_shape(env, &env_obs, &n, &Ot, &Aenv);
  if (rc == LG_OK && mem_s) rc = rnn_check(mem_s, h_s, c_s, n);
  if (rc == LG_OK && mem_s && mem_t) rc = rnn_check(mem_t, h_t, c_t, n);
  if (rc != LG_OK) return rc;
  DeviceScope ds_(student->device);
  if (!out->observations || !out->privileged_observations || !out->actions || !out->privileged_actions || !out->rewards || !out->dones)
    return lg_policy_fail(LG_ERR_INVALID, "null output row");
  if ((rc = distill_widths(student, teacher)) != LG_OK) return rc;
  const int A = student->h.dims[student->h.L];
  const int64_t Os = mem_s ? mem_s->input : student->h.dims[0];
  if ((mem_t ? mem_t->input : teacher->h.dims[0]) != Ot || A != Aenv)
    return lg_policy_fail(LG_ERR_INVALID, "network widths do not match the env (the teacher reads the env's observation row, one action per DOF)");
  if (mem_s && (student->h.dims[0] != mem_s->hidden || (mem_t && teacher->h.dims[0] != mem_t->hidden)))
    return lg_policy_fail(LG_ERR_INVALID, "an MLP's input width is not its memory's hidden width");
  if ((rc = derived_row_check(hist, Os, Ot, "student", "")) != LG_OK) return rc;
  const DistillHooks hk = hooks ? *hooks : DistillHooks();
  lg_obsnorm *norm_s = hk.normalizer_s, *norm_t = hk.normalizer_t;
  if (norm_s && lg_obsnorm_width(norm_s) != Os) return lg_policy_fail(LG_ERR_INVALID, "the student's normaliser does not have the student's input width");
  if (norm_t && lg_obsnorm_width(norm_t) != Ot) return lg_policy_fail(LG_ERR_INVALID, "the teacher's normaliser does not have the env's observation width");
  if (norm_s && norm_s == norm_t) return lg_policy_fail(LG_ERR_INVALID, "the student and the teacher need a normaliser each");
  hipStream_t st = (hipStream_t)stream;
  EnvRewardRows env_rows;
  if ((hk.raw_rewards || hk.extras) && (rc = lg_policy_reward_rows(env, &env_rows)) != LG_OK) return rc;
  // a normaliser's carried row: row 0 of this collection when it holds one, the normalised row after the last step when the loop is done
  float *carried_s = nullptr, *carried_t = nullptr; bool valid_s = false, valid_t = false;
  if (norm_s && (rc = lg_obsnorm_carried_begin(norm_s, n, Os, &carried_s, &valid_s)) != LG_OK) return rc;
  if (norm_t && (rc = lg_obsnorm_carried_begin(norm_t, n, Ot, &carried_t, &valid_t)) != LG_OK) return rc;
  if (mem_s) {          // the state BEFORE step 0: what seeds policy.reset(hidden_states=...) of the update
    const size_t ss = (size_t)mem_s->num_layers * n * mem_s->hidden * 4, stt = mem_t ? (size_t)mem_t->num_layers * n * mem_t->hidden * 4 : 0;
    if (h_s0) POLICY_TRY(hipMemcpyAsync(h_s0, h_s, ss, hipMemcpyDeviceToDevice, st));
    if (c_s0 && mem_s->type == LG_RNN_LSTM) POLICY_TRY(hipMemcpyAsync(c_s0, c_s, ss, hipMemcpyDeviceToDevice, st));
    if (mem_t && h_t0) POLICY_TRY(hipMemcpyAsync(h_t0, h_t, stt, hipMemcpyDeviceToDevice, st));
    if (mem_t && c_t0 && mem_t->type == LG_RNN_LSTM) POLICY_TRY(hipMemcpyAsync(c_t0, c_t, stt, hipMemcpyDeviceToDevice, st));
  }
  const size_t so = (size_t)n * Os, sp = (size_t)n * Ot, sa = (size_t)n * A;
  const DerivedRow student_row{hist, env_obs, n, Ot, Os, first_call, stream};          // the history layer, or the head of the teacher's row
  // row 0 of each stream: the carried row where one is held, else the env's raw row for the teacher and the clipped history (the column prefix)
  POLICY_TRY(hipMemcpyAsync(out->privileged_observations, valid_t ? carried_t : env_obs, sp * 4, hipMemcpyDeviceToDevice, st));
  if (valid_s) POLICY_TRY(hipMemcpyAsync(out->observations, carried_s, so * 4, hipMemcpyDeviceToDevice, st));
  else if ((rc = derived_row(student_row, -1, nullptr, out->observations)) != LG_OK) return rc;
  for (int t = 0; t < T; ++t) {
    float* act_t = out->actions + t * sa;
    float* dones_t = out->dones + (size_t)t * n;
    if (mem_s) rc = lg_distill_act_recurrent(mem_s, student, mem_t, teacher, out->observations + t * so, out->privileged_observations + t * sp, n, std, seed,
                                             first_call + (uint64_t)t, 0, h_s, c_s, h_t, c_t, nullptr, act_t, nullptr, out->privileged_actions + t * sa, stream);
    else rc = lg_distill_act(student, teacher, out->observations + t * so, out->privileged_observations + t * sp, n, std, seed, first_call + (uint64_t)t, 0, act_t,
                             nullptr, out->privileged_actions + t * sa, stream);
    if (rc != LG_OK) return rc;
    const bool more = t + 1 < T;
    // the teacher's next row; after the last step into its normaliser's carried row (none: the env's own row serves).
    // Distillation.process_env_step (distillation.py:98-101) stores the env's reward as it is: no value row, no time-out bootstrap
    float* next_t = more ? out->privileged_observations + (t + 1) * sp : carried_t;
    rc = lg_step_transition(env, act_t, next_t, nullptr, 0.f, out->rewards + (size_t)t * n, dones_t, stream);
    if (rc != LG_OK) return lg_policy_fail(rc, std::string("lg_step_transition failed: ") + lg_last_error(env));
    // the student's next row; after the last step the un-normalised row goes to last_observations and its normalised copy to the carried row
    float* norm_out_s = more ? out->observations + (t + 1) * so : carried_s;
    float* next_s = more ? norm_out_s : (out->last_observations ? out->last_observations : carried_s);
    if ((rc = derived_row(student_row, t, dones_t, next_s)) != LG_OK) return rc;
    if (norm_s && norm_t) rc = lg_obsnorm_step_pair(norm_s, next_s, Os, norm_out_s, norm_t, next_t, Ot, next_t, n, hk.update, stream);
    else if (norm_s) rc = lg_obsnorm_step(norm_s, next_s, n, Os, hk.update, norm_out_s, stream);
    else if (norm_t) rc = lg_obsnorm_step(norm_t, next_t, n, Ot, hk.update, next_t, stream);          // on_policy_runner.py:425-427
    if (rc != LG_OK) return rc;
    if (hk.raw_rewards) POLICY_TRY(hipMemcpyAsync(hk.raw_rewards + (size_t)t * n, env_rows.rew, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    if (hk.extras) POLICY_TRY(hipMemcpyAsync(hk.extras + (size_t)t * env_rows.K, env_rows.extras, (size_t)env_rows.K * 4, hipMemcpyDeviceToDevice, st));
    if (mem_s) {                                       // policy.reset(dones) (distillation.py:105)
      rc = lg_rnn_reset_rows(mem_s, h_s, c_s, dones_t, n, stream);
      if (rc == LG_OK && mem_t) rc = lg_rnn_reset_rows(mem_t, h_t, c_t, dones_t, n, stream);
      if (rc != LG_OK) return rc;
    }
  }
  POLICY_TRY(hipGetLastError());
  if (norm_s) lg_obsnorm_carried_commit(norm_s);
  if (norm_t) lg_obsnorm_carried_commit(norm_t);
  return LG_OK;
}
