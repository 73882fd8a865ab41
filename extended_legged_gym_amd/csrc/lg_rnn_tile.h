// lg_rnn_tile.h — the device tile of one LSTM / GRU layer step, shared by the inference kernel (lg_policy.hip: rnn_layer_kernel) and the
// training forward (lg_train_recurrent.hip).  One compile-time switch, SAVE, separates them: the k-chain, its order and the gate epilogue are
// the same code, so the training forward computes lg_rnn_step's values bit for bit, and the SAVE = false instance is the inference kernel as
// it was.  A third switch, SEED, is layer 0 of a wide memory (lg_rnn_create_wide): the x part of the chain was walked by rnn_wide_xproj_kernel
// and left unrounded in fp32 (`seed`, (n, G * 16 nch)); the accumulators start from it and the chain goes on over the h blocks, so the sum is the
// narrow chain cut at the x / h boundary.  The layer descriptor of such a layer has I = Ip = nbx = 0: the image holds h alone.  The SEED = false
// instances never read `seed` and are the kernels as they were.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lg_device.h"
#include "lg_policy_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct RnnStepArgs {                 // one memory's operands of a layer step (device pointers)
  RnnLayerDev L;
  const float* x;                    // (n, I): the observation, or the h' of the layer below
  float* h;                          // (n, H) of this layer, updated in place
  float* c;                          // (n, H) or null (GRU)
  const float* reset;                // (n) or null
  float* out;                        // (n, H) or null: a copy of h'
};

// SAVE: where a step's entering state comes from and where its gates go; every pointer is at THIS step's first row, (n, H) row-major.  A row
// whose previous step ended an episode (dprev != 0), and every row of the first step (dprev null), enters with the saved hidden row (hs, cs);
// every other row with its own state after the previous step (hprev, cprev).  S.h, S.c, S.reset and S.out are unused.
struct RnnSaveArgs {
  const float* hs; const float* cs;
  const float* hprev; const float* cprev;
  const float* dprev;                // (n) or null
  float* gate[4];                    // post-nonlinearity i f g o; GRU: r z n and the hidden-side pre-activation W_hn h + b_hn
  float* hin; float* cin;            // the entering state (cin null for a GRU)
  float* cnew; float* hnew;          // the new state (cnew null for a GRU)
};

LG_DEV float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// blocks [kb0, kb1) of a chunk: G gate fragments per block; gate 2 of a GRU accumulates into acc[NSLOT] (2: x part, 3: h part).
// Two fragment sets: the loads of the next block are issued before the 8 G MFMAs of the current one (sched_barrier pins that order, as in
// MLP_BLOCK), so the wait in front of a block's first MFMA is for loads issued a whole block earlier.
template <int G>
struct RnnFrag { float4 w[G], a0, a1; };
template <int G>
LG_DEV void rnn_load(RnnFrag<G>& f, const float4* __restrict__ wc, const float4* ap, int kb) {
#pragma unroll
  for (int g = 0; g < G; ++g) f.w[g] = wc[((size_t)kb * G + g) * 64];
  f.a0 = ap[kb * 128]; f.a1 = ap[kb * 128 + 64];
}
template <int G, int NSLOT>
LG_DEV void rnn_mfma(f32x4 (&acc)[4][2], const RnnFrag<G>& f) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float x0 = s == 0 ? f.a0.x : s == 1 ? f.a0.y : s == 2 ? f.a0.z : f.a0.w;
    const float x1 = s == 0 ? f.a1.x : s == 1 ? f.a1.y : s == 2 ? f.a1.z : f.a1.w;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float wv = s == 0 ? f.w[g].x : s == 1 ? f.w[g].y : s == 2 ? f.w[g].z : f.w[g].w;
      const int slot = (G == 3 && g == 2) ? NSLOT : g;
      acc[slot][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, wv, acc[slot][0], 0, 0, 0);
      acc[slot][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, wv, acc[slot][1], 0, 0, 0);
    }
  }
}
template <int G, int NSLOT>
LG_DEV void rnn_blocks(f32x4 (&acc)[4][2], const float4* __restrict__ wc, const float4* ap, int kb0, int kb1, int kzero) {
  if (kb0 >= kb1) return;
  RnnFrag<G> f0, f1;
  rnn_load<G>(f0, wc, ap, kb0);
  for (int kb = kb0; kb < kb1; kb += 2) {
    // an odd count's second half multiplies the chunk's all-zero weight block (kzero): no branch around the MFMAs, so the loads stay where they are
    const bool two = kb + 1 < kb1, more = kb + 2 < kb1;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < G; ++g) f1.w[g] = wc[((size_t)(two ? kb + 1 : kzero) * G + g) * 64];
    f1.a0 = ap[(two ? kb + 1 : kb) * 128]; f1.a1 = ap[(two ? kb + 1 : kb) * 128 + 64];
    __builtin_amdgcn_sched_barrier(0);
    rnn_mfma<G, NSLOT>(acc, f0);
    __builtin_amdgcn_sched_barrier(0);
    rnn_load<G>(f0, wc, ap, more ? kb + 2 : kb);             // past the end: an in-bounds block, unused
    __builtin_amdgcn_sched_barrier(0);
    rnn_mfma<G, NSLOT>(acc, f1);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool GRU, bool SAVE, bool SEED = false>
LG_DEV void rnn_tile(const RnnStepArgs& S, const RnnSaveArgs& V, int64_t row0, int64_t n, float* img, const float* __restrict__ seed = nullptr) {
  const RnnLayerDev& R = S.L;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = R.I, H = R.H, Ip = R.Ip, Kp = R.nb * 16;
  // stage [x ; h] of this workgroup's 32 rows.  The workgroup owns WHOLE rows and reads every h it will need here, before the barrier; h'
  // (and c') are stored only after it, and no other workgroup touches these rows: the state is updated in place without a second buffer.
  // A row whose reset flag is set enters with h = 0 (and c = 0 in the epilogue): Memory.reset(dones), memory.py:35-51, folded into the step.
  for (int base = 0; base < MLP_ROWS * Kp; base += 8 * MLP_THREADS) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * MLP_THREADS + tid, r = idx / Kp, k = idx - r * Kp;
      const int64_t row = row0 + r;
      float val = 0.f;
      if (idx < MLP_ROWS * Kp && row < n) {
        if (k < I) val = S.x[row * I + k];
        else if (k >= Ip && k < Ip + H) {
          if constexpr (SAVE) val = (!V.dprev || V.dprev[row] != 0.f) ? V.hs[row * H + (k - Ip)] : V.hprev[row * H + (k - Ip)];
          else val = (S.reset && S.reset[row] != 0.f) ? 0.f : S.h[row * H + (k - Ip)];
        }
      }
      v[u] = val;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * MLP_THREADS + tid, r = idx / Kp, k = idx - r * Kp;
      if (idx < MLP_ROWS * Kp) img[IMG(r, k)] = v[u];
    }
  }
  lds_barrier();
  constexpr int G = GRU ? 3 : 4;
  const float4* ap = reinterpret_cast<const float4*>(img) + (lane & 15) * 4 + (lane >> 4);
  const int Hp = 16 * R.nch;
  for (int c = wv; c < R.nch; c += MLP_THREADS / 64) {
    f32x4 acc[4][2];
#pragma unroll
    for (int g = 0; g < 4; ++g) { acc[g][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if constexpr (SEED) {                                      // slots 0 .. G - 1 from the projection; a GRU's slot 3 (the hidden side of n) from zero
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int64_t row = row0 + 4 * (lane >> 4) + i + 16 * hf;
            if (row < n) acc[g][hf][i] = seed[(row * G + g) * Hp + c * 16 + (lane & 15)];
          }
    }
    const float4* wc = reinterpret_cast<const float4*>(R.w) + (size_t)c * (R.nb + 1) * G * 64 + lane;
    if (GRU) {
      rnn_blocks<G, 2>(acc, wc, ap, 0, R.nbx, R.nb);
      rnn_blocks<G, 3>(acc, wc, ap, R.nbx, R.nb, R.nb);
    } else {
      rnn_blocks<G, 2>(acc, wc, ap, 0, R.nb, R.nb);
    }
    const int col = c * 16 + (lane & 15);
    const float b0 = R.b[col], b1 = R.b[Hp + col], b2 = R.b[2 * Hp + col], b3 = R.b[3 * Hp + col];
    // epilogue: C[m = 4 * (lane >> 4) + i (+ 16)][col]
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * (lane >> 4) + i + 16 * hf;
        const int64_t row = row0 + m;
        if (col >= H || row >= n) continue;
        float hn;
        if (GRU) {
          const float r = sigmoidf_(acc[0][hf][i] + b0), z = sigmoidf_(acc[1][hf][i] + b1);
          const float ng = tanhf((acc[2][hf][i] + b2) + r * (acc[3][hf][i] + b3));
          const float hold = img[IMG(m, Ip + col)];                 // the h this step used (after the reset mask)
          hn = (1.f - z) * ng + z * hold;
          if constexpr (SAVE) {
            const int64_t e = row * H + col;
            V.gate[0][e] = r; V.gate[1][e] = z; V.gate[2][e] = ng; V.gate[3][e] = acc[3][hf][i] + b3; V.hin[e] = hold;
          }
        } else {
          const float ig = sigmoidf_(acc[0][hf][i] + b0), fg = sigmoidf_(acc[1][hf][i] + b1);
          const float gg = tanhf(acc[2][hf][i] + b2), og = sigmoidf_(acc[3][hf][i] + b3);
          float cold;
          if constexpr (SAVE) cold = (!V.dprev || V.dprev[row] != 0.f) ? V.cs[row * H + col] : V.cprev[row * H + col];
          else cold = (S.reset && S.reset[row] != 0.f) ? 0.f : S.c[row * H + col];
          const float cn = fg * cold + ig * gg;
          if constexpr (SAVE) {
            const int64_t e = row * H + col;
            V.gate[0][e] = ig; V.gate[1][e] = fg; V.gate[2][e] = gg; V.gate[3][e] = og; V.hin[e] = img[IMG(m, Ip + col)]; V.cin[e] = cold; V.cnew[e] = cn;
          } else {
            S.c[row * H + col] = cn;
          }
          hn = og * tanhf(cn);
        }
        if constexpr (SAVE) {
          V.hnew[row * H + col] = hn;
        } else {
          S.h[row * H + col] = hn;
          if (S.out) S.out[row * H + col] = hn;
        }
      }
  }
}
