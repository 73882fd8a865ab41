// lg_train_recurrent_internal.h -- the memory kernels of lg_train_recurrent.hip (forward with saved gates, one step backwards, rows x transposed
// tiling, the masters -> the lg_rnn images) for ONE memory, as host launch functions: the estimator's trainer (lg_estimator_train.hip) runs truncated
// BPTT through them.  The kernels themselves live in lg_train_recurrent.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lg_rnn_tile.h"

struct RowsMatArgs {
  const float* A; int K, nbk;        // (n, K) and the k-blocks per chunk of the tiling
  const float* wt; int nch, nout;
  float* out;                        // (n, nout)
};

struct RnnBackArgs {                 // one memory's operands of a backward layer step; row pointers at THIS step's first row
  int gru, I, H, K, nbk;             // K = G H; nbk = K / 16 rounded up
  int nchx, nchh;                    // 16-column chunks of dx (0: the layer reads observations, no dx) and of dh_prev
  const float* wtx; const float* wth;
  const float* gate[4]; const float* hin; const float* cin; const float* cnew;
  const float* dup;                  // (n, H): dL/dh' from above (the MLP, or the layer above's dx)
  const float* dh_in; const float* dc_in;          // the carries out of step t + 1, or null
  const float* dprev;                // dones of step t - 1 (n), or null (t == 0): rows that entered from a saved row
  float* dh_out; float* dc_out;      // the carries into step t - 1
  float* dx;                         // (n, I) or null
  float* Dih; float* Dhh;            // (n, K): the gate derivatives as the weight gradients of weight_ih / weight_hh take them (LSTM: Dhh == Dih)
};

struct RnnRetile {                   // one memory layer's forward images and where its masters sit in the flat vector
  float* w; float* b;
  int G, I, H, Ip, nb, nch;
  int64_t wih, whh, bih, bhh;
};

// one step of one layer forward with SAVE (lg_rnn_tile.h), backwards, and (n, K) x tiling -> (n, nout)
void rec_launch_forward_one(const RnnStepArgs& S, const RnnSaveArgs& V, int64_t n, hipStream_t st);
void rec_launch_backward_one(const RnnBackArgs& B, int64_t n, hipStream_t st);
void rec_launch_rows_matmul_one(const RowsMatArgs& M, int64_t n, hipStream_t st);
// tab (device, count entries; big: the largest element count of an entry): the masters theta -> the forward images and bias rows
void rec_launch_retile(const RnnRetile* tab, int count, int64_t big, const float* theta, hipStream_t st);
