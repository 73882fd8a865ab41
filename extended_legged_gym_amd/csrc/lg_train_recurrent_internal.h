// lg_train_recurrent_internal.h -- the memory kernels of lg_train_recurrent.hip (forward with saved gates, one step backwards, rows x transposed
// tiling, the masters -> the lg_rnn images) for ONE memory, as host launch functions, and on top of them TrainMem: one trained memory with its
// carried state, and the host functions that run truncated BPTT through it (the estimator's trainer, lg_estimator_train.hip, and the recurrent
// student's, lg_distill_train_recurrent.hip, each hold one).  The kernels and those host functions live in lg_train_recurrent.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lg_rnn_tile.h"
#include "lg_train_internal.h"

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

// ---- one trained memory and its carried state
struct MemLayer {                    // one layer's workspaces for max_rows rows (step-major) and its transposed tilings
  float *gate[4], *hin, *cin, *cnew, *hnew, *dup, *Dih, *Dhh, *dh[2], *dc[2];
  float *wtx, *wth;
};

struct TrainMem {
  lg_rnn* rnn = nullptr;
  int device = 0, I = 0, H = 0, Gates = 0, ML = 0;
  int64_t max_rows = 0;
  MemLayer layer[RNN_MAX_LAYERS];
  float* zero_state = nullptr;       // (max_rows, H) zeros: the saved row of a step that enters from the step before, and the dones of a sequence without any
  float *carry_h = nullptr, *carry_c = nullptr, *cur_h = nullptr, *cur_c = nullptr;          // (ML, max_rows, H): at the sequence's step 0 / after the last group
  int64_t carry_n = 0;               // rows of the carry; 0: none yet (the next call opens a zero one)
  RnnRetile retile[RNN_MAX_LAYERS + 1];
  RnnRetile* d_retile = nullptr; int64_t retile_big = 0;
};

struct MemSpan {                     // steps [t0, t0 + nsteps) (time index modulo T) of a (T, N) sequence as one batch of nsteps * N rows
  int64_t T, N, t0, nsteps;
  const float* dones;                // (T, N), or NULL: no episode ends inside the sequence
};

// the state and every layer's workspaces for c->max_rows rows, owned by c; false + message on failure
bool mem_alloc(TrainCore* c, TrainMem* M, lg_rnn* rnn);
// layer l's tensors at *off of the flat vector (advanced) in the order weight_ih, weight_hh, bias_ih, bias_hh: the offsets of its two segments and its
// entry of the retile table; then, once, the table's upload
void mem_place_layer(TrainMem* M, int l, TrainSeg& Si, TrainSeg& Sh, int64_t* off);
bool mem_upload_retile(TrainCore* c, TrainMem* M);
int mem_retile(const TrainMem* M, const float* theta, hipStream_t st);
// refuses N rows while a carry of another row count stands
int mem_check_rows(const TrainMem* M, int64_t N);
// the first call after a reset: zero carry and running state for N rows
int mem_open_carry(TrainMem* M, int64_t N, hipStream_t st);
// forward through time.  Layer 0 reads rows of width I at x0 + k N I, k = the step's time index (x0_by_time) or its index in the batch.  A step with time
// index 0 enters with the carry, the batch's first step otherwise with the running state, both as constants; every other step with the step
// before's state, zero where its dones ended the episode.
void mem_forward(const TrainMem* M, const MemSpan& W, const float* x0, bool x0_by_time, hipStream_t st);
// dL/d(top layer's h') from the deltas of layer 0 of the network that reads it
void mem_top_matmul(const TrainMem* M, const TrainNet& head, int64_t n, hipStream_t st);
// backwards through time; dx0 (nsteps N, I): where layer 0 propagates to, or NULL (its inputs are data)
void mem_backward(const TrainMem* M, const MemSpan& W, float* dx0, hipStream_t st);
// the running state <- the memory after the span's last step (the owner then applies the dones); the carry <- the running state (an update's end)
int mem_keep_running(TrainMem* M, const MemSpan& W, hipStream_t st);
int mem_keep_carry(TrainMem* M, hipStream_t st);
// the bodies of <prefix>_get_carry / _set_carry / _reset_carry; kind: how the caller's h / c are reached (host arrays, or hipMemcpyDefault).  M may be NULL.
int64_t mem_get_carry(TrainMem* M, float* h, float* c, int64_t capacity_rows, int32_t running, hipMemcpyKind kind, void* stream);
int mem_set_carry(TrainMem* M, const float* h, const float* c, int64_t N, hipMemcpyKind kind, void* stream);
int mem_reset_carry(TrainMem* M);
