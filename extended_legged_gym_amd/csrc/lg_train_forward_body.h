// lg_train_forward_body.h — the body of the training forward kernels of lg_train.hip, included once per kernel with PPO_FORWARD_WIDE 0 (ppo_forward_kernel)
// and 1 (ppo_wide_forward_kernel: a trainer one of whose networks has more than MLP_MAXW inputs).  A body in a header and not a template function: a
// TrainNet handed on by reference is copied to scratch, while the kernel's own parameters are read where they lie.  Parameters in scope: NA, NC, obs,
// cobs, idx, n.
//
// The wide first layer is the split-K layer of mlp_wide_first_layer (lg_policy.hip): the gathered rows are staged in slabs of MLP_MAXW columns, and a wave
// keeps the accumulators of all its chunks across the slabs, so every output is the same single k-ascending chain and the saved activations stay
// lg_mlp_forward's bit for bit.
  __shared__ __attribute__((aligned(16))) float buf0[MLP_IMG];
  __shared__ __attribute__((aligned(16))) float buf1[MLP_IMG];
  const TrainNet& M = blockIdx.y == 0 ? NA : NC;
  const float* __restrict__ rows = blockIdx.y == 0 ? obs : cobs;
  const int64_t row0 = (int64_t)blockIdx.x * MLP_ROWS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* in = buf0; float* out = buf1;
  int l0 = 0;
  if (PPO_FORWARD_WIDE && M.fkpad[0] > MLP_MAXW) {
    constexpr int NC0 = MLP_MAXW / 16 / (MLP_THREADS / 64);           // chunks of a wave: layer 1 is at most MLP_MAXW wide
    const int K0p = M.fkpad[0], nblk0 = K0p >> 4, nch = M.fnch[0];
    const float4* ap = reinterpret_cast<const float4*>(buf0) + (lane & 15) * 4 + (lane >> 4);
    const float4* wl = reinterpret_cast<const float4*>(M.fw[0]) + lane;
    f32x4 acc[NC0][2];
#pragma unroll
    for (int ci = 0; ci < NC0; ++ci) { acc[ci][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[ci][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int k0 = 0; k0 < K0p; k0 += MLP_MAXW) {
      const int Kp = K0p - k0 < MLP_MAXW ? K0p - k0 : MLP_MAXW;
      if (k0) lds_barrier();                                          // every wave has read the slab before
      stage_rows(rows, idx, M.dims[0], Kp, row0, n, buf0, k0);
      lds_barrier();
#pragma unroll
      for (int ci = 0; ci < NC0; ++ci) {
        const int c = wv + ci * (MLP_THREADS / 64);
        if (c < nch) chunk_chain(wl + ((size_t)c * nblk0 + (k0 >> 4)) * 64, ap, Kp >> 4, acc[ci][0], acc[ci][1]);
      }
    }
#pragma unroll
    for (int ci = 0; ci < NC0; ++ci) {
      const int c = wv + ci * (MLP_THREADS / 64);
      if (c < nch) forward_chunk_out(M.fb[0], M.a[1], M.dims[1], M.L == 1, M.act, c, acc[ci][0], acc[ci][1], buf1, row0, n);
    }
    lds_barrier();
    in = buf1; out = buf0; l0 = 1;
  } else {
    stage_rows(rows, idx, M.dims[0], M.fkpad[0], row0, n, buf0);
    lds_barrier();
  }
  for (int l = l0; l < M.L; ++l) {
    const int nblk = M.fkpad[l] >> 4, nch = M.fnch[l], nout = M.dims[l + 1];
    const bool last = l == M.L - 1;
    const float4* ap = reinterpret_cast<const float4*>(in) + (lane & 15) * 4 + (lane >> 4);
    const float4* wl = reinterpret_cast<const float4*>(M.fw[l]) + lane;
    float* save = M.a[l + 1];
    for (int c = wv; c < nch; c += MLP_THREADS / 64) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      chunk_chain(wl + (size_t)c * nblk * 64, ap, nblk, acc0, acc1);
      forward_chunk_out(M.fb[l], save, nout, last, M.act, c, acc0, acc1, out, row0, n);
    }
    lds_barrier();
    float* t = in; in = out; out = t;
  }
