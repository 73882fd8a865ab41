// lg_chain_body.h — the body of the chain kernels (lg_step.hip: physics_kernel_chain for planes, height grids and grid meshes, physics_kernel_chain_bvh for
// the other triangle meshes).  Not a header: it is included inside each kernel's braces, where MODE, TMESH, MQ (CH_MESH_*, lg_chain.h), HELP, the
// kernel's parameters and its LDS (cst, lmod, XST / xst) are in scope.  One text for both, and the grid-mesh kernels compile exactly as they did when the
// body was written inline.
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // HALVES (the helper-wave instance at <= 16 envs per workgroup, i.e. N <= 4096): the upper 32 lanes of every wave would be idle copies; instead they MIRROR
  // the lower 32 -- same env, same leg, same arithmetic, same slot-record rows -- and the work that is per contact slot is split between the halves:
  // a helper wave detects two slots at once, the main wave sets up the even slots on its lower and the odd slots on its upper half.
  const bool halves = HELP && epb * GRP <= 32;
  const int le = halves ? (lane & 31) : lane;              // the lane's row in the slot records and in the published state
  const int half = halves ? (lane >> 5) : -1;
  const int kq = blockIdx.x * epb + le / GRP;
  const int l = lane % GRP;
  const bool live = kq < n && le / GRP < epb;
  const bool valid = live && half <= 0;                   // (the lower half stores)
  const int krow = live ? kq : n - 1;
  const int e = ids ? ids[krow] : krow;
  const lg_robot_model* __restrict__ m = &C->model;
  const lg_config& g = C->cfg;
  fill_leg_model(lmod, C->lmod, threadIdx.x, blockDim.x);
  lds_barrier();
  const LegModel lm_{lmod, l};
  if (HELP && wv > 0) {
    // ---- helper wave: per substep, the kinematics of the state the main wave published and the detection of this wave's slots
    PhysParams P;
    P.dt = g.sim_dt; P.grav = v3(g.gravity[0], g.gravity[1], g.gravity[2]); P.iters = g.solver_iterations;
    P.contact_offset = g.contact_offset; P.max_depen = g.max_depenetration_velocity; P.erp = g.erp; P.cfm = g.cfm; P.solver = g.solver_type; P.fric = g.friction_model;
    P.terrain_mu = C->terrain_mu; P.slide_mask = C->slide_mask; P.slot_perm = 0x76543210u; P.cache_reach = LG_MESH_CACHE_REACH;
    const TerrainView T = C->ter;
#pragma unroll 1
    for (int sub = 0; sub < nsub; ++sub) {
      lds_barrier();                                     // (A) the main wave has published root, q, qd of this substep
      float r13[13], qq[NJ], qdd[NJ];
      // (halves: a helper wave's two halves detect two slots of the same 32 rows at once -- the four slots take ONE slot's time on three waves instead of two)
      const float* x = xst + le * XST;
#pragma unroll
      for (int i = 0; i < 13; ++i) r13[i] = x[i];
#pragma unroll
      for (int j = 0; j < NJ; ++j) { qq[j] = x[13 + j]; qdd[j] = x[13 + NJ + j]; }
      const M3 Rb = quat_to_mat(r13 + 3);
      const V3 pb = v3(r13[0], r13[1], r13[2]), vb = v3(r13[7], r13[8], r13[9]), wb = v3(r13[10], r13[11], r13[12]);
      LegKin k;
      leg_kinematics(lm_, Rb, pb, vb, wb, qq, qdd, k);
      // slots dealt round-robin over the three helper waves (CH_NCP = 4: wave 1 takes slots 0 and 3)
      if (halves) {
        const int sl = lane < 32 ? wv - 1 : wv + 2;
        if (sl < CH_NCP) ch_detect_slot<TMESH, MQ>(sl, lm_, T, P, k, Rb, pb, cst, le);
      } else {
#pragma unroll 1
        for (int sl = wv - 1; sl < CH_NCP; sl += 3) ch_detect_slot<TMESH, MQ>(sl, lm_, T, P, k, Rb, pb, cst, lane);
      }
      lds_barrier();                                     // (A2) detection blocks complete
    }
    return;
  }
  QuadState s;
#pragma unroll
  for (int i = 0; i < 13; ++i) s.root[i] = C->root[(size_t)e * 13 + i];
  float last_qd[NJ], act[NJ], tau[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    s.q[j] = C->dof[((size_t)e * NDOF + NJ * l + j) * 2]; s.qd[j] = C->dof[((size_t)e * NDOF + NJ * l + j) * 2 + 1];
    last_qd[j] = C->last_dof_vel[(size_t)e * NDOF + NJ * l + j];
    act[j] = 0.f; tau[j] = 0.f;
  }
  if (MODE != 1) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float a = actions_in ? actions_in[(size_t)krow * act_stride + NJ * l + j] : C->actions[(size_t)e * NDOF + NJ * l + j];
      a = fminf(fmaxf(a, -g.clip_actions), g.clip_actions);        // LR:93-94
      act[j] = a;
      if (valid && actions_in) C->actions[(size_t)e * NDOF + NJ * l + j] = a;
    }
  }
  if (MODE == 2) {
    ch_leg_torques(g, lm_, act, s.q, s.qd, last_qd, tau);
    if (valid) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) C->torques[(size_t)e * NDOF + NJ * l + j] = tau[j];
    }
    return;
  }
  PhysParams P;
  P.dt = g.sim_dt; P.grav = v3(g.gravity[0], g.gravity[1], g.gravity[2]); P.iters = g.solver_iterations;
  P.contact_offset = g.contact_offset; P.max_depen = g.max_depenetration_velocity; P.erp = g.erp; P.cfm = g.cfm; P.solver = g.solver_type; P.fric = g.friction_model;
  P.terrain_mu = C->terrain_mu; P.slide_mask = C->slide_mask; P.slot_perm = 0x76543210u; P.cache_reach = LG_MESH_CACHE_REACH;
  const TerrainView T = C->ter;
  const SelfCol scol{C->sc_pairs, C->n_sc, nullptr, nullptr};
  const float mu_robot = C->friction[e], madd = C->mass_added[e];
  V3 fbody[NJ + 2];
#pragma unroll
  for (int b = 0; b < NJ + 2; ++b) fbody[b] = v3(0, 0, 0);
  bool fault = false;
#pragma unroll 1
  for (int sub = 0; sub < nsub; ++sub) {
    if (MODE == 0) ch_leg_torques(g, lm_, act, s.q, s.qd, last_qd, tau);
    else {
#pragma unroll
      for (int j = 0; j < NJ; ++j) tau[j] = C->torques[(size_t)e * NDOF + NJ * l + j];
    }
    float root0[7], q0[NJ];
#pragma unroll
    for (int i = 0; i < 7; ++i) root0[i] = s.root[i];
#pragma unroll
    for (int j = 0; j < NJ; ++j) q0[j] = s.q[j];
    if (HELP) {
      float* x = xst + le * XST;                           // (halves: both mirrors write the same values)
#pragma unroll
      for (int i = 0; i < 13; ++i) x[i] = s.root[i];
#pragma unroll
      for (int j = 0; j < NJ; ++j) { x[13 + j] = s.q[j]; x[13 + NJ + j] = s.qd[j]; }
      lds_barrier();                                     // (A)
    }
    chain_substep<TMESH, HELP, MQ>(m, lm_, T, P, le, cst, s, tau, mu_robot, madd, sub == nsub - 1 ? fbody : nullptr, scol, half);
    // fault guard: a non-finite or diverged state is rolled back to the pre-step pose at rest and flagged for termination
    float acc = 0.f, acc0 = 0.f;
#pragma unroll
    for (int i = 0; i < 13; ++i) acc += s.root[i] * 0.f;
#pragma unroll
    for (int i = 7; i < 13; ++i) acc += fabsf(s.root[i]) < 1e3f ? 0.f : 1.f;
    if (TMESH) {
      acc += (s.root[0] < C->mesh_lo[0] - LG_MESH_OOB_MARGIN || s.root[0] > C->mesh_hi[0] + LG_MESH_OOB_MARGIN ||
              s.root[1] < C->mesh_lo[1] - LG_MESH_OOB_MARGIN || s.root[1] > C->mesh_hi[1] + LG_MESH_OOB_MARGIN ||
              s.root[2] < C->mesh_lo[2] - LG_MESH_OOB_MARGIN) ? 1.f : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) { acc += s.q[j] * 0.f + s.qd[j] * 0.f; acc0 += q0[j] * 0.f; }
#pragma unroll
    for (int i = 0; i < 7; ++i) acc0 += root0[i] * 0.f;
    acc = grp_sum(acc); acc0 = grp_sum(acc0);
    if (!(acc == 0.f)) {
      const bool ok0 = acc0 == 0.f;
      fault = true;
#pragma unroll
      for (int i = 0; i < 13; ++i)
        s.root[i] = ok0 ? (i < 7 ? root0[i] : 0.f) : g.base_init_state[i] + (i < 3 ? C->origins[(size_t)e * 3 + i] : 0.f);
#pragma unroll
      for (int j = 0; j < NJ; ++j) { s.q[j] = ok0 ? q0[j] : lm_.f(LM_DEFAULT_POS + j); s.qd[j] = 0.f; }
#pragma unroll
      for (int b = 0; b < NJ + 2; ++b) fbody[b] = v3(0, 0, 0);
    }
  }
  if (!valid) return;
  if (fault && l == 0) C->reset_buf[e] = 2;
  if (l == 0) {
#pragma unroll
    for (int i = 0; i < 13; ++i) C->root[(size_t)e * 13 + i] = s.root[i];
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    C->dof[((size_t)e * NDOF + NJ * l + j) * 2] = s.q[j];
    C->dof[((size_t)e * NDOF + NJ * l + j) * 2 + 1] = s.qd[j];
    if (MODE == 0) C->torques[(size_t)e * NDOF + NJ * l + j] = tau[j];
  }
  const int per_leg = C->per_leg, B = C->B;
  {
    float* cf = C->cforce + (size_t)e * B * 3;
    if (l == 0) { cf[0] = fbody[0].x; cf[1] = fbody[0].y; cf[2] = fbody[0].z; }
    float* cl = cf + (size_t)(1 + per_leg * l) * 3;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      V3 f = fbody[1 + j];
      if (j == NJ - 1 && per_leg == NJ) f = f + fbody[NJ + 1];      // no separate foot body: its spheres report on the last link
      cl[3 * j] = f.x; cl[3 * j + 1] = f.y; cl[3 * j + 2] = f.z;
    }
    if (per_leg == NJ + 1) { cl[3 * NJ] = fbody[NJ + 1].x; cl[3 * NJ + 1] = fbody[NJ + 1].y; cl[3 * NJ + 2] = fbody[NJ + 1].z; }
  }
  write_rigid_body_state(C, lm_, e, l, s.root, s.q, s.qd);
