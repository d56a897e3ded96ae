// armenv_learner_kernels.inc -- the nine kernels of the fused updates (armenv_learner.h), included three times by that header:
//   LRN_POP 0   gemm_kernel, actor_back_kernel, adam_kernel (shared by every update) and the per-row heads actor_head_kernel,
//               critic_head_kernel (TD3), daddpg_actor_head_kernel, daddpg_critic_head_kernel (DADDPG), datd3_actor_head_kernel,
//               datd3_critic_head_kernel (DATD3 / DARC): one learner
//   LRN_POP 1   the *_pop_kernel forms of armenv_td3_pop_update, armenv_daddpg_pop_update and armenv_datd3_pop_update: grid
//               (workgroups of one member, members); member p = blockIdx.y works on member 0's problem with every operand moved by
//               p times its member stride (in elements), and draws its target-policy noise with key seed + p.  The strides are a
//               second kernel argument.
//   LRN_POP 2   the *_pop_hyper_kernel forms of the armenv_*_pop_update_hyper entry points: the population form of exactly the
//               kernels that read a hyper-parameter a member may have of its own -- adam (step_size, tau, loss_w1), the three critic
//               heads (gamma; DATD3 / DARC: w_min, w_max, reg) and the TD3 and DATD3 actor heads (policy_noise, noise_clip) -- with
//               every such scalar taken from a per-member table (MemberTable, further by-value kernel arguments) at blockIdx.y.  A
//               uniform index into the kernel-argument segment: a scalar load, no scratch.  gemm, actor_back and the DADDPG actor
//               head read none and have no such form.
// One text, three compilations: the population forms are compile-time variants, the single-learner kernels hold no member arithmetic,
// and all run the same operations in the same order, which is what makes member p of a population update equal the single update
// bit for bit.
#if LRN_POP == 2
#define LRN_KERNEL(name) name##_pop_hyper_kernel
#define LRN_POP_PARAM(decl) , decl
#define LRN_HYPER_PARAM(...) , __VA_ARGS__
#define LRN_MEMBER(ptr, stride) ((ptr) + (int64_t)blockIdx.y * (stride))
#elif LRN_POP
#define LRN_KERNEL(name) name##_pop_kernel
#define LRN_POP_PARAM(decl) , decl
#define LRN_HYPER_PARAM(...)
#define LRN_MEMBER(ptr, stride) ((ptr) + (int64_t)blockIdx.y * (stride))     // member blockIdx.y's `ptr`
#else
#define LRN_KERNEL(name) name##_kernel
#define LRN_POP_PARAM(decl)
#define LRN_HYPER_PARAM(...)
#define LRN_MEMBER(ptr, stride) ptr
#endif
#define LRN_OWN(field, table) P.field = table.v[blockIdx.y]     // LRN_POP 2: member blockIdx.y's own value of a scalar of P

#if LRN_POP < 2
__global__ __launch_bounds__(256) void LRN_KERNEL(gemm)(GemmList L LRN_POP_PARAM(GemmStrideList S)) {
  __shared__ float As[LRN_TK][LRN_TM + 4];
  __shared__ float Bs[LRN_TK][LRN_TN + 4];
  int pi = 0;
  while (pi + 1 < L.n && (int)blockIdx.x >= L.g[pi + 1].first_block) ++pi;
#if LRN_POP
  Gemm G = L.g[pi];
  {
    const GemmStride &T = S.g[pi];
    const int64_t p = blockIdx.y;
    G.a.p0 += p * T.a0; G.a.p1 += p * T.a1;
    G.b.p0 += p * T.b0; G.b.p1 += p * T.b1;
    G.C += p * T.C; G.bias += p * T.bias; G.mask += p * T.mask; G.w += p * T.w;   // an operand the epilogue does not read: NULL, stride 0
  }
#else
  const Gemm &G = L.g[pi];
#endif
  int t = (int)blockIdx.x - G.first_block;
  const int tn = t % G.tiles_n;
  t /= G.tiles_n;
  const int tm = t % G.tiles_m;
  const int s = t / G.tiles_m;
  const int m0 = tm * LRN_TM, n0 = tn * LRN_TN;
  const int64_t kbeg = (int64_t)s * G.kchunk;
  const int64_t kend = kbeg + G.kchunk < G.K ? kbeg + G.kchunk : G.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int64_t k0 = kbeg; k0 < kend; k0 += LRN_TK) {
    // stage the A and B slices; consecutive threads walk the operand's contiguous (feature) index
#pragma unroll
    for (int i = 0; i < LRN_TM * LRN_TK / 256; ++i) {
      const int e = tid + 256 * i;
      int mm, kk;
      if (G.ta) { mm = e % LRN_TM; kk = e / LRN_TM; } else { kk = e % LRN_TK; mm = e / LRN_TK; }
      const int64_t k = k0 + kk;
      float v = 0.f;
      if (k < kend) v = G.ta ? feat_at(G.a, k, m0 + mm) : feat_at(G.a, m0 + mm, (int)k);
      As[kk][mm] = v;
    }
#pragma unroll
    for (int i = 0; i < LRN_TN * LRN_TK / 256; ++i) {
      const int e = tid + 256 * i;
      int nn, kk;
      if (G.tb) { kk = e % LRN_TK; nn = e / LRN_TK; } else { nn = e % LRN_TN; kk = e / LRN_TN; }
      const int64_t k = k0 + kk;
      float v = 0.f;
      if (k < kend) v = G.tb ? feat_at(G.b, n0 + nn, (int)k) : feat_at(G.b, k, n0 + nn);
      Bs[kk][nn] = v;
    }
    __syncthreads();
    // 32x32x2: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
#pragma unroll
    for (int kk = 0; kk < LRN_TK; kk += 2) {
      const float av = As[kk + (lane >> 5)][wm + (lane & 31)];
      const float bv = Bs[kk + (lane >> 5)][wn + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }

  // accumulator r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
  float *C = G.C + (int64_t)s * G.split_stride;
  const int n = n0 + wn + (lane & 31);
  if (n >= G.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m >= G.M) continue;
    float v = acc[r];
    if (G.epi == EPI_BIAS_RELU) {
      v = v + G.bias[n];
      v = v > 0.f ? v : 0.f;
    } else if (G.epi == EPI_MASK) {
      v = G.mask[(int64_t)m * G.ldm + n] > 0.f ? v : 0.f;
    } else if (G.epi == EPI_DRELU_W) {
      v = (v + G.bias[n] > 0.f) ? G.scale * G.w[n] : 0.f;
    }
    C[(int64_t)m * G.ldc + n] = v;
  }
}
#endif

// blocks [0, ceil(B / 4)): target rows; the next ceil(B / 4): actor rows
__global__ __launch_bounds__(256) void LRN_KERNEL(actor_head)(ActorHeadArgs P LRN_POP_PARAM(HeadStride S)
                                                              LRN_HYPER_PARAM(MemberTable policy_noise, MemberTable noise_clip)) {
#if LRN_POP == 2
  LRN_OWN(policy_noise, policy_noise); LRN_OWN(noise_clip, noise_clip);
#endif
#if LRN_POP
  {
    const int64_t p = blockIdx.y;
    P.t_h2 += p * S.ws; P.a2 += p * S.ws; P.h2 += p * S.ws; P.a += p * S.ws; P.tanh_out += p * S.ws;
    P.t_W3 += p * S.W3; P.W3 += p * S.W3; P.t_b3 += p * S.b3; P.b3 += p * S.b3;
    if (P.noise) P.noise += p * S.noise;
    P.seed += (uint64_t)p;     // member p's Philox key
  }
#endif
  const int lane = threadIdx.x & 63;
  const int64_t nb = (P.B + 3) / 4;
  const bool actor = (int64_t)blockIdx.x >= nb;
  const int64_t b = ((int64_t)blockIdx.x - (actor ? nb : 0)) * 4 + (threadIdx.x >> 6);
  if (b >= P.B) return;
  float u[LRN_A];
  head3(actor ? P.h2 : P.t_h2, actor ? P.W3 : P.t_W3, actor ? P.b3 : P.t_b3, b, lane, u);
  if (lane != 0) return;
  if (actor) {
    store_action(u, P.bound, P.a, P.tanh_out, true, b);
    return;
  }
  float nz[LRN_A];
  row_noise(P.noise, P.seed, P.draw, P.policy_noise, P.noise_clip, b, nz);
#pragma unroll
  for (int j = 0; j < LRN_A; ++j) P.a2[b * LRN_A + j] = proposal(u[j], nz[j], P.bound);
}

// target = r + (1 - d) gamma min(tq1, tq2); loss = mse(q1, target) + mse(q2, target) and its deltas, one wave per row
__global__ __launch_bounds__(256) void LRN_KERNEL(critic_head)(CriticHeadArgs P LRN_POP_PARAM(HeadStride S)
                                                               LRN_HYPER_PARAM(MemberTable gamma)) {
#if LRN_POP == 2
  LRN_OWN(gamma, gamma);
#endif
#if LRN_POP
  {
    const int64_t p = blockIdx.y;
    P.rewards += p * S.rows; P.dones += p * S.rows; P.loss_rows += p * S.ws;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      P.t_h2[i] += p * S.ws; P.h2[i] += p * S.ws; P.d3[i] += p * S.ws; P.d2[i] += p * S.ws;
      P.t_W3[i] += p * S.W3; P.W3[i] += p * S.W3; P.t_b3[i] += p * S.b3; P.b3[i] += p * S.b3;
    }
  }
#endif
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= P.B) return;
  float tq[2], q[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    tq[i] = head1(P.t_h2[i], P.t_W3[i], P.t_b3[i], b, lane);
    q[i] = head1(P.h2[i], P.W3[i], P.b3[i], b, lane);
  }
  const float notdone = 1.0f - (P.dones[b] ? 1.0f : 0.0f);
  const float target = P.rewards[b] + notdone * P.gamma * fminf(tq[0], tq[1]);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float e = q[i] - target;
    const float d3 = 2.0f * e * P.inv_b;
    if (lane == 0) {
      P.d3[i][b] = d3;
      P.loss_rows[2 * b + i] = e * e;
    }
    store_d2(row4(P.h2[i], b, lane), row4(P.W3[i], 0, lane), d3, P.d2[i], b, lane);
  }
}

// DADDPG.  blocks [k ceil(B / 4), (k + 1) ceil(B / 4)): rows of problem k; no noise, no clamp (DADDPG_mlp.py:131-134).  The
// population form moves problem k's pointers where it reads them (LRN_MEMBER): shifting the argument's arrays in place and then
// indexing them by k would put them in scratch.
#if LRN_POP < 2
__global__ __launch_bounds__(256) void LRN_KERNEL(daddpg_actor_head)(DaddpgActorHeadArgs P LRN_POP_PARAM(HeadStride S)) {
  const int lane = threadIdx.x & 63;
  const int64_t nb = (P.B + 3) / 4;
  const int k = (int)((int64_t)blockIdx.x / nb);
  const int64_t b = ((int64_t)blockIdx.x - k * nb) * 4 + (threadIdx.x >> 6);
  if (k > 2 || b >= P.B) return;
  float u[LRN_A];
  head3(LRN_MEMBER(P.h2[k], S.ws), LRN_MEMBER(P.W3[k], S.W3), LRN_MEMBER(P.b3[k], S.b3), b, lane, u);
  if (lane != 0) return;
  store_action(u, P.bound, LRN_MEMBER(P.a[k], S.ws), LRN_MEMBER(P.tanh_out, S.ws), k == 2, b);
}
#endif

// DADDPG.  target = r + (1 - d) gamma min(tq(a2_1), tq(a2_2)); loss = mse(q, target) and its deltas, one wave per row
__global__ __launch_bounds__(256) void LRN_KERNEL(daddpg_critic_head)(DaddpgCriticHeadArgs P LRN_POP_PARAM(HeadStride S)
                                                                      LRN_HYPER_PARAM(MemberTable gamma)) {
#if LRN_POP == 2
  LRN_OWN(gamma, gamma);
#endif
#if LRN_POP
  {
    const int64_t p = blockIdx.y;
    P.rewards += p * S.rows; P.dones += p * S.rows;
    P.t_h2[0] += p * S.ws; P.t_h2[1] += p * S.ws; P.h2 += p * S.ws; P.d3 += p * S.ws; P.d2 += p * S.ws; P.loss_rows += p * S.ws;
    P.t_W3 += p * S.W3; P.W3 += p * S.W3; P.t_b3 += p * S.b3; P.b3 += p * S.b3;
  }
#endif
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= P.B) return;
  const float4 tw = row4(P.t_W3, 0, lane);
  const float tq0 = head1(row4(P.t_h2[0], b, lane), tw, P.t_b3);
  const float tq1 = head1(row4(P.t_h2[1], b, lane), tw, P.t_b3);
  const float4 h = row4(P.h2, b, lane), w = row4(P.W3, 0, lane);
  const float q = head1(h, w, P.b3);
  const float notdone = 1.0f - (P.dones[b] ? 1.0f : 0.0f);
  const float target = P.rewards[b] + notdone * P.gamma * fminf(tq0, tq1);
  const float e = q - target;
  const float d3 = 2.0f * e * P.inv_b;
  if (lane == 0) {
    P.d3[b] = d3;
    P.loss_rows[b] = e * e;
  }
  store_d2(h, w, d3, P.d2, b, lane);
}

// DATD3 / DARC.  blocks [0, ceil(B / 4)): target rows, one wave computes BOTH proposals of its row from one noise draw; the next
// ceil(B / 4): actor rows
__global__ __launch_bounds__(256) void LRN_KERNEL(datd3_actor_head)(Datd3ActorHeadArgs P LRN_POP_PARAM(HeadStride S)
                                                                    LRN_HYPER_PARAM(MemberTable policy_noise, MemberTable noise_clip)) {
#if LRN_POP == 2
  LRN_OWN(policy_noise, policy_noise); LRN_OWN(noise_clip, noise_clip);
#endif
#if LRN_POP
  {
    const int64_t p = blockIdx.y;
#pragma unroll
    for (int i = 0; i < 2; ++i) { P.t_h2[i] += p * S.ws; P.a2[i] += p * S.ws; P.t_W3[i] += p * S.W3; P.t_b3[i] += p * S.b3; }
    P.h2 += p * S.ws; P.a += p * S.ws; P.tanh_out += p * S.ws; P.W3 += p * S.W3; P.b3 += p * S.b3;
    if (P.noise) P.noise += p * S.noise;
    P.seed += (uint64_t)p;     // member p's Philox key; the counter (row, draw) is the single form's
  }
#endif
  const int lane = threadIdx.x & 63;
  const int64_t nb = (P.B + 3) / 4;
  const bool actor = (int64_t)blockIdx.x >= nb;
  const int64_t b = ((int64_t)blockIdx.x - (actor ? nb : 0)) * 4 + (threadIdx.x >> 6);
  if (b >= P.B) return;
  if (actor) {
    float u[LRN_A];
    head3(P.h2, P.W3, P.b3, b, lane, u);
    if (lane != 0) return;
    store_action(u, P.bound, P.a, P.tanh_out, true, b);
    return;
  }
  float u[2][LRN_A];
#pragma unroll
  for (int i = 0; i < 2; ++i) head3(P.t_h2[i], P.t_W3[i], P.t_b3[i], b, lane, u[i]);
  if (lane != 0) return;
  float nz[LRN_A];
  row_noise(P.noise, P.seed, P.draw, P.policy_noise, P.noise_clip, b, nz);
#pragma unroll
  for (int j = 0; j < LRN_A; ++j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) P.a2[i][b * LRN_A + j] = proposal(u[i][j], nz[j], P.bound);
  }
}

// DATD3 / DARC.  target = r + (1 - d) gamma T, T = min(tq1, tq2) (darc: w_min T + w_max T); loss = mse(q, target) (darc: + reg
// mse(q, q_other)) and its deltas, one wave per row
__global__ __launch_bounds__(256) void LRN_KERNEL(datd3_critic_head)(Datd3CriticHeadArgs P LRN_POP_PARAM(HeadStride S)
                                                                     LRN_HYPER_PARAM(MemberTable gamma, MemberTable w_min, MemberTable w_max,
                                                                                     MemberTable reg)) {
#if LRN_POP == 2
  LRN_OWN(gamma, gamma); LRN_OWN(w_min, w_min); LRN_OWN(w_max, w_max); LRN_OWN(reg, reg);     // the last three are read when darc
#endif
#if LRN_POP
  {
    const int64_t p = blockIdx.y;
    P.rewards += p * S.rows; P.dones += p * S.rows;
#pragma unroll
    for (int i = 0; i < 2; ++i) { P.t_h2[i] += p * S.ws; P.t_W3[i] += p * S.W3; P.t_b3[i] += p * S.b3; }
    P.h2 += p * S.ws; P.d3 += p * S.ws; P.d2 += p * S.ws; P.loss_rows += p * S.ws; P.W3 += p * S.W3; P.b3 += p * S.b3;
    if (P.darc) { P.o_h2 += p * S.ws; P.o_W3 += p * S.W3; P.o_b3 += p * S.b3; }     // NULL without darc
  }
#endif
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= P.B) return;
  const float tq0 = head1(P.t_h2[0], P.t_W3[0], P.t_b3[0], b, lane);
  const float tq1 = head1(P.t_h2[1], P.t_W3[1], P.t_b3[1], b, lane);
  const float4 h = row4(P.h2, b, lane), w = row4(P.W3, 0, lane);
  const float q = head1(h, w, P.b3);
  float t = fminf(tq0, tq1);
  if (P.darc) t = P.w_min * t + P.w_max * t;
  const float notdone = 1.0f - (P.dones[b] ? 1.0f : 0.0f);
  const float target = P.rewards[b] + notdone * P.gamma * t;
  const float e = q - target;
  float d3 = 2.0f * e * P.inv_b;
  if (P.darc) {
    const float eo = q - head1(P.o_h2, P.o_W3, P.o_b3, b, lane);
    d3 += P.reg * (2.0f * eo * P.inv_b);
    if (lane == 0) {
      P.loss_rows[2 * b] = e * e;
      P.loss_rows[2 * b + 1] = eo * eo;
    }
  } else if (lane == 0) {
    P.loss_rows[b] = e * e;
  }
  if (lane == 0) P.d3[b] = d3;
  store_d2(h, w, d3, P.d2, b, lane);
}

// back through cat(s, a) -> a = bound tanh(u) -> fc3 of the actor, one wave per row
#if LRN_POP < 2
__global__ __launch_bounds__(256) void LRN_KERNEL(actor_back)(ActorBackArgs P LRN_POP_PARAM(ActorBackStride S)) {
#if LRN_POP
  {
    const int64_t p = blockIdx.y;
    P.dc1 += p * S.ws; P.tanh_a += p * S.ws; P.h2 += p * S.ws; P.du += p * S.ws; P.da2 += p * S.ws;
    P.Wq1 += p * S.Wq1; P.W3 += p * S.W3;
  }
#endif
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= P.B) return;
  const float4 d = row4(P.dc1, b, lane);
  float du[LRN_A];
#pragma unroll
  for (int j = 0; j < LRN_A; ++j) {
    const float *w = P.Wq1 + P.state_dim + j;
    float4 wc;
    wc.x = w[(4 * lane + 0) * P.in_dim];
    wc.y = w[(4 * lane + 1) * P.in_dim];
    wc.z = w[(4 * lane + 2) * P.in_dim];
    wc.w = w[(4 * lane + 3) * P.in_dim];
    const float da = wave_sum(dot4(d, wc));
    const float th = P.tanh_a[b * LRN_A + j];
    du[j] = da * P.bound * (1.0f - th * th);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < LRN_A; ++j) P.du[b * LRN_A + j] = du[j];
  }
  const float4 h = row4(P.h2, b, lane);
  float4 w0 = row4(P.W3, 0, lane), w1 = row4(P.W3, 1, lane), w2 = row4(P.W3, 2, lane), o;
  o.x = h.x > 0.f ? du[0] * w0.x + du[1] * w1.x + du[2] * w2.x : 0.f;
  o.y = h.y > 0.f ? du[0] * w0.y + du[1] * w1.y + du[2] * w2.y : 0.f;
  o.z = h.z > 0.f ? du[0] * w0.z + du[1] * w1.z + du[2] * w2.z : 0.f;
  o.w = h.w > 0.f ? du[0] * w0.w + du[1] * w1.w + du[2] * w2.w : 0.f;
  reinterpret_cast<float4 *>(P.da2 + b * LRN_H)[lane] = o;
}
#endif

__global__ __launch_bounds__(256) void LRN_KERNEL(adam)(AdamArgs P LRN_POP_PARAM(int64_t ws_stride)
                                                        LRN_HYPER_PARAM(MemberTable step_size, MemberTable tau, MemberTable loss_w1)) {
  // P is read where it lies (t[] is indexed by a loop's result: a modified copy of P would live in scratch), so the member's own
  // scalars are named here and not written into it
#if LRN_POP == 2
#define LRN_STEP_SIZE step_size.v[blockIdx.y]
#define LRN_TAU tau.v[blockIdx.y]
#define LRN_LOSS_W1 loss_w1.v[blockIdx.y]
#else
#define LRN_STEP_SIZE P.step_size
#define LRN_TAU P.tau
#define LRN_LOSS_W1 P.loss_w1
#endif
#if LRN_POP
  // member p's tensors lie p times their own size (p, m, v, tp: rows x cols; partial and loss_rows: one workspace) behind member 0's,
  // and its loss is loss[p]; the step numbers, and so the bias corrections, are the population's
  const int64_t member = blockIdx.y;
#define LRN_LOSS_ROWS (P.loss_rows + member * ws_stride)
#define LRN_LOSS (P.loss + member)
#else
#define LRN_LOSS_ROWS P.loss_rows
#define LRN_LOSS P.loss
#endif
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t elem_blocks = ((int64_t)P.total + 255) / 256;
  if ((int64_t)blockIdx.x >= elem_blocks) {
    // loss = mean(column 0) + loss_w1 mean(column 1) (one column: its mean), each summed in a fixed order
    __shared__ float red[2][256];
    float s0 = 0.f, s1 = 0.f;
    if (P.loss_cols == 2) {
      for (int64_t b = threadIdx.x; b < P.B; b += 256) {
        s0 += LRN_LOSS_ROWS[2 * b];
        s1 += LRN_LOSS_ROWS[2 * b + 1];
      }
    } else {
      for (int64_t b = threadIdx.x; b < P.B; b += 256) s0 += LRN_LOSS_ROWS[b];
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
      if ((int)threadIdx.x < o) {
        red[0][threadIdx.x] += red[0][threadIdx.x + o];
        red[1][threadIdx.x] += red[1][threadIdx.x + o];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0 && P.loss) LRN_LOSS[0] = P.loss_cols == 2 ? red[0][0] * P.inv_b + LRN_LOSS_W1 * (red[1][0] * P.inv_b) : red[0][0] * P.inv_b;
    return;
  }
  if (e >= P.total) return;
  int ti = 0;
  while (ti + 1 < P.n && e >= P.t[ti + 1].first) ++ti;
#if LRN_POP
  AdamTensor T = P.t[ti];
  {
    const int64_t own = member * ((int64_t)T.rows * T.cols);
    T.p += own; T.m += own; T.v += own; T.tp += own; T.partial += member * ws_stride;
  }
#else
  const AdamTensor &T = P.t[ti];
#endif
  const int i = (int)(e - T.first);
  const int r = i / T.cols, c = i % T.cols;
  const float *g_p = T.partial + (int64_t)r * T.ldp + T.c0 + c;
  float g = 0.f;
  for (int s = 0; s < P.splits; ++s) g += g_p[(int64_t)s * P.split_stride];
  const float m = P.beta1 * T.m[i] + (1.0f - P.beta1) * g;
  const float v = P.beta2 * T.v[i] + (1.0f - P.beta2) * g * g;
  T.m[i] = m;
  T.v[i] = v;
  const float p = T.p[i] - LRN_STEP_SIZE * m / (sqrtf(v) / P.bc2_sqrt + P.eps);
  T.p[i] = p;
  if (P.soft) T.tp[i] = T.tp[i] * (1.0f - LRN_TAU) + LRN_TAU * p;
}

#undef LRN_LOSS_ROWS
#undef LRN_LOSS
#undef LRN_STEP_SIZE
#undef LRN_TAU
#undef LRN_LOSS_W1
#undef LRN_KERNEL
#undef LRN_MEMBER
#undef LRN_POP_PARAM
#undef LRN_HYPER_PARAM
#undef LRN_OWN
