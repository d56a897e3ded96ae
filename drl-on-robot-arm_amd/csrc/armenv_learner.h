// armenv_learner.h -- kernels of the fused learner updates (armenv_learner.hip): armenv_td3_update, TD3_MLP.train (the reference's
// algo/TD3/TD3_mlp.py:114-161), armenv_daddpg_update, DADDPG_MLP.update (algo/DADDPG/DADDPG_mlp.py:117-171), and armenv_datd3_update,
// DATD3_MLP.update / DARC_MLP.update (algo/DATD3/DATD3_mlp.py:146-211, algo/DARC/DARC_mlp.py:140-222), over the networks of
// net_mlp.py, hidden width 256, exact f32.
//
// Three kinds of kernel, each launched over a LIST of independent problems so that every stage of the update is one launch:
//   gemm_kernel        C = A . B on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: no xf32 on gfx950).  A 64 x 64 output tile
//                      per 256-thread workgroup, 32 x 32 per wave, K streamed through LDS in slices of 16.  Every contraction
//                      of the update is one of three forms of the same product, expressed through `Feat` operands:
//                        forward       Y[b][o]  = X[b][:] . W[o][:]     (+ bias, relu)
//                        backward      D1[b][i] = D2[b][:] . W[:][i]    (* relu'(H1))
//                        weight grad   G[o][i]  = D[:][o] . X[:][i]     (K = the batch; [X | 1] gives the bias column)
//                      Weight gradients are reduced over the batch in slices of LRN_KSPLIT rows: slice s writes its own partial
//                      (no atomics); the optimiser kernel adds the partials in slice order.  Every sum of the update therefore has
//                      one fixed order, and an update is bitwise reproducible run to run.
//   *_head_kernel      the per-row work of the 256 -> 3 / 256 -> 1 layers: one wave per batch row, a 256-long dot product as
//                      four values per lane and a fixed xor-butterfly, then the row's deltas.
//   adam_kernel        torch.optim.Adam (no weight decay, bias correction from the step number) over all tensors of one optimiser,
//                      the Polyak soft update of the matching target network folded in, and (critic) the loss.
// The DADDPG update shares gemm_kernel, actor_back_kernel and adam_kernel; its two per-row heads are daddpg_actor_head_kernel and
// daddpg_critic_head_kernel (two actors and their targets, ONE critic, no target-policy noise).
// The DATD3 / DARC update shares the same three; its heads are datd3_actor_head_kernel (both target actors' proposals under ONE noise
// draw per row, and the stepped actor's action) and datd3_critic_head_kernel (two target critics, the stepped critic, and with `darc`
// the mixed target and the pull towards the other critic).
// No kernel uses atomics, scratch or a memset; nothing is allocated: all intermediates live in the caller's workspace.
// All nine kernels -- gemm, actor_back, adam and the three updates' actor and critic heads -- are written in
// armenv_learner_kernels.inc, which the end of this header includes three times: as the single-learner kernels named above, as the
// *_pop_kernel forms of armenv_td3_pop_update, armenv_daddpg_pop_update and armenv_datd3_pop_update, where a second grid dimension is
// the member of a population of stacked learners, and as the *_pop_hyper_kernel forms of the armenv_*_pop_update_hyper entry points,
// where adam and the heads that read a hyper-parameter take it from a per-member table.  This header holds their argument structs and
// the per-row pieces they are built from.
// A tenth kernel, pop_exploit_kernel (armenv_pop_exploit), is written once at the end of this header: it copies whole members of
// the populations' stacks, source to destination, in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "armenv_math.h"

namespace armenv {
namespace learner {

constexpr int LRN_H = 256;        // hidden width (config.py:56)
constexpr int LRN_A = 3;          // action dim
constexpr int LRN_TM = 64, LRN_TN = 64, LRN_TK = 16;   // gemm_kernel's workgroup tile and K slice
constexpr int LRN_KSPLIT = 256;   // batch rows per weight-gradient partial
constexpr int LRN_MAX_GEMMS = 6;
constexpr int LRN_MAX_TENSORS = 12;

// A row-major "feature matrix" F[r][f]: features f < split come from p0 (row stride ld0), split <= f < nf from p1 (row stride ld1),
// f == nf is a column of ones when `aug` (the bias column of a weight gradient), anything else reads 0.  Two pointers let cat(s, a)
// feed the critics without being materialised.
struct Feat {
  const float *p0, *p1;
  int ld0, ld1, split, nf, aug;
  int64_t rows;
};

AE_DEV float feat_at(const Feat &F, int64_t r, int f) {
  if (r >= F.rows) return 0.f;
  if (f < F.split) return F.p0[r * F.ld0 + f];
  if (f < F.nf) return F.p1[r * F.ld1 + (f - F.split)];
  return (F.aug && f == F.nf) ? 1.f : 0.f;
}

enum { EPI_STORE = 0,        // C = acc
       EPI_BIAS_RELU = 1,    // C = relu(acc + bias[n])
       EPI_MASK = 2,         // C = acc * (mask[m][n] > 0)             (backward through a relu)
       EPI_DRELU_W = 3 };    // C = (acc + bias[n] > 0) ? scale * w[n] : 0  (a 256 -> 1 layer's delta through the relu in front of it)

// C[m][n] = sum_k A(m, k) B(k, n) with A(m, k) = ta ? a[k][m] : a[m][k] and B(k, n) = tb ? b[n][k] : b[k][n] (Feat indexing).
// K is cut into `splits` ranges of kchunk; range s writes C + s * split_stride.
struct Gemm {
  Feat a, b;
  int ta, tb;
  int M, N;
  int64_t K, kchunk;
  int splits, tiles_m, tiles_n, first_block;
  float *C;
  int ldc;
  int64_t split_stride;
  int epi;
  const float *bias, *mask, *w;
  int ldm;
  float scale;
};

struct GemmList {
  Gemm g[LRN_MAX_GEMMS];
  int n;
};


AE_DEV float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// four hidden units per lane: h[b][4 lane .. 4 lane + 3]
AE_DEV float4 row4(const float *p, int64_t b, int lane) { return reinterpret_cast<const float4 *>(p + b * LRN_H)[lane]; }
AE_DEV float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// standard normal pair from two 32-bit words (Box-Muller in f32; u1 in (0, 1])
AE_DEV void box_muller(uint32_t w0, uint32_t w1, float &z0, float &z1) {
  const float u1 = (float)((w0 >> 8) + 1u) * (1.0f / 16777216.0f);
  const float u2 = (float)(w1 >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

// The per-row pieces of the head kernels, each written once.  The build has -ffp-contract=off, so a kernel built from them performs
// the IEEE operations it would perform written out, in the same order.

// the 256 -> 3 head of row b: u[j] = h2[b] . W3[j] + b3[j], the same value in every lane
AE_DEV void head3(const float *h2, const float *W3, const float *b3, int64_t b, int lane, float (&u)[LRN_A]) {
  const float4 h = row4(h2, b, lane);
#pragma unroll
  for (int j = 0; j < LRN_A; ++j) u[j] = wave_sum(dot4(h, row4(W3, j, lane))) + b3[j];
}

// the 256 -> 1 head of a row from its lane's four hidden units h and weights w: h2[b] . W3[0] + b3[0]
AE_DEV float head1(float4 h, float4 w, const float *b3) { return wave_sum(dot4(h, w)) + b3[0]; }
AE_DEV float head1(const float *h2, const float *W3, const float *b3, int64_t b, int lane) {
  return head1(row4(h2, b, lane), row4(W3, 0, lane), b3);
}

// row b's target-policy noise clamp(z policy_noise, +-noise_clip): z from `noise` [B][3] when given, else drawn by Philox4x32-10
// keyed by seed, counter (row, draw) -- independent of launch geometry -- and Box-Muller
AE_DEV void row_noise(const float *noise, uint64_t seed, uint64_t draw, float policy_noise, float noise_clip, int64_t b,
                      float (&nz)[LRN_A]) {
  float z[4];
  if (noise) {
#pragma unroll
    for (int j = 0; j < LRN_A; ++j) z[j] = noise[b * LRN_A + j];
  } else {
    uint32_t c[4] = {(uint32_t)b, (uint32_t)((uint64_t)b >> 32), (uint32_t)draw, (uint32_t)(draw >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    box_muller(c[0], c[1], z[0], z[1]);
    box_muller(c[2], c[3], z[2], z[3]);
  }
#pragma unroll
  for (int j = 0; j < LRN_A; ++j) nz[j] = fminf(fmaxf(z[j] * policy_noise, -noise_clip), noise_clip);
}

// the noisy clamped proposal clamp(bound tanh(u) + nz, +-bound)
AE_DEV float proposal(float u, float nz, float bound) {
  const float v = tanhf(u) * bound + nz;
  return fminf(fmaxf(v, -bound), bound);
}

// a = bound tanh(u) of row b, and tanh itself when `keep_tanh` (the backward pass reads it)
AE_DEV void store_action(const float (&u)[LRN_A], float bound, float *a, float *tanh_out, bool keep_tanh, int64_t b) {
#pragma unroll
  for (int j = 0; j < LRN_A; ++j) {
    const float th = tanhf(u[j]);
    if (keep_tanh) tanh_out[b * LRN_A + j] = th;
    a[b * LRN_A + j] = th * bound;
  }
}

// d2[b] = (d3 W3) relu'(h2[b]): the lane's four hidden units h and weights w
AE_DEV void store_d2(float4 h, float4 w, float d3, float *d2, int64_t b, int lane) {
  float4 d;
  d.x = h.x > 0.f ? d3 * w.x : 0.f;
  d.y = h.y > 0.f ? d3 * w.y : 0.f;
  d.z = h.z > 0.f ? d3 * w.z : 0.f;
  d.w = h.w > 0.f ? d3 * w.w : 0.f;
  reinterpret_cast<float4 *>(d2 + b * LRN_H)[lane] = d;
}

struct ActorHeadArgs {
  int64_t B;
  // target rows: a2 = clamp(bound tanh(h2 W3^T + b3) + clamp(noise policy_noise, +-noise_clip), +-bound)
  const float *t_h2, *t_W3, *t_b3, *noise;
  uint64_t seed, draw;
  float bound, policy_noise, noise_clip;
  float *a2;
  // actor rows (when `with_actor`): a = bound tanh(h2 W3^T + b3), and tanh kept for the backward pass
  int with_actor;
  const float *h2, *W3, *b3;
  float *a, *tanh_out;
};


struct CriticHeadArgs {
  int64_t B;
  float gamma, inv_b;
  const float *rewards;
  const uint8_t *dones;
  const float *t_h2[2], *t_W3[2], *t_b3[2];    // target twin critic's last hidden layer and fc3 / fc6
  const float *h2[2], *W3[2], *b3[2];          // critic's
  float *d3[2];                                // out [B]: dLoss / dq
  float *d2[2];                                // out [B][H]: (d3 W3) * relu'(h2)
  float *loss_rows;                            // out [B][2]: (q1 - target)^2, (q2 - target)^2
};


struct DaddpgActorHeadArgs {
  int64_t B;
  float bound;
  // problem k: a_k = bound tanh(h2_k W3_k^T + b3_k); k = 0, 1 the two target actors over s2, k = 2 the updated actor over s
  const float *h2[3], *W3[3], *b3[3];
  float *a[3];               // out [B][3] each
  float *tanh_out;           // out [B][3]: tanh of problem 2, kept for the backward pass
};

struct DaddpgCriticHeadArgs {
  int64_t B;
  float gamma, inv_b;
  const float *rewards;
  const uint8_t *dones;
  const float *t_h2[2];                        // the target critic's last hidden layer over cat(s2, a2_1) and cat(s2, a2_2)
  const float *t_W3, *t_b3;                    // the target critic's fc3
  const float *h2, *W3, *b3;                   // the critic's, over cat(s, a)
  float *d3;                                   // out [B]: dLoss / dq
  float *d2;                                   // out [B][H]: (d3 W3) * relu'(h2)
  float *loss_rows;                            // out [B]: (q - target)^2
};

struct Datd3ActorHeadArgs {
  int64_t B;
  float bound, policy_noise, noise_clip;
  const float *noise;        // nullable [B][3] standard normals in place of the draw
  uint64_t seed, draw;
  // target rows: a2_j = clamp(bound tanh(h2_j W3_j^T + b3_j) + clamp(z policy_noise, +-noise_clip), +-bound), j = 0, 1, ONE z per row
  const float *t_h2[2], *t_W3[2], *t_b3[2];
  float *a2[2];              // out [B][3] each
  // actor rows: a = bound tanh(h2 W3^T + b3) of the stepped actor over s, and tanh kept for the backward pass
  const float *h2, *W3, *b3;
  float *a, *tanh_out;
};

struct Datd3CriticHeadArgs {
  int64_t B;
  float gamma, inv_b;
  int darc;
  float w_min, w_max, reg;                     // darc: q_weight, 1 - q_weight, regularization_weight
  const float *rewards;
  const uint8_t *dones;
  const float *t_h2[2], *t_W3[2], *t_b3[2];    // target critic j's last hidden layer over cat(s2, a2_j) and its fc3
  const float *h2, *W3, *b3;                   // the stepped critic's, over cat(s, a)
  const float *o_h2, *o_W3, *o_b3;             // darc: the other critic's, over cat(s, a)
  float *d3;                                   // out [B]: dLoss / dq
  float *d2;                                   // out [B][H]: (d3 W3) * relu'(h2)
  float *loss_rows;                            // out [B]: (q - target)^2; darc [B][2]: and (q - q_other)^2
};

struct ActorBackArgs {
  int64_t B;
  int in_dim;            // state_dim + 3: row length of Q1's fc1 weight
  int state_dim;
  float bound;
  const float *dc1;      // [B][H]: delta at Q1's first hidden layer
  const float *Wq1;      // [H][in_dim]
  const float *tanh_a;   // [B][3]
  const float *h2, *W3;  // actor's last hidden layer [B][H], fc3 weight [3][H]
  float *du;             // out [B][3]: delta at the actor's pre-tanh output
  float *da2;            // out [B][H]: (du W3) * relu'(h2)
};


// One parameter tensor of an optimiser: `rows` x `cols` elements; its gradient is sum_s partial[s * split_stride + r * ldp + c0 + c].
struct AdamTensor {
  float *p, *m, *v, *tp;     // tp: the target network's tensor (soft-updated when AdamArgs.soft)
  const float *partial;
  int rows, cols, ldp, c0;
  int first;                 // index of the tensor's first element in the launch
};

struct AdamArgs {
  AdamTensor t[LRN_MAX_TENSORS];
  int n, total, splits;
  int64_t split_stride;
  float step_size, bc2_sqrt, beta1, beta2, eps, tau;
  int soft;
  // the critic's launch also reduces the loss: one extra block after the elementwise ones
  const float *loss_rows;
  int loss_cols;             // loss_rows is [B][loss_cols]: 2 (TD3's twin critic; DARC's two terms) or 1 (DADDPG's / DATD3's one)
  float loss_w1;             // weight of column 1's mean: 1 (TD3), regularization_weight (DARC)
  int64_t B;
  float inv_b;
  float *loss;
};


// Member strides of the population kernels (armenv_*_pop_update), in elements per member.  They ride beside the single-learner
// argument structs, not inside them, so the single-learner kernels keep their arguments.
struct GemmStride {
  int64_t a0, a1, b0, b1;      // the Feat operands' two bases
  int64_t C, bias, mask, w;
};

struct GemmStrideList {
  GemmStride g[LRN_MAX_GEMMS];
};

// the head kernels': `ws` for everything in the workspace, `W3` / `b3` for the heads' tensors (the nets of one launch have one
// shape), `rows` for rewards and dones, `noise` for the given noise
struct HeadStride {
  int64_t ws, W3, b3, rows, noise;
};

struct ActorBackStride {
  int64_t ws, Wq1, W3;
};

// One scalar of the *_pop_hyper_kernel forms (armenv_*_pop_update_hyper): v[p] is member p's value.  A by-value kernel argument
// beside the strides, filled by the host from the call's ArmEnvPopHyper array; a kernel reads v[blockIdx.y].
constexpr int LRN_MAX_MEMBERS = 64;
struct MemberTable {
  float v[LRN_MAX_MEMBERS];
};

#define LRN_POP 0
#include "armenv_learner_kernels.inc"
#undef LRN_POP
#define LRN_POP 1
#include "armenv_learner_kernels.inc"
#undef LRN_POP
#define LRN_POP 2
#include "armenv_learner_kernels.inc"
#undef LRN_POP

// pop_exploit_kernel (armenv_pop_exploit): the exploit step of population-based training.  Member blockIdx.y of every stack
// [P][elems] of the table becomes a copy of member src.v[blockIdx.y]; a member that is its own source returns at once.  Grid
// (blocks over one member's elements of all tensors, members): tensor t owns the blocks from t.first on, one block per
// LRN_EXPLOIT_CHUNK floats.  The host refuses a plan in which a source is itself replaced, so no block reads what another writes.
constexpr int LRN_EXPLOIT_MAX_TENSORS = 128;
constexpr int LRN_EXPLOIT_CHUNK = 4096;    // floats per block: four float4 per thread (pop_exploit_kernel spells the four out)

struct ExploitTensor {
  float *base;       // member 0's array of the stack
  int64_t elems;     // floats per member = the member stride
  int32_t first;     // the tensor's first block
};

struct ExploitTable {
  ExploitTensor t[LRN_EXPLOIT_MAX_TENSORS];
  int32_t n;
};

struct ExploitSources {
  int32_t v[LRN_MAX_MEMBERS];
};

__global__ __launch_bounds__(256) void pop_exploit_kernel(ExploitTable T, ExploitSources src) {
  const int dst = (int)blockIdx.y, from_member = src.v[blockIdx.y];
  if (from_member == dst) return;
  // the last tensor whose first block is not after this one (wave-uniform: the table is read where it lies)
  int lo = 0, hi = T.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.t[mid].first <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int64_t elems = T.t[lo].elems;
  const int64_t start = (int64_t)((int)blockIdx.x - T.t[lo].first) * LRN_EXPLOIT_CHUNK;
  if (start >= elems) return;
  const int n = (int)(elems - start < LRN_EXPLOIT_CHUNK ? elems - start : LRN_EXPLOIT_CHUNK);
  const float *from = T.t[lo].base + (int64_t)from_member * elems + start;
  float *to = T.t[lo].base + (int64_t)dst * elems + start;
  // A member's base is only 4-byte aligned where elems is no multiple of 4 (a b3 of 1 or 3 floats): float4 where both sides allow
  // it, with the chunk's last n % 4 floats one by one; else float by float.
  if ((((uintptr_t)from | (uintptr_t)to) & 15) == 0) {
    const int n4 = n >> 2;
    // all of the thread's loads are in flight before its first store
    const float4 *from4 = reinterpret_cast<const float4 *>(from);
    float4 *to4 = reinterpret_cast<float4 *>(to);
    const int i0 = (int)threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
    if (i0 < n4) r0 = from4[i0];
    if (i1 < n4) r1 = from4[i1];
    if (i2 < n4) r2 = from4[i2];
    if (i3 < n4) r3 = from4[i3];
    if (i0 < n4) to4[i0] = r0;
    if (i1 < n4) to4[i1] = r1;
    if (i2 < n4) to4[i2] = r2;
    if (i3 < n4) to4[i3] = r3;
    const int i = 4 * n4 + (int)threadIdx.x;
    if (i < n) to[i] = from[i];
  } else {
    for (int i = (int)threadIdx.x; i < n; i += 256) to[i] = from[i];
  }
}

}  // namespace learner
}  // namespace armenv
