// armenv_learner.hip -- armenv_td3_update / armenv_td3_workspace_bytes, armenv_daddpg_update / armenv_daddpg_workspace_bytes and
// armenv_datd3_update / armenv_datd3_workspace_bytes (include/armenv.h): argument checks, the workspace layout and the ONE launch
// sequence of the fused TD3, DADDPG and DATD3 / DARC updates over the kernels of armenv_learner.h.
//
// An entry point describes its update as an `Update` (which nets take part, below) and run_update walks the stages over it; stages 3
// and 6 are the entry point's own head kernels.  B rows, H = 256, D = state_dim, K1 = D + 3; every stage is one launch over all its
// independent problems, in the order written.  k = update_actor, `other` = 3 - k.
//      kind   what                                         TD3                        DADDPG                   DATD3 / DARC
//   1  gemm   layer 1: target actors (s2),                 the target actor           target actors 1, 2       target actors 1, 2
//               stepped critics (cat(s, a)),               Q1, Q2                     the critic               critic k
//               the stepped actor (s),                     the actor (with_actor)     actor k                  actor k
//               the read-only other critic (cat(s, a))     --                         --                       darc: critic `other`
//   2  gemm   layer 2 of the same nets
//   3  head   the actors' fc3: proposals a2 and            actor_head_kernel:         daddpg_actor_head_..:    datd3_actor_head_kernel:
//               a = actor(s) with its tanh                 a2 with noise, clamped     a2_1, a2_2 as they are   a2_1, a2_2, ONE noise draw
//   4  gemm   layer 1 of the two target-critic             (TQ1, a2), (TQ2, a2)       (TQ, a2_1), (TQ, a2_2)   (TQ1, a2_1), (TQ2, a2_2)
//               evaluations (net, proposal) over cat(s2, .)
//   5  gemm   layer 2 of the same two problems
//   6  head   target = r + (1 - d) gamma T, T = min(tq1,    critic_head_kernel:        daddpg_critic_head_..:   datd3_critic_head_kernel:
//               tq2); the stepped critics' fc3, loss rows, both heads, loss [B][2]    loss [B]                 darc: T = q_weight T +
//               d3 and d2 = (d3 W3) relu'(h2)                                                                   (1 - q_weight) T, d3 += the
//                                                                                                              pull to `other`, loss [B][2]
//   7  gemm   per stepped critic: d1 = (d2 W2) relu'(h1); dW3 | db3 and dW2 | db2 partials
//   8  gemm   per stepped critic: dW1 | db1 partials
//   9  adam   stepped critics (6 tensors each) + the loss;  soft = with_actor           soft = (k == 2)          soft always, of target
//               soft: their targets' soft update (the        loss = m0 + m1             loss = m0                critic k; loss = m0 (darc:
//               critics are final by then)                                                                      + regularization_weight m1)
//      TD3 without with_actor ends here (9 launches); everything else goes on (16 launches):
//  10  gemm   layer 1 of Qa over cat(s, a), Qa the stepped  Qa = Q1                    Qa = the critic          Qa = critic k
//               critic that the actor's loss reads
//  11  gemm   Qa's layer 2 with its epilogue producing the delta of -mean(Qa): (-1/B) W3 relu'(.)
//  12  gemm   dc1 = (dc2 W2) relu'(c1)
//  13  head   actor_back_kernel: back through cat -> tanh -> the stepped actor's fc3: du, da2
//  14  gemm   da1 = (da2 W2a) relu'(h1a); dW3a | db3a and dW2a | db2a partials (the critics' partials are consumed: same slices)
//  15  gemm   dW1a | db1a partials
//  16  adam   the stepped actor (6 tensors) + its target's soft update
// The other critic is read (darc) and never written; the actor's loss never reads a target.
//
// armenv_td3_pop_update, armenv_daddpg_pop_update, armenv_datd3_pop_update and their *_pop_workspace_bytes: the same column for P
// stacked learners.  The same launches with the *_pop_kernel forms over (workgroups of one member, P); member p's operands lie p
// member strides behind member 0's (MemberStrides).
//
// armenv_td3_pop_update_hyper, armenv_daddpg_pop_update_hyper and armenv_datd3_pop_update_hyper: the population column once more, with
// a HOST array ArmEnvPopHyper[P] of the members' own hyper-parameters (MemberStrides.hyper).  Stages 3, 6, 9 and 16 -- the only ones
// whose kernels read such a scalar -- launch their *_pop_hyper_kernel forms with the members' values as MemberTable arguments, each
// derived scalar formed per member by the single path's expression; every other launch is the population's.
//
// armenv_pop_exploit: the exploit step of population-based training over any population's stacks -- ONE launch of pop_exploit_kernel
// (armenv_learner.h) in which member p of every stack becomes a copy of member src[p].  The whole plan is checked first; a source
// that is itself replaced is refused, so the launch has no read that races a write.
#include <cmath>
#include <initializer_list>

#include "armenv_engine.h"
#include "armenv_learner.h"

using namespace armenv::learner;

namespace {

// workspace layout: offsets in floats; every region starts on a 64-float (256-byte) boundary
struct Ws {
  int64_t S;                                        // number of weight-gradient partials
  int64_t ta1[2], ta2[2], a2[2];                    // per target actor: hidden layers [B][H], proposal [B][3]
  int64_t tq1[2], tq2[2];                           // per target-critic evaluation: hidden layers [B][H]
  int64_t h1[2], h2[2], d2[2], d1[2], d3[2];        // per stepped critic: [B][H] each, d3 [B]
  int64_t pW3[2], pW2[2], pW1[2];                   // per stepped critic: partials [S][rows][ld]
  int64_t ah1, ah2, api, tanh_a, du;                // the stepped actor: [B][H], [B][H], [B][3] each
  int64_t pa3, pa2, pa1;                            // the actor's partials, in the critics' slices
  int64_t oh1, oh2;                                 // the read-only other critic: [B][H] each
  int64_t loss1, loss2;                             // loss rows [B] and [B][2]
  int64_t split_stride;                             // floats per partial slice
  int64_t total;
};

constexpr int kW1Ld = 16;   // row length of a W1 | b1 partial: state_dim + 3 + 1 <= 16

int64_t up64(int64_t x) { return (x + 63) & ~(int64_t)63; }

// TD3: (1, 2, false); DADDPG: (2, 1, false); DATD3 / DARC: (2, 1, true).  There are always two target-critic evaluations and one
// stepped actor; a region that an algorithm does not have takes no room.
Ws layout(int64_t B, int target_actors, int critics, bool other_critic) {
  Ws w{};
  w.S = (B + LRN_KSPLIT - 1) / LRN_KSPLIT;
  const int64_t H = LRN_H, BH = B * H;
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t r = o; o += up64(n); return r; };
  for (int i = 0; i < target_actors; ++i) { w.ta1[i] = take(BH); w.ta2[i] = take(BH); w.a2[i] = take(3 * B); }
  for (int i = 0; i < 2; ++i) { w.tq1[i] = take(BH); w.tq2[i] = take(BH); }
  for (int i = 0; i < critics; ++i) { w.h1[i] = take(BH); w.h2[i] = take(BH); w.d2[i] = take(BH); w.d1[i] = take(BH); w.d3[i] = take(B); }
  w.ah1 = take(BH); w.ah2 = take(BH); w.api = take(3 * B); w.tanh_a = take(3 * B); w.du = take(3 * B);
  if (other_critic) { w.oh1 = take(BH); w.oh2 = take(BH); }
  // a one-column loss block where ONE critic is stepped, a two-column one where the loss has two terms (a twin critic, or the pull
  // towards the other critic, which only `darc` writes)
  if (critics == 1) w.loss1 = take(B);
  if (critics == 2 || other_critic) w.loss2 = take(2 * B);
  // one partial slice holds every stepped critic's W3 | b3 [1][H+1], W2 | b2 [H][H+1], W1 | b1 [H][16] OR the actor's W3 | b3
  // [3][H+1], ...: the two never live at the same time (the critics' are consumed by their Adam launch before the actor's are
  // written), so the slice is the larger of the two -- the critics' with two of them, the actor's with one
  int64_t qc = 0, qa = 0;
  auto sub = [](int64_t &q, int64_t n) { const int64_t r = q; q += up64(n); return r; };
  for (int i = 0; i < critics; ++i) { w.pW3[i] = sub(qc, H + 1); w.pW2[i] = sub(qc, H * (H + 1)); w.pW1[i] = sub(qc, H * kW1Ld); }
  w.pa3 = sub(qa, 3 * (H + 1)); w.pa2 = sub(qa, H * (H + 1)); w.pa1 = sub(qa, H * kW1Ld);
  w.split_stride = qc > qa ? qc : qa;
  const int64_t part = take(w.S * w.split_stride);
  for (int i = 0; i < critics; ++i) { w.pW3[i] += part; w.pW2[i] += part; w.pW1[i] += part; }
  w.pa3 += part; w.pa2 += part; w.pa1 += part;
  w.total = o;
  return w;
}

Feat feat(const float *p, int ld, int nf, int64_t rows, int aug = 0) { return Feat{p, p, ld, ld, nf, nf, aug, rows}; }
Feat feat2(const float *p0, int ld0, const float *p1, int ld1, int nf, int64_t rows, int aug = 0) {
  return Feat{p0, p1, ld0, ld1, ld0, nf, aug, rows};
}

// Member strides of a population update (armenv_*_pop_update): every array of the call is member 0's array of a stack [P][...],
// so an operand's stride is the size, in elements, of the member-0 array that it points into -- a net or moment tensor, a batch
// array, or the whole single-learner workspace.  The entry point registers those arrays; of() finds the one that holds a pointer.
struct MemberStrides {
  struct Array { uintptr_t lo, hi; int64_t stride; };
  Array arrays[16 * 6 + 8];   // DATD3 / DARC: 16 nets and moments of six tensors, the workspace, five batch arrays, the noise
  int n = 0;
  int members = 1;
  int64_t ws = 0;              // the workspace's stride: floats of one single-learner workspace
  const ArmEnvPopHyper *hyper = nullptr;   // set (host, [members]): armenv_*_pop_update_hyper, the members' own hyper-parameters
  // member p's value of a scalar: f(hyper[p]), p < members
  template <class F>
  MemberTable table(F f) const {
    MemberTable t{};
    for (int p = 0; p < members; ++p) t.v[p] = f(hyper[p]);
    return t;
  }
  MemberTable table(float ArmEnvPopHyper::*field) const {
    return table([field](const ArmEnvPopHyper &h) { return h.*field; });
  }
  void add(const void *p, int64_t elems, int64_t elem_bytes = sizeof(float)) {
    if (p) arrays[n++] = Array{(uintptr_t)p, (uintptr_t)p + (uintptr_t)(elems * elem_bytes), elems};
  }
  void add(const ArmEnvMlpRW &m, int in, int out) {
    add(m.W1, (int64_t)LRN_H * in); add(m.b1, LRN_H); add(m.W2, (int64_t)LRN_H * LRN_H); add(m.b2, LRN_H);
    add(m.W3, (int64_t)out * LRN_H); add(m.b3, out);
  }
  // NULL: 0 (an operand that is not read); a pointer outside every registered array: -1
  int64_t of(const void *p) const {
    if (!p) return 0;
    for (int i = 0; i < n; ++i)
      if ((uintptr_t)p >= arrays[i].lo && (uintptr_t)p < arrays[i].hi) return arrays[i].stride;
    return -1;
  }
};

struct Launcher {
  GemmList L{};
  GemmStrideList S{};
  int blocks = 0;
  const MemberStrides *pop = nullptr;    // set: a population update, launched as gemm_pop_kernel over (blocks, members)
  bool unknown = false;                  // an operand that `pop` cannot place
  void add(const Gemm &g0) {
    Gemm g = g0;
    g.tiles_m = (g.M + LRN_TM - 1) / LRN_TM;
    g.tiles_n = (g.N + LRN_TN - 1) / LRN_TN;
    g.splits = (int)((g.K + g.kchunk - 1) / g.kchunk);
    g.first_block = blocks;
    blocks += g.tiles_m * g.tiles_n * g.splits;
    if (pop) {
      GemmStride &t = S.g[L.n];
      t = GemmStride{pop->of(g.a.p0), pop->of(g.a.p1), pop->of(g.b.p0), pop->of(g.b.p1),
                     pop->of(g.C),    pop->of(g.bias), pop->of(g.mask), pop->of(g.w)};
      for (int64_t v : {t.a0, t.a1, t.b0, t.b1, t.C, t.bias, t.mask, t.w}) unknown = unknown || v < 0;
    }
    L.g[L.n++] = g;
  }
  // Y[B][H] = epilogue(X W^T): X a Feat of B rows and `in` features
  void forward(const Feat &x, int in, const float *W, const float *bias, float *Y, int64_t B, int epi = EPI_BIAS_RELU,
               const float *w = nullptr, float scale = 0.f) {
    Gemm g{};
    g.a = x; g.ta = 0;
    g.b = feat(W, in, in, LRN_H); g.tb = 1;
    g.M = (int)B; g.N = LRN_H; g.K = in; g.kchunk = in;
    g.C = Y; g.ldc = LRN_H; g.epi = epi; g.bias = bias; g.w = w; g.scale = scale;
    add(g);
  }
  // D1[B][H] = (D2 W) relu'(mask): back through a square H x H layer
  void backward(const float *D2, const float *W, const float *mask, float *D1, int64_t B) {
    Gemm g{};
    g.a = feat(D2, LRN_H, LRN_H, B); g.ta = 0;
    g.b = feat(W, LRN_H, LRN_H, LRN_H); g.tb = 0;
    g.M = (int)B; g.N = LRN_H; g.K = LRN_H; g.kchunk = LRN_H;
    g.C = D1; g.ldc = LRN_H; g.epi = EPI_MASK; g.mask = mask; g.ldm = LRN_H;
    add(g);
  }
  // partial[s][o][i] = sum over batch slice s of delta[b][o] [x | 1][b][i]: weight (i < in) and bias (i == in) gradients
  void wgrad(const float *delta, int out, const Feat &x_aug, int in, float *P, int ldp, int64_t B, int64_t split_stride) {
    Gemm g{};
    g.a = feat(delta, out, out, B); g.ta = 1;
    g.b = x_aug; g.tb = 0;
    g.M = out; g.N = in + 1; g.K = B; g.kchunk = LRN_KSPLIT;
    g.C = P; g.ldc = ldp; g.split_stride = split_stride; g.epi = EPI_STORE;
    add(g);
  }
  int launch(hipStream_t s) {
    if (unknown) return fail(ARMENV_EINVAL, "fused update: an operand lies outside the population's arrays");
    if (pop)
      hipLaunchKernelGGL(gemm_pop_kernel, dim3((unsigned)blocks, (unsigned)pop->members), dim3(256), 0, s, L, S);
    else
      hipLaunchKernelGGL(gemm_kernel, dim3((unsigned)blocks), dim3(256), 0, s, L);
    HIP_TRY(hipGetLastError());
    L = GemmList{};
    blocks = 0;
    return ARMENV_OK;
  }
};

#define LRN_TRY(expr)                 \
  do {                                \
    const int rc_ = (expr);           \
    if (rc_ != ARMENV_OK) return rc_; \
  } while (0)

void adam_tensors(AdamArgs &P, const ArmEnvMlpRW &p, const ArmEnvMlpRW &m, const ArmEnvMlpRW &v, const ArmEnvMlpRW &tp, int in, int out,
                  const float *pW1, const float *pW2, const float *pW3) {
  const int H = LRN_H;
  struct R { float *p, *m, *v, *t; const float *part; int rows, cols, ldp, c0; };
  const R rs[6] = {{p.W1, m.W1, v.W1, tp.W1, pW1, H, in, kW1Ld, 0},   {p.b1, m.b1, v.b1, tp.b1, pW1, H, 1, kW1Ld, in},
                   {p.W2, m.W2, v.W2, tp.W2, pW2, H, H, H + 1, 0},    {p.b2, m.b2, v.b2, tp.b2, pW2, H, 1, H + 1, H},
                   {p.W3, m.W3, v.W3, tp.W3, pW3, out, H, H + 1, 0},  {p.b3, m.b3, v.b3, tp.b3, pW3, out, 1, H + 1, H}};
  for (const R &r : rs) {
    AdamTensor &T = P.t[P.n++];
    T.p = r.p; T.m = r.m; T.v = r.v; T.tp = r.t; T.partial = r.part;
    T.rows = r.rows; T.cols = r.cols; T.ldp = r.ldp; T.c0 = r.c0; T.first = P.total;
    P.total += r.rows * r.cols;
  }
}

// A kernel's argument block: its by-value arguments laid out in order, each at its own alignment.
template <class... KArgs>
constexpr size_t kernarg_bytes() {
  size_t o = 0;
  ((o = (o + alignof(KArgs) - 1) / alignof(KArgs) * alignof(KArgs) + sizeof(KArgs)), ...);
  return o;
}
constexpr size_t kMaxKernarg = 4096;
static_assert(kernarg_bytes<GemmList, GemmStrideList>() <= kMaxKernarg, "gemm_pop_kernel's arguments");
static_assert(kernarg_bytes<AdamArgs, int64_t, MemberTable, MemberTable, MemberTable>() <= kMaxKernarg, "adam_pop_hyper_kernel's arguments");
static_assert(kernarg_bytes<ActorHeadArgs, HeadStride, MemberTable, MemberTable>() <= kMaxKernarg, "actor_head_pop_hyper_kernel's arguments");
static_assert(kernarg_bytes<CriticHeadArgs, HeadStride, MemberTable>() <= kMaxKernarg, "critic_head_pop_hyper_kernel's arguments");
static_assert(kernarg_bytes<DaddpgCriticHeadArgs, HeadStride, MemberTable>() <= kMaxKernarg, "daddpg_critic_head_pop_hyper_kernel's arguments");
static_assert(kernarg_bytes<Datd3ActorHeadArgs, HeadStride, MemberTable, MemberTable>() <= kMaxKernarg,
              "datd3_actor_head_pop_hyper_kernel's arguments");
static_assert(kernarg_bytes<Datd3CriticHeadArgs, HeadStride, MemberTable, MemberTable, MemberTable, MemberTable>() <= kMaxKernarg,
              "datd3_critic_head_pop_hyper_kernel's arguments");
static_assert(kernarg_bytes<ExploitTable, ExploitSources>() <= kMaxKernarg, "pop_exploit_kernel's arguments");
static_assert(LRN_EXPLOIT_MAX_TENSORS == ARMENV_EXPLOIT_MAX_TENSORS, "the header's bound is the table's");

// Args: ArmEnvTd3Args, ArmEnvDaddpgArgs or ArmEnvDatd3Args (beta1, beta2, eps, tau).  `lr` is the args' learning rate of this
// optimiser and `lr_of` the same field of a member's ArmEnvPopHyper; `loss_w1_of`: the member's field that P.loss_w1 is, or NULL
// where it is no hyper-parameter.
template <class Args>
int launch_adam(AdamArgs &P, float lr, float ArmEnvPopHyper::*lr_of, float ArmEnvPopHyper::*loss_w1_of, int64_t step, const Args *a,
                const MemberStrides *pop, hipStream_t s) {
  P.beta1 = a->beta1; P.beta2 = a->beta2; P.eps = a->eps; P.tau = a->tau;
  const double bc1 = 1.0 - std::pow((double)a->beta1, (double)step), bc2 = 1.0 - std::pow((double)a->beta2, (double)step);
  P.step_size = (float)(lr / bc1);
  P.bc2_sqrt = (float)std::sqrt(bc2);
  const unsigned blocks = (unsigned)((P.total + 255) / 256) + (P.loss_rows ? 1u : 0u);
  if (pop && pop->hyper) {
    const float shared_w1 = P.loss_w1;
    hipLaunchKernelGGL(adam_pop_hyper_kernel, dim3(blocks, (unsigned)pop->members), dim3(256), 0, s, P, pop->ws,
                       pop->table([=](const ArmEnvPopHyper &h) { return (float)(h.*lr_of / bc1); }), pop->table(&ArmEnvPopHyper::tau),
                       pop->table([=](const ArmEnvPopHyper &h) { return loss_w1_of ? h.*loss_w1_of : shared_w1; }));
  } else if (pop)
    hipLaunchKernelGGL(adam_pop_kernel, dim3(blocks, (unsigned)pop->members), dim3(256), 0, s, P, pop->ws);
  else
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, s, P);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

bool mlp_ok(const ArmEnvMlpRW &m) { return m.W1 && m.b1 && m.W2 && m.b2 && m.W3 && m.b3; }
bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool mlp_aligned(const ArmEnvMlpRW &m) { return al16(m.W1) && al16(m.b1) && al16(m.W2) && al16(m.b2) && al16(m.W3) && al16(m.b3); }

constexpr int64_t kMaxBatch = (int64_t)1 << 20;

// Argument checks the updates share (Args: ArmEnvTd3Args, ArmEnvDaddpgArgs or ArmEnvDatd3Args); each names the field it refuses.
template <class Args>
int check_sizes(const char *fn, const Args *a) {
  if (!a) return fail(ARMENV_EINVAL, "%s: args is NULL", fn);
  if (a->device < 0) return fail(ARMENV_EINVAL, "%s: device %d", fn, a->device);
  if (a->state_dim < 1 || a->state_dim > 12) return fail(ARMENV_EINVAL, "%s: state_dim %d outside 1..12", fn, a->state_dim);
  if (a->action_dim != LRN_A) return fail(ARMENV_EINVAL, "%s: action_dim %d; the fused update is built for 3", fn, a->action_dim);
  if (a->hidden_dim != LRN_H) return fail(ARMENV_EINVAL, "%s: hidden_dim %d; the fused update is built for %d", fn, a->hidden_dim, LRN_H);
  if (a->batch < 1 || a->batch > kMaxBatch) return fail(ARMENV_EINVAL, "%s: batch %lld outside 1..%lld", fn, (long long)a->batch, (long long)kMaxBatch);
  return ARMENV_OK;
}

struct NamedF { const char *name; float v; bool ok; };
struct NamedNet { const char *name; const ArmEnvMlpRW *m; };

// Hyper-parameters, the nets and moments, the batch buffers and the workspace (`need` bytes).  The hyper-parameters are checked in
// the order action_bound, gamma, tau, `after_tau` (the algorithm's own), actor_lr, critic_lr, beta1, beta2, eps, `last` (its own):
// the first one out of range is the one named.
template <class Args, size_t NN>
int check_buffers(const char *fn, const Args *a, std::initializer_list<NamedF> after_tau, std::initializer_list<NamedF> last,
                  const NamedNet (&nets)[NN], int64_t need, const char *ws_fn) {
  const NamedF first[] = {{"action_bound", a->action_bound, a->action_bound > 0.f}, {"gamma", a->gamma, a->gamma >= 0.f && a->gamma <= 1.f},
                          {"tau", a->tau, a->tau >= 0.f && a->tau <= 1.f}};
  const NamedF optimiser[] = {{"actor_lr", a->actor_lr, a->actor_lr >= 0.f}, {"critic_lr", a->critic_lr, a->critic_lr >= 0.f},
                              {"beta1", a->beta1, a->beta1 >= 0.f && a->beta1 < 1.f}, {"beta2", a->beta2, a->beta2 >= 0.f && a->beta2 < 1.f},
                              {"eps", a->eps, a->eps > 0.f}};
  const struct { const NamedF *b, *e; } groups[] = {{first, first + 3}, {after_tau.begin(), after_tau.end()}, {optimiser, optimiser + 5},
                                                    {last.begin(), last.end()}};
  for (const auto &grp : groups)
    for (const NamedF *h = grp.b; h != grp.e; ++h)
      if (!std::isfinite(h->v) || !h->ok) return fail(ARMENV_EINVAL, "%s: %s = %g out of range", fn, h->name, (double)h->v);
  for (const auto &n : nets) {
    if (!mlp_ok(*n.m)) return fail(ARMENV_EINVAL, "%s: %s has a NULL pointer", fn, n.name);
    if (!mlp_aligned(*n.m)) return fail(ARMENV_EINVAL, "%s: %s has a pointer that is not 16-byte aligned", fn, n.name);
  }
  const struct { const char *name; const void *p; } bufs[] = {
      {"states_dev", a->states_dev}, {"actions_dev", a->actions_dev}, {"next_states_dev", a->next_states_dev},
      {"rewards_dev", a->rewards_dev}, {"dones_dev", a->dones_dev}, {"workspace_dev", a->workspace_dev}};
  for (const auto &b : bufs)
    if (!b.p) return fail(ARMENV_EINVAL, "%s: %s is NULL", fn, b.name);
  if (!al16(a->workspace_dev)) return fail(ARMENV_EINVAL, "%s: workspace_dev is not 16-byte aligned", fn);
  if (a->workspace_bytes < need)
    return fail(ARMENV_EINVAL, "%s: workspace_bytes %lld, need %lld (%s)", fn, (long long)a->workspace_bytes, (long long)need, ws_fn);
  return ARMENV_OK;
}

// The members' own hyper-parameters of an armenv_*_pop_update_hyper call: of each hyper[p], the fields the agent reads (`noise`: the
// target-policy noise's two; `darc`: DARC's two) against the ranges of check_buffers, the first one out of range named.
int check_hyper(const char *fn, const ArmEnvPopHyper *hyper, int members, bool noise, bool darc) {
  for (int p = 0; p < members; ++p) {
    const ArmEnvPopHyper &h = hyper[p];
    const struct { const char *name; float v; bool read, ok; } fields[] = {
        {"gamma", h.gamma, true, h.gamma >= 0.f && h.gamma <= 1.f},
        {"tau", h.tau, true, h.tau >= 0.f && h.tau <= 1.f},
        {"policy_noise", h.policy_noise, noise, h.policy_noise >= 0.f},
        {"noise_clip", h.noise_clip, noise, h.noise_clip >= 0.f},
        {"actor_lr", h.actor_lr, true, h.actor_lr >= 0.f},
        {"critic_lr", h.critic_lr, true, h.critic_lr >= 0.f},
        {"q_weight", h.q_weight, darc, h.q_weight >= 0.f && h.q_weight <= 1.f},
        {"regularization_weight", h.regularization_weight, darc, h.regularization_weight >= 0.f}};
    for (const auto &f : fields)
      if (f.read && (!std::isfinite(f.v) || !f.ok)) return fail(ARMENV_EINVAL, "%s: hyper[%d].%s = %g out of range", fn, p, f.name, (double)f.v);
  }
  return ARMENV_OK;
}

// the target-policy noise's two, which TD3 and DATD3 / DARC check after tau
#define LRN_NOISE_HP(a) \
  {"policy_noise", (a)->policy_noise, (a)->policy_noise >= 0.f}, {"noise_clip", (a)->noise_clip, (a)->noise_clip >= 0.f}

// the *_workspace_bytes queries: bytes of `w`, or -1 outside the shapes the update is built for
bool shape_ok(int32_t state_dim, int32_t hidden_dim, int64_t batch) {
  return state_dim >= 1 && state_dim <= 12 && hidden_dim == LRN_H && batch >= 1 && batch <= kMaxBatch;
}
int64_t bytes_of(const Ws &w) { return w.total * (int64_t)sizeof(float); }

// A net that an update steps: its parameters, Adam moments and the target that its Adam launch soft-updates.
struct Stepped {
  const ArmEnvMlpRW *p, *m, *v, *tp;
};

// One update as run_update reads it; each entry point fills it from its own Args.
struct Update {
  Ws w;
  float *ws;
  int n_ta;                    // target actors: 1 (TD3) or 2; target actor i writes proposal a2[i]
  const ArmEnvMlpRW *TA[2];
  int n_q;                     // stepped critics: 2 (TD3) or 1
  Stepped Q[2];
  const ArmEnvMlpRW *TQ[2];    // target-critic evaluation i: net TQ[i] over cat(s2, a2[tq_a2[i]])
  int tq_a2[2];
  const ArmEnvMlpRW *other;    // darc: the read-only other critic; else NULL
  Stepped act;                 // the actor to step; act.p NULL (TD3 without with_actor): none, and the update ends after stage 9
  const ArmEnvMlpRW *Qa;       // the stepped critic that the actor's loss reads
  int critic_soft;             // stage 9: soft-update the stepped critics' targets
  int loss_cols;               // stage 9: columns of the loss rows
  float loss_w1;               //          and the weight of column 1's mean
  float ArmEnvPopHyper::*loss_w1_of;   //      and, where that weight is a hyper-parameter (DARC), a member's field of it; else NULL
  int64_t loss_rows;           //          and where they are in the workspace
  const MemberStrides *pop;    // a population update: its member count, strides and (hyper) the members' own hyper-parameters; NULL:
                               // one learner, the single-learner kernels
};

// one launch of a per-row kernel (256 threads: four rows per workgroup)
template <class Kernel, class KArgs>
int launch_rows(Kernel kernel, unsigned blocks, const KArgs &args, hipStream_t s) {
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, args);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

// ... and of its population form over (blocks, members); `tables`: the further arguments of a *_pop_hyper_kernel
template <class Kernel, class KArgs, class KStride, class... Tables>
int launch_rows_pop(Kernel kernel, unsigned blocks, int members, const KArgs &args, const KStride &strides, hipStream_t s,
                    const Tables &...tables) {
  hipLaunchKernelGGL(kernel, dim3(blocks, (unsigned)members), dim3(256), 0, s, args, strides, tables...);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

// Stages 1-2, 4-5, 7-9 and 10-16 over `u`; actor_heads(row_blocks) is stage 3 and critic_heads(row_blocks) stage 6, each the entry
// point's own launch returning ARMENV_OK or a failure.  Args: ArmEnvTd3Args, ArmEnvDaddpgArgs or ArmEnvDatd3Args.
template <class Args, class ActorHeads, class CriticHeads>
int run_update(const Args *a, const Update &u, hipStream_t s, ActorHeads actor_heads, CriticHeads critic_heads) {
  const int D = a->state_dim, K1 = D + LRN_A, H = LRN_H;
  const int64_t B = a->batch;
  const Ws &w = u.w;
  float *ws = u.ws;
  const float inv_b = 1.0f / (float)B;
  const bool with_actor = u.act.p != nullptr;
  const Feat s_only = feat(a->states_dev, D, D, B), s2_only = feat(a->next_states_dev, D, D, B);
  const Feat sa = feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B);
  auto hidden = [&](int64_t off, int aug = 0) { return feat(ws + off, H, H, B, aug); };
  Launcher L;
  L.pop = u.pop;

  // 1-2: layers 1 and 2 of the target actors, the stepped critics, the stepped actor and the other critic
  for (int i = 0; i < u.n_ta; ++i) L.forward(s2_only, D, u.TA[i]->W1, u.TA[i]->b1, ws + w.ta1[i], B);
  for (int i = 0; i < u.n_q; ++i) L.forward(sa, K1, u.Q[i].p->W1, u.Q[i].p->b1, ws + w.h1[i], B);
  if (with_actor) L.forward(s_only, D, u.act.p->W1, u.act.p->b1, ws + w.ah1, B);
  if (u.other) L.forward(sa, K1, u.other->W1, u.other->b1, ws + w.oh1, B);
  LRN_TRY(L.launch(s));
  for (int i = 0; i < u.n_ta; ++i) L.forward(hidden(w.ta1[i]), H, u.TA[i]->W2, u.TA[i]->b2, ws + w.ta2[i], B);
  for (int i = 0; i < u.n_q; ++i) L.forward(hidden(w.h1[i]), H, u.Q[i].p->W2, u.Q[i].p->b2, ws + w.h2[i], B);
  if (with_actor) L.forward(hidden(w.ah1), H, u.act.p->W2, u.act.p->b2, ws + w.ah2, B);
  if (u.other) L.forward(hidden(w.oh1), H, u.other->W2, u.other->b2, ws + w.oh2, B);
  LRN_TRY(L.launch(s));

  // 3: the actors' heads
  const unsigned row_blocks = grid_for(B, 4);
  LRN_TRY(actor_heads(row_blocks));

  // 4-5: the two target-critic evaluations, each over its proposal
  for (int i = 0; i < 2; ++i)
    L.forward(feat2(a->next_states_dev, D, ws + w.a2[u.tq_a2[i]], LRN_A, K1, B), K1, u.TQ[i]->W1, u.TQ[i]->b1, ws + w.tq1[i], B);
  LRN_TRY(L.launch(s));
  for (int i = 0; i < 2; ++i) L.forward(hidden(w.tq1[i]), H, u.TQ[i]->W2, u.TQ[i]->b2, ws + w.tq2[i], B);
  LRN_TRY(L.launch(s));

  // 6: target, loss rows, the stepped critics' deltas
  LRN_TRY(critic_heads(row_blocks));

  // 7-8: the stepped critics' backward and weight-gradient partials
  for (int i = 0; i < u.n_q; ++i) {
    L.backward(ws + w.d2[i], u.Q[i].p->W2, ws + w.h1[i], ws + w.d1[i], B);
    L.wgrad(ws + w.d3[i], 1, hidden(w.h2[i], 1), H, ws + w.pW3[i], H + 1, B, w.split_stride);
    L.wgrad(ws + w.d2[i], H, hidden(w.h1[i], 1), H, ws + w.pW2[i], H + 1, B, w.split_stride);
  }
  LRN_TRY(L.launch(s));
  const Feat sa_aug = feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B, 1);
  for (int i = 0; i < u.n_q; ++i) L.wgrad(ws + w.d1[i], H, sa_aug, K1, ws + w.pW1[i], kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 9: the stepped critics' Adam + the loss (+ their targets' soft update: the critics are final by then)
  {
    AdamArgs P{};
    for (int i = 0; i < u.n_q; ++i)
      adam_tensors(P, *u.Q[i].p, *u.Q[i].m, *u.Q[i].v, *u.Q[i].tp, K1, 1, ws + w.pW1[i], ws + w.pW2[i], ws + w.pW3[i]);
    P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = u.critic_soft;
    P.loss_rows = ws + u.loss_rows; P.loss_cols = u.loss_cols; P.loss_w1 = u.loss_w1; P.B = B; P.inv_b = inv_b; P.loss = a->loss_dev;
    LRN_TRY(launch_adam(P, a->critic_lr, &ArmEnvPopHyper::critic_lr, u.loss_w1_of, a->critic_step, a, u.pop, s));
  }
  if (!with_actor) return ARMENV_OK;

  // 10-12: Qa(s, actor(s)) with the stepped critic and its backward to Qa's input; c1 / dc2 / dc1 / da2 / da1 reuse the target path's
  // buffers
  const ArmEnvMlpRW &Qa = *u.Qa, &act = *u.act.p;
  float *c1 = ws + w.ta1[0], *dc2 = ws + w.ta2[0], *dc1 = ws + w.tq1[0], *da2 = ws + w.tq1[1], *da1 = ws + w.tq2[0];
  L.forward(feat2(a->states_dev, D, ws + w.api, LRN_A, K1, B), K1, Qa.W1, Qa.b1, c1, B);
  LRN_TRY(L.launch(s));
  L.forward(feat(c1, H, H, B), H, Qa.W2, Qa.b2, dc2, B, EPI_DRELU_W, Qa.W3, -1.0f / (float)B);
  LRN_TRY(L.launch(s));
  L.backward(dc2, Qa.W2, c1, dc1, B);
  LRN_TRY(L.launch(s));

  // 13: through cat -> tanh -> the stepped actor's fc3
  ActorBackArgs ab{};
  ab.B = B; ab.in_dim = K1; ab.state_dim = D; ab.bound = a->action_bound; ab.dc1 = dc1; ab.Wq1 = Qa.W1;
  ab.tanh_a = ws + w.tanh_a; ab.h2 = ws + w.ah2; ab.W3 = act.W3; ab.du = ws + w.du; ab.da2 = da2;
  if (u.pop)
    LRN_TRY(launch_rows_pop(actor_back_pop_kernel, row_blocks, u.pop->members, ab,
                            ActorBackStride{u.pop->ws, (int64_t)H * K1, (int64_t)LRN_A * H}, s));
  else
    LRN_TRY(launch_rows(actor_back_kernel, row_blocks, ab, s));

  // 14-15: the stepped actor's backward and weight-gradient partials (the critics' partials are consumed: same slices)
  L.backward(da2, act.W2, ws + w.ah1, da1, B);
  L.wgrad(ws + w.du, LRN_A, hidden(w.ah2, 1), H, ws + w.pa3, H + 1, B, w.split_stride);
  L.wgrad(da2, H, hidden(w.ah1, 1), H, ws + w.pa2, H + 1, B, w.split_stride);
  LRN_TRY(L.launch(s));
  L.wgrad(da1, H, feat(a->states_dev, D, D, B, 1), D, ws + w.pa1, kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 16: the stepped actor's Adam + its target's soft update
  AdamArgs P{};
  adam_tensors(P, act, *u.act.m, *u.act.v, *u.act.tp, D, LRN_A, ws + w.pa1, ws + w.pa2, ws + w.pa3);
  P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = 1;
  return launch_adam(P, a->actor_lr, &ArmEnvPopHyper::actor_lr, nullptr, a->actor_step, a, u.pop, s);
}

}  // namespace

extern "C" {

int64_t armenv_td3_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch) {
  return shape_ok(state_dim, hidden_dim, batch) ? bytes_of(layout(batch, 1, 2, false)) : -1;
}

}  // extern "C"

namespace {

constexpr int kMaxMembers = 64;

// armenv_td3_update (members 1, pop false: the single-learner kernels), armenv_td3_pop_update (pop true: the population kernels
// over `members` stacked learners, `a` being member 0's arguments) and armenv_td3_pop_update_hyper (pop true and `hyper`, the members'
// own hyper-parameters, set)
int td3_update(const char *fn, const ArmEnvTd3Args *a, int members, bool pop, const ArmEnvPopHyper *hyper, const char *ws_fn,
               void *stream) {
  LRN_TRY(check_sizes(fn, a));
  if (a->with_actor != 0 && a->with_actor != 1) return fail(ARMENV_EINVAL, "%s: with_actor must be 0 or 1", fn);
  if (a->critic_step < 1) return fail(ARMENV_EINVAL, "%s: critic_step must be >= 1", fn);
  if (a->with_actor && a->actor_step < 1) return fail(ARMENV_EINVAL, "%s: actor_step must be >= 1", fn);
  const NamedNet nets[] = {
      {"actor", &a->actor}, {"q1", &a->q1}, {"q2", &a->q2}, {"target_actor", &a->target_actor}, {"target_q1", &a->target_q1},
      {"target_q2", &a->target_q2}, {"actor_m", &a->actor_m}, {"actor_v", &a->actor_v}, {"q1_m", &a->q1_m}, {"q1_v", &a->q1_v},
      {"q2_m", &a->q2_m}, {"q2_v", &a->q2_v}};
  const int64_t ws_bytes = armenv_td3_workspace_bytes(a->state_dim, a->hidden_dim, a->batch);
  LRN_TRY(check_buffers(fn, a, {LRN_NOISE_HP(a)}, {}, nets, ws_bytes * members, ws_fn));
  if (hyper) LRN_TRY(check_hyper(fn, hyper, members, true, false));

  DeviceGuard guard_(a->device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", fn, (int)a->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t B = a->batch;
  Update u{};
  u.w = layout(B, 1, 2, false);
  u.ws = static_cast<float *>(a->workspace_dev);
  const Ws &w = u.w;
  float *ws = u.ws;
  u.n_ta = 1; u.TA[0] = &a->target_actor;
  u.n_q = 2; u.Q[0] = {&a->q1, &a->q1_m, &a->q1_v, &a->target_q1}; u.Q[1] = {&a->q2, &a->q2_m, &a->q2_v, &a->target_q2};
  u.TQ[0] = &a->target_q1; u.TQ[1] = &a->target_q2;                         // both over the ONE proposal
  if (a->with_actor) u.act = {&a->actor, &a->actor_m, &a->actor_v, &a->target_actor};
  u.Qa = &a->q1;
  u.critic_soft = a->with_actor; u.loss_cols = 2; u.loss_w1 = 1.0f; u.loss_rows = w.loss2;

  const int D = a->state_dim, K1 = D + LRN_A;
  MemberStrides ms;
  if (pop) {
    ms.members = members;
    ms.hyper = hyper;
    ms.ws = ws_bytes / (int64_t)sizeof(float);
    ms.add(a->workspace_dev, ms.ws);
    for (const ArmEnvMlpRW *m : {&a->actor, &a->target_actor, &a->actor_m, &a->actor_v}) ms.add(*m, D, LRN_A);
    for (const ArmEnvMlpRW *m : {&a->q1, &a->q2, &a->target_q1, &a->target_q2, &a->q1_m, &a->q1_v, &a->q2_m, &a->q2_v}) ms.add(*m, K1, 1);
    ms.add(a->states_dev, B * D); ms.add(a->next_states_dev, B * D); ms.add(a->actions_dev, B * LRN_A);
    ms.add(a->rewards_dev, B); ms.add(a->dones_dev, B, 1); ms.add(a->noise_dev, B * LRN_A);
    u.pop = &ms;
  }

  ActorHeadArgs ah{};
  ah.B = B; ah.t_h2 = ws + w.ta2[0]; ah.t_W3 = a->target_actor.W3; ah.t_b3 = a->target_actor.b3; ah.noise = a->noise_dev;
  ah.seed = a->seed; ah.draw = a->draw; ah.bound = a->action_bound; ah.policy_noise = a->policy_noise; ah.noise_clip = a->noise_clip;
  ah.a2 = ws + w.a2[0]; ah.with_actor = a->with_actor; ah.h2 = ws + w.ah2; ah.W3 = a->actor.W3; ah.b3 = a->actor.b3;
  ah.a = ws + w.api; ah.tanh_out = ws + w.tanh_a;

  CriticHeadArgs ch{};
  ch.B = B; ch.gamma = a->gamma; ch.inv_b = 1.0f / (float)B; ch.rewards = a->rewards_dev; ch.dones = a->dones_dev;
  for (int i = 0; i < 2; ++i) {
    ch.t_h2[i] = ws + w.tq2[i]; ch.t_W3[i] = u.TQ[i]->W3; ch.t_b3[i] = u.TQ[i]->b3;
    ch.h2[i] = ws + w.h2[i]; ch.W3[i] = u.Q[i].p->W3; ch.b3[i] = u.Q[i].p->b3;
    ch.d3[i] = ws + w.d3[i]; ch.d2[i] = ws + w.d2[i];
  }
  ch.loss_rows = ws + u.loss_rows;

  if (pop) {
    const HeadStride actor_st{ms.ws, (int64_t)LRN_A * LRN_H, LRN_A, B, B * LRN_A}, critic_st{ms.ws, LRN_H, 1, B, 0};
    return run_update(
        a, u, s,
        [&](unsigned row_blocks) {
          const unsigned blocks = row_blocks * (a->with_actor ? 2u : 1u);
          if (hyper)
            return launch_rows_pop(actor_head_pop_hyper_kernel, blocks, members, ah, actor_st, s, ms.table(&ArmEnvPopHyper::policy_noise),
                                   ms.table(&ArmEnvPopHyper::noise_clip));
          return launch_rows_pop(actor_head_pop_kernel, blocks, members, ah, actor_st, s);
        },
        [&](unsigned row_blocks) {
          if (hyper) return launch_rows_pop(critic_head_pop_hyper_kernel, row_blocks, members, ch, critic_st, s, ms.table(&ArmEnvPopHyper::gamma));
          return launch_rows_pop(critic_head_pop_kernel, row_blocks, members, ch, critic_st, s);
        });
  }
  return run_update(
      a, u, s, [&](unsigned row_blocks) { return launch_rows(actor_head_kernel, row_blocks * (a->with_actor ? 2u : 1u), ah, s); },
      [&](unsigned row_blocks) { return launch_rows(critic_head_kernel, row_blocks, ch, s); });
}

}  // namespace

extern "C" {

int armenv_td3_update(const ArmEnvTd3Args *a, void *stream) {
  return td3_update("armenv_td3_update", a, 1, false, nullptr, "armenv_td3_workspace_bytes", stream);
}

int64_t armenv_td3_pop_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch, int32_t members) {
  if (members < 1 || members > kMaxMembers) return -1;
  const int64_t one = armenv_td3_workspace_bytes(state_dim, hidden_dim, batch);
  return one < 0 ? -1 : one * members;
}

int armenv_td3_pop_update(const ArmEnvTd3PopArgs *a, void *stream) {
  static const char *fn = "armenv_td3_pop_update";
  if (!a) return fail(ARMENV_EINVAL, "%s: args is NULL", fn);
  if (a->members < 1 || a->members > kMaxMembers) return fail(ARMENV_EINVAL, "%s: members %d outside 1..%d", fn, (int)a->members, kMaxMembers);
  return td3_update(fn, &a->one, a->members, true, nullptr, "armenv_td3_pop_workspace_bytes", stream);
}

int64_t armenv_daddpg_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch) {
  return shape_ok(state_dim, hidden_dim, batch) ? bytes_of(layout(batch, 2, 1, false)) : -1;
}

}  // extern "C"

namespace {

// armenv_daddpg_update (members 1, pop false), armenv_daddpg_pop_update (pop true, `a` being member 0's arguments) and
// armenv_daddpg_pop_update_hyper (and `hyper` set), as td3_update
int daddpg_update(const char *fn, const ArmEnvDaddpgArgs *a, int members, bool pop, const ArmEnvPopHyper *hyper, const char *ws_fn,
                  void *stream) {
  LRN_TRY(check_sizes(fn, a));
  if (a->update_actor != 1 && a->update_actor != 2) return fail(ARMENV_EINVAL, "%s: update_actor %d must be 1 or 2", fn, a->update_actor);
  if (a->critic_step < 1) return fail(ARMENV_EINVAL, "%s: critic_step must be >= 1", fn);
  if (a->actor_step < 1) return fail(ARMENV_EINVAL, "%s: actor_step must be >= 1", fn);
  const NamedNet nets[] = {
      {"actor1", &a->actor1}, {"actor2", &a->actor2}, {"critic", &a->critic}, {"target_actor1", &a->target_actor1},
      {"target_actor2", &a->target_actor2}, {"target_critic", &a->target_critic}, {"actor1_m", &a->actor1_m},
      {"actor1_v", &a->actor1_v}, {"actor2_m", &a->actor2_m}, {"actor2_v", &a->actor2_v}, {"critic_m", &a->critic_m},
      {"critic_v", &a->critic_v}};
  const int64_t ws_bytes = armenv_daddpg_workspace_bytes(a->state_dim, a->hidden_dim, a->batch);
  LRN_TRY(check_buffers(fn, a, {}, {}, nets, ws_bytes * members, ws_fn));
  if (hyper) LRN_TRY(check_hyper(fn, hyper, members, false, false));

  DeviceGuard guard_(a->device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", fn, (int)a->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t B = a->batch;
  const bool second = a->update_actor == 2;
  Update u{};
  u.w = layout(B, 2, 1, false);
  u.ws = static_cast<float *>(a->workspace_dev);
  const Ws &w = u.w;
  float *ws = u.ws;
  u.n_ta = 2; u.TA[0] = &a->target_actor1; u.TA[1] = &a->target_actor2;
  u.n_q = 1; u.Q[0] = {&a->critic, &a->critic_m, &a->critic_v, &a->target_critic};
  u.TQ[0] = u.TQ[1] = &a->target_critic; u.tq_a2[1] = 1;                    // the ONE target critic over both proposals
  u.act = second ? Stepped{&a->actor2, &a->actor2_m, &a->actor2_v, &a->target_actor2}
                 : Stepped{&a->actor1, &a->actor1_m, &a->actor1_v, &a->target_actor1};
  u.Qa = &a->critic;
  u.critic_soft = second; u.loss_cols = 1; u.loss_rows = w.loss1;            // the target critic moves when actor 2 is stepped

  DaddpgActorHeadArgs ah{};
  ah.B = B; ah.bound = a->action_bound;
  for (int i = 0; i < 2; ++i) { ah.h2[i] = ws + w.ta2[i]; ah.W3[i] = u.TA[i]->W3; ah.b3[i] = u.TA[i]->b3; ah.a[i] = ws + w.a2[i]; }
  ah.h2[2] = ws + w.ah2; ah.W3[2] = u.act.p->W3; ah.b3[2] = u.act.p->b3; ah.a[2] = ws + w.api; ah.tanh_out = ws + w.tanh_a;

  DaddpgCriticHeadArgs ch{};
  ch.B = B; ch.gamma = a->gamma; ch.inv_b = 1.0f / (float)B; ch.rewards = a->rewards_dev; ch.dones = a->dones_dev;
  ch.t_h2[0] = ws + w.tq2[0]; ch.t_h2[1] = ws + w.tq2[1]; ch.t_W3 = a->target_critic.W3; ch.t_b3 = a->target_critic.b3;
  ch.h2 = ws + w.h2[0]; ch.W3 = a->critic.W3; ch.b3 = a->critic.b3; ch.d3 = ws + w.d3[0]; ch.d2 = ws + w.d2[0];
  ch.loss_rows = ws + u.loss_rows;

  const int D = a->state_dim, K1 = D + LRN_A;
  MemberStrides ms;
  if (pop) {
    ms.members = members;
    ms.hyper = hyper;
    ms.ws = ws_bytes / (int64_t)sizeof(float);
    ms.add(a->workspace_dev, ms.ws);
    for (const ArmEnvMlpRW *m : {&a->actor1, &a->actor2, &a->target_actor1, &a->target_actor2, &a->actor1_m, &a->actor1_v, &a->actor2_m,
                                 &a->actor2_v})
      ms.add(*m, D, LRN_A);
    for (const ArmEnvMlpRW *m : {&a->critic, &a->target_critic, &a->critic_m, &a->critic_v}) ms.add(*m, K1, 1);
    ms.add(a->states_dev, B * D); ms.add(a->next_states_dev, B * D); ms.add(a->actions_dev, B * LRN_A);
    ms.add(a->rewards_dev, B); ms.add(a->dones_dev, B, 1);
    u.pop = &ms;
    const HeadStride actor_st{ms.ws, (int64_t)LRN_A * LRN_H, LRN_A, B, 0}, critic_st{ms.ws, LRN_H, 1, B, 0};
    return run_update(
        a, u, s,
        [&](unsigned row_blocks) { return launch_rows_pop(daddpg_actor_head_pop_kernel, row_blocks * 3u, members, ah, actor_st, s); },
        [&](unsigned row_blocks) {
          if (hyper)
            return launch_rows_pop(daddpg_critic_head_pop_hyper_kernel, row_blocks, members, ch, critic_st, s, ms.table(&ArmEnvPopHyper::gamma));
          return launch_rows_pop(daddpg_critic_head_pop_kernel, row_blocks, members, ch, critic_st, s);
        });
  }
  return run_update(
      a, u, s, [&](unsigned row_blocks) { return launch_rows(daddpg_actor_head_kernel, row_blocks * 3u, ah, s); },
      [&](unsigned row_blocks) { return launch_rows(daddpg_critic_head_kernel, row_blocks, ch, s); });
}

// the checks of a *_pop_update entry point's own fields
template <class PopArgs>
int check_members(const char *fn, const PopArgs *a) {
  if (!a) return fail(ARMENV_EINVAL, "%s: args is NULL", fn);
  if (a->members < 1 || a->members > kMaxMembers) return fail(ARMENV_EINVAL, "%s: members %d outside 1..%d", fn, (int)a->members, kMaxMembers);
  return ARMENV_OK;
}

int64_t pop_bytes(int64_t one, int32_t members) { return members < 1 || members > kMaxMembers || one < 0 ? -1 : one * members; }

}  // namespace

extern "C" {

int armenv_daddpg_update(const ArmEnvDaddpgArgs *a, void *stream) {
  return daddpg_update("armenv_daddpg_update", a, 1, false, nullptr, "armenv_daddpg_workspace_bytes", stream);
}

int64_t armenv_daddpg_pop_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch, int32_t members) {
  return pop_bytes(armenv_daddpg_workspace_bytes(state_dim, hidden_dim, batch), members);
}

int armenv_daddpg_pop_update(const ArmEnvDaddpgPopArgs *a, void *stream) {
  static const char *fn = "armenv_daddpg_pop_update";
  LRN_TRY(check_members(fn, a));
  return daddpg_update(fn, &a->one, a->members, true, nullptr, "armenv_daddpg_pop_workspace_bytes", stream);
}

int64_t armenv_datd3_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch) {
  return shape_ok(state_dim, hidden_dim, batch) ? bytes_of(layout(batch, 2, 1, true)) : -1;
}

}  // extern "C"

namespace {

// armenv_datd3_update (members 1, pop false), armenv_datd3_pop_update (pop true, `a` being member 0's arguments) and
// armenv_datd3_pop_update_hyper (and `hyper` set), as td3_update
int datd3_update(const char *fn, const ArmEnvDatd3Args *a, int members, bool pop, const ArmEnvPopHyper *hyper, const char *ws_fn,
                 void *stream) {
  LRN_TRY(check_sizes(fn, a));
  if (a->update_actor != 1 && a->update_actor != 2) return fail(ARMENV_EINVAL, "%s: update_actor %d must be 1 or 2", fn, a->update_actor);
  if (a->darc != 0 && a->darc != 1) return fail(ARMENV_EINVAL, "%s: darc %d must be 0 or 1", fn, a->darc);
  if (a->critic_step < 1) return fail(ARMENV_EINVAL, "%s: critic_step must be >= 1", fn);
  if (a->actor_step < 1) return fail(ARMENV_EINVAL, "%s: actor_step must be >= 1", fn);
  const bool darc = a->darc == 1;
  const NamedNet nets[] = {
      {"actor1", &a->actor1}, {"actor2", &a->actor2}, {"critic1", &a->critic1}, {"critic2", &a->critic2},
      {"target_actor1", &a->target_actor1}, {"target_actor2", &a->target_actor2}, {"target_critic1", &a->target_critic1},
      {"target_critic2", &a->target_critic2}, {"actor1_m", &a->actor1_m}, {"actor1_v", &a->actor1_v}, {"actor2_m", &a->actor2_m},
      {"actor2_v", &a->actor2_v}, {"critic1_m", &a->critic1_m}, {"critic1_v", &a->critic1_v}, {"critic2_m", &a->critic2_m},
      {"critic2_v", &a->critic2_v}};
  // q_weight and regularization_weight are read only when darc
  const int64_t ws_bytes = armenv_datd3_workspace_bytes(a->state_dim, a->hidden_dim, a->batch);
  LRN_TRY(check_buffers(fn, a, {LRN_NOISE_HP(a)},
                        {{"q_weight", darc ? a->q_weight : 0.f, !darc || (a->q_weight >= 0.f && a->q_weight <= 1.f)},
                         {"regularization_weight", darc ? a->regularization_weight : 0.f, !darc || a->regularization_weight >= 0.f}},
                        nets, ws_bytes * members, ws_fn));
  if (hyper) LRN_TRY(check_hyper(fn, hyper, members, true, darc));

  DeviceGuard guard_(a->device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", fn, (int)a->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t B = a->batch;
  const bool second = a->update_actor == 2;
  const ArmEnvMlpRW &Qo = second ? a->critic1 : a->critic2;     // read only (darc)
  Update u{};
  u.w = layout(B, 2, 1, true);
  u.ws = static_cast<float *>(a->workspace_dev);
  const Ws &w = u.w;
  float *ws = u.ws;
  u.n_ta = 2; u.TA[0] = &a->target_actor1; u.TA[1] = &a->target_actor2;
  u.n_q = 1;
  u.Q[0] = second ? Stepped{&a->critic2, &a->critic2_m, &a->critic2_v, &a->target_critic2}
                  : Stepped{&a->critic1, &a->critic1_m, &a->critic1_v, &a->target_critic1};
  u.TQ[0] = &a->target_critic1; u.TQ[1] = &a->target_critic2; u.tq_a2[1] = 1;   // target critic j over its own actor's proposal
  if (darc) u.other = &Qo;
  u.act = second ? Stepped{&a->actor2, &a->actor2_m, &a->actor2_v, &a->target_actor2}
                 : Stepped{&a->actor1, &a->actor1_m, &a->actor1_v, &a->target_actor1};
  u.Qa = u.Q[0].p;
  // target critic k always moves: the actor's loss does not read it
  u.critic_soft = 1; u.loss_cols = darc ? 2 : 1; u.loss_w1 = darc ? a->regularization_weight : 0.f; u.loss_rows = darc ? w.loss2 : w.loss1;
  if (darc) u.loss_w1_of = &ArmEnvPopHyper::regularization_weight;

  Datd3ActorHeadArgs ah{};
  ah.B = B; ah.bound = a->action_bound; ah.policy_noise = a->policy_noise; ah.noise_clip = a->noise_clip;
  ah.noise = a->noise_dev; ah.seed = a->seed; ah.draw = a->draw;
  for (int i = 0; i < 2; ++i) { ah.t_h2[i] = ws + w.ta2[i]; ah.t_W3[i] = u.TA[i]->W3; ah.t_b3[i] = u.TA[i]->b3; ah.a2[i] = ws + w.a2[i]; }
  ah.h2 = ws + w.ah2; ah.W3 = u.act.p->W3; ah.b3 = u.act.p->b3; ah.a = ws + w.api; ah.tanh_out = ws + w.tanh_a;

  Datd3CriticHeadArgs ch{};
  ch.B = B; ch.gamma = a->gamma; ch.inv_b = 1.0f / (float)B; ch.rewards = a->rewards_dev; ch.dones = a->dones_dev;
  ch.darc = a->darc;
  if (darc) {
    ch.w_min = a->q_weight; ch.w_max = (float)(1.0 - (double)a->q_weight); ch.reg = a->regularization_weight;
    ch.o_h2 = ws + w.oh2; ch.o_W3 = Qo.W3; ch.o_b3 = Qo.b3;
  }
  for (int i = 0; i < 2; ++i) { ch.t_h2[i] = ws + w.tq2[i]; ch.t_W3[i] = u.TQ[i]->W3; ch.t_b3[i] = u.TQ[i]->b3; }
  ch.h2 = ws + w.h2[0]; ch.W3 = u.Q[0].p->W3; ch.b3 = u.Q[0].p->b3; ch.d3 = ws + w.d3[0]; ch.d2 = ws + w.d2[0];
  ch.loss_rows = ws + u.loss_rows;

  const int D = a->state_dim, K1 = D + LRN_A;
  MemberStrides ms;
  if (pop) {
    ms.members = members;
    ms.hyper = hyper;
    ms.ws = ws_bytes / (int64_t)sizeof(float);
    ms.add(a->workspace_dev, ms.ws);
    for (const ArmEnvMlpRW *m : {&a->actor1, &a->actor2, &a->target_actor1, &a->target_actor2, &a->actor1_m, &a->actor1_v, &a->actor2_m,
                                 &a->actor2_v})
      ms.add(*m, D, LRN_A);
    for (const ArmEnvMlpRW *m : {&a->critic1, &a->critic2, &a->target_critic1, &a->target_critic2, &a->critic1_m, &a->critic1_v,
                                 &a->critic2_m, &a->critic2_v})
      ms.add(*m, K1, 1);
    ms.add(a->states_dev, B * D); ms.add(a->next_states_dev, B * D); ms.add(a->actions_dev, B * LRN_A);
    ms.add(a->rewards_dev, B); ms.add(a->dones_dev, B, 1); ms.add(a->noise_dev, B * LRN_A);
    u.pop = &ms;
    const HeadStride actor_st{ms.ws, (int64_t)LRN_A * LRN_H, LRN_A, B, B * LRN_A}, critic_st{ms.ws, LRN_H, 1, B, 0};
    return run_update(
        a, u, s,
        [&](unsigned row_blocks) {
          if (hyper)
            return launch_rows_pop(datd3_actor_head_pop_hyper_kernel, row_blocks * 2u, members, ah, actor_st, s,
                                   ms.table(&ArmEnvPopHyper::policy_noise), ms.table(&ArmEnvPopHyper::noise_clip));
          return launch_rows_pop(datd3_actor_head_pop_kernel, row_blocks * 2u, members, ah, actor_st, s);
        },
        [&](unsigned row_blocks) {
          // w_min, w_max and reg as the single path forms them from a->q_weight and a->regularization_weight (read when darc)
          if (hyper)
            return launch_rows_pop(datd3_critic_head_pop_hyper_kernel, row_blocks, members, ch, critic_st, s, ms.table(&ArmEnvPopHyper::gamma),
                                   ms.table(&ArmEnvPopHyper::q_weight),
                                   ms.table([](const ArmEnvPopHyper &h) { return (float)(1.0 - (double)h.q_weight); }),
                                   ms.table(&ArmEnvPopHyper::regularization_weight));
          return launch_rows_pop(datd3_critic_head_pop_kernel, row_blocks, members, ch, critic_st, s);
        });
  }
  return run_update(
      a, u, s, [&](unsigned row_blocks) { return launch_rows(datd3_actor_head_kernel, row_blocks * 2u, ah, s); },
      [&](unsigned row_blocks) { return launch_rows(datd3_critic_head_kernel, row_blocks, ch, s); });
}

}  // namespace

extern "C" {

int armenv_datd3_update(const ArmEnvDatd3Args *a, void *stream) {
  return datd3_update("armenv_datd3_update", a, 1, false, nullptr, "armenv_datd3_workspace_bytes", stream);
}

int64_t armenv_datd3_pop_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch, int32_t members) {
  return pop_bytes(armenv_datd3_workspace_bytes(state_dim, hidden_dim, batch), members);
}

int armenv_datd3_pop_update(const ArmEnvDatd3PopArgs *a, void *stream) {
  static const char *fn = "armenv_datd3_pop_update";
  LRN_TRY(check_members(fn, a));
  return datd3_update(fn, &a->one, a->members, true, nullptr, "armenv_datd3_pop_workspace_bytes", stream);
}

int armenv_td3_pop_update_hyper(const ArmEnvTd3PopArgs *a, const ArmEnvPopHyper *hyper, void *stream) {
  static const char *fn = "armenv_td3_pop_update_hyper";
  LRN_TRY(check_members(fn, a));
  if (!hyper) return fail(ARMENV_EINVAL, "%s: hyper is NULL", fn);
  return td3_update(fn, &a->one, a->members, true, hyper, "armenv_td3_pop_workspace_bytes", stream);
}

int armenv_daddpg_pop_update_hyper(const ArmEnvDaddpgPopArgs *a, const ArmEnvPopHyper *hyper, void *stream) {
  static const char *fn = "armenv_daddpg_pop_update_hyper";
  LRN_TRY(check_members(fn, a));
  if (!hyper) return fail(ARMENV_EINVAL, "%s: hyper is NULL", fn);
  return daddpg_update(fn, &a->one, a->members, true, hyper, "armenv_daddpg_pop_workspace_bytes", stream);
}

int armenv_datd3_pop_update_hyper(const ArmEnvDatd3PopArgs *a, const ArmEnvPopHyper *hyper, void *stream) {
  static const char *fn = "armenv_datd3_pop_update_hyper";
  LRN_TRY(check_members(fn, a));
  if (!hyper) return fail(ARMENV_EINVAL, "%s: hyper is NULL", fn);
  return datd3_update(fn, &a->one, a->members, true, hyper, "armenv_datd3_pop_workspace_bytes", stream);
}

int armenv_pop_exploit(const ArmEnvPopExploitArgs *a, void *stream) {
  static const char *fn = "armenv_pop_exploit";
  if (!a) return fail(ARMENV_EINVAL, "%s: args is NULL", fn);
  if (!a->src) return fail(ARMENV_EINVAL, "%s: src is NULL", fn);
  if (!a->base) return fail(ARMENV_EINVAL, "%s: base is NULL", fn);
  if (!a->elems) return fail(ARMENV_EINVAL, "%s: elems is NULL", fn);
  if (a->device < 0) return fail(ARMENV_EINVAL, "%s: device %d", fn, (int)a->device);
  if (a->members < 1 || a->members > kMaxMembers) return fail(ARMENV_EINVAL, "%s: members %d outside 1..%d", fn, (int)a->members, kMaxMembers);
  if (a->tensors < 1 || a->tensors > LRN_EXPLOIT_MAX_TENSORS)
    return fail(ARMENV_EINVAL, "%s: tensors %d outside 1..%d", fn, (int)a->tensors, LRN_EXPLOIT_MAX_TENSORS);
  ExploitTable T{};
  int64_t blocks = 0;
  for (int t = 0; t < a->tensors; ++t) {
    if (!a->base[t]) return fail(ARMENV_EINVAL, "%s: base[%d] is NULL", fn, t);
    if (a->elems[t] < 1) return fail(ARMENV_EINVAL, "%s: elems[%d] = %lld must be >= 1", fn, t, (long long)a->elems[t]);
    T.t[t] = ExploitTensor{a->base[t], a->elems[t], (int32_t)blocks};
    blocks += (a->elems[t] - 1) / LRN_EXPLOIT_CHUNK + 1;
    if (blocks > INT32_MAX) return fail(ARMENV_EINVAL, "%s: elems[0..%d] need more than %d blocks", fn, t, INT32_MAX);
  }
  T.n = a->tensors;
  ExploitSources S{};
  bool identity = true;
  for (int p = 0; p < a->members; ++p) {
    const int32_t s = a->src[p];
    if (s < 0 || s >= a->members) return fail(ARMENV_EINVAL, "%s: src[%d] = %d outside 0..%d", fn, p, (int)s, (int)a->members - 1);
    S.v[p] = s;
    identity = identity && s == p;
  }
  // a source must keep itself: no block of the launch then reads what another block writes
  for (int p = 0; p < a->members; ++p)
    if (a->src[a->src[p]] != a->src[p])
      return fail(ARMENV_EINVAL, "%s: src[%d] = %d is itself replaced (src[%d] = %d)", fn, p, (int)a->src[p], (int)a->src[p],
                  (int)a->src[a->src[p]]);
  if (identity) return ARMENV_OK;

  DeviceGuard guard_(a->device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", fn, (int)a->device);
  hipLaunchKernelGGL(pop_exploit_kernel, dim3((unsigned)blocks, (unsigned)a->members), dim3(256), 0, static_cast<hipStream_t>(stream), T, S);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

}  // extern "C"
