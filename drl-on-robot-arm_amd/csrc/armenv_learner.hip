// armenv_learner.hip -- armenv_td3_update / armenv_td3_workspace_bytes, armenv_daddpg_update / armenv_daddpg_workspace_bytes and
// armenv_datd3_update / armenv_datd3_workspace_bytes (include/armenv.h): argument checks, workspace layouts and the launch sequences
// of the fused TD3, DADDPG and DATD3 / DARC updates over the kernels of armenv_learner.h.
//
// TD3 launches (B rows, H = 256, D = state_dim, K1 = D + 3); every stage is one launch over all its independent problems:
//   1 gemm    layer 1: target actor (s2), critic Q1 and Q2 (cat(s, a)), actor (s) when with_actor
//   2 gemm    layer 2 of the same nets
//   3 head    target actor's fc3 + noise -> a2; actor's fc3 -> a = actor(s) (the actor pass's forward needs no critic)
//   4 gemm    layer 1 of the target twin critic over cat(s2, a2)
//   5 gemm    layer 2 of the target twin critic
//   6 head    target, both critics' fc3, loss rows, d3 and d2 = (d3 W3) relu'(h2)
//   7 gemm    d1 = (d2 W2) relu'(h1); dW3 | db3 and dW2 | db2 partials of both heads
//   8 gemm    dW1 | db1 partials of both heads
//   9 adam    critic (12 tensors) + the loss; with_actor: the target critic's soft update (the critic is final by then)
// with_actor:
//  10 gemm    Q1 layer 1 over cat(s, a) with the stepped critic
//  11 gemm    Q1 layer 2 with its epilogue producing the delta of -mean(Q1): (-1/B) W3 relu'(.)
//  12 gemm    dc1 = (dc2 W2) relu'(c1)
//  13 head    back through cat -> tanh -> the actor's fc3: du, da2
//  14 gemm    da1 = (da2 W2a) relu'(h1a); dW3a | db3a and dW2a | db2a partials
//  15 gemm    dW1a | db1a partials
//  16 adam    actor (6 tensors) + the target actor's soft update
//
// DADDPG launches (two actors, ONE critic; actor k = update_actor is stepped), always 16:
//   1 gemm    layer 1: target actors 1 and 2 (s2), critic (cat(s, a)), actor k (s)
//   2 gemm    layer 2 of the same nets
//   3 head    target actors' fc3 -> a2_1, a2_2 (no noise, no clamp); actor k's fc3 -> a = actor_k(s) and its tanh
//   4 gemm    layer 1 of the target critic over cat(s2, a2_1) and cat(s2, a2_2)
//   5 gemm    layer 2 of the same two problems
//   6 head    target = r + (1 - d) gamma min(tq1, tq2), the critic's fc3, loss rows, d3 and d2 = (d3 W3) relu'(h2)
//   7 gemm    d1 = (d2 W2) relu'(h1); dW3 | db3 and dW2 | db2 partials
//   8 gemm    dW1 | db1 partials
//   9 adam    critic (6 tensors) + the loss; update_actor == 2: the target critic's soft update (the critic is final by then)
//  10-16      as TD3's 10-16 with the ONE critic in Q1's place and actor k in the actor's; 16 soft-updates target actor k only
//
// DATD3 / DARC launches (two actors, TWO critics; critic k and actor k = update_actor are stepped, `other` = 3 - k), always 16:
//   1 gemm    layer 1: target actors 1 and 2 (s2), critic k (cat(s, a)), actor k (s); darc: critic `other` (cat(s, a)) as a fifth problem
//   2 gemm    layer 2 of the same nets
//   3 head    target actors' fc3 + ONE noise draw per row, clamped -> a2_1, a2_2; actor k's fc3 -> a = actor_k(s) and its tanh
//   4 gemm    layer 1 of target critic 1 over cat(s2, a2_1) and of target critic 2 over cat(s2, a2_2)
//   5 gemm    layer 2 of the same two problems
//   6 head    T = min(tq1, tq2) (darc: q_weight T + (1 - q_weight) T), target = r + (1 - d) gamma T, critic k's fc3 (darc: and the
//             other's), loss row(s), d3 = 2/B (q - target) (darc: + 2 w/B (q - q_other)) and d2 = (d3 W3) relu'(h2)
//   7 gemm    d1 = (d2 W2) relu'(h1); dW3 | db3 and dW2 | db2 partials of critic k
//   8 gemm    dW1 | db1 partials
//   9 adam    critic k (6 tensors) + the loss + target critic k's soft update (critic k is final by then; the actor's loss does not
//             read the target)
//  10-16      as DADDPG's 10-16 with critic k in the critic's place; 16 soft-updates target actor k
// The other critic is read (darc) and never written; DATD3 has no fifth problem and takes its target from T itself.
#include <cmath>

#include "armenv_engine.h"
#include "armenv_learner.h"

using namespace armenv::learner;

namespace {

// workspace layout in floats; every region starts on a 64-float (256-byte) boundary
struct Ws {
  int64_t B, S;                                     // S = number of weight-gradient partials
  int64_t ta1, ta2, tq1[2], tq2[2], h1[2], h2[2], d2[2], d1[2], ah1, ah2;    // [B][H] each
  int64_t a2, api, tanh_a, du, d3[2], loss_rows;
  int64_t pW3[2], pW2[2], pW1[2];                    // critic partials [S][rows][ld]
  int64_t pa3, pa2, pa1;                             // actor partials (reuse the critic's region)
  int64_t split_stride;                              // floats per partial slice
  int64_t total;
};

constexpr int kW1Ld = 16;   // row length of a W1 | b1 partial: state_dim + 3 + 1 <= 16

int64_t up64(int64_t x) { return (x + 63) & ~(int64_t)63; }

Ws layout(int D, int64_t B) {
  Ws w{};
  w.B = B;
  w.S = (B + LRN_KSPLIT - 1) / LRN_KSPLIT;
  const int64_t H = LRN_H, BH = up64(B * H);
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t r = o; o += up64(n); return r; };
  (void)D;
  w.ta1 = take(BH); w.ta2 = take(BH);
  for (int i = 0; i < 2; ++i) { w.tq1[i] = take(BH); w.tq2[i] = take(BH); }
  for (int i = 0; i < 2; ++i) { w.h1[i] = take(BH); w.h2[i] = take(BH); w.d2[i] = take(BH); w.d1[i] = take(BH); }
  w.ah1 = take(BH); w.ah2 = take(BH);
  w.a2 = take(3 * B); w.api = take(3 * B); w.tanh_a = take(3 * B); w.du = take(3 * B);
  w.d3[0] = take(B); w.d3[1] = take(B); w.loss_rows = take(2 * B);
  // one partial slice: both critic heads' W3 | b3 [1][H+1], W2 | b2 [H][H+1], W1 | b1 [H][16]
  int64_t q = 0;
  auto sub = [&](int64_t n) { const int64_t r = q; q += up64(n); return r; };
  for (int i = 0; i < 2; ++i) { w.pW3[i] = sub(H + 1); w.pW2[i] = sub(H * (H + 1)); w.pW1[i] = sub(H * kW1Ld); }
  w.split_stride = q;
  // the actor's slice (3 (H+1) + H (H+1) + H 16 floats) fits in the critic's
  w.pa3 = 0; w.pa2 = up64(3 * (H + 1)); w.pa1 = w.pa2 + up64(H * (H + 1));
  const int64_t part = take(w.S * w.split_stride);
  for (int i = 0; i < 2; ++i) { w.pW3[i] += part; w.pW2[i] += part; w.pW1[i] += part; }
  w.pa3 += part; w.pa2 += part; w.pa1 += part;
  w.total = o;
  return w;
}

Feat feat(const float *p, int ld, int nf, int64_t rows, int aug = 0) { return Feat{p, p, ld, ld, nf, nf, aug, rows}; }
Feat feat2(const float *p0, int ld0, const float *p1, int ld1, int nf, int64_t rows, int aug = 0) {
  return Feat{p0, p1, ld0, ld1, ld0, nf, aug, rows};
}

struct Launcher {
  GemmList L{};
  int blocks = 0;
  void add(const Gemm &g0) {
    Gemm g = g0;
    g.tiles_m = (g.M + LRN_TM - 1) / LRN_TM;
    g.tiles_n = (g.N + LRN_TN - 1) / LRN_TN;
    g.splits = (int)((g.K + g.kchunk - 1) / g.kchunk);
    g.first_block = blocks;
    blocks += g.tiles_m * g.tiles_n * g.splits;
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

// Args: ArmEnvTd3Args, ArmEnvDaddpgArgs or ArmEnvDatd3Args (beta1, beta2, eps, tau)
template <class Args>
int launch_adam(AdamArgs &P, float lr, int64_t step, const Args *a, hipStream_t s) {
  P.beta1 = a->beta1; P.beta2 = a->beta2; P.eps = a->eps; P.tau = a->tau;
  const double bc1 = 1.0 - std::pow((double)a->beta1, (double)step), bc2 = 1.0 - std::pow((double)a->beta2, (double)step);
  P.step_size = (float)(lr / bc1);
  P.bc2_sqrt = (float)std::sqrt(bc2);
  const unsigned blocks = (unsigned)((P.total + 255) / 256) + (P.loss_rows ? 1u : 0u);
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

// hyper-parameters, the nets and moments, the batch buffers and the workspace (`need` bytes)
template <class Args, size_t NH, size_t NN>
int check_buffers(const char *fn, const Args *a, const NamedF (&hp)[NH], const NamedNet (&nets)[NN], int64_t need, const char *ws_fn) {
  for (const auto &h : hp)
    if (!std::isfinite(h.v) || !h.ok) return fail(ARMENV_EINVAL, "%s: %s = %g out of range", fn, h.name, (double)h.v);
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

// DADDPG's workspace layout in floats (64-float boundaries, as Ws)
struct WsD {
  int64_t B, S;
  int64_t ta1[2], ta2[2], tq1[2], tq2[2], h1, h2, d2, d1, ah1, ah2;   // [B][H] each; [2]: target actor / proposal 1 and 2
  int64_t a2[2], api, tanh_a, du, d3, loss_rows;
  int64_t pW3, pW2, pW1;                              // critic partials [S][rows][ld]
  int64_t pa3, pa2, pa1;                              // actor partials, in the same slices
  int64_t split_stride;
  int64_t total;
};

WsD daddpg_layout(int64_t B) {
  WsD w{};
  w.B = B;
  w.S = (B + LRN_KSPLIT - 1) / LRN_KSPLIT;
  const int64_t H = LRN_H, BH = up64(B * H);
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t r = o; o += up64(n); return r; };
  for (int i = 0; i < 2; ++i) { w.ta1[i] = take(BH); w.ta2[i] = take(BH); w.tq1[i] = take(BH); w.tq2[i] = take(BH); }
  w.h1 = take(BH); w.h2 = take(BH); w.d2 = take(BH); w.d1 = take(BH); w.ah1 = take(BH); w.ah2 = take(BH);
  w.a2[0] = take(3 * B); w.a2[1] = take(3 * B); w.api = take(3 * B); w.tanh_a = take(3 * B); w.du = take(3 * B);
  w.d3 = take(B); w.loss_rows = take(B);
  // one partial slice holds the critic's W3 | b3 [1][H+1], W2 | b2 [H][H+1], W1 | b1 [H][16] OR the actor's W3 | b3 [3][H+1], ...:
  // the two never live at the same time (the critic's are consumed by its Adam launch before the actor's are written), and with ONE
  // critic the actor's slice is the larger -- the slice is the larger of the two
  int64_t qc = 0, qa = 0;
  auto sub = [](int64_t &q, int64_t n) { const int64_t r = q; q += up64(n); return r; };
  w.pW3 = sub(qc, H + 1); w.pW2 = sub(qc, H * (H + 1)); w.pW1 = sub(qc, H * kW1Ld);
  w.pa3 = sub(qa, 3 * (H + 1)); w.pa2 = sub(qa, H * (H + 1)); w.pa1 = sub(qa, H * kW1Ld);
  w.split_stride = qc > qa ? qc : qa;
  const int64_t part = take(w.S * w.split_stride);
  w.pW3 += part; w.pW2 += part; w.pW1 += part;
  w.pa3 += part; w.pa2 += part; w.pa1 += part;
  w.total = o;
  return w;
}

// DATD3 / DARC: DADDPG's layout (the same activations, deltas and actor-sized partial slices, for ONE stepped critic) followed by the
// other critic's two hidden layers and a two-column loss block, both written only when `darc`
struct WsT : WsD {
  int64_t oh1, oh2, loss2;
};

WsT datd3_layout(int64_t B) {
  WsT w{};
  static_cast<WsD &>(w) = daddpg_layout(B);
  int64_t o = w.total;
  auto take = [&](int64_t n) { const int64_t r = o; o += up64(n); return r; };
  w.oh1 = take(B * LRN_H); w.oh2 = take(B * LRN_H); w.loss2 = take(2 * B);
  w.total = o;
  return w;
}

}  // namespace

extern "C" {

int64_t armenv_td3_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch) {
  if (state_dim < 1 || state_dim > 12 || hidden_dim != LRN_H || batch < 1 || batch > kMaxBatch) return -1;
  return layout(state_dim, batch).total * (int64_t)sizeof(float);
}

int armenv_td3_update(const ArmEnvTd3Args *a, void *stream) {
  static const char *fn = "armenv_td3_update";
  LRN_TRY(check_sizes(fn, a));
  if (a->with_actor != 0 && a->with_actor != 1) return fail(ARMENV_EINVAL, "%s: with_actor must be 0 or 1", fn);
  if (a->critic_step < 1) return fail(ARMENV_EINVAL, "%s: critic_step must be >= 1", fn);
  if (a->with_actor && a->actor_step < 1) return fail(ARMENV_EINVAL, "%s: actor_step must be >= 1", fn);
  const NamedF hp[] = {
      {"action_bound", a->action_bound, a->action_bound > 0.f}, {"gamma", a->gamma, a->gamma >= 0.f && a->gamma <= 1.f},
      {"tau", a->tau, a->tau >= 0.f && a->tau <= 1.f}, {"policy_noise", a->policy_noise, a->policy_noise >= 0.f},
      {"noise_clip", a->noise_clip, a->noise_clip >= 0.f}, {"actor_lr", a->actor_lr, a->actor_lr >= 0.f},
      {"critic_lr", a->critic_lr, a->critic_lr >= 0.f}, {"beta1", a->beta1, a->beta1 >= 0.f && a->beta1 < 1.f},
      {"beta2", a->beta2, a->beta2 >= 0.f && a->beta2 < 1.f}, {"eps", a->eps, a->eps > 0.f}};
  const NamedNet nets[] = {
      {"actor", &a->actor}, {"q1", &a->q1}, {"q2", &a->q2}, {"target_actor", &a->target_actor}, {"target_q1", &a->target_q1},
      {"target_q2", &a->target_q2}, {"actor_m", &a->actor_m}, {"actor_v", &a->actor_v}, {"q1_m", &a->q1_m}, {"q1_v", &a->q1_v},
      {"q2_m", &a->q2_m}, {"q2_v", &a->q2_v}};
  LRN_TRY(check_buffers(fn, a, hp, nets, armenv_td3_workspace_bytes(a->state_dim, a->hidden_dim, a->batch), "armenv_td3_workspace_bytes"));

  DeviceGuard guard_(a->device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", fn, (int)a->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int D = a->state_dim, K1 = D + LRN_A, H = LRN_H;
  const int64_t B = a->batch;
  const Ws w = layout(D, B);
  float *ws = static_cast<float *>(a->workspace_dev);
  const ArmEnvMlpRW *Q[2] = {&a->q1, &a->q2}, *TQ[2] = {&a->target_q1, &a->target_q2};
  const Feat s_only = feat(a->states_dev, D, D, B);
  const Feat sa = feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B);
  Launcher L;

  // 1-2: layers 1 and 2 of the target actor, both critic heads and (with_actor) the actor
  L.forward(feat(a->next_states_dev, D, D, B), D, a->target_actor.W1, a->target_actor.b1, ws + w.ta1, B);
  for (int i = 0; i < 2; ++i) L.forward(sa, K1, Q[i]->W1, Q[i]->b1, ws + w.h1[i], B);
  if (a->with_actor) L.forward(s_only, D, a->actor.W1, a->actor.b1, ws + w.ah1, B);
  LRN_TRY(L.launch(s));
  L.forward(feat(ws + w.ta1, H, H, B), H, a->target_actor.W2, a->target_actor.b2, ws + w.ta2, B);
  for (int i = 0; i < 2; ++i) L.forward(feat(ws + w.h1[i], H, H, B), H, Q[i]->W2, Q[i]->b2, ws + w.h2[i], B);
  if (a->with_actor) L.forward(feat(ws + w.ah1, H, H, B), H, a->actor.W2, a->actor.b2, ws + w.ah2, B);
  LRN_TRY(L.launch(s));

  // 3: the actors' heads
  ActorHeadArgs ah{};
  ah.B = B; ah.t_h2 = ws + w.ta2; ah.t_W3 = a->target_actor.W3; ah.t_b3 = a->target_actor.b3; ah.noise = a->noise_dev;
  ah.seed = a->seed; ah.draw = a->draw; ah.bound = a->action_bound; ah.policy_noise = a->policy_noise; ah.noise_clip = a->noise_clip;
  ah.a2 = ws + w.a2; ah.with_actor = a->with_actor; ah.h2 = ws + w.ah2; ah.W3 = a->actor.W3; ah.b3 = a->actor.b3;
  ah.a = ws + w.api; ah.tanh_out = ws + w.tanh_a;
  const unsigned row_blocks = grid_for(B, 4);
  hipLaunchKernelGGL(actor_head_kernel, dim3(row_blocks * (a->with_actor ? 2u : 1u)), dim3(256), 0, s, ah);
  HIP_TRY(hipGetLastError());

  // 4-5: target twin critic over cat(s2, a2)
  const Feat s2a2 = feat2(a->next_states_dev, D, ws + w.a2, LRN_A, K1, B);
  for (int i = 0; i < 2; ++i) L.forward(s2a2, K1, TQ[i]->W1, TQ[i]->b1, ws + w.tq1[i], B);
  LRN_TRY(L.launch(s));
  for (int i = 0; i < 2; ++i) L.forward(feat(ws + w.tq1[i], H, H, B), H, TQ[i]->W2, TQ[i]->b2, ws + w.tq2[i], B);
  LRN_TRY(L.launch(s));

  // 6: target, loss rows, critic deltas
  CriticHeadArgs ch{};
  ch.B = B; ch.gamma = a->gamma; ch.inv_b = 1.0f / (float)B; ch.rewards = a->rewards_dev; ch.dones = a->dones_dev;
  for (int i = 0; i < 2; ++i) {
    ch.t_h2[i] = ws + w.tq2[i]; ch.t_W3[i] = TQ[i]->W3; ch.t_b3[i] = TQ[i]->b3;
    ch.h2[i] = ws + w.h2[i]; ch.W3[i] = Q[i]->W3; ch.b3[i] = Q[i]->b3;
    ch.d3[i] = ws + w.d3[i]; ch.d2[i] = ws + w.d2[i];
  }
  ch.loss_rows = ws + w.loss_rows;
  hipLaunchKernelGGL(critic_head_kernel, dim3(row_blocks), dim3(256), 0, s, ch);
  HIP_TRY(hipGetLastError());

  // 7-8: critic backward and weight-gradient partials
  for (int i = 0; i < 2; ++i) {
    L.backward(ws + w.d2[i], Q[i]->W2, ws + w.h1[i], ws + w.d1[i], B);
    L.wgrad(ws + w.d3[i], 1, feat(ws + w.h2[i], H, H, B, 1), H, ws + w.pW3[i], H + 1, B, w.split_stride);
    L.wgrad(ws + w.d2[i], H, feat(ws + w.h1[i], H, H, B, 1), H, ws + w.pW2[i], H + 1, B, w.split_stride);
  }
  LRN_TRY(L.launch(s));
  const Feat sa_aug = feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B, 1);
  for (int i = 0; i < 2; ++i) L.wgrad(ws + w.d1[i], H, sa_aug, K1, ws + w.pW1[i], kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 9: critic Adam (+ loss, + the target critic's soft update on actor steps)
  {
    AdamArgs P{};
    for (int i = 0; i < 2; ++i)
      adam_tensors(P, *Q[i], i ? a->q2_m : a->q1_m, i ? a->q2_v : a->q1_v, *TQ[i], K1, 1, ws + w.pW1[i], ws + w.pW2[i], ws + w.pW3[i]);
    P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = a->with_actor;
    P.loss_rows = ws + w.loss_rows; P.loss_cols = 2; P.loss_w1 = 1.0f; P.B = B; P.inv_b = 1.0f / (float)B; P.loss = a->loss_dev;
    LRN_TRY(launch_adam(P, a->critic_lr, a->critic_step, a, s));
  }
  if (!a->with_actor) return ARMENV_OK;

  // 10-12: Q1(s, actor(s)) with the stepped critic and its backward to Q1's input; c1 / dc2 / dc1 reuse the target path's buffers
  float *c1 = ws + w.ta1, *dc2 = ws + w.ta2, *dc1 = ws + w.tq1[0], *da2 = ws + w.tq1[1], *da1 = ws + w.tq2[0];
  L.forward(feat2(a->states_dev, D, ws + w.api, LRN_A, K1, B), K1, a->q1.W1, a->q1.b1, c1, B);
  LRN_TRY(L.launch(s));
  L.forward(feat(c1, H, H, B), H, a->q1.W2, a->q1.b2, dc2, B, EPI_DRELU_W, a->q1.W3, -1.0f / (float)B);
  LRN_TRY(L.launch(s));
  L.backward(dc2, a->q1.W2, c1, dc1, B);
  LRN_TRY(L.launch(s));

  // 13: through cat -> tanh -> the actor's fc3
  ActorBackArgs ab{};
  ab.B = B; ab.in_dim = K1; ab.state_dim = D; ab.bound = a->action_bound; ab.dc1 = dc1; ab.Wq1 = a->q1.W1;
  ab.tanh_a = ws + w.tanh_a; ab.h2 = ws + w.ah2; ab.W3 = a->actor.W3; ab.du = ws + w.du; ab.da2 = da2;
  hipLaunchKernelGGL(actor_back_kernel, dim3(row_blocks), dim3(256), 0, s, ab);
  HIP_TRY(hipGetLastError());

  // 14-15: actor backward and weight-gradient partials
  L.backward(da2, a->actor.W2, ws + w.ah1, da1, B);
  L.wgrad(ws + w.du, LRN_A, feat(ws + w.ah2, H, H, B, 1), H, ws + w.pa3, H + 1, B, w.split_stride);
  L.wgrad(da2, H, feat(ws + w.ah1, H, H, B, 1), H, ws + w.pa2, H + 1, B, w.split_stride);
  LRN_TRY(L.launch(s));
  L.wgrad(da1, H, feat(a->states_dev, D, D, B, 1), D, ws + w.pa1, kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 16: actor Adam + the target actor's soft update
  AdamArgs P{};
  adam_tensors(P, a->actor, a->actor_m, a->actor_v, a->target_actor, D, LRN_A, ws + w.pa1, ws + w.pa2, ws + w.pa3);
  P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = 1;
  return launch_adam(P, a->actor_lr, a->actor_step, a, s);
}

int64_t armenv_daddpg_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch) {
  if (state_dim < 1 || state_dim > 12 || hidden_dim != LRN_H || batch < 1 || batch > kMaxBatch) return -1;
  return daddpg_layout(batch).total * (int64_t)sizeof(float);
}

int armenv_daddpg_update(const ArmEnvDaddpgArgs *a, void *stream) {
  static const char *fn = "armenv_daddpg_update";
  LRN_TRY(check_sizes(fn, a));
  if (a->update_actor != 1 && a->update_actor != 2) return fail(ARMENV_EINVAL, "%s: update_actor %d must be 1 or 2", fn, a->update_actor);
  if (a->critic_step < 1) return fail(ARMENV_EINVAL, "%s: critic_step must be >= 1", fn);
  if (a->actor_step < 1) return fail(ARMENV_EINVAL, "%s: actor_step must be >= 1", fn);
  const NamedF hp[] = {
      {"action_bound", a->action_bound, a->action_bound > 0.f}, {"gamma", a->gamma, a->gamma >= 0.f && a->gamma <= 1.f},
      {"tau", a->tau, a->tau >= 0.f && a->tau <= 1.f}, {"actor_lr", a->actor_lr, a->actor_lr >= 0.f},
      {"critic_lr", a->critic_lr, a->critic_lr >= 0.f}, {"beta1", a->beta1, a->beta1 >= 0.f && a->beta1 < 1.f},
      {"beta2", a->beta2, a->beta2 >= 0.f && a->beta2 < 1.f}, {"eps", a->eps, a->eps > 0.f}};
  const NamedNet nets[] = {
      {"actor1", &a->actor1}, {"actor2", &a->actor2}, {"critic", &a->critic}, {"target_actor1", &a->target_actor1},
      {"target_actor2", &a->target_actor2}, {"target_critic", &a->target_critic}, {"actor1_m", &a->actor1_m},
      {"actor1_v", &a->actor1_v}, {"actor2_m", &a->actor2_m}, {"actor2_v", &a->actor2_v}, {"critic_m", &a->critic_m},
      {"critic_v", &a->critic_v}};
  LRN_TRY(check_buffers(fn, a, hp, nets, armenv_daddpg_workspace_bytes(a->state_dim, a->hidden_dim, a->batch),
                        "armenv_daddpg_workspace_bytes"));

  DeviceGuard guard_(a->device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", fn, (int)a->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int D = a->state_dim, K1 = D + LRN_A, H = LRN_H;
  const int64_t B = a->batch;
  const WsD w = daddpg_layout(B);
  float *ws = static_cast<float *>(a->workspace_dev);
  const bool second = a->update_actor == 2;
  const ArmEnvMlpRW &Q = a->critic, &TQ = a->target_critic;
  const ArmEnvMlpRW &act = second ? a->actor2 : a->actor1, &t_act = second ? a->target_actor2 : a->target_actor1;
  const ArmEnvMlpRW *TA[2] = {&a->target_actor1, &a->target_actor2};
  const Feat s2_only = feat(a->next_states_dev, D, D, B);
  Launcher L;

  // 1-2: layers 1 and 2 of both target actors, the critic and actor k
  for (int i = 0; i < 2; ++i) L.forward(s2_only, D, TA[i]->W1, TA[i]->b1, ws + w.ta1[i], B);
  L.forward(feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B), K1, Q.W1, Q.b1, ws + w.h1, B);
  L.forward(feat(a->states_dev, D, D, B), D, act.W1, act.b1, ws + w.ah1, B);
  LRN_TRY(L.launch(s));
  for (int i = 0; i < 2; ++i) L.forward(feat(ws + w.ta1[i], H, H, B), H, TA[i]->W2, TA[i]->b2, ws + w.ta2[i], B);
  L.forward(feat(ws + w.h1, H, H, B), H, Q.W2, Q.b2, ws + w.h2, B);
  L.forward(feat(ws + w.ah1, H, H, B), H, act.W2, act.b2, ws + w.ah2, B);
  LRN_TRY(L.launch(s));

  // 3: the three actor heads
  DaddpgActorHeadArgs ah{};
  ah.B = B; ah.bound = a->action_bound;
  for (int i = 0; i < 2; ++i) { ah.h2[i] = ws + w.ta2[i]; ah.W3[i] = TA[i]->W3; ah.b3[i] = TA[i]->b3; ah.a[i] = ws + w.a2[i]; }
  ah.h2[2] = ws + w.ah2; ah.W3[2] = act.W3; ah.b3[2] = act.b3; ah.a[2] = ws + w.api; ah.tanh_out = ws + w.tanh_a;
  const unsigned row_blocks = grid_for(B, 4);
  hipLaunchKernelGGL(daddpg_actor_head_kernel, dim3(row_blocks * 3u), dim3(256), 0, s, ah);
  HIP_TRY(hipGetLastError());

  // 4-5: the ONE target critic over both proposals
  for (int i = 0; i < 2; ++i) L.forward(feat2(a->next_states_dev, D, ws + w.a2[i], LRN_A, K1, B), K1, TQ.W1, TQ.b1, ws + w.tq1[i], B);
  LRN_TRY(L.launch(s));
  for (int i = 0; i < 2; ++i) L.forward(feat(ws + w.tq1[i], H, H, B), H, TQ.W2, TQ.b2, ws + w.tq2[i], B);
  LRN_TRY(L.launch(s));

  // 6: target, loss rows, critic deltas
  DaddpgCriticHeadArgs ch{};
  ch.B = B; ch.gamma = a->gamma; ch.inv_b = 1.0f / (float)B; ch.rewards = a->rewards_dev; ch.dones = a->dones_dev;
  ch.t_h2[0] = ws + w.tq2[0]; ch.t_h2[1] = ws + w.tq2[1]; ch.t_W3 = TQ.W3; ch.t_b3 = TQ.b3;
  ch.h2 = ws + w.h2; ch.W3 = Q.W3; ch.b3 = Q.b3; ch.d3 = ws + w.d3; ch.d2 = ws + w.d2; ch.loss_rows = ws + w.loss_rows;
  hipLaunchKernelGGL(daddpg_critic_head_kernel, dim3(row_blocks), dim3(256), 0, s, ch);
  HIP_TRY(hipGetLastError());

  // 7-8: critic backward and weight-gradient partials
  L.backward(ws + w.d2, Q.W2, ws + w.h1, ws + w.d1, B);
  L.wgrad(ws + w.d3, 1, feat(ws + w.h2, H, H, B, 1), H, ws + w.pW3, H + 1, B, w.split_stride);
  L.wgrad(ws + w.d2, H, feat(ws + w.h1, H, H, B, 1), H, ws + w.pW2, H + 1, B, w.split_stride);
  LRN_TRY(L.launch(s));
  L.wgrad(ws + w.d1, H, feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B, 1), K1, ws + w.pW1, kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 9: critic Adam (+ loss, + the target critic's soft update when actor 2 is stepped)
  {
    AdamArgs P{};
    adam_tensors(P, Q, a->critic_m, a->critic_v, TQ, K1, 1, ws + w.pW1, ws + w.pW2, ws + w.pW3);
    P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = second;
    P.loss_rows = ws + w.loss_rows; P.loss_cols = 1; P.B = B; P.inv_b = 1.0f / (float)B; P.loss = a->loss_dev;
    LRN_TRY(launch_adam(P, a->critic_lr, a->critic_step, a, s));
  }

  // 10-12: critic(s, actor_k(s)) with the stepped critic and its backward to the critic's input; c1 / dc2 / dc1 / da2 / da1 reuse
  // the target path's buffers
  float *c1 = ws + w.ta1[0], *dc2 = ws + w.ta2[0], *dc1 = ws + w.tq1[0], *da2 = ws + w.tq1[1], *da1 = ws + w.tq2[0];
  L.forward(feat2(a->states_dev, D, ws + w.api, LRN_A, K1, B), K1, Q.W1, Q.b1, c1, B);
  LRN_TRY(L.launch(s));
  L.forward(feat(c1, H, H, B), H, Q.W2, Q.b2, dc2, B, EPI_DRELU_W, Q.W3, -1.0f / (float)B);
  LRN_TRY(L.launch(s));
  L.backward(dc2, Q.W2, c1, dc1, B);
  LRN_TRY(L.launch(s));

  // 13: through cat -> tanh -> actor k's fc3
  ActorBackArgs ab{};
  ab.B = B; ab.in_dim = K1; ab.state_dim = D; ab.bound = a->action_bound; ab.dc1 = dc1; ab.Wq1 = Q.W1;
  ab.tanh_a = ws + w.tanh_a; ab.h2 = ws + w.ah2; ab.W3 = act.W3; ab.du = ws + w.du; ab.da2 = da2;
  hipLaunchKernelGGL(actor_back_kernel, dim3(row_blocks), dim3(256), 0, s, ab);
  HIP_TRY(hipGetLastError());

  // 14-15: actor k's backward and weight-gradient partials (the critic's partials are consumed: same slices)
  L.backward(da2, act.W2, ws + w.ah1, da1, B);
  L.wgrad(ws + w.du, LRN_A, feat(ws + w.ah2, H, H, B, 1), H, ws + w.pa3, H + 1, B, w.split_stride);
  L.wgrad(da2, H, feat(ws + w.ah1, H, H, B, 1), H, ws + w.pa2, H + 1, B, w.split_stride);
  LRN_TRY(L.launch(s));
  L.wgrad(da1, H, feat(a->states_dev, D, D, B, 1), D, ws + w.pa1, kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 16: actor k's Adam + its target's soft update
  AdamArgs P{};
  adam_tensors(P, act, second ? a->actor2_m : a->actor1_m, second ? a->actor2_v : a->actor1_v, t_act, D, LRN_A, ws + w.pa1, ws + w.pa2,
               ws + w.pa3);
  P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = 1;
  return launch_adam(P, a->actor_lr, a->actor_step, a, s);
}

int64_t armenv_datd3_workspace_bytes(int32_t state_dim, int32_t hidden_dim, int64_t batch) {
  if (state_dim < 1 || state_dim > 12 || hidden_dim != LRN_H || batch < 1 || batch > kMaxBatch) return -1;
  return datd3_layout(batch).total * (int64_t)sizeof(float);
}

int armenv_datd3_update(const ArmEnvDatd3Args *a, void *stream) {
  static const char *fn = "armenv_datd3_update";
  LRN_TRY(check_sizes(fn, a));
  if (a->update_actor != 1 && a->update_actor != 2) return fail(ARMENV_EINVAL, "%s: update_actor %d must be 1 or 2", fn, a->update_actor);
  if (a->darc != 0 && a->darc != 1) return fail(ARMENV_EINVAL, "%s: darc %d must be 0 or 1", fn, a->darc);
  if (a->critic_step < 1) return fail(ARMENV_EINVAL, "%s: critic_step must be >= 1", fn);
  if (a->actor_step < 1) return fail(ARMENV_EINVAL, "%s: actor_step must be >= 1", fn);
  const bool darc = a->darc == 1;
  // q_weight and regularization_weight are read only when darc
  const NamedF hp[] = {
      {"action_bound", a->action_bound, a->action_bound > 0.f}, {"gamma", a->gamma, a->gamma >= 0.f && a->gamma <= 1.f},
      {"tau", a->tau, a->tau >= 0.f && a->tau <= 1.f}, {"policy_noise", a->policy_noise, a->policy_noise >= 0.f},
      {"noise_clip", a->noise_clip, a->noise_clip >= 0.f}, {"actor_lr", a->actor_lr, a->actor_lr >= 0.f},
      {"critic_lr", a->critic_lr, a->critic_lr >= 0.f}, {"beta1", a->beta1, a->beta1 >= 0.f && a->beta1 < 1.f},
      {"beta2", a->beta2, a->beta2 >= 0.f && a->beta2 < 1.f}, {"eps", a->eps, a->eps > 0.f},
      {"q_weight", darc ? a->q_weight : 0.f, !darc || (a->q_weight >= 0.f && a->q_weight <= 1.f)},
      {"regularization_weight", darc ? a->regularization_weight : 0.f, !darc || a->regularization_weight >= 0.f}};
  const NamedNet nets[] = {
      {"actor1", &a->actor1}, {"actor2", &a->actor2}, {"critic1", &a->critic1}, {"critic2", &a->critic2},
      {"target_actor1", &a->target_actor1}, {"target_actor2", &a->target_actor2}, {"target_critic1", &a->target_critic1},
      {"target_critic2", &a->target_critic2}, {"actor1_m", &a->actor1_m}, {"actor1_v", &a->actor1_v}, {"actor2_m", &a->actor2_m},
      {"actor2_v", &a->actor2_v}, {"critic1_m", &a->critic1_m}, {"critic1_v", &a->critic1_v}, {"critic2_m", &a->critic2_m},
      {"critic2_v", &a->critic2_v}};
  LRN_TRY(check_buffers(fn, a, hp, nets, armenv_datd3_workspace_bytes(a->state_dim, a->hidden_dim, a->batch),
                        "armenv_datd3_workspace_bytes"));

  DeviceGuard guard_(a->device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", fn, (int)a->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int D = a->state_dim, K1 = D + LRN_A, H = LRN_H;
  const int64_t B = a->batch;
  const WsT w = datd3_layout(B);
  float *ws = static_cast<float *>(a->workspace_dev);
  const bool second = a->update_actor == 2;
  const ArmEnvMlpRW &Q = second ? a->critic2 : a->critic1, &TQk = second ? a->target_critic2 : a->target_critic1;
  const ArmEnvMlpRW &Qo = second ? a->critic1 : a->critic2;     // read only (darc)
  const ArmEnvMlpRW &act = second ? a->actor2 : a->actor1, &t_act = second ? a->target_actor2 : a->target_actor1;
  const ArmEnvMlpRW *TA[2] = {&a->target_actor1, &a->target_actor2}, *TQ[2] = {&a->target_critic1, &a->target_critic2};
  const Feat s2_only = feat(a->next_states_dev, D, D, B);
  const Feat sa = feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B);
  Launcher L;

  // 1-2: layers 1 and 2 of both target actors, critic k, actor k and (darc) the other critic
  for (int i = 0; i < 2; ++i) L.forward(s2_only, D, TA[i]->W1, TA[i]->b1, ws + w.ta1[i], B);
  L.forward(sa, K1, Q.W1, Q.b1, ws + w.h1, B);
  L.forward(feat(a->states_dev, D, D, B), D, act.W1, act.b1, ws + w.ah1, B);
  if (darc) L.forward(sa, K1, Qo.W1, Qo.b1, ws + w.oh1, B);
  LRN_TRY(L.launch(s));
  for (int i = 0; i < 2; ++i) L.forward(feat(ws + w.ta1[i], H, H, B), H, TA[i]->W2, TA[i]->b2, ws + w.ta2[i], B);
  L.forward(feat(ws + w.h1, H, H, B), H, Q.W2, Q.b2, ws + w.h2, B);
  L.forward(feat(ws + w.ah1, H, H, B), H, act.W2, act.b2, ws + w.ah2, B);
  if (darc) L.forward(feat(ws + w.oh1, H, H, B), H, Qo.W2, Qo.b2, ws + w.oh2, B);
  LRN_TRY(L.launch(s));

  // 3: both noisy clamped proposals and actor k's action
  Datd3ActorHeadArgs ah{};
  ah.B = B; ah.bound = a->action_bound; ah.policy_noise = a->policy_noise; ah.noise_clip = a->noise_clip;
  ah.noise = a->noise_dev; ah.seed = a->seed; ah.draw = a->draw;
  for (int i = 0; i < 2; ++i) { ah.t_h2[i] = ws + w.ta2[i]; ah.t_W3[i] = TA[i]->W3; ah.t_b3[i] = TA[i]->b3; ah.a2[i] = ws + w.a2[i]; }
  ah.h2 = ws + w.ah2; ah.W3 = act.W3; ah.b3 = act.b3; ah.a = ws + w.api; ah.tanh_out = ws + w.tanh_a;
  const unsigned row_blocks = grid_for(B, 4);
  hipLaunchKernelGGL(datd3_actor_head_kernel, dim3(row_blocks * 2u), dim3(256), 0, s, ah);
  HIP_TRY(hipGetLastError());

  // 4-5: target critic j over its own actor's proposal
  for (int i = 0; i < 2; ++i) L.forward(feat2(a->next_states_dev, D, ws + w.a2[i], LRN_A, K1, B), K1, TQ[i]->W1, TQ[i]->b1, ws + w.tq1[i], B);
  LRN_TRY(L.launch(s));
  for (int i = 0; i < 2; ++i) L.forward(feat(ws + w.tq1[i], H, H, B), H, TQ[i]->W2, TQ[i]->b2, ws + w.tq2[i], B);
  LRN_TRY(L.launch(s));

  // 6: target, loss rows, critic k's deltas
  float *loss_rows = ws + (darc ? w.loss2 : w.loss_rows);
  Datd3CriticHeadArgs ch{};
  ch.B = B; ch.gamma = a->gamma; ch.inv_b = 1.0f / (float)B; ch.rewards = a->rewards_dev; ch.dones = a->dones_dev;
  ch.darc = a->darc;
  if (darc) {
    ch.w_min = a->q_weight; ch.w_max = (float)(1.0 - (double)a->q_weight); ch.reg = a->regularization_weight;
    ch.o_h2 = ws + w.oh2; ch.o_W3 = Qo.W3; ch.o_b3 = Qo.b3;
  }
  for (int i = 0; i < 2; ++i) { ch.t_h2[i] = ws + w.tq2[i]; ch.t_W3[i] = TQ[i]->W3; ch.t_b3[i] = TQ[i]->b3; }
  ch.h2 = ws + w.h2; ch.W3 = Q.W3; ch.b3 = Q.b3; ch.d3 = ws + w.d3; ch.d2 = ws + w.d2; ch.loss_rows = loss_rows;
  hipLaunchKernelGGL(datd3_critic_head_kernel, dim3(row_blocks), dim3(256), 0, s, ch);
  HIP_TRY(hipGetLastError());

  // 7-8: critic k's backward and weight-gradient partials
  L.backward(ws + w.d2, Q.W2, ws + w.h1, ws + w.d1, B);
  L.wgrad(ws + w.d3, 1, feat(ws + w.h2, H, H, B, 1), H, ws + w.pW3, H + 1, B, w.split_stride);
  L.wgrad(ws + w.d2, H, feat(ws + w.h1, H, H, B, 1), H, ws + w.pW2, H + 1, B, w.split_stride);
  LRN_TRY(L.launch(s));
  L.wgrad(ws + w.d1, H, feat2(a->states_dev, D, a->actions_dev, LRN_A, K1, B, 1), K1, ws + w.pW1, kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 9: critic k's Adam + the loss + target critic k's soft update
  {
    AdamArgs P{};
    adam_tensors(P, Q, second ? a->critic2_m : a->critic1_m, second ? a->critic2_v : a->critic1_v, TQk, K1, 1, ws + w.pW1, ws + w.pW2,
                 ws + w.pW3);
    P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = 1;
    P.loss_rows = loss_rows; P.loss_cols = darc ? 2 : 1; P.loss_w1 = darc ? a->regularization_weight : 0.f;
    P.B = B; P.inv_b = 1.0f / (float)B; P.loss = a->loss_dev;
    LRN_TRY(launch_adam(P, a->critic_lr, a->critic_step, a, s));
  }

  // 10-12: critic_k(s, actor_k(s)) with the stepped critic and its backward to the critic's input; c1 / dc2 / dc1 / da2 / da1 reuse
  // the target path's buffers
  float *c1 = ws + w.ta1[0], *dc2 = ws + w.ta2[0], *dc1 = ws + w.tq1[0], *da2 = ws + w.tq1[1], *da1 = ws + w.tq2[0];
  L.forward(feat2(a->states_dev, D, ws + w.api, LRN_A, K1, B), K1, Q.W1, Q.b1, c1, B);
  LRN_TRY(L.launch(s));
  L.forward(feat(c1, H, H, B), H, Q.W2, Q.b2, dc2, B, EPI_DRELU_W, Q.W3, -1.0f / (float)B);
  LRN_TRY(L.launch(s));
  L.backward(dc2, Q.W2, c1, dc1, B);
  LRN_TRY(L.launch(s));

  // 13: through cat -> tanh -> actor k's fc3
  ActorBackArgs ab{};
  ab.B = B; ab.in_dim = K1; ab.state_dim = D; ab.bound = a->action_bound; ab.dc1 = dc1; ab.Wq1 = Q.W1;
  ab.tanh_a = ws + w.tanh_a; ab.h2 = ws + w.ah2; ab.W3 = act.W3; ab.du = ws + w.du; ab.da2 = da2;
  hipLaunchKernelGGL(actor_back_kernel, dim3(row_blocks), dim3(256), 0, s, ab);
  HIP_TRY(hipGetLastError());

  // 14-15: actor k's backward and weight-gradient partials (the critic's partials are consumed: same slices)
  L.backward(da2, act.W2, ws + w.ah1, da1, B);
  L.wgrad(ws + w.du, LRN_A, feat(ws + w.ah2, H, H, B, 1), H, ws + w.pa3, H + 1, B, w.split_stride);
  L.wgrad(da2, H, feat(ws + w.ah1, H, H, B, 1), H, ws + w.pa2, H + 1, B, w.split_stride);
  LRN_TRY(L.launch(s));
  L.wgrad(da1, H, feat(a->states_dev, D, D, B, 1), D, ws + w.pa1, kW1Ld, B, w.split_stride);
  LRN_TRY(L.launch(s));

  // 16: actor k's Adam + its target's soft update
  AdamArgs P{};
  adam_tensors(P, act, second ? a->actor2_m : a->actor1_m, second ? a->actor2_v : a->actor1_v, t_act, D, LRN_A, ws + w.pa1, ws + w.pa2,
               ws + w.pa3);
  P.splits = (int)w.S; P.split_stride = w.split_stride; P.soft = 1;
  return launch_adam(P, a->actor_lr, a->actor_step, a, s);
}

}  // extern "C"
