// armenv_replay.h -- device-resident trajectory store indexing and the HER-"future" sampler, the immediate consumer of
// the step outputs.  Replaces the per-sample Python loops of
// /root/reference/utils/rl_utils.py:108-152 (ReplayBuffer_Trajectory_reach.sample) and :154-199 (..._push.sample)
// for rollout buffers that never leave HBM.
//
// Storage convention (what armenv_rollout writes, time-major):
//   obs0      f32 [N][D]      observation before step 0 of the chunk
//   obs_after f32 [T][N][D]   row t = observation returned by step t (after an auto-reset: the new episode's first obs)
//   next_obs  f32 [T][N][D]   row t = terminal_obs of step t = the true next state of the transition
//   action f32 [T][N][3], reward f32 [T][N], done u8 [T][N]
// A trajectory (rl_utils.py:91-105) is one episode of one env: states[0..L], actions/rewards/dones[0..L-1];
//   states[0]   = the observation before its first step   (obs0 or obs_after[t_start-1])
//   states[j>0] = next_obs[t_start + j - 1]
// Only complete episodes (start and terminating done inside the chunk) are indexed, as the reference only stores
// finished trajectories (main.py:129).
#pragma once
#include "armenv_math.h"

namespace armenv {

// pass 1: number of complete episodes per env column; pass 2 (write != nullptr): emit (env, t_start, length).
// `starts_at_reset`: the chunk began right after a reset of every env, so the first episode's start is inside it.
// The buffers may be a ring: logical step t lives in physical row (ring_base + t) % ring_cap (ring_cap >= T).
AE_DEV void index_episodes_column(int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap, const uint8_t *done,
                                  int32_t starts_at_reset, int32_t *counts, const int64_t *offsets, int32_t *episodes, int64_t n) {
  int32_t cnt = 0;
  int64_t start = starts_at_reset ? 0 : -1;
  int64_t w = episodes ? (offsets[n] - (int64_t)counts[n]) : 0;   // offsets = inclusive cumsum of counts
  for (int64_t t = 0; t < T; ++t) {
    if (done[((ring_base + t) % ring_cap) * N + n]) {
      if (start >= 0) {
        if (episodes) {
          int32_t *e = episodes + 3 * w;
          e[0] = (int32_t)n; e[1] = (int32_t)start; e[2] = (int32_t)(t - start + 1);
          ++w;
        }
        ++cnt;
      }
      start = t + 1;
    }
  }
  if (!episodes) counts[n] = cnt;
}

__global__ __launch_bounds__(256) void index_episodes_kernel(int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap,
                                                            const uint8_t *done, int32_t starts_at_reset,
                                                            int32_t *counts, const int64_t *offsets, int32_t *episodes) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  index_episodes_column(T, N, ring_base, ring_cap, done, starts_at_reset, counts, offsets, episodes, n);
}

// The population form: member blockIdx.y of P rings of one geometry, done u8 [P][ring_cap][N], counts i32 [P][N], offsets i64 [P][N]
// (the inclusive cumsum WITHIN each member), episodes i32 [P][episodes_stride][3].  One thread per (member, env column); a member's
// list is what index_episodes_kernel writes for that member's ring alone.
__global__ __launch_bounds__(256) void index_episodes_pop_kernel(int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap,
                                                                const uint8_t *done, int32_t starts_at_reset, int32_t *counts,
                                                                const int64_t *offsets, int32_t *episodes,
                                                                int32_t members, int64_t episodes_stride) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = blockIdx.y;
  if (n >= N || p >= members) return;
  index_episodes_column(T, N, ring_base, ring_cap, done + p * ring_cap * N, starts_at_reset, counts + p * N,
                        episodes ? offsets + p * N : nullptr, episodes ? episodes + p * episodes_stride * 3 : nullptr, n);
}

struct HerArgs {
  int64_t T, N, ring_base, ring_cap;
  int32_t D;                 // 6 reach, 9 push
  const float *obs0, *obs_after, *next_obs, *action, *reward;
  const uint8_t *done;
  const int32_t *episodes;   // [E][3]
  const int64_t *num_episodes;  // device scalar E
  int64_t B;
  const int32_t *picks_in;   // nullable [B][4] = (episode, step_state, use_her, step_goal): teacher-forced draws
  uint64_t seed, draw;
  int32_t use_her;
  double her_ratio, dis_threshold;   // the caller's doubles: the reference compares against Python floats
  float *states, *actions, *next_states, *rewards;
  uint8_t *dones;
  int32_t *picks_out;        // nullable
};

// row b of a batch with nothing to sample from: defined and inert (zeros, done = 1); the picks are the caller's to write
template <int D>
AE_DEV void her_inert_row(const HerArgs &A, int64_t b) {
  for (int k = 0; k < D; ++k) { A.states[b * D + k] = 0.f; A.next_states[b * D + k] = 0.f; }
  A.actions[3 * b] = A.actions[3 * b + 1] = A.actions[3 * b + 2] = 0.f;
  A.rewards[b] = 0.f;
  A.dones[b] = 1;
}

// Row b of a batch from the pick (episode, step_state, use_her, step_goal): the transition, gathered from A's rings through A's
// episode list and relabelled, written to row b of A's outputs.  The one gather of every sampler kernel; the picks are the caller's
// to write.
template <int D>
AE_DEV void her_row(const HerArgs &A, int64_t b, int32_t ep, int32_t st, int32_t her, int32_t sg) {
  const int32_t *e = A.episodes + 3 * ep;
  const int64_t n = e[0], t0 = e[1];
  auto row = [&](int64_t lt) { return (A.ring_base + lt) % A.ring_cap; };   // logical step -> physical row
  const int64_t t = row(t0 + st);                           // physical row of the transition
  auto state_ptr = [&](int64_t j) -> const float * {        // traj.states[j]
    const int64_t tt = t0 + j;                              // states[j] is the observation before logical step tt
    if (j == 0) return tt == 0 ? A.obs0 + n * D : A.obs_after + (row(tt - 1) * A.N + n) * D;
    return A.next_obs + (row(tt - 1) * A.N + n) * D;
  };
  const float *s = state_ptr(st), *s2 = state_ptr(st + 1);
  float sv[D], nv[D];
#pragma unroll
  for (int k = 0; k < D; ++k) { sv[k] = s[k]; nv[k] = s2[k]; }
  float r = A.reward[t * A.N + n];
  uint8_t dn = A.done[t * A.N + n];
  if (her) {
    const float *gsrc = state_ptr(sg);                      // goal = traj.states[step_goal][:3]   :136
    const float g0 = gsrc[0], g1 = gsrc[1], g2 = gsrc[2];
    bool far;
    if (D == 9) {   // push observations are float64 in the reference (rl_push_env.py:308): f64 arithmetic
      const double d0 = (double)nv[0] - (double)g0, d1 = (double)nv[1] - (double)g1, d2 = (double)nv[2] - (double)g2;
      far = ::sqrt((d0 * d0 + d1 * d1) + d2 * d2) > A.dis_threshold;
    } else {        // reach observations are float32: np.sqrt(np.sum(np.square(f32[3])))  :137
      const float d0 = nv[0] - g0, d1 = nv[1] - g1, d2 = nv[2] - g2;
      far = (double)sqrtf((d0 * d0 + d1 * d1) + d2 * d2) > A.dis_threshold;
    }
    r = far ? -0.1f : 1.0f;                                 // :138
    dn = far ? 0 : 1;                                       // :139
    if (D == 9) {                                           // push: state[6:10] kept from `state` for BOTH rows, :187-188
      nv[6] = sv[6]; nv[7] = sv[7]; nv[8] = sv[8];
    }
    sv[3] = g0; sv[4] = g1; sv[5] = g2;                     // :140-141 / :187-188
    nv[3] = g0; nv[4] = g1; nv[5] = g2;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) { A.states[b * D + k] = sv[k]; A.next_states[b * D + k] = nv[k]; }
  const float *a = A.action + (t * A.N + n) * 3;
  A.actions[3 * b] = a[0]; A.actions[3 * b + 1] = a[1]; A.actions[3 * b + 2] = a[2];
  A.rewards[b] = r;
  A.dones[b] = dn;
}

// The sampler's own Philox key: with the env's key, (batch slot b, draw d) would read exactly the uniforms that chose the goal of
// env b in episode d whenever a caller seeds both with the same number (armenv.train does)
constexpr uint64_t HER_KEY_XOR = 0x5DEECE66D1CE4E5Bull;

// (step_state, use_her, step_goal) of a pick inside an episode of L steps, from the uniforms u1..u3 of its row
AE_DEV void her_draw_steps(const HerArgs &A, int32_t L, double u1, double u2, double u3, int32_t &st, int32_t &her, int32_t &sg) {
  st = (int32_t)(u1 * (double)L);                           // np.random.randint(length)     rl_utils.py:127
  her = (A.use_her && u2 <= A.her_ratio) ? 1 : 0;           // np.random.uniform() <= ratio  :134
  sg = st + 1 + (int32_t)(u3 * (double)(L - st));           // randint(step+1, length+1)     :135
}

// sample b of the batch: the one body of her_sample_kernel and her_sample_pop_kernel
template <int D>
AE_DEV void her_sample_one(const HerArgs &A, int64_t b) {
  const int64_t E = *A.num_episodes;
  int32_t ep, st, her, sg;
  if (A.picks_in) {
    ep = A.picks_in[4 * b]; st = A.picks_in[4 * b + 1]; her = A.picks_in[4 * b + 2]; sg = A.picks_in[4 * b + 3];
  } else {
    if (E <= 0) {   // nothing to sample from: a defined, inert batch
      her_inert_row<D>(A, b);
      if (A.picks_out) { A.picks_out[4 * b] = -1; A.picks_out[4 * b + 1] = A.picks_out[4 * b + 2] = A.picks_out[4 * b + 3] = 0; }
      return;
    }
    double u0, u1, u2, u3;
    const uint64_t key = A.seed ^ HER_KEY_XOR;
    philox_pair(key, (uint64_t)b, (uint32_t)A.draw, 0u, u0, u1);
    philox_pair(key, (uint64_t)b, (uint32_t)A.draw, 1u, u2, u3);
    ep = (int32_t)(u0 * (double)E);                         // random.sample(buffer, 1)      rl_utils.py:126
    her_draw_steps(A, A.episodes[3 * ep + 2], u1, u2, u3, st, her, sg);
  }
  her_row<D>(A, b, ep, st, her, sg);
  if (A.picks_out) { A.picks_out[4 * b] = ep; A.picks_out[4 * b + 1] = st; A.picks_out[4 * b + 2] = her; A.picks_out[4 * b + 3] = sg; }
}

template <int D>
__global__ __launch_bounds__(256) void her_sample_kernel(HerArgs A) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= A.B) return;
  her_sample_one<D>(A, b);
}

// The population form: A is member 0's arguments, member p = blockIdx.y reads and writes the same arrays p x (one member's extent)
// further on (the rings [P][ring_cap][N][...], obs0 [P][N][D], episodes [P][episodes_stride][3], num_episodes [P], the outputs
// [P][B][...], the picks [P][B][4]) and draws with seed + p and the shared draw: member p's slices hold what her_sample_kernel
// leaves when it is given member p's arrays.
template <int D>
__global__ __launch_bounds__(256) void her_sample_pop_kernel(HerArgs A, int32_t members, int64_t episodes_stride) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = blockIdx.y;
  if (b >= A.B || p >= members) return;
  const int64_t ring = p * A.ring_cap * A.N, out = p * A.B;
  A.obs0 += p * A.N * D;
  A.obs_after += ring * D; A.next_obs += ring * D; A.action += ring * 3; A.reward += ring; A.done += ring;
  A.episodes += p * episodes_stride * 3;
  A.num_episodes += p;
  A.states += out * D; A.next_states += out * D; A.actions += out * 3; A.rewards += out; A.dones += out;
  if (A.picks_in) A.picks_in += out * 4;
  if (A.picks_out) A.picks_out += out * 4;
  A.seed += (uint64_t)p;
  her_sample_one<D>(A, b);
}

// The population form with a shared pool: her_sample_pop_kernel's grid and arrays, but a row of member p's batch may come from ANY
// member's trajectories.  Member p draws u0..u3 as her_sample_pop_kernel does (key (seed + p) ^ HER_KEY_XOR, counter blocks 0 and
// 1) and u4 from counter block 2 (words 0, 1; words 2, 3 are reserved and unread); the row is shared when u4 < share_ratio.
//   not shared: source member m = p, episode (int32)(u0 E_p) -- her_sample_pop_kernel's row
//   shared:     g = (int64)(u0 E_tot), E_tot = sum of num_episodes; m = the smallest member with g < E_0 + ... + E_m, episode
//               g - (E_0 + ... + E_(m-1)) -- random.sample(buffer, 1) over the concatenation of the members' trajectory lists,
//               which is her_sample_kernel's row on the members' rings merged column-wise ([cap][P N][...]) with seed + p
// The step, the relabel flag and the goal step come from u1..u3 and the length of member m's episode; the transition is read from
// member m's rings, the row is written into member p's outputs.  An empty pool (E_tot shared, E_p not) gives the inert row.
// Picks in and out are [P][B][5] = (member, episode within it, step_state, use_her, step_goal), the inert row's (-1, -1, 0, 0, 0);
// with picks supplied nothing is drawn, and a pick that names no member or none of its episodes gives the inert row.
template <int D>
__global__ __launch_bounds__(256) void her_sample_pop_shared_kernel(HerArgs A, int32_t members, int64_t episodes_stride,
                                                                   double share_ratio) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = blockIdx.y;
  if (b >= A.B || p >= members) return;
  const int64_t *counts = A.num_episodes;                   // i64 [P]
  const int64_t out = p * A.B;
  A.states += out * D; A.next_states += out * D; A.actions += out * 3; A.rewards += out; A.dones += out;
  int32_t *picks_out = A.picks_out ? A.picks_out + (out + b) * 5 : nullptr;
  int32_t m = -1, ep = -1, st = 0, her = 0, sg = 0;
  double u1 = 0.0, u2 = 0.0, u3 = 0.0;
  if (A.picks_in) {
    const int32_t *pk = A.picks_in + (out + b) * 5;
    m = pk[0]; ep = pk[1]; st = pk[2]; her = pk[3]; sg = pk[4];
    if (m < 0 || m >= members || ep < 0 || (int64_t)ep >= counts[m]) m = -1;
  } else {
    double u0, u4 = 1.0, unread;
    const uint64_t key = (A.seed + (uint64_t)p) ^ HER_KEY_XOR;
    philox_pair(key, (uint64_t)b, (uint32_t)A.draw, 0u, u0, u1);
    philox_pair(key, (uint64_t)b, (uint32_t)A.draw, 1u, u2, u3);
    if (share_ratio > 0.0) philox_pair(key, (uint64_t)b, (uint32_t)A.draw, 2u, u4, unread);   // else: u4 < 0 never holds
    if (u4 < share_ratio) {
      int64_t total = 0;
      for (int32_t j = 0; j < members; ++j) total += counts[j] > 0 ? counts[j] : 0;
      if (total > 0) {
        const int64_t g = (int64_t)(u0 * (double)total);    // < total: u0 <= 1 - 2^-53 and total < 2^31
        int64_t before = 0;                                 // E_0 + ... + E_(m-1)
        for (int32_t j = 0; j < members; ++j) {
          const int64_t Ej = counts[j];
          if (Ej <= 0) continue;                            // an empty member is passed over
          if (m >= 0) before += counts[m];
          m = j;
          if (g < before + Ej) break;
        }
        const int64_t within = g - before;
        ep = (int32_t)(within < counts[m] ? within : counts[m] - 1);
      }
    } else if (counts[p] > 0) {
      m = (int32_t)p;
      ep = (int32_t)(u0 * (double)counts[p]);
    }
  }
  if (m < 0) {
    her_inert_row<D>(A, b);
    if (picks_out) { picks_out[0] = picks_out[1] = -1; picks_out[2] = picks_out[3] = picks_out[4] = 0; }
    return;
  }
  const int64_t ring = (int64_t)m * A.ring_cap * A.N;       // the source: member m's rings and episode list
  A.obs0 += (int64_t)m * A.N * D;
  A.obs_after += ring * D; A.next_obs += ring * D; A.action += ring * 3; A.reward += ring; A.done += ring;
  A.episodes += (int64_t)m * episodes_stride * 3;
  if (!A.picks_in) her_draw_steps(A, A.episodes[3 * ep + 2], u1, u2, u3, st, her, sg);
  her_row<D>(A, b, ep, st, her, sg);
  if (picks_out) { picks_out[0] = m; picks_out[1] = ep; picks_out[2] = st; picks_out[3] = her; picks_out[4] = sg; }
}

}  // namespace armenv
