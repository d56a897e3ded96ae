// armenv.hip -- the C ABI of include/armenv.h: handle life-cycle, argument checks, dispatch to the engine of the
// handle's (task, precision) (armenv_engine.h / armenv_task.hip), the fused actor's weight packing and entry kernel,
// and the trajectory-store kernels (armenv_replay.h).
#include "armenv_engine.h"
#include "armenv_replay.h"

static thread_local std::string g_err;

int armenv_fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// DATD3_MLP.take_action (/root/reference/algo/DATD3/DATD3_mlp.py:88-109) for n reach states (6 floats): actions [n][3], and (nullable)
// the two Q values and which actor was picked.
template <int OBS>
static __global__ __launch_bounds__(256) void datd3_kernel(const ActorParams *nets, const ActorParamsH *nets_h, int64_t n, const float *states,
                                                    float *actions, float *q1_out, float *q2_out, uint8_t *picked_out) {
  __shared__ float4 w1_lds[ACTOR_W1_LDS_FLOATS_H / 4];
  __shared__ uint4 w2_ring[ACTOR_RING_UINT4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // grid covers n rounded up to 256: every wave is live
  const int64_t ic = i < n ? i : n - 1;
  float s[OBS], a[3], q1, q2;
  int picked;
  static_for<0, OBS>([&](auto DI) { constexpr int d = DI; s[d] = states[ic * OBS + d]; });
  datd3_forward_wg<OBS>(nets, nets_h, w1_lds, w2_ring, 4, s, a, q1, q2, picked);
  actor_ring_drain();
  if (i < n) {
    actions[3 * i] = a[0]; actions[3 * i + 1] = a[1]; actions[3 * i + 2] = a[2];
    if (q1_out) q1_out[i] = q1;
    if (q2_out) q2_out[i] = q2;
    if (picked_out) picked_out[i] = (uint8_t)picked;
  }
}

// the LDS tables of a nine-input net (actor_stage_w1 + actor_stage_w1h) built once in a workgroup's LDS and written out as an image
static __global__ __launch_bounds__(256) void actor_lds_image_kernel(const float *W1P, const float4 *B2W3, float4 *image, int in_dim) {
  __shared__ float4 tab[ACTOR_W1_LDS_FLOATS_H / 4];
  actor_stage_w1(W1P, tab, B2W3, in_dim);
  actor_stage_w1h(W1P, tab, in_dim);
  __syncthreads();
  for (int i = threadIdx.x; i < ACTOR_W1_LDS_FLOATS_H / 4; i += blockDim.x) image[i] = tab[i];
}

// One 256-wide MLP packed into `base` for the device: W1P | W2P | B2W3 | W2H + W2L [| LDS image], described by A and H.
// in_dim: the columns of m.W1; rows: the rows of m.W3 (3: PolicyNet, 1: QValueNet); raw: A.raw.  image_dim > 0: the net runs as
// an image_dim-input net (W1P's zero columns behind in_dim) and the LDS tables for it are built once behind W2L (lds_image).
int EngineBase::pack_net(const ArmEnvMlp &m, int in_dim, int rows, bool raw, int image_dim, float bound, float *base,
                         ActorParams &A, ActorParamsH &H, hipStream_t s) {
  float *W1P = base, *W2P = base + kNetW2P, *B2W3 = base + kNetB2W3;
  _Float16 *W2H = reinterpret_cast<_Float16 *>(base + kNetW2H), *W2L = W2H + kNetW2;
  float4 *image = image_dim > 0 ? reinterpret_cast<float4 *>(base + kNetImage) : nullptr;
  hipLaunchKernelGGL(actor_pack_kernel, dim3((unsigned)(kNetW2 / 256)), dim3(256), 0, s, m.W1, m.b1, m.W2, m.b2, m.W3, in_dim, W1P,
                     W2P, B2W3, W2H, W2L, rows);
  if (image)
    hipLaunchKernelGGL(actor_lds_image_kernel, dim3(1), dim3(256), 0, s, W1P, reinterpret_cast<const float4 *>(B2W3), image, image_dim);
  HIP_TRY(hipGetLastError());
  float hb3[3] = {0.f, 0.f, 0.f};
  HIP_TRY(hipMemcpyAsync(hb3, m.b3, sizeof(float) * rows, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  A.W1P = W1P;
  A.W2P = reinterpret_cast<const float4 *>(W2P);
  A.B2W3 = reinterpret_cast<const float4 *>(B2W3);
  for (int k = 0; k < 3; ++k) A.b3[k] = hb3[k];
  A.bound = bound;
  A.in_dim = image ? image_dim : in_dim;
  A.raw = raw ? 1 : 0;
  A.lds_image = image;
  H.W2H = reinterpret_cast<const half8 *>(W2H);
  H.W2L = reinterpret_cast<const half8 *>(W2L);
  return ARMENV_OK;
}

int EngineBase::set_actor(const ArmEnvMlp &m, int in_dim, float bound, hipStream_t s) {
  if (!actor_buf && hipMalloc(reinterpret_cast<void **>(&actor_buf), kNetImage * sizeof(float)) != hipSuccess)
    return fail(ARMENV_ENOMEM, "armenv_set_policy: hipMalloc failed");
  return pack_net(m, in_dim, 3, false, 0, bound, actor_buf, pol.actor, pol.actor_h, s);
}

// armenv_set_policy_datd3: the four nets packed like set_actor packs one (the W2P table of the exact-f32 actor is not needed: the
// fused DATD3 policy runs the f16x3 passes only), every net as an (obs_dim + 3)-input net (datd3_forward_wg): the actors' W1 rows carry
// zeros in the three columns behind obs_dim, the critics' W1 is [hidden][obs_dim + 3] as it is.
int EngineBase::set_datd3(const ArmEnvMlp *const nets[4], int obs_dim, float bound, hipStream_t s) {
  const size_t per_net = kNetImage + ACTOR_W1_LDS_FLOATS_H;
  const size_t tab = (4 * sizeof(ActorParams) + 4 * sizeof(ActorParamsH) + sizeof(float) - 1) / sizeof(float);
  if (!datd3_buf && hipMalloc(reinterpret_cast<void **>(&datd3_buf), (4 * per_net + tab) * sizeof(float)) != hipSuccess)
    return fail(ARMENV_ENOMEM, "armenv_set_policy_datd3: hipMalloc failed");
  ActorParams A[4];
  ActorParamsH H[4];
  for (int k = 0; k < 4; ++k) {
    const ArmEnvMlp &m = *nets[k];
    const bool critic = k >= 2;
    // DADDPG (armenv_set_policy_daddpg): ONE critic values both proposals -- the fourth entry of the table IS the third (same packed
    // weights, same LDS image), which datd3_forward_wg recognises and runs on the tables and the ring the third pass left behind
    if (k == 3 && m.W1 == nets[2]->W1 && m.b1 == nets[2]->b1 && m.W2 == nets[2]->W2 && m.b2 == nets[2]->b2 && m.W3 == nets[2]->W3 &&
        m.b3 == nets[2]->b3) {
      A[3] = A[2];
      H[3] = H[2];
      continue;
    }
    const int rc = pack_net(m, critic ? obs_dim + 3 : obs_dim, critic ? 1 : 3, critic, obs_dim + 3, bound, datd3_buf + k * per_net,
                            A[k], H[k], s);
    if (rc != ARMENV_OK) return rc;
  }
  char *t = reinterpret_cast<char *>(datd3_buf + 4 * per_net);
  HIP_TRY(hipMemcpyAsync(t, A, sizeof A, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(t + sizeof A, H, sizeof H, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  pol.datd3 = reinterpret_cast<const ActorParams *>(t);
  pol.datd3_h = reinterpret_cast<const ActorParamsH *>(t + sizeof A);
  datd3_obs = obs_dim;
  return ARMENV_OK;
}

// f(std::integral_constant<int, 6 | 9>): a net's observation width (reach | push, pick) as a template argument
template <class F> static void with_obs(int obs_dim, F &&f) {
  if (obs_dim == 6) f(std::integral_constant<int, 6>{});
  else f(std::integral_constant<int, 9>{});
}

int EngineBase::datd3_forward(int64_t n, const float *states, float *actions, float *q1, float *q2, uint8_t *picked, hipStream_t s) {
  if (!pol.datd3) return fail(ARMENV_ESTATE, "armenv_datd3_forward: no DATD3 policy installed (armenv_set_policy_datd3)");
  with_obs(datd3_obs, [&](auto obs) {
    hipLaunchKernelGGL(datd3_kernel<decltype(obs)::value>, dim3(grid_for(n, 256)), dim3(256), 0, s, pol.datd3, pol.datd3_h, n, states,
                       actions, q1, q2, picked);
  });
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int EngineBase::actor_forward(int64_t n, const float *states, float *actions, hipStream_t s) {
  if (!pol.actor.W2P) return fail(ARMENV_ESTATE, "armenv_actor_forward: no actor installed (armenv_set_policy)");
  const bool fast = pol.kind == ARMENV_POLICY_ACTOR_F16X3;
  with_obs(pol.actor.in_dim, [&](auto obs) {
    constexpr int D = decltype(obs)::value;
    if (fast) hipLaunchKernelGGL((actor_kernel<D, 1>), dim3(grid_for(n, 256)), dim3(256), 0, s, pol.actor, pol.actor_h, n, states, actions);
    else hipLaunchKernelGGL((actor_kernel<D, 0>), dim3(grid_for(n, 256)), dim3(256), 0, s, pol.actor, pol.actor_h, n, states, actions);
  });
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

struct ArmEnv {
  ArmEnvConfig cfg;
  std::unique_ptr<EngineBase> eng;
};

static EngineBase *make_engine(const ArmEnvConfig &cfg) {
#ifdef ARMENV_TIMELINE   // the instrumented build (make timeline) carries the f64 reach engine only
  return cfg.task == ARMENV_TASK_REACH && cfg.precision == 64 ? armenv_make_engine_reach_f64(cfg) : nullptr;
#endif
  const bool d = cfg.precision == 64;
  switch (cfg.task) {
    case ARMENV_TASK_REACH: return d ? armenv_make_engine_reach_f64(cfg) : armenv_make_engine_reach_f32(cfg);
    case ARMENV_TASK_PUSH: return d ? armenv_make_engine_push_f64(cfg) : armenv_make_engine_push_f32(cfg);
    case ARMENV_TASK_PICK: return d ? armenv_make_engine_pick_f64(cfg) : armenv_make_engine_pick_f32(cfg);
  }
  return nullptr;
}

static void fill_chain(ArmEnvChain *out, const double (*xyz)[3], const double (*rpy)[3], const double *lo,
                       const double *hi) {
  std::memset(out, 0, sizeof *out);
  for (int j = 0; j < NJ; ++j) {
    for (int k = 0; k < 3; ++k) { out->origin_xyz[j][k] = xyz[j][k]; out->origin_rpy[j][k] = rpy[j][k]; }
    out->limit_lo[j] = lo[j];
    out->limit_hi[j] = hi[j];
  }
}

// Issue rate of the vector pipe as the env kernels use it (armenv_probe_issue_rate): waves of 64 lanes, `per_simd` of them on
// every SIMD of the device, back-to-back independent v_fma on sixteen chains with vector operands, nothing else in the loop.
template <typename T>
__global__ __launch_bounds__(256) void issue_probe_kernel(T *out, int iters, T a, T b) {
  T x[16];
  static_for<0, 16>([&](auto I) { constexpr int t = I; x[t] = a * (T)(t + (int)threadIdx.x); });
  T av = a, bv = b;
  asm volatile("" : "+v"(av), "+v"(bv));
  // 128 instructions per trip: a taken backward branch costs a lone wave tens of cycles (a 16-instruction body measured 12 cycles
  // per instruction instead of 6.6)
  for (int i = 0; i < iters; ++i)
    static_for<0, 128>([&](auto I) { constexpr int t = I % 16; x[t] = Mth<T>::fma(x[t], av, bv); asm volatile("" : "+v"(x[t])); });   // (no SLP packing into v_pk_fma_f32)
  T s = T(0);
  static_for<0, 16>([&](auto I) { constexpr int t = I; s += x[t]; });
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <typename T>
static int issue_probe(int device, int waves_per_simd, double *ns_out) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  const int blocks = prop.multiProcessorCount * waves_per_simd;   // 256 threads = one wave on each of a CU's four SIMDs
  T *out = nullptr;
  HIP_TRY(hipMalloc(&out, sizeof(T) * 256 * (size_t)blocks));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  const int iters = 512;
  double best = 1e30;
  // an idle MI355X needs ~30 ms of load to reach its steady clocks (tests/tools/clock_ramp.py): ~55 ms of the same kernel first
  for (int k = 0; k < 300 / waves_per_simd; ++k) hipLaunchKernelGGL(issue_probe_kernel<T>, dim3(blocks), dim3(256), 0, 0, out, iters, T(0.999), T(1e-3));
  for (int rep = 0; rep < 5; ++rep) {
    HIP_TRY(hipEventRecord(e0, 0));
    for (int k = 0; k < 5; ++k) hipLaunchKernelGGL(issue_probe_kernel<T>, dim3(blocks), dim3(256), 0, 0, out, iters, T(0.999), T(1e-3));
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    const double ns = (double)ms * 1e6 / 5 / ((double)iters * 128) / waves_per_simd;
    if (ns < best) best = ns;
  }
  HIP_TRY(hipGetLastError());
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(out);
  *ns_out = best;
  return ARMENV_OK;
}

// armenv_probe_clock: one wave on every SIMD of the device runs a fixed dependent chain of CLOCK_PROBE_CHAIN v_fma_f32 (its duration
// in shader cycles does not depend on anything but the chain) between two readings of the constant-rate counter (s_memrealtime,
// 100 MHz) and of s_memtime.  Row w of out (one row per wave): [0] chain duration in 10 ns ticks (inversely proportional to the
// shader clock of the wave's XCD at that moment), [1] the same in s_memtime ticks, [2] the 100 MHz counter at the start (the device's
// own time line), [3] the XCD the wave ran on (HW_REG_XCC_ID) in bits 0..3 and the chain length in bits 8...
constexpr int CLOCK_PROBE_CHAIN = 2048;
__global__ __launch_bounds__(256) void clock_probe_kernel(unsigned long long *out, float a, float b) {
  float x = a * (float)threadIdx.x;
  asm volatile("" : "+v"(x), "+v"(a), "+v"(b));
  const unsigned long long w0 = wall_clock64(), c0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int i = 0; i < CLOCK_PROBE_CHAIN / 128; ++i)
    static_for<0, 128>([&](auto) { x = __builtin_fmaf(x, a, b); asm volatile("" : "+v"(x)); });
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), w1 = wall_clock64();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *row = out + 4 * ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    row[0] = w1 - w0; row[1] = c1 - c0; row[2] = w0;
    row[3] = (unsigned long long)(xcc & 15u) | ((unsigned long long)CLOCK_PROBE_CHAIN << 8) | (x == 12345.f ? 1ull << 63 : 0ull);
  }
}

// What armenv_set_policy and armenv_set_policy_datd3 share: the noise check, the checks of a fused policy (`pack` then installs its
// nets) and the policy itself.  fn, nets_are, need64, book: the caller's wording of the errors.
template <class Pack>
static int install_policy(ArmEnv *env, int32_t kind, int32_t hidden_dim, float action_bound, float noise_sigma, float noise_clip,
                          const char *fn, const char *nets_are, const char *need64, const char *book, Pack &&pack) {
  if (kind != ARMENV_POLICY_EXTERNAL && !(noise_sigma >= 0.f && noise_clip > 0.f))
    return fail(ARMENV_EINVAL, "%s: need noise_sigma >= 0 and noise_clip > 0", fn);
  if (fused_policy(kind)) {
    if (hidden_dim != ACTOR_HID)
      return fail(ARMENV_EINVAL, "%s: hidden_dim %d; the fused %s built for %d (config.py:56)", fn, hidden_dim, nets_are, ACTOR_HID);
    if (env->cfg.num_envs % 64 != 0) return fail(ARMENV_EINVAL, "%s: %s", fn, need64);
    if (env->cfg.fence_counters) return fail(ARMENV_ESTATE, "%s: %s", fn, book);
    const int rc = pack();
    if (rc != ARMENV_OK) return rc;
  }
  env->eng->pol.kind = kind;
  env->eng->pol.sigma = noise_sigma;
  env->eng->pol.clip = noise_clip;
  env->eng->pol.bound = action_bound;
  return ARMENV_OK;
}

extern "C" {

int armenv_probe_clock(int32_t device, uint64_t *out_dev, int32_t *rows, void *stream) {
  DeviceGuard guard_(device);
  if (!guard_.ok) return fail(ARMENV_ENODEV, "armenv_probe_clock: hipSetDevice(%d) failed", (int)device);
  static thread_local int cus[64];
  if (device < 0 || device >= 64) return fail(ARMENV_ENODEV, "armenv_probe_clock: device %d", (int)device);
  if (!cus[device]) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    cus[device] = prop.multiProcessorCount;
  }
  if (rows) *rows = 4 * cus[device];
  if (!out_dev) return ARMENV_OK;       // size query
  hipLaunchKernelGGL(clock_probe_kernel, dim3(cus[device]), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<unsigned long long *>(out_dev), 0.999f, 1e-3f);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int32_t armenv_abi_version(void) { return ARMENV_ABI_VERSION; }
const char *armenv_last_error(void) { return g_err.c_str(); }

int armenv_builtin_chain(int32_t robot, ArmEnvChain *out) {
  if (!out) return fail(ARMENV_EINVAL, "armenv_builtin_chain: out is NULL");
  if (robot == ARMENV_ROBOT_KUKA) fill_chain(out, KukaChain::xyz, KukaChain::rpy, KukaChain::limit_lo, KukaChain::limit_hi);
  else if (robot == ARMENV_ROBOT_DIANA) fill_chain(out, DianaChain::xyz, DianaChain::rpy, DianaChain::limit_lo, DianaChain::limit_hi);
  else return fail(ARMENV_EINVAL, "armenv_builtin_chain: unknown robot %d", robot);
  return ARMENV_OK;
}

int armenv_default_config(int32_t task, ArmEnvConfig *c) {
  if (!c) return fail(ARMENV_EINVAL, "armenv_default_config: cfg is NULL");
  if (task < ARMENV_TASK_REACH || task > ARMENV_TASK_PICK) return fail(ARMENV_EINVAL, "unknown task %d", task);
  std::memset(c, 0, sizeof *c);
  c->abi_version = ARMENV_ABI_VERSION;
  c->device = 0;
  c->num_envs = 1;
  c->task = task;
  c->precision = 64;
  c->fk_path = ARMENV_FK_AUTO;
  c->auto_reset = 1;
  c->seed = 0;
  c->env_id_offset = 0;
  c->dv = task == ARMENV_TASK_REACH ? 0.02 : 0.08;
  c->reach_dis = 0.01;
  c->max_steps = 500;
  c->clamp_joint_limits = 0;
  c->limit_erp = 0.2;      // Bullet's default constraint ERP (btContactSolverInfo::m_erp); read by clamp_joint_limits == 2 only
  c->fence_counters = 0;   // diagnostics off by default (costs ~6 % of a reach step when the limits are crossed as often as under the random policy)
  c->fence_z = 0.05;   // arm-table contact acts when the flange is driven to z <~ 0.05
  c->fence_pivot = 1e-2;   // conditioning term of the fence: amplification of rounding differences >~ 100
  const double lo[3] = {0.2, -0.3, 0.0}, hi[3] = {0.7, 0.3, 0.55};
  for (int k = 0; k < 3; ++k) { c->box_lo[k] = lo[k]; c->box_hi[k] = hi[k]; c->goal_lo[k] = lo[k]; c->goal_hi[k] = hi[k]; }
  if (task == ARMENV_TASK_PUSH) c->box_hi[2] = 0.1;                 // rl_push_env.py:314
  if (task == ARMENV_TASK_PICK) c->box_hi[2] = 0.55 + 0.257;       // rl_pick_env.py:313
  // p.getQuaternionFromEuler([0, -pi, pi/2]) (Bullet setEulerZYX)
  {
    const double pi = 3.14159265358979323846;
    const double hr = 0.0, hp = -pi * 0.5, hy = pi * 0.25;
    const double cr = std::cos(hr), sr = std::sin(hr), cp = std::cos(hp), sp = std::sin(hp), cy = std::cos(hy), sy = std::sin(hy);
    c->target_quat[0] = sr * cp * cy - cr * sp * sy;
    c->target_quat[1] = cr * sp * cy + sr * cp * sy;
    c->target_quat[2] = cr * cp * sy - sr * sp * cy;
    c->target_quat[3] = cr * cp * cy + sr * sp * sy;
  }
  const double qi[NJ] = {0.006418, 0.413184, -0.011401, -1.589317, 0.005379, 1.137684, -0.006539};
  for (int j = 0; j < NJ; ++j) c->q_init[j] = qi[j];
  c->ik_lambda = 1e-5;
  c->ik_residual = 1e-4;
  c->ik_max_dtheta = 45.0 * 3.14159265358979323846 / 180.0;
  c->ik_max_iters = 20;
  c->ik_exit_mode = 0;
  c->ik_angle_f32 = 1;
  c->ik_tip_offset[0] = c->ik_tip_offset[1] = c->ik_tip_offset[2] = 0.0;   // the URDF link-7 frame (what getLinkState(...)[4] returns)
  c->push_success_dis = 0.05;
  c->push_cube_half = 0.02;
  c->push_eef_radius = 0.03;
  c->push_place_z = 0.01;      // rl_push_env.py:199,206 (pick :194): spawn height of cube and target
  // where Bullet lets the cube come to rest on the table: fitted to the reference's recorded push run (visdata/push/origin_TD3), whose
  // untouched episodes return -500 - 50 sqrt(planar^2 + 0.01474^2) to 2e-3 (tests/reference_run.py); table top -0.025 + half a cube
  c->push_rest_z = 0.01 - 0.01474;
  c->push_place_min = 0.22;
  c->push_place_max = 0.25;
  // the cube under stepSimulation (include/armenv.h, push_contact_model): fall constants from the reference's scene, tool geometry
  // nominal, push_contact_erp and push_friction fitted to its two recorded push runs (tests/tools/fit_bullet.py part C)
  c->push_contact_model = 1;
  c->push_tool_radius = 0.045;      // the KUKA flange's nominal geometry: 45 mm radius, its face 45 mm below the link-7 frame
  c->push_tool_below = 0.045;
  c->push_contact_erp = 0.01;       // fitted (with push_friction)
  c->push_contact_split = 0.04;
  c->push_friction = 0.03;
  c->push_gravity = 10.0;           // rl_push_env.py:155
  c->push_dt = 1.0 / 240.0;
  c->push_drop_contact = 0.015;
  c->push_drop_relax = 0.1;
  c->pick_gripper_length = 0.257;   // rl_pick_env.py:79
  c->pick_trigger_dis = 0.006;      // rl_pick_env.py:412
  c->pick_jaw_half = 0.02;
  // measured at 32 768 envs, 100-step launches: pick 27.6 -> 23.3 us per step at 62; push and reach are
  // faster in lockstep (their per-wave maxima are close to their means, and every transition round costs a tail block)
  c->rollout_ready_lanes = task == ARMENV_TASK_PICK ? 62 : 0;
  // the transition rule that lets every lane on its way to the iteration cap run on (round 3; same size: 22.8 -> 21.1 us per
  // step, 1 000-step launches 16.0 -> 14.3; tests/tools/ready_lanes_sweep.py, profiles/r03_async_schedule.txt)
  c->rollout_straggler_trips = task == ARMENV_TASK_PICK ? 6 : 0;
  return armenv_builtin_chain(ARMENV_ROBOT_KUKA, &c->chain);
}

int armenv_create(const ArmEnvConfig *cfg, ArmEnv **out) {
  if (!cfg || !out) return fail(ARMENV_EINVAL, "armenv_create: NULL argument");
  *out = nullptr;
  if (cfg->abi_version != ARMENV_ABI_VERSION)
    return fail(ARMENV_EINVAL, "armenv_create: abi_version %d, library is %d", cfg->abi_version, ARMENV_ABI_VERSION);
  if (cfg->num_envs < 1) return fail(ARMENV_EINVAL, "armenv_create: num_envs must be >= 1");
  if (cfg->precision != 64 && cfg->precision != 32) return fail(ARMENV_EINVAL, "armenv_create: precision must be 32 or 64");
  if (cfg->task < ARMENV_TASK_REACH || cfg->task > ARMENV_TASK_PICK) return fail(ARMENV_EINVAL, "armenv_create: unknown task %d", cfg->task);
  if (cfg->ik_max_iters < 0 || cfg->ik_max_iters > 1000) return fail(ARMENV_EINVAL, "armenv_create: ik_max_iters out of range");
  const bool tip = cfg->ik_tip_offset[0] != 0.0 || cfg->ik_tip_offset[1] != 0.0 || cfg->ik_tip_offset[2] != 0.0;
  // the bookkeeping builds report a call's update count in a u8 (ik_updates) and fold a wave's trip maximum over 8 bits
  if ((cfg->fence_counters || tip) && cfg->ik_max_iters > 254)
    return fail(ARMENV_EINVAL, "armenv_create: fence_counters / ik_tip_offset need ik_max_iters <= 254 (the per-step update count is a u8)");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(cfg->ik_tip_offset[k])) return fail(ARMENV_EINVAL, "armenv_create: ik_tip_offset is not finite");
  if (cfg->fence_counters < 0 || cfg->fence_counters > 2) return fail(ARMENV_EINVAL, "armenv_create: fence_counters must be 0, 1 or 2");
  if (cfg->clamp_joint_limits < 0 || cfg->clamp_joint_limits > 2) return fail(ARMENV_EINVAL, "armenv_create: clamp_joint_limits must be 0, 1 or 2");
  if (cfg->clamp_joint_limits == 2 && !(cfg->limit_erp > 0.0 && cfg->limit_erp <= 1.0)) return fail(ARMENV_EINVAL, "armenv_create: limit_erp must be in (0, 1]");
  if (cfg->rollout_lanes_per_wave != 0 && cfg->rollout_lanes_per_wave != 32 && cfg->rollout_lanes_per_wave != 64)
    return fail(ARMENV_EINVAL, "armenv_create: rollout_lanes_per_wave must be 0, 32 or 64");
  if (cfg->rollout_straggler_trips < 0 || cfg->rollout_straggler_trips > 64)
    return fail(ARMENV_EINVAL, "armenv_create: rollout_straggler_trips must be in 0..64");
  if (cfg->rollout_waves_per_simd < 0 || cfg->rollout_waves_per_simd > 2) return fail(ARMENV_EINVAL, "armenv_create: rollout_waves_per_simd must be 0, 1 or 2");
  if (cfg->push_contact_model < 0 || cfg->push_contact_model > 1 || cfg->reserved0 != 0) return fail(ARMENV_EINVAL, "armenv_create: push_contact_model must be 0 or 1 (reserved0 0)");
  if (cfg->task != ARMENV_TASK_REACH && cfg->push_contact_model == 1 &&
      !(cfg->push_dt > 0.0 && cfg->push_gravity > 0.0 && cfg->push_drop_contact > 0.0 && cfg->push_drop_contact < 1.0 && cfg->push_drop_relax > 0.0 &&
        cfg->push_drop_relax <= 1.0 && cfg->push_contact_erp >= 0.0 && cfg->push_friction >= 0.0 && cfg->push_tool_radius > 0.0))
    return fail(ARMENV_EINVAL, "armenv_create: push_contact_model 1 needs push_dt, push_gravity, push_tool_radius > 0, push_drop_contact in (0, 1), push_drop_relax in (0, 1], push_contact_erp, push_friction >= 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ARMENV_ENODEV, "armenv_create: no HIP device is visible (this library has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(ARMENV_ENODEV, "armenv_create: device %d of %d", cfg->device, ndev);
  DeviceGuard guard(cfg->device);
  if (!guard.ok) return fail(ARMENV_ENODEV, "armenv_create: hipSetDevice(%d) failed", cfg->device);
  std::unique_ptr<ArmEnv> env(new (std::nothrow) ArmEnv());
  if (!env) return fail(ARMENV_ENOMEM, "armenv_create: host allocation failed");
  env->cfg = *cfg;
  if (tip) env->cfg.fence_counters = 2;   // the tip offset lives in the MODE 2 bookkeeping build of the kernels (armenv_kin.h)
  env->eng.reset(make_engine(env->cfg));
  if (!env->eng) return fail(ARMENV_ENOMEM, "armenv_create: host allocation failed");
  const int rc = env->eng->init(env->cfg);
  if (rc != ARMENV_OK) return rc;
  *out = env.release();
  return ARMENV_OK;
}

void armenv_destroy(ArmEnv *env) {
  if (!env) return;
  DeviceGuard guard(env->cfg.device);
  delete env;
}

#define ENV_ENTER(env)                                                                  \
  if (!(env)) return fail(ARMENV_EINVAL, "%s: env is NULL", __func__);                  \
  DeviceGuard guard_((env)->cfg.device);                                                \
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice failed", __func__)

int armenv_reset(ArmEnv *env, const uint8_t *mask_dev, float *obs_dev, void *stream) {
  ENV_ENTER(env);
  return env->eng->reset(mask_dev, nullptr, obs_dev, static_cast<hipStream_t>(stream));
}

int armenv_reset_with_goal(ArmEnv *env, const uint8_t *mask_dev, const float *goal_dev, float *obs_dev, void *stream) {
  ENV_ENTER(env);
  if (!goal_dev) return fail(ARMENV_EINVAL, "armenv_reset_with_goal: goal_dev is NULL");
  return env->eng->reset(mask_dev, goal_dev, obs_dev, static_cast<hipStream_t>(stream));
}

int armenv_step(ArmEnv *env, const float *action_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
                uint8_t *success_dev, float *terminal_obs_dev, uint8_t *ik_updates_dev, double *diag_dev, void *stream) {
  ENV_ENTER(env);
  if (!obs_dev || !reward_dev || !done_dev || !success_dev) return fail(ARMENV_EINVAL, "armenv_step: NULL output buffer");
  if (ik_updates_dev && !env->cfg.fence_counters)
    return fail(ARMENV_ESTATE, "armenv_step: ik_updates_dev needs a handle created with fence_counters >= 1 (the bookkeeping build of the kernels)");
  if (diag_dev && env->cfg.fence_counters != 2)
    return fail(ARMENV_ESTATE, "armenv_step: diag_dev needs a handle created with fence_counters = 2");
  if (diag_dev && !action_dev && fused_policy(env->eng->pol.kind))
    return fail(ARMENV_ESTATE, "armenv_step: diag_dev is not available with a fused actor");
  StepIO io{action_dev, obs_dev, reward_dev, done_dev, success_dev, terminal_obs_dev, ik_updates_dev, diag_dev};
  if (!action_dev) {   // fused policy: a one-step rollout
    if (env->eng->pol.kind == ARMENV_POLICY_EXTERNAL)
      return fail(ARMENV_ESTATE, "armenv_step: action_dev is NULL and no fused policy is installed");
    return env->eng->rollout(1, nullptr, io, nullptr, static_cast<hipStream_t>(stream));
  }
  return env->eng->step(io, static_cast<hipStream_t>(stream));
}

int armenv_fk(ArmEnv *env, int64_t n, const double *q_dev, double *pos_dev, double *quat_dev, void *stream) {
  ENV_ENTER(env);
  if (n < 0 || (n > 0 && (!q_dev || !pos_dev))) return fail(ARMENV_EINVAL, "armenv_fk: bad arguments");
  if (n == 0) return ARMENV_OK;
  return env->eng->fk(n, q_dev, pos_dev, quat_dev, static_cast<hipStream_t>(stream));
}

int armenv_ik(ArmEnv *env, int64_t n, const double *q_dev, const double *target_pos_dev, double *q_out_dev,
              int32_t *iters_dev, void *stream) {
  ENV_ENTER(env);
  if (n < 0 || (n > 0 && (!q_dev || !target_pos_dev || !q_out_dev))) return fail(ARMENV_EINVAL, "armenv_ik: bad arguments");
  if (n == 0) return ARMENV_OK;
  return env->eng->ik(n, q_dev, target_pos_dev, q_out_dev, iters_dev, static_cast<hipStream_t>(stream));
}

int armenv_get_state(ArmEnv *env, double *q_dev, float *goal_dev, int32_t *step_dev, uint32_t *episode_dev,
                     double *ep_return_dev, double *aux_dev, double *trig_dev, void *stream) {
  ENV_ENTER(env);
  if (aux_dev && env->cfg.task == ARMENV_TASK_REACH) return fail(ARMENV_EINVAL, "armenv_get_state: aux is only defined for the push and pick tasks");
  if (goal_dev && env->cfg.task != ARMENV_TASK_REACH) return fail(ARMENV_EINVAL, "armenv_get_state: push / pick keep cube and target in aux, not goal");
  return env->eng->get_state(q_dev, goal_dev, step_dev, episode_dev, ep_return_dev, aux_dev, trig_dev, static_cast<hipStream_t>(stream));
}

int armenv_set_state(ArmEnv *env, const double *q_dev, const float *goal_dev, const int32_t *step_dev,
                     const uint32_t *episode_dev, const double *ep_return_dev, const double *aux_dev,
                     const double *trig_dev, void *stream) {
  ENV_ENTER(env);
  if (aux_dev && env->cfg.task == ARMENV_TASK_REACH) return fail(ARMENV_EINVAL, "armenv_set_state: aux is only defined for the push and pick tasks");
  if (goal_dev && env->cfg.task != ARMENV_TASK_REACH) return fail(ARMENV_EINVAL, "armenv_set_state: push / pick keep cube and target in aux, not goal");
  return env->eng->set_state(q_dev, goal_dev, step_dev, episode_dev, ep_return_dev, aux_dev, trig_dev, static_cast<hipStream_t>(stream));
}

int armenv_episode_stats(ArmEnv *env, double *last_return_dev, int32_t *last_len_dev, uint8_t *last_success_dev,
                         void *stream) {
  ENV_ENTER(env);
  return env->eng->episode_stats(last_return_dev, last_len_dev, last_success_dev, static_cast<hipStream_t>(stream));
}

int armenv_episode_returns_f32(ArmEnv *env, float *last_return_dev, void *stream) {
  ENV_ENTER(env);
  if (!last_return_dev) return fail(ARMENV_EINVAL, "armenv_episode_returns_f32: last_return_dev is NULL");
  return env->eng->episode_returns_f32(last_return_dev, static_cast<hipStream_t>(stream));
}

int armenv_counters(ArmEnv *env, uint64_t out[16], void *stream) {
  ENV_ENTER(env);
  if (!out) return fail(ARMENV_EINVAL, "armenv_counters: out is NULL");
  return env->eng->counters(out, static_cast<hipStream_t>(stream));
}

int armenv_summary(ArmEnv *env, double *out_dev, void *stream) {
  ENV_ENTER(env);
  if (!out_dev) return fail(ARMENV_EINVAL, "armenv_summary: out_dev is NULL");
  return env->eng->summary(out_dev, static_cast<hipStream_t>(stream));
}

int armenv_set_policy(ArmEnv *env, int32_t policy, const float *W1_dev, const float *b1_dev, const float *W2_dev,
                      const float *b2_dev, const float *W3_dev, const float *b3_dev, int32_t hidden_dim, float action_bound,
                      float noise_sigma, float noise_clip, void *stream) {
  ENV_ENTER(env);
  if (policy < ARMENV_POLICY_EXTERNAL || policy > ARMENV_POLICY_ACTOR_F16X3)
    return fail(ARMENV_EINVAL, "armenv_set_policy: unknown policy %d", policy);
  if (fused_policy(policy) && (!W1_dev || !b1_dev || !W2_dev || !b2_dev || !W3_dev || !b3_dev))
    return fail(ARMENV_EINVAL, "armenv_set_policy: NULL weight pointer");
  const ArmEnvMlp m{W1_dev, b1_dev, W2_dev, b2_dev, W3_dev, b3_dev};
  return install_policy(env, policy, hidden_dim, action_bound, noise_sigma, noise_clip, "armenv_set_policy", "actor is",
                        "the fused actor needs num_envs to be a multiple of 64 (full wavefronts)",
                        "the bookkeeping builds of the kernels (fence_counters, ik_tip_offset) exist for external "
                        "actions and the in-kernel random policy, not for the fused actors",
                        [&] { return env->eng->set_actor(m, armenv_obs_dim(env), action_bound, static_cast<hipStream_t>(stream)); });
}

int armenv_set_policy_datd3(ArmEnv *env, const ArmEnvMlp *actor1, const ArmEnvMlp *actor2, const ArmEnvMlp *critic1,
                            const ArmEnvMlp *critic2, int32_t hidden_dim, float action_bound, float noise_sigma, float noise_clip,
                            void *stream) {
  ENV_ENTER(env);
  const ArmEnvMlp *nets[4] = {actor1, actor2, critic1, critic2};
  for (const ArmEnvMlp *m : nets)
    if (!m || !m->W1 || !m->b1 || !m->W2 || !m->b2 || !m->W3 || !m->b3) return fail(ARMENV_EINVAL, "armenv_set_policy_datd3: NULL network or weight pointer");
  return install_policy(env, ARMENV_POLICY_DATD3, hidden_dim, action_bound, noise_sigma, noise_clip, "armenv_set_policy_datd3", "nets are",
                        "num_envs must be a multiple of 64 (full wavefronts)",
                        "not on a bookkeeping handle (fence_counters, ik_tip_offset)",
                        [&] { return env->eng->set_datd3(nets, armenv_obs_dim(env), action_bound, static_cast<hipStream_t>(stream)); });
}

int armenv_set_policy_daddpg(ArmEnv *env, const ArmEnvMlp *actor1, const ArmEnvMlp *actor2, const ArmEnvMlp *critic, int32_t hidden_dim,
                             float action_bound, float noise_sigma, float noise_clip, void *stream) {
  const int rc = armenv_set_policy_datd3(env, actor1, actor2, critic, critic, hidden_dim, action_bound, noise_sigma, noise_clip, stream);
  if (rc != ARMENV_OK) return rc;
  env->eng->pol.kind = ARMENV_POLICY_DADDPG;
  return ARMENV_OK;
}

int armenv_datd3_forward(ArmEnv *env, int64_t n, const float *states_dev, float *actions_dev, float *q1_dev, float *q2_dev,
                         uint8_t *picked_dev, void *stream) {
  ENV_ENTER(env);
  if (n < 0 || (n > 0 && (!states_dev || !actions_dev))) return fail(ARMENV_EINVAL, "armenv_datd3_forward: bad arguments");
  if (n == 0) return ARMENV_OK;
  return env->eng->datd3_forward(n, states_dev, actions_dev, q1_dev, q2_dev, picked_dev, static_cast<hipStream_t>(stream));
}

int armenv_actor_forward(ArmEnv *env, int64_t n, const float *states_dev, float *actions_dev, void *stream) {
  ENV_ENTER(env);
  if (n < 0 || (n > 0 && (!states_dev || !actions_dev))) return fail(ARMENV_EINVAL, "armenv_actor_forward: bad arguments");
  if (n == 0) return ARMENV_OK;
  return env->eng->actor_forward(n, states_dev, actions_dev, static_cast<hipStream_t>(stream));
}

int armenv_rollout(ArmEnv *env, int32_t steps, const float *actions_dev, float *obs_dev, float *reward_dev,
                   uint8_t *done_dev, uint8_t *success_dev, float *actions_out_dev, float *terminal_obs_dev,
                   uint8_t *ik_updates_dev, double *diag_dev, void *stream) {
  ENV_ENTER(env);
  if (steps < 0) return fail(ARMENV_EINVAL, "armenv_rollout: steps < 0");
  if (steps == 0) return ARMENV_OK;
  if (!obs_dev || !reward_dev || !done_dev || !success_dev) return fail(ARMENV_EINVAL, "armenv_rollout: NULL output buffer");
  if (!actions_dev && env->eng->pol.kind == ARMENV_POLICY_EXTERNAL)
    return fail(ARMENV_ESTATE, "armenv_rollout: actions_dev is NULL and no fused policy is installed");
  if (ik_updates_dev && !env->cfg.fence_counters)
    return fail(ARMENV_ESTATE, "armenv_rollout: ik_updates_dev needs a handle created with fence_counters >= 1 (the bookkeeping build of the kernels)");
  if (diag_dev && env->cfg.fence_counters != 2)
    return fail(ARMENV_ESTATE, "armenv_rollout: diag_dev needs a handle created with fence_counters = 2");
  if ((ik_updates_dev || diag_dev) && !actions_dev && fused_policy(env->eng->pol.kind))
    return fail(ARMENV_ESTATE, "armenv_rollout: ik_updates_dev / diag_dev are not available with a fused actor");
  StepIO io{nullptr, obs_dev, reward_dev, done_dev, success_dev, terminal_obs_dev, ik_updates_dev, diag_dev};
  return env->eng->rollout(steps, actions_dev, io, actions_out_dev, static_cast<hipStream_t>(stream));
}

#define DEV_ENTER(device)                                                              \
  DeviceGuard guard_(device);                                                          \
  if (!guard_.ok) return fail(ARMENV_ENODEV, "%s: hipSetDevice(%d) failed", __func__, (int)(device))

int armenv_probe_issue_rate(int32_t device, int32_t precision, int32_t waves_per_simd, double *ns_per_instruction) {
  DEV_ENTER(device);
  if (!ns_per_instruction || waves_per_simd < 1 || waves_per_simd > 8 || (precision != 32 && precision != 64))
    return fail(ARMENV_EINVAL, "armenv_probe_issue_rate: precision 32 | 64, 1..8 waves per SIMD");
  return precision == 64 ? issue_probe<double>(device, waves_per_simd, ns_per_instruction) : issue_probe<float>(device, waves_per_simd, ns_per_instruction);
}

}  // extern "C"

static HerArgs her_args(const ArmEnvHerArgs *a) {
  HerArgs h;
  h.T = a->T; h.N = a->N; h.ring_base = a->ring_base; h.ring_cap = a->ring_cap; h.D = a->obs_dim;
  h.obs0 = a->obs0_dev; h.obs_after = a->obs_after_dev; h.next_obs = a->next_obs_dev; h.action = a->action_dev;
  h.reward = a->reward_dev; h.done = a->done_dev; h.episodes = a->episodes_dev; h.num_episodes = a->num_episodes_dev;
  h.B = a->batch; h.picks_in = a->picks_dev; h.seed = a->seed; h.draw = a->draw; h.use_her = a->use_her;
  h.her_ratio = a->her_ratio; h.dis_threshold = a->dis_threshold;
  h.states = a->states_dev; h.actions = a->actions_dev; h.next_states = a->next_states_dev; h.rewards = a->rewards_dev;
  h.dones = a->dones_dev; h.picks_out = a->picks_out_dev;
  return h;
}

extern "C" {

// ---- the trajectory store.  All seven entry points refuse a bad argument by its name before the first HIP call, return ARMENV_OK
// without a launch for an empty batch, then launch their own kernel form.  One set of checks: the single forms are members = 1.
#define STORE_REFUSE(why) \
  if (const char *why_ = (why)) return fail(ARMENV_EINVAL, "%s: %s", __func__, why_)

// what is wrong with the geometry of an index pass and the pointers it reads: the first broken field, or nullptr.  The count pass
// reads neither offsets_dev nor episodes_dev (write = false).
static const char *index_refusal(int32_t members, int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap, const void *done_dev,
                                 const void *counts_dev, bool write = false, const void *offsets_dev = nullptr,
                                 const void *episodes_dev = nullptr, int64_t episodes_stride = 1) {
  if (members < 1 || members > 64) return "members must be 1..64";
  if (T < 0) return "T must be >= 0";
  if (N < 1) return "N must be >= 1";
  if (ring_cap < 1 || ring_cap < T) return "ring_cap must be >= max(T, 1)";
  if (ring_base < 0) return "ring_base must be >= 0";
  if (!done_dev) return "done_dev is NULL";
  if (!counts_dev) return "counts_dev is NULL";
  if (write && !offsets_dev) return "offsets_dev is NULL";
  if (write && !episodes_dev) return "episodes_dev is NULL";
  if (write && episodes_stride < 1) return "episodes_stride must be >= 1";
  return nullptr;
}

// the same for the arguments of a sample; `pop`: the population struct around `a`, or nullptr
static const char *her_refusal(const ArmEnvHerArgs *a, const ArmEnvHerPopArgs *pop = nullptr) {
  if (!a) return "args is NULL";
  if (pop && (pop->members < 1 || pop->members > 64)) return "members must be 1..64";
  if (pop && pop->episodes_stride < 1) return "episodes_stride must be >= 1";
  if (a->obs_dim != 6 && a->obs_dim != 9) return "obs_dim must be 6 or 9";
  if (a->batch < 0) return "batch must be >= 0";
  if (a->T < 1) return "T must be >= 1";
  if (a->N < 1) return "N must be >= 1";
  if (a->ring_cap < a->T) return "ring_cap must be >= T";
  if (a->ring_base < 0) return "ring_base must be >= 0";
#define NEEDS(field) if (!a->field) return #field " is NULL"
  NEEDS(obs0_dev); NEEDS(obs_after_dev); NEEDS(next_obs_dev); NEEDS(action_dev); NEEDS(reward_dev); NEEDS(done_dev);
  NEEDS(episodes_dev); NEEDS(num_episodes_dev); NEEDS(states_dev); NEEDS(actions_dev); NEEDS(next_states_dev); NEEDS(rewards_dev);
  NEEDS(dones_dev);
#undef NEEDS
  if (!(a->her_ratio >= 0.0 && a->her_ratio <= 1.0)) return "her_ratio outside [0,1]";
  return nullptr;
}

int armenv_count_episodes(int32_t device, int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap, const uint8_t *done_dev,
                          int32_t starts_at_reset, int32_t *counts_dev, void *stream) {
  STORE_REFUSE(index_refusal(1, T, N, ring_base, ring_cap, done_dev, counts_dev));
  DEV_ENTER(device);
  hipLaunchKernelGGL(index_episodes_kernel, dim3(grid_for(N, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), T, N,
                     ring_base, ring_cap, done_dev, starts_at_reset, counts_dev, (const int64_t *)nullptr, (int32_t *)nullptr);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int armenv_write_episodes(int32_t device, int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap, const uint8_t *done_dev,
                          int32_t starts_at_reset, const int32_t *counts_dev, const int64_t *offsets_dev,
                          int32_t *episodes_dev, void *stream) {
  STORE_REFUSE(index_refusal(1, T, N, ring_base, ring_cap, done_dev, counts_dev, true, offsets_dev, episodes_dev));
  DEV_ENTER(device);
  hipLaunchKernelGGL(index_episodes_kernel, dim3(grid_for(N, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), T, N,
                     ring_base, ring_cap, done_dev, starts_at_reset, const_cast<int32_t *>(counts_dev), offsets_dev, episodes_dev);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int armenv_her_sample(int32_t device, const ArmEnvHerArgs *a, void *stream) {
  STORE_REFUSE(her_refusal(a));
  if (a->batch == 0) return ARMENV_OK;
  DEV_ENTER(device);
  const HerArgs h = her_args(a);
  const dim3 grid(grid_for(a->batch, 256)), block(256);
  if (a->obs_dim == 6) hipLaunchKernelGGL((her_sample_kernel<6>), grid, block, 0, static_cast<hipStream_t>(stream), h);
  else hipLaunchKernelGGL((her_sample_kernel<9>), grid, block, 0, static_cast<hipStream_t>(stream), h);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int armenv_pop_count_episodes(int32_t device, int32_t members, int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap,
                              const uint8_t *done_dev, int32_t starts_at_reset, int32_t *counts_dev, void *stream) {
  STORE_REFUSE(index_refusal(members, T, N, ring_base, ring_cap, done_dev, counts_dev));
  DEV_ENTER(device);
  hipLaunchKernelGGL(index_episodes_pop_kernel, dim3(grid_for(N, 256), members), dim3(256), 0, static_cast<hipStream_t>(stream), T, N,
                     ring_base, ring_cap, done_dev, starts_at_reset, counts_dev, (const int64_t *)nullptr, (int32_t *)nullptr,
                     members, (int64_t)0);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int armenv_pop_write_episodes(int32_t device, int32_t members, int64_t T, int64_t N, int64_t ring_base, int64_t ring_cap,
                              const uint8_t *done_dev, int32_t starts_at_reset, const int32_t *counts_dev,
                              const int64_t *offsets_dev, int32_t *episodes_dev, int64_t episodes_stride, void *stream) {
  STORE_REFUSE(index_refusal(members, T, N, ring_base, ring_cap, done_dev, counts_dev, true, offsets_dev, episodes_dev, episodes_stride));
  DEV_ENTER(device);
  hipLaunchKernelGGL(index_episodes_pop_kernel, dim3(grid_for(N, 256), members), dim3(256), 0, static_cast<hipStream_t>(stream), T, N,
                     ring_base, ring_cap, done_dev, starts_at_reset, const_cast<int32_t *>(counts_dev), offsets_dev, episodes_dev,
                     members, episodes_stride);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int armenv_her_pop_sample(int32_t device, const ArmEnvHerPopArgs *args, void *stream) {
  STORE_REFUSE(her_refusal(args ? &args->one : nullptr, args));
  const ArmEnvHerArgs *a = &args->one;
  if (a->batch == 0) return ARMENV_OK;
  DEV_ENTER(device);
  const HerArgs h = her_args(a);
  const dim3 grid(grid_for(a->batch, 256), args->members), block(256);
  if (a->obs_dim == 6)
    hipLaunchKernelGGL((her_sample_pop_kernel<6>), grid, block, 0, static_cast<hipStream_t>(stream), h, args->members, args->episodes_stride);
  else
    hipLaunchKernelGGL((her_sample_pop_kernel<9>), grid, block, 0, static_cast<hipStream_t>(stream), h, args->members, args->episodes_stride);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}

int armenv_her_pop_sample_shared(int32_t device, const ArmEnvHerPopSharedArgs *args, void *stream) {
  STORE_REFUSE(her_refusal(args ? &args->pop.one : nullptr, args ? &args->pop : nullptr));
  STORE_REFUSE(args->share_ratio >= 0.0 && args->share_ratio <= 1.0 ? nullptr : "share_ratio outside [0,1]");
  const ArmEnvHerArgs *a = &args->pop.one;
  if (a->batch == 0) return ARMENV_OK;
  DEV_ENTER(device);
  const HerArgs h = her_args(a);
  const dim3 grid(grid_for(a->batch, 256), args->pop.members), block(256);
  if (a->obs_dim == 6)
    hipLaunchKernelGGL((her_sample_pop_shared_kernel<6>), grid, block, 0, static_cast<hipStream_t>(stream), h, args->pop.members,
                       args->pop.episodes_stride, args->share_ratio);
  else
    hipLaunchKernelGGL((her_sample_pop_shared_kernel<9>), grid, block, 0, static_cast<hipStream_t>(stream), h, args->pop.members,
                       args->pop.episodes_stride, args->share_ratio);
  HIP_TRY(hipGetLastError());
  return ARMENV_OK;
}
#undef STORE_REFUSE

int64_t armenv_num_envs(const ArmEnv *env) { return env ? env->cfg.num_envs : 0; }
int32_t armenv_obs_dim(const ArmEnv *env) { return env ? (env->cfg.task == ARMENV_TASK_REACH ? 6 : 9) : 0; }
int32_t armenv_aux_dim(const ArmEnv *env) {
  if (!env) return 0;
  return env->cfg.task == ARMENV_TASK_PUSH ? 10 : (env->cfg.task == ARMENV_TASK_PICK ? 12 : 0);
}
int32_t armenv_action_dim(const ArmEnv *) { return 3; }
const char *armenv_kernel_name(const ArmEnv *env) { return env ? env->eng->name() : ""; }

}  // extern "C"
