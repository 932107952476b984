// Runs dmc_step of the included kernel source for ONE workgroup on the host
// under sanitizers, one OS thread per lane (shim.h), and prints every env's
// qpos/qvel and counters after each step (tests/shim_runner.py compares them
// with the oracle).  TEST INFRASTRUCTURE ONLY.
//   stdin: <steps> <nsub>, then per env: <model-parameter block> <qpos> <qvel> <ctrl>
//   stdout: STEP <t> <env> <qpos> <qvel> | <ncon> <nefc> <iters> <warn>
// `harness init`: one launch of dmc_init_episode over a batch of any size, every
// field in a heap block of its own of exactly the unpadded size, pre-filled with
// INIT_SENTINEL (tests/shim_runner.py compares with tests/device_init_model.py).
//   stdin: <nenv> <seed> <flags> <task_param_i> [per env: <ncon> for the stats column]
//   stdout: INIT <env> <qpos> | <qvel> | <warm> | <ctrl> | <time> | <return> |
//           <taskdata> | <model-parameter block>
// `harness observe`: dmc_observe over a batch of any size, workgroup after
// workgroup, then one dmc_step of <nsub> substeps under the stored controls,
// every field in a heap block of exactly its size (tests/shim_runner.py compares
// both with tests/output_model.py).  One env per lane: the lanes of a workgroup
// that have an env are one OS thread each, so the transposed observation store
// runs with a partial block.  <layout> 0: the observation in the agent layout
// [env][k]; 1: [k][env] through the explicit strides.
//   stdin: <nenv> <nsub> <task_param_i> <task_param_r0> <layout>, then per env:
//          <qpos> <qvel> <ctrl> <taskdata>
//   stdout: OBSERVE|STEPPED <env> <qpos> | <qvel> | <obs> | <reward> |
//           <sensordata> | <xpos> | <xmat> | <warn>
#include "shim.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include DMC_KERNEL_SOURCE

// The shape, from what the kernel source defines: the envs of one workgroup of
// dmc_coop.hip (G lanes each, which never use the workspace: one word per env),
// else one env, advanced by one lane or by the TEAM lanes of team mode.
#ifdef DMC_COOP_BUILD
constexpr int HARNESS_ENVS = EPB, HARNESS_LANES = NTHREADS, HARNESS_WS = EPB;
static_assert(G == SHIM_GROUP, "shim.h and the kernel source disagree on the group");
#else
constexpr int HARNESS_ENVS = 1, HARNESS_LANES = TEAM, HARNESS_WS = WS_WORDS > 0 ? WS_WORDS : 1;
static_assert(TEAM == SHIM_GROUP, "shim.h and the kernel source disagree on the team");
#endif
constexpr int NMP = DMC_NMODELPARAM;
// observe mode: envs and lanes of a workgroup as the device launches it, and
// the workspace words an env owns
#ifdef DMC_COOP_BUILD
constexpr int HARNESS_ENVS_PER_BLOCK = EPB, HARNESS_BLOCK_LANES = NTHREADS, HARNESS_WS_PER_ENV = 1;
#else
constexpr int HARNESS_ENVS_PER_BLOCK = 64, HARNESS_BLOCK_LANES = 64,
              HARNESS_WS_PER_ENV = WS_WORDS > 0 ? WS_WORDS : 1;
#endif

static DmcArgs g_args;
static void* lane_main(void* arg) {
  threadIdx.x = (unsigned)(size_t)arg;
  blockIdx.x = 0;
  dmc_step(g_args);
  return nullptr;
}

// --------------------------------------------------------------------------
// init mode
// --------------------------------------------------------------------------
constexpr double INIT_SENTINEL = -777.25;
// the layout of a 2-D field as DESIGN.md 2 states it, not through the kernel's sidx
static size_t init_at(int k, int e, int n, int K) {
  return DMC_ENV_MAJOR ? (size_t)e*K + k : (size_t)k*n + e;
}
static real* init_field(size_t words) {
  real* p = new real[words];       // exactly `words`: one past the end is a report
  for (size_t i = 0; i < words; i++) p[i] = (real)INIT_SENTINEL;
  return p;
}
static void init_print(const real* p, int K, int e, int n, const char* sep) {
  for (int k = 0; k < K; k++)
    printf(" %.17g", (double)p[init_at(k, e, n, K > 0 ? K : 1)]);
  printf("%s", sep);
}

static int init_main() {
  int n, flags, param;
  unsigned long long seed;
  if (scanf("%d %llu %d %d", &n, &seed, &flags, &param) != 4 || n < 1) {
    fprintf(stderr, "expected <nenv> <seed> <flags> <task_param_i>\n");
    return 2;
  }
  int* stats = new int[3*(size_t)n];
  for (int i = 0; i < 3*n; i++) stats[i] = 0;
  for (int e = 0, ncon; e < n && scanf("%d", &ncon) == 1; e++) stats[init_at(0, e, n, 3)] = ncon;
  DmcArgs a;
  memset(&a, 0, sizeof a);
  a.nenv = n; a.nsub = 1; a.flags = flags; a.task_param_i = param; a.seed = seed;
  a.qpos = init_field((size_t)NQX*n); a.qvel = init_field((size_t)NVX*n);
  a.warm = init_field((size_t)NVX*n); a.ctrl_store = init_field((size_t)NUX*n);
  a.time = init_field(n); a.episode_return = init_field(n);
  a.taskdata = init_field((size_t)NTDX*n);
  if (NMP > 0) a.modelparam = init_field((size_t)NMP*n);
  a.stats = stats;
  // one env per lane of 64-lane workgroups; the kernel has no barrier, so the
  // lanes run one after the other on this thread
  for (int b = 0; b < (n + 63)/64; b++)
    for (int t = 0; t < 64; t++) {
      blockIdx.x = (unsigned)b; threadIdx.x = (unsigned)t;
      dmc_init_episode(a);
    }
  for (int e = 0; e < n; e++) {
    printf("INIT %d", e);
    init_print(a.qpos, NQ, e, n, " |"); init_print(a.qvel, NV, e, n, " |");
    init_print(a.warm, NV, e, n, " |"); init_print(a.ctrl_store, NU, e, n, " |");
    init_print(a.time + e, 1, 0, 1, " |"); init_print(a.episode_return + e, 1, 0, 1, " |");
    init_print(a.taskdata, NTASKDATA, e, n, " |");
    if (NMP > 0) init_print(a.modelparam, NMP, e, n, "");
    printf("\n");
  }
  return 0;
}

// --------------------------------------------------------------------------
// observe mode
// --------------------------------------------------------------------------
static void (*g_kernel)(DmcArgs);
static unsigned g_block;
static void* observe_lane(void* arg) {
  threadIdx.x = (unsigned)(size_t)arg;
  blockIdx.x = g_block;
  g_kernel(g_args);
  return nullptr;
}
// one workgroup after the other; of the one-env-per-lane source only the lanes
// that have an env (the others leave before the first barrier on the device too)
static void observe_launch(void (*kernel)(DmcArgs), int n) {
  g_kernel = kernel;
  const int blocks = (n + HARNESS_ENVS_PER_BLOCK - 1)/HARNESS_ENVS_PER_BLOCK;
  for (int b = 0; b < blocks; b++) {
    int lanes = HARNESS_BLOCK_LANES;
    if (HARNESS_ENVS_PER_BLOCK == 64 && n - 64*b < 64) lanes = n - 64*b;
    pthread_barrier_init(&shim_block_barrier, nullptr, lanes);
    g_block = (unsigned)b;
    std::vector<pthread_t> th(lanes);
    for (size_t i = 0; i < (size_t)lanes; i++) pthread_create(&th[i], nullptr, observe_lane, (void*)i);
    for (int i = 0; i < lanes; i++) pthread_join(th[i], nullptr);
    pthread_barrier_destroy(&shim_block_barrier);
  }
}

static int observe_main() {
  int n, nsub, param, layout;
  double param_r;
  if (scanf("%d %d %d %lf %d", &n, &nsub, &param, &param_r, &layout) != 5 || n < 1 || NMP > 0 ||
      TEAMED || n % (HARNESS_ENVS_PER_BLOCK == 64 ? 1 : HARNESS_ENVS_PER_BLOCK)) {
    fprintf(stderr, "expected <nenv> <nsub> <task_param_i> <task_param_r0> <layout> "
            "(whole workgroups of a several-lanes build; no team, no model-parameter block)\n");
    return 2;
  }
  constexpr int NSD = NSENSORDATA > 0 ? NSENSORDATA : 1, NOB = NOBS > 0 ? NOBS : 1;
  DmcArgs& a = g_args;
  memset(&a, 0, sizeof a);
  a.nenv = n; a.nsub = nsub; a.task_param_i = param; a.task_param_r[0] = param_r;
  a.qpos = init_field((size_t)NQX*n); a.qvel = init_field((size_t)NVX*n);
  a.warm = init_field((size_t)NVX*n); a.ctrl_store = init_field((size_t)NUX*n);
  a.time = init_field(n); a.episode_return = init_field(n); a.reward = init_field(n);
  a.taskdata = init_field((size_t)NTDX*n);
  a.obs = init_field((size_t)NOB*n);
  a.obs_sk = layout ? n : 1; a.obs_se = layout ? 1 : NOBS;
  a.sensordata = init_field((size_t)NSD*n);
  a.xpos = init_field((size_t)NBODY*3*n); a.xmat = init_field((size_t)NBODY*9*n);
  a.ws = init_field((size_t)HARNESS_WS_PER_ENV*n);
  a.warn = new unsigned[n]; a.stats = new int[3*(size_t)n];
  for (int e = 0; e < n; e++) {
    double x;
    a.warn[e] = 0; a.time[e] = 0; a.episode_return[e] = 0;
    for (int k = 0; k < 3; k++) a.stats[init_at(k, e, n, 3)] = 0;
    for (int i = 0; i < NQ; i++) { if (scanf("%lf", &x) != 1) return 2; a.qpos[init_at(i, e, n, NQX)] = (real)x; }
    for (int i = 0; i < NV; i++) {
      if (scanf("%lf", &x) != 1) return 2;
      a.qvel[init_at(i, e, n, NVX)] = (real)x; a.warm[init_at(i, e, n, NVX)] = 0;
    }
    for (int i = 0; i < NU; i++) { if (scanf("%lf", &x) != 1) return 2; a.ctrl_store[init_at(i, e, n, NUX)] = (real)x; }
    for (int i = 0; i < NTASKDATA; i++) { if (scanf("%lf", &x) != 1) return 2; a.taskdata[init_at(i, e, n, NTDX)] = (real)x; }
  }
  for (int t = 0; t < 128/SHIM_GROUP; t++) pthread_barrier_init(&shim_teams[t].bar, nullptr, SHIM_GROUP);
  for (int pass = 0; pass < 2; pass++) {
    observe_launch(pass ? dmc_step : dmc_observe, n);
    for (int e = 0; e < n; e++) {
      printf("%s %d", pass ? "STEPPED" : "OBSERVE", e);
      init_print(a.qpos, NQ, e, n, " |"); init_print(a.qvel, NV, e, n, " |");
      for (int k = 0; k < NOBS; k++) printf(" %.17g", (double)a.obs[k*a.obs_sk + e*a.obs_se]);
      printf(" |"); init_print(a.reward + e, 1, 0, 1, " |");
      init_print(a.sensordata, NSENSORDATA, e, n, " |");
      init_print(a.xpos, NBODY*3, e, n, " |"); init_print(a.xmat, NBODY*9, e, n, " |");
      printf(" %u\n", a.warn[e]);
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "init")) return init_main();
  if (argc > 1 && !strcmp(argv[1], "observe")) return observe_main();
  const int n = HARNESS_ENVS;
  const int nq = NQ > 0 ? NQ : 1, nv = NV > 0 ? NV : 1, nu = NU > 0 ? NU : 1;
  std::vector<real> qpos(nq*n), qvel(nv*n), warm(nv*n, 0), tm(n, 0), ctrl(nu*n),
      obs((NOBS > 0 ? NOBS : 1)*n), rew(n), ret(n, 0),
      sens((NSENSORDATA > 0 ? NSENSORDATA : 1)*n), xpos(NBODY*3*n), xmat(NBODY*9*n),
      qacc(nv*n), ws(HARNESS_WS), mp(NMP*n);
  std::vector<unsigned> warn(n, 0);
  std::vector<int> stats(3*n, 0);
  std::vector<double> in;
  for (double x; scanf("%lf", &x) == 1;) in.push_back(x);
  const size_t expected = 2 + (size_t)n*(NMP + NQ + NV + NU);
  if (in.size() != expected || !feof(stdin)) {
    fprintf(stderr, "expected %zu numbers (steps nsub, then for each of %d envs %d block + %d qpos + "
            "%d qvel + %d ctrl), got %zu\n", expected, n, NMP, NQ, NV, NU, in.size());
    return 2;
  }
  const int steps = (int)in[0];
  const double* at = in.data() + 2;
  // several-lanes-per-env code objects keep the state env-major: [env][k]
  for (int e = 0; e < n; e++) {
    for (int i = 0; i < NMP; i++) mp[e*NMP + i] = (real)*at++;
    for (int i = 0; i < NQ; i++) qpos[e*nq + i] = (real)*at++;
    for (int i = 0; i < NV; i++) qvel[e*nv + i] = (real)*at++;
    for (int i = 0; i < NU; i++) ctrl[e*nu + i] = (real)*at++;   // constant: re-applied from ctrl_store
  }
  DmcArgs& a = g_args;
  memset(&a, 0, sizeof a);
  a.nenv = n; a.nsub = (int)in[1]; a.flags = 0;
  a.qpos = qpos.data(); a.qvel = qvel.data(); a.warm = warm.data(); a.time = tm.data();
  a.ctrl_store = ctrl.data(); a.obs = obs.data(); a.obs_sk = 1; a.obs_se = NOBS;
  a.reward = rew.data(); a.episode_return = ret.data(); a.sensordata = sens.data();
  a.xpos = xpos.data(); a.xmat = xmat.data(); a.qacc = qacc.data();
  a.warn = warn.data(); a.stats = stats.data(); a.ws = ws.data();
  if (NMP > 0) a.modelparam = mp.data();   // else null: a default build that read the block faults
  if (TEAMED) blockDim.x = TEAM;
  for (int t = 0; t < HARNESS_LANES/SHIM_GROUP; t++)
    pthread_barrier_init(&shim_teams[t].bar, nullptr, SHIM_GROUP);
  pthread_barrier_init(&shim_block_barrier, nullptr, HARNESS_LANES);
  pthread_attr_t attr;
  pthread_attr_init(&attr);
  if (TEAMED) pthread_attr_setstacksize(&attr, 256u << 20);     // the per-lane arrays of a big scene
  for (int t = 0; t < steps; t++) {
    if (HARNESS_LANES == 1) {
      lane_main(nullptr);
    } else {
      pthread_t th[HARNESS_LANES];
      for (size_t i = 0; i < HARNESS_LANES; i++) pthread_create(&th[i], &attr, lane_main, (void*)i);
      for (int i = 0; i < HARNESS_LANES; i++) pthread_join(th[i], nullptr);
    }
    for (int e = 0; e < n; e++) {
      printf("STEP %d %d", t, e);
      for (int i = 0; i < NQ; i++) printf(" %.17g", (double)qpos[e*nq + i]);
      for (int i = 0; i < NV; i++) printf(" %.17g", (double)qvel[e*nv + i]);
      printf(" | %d %d %d %u\n", stats[3*e], stats[3*e + 1], stats[3*e + 2], warn[e]);
    }
  }
  return 0;
}
