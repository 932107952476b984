// Runs the TASK_SOCCER output stage of csrc/dmc_kernels.hip on the host under
// sanitizers, one OS thread per lane (shim.h): the team source (-DDMC_TEAM=<lanes>)
// or the same source with TEAM = 1.  One dmc_observe over the batch, then one
// dmc_step of <nsub> substeps under new controls; every field is a heap block of
// exactly its size, so an index past the row is a report.  tests/test_soccer_fused.py
// compares what is printed with the host formulas of locomotion/soccer.
// TEST INFRASTRUCTURE ONLY.
//   stdin: <nenv> <nsub>, then per env: <qpos> <qvel> <stored ctrl> <new ctrl>
//   stdout: OBSERVE|STEPPED <env> <qpos> | <qvel> | <obs> | <reward> | <return> |
//           <stored ctrl> | <warn>
#include "shim.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include DMC_KERNEL_SOURCE

#ifndef DMC_TASK_SOCCER
#error "soccer_harness.cpp needs a TASK_SOCCER model header"
#endif
static_assert(TEAM == SHIM_GROUP, "shim.h and the kernel source disagree on the team");
constexpr int WS_PER_ENV = WS_WORDS > 0 ? WS_WORDS : 1;
constexpr double SENTINEL = -777.25;

static DmcArgs g_args;
static void (*g_kernel)(DmcArgs);
static unsigned g_block;
static void* lane_main(void* arg) {
  threadIdx.x = (unsigned)(size_t)arg;
  blockIdx.x = g_block;
  g_kernel(g_args);
  return nullptr;
}
// one env per workgroup of TEAM lanes (blockDim.x = TEAM: env e is block e)
static void launch(void (*kernel)(DmcArgs), int n) {
  g_kernel = kernel;
  pthread_attr_t attr;
  pthread_attr_init(&attr);
  pthread_attr_setstacksize(&attr, 64u << 20);
  for (int b = 0; b < n; b++) {
    g_block = (unsigned)b;
    pthread_t th[TEAM];
    for (size_t i = 0; i < TEAM; i++) pthread_create(&th[i], &attr, lane_main, (void*)i);
    for (int i = 0; i < TEAM; i++) pthread_join(th[i], nullptr);
  }
}
static real* field(size_t words) {
  real* p = new real[words];
  for (size_t i = 0; i < words; i++) p[i] = (real)SENTINEL;
  return p;
}
static void print(const real* p, int K, int e, int n, const char* sep) {
  for (int k = 0; k < K; k++) printf(" %.17g", (double)p[(size_t)k*n + e]);
  printf("%s", sep);
}

int main() {
  int n, nsub;
  if (scanf("%d %d", &n, &nsub) != 2 || n < 1 || nsub < 1) {
    fprintf(stderr, "expected <nenv> <nsub>\n");
    return 2;
  }
  DmcArgs& a = g_args;
  memset(&a, 0, sizeof a);
  a.nenv = n; a.nsub = nsub;
  a.qpos = field((size_t)NQX*n); a.qvel = field((size_t)NVX*n); a.warm = field((size_t)NVX*n);
  a.ctrl_store = field((size_t)NUX*n); a.time = field(n); a.episode_return = field(n);
  a.reward = field(n); a.obs = field((size_t)NOBS*n); a.obs_sk = 1; a.obs_se = NOBS;
  a.ws = field((size_t)WS_PER_ENV*n);
  a.warn = new unsigned[n]; a.stats = new int[3*(size_t)n];
  real* ctrl = field((size_t)NUX*n);          // the new controls, [env][NU]
  for (int e = 0; e < n; e++) {
    double x;
    a.warn[e] = 0; a.time[e] = 0; a.episode_return[e] = 0;
    for (int k = 0; k < 3; k++) a.stats[(size_t)k*n + e] = 0;
    for (int i = 0; i < NQ; i++) { if (scanf("%lf", &x) != 1) return 2; a.qpos[(size_t)i*n + e] = (real)x; }
    for (int i = 0; i < NV; i++) {
      if (scanf("%lf", &x) != 1) return 2;
      a.qvel[(size_t)i*n + e] = (real)x; a.warm[(size_t)i*n + e] = 0;
    }
    for (int i = 0; i < NU; i++) { if (scanf("%lf", &x) != 1) return 2; a.ctrl_store[(size_t)i*n + e] = (real)x; }
    for (int i = 0; i < NU; i++) { if (scanf("%lf", &x) != 1) return 2; ctrl[(size_t)e*NU + i] = (real)x; }
  }
  blockDim.x = TEAM;
  pthread_barrier_init(&shim_teams[0].bar, nullptr, SHIM_GROUP);
  pthread_barrier_init(&shim_block_barrier, nullptr, TEAM);
  for (int pass = 0; pass < 2; pass++) {
    if (pass) { a.flags = DMC_FLAG_CTRL; a.ctrl = ctrl; a.ctrl_sk = 1; a.ctrl_se = NU; }
    launch(pass ? dmc_step : dmc_observe, n);
    for (int e = 0; e < n; e++) {
      printf("%s %d", pass ? "STEPPED" : "OBSERVE", e);
      print(a.qpos, NQ, e, n, " |"); print(a.qvel, NV, e, n, " |");
      for (int k = 0; k < NOBS; k++) printf(" %.17g", (double)a.obs[k*a.obs_sk + e*a.obs_se]);
      printf(" |"); print(a.reward + e, 1, 0, 1, " |"); print(a.episode_return + e, 1, 0, 1, " |");
      print(a.ctrl_store, NU, e, n, " |");
      printf(" %u\n", a.warn[e]);
    }
  }
  return 0;
}
