// Runs dmc_init_episode and dmc_step of the included kernel source on the host
// under sanitizers with the per-env episode contract of csrc/dmc_args.h switched
// on: an env mask, step counters and done flags (tests/test_episodes.py).  A
// stand-alone program like harness.cpp, which keeps meaning "a zero-filled
// block"; this one fills the members at the end of DmcArgs.  TEST INFRASTRUCTURE ONLY.
//
// `episode_harness init`: one launch of dmc_init_episode, every field a heap block
// of exactly nenv envs filled with INIT_SENTINEL, the episode block and the warning
// mask filled with INT_SENTINEL.
//   stdin: <nenv> <seed> <flags> <task_param_i>, then per env: <ncon> <mask>
//   stdout: INIT <env> <qpos> | <qvel> | <warm> | <ctrl> | <time> | <return> |
//           <taskdata> | <model-parameter block> | <ep_step> <ep_done> <warn>
// `episode_harness step`: <steps> launches of dmc_step over nenv envs, one OS
// thread per lane, workgroup after workgroup.  A lane that leaves the kernel
// leaves the workgroup's barrier too (on the device a wavefront's barrier counts
// the lanes that are still there), so a launch in which the lanes that stay
// wait for one that left would hang here: run with a timeout.
//   stdin: <nenv> <steps> <nsub> <flags> <step_limit>, then per env:
//          <mask> <ep_step> <ep_done> <model-parameter block> <qpos> <qvel> <ctrl>
//   stdout: STEP <t> <env> <qpos> <qvel> | <ncon> <nefc> <iters> <warn> |
//           <ep_step> <ep_done> | <every word of the env in every array>
//           (t = -1: before the first launch)
#include "shim.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

// a barrier over the lanes of the workgroup that are still in the kernel
struct LeaveBarrier {
  pthread_mutex_t m = PTHREAD_MUTEX_INITIALIZER;
  pthread_cond_t c = PTHREAD_COND_INITIALIZER;
  int parties = 0, waiting = 0;
  unsigned generation = 0;
  void open() { waiting = 0; generation++; pthread_cond_broadcast(&c); }
  void wait() {
    pthread_mutex_lock(&m);
    if (++waiting == parties) open();
    else for (const unsigned g = generation; g == generation;) pthread_cond_wait(&c, &m);
    pthread_mutex_unlock(&m);
  }
  void leave() {
    pthread_mutex_lock(&m);
    if (--parties > 0 && waiting == parties) open();
    pthread_mutex_unlock(&m);
  }
};
static LeaveBarrier episode_barrier;
static inline void episode_syncthreads() { episode_barrier.wait(); }
#define __syncthreads episode_syncthreads

// block_ballot of the one-env-per-lane source over this program's threads
#define DMC_SHIM_BLOCK_BALLOT 1
static unsigned char episode_votes[64];
static inline unsigned long long block_ballot(bool p) {
  episode_votes[threadIdx.x] = p;
  __syncthreads();
  unsigned long long live = 0;
  for (int i = 0; i < 64; i++) live |= (unsigned long long)(episode_votes[i] != 0) << i;
  __syncthreads();       // every lane has read the votes before the next ballot
  return live;
}

#include DMC_KERNEL_SOURCE

#ifdef DMC_COOP_BUILD
constexpr int BLOCK_ENVS = EPB, BLOCK_LANES = NTHREADS;
static_assert(G == SHIM_GROUP, "shim.h and the kernel source disagree on the group");
#else
constexpr int BLOCK_ENVS = 64, BLOCK_LANES = 64;
static_assert(!TEAMED, "team mode takes no env mask");
// the masked observation store under test is the one that transposes through LDS
#ifdef EPISODE_EXPECT_OBS_STAGE
static_assert(OBS_STAGE_FITS, "build with an LDS budget that holds the observation stage");
#endif
#endif
static_assert(EPISODE_CAPS == (DMC_FLAG_MASKED | DMC_FLAG_EPISODES | DMC_FLAG_ZERO_TIME),
              "the kernel source honours the episode flags");
constexpr int NMP = DMC_NMODELPARAM;
constexpr double INIT_SENTINEL = -777.25;
constexpr int INT_SENTINEL = 7777;

// the layout of a 2-D field as DESIGN.md 2 states it, not through the kernel's sidx
static size_t at(int k, int e, int n, int K) {
  return DMC_ENV_MAJOR ? (size_t)e*K + k : (size_t)k*n + e;
}
static real* field(size_t words) {
  real* p = new real[words];       // exactly `words`: one past the end is a report
  for (size_t i = 0; i < words; i++) p[i] = (real)INIT_SENTINEL;
  return p;
}
template <class T>
static T* ints(size_t words) {
  T* p = new T[words];
  for (size_t i = 0; i < words; i++) p[i] = (T)INT_SENTINEL;
  return p;
}
static void print(const real* p, int K, int e, int n, const char* sep) {
  for (int k = 0; k < K; k++) printf(" %.17g", (double)p[at(k, e, n, K > 0 ? K : 1)]);
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
  int* mask = new int[n];
  for (int e = 0; e < n; e++) {
    int ncon;
    if (scanf("%d %d", &ncon, &mask[e]) != 2) { fprintf(stderr, "expected <ncon> <mask> per env\n"); return 2; }
    stats[at(0, e, n, 3)] = ncon;
  }
  DmcArgs a;
  memset(&a, 0, sizeof a);
  a.nenv = n; a.nsub = 1; a.flags = flags; a.task_param_i = param; a.seed = seed;
  a.qpos = field((size_t)NQX*n); a.qvel = field((size_t)NVX*n);
  a.warm = field((size_t)NVX*n); a.ctrl_store = field((size_t)NUX*n);
  a.time = field(n); a.episode_return = field(n);
  a.taskdata = field((size_t)NTDX*n);
  if (NMP > 0) a.modelparam = field((size_t)NMP*n);
  a.stats = stats;
  a.env_mask = mask; a.ep_step = ints<int>(n); a.ep_done = ints<int>(n); a.warn = ints<unsigned>(n);
  for (int b = 0; b < (n + 63)/64; b++)
    for (int t = 0; t < 64; t++) {       // (the kernel has no barrier: lane after lane)
      blockIdx.x = (unsigned)b; threadIdx.x = (unsigned)t;
      dmc_init_episode(a);
    }
  for (int e = 0; e < n; e++) {
    printf("INIT %d", e);
    print(a.qpos, NQ, e, n, " |"); print(a.qvel, NV, e, n, " |");
    print(a.warm, NV, e, n, " |"); print(a.ctrl_store, NU, e, n, " |");
    print(a.time + e, 1, 0, 1, " |"); print(a.episode_return + e, 1, 0, 1, " |");
    print(a.taskdata, NTASKDATA, e, n, " |");
    if (NMP > 0) print(a.modelparam, NMP, e, n, "");
    printf(" | %d %d %u\n", a.ep_step[e], a.ep_done[e], a.warn[e]);
  }
  return 0;
}

static DmcArgs g_args;
static unsigned g_block;
static void* lane_main(void* arg) {
  threadIdx.x = (unsigned)(size_t)arg;
  blockIdx.x = g_block;
  dmc_step(g_args);
  episode_barrier.leave();
  return nullptr;
}

static int step_main() {
  int n, steps, nsub, flags, limit;
  if (scanf("%d %d %d %d %d", &n, &steps, &nsub, &flags, &limit) != 5 || n < 1) {
    fprintf(stderr, "expected <nenv> <steps> <nsub> <flags> <step_limit>\n");
    return 2;
  }
  const int nq = NQ > 0 ? NQ : 1, nv = NV > 0 ? NV : 1, nu = NU > 0 ? NU : 1,
            nobs = NOBS > 0 ? NOBS : 1, nsd = NSENSORDATA > 0 ? NSENSORDATA : 1;
  DmcArgs& a = g_args;
  memset(&a, 0, sizeof a);
  a.nenv = n; a.nsub = nsub; a.flags = flags; a.step_limit = limit;
  real *qpos = field((size_t)nq*n), *qvel = field((size_t)nv*n), *warm = field((size_t)nv*n),
       *tm = field(n), *ctrl = field((size_t)nu*n), *obs = field((size_t)nobs*n), *rew = field(n),
       *ret = field(n), *sens = field((size_t)nsd*n), *xpos = field((size_t)NBODY*3*n),
       *xmat = field((size_t)NBODY*9*n), *qacc = field((size_t)nv*n),
       *mp = field((size_t)(NMP > 0 ? NMP : 1)*n);
#ifdef DMC_COOP_BUILD
  real* ws = field(n);
#else
  real* ws = field((size_t)(WS_WORDS > 0 ? WS_WORDS : 1)*n);
#endif
  int *stats = ints<int>(3*(size_t)n), *mask = new int[n], *ep_step = new int[n], *ep_done = new int[n];
  unsigned* warn = new unsigned[n];
  for (int e = 0; e < n; e++) {
    if (scanf("%d %d %d", &mask[e], &ep_step[e], &ep_done[e]) != 3) { fprintf(stderr, "short input\n"); return 2; }
    double x;
    bool ok = true;
    for (int i = 0; i < NMP; i++) { ok &= scanf("%lf", &x) == 1; mp[at(i, e, n, NMP)] = (real)x; }
    for (int i = 0; i < NQ; i++) { ok &= scanf("%lf", &x) == 1; qpos[at(i, e, n, nq)] = (real)x; }
    for (int i = 0; i < NV; i++) { ok &= scanf("%lf", &x) == 1; qvel[at(i, e, n, nv)] = (real)x; }
    for (int i = 0; i < NU; i++) { ok &= scanf("%lf", &x) == 1; ctrl[at(i, e, n, nu)] = (real)x; }
    if (!ok) { fprintf(stderr, "short input for env %d\n", e); return 2; }
    for (int i = 0; i < NV; i++) warm[at(i, e, n, nv)] = 0;
    tm[e] = 0; ret[e] = 0; warn[e] = 0;
  }
  a.qpos = qpos; a.qvel = qvel; a.warm = warm; a.time = tm; a.ctrl_store = ctrl;
  a.obs = obs; a.obs_sk = 1; a.obs_se = NOBS; a.reward = rew; a.episode_return = ret;
  a.sensordata = sens; a.xpos = xpos; a.xmat = xmat; a.qacc = qacc; a.warn = warn;
  a.stats = stats; a.ws = ws;
  if (NMP > 0) a.modelparam = mp;
  a.env_mask = mask; a.ep_step = ep_step; a.ep_done = ep_done;
  for (int t = 0; t < BLOCK_LANES/SHIM_GROUP; t++)
    pthread_barrier_init(&shim_teams[t].bar, nullptr, SHIM_GROUP);
  for (int t = -1; t < steps; t++) {
    for (int b = 0; t >= 0 && b < (n + BLOCK_ENVS - 1)/BLOCK_ENVS; b++) {
      int lanes = BLOCK_LANES;
#ifndef DMC_COOP_BUILD
      if (n - b*64 < 64) lanes = n - b*64;     // (the lanes past the batch leave at once)
#endif
      g_block = (unsigned)b;
      episode_barrier.parties = lanes; episode_barrier.waiting = 0;
      memset(episode_votes, 0, sizeof episode_votes);
      pthread_t th[BLOCK_LANES];
      for (size_t i = 0; i < (size_t)lanes; i++) pthread_create(&th[i], nullptr, lane_main, (void*)i);
      for (int i = 0; i < lanes; i++) pthread_join(th[i], nullptr);
    }
    for (int e = 0; e < n; e++) {
      printf("STEP %d %d", t, e);
      print(qpos, NQ, e, n, ""); print(qvel, NV, e, n, "");
      printf(" | %d %d %d %u | %d %d |", stats[at(0, e, n, 3)], stats[at(1, e, n, 3)],
             stats[at(2, e, n, 3)], warn[e], ep_step[e], ep_done[e]);
      print(qpos, NQ, e, n, ""); print(qvel, NV, e, n, ""); print(warm, NV, e, n, "");
      print(tm + e, 1, 0, 1, ""); print(ctrl, NU, e, n, "");
      for (int k = 0; k < NOBS; k++) printf(" %.17g", (double)obs[(size_t)e*NOBS + k]);
      print(rew + e, 1, 0, 1, ""); print(ret + e, 1, 0, 1, ""); print(sens, NSENSORDATA, e, n, "");
      print(xpos, NBODY*3, e, n, ""); print(xmat, NBODY*9, e, n, ""); print(qacc, NV, e, n, "");
      printf(" %d %d %d %u %d %d\n", stats[at(0, e, n, 3)], stats[at(1, e, n, 3)],
             stats[at(2, e, n, 3)], warn[e], ep_step[e], ep_done[e]);
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "init")) return init_main();
  if (argc > 1 && !strcmp(argv[1], "step")) return step_main();
  fprintf(stderr, "usage: episode_harness init|step\n");
  return 2;
}
