// Runs dmc_step of csrc/dmc_kernels.hip built with -DDMC_ROLLOUT=1
// -DDMC_POLICY_POPULATION=1 on the host under sanitizers (tests/test_population_host.py):
// rollout_harness.cpp with a population of policies, one per group of nenv/members
// envs.  A stand-alone program: one OS thread per lane, workgroup after workgroup;
// every array a heap block of exactly its size (the weights: nparams*members words), so
// one word past an end is a report.  TEST INFRASTRUCTURE ONLY.
//
// stdin: <nenv> <T> <nsub> <records 0|1> <has_ctrl 0|1> <nlayers 0|1|2> <w0> <w1>
//        <members> <ncalls> <steps of call 0> ...
//        nlayers > 0: the weights, [nparams][members] (nparams follows from the widths)
//        per env: <qpos> <qvel>
//        has_ctrl: T x nenv x NU controls, [t][env][k]
// The T steps are issued as `ncalls` launches (their lengths sum to T), every pointer
// advanced by the steps done, as dmc_batch_rollout chunks them.
// stdout: CALL <c> <env> <obs> | <reward>          the fields after launch c
//         TRAJ <t> <env> <obs> | <reward> | <action>     (records = 1)
//         FINAL <env> <every word of the env in every field>
#include "shim.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using std::tanh;

#include DMC_KERNEL_SOURCE

static_assert(!TEAMED, "one env per lane");
static_assert(ROLLOUT_CAPS == (DMC_ROLLOUT_CAP_OUTPUTS | DMC_ROLLOUT_CAP_POLICY |
                               DMC_ROLLOUT_CAP_POPULATION |
                               (DMC_POLICY_MAX_WIDTH << DMC_ROLLOUT_CAP_WIDTH_SHIFT)),
              "the capability word of a population build: bit 4, the width field still 64");
static_assert(sizeof(DmcArgs) == 352, "policy_members took padding");
static_assert(ROLLOUT_LDS_WORDS >= LANES*DMC_POLICY_MAX_WIDTH && ROLLOUT_LDS_WORDS >= LDS_WORDS,
              "the LDS array holds a hidden vector per lane");
#ifdef ROLLOUT_EXPECT_POLICY_SIZED
static_assert(LDS_WORDS < LANES*DMC_POLICY_MAX_WIDTH, "the policy, not the rows, sizes the array");
#endif
static_assert(ROLLOUT_OBS_STAGE_FITS, "the transposed record store is under test");
constexpr double SENTINEL = -777.25;

static real* field(size_t words) {
  real* p = new real[words];
  for (size_t i = 0; i < words; i++) p[i] = (real)SENTINEL;
  return p;
}
static void print(const real* p, int K, int e, int n) {
  for (int k = 0; k < K; k++) printf(" %.17g", (double)p[(size_t)k*n + e]);
}

static DmcArgs g_args;
static unsigned g_block;
static void* lane_main(void* arg) {
  threadIdx.x = (unsigned)(size_t)arg;
  blockIdx.x = g_block;
  dmc_step(g_args);
  return nullptr;
}

int main() {
  int n, T, nsub, records, has_ctrl, nlayers, w0, w1, members, ncalls;
  if (scanf("%d %d %d %d %d %d %d %d %d %d", &n, &T, &nsub, &records, &has_ctrl, &nlayers, &w0,
            &w1, &members, &ncalls) != 10 || n < 1 || T < 1 || ncalls < 1 || members < 1 ||
      n % members) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  std::vector<int> calls(ncalls);
  int total = 0;
  for (int& c : calls) { if (scanf("%d", &c) != 1) return 2; total += c; }
  if (total != T) { fprintf(stderr, "the calls do not sum to T\n"); return 2; }
  const int nq = NQ > 0 ? NQ : 1, nv = NV > 0 ? NV : 1, nu = NU > 0 ? NU : 1,
            nobs = NOBS > 0 ? NOBS : 1, nsd = NSENSORDATA > 0 ? NSENSORDATA : 1;
  double x;
  real* weights = nullptr;
  if (nlayers > 0) {
    const size_t count = members*(nlayers == 1 ? (size_t)w0*NOBS + w0 + (size_t)NU*w0 + NU
                                               : (size_t)w0*NOBS + w0 + (size_t)w1*w0 + w1 +
                                                     (size_t)NU*w1 + NU);
    weights = field(count);
    for (size_t i = 0; i < count; i++) { if (scanf("%lf", &x) != 1) return 2; weights[i] = (real)x; }
  }
  real *qpos = field((size_t)nq*n), *qvel = field((size_t)nv*n), *warm = field((size_t)nv*n),
       *tm = field(n), *held = field((size_t)nu*n), *obs = field((size_t)nobs*n), *rew = field(n),
       *ret = field(n), *sens = field((size_t)nsd*n),
       *ws = field((size_t)(WS_WORDS > 0 ? WS_WORDS : 1)*n);
  int* stats = new int[3*(size_t)n];
  unsigned* warn = new unsigned[n];
  for (int e = 0; e < n; e++) {
    bool ok = true;
    for (int i = 0; i < NQ; i++) { ok &= scanf("%lf", &x) == 1; qpos[(size_t)i*n + e] = (real)x; }
    for (int i = 0; i < NV; i++) { ok &= scanf("%lf", &x) == 1; qvel[(size_t)i*n + e] = (real)x; }
    if (!ok) { fprintf(stderr, "short input for env %d\n", e); return 2; }
    for (int i = 0; i < NV; i++) warm[(size_t)i*n + e] = 0;
    for (int i = 0; i < NU; i++) held[(size_t)i*n + e] = 0;
    tm[e] = 0; ret[e] = 0; warn[e] = 0;
    stats[e] = stats[n + e] = stats[2*n + e] = 0;
  }
  real* ctrl = nullptr;
  if (has_ctrl) {
    ctrl = field((size_t)T*n*NU);
    for (size_t i = 0; i < (size_t)T*n*NU; i++) { if (scanf("%lf", &x) != 1) return 2; ctrl[i] = (real)x; }
  }
  real *obs_out = records ? field((size_t)T*n*NOBS) : nullptr,
       *rew_out = records ? field((size_t)T*n) : nullptr,
       *act_out = records ? field((size_t)T*n*NU) : nullptr;
  DmcArgs& a = g_args;
  memset(&a, 0, sizeof a);
  a.nenv = n; a.nsub = nsub;
  a.qpos = qpos; a.qvel = qvel; a.warm = warm; a.time = tm; a.ctrl_store = held;
  a.obs = obs; a.obs_sk = 1; a.obs_se = NOBS; a.reward = rew; a.episode_return = ret;
  a.sensordata = sens; a.warn = warn; a.stats = stats; a.ws = ws;
  for (int k = 0; k < 64/SHIM_GROUP; k++) pthread_barrier_init(&shim_teams[k].bar, nullptr, SHIM_GROUP);
  const auto launch = [&]() {
    for (int b = 0; b < (n + 63)/64; b++) {
      const int lanes = n - b*64 < 64 ? n - b*64 : 64;    // (the lanes past the batch leave at once)
      g_block = (unsigned)b;
      pthread_barrier_init(&shim_block_barrier, nullptr, lanes);
      pthread_t th[64];
      for (size_t i = 0; i < (size_t)lanes; i++) pthread_create(&th[i], nullptr, lane_main, (void*)i);
      for (int i = 0; i < lanes; i++) pthread_join(th[i], nullptr);
      pthread_barrier_destroy(&shim_block_barrier);
    }
  };
  // o_0: the observation of the initial state, as dmc_batch_forward leaves it.  The
  // harness has no dmc_observe pass: a launch of zero substeps computes the outputs.
  a.nsub = 0; a.nsteps = 1;
  launch();
  for (int e = 0; e < n; e++) { ret[e] = 0; }
  a.nsub = nsub;
  int t = 0;
  for (int c = 0; c < ncalls; c++) {
    a.flags = 0;
    a.nsteps = calls[c];
    if (has_ctrl) {
      a.flags |= DMC_FLAG_CTRL;
      a.ctrl = ctrl + (size_t)t*n*NU; a.ctrl_sk = 1; a.ctrl_se = NU; a.ctrl_st = (long long)n*NU;
    }
    if (nlayers > 0) {
      a.flags |= DMC_FLAG_POLICY;
      a.policy = weights; a.policy_nlayers = nlayers; a.policy_width[0] = w0; a.policy_width[1] = w1;
      a.policy_members = members > 1 ? members : 0;     // (as rollout_args writes it)
    }
    if (records) {
      a.obs_out = obs_out + (size_t)t*n*NOBS; a.obs_out_st = (long long)n*NOBS;
      a.reward_out = rew_out + (size_t)t*n; a.reward_out_st = n;
      a.action_out = act_out + (size_t)t*n*NU; a.action_out_st = (long long)n*NU;
    }
    launch();
    t += calls[c];
    for (int e = 0; e < n; e++) {
      printf("CALL %d %d", c, e);
      for (int k = 0; k < NOBS; k++) printf(" %.17g", (double)obs[(size_t)e*NOBS + k]);
      printf(" | %.17g\n", (double)rew[e]);
    }
  }
  for (int s = 0; records && s < T; s++)
    for (int e = 0; e < n; e++) {
      printf("TRAJ %d %d", s, e);
      for (int k = 0; k < NOBS; k++) printf(" %.17g", (double)obs_out[((size_t)s*n + e)*NOBS + k]);
      printf(" | %.17g |", (double)rew_out[(size_t)s*n + e]);
      for (int k = 0; k < NU; k++) printf(" %.17g", (double)act_out[((size_t)s*n + e)*NU + k]);
      printf("\n");
    }
  for (int e = 0; e < n; e++) {
    printf("FINAL %d", e);
    print(qpos, NQ, e, n); print(qvel, NV, e, n); print(warm, NV, e, n); print(tm + e, 1, 0, 1);
    print(held, NU, e, n);
    for (int k = 0; k < NOBS; k++) printf(" %.17g", (double)obs[(size_t)e*NOBS + k]);
    print(rew + e, 1, 0, 1); print(ret + e, 1, 0, 1); print(sens, NSENSORDATA, e, n);
    printf(" %d %d %d %u\n", stats[e], stats[n + e], stats[2*n + e], warn[e]);
  }
  return 0;
}
