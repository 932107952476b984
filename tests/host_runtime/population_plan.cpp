// population_plan.cpp -- the argument block of a rollout over a population of policies
// (rollout_args of csrc/dmc_launch.h with a member count) without a device.  Built with
// the sanitizers and run by tests/test_population_host.py.  Prints "population ok".
#include "dmc_launch.h"

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);             \
      failures++;                                                    \
    }                                                                \
  } while (0)

void* fake(int n) { return (void*)(uintptr_t)(0x100000 + 0x1000*n); }

}  // namespace

int main() {
  static_assert(sizeof(DmcArgs) == 352, "the block keeps its size");
  // the member sits in what was padding between policy_width[2] and reward_out
  static_assert(offsetof(DmcArgs, policy_members) == offsetof(DmcArgs, policy_width) + 8,
                "directly after policy_width[2]");
  static_assert(offsetof(DmcArgs, reward_out) == offsetof(DmcArgs, policy_members) + 4,
                "reward_out stays where it was");
  static_assert(offsetof(DmcArgs, policy) == 280 && offsetof(DmcArgs, reward_out) == 304 &&
                    offsetof(DmcArgs, action_out_st) == 344,
                "no member of the rollout part moved");
  DmcState s;
  s.nenv = 130;
  s.code.info.nobs = 17;
  s.code.info.nu = 6;
  s.code.info.real_size = 4;
  s.step_limit = 1000;
  DmcTarget t;
  for (int f = 0; f < DMC_FIELD_COUNT; f++) t.field[f] = fake(1 + f);
  t.ws = fake(30);
  for (int bits = 0; bits < 4; bits++) {
    dmc_rollout r{};
    r.nsteps = 200;
    r.nsub = 4;
    r.ctrl = (bits & 1) ? fake(60) : nullptr;
    r.ctrl_stride_k = 1, r.ctrl_stride_env = 6, r.ctrl_stride_t = 780;
    r.policy = (bits & 2) ? fake(61) : nullptr;
    r.nlayers = 2;
    r.width[0] = 32, r.width[1] = 16, r.width[2] = 6;
    r.reward_out = fake(62), r.obs_out = fake(63), r.action_out = fake(64);
    r.reward_stride_t = 130, r.obs_stride_t = 130*17, r.action_stride_t = 780;
    const DmcArgs today = rollout_args(s, t, r, 64, 36);     // today's signature
    const DmcArgs one = rollout_args(s, t, r, 64, 36, 1);
    CHECK(memcmp(&today, &one, sizeof one) == 0);
    CHECK(one.policy_members == 0);      // (a zero-filled block means one member)
    DmcArgs five = rollout_args(s, t, r, 64, 36, 5);
    CHECK(five.policy_members == ((bits & 2) ? 5 : 0));
    five.policy_members = 0;             // ... and nothing else differs
    CHECK(memcmp(&today, &five, sizeof five) == 0);
  }
  if (failures) return 1;
  printf("population ok\n");
  return 0;
}
