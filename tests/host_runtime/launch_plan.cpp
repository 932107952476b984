// launch_plan.cpp -- the pure half of the host runtime (csrc/dmc_launch.h) without a
// device: flags and members of every kind of launch, the shadow target of an episode
// prefetch, the chunks of a sequence, the grid.  Built with the sanitizers and run by
// tests/test_launch_plan.py, one case per argv[1].  Flag bits are written out as
// numbers on purpose: the builders' own expressions are what is under test.
#include "dmc_launch.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);             \
      failures++;                                                    \
    }                                                                \
  } while (0)

// distinct addresses that nothing dereferences
void* fake(int n) { return (void*)(uintptr_t)(0x100000 + 0x1000*n); }
char* bytes_past(const void* p, long long n) { return (char*)p + n; }

DmcState state(bool aux, bool episodes, bool masked, int nu = 6, int real_size = 4) {
  DmcState s;
  s.nenv = 130;
  s.code.info.nobs = 17;
  s.code.info.nu = nu;
  s.code.info.real_size = real_size;
  s.task_param_i = 3;
  s.task_param_r[1] = 2.5;
  s.aux_outputs = aux;
  s.episodes = episodes;
  s.masked = masked;
  s.step_limit = 1000;
  for (int k = 0; k < DMC_EPISODE_COUNT; k++) s.episode[k] = (int*)fake(40 + k);
  return s;
}

DmcTarget own_target() {
  DmcTarget t;
  for (int f = 0; f < DMC_FIELD_COUNT; f++) t.field[f] = fake(1 + f);
  t.ws = fake(30);
  return t;
}

// what every block carries, whatever its kind
void check_common(const DmcArgs& a, const DmcState& s, const DmcTarget& t, int nsub, int nsteps) {
  CHECK(a.nenv == 130 && a.task_param_i == 3 && a.task_param_r[1] == 2.5);
  CHECK((a.xpos != nullptr) == s.aux_outputs && (a.xmat != nullptr) == s.aux_outputs &&
        (a.qacc != nullptr) == s.aux_outputs);
  if (s.aux_outputs)
    CHECK(a.xpos == t.field[DMC_FIELD_XPOS] && a.xmat == t.field[DMC_FIELD_XMAT] &&
          a.qacc == t.field[DMC_FIELD_QACC]);
  CHECK(a.obs_sk == 1 && a.obs_se == 17);
  CHECK(a.nsub == nsub && a.nsteps == nsteps);
  CHECK(a.qpos == t.field[DMC_FIELD_QPOS] && a.qvel == t.field[DMC_FIELD_QVEL] &&
        a.warm == t.field[DMC_FIELD_WARMSTART] && a.time == t.field[DMC_FIELD_TIME] &&
        a.ctrl_store == t.field[DMC_FIELD_CTRL] && a.obs == t.field[DMC_FIELD_OBS] &&
        a.reward == t.field[DMC_FIELD_REWARD] && a.sensordata == t.field[DMC_FIELD_SENSORDATA] &&
        a.warn == t.field[DMC_FIELD_WARN] && a.stats == t.field[DMC_FIELD_STATS] &&
        a.episode_return == t.field[DMC_FIELD_RETURN] &&
        a.taskdata == t.field[DMC_FIELD_TASKDATA] &&
        a.modelparam == t.field[DMC_FIELD_MODELPARAM] && a.ws == t.ws);
  CHECK(a.ep_step == s.episode[DMC_EPISODE_STEP] && a.ep_done == s.episode[DMC_EPISODE_DONE] &&
        a.env_mask == s.episode[DMC_EPISODE_MASK] && a.step_limit == 1000);
}

void case_flags() {
  const DmcTarget t = own_target();
  for (int combo = 0; combo < 8; combo++) {
    const bool aux = combo & 1, episodes = combo & 2, masked = combo & 4;
    const int M = masked ? 128 : 0, E = episodes ? 256 : 0;
    const DmcState s = state(aux, episodes, masked);
    DmcArgs a = create_defaults_args(s, t);
    CHECK(a.flags == (M | 16 | 32));
    check_common(a, s, t, 1, 0);
    a = reset_args(s, t);
    CHECK(a.flags == (16 | E));
    check_common(a, s, t, 1, 0);
    for (int oc = 0; oc < 2; oc++) {
      a = init_episode_args(s, t, 0x123456789abcdefULL, oc);
      CHECK(a.flags == (M | (oc ? 8 : 0) | E));
      CHECK(a.seed == 0x123456789abcdefULL);
      check_common(a, s, t, 1, 0);
    }
    for (int cc = 0; cc < 2; cc++) {
      a = forward_args(s, t, cc);
      CHECK(a.flags == (M | (cc ? 4 : 0)));
      check_common(a, s, t, 1, 0);
    }
    // step: DMC_STEP_OUTPUTS 1, DMC_STEP_STALE_FIRST 2, DMC_STEP_ZERO_TIME 4
    for (int bits = 0; bits < 32; bits++) {
      const bool outputs = bits & 1, stale = bits & 2, zero = bits & 4, given = bits & 8;
      const int nu = (bits & 16) ? 6 : 0;
      const DmcState sn = state(aux, episodes, masked, nu);
      a = step_args(sn, t, (outputs ? 1 : 0) | (stale ? 2 : 0) | (zero ? 4 : 0),
                    given ? fake(60) : nullptr, 130, 1, 0, 0, 1, 5);
      CHECK(a.flags == (M | (outputs ? E : 2) | (stale ? 64 : 0) | (zero ? 512 : 0) |
                        (given && nu > 0 ? 1 : 0)));
      CHECK(a.ctrl == (given && nu > 0 ? fake(60) : nullptr));
      check_common(a, sn, t, 5, 1);
    }
    for (int bits = 0; bits < 8; bits++) {
      const bool given = bits & 1, policy = bits & 2;
      const int nu = (bits & 4) ? 6 : 0;
      const DmcState sn = state(aux, episodes, masked, nu);
      dmc_rollout r{};
      r.nsteps = 200;
      r.nsub = 4;
      r.ctrl = given ? fake(60) : nullptr;
      r.policy = policy ? fake(61) : nullptr;
      r.nlayers = 2;
      r.width[0] = 32, r.width[1] = 16, r.width[2] = nu;
      r.action_out = fake(62);
      a = rollout_args(sn, t, r, 0, 64);
      CHECK(a.flags == (M | (given && nu > 0 ? 1 : 0) | (policy && nu > 0 ? 1024 : 0)));
      CHECK(a.policy == (policy && nu > 0 ? fake(61) : nullptr));
      CHECK(a.action_out == (nu > 0 ? fake(62) : nullptr));
      if (policy && nu > 0)
        CHECK(a.policy_nlayers == 2 && a.policy_width[0] == 32 && a.policy_width[1] == 16);
      check_common(a, sn, t, 4, 64);
    }
  }
}

// the reset, init and settle blocks of a prefetch are the ordinary ones with the
// shadow pointers substituted, and nothing else
void case_shadow() {
  const DmcTarget own = own_target();
  DmcTarget shadow;
  for (dmc_field f : DMC_SHADOWED) shadow.field[f] = fake(101 + f);
  shadow.ws = fake(130);
  share_unshadowed(shadow, own);
  CHECK(sizeof DMC_SHADOWED/sizeof DMC_SHADOWED[0] == 10);
  for (int aux = 0; aux < 2; aux++) {
    const DmcState s = state(aux, false, false);
    for (int kind = 0; kind < 3; kind++) {
      const auto build = [&](const DmcTarget& t) {
        return kind == 0   ? reset_args(s, t)
               : kind == 1 ? init_episode_args(s, t, 77, false)
                           : step_args(s, t, 2 | 4, nullptr, 0, 0, 0, 0, 1, 25);
      };
      DmcArgs want = build(own);
      const DmcArgs got = build(shadow);
      want.qpos = fake(101 + DMC_FIELD_QPOS);
      want.qvel = fake(101 + DMC_FIELD_QVEL);
      want.warm = fake(101 + DMC_FIELD_WARMSTART);
      want.time = fake(101 + DMC_FIELD_TIME);
      want.ctrl_store = fake(101 + DMC_FIELD_CTRL);
      if (aux) want.qacc = fake(101 + DMC_FIELD_QACC);
      want.warn = (unsigned*)fake(101 + DMC_FIELD_WARN);
      want.stats = (int*)fake(101 + DMC_FIELD_STATS);
      want.episode_return = fake(101 + DMC_FIELD_RETURN);
      want.taskdata = fake(101 + DMC_FIELD_TASKDATA);
      want.ws = fake(130);
      want.xpos = want.xmat = nullptr;
      CHECK(memcmp(&want, &got, sizeof want) == 0);
      // (and the substitution left the batch's own where the issue says so)
      CHECK(got.obs == own.field[DMC_FIELD_OBS] && got.reward == own.field[DMC_FIELD_REWARD] &&
            got.sensordata == own.field[DMC_FIELD_SENSORDATA] &&
            got.modelparam == own.field[DMC_FIELD_MODELPARAM]);
      CHECK((got.qacc != nullptr) == (aux != 0));
    }
  }
}

void case_chunks() {
  const DmcTarget t = own_target();
  const int counts[] = {0, 1, 63, 64, 65, 129};
  // (seq_launch, episodes, rollout) and the largest chunk each may use
  const struct { bool seq, episodes, rollout; int max; } kinds[] = {
      {true, false, false, 64}, {true, true, false, 1}, {false, false, false, 1},
      {false, false, true, 64}};
  for (int real_size : {4, 8})
    for (const auto& k : kinds)
      for (int nsteps : counts) {
        DmcState s = state(false, k.episodes, false, 6, real_size);
        s.code.info.seq_launch = k.seq;
        const int max = chunk_max(s, k.rollout);
        CHECK(max == k.max);
        dmc_rollout r{};
        r.nsub = 2;
        r.ctrl = fake(60), r.ctrl_stride_k = 130, r.ctrl_stride_env = 1, r.ctrl_stride_t = 7;
        r.reward_out = fake(61), r.reward_stride_t = 3;
        r.obs_out = nullptr, r.obs_stride_t = 5;       // a null record stays null
        r.action_out = fake(63), r.action_stride_t = 11;
        int t0 = 0, launches = 0;
        while (t0 < nsteps) {
          const int chunk = next_chunk(t0, nsteps, max);
          CHECK(chunk >= 1 && chunk <= k.max && t0 + chunk <= nsteps);
          if (chunk < 1) return;
          CHECK(chunk == k.max || t0 + chunk == nsteps);     // only the last one is short
          const DmcArgs a = k.rollout ? rollout_args(s, t, r, t0, chunk)
                                      : step_args(s, t, 1 | 2, fake(60), 130, 1, 7, t0, chunk, 2);
          CHECK(a.nsteps == chunk && a.nsub == 2 && a.ctrl_st == 7);
          CHECK((char*)a.ctrl == bytes_past(fake(60), (long long)t0*7*real_size));
          if (k.rollout) {
            CHECK((char*)a.reward_out == bytes_past(fake(61), (long long)t0*3*real_size));
            CHECK(a.obs_out == nullptr);
            CHECK((char*)a.action_out == bytes_past(fake(63), (long long)t0*11*real_size));
            CHECK(a.reward_out_st == 3 && a.obs_out_st == 5 && a.action_out_st == 11);
          } else {
            CHECK(((a.flags & 64) != 0) == (t0 == 0));       // DMC_FLAG_STALE_FIRST
          }
          t0 += chunk;
          launches++;
        }
        CHECK(t0 == nsteps && launches == (nsteps + k.max - 1)/k.max);
      }
}

void case_geometry() {
  const struct { int envs_per_block, lanes_per_env; } shapes[] = {
      {64, 1}, {32, 1}, {16, 1}, {2, 32}, {8, 8}, {1, 64}, {1, 128}};
  for (int nenv : {1, 63, 64, 65, 130})
    for (const auto& sh : shapes) {
      DmcState s = state(false, false, false);
      s.nenv = nenv;
      s.code.info.envs_per_block = sh.envs_per_block;
      s.code.info.lanes_per_env = sh.lanes_per_env;
      const DmcGeometry g = geometry(s, MODEL_SHAPED);
      CHECK(g.grid >= 1 && (long long)(g.grid - 1)*sh.envs_per_block < nenv &&
            nenv <= (long long)g.grid*sh.envs_per_block);
      CHECK(g.block == (unsigned)(sh.lanes_per_env*sh.envs_per_block));
      const DmcGeometry i = geometry(s, TASK_SETUP);
      CHECK(i.block == 64 && (long long)(i.grid - 1)*64 < nenv && nenv <= (long long)i.grid*64);
    }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string name = argc > 1 ? argv[1] : "";
  if (name == "flags") case_flags();
  else if (name == "shadow") case_shadow();
  else if (name == "chunks") case_chunks();
  else if (name == "geometry") case_geometry();
  else {
    fprintf(stderr, "usage: launch_plan flags|shadow|chunks|geometry\n");
    return 2;
  }
  if (failures) fprintf(stderr, "%s: %d checks failed\n", name.c_str(), failures);
  else printf("%s ok\n", name.c_str());
  return failures ? 1 : 0;
}
