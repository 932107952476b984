// dmc_launch.h -- what a launch looks like: the kernel argument block of every kind
// of launch with its `flags`, the chunks of a sequence of control steps, the grid.
// Plain integers and pointers, nothing of HIP: dmc_api.cpp launches what these
// functions return, tests/host_runtime/launch_plan.cpp checks them without a device.
#pragma once

#include <cstring>

#include "../../include/dmc_hip.h"
#include "dmc_args.h"

// what a loaded code object says about itself (dmc_model derives from it)
struct DmcCodeObject {
  dmc_model_info info{};
  // its dmc_episode_caps (DMC_FLAG_* bits) and dmc_rollout_caps; 0: it exports none
  int episode_caps = 0, rollout_caps = 0;
};

// what of a batch its argument blocks are made from (dmc_batch derives from it)
struct DmcState {
  int nenv = 0;
  DmcCodeObject code;        // the model's, copied when the batch is created
  int task_param_i = 0;
  bool aux_outputs = false;
  double task_param_r[4] = {0, 0, 0, 0};
  // per-env episodes: device int32[nenv] arrays indexed by dmc_episode_array
  int* episode[DMC_EPISODE_COUNT] = {};
  bool episodes = false;   // init and output-producing steps carry DMC_FLAG_EPISODES
  bool masked = false;     // init, forward and step carry DMC_FLAG_MASKED
  int step_limit = 0;
};

// where a launch reads and writes: the batch's own, or the shadows of a prefetch
struct DmcTarget {
  void* field[DMC_FIELD_COUNT] = {};
  void* ws = nullptr;
};

// Every field that dmc_init_episode or a dmc_step without outputs writes (load_env /
// store_env and the tail of dmc_step in the kernel sources): what a prefetch shadows
// and a take copies back.  The workspace is shadowed whole: overflow rows of two
// concurrent launches must not collide, and a `mixed` build keeps the low words of
// its state there.
constexpr dmc_field DMC_SHADOWED[] = {
    DMC_FIELD_QPOS, DMC_FIELD_QVEL, DMC_FIELD_WARMSTART, DMC_FIELD_TIME, DMC_FIELD_CTRL,
    DMC_FIELD_QACC, DMC_FIELD_WARN, DMC_FIELD_STATS, DMC_FIELD_RETURN, DMC_FIELD_TASKDATA};

// The rest of a prefetch target: what its launches read, or (outputs) leave alone, is
// the batch's own; the frames stay null, none of its launches stores them.
constexpr dmc_field DMC_SHARED[] = {DMC_FIELD_OBS, DMC_FIELD_REWARD, DMC_FIELD_SENSORDATA,
                                    DMC_FIELD_MODELPARAM};
inline void share_unshadowed(DmcTarget& shadow, const DmcTarget& own) {
  for (dmc_field f : DMC_SHARED) shadow.field[f] = own.field[f];
}

// `p` advanced by `reals` elements of the code object's real type; null stays null
inline void* advanced(const DmcState& s, const void* p, long long reals) {
  return p ? (char*)p + reals*(long long)s.code.info.real_size : nullptr;
}

// what every launch carries, with the `flags` of its kind next to the base (the mask bit)
inline DmcArgs base_args(const DmcState& s, const DmcTarget& t, int flags = 0) {
  DmcArgs a;
  memset(&a, 0, sizeof a);
  a.nenv = s.nenv;
  a.nsub = 1;
  a.task_param_i = s.task_param_i;
  memcpy(a.task_param_r, s.task_param_r, sizeof a.task_param_r);
  a.qpos = t.field[DMC_FIELD_QPOS];
  a.qvel = t.field[DMC_FIELD_QVEL];
  a.warm = t.field[DMC_FIELD_WARMSTART];
  a.time = t.field[DMC_FIELD_TIME];
  a.ctrl_store = t.field[DMC_FIELD_CTRL];
  a.obs = t.field[DMC_FIELD_OBS];
  a.obs_sk = 1;                       // agent layout [nenv][nobs]
  a.obs_se = s.code.info.nobs;
  a.reward = t.field[DMC_FIELD_REWARD];
  a.episode_return = t.field[DMC_FIELD_RETURN];
  a.taskdata = t.field[DMC_FIELD_TASKDATA];
  a.modelparam = t.field[DMC_FIELD_MODELPARAM];
  a.sensordata = t.field[DMC_FIELD_SENSORDATA];
  a.xpos = s.aux_outputs ? t.field[DMC_FIELD_XPOS] : nullptr;
  a.xmat = s.aux_outputs ? t.field[DMC_FIELD_XMAT] : nullptr;
  a.qacc = s.aux_outputs ? t.field[DMC_FIELD_QACC] : nullptr;
  a.warn = (unsigned*)t.field[DMC_FIELD_WARN];
  a.stats = (int*)t.field[DMC_FIELD_STATS];
  a.ws = t.ws;
  a.env_mask = s.episode[DMC_EPISODE_MASK];
  a.ep_step = s.episode[DMC_EPISODE_STEP];
  a.ep_done = s.episode[DMC_EPISODE_DONE];
  a.step_limit = s.step_limit;
  a.flags = flags | (s.masked ? DMC_FLAG_MASKED : 0);
  return a;
}

// dmc_batch_create: per-instance task data and model parameters start from the
// compiled model's values
inline DmcArgs create_defaults_args(const DmcState& s, const DmcTarget& t) {
  return base_args(s, t, DMC_FLAG_RESET_ONLY | DMC_FLAG_TASKDATA_DEFAULT);
}

// mj_resetData: an init_episode launch with a task-less code path would need the
// model tables; instead dmc_init_episode runs with the task's part masked off via
// DMC_FLAG_RESET_ONLY.  The whole batch, whatever dmc_batch_set_masked says; with
// episodes enabled every env's step count and done bits restart with its state.
inline DmcArgs reset_args(const DmcState& s, const DmcTarget& t) {
  DmcArgs a = base_args(s, t);
  a.flags = DMC_FLAG_RESET_ONLY | (s.episodes ? DMC_FLAG_EPISODES : 0);
  return a;
}

inline DmcArgs init_episode_args(const DmcState& s, const DmcTarget& t, unsigned long long seed,
                                 bool only_colliding) {
  DmcArgs a = base_args(s, t, (only_colliding ? DMC_FLAG_ONLY_COLLIDING : 0) |
                                  (s.episodes ? DMC_FLAG_EPISODES : 0));
  a.seed = seed;
  return a;
}

inline DmcArgs forward_args(const DmcState& s, const DmcTarget& t, bool count_contacts) {
  return base_args(s, t, count_contacts ? DMC_FLAG_COUNT_CONTACTS : 0);
}

// Sequences of control steps go out as one launch per chunk where the code object
// loops over the steps itself (bounded, so that no launch occupies a shared device
// for long), else as one launch per step.  With per-env episodes every control step
// is a launch: an env freezes between steps.  A rollout build always loops.
inline int chunk_max(const DmcState& s, bool rollout) {
  return rollout || (s.code.info.seq_launch && !s.episodes) ? DMC_SEQ_LAUNCH_MAX_STEPS : 1;
}
inline int next_chunk(int t, int nsteps, int max) { return nsteps - t < max ? nsteps - t : max; }

// the dmc_step launch of steps [t, t + nsteps) of a sequence with the controls of step 0
// at `ctrl` and the DMC_STEP_* bits `want_outputs` (DMC_STEP_STALE_FIRST: of its first step)
inline DmcArgs step_args(const DmcState& s, const DmcTarget& tg, int want_outputs, const void* ctrl,
                         long long stride_k, long long stride_env, long long stride_t, int t,
                         int nsteps, int nsub) {
  DmcArgs a = base_args(s, tg);
  a.nsub = nsub;
  a.flags |= (want_outputs & DMC_STEP_OUTPUTS) ? (s.episodes ? DMC_FLAG_EPISODES : 0)
                                               : DMC_FLAG_NO_OUTPUT;
  if ((want_outputs & DMC_STEP_STALE_FIRST) && t == 0) a.flags |= DMC_FLAG_STALE_FIRST;
  if (want_outputs & DMC_STEP_ZERO_TIME) a.flags |= DMC_FLAG_ZERO_TIME;
  if (ctrl && s.code.info.nu > 0) {
    a.flags |= DMC_FLAG_CTRL;
    a.ctrl = advanced(s, ctrl, t*stride_t);
    a.ctrl_sk = stride_k;
    a.ctrl_se = stride_env;
  }
  a.nsteps = nsteps;
  a.ctrl_st = stride_t;
  return a;
}

// the launch of steps [t, t + nsteps) of a rollout, every pointer advanced to step t;
// `members` policies at r.policy (1: the block says nothing of members, as it always did)
inline DmcArgs rollout_args(const DmcState& s, const DmcTarget& tg, const dmc_rollout& r, int t,
                            int nsteps, int members = 1) {
  const int nu = s.code.info.nu;
  DmcArgs a = base_args(s, tg);
  a.nsub = r.nsub;
  a.nsteps = nsteps;
  if (r.ctrl && nu > 0) {
    a.flags |= DMC_FLAG_CTRL;
    a.ctrl = advanced(s, r.ctrl, t*r.ctrl_stride_t);
    a.ctrl_sk = r.ctrl_stride_k;
    a.ctrl_se = r.ctrl_stride_env;
    a.ctrl_st = r.ctrl_stride_t;
  }
  if (r.policy && nu > 0) {
    a.flags |= DMC_FLAG_POLICY;
    a.policy = r.policy;
    a.policy_nlayers = r.nlayers;
    a.policy_width[0] = r.width[0];
    a.policy_width[1] = r.nlayers == 2 ? r.width[1] : 0;
    a.policy_members = members > 1 ? members : 0;
  }
  a.reward_out = advanced(s, r.reward_out, t*r.reward_stride_t);
  a.reward_out_st = r.reward_stride_t;
  a.obs_out = advanced(s, r.obs_out, t*r.obs_stride_t);
  a.obs_out_st = r.obs_stride_t;
  a.action_out = nu > 0 ? advanced(s, r.action_out, t*r.action_stride_t) : nullptr;
  a.action_out_st = r.action_stride_t;
  return a;
}

// TASK_SETUP (dmc_init_episode): always one env per lane of a full wave.
// MODEL_SHAPED (dmc_step, dmc_observe): the shape the code object reports in
// dmc_info -- envs_per_block envs per workgroup, lanes_per_env lanes each (one
// lane, a group within a wavefront, or two wavefronts per env).
enum DmcShape { TASK_SETUP, MODEL_SHAPED };
struct DmcGeometry { unsigned grid, block; };
inline DmcGeometry geometry(const DmcState& s, DmcShape shape) {
  const dmc_model_info& mi = s.code.info;
  const unsigned per_block = shape == MODEL_SHAPED ? (unsigned)mi.envs_per_block : 64;
  const unsigned lanes = shape == MODEL_SHAPED ? (unsigned)mi.lanes_per_env : 1;
  return {(unsigned)((s.nenv + per_block - 1)/per_block), lanes*per_block};
}
