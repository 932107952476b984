// dmc_args.h -- the whole contract between the host runtime (dmc_api.cpp) and
// the device code (dmc_kernels.hip, dmc_coop.hip): the kernel argument block,
// the bits of its `flags`, and the code object's self-description `dmc_info`.
// Plain pointers and sizes only; `real`-typed arrays are void* on the host side
// because the element type (float/double) is a property of the loaded code object.
#pragma once
#ifndef DMC_REALPTR
#define DMC_REALPTR void*
#define DMC_CREALPTR const void*
#endif
struct DmcArgs {
  int nenv, nsub, flags, task_param_i;
  unsigned long long seed;
  DMC_REALPTR qpos;        // [NQ][nenv]
  DMC_REALPTR qvel;        // [NV][nenv]
  DMC_REALPTR warm;        // [NV][nenv] qacc_warmstart
  DMC_REALPTR time;        // [nenv]
  DMC_CREALPTR ctrl;       // element (k, env) at ctrl[k*ctrl_sk + env*ctrl_se]
  long long ctrl_sk, ctrl_se;
  DMC_REALPTR ctrl_store;  // [NU][nenv] last applied control (data.ctrl)
  DMC_REALPTR obs;         // element (k, env) at obs[k*obs_sk + env*obs_se]
  long long obs_sk, obs_se;
  DMC_REALPTR reward;      // [nenv]
  DMC_REALPTR episode_return;  // [nenv] sum of rewards since the last reset
  DMC_REALPTR sensordata;  // [NSENSORDATA][nenv]
  DMC_REALPTR xpos;        // [NBODY*3][nenv] (may be null)
  DMC_REALPTR xmat;        // [NBODY*9][nenv] (may be null)
  DMC_REALPTR qacc;        // [NV][nenv] (may be null)
  unsigned* warn;          // [nenv] sticky mjtWarning bit mask
  int* stats;              // [3][nenv]: ncon, nefc, solver iterations
  DMC_REALPTR ws;          // workspace, ws_per_env reals per env, [idx][nenv]
  DMC_REALPTR taskdata;    // [NTASKDATA][nenv] per-instance task parameters
  double task_param_r[4];
  DMC_REALPTR modelparam;  // [NMODELPARAM][nenv] model fields read per env (builds with per-env fields)
  // sequence launch (one-env-per-lane dmc_step of code objects that report it in
  // dmc_info): control steps in this launch, step t reading its controls at
  // ctrl + t*ctrl_st.  A zero-filled block (nsteps 0) is one step.
  int nsteps;
  long long ctrl_st;
  // per-env episodes (code objects that report the flags in dmc_episode_caps).
  // A zero-filled block is a launch over the whole batch without bookkeeping.
  const int* env_mask;     // [nenv] DMC_FLAG_MASKED: the launch touches env e only if env_mask[e] != 0
  int* ep_step;            // [nenv] DMC_FLAG_EPISODES: control steps of the episode
  int* ep_done;            // [nenv] DMC_FLAG_EPISODES: DMC_EP_DONE_* bits, nonzero = frozen until re-initialised
  int step_limit;          // ep_done gets DMC_EP_DONE_LIMIT once ep_step >= step_limit (<= 0: never)
  // rollouts (code objects built with -DDMC_ROLLOUT=1, which report it in
  // dmc_rollout_caps).  A zero-filled block is a launch without them.
  // DMC_FLAG_POLICY: the control of step t is an MLP over the observation (plus
  // ctrl[t] with DMC_FLAG_CTRL).  Weights shared by the batch, packed per layer as
  // W[out][in] row-major then b[out]: policy_nlayers (1 or 2) tanh layers of
  // policy_width[l] units, then the linear output layer of NU units.
  // policy_members P > 1 (code objects with DMC_ROLLOUT_CAP_POPULATION): P policies of
  // that shape, env e acting with member e / (nenv/P); word j of the packed order of
  // member m at policy[j*P + m].  0 reads as 1, the shared block.
  DMC_CREALPTR policy;
  int policy_nlayers;
  int policy_width[2];
  int policy_members;      // (where the pointer below left 4 bytes of padding)
  // per-step outputs of the launch's step t, each optional (null: not stored):
  DMC_REALPTR reward_out;  // [nenv] at reward_out + t*reward_out_st: reward of the state after step t
  DMC_REALPTR obs_out;     // [nenv][NOBS] at obs_out + t*obs_out_st: its observation
  DMC_REALPTR action_out;  // [nenv][NU] at action_out + t*action_out_st: the control applied at
                           // step t, before the ctrlrange clamp and the bad-control check
  long long reward_out_st, obs_out_st, action_out_st;
};
// bits of DmcArgs.flags
#define DMC_FLAG_CTRL 1          // ctrl pointer valid (else reuse ctrl_store)
#define DMC_FLAG_NO_OUTPUT 2     // skip observation/reward (settle steps)
#define DMC_FLAG_COUNT_CONTACTS 4
#define DMC_FLAG_ONLY_COLLIDING 8
#define DMC_FLAG_RESET_ONLY 16     // dmc_init_episode: mj_resetData only
#define DMC_FLAG_TASKDATA_DEFAULT 32  // dmc_init_episode: task data and model parameters <- model values
#define DMC_FLAG_STALE_FIRST 64    // dmc_step: first substep takes its acceleration from the reset state
#define DMC_FLAG_MASKED 128        // all kernels: envs with env_mask[e] == 0 are left alone, every field bit for bit
#define DMC_FLAG_EPISODES 256      // dmc_step with outputs: skip envs with ep_done != 0, count ep_step, set ep_done;
                                   // dmc_init_episode: ep_step, ep_done and warn <- 0 for the envs it writes
#define DMC_FLAG_ZERO_TIME 512     // dmc_step: store time = 0 for the envs it stepped (settle launches of a reset)
#define DMC_FLAG_POLICY 1024       // dmc_step of a rollout build: controls from the MLP at `policy`
// bits of ep_done (enum dmc_done_bit of the header)
#define DMC_EP_DONE_LIMIT 1        // the episode reached step_limit
#define DMC_EP_DONE_BAD_STATE 2    // a launch raised a warning bit (mjtWarning) for the env

// `dmc_info`: what a code object says about itself, read by dmc_api.cpp through
// hipModuleGetGlobal.  The member order is the layout in the code object; new
// members go at the end (an older code object then reads as 0 there).  Aligned as
// the compiler aligns the `int[20]` it used to be, so that it stays where it was.
struct alignas(16) DmcInfo {
  int abi;                // 1
  int real_size;          // sizeof(real)
  int nq, nv, nu, nbody, nobs, nsensordata;
  int ws_per_env;         // workspace reals per env
  int task, ncon_max, nefc_max, integrator, npair;
  int envs_per_block;     // envs per workgroup of dmc_step / dmc_observe (0: 64); the
                          // workspace is sized for the batch rounded up to this
  int env_major;          // 0: the 2-D state fields are [k][env] in HBM; else [env][k]
  int ntaskdata;
  int threads_per_block;  // = envs_per_block unless several lanes share an env
  int nmodelparam;        // rows of the model-parameter block
  int seq_launch;         // 1: dmc_step runs DmcArgs.nsteps control steps per launch
};
static_assert(sizeof(DmcArgs) == 352, "policy_members took padding: no member moved");
static_assert(sizeof(DmcInfo) == 20*sizeof(int), "dmc_info is 20 ints");

// `dmc_episode_caps`: a second device global next to `dmc_info` (whose size is
// part of the ABI): the DMC_FLAG_* bits of the per-env episode contract that the
// code object honours.  A code object without the global, or with a bit clear
// (team mode), makes the host refuse the entry points that need it.
typedef int DmcEpisodeCaps;

// `dmc_rollout_caps`: a third device global, exported by rollout builds only
// (-DDMC_ROLLOUT=1, one env per lane): what dmc_batch_rollout may ask of the code
// object.  Absent (read as 0) in every other build.
typedef int DmcRolloutCaps;
#define DMC_ROLLOUT_CAP_OUTPUTS 1         // per-step reward / observation / action stores
#define DMC_ROLLOUT_CAP_POLICY 2          // DMC_FLAG_POLICY
#define DMC_ROLLOUT_CAP_POPULATION 4      // DmcArgs.policy_members > 1 (-DDMC_POLICY_POPULATION=1)
#define DMC_ROLLOUT_CAP_WIDTH_SHIFT 8     // caps >> 8: the widest hidden layer it takes
