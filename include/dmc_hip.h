/* dmc_hip.h -- C ABI of the MI355X batched physics step (libdmc_hip.so).
 *
 * Drop-in boundary for the path the reference reaches through the ctypes
 * handle `mjlib` (/root/reference/dm_control/mujoco/wrapper/util.py:107-120).
 * Every entry point is extern "C", takes plain pointers and sizes, returns an
 * int status (0 = ok) and leaves a message for dmc_last_error() on failure.
 * Per-environment physics faults never abort: they are reported through the
 * sticky `DMC_FIELD_WARN` bit mask whose bit order is mjtWarning
 * (engine.py:307-330 turns new warnings into PhysicsError).
 *
 * Batched counterparts (B = nenv independent instances, struct-of-arrays
 * [k][env] in device memory unless a stride is given):
 *
 *   reference call (file:line)                          this ABI
 *   --------------------------------------------------  ----------------------
 *   mj_version            wrapper/core.py:65            dmc_version
 *   mj_loadXML            wrapper/core.py:312-328       dmc_model_compile /
 *                                                       dmc_model_load (*)
 *   mj_deleteModel        wrapper/core.py:326           dmc_model_free
 *   mj_makeData           wrapper/core.py:646           dmc_batch_create
 *   mj_deleteData         wrapper/core.py:649           dmc_batch_free
 *   mj_resetData          engine.py:280                 dmc_batch_reset
 *   np.copyto(qpos/qvel)  suite tasks' initialize_episode dmc_batch_set_state,
 *                                                       dmc_batch_init_episode
 *   mj_forward            engine.py:305 (after_reset)   dmc_batch_forward
 *   mj_step2/mj_step +    engine.py:162-166             dmc_batch_step
 *     mj_step1
 *   mjData field views    wrapper/core.py:630-776       dmc_batch_read,
 *                                                       dmc_batch_device_ptr
 *   mj_copyData           engine.py:262                 dmc_batch_copy_state
 *
 * (*) MJCF parsing/compilation is host logic in Python
 *     (dm_control_amd/mjcf/compiler.py); what crosses the ABI is the model as a
 *     table of constants (dm_control_amd/codegen.py) -- either already built
 *     into a gfx950 code object (dmc_model_load) or as text that
 *     dmc_model_compile turns into one in-process, without the hipcc toolchain.
 */
#ifndef DMC_HIP_H_
#define DMC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_model dmc_model;
typedef struct dmc_batch dmc_batch;

/* fields addressable through dmc_batch_read / dmc_batch_device_ptr */
enum dmc_field {
  DMC_FIELD_QPOS = 0,       /* real [nq][nenv] */
  DMC_FIELD_QVEL = 1,       /* real [nv][nenv] */
  DMC_FIELD_WARMSTART = 2,  /* real [nv][nenv]  (qacc_warmstart) */
  DMC_FIELD_TIME = 3,       /* real [nenv] */
  DMC_FIELD_CTRL = 4,       /* real [nu][nenv]  (last applied data.ctrl) */
  DMC_FIELD_OBS = 5,        /* real [nenv][nobs] (row-major, agent layout) */
  DMC_FIELD_REWARD = 6,     /* real [nenv] */
  DMC_FIELD_SENSORDATA = 7, /* real [nsensordata][nenv] */
  DMC_FIELD_XPOS = 8,       /* real [nbody*3][nenv] */
  DMC_FIELD_XMAT = 9,       /* real [nbody*9][nenv] */
  DMC_FIELD_QACC = 10,      /* real [nv][nenv] */
  DMC_FIELD_WARN = 11,      /* uint32 [nenv] sticky mjtWarning bit mask */
  DMC_FIELD_STATS = 12,     /* int32 [3][nenv]: ncon, nefc, solver iterations */
  DMC_FIELD_RETURN = 13,    /* real [nenv] sum of rewards since the last reset */
  DMC_FIELD_TASKDATA = 14,  /* real [ntaskdata][nenv] per-instance task parameters (e.g.
                               the reacher's target position, which the reference
                               writes into model.geom_pos per episode) */
  DMC_FIELD_MODELPARAM = 15, /* real [nmodelparam][nenv] model fields that a build reads per
                               env instead of from its compiled tables (domain
                               randomisation): rows as laid out by
                               codegen.model_param_layout; starts with the compiled
                               model's values, untouched by reset / init_episode */
  DMC_FIELD_COUNT = 16
};

enum dmc_warn_bit {
  DMC_WARN_INERTIA = 1, DMC_WARN_CONTACTFULL = 2, DMC_WARN_CNSTRFULL = 4,
  DMC_WARN_VGEOMFULL = 8, DMC_WARN_BADQPOS = 16, DMC_WARN_BADQVEL = 32,
  DMC_WARN_BADQACC = 64, DMC_WARN_BADCTRL = 128
};

/* sizes of a loaded model (read back from the code object) */
typedef struct dmc_model_info {
  int abi, real_size, nq, nv, nu, nbody, nobs, nsensordata, ws_per_env, task,
      ncon_max, nefc_max, integrator, npair,
      ntaskdata,     /* per-instance task parameters (DMC_FIELD_TASKDATA rows) */
      envs_per_block, /* envs per workgroup of the step kernel */
      lanes_per_env, /* 1, or the group size of a several-lanes-per-env build
                        (8..64; 128 = one env per workgroup of two wavefronts) */
      env_major,     /* 1: the 2-D state fields are [nenv][k] in HBM (what
                        dmc_batch_device_ptr returns); dmc_batch_read and
                        dmc_batch_set_state present [k][nenv] regardless */
      nmodelparam,   /* rows of DMC_FIELD_MODELPARAM (0: no per-env model fields) */
      seq_launch;    /* 1: the step kernel runs a whole sequence of control steps per
                        launch (dmc_batch_step_n); 0: one launch per control step */
} dmc_model_info;

/* 101: dmc_model_info gained `nmodelparam` at its end and DMC_FIELD_MODELPARAM exists; a
 * caller built against the 100 header must be rebuilt (dmc_model_get_info fills the whole
 * struct)
 * 102: dmc_model_info gained `seq_launch` at its end (same rule)
 * 103: per-env episodes (dmc_batch_episodes_enable ... dmc_batch_set_masked, DMC_STEP_ZERO_TIME);
 *      code objects export `dmc_episode_caps`; older ones still load and step
 * 104: rollouts (dmc_model_rollout_caps, dmc_batch_rollout); rollout builds export
 *      `dmc_rollout_caps`, every other code object loads and steps as before
 * 105: episode prefetch (dmc_batch_episode_prefetch, dmc_batch_episode_take); host side
 *      only, every code object takes it
 * 106: populations of policies (dmc_batch_rollout_population, DMC_ROLLOUT_POPULATION);
 *      `dmc_rollout` is unchanged and every older code object rolls out as before */
int dmc_version(void);
const char* dmc_last_error(void);
int dmc_device_count(void);

/* model = gfx950 code object specialised for one compiled MJCF */
int dmc_model_load(const char* code_object_path, int device_id, dmc_model** out);
/* The compile half of mj_loadXML (wrapper/core.py:312-328) at the C boundary,
 * for a model that was not pre-built: `source` (the text of csrc/dmc_kernels.hip
 * or csrc/dmc_coop.hip) is compiled for gfx950 against `nheaders` in-memory
 * headers -- the generated model constants and the sources' own includes, each
 * under the name it is #included by -- with the given compiler options, through
 * the HIP runtime-compilation library of the ROCm runtime (libhiprtc, opened on
 * first use): no hipcc executable, no files.  The code object is returned in a
 * buffer owned by the library (dmc_code_free); load it with dmc_model_load_data
 * and/or store it.  On failure the compiler log is copied into `log` (like the
 * `char error[1000]` of mj_loadXML). */
int dmc_model_compile(const char* source, const char* source_name,
                      const char* const* header_names,
                      const char* const* header_texts, int nheaders,
                      const char* const* options, int noptions,
                      void** code, size_t* code_size, char* log, size_t log_size);
void dmc_code_free(void* code);
int dmc_model_load_data(const void* code, size_t code_size, int device_id,
                        dmc_model** out);
int dmc_model_get_info(const dmc_model* model, dmc_model_info* info);
void dmc_model_free(dmc_model* model);

/* batch of nenv instances resident in the HBM of the model's device */
int dmc_batch_create(const dmc_model* model, int nenv, dmc_batch** out);
void dmc_batch_free(dmc_batch* batch);
int dmc_batch_nenv(const dmc_batch* batch);

/* auxiliary per-step outputs (DMC_FIELD_XPOS, _XMAT, _QACC).  Off by default:
 * they are 105 extra words per env-step for cheetah, three times the
 * algorithmic output; switch them on when the caller reads those fields. */
int dmc_batch_set_aux_outputs(dmc_batch* batch, int enabled);

/* task parameters: integer flags + up to 4 reals (meaning is per task, e.g.
 * cartpole {bit0 sparse, bit1 swing_up}; humanoid r[0] = move_speed) */
int dmc_batch_set_task_params(dmc_batch* batch, int iparam, const double* rparam,
                              int nr);

/* mj_resetData for every env: qpos <- qpos0, qvel/ctrl/warmstart/time <- 0,
 * warning mask cleared */
int dmc_batch_reset(dmc_batch* batch);
/* explicit state upload, host pointers, `real`-typed [k][nenv]; NULL = keep */
int dmc_batch_set_state(dmc_batch* batch, const void* qpos, const void* qvel,
                        const void* warmstart, const void* time);
/* generic host -> device write of a writable field (QPOS, QVEL, WARMSTART,
 * TIME, TASKDATA), `real`-typed [k][nenv]; replaces the reference's in-place
 * writes through numpy views on mjData / mjModel (wrapper/core.py:630-776) */
int dmc_batch_write(dmc_batch* batch, int field, const void* src, size_t bytes);
/* task.initialize_episode on device (counter-based RNG keyed by seed, env).
 * only_colliding != 0 redraws only envs whose last contact count was > 0. */
int dmc_batch_init_episode(dmc_batch* batch, uint64_t seed, int only_colliding);
/* position/velocity stage + observation/reward/sensors of the current state
 * (what the task reads after reset_context; count_contacts != 0 also runs the
 * narrowphase so DMC_FIELD_STATS[0] = ncon) */
int dmc_batch_forward(dmc_batch* batch, int count_contacts);

/* bits of the `want_outputs` argument of dmc_batch_step / dmc_batch_step_n */
#define DMC_STEP_OUTPUTS 1       /* compute observation/reward after the last substep
                                  * (0: settle steps, task.initialize_episode) */
#define DMC_STEP_STALE_FIRST 2   /* the FIRST substep takes its acceleration from the
                                  * position/velocity stage of the reset state (qpos0,
                                  * zero velocity): what mj_step2 sees when a task
                                  * rewrites qpos after reset_context's mj_forward and
                                  * steps without a forward pass
                                  * (suite/cheetah.py:63-77, engine.py:149-166) */
/* a further bit of `want_outputs` (version 103 code objects): store time = 0 for the
 * envs the launch stepped -- the settle steps of a reset that runs under an env mask,
 * where a whole-field write of DMC_FIELD_TIME would touch the other envs */
enum dmc_step_bit { DMC_STEP_ZERO_TIME = 4 };

/* nsub x Physics.step, then observation + reward.
 * ctrl: element (k, env) at ctrl[k*stride_k + env*stride_env] (in reals);
 * host pointer when on_device == 0 (copied), device pointer otherwise
 * (zero-copy, e.g. a torch tensor).  ctrl == NULL keeps the previous control.
 * want_outputs: DMC_STEP_* bits (0 skips observation/reward). */
int dmc_batch_step(dmc_batch* batch, const void* ctrl, long long stride_k,
                   long long stride_env, int on_device, int nsub,
                   int want_outputs);
/* `nsteps` control steps back to back on the batch's stream, step t reading
 * its controls at ctrl + t*stride_t reals (device memory): the n_sub_steps loop
 * of control.Environment.step (rl/control.py:101-102) over a pre-computed action
 * sequence (open-loop rollouts, benchmarks; stride_t = 0: action repeat) without
 * a host round trip per step.  The observation / reward / sensor / stats fields
 * hold those of the last step, DMC_FIELD_RETURN has every step's reward added,
 * DMC_STEP_STALE_FIRST applies to the first step.  Same results, bit for bit, as
 * `nsteps` calls of dmc_batch_step.  On a code object with
 * dmc_model_info.seq_launch this is one launch per chunk of at most
 * DMC_SEQ_LAUNCH_MAX_STEPS control steps (state, warm start and episode return
 * stay in registers in between; outputs are written once per chunk); otherwise
 * one launch per control step.  The batch timer counts control steps either way. */
#define DMC_SEQ_LAUNCH_MAX_STEPS 64
int dmc_batch_step_n(dmc_batch* batch, const void* ctrl, long long stride_k,
                     long long stride_env, long long stride_t, int nsteps,
                     int nsub, int want_outputs);

/* device -> host copy of a whole field (synchronises the batch stream) */
int dmc_batch_read(dmc_batch* batch, int field, void* dst, size_t bytes);
size_t dmc_batch_field_bytes(const dmc_batch* batch, int field);
/* borrowed device pointer; lifetime = the batch handle */
void* dmc_batch_device_ptr(dmc_batch* batch, int field);
int dmc_batch_clear_warnings(dmc_batch* batch);
int dmc_batch_copy_state(dmc_batch* dst, const dmc_batch* src);
int dmc_batch_sync(dmc_batch* batch);
/* run every later launch/copy of this batch on a caller-owned hipStream_t (for
 * example torch.cuda.current_stream().cuda_stream, so the step is ordered with
 * the caller's own kernels without extra synchronisation).  external != 0:
 * use `stream` as given (NULL is HIP's legacy default stream, which is what
 * torch's default stream is); external == 0: back to the batch's own stream */
int dmc_batch_set_stream(dmc_batch* batch, void* stream, int external);
/* the batch's hipStream_t, for callers that enqueue their own work behind the
 * step (e.g. torch.cuda.ExternalStream) */
void* dmc_batch_stream(dmc_batch* batch);

/* Per-env episodes (version 103).  The episode block is three device int32[nenv]
 * arrays next to the fields (not dmc_fields): the control steps of every env's
 * episode, its done bits, and the env mask of masked launches.
 *
 * dmc_batch_episodes_enable allocates and zeroes the block; from then on
 *   - an output-producing dmc_batch_step skips every env whose done word is nonzero
 *     (it stays frozen, every field bit for bit, until it is re-initialised), adds 1
 *     to the step count of every env it stepped and sets that env's done word to
 *     DMC_DONE_LIMIT (step_limit > 0 and count >= step_limit) | DMC_DONE_BAD_STATE (the
 *     launch raised a DMC_FIELD_WARN bit for the env: mj_checkPos put it back to qpos0);
 *     settle steps (no outputs) neither count nor skip;
 *   - dmc_batch_init_episode and dmc_batch_reset zero the step count, the done word and
 *     the warning mask of every env they write;
 *   - dmc_batch_step_n takes one launch per control step.
 * dmc_batch_set_masked(on): while on, dmc_batch_init_episode, dmc_batch_forward and
 * dmc_batch_step leave every env with mask[e] == 0 alone -- all of its fields and its
 * part of the episode block are bit-identical after the launch; only_colliding
 * composes (both conditions must hold).  dmc_batch_reset always covers the batch.
 * dmc_batch_mask_from_done copies done -> mask on the batch's stream (no host
 * synchronisation): the mask of a reset pass, which survives the init launch
 * clearing the done words.  None of these calls, nor a masked launch, waits for the
 * device; dmc_batch_episode_read / _write do (whole arrays, nenv*4 bytes).
 * Code objects of team mode, and ones built before version 103, are refused with a
 * message by every entry point that would need the flags. */
enum dmc_episode_array {
  DMC_EPISODE_STEP = 0, DMC_EPISODE_DONE = 1, DMC_EPISODE_MASK = 2, DMC_EPISODE_COUNT = 3
};
enum dmc_done_bit { DMC_DONE_LIMIT = 1, DMC_DONE_BAD_STATE = 2 };
int dmc_batch_episodes_enable(dmc_batch* batch, int step_limit);
/* borrowed device pointer (NULL before the block exists); lifetime = the batch handle */
void* dmc_batch_episode_ptr(dmc_batch* batch, int which);
int dmc_batch_episode_read(dmc_batch* batch, int which, int* dst, size_t bytes);
int dmc_batch_episode_write(dmc_batch* batch, int which, const int* src, size_t bytes);
int dmc_batch_mask_from_done(dmc_batch* batch);
int dmc_batch_set_masked(dmc_batch* batch, int on);

/* Episode prefetch (version 105): the start of the batch's NEXT episode, computed beside
 * the steps of the current one.  What a whole-batch reset launches on the batch's stream --
 * dmc_batch_reset, dmc_batch_init_episode(seed, 0), then the settle steps of the task
 * (dmc_batch_step without controls or outputs: `settle_nsub` substeps under `step_flags`,
 * the DMC_STEP_* bits without DMC_STEP_OUTPUTS) -- depends on the seed, the model and the
 * task data alone, not on anything the current episode computes.  A prefetch runs those
 * launches on a side stream of the lowest priority into shadow copies of every field they
 * write (state, warm start, time, data.ctrl, task data, warning mask, stats, episode
 * return, and DMC_FIELD_QACC with the auxiliary outputs on) and of the workspace; the
 * model parameters and task parameters are read from the batch.  With fewer workgroups
 * than compute units (one env per lane: up to 64 envs per CU) it occupies units the step
 * launches leave empty.
 *
 * dmc_batch_episode_prefetch records the request; it is issued from inside the
 * dmc_batch_step / _step_n / _rollout call that brings the control steps issued since
 * the request to `after_steps` (0: at once), ordered behind what the batch's stream holds
 * at that moment.  (A prefetch issued right after a reset would still be running at the
 * caller's next device-wide synchronisation, and be paid for there.)  A new request
 * replaces an earlier one.  Refused with a message while an env mask is set or per-env
 * episodes are enabled, and for step_flags with DMC_STEP_OUTPUTS.
 *
 * dmc_batch_episode_take returns 1 after making the batch's stream wait for a prefetch
 * issued with exactly these arguments (an event; the host does not wait) and copying the
 * shadows over the fields, device to device, on the batch's stream: the fields then hold,
 * bit for bit, what dmc_batch_init_episode(seed, 0) and the settle step leave after a
 * dmc_batch_reset.  Pointers handed out by dmc_batch_device_ptr stay valid.  It returns 0,
 * and forgets the request, when there is nothing usable (none issued yet, other arguments,
 * or dropped): the caller then runs the ordinary launches.  -1 is an error.
 *
 * A request is dropped (after waiting for the side stream) by whatever changes the
 * prefetch's inputs or the launches of a reset: dmc_batch_write of task data or model
 * parameters, dmc_batch_copy_state into the batch, dmc_batch_set_task_params,
 * dmc_batch_set_aux_outputs, dmc_batch_set_masked(on), dmc_batch_episodes_enable and
 * dmc_batch_set_stream.  A write to task data through dmc_batch_device_ptr is not seen:
 * follow it with a new request.  A step call that issues the prefetch records an event
 * and launches on a second stream: not inside a stream capture. */
int dmc_batch_episode_prefetch(dmc_batch* batch, uint64_t seed, int settle_nsub,
                               int step_flags, long long after_steps);
int dmc_batch_episode_take(dmc_batch* batch, uint64_t seed, int settle_nsub, int step_flags);

/* Rollouts (version 104): T control steps in one launch per chunk of at most
 * DMC_SEQ_LAUNCH_MAX_STEPS, with every step's reward, observation and control
 * recorded, and optionally the controls computed on the device by an MLP over the
 * observation.  Needs a code object built as a rollout build of the
 * one-env-per-lane kernel (build.build_model(..., rollout=True)); its capability
 * word is dmc_model_rollout_caps (0: the code object takes no rollouts).
 *
 * Control of step t = policy(o_t) if `policy` is given, plus ctrl[t] if `ctrl` is
 * given (the exploration term of a closed-loop rollout, or the whole action of an
 * open-loop one); with neither, the held control.  o_0 is DMC_FIELD_OBS as the
 * batch holds it, o_t the observation after step t-1.  A NaN / inf control raises
 * DMC_WARN_BADCTRL and is applied as zeros, like a loaded one.
 *
 * policy: device memory, elements of the code object's real type, shared by the
 * batch: per layer W[out][in] row-major then b[out]; `nlayers` (1 or 2) tanh layers
 * of width[l] units (each <= the cap in the capability word), then a linear layer
 * of width[nlayers] units, which must be the model's nu.
 * Outputs (device memory, each may be NULL; strides in reals between steps):
 *   reward_out + t*reward_stride_t   [nenv]        reward of the state after step t
 *   obs_out    + t*obs_stride_t      [nenv][nobs]  its observation
 *   action_out + t*action_stride_t   [nenv][nu]    the control of step t, before the
 *                                                  ctrlrange clamp and the bad-control check
 *                                                  (not written when the held control is used)
 * The fields afterwards are those of `nsteps` calls of dmc_batch_step (the last
 * step's outputs, DMC_FIELD_RETURN with every reward added); one call of T steps
 * equals T calls of one step bit for bit.  Lock-step only: refused for a batch with
 * per-env episodes enabled or an env mask set.  The batch timer counts control steps. */
enum dmc_rollout_cap {
  DMC_ROLLOUT_OUTPUTS = 1,        /* per-step outputs */
  DMC_ROLLOUT_POLICY = 2,         /* device MLP policy */
  DMC_ROLLOUT_POPULATION = 4,     /* one policy per group of envs (version 106) */
  DMC_ROLLOUT_WIDTH_SHIFT = 8     /* caps >> 8: the widest hidden layer */
};
typedef struct dmc_rollout {
  int nsteps, nsub;
  const void* ctrl;               /* element (t, k, env) at ctrl[t*ctrl_stride_t + k*ctrl_stride_k
                                     + env*ctrl_stride_env]; NULL: none */
  long long ctrl_stride_k, ctrl_stride_env, ctrl_stride_t;
  const void* policy;             /* NULL: no policy */
  int nlayers, width[3];          /* hidden widths, then width[nlayers] = the output width */
  void* reward_out;
  long long reward_stride_t;
  void* obs_out;
  long long obs_stride_t;
  void* action_out;
  long long action_stride_t;
} dmc_rollout;
int dmc_model_rollout_caps(const dmc_model* model);
int dmc_batch_rollout(dmc_batch* batch, const dmc_rollout* rollout);
/* Populations (version 106): the same rollout with `members` = P policies of one shape
 * (evolution strategies, population-based training, sweeps, K checkpoints).  The nenv
 * envs are split into P groups of nenv/P consecutive envs, and env e acts with member
 * m = e / (nenv/P).  rollout->policy then holds [nparams][P] elements of the code
 * object's real type, one column per member: word j of member m at policy[j*P + m],
 * with j running over the packed order of a single policy (per layer W[out][in]
 * row-major, then b[out]).  P = 1 is the flat block of dmc_batch_rollout, which is this
 * call with members = 1.  Needs a code object whose capability word has
 * DMC_ROLLOUT_POPULATION (build.build_model(..., rollout=True, population=True)) for
 * members > 1; members < 1 and a member count that does not divide nenv are refused.
 * A member whose weights make a control NaN / inf raises DMC_WARN_BADCTRL in its own
 * envs only. */
int dmc_batch_rollout_population(dmc_batch* batch, const dmc_rollout* rollout, int members);

/* timing of the step kernel on the batch's own stream (HIP events around the
 * launches issued since dmc_batch_timer_start); returns accumulated device
 * milliseconds and the number of launches */
int dmc_batch_timer_start(dmc_batch* batch);
int dmc_batch_timer_stop(dmc_batch* batch, double* ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_HIP_H_ */
