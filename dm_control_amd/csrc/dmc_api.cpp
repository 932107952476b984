// dmc_api.cpp -- host runtime behind the C ABI of include/dmc_hip.h.
//
// Owns: the HIP module of a model-specialised code object, the HBM-resident
// struct-of-arrays state of a batch, one HIP stream per batch (and the side stream
// and shadow buffers of an episode prefetch), and the launch of the step / observe /
// init kernels.  No torch types, no CPU fallback: if
// HIP or the code object is unavailable every call fails with a message.
//
// Reference counterparts: wrapper/core.py (MjModel :444-627, MjData :630-776,
// error convention :85-101,312-328) and engine.py:149-166,268-305.

#include "../../include/dmc_hip.h"

#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "dmc_args.h"
static_assert(DMC_EP_DONE_LIMIT == DMC_DONE_LIMIT && DMC_EP_DONE_BAD_STATE == DMC_DONE_BAD_STATE,
              "the done bits of the header are the kernels'");

namespace {

thread_local std::string g_error;

int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
  return -1;
}

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t err_ = (expr);                                                \
    if (err_ != hipSuccess) {                                                \
      (void)hipGetLastError(); /* do not leak sticky state to other users */ \
      return fail("%s failed: %s", #expr, hipGetErrorString(err_));          \
    }                                                                        \
  } while (0)

}  // namespace

struct dmc_model {
  int device = 0;
  hipModule_t module = nullptr;
  hipFunction_t k_step = nullptr, k_observe = nullptr, k_init = nullptr;
  dmc_model_info info{};
  int episode_caps = 0;   // DMC_FLAG_* bits of the code object's dmc_episode_caps (0: it has none)
  int rollout_caps = 0;   // the code object's dmc_rollout_caps (0: not a rollout build)
};

struct dmc_batch {
  const dmc_model* model = nullptr;
  int nenv = 0;
  hipStream_t stream = nullptr;       // stream in use (own or caller's)
  hipStream_t own_stream = nullptr;   // created with the batch
  void* field[DMC_FIELD_COUNT] = {};
  size_t bytes[DMC_FIELD_COUNT] = {};
  size_t rows[DMC_FIELD_COUNT] = {};   // k extent of the field (1: per-env scalar)
  size_t elem[DMC_FIELD_COUNT] = {};   // bytes per element
  void* ws = nullptr;
  void* ctrl_staging = nullptr;   // device copy of host-provided controls
  size_t ctrl_staging_bytes = 0;
  int task_param_i = 0;
  bool aux_outputs = false;
  double task_param_r[4] = {0, 0, 0, 0};
  // per-env episodes: device int32[nenv] arrays indexed by dmc_episode_array
  int* episode[DMC_EPISODE_COUNT] = {};
  bool episodes = false;   // init and output-producing steps carry DMC_FLAG_EPISODES
  bool masked = false;     // init, forward and step carry DMC_FLAG_MASKED
  int step_limit = 0;
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timing = false;
  long long launches = 0;
  size_t ws_bytes = 0;
  // episode prefetch (dmc_batch_episode_prefetch): the request, and what its first
  // issue allocates -- side stream, events, shadow fields and shadow workspace
  struct Prefetch {
    enum State { NONE, PENDING, ISSUED } state = NONE;
    uint64_t seed = 0;
    int nsub = 0, step_flags = 0;
    long long after_steps = 0, issued = 0;   // control steps: asked for, seen since the request
    bool qacc = false;                       // the settle launch stored DMC_FIELD_QACC
    hipStream_t side = nullptr;
    hipEvent_t ready = nullptr;    // on the batch's stream: what the issue is ordered behind
    hipEvent_t done = nullptr;     // on the side stream: the shadows are complete
    void* field[DMC_FIELD_COUNT] = {};
    void* ws = nullptr;
  } prefetch;
};

namespace {

// Every dmc_field, in enum order: what dmc_batch_create allocates and what
// read / write / set_state may do with it.
enum Kind { REAL, INT32, UINT32 };
struct Field {
  dmc_field id;
  int dmc_model_info::*count;   // the member that counts the rows (nullptr: one)
  int mult;                     // rows per count
  bool pad;                     // an empty count still has one row
  Kind kind;
  bool writable;   // by dmc_batch_write: the state, task data, model parameters and
                   // what else a checkpoint restores (control, return, warning mask)
  bool agent;      // [nenv][k] in every code object, never flipped
};
using Info = dmc_model_info;
constexpr Field FIELDS[] = {
    {DMC_FIELD_QPOS, &Info::nq, 1, true, REAL, true, false},
    {DMC_FIELD_QVEL, &Info::nv, 1, true, REAL, true, false},
    {DMC_FIELD_WARMSTART, &Info::nv, 1, true, REAL, true, false},
    {DMC_FIELD_TIME, nullptr, 1, false, REAL, true, false},
    {DMC_FIELD_CTRL, &Info::nu, 1, true, REAL, true, false},
    {DMC_FIELD_OBS, &Info::nobs, 1, true, REAL, false, true},
    {DMC_FIELD_REWARD, nullptr, 1, false, REAL, false, false},
    {DMC_FIELD_SENSORDATA, &Info::nsensordata, 1, true, REAL, false, false},
    {DMC_FIELD_XPOS, &Info::nbody, 3, false, REAL, false, false},
    {DMC_FIELD_XMAT, &Info::nbody, 9, false, REAL, false, false},
    {DMC_FIELD_QACC, &Info::nv, 1, true, REAL, false, false},
    {DMC_FIELD_WARN, nullptr, 1, false, UINT32, true, false},
    {DMC_FIELD_STATS, nullptr, 3, false, INT32, false, false},
    {DMC_FIELD_RETURN, nullptr, 1, false, REAL, true, false},
    {DMC_FIELD_TASKDATA, &Info::ntaskdata, 1, true, REAL, true, false},
    {DMC_FIELD_MODELPARAM, &Info::nmodelparam, 1, true, REAL, true, false},
};
static_assert(sizeof FIELDS/sizeof FIELDS[0] == DMC_FIELD_COUNT, "one row per dmc_field");
constexpr bool fields_in_enum_order(int f = 0) {
  return f == DMC_FIELD_COUNT || (FIELDS[f].id == f && fields_in_enum_order(f + 1));
}
static_assert(fields_in_enum_order(), "FIELDS[f] describes field f");

// code objects with env-major state keep a 2-D field as [nenv][k] in HBM while
// the ABI presents [k][nenv]
bool flipped(const dmc_batch* b, int f) {
  return b->model->info.env_major && !FIELDS[f].agent && b->rows[f] > 1;
}

enum Shape { TASK_SETUP, MODEL_SHAPED };

int launch_on(dmc_batch* b, hipStream_t stream, hipFunction_t fn, DmcArgs& args, Shape shape) {
  size_t size = sizeof(DmcArgs);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args,
                    HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  // TASK_SETUP (dmc_init_episode): always one env per lane of a full wave.
  // MODEL_SHAPED (dmc_step, dmc_observe): the shape the code object reports in
  // dmc_info -- envs_per_block envs per workgroup, lanes_per_env lanes each (one
  // lane, a group within a wavefront, or two wavefronts per env).
  const dmc_model_info& mi = b->model->info;
  unsigned block = 64, per_block = 64;
  if (shape == MODEL_SHAPED) {
    per_block = (unsigned)mi.envs_per_block;
    block = (unsigned)(mi.lanes_per_env*mi.envs_per_block);
  }
  const unsigned grid = (unsigned)((b->nenv + per_block - 1)/per_block);
  HIP_TRY(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, stream,
                                nullptr, config));
  return 0;
}

int launch(dmc_batch* b, hipFunction_t fn, DmcArgs& args, Shape shape) {
  return launch_on(b, b->stream, fn, args, shape);
}

// [rows][n] <-> [n][rows] on the host (elements of `elem` bytes), see `flipped`
void transpose_host(const char* src, char* dst, size_t src_rows, size_t src_cols,
                    size_t elem) {
  for (size_t r = 0; r < src_rows; r++)
    for (size_t c = 0; c < src_cols; c++)
      memcpy(dst + (c*src_rows + r)*elem, src + (r*src_cols + c)*elem, elem);
}

void fill_args(dmc_batch* b, DmcArgs& a) {
  memset(&a, 0, sizeof a);
  a.nenv = b->nenv;
  a.nsub = 1;
  a.task_param_i = b->task_param_i;
  memcpy(a.task_param_r, b->task_param_r, sizeof a.task_param_r);
  a.qpos = b->field[DMC_FIELD_QPOS];
  a.qvel = b->field[DMC_FIELD_QVEL];
  a.warm = b->field[DMC_FIELD_WARMSTART];
  a.time = b->field[DMC_FIELD_TIME];
  a.ctrl_store = b->field[DMC_FIELD_CTRL];
  a.obs = b->field[DMC_FIELD_OBS];
  a.obs_sk = 1;                       // agent layout [nenv][nobs]
  a.obs_se = b->model->info.nobs;
  a.reward = b->field[DMC_FIELD_REWARD];
  a.episode_return = b->field[DMC_FIELD_RETURN];
  a.taskdata = b->field[DMC_FIELD_TASKDATA];
  a.modelparam = b->field[DMC_FIELD_MODELPARAM];
  a.sensordata = b->field[DMC_FIELD_SENSORDATA];
  a.xpos = b->aux_outputs ? b->field[DMC_FIELD_XPOS] : nullptr;
  a.xmat = b->aux_outputs ? b->field[DMC_FIELD_XMAT] : nullptr;
  a.qacc = b->aux_outputs ? b->field[DMC_FIELD_QACC] : nullptr;
  a.warn = (unsigned*)b->field[DMC_FIELD_WARN];
  a.stats = (int*)b->field[DMC_FIELD_STATS];
  a.ws = b->ws;
  a.env_mask = b->episode[DMC_EPISODE_MASK];
  a.ep_step = b->episode[DMC_EPISODE_STEP];
  a.ep_done = b->episode[DMC_EPISODE_DONE];
  a.step_limit = b->step_limit;
  if (b->masked) a.flags |= DMC_FLAG_MASKED;   // (callers OR their own bits into `flags`)
}

// the episode block: allocated (and zeroed, on the batch's stream) on first use
int episode_block(dmc_batch* b, const char* who) {
  const int need = DMC_FLAG_MASKED | DMC_FLAG_EPISODES | DMC_FLAG_ZERO_TIME;
  if ((b->model->episode_caps & need) != need)
    return fail("%s: this code object does not take an env mask or per-env episodes "
                "(a team-mode build, or one built before version 103)", who);
  if (b->episode[0]) return 0;
  HIP_TRY(hipSetDevice(b->model->device));
  const size_t bytes = (size_t)b->nenv*sizeof(int);
  for (int k = 0; k < DMC_EPISODE_COUNT; k++) {
    HIP_TRY(hipMalloc((void**)&b->episode[k], bytes));
    HIP_TRY(hipMemsetAsync(b->episode[k], 0, bytes, b->stream));
  }
  return 0;
}

int episode_array(const dmc_batch* b, int which, size_t bytes, const char* who) {
  if (which < 0 || which >= DMC_EPISODE_COUNT) return fail("%s: unknown array %d", who, which);
  if (!b->episode[0]) return fail("%s: the batch has no episode block "
                                  "(dmc_batch_episodes_enable)", who);
  if (bytes != (size_t)b->nenv*sizeof(int))
    return fail("%s: the array has %zu bytes, caller passed %zu", who,
                (size_t)b->nenv*sizeof(int), bytes);
  return 0;
}

// -- episode prefetch ----------------------------------------------------------
// Every field that dmc_init_episode or a dmc_step without outputs writes (load_env /
// store_env and the tail of dmc_step in the kernel sources): what a prefetch shadows
// and a take copies back.  The workspace is shadowed whole: overflow rows of two
// concurrent launches must not collide, and a `mixed` build keeps the low words of
// its state there.
constexpr dmc_field SHADOWED[] = {
    DMC_FIELD_QPOS, DMC_FIELD_QVEL, DMC_FIELD_WARMSTART, DMC_FIELD_TIME, DMC_FIELD_CTRL,
    DMC_FIELD_QACC, DMC_FIELD_WARN, DMC_FIELD_STATS, DMC_FIELD_RETURN, DMC_FIELD_TASKDATA};

void prefetch_free(dmc_batch* b) {
  dmc_batch::Prefetch& p = b->prefetch;
  if (p.side) (void)hipStreamSynchronize(p.side);
  for (dmc_field f : SHADOWED)
    if (p.field[f]) (void)hipFree(p.field[f]);
  if (p.ws) (void)hipFree(p.ws);
  if (p.ready) (void)hipEventDestroy(p.ready);
  if (p.done) (void)hipEventDestroy(p.done);
  if (p.side) (void)hipStreamDestroy(p.side);
  p = dmc_batch::Prefetch();
}

// forgets the request; a prefetch that may still run (an issued one, or one that a
// take declined) is waited for first, so that the caller may change what it reads
int prefetch_drop(dmc_batch* b) {
  dmc_batch::Prefetch& p = b->prefetch;
  p.state = p.NONE;
  if (p.side) {
    HIP_TRY(hipSetDevice(b->model->device));
    HIP_TRY(hipStreamSynchronize(p.side));
  }
  return 0;
}

// side stream, events, shadows (`ws` last: it tells that all of them exist)
int prefetch_alloc(dmc_batch* b) {
  dmc_batch::Prefetch& p = b->prefetch;
  // the lowest priority: a step launch is never queued behind the settle
  int least = 0, greatest = 0;
  HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
  HIP_TRY(hipStreamCreateWithPriority(&p.side, hipStreamNonBlocking, least));
  HIP_TRY(hipEventCreateWithFlags(&p.ready, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&p.done, hipEventDisableTiming));
  for (dmc_field f : SHADOWED) {
    HIP_TRY(hipMalloc(&p.field[f], b->bytes[f]));
    HIP_TRY(hipMemsetAsync(p.field[f], 0, b->bytes[f], p.side));
  }
  void* ws = nullptr;
  HIP_TRY(hipMalloc(&ws, b->ws_bytes));
  p.ws = ws;
  HIP_TRY(hipMemsetAsync(p.ws, 0, b->ws_bytes, p.side));
  return 0;
}

// what a whole-batch reset launches, on the side stream into the shadows
int prefetch_issue(dmc_batch* b) {
  dmc_batch::Prefetch& p = b->prefetch;
  HIP_TRY(hipSetDevice(b->model->device));
  if (!p.ws && prefetch_alloc(b)) {
    prefetch_free(b);
    return -1;
  }
  // behind what the batch's stream holds now: the steps counted by `after_steps`,
  // a take that still copies from the shadows, launches that write the task data
  HIP_TRY(hipEventRecord(p.ready, b->stream));
  HIP_TRY(hipStreamWaitEvent(p.side, p.ready, 0));
  HIP_TRY(hipMemcpyAsync(p.field[DMC_FIELD_TASKDATA], b->field[DMC_FIELD_TASKDATA],
                         b->bytes[DMC_FIELD_TASKDATA], hipMemcpyDeviceToDevice, p.side));
  DmcArgs a;
  fill_args(b, a);   // (neither masked nor per-env episodes: the request was refused then)
  a.qpos = p.field[DMC_FIELD_QPOS];
  a.qvel = p.field[DMC_FIELD_QVEL];
  a.warm = p.field[DMC_FIELD_WARMSTART];
  a.time = p.field[DMC_FIELD_TIME];
  a.ctrl_store = p.field[DMC_FIELD_CTRL];
  a.episode_return = p.field[DMC_FIELD_RETURN];
  a.taskdata = p.field[DMC_FIELD_TASKDATA];
  a.warn = (unsigned*)p.field[DMC_FIELD_WARN];
  a.stats = (int*)p.field[DMC_FIELD_STATS];
  a.ws = p.ws;
  p.qacc = b->aux_outputs;
  a.qacc = p.qacc ? p.field[DMC_FIELD_QACC] : nullptr;
  a.xpos = a.xmat = nullptr;      // (outputs: none of these launches writes them)
  DmcArgs reset = a;              // dmc_batch_reset
  reset.flags = DMC_FLAG_RESET_ONLY;
  if (launch_on(b, p.side, b->model->k_init, reset, TASK_SETUP)) return -1;
  HIP_TRY(hipMemsetAsync(p.field[DMC_FIELD_WARN], 0, b->bytes[DMC_FIELD_WARN], p.side));
  HIP_TRY(hipMemsetAsync(p.field[DMC_FIELD_STATS], 0, b->bytes[DMC_FIELD_STATS], p.side));
  DmcArgs init = a;               // dmc_batch_init_episode(seed, 0)
  init.seed = p.seed;
  if (launch_on(b, p.side, b->model->k_init, init, TASK_SETUP)) return -1;
  DmcArgs settle = a;             // dmc_batch_step(NULL, ..., nsub, step_flags)
  settle.nsub = p.nsub;
  settle.nsteps = 1;
  settle.flags |= DMC_FLAG_NO_OUTPUT |
                  ((p.step_flags & DMC_STEP_STALE_FIRST) ? DMC_FLAG_STALE_FIRST : 0) |
                  ((p.step_flags & DMC_STEP_ZERO_TIME) ? DMC_FLAG_ZERO_TIME : 0);
  if (launch_on(b, p.side, b->model->k_step, settle, MODEL_SHAPED)) return -1;
  HIP_TRY(hipEventRecord(p.done, p.side));
  p.state = p.ISSUED;
  return 0;
}

// `nsteps` more control steps have been issued on the batch's stream
int prefetch_count(dmc_batch* b, int nsteps) {
  dmc_batch::Prefetch& p = b->prefetch;
  if (p.state != p.PENDING) return 0;
  p.issued += nsteps;
  if (p.issued < p.after_steps) return 0;
  if (prefetch_issue(b)) {
    p.state = p.NONE;    // (not tried again with every step)
    return -1;
  }
  return 0;
}

}  // namespace

extern "C" {

// 101: dmc_model_info.nmodelparam, DMC_FIELD_MODELPARAM; 102: dmc_model_info.seq_launch;
// 103: per-env episodes (dmc_batch_episodes_enable and what follows it in the header)
// 104: rollouts (dmc_model_rollout_caps, dmc_batch_rollout)
// 105: episode prefetch (dmc_batch_episode_prefetch, dmc_batch_episode_take)
int dmc_version(void) { return 105; }

const char* dmc_last_error(void) { return g_error.c_str(); }

int dmc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

namespace {

// shared by dmc_model_load (file) and dmc_model_load_data (memory image)
int load_model(const char* path, const void* image, int device_id, dmc_model** out);

// libhiprtc is opened on first use, so that the library loads (and every other
// entry point works) on systems without it
struct Hiprtc {
  void* lib = nullptr;
  decltype(&hiprtcCreateProgram) create = nullptr;
  decltype(&hiprtcCompileProgram) compile = nullptr;
  decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
  decltype(&hiprtcGetProgramLog) log = nullptr;
  decltype(&hiprtcGetCodeSize) code_size = nullptr;
  decltype(&hiprtcGetCode) code = nullptr;
  decltype(&hiprtcDestroyProgram) destroy = nullptr;
  decltype(&hiprtcGetErrorString) error_string = nullptr;
};

// Opens libhiprtc once (thread-safe: a function-local static is initialised
// exactly once) and keeps the reason when that fails -- dlerror() is cleared by
// the call that reads it and overwritten by any later dl* call, so it is read
// once, right where the failure happened.
struct HiprtcOnce {
  Hiprtc rtc{};
  std::string why;
  HiprtcOnce() {
    for (const char* name : {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"}) {
      rtc.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (rtc.lib) break;
      const char* e = dlerror();
      if (e) why = e;
    }
    if (!rtc.lib) {
      if (why.empty()) why = "dlopen failed";
      return;
    }
    why.clear();
#define DMC_SYM(field, symbol)                                              \
    if (rtc.lib) {                                                          \
      rtc.field = (decltype(rtc.field))dlsym(rtc.lib, #symbol);             \
      if (!rtc.field) {                                                     \
        const char* e = dlerror();                                          \
        why = e ? e : "symbol " #symbol " missing";                         \
        dlclose(rtc.lib);                                                   \
        rtc.lib = nullptr;                                                  \
      }                                                                     \
    }
    DMC_SYM(create, hiprtcCreateProgram)
    DMC_SYM(compile, hiprtcCompileProgram)
    DMC_SYM(log_size, hiprtcGetProgramLogSize)
    DMC_SYM(log, hiprtcGetProgramLog)
    DMC_SYM(code_size, hiprtcGetCodeSize)
    DMC_SYM(code, hiprtcGetCode)
    DMC_SYM(destroy, hiprtcDestroyProgram)
    DMC_SYM(error_string, hiprtcGetErrorString)
#undef DMC_SYM
  }
};

const HiprtcOnce* hiprtc_once() {
  static const HiprtcOnce once;
  return &once;
}

const Hiprtc* hiprtc() {
  const HiprtcOnce* o = hiprtc_once();
  return o->rtc.lib ? &o->rtc : nullptr;
}

}  // namespace

int dmc_model_compile(const char* source, const char* source_name,
                      const char* const* header_names,
                      const char* const* header_texts, int nheaders,
                      const char* const* options, int noptions,
                      void** code, size_t* code_size, char* log, size_t log_size) {
  if (log && log_size) log[0] = 0;
  if (!source || !code || !code_size || nheaders < 0 || noptions < 0 ||
      (nheaders && (!header_names || !header_texts)) || (noptions && !options))
    return fail("dmc_model_compile: bad argument");
  *code = nullptr;
  *code_size = 0;
  const Hiprtc* rtc = hiprtc();
  if (!rtc)
    return fail("dmc_model_compile: the HIP runtime-compilation library "
                "(libhiprtc) is not available: %s", hiprtc_once()->why.c_str());
  hiprtcProgram prog = nullptr;
  hiprtcResult rc = rtc->create(&prog, source, source_name ? source_name : "dmc_model.hip",
                                nheaders, const_cast<const char**>(header_texts),
                                const_cast<const char**>(header_names));
  if (rc != HIPRTC_SUCCESS)
    return fail("hiprtcCreateProgram failed: %s", rtc->error_string(rc));
  rc = rtc->compile(prog, noptions, const_cast<const char**>(options));
  size_t n = 0;
  if (log && log_size && rtc->log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) {
    std::vector<char> text(n + 1, 0);
    if (rtc->log(prog, text.data()) == HIPRTC_SUCCESS) {
      // keep the END of a long log: that is where the errors are
      const size_t keep = n < log_size ? n : log_size - 1;
      memcpy(log, text.data() + (n - keep), keep);
      log[keep] = 0;
    }
  }
  if (rc != HIPRTC_SUCCESS) {
    rtc->destroy(&prog);
    return fail("hiprtcCompileProgram failed: %s (see the log)", rtc->error_string(rc));
  }
  size_t size = 0;
  rc = rtc->code_size(prog, &size);
  void* buf = (rc == HIPRTC_SUCCESS && size) ? malloc(size) : nullptr;
  if (buf) rc = rtc->code(prog, (char*)buf);
  rtc->destroy(&prog);
  if (!buf || rc != HIPRTC_SUCCESS) {
    free(buf);
    return fail("hiprtcGetCode failed: %s", rtc->error_string(rc));
  }
  *code = buf;
  *code_size = size;
  return 0;
}

void dmc_code_free(void* code) { free(code); }

int dmc_model_load(const char* path, int device_id, dmc_model** out) {
  if (!path || !out) return fail("dmc_model_load: null argument");
  return load_model(path, nullptr, device_id, out);
}

int dmc_model_load_data(const void* code, size_t code_size, int device_id,
                        dmc_model** out) {
  if (!code || !code_size || !out) return fail("dmc_model_load_data: null argument");
  return load_model("<memory image>", code, device_id, out);
}

}  // extern "C"

namespace {

int load_model(const char* path, const void* image, int device_id, dmc_model** out) {
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail("dmc_model_load: no HIP device available (the physics step "
                "has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev)
    return fail("dmc_model_load: device %d out of range (%d devices)",
                device_id, ndev);
  HIP_TRY(hipSetDevice(device_id));
  dmc_model* m = new (std::nothrow) dmc_model;
  if (!m) return fail("out of host memory");
  m->device = device_id;
  hipError_t err = image ? hipModuleLoadData(&m->module, image)
                         : hipModuleLoad(&m->module, path);
  if (err != hipSuccess) {
    delete m;
    (void)hipGetLastError();   // clear the runtime's sticky last-error
    return fail("hipModuleLoad(%s) failed: %s", path, hipGetErrorString(err));
  }
  struct { const char* name; hipFunction_t* fn; } fns[] = {
      {"dmc_step", &m->k_step}, {"dmc_observe", &m->k_observe},
      {"dmc_init_episode", &m->k_init}};
  for (auto& f : fns) {
    err = hipModuleGetFunction(f.fn, m->module, f.name);
    if (err != hipSuccess) {
      (void)hipModuleUnload(m->module);
      delete m;
      (void)hipGetLastError();
      return fail("code object %s lacks kernel %s", path, f.name);
    }
  }
  hipDeviceptr_t dptr = nullptr;
  size_t bytes = 0;
  err = hipModuleGetGlobal(&dptr, &bytes, m->module, "dmc_info");
  DmcInfo d{};
  if (err == hipSuccess && bytes >= sizeof d)
    err = hipMemcpy(&d, dptr, sizeof d, hipMemcpyDeviceToHost);
  if (err != hipSuccess || d.abi != 1) {
    (void)hipModuleUnload(m->module);
    delete m;
    return fail("code object %s has no valid dmc_info table", path);
  }
  dmc_model_info& i = m->info;
  i.abi = d.abi; i.real_size = d.real_size; i.nq = d.nq; i.nv = d.nv;
  i.nu = d.nu; i.nbody = d.nbody; i.nobs = d.nobs; i.nsensordata = d.nsensordata;
  i.ws_per_env = d.ws_per_env; i.task = d.task; i.ncon_max = d.ncon_max;
  i.nefc_max = d.nefc_max; i.integrator = d.integrator; i.npair = d.npair;
  i.ntaskdata = d.ntaskdata;
  // one env per lane (64, 32 or 16 envs in a 64-wide wave) or a group of lanes per env
  i.envs_per_block = d.envs_per_block > 0 ? d.envs_per_block : 64;
  i.lanes_per_env = d.threads_per_block > i.envs_per_block
                        ? d.threads_per_block/i.envs_per_block : 1;
  i.env_major = d.env_major != 0;
  i.nmodelparam = d.nmodelparam > 0 ? d.nmodelparam : 0;
  i.seq_launch = d.seq_launch == 1;
  DmcEpisodeCaps caps = 0;
  if (hipModuleGetGlobal(&dptr, &bytes, m->module, "dmc_episode_caps") == hipSuccess &&
      bytes >= sizeof caps &&
      hipMemcpy(&caps, dptr, sizeof caps, hipMemcpyDeviceToHost) == hipSuccess)
    m->episode_caps = caps;
  else
    (void)hipGetLastError();   // an older code object: the episode entry points refuse it
  DmcRolloutCaps rcaps = 0;
  if (hipModuleGetGlobal(&dptr, &bytes, m->module, "dmc_rollout_caps") == hipSuccess &&
      bytes >= sizeof rcaps &&
      hipMemcpy(&rcaps, dptr, sizeof rcaps, hipMemcpyDeviceToHost) == hipSuccess)
    m->rollout_caps = rcaps;
  else
    (void)hipGetLastError();   // not a rollout build: dmc_batch_rollout refuses it
  *out = m;
  return 0;
}

}  // namespace

extern "C" {

int dmc_model_get_info(const dmc_model* model, dmc_model_info* info) {
  if (!model || !info) return fail("dmc_model_get_info: null argument");
  *info = model->info;
  return 0;
}

void dmc_model_free(dmc_model* m) {
  if (!m) return;
  if (m->module) (void)hipModuleUnload(m->module);
  delete m;
}

int dmc_batch_create(const dmc_model* model, int nenv, dmc_batch** out) {
  if (!model || !out) return fail("dmc_batch_create: null argument");
  if (nenv <= 0) return fail("dmc_batch_create: nenv must be positive");
  *out = nullptr;
  HIP_TRY(hipSetDevice(model->device));
  dmc_batch* b = new (std::nothrow) dmc_batch;
  if (!b) return fail("out of host memory");
  b->model = model;
  b->nenv = nenv;
  const dmc_model_info& i = model->info;
  const size_t rs = (size_t)i.real_size, n = (size_t)nenv;
  auto atleast1 = [](int v) { return (size_t)(v > 0 ? v : 1); };
  for (int f = 0; f < DMC_FIELD_COUNT; f++) {
    const Field& d = FIELDS[f];
    const size_t count = !d.count ? 1 : d.pad ? atleast1(i.*d.count) : (size_t)(i.*d.count);
    b->rows[f] = count*(size_t)d.mult;
    b->elem[f] = d.kind == REAL ? rs : d.kind == INT32 ? sizeof(int) : sizeof(unsigned);
    b->bytes[f] = b->rows[f]*n*b->elem[f];
  }
  hipError_t err = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  b->stream = b->own_stream;
  for (int f = 0; f < DMC_FIELD_COUNT && err == hipSuccess; f++) {
    err = hipMalloc(&b->field[f], b->bytes[f]);
    // on the batch's stream: it does not wait for the null stream (non-blocking),
    // so a hipMemset there could land after the launches below and after later writes
    if (err == hipSuccess) err = hipMemsetAsync(b->field[f], 0, b->bytes[f], b->stream);
  }
  // workspace: ws_per_env reals per env, laid out for the batch rounded up to
  // whole 64-env workgroups (surplus lanes of the last workgroup own a slot)
  const size_t npad = (n + 63)/64*64;
  b->ws_bytes = atleast1(i.ws_per_env)*npad*rs;
  if (err == hipSuccess)
    err = hipMalloc(&b->ws, b->ws_bytes);
  if (err == hipSuccess)
    err = hipMemsetAsync(b->ws, 0, b->ws_bytes, b->stream);
  if (err == hipSuccess) err = hipEventCreate(&b->ev0);
  if (err == hipSuccess) err = hipEventCreate(&b->ev1);
  if (err != hipSuccess) {
    dmc_batch_free(b);
    (void)hipGetLastError();
    return fail("dmc_batch_create: %s", hipGetErrorString(err));
  }
  *out = b;
  {   // per-instance task data and model parameters start from the compiled model's values
    DmcArgs a;
    fill_args(b, a);
    a.flags |= DMC_FLAG_RESET_ONLY | DMC_FLAG_TASKDATA_DEFAULT;
    if (launch(b, model->k_init, a, TASK_SETUP)) return -1;
  }
  return dmc_batch_reset(b);
}

void dmc_batch_free(dmc_batch* b) {
  if (!b) return;
  // (not a word about b->model: a caller may have freed the model first)
  prefetch_free(b);     // waits for the side stream: it reads the fields freed below
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (int f = 0; f < DMC_FIELD_COUNT; f++)
    if (b->field[f]) (void)hipFree(b->field[f]);
  if (b->ws) (void)hipFree(b->ws);
  if (b->ctrl_staging) (void)hipFree(b->ctrl_staging);
  for (int k = 0; k < DMC_EPISODE_COUNT; k++)
    if (b->episode[k]) (void)hipFree(b->episode[k]);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
}

int dmc_batch_nenv(const dmc_batch* b) { return b ? b->nenv : 0; }

int dmc_batch_set_aux_outputs(dmc_batch* b, int enabled) {
  if (!b) return fail("null batch");
  if (b->aux_outputs != (enabled != 0) && prefetch_drop(b)) return -1;   // (the settle stores qacc or not)
  b->aux_outputs = enabled != 0;
  return 0;
}

int dmc_batch_set_task_params(dmc_batch* b, int iparam, const double* r, int nr) {
  if (!b) return fail("null batch");
  if (nr < 0 || nr > 4) return fail("at most 4 real task parameters");
  if (prefetch_drop(b)) return -1;
  b->task_param_i = iparam;
  for (int k = 0; k < nr; k++) b->task_param_r[k] = r[k];
  return 0;
}

int dmc_batch_reset(dmc_batch* b) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  // mj_resetData: an init_episode launch with a task-less code path would
  // need the model tables; instead run dmc_init_episode with the task's part
  // masked off via DMC_FLAG_RESET_ONLY.
  DmcArgs a;
  fill_args(b, a);
  // (the whole batch, whatever dmc_batch_set_masked says; with episodes enabled
  // every env's step count and done bits restart with its state)
  a.flags = DMC_FLAG_RESET_ONLY | (b->episodes ? DMC_FLAG_EPISODES : 0);
  if (launch(b, b->model->k_init, a, TASK_SETUP)) return -1;
  HIP_TRY(hipMemsetAsync(b->field[DMC_FIELD_WARN], 0, b->bytes[DMC_FIELD_WARN],
                         b->stream));
  HIP_TRY(hipMemsetAsync(b->field[DMC_FIELD_STATS], 0,
                         b->bytes[DMC_FIELD_STATS], b->stream));
  return 0;
}

int dmc_batch_set_state(dmc_batch* b, const void* qpos, const void* qvel,
                        const void* warm, const void* time) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  struct { const void* src; int f; } items[] = {
      {qpos, DMC_FIELD_QPOS}, {qvel, DMC_FIELD_QVEL},
      {warm, DMC_FIELD_WARMSTART}, {time, DMC_FIELD_TIME}};
  std::vector<char> tmp;
  for (auto& it : items) {
    if (!it.src) continue;
    const void* src = it.src;
    if (flipped(b, it.f)) {
      tmp.resize(b->bytes[it.f]);
      transpose_host((const char*)it.src, tmp.data(), b->rows[it.f],
                     (size_t)b->nenv, b->elem[it.f]);
      src = tmp.data();
    }
    HIP_TRY(hipMemcpyAsync(b->field[it.f], src, b->bytes[it.f],
                           hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));   // `tmp` is reused
  }
  return 0;
}

int dmc_batch_write(dmc_batch* b, int field, const void* src, size_t bytes) {
  if (!b || !src) return fail("dmc_batch_write: null argument");
  if (field < 0 || field >= DMC_FIELD_COUNT || !FIELDS[field].writable)
    return fail("dmc_batch_write: field %d is not writable", field);
  if (bytes != b->bytes[field])
    return fail("dmc_batch_write: field %d has %zu bytes, caller passed %zu",
                field, b->bytes[field], bytes);
  HIP_TRY(hipSetDevice(b->model->device));
  if ((field == DMC_FIELD_TASKDATA || field == DMC_FIELD_MODELPARAM) && prefetch_drop(b))
    return -1;     // (a prefetch reads both)
  std::vector<char> tmp;
  if (flipped(b, field)) {
    tmp.resize(bytes);
    transpose_host((const char*)src, tmp.data(), b->rows[field], (size_t)b->nenv,
                   b->elem[field]);
    src = tmp.data();
  }
  HIP_TRY(hipMemcpyAsync(b->field[field], src, bytes, hipMemcpyHostToDevice,
                         b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int dmc_batch_init_episode(dmc_batch* b, uint64_t seed, int only_colliding) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  DmcArgs a;
  fill_args(b, a);
  a.seed = seed;
  a.flags |= (only_colliding ? DMC_FLAG_ONLY_COLLIDING : 0) |
             (b->episodes ? DMC_FLAG_EPISODES : 0);
  return launch(b, b->model->k_init, a, TASK_SETUP);
}

int dmc_batch_forward(dmc_batch* b, int count_contacts) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  DmcArgs a;
  fill_args(b, a);
  a.flags |= count_contacts ? DMC_FLAG_COUNT_CONTACTS : 0;
  return launch(b, b->model->k_observe, a, MODEL_SHAPED);
}

}  // extern "C"

namespace {

// one launch of dmc_step: `nsteps` control steps (more than one only on a code
// object with `seq_launch`), step t reading its controls at ctrl + t*stride_t
int step_launch(dmc_batch* b, const void* ctrl, long long stride_k,
                long long stride_env, long long stride_t, int nsteps, int on_device,
                int nsub, int want_outputs) {
  HIP_TRY(hipSetDevice(b->model->device));
  const dmc_model_info& i = b->model->info;
  DmcArgs a;
  fill_args(b, a);
  a.nsub = nsub;
  a.flags |= (want_outputs & DMC_STEP_OUTPUTS) ? (b->episodes ? DMC_FLAG_EPISODES : 0)
                                               : DMC_FLAG_NO_OUTPUT;
  if (want_outputs & DMC_STEP_STALE_FIRST) a.flags |= DMC_FLAG_STALE_FIRST;
  if (want_outputs & DMC_STEP_ZERO_TIME) {
    if (!(b->model->episode_caps & DMC_FLAG_ZERO_TIME))
      return fail("dmc_batch_step: this code object does not take DMC_STEP_ZERO_TIME "
                  "(a team-mode build, or one built before version 103)");
    a.flags |= DMC_FLAG_ZERO_TIME;
  }
  if (ctrl && i.nu > 0) {
    a.flags |= DMC_FLAG_CTRL;
    if (on_device) {
      a.ctrl = ctrl;
    } else {
      // host controls: extent = 1 + (nu-1)*sk + (nenv-1)*se reals
      const size_t extent = (size_t)(1 + (i.nu - 1)*stride_k +
                                     (long long)(b->nenv - 1)*stride_env);
      const size_t bytes = extent*(size_t)i.real_size;
      if (bytes > b->ctrl_staging_bytes) {
        if (b->ctrl_staging) HIP_TRY(hipFree(b->ctrl_staging));
        b->ctrl_staging = nullptr;
        HIP_TRY(hipMalloc(&b->ctrl_staging, bytes));
        b->ctrl_staging_bytes = bytes;
      }
      HIP_TRY(hipMemcpyAsync(b->ctrl_staging, ctrl, bytes,
                             hipMemcpyHostToDevice, b->stream));
      a.ctrl = b->ctrl_staging;
    }
    a.ctrl_sk = stride_k;
    a.ctrl_se = stride_env;
  }
  a.nsteps = nsteps;
  a.ctrl_st = stride_t;
  if (launch(b, b->model->k_step, a, MODEL_SHAPED)) return -1;
  if (b->timing) b->launches += nsteps;   // (the timer's average stays per control step)
  return prefetch_count(b, nsteps);
}

}  // namespace

extern "C" {

int dmc_batch_step(dmc_batch* b, const void* ctrl, long long stride_k,
                   long long stride_env, int on_device, int nsub,
                   int want_outputs) {
  if (!b) return fail("null batch");
  if (nsub < 0) return fail("nsub must be >= 0");
  return step_launch(b, ctrl, stride_k, stride_env, 0, 1, on_device, nsub, want_outputs);
}

int dmc_batch_step_n(dmc_batch* b, const void* ctrl, long long stride_k,
                     long long stride_env, long long stride_t, int nsteps,
                     int nsub, int want_outputs) {
  if (!b) return fail("null batch");
  if (!ctrl) return fail("dmc_batch_step_n: device controls required");
  if (nsteps < 0) return fail("nsteps must be >= 0");
  if (nsub < 0) return fail("nsub must be >= 0");
  const long long rs = (long long)b->model->info.real_size;
  // One launch per chunk of control steps where the code object loops over them
  // itself (bounded, so that no launch occupies a shared device for long), else
  // one launch per step.  DMC_STEP_STALE_FIRST is about the sequence's first step.
  // (with per-env episodes every control step is a launch: an env freezes between steps)
  const int chunk_max = b->model->info.seq_launch && !b->episodes ? DMC_SEQ_LAUNCH_MAX_STEPS : 1;
  for (int t = 0; t < nsteps;) {
    const int chunk = nsteps - t < chunk_max ? nsteps - t : chunk_max;
    if (step_launch(b, (const char*)ctrl + (long long)t*stride_t*rs, stride_k, stride_env,
                    stride_t, chunk, 1, nsub,
                    t == 0 ? want_outputs : want_outputs & ~DMC_STEP_STALE_FIRST))
      return -1;
    t += chunk;
  }
  return 0;
}

int dmc_model_rollout_caps(const dmc_model* model) { return model ? model->rollout_caps : 0; }

int dmc_batch_rollout(dmc_batch* b, const dmc_rollout* r) {
  if (!b || !r) return fail("dmc_batch_rollout: null argument");
  const dmc_model_info& i = b->model->info;
  const int caps = b->model->rollout_caps;
  if (!(caps & DMC_ROLLOUT_CAP_OUTPUTS))
    return fail("dmc_batch_rollout: this code object takes no rollouts; build the model "
                "with rollout=True (the one-env-per-lane kernel, -DDMC_ROLLOUT=1)");
  if (b->episodes || b->masked)
    return fail("dmc_batch_rollout: rollouts are lock-step; the batch has %s",
                b->episodes ? "per-env episodes enabled" : "an env mask set");
  if (r->nsteps < 0) return fail("dmc_batch_rollout: nsteps must be >= 0");
  if (r->nsub < 0) return fail("dmc_batch_rollout: nsub must be >= 0");
  if (r->policy) {
    const int cap = caps >> DMC_ROLLOUT_CAP_WIDTH_SHIFT;
    if (!(caps & DMC_ROLLOUT_CAP_POLICY))
      return fail("dmc_batch_rollout: this code object takes no policy");
    if (r->nlayers != 1 && r->nlayers != 2)
      return fail("dmc_batch_rollout: a policy has 1 or 2 hidden layers, not %d", r->nlayers);
    for (int l = 0; l < r->nlayers; l++)
      if (r->width[l] < 1 || r->width[l] > cap)
        return fail("dmc_batch_rollout: hidden layer %d has %d units; this code object "
                    "takes 1 to %d", l, r->width[l], cap);
    if (r->width[r->nlayers] != i.nu)
      return fail("dmc_batch_rollout: the policy puts out %d values, the model has %d controls",
                  r->width[r->nlayers], i.nu);
  }
  HIP_TRY(hipSetDevice(b->model->device));
  const long long rs = (long long)i.real_size;
  const auto at = [rs](const void* p, long long words) -> void* {
    return p ? (char*)p + words*rs : nullptr;
  };
  // one launch per chunk of control steps, every pointer advanced by the chunk
  for (int t = 0; t < r->nsteps;) {
    const int chunk = r->nsteps - t < DMC_SEQ_LAUNCH_MAX_STEPS ? r->nsteps - t
                                                               : DMC_SEQ_LAUNCH_MAX_STEPS;
    DmcArgs a;
    fill_args(b, a);
    a.nsub = r->nsub;
    a.nsteps = chunk;
    if (r->ctrl && i.nu > 0) {
      a.flags |= DMC_FLAG_CTRL;
      a.ctrl = at(r->ctrl, t*r->ctrl_stride_t);
      a.ctrl_sk = r->ctrl_stride_k;
      a.ctrl_se = r->ctrl_stride_env;
      a.ctrl_st = r->ctrl_stride_t;
    }
    if (r->policy && i.nu > 0) {
      a.flags |= DMC_FLAG_POLICY;
      a.policy = r->policy;
      a.policy_nlayers = r->nlayers;
      a.policy_width[0] = r->width[0];
      a.policy_width[1] = r->nlayers == 2 ? r->width[1] : 0;
    }
    a.reward_out = at(r->reward_out, t*r->reward_stride_t);
    a.reward_out_st = r->reward_stride_t;
    a.obs_out = at(r->obs_out, t*r->obs_stride_t);
    a.obs_out_st = r->obs_stride_t;
    a.action_out = i.nu > 0 ? at(r->action_out, t*r->action_stride_t) : nullptr;
    a.action_out_st = r->action_stride_t;
    if (launch(b, b->model->k_step, a, MODEL_SHAPED)) return -1;
    if (b->timing) b->launches += chunk;   // (the timer's average stays per control step)
    if (prefetch_count(b, chunk)) return -1;
    t += chunk;
  }
  return 0;
}

size_t dmc_batch_field_bytes(const dmc_batch* b, int field) {
  if (!b || field < 0 || field >= DMC_FIELD_COUNT) return 0;
  return b->bytes[field];
}

int dmc_batch_read(dmc_batch* b, int field, void* dst, size_t bytes) {
  if (!b || !dst) return fail("dmc_batch_read: null argument");
  if (field < 0 || field >= DMC_FIELD_COUNT) return fail("unknown field %d", field);
  if (bytes != b->bytes[field])
    return fail("dmc_batch_read: field %d has %zu bytes, caller asked for %zu",
                field, b->bytes[field], bytes);
  HIP_TRY(hipSetDevice(b->model->device));
  const bool flip = flipped(b, field);
  std::vector<char> tmp(flip ? bytes : 0);
  HIP_TRY(hipMemcpyAsync(flip ? (void*)tmp.data() : dst, b->field[field], bytes,
                         hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (flip)
    transpose_host(tmp.data(), (char*)dst, (size_t)b->nenv, b->rows[field],
                   b->elem[field]);
  return 0;
}

void* dmc_batch_device_ptr(dmc_batch* b, int field) {
  if (!b || field < 0 || field >= DMC_FIELD_COUNT) return nullptr;
  return b->field[field];
}

int dmc_batch_clear_warnings(dmc_batch* b) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipMemsetAsync(b->field[DMC_FIELD_WARN], 0, b->bytes[DMC_FIELD_WARN],
                         b->stream));
  return 0;
}

int dmc_batch_copy_state(dmc_batch* dst, const dmc_batch* src) {
  if (!dst || !src) return fail("null batch");
  if (dst->nenv != src->nenv || dst->model->info.nq != src->model->info.nq ||
      dst->model->info.real_size != src->model->info.real_size ||
      dst->model->info.env_major != src->model->info.env_major ||
      dst->model->info.ntaskdata != src->model->info.ntaskdata ||
      dst->model->info.nmodelparam != src->model->info.nmodelparam)
    return fail("dmc_batch_copy_state: incompatible batches");
  HIP_TRY(hipSetDevice(dst->model->device));
  if (prefetch_drop(dst)) return -1;    // (task data and model parameters change)
  HIP_TRY(hipStreamSynchronize(src->stream));
  for (int f = 0; f < DMC_FIELD_COUNT; f++)
    HIP_TRY(hipMemcpyAsync(dst->field[f], src->field[f], dst->bytes[f],
                           hipMemcpyDeviceToDevice, dst->stream));
  if (src->episode[0]) {
    if (episode_block(dst, "dmc_batch_copy_state")) return -1;
    for (int k = 0; k < DMC_EPISODE_COUNT; k++)
      HIP_TRY(hipMemcpyAsync(dst->episode[k], src->episode[k], (size_t)dst->nenv*sizeof(int),
                             hipMemcpyDeviceToDevice, dst->stream));
    dst->episodes = src->episodes;
    dst->step_limit = src->step_limit;
  }
  dst->task_param_i = src->task_param_i;
  dst->aux_outputs = src->aux_outputs;
  memcpy(dst->task_param_r, src->task_param_r, sizeof dst->task_param_r);
  HIP_TRY(hipStreamSynchronize(dst->stream));
  return 0;
}

int dmc_batch_episodes_enable(dmc_batch* b, int step_limit) {
  if (!b) return fail("null batch");
  if (episode_block(b, "dmc_batch_episodes_enable")) return -1;
  if (prefetch_drop(b)) return -1;      // (a whole-batch episode start no longer applies)
  b->episodes = true;
  b->step_limit = step_limit;
  return 0;
}

void* dmc_batch_episode_ptr(dmc_batch* b, int which) {
  if (!b || which < 0 || which >= DMC_EPISODE_COUNT) return nullptr;
  return b->episode[which];
}

int dmc_batch_episode_read(dmc_batch* b, int which, int* dst, size_t bytes) {
  if (!b || !dst) return fail("dmc_batch_episode_read: null argument");
  if (episode_array(b, which, bytes, "dmc_batch_episode_read")) return -1;
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipMemcpyAsync(dst, b->episode[which], bytes, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int dmc_batch_episode_write(dmc_batch* b, int which, const int* src, size_t bytes) {
  if (!b || !src) return fail("dmc_batch_episode_write: null argument");
  if (episode_array(b, which, bytes, "dmc_batch_episode_write")) return -1;
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipMemcpyAsync(b->episode[which], src, bytes, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int dmc_batch_mask_from_done(dmc_batch* b) {
  if (!b) return fail("null batch");
  if (episode_array(b, DMC_EPISODE_MASK, (size_t)b->nenv*sizeof(int), "dmc_batch_mask_from_done"))
    return -1;
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipMemcpyAsync(b->episode[DMC_EPISODE_MASK], b->episode[DMC_EPISODE_DONE],
                         (size_t)b->nenv*sizeof(int), hipMemcpyDeviceToDevice, b->stream));
  return 0;
}

int dmc_batch_set_masked(dmc_batch* b, int on) {
  if (!b) return fail("null batch");
  if (on && episode_block(b, "dmc_batch_set_masked")) return -1;
  if (on && prefetch_drop(b)) return -1;
  b->masked = on != 0;
  return 0;
}

int dmc_batch_episode_prefetch(dmc_batch* b, uint64_t seed, int settle_nsub, int step_flags,
                               long long after_steps) {
  if (!b) return fail("null batch");
  if (b->masked || b->episodes)
    return fail("dmc_batch_episode_prefetch: a prefetch is the start of a whole-batch "
                "episode; the batch has %s",
                b->episodes ? "per-env episodes enabled" : "an env mask set");
  if (settle_nsub < 0) return fail("dmc_batch_episode_prefetch: settle_nsub must be >= 0");
  if (after_steps < 0) return fail("dmc_batch_episode_prefetch: after_steps must be >= 0");
  if (step_flags & ~(DMC_STEP_STALE_FIRST | DMC_STEP_ZERO_TIME))
    return fail("dmc_batch_episode_prefetch: the settle steps take DMC_STEP_STALE_FIRST and "
                "DMC_STEP_ZERO_TIME, no outputs (step_flags %d)", step_flags);
  if ((step_flags & DMC_STEP_ZERO_TIME) && !(b->model->episode_caps & DMC_FLAG_ZERO_TIME))
    return fail("dmc_batch_episode_prefetch: this code object does not take DMC_STEP_ZERO_TIME "
                "(a team-mode build, or one built before version 103)");
  dmc_batch::Prefetch& p = b->prefetch;
  p.state = p.PENDING;      // (an earlier one is replaced; the side stream orders the two)
  p.seed = seed;
  p.nsub = settle_nsub;
  p.step_flags = step_flags;
  p.after_steps = after_steps;
  p.issued = 0;
  return prefetch_count(b, 0);
}

int dmc_batch_episode_take(dmc_batch* b, uint64_t seed, int settle_nsub, int step_flags) {
  if (!b) return fail("null batch");
  dmc_batch::Prefetch& p = b->prefetch;
  const bool usable = p.state == p.ISSUED && p.seed == seed && p.nsub == settle_nsub &&
                      p.step_flags == step_flags;
  p.state = p.NONE;         // taken, or stale from here on
  if (!usable) return 0;
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipStreamWaitEvent(b->stream, p.done, 0));
  for (dmc_field f : SHADOWED)
    if (f != DMC_FIELD_QACC || p.qacc)
      HIP_TRY(hipMemcpyAsync(b->field[f], p.field[f], b->bytes[f], hipMemcpyDeviceToDevice,
                             b->stream));
  HIP_TRY(hipMemcpyAsync(b->ws, p.ws, b->ws_bytes, hipMemcpyDeviceToDevice, b->stream));
  return 1;
}

int dmc_batch_sync(dmc_batch* b) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int dmc_batch_set_stream(dmc_batch* b, void* stream, int external) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (prefetch_drop(b)) return -1;
  b->stream = external ? (hipStream_t)stream : b->own_stream;
  return 0;
}

void* dmc_batch_stream(dmc_batch* b) { return b ? (void*)b->stream : nullptr; }

int dmc_batch_timer_start(dmc_batch* b) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipEventRecord(b->ev0, b->stream));
  b->timing = true;
  b->launches = 0;
  return 0;
}

int dmc_batch_timer_stop(dmc_batch* b, double* ms, long long* launches) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  HIP_TRY(hipEventRecord(b->ev1, b->stream));
  HIP_TRY(hipEventSynchronize(b->ev1));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, b->ev0, b->ev1));
  if (ms) *ms = t;
  if (launches) *launches = b->launches;
  b->timing = false;
  return 0;
}

}  // extern "C"
