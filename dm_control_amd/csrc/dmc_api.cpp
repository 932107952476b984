// dmc_api.cpp -- host runtime behind the C ABI of include/dmc_hip.h.
//
// Owns: the HIP module of a model-specialised code object, the HBM-resident
// struct-of-arrays state of a batch, one HIP stream per batch (and the side stream
// and shadow buffers of an episode prefetch), and the launch of the step / observe /
// init kernels.  What a launch looks like -- argument block, flags, chunks, grid --
// is decided in dmc_launch.h; here it is sent to a stream.  No torch types, no CPU
// fallback: if HIP or the code object is unavailable every call fails with a message.
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
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "dmc_launch.h"
static_assert(DMC_EP_DONE_LIMIT == DMC_DONE_LIMIT && DMC_EP_DONE_BAD_STATE == DMC_DONE_BAD_STATE,
              "the done bits of the header are the kernels'");

struct dmc_model : DmcCodeObject {
  int device = 0;
  hipModule_t module = nullptr;
  hipFunction_t k_step = nullptr, k_observe = nullptr, k_init = nullptr;
};

struct dmc_batch : DmcState, DmcTarget {   // (DmcTarget: its own `field[]` and `ws`)
  const dmc_model* model = nullptr;
  hipStream_t stream = nullptr;       // stream in use (own or caller's)
  hipStream_t own_stream = nullptr;   // created with the batch
  size_t bytes[DMC_FIELD_COUNT] = {};
  size_t rows[DMC_FIELD_COUNT] = {};   // k extent of the field (1: per-env scalar)
  size_t elem[DMC_FIELD_COUNT] = {};   // bytes per element
  void* ctrl_staging = nullptr;   // device copy of host-provided controls
  size_t ctrl_staging_bytes = 0;
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timing = false;
  long long launches = 0;
  size_t ws_bytes = 0;
  // episode prefetch (dmc_batch_episode_prefetch): the request, and what its first
  // issue allocates -- side stream, events, and the target of its launches: shadows
  // at the DMC_SHADOWED fields and `ws`, the batch's own elsewhere (share_unshadowed)
  struct Prefetch : DmcTarget {
    enum State { NONE, PENDING, ISSUED } state = NONE;
    uint64_t seed = 0;
    int nsub = 0, step_flags = 0;
    long long after_steps = 0, issued = 0;   // control steps: asked for, seen since the request
    bool qacc = false;                       // the settle launch stored DMC_FIELD_QACC
    hipStream_t side = nullptr;
    hipEvent_t ready = nullptr;    // on the batch's stream: what the issue is ordered behind
    hipEvent_t done = nullptr;     // on the side stream: the shadows are complete
  } prefetch;
};

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
  return b->code.info.env_major && !FIELDS[f].agent && b->rows[f] > 1;
}

int launch(dmc_batch* b, hipStream_t stream, hipFunction_t fn, const DmcArgs& args,
           DmcShape shape) {
  size_t size = sizeof(DmcArgs);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<DmcArgs*>(&args),   // (only read)
                    HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  const DmcGeometry g = geometry(*b, shape);
  HIP_TRY(hipModuleLaunchKernel(fn, g.grid, 1, 1, g.block, 1, 1, 0, stream,
                                nullptr, config));
  return 0;
}

// [rows][n] <-> [n][rows] on the host (elements of `elem` bytes), see `flipped`
void transpose_host(const char* src, char* dst, size_t src_rows, size_t src_cols,
                    size_t elem) {
  for (size_t r = 0; r < src_rows; r++)
    for (size_t c = 0; c < src_cols; c++)
      memcpy(dst + (c*src_rows + r)*elem, src + (r*src_cols + c)*elem, elem);
}

// host [k][nenv] -> the whole field; synchronises (the transposed copy lives until then)
int upload(dmc_batch* b, int f, const void* src) {
  std::vector<char> tmp;
  if (flipped(b, f)) {
    tmp.resize(b->bytes[f]);
    transpose_host((const char*)src, tmp.data(), b->rows[f], (size_t)b->nenv, b->elem[f]);
    src = tmp.data();
  }
  HIP_TRY(hipMemcpyAsync(b->field[f], src, b->bytes[f], hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// the whole field -> host [k][nenv]; synchronises the batch's stream
int download(dmc_batch* b, int f, void* dst) {
  const bool flip = flipped(b, f);
  std::vector<char> tmp(flip ? b->bytes[f] : 0);
  HIP_TRY(hipMemcpyAsync(flip ? (void*)tmp.data() : dst, b->field[f], b->bytes[f],
                         hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (flip)
    transpose_host(tmp.data(), (char*)dst, (size_t)b->nenv, b->rows[f], b->elem[f]);
  return 0;
}

// mj_resetData of a target on a stream: the batch's own, or a prefetch's
int reset_on(dmc_batch* b, const DmcTarget& t, hipStream_t stream) {
  if (launch(b, stream, b->model->k_init, reset_args(*b, t), TASK_SETUP)) return -1;
  HIP_TRY(hipMemsetAsync(t.field[DMC_FIELD_WARN], 0, b->bytes[DMC_FIELD_WARN], stream));
  HIP_TRY(hipMemsetAsync(t.field[DMC_FIELD_STATS], 0, b->bytes[DMC_FIELD_STATS], stream));
  return 0;
}

int zero_time_refused(const dmc_batch* b, int step_flags, const char* who) {
  if ((step_flags & DMC_STEP_ZERO_TIME) && !(b->code.episode_caps & DMC_FLAG_ZERO_TIME))
    return fail("%s: this code object does not take DMC_STEP_ZERO_TIME "
                "(a team-mode build, or one built before version 103)", who);
  return 0;
}

// the episode block: allocated (and zeroed, on the batch's stream) on first use
int episode_block(dmc_batch* b, const char* who) {
  const int need = DMC_FLAG_MASKED | DMC_FLAG_EPISODES | DMC_FLAG_ZERO_TIME;
  if ((b->code.episode_caps & need) != need)
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

// dmc_batch_episode_read (`dst`) and _write (`src`): a whole array, synchronised
int episode_copy(dmc_batch* b, int which, int* dst, const int* src, size_t bytes,
                 const char* who) {
  if (!b || !(dst || src)) return fail("%s: null argument", who);
  if (episode_array(b, which, bytes, who)) return -1;
  HIP_TRY(hipSetDevice(b->model->device));
  if (dst)
    HIP_TRY(hipMemcpyAsync(dst, b->episode[which], bytes, hipMemcpyDeviceToHost, b->stream));
  else
    HIP_TRY(hipMemcpyAsync(b->episode[which], src, bytes, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// -- episode prefetch ----------------------------------------------------------
void prefetch_free(dmc_batch* b) {
  dmc_batch::Prefetch& p = b->prefetch;
  if (p.side) (void)hipStreamSynchronize(p.side);
  for (dmc_field f : DMC_SHADOWED)
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
  share_unshadowed(p, *b);
  for (dmc_field f : DMC_SHADOWED) {
    HIP_TRY(hipMalloc(&p.field[f], b->bytes[f]));
    HIP_TRY(hipMemsetAsync(p.field[f], 0, b->bytes[f], p.side));
  }
  void* ws = nullptr;
  HIP_TRY(hipMalloc(&ws, b->ws_bytes));
  p.ws = ws;
  HIP_TRY(hipMemsetAsync(p.ws, 0, b->ws_bytes, p.side));
  return 0;
}

// what a whole-batch reset launches -- dmc_batch_reset, dmc_batch_init_episode(seed, 0),
// dmc_batch_step(NULL, ..., nsub, step_flags) -- on the side stream into the shadows
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
  p.qacc = b->aux_outputs;
  // (neither masked nor per-env episodes: the request was refused, or dropped, then)
  if (reset_on(b, p, p.side) ||
      launch(b, p.side, b->model->k_init, init_episode_args(*b, p, p.seed, false), TASK_SETUP) ||
      launch(b, p.side, b->model->k_step,
             step_args(*b, p, p.step_flags, nullptr, 0, 0, 0, 0, 1, p.nsub), MODEL_SHAPED))
    return -1;
  HIP_TRY(hipEventRecord(p.done, p.side));
  p.state = p.ISSUED;
  return 0;
}

// `nsteps` more control steps have been issued on the batch's stream: the timer's
// count (its average stays per control step), and a pending prefetch's
int steps_issued(dmc_batch* b, int nsteps) {
  dmc_batch::Prefetch& p = b->prefetch;
  if (b->timing) b->launches += nsteps;
  if (p.state != p.PENDING) return 0;
  p.issued += nsteps;
  if (p.issued < p.after_steps) return 0;
  if (prefetch_issue(b)) {
    p.state = p.NONE;    // (not tried again with every step)
    return -1;
  }
  return 0;
}

// `nsteps` control steps on the batch's stream, one launch per chunk (chunk_max),
// step t reading its controls at ctrl + t*stride_t
int step_run(dmc_batch* b, const void* ctrl, long long stride_k, long long stride_env,
             long long stride_t, int nsteps, int on_device, int nsub, int want_outputs) {
  if (nsub < 0) return fail("nsub must be >= 0");
  if (nsteps == 0) return 0;
  HIP_TRY(hipSetDevice(b->model->device));
  if (zero_time_refused(b, want_outputs, "dmc_batch_step")) return -1;
  const dmc_model_info& i = b->code.info;
  if (ctrl && i.nu > 0 && !on_device) {
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
    HIP_TRY(hipMemcpyAsync(b->ctrl_staging, ctrl, bytes, hipMemcpyHostToDevice, b->stream));
    ctrl = b->ctrl_staging;
  }
  const int max = chunk_max(*b, false);
  for (int t = 0, chunk; t < nsteps; t += chunk) {
    chunk = next_chunk(t, nsteps, max);
    const DmcArgs a = step_args(*b, *b, want_outputs, ctrl, stride_k, stride_env, stride_t, t,
                                chunk, nsub);
    if (launch(b, b->stream, b->model->k_step, a, MODEL_SHAPED) || steps_issued(b, chunk))
      return -1;
  }
  return 0;
}

// the module's device global `name`; false, and no sticky error left, if it has none
template <class T>
bool read_global(hipModule_t module, const char* name, T* value) {
  hipDeviceptr_t dptr = nullptr;
  size_t bytes = 0;
  if (hipModuleGetGlobal(&dptr, &bytes, module, name) == hipSuccess && bytes >= sizeof *value &&
      hipMemcpy(value, dptr, sizeof *value, hipMemcpyDeviceToHost) == hipSuccess)
    return true;
  (void)hipGetLastError();
  return false;
}

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
  // a failure below releases what is open and clears the runtime's sticky last-error
  const auto give_up = [](dmc_model* m) { dmc_model_free(m); (void)hipGetLastError(); };
  std::unique_ptr<dmc_model, decltype(give_up)> m(new (std::nothrow) dmc_model, give_up);
  if (!m) return fail("out of host memory");
  m->device = device_id;
  hipError_t err = image ? hipModuleLoadData(&m->module, image)
                         : hipModuleLoad(&m->module, path);
  if (err != hipSuccess)
    return fail("hipModuleLoad(%s) failed: %s", path, hipGetErrorString(err));
  struct { const char* name; hipFunction_t* fn; } fns[] = {
      {"dmc_step", &m->k_step}, {"dmc_observe", &m->k_observe},
      {"dmc_init_episode", &m->k_init}};
  for (auto& f : fns)
    if (hipModuleGetFunction(f.fn, m->module, f.name) != hipSuccess)
      return fail("code object %s lacks kernel %s", path, f.name);
  DmcInfo d{};
  if (!read_global(m->module, "dmc_info", &d) || d.abi != 1)
    return fail("code object %s has no valid dmc_info table", path);
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
  // absent (0) in an older code object: the episode entry points refuse it; in one
  // that is no rollout build: dmc_batch_rollout refuses it
  (void)read_global(m->module, "dmc_episode_caps", &m->episode_caps);
  (void)read_global(m->module, "dmc_rollout_caps", &m->rollout_caps);
  *out = m.release();
  return 0;
}

}  // namespace

extern "C" {

// 101: dmc_model_info.nmodelparam, DMC_FIELD_MODELPARAM; 102: dmc_model_info.seq_launch;
// 103: per-env episodes (dmc_batch_episodes_enable and what follows it in the header)
// 104: rollouts (dmc_model_rollout_caps, dmc_batch_rollout)
// 105: episode prefetch (dmc_batch_episode_prefetch, dmc_batch_episode_take)
// 106: populations of policies (dmc_batch_rollout_population)
int dmc_version(void) { return 106; }

const char* dmc_last_error(void) { return g_error.c_str(); }

int dmc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

namespace {

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
  b->code = *model;
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
  if (launch(b, b->stream, model->k_init, create_defaults_args(*b, *b), TASK_SETUP)) return -1;
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
  return reset_on(b, *b, b->stream);
}

int dmc_batch_set_state(dmc_batch* b, const void* qpos, const void* qvel,
                        const void* warm, const void* time) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  struct { const void* src; int f; } items[] = {
      {qpos, DMC_FIELD_QPOS}, {qvel, DMC_FIELD_QVEL},
      {warm, DMC_FIELD_WARMSTART}, {time, DMC_FIELD_TIME}};
  for (auto& it : items)
    if (it.src && upload(b, it.f, it.src)) return -1;
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
  return upload(b, field, src);
}

int dmc_batch_init_episode(dmc_batch* b, uint64_t seed, int only_colliding) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  return launch(b, b->stream, b->model->k_init,
                init_episode_args(*b, *b, seed, only_colliding != 0), TASK_SETUP);
}

int dmc_batch_forward(dmc_batch* b, int count_contacts) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->model->device));
  return launch(b, b->stream, b->model->k_observe, forward_args(*b, *b, count_contacts != 0),
                MODEL_SHAPED);
}

int dmc_batch_step(dmc_batch* b, const void* ctrl, long long stride_k,
                   long long stride_env, int on_device, int nsub,
                   int want_outputs) {
  if (!b) return fail("null batch");
  return step_run(b, ctrl, stride_k, stride_env, 0, 1, on_device, nsub, want_outputs);
}

int dmc_batch_step_n(dmc_batch* b, const void* ctrl, long long stride_k,
                     long long stride_env, long long stride_t, int nsteps,
                     int nsub, int want_outputs) {
  if (!b) return fail("null batch");
  if (!ctrl) return fail("dmc_batch_step_n: device controls required");
  if (nsteps < 0) return fail("nsteps must be >= 0");
  return step_run(b, ctrl, stride_k, stride_env, stride_t, nsteps, 1, nsub, want_outputs);
}

int dmc_model_rollout_caps(const dmc_model* model) { return model ? model->rollout_caps : 0; }

int dmc_batch_rollout(dmc_batch* b, const dmc_rollout* r) {
  return dmc_batch_rollout_population(b, r, 1);
}

int dmc_batch_rollout_population(dmc_batch* b, const dmc_rollout* r, int members) {
  if (!b || !r) return fail("dmc_batch_rollout: null argument");
  const dmc_model_info& i = b->code.info;
  const int caps = b->code.rollout_caps;
  if (!(caps & DMC_ROLLOUT_CAP_OUTPUTS))
    return fail("dmc_batch_rollout: this code object takes no rollouts; build the model "
                "with rollout=True (the one-env-per-lane kernel, -DDMC_ROLLOUT=1)");
  if (b->episodes || b->masked)
    return fail("dmc_batch_rollout: rollouts are lock-step; the batch has %s",
                b->episodes ? "per-env episodes enabled" : "an env mask set");
  if (r->nsteps < 0) return fail("dmc_batch_rollout: nsteps must be >= 0");
  if (r->nsub < 0) return fail("dmc_batch_rollout: nsub must be >= 0");
  if (members < 1) return fail("dmc_batch_rollout_population: members must be >= 1, not %d", members);
  if (members > 1 && !(caps & DMC_ROLLOUT_CAP_POPULATION))
    return fail("dmc_batch_rollout_population: this code object takes one policy shared by the "
                "batch; build the model with rollout=True, population=True "
                "(-DDMC_POLICY_POPULATION=1)");
  if (b->nenv % members != 0)
    return fail("dmc_batch_rollout_population: %d members do not divide the %d envs of the batch "
                "(env e acts with member e / (nenv/members))", members, b->nenv);
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
  const int max = chunk_max(*b, true);
  for (int t = 0, chunk; t < r->nsteps; t += chunk) {
    chunk = next_chunk(t, r->nsteps, max);
    if (launch(b, b->stream, b->model->k_step, rollout_args(*b, *b, *r, t, chunk, members),
               MODEL_SHAPED) ||
        steps_issued(b, chunk))
      return -1;
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
  return download(b, field, dst);
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
  const dmc_model_info &d = dst->code.info, &s = src->code.info;
  if (dst->nenv != src->nenv || d.nq != s.nq || d.real_size != s.real_size ||
      d.env_major != s.env_major || d.ntaskdata != s.ntaskdata ||
      d.nmodelparam != s.nmodelparam)
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
  return episode_copy(b, which, dst, nullptr, bytes, "dmc_batch_episode_read");
}

int dmc_batch_episode_write(dmc_batch* b, int which, const int* src, size_t bytes) {
  return episode_copy(b, which, nullptr, src, bytes, "dmc_batch_episode_write");
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
  if (zero_time_refused(b, step_flags, "dmc_batch_episode_prefetch")) return -1;
  dmc_batch::Prefetch& p = b->prefetch;
  p.state = p.PENDING;      // (an earlier one is replaced; the side stream orders the two)
  p.seed = seed;
  p.nsub = settle_nsub;
  p.step_flags = step_flags;
  p.after_steps = after_steps;
  p.issued = 0;
  return steps_issued(b, 0);
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
  for (dmc_field f : DMC_SHADOWED)
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
