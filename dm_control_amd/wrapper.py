"""ctypes shim over libdmc_hip.so (include/dmc_hip.h).

Counterpart of the reference's wrapper layer:
  library discovery  /root/reference/dm_control/mujoco/wrapper/util.py:39-67,107-120
                     (`$MJLIB_PATH` -> here `$DMC_HIP_LIB`, else the in-tree build)
  error convention   wrapper/core.py:85-101,312-328 (`wrapper.Error`)
  MjModel / MjData   wrapper/core.py:444-776

There is no CPU fallback: if the library cannot be loaded, or no MI355X-class
device is present, construction raises `Error`.
"""

import contextlib
import ctypes
import os
import sys

import numpy as np

ENV_DMC_HIP_LIB = 'DMC_HIP_LIB'
_DEFAULT_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                            'csrc', 'libdmc_hip.so')

# enum dmc_field, in the header's order: (name, the ModelInfo member that counts
# the rows or None, rows per count, an empty count still has one row, element
# kind, agent layout [nenv][k]).  FIELD_<name> is the row's index.
FIELDS = (
    ('QPOS', 'nq', 1, True, 'real', False),
    ('QVEL', 'nv', 1, True, 'real', False),
    ('WARMSTART', 'nv', 1, True, 'real', False),
    ('TIME', None, 1, False, 'real', False),
    ('CTRL', 'nu', 1, True, 'real', False),
    ('OBS', 'nobs', 1, True, 'real', True),
    ('REWARD', None, 1, False, 'real', False),
    ('SENSORDATA', 'nsensordata', 1, True, 'real', False),
    ('XPOS', 'nbody', 3, False, 'real', False),
    ('XMAT', 'nbody', 9, False, 'real', False),
    ('QACC', 'nv', 1, True, 'real', False),
    ('WARN', None, 1, False, 'uint32', False),
    ('STATS', None, 3, False, 'int32', False),
    ('RETURN', None, 1, False, 'real', False),
    ('TASKDATA', 'ntaskdata', 1, True, 'real', False),
    ('MODELPARAM', 'nmodelparam', 1, True, 'real', False),
)
globals().update(('FIELD_' + f[0], k) for k, f in enumerate(FIELDS))

# bits of `want_outputs` (DMC_STEP_* of the header)
STEP_OUTPUTS, STEP_STALE_FIRST = 1, 2
STEP_ZERO_TIME = 4   # enum dmc_step_bit
# enum dmc_episode_array: the int32 [nenv] arrays of the episode block
EPISODE_STEP, EPISODE_DONE, EPISODE_MASK = 0, 1, 2
# enum dmc_done_bit
DONE_LIMIT, DONE_BAD_STATE = 1, 2


class Error(Exception):
  """Base class for errors raised by the HIP runtime (cf. wrapper.Error)."""


class ModelInfo(ctypes.Structure):
  _fields_ = [(n, ctypes.c_int) for n in (
      'abi', 'real_size', 'nq', 'nv', 'nu', 'nbody', 'nobs', 'nsensordata',
      'ws_per_env', 'task', 'ncon_max', 'nefc_max', 'integrator', 'npair',
      'ntaskdata', 'envs_per_block', 'lanes_per_env', 'env_major',
      'nmodelparam', 'seq_launch')]


_vp, _ci, _cll, _cs = (ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong,
                       ctypes.c_size_t)

# enum dmc_rollout_cap
ROLLOUT_OUTPUTS, ROLLOUT_POLICY, ROLLOUT_POPULATION, ROLLOUT_WIDTH_SHIFT = 1, 2, 4, 8


class Rollout(ctypes.Structure):
  """struct dmc_rollout."""
  _fields_ = [('nsteps', _ci), ('nsub', _ci), ('ctrl', _vp),
              ('ctrl_stride_k', _cll), ('ctrl_stride_env', _cll), ('ctrl_stride_t', _cll),
              ('policy', _vp), ('nlayers', _ci), ('width', _ci*3),
              ('reward_out', _vp), ('reward_stride_t', _cll),
              ('obs_out', _vp), ('obs_stride_t', _cll),
              ('action_out', _vp), ('action_stride_t', _cll)]


# every symbol declared in include/dmc_hip.h: (restype, argtypes)
SIGNATURES = {
    'dmc_version': (_ci, []),
    'dmc_last_error': (ctypes.c_char_p, []),
    'dmc_device_count': (_ci, []),
    'dmc_model_load': (_ci, [ctypes.c_char_p, _ci, ctypes.POINTER(_vp)]),
    'dmc_model_compile': (_ci, [
        ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p),
        ctypes.POINTER(ctypes.c_char_p), _ci, ctypes.POINTER(ctypes.c_char_p), _ci,
        ctypes.POINTER(_vp), ctypes.POINTER(_cs), ctypes.c_char_p, _cs]),
    'dmc_code_free': (None, [_vp]),
    'dmc_model_load_data': (_ci, [_vp, _cs, _ci, ctypes.POINTER(_vp)]),
    'dmc_model_get_info': (_ci, [_vp, ctypes.POINTER(ModelInfo)]),
    'dmc_model_free': (None, [_vp]),
    'dmc_batch_create': (_ci, [_vp, _ci, ctypes.POINTER(_vp)]),
    'dmc_batch_free': (None, [_vp]),
    'dmc_batch_nenv': (_ci, [_vp]),
    'dmc_batch_set_aux_outputs': (_ci, [_vp, _ci]),
    'dmc_batch_set_task_params': (
        _ci, [_vp, _ci, ctypes.POINTER(ctypes.c_double), _ci]),
    'dmc_batch_reset': (_ci, [_vp]),
    'dmc_batch_set_state': (_ci, [_vp, _vp, _vp, _vp, _vp]),
    'dmc_batch_write': (_ci, [_vp, _ci, _vp, _cs]),
    'dmc_batch_init_episode': (_ci, [_vp, ctypes.c_uint64, _ci]),
    'dmc_batch_forward': (_ci, [_vp, _ci]),
    'dmc_batch_step': (_ci, [_vp, _vp, _cll, _cll, _ci, _ci, _ci]),
    'dmc_batch_step_n': (_ci, [_vp, _vp, _cll, _cll, _cll, _ci, _ci, _ci]),
    'dmc_model_rollout_caps': (_ci, [_vp]),
    'dmc_batch_rollout': (_ci, [_vp, ctypes.POINTER(Rollout)]),
    'dmc_batch_rollout_population': (_ci, [_vp, ctypes.POINTER(Rollout), _ci]),
    'dmc_batch_read': (_ci, [_vp, _ci, _vp, _cs]),
    'dmc_batch_field_bytes': (_cs, [_vp, _ci]),
    'dmc_batch_device_ptr': (_vp, [_vp, _ci]),
    'dmc_batch_clear_warnings': (_ci, [_vp]),
    'dmc_batch_copy_state': (_ci, [_vp, _vp]),
    'dmc_batch_episodes_enable': (_ci, [_vp, _ci]),
    'dmc_batch_episode_ptr': (_vp, [_vp, _ci]),
    'dmc_batch_episode_read': (_ci, [_vp, _ci, _vp, _cs]),
    'dmc_batch_episode_write': (_ci, [_vp, _ci, _vp, _cs]),
    'dmc_batch_mask_from_done': (_ci, [_vp]),
    'dmc_batch_set_masked': (_ci, [_vp, _ci]),
    'dmc_batch_episode_prefetch': (_ci, [_vp, ctypes.c_uint64, _ci, _ci, _cll]),
    'dmc_batch_episode_take': (_ci, [_vp, ctypes.c_uint64, _ci, _ci]),
    'dmc_batch_sync': (_ci, [_vp]),
    'dmc_batch_stream': (_vp, [_vp]),
    'dmc_batch_set_stream': (_ci, [_vp, _vp, _ci]),
    'dmc_batch_timer_start': (_ci, [_vp]),
    'dmc_batch_timer_stop': (_ci, [_vp, ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(_cll)]),
}

_lib = None


def get_lib_path():
  return os.environ.get(ENV_DMC_HIP_LIB) or _DEFAULT_LIB


def get_lib():
  """Loads libdmc_hip.so (cf. `util.get_mjlib`, wrapper/util.py:107-120)."""
  global _lib
  if _lib is not None:
    return _lib
  # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as the
  # system one libdmc_hip.so links to).  Whichever is mapped first serves the
  # whole process, and torch fails to find devices when the system runtime got
  # there first, so let torch map its copy before ours when it is installed.
  if 'torch' not in sys.modules and not os.environ.get('DMC_NO_TORCH_PRELOAD'):
    try:
      import torch  # noqa: F401  pylint: disable=unused-import,g-import-not-at-top
    except ImportError:
      pass
  path = get_lib_path()
  if not os.path.exists(path):
    raise Error('HIP extension not found at {!r}; run '
                '`python -c "import __graft_entry__ as g; g.build()"` '
                '(there is no CPU fallback)'.format(path))
  try:
    lib = ctypes.cdll.LoadLibrary(path)
  except OSError as e:
    raise Error('cannot load {!r}: {}'.format(path, e))
  for name, (res, args) in SIGNATURES.items():
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = res, args
  _lib = lib
  return lib


def _check(rc):
  if rc != 0:
    raise Error(get_lib().dmc_last_error().decode('utf-8', 'replace'))


def compile_code_object(source, source_name, headers, options):
  """gfx950 code object (bytes) of `source` built in-process by
  `dmc_model_compile` -- HIP runtime compilation, no hipcc executable.

  headers: {include name: text}; options: compiler flags.  Needs no GPU."""
  lib = get_lib()
  names = list(headers)
  arr = ctypes.c_char_p*max(1, len(names))
  hn = arr(*[n.encode() for n in names])
  ht = arr(*[headers[n].encode() for n in names])
  opts = (ctypes.c_char_p*max(1, len(options)))(*[o.encode() for o in options])
  code, size = _vp(), _cs()
  log = ctypes.create_string_buffer(1 << 16)
  rc = lib.dmc_model_compile(source.encode(), source_name.encode(), hn, ht, len(names),
                             opts, len(options), ctypes.byref(code),
                             ctypes.byref(size), log, len(log))
  if rc != 0:
    raise Error('%s\n%s' % (lib.dmc_last_error().decode('utf-8', 'replace'),
                            log.value.decode('utf-8', 'replace')[-4000:]))
  try:
    return ctypes.string_at(code.value, size.value), log.value.decode('utf-8', 'replace')
  finally:
    lib.dmc_code_free(code)


class HipModel:
  """Loaded code object of one compiled model (cf. `MjModel`)."""

  def __init__(self, code_object_path, device_id=0, code=None):
    self._lib = get_lib()
    self.ptr = _vp()
    if code is not None:
      self._code = bytes(code)     # (the module keeps no reference to the image)
      _check(self._lib.dmc_model_load_data(self._code, len(self._code), device_id,
                                           ctypes.byref(self.ptr)))
    else:
      _check(self._lib.dmc_model_load(code_object_path.encode(), device_id,
                                      ctypes.byref(self.ptr)))
    self.info = ModelInfo()
    _check(self._lib.dmc_model_get_info(self.ptr, ctypes.byref(self.info)))
    self.device_id = device_id
    self.dtype = np.float32 if self.info.real_size == 4 else np.float64

  @property
  def rollout_caps(self):
    """ROLLOUT_* bits and, above ROLLOUT_WIDTH_SHIFT, the widest hidden layer of
    a device policy; 0: not a rollout build (`build_model(..., rollout=True)`)."""
    return self._lib.dmc_model_rollout_caps(self.ptr)

  @classmethod
  def from_code(cls, code, device_id=0):
    """Loads a code object held in memory (`build.code_object_bytes`,
    `dmc_model_compile`) -- no file involved."""
    return cls(None, device_id, code=code)

  def free(self):
    if self.ptr:
      self._lib.dmc_model_free(self.ptr)
      self.ptr = _vp()

  def __del__(self):
    try:
      self.free()
    except Exception:  # pylint: disable=broad-except
      pass


class HipBatch:
  """HBM-resident state of `nenv` instances (cf. `MjData`)."""

  def __init__(self, model, nenv):
    self._lib = get_lib()
    self.model = model  # keeps the module alive (core.py:643)
    self.nenv = int(nenv)
    self.ptr = _vp()
    self.is_masked = False      # inside `masked()`
    self.episodes = False       # after `episodes_enable`
    self.step_limit = 0
    self.control_steps = 0      # output-producing steps issued so far (settle steps: not counted)
    _check(self._lib.dmc_batch_create(model.ptr, self.nenv,
                                      ctypes.byref(self.ptr)))

  # -- shapes ---------------------------------------------------------------
  def _shape(self, field):
    _, count, mult, pad, _, agent = FIELDS[field]
    if count is None and mult == 1:
      return (self.nenv,)
    rows = mult
    if count is not None:
      rows *= max(getattr(self.model.info, count), int(pad))
    return (self.nenv, rows) if agent else (rows, self.nenv)

  def _dtype(self, field):
    kind = FIELDS[field][4]
    return self.model.dtype if kind == 'real' else np.dtype(kind).type

  def read(self, field):
    """Device -> host copy of a whole field, native [k][env] layout."""
    out = np.empty(self._shape(field), self._dtype(field))
    _check(self._lib.dmc_batch_read(self.ptr, field, out.ctypes.data,
                                    out.nbytes))
    return out

  def device_ptr(self, field):
    return self._lib.dmc_batch_device_ptr(self.ptr, field)

  # -- state ------------------------------------------------------------------
  def reset(self):
    _check(self._lib.dmc_batch_reset(self.ptr))

  def write(self, field, array):
    """Uploads a writable field given as [k][nenv] (any float dtype)."""
    a = np.ascontiguousarray(array, dtype=self._dtype(field))
    if a.shape != self._shape(field):
      raise ValueError('expected shape {}, got {}'.format(
          self._shape(field), a.shape))
    _check(self._lib.dmc_batch_write(self.ptr, field, a.ctypes.data, a.nbytes))

  def set_state(self, qpos=None, qvel=None, warmstart=None, time=None):
    """Uploads [k][nenv] arrays (any float dtype; converted to the batch's)."""
    keep = []

    def prep(a, field):
      if a is None:
        return None
      a = np.ascontiguousarray(a, dtype=self.model.dtype)
      if a.shape != self._shape(field):
        raise ValueError('expected shape {}, got {}'.format(
            self._shape(field), a.shape))
      keep.append(a)
      return a.ctypes.data
    _check(self._lib.dmc_batch_set_state(
        self.ptr, prep(qpos, FIELD_QPOS), prep(qvel, FIELD_QVEL),
        prep(warmstart, FIELD_WARMSTART), prep(time, FIELD_TIME)))

  def set_aux_outputs(self, enabled):
    _check(self._lib.dmc_batch_set_aux_outputs(self.ptr, int(bool(enabled))))

  def set_task_params(self, iparam=0, rparams=()):
    arr = (ctypes.c_double*4)(*(list(rparams) + [0.0]*4)[:4])
    _check(self._lib.dmc_batch_set_task_params(self.ptr, int(iparam), arr,
                                               len(rparams)))

  def init_episode(self, seed, only_colliding=False):
    _check(self._lib.dmc_batch_init_episode(self.ptr, int(seed) & (2**64 - 1),
                                            int(only_colliding)))

  def forward(self, count_contacts=False):
    _check(self._lib.dmc_batch_forward(self.ptr, int(count_contacts)))

  def step_host(self, ctrl, nsub=1, want_outputs=True, stale_first=False,
                zero_time=False):
    """ctrl: host array [nenv, nu] (agent layout) or None.

    stale_first: DMC_STEP_STALE_FIRST (the first substep takes its acceleration
    from the reset state; the reference cheetah's first settle step).
    zero_time: DMC_STEP_ZERO_TIME (the stepped envs end with time 0)."""
    want_outputs = ((STEP_OUTPUTS if want_outputs else 0) |
                    (STEP_STALE_FIRST if stale_first else 0) |
                    (STEP_ZERO_TIME if zero_time else 0))
    self.control_steps += want_outputs & STEP_OUTPUTS
    if ctrl is None:
      _check(self._lib.dmc_batch_step(self.ptr, None, 0, 0, 0, nsub,
                                      want_outputs))
      return
    c = np.ascontiguousarray(ctrl, dtype=self.model.dtype)
    nu = self.model.info.nu
    if c.shape != (self.nenv, nu):
      raise ValueError('ctrl must have shape ({}, {}), got {}'.format(
          self.nenv, nu, c.shape))
    _check(self._lib.dmc_batch_step(self.ptr, c.ctypes.data, 1, nu, 0, nsub,
                                    int(want_outputs)))

  def step_device(self, ctrl_ptr, stride_k, stride_env, nsub=1,
                  want_outputs=True):
    """ctrl_ptr: device address; element (k, env) at k*stride_k+env*stride_env."""
    _check(self._lib.dmc_batch_step(self.ptr, ctrl_ptr, stride_k, stride_env,
                                    1, nsub, int(want_outputs)))
    self.control_steps += int(want_outputs) & STEP_OUTPUTS

  def step_device_n(self, ctrl_ptr, stride_k, stride_env, stride_t, nsteps,
                    nsub=1, want_outputs=True):
    """`nsteps` control steps; step t reads ctrl_ptr + t*stride_t reals."""
    _check(self._lib.dmc_batch_step_n(self.ptr, ctrl_ptr, stride_k, stride_env,
                                      stride_t, nsteps, nsub, int(want_outputs)))
    self.control_steps += int(nsteps)*(int(want_outputs) & STEP_OUTPUTS)

  def rollout(self, nsteps, nsub=1, ctrl=None, policy=None, reward_out=None,
              obs_out=None, action_out=None):
    """`dmc_batch_rollout` over device memory of the batch's real type.

    ctrl: None or (ptr, stride_k, stride_env, stride_t), in reals; policy: None
    or (ptr, widths) with widths = hidden widths then the output width (nu), the
    weights packed as `rl.policy.MLPPolicy.packed` lays them out, or (ptr, widths,
    members): `dmc_batch_rollout_population` over [nparams][members] weights as
    `rl.policy.MLPPopulation.packed` lays them out, env e acting with member
    e // (nenv // members); *_out: None or (ptr, stride_t): [nsteps][nenv],
    [nsteps][nenv][nobs], [nsteps][nenv][nu]."""
    r = Rollout()
    r.nsteps, r.nsub = int(nsteps), int(nsub)
    if ctrl is not None:
      r.ctrl, r.ctrl_stride_k, r.ctrl_stride_env, r.ctrl_stride_t = ctrl
    members = None
    if policy is not None:
      ptr, widths = policy[:2]
      if len(policy) > 2:
        members = int(policy[2])
      widths = [int(w) for w in widths]
      r.policy, r.nlayers = ptr, len(widths) - 1
      for l, w in enumerate(widths[:3]):
        r.width[l] = w
    for name, out in (('reward', reward_out), ('obs', obs_out), ('action', action_out)):
      if out is not None:
        setattr(r, name + '_out', out[0])
        setattr(r, name + '_stride_t', out[1])
    if members is None:
      _check(self._lib.dmc_batch_rollout(self.ptr, ctypes.byref(r)))
    else:
      _check(self._lib.dmc_batch_rollout_population(self.ptr, ctypes.byref(r), members))
    self.control_steps += r.nsteps

  # -- per-env episodes --------------------------------------------------------
  def episodes_enable(self, step_limit=0):
    """Allocates the episode block (step counts, done bits, env mask; zeroed).
    From now on output-producing steps count and freeze per env, see
    include/dmc_hip.h.  step_limit <= 0: no time limit."""
    _check(self._lib.dmc_batch_episodes_enable(self.ptr, int(step_limit)))
    self.episodes, self.step_limit = True, int(step_limit)

  def episode_ptr(self, which):
    return self._lib.dmc_batch_episode_ptr(self.ptr, which)

  def episode_read(self, which):
    out = np.empty(self.nenv, np.int32)
    _check(self._lib.dmc_batch_episode_read(self.ptr, which, out.ctypes.data, out.nbytes))
    return out

  def episode_write(self, which, array):
    a = np.ascontiguousarray(array, dtype=np.int32)
    if a.shape != (self.nenv,):
      raise ValueError('expected shape ({},), got {}'.format(self.nenv, a.shape))
    _check(self._lib.dmc_batch_episode_write(self.ptr, which, a.ctypes.data, a.nbytes))

  def mask_from_done(self):
    """mask <- done, on the batch's stream (no host synchronisation)."""
    _check(self._lib.dmc_batch_mask_from_done(self.ptr))

  def set_masked(self, on):
    _check(self._lib.dmc_batch_set_masked(self.ptr, int(bool(on))))
    self.is_masked = bool(on)

  @contextlib.contextmanager
  def masked(self, mask=None):
    """Inside, init_episode / forward / step leave envs with mask[e] == 0 alone.
    mask: int or bool [nenv] to upload first (a host write, it synchronises);
    None: the mask the device holds (`mask_from_done`, an earlier upload)."""
    if mask is not None:
      self.set_masked(True)      # (allocates the block on first use)
      self.episode_write(EPISODE_MASK, np.asarray(mask) != 0)
    self.set_masked(True)
    try:
      yield self
    finally:
      self.set_masked(False)

  # -- episode prefetch ----------------------------------------------------------
  @staticmethod
  def _settle_flags(stale_first, zero_time):
    return ((STEP_STALE_FIRST if stale_first else 0) |
            (STEP_ZERO_TIME if zero_time else 0))

  def episode_prefetch(self, seed, settle_nsub, stale_first=False, zero_time=False,
                       after_steps=0):
    """Asks for the start of the next whole-batch episode -- reset,
    `init_episode(seed)`, `settle_nsub` settle substeps -- to be computed on a side
    stream into shadow buffers once `after_steps` more control steps have been
    issued (`dmc_batch_episode_prefetch`).  Raises `Error` on a masked batch or
    one with per-env episodes."""
    _check(self._lib.dmc_batch_episode_prefetch(
        self.ptr, int(seed) & (2**64 - 1), int(settle_nsub),
        self._settle_flags(stale_first, zero_time), int(after_steps)))

  def episode_take(self, seed, settle_nsub, stale_first=False, zero_time=False):
    """True: the fields now hold (on the batch's stream, no host wait) what
    `reset()`, `init_episode(seed)` and the settle step would have left, from a
    prefetch with exactly these arguments.  False: there was none to use; run them."""
    rc = self._lib.dmc_batch_episode_take(
        self.ptr, int(seed) & (2**64 - 1), int(settle_nsub),
        self._settle_flags(stale_first, zero_time))
    if rc < 0:
      _check(rc)
    return rc == 1

  def clear_warnings(self):
    _check(self._lib.dmc_batch_clear_warnings(self.ptr))

  def copy_state_from(self, other):
    _check(self._lib.dmc_batch_copy_state(self.ptr, other.ptr))
    self.episodes, self.step_limit = other.episodes, other.step_limit

  def stream(self):
    return self._lib.dmc_batch_stream(self.ptr)

  def set_stream(self, stream_ptr, external=True):
    """Runs later launches on a caller-owned hipStream_t.

    `stream_ptr` 0/None with external=True is HIP's default (null) stream;
    external=False restores the batch's own stream.
    """
    _check(self._lib.dmc_batch_set_stream(self.ptr, stream_ptr or None,
                                          int(external)))

  def sync(self):
    _check(self._lib.dmc_batch_sync(self.ptr))

  def timer_start(self):
    _check(self._lib.dmc_batch_timer_start(self.ptr))

  def timer_stop(self):
    ms, n = ctypes.c_double(), _cll()
    _check(self._lib.dmc_batch_timer_stop(self.ptr, ctypes.byref(ms),
                                          ctypes.byref(n)))
    return ms.value, n.value

  def free(self):
    if self.ptr:
      self._lib.dmc_batch_free(self.ptr)
      self.ptr = _vp()

  def __del__(self):
    try:
      self.free()
    except Exception:  # pylint: disable=broad-except
      pass
