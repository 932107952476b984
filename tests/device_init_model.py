"""Host model of the device-side episode initialiser (`dmc_init_episode`),
written from its contract, not from the kernel: every value the
kernel writes for (seed, env) is a pure function of counted draws from a
stateless generator, so it can be computed here exactly and compared value by
value.  Integers are numpy uint64 with wrap-around; floating point is done in
`dtype` -- float64 for the reference that tests compare a device with, float32
and longdouble only to measure what rounding alone can do (`rounding_figure`).

Arrays are [env, k] (the transpose of what `HipBatch.read` returns).
"""

import numpy as np

from dm_control_amd import codegen
from dm_control_amd import model_params
from dm_control_amd.mjcf import model as mdl

FLAG_ONLY_COLLIDING = 8       # csrc/dmc_args.h
FLAG_RESET_ONLY = 16
FLAG_TASKDATA_DEFAULT = 32

_KEY_MUL = np.uint64(0x2545F4914F6CDD1D)
_GOLDEN = np.uint64(0x9e3779b97f4a7c15)
_MIX_A = np.uint64(0xff51afd7ed558ccd)
_MIX_B = np.uint64(0xc4ceb9fe1a85ec53)
_S33, _S16, _S8 = np.uint64(33), np.uint64(16), np.uint64(8)
_LOW32 = np.uint64(0xffffffff)

# Part of the contract: the largest number of candidates for point_mass's
# second direction; the last one is kept whatever its angle.
POINT_MASS_TRIES = 64

# --- tolerances (see `atol`) -------------------------------------------------
# Values that go through log / cos / sin / sqrt or a normalisation are compared
# within  max(8, 4*figure) * eps(real) * scale,  scale = sigma of the normal
# draw, 0.2 for the reacher's target, 1 for unit vectors.  `figure` is what
# rounding alone does to this model's formulas on the CPU: the largest
# difference, over every case that is compared with a device (`compared_cases`
# at 130 envs: the 67 and 1 of tests/test_gpu_device_init.py and the shapes of
# the host-shim runs are its first rows), between the evaluation in `real` and
# one in the next wider type (float32 against float64, float64 against
# longdouble), in eps(real)*scale.  tests/test_device_init_model.py recomputes
# the figures and asserts these values (rounded up here).
# Two classes, so that one term does not set everybody's bound: 'offset' is a
# normal draw added to a mean far above its sigma -- the pole angle
# pi + 0.01 z alone, where half an ulp of pi is about 100 eps * 0.01 -- and
# 'plain' is everything else (its largest term: the rounding of the argument
# 2 pi u of the cosine, times a large sqrt(-2 log u1)).
CPU_ROUNDING_FIGURE = {4: {'plain': 30.1, 'offset': 174.0},
                       8: {'plain': 18.2, 'offset': 101.0}}
# Largest difference seen on the MI355X between a code object and the float64
# model over the same cases, same unit (tests/test_gpu_device_init.py prints it):
# point_mass directions in f32, the cart-pole's normals in f64; the f32 pole
# angle carries the CPU's own term, float(pi) + 0.01 z, and the f64 one none.
GPU_SEEN_FIGURE = {4: {'plain': 7.3, 'offset': 173.1}, 8: {'plain': 1.6, 'offset': 0.0}}
KINDS = ('plain', 'offset')


def bound_in_eps(real_size, kind='plain'):
  return max(8.0, 4.0*CPU_ROUNDING_FIGURE[real_size][kind])


def mix32(x):
  """64-bit finaliser (two xor-shift-multiply rounds and a last xor-shift by
  33), of which bits 16..47 are kept."""
  x = np.asarray(x, np.uint64)
  x = x ^ (x >> _S33)
  x = x*_MIX_A
  x = x ^ (x >> _S33)
  x = x*_MIX_B
  x = x ^ (x >> _S33)
  return (x >> _S16) & _LOW32


class Rng:
  """One stream per env: key = seed*0x2545F4914F6CDD1D + env (mod 2^64); draw
  number c = 1, 2, ... is mix32(key + 0x9e3779b97f4a7c15*c) >> 8, 24 bits."""

  def __init__(self, seed, nenv, dtype=np.float64):
    seed = np.array([int(seed) & (2**64 - 1)], np.uint64)
    self.key = seed*_KEY_MUL + np.arange(nenv, dtype=np.uint64)
    self.ctr = np.zeros(nenv, np.uint64)
    self.dtype = dtype

  def uniform(self, active=None):
    """[0, 1) on a 2^-24 grid; `active` (mask): only those envs draw -- the
    others keep their counter and get a value that must not be used."""
    self.ctr = self.ctr + (np.uint64(1) if active is None else active.astype(np.uint64))
    bits = mix32(self.key + _GOLDEN*self.ctr) >> _S8
    return bits.astype(self.dtype)*self.dtype(2.0**-24)     # exact in every dtype

  def normal(self, active=None):
    """Box-Muller, cosine branch: two uniforms per normal."""
    t = self.dtype
    u1 = np.maximum(self.uniform(active), t(1e-7))
    u2 = self.uniform(active)
    return np.sqrt(t(-2)*np.log(u1))*np.cos(t(2*np.pi)*u2)


class Draw:
  """What one launch writes.  `written` [nenv]: envs the launch touches at all;
  `taskdata` / `modelparam`: None where the launch leaves the field alone.
  `uscale[f]` / `tscale[f]` / `oscale[f]` [k]: see `atol`.  `min_norm`, `min_margin`: how far
  the draw stayed from a decision that rounding could turn (norm of a vector
  before it is normalised; | |d1.d2| - 0.9 | over point_mass candidates)."""

  def __init__(self, model, nenv, dtype, ntaskdata):
    nu = model.nu
    self.qpos = np.tile(np.asarray(model.qpos0, np.float64).astype(dtype), (nenv, 1))
    self.qvel = np.zeros((nenv, model.nv), dtype)
    self.warm = np.zeros((nenv, model.nv), dtype)
    self.ctrl = np.zeros((nenv, nu), dtype)
    self.time = np.zeros(nenv, dtype)
    self.episode_return = np.zeros(nenv, dtype)
    self.taskdata = None
    self.modelparam = None
    self.written = np.ones(nenv, bool)
    self.uscale = {'qpos': np.zeros(model.nq), 'qvel': np.zeros(model.nv),
                   'taskdata': np.zeros(ntaskdata)}
    self.tscale = {k: v.copy() for k, v in self.uscale.items()}
    self.oscale = {k: v.copy() for k, v in self.uscale.items()}
    self.min_norm = np.inf
    self.min_margin = np.inf
    self.randomised = []          # qpos columns that carry a draw


def atol(d, field, real_size):
  """[k] absolute tolerance of `field` of draw `d` for a device whose `real` has
  `real_size` bytes, against the float64 model:
    exact (zeros, qpos0, defaults): 0 -- the caller rounds the model to `real`;
    lo + (hi - lo)*u with u exact: 4 eps max(|lo|, |hi|)  (rounding of the two
      constants, of the product and of the sum: at most 8 half-ulps of the
      larger bound);
    through log / cos / sin / sqrt / a normalisation: bound_in_eps * eps * scale,
      the scale in `tscale` ('plain') or `oscale` ('offset')."""
  eps = float(np.finfo(np.float32 if real_size == 4 else np.float64).eps)
  zero = np.zeros(getattr(d, field).shape[-1] if getattr(d, field).ndim > 1 else 1)
  u = d.uscale.get(field, zero)
  t = d.tscale.get(field, zero)
  o = d.oscale.get(field, zero)
  return 4*eps*u + bound_in_eps(real_size)*eps*t + bound_in_eps(real_size, 'offset')*eps*o


def _between(d, rng, column, lo, hi):
  t = rng.dtype
  d.qpos[:, column] = t(lo) + (t(hi) - t(lo))*rng.uniform()
  d.uscale['qpos'][column] = max(abs(lo), abs(hi))
  d.randomised.append(column)


def _gaussian(d, rng, field, column, mean, sigma):
  t = rng.dtype
  z = t(sigma)*rng.normal()
  getattr(d, field)[:, column] = z if mean == 0 else t(mean) + z
  (d.tscale if abs(mean) <= sigma else d.oscale)[field][column] = sigma
  if field == 'qpos':
    d.randomised.append(column)


def cartpole(d, rng, model, swing_up):
  """cartpole.py:186-194.  Swing-up: cart N(0, 0.01), first pole N(pi, 0.01),
  further poles (`qpos[2:]`) N(0, 0.1); balance: cart U(-0.1, 0.1), every pole
  U(-0.034, 0.034).  Then every velocity N(0, 0.01).  Positions first, in
  index order."""
  if swing_up:
    _gaussian(d, rng, 'qpos', 0, 0.0, 0.01)
    _gaussian(d, rng, 'qpos', 1, np.pi, 0.01)
    for i in range(2, model.nq):
      _gaussian(d, rng, 'qpos', i, 0.0, 0.1)
  else:
    # the reference's uniform(lo, hi) is lo + (hi - lo)*u; the width is the
    # literal 0.2 (0.068), not the difference of the rounded bounds
    t = rng.dtype
    d.qpos[:, 0] = t(-0.1) + t(0.2)*rng.uniform()
    d.uscale['qpos'][0] = 0.1
    for i in range(1, model.nq):
      d.qpos[:, i] = t(-0.034) + t(0.068)*rng.uniform()
      d.uscale['qpos'][i] = 0.034
    d.randomised += list(range(model.nq))
  for i in range(model.nv):
    _gaussian(d, rng, 'qvel', i, 0.0, 0.01)


def joint_walk(d, rng, model, limited_only):
  """randomizers.py:61-86, joints in model order: a limited hinge or slider is
  uniform on its range; an unlimited hinge uniform on [-pi, pi]; a free joint
  gets rand(4) normalised as its quaternion and keeps its translation; an
  unlimited slider keeps qpos0.  `limited_only` (cheetah.py:67-69): the limited
  joints alone."""
  t = rng.dtype
  for j in range(model.njnt):
    kind, adr = int(model.jnt_type[j]), int(model.jnt_qposadr[j])
    if model.jnt_limited[j]:
      if kind in (mdl.JNT_HINGE, mdl.JNT_SLIDE):
        lo, hi = (float(x) for x in model.jnt_range[j])
        _between(d, rng, adr, lo, hi)
    elif limited_only:
      continue
    elif kind == mdl.JNT_HINGE:
      d.qpos[:, adr] = t(-np.pi) + t(2*np.pi)*rng.uniform()
      d.uscale['qpos'][adr] = np.pi
      d.randomised.append(adr)
    elif kind == mdl.JNT_FREE:
      q = np.stack([rng.uniform() for _ in range(4)], axis=1)
      norm = np.sqrt((q*q).sum(axis=1, dtype=t))
      d.min_norm = min(d.min_norm, float(norm.min()))
      d.qpos[:, adr + 3:adr + 7] = q/norm[:, None]
      d.tscale['qpos'][adr + 3:adr + 7] = 1.0
      d.randomised += list(range(adr + 3, adr + 7))


def reacher_target(d, rng):
  """reacher.py:95-98, after the joints: angle U(0, 2 pi), then radius
  U(0.05, 0.2); the target is (radius sin(angle), radius cos(angle))."""
  t = rng.dtype
  angle = t(2*np.pi)*rng.uniform()
  radius = t(0.05) + t(0.15)*rng.uniform()
  d.taskdata[:, 0] = radius*np.sin(angle)
  d.taskdata[:, 1] = radius*np.cos(angle)
  d.tscale['taskdata'][:] = 0.2
  return angle, radius


def _unit2(d, rng, active):
  x, y = rng.normal(active), rng.normal(active)
  norm = np.sqrt(x*x + y*y)
  d.min_norm = min(d.min_norm, float(norm[active].min()))
  with np.errstate(invalid='ignore', divide='ignore'):
    return x/norm, y/norm


def point_mass_directions(d, rng, hard):
  """point_mass.py:97-107, after the joints.  Easy: the model's own tendon
  coefficients.  Hard: d1 = randn(2) normalised; d2 likewise, drawn again while
  |d1.d2| > 0.9, POINT_MASS_TRIES candidates at the most."""
  if not hard:
    return
  every = np.ones(len(d.qpos), bool)
  d1x, d1y = _unit2(d, rng, every)
  d2x, d2y = d1x.copy(), d1y.copy()
  searching = every.copy()
  for _ in range(POINT_MASS_TRIES):
    cx, cy = _unit2(d, rng, searching)
    d2x[searching], d2y[searching] = cx[searching], cy[searching]
    dot = np.abs(d1x*d2x + d1y*d2y)
    d.min_margin = min(d.min_margin, float(np.abs(dot[searching].astype(np.float64) - 0.9).min()))
    searching = searching & (dot > rng.dtype(0.9))
    if not searching.any():
      break
  d.taskdata[:] = np.stack([d1x, d1y, d2x, d2y], axis=1)
  d.tscale['taskdata'][:] = 1.0


def draw(model, task_id, task_param_i, seed, nenv, flags=0, stats_ncon=None,
         per_env=(), dtype=np.float64):
  """The fields after one launch of the initialiser on a batch of `nenv` envs.
  flags: FLAG_* bits; stats_ncon [nenv]: the contact counts ONLY_COLLIDING
  reads.  A launch always writes qpos, qvel, warm start, control, time and
  return of the envs it touches; the draw of an env depends on (seed, env)
  alone, so an env skipped by ONLY_COLLIDING is simply not written."""
  ntd = codegen.task_data_size(task_id)
  d = Draw(model, nenv, dtype, ntd)
  rng = Rng(seed, nenv, dtype)
  if flags & FLAG_ONLY_COLLIDING:
    d.written = np.asarray(stats_ncon) != 0
  defaults = np.asarray(codegen.task_data_default(model, task_id), np.float64).astype(dtype)
  if flags & FLAG_TASKDATA_DEFAULT:
    d.taskdata = np.tile(defaults, (nenv, 1)).reshape(nenv, ntd)
    if per_env:
      d.modelparam = model_params.ModelParams(model, per_env, nenv).block().T.astype(dtype)
  if flags & FLAG_RESET_ONLY:
    return d
  if task_id == codegen.TASK_CARTPOLE:
    cartpole(d, rng, model, bool(task_param_i & 2))
  elif task_id != codegen.TASK_NONE:
    joint_walk(d, rng, model, limited_only=task_id == codegen.TASK_CHEETAH)
  if task_id == codegen.TASK_POINTMASS:
    d.taskdata = np.tile(defaults, (nenv, 1))
    point_mass_directions(d, rng, bool(task_param_i & 1))
  elif task_id == codegen.TASK_REACHER:
    d.taskdata = np.zeros((nenv, 2), dtype)
    reacher_target(d, rng)
  d.draws = rng.ctr
  return d


# --- the cases every comparison with a device runs ---------------------------
# (label, domain, number of poles or None, task_param_i): one line per branch of
# the recipes
CASES = (
    ('cartpole_swingup', 'cartpole', 1, 2), ('cartpole_balance', 'cartpole', 1, 0),
    ('cartpole_three_poles', 'cartpole', 3, 2), ('cheetah_run', 'cheetah', None, 0),
    ('walker_walk', 'walker', None, 0), ('hopper_hop', 'hopper', None, 1),
    ('pendulum_swingup', 'pendulum', None, 0), ('acrobot_swingup', 'acrobot', None, 0),
    ('reacher_hard', 'reacher', None, 0), ('point_mass_hard', 'point_mass', None, 1),
    ('point_mass_easy', 'point_mass', None, 0), ('humanoid_stand', 'humanoid', None, 0))
# a small seed, and one of the product's form (base << 20) + episode with base
# near 2^31: seed*0x2545F4914F6CDD1D then needs all 64 bits of the key
SEEDS = (11, (2147483000 << 20) + 5)
SEED_ONLY_COLLIDING = (1234567 << 20) + 2
PUBLIC_RANDOM = 3          # `random` of the environments of the public-path tests
NENV = 67


def product_seeds(random, count):
  """The seeds `Task.device_seed()` hands to the device, replayed: episode k
  (1, 2, ...) gets (RandomState(random).randint(0, 2**31 - 1) << 20) + k."""
  rs = np.random.RandomState(random)
  return [(int(rs.randint(0, 2**31 - 1)) << 20) + k for k in range(1, count + 1)]


def case_model(domain, poles):
  from dm_control_amd.mjcf import compiler
  from dm_control_amd.suite import cartpole, common
  if poles and poles > 1:
    return compiler.from_xml_string(*cartpole.get_model_and_assets(poles))
  return compiler.from_xml_string(common.read_model(domain + '.xml'))


def compared_cases(nenv=NENV):
  """(model, task, task_param_i, seed, nenv) of every comparison with a device:
  CASES under SEEDS, the redraw seed and the seeds of the public-path tests."""
  task_of = {'cartpole': codegen.TASK_CARTPOLE, 'cheetah': codegen.TASK_CHEETAH,
             'humanoid': codegen.TASK_HUMANOID, 'walker': codegen.TASK_WALKER,
             'pendulum': codegen.TASK_PENDULUM, 'acrobot': codegen.TASK_ACROBOT,
             'hopper': codegen.TASK_HOPPER, 'reacher': codegen.TASK_REACHER,
             'point_mass': codegen.TASK_POINTMASS}
  seeds = SEEDS + (SEED_ONLY_COLLIDING,) + tuple(product_seeds(PUBLIC_RANDOM, 8))
  out = []
  for _, domain, poles, param in CASES:
    model = case_model(domain, poles)
    out += [(model, task_of[domain], param, seed, nenv) for seed in seeds]
  return out


def scales(d, kind):
  return d.tscale if kind == 'plain' else d.oscale


def rounding_figure(cases, real, kind='plain'):
  """Largest |draw in `real` - draw in the next wider type| over `cases`
  ((model, task, task_param_i, seed, nenv) tuples), in eps(real)*scale, over the
  values of class `kind` (`CPU_ROUNDING_FIGURE`)."""
  wide = np.float64 if real == np.float32 else np.longdouble
  eps = float(np.finfo(real).eps)
  worst = 0.0
  for model, task, param, seed, nenv in cases:
    a = draw(model, task, param, seed, nenv, dtype=real)
    b = draw(model, task, param, seed, nenv, dtype=wide)
    for field in ('qpos', 'qvel', 'taskdata'):
      scale = scales(a, kind)[field]
      if getattr(a, field) is None or not scale.any():
        continue
      diff = np.abs(getattr(a, field).astype(wide) - getattr(b, field))[:, scale > 0]
      worst = max(worst, float((diff/(eps*scale[scale > 0])).max()))
  return worst
