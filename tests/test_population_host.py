"""Populations of policies without a GPU: the build spec, the argument block
(tests/host_runtime/population_plan.cpp), `rl.policy.MLPPopulation`, the tier and the
capability word of the population builds, and the population variant of the step
kernel run on the host under ASan + UBSan (tests/host_shim/population_harness.cpp, a
stand-alone program run directly).  The MI355X counterpart is
tests/test_gpu_population.py.
"""

import os
import struct
import subprocess

import numpy as np
import pytest

import helpers
import population_cases
import rollout_cases
import shim_runner
from dm_control_amd import build
from dm_control_amd import codegen
from dm_control_amd.rl import policy as policy_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- build.spec --------------------------------------------------------------------

def _spec(model, task, precision='f32', mode='auto', **kw):
  return build.spec(model, task, precision, None, (), mode, None, 64, **kw)


def test_spec_population_adds_one_flag_after_rollout_and_changes_the_key():
  model = helpers.load_model('cheetah')
  task = helpers.TASKS['cheetah']
  with pytest.raises(ValueError, match='rollout=True'):
    _spec(model, task, population=True)
  with pytest.raises(ValueError, match='rollout=True'):
    build.build_model(model, task, population=True)
  roll = _spec(model, task, rollout=True)
  pop = _spec(model, task, rollout=True, population=True)
  assert pop.flags == ('-DDMC_ROLLOUT=1', '-DDMC_POLICY_POPULATION=1')
  assert pop.tiers == roll.tiers and pop.source == roll.source == 'dmc_kernels.hip'
  # pylint: disable=protected-access
  keys = lambda s: [build._key(s, t) for t in s.tiers]
  assert not set(keys(pop)) & set(keys(roll))
  assert not set(keys(pop)) & set(keys(_spec(model, task)))
  # population=False: the specs and keys of today
  assert _spec(model, task, population=False) == _spec(model, task)
  assert _spec(model, task, rollout=True, population=False) == roll
  assert roll.flags == ('-DDMC_ROLLOUT=1',)
  assert keys(_spec(model, task)) == [
      build.model_key(model, task, 'f32', None, (), t.unroll, ()) for t in roll.tiers]
  assert keys(roll) == [build.model_key(model, task, 'f32', None, ('-DDMC_ROLLOUT=1',),
                                        t.unroll, ()) for t in roll.tiers]
  assert _spec(model, task, 'mixed', rollout=True, population=True).flags == (
      '-DDMC_STATE_COMP=1', '-DDMC_ROLLOUT=1', '-DDMC_POLICY_POPULATION=1')


def test_keyword_reaches_physics_and_the_suite():
  import inspect
  from dm_control_amd import engine
  from dm_control_amd import vec_env
  from dm_control_amd.suite import common
  assert 'population' in common.PHYSICS_KWARGS
  for fn in (build.spec, build.build_model, engine.Physics.__init__, vec_env.VecEnv.__init__):
    params = list(inspect.signature(fn).parameters.values())
    assert params[-1].name == 'population' and params[-1].default is False, fn
  with pytest.raises(ValueError, match='rollout=True'):
    engine.Physics(helpers.load_model('cartpole'), batch_size=4, population=True)


# -- the argument block ------------------------------------------------------------------

def test_population_launch_plan(tmp_path):
  exe = str(tmp_path/'population_plan')
  subprocess.check_call(
      ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
       '-fno-sanitize-recover=undefined', '-Wall', '-I', shim_runner.CSRC,
       os.path.join(ROOT, 'tests', 'host_runtime', 'population_plan.cpp'), '-o', exe])
  out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
  assert out.returncode == 0, out.stderr[-3000:]
  assert out.stdout.strip() == 'population ok'


# -- MLPPopulation ------------------------------------------------------------------------

@pytest.mark.parametrize('hidden', [(5,), (5, 64)])
def test_population_layout_round_trip(hidden):
  members = [rollout_cases.make_policy(17, hidden, 6, seed=s) for s in range(5)]
  pop = policy_lib.MLPPopulation.from_policies(members)
  nparams = members[0].packed(np.float64).size
  assert pop.num_members == 5 and pop.nparams == nparams
  assert pop.obs_dim == 17 and pop.action_dim == 6 and pop.widths == tuple(hidden) + (6,)
  for dtype in (np.float64, np.float32):
    packed = pop.packed(dtype)
    assert packed.shape == (nparams, 5) and packed.dtype == dtype
    assert packed.flags['C_CONTIGUOUS']
    for i, p in enumerate(members):                  # one column per member
      np.testing.assert_array_equal(packed[:, i], p.packed(dtype))
      np.testing.assert_array_equal(pop.member(i).packed(dtype), p.packed(dtype))
  # word j of member m at flat index j*P + m
  flat = pop.packed(np.float64).ravel()
  np.testing.assert_array_equal(flat[7*5 + 3], members[3].packed(np.float64)[7])
  theta = np.stack([p.packed(np.float64) for p in members])
  again = policy_lib.MLPPopulation.from_flat(theta, 17, pop.widths)
  np.testing.assert_array_equal(again.packed(np.float64), pop.packed(np.float64))
  one = policy_lib.MLPPopulation.from_policies(members[:1])        # P = 1: the flat block
  np.testing.assert_array_equal(one.packed(np.float64).ravel(), members[0].packed(np.float64))


def test_population_shape_errors_and_update():
  widths, nparams = (3, 2), 3*6 + 2*4
  theta = np.arange(4.0*nparams).reshape(4, nparams)
  pop = policy_lib.MLPPopulation.from_flat(theta, 5, widths)
  assert pop.version == 0 and pop.num_members == 4
  with pytest.raises(ValueError, match='theta must have shape'):
    policy_lib.MLPPopulation.from_flat(theta[:, :-1], 5, widths)
  with pytest.raises(ValueError, match='theta must have shape'):
    policy_lib.MLPPopulation.from_flat(theta[0], 5, widths)
  with pytest.raises(ValueError, match='1 or 2 hidden layers'):
    policy_lib.MLPPopulation.from_flat(theta, 5, (3, 2, 2, 2))
  pop.update_(theta + 1)
  assert pop.version == 1 and pop.member(2).weights[0][0, 0] == theta[2, 0] + 1
  with pytest.raises(ValueError, match='theta must have shape'):
    pop.update_(theta[:3])                   # (the member count stays)
  with pytest.raises(ValueError, match='theta must have shape'):
    pop.update_(theta[:, :-1])
  assert pop.version == 1
  a = rollout_cases.make_policy(5, (3,), 2, seed=0)
  with pytest.raises(ValueError, match='one shape'):
    policy_lib.MLPPopulation.from_policies([a, rollout_cases.make_policy(5, (4,), 2, seed=1)])
  with pytest.raises(ValueError, match='one shape'):
    policy_lib.MLPPopulation.from_policies([a, rollout_cases.make_policy(5, (3, 3), 2, seed=1)])
  with pytest.raises(ValueError, match='at least one member'):
    policy_lib.MLPPopulation.from_policies([])


# -- tier and capability word ---------------------------------------------------------------

def _device_global(path, name):
  """The int32 value of the device global `name` in the gfx950 code object at `path`
  (an ELF, possibly inside an offload bundle), or None if it has no such symbol."""
  with open(path, 'rb') as f:
    data = f.read()
  elf = data[data.index(b'\x7fELF'):]
  shoff, = struct.unpack_from('<Q', elf, 0x28)
  shentsize, shnum = struct.unpack_from('<HH', elf, 0x3A)
  sections = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + k*shentsize) for k in range(shnum)]
  for sec in sections:
    if sec[1] not in (2, 11):                  # SHT_SYMTAB, SHT_DYNSYM
      continue
    strtab = sections[sec[6]]
    for at in range(sec[4], sec[4] + sec[5], sec[9]):
      st_name, _, _, shndx, value, size = struct.unpack_from('<IBBHQQ', elf, at)
      end = elf.index(b'\0', strtab[4] + st_name)
      if elf[strtab[4] + st_name:end] == name.encode() and size == 4:
        home = sections[shndx]
        return struct.unpack_from('<i', elf, home[4] + value - home[3])[0]
  return None


def _tier_of(spec_, path):
  # pylint: disable=protected-access
  names = ['dmc_%s.hsaco' % build._key(spec_, t) for t in spec_.tiers]
  return names.index(os.path.basename(path))


@pytest.mark.timeout(900)
@pytest.mark.parametrize('name,precision', [('cheetah', 'f32'), ('cartpole', 'f64')])
def test_population_builds_cross_compile_on_the_tier_of_their_rollout_builds(name, precision):
  model, task = helpers.load_model(name), helpers.TASKS[name]
  pop_path = build.build_model(model, task, precision, rollout=True, population=True)
  roll_path = build.build_model(model, task, precision, rollout=True)
  assert build._recorded(pop_path)[0] == 'ok'             # pylint: disable=protected-access
  assert pop_path != roll_path
  lds = build.lds_budget_for(None)
  pop = build.spec(model, task, precision, None, None, 'auto', lds, 64, (), True, True)
  roll = build.spec(model, task, precision, None, None, 'auto', lds, 64, (), True)
  assert _tier_of(pop, pop_path) == _tier_of(roll, roll_path)
  caps = _device_global(pop_path, 'dmc_rollout_caps')
  assert caps is not None and caps & 4 and caps & 3 == 3 and caps >> 8 == 64
  plain = _device_global(roll_path, 'dmc_rollout_caps')
  assert plain is not None and not plain & 4 and plain & 3 == 3 and plain >> 8 == 64


# -- the kernel on the host, under sanitizers -----------------------------------------

NENV, NSTEPS = 66, 3        # a full workgroup and a 2-env tail
HIDDEN = (5, 64)
RUN_TIMEOUT = 600


def _build_harness(name, tmp_path, extra=()):
  model = helpers.load_model(name)
  header = tmp_path/'model.h'
  text = codegen.generate_header(model, helpers.TASKS[name], unroll=True)
  header.write_text(text.replace('static __device__ constexpr', 'static constexpr'))
  exe = tmp_path/'population_harness'
  subprocess.check_call(
      ['g++', '-std=c++17', '-w', '-pthread', '-O1', '-g', '-fsanitize=address,undefined',
       '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-DDMC_REAL_IS_DOUBLE',
       '-DDMC_ROLLOUT=1', '-DDMC_POLICY_POPULATION=1'] + list(extra) + [
           '-DDMC_MODEL_HEADER="%s"' % header,
           '-DDMC_KERNEL_SOURCE="%s"' % os.path.join(shim_runner.CSRC, 'dmc_kernels.hip'),
           '-I', shim_runner.CSRC, '-I', shim_runner.SHIM, '-x', 'c++',
           os.path.join(shim_runner.SHIM, 'population_harness.cpp'), '-o', str(exe)])
  return model, str(exe)


def _run(exe, model, qpos, qvel, calls, ctrl=None, pop=None):
  """-> dict: 'obs' / 'reward' / 'action' (the records) and 'final' [n, ...]."""
  widths = (0, 0) if pop is None else (pop.widths[:-1] + (0,))[:2]
  text = '%d %d 1 1 %d %d %d %d %d %d %s\n' % (
      NENV, NSTEPS, ctrl is not None, 0 if pop is None else len(pop.widths) - 1,
      widths[0], widths[1], 1 if pop is None else pop.num_members, len(calls),
      ' '.join('%d' % c for c in calls))
  if pop is not None:
    text += ' '.join('%.17g' % x for x in pop.packed(np.float64).ravel()) + '\n'
  for e in range(NENV):
    text += ' '.join('%.17g' % x for x in np.concatenate([qpos[e], qvel[e]])) + '\n'
  if ctrl is not None:
    text += ' '.join('%.17g' % x for x in np.asarray(ctrl).ravel()) + '\n'
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
  out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=RUN_TIMEOUT)
  assert out.returncode == 0, out.stderr[-3000:]
  rows = {'CALL': [], 'TRAJ': [], 'FINAL': []}
  for line in out.stdout.splitlines():
    tag, _, rest = line.partition(' ')
    rows[tag].append([float(x) for x in rest.replace('|', ' ').split()])
  nobs, nu = len(rows['CALL'][0]) - 3, model.nu
  traj = np.array(rows['TRAJ']).reshape(NSTEPS, NENV, -1)[:, :, 2:]
  assert traj.shape[2] == nobs + 1 + nu
  return {'final': np.array(rows['FINAL'])[:, 1:], 'obs': traj[:, :, :nobs],
          'reward': traj[:, :, nobs], 'action': traj[:, :, nobs + 1:]}


def _same(a, b, keys=('obs', 'reward', 'action', 'final')):
  for k in keys:
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.timeout(3600)
@pytest.mark.parametrize('name,extra', [
    ('cheetah', ('-DDMC_LDS_BUDGET=16384',)),    # rows in LDS and in the workspace
    ('cartpole', ())])                           # the policy sizes the LDS array
def test_population_kernel_on_the_host(name, extra, tmp_path):
  """fp64, 66 envs, T = 3, two hidden layers (5, 64) plus noise; 66 members (one per
  env), 2 (a member boundary inside the first workgroup) and 1: (a) every env acts with
  its own member's MLP, (b) one launch equals T launches, (c) the recorded actions
  replay the rollout, (d) 66 copies of one policy equal the one-member run of that
  policy -- (b) to (d) bit for bit."""
  model, exe = _build_harness(name, tmp_path, extra)
  qpos, qvel = helpers.initial_states(model, name, NENV, seed=7)
  nobs, nu = population_cases.DIMS[name]
  noise = 0.3*np.random.RandomState(3).randn(NSTEPS, NENV, nu)
  single = None
  for members in (66, 2, 1):
    pop = population_cases.make_population(nobs, HIDDEN, nu, members, seed=4)
    one = _run(exe, model, qpos, qvel, [NSTEPS], ctrl=noise, pop=pop)
    assert np.isfinite(one['final']).all() and not one['final'][:, -1].any()   # (no warning bit)
    # the precondition: a neighbour's weights would be told apart, for every env
    population_cases.assert_members_tell_apart(pop, one['obs'][:-1], np.float64, 1.0)
    want, bound = population_cases.member_actions(pop, one['obs'][:-1], np.float64, 1.0)
    err = np.abs(one['action'][1:] - noise[1:] - want)
    assert np.all(err <= 2*bound), (members, float((err/bound).max()))          # (a)
    _same(one, _run(exe, model, qpos, qvel, [1]*NSTEPS, ctrl=noise, pop=pop))   # (b)
    _same(one, _run(exe, model, qpos, qvel, [NSTEPS], ctrl=one['action']))      # (c)
    if members == 1:
      single = (pop, one)
  if name == 'cheetah':
    assert single[1]['final'][:, -4].max() > 0       # (contacts: the solver ran)
  copies = policy_lib.MLPPopulation.from_policies([single[0].member(0)]*NENV)
  _same(single[1], _run(exe, model, qpos, qvel, [NSTEPS], ctrl=noise, pop=copies))   # (d)
