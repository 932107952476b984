"""Per-env model parameters (domain randomisation) without a GPU: the block
layout and the generated header, the batched mj_setConst, the kernel sources on
the host under sanitizers next to the oracle, and the Python surface against a
stub batch.  The expected trajectory of an env is always the fp64 oracle on a
deepcopy of the model with that env's values."""

import os
import subprocess

import numpy as np
import pytest

import helpers
import kat_models
import model_param_cases as mpc
from dm_control_amd import build
from dm_control_amd import codegen
from dm_control_amd.mjcf import compiler
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, 'tests', 'host_shim')
CSRC = os.path.join(ROOT, 'dm_control_amd', 'csrc')
ALL = mpc.ALL_FIELDS


# ---------------------------------------------------------------------------
# 1. layout and header
# ---------------------------------------------------------------------------
def test_header_without_per_env_is_the_plain_header():
  m, task = helpers.load_model('cheetah'), helpers.TASKS['cheetah']
  for unroll in (True, False):
    plain = codegen.generate_header(m, task, unroll=unroll)
    assert codegen.generate_header(m, task, unroll=unroll, per_env=()) == plain
    assert 'DMC_VARY' not in plain and 'NMODELPARAM' not in plain
  assert codegen.model_param_layout(m, ()) == {}


def test_varied_header_defines_switches_and_block_size():
  m, task = helpers.load_model('cheetah'), helpers.TASKS['cheetah']
  layout = codegen.model_param_layout(m, ALL)
  total = sum(n for _, n in layout.values())
  # contiguous, in order, no overlap
  at = 0
  for name, (off, n) in layout.items():
    assert off == at and n > 0
    at += n
  assert set(layout) == set(codegen.MODEL_PARAM_ROWS)
  text = codegen.generate_header(m, task, per_env=ALL)
  for name, (off, _) in layout.items():
    assert '#define DMC_VARY_%s 1' % name.upper() in text
    assert '#define DMC_MP_%s %d\n' % (name.upper(), off) in text
  assert '#define DMC_NMODELPARAM %d\n' % total in text
  assert 'constexpr int NMODELPARAM = %d;' % total in text
  assert 'model_param_default[]' in text
  # the defaults are the compiled model's values
  vals = codegen.model_param_values(m, layout)
  o, n = layout['body_mass']
  np.testing.assert_array_equal(vals[o:o + n], m.body_mass)
  o, n = layout['gravity']
  np.testing.assert_array_equal(vals[o:o + n], m.opt.gravity)
  # one field: its rows and what follows from it, nothing else
  assert list(codegen.model_param_layout(m, ('geom_friction',))) == ['pair_friction', 'pair_diag']
  assert list(codegen.model_param_layout(m, ('body_mass',))) == [
      'body_mass', 'body_subtreemass', 'dof_invweight0', 'meaninertia', 'pair_diag']
  assert list(codegen.model_param_layout(m, ('opt.gravity',))) == ['gravity']
  one = codegen.generate_header(m, task, per_env=('gravity',))
  assert 'DMC_VARY_GRAVITY 1' in one and 'DMC_VARY_BODY_MASS' not in one


def test_unknown_field_and_team_mode_raise():
  m = helpers.load_model('cheetah')
  with pytest.raises(ValueError) as err:
    codegen.model_param_layout(m, ('geom_size',))
  assert 'geom_size' in str(err.value) and 'body_mass' in str(err.value)
  with pytest.raises(ValueError):
    build.spec(m, 2, 'f32', None, (), 'auto', None, 64, ('body_pos',))
  with pytest.raises(codegen.UnsupportedModelError) as err:
    build.spec(m, 0, 'f32', 64, (), 'team', None, 64, ('body_mass',))
  assert 'team' in str(err.value)
  # per_env enters the spec and the content key; () keeps the key of today
  plain = build.spec(m, 2, 'f32', None, (), 'auto', None, 64)
  varied = build.spec(m, 2, 'f32', None, (), 'auto', None, 64, ('gravity', 'body_mass'))
  assert plain.per_env == () and varied.per_env == ('body_mass', 'gravity')
  assert build._key(plain, plain.tiers[0]) != build._key(varied, varied.tiers[0])
  assert build._key(plain, plain.tiers[0]) == build.model_key(m, 2, 'f32', None, (), True)


# ---------------------------------------------------------------------------
# 3. the kernel sources on the host (ASan + UBSan, fp64) next to the oracle
# ---------------------------------------------------------------------------
def _header(model, task, tmp_path, unroll, per_env):
  header = tmp_path/'model.h'
  text = codegen.generate_header(model, task, unroll=unroll, per_env=per_env)
  header.write_text(text.replace('static __device__ constexpr', 'static constexpr'))
  return header


def _build_one_lane(model, task, tmp_path, unroll, per_env):
  header = _header(model, task, tmp_path, unroll, per_env)
  exe = tmp_path/'harness_mp'
  subprocess.check_call(
      ['g++', '-std=c++17', '-w', '-O1', '-g', '-fsanitize=address,undefined',
       '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
       '-DDMC_REAL_IS_DOUBLE', '-DDMC_LDS_BUDGET=16384',
       '-DDMC_MODEL_HEADER="%s"' % header,
       '-DDMC_KERNEL_SOURCE="%s"' % os.path.join(CSRC, 'dmc_kernels.hip'),
       '-I', CSRC, '-I', SHIM, '-x', 'c++', os.path.join(SHIM, 'harness_mp.cpp'),
       '-o', str(exe)])
  return str(exe)


def _build_coop(model, task, tmp_path, group, per_env):
  header = _header(model, task, tmp_path, True, per_env)
  exe = tmp_path/'harness_coop_mp'
  subprocess.check_call(
      ['g++', '-fno-sanitize-recover=undefined', '-std=c++17', '-O1', '-g', '-pthread',
       '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
       '-DDMC_REAL_IS_DOUBLE', '-DDMC_GROUP=%d' % min(group, 64),
       '-DDMC_COOP_DUO=%d' % (group == 128),
       '-DDMC_MODEL_HEADER="%s"' % header,
       '-DDMC_KERNEL_SOURCE="%s"' % os.path.join(CSRC, 'dmc_coop.hip'),
       '-I', CSRC, '-I', SHIM, '-x', 'c++', os.path.join(SHIM, 'harness_coop_mp.cpp'),
       '-o', str(exe)])
  return str(exe)


def _fmt(values):
  return ['%.17g' % v for v in np.asarray(values, float).ravel()]


def _steps_of(stdout, has_env):
  for line in stdout.splitlines():
    if line.startswith('STEP'):
      vals, tail = line.split('|')
      f = vals.split()
      e = int(f[2]) if has_env else 0
      yield e, np.array([float(x) for x in f[3 if has_env else 2:]]), [int(x) for x in tail.split()]


def _oracle_at(model, qpos, qvel):
  d = oracle.OracleData(oracle.OracleModel(model))
  d.qpos[:] = qpos
  d.qvel[:] = qvel
  d.ctrl[:] = mpc.harness_ctrl(model.nu)
  d.step1()
  return d


def _check_next_to_oracle(rows, models, nominal, q, v, steps):
  """rows: (env, state, (ncon, nefc, iters, warn)) in step order.  models[e]: the
  perturbed copy of env e.  Bounds of tests/test_kernel_sanitizers.py."""
  nq = nominal.nq
  datas = [_oracle_at(m, q[e], v[e]) for e, m in enumerate(models)]
  plain = [_oracle_at(nominal, q[e], v[e]) for e in range(len(models))]
  seen, touched = 0, False
  for e, state, (ncon, nefc, iters, warn) in rows:
    d = datas[e]
    touched |= d.nefc > 0
    assert (ncon, nefc) == (d.ncon, d.nefc)
    d.physics_step()
    assert warn == 0
    np.testing.assert_allclose(state[:nq], d.qpos, rtol=0, atol=1e-9)
    np.testing.assert_allclose(state[nq:], d.qvel, rtol=0, atol=1e-8)
    seen += 1
  assert seen == steps*len(models)
  assert touched
  # not vacuous: the perturbed and the nominal model have moved apart
  for e, d in enumerate(datas):
    for _ in range(steps):
      plain[e].physics_step()
    gap = max(np.abs(plain[e].qpos - d.qpos).max(), np.abs(plain[e].qvel - d.qvel).max())
    assert gap > 1e-6, 'env %d: perturbed and nominal oracle differ by %g only' % (e, gap)


def _case(name):
  if name == 'primitives':
    model, task = compiler.from_xml_string(kat_models.PRIMITIVES), 0
    qpos, qvel = model.qpos0.copy(), np.zeros(model.nv)
    qpos[2], qpos[9], qpos[16] = 0.11, 0.2, 0.3     # stacked, in contact
    return model, task, qpos, qvel, 40
  if name == 'servo_arm':
    model = compiler.from_xml_string(mpc.SERVO_ARM)
    return model, 0, np.array([0.35, -0.6]), np.array([1.5, -0.8]), 60   # runs into the limit
  model, task = helpers.load_model(name), helpers.TASKS[name]
  q, v = helpers.initial_states(model, name, 4, seed=7)
  return model, task, q[1], v[1], 25


@pytest.mark.timeout(900)
@pytest.mark.parametrize('name,unroll,fields', [
    ('cheetah', True, ALL), ('cheetah', False, ALL), ('hopper', True, ALL),
    ('primitives', False, ALL)] +
    # one field at a time.  The cheetah's motors have no bias term (biastype
    # none, all actuator_biasprm zero), so its kernels never read that row: the
    # servo arm, whose actuators have one, stands in for that single case and
    # also runs with gear, gain and bias varied together, unrolled and rolled
    [('cheetah', True, (f,)) for f in ALL if f != 'actuator_biasprm'] +
    [('servo_arm', True, ('actuator_biasprm',)), ('servo_arm', True, mpc.ACTUATOR_FIELDS),
     ('servo_arm', False, mpc.ACTUATOR_FIELDS), ('servo_arm', True, ALL)])
def test_one_lane_source_reads_the_block(name, unroll, fields, tmp_path):
  model, task, qpos, qvel, steps = _case(name)
  assert np.any(getattr(model, fields[0]) if fields[0] != 'gravity' else model.opt.gravity)
  p = mpc.perturbed(model, np.random.RandomState(23), fields)
  layout = codegen.model_param_layout(model, fields)
  exe = _build_one_lane(model, task, tmp_path, unroll, fields)
  args = [exe, str(steps)] + _fmt(mpc.block_of(p, layout)) + _fmt(qpos) + _fmt(qvel)
  out = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
  assert out.returncode == 0, out.stderr[-3000:]
  _check_next_to_oracle(list(_steps_of(out.stdout, False)), [p], model, [qpos], [qvel], steps)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('name,group,steps', [('humanoid', 64, 9), ('humanoid', 128, 9),
                                              ('cheetah', 32, 12), ('servo_arm', 64, 40),
                                              ('servo_arm', 32, 40)])
def test_several_lanes_source_reads_the_block(name, group, steps, tmp_path):
  """csrc/dmc_coop.hip through shim_coop.h, every env of the workgroup with its
  own parameters (one env per wavefront, with the helper wavefront, two envs
  per wavefront)."""
  nenv = max(1, 64//group)
  if name == 'servo_arm':       # actuators with a bias term: every actuator row is read
    model, task = compiler.from_xml_string(mpc.SERVO_ARM), 0
    q = np.array([[0.35, -0.6], [-0.3, 0.9]])[:nenv]
    v = np.array([[1.5, -0.8], [-2.0, 0.5]])[:nenv]
  else:
    model, task = helpers.load_model(name), helpers.TASKS[name]
    q, v = helpers.initial_states(model, name, max(nenv, 2), seed=7)
    q, v = q[-nenv:], v[-nenv:]
  rs = np.random.RandomState(23)
  models = [mpc.perturbed(model, rs) for _ in range(nenv)]
  layout = codegen.model_param_layout(model, ALL)
  exe = _build_coop(model, task, tmp_path, group, ALL)
  args = [exe, str(steps), '1']
  for e in range(nenv):
    args += _fmt(mpc.block_of(models[e], layout)) + _fmt(q[e]) + _fmt(v[e])
  out = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=1100,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
  assert out.returncode == 0, out.stderr[-3000:]
  _check_next_to_oracle(list(_steps_of(out.stdout, True)), models, model, q, v, steps)


# ---------------------------------------------------------------------------
# 2. batched mj_setConst against compiler._set_const
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cheetah', 'hopper', 'humanoid'])
def test_batched_set_const_agrees_with_the_compiler(name):
  from dm_control_amd import model_params
  model = helpers.load_model(name)
  rs = np.random.RandomState(23)
  models = [mpc.perturbed(model, rs) for _ in range(8)]
  P = model_params.ModelParams(model, ALL, 8)
  block = P.set({
      'body_mass': np.array([m.body_mass for m in models]),
      'body_inertia': np.array([m.body_inertia for m in models]),
      'dof_damping': np.array([m.dof_damping for m in models]),
      'dof_armature': np.array([m.dof_armature for m in models]),
      'jnt_stiffness': np.array([m.jnt_stiffness for m in models]),
      'actuator_gear': np.array([m.actuator_gear for m in models]),
      'actuator_gainprm': np.array([m.actuator_gainprm for m in models]),
      'actuator_biasprm': np.array([m.actuator_biasprm for m in models]),
      'geom_friction': np.array([m.geom_friction for m in models]),
      'gravity': np.array([m.opt.gravity for m in models])})
  assert block.shape == (P.nrows, 8)
  for e, m in enumerate(models):
    want = codegen.model_param_values(m, P.layout)
    for row, (o, n) in P.layout.items():
      gap = np.abs(block[o:o + n, e] - want[o:o + n])/np.maximum(np.abs(want[o:o + n]), 1e-300)
      print(name, e, row, gap.max() if n else 0.0)
      np.testing.assert_allclose(block[o:o + n, e], want[o:o + n], rtol=1e-12, atol=0,
                                 err_msg='%s env %d row %s' % (name, e, row))


# ---------------------------------------------------------------------------
# 4. the Python surface against a stub batch
# ---------------------------------------------------------------------------
class _StubBatch:
  def __init__(self):
    self.writes = []

  def write(self, field, array):
    self.writes.append((field, np.array(array)))


def _stub_physics(per_env, nenv=4, name='cheetah'):
  from dm_control_amd import engine, model_params
  phys = engine.Physics.__new__(engine.Physics)
  phys.model = helpers.load_model(name)
  phys._params = model_params.ModelParams(phys.model, per_env, nenv)
  phys._batch = _StubBatch()
  phys._dirty = False
  phys.named = engine._Named.__new__(engine._Named)
  phys.named.model = engine._NamedModel(phys.model, phys)
  return phys


def test_set_model_params_shapes_masks_and_errors():
  from dm_control_amd import wrapper
  phys = _stub_physics(('body_mass', 'geom_friction', 'gravity'))
  m = phys.model
  assert phys.per_env == ('body_mass', 'geom_friction', 'gravity')
  before = phys.get_model_params('body_mass')
  assert before.shape == (4, m.nbody)
  np.testing.assert_array_equal(before, np.tile(m.body_mass, (4, 1)))
  # broadcast [nbody] to every env; the block goes to the device field
  phys.set_model_params(body_mass=1.5*m.body_mass)
  field, block = phys._batch.writes[-1]
  assert field == wrapper.FIELD_MODELPARAM and block.shape == (phys._params.nrows, 4)
  np.testing.assert_array_equal(phys.get_model_params('body_mass'), np.tile(1.5*m.body_mass, (4, 1)))
  o, n = phys._params.layout['body_mass']
  np.testing.assert_array_equal(block[o:o + n, 2], 1.5*m.body_mass)
  # derived rows followed (mj_setConst): subtree mass of the world = total mass
  o, n = phys._params.layout['body_subtreemass']
  np.testing.assert_allclose(block[o, 0], 1.5*m.body_mass.sum(), rtol=1e-14)
  # a mask touches only the masked envs, bit for bit
  mask = np.array([False, True, False, True])
  keep = phys.get_model_params('body_mass')
  keep_diag = phys.get_model_params('pair_diag')
  phys.set_model_params(body_mass=np.stack([0.8*m.body_mass, 0.9*m.body_mass]), envs=mask)
  now = phys.get_model_params('body_mass')
  np.testing.assert_array_equal(now[[0, 2]], keep[[0, 2]])
  np.testing.assert_array_equal(phys.get_model_params('pair_diag')[[0, 2]], keep_diag[[0, 2]])
  np.testing.assert_array_equal(now[1], 0.8*m.body_mass)
  np.testing.assert_array_equal(now[3], 0.9*m.body_mass)
  # index arrays; set_const=False leaves the derived rows alone
  diag = phys.get_model_params('pair_diag')
  phys.set_model_params(body_mass=2*m.body_mass, envs=[0], set_const=False)
  np.testing.assert_array_equal(phys.get_model_params('pair_diag'), diag)
  np.testing.assert_array_equal(phys.get_model_params('body_mass')[0], 2*m.body_mass)
  # errors: wrong shape, field outside per_env, mask of the wrong length, not SPD
  nwrites = len(phys._batch.writes)
  with pytest.raises(ValueError):
    phys.set_model_params(body_mass=np.ones(3))
  with pytest.raises(ValueError) as err:
    phys.set_model_params(dof_damping=np.ones(m.nv))
  assert 'immutable' in str(err.value) and 'per_env' in str(err.value)
  with pytest.raises(ValueError):
    phys.set_model_params(gravity=[0, 0, -1.0], envs=np.array([True, False]))
  with pytest.raises(ValueError) as err:
    phys.set_model_params(body_mass=-m.body_mass, envs=[2])
  assert 'positive definite' in str(err.value) and '2' in str(err.value)
  assert len(phys._batch.writes) == nwrites            # nothing was written


def test_named_model_routes_writes_of_per_env_fields():
  phys = _stub_physics(('body_mass', 'geom_friction'))
  m = phys.model
  torso = m.name2id('torso', 'body')
  phys.named.model.body_mass['torso'] = 1.3*m.body_mass[torso]        # scalar: every env
  got = phys.get_model_params('body_mass')
  np.testing.assert_array_equal(got[:, torso], np.full(4, 1.3*m.body_mass[torso]))
  other = [b for b in range(m.nbody) if b != torso]
  np.testing.assert_array_equal(got[:, other], np.tile(m.body_mass[other], (4, 1)))
  per_env = np.array([1.0, 2.0, 3.0, 4.0])
  phys.named.model.body_mass['torso'] = per_env                        # [B]
  np.testing.assert_array_equal(phys.get_model_params('body_mass')[:, torso], per_env)
  phys.named.model.geom_friction['ground', 0] = 0.5
  np.testing.assert_array_equal(
      phys.get_model_params('geom_friction')[:, m.name2id('ground', 'geom'), 0], np.full(4, 0.5))
  # reads still show the compiled model; other fields refuse as before
  assert phys.named.model.body_mass['torso'] == m.body_mass[torso]
  with pytest.raises(ValueError) as err:
    phys.named.model.jnt_stiffness[0] = 1.0
  assert 'the compiled model is immutable' in str(err.value) and 'per_env' in str(err.value)


def test_randomize_model_params_draws_inside_the_range():
  from dm_control_amd.suite import randomizers
  phys = _stub_physics(('body_mass', 'body_inertia', 'gravity'), nenv=16)
  m = phys.model
  out = randomizers.randomize_model_params(phys, np.random.RandomState(1), scale=1.3)
  assert set(out) == {'body_mass', 'body_inertia', 'gravity'}
  mass = phys.get_model_params('body_mass')
  live = m.body_mass > 0
  ratio = mass[:, live]/m.body_mass[live]
  assert np.all(ratio >= 1/1.3 - 1e-12) and np.all(ratio <= 1.3 + 1e-12) and ratio.std() > 0.01
  g = phys.get_model_params('gravity')
  assert np.all(g[:, :2] == 0) and len(set(g[:, 2])) == 16
  inertia = phys.get_model_params('body_inertia')[:, live]/m.body_inertia[live]
  np.testing.assert_allclose(inertia[..., 0], inertia[..., 1], rtol=1e-14)
