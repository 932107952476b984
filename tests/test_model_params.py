"""Per-env model parameters (domain randomisation) without a GPU: the block
layout and the generated header, the batched mj_setConst, the kernel sources on
the host under sanitizers next to the oracle, and the Python surface against a
stub batch.  The expected trajectory of an env is always the fp64 oracle on a
deepcopy of the model with that env's values."""

import numpy as np
import pytest

import helpers
import model_param_cases as mpc
import shim_runner
from dm_control_amd import build
from dm_control_amd import codegen

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
def _check_next_to_oracle(rows, models, nominal, q, v, ctrl, steps):
  """rows of shim_runner.run.  models[e]: the perturbed copy of env e."""
  touched, datas = shim_runner.compare(rows, models, q, v, ctrl, steps)
  assert touched
  # not vacuous: the perturbed and the nominal model have moved apart
  for e, d in enumerate(datas):
    plain = shim_runner.oracle_at(nominal, q[e], v[e], ctrl)
    for _ in range(steps):
      plain.physics_step()
    gap = max(np.abs(plain.qpos - d.qpos).max(), np.abs(plain.qvel - d.qvel).max())
    assert gap > 1e-6, 'env %d: perturbed and nominal oracle differ by %g only' % (e, gap)


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
  model, task, q, v, steps = shim_runner.case(name)
  assert np.any(getattr(model, fields[0]) if fields[0] != 'gravity' else model.opt.gravity)
  p = mpc.perturbed(model, np.random.RandomState(23), fields)
  layout = codegen.model_param_layout(model, fields)
  # a constant, non-zero control: the actuator rows matter
  ctrl = mpc.alternating_ctrl(model.nu)
  exe = shim_runner.build(model, task, tmp_path, unroll=unroll, per_env=fields)
  rows = shim_runner.run(exe, steps, q, v, ctrl, blocks=[mpc.block_of(p, layout)])
  _check_next_to_oracle(rows, [p], model, q, v, ctrl, steps)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('name,group,steps', [('humanoid', 64, 9), ('humanoid', 128, 9),
                                              ('cheetah', 32, 12), ('servo_arm', 64, 40),
                                              ('servo_arm', 32, 40)])
def test_several_lanes_source_reads_the_block(name, group, steps, tmp_path):
  """csrc/dmc_coop.hip through the host shim, every env of the workgroup with
  its own parameters (one env per wavefront, with the helper wavefront, two envs
  per wavefront).  The servo arm's actuators have a bias term: every actuator
  row is read."""
  nenv = max(1, 64//group)
  model, task, q, v, _ = shim_runner.case(name, nenv)
  rs = np.random.RandomState(23)
  models = [mpc.perturbed(model, rs) for _ in range(nenv)]
  layout = codegen.model_param_layout(model, ALL)
  ctrl = mpc.alternating_ctrl(model.nu)
  exe = shim_runner.build(model, task, tmp_path, group=group, per_env=ALL)
  rows = shim_runner.run(exe, steps, q, v, ctrl, timeout=1100,
                         blocks=[mpc.block_of(m, layout) for m in models])
  _check_next_to_oracle(rows, models, model, q, v, ctrl, steps)


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
