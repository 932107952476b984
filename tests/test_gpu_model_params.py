"""Per-env model parameters on the device (MI355X): every env of a batch with
its own masses, inertias, damping, armature, stiffness, friction, gears and
gravity, compared per step with the fp64 oracle on a perturbed copy of the
model -- never with the device itself."""

import numpy as np
import pytest

import helpers
import kat_models
import model_param_cases as mpc
from dm_control_amd import build
from dm_control_amd import codegen
from dm_control_amd import wrapper as W
from dm_control_amd.mjcf import compiler
from oracle import oracle

pytestmark = pytest.mark.gpu
ALL = mpc.ALL_FIELDS
NENV, STEPS = 16, 8


def _varied_batch(model, task, precision, mode, group, lds, models, fields=ALL):
  path = build.build_model(model, task, precision, mode=mode, group=group,
                           lds_budget=lds, per_env=fields)
  hm = W.HipModel(path)
  hb = W.HipBatch(hm, len(models))
  layout = codegen.model_param_layout(model, fields)
  assert hm.info.nmodelparam == sum(n for _, n in layout.values())
  # a fresh batch holds the compiled model's values in every env
  fresh = hb.read(W.FIELD_MODELPARAM).astype(np.float64)
  want = codegen.model_param_values(model, layout)
  np.testing.assert_allclose(fresh, np.tile(want[:, None], (1, len(models))),
                             rtol=1e-6 if precision == 'f32' else 0, atol=0)
  if models[0] is not model:
    hb.write(W.FIELD_MODELPARAM, np.array([mpc.block_of(m, layout) for m in models]).T)
  return hm, hb, path


def _teacher_forced(name, precision, mode, group, lds, models, fields=ALL):
  """helpers._teacher_forced with one oracle model per env."""
  if name == 'servo_arm':
    model, task = compiler.from_xml_string(mpc.SERVO_ARM), 0
  else:
    model, task = helpers.load_model(name), helpers.TASKS[name]
  models = models(model)
  nenv = len(models)
  hm, hb, path = _varied_batch(model, task, precision, mode, group, lds, models, fields)
  if name == 'servo_arm':      # around and beyond the shoulder's limit
    rs0 = np.random.RandomState(7)
    qpos, qvel = rs0.uniform(-0.5, 0.5, (nenv, 2)), rs0.randn(nenv, 2)
  else:
    qpos, qvel = helpers.initial_states(model, name, nenv, seed=7)
  datas = []
  for e in range(nenv):
    d = oracle.OracleData(oracle.OracleModel(models[e]))
    d.qpos[:] = qpos[e]
    d.qvel[:] = qvel[e]
    d.step1()
    datas.append(d)
  rs = np.random.RandomState(11)
  errs, rows, nskip = [], 0, 0
  for _ in range(STEPS):
    oq = np.array([d.qpos.copy() for d in datas])
    ov = np.array([d.qvel.copy() for d in datas])
    ow = np.array([d.qacc_warmstart.copy() for d in datas])
    skip = np.array([helpers._degenerate(d, models[e]) for e, d in enumerate(datas)])
    rows += sum(int(d.nefc) for d in datas)
    hb.set_state(oq.T, ov.T, ow.T)
    ctrl = rs.uniform(-1, 1, (nenv, model.nu))
    hb.step_host(ctrl, 1)
    q = hb.read(W.FIELD_QPOS).T.astype(np.float64)
    v = hb.read(W.FIELD_QVEL).T.astype(np.float64)
    for e, d in enumerate(datas):
      d.ctrl[:] = ctrl[e]
      skip[e] |= helpers._degenerate(d, models[e])
      d.physics_step()
    nq = np.array([d.qpos.copy() for d in datas])
    nv = np.array([d.qvel.copy() for d in datas])
    e_ = np.maximum(helpers.rel_err(q, nq), helpers.rel_err(v, nv))
    errs.append(e_[~skip])
    nskip += int(skip.sum())
  assert not hb.read(W.FIELD_WARN).any()
  errs = np.concatenate(errs)
  verdict = open(path + '.verdict').read().strip()
  print('%s %s %s group=%s lds=%s [%s]: max %.3g median %.3g p99 %.3g, %d rows, %d skipped'
        % (name, precision, mode, group, lds, verdict, errs.max(), np.median(errs),
           np.percentile(errs, 99), rows, nskip))
  assert nskip <= 0.02*nenv*STEPS
  if name in ('cheetah', 'humanoid', 'hopper', 'walker', 'servo_arm'):
    assert rows > 0, 'no constraint row was in play'
  if precision == 'f64':
    assert errs.max() <= 1e-9, (name, errs.max())
  else:
    helpers._assert_fp32_per_step(name, errs)
  return verdict


def test_one_lane_varied_builds_cover_the_tiers():
  """The one-lane shapes of the parity test land on the unrolled tier and on the
  generic ones (read from the builds' records, so no device is needed beyond
  the marker): a varied build walks the same ladder as any other."""
  tiers = set()
  for name, precision, mode, group, lds in mpc.gpu_shapes():
    if mode != 'auto':
      continue
    model = helpers.load_model(name)
    s = build.spec(model, helpers.TASKS[name], precision, None, None, mode, lds, group, ALL)
    path = build.realise(s)
    for t in s.tiers:
      if path.endswith('dmc_%s.hsaco' % build._key(s, t)):
        tiers.add(t.unroll)
  print('tiers of the varied one-lane builds:', tiers)
  assert tiers == {True, 'semi', False}       # unrolled, generic with the unroller on, strictly rolled


@pytest.mark.timeout(600)
@pytest.mark.parametrize('mode,group', [('auto', 64), ('coop', 64)])
def test_biased_actuators_read_their_rows(mode, group):
  """Gear, gain and bias parameters per env on actuators that have a bias term
  (position servo, affine general actuator): fp64, 16 parameter sets."""
  def models(model):
    rs = np.random.RandomState(23)
    return [mpc.perturbed(model, rs, mpc.ACTUATOR_FIELDS) for _ in range(NENV)]
  _teacher_forced('servo_arm', 'f64', mode, group, None, models, mpc.ACTUATOR_FIELDS)


def _perturbed_models(model):
  rs = np.random.RandomState(23)
  return [mpc.perturbed(model, rs) for _ in range(NENV)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize('name,precision,mode,group,lds', mpc.gpu_shapes())
def test_per_step_parity_with_sixteen_parameter_sets(name, precision, mode, group, lds):
  _teacher_forced(name, precision, mode, group, lds, _perturbed_models)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('name,precision,mode,group,lds', [
    s for s in mpc.gpu_shapes() if s[0] in ('cheetah', 'humanoid')])
def test_varied_build_left_at_defaults_is_the_nominal_model(name, precision, mode, group, lds):
  _teacher_forced(name, precision, mode, group, lds, lambda model: [model]*NENV)


@pytest.mark.timeout(600)
def test_free_fall_under_per_env_gravity_is_the_euler_sum():
  """A ball above the floor, 64 envs, each with its own gravity g_e: after n
  steps of semi-implicit Euler z = z0 - g_e h^2 n (n + 1)/2, accumulated here
  the way the integrator does (v += h a; z += h v) -- no oracle involved."""
  model = compiler.from_xml_string(kat_models.BALL_ON_FLOOR)
  nenv, steps = 64, 50
  hm = W.HipModel(build.build_model(model, 0, 'f64', per_env=('gravity',)))
  hb = W.HipBatch(hm, nenv)
  g = np.linspace(2.0, 12.0, nenv)
  block = np.zeros((3, nenv))
  block[2] = -g
  hb.write(W.FIELD_MODELPARAM, block)
  qpos = np.tile(model.qpos0, (nenv, 1))
  qpos[:, 2] = 5.0                         # 4.9 m above the floor: 50 steps fall far less
  hb.set_state(qpos.T, np.zeros((model.nv, nenv)))
  h = float(model.opt.timestep)
  z, vz = np.full(nenv, 5.0), np.zeros(nenv)
  for _ in range(steps):
    hb.step_host(None, 1)
    vz = vz + h*(-g)
    z = z + h*vz
  got = hb.read(W.FIELD_QPOS)[2]
  assert (5.0 - z).max() < 4.0 and not hb.read(W.FIELD_WARN).any()
  assert hb.read(W.FIELD_STATS)[0].max() == 0          # no contact on the way
  np.testing.assert_allclose(got, z, rtol=0, atol=1e-12)
  assert np.ptp(got) > 1e-3


@pytest.mark.timeout(900)
def test_public_api_parameters_survive_resets_masks_and_checkpoints(tmp_path):
  from dm_control_amd import suite
  env = suite.load('cheetah', 'run', environment_kwargs={'batch_size': 64, 'per_env': ALL})
  p = env.physics
  m = p.model
  assert p.per_env == ALL
  rs = np.random.RandomState(23)
  mass = m.body_mass*rs.uniform(0.7, 1.3, (64, m.nbody))
  fric = np.array(m.geom_friction)*np.ones((64, 1, 1))
  fric[:, :, 0] *= rs.uniform(0.4, 1.2, (64, m.ngeom))
  p.set_model_params(body_mass=mass, geom_friction=fric)
  block = p.batch.read(W.FIELD_MODELPARAM).copy()
  assert np.ptp(block, axis=1).max() > 0
  env.reset()
  np.testing.assert_array_equal(p.batch.read(W.FIELD_MODELPARAM), block)
  ts = env.step(np.zeros((64, m.nu)))
  while not ts.last():                     # across an episode boundary
    ts = env.step(rs.uniform(-1, 1, (64, m.nu)))
  env.reset()
  np.testing.assert_array_equal(p.batch.read(W.FIELD_MODELPARAM), block)
  np.testing.assert_array_equal(p.get_model_params('body_mass'), mass)
  # a mask touches only the masked envs
  mask = np.arange(64) % 3 == 0
  before = p.get_model_params('body_mass')
  p.set_model_params(body_mass=1.1*m.body_mass, envs=mask)
  after = p.get_model_params('body_mass')
  np.testing.assert_array_equal(after[~mask], before[~mask])
  np.testing.assert_array_equal(after[mask], np.tile(1.1*m.body_mass, (mask.sum(), 1)))
  now = p.batch.read(W.FIELD_MODELPARAM)
  np.testing.assert_array_equal(now[:, ~mask], block[:, ~mask])
  assert np.abs(now[:, mask] - block[:, mask]).max() > 0
  # checkpoint round trip
  p.save_checkpoint(tmp_path/'ck')
  p.set_model_params(body_mass=m.body_mass)
  assert np.abs(p.batch.read(W.FIELD_MODELPARAM) - now).max() > 0
  p.load_checkpoint(tmp_path/'ck')
  np.testing.assert_array_equal(p.batch.read(W.FIELD_MODELPARAM), now)
  np.testing.assert_array_equal(p.get_model_params('body_mass'), after)
  # a field outside per_env of a batch built without it
  plain = suite.load('cheetah', 'run', environment_kwargs={'batch_size': 64})
  with pytest.raises(ValueError):
    plain.physics.set_model_params(body_mass=m.body_mass)


@pytest.mark.timeout(900)
def test_vec_env_steps_with_randomised_parameters():
  import torch
  from dm_control_amd import vec_env
  from dm_control_amd.suite import randomizers
  env = vec_env.VecEnv('cheetah', 'run', 64, seed=1, torch_io=True, per_env=ALL)
  p = env.environment.physics
  randomizers.randomize_model_params(p, np.random.RandomState(5), scale=1.3)
  env.reset()
  act = torch.zeros((64, env.action_dim), device='cuda')
  for t in range(100):
    act.uniform_(-1, 1)
    env.step(act)
  torch.cuda.synchronize()
  assert not p.batch.read(W.FIELD_WARN).any()
  assert np.all(np.isfinite(p.batch.read(W.FIELD_OBS)))
