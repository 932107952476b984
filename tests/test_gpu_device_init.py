"""The episode initialiser of the shipped code objects (MI355X) against the
host model of its draws (tests/device_init_model.py): every value that
`dmc_init_episode` writes, for one line per recipe branch, in f32 and f64
(cart-pole also `mixed`), on batches of 67 envs and of one env.  The reference
of every comparison is the float64 model, the tolerance the one it derives or
measured on the CPU (`device_init_model.atol`); each test prints the largest
error it saw in that unit.
"""

import numpy as np
import pytest

import device_init_model as dim
import helpers
import model_param_cases as mpc
import shim_runner
from dm_control_amd import build
from dm_control_amd import suite
from dm_control_amd import wrapper as W

pytestmark = pytest.mark.gpu

FIELDS = {'qpos': W.FIELD_QPOS, 'qvel': W.FIELD_QVEL, 'warm': W.FIELD_WARMSTART,
          'ctrl': W.FIELD_CTRL, 'time': W.FIELD_TIME, 'episode_return': W.FIELD_RETURN,
          'taskdata': W.FIELD_TASKDATA, 'modelparam': W.FIELD_MODELPARAM}
STATE = ('qpos', 'qvel', 'taskdata')


def _read(hb, fields=shim_runner.INIT_FIELDS):
  """{field: [nenv, k]} as float64 (exact for either `real`)."""
  return {f: hb.read(FIELDS[f]).T.reshape(hb.nenv, -1).astype(np.float64) for f in fields}


def _batch(domain, poles, precision, nenv, param):
  """The humanoid on the env-major code object `Physics` selects for it (64
  lanes per env and a helper wavefront), every other domain on its
  one-env-per-lane code object (whatever `Physics` would pick for the batch
  size: the public-path tests below run that)."""
  model = dim.case_model(domain, poles)
  kw = {'mode': 'coop', 'group': 128} if domain == 'humanoid' else {}
  hm = W.HipModel(build.build_model(model, helpers.TASKS[domain], precision, **kw))
  assert bool(hm.info.env_major) == (domain == 'humanoid')
  hb = W.HipBatch(hm, nenv)
  hb.set_task_params(param)
  return model, hm, hb


def _dirty(hb, model, nenv):
  """A few steps under random controls, so that warm start, control, time and
  return hold something for the initialiser to clear."""
  rs = np.random.RandomState(3)
  for _ in range(3):
    hb.step_host(rs.uniform(-1, 1, (nenv, model.nu)), 1)
  hb.write(W.FIELD_RETURN, hb.read(W.FIELD_RETURN) + 1)
  before = _read(hb)
  for f in ('warm', 'ctrl', 'time', 'episode_return'):
    assert np.all(np.any(before[f] != 0, axis=1)), f
  return before


_LINES = [(c, p) for c in dim.CASES for p in ('f32', 'f64')] + [(dim.CASES[0], 'mixed')]


@pytest.mark.parametrize('case,precision', _LINES,
                         ids=['%s-%s' % (c[0], p) for c, p in _LINES])
def test_init_episode_writes_the_model_draw(case, precision):
  label, domain, poles, param = case
  worst = dict.fromkeys(dim.KINDS, 0.0)
  for nenv in (dim.NENV, 1):
    model, hm, hb = _batch(domain, poles, precision, nenv, param)
    assert hm.info.real_size == (8 if precision == 'f64' else 4)
    for seed in dim.SEEDS:
      before = _dirty(hb, model, nenv)
      hb.init_episode(seed)
      got = dict(_read(hb), before=before)
      want = dim.draw(model, helpers.TASKS[domain], param, seed, nenv)
      seen = shim_runner.compare_init(got, want, hm.info.real_size)
      worst = {k: max(worst[k], seen[k]) for k in dim.KINDS}
    hb.free()
    hm.free()
  print('%s %s: largest error of a measured-bound value, in eps*scale: %s'
        % (label, precision, ', '.join('%s %.1f (bound %.0f)' % (
            k, worst[k], dim.bound_in_eps(hm.info.real_size, k)) for k in dim.KINDS)))


@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_only_colliding_redraws_exactly_the_colliding_envs(precision):
  nenv = 64
  model, hm, hb = _batch('humanoid', None, precision, nenv, 0)
  planted = np.arange(nenv) % 3 == 1
  rs = np.random.RandomState(5)
  qpos = np.tile(model.qpos0, (nenv, 1))
  qpos[:, 0] = 1e-3*np.arange(nenv)            # every env its own words
  qpos[planted, 2] = 0.2                       # the torso into the floor
  hb.set_state(qpos.T, 0.1*rs.randn(model.nv, nenv), rs.randn(model.nv, nenv),
               1.0 + np.arange(nenv))
  hb.write(W.FIELD_RETURN, 2.0 + np.arange(nenv))
  hb.forward(count_contacts=True)
  ncon = hb.read(W.FIELD_STATS)[0]
  assert np.all(ncon[planted] > 0) and (ncon == 0).sum() >= nenv//3
  before = _read(hb)
  hb.init_episode(dim.SEED_ONLY_COLLIDING, only_colliding=True)
  got = dict(_read(hb), before=before)
  want = dim.draw(model, helpers.TASKS['humanoid'], 0, dim.SEED_ONLY_COLLIDING, nenv,
                  dim.FLAG_ONLY_COLLIDING, stats_ncon=ncon)
  # the envs with ncon > 0 are the model's draw for the new seed, the rest bit
  # for bit what they were
  worst = shim_runner.compare_init(got, want, hm.info.real_size)
  assert (got['qpos'][ncon == 0] == before['qpos'][ncon == 0]).all()
  assert (got['qpos'][ncon > 0, 3:] != before['qpos'][ncon > 0, 3:]).all()
  print('only_colliding %s: %d of %d envs redrawn, %.1f eps*scale'
        % (precision, (ncon > 0).sum(), nenv, worst['plain']))


def _recording(physics):
  """Wraps batch.init_episode: (seed, only_colliding, the contact counts the
  device held when it was called)."""
  calls = []
  launch = physics.batch.init_episode

  def init_episode(seed, only_colliding=False):
    calls.append((seed, only_colliding, physics.batch.read(W.FIELD_STATS)[0].copy()))
    launch(seed, only_colliding)
  physics.batch.init_episode = init_episode
  return calls


@pytest.mark.parametrize('domain,task_name,param', [('cartpole', 'swingup', 2), ('reacher', 'hard', 0)])
def test_public_reset_starts_from_the_draw_of_the_seed_it_hands_over(domain, task_name, param):
  env = suite.load(domain, task_name, task_kwargs={'random': dim.PUBLIC_RANDOM},
                   environment_kwargs={'batch_size': dim.NENV, 'device_init': True})
  physics = env.physics
  calls = _recording(physics)
  real_size = physics.batch.model.info.real_size
  for episode in (1, 2):
    env.reset()
    assert len(calls) == episode and not calls[-1][1]
    # nothing follows the draw in these tasks: state and target are the model's
    want = dim.draw(physics.model, helpers.TASKS[domain], param, calls[-1][0], dim.NENV)
    fields = STATE if want.taskdata is not None else STATE[:2]
    shim_runner.compare_init(_read(physics.batch, fields), want, real_size, fields)
  seeds = [c[0] for c in calls]
  assert seeds == dim.product_seeds(dim.PUBLIC_RANDOM, 2) and seeds[0] != seeds[1]
  physics.free()


def test_public_humanoid_reset_keeps_each_env_at_its_first_clean_draw():
  nenv = 64
  env = suite.load('humanoid', 'stand', task_kwargs={'random': dim.PUBLIC_RANDOM},
                   environment_kwargs={'batch_size': nenv, 'device_init': True})
  physics = env.physics
  calls = _recording(physics)
  env.reset()
  seeds = [c[0] for c in calls]
  assert seeds == dim.product_seeds(dim.PUBLIC_RANDOM, len(seeds)) and len(set(seeds)) == len(seeds)
  assert len(seeds) >= 2, 'no env collided: the redraw was not exercised'
  assert not calls[0][1] and all(c[1] for c in calls[1:])
  # round r redraws the envs the device reported as colliding after round r - 1,
  # so an env ends on the seed of the first round after which it was clean
  colliding = np.array([c[2] > 0 for c in calls[1:]])                # [rounds - 1, nenv]
  final = np.array([int(np.argmin(np.append(colliding[:, e], False))) for e in range(nenv)])
  assert np.all(np.cumprod(colliding, axis=0) == colliding), 'a clean env was reported colliding later'
  real_size = physics.batch.model.info.real_size
  qpos = _read(physics.batch, ('qpos',))['qpos']
  draws = [dim.draw(physics.model, helpers.TASKS['humanoid'], 0, s, nenv) for s in seeds]
  tol = dim.atol(draws[0], 'qpos', real_size)
  real = np.float32 if real_size == 4 else np.float64

  def is_draw(row, d):       # exact columns: the model rounded to `real`; the others within `tol`
    return bool(np.all(np.where(tol > 0, np.abs(row - d) <= tol,
                                row == d.astype(real).astype(np.float64))))
  for e in range(nenv):
    match = [is_draw(qpos[e], d.qpos[e]) for d in draws]
    assert match == [r == final[e] for r in range(len(seeds))], (e, match, final[e])
  assert final.max() == len(seeds) - 1 and (final == 0).any()
  assert not np.any(np.atleast_1d(physics.data.ncon) > 0)
  physics.free()


def test_reset_of_a_per_env_batch_keeps_parameters_and_task_data():
  env = suite.load('cheetah', 'run', environment_kwargs={'batch_size': 64, 'per_env': mpc.ALL_FIELDS})
  p, m = env.physics, env.physics.model
  rs = np.random.RandomState(23)
  p.set_model_params(body_mass=m.body_mass*rs.uniform(0.7, 1.3, (64, m.nbody)))
  p.batch.write(W.FIELD_TASKDATA, 1.0 + np.arange(64.0)[None])     # (the padding row of a task without task data)
  before = _dirty(p.batch, m, 64)
  assert np.ptp(before['modelparam'], axis=0).max() > 0
  p.reset()
  got = dict(_read(p.batch), before=before)
  want = dim.draw(m, helpers.TASKS['cheetah'], 0, 0, 64, dim.FLAG_RESET_ONLY)
  shim_runner.compare_init(got, want, p.batch.model.info.real_size)
  np.testing.assert_array_equal(got['modelparam'], before['modelparam'])
  np.testing.assert_array_equal(got['taskdata'], before['taskdata'])
  np.testing.assert_array_equal(got['qpos'], np.tile(m.qpos0, (64, 1)))
  p.free()
