"""Per-env episodes on the MI355X: env mask, step counters, done flags.

Twin tests.  A draw of the initialiser depends on (seed, env) alone and a step
of an env on that env alone, so a launch under a mask is compared bit for bit
with the same launch without one on a second batch (the twin): the envs inside
the mask equal the twin's, the envs outside equal what they held before, in
every field.  No tolerance is involved.  The initialiser's draws are also
compared with tests/device_init_model.py (`shim_runner.compare_init`).
The host-side counterpart under sanitizers is tests/test_episodes.py.
"""

import numpy as np
import pytest

import device_init_model as dim
import helpers
import model_param_cases as mpc
import shim_runner
from dm_control_amd import build
from dm_control_amd import model_params
from dm_control_amd import suite
from dm_control_amd import vec_env
from dm_control_amd import wrapper as W

pytestmark = pytest.mark.gpu

NENV = 67           # two workgroups of the one-lane kernel, the second ragged
INIT = {'qpos': W.FIELD_QPOS, 'qvel': W.FIELD_QVEL, 'warm': W.FIELD_WARMSTART,
        'ctrl': W.FIELD_CTRL, 'time': W.FIELD_TIME, 'episode_return': W.FIELD_RETURN,
        'taskdata': W.FIELD_TASKDATA, 'modelparam': W.FIELD_MODELPARAM}


def _fields(hb):
  """Every field of the batch, and its episode block if it has one, [nenv, ...]."""
  out = {}
  for k, row in enumerate(W.FIELDS):
    a = hb.read(k)
    out[row[0]] = a if row[0] == 'OBS' or a.ndim == 1 else np.ascontiguousarray(a.T)
  if hb.episode_ptr(W.EPISODE_STEP):
    for name, which in (('ep_step', W.EPISODE_STEP), ('ep_done', W.EPISODE_DONE)):
      out[name] = hb.episode_read(which)
  return out


def _same(a, b, envs, names=None, what=''):
  for name in names or [n for n in a if n in b]:
    assert a[name][envs].tobytes() == b[name][envs].tobytes(), (what, name)


def _init_view(hb):
  return {f: hb.read(k).T.reshape(hb.nenv, -1).astype(np.float64) for f, k in INIT.items()}


# ---------------------------------------------------------------------------
# a masked launch against an unmasked twin
# ---------------------------------------------------------------------------
LAUNCH_CASES = {
    # one env per lane: two workgroups, the second ragged
    'cheetah_one_lane': ('cheetah', dict(precision='f32'), NENV, ()),
    'hopper_one_lane': ('hopper', dict(precision='f32'), NENV, ()),
    # several lanes per env
    'hopper_32_lanes': ('hopper', dict(precision='f32', mode='coop', group=32), 5, ()),
    'humanoid_128_lanes': ('humanoid', dict(precision='f32', mode='coop', group=128), 3, ()),
    'cheetah_64_lanes_per_env_fields': (
        'cheetah', dict(precision='f32', mode='coop', group=64, per_env=mpc.ALL_FIELDS), 3,
        mpc.ALL_FIELDS),
}


@pytest.mark.parametrize('which', sorted(LAUNCH_CASES))
def test_masked_launches_against_an_unmasked_twin(which):
  domain, kw, nenv, per_env = LAUNCH_CASES[which]
  model = helpers.load_model(domain)
  hm = W.HipModel(build.build_model(model, helpers.TASKS[domain], **kw))
  a, twin = W.HipBatch(hm, nenv), W.HipBatch(hm, nenv)
  rs = np.random.RandomState(17)
  if per_env:
    params = model_params.ModelParams(model, per_env, nenv)
    block = params.set({'body_mass': model.body_mass*rs.uniform(0.7, 1.3, (nenv, model.nbody)),
                        'dof_damping': model.dof_damping*rs.uniform(0.8, 1.2, (nenv, model.nv))})
  for hb in (a, twin):
    if per_env:
      hb.write(W.FIELD_MODELPARAM, block)
    hb.set_aux_outputs(True)
    hb.init_episode(dim.SEEDS[0])
    hb.forward()
  mask = np.arange(nenv) % 3 != 1             # of 64, 65, 66: one out, two in
  _same(_fields(a), _fields(twin), slice(None), what='same start')
  # the initialiser and the observation pass under the mask: a new draw inside only
  before = _fields(a)
  with a.masked(mask):
    a.init_episode(dim.SEEDS[1])
    a.forward(count_contacts=True)
  twin.init_episode(dim.SEEDS[1])
  twin.forward(count_contacts=True)
  got, want = _fields(a), _fields(twin)
  _same(got, want, mask, what='init inside the mask')
  _same(got, before, ~mask, what='init outside the mask')
  assert (got['QPOS'][mask] != before['QPOS'][mask]).any(axis=1).all()
  # three steps under seeded actions
  for t in range(3):
    ctrl = rs.uniform(-1, 1, (nenv, model.nu))
    with a.masked():
      a.step_host(ctrl, 2)
    twin.step_host(ctrl, 2)
    got, want = _fields(a), _fields(twin)
    _same(got, want, mask, what='step %d inside the mask' % t)
    _same(got, before, ~mask, what='step %d outside the mask' % t)
  assert (got['TIME'][mask] > 0).any()
  # the mask is a launch mode: it is off again
  a.step_host(ctrl, 1)
  assert (_fields(a)['TIME'][~mask] > before['TIME'][~mask]).any()
  for hb in (a, twin):
    hb.free()
  hm.free()


# ---------------------------------------------------------------------------
# Task.reset_done against a twin that ran the whole recipe
# ---------------------------------------------------------------------------
def _checked_init(physics, param, mask_of):
  """Wraps batch.init_episode: every launch is compared with the host model of
  its draw, restricted to the mask in force (mask_of() -> bool [B])."""
  hb = physics.batch
  seeds = []
  launch = hb.init_episode
  domain_task = physics._task_id      # pylint: disable=protected-access

  def init_episode(seed, only_colliding=False):
    before = _init_view(hb)
    ncon = hb.read(W.FIELD_STATS)[0].copy()
    launch(seed, only_colliding)
    want = dim.draw(physics.model, domain_task, param, seed, hb.nenv,
                    dim.FLAG_ONLY_COLLIDING if only_colliding else 0, ncon)
    want.written &= mask_of()
    shim_runner.compare_init(dict(_init_view(hb), before=before), want,
                             hb.model.info.real_size)
    seeds.append(seed)
  hb.init_episode = init_episode
  return seeds


RESET_CASES = [('cheetah', 'run', 0), ('hopper', 'hop', 1), ('humanoid', 'stand', 0),
               ('reacher', 'hard', 0), ('cartpole', 'swingup', 2)]
DONE = [0, 64, 66]


@pytest.mark.parametrize('domain,task_name,param', RESET_CASES, ids=[c[0] for c in RESET_CASES])
def test_reset_done_against_a_twin(domain, task_name, param):
  """cheetah: 200 settle steps, the first one stale, time 0; hopper: the reset
  forward pass of the touch sensors; humanoid: rejection rounds; reacher: the
  target in the task data."""
  envs = [suite.load(domain, task_name, task_kwargs={'random': 5},
                     environment_kwargs={'batch_size': NENV, 'device_init': True})
          for _ in range(2)]
  a, twin = envs
  rs = np.random.RandomState(2)
  for env in envs:
    env.reset()
  for _ in range(2):
    action = rs.uniform(-1, 1, (NENV, a.physics.model.nu))
    for env in envs:
      env.step(action)
  mask = np.zeros(NENV, bool)
  mask[DONE] = True
  before = _fields(a.physics.batch)
  _same(before, _fields(twin.physics.batch), slice(None), what='same start')
  seeds = _checked_init(a.physics, param, lambda: mask)
  twin_seeds = _checked_init(twin.physics, param, lambda: np.ones(NENV, bool))
  a.task.reset_done(a.physics, envs=DONE)
  with twin.physics.reset_context():
    twin.task.initialize_episode(twin.physics)
  assert seeds and seeds == twin_seeds[:len(seeds)]
  if domain == 'humanoid':
    assert len(twin_seeds) >= 2, 'no env collided: the rejection rounds were not exercised'
  got, want = _fields(a.physics.batch), _fields(twin.physics.batch)
  _same(got, want, mask, ('QPOS', 'QVEL', 'WARMSTART', 'TIME', 'OBS', 'SENSORDATA', 'TASKDATA',
                          'CTRL', 'RETURN', 'REWARD', 'WARN'), what='inside the mask')
  _same(got, before, ~mask, what='outside the mask')
  assert (got['TIME'][mask] == 0).all() and (got['TIME'][~mask] > 0).all()
  assert (got['QPOS'][mask] != before['QPOS'][mask]).any(axis=1).all()
  if domain == 'reacher':
    assert (got['TASKDATA'][mask] != before['TASKDATA'][mask]).any(axis=1).all()
  for env in envs:
    env.physics.free()


# ---------------------------------------------------------------------------
# VecEnv(per_env_episodes=True)
# ---------------------------------------------------------------------------
def _staggered_env(torch_io, seed=3):
  # cart-pole: 0.01 s per control step, so 0.045 s is a limit of 5 steps
  env = vec_env.VecEnv('cartpole', 'swingup', NENV, seed=seed, torch_io=torch_io,
                       task_kwargs={'time_limit': 0.045},
                       environment_kwargs={'device_init': True}, per_env_episodes=True,
                       episode_offsets=np.arange(NENV) % 5)
  assert env._batch.step_limit == 5             # pylint: disable=protected-access
  return env


def _watch_reset_pass(env):
  """Records the observation buffer as the step left it, before each reset pass."""
  seen = []
  task, hb = env.environment.task, env.environment.physics.batch
  reset_done = task.reset_done

  def wrapped(physics, envs=None):
    seen.append(hb.read(W.FIELD_OBS).copy())
    reset_done(physics, envs)
  task.reset_done = wrapped
  return seen


@pytest.mark.parametrize('torch_io', [True, False], ids=['torch', 'numpy'])
def test_vec_env_staggered_episodes(torch_io):
  env = _staggered_env(torch_io)
  hb = env._batch                               # pylint: disable=protected-access
  seen = _watch_reset_pass(env)
  obs = env.reset()
  np.testing.assert_array_equal(hb.episode_read(W.EPISODE_STEP), np.arange(NENV) % 5)
  rs = np.random.RandomState(9)
  e = np.arange(NENV)
  if torch_io:
    import torch
  for t in range(12):
    action = rs.uniform(-1, 1, (NENV, env.action_dim))
    if torch_io:
      action = torch.as_tensor(action, dtype=torch.float32, device='cuda')
    npass = len(seen)
    obs, rewards, dones, infos = env.step(action)
    if torch_io:
      obs, dones = obs.cpu().numpy(), dones.cpu().numpy()
      terminal = infos['terminal_observation'].cpu().numpy()
      bad = infos['bad_state'].cpu().numpy()
      assert len(seen) == npass + 1             # issued every step, no host read of `done`
    else:
      bad = np.array([i['bad_state'] for i in infos])
      assert [('terminal_observation' in i) for i in infos] == list(dones)
      assert len(seen) == npass + int(dones.any())
    want = (e % 5 + t + 1) % 5 == 0
    np.testing.assert_array_equal(dones, want, err_msg='step %d' % t)
    assert dones.dtype == bool and not bad.any()
    steps = hb.episode_read(W.EPISODE_STEP)
    np.testing.assert_array_equal(steps, np.where(want, 0, (e % 5 + t + 1) % 5))
    assert not hb.episode_read(W.EPISODE_DONE).any()
    if want.any():
      buffer = seen[-1]                         # what the step launch wrote
      for i in np.nonzero(want)[0]:
        term = terminal[i] if torch_io else infos[i]['terminal_observation']
        np.testing.assert_array_equal(term, buffer[i])
      # done envs report the first observation of their new episode, the others the step's
      np.testing.assert_array_equal(obs[~want], buffer[~want])
      assert (obs[want] != buffer[want]).any(axis=1).all()
    np.testing.assert_array_equal(obs, hb.read(W.FIELD_OBS))
  assert np.isfinite(np.asarray(rewards.cpu() if torch_io else rewards)).all()
  env.close()


def test_vec_env_per_env_episodes_needs_device_init():
  with pytest.raises(ValueError, match='device_init'):
    vec_env.VecEnv('cartpole', 'swingup', 4, per_env_episodes=True)


def test_bad_state_is_a_done_flag_and_a_fresh_draw():
  env, twin = _staggered_env(False), _staggered_env(False)
  for v in (env, twin):
    v.reset()
  physics, hb = env.environment.physics, env._batch       # pylint: disable=protected-access
  qvel = hb.read(W.FIELD_QVEL)
  qvel[0, 6] = np.nan
  hb.write(W.FIELD_QVEL, qvel)
  mask = np.zeros(NENV, bool)
  seeds = _checked_init(physics, 2, lambda: mask)
  action = np.random.RandomState(1).uniform(-1, 1, (NENV, env.action_dim))
  e = np.arange(NENV)
  mask[:] = (e % 5 == 4) | (e == 6)            # the envs at their limit, and the bad one
  obs, _, dones, infos = env.step(action)      # (raises nothing)
  twin.step(action)
  assert [i['bad_state'] for i in infos] == list(e == 6)
  np.testing.assert_array_equal(dones, mask)
  assert len(seeds) == 1 and np.isfinite(obs).all()
  got, want = _fields(hb), _fields(twin._batch)           # pylint: disable=protected-access
  _same(got, want, e != 6, what='the undisturbed envs')
  assert got['WARN'].tolist() == [0]*NENV and not got['ep_done'].any()
  assert got['ep_step'][6] == 0 and np.isfinite(got['QPOS'][6]).all()
  assert not physics._warn_seen.any()                     # pylint: disable=protected-access
  env.close()
  twin.close()


def test_checkpoint_carries_the_episode_block(tmp_path):
  env = _staggered_env(False)
  env.reset()
  physics, hb = env.environment.physics, env._batch       # pylint: disable=protected-access
  rs = np.random.RandomState(4)
  actions = rs.uniform(-1, 1, (5, NENV, env.action_dim))

  def play(acts):      # (Physics alone: nobody resets, finished envs freeze)
    for act in acts:
      physics.set_control(act)
      physics.step(1, check=False)
    return _fields(hb)
  play(actions[:3])
  saved = _fields(hb)
  assert saved['ep_done'].any() and not saved['ep_done'].all()
  physics.save_checkpoint(tmp_path/'episodes')
  after = play(actions[3:])
  assert (after['ep_step'] != saved['ep_step']).any()
  hb.episode_write(W.EPISODE_STEP, np.full(NENV, 99))
  physics.load_checkpoint(tmp_path/'episodes')
  _same(_fields(hb), saved, slice(None), ('ep_step', 'ep_done', 'QPOS', 'QVEL', 'TIME'))
  _same(play(actions[3:]), after, slice(None), what='replayed from the checkpoint')
  # a batch without episodes does not take this checkpoint silently
  plain = suite.load('cartpole', 'swingup', environment_kwargs={'batch_size': NENV})
  with pytest.raises(ValueError, match='per-env episodes'):
    plain.physics.load_checkpoint(tmp_path/'episodes')
  plain.physics.free()
  env.close()


def test_team_build_refuses_the_mask_and_episodes():
  from dm_control_amd.locomotion import soccer as soccer_env
  env = soccer_env.load(1, random_state=5,
                        environment_kwargs={'batch_size': 3, 'precision': 'f64'})
  assert 'team mode' in env.physics.kernel_shape
  hb = env.physics.batch
  for call in (lambda: hb.episodes_enable(5), lambda: hb.set_masked(True),
               lambda: hb.step_host(None, 1, False, False, True)):
    with pytest.raises(W.Error, match='team-mode build'):
      call()
  assert not hb.episode_ptr(W.EPISODE_STEP)
  env.physics.free()
