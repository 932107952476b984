"""Host logic of per-env episodes without a device: `VecEnv(per_env_episodes=True)`
in numpy mode and `Task.reset_done` over a stand-in for the batch that does the
kernels' bookkeeping in numpy (count, done at the limit, freeze, clear on init).
What the kernels themselves do is tests/test_episodes.py (host shim) and
tests/test_gpu_episodes.py (MI355X)."""

import contextlib
import types

import numpy as np
import pytest

from dm_control_amd import engine
from dm_control_amd import suite
from dm_control_amd import vec_env
from dm_control_amd import wrapper as W
from dm_control_amd.suite import cartpole


class _Batch:
  """The episode block and the launch modes of `wrapper.HipBatch`."""

  masked = W.HipBatch.masked

  def __init__(self, n, nobs=5):
    self.nenv, self.is_masked, self.episodes, self.step_limit = n, False, False, 0
    self.block = np.zeros((3, n), np.int32)
    self.obs = np.zeros((n, nobs), np.float32)
    self.model = types.SimpleNamespace(info=types.SimpleNamespace(nobs=nobs))
    self.launches = []

  def episodes_enable(self, limit):
    self.episodes, self.step_limit = True, limit

  def episode_read(self, which):
    return self.block[which].copy()

  def episode_write(self, which, array):
    self.block[which] = np.ascontiguousarray(array, dtype=np.int32)

  def mask_from_done(self):
    self.block[W.EPISODE_MASK] = self.block[W.EPISODE_DONE]

  def set_masked(self, on):
    self.is_masked = bool(on)

  def init_episode(self, seed, only_colliding=False):
    sel = self.block[W.EPISODE_MASK] != 0 if self.is_masked else np.ones(self.nenv, bool)
    self.launches.append(('init', sel.copy()))
    self.block[W.EPISODE_STEP][sel] = 0
    self.block[W.EPISODE_DONE][sel] = 0
    self.obs[sel] = -1 - seed % 89           # the first observation of a new episode

  def free(self):
    pass


class _Physics:
  enable_episodes = engine.Physics.enable_episodes
  episode_done = engine.Physics.episode_done

  def __init__(self, n):
    self._batch = _Batch(n)
    self.batch_size = n
    self._warn_seen = np.ones(n, np.uint32)
    self.bad = np.zeros(n, bool)             # envs whose next step raises a warning

  batch = property(lambda self: self._batch)

  def set_control(self, action):
    self.action = action

  def step(self, nsub, check=True):
    assert not check                        # a bad state must not raise in this mode
    b = self._batch
    step, done = b.block[W.EPISODE_STEP], b.block[W.EPISODE_DONE]
    live = done == 0
    step[live] += 1
    done[live] = ((step[live] >= b.step_limit)*W.DONE_LIMIT) | (self.bad[live]*W.DONE_BAD_STATE)
    self.bad[:] = False
    b.obs[live] += 1

  def fused_observation(self):
    return self._batch.obs.astype(np.float64)

  def fused_reward(self):
    return np.zeros(self.batch_size)

  @contextlib.contextmanager
  def reset_context(self):
    self._batch.block[:2] = 0
    yield self
    self.after_reset()

  def after_reset(self):
    self._batch.launches.append(('forward', self._batch.is_masked))

  def free(self):
    pass


@pytest.fixture
def fake_suite(monkeypatch):
  def load(domain_name, task_name, task_kwargs=None, environment_kwargs=None):
    kw = environment_kwargs
    task = cartpole.Balance(True, False, random=task_kwargs.get('random'),
                            device_init=kw['device_init'])
    spec = types.SimpleNamespace(minimum=-1.0, maximum=1.0, shape=(1,))
    return types.SimpleNamespace(physics=_Physics(kw['batch_size']), task=task, _n_sub_steps=1,
                                 _step_limit=4.5, action_spec=lambda: spec)
  monkeypatch.setattr(suite, 'load', load)


def _env(n, **kw):
  return vec_env.VecEnv('cartpole', 'swingup', n, seed=1,
                        environment_kwargs={'device_init': True}, per_env_episodes=True, **kw)


def test_vec_env_numpy_mode_staggered_episodes(fake_suite):
  n = 7
  env = _env(n, episode_offsets=np.arange(n) % 5)
  batch, physics = env._batch, env._physics          # pylint: disable=protected-access
  assert batch.step_limit == 5                       # ceil(4.5): `count >= limit` of Environment
  env.reset()
  np.testing.assert_array_equal(batch.block[W.EPISODE_STEP], np.arange(n) % 5)
  phase = np.arange(n) % 5
  for t in range(12):
    before = batch.obs.copy()
    npass = len(batch.launches)
    if t == 5:
      physics.bad[2] = True
    obs, rewards, dones, infos = env.step(np.zeros((n, 1)))
    want = (phase + t + 1) % 5 == 0
    bad = (np.arange(n) == 2) & (t == 5)
    assert not (want & bad).any()
    np.testing.assert_array_equal(dones, want | bad)
    assert dones.dtype == bool and rewards.shape == (n,)
    assert [i['bad_state'] for i in infos] == list(bad)
    for i in range(n):
      if dones[i]:          # the step's observation, before the reset; then a new episode's first
        np.testing.assert_array_equal(infos[i]['terminal_observation'], before[i] + 1)
        assert obs[i, 0] < 0 and batch.block[W.EPISODE_STEP][i] == 0
      else:
        assert 'terminal_observation' not in infos[i]
        np.testing.assert_array_equal(obs[i], before[i] + 1)
    assert not batch.block[W.EPISODE_DONE].any() and not batch.is_masked
    if dones.any():         # one masked init and one masked observation pass, over the done envs
      (kind, sel), forward = batch.launches[npass:]
      assert kind == 'init' and (sel == dones).all() and forward == ('forward', True)
      assert not physics._warn_seen.any()            # pylint: disable=protected-access
    else:                   # numpy mode has read `done` anyway: no pass
      assert len(batch.launches) == npass
    if t == 5:
      phase[2] = 4                                   # env 2 restarted after step 5: next limit at step 10


def test_episode_offsets_and_refusals(fake_suite):
  np.testing.assert_array_equal(_env(7, episode_offsets='staggered')._offsets, [0, 0, 1, 2, 2, 3, 4])   # pylint: disable=protected-access
  assert not _env(3)._offsets.any()                  # pylint: disable=protected-access
  with pytest.raises(ValueError, match='device_init'):
    vec_env.VecEnv('cartpole', 'swingup', 3, per_env_episodes=True)
  with pytest.raises(ValueError, match='shape'):
    _env(3, episode_offsets=[0, 1])
  with pytest.raises(ValueError, match='per_env_episodes'):
    vec_env.VecEnv('cartpole', 'swingup', 3, episode_offsets='staggered')


def test_reset_done_of_chosen_envs_and_refusals(fake_suite):
  env = _env(5)
  task, physics, batch = env.environment.task, env._physics, env._batch   # pylint: disable=protected-access
  env.reset()
  task.reset_done(physics, envs=[1, 3])
  (kind, sel), forward = batch.launches[-2:]
  assert kind == 'init' and sel.tolist() == [False, True, False, True, False]
  assert forward == ('forward', True) and not batch.is_masked
  assert physics._warn_seen.tolist() == [1, 0, 1, 0, 1]                   # pylint: disable=protected-access
  host = cartpole.Balance(True, False, random=0, device_init=False)
  with pytest.raises(ValueError, match='device_init'):
    host.reset_done(physics)
