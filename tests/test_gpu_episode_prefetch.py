"""Episode prefetch on the MI355X: the next whole-batch episode start computed
on a side stream into shadow buffers (`dmc_batch_episode_prefetch`) and handed
over at the reset (`dmc_batch_episode_take`).

Twin tests: a batch that takes a prefetch against one that runs the ordinary
launches (reset, draw, settle step) with the same seed.  A draw depends on
(seed, env) alone and the settle on the drawn state alone, so every comparison
is bitwise; no tolerance is involved.  The host side (seed look-ahead, firing
arithmetic) is tests/test_episode_prefetch_host.py.
"""

import numpy as np
import pytest
import torch

import helpers
import model_param_cases as mpc
from dm_control_amd import suite
from dm_control_amd import wrapper as W
from test_gpu_step_sequence import FIELDS as STEP_FIELDS

pytestmark = pytest.mark.gpu

NENV = 130          # one env per lane: two full workgroups and a 2-env tail
NSUB_SETTLE = 200   # suite/cheetah.py
FIELDS = STEP_FIELDS + (('taskdata', W.FIELD_TASKDATA),)
SETTLE = dict(stale_first=True, zero_time=True)


def _fields(hb):
  return {name: hb.read(fid) for name, fid in FIELDS}


def _assert_same(a, b, what):
  for name, _ in FIELDS:
    assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (what, name)


# ---------------------------------------------------------------------------
# through the suite: cheetah-run with device-side initialisation
# ---------------------------------------------------------------------------
def _env(prefetch, per_env=(), nenv=NENV):
  """cheetah-run on the one-env-per-lane kernel; `takes` records what every
  `episode_take` of the batch answered."""
  env = suite.load('cheetah', 'run', task_kwargs={'random': 5},
                   environment_kwargs={'batch_size': nenv, 'device_init': True,
                                       'build_mode': 'auto', 'per_env': per_env})
  assert env.physics.batch.model.info.lanes_per_env == 1
  env.task.prefetch = prefetch
  batch = env.physics.batch
  env.takes = []
  take = batch.episode_take
  batch.episode_take = lambda *a, **kw: env.takes.append(take(*a, **kw)) or env.takes[-1]
  return env


def _actions(seed):
  gen = torch.Generator(device='cuda')
  gen.manual_seed(seed)
  return torch.rand(5, NENV, 6, device='cuda', dtype=torch.float32, generator=gen)*2 - 1


def _step5(env, acts):
  env.physics.batch.step_device_n(acts.data_ptr(), 1, 6, NENV*6, 5,
                                  env._n_sub_steps)   # pylint: disable=protected-access


def _free(*envs):
  for env in envs:
    env.physics.free()


def test_prefetched_resets_equal_ordinary_ones_bit_for_bit():
  a, twin = _env(True), _env(False)
  acts = _actions(0)
  for episode in range(2):
    for env in (a, twin):
      env.reset()
    _assert_same(_fields(a.physics.batch), _fields(twin.physics.batch), 'reset %d' % episode)
    for env in (a, twin):
      _step5(env, acts)
    got = _fields(a.physics.batch)
    _assert_same(got, _fields(twin.physics.batch), 'steps of episode %d' % episode)
  # the first reset found no prefetch and started one (at once: no episode length
  # to go by yet); the second took it; the twin never asked
  assert a.takes == [False, True] and twin.takes == []
  assert got['stats'][0].max() > 0 and got['time'].min() > 0 and not got['warn'].any()
  _free(a, twin)


def test_a_draw_from_the_task_stream_declines_the_take():
  a, twin = _env(True), _env(False)
  for env in (a, twin):
    env.reset()
    env.task.random.uniform()          # the next device seed is no longer the one looked ahead
    env.reset()
  assert a.takes == [False, False]
  _assert_same(_fields(a.physics.batch), _fields(twin.physics.batch), 'declined take')
  # the prefetch of that reset is good again
  for env in (a, twin):
    env.reset()
  assert a.takes == [False, False, True]
  _assert_same(_fields(a.physics.batch), _fields(twin.physics.batch), 'next take')
  _free(a, twin)


def test_a_model_parameter_write_invalidates_the_prefetch():
  a, twin = _env(True, mpc.ALL_FIELDS), _env(False, mpc.ALL_FIELDS)
  m = a.physics.model
  mass = m.body_mass*np.random.RandomState(3).uniform(0.7, 1.3, (NENV, m.nbody))
  for env in (a, twin):
    env.reset()                        # (a: the prefetch reads the compiled model's masses)
    env.physics.set_model_params(body_mass=mass)
    env.reset()
  assert a.takes == [False, False]
  default = _env(False, mpc.ALL_FIELDS)
  default.reset()
  default.reset()
  got = _fields(a.physics.batch)
  _assert_same(got, _fields(twin.physics.batch), 'after the write')
  assert got['qpos'].tobytes() != _fields(default.physics.batch)['qpos'].tobytes()
  # the prefetch started after the write reads the new masses
  for env in (a, twin):
    env.reset()
  assert a.takes == [False, False, True]
  _assert_same(_fields(a.physics.batch), _fields(twin.physics.batch), 'take after the write')
  _free(a, twin, default)


def test_only_batches_that_leave_half_the_chip_empty_prefetch():
  """128 workgroups of 64 envs ask for a prefetch, 129 do not (suite/cheetah.py)."""
  for nenv, takes in ((8192, [False, True]), (8193, [])):
    env = _env(True, nenv=nenv)
    env.reset()
    env.reset()
    assert env.takes == takes, nenv
    assert not env.physics.batch.read(W.FIELD_WARN).any()
    _free(env)


# ---------------------------------------------------------------------------
# through the C ABI
# ---------------------------------------------------------------------------
def _batches(count, precision='f32', nenv=NENV, **kw):
  hm, first = helpers._device_batch(    # pylint: disable=protected-access
      helpers.load_model('cheetah'), helpers.TASKS['cheetah'], precision, nenv, **kw)
  return hm, [first] + [W.HipBatch(hm, nenv) for _ in range(count - 1)]


def _ordinary(hb, seed, nsub):
  hb.reset()
  hb.init_episode(seed)
  hb.step_host(None, nsub, want_outputs=False, **SETTLE)


def _steps(hb, n, seed=1):
  rs = np.random.RandomState(seed)
  for _ in range(n):
    hb.step_host(rs.uniform(-1, 1, (hb.nenv, 6)), 1)


def test_the_request_fires_after_the_steps_it_names():
  hm, (a, twin) = _batches(2)
  a.episode_prefetch(77, NSUB_SETTLE, after_steps=8, **SETTLE)
  _steps(a, 5)
  assert a.episode_take(77, NSUB_SETTLE, **SETTLE) is False     # not issued yet, and forgotten
  _steps(a, 8)
  assert a.episode_take(77, NSUB_SETTLE, **SETTLE) is False
  a.episode_prefetch(77, NSUB_SETTLE, after_steps=8, **SETTLE)
  _steps(a, 8)
  a.reset()
  assert a.episode_take(78, NSUB_SETTLE, **SETTLE) is False     # another seed
  a.episode_prefetch(77, NSUB_SETTLE, after_steps=8, **SETTLE)
  _steps(a, 8)
  a.reset()
  assert a.episode_take(77, NSUB_SETTLE, **SETTLE) is True
  assert a.episode_take(77, NSUB_SETTLE, **SETTLE) is False     # taken once
  _ordinary(twin, 77, NSUB_SETTLE)
  for hb in (a, twin):
    hb.forward(count_contacts=True)
  _assert_same(_fields(a), _fields(twin), 'take after 8 steps')
  for hb in (a, twin):
    hb.free()
  hm.free()


def test_free_right_after_a_prefetch_was_issued():
  hm, (a,) = _batches(1)
  a.episode_prefetch(9, NSUB_SETTLE, after_steps=0, **SETTLE)    # in flight
  a.free()
  b, twin = W.HipBatch(hm, NENV), W.HipBatch(hm, NENV)
  for hb in (b, twin):
    _ordinary(hb, 10, 3)
    _steps(hb, 3)
  got = _fields(b)
  _assert_same(got, _fields(twin), 'a new batch on the same model')
  assert np.all(np.isfinite(got['qpos'])) and got['time'].min() > 0 and not got['warn'].any()
  for hb in (b, twin):
    hb.free()
  hm.free()


def test_masked_and_per_env_episode_batches_refuse():
  hm, (a, b) = _batches(2, nenv=67)
  with a.masked(np.arange(67) % 2 == 0):
    with pytest.raises(W.Error, match='whole-batch episode; the batch has an env mask set'):
      a.episode_prefetch(1, NSUB_SETTLE, **SETTLE)
  b.episodes_enable(10)
  with pytest.raises(W.Error, match='the batch has per-env episodes enabled'):
    b.episode_prefetch(1, NSUB_SETTLE, **SETTLE)
  lib = W.get_lib()                    # settle steps produce no outputs
  assert lib.dmc_batch_episode_prefetch(a.ptr, 1, 20, W.STEP_OUTPUTS | W.STEP_ZERO_TIME, 0) != 0
  assert b'no outputs' in lib.dmc_last_error()
  # ... and a request made before the mask went on is dropped by it
  a.episode_prefetch(1, 20, **SETTLE)
  with a.masked():
    pass
  a.reset()
  assert a.episode_take(1, 20, **SETTLE) is False
  for hb in (a, b):
    hb.free()
  hm.free()


@pytest.mark.parametrize('precision,kw,nenv', [
    ('f32', {}, NENV),
    ('mixed', {}, 66),                           # the low words of the state live in the workspace
    ('f32', dict(mode='coop', group=64), 5),     # several lanes per env, env-major fields
])
def test_short_settle_through_the_c_api(precision, kw, nenv):
  """settle_nsub = 20: a take against the ordinary launches, then three steps."""
  hm, (a, twin) = _batches(2, precision, nenv, **kw)
  for hb in (a, twin):
    _ordinary(hb, 3, 5)                # an episode that leaves state, warm start and workspace behind
    _steps(hb, 2)
  a.episode_prefetch(41, 20, **SETTLE)
  _steps(a, 2, seed=2)
  _steps(twin, 2, seed=2)
  a.reset()
  assert a.episode_take(41, 20, **SETTLE) is True
  _ordinary(twin, 41, 20)
  for hb in (a, twin):
    hb.forward(count_contacts=True)
  got = _fields(a)
  _assert_same(got, _fields(twin), 'after the take')
  assert not got['time'].any() and np.ptp(got['qpos'], axis=1).min() > 0
  for hb in (a, twin):
    _steps(hb, 3, seed=4)
  got = _fields(a)
  _assert_same(got, _fields(twin), 'three steps on')
  assert got['time'].min() > 0
  for hb in (a, twin):
    hb.free()
  hm.free()
