"""The fused soccer task layer on the MI355X: `soccer.load(..., fused_task=True)`
and `soccer.SoccerVecEnv` against the host path.  Every word of the device's
observation row is compared with `Task.get_observation` / `PitchGeometry` evaluated
in fp64 on the state read back from the same batch, within the forward error
bound of its formula (tests/soccer_fused_model.py: value, bound, and why); copies,
the game block and the rewards must be equal.  The code objects are pre-built by
`__graft_entry__.build()`; the host-shim counterpart is tests/test_soccer_fused.py.
"""

import numpy as np
import pytest

import soccer_fused_model as sfm
from dm_control_amd import codegen
from dm_control_amd import wrapper
from dm_control_amd.locomotion import soccer

pytestmark = pytest.mark.gpu

CMU = codegen.CMU_WALKER_EXTENTS
_ENVS = {}


def _env(team_size, precision, batch, **kw):
  """One environment per configuration for the whole module (a Physics is a few
  hundred MB of workspace for nothing if it is rebuilt per test)."""
  key = (team_size, precision, batch, tuple(sorted(kw.items())))
  if key not in _ENVS:
    _ENVS[key] = soccer.load(team_size, random_state=7, environment_kwargs=dict(
        batch_size=batch, precision=precision), **kw)
  return _ENVS[key]


def _real(precision):
  return np.float64 if precision == 'f64' else np.float32


def _state(physics):
  return (np.asarray(physics.data.qpos, np.float64), np.asarray(physics.data.qvel, np.float64))


def _check(physics, pitch, prev_action, real, label):
  row, reward = physics.fused_observation(), physics.fused_reward()
  qpos, qvel = _state(physics)
  players = (physics.model.nu//CMU[2])
  ratio = sfm.compare(row, reward, pitch, players, CMU, qpos, qvel, prev_action, real, label)
  np.testing.assert_array_equal(reward, row[:, -2])       # the reward IS the goal code
  return ratio


@pytest.mark.parametrize('team_size,precision,batch', [(1, 'f64', 3), (1, 'f32', 3), (2, 'f32', 2)])
def test_every_word_within_its_bound(team_size, precision, batch):
  """Seeded states with random root headings, tilts and joint angles and the ball in
  the air: `forward()`, then one nsub = 1 step under non-zero actions.  2v2 is the
  smallest scene with a teammate and two opponents: it checks the prefix order and
  both teams' rotation of the arena list."""
  env = _env(team_size, precision, batch, fused_task=True)
  physics, pitch, real = env.physics, env.task.pitch, _real(precision)
  assert physics.kernel_shape.startswith('one wavefront per env')
  assert physics.batch.model.info.task == codegen.TASK_SOCCER
  assert physics.batch.model.info.nobs == 2*team_size*(199 + 15*(2*team_size - 1)) + 2
  physics.reset()
  qpos, qvel = sfm.seeded_states(physics.model, 2*team_size, CMU, batch, 21 + team_size, pitch)
  physics.set_state(np.concatenate([qpos, qvel], axis=1))
  physics.forward()
  _check(physics, pitch, np.zeros((batch, physics.model.nu)), real,
         '%dv%d %s forward' % (team_size, team_size, precision))
  action = np.random.RandomState(4).uniform(-1, 1, (batch, physics.model.nu))
  action[0, 0] = 1/3          # (not a `real` number in either precision)
  physics.set_control(action)
  physics.step(1)
  stored = action.astype(real).astype(np.float64)
  _check(physics, pitch, stored, real, '%dv%d %s step' % (team_size, team_size, precision))
  # prev_action is the action given, as the device stores it
  layout = codegen.soccer_observation_layout(2*team_size)
  row = physics.fused_observation()
  for p in range(2*team_size):
    o, n = layout[(p, 'prev_action')]
    np.testing.assert_array_equal(row[:, o:o + n], stored[:, CMU[2]*p:CMU[2]*(p + 1)])
  # one output-producing step since the reset: the episode return is its reward
  np.testing.assert_array_equal(physics.batch.read(wrapper.FIELD_RETURN), physics.fused_reward())


def test_goal_and_off_court_flags_through_set_state():
  """Each goal box, outside the field, inside the field -- and, since the detector
  compares in fp64 against the fp64 boxes, a ball ON a goal-box face and the next
  fp32 number in front of it, in the fp32 build."""
  env = _env(1, 'f32', 3, fused_task=True)
  physics, pitch = env.physics, env.task.pitch
  away_lo, away_hi, away_mid = pitch.away_goal
  home_lo, home_hi, home_mid = pitch.home_goal
  on_face = np.float32(away_lo[0])
  if on_face < away_lo[0]:
    on_face = np.nextafter(on_face, np.float32(np.inf))
  in_front = np.nextafter(on_face, np.float32(-np.inf))
  balls = [(tuple(away_mid), 1, 1), (tuple(home_mid), -1, 1),
           ((0.0, pitch.field[1][1] + 0.5, 0.4), 0, 1), ((1.0, -2.0, 0.4), 0, 0),
           ((float(on_face), 0.5, 0.4), 1, None), ((float(in_front), 0.5, 0.4), 0, None)]
  physics.reset()
  base_q, base_v = sfm.seeded_states(physics.model, 2, CMU, 3, 9, pitch)
  for chunk in (balls[:3], balls[3:]):
    qpos = base_q.copy()
    qpos[:, 126:129] = [b[0] for b in chunk]
    physics.set_state(np.concatenate([qpos, base_v], axis=1))
    physics.forward()
    _check(physics, pitch, np.zeros((3, physics.model.nu)), np.float32, 'flags')
    game = physics.fused_observation()[:, -2:]
    np.testing.assert_array_equal(game[:, 0], [b[1] for b in chunk])
    for e, b in enumerate(chunk):
      if b[2] is not None:
        assert game[e, 1] == b[2], (e, b)
    np.testing.assert_array_equal(physics.fused_reward(), game[:, 0])


def _spy(task, log):
  kick, throw = task.initialize_episode, task._throw_in     # pylint: disable=protected-access
  def initialize_episode(physics, only=None):
    log.append(('kick-off', None if only is None else tuple(np.nonzero(only)[0])))
    return kick(physics, only=only)
  def throw_in(physics, mask):
    log.append(('throw-in', tuple(np.nonzero(mask)[0])))
    return throw(physics, mask)
  task.initialize_episode, task._throw_in = initialize_episode, throw_in   # pylint: disable=protected-access


def _move_ball(physics, pitch_index, pos, vel):
  state = np.asarray(physics.get_state(), np.float64)
  nq = physics.model.nq
  state[pitch_index, 126:129] = pos
  state[pitch_index, nq + 124:nq + 130] = list(vel) + [0, 0, 0]
  physics.set_state(state)


def _shot(pitch):
  """A ball just inside the field's edge in front of the away goal, fast enough to
  be inside the goal box after one control step (0.025 s)."""
  return (pitch.field[1][0] - 0.1, 0.0, 0.3), (15.0, 0.0, 0.0)


def test_twin_environments_give_the_same_timesteps():
  """`load(1, fused_task=True)` next to `load(1)`: same seed, 2 pitches, same random
  actions, 6 control steps; pitch 0's ball is shot into the away goal after step 2
  (it crosses the line during step 3) and pitch 1's ball is put off court after
  step 4.  Rewards, discounts and step types are equal, the pitches that kicked off
  and threw in are the same, and the fused observations lie within their bounds of
  the host formulas on the fused batch's own state, and of the twin's observations."""
  fused = soccer.load(1, random_state=11, fused_task=True,
                      environment_kwargs=dict(batch_size=2, precision='f64'))
  plain = soccer.load(1, random_state=11,
                      environment_kwargs=dict(batch_size=2, precision='f64'))
  assert isinstance(fused.task, soccer.FusedTask) and type(plain.task) is soccer.Task
  logs = {'fused': [], 'plain': []}
  _spy(fused.task, logs['fused'])
  _spy(plain.task, logs['plain'])
  pitch = plain.task.pitch
  steps = [(fused.reset(), plain.reset())]
  rs = np.random.RandomState(2)
  layout = codegen.soccer_observation_layout(2)
  worst = 0.0
  for t in range(6):
    action = [rs.uniform(-1, 1, (2, CMU[2])) for _ in range(2)]
    steps.append((fused.step(action), plain.step(action)))
    tf, tp = steps[-1]
    # the fused row against the host formulas on the fused batch's own state
    worst = max(worst, _check(fused.physics, pitch, np.concatenate(action, axis=1),
                              np.float64, 'twin step %d' % t))
    # ... and against the twin's observations, whose formulas ran on the twin's state
    bound = sfm.bounds(pitch, 2, CMU, *_state(plain.physics), np.float64)
    for (p, name), (o, n) in ((k, v) for k, v in layout.items() if k != 'game'):
      a = np.asarray(tf.observation[p][name]).reshape(2, n)
      b = np.asarray(tp.observation[p][name]).reshape(2, n)
      assert np.all(np.abs(a - b) <= 2*bound[:, o:o + n]), (t, p, name, np.abs(a - b).max())
    if t == 1:
      for env in (fused, plain):
        _move_ball(env.physics, 0, *_shot(pitch))
    if t == 3:
      for env in (fused, plain):
        _move_ball(env.physics, 1, (0.0, pitch.field[1][1] + 0.3, 0.5), (0, 0, 0))
  for t, (tf, tp) in enumerate(steps):
    assert tf.step_type == tp.step_type, t
    if t == 0:
      assert tf.reward is None and tp.reward is None and tf.discount is None
    else:
      np.testing.assert_array_equal(np.stack(tf.reward), np.stack(tp.reward), err_msg=str(t))
      np.testing.assert_array_equal(tf.discount, tp.discount, err_msg=str(t))
    for p in range(2):
      assert list(tf.observation[p]) == list(tp.observation[p])
      for name in tf.observation[p]:
        assert np.shape(tf.observation[p][name]) == np.shape(tp.observation[p][name]), name
  # the goal: reward +1 for the home player, -1 away, discount 0, on pitch 0 at step 3
  np.testing.assert_array_equal(np.stack(steps[3][0].reward), [[1, 0], [-1, 0]])
  np.testing.assert_array_equal(steps[3][0].discount, [0, 1])
  assert logs['fused'] == logs['plain']
  assert ('kick-off', (0,)) in logs['fused'] and ('throw-in', (1,)) in logs['fused']
  # same physics, same host recipes: the twins' states are the same to rounding
  qf, vf = _state(fused.physics)
  qp, vp = _state(plain.physics)
  print('twin: largest state difference %.3e, largest ratio %.3f'
        % (max(np.abs(qf - qp).max(), np.abs(vf - vp).max()), worst))
  np.testing.assert_allclose(qf, qp, rtol=0, atol=1e-9)
  fused.physics.free()
  plain.physics.free()


def test_soccer_vec_env():
  """`SoccerVecEnv`: shapes, `obs` aliasing the device field, rewards and dones equal
  to the numpy twin's (a goal at step 2, the time limit at step 3), CUDA actions
  required."""
  import torch
  kw = dict(time_limit=0.07, environment_kwargs=dict(precision='f64'))
  vec = soccer.SoccerVecEnv(1, 2, seed=5, **kw)
  twin = soccer.load(1, random_state=5, fused_task=True, time_limit=0.07,
                     environment_kwargs=dict(batch_size=2, precision='f64'))
  d = 199 + 15
  obs = vec.reset()
  twin.reset()
  assert tuple(obs.shape) == (2, 2, d) and obs.is_cuda and obs.dtype == torch.float64
  assert obs.data_ptr() == vec.environment.physics.batch.device_ptr(wrapper.FIELD_OBS)
  assert obs.stride() == (2*d + 2, d, 1)
  assert list(vec.layout)[:3] == ['joints_pos', 'joints_vel', 'body_height']
  assert vec.layout['prev_action'] == slice(116, 172) and vec.observation_dim == d
  with pytest.raises(ValueError, match='CUDA'):
    vec.step(torch.zeros(2, 2, 56, dtype=torch.float64))
  with pytest.raises(ValueError, match='shape'):
    vec.step(torch.zeros(2, 112, dtype=torch.float64, device='cuda'))
  rs = np.random.RandomState(8)
  pitch = twin.task.pitch
  for t in range(3):
    if t == 1:
      for env in (vec.environment, twin):
        _move_ball(env.physics, 1, *_shot(pitch))
    action = rs.uniform(-1, 1, (2, 2, 56))
    obs, rewards, dones, infos = vec.step(torch.as_tensor(action, device='cuda'))
    ts = twin.step([action[:, 0], action[:, 1]])
    assert tuple(obs.shape) == (2, 2, d) and tuple(rewards.shape) == (2, 2)
    assert tuple(dones.shape) == (2,) and rewards.is_cuda and dones.is_cuda
    np.testing.assert_array_equal(rewards.cpu().numpy(), np.stack(ts.reward, axis=1))
    np.testing.assert_array_equal(dones.cpu().numpy(), np.full(2, ts.last()))
    np.testing.assert_array_equal(infos['discount'].cpu().numpy(), twin.task.discount(twin.physics))
    np.testing.assert_array_equal(infos['goal'].cpu().numpy(), np.asarray(ts.reward[0]))
    if not ts.last():
      for p in range(2):
        o, n = vec.layout['ball_ego_position'].start, 3
        np.testing.assert_array_equal(obs[:, p, o:o + n].cpu().numpy(),
                                      ts.observation[p]['ball_ego_position'])
    if t == 1:
      np.testing.assert_array_equal(rewards.cpu().numpy(), [[0, 0], [1, -1]])
  assert ts.last() and 'terminal_observation' in infos
  vec.close()
  twin.physics.free()
