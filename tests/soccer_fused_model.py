"""What the tests of the fused soccer task layer share (tests/test_soccer_fused.py
on the host shim, tests/test_gpu_soccer_fused.py on the MI355X): the yardstick, the
error bound of every word of the observation row, and a scene of toy walkers.

The yardstick is the product's own host path: `soccer.Task.get_observation`,
`PitchGeometry.in_goal` and `PitchGeometry.off_court`, evaluated in fp64 on the
state the device (or the shim) hands back.  Next to it, `bounds` restates each
formula's operations and gives its first-order forward error bound in `real`,
k*u*sum|terms| with u = eps/2; a word of the device row must lie within 2*bound of
the host's (each side has its own rounding), a word whose bound is 0 must be
equal.  No bound is taken from what the kernel returns.

Operation counts (standard model, one rounding per +, -, *; an FMA only removes
one).  q = (w, x, y, z) is a root quaternion AS STORED, so it carries no error:

  m  diagonal    1 - 2*(a*a + b*b)      2 products, 1 sum, 1 difference (x2 is
                 exact): k = 3 over |1| + 2*(a*a + b*b)
     other       2*(a*b +- c*d)         2 products, 1 sum: k = 2 over 2*(|ab| + |cd|)
     `absm` is that sum of |terms| per entry, KM = 3 covers both.
  world_zaxis    row 2 of m: KM*u*absm
  v . m (n = 2, 3 terms), v = a - b of stored words:
                 1 difference, n products and n - 1 sums on top of m's own error:
                 k = 1 + n + KM over sum_i |v_i|*absm_ij          (7 and 6)
  arena features the same with a = the fp64 feature rounded to `real` (one more
                 rounding, of relative size u, on |a_i| instead of |v_i|): the
                 term u*sum_i |a_i|*absm_ij is added
  ball angular velocity: first v = mb . w_local (3 products, 2 sums over mb's
                 error: k = 3 + KM = 6 over absv_i = sum_c absmb_ic*|w_c|), then
                 v . m with that v: k = 6 + 3 + KM = 12 over sum_i absv_i*absm_ij
  orientation    sum_j m_ji*mo_jk: 3 products, 2 sums, two matrices' errors:
                 k = 3 + 2*KM = 9 over sum_j absm_ji*absmo_jk
  joints_pos, joints_vel, body_height, prev_action: copies, bound 0
  game block, reward: decided in fp64 against the fp64 boxes, bound 0
"""

import collections
import contextlib
import types

import numpy as np

from dm_control_amd import codegen
from dm_control_amd.locomotion import soccer

KM = 3

# Two toy walkers (a free trunk, two hinged limbs with motors: nq 9, nv 8, nu 2)
# and a ball: the smallest scene `codegen.soccer_trees` accepts.
TOY_EXTENTS = (9, 8, 2)


def _toy_walker(i, x):
  return """
    <body name='w{i}' pos='{x} 0 0.6'>
      <freejoint name='w{i}_root'/>
      <geom name='w{i}_trunk' type='capsule' fromto='0 0 -0.15 0 0 0.15' size='0.08' mass='2'/>
      <body name='w{i}_leg' pos='0 0.1 -0.2'>
        <joint name='w{i}_hip' type='hinge' axis='0 1 0' damping='0.1'/>
        <geom name='w{i}_leg' type='capsule' fromto='0 0 0 0 0 -0.25' size='0.04' mass='0.5'/>
      </body>
      <body name='w{i}_arm' pos='0 -0.1 0.1'>
        <joint name='w{i}_shoulder' type='hinge' axis='1 0 0' damping='0.1'/>
        <geom name='w{i}_arm' type='capsule' fromto='0 0 0 0 -0.2 0' size='0.03' mass='0.3'/>
      </body>
    </body>""".format(i=i, x=x)


def toy_scene_xml(num_walkers=2, with_ball=True, odd_walker=False):
  """`odd_walker`: the last walker loses its arm (the players then differ)."""
  bodies = ''.join(_toy_walker(i, -1.0 + 2.0*i) for i in range(num_walkers))
  if odd_walker:
    cut = bodies.rindex("<body name='w%d_arm'" % (num_walkers - 1))
    end = bodies.index('</body>', cut) + len('</body>')
    bodies = bodies[:cut] + bodies[end:]
  motors = ''.join(
      "<motor name='w{i}_{j}' joint='w{i}_{j}' gear='2'/>".format(i=i, j=j)
      for i in range(num_walkers) for j in ('hip', 'shoulder')
      if not (odd_walker and i == num_walkers - 1 and j == 'shoulder'))
  ball = """
    <body name='ball' pos='0 0 0.5'>
      <freejoint name='ball_free'/>
      <geom name='ball' type='sphere' size='0.1' mass='0.2'/>
    </body>""" if with_ball else ''
  return """
<mujoco model='toy_soccer'>
  <option timestep='0.005'/>
  <worldbody>
    <geom name='ground' type='plane' size='20 20 0.1'/>
    {bodies}{ball}
  </worldbody>
  <actuator>{motors}</actuator>
</mujoco>""".format(bodies=bodies, ball=ball, motors=motors)


TOY_PITCH = (6.0, 4.5) + soccer.MINI_FOOTBALL_GOAL_SIZE


@contextlib.contextmanager
def host_extents(extents):
  """`soccer.Task` reads the walker extents from its module: inside, they are
  `extents` (the toy walkers'), so that the host formulas run on a toy scene."""
  names = ('NQ_WALKER', 'NV_WALKER', 'NU_WALKER')
  saved = [getattr(soccer, n) for n in names]
  for n, v in zip(names, extents):
    setattr(soccer, n, v)
  try:
    yield
  finally:
    for n, v in zip(names, saved):
      setattr(soccer, n, v)


def host_row(pitch, num_players, extents, qpos, qvel, prev_action):
  """The observation row [B, NOBS] and the home reward [B] of the HOST path on the
  state (qpos, qvel) [B, ...] in fp64: `Task.get_observation` laid out by
  `codegen.soccer_observation_layout`, then the goal code and the off-court flag
  from `PitchGeometry.in_goal` / `off_court` as `Task.after_step` applies them."""
  qpos, qvel = np.asarray(qpos, np.float64), np.asarray(qvel, np.float64)
  layout = codegen.soccer_observation_layout(num_players, extents)
  with host_extents(extents):
    task = soccer.Task(num_players//2, pitch, random=0)
    task._prev_action = np.asarray(prev_action, np.float64)   # pylint: disable=protected-access
    physics = types.SimpleNamespace(
        data=types.SimpleNamespace(qpos=qpos, qvel=qvel), batch_size=len(qpos))
    obs = task.get_observation(physics)
    task.after_step(physics)
    reward = np.asarray(task.get_reward(physics)[0], np.float64)     # a home player's
    ball = qpos[:, task._ball_q:task._ball_q + 3]             # pylint: disable=protected-access
  row = np.zeros((len(qpos), layout['game'][0] + 2))
  for key, (offset, extent) in layout.items():
    if key != 'game':
      row[:, offset:offset + extent] = np.asarray(obs[key[0]][key[1]]).reshape(len(qpos), extent)
  at = layout['game'][0]
  row[:, at] = reward
  row[:, at + 1] = pitch.off_court(ball)
  return row, reward


def _mat_abs(q):
  """(m, absm) [B, 3, 3]: `soccer._quat_to_mat` and the sum of |terms| per entry."""
  w, x, y, z = (q[..., k] for k in range(4))
  m = soccer._quat_to_mat(q)      # pylint: disable=protected-access
  a = np.empty_like(m)
  a[..., 0, 0] = 1 + 2*(y*y + z*z); a[..., 1, 1] = 1 + 2*(x*x + z*z); a[..., 2, 2] = 1 + 2*(x*x + y*y)
  a[..., 0, 1] = a[..., 1, 0] = 2*(np.abs(x*y) + np.abs(w*z))
  a[..., 0, 2] = a[..., 2, 0] = 2*(np.abs(x*z) + np.abs(w*y))
  a[..., 1, 2] = a[..., 2, 1] = 2*(np.abs(y*z) + np.abs(w*x))
  return m, a


def bounds(pitch, num_players, extents, qpos, qvel, real):
  """[B, NOBS]: the forward error bound of every word (module docstring); 0: exact."""
  qpos, qvel = np.asarray(qpos, np.float64), np.asarray(qvel, np.float64)
  u = np.finfo(real).eps/2
  nq, nv, _ = extents
  layout = codegen.soccer_observation_layout(num_players, extents)
  bq, bv = nq*num_players, nv*num_players
  B = len(qpos)
  out = np.zeros((B, layout['game'][0] + 2))
  mats = [_mat_abs(qpos[:, nq*k + 3:nq*k + 7]) for k in range(num_players)]
  _, absmb = _mat_abs(qpos[:, bq + 3:bq + 7])
  absv_ball = np.einsum('bic,bc->bi', absmb, np.abs(qvel[:, bv + 3:bv + 6]))
  box = codegen.soccer_boxes(tuple(pitch.size) + tuple(pitch.goal_size))
  def ego(v, absm, k):      # k*u*sum_i |v_i|*absm_ij
    n = v.shape[-1]
    return k*u*np.einsum('bi,bij->bj', np.abs(v), absm[:, :n, :n])
  for (p, name), (offset, extent) in ((k, v) for k, v in layout.items() if k != 'game'):
    pos, lin = qpos[:, nq*p:nq*p + 3], qvel[:, nv*p:nv*p + 3]
    _, absm = mats[p]
    sl = slice(offset, offset + extent)
    if name in ('joints_pos', 'joints_vel', 'body_height', 'prev_action'):
      continue
    if name == 'world_zaxis':
      out[:, sl] = KM*u*absm[:, 2, :]
    elif name == 'ball_ego_angular_velocity':
      out[:, sl] = ego(absv_ball, absm, 12)
    elif name == 'ball_ego_position':
      out[:, sl] = ego(qpos[:, bq:bq + 3] - pos, absm, 1 + 3 + KM)
    elif name == 'ball_ego_linear_velocity':
      out[:, sl] = ego(qvel[:, bv:bv + 3] - lin, absm, 1 + 3 + KM)
    elif name.endswith('_ego_linear_velocity') or name.endswith('_ego_position') or \
        name.endswith('_ego_orientation'):
      # the j-th other player in index order
      kind, index = name.split('_')[0], int(name.split('_')[1])
      half = num_players//2
      same = [j for j in range(num_players) if j != p and (j < half) == (p < half)]
      rest = [j for j in range(num_players) if (j < half) != (p < half)]
      j = (same if kind == 'teammate' else rest)[index]
      if name.endswith('_ego_linear_velocity'):
        out[:, sl] = ego(qvel[:, nv*j:nv*j + 3] - lin, absm, 1 + 3 + KM)
      elif name.endswith('_ego_position'):
        out[:, sl] = ego(qpos[:, nq*j:nq*j + 3] - pos, absm, 1 + 3 + KM)
      else:
        out[:, sl] = ((3 + 2*KM)*u*np.einsum('bji,bjk->bik', absm, mats[j][1])).reshape(B, 9)
    else:
      s = [n for n, _ in codegen.SOCCER_ARENA].index(name)
      f = (s + (4 if p >= num_players//2 else 0)) % 8
      feature = box['features'][f][:extent]
      out[:, sl] = (ego(feature[None] - pos[:, :extent], absm, 1 + extent + KM) +
                    ego(np.broadcast_to(feature, (B, extent)), absm, 1))
  return out


def compare(got_row, got_reward, pitch, num_players, extents, qpos, qvel, prev_action, real,
            label=''):
  """Asserts a device (or shim) row [B, NOBS] and reward [B] against the host path
  on the state (qpos, qvel) it was computed from; prints and returns the largest
  |device - host| / bound."""
  want, reward = host_row(pitch, num_players, extents, qpos, qvel, prev_action)
  bound = bounds(pitch, num_players, extents, qpos, qvel, real)
  got_row = np.asarray(got_row, np.float64)
  assert got_row.shape == want.shape
  exact = bound == 0
  layout = codegen.soccer_observation_layout(num_players, extents)
  names = np.empty(want.shape[1], object)
  for key, (offset, extent) in layout.items():
    names[offset:offset + extent] = '%s' % (key,)
  bad = exact & (got_row != want)
  assert not bad.any(), ('exact words differ', sorted(set(names[bad.any(axis=0)])))
  err = np.abs(got_row - want)
  ratio = np.where(exact, 0.0, err/np.where(exact, 1.0, bound))
  worst = np.unravel_index(ratio.argmax(), ratio.shape)
  print('%s largest |device - host| / bound: %.3f at %s (env %d)'
        % (label, ratio.max(), names[worst[1]], worst[0]))
  assert ratio.max() <= 2.0, (names[worst[1]], int(worst[0]), float(ratio.max()))
  np.testing.assert_array_equal(np.asarray(got_reward, np.float64), reward)
  return float(ratio.max())


def seeded_states(model, num_players, extents, n, seed, pitch, airborne=True):
  """[n] states: random root places inside the field, headings, tilts and joint
  angles, random velocities, the ball in the air."""
  rs = np.random.RandomState(seed)
  nq, nv, _ = extents
  qpos = np.tile(np.asarray(model.qpos0, np.float64), (n, 1))
  qvel = 0.5*rs.randn(n, model.nv)
  span = np.asarray(pitch.size)*0.5
  for k in range(num_players + 1):
    a = nq*k
    qpos[:, a:a + 2] = rs.uniform(-span, span, size=(n, 2))
    quat = rs.randn(n, 4)*[1.0, 0.25, 0.25, 1.0]       # any heading, a moderate tilt
    qpos[:, a + 3:a + 7] = quat/np.linalg.norm(quat, axis=1, keepdims=True)
    if k < num_players:
      qpos[:, a + 2] = 1.3 + 0.2*rs.rand(n)
      qpos[:, a + 7:a + nq] += 0.2*rs.randn(n, nq - 7)
  qpos[:, nq*num_players + 2] = (1.5 + rs.rand(n)) if airborne else 0.5
  return qpos, qvel
