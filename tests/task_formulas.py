"""Host restatement of the suite tasks' reward formulas.

Test infrastructure: validated against tests/golden/tasks.json (outputs of the
reference's own `get_reward` on canned readings) in test_host_logic.py, then
used by the GPU tests to check the device-fused rewards from read-back physics
quantities, and by tests/output_model.py as the reward path of the host model
of the output stage.  Formulas: suite/cartpole.py:204-225, suite/cheetah.py:87-93,
suite/humanoid.py:183-207 of the reference.

Every function takes scalars (one env) or arrays with the env on the leading
axis, and computes in the dtype of its array inputs (float64 for scalars and
lists), so that the same formulas run in float32 are an fp32 reference.
`tolerance` is `dm_control_amd.utils.rewards.tolerance` for the three sigmoids
the tasks use, dtype-honouring (tests/test_output_model.py compares the two on
tests/golden/rewards.json); inside `recording()` it also notes every term's
input and branch.
"""

import contextlib

import numpy as np

_recorded = None


@contextlib.contextmanager
def recording():
  """Inside, every `tolerance` call appends (name, x, branch, bounds, margin, sigmoid):
  branch 0 in bounds, 1 on the slope, 2 on the floor (past the cut-off of the
  linear / quadratic sigmoid, or out of bounds with margin 0)."""
  global _recorded
  before, _recorded = _recorded, []
  try:
    yield _recorded
  finally:
    _recorded = before


def _array(x):
  x = np.asarray(x)
  return x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)


def tolerance(x, bounds=(0.0, 0.0), margin=0.0, sigmoid='gaussian', value_at_margin=0.1,
              name=None):
  x = _array(x)
  dt = x.dtype.type
  lower, upper, margin = dt(bounds[0]), dt(bounds[1]), dt(margin)
  assert lower <= upper and margin >= 0
  in_bounds = np.logical_and(lower <= x, x <= upper)
  if margin == 0:
    value = np.where(in_bounds, dt(1), dt(0))
    branch = np.where(in_bounds, 0, 2)
  else:
    d = np.where(x < lower, lower - x, x - upper)/margin
    if sigmoid == 'gaussian':
      scale = np.sqrt(dt(-2)*np.log(dt(value_at_margin)))
      sig, floor = np.exp(dt(-0.5)*(d*scale)**2), np.zeros(x.shape, bool)
    elif sigmoid == 'linear':
      sx = d*(dt(1) - dt(value_at_margin))
      floor = ~(abs(sx) < 1)
      sig = np.where(floor, dt(0), dt(1) - sx)
    elif sigmoid == 'quadratic':
      sx = d*np.sqrt(dt(1) - dt(value_at_margin))
      floor = ~(abs(sx) < 1)
      sig = np.where(floor, dt(0), dt(1) - sx**2)
    else:
      raise ValueError('no suite task uses sigmoid %r' % (sigmoid,))
    value = np.where(in_bounds, dt(1), sig)
    branch = np.where(in_bounds, 0, np.where(floor, 2, 1))
  if _recorded is not None:
    _recorded.append((name, x, branch, (float(bounds[0]), float(bounds[1])), float(margin),
                      sigmoid))
  assert value.dtype == x.dtype
  return value


def _c(x, value):
  """The constant `value` in the dtype of x."""
  return x.dtype.type(value)


def cartpole_reward(x, cos, ctrl, angular_vel, sparse):
  """x, ctrl: per env; cos [..., npole]; angular_vel [..., npole]."""
  x = _array(x)
  cos = _array(cos).astype(x.dtype)
  if cos.ndim == x.ndim:
    cos = cos[..., None]
  if sparse:
    return (tolerance(x, (-.25, .25), name='cart') *
            tolerance(cos, (.995, 1), name='pole_cos').prod(axis=-1))
  ctrl, angular_vel = _array(ctrl).astype(x.dtype), _array(angular_vel).astype(x.dtype)
  if ctrl.ndim > x.ndim:
    ctrl = ctrl[..., 0]
  if angular_vel.ndim == x.ndim:
    angular_vel = angular_vel[..., None]
  upright = (cos + _c(x, 1))/_c(x, 2)
  centered = (_c(x, 1) + tolerance(x, margin=2, name='centered'))/_c(x, 2)
  small_control = tolerance(ctrl, margin=1, value_at_margin=0, sigmoid='quadratic',
                            name='small_control')
  small_control = (_c(x, 4) + small_control)/_c(x, 5)
  small_velocity = tolerance(angular_vel, margin=5, name='small_velocity').min(axis=-1)
  small_velocity = (_c(x, 1) + small_velocity)/_c(x, 2)
  return upright.mean(axis=-1, dtype=x.dtype)*small_control*small_velocity*centered


def cheetah_reward(speed):
  return tolerance(speed, bounds=(10, float('inf')), margin=10,
                   value_at_margin=0, sigmoid='linear', name='speed')


def humanoid_reward(head_height, torso_upright, ctrl, com_velocity, move_speed):
  head_height = _array(head_height)
  dt = head_height.dtype
  standing = tolerance(head_height, bounds=(1.4, float('inf')), margin=1.4/4,
                       name='standing')
  upright = tolerance(_array(torso_upright).astype(dt), bounds=(0.9, float('inf')),
                      sigmoid='linear', margin=1.9, value_at_margin=0, name='upright')
  stand_reward = standing*upright
  small_control = tolerance(_array(ctrl).astype(dt), margin=1, value_at_margin=0,
                            sigmoid='quadratic', name='small_control').mean(axis=-1, dtype=dt)
  small_control = (_c(standing, 4) + small_control)/_c(standing, 5)
  com_velocity = _array(com_velocity).astype(dt)
  if move_speed == 0:
    dont_move = tolerance(com_velocity[..., :2], margin=2,
                          name='dont_move').mean(axis=-1, dtype=dt)
    return small_control*stand_reward*dont_move
  speed = np.sqrt(com_velocity[..., 0]**2 + com_velocity[..., 1]**2)
  move = tolerance(speed, bounds=(move_speed, float('inf')), margin=move_speed,
                   value_at_margin=0, sigmoid='linear', name='move')
  move = (_c(standing, 5)*move + _c(standing, 1))/_c(standing, 6)
  return small_control*stand_reward*move


def walker_reward(torso_height, torso_upright, horizontal_velocity, move_speed):
  """suite/walker.py:144-160."""
  torso_height = _array(torso_height)
  dt = torso_height.dtype
  one = _c(torso_height, 1)
  standing = tolerance(torso_height, bounds=(1.2, float('inf')), margin=1.2/2,
                       name='standing')
  upright = (one + _array(torso_upright).astype(dt))/_c(standing, 2)
  stand_reward = (_c(standing, 3)*standing + upright)/_c(standing, 4)
  if move_speed == 0:
    return stand_reward
  move = tolerance(_array(horizontal_velocity).astype(dt),
                   bounds=(move_speed, float('inf')),
                   margin=move_speed/2, value_at_margin=0.5,
                   sigmoid='linear', name='move')
  return stand_reward*(_c(standing, 5)*move + one)/_c(standing, 6)


def pendulum_reward(pole_vertical):
  """suite/pendulum.py:119-120."""
  return tolerance(pole_vertical, (np.cos(np.deg2rad(8)), 1), name='pole_vertical')


def acrobot_reward(to_target, sparse, target_radius=0.2):
  """suite/acrobot.py:116-126."""
  return tolerance(to_target, bounds=(0, target_radius),
                   margin=0 if sparse else 1, name='to_target')


def hopper_reward(height, speed, ctrl, hopping):
  """suite/hopper.py:124-140."""
  height = _array(height)
  dt = height.dtype
  standing = tolerance(height, (0.6, 2), name='height')
  if hopping:
    return standing*tolerance(_array(speed).astype(dt), bounds=(2, float('inf')), margin=1,
                              value_at_margin=0.5, sigmoid='linear', name='hopping')
  small_control = tolerance(_array(ctrl).astype(dt), margin=1, value_at_margin=0,
                            sigmoid='quadratic', name='small_control').mean(axis=-1, dtype=dt)
  return standing*(small_control + _c(standing, 4))/_c(standing, 5)


def reacher_reward(finger_to_target_dist, target_size, finger_size=0.01):
  """suite/reacher.py:118-120."""
  return tolerance(finger_to_target_dist, (0, target_size + finger_size),
                   name='finger_to_target')


def point_mass_reward(mass_to_target_dist, ctrl, target_size=0.015):
  """suite/point_mass.py:122-130."""
  near = tolerance(mass_to_target_dist, bounds=(0, target_size),
                   margin=target_size, name='near')
  dt = near.dtype
  control_reward = tolerance(_array(ctrl).astype(dt), margin=1, value_at_margin=0,
                             sigmoid='quadratic', name='small_control').mean(axis=-1, dtype=dt)
  return near*(control_reward + _c(near, 4))/_c(near, 5)
