"""Initial-state randomisers (cf. suite/utils/randomizers.py:35-86)."""

import numpy as np

from dm_control_amd import model_params
from dm_control_amd.mjcf import model as mdl


def randomize_limited_and_rotational_joints(model, qpos, random):
  """The reference's rules applied to a plain qpos vector, same draw order.

  Bounded hinges/sliders: uniform in range; unbounded hinges: uniform in
  [-pi, pi]; free joints: only the quaternion (normalised `rand(4)`); ball
  joints: normalised `randn(4)`.
  """
  for j in range(model.njnt):
    jtype = model.jnt_type[j]
    a = model.jnt_qposadr[j]
    lo, hi = model.jnt_range[j]
    if model.jnt_limited[j]:
      if jtype in (mdl.JNT_HINGE, mdl.JNT_SLIDE):
        qpos[a] = random.uniform(lo, hi)
    else:
      if jtype == mdl.JNT_HINGE:
        qpos[a] = random.uniform(-np.pi, np.pi)
      elif jtype == mdl.JNT_BALL:
        quat = random.randn(4)
        qpos[a:a + 4] = quat/np.linalg.norm(quat)
      elif jtype == mdl.JNT_FREE:
        quat = random.rand(4)
        qpos[a + 3:a + 7] = quat/np.linalg.norm(quat)


def randomized_qpos(task, physics):
  """[B, nq] initial positions, one RandomState stream per instance."""
  rows = []
  for rs in task.streams(physics):
    qpos = physics.model.qpos0.copy()
    randomize_limited_and_rotational_joints(physics.model, qpos, rs)
    rows.append(qpos)
  return np.array(rows)


def randomize_model_params(physics, random, scale=1.3, envs=None):
  """Domain randomisation: every field named in the `per_env` argument of
  `physics` is multiplied, per env and per entry, by a log-uniform factor in
  [1/scale, scale] of the compiled model's value (`scale`: one number, or
  {field: number}), then `mj_setConst` is re-done (`Physics.set_model_params`).
  `random`: a `numpy.random.RandomState`.  Gravity gets one factor per env, a
  body's three moments of inertia share one.  Returns {field: values written}."""
  nenv = physics.get_model_params('gravity').shape[0]
  written = {}
  for name in physics.per_env:
    s = float(scale.get(name, 1.0) if isinstance(scale, dict) else scale)
    if s < 1:
      raise ValueError('scale must be >= 1')
    nominal = model_params._model_value(physics.model, name)[None]    # pylint: disable=protected-access
    shape = (nenv,) + nominal.shape[1:]
    if name == 'gravity':
      shape = (nenv, 1)
    elif name == 'body_inertia':
      shape = (nenv, nominal.shape[1], 1)
    written[name] = nominal*np.exp(random.uniform(-np.log(s), np.log(s), shape))
  if envs is not None:
    sel = np.arange(nenv)[envs]
    written = {k: v[sel] for k, v in written.items()}
  physics.set_model_params(envs=envs, **written)
  return written
