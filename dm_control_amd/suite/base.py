"""Base class of the suite tasks (cf. /root/reference/dm_control/suite/base.py).

Actions map directly to actuator controls (base.py:73-77).  Observation and
reward are produced by the step kernel; the task classes only slice the fused
vector into the reference's OrderedDict layout.  Initial states follow each
domain's `initialize_episode` recipe either on the host (numpy RandomState,
same call order as the reference, one stream per instance) or on the device
(`device_init=True`, counter-based RNG; same distributions).
"""

import numpy as np

from dm_control_amd import engine
from dm_control_amd import wrapper
from dm_control_amd.rl import control


class Task(control.Task):
  """Control Suite task over a batched Physics."""

  def __init__(self, random=None, device_init=False):
    if not isinstance(random, np.random.RandomState):
      random = np.random.RandomState(random)
    self._random = random
    self._visualize_reward = False
    self._device_init = bool(device_init)
    self._episode = 0
    self._streams = None
    self._reset_at = None     # control steps the batch had issued at the last reset

  @property
  def random(self):
    return self._random

  def streams(self, physics):
    """One RandomState per instance (instance 0 = `self.random`)."""
    n = physics.batch_size
    if n is None:
      return [self._random]
    if self._streams is None or len(self._streams) != n:
      # seeds for instances 1.. come from a COPY of stream 0, so instance 0
      # draws exactly what the reference's single env would draw
      fork = np.random.RandomState()
      fork.set_state(self._random.get_state())
      seeds = fork.randint(0, 2**31 - 1, size=n - 1) if n > 1 else []
      self._streams = [self._random] + [np.random.RandomState(int(s))
                                        for s in seeds]
    return self._streams

  def device_seed(self):
    self._episode += 1
    base = int(self._random.randint(0, 2**31 - 1))
    return (base << 20) + self._episode

  def next_device_seed(self):
    """What the next `device_seed()` returns if nobody draws from `self.random`
    before it: drawn from a copy of the stream, which is left as it is."""
    fork = np.random.RandomState()
    fork.set_state(self._random.get_state())
    return (int(fork.randint(0, 2**31 - 1)) << 20) + self._episode + 1

  def prefetch_after_steps(self, control_steps):
    """`after_steps` of the prefetch started at a reset: half the control steps
    issued between the last two resets, so that the prefetch is neither still
    running when the caller synchronises right after a reset nor late for the next
    one; 0 (at once) before there are two.  control_steps: the batch's count of
    issued control steps at this reset."""
    last, self._reset_at = self._reset_at, int(control_steps)
    return 0 if last is None else max(0, self._reset_at - last)//2

  def reset_done(self, physics, envs=None):
    """Starts a new episode in the envs that are done, and only there.

    Runs this task's `initialize_episode` recipe (device-init path) followed by
    `physics.after_reset()` with every launch under the env mask, so each env
    outside the mask keeps all of its fields bit for bit, and each env inside
    gets what a whole-batch `reset_context` + `initialize_episode` with the same
    seed would have given it (a draw depends on (seed, env) alone).

    envs: None -- the mask is the done word of every env, copied on the device
    (no host read; a pass over a batch where nobody is done launches kernels
    that find an empty mask and exit); else an index array or boolean mask."""
    if not self._device_init:
      raise ValueError('reset_done needs device_init=True: the host-RNG recipes '
                       'rewrite whole fields')
    if physics.batch_size is None:
      raise ValueError('reset_done needs a batched Physics')
    batch = physics.batch
    if envs is None:
      batch.set_masked(True)       # (allocates the block on first use)
      batch.mask_from_done()
      # with per-env episodes a warning bit is a done bit: every env that had
      # one is inside this mask, so after the pass no env has one
      physics._warn_seen[:] = 0    # pylint: disable=protected-access
      mask = None
    else:
      mask = np.zeros(batch.nenv, bool)
      mask[np.asarray(envs)] = True
      physics._warn_seen[mask] = 0   # pylint: disable=protected-access
    with batch.masked(mask):
      self.initialize_episode(physics)
      physics.after_reset()

  def selected_envs(self, physics):
    """Boolean [B]: the envs the current launches reach (all of them unless a
    `reset_done` pass is running; a device read)."""
    batch = physics.batch
    if not batch.is_masked:
      return np.ones(batch.nenv, bool)
    return batch.episode_read(wrapper.EPISODE_MASK) != 0

  def action_spec(self, physics):
    return engine.action_spec(physics)

  def initialize_episode(self, physics):
    self.after_step(physics)

  def before_step(self, action, physics):
    action = getattr(action, 'continuous_actions', action)
    physics.set_control(action)

  def after_step(self, physics):
    """Reward colouring is a rendering-only side effect (base.py:79-83)."""

  @property
  def visualize_reward(self):
    return self._visualize_reward

  @visualize_reward.setter
  def visualize_reward(self, value):
    if not isinstance(value, bool):
      raise ValueError('Expected a boolean, got {}.'.format(type(value)))
    self._visualize_reward = value

  def get_reward(self, physics):
    return physics.fused_reward()

  def _obs_dict(self, physics, fields):
    """Slices the fused [B, nobs] vector into named leaves."""
    vec = physics.fused_observation()
    obs = control.BatchedObservation()
    obs.batch_size = physics.batch_size
    start = 0
    for name, size, scalar in fields:
      leaf = vec[..., start:start + size]
      if scalar:
        leaf = leaf[..., 0]
      obs[name] = np.array(leaf, dtype=np.float64)
      start += size
    return obs
