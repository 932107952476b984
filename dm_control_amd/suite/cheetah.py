"""Cheetah domain (cf. /root/reference/dm_control/suite/cheetah.py)."""

import numpy as np

from dm_control_amd import codegen
from dm_control_amd import engine
from dm_control_amd.rl import control
from dm_control_amd.suite import base
from dm_control_amd.suite import common
from dm_control_amd.utils import containers

_DEFAULT_TIME_LIMIT = 10
_RUN_SPEED = 10   # fused on the device: tolerance(speed, (10, inf), margin 10)
_SETTLE_STEPS = 200
# The episode prefetch runs where it was measured to pay: on the one-env-per-lane
# kernel with up to this many workgroups (8192 envs), whose step launches leave half
# of the chip's 256 compute units empty.  On a full chip (16384 envs) a step beside
# the settle launch takes twice as long and whole episodes came out 0.7 % slower;
# the several-lanes kernels of small batches were not measured.
_PREFETCH_MAX_WORKGROUPS = 128

SUITE = containers.TaggedTasks()


def get_model_and_assets():
  return common.read_model('cheetah.xml'), common.ASSETS


@SUITE.add('benchmarking')
def run(time_limit=_DEFAULT_TIME_LIMIT, random=None, environment_kwargs=None):
  """Returns the run task (cheetah.py:42-49)."""
  phys_kw, task_kw, env_kw = common.split_kwargs(environment_kwargs)
  physics = Physics.from_xml_string(*get_model_and_assets(), **phys_kw)
  task = Cheetah(random=random, **task_kw)
  return control.Environment(physics, task, time_limit=time_limit, **env_kw)


class Physics(engine.Physics):

  _TASK = codegen.TASK_CHEETAH
  # one env per wavefront up to 2048 envs (measured cross-over)
  _COOP_POLICY = ((1024, 128), (2048, 64))
  _COOP_POLICY_F64 = ((4096, 128),)

  def speed(self):
    """Horizontal speed of the Cheetah (cheetah.py:55-57)."""
    return self.named.data.sensordata['torso_subtreelinvel'][..., 0]


class Cheetah(base.Task):
  """Running task (cheetah.py:60-93)."""

  # Device-init path, whole-batch resets: the start of the NEXT episode (reset,
  # draw, settle steps) is computed on a side stream while this one steps, and
  # taken over at the next reset (`HipBatch.episode_prefetch`; DESIGN.md 5, "Reset
  # prefetch").  Same bits either way; False: every reset runs its own launches.
  prefetch = True

  def initialize_episode(self, physics):
    m = physics.model
    assert m.nq == m.njnt
    # Stabilize the model before the actual simulation: 200 physics steps in
    # one launch, no observation/reward work (cheetah.py:72-73).  The reference
    # takes them right after overwriting qpos, without a forward pass, so its
    # first mj_step2 still works on the mass matrix, bias and contacts that
    # reset_context computed at qpos0: `stale_first`.
    if self._device_init:
      batch = physics.batch
      seed = self.device_seed()
      # The episode starts at time 0: stored by the settle launch itself, so that
      # under the env mask of `reset_done` the other envs keep their clocks.
      settle = dict(stale_first=True, zero_time=True)
      # (a masked pass of `reset_done`, or per-env episodes: not a whole-batch start)
      info = batch.model.info
      whole = (self.prefetch and not batch.is_masked and not batch.episodes and
               info.lanes_per_env == 1 and
               batch.nenv <= _PREFETCH_MAX_WORKGROUPS*info.envs_per_block)
      if not (whole and physics.take_prefetched_episode(seed, _SETTLE_STEPS, **settle)):
        batch.init_episode(seed)
        physics.step(_SETTLE_STEPS, outputs=False, check=False, **settle)
      physics.check_invalid_state()
      super().initialize_episode(physics)
      if whole:
        # the seed the next reset draws, unless somebody uses `self.random` before
        # it; then the seeds differ and that reset runs its own launches
        batch.episode_prefetch(self.next_device_seed(), _SETTLE_STEPS,
                               after_steps=self.prefetch_after_steps(batch.control_steps),
                               **settle)
      return
    is_limited = m.jnt_limited == 1
    lower, upper = m.jnt_range[is_limited].T
    rows = []
    for rs in self.streams(physics):
      qpos = m.qpos0.copy()
      qpos[is_limited] = rs.uniform(lower, upper)
      rows.append(qpos)
    qpos = np.array(rows)
    physics.data.qpos[:] = qpos[0] if physics.batch_size is None else qpos
    physics.step(_SETTLE_STEPS, outputs=False, stale_first=True)
    physics.data.time = 0
    super().initialize_episode(physics)

  def get_observation(self, physics):
    m = physics.model
    return self._obs_dict(physics, [('position', m.nq - 1, False),
                                    ('velocity', m.nv, False)])
