"""Host side of the episode prefetch (suite/base.py): the look-ahead of the
device seed and the firing rule's arithmetic.  No device involved; the device
side is tests/test_gpu_episode_prefetch.py."""

import numpy as np

from dm_control_amd.suite import cheetah


def _same_state(a, b):
  return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_look_ahead_leaves_the_stream_alone():
  task = cheetah.Cheetah(random=7, device_init=True)
  before = task.random.get_state()
  for _ in range(3):
    task.next_device_seed()
  assert _same_state(task.random.get_state(), before)
  assert task._episode == 0                       # pylint: disable=protected-access
  # ... and the stream then gives what it would have given
  twin = cheetah.Cheetah(random=7)
  assert task.random.randint(0, 2**31 - 1) == twin.random.randint(0, 2**31 - 1)


def test_look_ahead_predicts_the_next_seed_over_several_episodes():
  task = cheetah.Cheetah(random=11, device_init=True)
  seeds = []
  for _ in range(6):
    ahead = task.next_device_seed()
    assert task.next_device_seed() == ahead       # (asking twice changes nothing)
    seed = task.device_seed()
    assert seed == ahead
    seeds.append(seed)
  assert len(set(seeds)) == 6
  assert [s & (2**20 - 1) for s in seeds] == [1, 2, 3, 4, 5, 6]   # the episode number


def test_a_draw_in_between_makes_the_seeds_differ():
  task = cheetah.Cheetah(random=11, device_init=True)
  ahead = task.next_device_seed()
  task.random.uniform()
  assert task.device_seed() != ahead


def test_after_steps_is_half_the_last_episode():
  task = cheetah.Cheetah(random=0)
  assert task.prefetch_after_steps(0) == 0        # first reset: nothing to go by
  assert task.prefetch_after_steps(1000) == 500   # bench.py: 50 warm-up + 950 timed steps
  assert task.prefetch_after_steps(1007) == 3     # (rounded down)
  assert task.prefetch_after_steps(1007) == 0     # a reset right after a reset
  assert task.prefetch_after_steps(1008) == 0
  # a task handed another batch, whose count starts again: never negative
  assert task.prefetch_after_steps(5) == 0
  assert task.prefetch_after_steps(25) == 10
