"""Sequence launches: `dmc_batch_step_n` on a code object that steps a whole
action sequence in one launch of the one-env-per-lane kernel (state, warm start
and episode return stay in registers, only the last step's outputs are written)
against the same number of `dmc_batch_step` calls on a twin batch.  Every
comparison is bitwise.
"""

import numpy as np
import pytest
import torch

import helpers
from dm_control_amd import codegen
from dm_control_amd import wrapper

pytestmark = pytest.mark.gpu

W = wrapper
_device_batch = helpers._device_batch     # pylint: disable=protected-access

FIELDS = (('qpos', W.FIELD_QPOS), ('qvel', W.FIELD_QVEL), ('warmstart', W.FIELD_WARMSTART),
          ('time', W.FIELD_TIME), ('obs', W.FIELD_OBS), ('reward', W.FIELD_REWARD),
          ('episode_return', W.FIELD_RETURN), ('stats', W.FIELD_STATS), ('warn', W.FIELD_WARN),
          ('ctrl', W.FIELD_CTRL), ('sensordata', W.FIELD_SENSORDATA))


def _actions(nsteps, nenv, nu, dtype, seed):
  gen = torch.Generator(device='cuda')
  gen.manual_seed(seed)
  return torch.rand(nsteps, nenv, nu, device='cuda', dtype=dtype, generator=gen)*2 - 1


def _run(name, precision, nenv, acts, nsteps, nsub, sequence, stride_t=None, mode='auto',
         group=64, seq_launch=1, seed=4):
  """All fields after `nsteps` control steps from seeded initial states: one
  `step_device_n` call (`sequence`) or `nsteps` `step_device` calls."""
  model = helpers.load_model(name)
  hm, hb = _device_batch(model, helpers.TASKS[name], precision, nenv, mode, group=group)
  assert hm.info.seq_launch == seq_launch
  qpos, qvel = helpers.initial_states(model, name, nenv, seed=seed)
  hb.set_state(qpos.T, qvel.T)
  nu = model.nu
  if stride_t is None:
    stride_t = nenv*nu
  if sequence:
    hb.step_device_n(acts.data_ptr(), 1, nu, stride_t, nsteps, nsub)
  else:
    for t in range(nsteps):
      hb.step_device(acts.data_ptr() + t*stride_t*acts.element_size(), 1, nu, nsub)
  out = {field: hb.read(fid) for field, fid in FIELDS}
  hb.free()
  hm.free()
  return out


def _assert_same(a, b, envs=None):
  for field, _ in FIELDS:
    x, y = a[field], b[field]
    if envs is not None:
      x, y = (x[envs], y[envs]) if field == 'obs' else (x[..., envs], y[..., envs])
    np.testing.assert_array_equal(x, y, err_msg=field)


@pytest.mark.parametrize('nsteps', [5, 1])
def test_cheetah_sequence_equals_single_steps(nsteps):
  """130 envs: two full workgroups and a 2-env tail."""
  acts = _actions(5, 130, 6, torch.float32, 0)
  seq = _run('cheetah', 'f32', 130, acts, nsteps, 1, True)
  one = _run('cheetah', 'f32', 130, acts, nsteps, 1, False)
  assert seq['stats'][0].max() > 0          # (contacts: the solver ran)
  _assert_same(seq, one)


def test_action_repeat_equals_single_steps_with_the_same_action():
  acts = _actions(1, 130, 6, torch.float32, 1)
  seq = _run('cheetah', 'f32', 130, acts, 4, 1, True, stride_t=0)
  one = _run('cheetah', 'f32', 130, acts, 4, 1, False, stride_t=0)
  _assert_same(seq, one)


def test_hopper_substeps_and_touch_sensors():
  """nsub=4 inside every control step of the sequence; touch sensors in the observation."""
  acts = _actions(3, 70, 4, torch.float32, 2)
  seq = _run('hopper', 'f32', 70, acts, 3, 4, True)
  one = _run('hopper', 'f32', 70, acts, 3, 4, False)
  assert seq['stats'][0].max() > 0
  _assert_same(seq, one)


@pytest.mark.parametrize('name,precision', [('cartpole', 'f64'), ('cheetah', 'mixed')])
def test_sequence_longer_than_one_chunk(name, precision):
  """70 steps: two launches (64 + 6 control steps)."""
  nu = {'cartpole': 1, 'cheetah': 6}[name]
  acts = _actions(70, 66, nu, torch.float64 if precision == 'f64' else torch.float32, 3)
  seq = _run(name, precision, 66, acts, 70, 1, True)
  one = _run(name, precision, 66, acts, 70, 1, False)
  _assert_same(seq, one)


def test_nan_control_in_the_middle_of_a_sequence():
  """One env is given a NaN control at step 3 of 5: it carries the bad-control
  warning bit and equals the single-step path; the others are untouched."""
  nenv, bad_env = 130, 77
  clean = _actions(5, nenv, 6, torch.float32, 5)
  acts = clean.clone()
  acts[2, bad_env, 3] = float('nan')
  seq = _run('cheetah', 'f32', nenv, acts, 5, 1, True)
  one = _run('cheetah', 'f32', nenv, acts, 5, 1, False)
  ref = _run('cheetah', 'f32', nenv, clean, 5, 1, True)
  _assert_same(seq, one)
  assert seq['warn'][bad_env] & 128                 # DMC_WARN_BADCTRL
  others = np.arange(nenv) != bad_env
  assert not (seq['warn'][others] & 128).any()
  _assert_same(seq, ref, envs=others)
  assert not np.array_equal(seq['qpos'][:, bad_env], ref['qpos'][:, bad_env])


def test_code_object_without_the_capability_takes_the_loop():
  """The several-lanes kernel does not loop over control steps: one launch per step."""
  acts = _actions(5, 61, 6, torch.float32, 6)
  kw = dict(mode='coop', group=64, seq_launch=0)
  seq = _run('cheetah', 'f32', 61, acts, 5, 1, True, **kw)
  one = _run('cheetah', 'f32', 61, acts, 5, 1, False, **kw)
  _assert_same(seq, one)


def test_timer_counts_control_steps():
  model = helpers.load_model('cheetah')
  hm, hb = _device_batch(model, codegen.TASK_CHEETAH, 'f32', 130)
  acts = _actions(5, 130, 6, torch.float32, 7)
  hb.timer_start()
  hb.step_device_n(acts.data_ptr(), 1, 6, 130*6, 5, 1)
  ms, count = hb.timer_stop()
  assert count == 5 and ms > 0
  hb.free()
  hm.free()
