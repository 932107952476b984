"""Every code object the product can select, on the device.

tests/selection_matrix.py lists what `Physics` picks from (domain, precision,
batch size); tests/test_selection.py keeps that list equal to the policy.
Here every line of it
  * is built with exactly the line's arguments (never under the spill-budget
    override) and compared per control step with the fp64 oracle, teacher-
    forced, under the project's existing bounds (fp64 1e-9; f32 and mixed the
    per-model `helpers.FP32_PER_STEP`), with a partial last workgroup;
  * is selected through `suite.load` at the batch sizes that select it, where
    the same 64 states tiled over the whole batch must give bit-identical
    replicas, identical to those 64 envs run alone on the same code object.
The 8 and 16 lanes-per-env builds, reachable through the public `group`
keyword only, get the same per-step comparison or a pinned refusal.
"""

import os

import numpy as np
import pytest

import helpers
import selection_matrix as sm
from dm_control_amd import build
from dm_control_amd import suite
from dm_control_amd import wrapper

pytestmark = pytest.mark.gpu

W = wrapper

# physics steps per control step, as in test_fp64_build_matches_oracle_per_step
NSUB = {'cartpole': 1, 'cheetah': 1, 'humanoid': 5, 'walker': 10, 'pendulum': 1,
        'acrobot': 1, 'hopper': 4, 'reacher': 1, 'point_mass': 1}
# 129 envs: two full wavefronts of the one-lane kernel and one lane of a third;
# odd, so the two-envs-per-wave build ends on a half-filled wave too
PARITY_NENV, PARITY_STEPS = 129, 12
# `helpers._degenerate` may leave out at most this share of a run's samples
# (with these seeds the oracle alone drops none in any of the nine domains)
MAX_EXCLUDED = 0.01


def _per_step(name, precision, nenv, steps, what, **kwargs):
  assert os.environ.get('DMC_ALLOW_OVERBUDGET') != '1'
  e = helpers._teacher_forced(name, precision, nenv=nenv, steps=steps,    # pylint: disable=protected-access
                              nsub=NSUB[name], **kwargs)
  assert len(e) >= (1 - MAX_EXCLUDED)*nenv*steps, (len(e), nenv*steps)
  if precision == 'f64':
    print('OBSERVED fp64 per-step %s: max %.2e' % (what, e.max()))
    assert e.max() <= 1e-9, e.max()
  else:
    print('OBSERVED %s per-step %s: median %.2e p99 %.2e max %.2e'
          % (precision, what, np.median(e), np.percentile(e, 99), e.max()))
    helpers._assert_fp32_per_step(name, e)    # pylint: disable=protected-access


@pytest.mark.parametrize('line', sm.SHIPPED, ids=sm.line_id)
def test_shipped_code_object_matches_oracle_per_step(line):
  domain, precision, mode, group, lds_budget, _, _ = line
  if mode == sm.REFUSED:
    with pytest.raises(ValueError, match='one-env-per-lane'):
      build.build_model(helpers.load_model(domain), helpers.TASKS[domain],
                        precision, mode=helpers.MODES[domain])
    return
  _per_step(domain, precision, PARITY_NENV, PARITY_STEPS, sm.line_id(line),
            mode=mode, lds_budget=lds_budget, group=group or 64)


def _shape_name(mode, group):
  if mode != 'coop':
    return 'one env per lane (csrc/dmc_kernels.hip)'
  if group == 128:
    return '64 lanes per env + a second wavefront'
  return '%d lanes per env (csrc/dmc_coop.hip)' % group


def _flat(observation):
  return np.concatenate([np.asarray(observation[k], np.float64).reshape(
      len(observation[k]), -1) for k in sorted(observation)], axis=1)


def _run_tiled(env, qpos, qvel, taskdata, actions, index):
  """Resets `env`, gives env i the state / task data / actions of sample
  index[i], takes len(actions) control steps.  -> per step (qpos, qvel, fused
  observation, fused reward) as stored on the device, plus the TimeStep's
  observation and reward."""
  env.reset()
  physics = env.physics
  batch = physics.batch
  n = len(index)
  if taskdata is not None:
    batch.write(W.FIELD_TASKDATA, taskdata[:, index])
  physics.set_state(np.hstack([qpos[index], qvel[index]]))
  batch.set_state(warmstart=np.zeros((max(physics.model.nv, 1), n)), time=np.zeros(n))
  out = []
  for a in actions:
    ts = env.step(a[index])
    assert not ts.last()
    out.append((batch.read(W.FIELD_QPOS), batch.read(W.FIELD_QVEL),
                batch.read(W.FIELD_OBS).T, batch.read(W.FIELD_REWARD)[None],
                _flat(ts.observation).T, np.asarray(ts.reward)[None]))
  assert not batch.read(W.FIELD_WARN).any()
  return out


# (the episodes start with the device-side reset: drawing 65536 start states on
# the host costs seconds per batch, and the states are overwritten anyway)
TILE, TILE_STEPS = 64, 6


@pytest.mark.parametrize('line', sm.SHIPPED, ids=sm.line_id)
def test_policy_selects_the_line_and_envs_are_independent(line, monkeypatch):
  domain, precision, mode, group, lds_budget, lo_batch, hi_batch = line
  task = sm.first_task(domain)
  if mode == sm.REFUSED:
    for b in (1, 8192):
      with pytest.raises(ValueError, match='one-env-per-lane'):
        suite.load(domain, task, task_kwargs={'random': 1},
                   environment_kwargs={'batch_size': b, 'precision': precision})
    return
  assert os.environ.get('DMC_ALLOW_OVERBUDGET') != '1'
  model = helpers.load_model(domain)
  path = build.build_model(model, helpers.TASKS[domain], **sm.build_args(line))
  if hi_batch is None:    # a domain with one shape at every size: 8192 will do
    hi_batch = 8192 if lo_batch == 1 else 65536
  qpos, qvel = helpers.initial_states(model, domain, TILE, seed=7)
  actions = np.random.RandomState(11).uniform(-1, 1, (TILE_STEPS, TILE, model.nu))

  # the 64 envs alone, on the same code object: the policy would pick another
  # shape for 64 envs, so mode / group are given and the LDS budget is the line's
  with monkeypatch.context() as mp:
    mp.setattr(build, 'lds_budget_for', lambda nenv: lds_budget)
    alone = suite.load(domain, task, task_kwargs={'random': 1}, environment_kwargs={
        'batch_size': TILE, 'precision': precision, 'build_mode': mode,
        'group': group or 64, 'device_init': True})
  assert alone.physics.code_object == path
  alone.reset()
  info = alone.physics.batch.model.info
  taskdata = (alone.physics.batch.read(W.FIELD_TASKDATA) if info.ntaskdata > 0
              else None)
  want = _run_tiled(alone, qpos, qvel, taskdata, actions, np.arange(TILE))
  alone.physics.free()

  for b in sorted({lo_batch, hi_batch}):
    env = suite.load(domain, task, task_kwargs={'random': 1},
                     environment_kwargs={'batch_size': b, 'precision': precision,
                                         'device_init': True})
    physics = env.physics
    assert physics.code_object == path, (b, physics.kernel_shape)
    assert physics.kernel_shape.startswith(_shape_name(mode, group)), physics.kernel_shape
    index = np.arange(b) % TILE
    got = _run_tiled(env, qpos, qvel, taskdata, actions, index)
    physics.free()
    for t in range(TILE_STEPS):
      for k, (g, w) in enumerate(zip(got[t], want[t])):
        # [k][env]: every replica equals the sample run alone, bit for bit
        # (and hence replica 0)
        bits = 'u%d' % g.dtype.itemsize
        same = (np.ascontiguousarray(g).view(bits)
                == np.ascontiguousarray(w[:, index]).view(bits)).all(axis=0)
        assert same.all(), (
            'batch %d step %d field %d: %d envs differ from the 64 run alone, first %s'
            % (b, t, k, (~same).sum(), np.nonzero(~same)[0][:8]))


@pytest.mark.parametrize('nenv', [61, 67])
@pytest.mark.parametrize('domain,group,precision', sm.SMALL_GROUPS)
def test_eight_and_sixteen_lanes_per_env(domain, group, precision, nenv):
  """`group` 8 / 16 (eight / four envs per wavefront), reachable through
  `environment_kwargs={'build_mode': 'coop', 'group': ...}`: the same per-step
  comparison and bounds as the shipped shapes, batch sizes that are no multiple
  of the envs per wavefront -- or the pinned refusal."""
  if (domain, group, precision) in sm.SMALL_GROUPS_REFUSED:
    with pytest.raises(ValueError, match='do not fit in LDS'):
      build.build_model(helpers.load_model(domain), helpers.TASKS[domain],
                        precision, mode='coop', group=group)
    return
  _per_step(domain, precision, nenv, 10, '%s-%s-g%d x%d' % (domain, precision, group, nenv),
            mode='coop', group=group)
