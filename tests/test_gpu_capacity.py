"""The shipped code objects at contact capacity, on the device.

tests/test_capacity.py steps the kernel SOURCES at capacity on the host under
sanitizers; here the gfx950 code objects of `capacity_cases.GPU_BUILDS` (built
by `build.build_model(..., ncon_max=K)`) step the 129 envs of
tests/capacity_cases.py once, teacher-forced, next to the oracle with
`nconmax = K` ("at capacity"):
  * stats[0] and the warning word, per env, are the oracle's -- after
    `forward(count_contacts=True)` already, and after the step;
  * the state: fp64 <= 1e-9 (`helpers.rel_err`), fp32 / mixed within
    `helpers.FP32_PER_STEP` of the model, no env excluded;
  * the unsaturated envs are bit-identical to a twin batch whose saturated envs
    are airborne, and the launch repeated gives the same words.
The team build (one wavefront per env) steps two walkers and a ball at caps
far below, one below, at and one above the scene's contact count.
Not on the device: the humanoid with 128 lanes at K = 8 in fp64 and the
unrolled fp64 cheetah (beyond the spill budget: `build_model` refuses them, and
no over-budget build runs at capacity).
"""

import functools

import numpy as np
import pytest

import capacity_cases as cc
import helpers
from dm_control_amd import build
from dm_control_amd import wrapper as W

# every test its own time limit: a hung launch ends the test, not the session
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

_BUILD_IDS = ['%s-K%s-%s-%s' % (n, k or 'default', kw['precision'],
                                'g%d' % kw['group'] if 'group' in kw else kw['mode'])
              for n, k, kw in cc.GPU_BUILDS]


def _case(name, cap):
  """States of the case and the cap the code object runs with."""
  if cap is None:
    return cc.default_cap_states() + (cc.DEFAULT_CAP,)
  return cc.states(name) + (cap,)


@functools.lru_cache(maxsize=None)
def _reference(name, cap):
  """Per env, from the oracle capped at K, computed once: (ncon, warn, qpos,
  qvel after one step under the case's controls), and the controls."""
  model, qpos, qvel, _, K = _case(name, cap)
  ctrl = np.random.RandomState(11).uniform(-1, 1, (cc.NENV, model.nu))
  om = cc.oracle_model(model, K)
  out = [cc.expected(om, qpos[e], qvel[e], ctrl[e]) for e in range(cc.NENV)]
  ref = dict(ncon=np.array([o[0] for o in out]), nefc=np.array([o[1] for o in out]),
             warn=np.array([o[2] for o in out]), qpos=np.array([o[3] for o in out]),
             qvel=np.array([o[4] for o in out]), ctrl=ctrl)
  for a in ref.values():
    a.setflags(write=False)
  return ref


def _launch(hb, qpos, qvel, ctrl):
  """forward(count_contacts) and one control step from the state: every word
  the comparison reads."""
  hb.clear_warnings()
  hb.set_state(qpos.T, qvel.T, np.zeros_like(qvel.T), np.zeros(len(qpos)))
  hb.forward(count_contacts=True)
  out = dict(ncon0=hb.read(W.FIELD_STATS)[0].copy(), warn0=hb.read(W.FIELD_WARN).copy())
  hb.set_state(qpos.T, qvel.T, np.zeros_like(qvel.T), np.zeros(len(qpos)))
  hb.step_host(ctrl, 1)
  out.update(qpos=hb.read(W.FIELD_QPOS).T.copy(), qvel=hb.read(W.FIELD_QVEL).T.copy(),
             stats=hb.read(W.FIELD_STATS).copy(), warn=hb.read(W.FIELD_WARN).copy())
  return out


@functools.lru_cache(maxsize=None)
def _device(index):
  """The launch of GPU_BUILDS[index], its repeat and its twin, run once."""
  name, cap, kw = cc.GPU_BUILDS[index]
  model, qpos, qvel, count, K = _case(name, cap)
  ref = _reference(name, cap)
  hm = W.HipModel(build.build_model(model, helpers.TASKS[name], ncon_max=cap, **kw))
  assert hm.info.ncon_max == K
  hb = W.HipBatch(hm, cc.NENV)
  first = _launch(hb, qpos, qvel, ref['ctrl'])
  again = _launch(hb, qpos, qvel, ref['ctrl'])
  full = count > K
  airborne = int(np.flatnonzero(count == 0)[0])
  twin_q, twin_v = qpos.copy(), qvel.copy()
  twin_q[full], twin_v[full] = qpos[airborne], qvel[airborne]
  twin = _launch(hb, twin_q, twin_v, ref['ctrl'])
  hb.free()
  hm.free()
  return first, again, twin, full


@pytest.mark.parametrize('index', range(len(cc.GPU_BUILDS)), ids=_BUILD_IDS)
def test_code_object_at_contact_capacity_matches_the_capped_oracle(index):
  name, cap, kw = cc.GPU_BUILDS[index]
  _, _, _, count, K = _case(name, cap)
  ref = _reference(name, cap)
  first, again, twin, full = _device(index)
  assert full.sum() >= 4 and (~full).sum() >= 4
  # counts and warning bits: the oracle's, before any dynamics and after the step
  np.testing.assert_array_equal(first['ncon0'], np.minimum(count, K))
  np.testing.assert_array_equal(first['warn0'], np.where(full, cc.WARN_CONTACTFULL, 0))
  np.testing.assert_array_equal(first['stats'][0], ref['ncon'])
  np.testing.assert_array_equal(first['stats'][1], ref['nefc'])
  np.testing.assert_array_equal(first['warn'], ref['warn'])
  # the step: the capped oracle's
  err = np.maximum(helpers.rel_err(first['qpos'], ref['qpos']),
                   helpers.rel_err(first['qvel'], ref['qvel']))
  print('OBSERVED %s: per-step rel err median %.2e p99 %.2e max %.2e (env %d); saturated envs '
        'max %.2e, %d of %d envs saturated' % (
            _BUILD_IDS[index], np.median(err), np.percentile(err, 99), err.max(),
            int(err.argmax()), err[full].max(), full.sum(), cc.NENV))
  assert np.isfinite(first['qpos']).all() and np.isfinite(first['qvel']).all()
  if kw['precision'] == 'f64':
    assert err.max() <= 1e-9, (int(err.argmax()), err.max())
  else:
    helpers._assert_fp32_per_step(name, err)      # pylint: disable=protected-access
  # the launch repeated: the same words
  for key in first:
    np.testing.assert_array_equal(first[key], again[key], err_msg=key)
  # next to airborne envs instead of saturated ones: the same words
  for key in ('ncon0', 'warn0', 'warn'):
    np.testing.assert_array_equal(first[key][~full], twin[key][~full], err_msg=key)
    assert not twin[key][full].any()
  for key in ('qpos', 'qvel'):
    np.testing.assert_array_equal(first[key][~full], twin[key][~full], err_msg=key)
  np.testing.assert_array_equal(first['stats'][:, ~full], twin['stats'][:, ~full])


def test_default_cap_builds_are_what_physics_selects():
  """The humanoid lines of GPU_BUILDS without a cap: the shape and the capacity
  `suite.load` builds for a batch of NENV envs."""
  import selection_matrix
  from dm_control_amd import codegen
  picked = [kw for name, cap, kw in cc.GPU_BUILDS if name == 'humanoid' and cap is None]
  assert sorted(kw['precision'] for kw in picked) == ['f32', 'f64']
  for kw in picked:
    assert selection_matrix.select('humanoid', kw['precision'], cc.NENV) == (
        kw['mode'], kw['group'], None)
  model = helpers.load_model('humanoid')
  assert codegen.model_info(model, helpers.TASKS['humanoid'])['ncon_max'] == cc.DEFAULT_CAP


# ---------------------------------------------------------------------------
# team mode: one wavefront per env (what `locomotion.soccer` runs)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _team_envs():
  """Three envs: the scene, the scene lifted off the floor (the contacts among
  the walkers and the ball remain: fewer than the scene's), the scene."""
  m, q, v = cc.team_scene()
  lifted = q.copy()
  lifted[[2, 65, 128]] += 1.0         # both walkers' roots and the ball
  return m, np.array([q, lifted, q]), np.array([v, v, v])


@pytest.mark.parametrize('K', cc.TEAM_CAPS)
def test_team_code_object_at_contact_capacity_matches_the_capped_oracle(K):
  """`detect_contacts_team` on the device: slots from the prefix scan over the
  lanes, written only below NCON_MAX; contacts between the trees are among the
  dropped ones.  Exact counts and warning word, fp64 <= 1e-9, the launch
  repeated bit-identical; the env in the middle has fewer contacts.  At cap 5
  the capped step differs from the uncapped one by 17 in qvel, so a wrong kept
  set shows in the state; at n-1 the one dropped contact carries no force, and
  the count and the warning word are what tell.  (About
  ten seconds per cap, nearly all of it the load of a team code object and its
  workspace, as in the team tests of tests/test_soccer_model.py.)"""
  m, qpos, qvel = _team_envs()
  n = cc.TEAM_NCON
  ctrl = np.zeros((3, m.nu))
  om = cc.oracle_model(m, K)
  want = [cc.expected(om, qpos[e], qvel[e], ctrl[e]) for e in range(3)]
  assert cc.at(cc.oracle_model(m, 4*n), qpos[0], qvel[0]).ncon == n
  lifted = cc.at(cc.oracle_model(m, 4*n), qpos[1], qvel[1]).ncon
  assert 5 < lifted < n - 1       # full at the smallest cap only
  assert [w[0] for w in want] == [min(K, n), min(K, lifted), min(K, n)]
  assert [w[2] for w in want] == [cc.WARN_CONTACTFULL if K < c else 0 for c in (n, lifted, n)]
  hm = W.HipModel(build.build_model(m, 0, ncon_max=K, **cc.TEAM_BUILD))
  assert hm.info.ncon_max == K
  hb = W.HipBatch(hm, 3)
  first = _launch(hb, qpos, qvel, ctrl)
  again = _launch(hb, qpos, qvel, ctrl)
  hb.free()
  hm.free()
  np.testing.assert_array_equal(first['ncon0'], [w[0] for w in want])
  np.testing.assert_array_equal(first['warn0'], [w[2] for w in want])
  np.testing.assert_array_equal(first['stats'][0], [w[0] for w in want])
  np.testing.assert_array_equal(first['stats'][1], [w[1] for w in want])
  np.testing.assert_array_equal(first['warn'], [w[2] for w in want])
  err = np.maximum(helpers.rel_err(first['qpos'], np.array([w[3] for w in want])),
                   helpers.rel_err(first['qvel'], np.array([w[4] for w in want])))
  print('OBSERVED team-K%d-f64: per-step rel err max %.2e (%d of %d contacts kept)'
        % (K, err.max(), min(K, n), n))
  assert err.max() <= 1e-9, err
  for key in first:
    np.testing.assert_array_equal(first[key], again[key], err_msg=key)
  np.testing.assert_array_equal(first['qpos'][0], first['qpos'][2])


def test_code_objects_of_a_model_and_cap_count_the_same():
  groups = {}
  for index, (name, cap, _) in enumerate(cc.GPU_BUILDS):
    groups.setdefault((name, cap), []).append(index)
  assert any(len(g) > 1 for g in groups.values())
  for indices in groups.values():
    base = _device(indices[0])[0]
    for index in indices[1:]:
      other = _device(index)[0]
      for key in ('ncon0', 'warn0', 'warn'):
        np.testing.assert_array_equal(base[key], other[key], err_msg=_BUILD_IDS[index])
      np.testing.assert_array_equal(base['stats'][0], other['stats'][0])


# ---------------------------------------------------------------------------
# the runtime layer at capacity
# ---------------------------------------------------------------------------
def _saturating_batch(**env_kw):
  """cheetah-run with ncon_max = 4 on 129 envs of the one-env-per-lane kernel
  (a code object of GPU_BUILDS), at the case's states."""
  from dm_control_amd import suite
  env = suite.load('cheetah', 'run', task_kwargs={'random': 0}, environment_kwargs=dict(
      batch_size=cc.NENV, precision='f32', ncon_max=4, build_mode='auto', **env_kw))
  _, qpos, qvel, count = cc.states('cheetah')
  return env, qpos, qvel, count > 4


def test_physics_raises_contactfull_and_names_the_envs():
  from dm_control_amd.rl import control
  env, qpos, qvel, full = _saturating_batch()
  env.reset()
  physics = env.physics
  physics.batch.set_state(qpos.T, qvel.T)
  with pytest.raises(control.PhysicsError) as raised:
    physics.step()
    physics.check_invalid_state()
  message = str(raised.value)
  assert 'mjWARN_CONTACTFULL' in message
  assert str(np.flatnonzero(full)[:8].tolist()) in message
  np.testing.assert_array_equal(physics.batch.read(W.FIELD_WARN) & cc.WARN_CONTACTFULL != 0, full)
  physics.free()


def test_saturated_envs_are_done_frozen_and_come_back_clean():
  """`VecEnv(per_env_episodes=True)` on the ncon_max = 4 build: CONTACTFULL is
  `done` bit 1 and no error; the env stops where it is; `Task.reset_done`
  starts its next episode with the done word, the warning word, the step count
  and `Physics`' record of warnings seen all clear, so the next step reports
  nothing for it."""
  from dm_control_amd import vec_env
  from dm_control_amd.rl import control
  env = vec_env.VecEnv('cheetah', 'run', cc.NENV, seed=3, per_env_episodes=True,
                       environment_kwargs=dict(device_init=True, ncon_max=4,
                                               build_mode='auto'))
  env.reset()
  physics, task = env.environment.physics, env.environment.task
  hb = physics.batch
  assert hb.model.info.ncon_max == 4 and hb.episodes
  _, qpos, qvel, count = cc.states('cheetah')
  full = count > 4
  hb.set_state(qpos.T, qvel.T)
  physics.set_control(_reference('cheetah', 4)['ctrl'])
  physics.step(check=False)                       # (raises nothing)
  done = physics.episode_done()
  np.testing.assert_array_equal(done & W.DONE_BAD_STATE != 0, full)
  np.testing.assert_array_equal(hb.read(W.FIELD_WARN) & cc.WARN_CONTACTFULL != 0, full)
  frozen_q, frozen_steps = hb.read(W.FIELD_QPOS).copy(), physics.episode_steps()
  physics.step(check=False)
  after = hb.read(W.FIELD_QPOS)
  np.testing.assert_array_equal(after[:, full], frozen_q[:, full])
  assert (after[:, ~full] != frozen_q[:, ~full]).any()
  np.testing.assert_array_equal(physics.episode_steps()[full], frozen_steps[full])
  with pytest.raises(control.PhysicsError, match='mjWARN_CONTACTFULL'):
    physics.check_invalid_state()                 # (what a caller who checks is told)
  assert physics._warn_seen[full].all()           # pylint: disable=protected-access
  still_running = physics.episode_done() == 0
  before = hb.read(W.FIELD_QPOS).copy()
  task.reset_done(physics)
  assert not physics.episode_done()[full].any()
  assert not hb.read(W.FIELD_WARN)[full].any()
  assert not physics.episode_steps()[full].any()
  assert not physics._warn_seen[full].any()       # pylint: disable=protected-access
  now = hb.read(W.FIELD_QPOS)
  assert (now[:, full] != before[:, full]).any(axis=0).all()
  np.testing.assert_array_equal(now[:, still_running], before[:, still_running])
  fresh = hb.read(W.FIELD_STATS)[0][full]
  print('OBSERVED contacts of the re-initialised envs: up to %d (ncon_max 4)' % fresh.max())
  # the next step: the re-initialised envs step and report nothing
  physics.step(check=False)
  warn = hb.read(W.FIELD_WARN)
  assert not warn[full].any() and not physics.episode_done()[full].any()
  assert (physics.episode_steps()[full] == 1).all()
  try:
    physics.check_invalid_state()
  except control.PhysicsError:                     # (envs that ran on may have filled up since)
    pass
  assert not (physics._warn_seen[full]).any()      # pylint: disable=protected-access
  env.close()


def test_sequence_launch_with_a_saturated_env_equals_single_steps():
  import torch
  model, qpos, qvel, count = cc.states('cheetah')
  hm = W.HipModel(build.build_model(model, helpers.TASKS['cheetah'], 'f32', ncon_max=4))
  assert hm.info.seq_launch == 1
  gen = torch.Generator(device='cuda')
  gen.manual_seed(3)
  acts = torch.rand(8, cc.NENV, model.nu, device='cuda', dtype=torch.float32, generator=gen)*2 - 1
  out = []
  for sequence in (True, False):
    hb = W.HipBatch(hm, cc.NENV)
    hb.set_state(qpos.T, qvel.T)
    if sequence:
      hb.step_device_n(acts.data_ptr(), 1, model.nu, cc.NENV*model.nu, 8, 1)
    else:
      for t in range(8):
        hb.step_device(acts.data_ptr() + t*cc.NENV*model.nu*4, 1, model.nu, 1)
    out.append({f: hb.read(getattr(W, 'FIELD_' + f)) for f in (
        'QPOS', 'QVEL', 'WARMSTART', 'TIME', 'OBS', 'REWARD', 'STATS', 'WARN')})
    hb.free()
  for f in out[0]:
    np.testing.assert_array_equal(out[0][f], out[1][f], err_msg=f)
  assert (out[0]['WARN'][count > 4] & cc.WARN_CONTACTFULL).all()
  hm.free()
