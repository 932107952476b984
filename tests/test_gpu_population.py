"""Rollouts over a population of policies (`dmc_batch_rollout_population` on a
population build of the one-env-per-lane kernel): env e acts with the weights of
member e // (nenv // P).  Every "equal" is bitwise, over the fields of
tests/test_gpu_step_sequence.py and the three recorded trajectories; all runs that
are compared bit for bit use the same code object.
"""

import numpy as np
import pytest
import torch

import helpers
import population_cases
import test_gpu_rollout as roll
from dm_control_amd import build
from dm_control_amd import wrapper
from dm_control_amd.rl import policy as policy_lib

pytestmark = pytest.mark.gpu

W = wrapper
FIELDS = roll.FIELDS
TRAJECTORIES = roll.TRAJECTORIES
TANH_ULPS = roll.TANH_ULPS
WARN_BADCTRL = 128


def _start(name, precision, nenv, population=True, seed=4):
  """A population (or plain rollout) code object and a batch at seeded initial
  states, outputs current."""
  model = helpers.load_model(name)
  hm = W.HipModel(build.build_model(model, helpers.TASKS[name], precision, rollout=True,
                                    population=population))
  assert hm.rollout_caps & W.ROLLOUT_OUTPUTS and hm.rollout_caps & W.ROLLOUT_POLICY
  assert bool(hm.rollout_caps & W.ROLLOUT_POPULATION) == population
  assert hm.rollout_caps >> W.ROLLOUT_WIDTH_SHIFT == 64
  hb = W.HipBatch(hm, nenv)
  qpos, qvel = helpers.initial_states(model, name, nenv, seed=seed)
  hb.set_state(qpos.T, qvel.T)
  hb.forward()
  return model, hm, hb


def _rollout(name, precision, nenv, nsteps, ctrl=None, pop=None, calls=None, population=True,
             members=True):
  """All fields and the three trajectories after `nsteps` control steps issued as the
  calls of `calls` (lengths; default one call), plus the observation before.  `pop`:
  an MLPPopulation; members=False passes its one member through dmc_batch_rollout."""
  _, hm, hb = _start(name, precision, nenv, population)
  info, dt = hm.info, roll._torch_dtype(hm)        # pylint: disable=protected-access
  nu, nobs = info.nu, info.nobs
  out = {'obs_out': torch.full((nsteps, nenv, nobs), -7.0, device='cuda', dtype=dt),
         'reward_out': torch.full((nsteps, nenv), -7.0, device='cuda', dtype=dt),
         'action_out': torch.full((nsteps, nenv, nu), -7.0, device='cuda', dtype=dt)}
  policy = None
  if pop is not None:
    weights = torch.from_numpy(pop.packed(hm.dtype)).cuda()
    assert weights.shape == (pop.nparams, pop.num_members) and weights.is_contiguous()
    policy = (weights.data_ptr(), pop.widths) + ((pop.num_members,) if members else ())
  first = hb.read(W.FIELD_OBS)
  torch.cuda.synchronize()
  es, t = out['obs_out'].element_size(), 0
  for n in calls or [nsteps]:
    hb.rollout(
        n, 1,
        ctrl=None if ctrl is None else (ctrl.data_ptr() + t*nenv*nu*es, 1, nu, nenv*nu),
        policy=policy,
        reward_out=(out['reward_out'].data_ptr() + t*nenv*es, nenv),
        obs_out=(out['obs_out'].data_ptr() + t*nenv*nobs*es, nenv*nobs),
        action_out=(out['action_out'].data_ptr() + t*nenv*nu*es, nenv*nu))
    t += n
  assert t == nsteps
  res = {field: hb.read(fid) for field, fid in FIELDS}      # (synchronises)
  res.update((k, v.cpu().numpy()) for k, v in out.items())
  res['first_obs'] = first
  hb.free()
  hm.free()
  return res


def _of_envs(res, field, envs):
  a = res[field]
  if field in TRAJECTORIES:
    return a[:, envs]
  return a[envs] if a.ndim == 1 or field == 'obs' else a[:, envs]


def _model_error(got, pop, noise, real):
  """(err, bound, want) of action_out - noise against every env's own member on o_t,
  after asserting that a neighbouring member's weights would be told apart."""
  obs = np.concatenate([got['first_obs'][None], got['obs_out'][:-1]]).astype(np.float64)
  population_cases.assert_members_tell_apart(pop, obs, real, TANH_ULPS[real])
  want, bound = population_cases.member_actions(pop, obs, real, TANH_ULPS[real])
  err = np.abs(got['action_out'].astype(np.float64) - noise.cpu().numpy().astype(np.float64) - want)
  return err, bound, want


# -- members act with their own weights ------------------------------------------------

@pytest.mark.parametrize('name,precision,nenv,members', [
    ('cheetah', 'f32', 130, 130),      # group size 1: a coalesced wave access
    ('cheetah', 'f32', 130, 65),       # group size 2
    ('cheetah', 'f32', 130, 2),        # group size 65: a boundary at lane 1 of the second wave
    ('cartpole', 'f64', 66, 66), ('cartpole', 'f64', 66, 2)])
@pytest.mark.parametrize('hidden', [(64,), (3, 64)])
def test_members_act_with_their_own_weights(name, precision, nenv, members, hidden):
  """action_out[t] - noise[t] of every env against the fp64 model of ITS member on
  o_t within twice the forward error bound; cheetah at 130 envs is two workgroups and
  a 2-env tail."""
  nobs, nu = population_cases.DIMS[name]
  real = np.float32 if precision == 'f32' else np.float64
  pop = population_cases.make_population(nobs, hidden, nu, members, seed=len(hidden))
  noise = roll._noise(3, nenv, nu, torch.float32 if precision == 'f32' else torch.float64,   # pylint: disable=protected-access
                      5, scale=0.1)
  got = _rollout(name, precision, nenv, 3, ctrl=noise, pop=pop)
  err, bound, want = _model_error(got, pop, noise, real)
  print('%s P=%d %r: policy error / bound: max %.3f' % (name, members, hidden, (err/bound).max()))
  assert np.all(err <= 2*bound), float((err/bound).max())
  assert np.abs(want).max() > 0.1 and not got['warn'].any()


# -- one launch equals single launches, and the replay -----------------------------------------

def test_one_launch_equals_single_launches():
  """cheetah f32, 66 envs, 66 members, 70 steps: one call (two chunks, 64 + 6), 70
  calls, and calls of 64 and 6."""
  pop = population_cases.make_population(17, (5, 64), 6, 66, seed=1)
  noise = roll._noise(70, 66, 6, torch.float32, 2, scale=0.3)     # pylint: disable=protected-access
  kw = dict(ctrl=noise, pop=pop)
  one = _rollout('cheetah', 'f32', 66, 70, **kw)
  roll._assert_same(one, _rollout('cheetah', 'f32', 66, 70, calls=[1]*70, **kw))   # pylint: disable=protected-access
  roll._assert_same(one, _rollout('cheetah', 'f32', 66, 70, calls=[64, 6], **kw))  # pylint: disable=protected-access
  assert not one['warn'].any()
  assert np.abs(one['action_out'] - noise.cpu().numpy()).max() > 0.05     # (the policies acted)


def test_recorded_actions_replay_the_rollout():
  pop = population_cases.make_population(17, (5, 64), 6, 65, seed=3)
  noise = roll._noise(5, 130, 6, torch.float32, 4, scale=0.3)     # pylint: disable=protected-access
  closed = _rollout('cheetah', 'f32', 130, 5, ctrl=noise, pop=pop)
  replay = _rollout('cheetah', 'f32', 130, 5, ctrl=torch.from_numpy(closed['action_out']).cuda())
  roll._assert_same(closed, replay)                               # pylint: disable=protected-access
  assert closed['stats'][0].max() > 0


# -- one member ----------------------------------------------------------------------------

@pytest.mark.parametrize('name,precision,nenv', [('cheetah', 'f32', 130), ('cartpole', 'f64', 66)])
def test_one_member_on_a_population_build(name, precision, nenv):
  """members = 1 on a population build against the plain rollout build, the same
  policy.  Two code objects: each evaluation is within `bound` of the exact MLP to
  first order, so wherever the two acted on the same observation (o_0 always) their
  actions are within 2*bound of each other.  Prints whether they were equal bit for bit."""
  nobs, nu = population_cases.DIMS[name]
  real = np.float32 if precision == 'f32' else np.float64
  pop = population_cases.make_population(nobs, (64, 64), nu, 1, seed=7)
  noise = roll._noise(3, nenv, nu, torch.float32 if precision == 'f32' else torch.float64,   # pylint: disable=protected-access
                      6, scale=0.1)
  runs = {'population build, members = 1': _rollout(name, precision, nenv, 3, ctrl=noise, pop=pop),
          'population build, dmc_batch_rollout': _rollout(name, precision, nenv, 3, ctrl=noise,
                                                          pop=pop, members=False),
          'rollout build': _rollout(name, precision, nenv, 3, ctrl=noise, pop=pop,
                                    population=False, members=False)}
  for what, got in runs.items():
    err, bound, _ = _model_error(got, pop, noise, real)
    assert np.all(err <= 2*bound), (what, float((err/bound).max()))
    assert not got['warn'].any()
  a, b = runs['population build, members = 1'], runs['rollout build']
  roll._assert_same(a, runs['population build, dmc_batch_rollout'])   # pylint: disable=protected-access
  np.testing.assert_array_equal(a['first_obs'], b['first_obs'])
  compared = 0
  for t in range(3):
    before = (lambda r: r['first_obs'] if t == 0 else r['obs_out'][t - 1])
    if np.array_equal(before(a), before(b)):
      apart = np.abs(a['action_out'][t].astype(np.float64) - b['action_out'][t])
      assert np.all(apart <= 2*bound[t]), (t, float((apart/bound[t]).max()))
      compared += 1
  print('%s %s: compared at %d of 3 steps' % (name, precision, compared))
  same = all(np.array_equal(a[f], b[f]) for f in [f for f, _ in FIELDS] + list(TRAJECTORIES))
  print('%s %s: members = 1 on the population build %s the rollout build bit for bit'
        % (name, precision, 'equals' if same else 'does not equal'))


# -- isolation -----------------------------------------------------------------------------

def test_a_bad_member_stays_in_its_own_envs():
  """Member 3 of 65 puts out NaN: envs 6 and 7 carry DMC_WARN_BADCTRL and move like a
  zero-action twin, every other env is bit for bit what it is without the NaN."""
  clean = population_cases.make_population(17, (5,), 6, 65, seed=6)
  members = [clean.member(i) for i in range(65)]
  members[3].biases[-1][:] = np.nan
  broken = policy_lib.MLPPopulation.from_policies(members)
  bad = _rollout('cheetah', 'f32', 130, 3, pop=broken)
  good = _rollout('cheetah', 'f32', 130, 3, pop=clean)
  zero = _rollout('cheetah', 'f32', 130, 3, ctrl=torch.zeros(3, 130, 6, device='cuda'))
  its = population_cases.member_of_env(130, 65) == 3
  assert its.sum() == 2 and its[6] and its[7]
  assert np.all(bad['warn'][its] & WARN_BADCTRL) and not bad['warn'][~its].any()
  assert not good['warn'].any() and not zero['warn'].any()
  assert np.isnan(bad['action_out'][:, its]).all() and np.isfinite(bad['action_out'][:, ~its]).all()
  for field in [f for f, _ in FIELDS] + list(TRAJECTORIES):
    np.testing.assert_array_equal(_of_envs(bad, field, ~its), _of_envs(good, field, ~its),
                                  err_msg=field)
    if field not in ('warn', 'action_out'):
      np.testing.assert_array_equal(_of_envs(bad, field, its), _of_envs(zero, field, its),
                                    err_msg=field)


# -- refusals ------------------------------------------------------------------------------

def test_refusals_leave_a_batch_that_steps():
  pop = population_cases.make_population(17, (5,), 6, 130, seed=8)
  weights = torch.from_numpy(pop.packed(np.float32)).cuda()
  _, hm, hb = _start('cheetah', 'f32', 130, population=False)
  with pytest.raises(W.Error, match='population=True'):
    hb.rollout(2, 1, policy=(weights.data_ptr(), pop.widths, 2))
  roll._still_steps(hb, 6)                     # pylint: disable=protected-access
  hb.rollout(2, 1, policy=(weights.data_ptr(), pop.widths, 1))     # (one member: any rollout build)
  hb.free()
  hm.free()
  _, hm, hb = _start('cheetah', 'f32', 130)
  for members, message in ((0, 'members must be >= 1'), (-3, 'members must be >= 1'),
                           (4, '4 members .* 130 envs'), (260, '260 members .* 130 envs')):
    with pytest.raises(W.Error, match=message):
      hb.rollout(2, 1, policy=(weights.data_ptr(), pop.widths, members))
    roll._still_steps(hb, 6)                   # pylint: disable=protected-access
  hb.rollout(2, 1, policy=(weights.data_ptr(), pop.widths, 130))
  assert not hb.read(W.FIELD_WARN).any()
  hb.free()
  hm.free()


# -- VecEnv ----------------------------------------------------------------------------------

def _vec_env(**kw):
  from dm_control_amd import vec_env
  # time limit 0.065 s: the episode ends with the 7th step of 0.01 s
  return vec_env.VecEnv('cheetah', 'run', 130, seed=0, torch_io=True,
                        task_kwargs={'time_limit': 0.065}, **kw)


def test_vec_env_rollout_over_a_population():
  from dm_control_amd import vec_env
  with pytest.raises(ValueError, match='rollout=True'):
    vec_env.VecEnv('cheetah', 'run', 4, torch_io=True, population=True)
  pop = population_cases.make_population(17, (64, 64), 6, 65, seed=9)
  noise = roll._noise(10, 130, 6, torch.float32, 10, scale=0.2)     # pylint: disable=protected-access
  env, twin = _vec_env(rollout=True, population=True), _vec_env(rollout=True, population=True)
  assert 'one env per lane' in env.environment.physics.kernel_shape
  with pytest.raises(ValueError, match='set by a rollout'):
    env.member_of_env    # pylint: disable=pointless-statement
  first = env.reset()
  np.testing.assert_array_equal(first.cpu().numpy(), twin.reset().cpu().numpy())
  out = env.rollout(10, policy=pop, noise=noise)
  assert out['obs'].shape == (7, 130, 17) and out['actions'].shape == (7, 130, 6)
  assert out['rewards'].shape == (7, 130) and out['dones'].shape == (7, 130)
  assert out['dones'][-1].all() and not out['dones'][:-1].any()
  np.testing.assert_array_equal(out['terminal_observation'].cpu().numpy(),
                                out['obs'][-1].cpu().numpy())
  of_env = env.member_of_env
  assert of_env.dtype == torch.int64 and of_env.is_cuda and of_env.shape == (130,)
  np.testing.assert_array_equal(of_env.cpu().numpy(), population_cases.member_of_env(130, 65))
  fitness = out['rewards'].sum(0).view(65, -1).mean(1)
  by_index = torch.zeros(65, device='cuda').index_add_(0, of_env, out['rewards'].sum(0))/2
  np.testing.assert_allclose(fitness.cpu().numpy(), by_index.cpu().numpy(), rtol=1e-6)
  obs = np.concatenate([first.cpu().numpy()[None], out['obs'][:-1].cpu().numpy()]).astype(np.float64)
  population_cases.assert_members_tell_apart(pop, obs, np.float32, TANH_ULPS[np.float32])
  want, bound = population_cases.member_actions(pop, obs, np.float32, TANH_ULPS[np.float32])
  err = np.abs(out['actions'].cpu().numpy().astype(np.float64)
               - noise[:7].cpu().numpy().astype(np.float64) - want)
  assert np.all(err <= 2*bound), float((err/bound).max())
  # a device tensor is read in place: no upload, the same steps
  held = torch.from_numpy(pop.packed(np.float32)).cuda()
  resident = policy_lib.MLPPopulation.from_device(held, 17, pop.widths)
  assert resident.num_members == 65
  assert twin._policy_device(resident)[0] == held.data_ptr()     # pylint: disable=protected-access
  assert not twin._policy_cache                                   # pylint: disable=protected-access
  again = twin.rollout(10, policy=resident, noise=noise)
  for key in ('obs', 'actions', 'rewards', 'dones', 'next_obs'):
    np.testing.assert_array_equal(again[key].cpu().numpy(), out[key].cpu().numpy(), err_msg=key)
  with pytest.raises(ValueError, match='population=True'):
    plain = _vec_env(rollout=True)
    plain.rollout(3, policy=pop, noise=noise)
  plain.close()
  env.close()
  twin.close()
